"""bundle_adjust without a GPU: every argument the entry points reject is rejected before a device is touched, the
wrappers refuse what the library would, calls with nothing to do return without a device, and pose_from_camera
inverts camera_from_pose whatever the camera's scale and sign."""
import numpy as np
import pytest

from tests import bundle_cases as bc

EYE = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(12)
KK = bc.K0.reshape(9)


def raw_args(**over):
    """Valid arguments of the raw entry points on host arrays (the device entry checks before it launches)."""
    a = dict(geom=np.zeros((6, 4), np.float32), seg=np.array([0, 2, 6], np.int64), nseg=2, K=np.stack([KK, KK]),
             poses=np.stack([EYE, EYE]), mode=np.array([2, 1], np.int32), off=np.array([0, 2, 5], np.int64), nt=2,
             mem=np.zeros((5, 2), np.int32), nm=5, X=np.full((2, 4), 5.0), use=None, huber=np.inf, max_steps=3, lambda0=1e-4,
             ftol=1e-10, gtol=1e-10, cg_tol=1e-8, cg_max=16, err=np.zeros(5), active=np.zeros(2, np.uint8),
             trace=np.full((3, 6), 7.0), info=np.full(7, 7.0))
    a.update(over)
    return a


def ptr(x):
    if x is None or isinstance(x, int):
        return x
    return x.ctypes.data


def call_raw(a, device_form):
    from spectavi_amd._lib import clib
    args = [ptr(a["geom"]), ptr(a["seg"]), a["nseg"], ptr(a["K"]), ptr(a["poses"]), ptr(a["mode"]), ptr(a["off"]), a["nt"],
            ptr(a["mem"]), a["nm"], ptr(a["X"]), ptr(a["use"]), a["huber"], a["max_steps"], a["lambda0"], a["ftol"], a["gtol"],
            a["cg_tol"], a["cg_max"], ptr(a["err"]), ptr(a["active"]), ptr(a["trace"]), ptr(a["info"])]
    if device_form:
        return clib.spv_bundle_adjust_device(*args, None, 0, None)
    return clib.spv_bundle_adjust(*args)


def k_with(i, v):
    k = KK.copy()
    k[i] = v
    return np.stack([KK, k])


def pose_with(R):
    p = EYE.reshape(3, 4).copy()
    p[:, :3] = R
    return np.stack([EYE, p.reshape(12)])


TILT = bc.rodrigues(np.array([0.1, -0.2, 0.3]))
BAD = {
    "track_off starts at 1": dict(off=np.array([1, 2, 5], np.int64)),
    "track_off decreases": dict(off=np.array([0, 3, 2], np.int64), nm=2),
    "track_off ends short of nmembers": dict(off=np.array([0, 2, 4], np.int64)),
    "track_off ends beyond nmembers": dict(off=np.array([0, 2, 6], np.int64)),
    "nmembers 2^31": dict(off=np.array([0, 2, 2 ** 31], np.int64), nm=2 ** 31),
    "total_rows 2^31": dict(seg=np.array([0, 2, 2 ** 31], np.int64)),
    "seg_off starts at 1": dict(seg=np.array([1, 2, 6], np.int64)),
    "seg_off decreases": dict(seg=np.array([0, 7, 6], np.int64)),
    "negative nseg": dict(nseg=-1),
    "negative ntracks": dict(nt=-1),
    "negative nmembers": dict(nm=-1),
    "mode 3": dict(mode=np.array([2, 3], np.int32)),
    "mode -1": dict(mode=np.array([-1, 1], np.int32)),
    "K[8] not 1": dict(K=k_with(8, 2.0)),
    "K[3] not 0": dict(K=k_with(3, 1e-3)),
    "K[6] not 0": dict(K=k_with(6, 1e-3)),
    "K[7] not 0": dict(K=k_with(7, 1e-3)),
    "K[0] zero": dict(K=k_with(0, 0.0)),
    "K[4] zero": dict(K=k_with(4, 0.0)),
    "K[2] NaN": dict(K=k_with(2, np.nan)),
    "K[0] inf": dict(K=k_with(0, np.inf)),
    "R scaled": dict(poses=pose_with(TILT * (1 + 1e-5))),
    "R sheared": dict(poses=pose_with(TILT + 1e-5 * np.eye(3)[[1, 0, 2]])),
    "R a reflection": dict(poses=pose_with(TILT @ np.diag([1., 1., -1.]))),
    "R NaN": dict(poses=pose_with(np.full((3, 3), np.nan))),
    "t inf": dict(poses=np.stack([EYE, np.concatenate([EYE[:11], [np.inf]])])),
    "huber NaN": dict(huber=np.nan),
    "huber zero": dict(huber=0.0),
    "huber negative": dict(huber=-1.0),
    "lambda0 NaN": dict(lambda0=np.nan),
    "lambda0 negative": dict(lambda0=-1e-4),
    "ftol NaN": dict(ftol=np.nan),
    "ftol negative": dict(ftol=-1.0),
    "gtol NaN": dict(gtol=np.nan),
    "gtol negative": dict(gtol=-1.0),
    "cg_tol NaN": dict(cg_tol=np.nan),
    "cg_tol negative": dict(cg_tol=-1.0),
    "max_steps negative": dict(max_steps=-1),
    "cg_max negative": dict(cg_max=-1),
    "null seg_off": dict(seg=None),
    "null track_off": dict(off=None),
    "null K": dict(K=None),
    "null poses": dict(poses=None),
    "null mode": dict(mode=None),
    "null members": dict(mem=None),
    "null geom": dict(geom=None),
    "null X": dict(X=None),
    "null info": dict(info=None),
    "misaligned X": dict(X="off by 4"),
    "misaligned err": dict(err="off by 4"),
    "misaligned trace": dict(trace="off by 4"),
    "misaligned info": dict(info="off by 4"),
    "misaligned poses": dict(poses="off by 4"),
}


@pytest.mark.parametrize("device_form", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("what", sorted(BAD))
def test_raw_calls_reject(what, device_form):
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    room = np.zeros(64)
    over = {k: room.ctypes.data + int(v.split()[-1]) if isinstance(v, str) else v for k, v in BAD[what].items()}
    a = raw_args(**over)
    before = {k: v.copy() for k, v in a.items() if isinstance(v, np.ndarray)}
    assert call_raw(a, device_form) == SPV_ERR_INVALID, what
    assert clib.spv_last_error(), what
    for k, v in before.items():
        assert a[k].tobytes() == v.tobytes(), "nothing is written (%s)" % k


def test_a_mode_0_set_is_not_read():
    """NaN K and poses in a set without a camera pass the checks (the call then needs a device: not made here);
    with every set at mode 0 there is nothing to do."""
    a = raw_args(K=np.stack([np.full(9, np.nan)] * 2), poses=np.full((2, 12), np.nan), mode=np.zeros(2, np.int32))
    for device_form in (False, True):
        a["trace"][:], a["info"][:] = 7.0, 7.0
        if device_form:
            a["err"], a["active"] = None, None   # (device outputs: the host form's are checked below)
        else:
            a["active"][:] = 7
        assert call_raw(a, device_form) == 0
        assert np.all(np.isnan(a["trace"])) and np.all(a["info"] == 0) and np.all(a["X"] == 5.0)
        assert np.all(np.isnan(a["poses"]))
        if not device_form:
            assert np.all(a["active"] == 0) and np.all(np.isnan(a["err"]))


def test_raw_calls_accept_nothing_to_do():
    """No track, or no camera: SPV_OK without a device, whatever else is empty or NULL."""
    none = dict(off=np.array([0], np.int64), nt=0, nm=0, mem=None, X=None, err=None, active=None)
    for a in (raw_args(**none), raw_args(seg=np.array([0], np.int64), nseg=0, K=None, poses=None, mode=None, geom=None, **none),
              raw_args(seg=np.array([0], np.int64), nseg=0, K=None, poses=None, mode=None, geom=None, err=None, active=None),
              raw_args(trace=None, **none), raw_args(max_steps=0, **none)):
        for device_form in (True, False):
            a["info"][:] = 7.0
            assert call_raw(a, device_form) == 0
            assert np.all(a["info"] == 0)
            if a["trace"] is not None:
                assert np.all(np.isnan(a["trace"][:a["max_steps"]]))


def test_workspace_entry():
    from spectavi_amd._lib import clib
    small, big = clib.spv_bundle_adjust_workspace_bytes(2, 10, 30), clib.spv_bundle_adjust_workspace_bytes(2, 10, 3000)
    assert 0 < small < big and small % 256 == 0
    assert big - small >= (3000 - 30) * (16 + 4 * 4)      # per member: the weighted residual and four int32 tables
    assert clib.spv_bundle_adjust_workspace_bytes(-1, 10, 30) == 0 and clib.spv_bundle_adjust_workspace_bytes(2, 10, -1) == 0


def test_pose_and_camera_round_trip():
    from spectavi_amd import mvg
    rng = np.random.default_rng(5)
    for k in range(20):
        R, t = bc.rodrigues(rng.standard_normal(3)), rng.standard_normal(3) * 3
        K = np.array([[900. + 50 * k, 0.3 * k, 600.], [0., 950., 400. + k], [0., 0., 1.]])
        P = mvg.camera_from_pose(R, t, K)
        assert np.allclose(P, K @ np.hstack([R, t[:, None]]), rtol=0, atol=1e-12)
        for scale in (1.0, -1.0, 3.7, -0.02, 1e6, -1e-6):
            R2, t2 = mvg.pose_from_camera(scale * P, K)
            # K^-1 P at cond(K) ~ 1e3: the entries of R carry about 1e-13
            assert np.max(np.abs(R2 - R)) < 1e-11 and np.max(np.abs(t2 - t)) < 1e-10, (k, scale)
            assert abs(np.linalg.det(R2) - 1) < 1e-12 and np.max(np.abs(R2.T @ R2 - np.eye(3))) < 1e-12
    # a camera that is no K [R | t]: the nearest rotation, still a rotation
    R2, t2 = mvg.pose_from_camera(bc.K0 @ np.hstack([TILT + 0.01 * rng.standard_normal((3, 3)), np.ones((3, 1))]), bc.K0)
    assert np.max(np.abs(R2.T @ R2 - np.eye(3))) < 1e-12 and np.max(np.abs(R2 - TILT)) < 0.05
    for bad in (np.zeros((3, 4)), np.zeros((4, 4))):
        with pytest.raises(ValueError):
            mvg.pose_from_camera(bad, bc.K0)
    with pytest.raises(ValueError):
        mvg.camera_from_pose(np.eye(4), np.zeros(3), bc.K0)


def test_python_forms_raise_value_error_before_a_device():
    import torch
    from spectavi_amd import device, mvg
    geom = torch.zeros((6, 4), dtype=torch.float32)      # CPU tensors: a call that got past its checks would raise
    mem = torch.zeros((5, 2), dtype=torch.int32)         # TypeError ("on the GPU"), never ValueError
    X = torch.ones((2, 4), dtype=torch.float64)
    eye = EYE.reshape(3, 4)
    good = dict(geom=geom, seg_off=[0, 2, 6], K=bc.K0, poses=[eye, eye], track_off=[0, 2, 5], members=mem, X=X)
    with pytest.raises(TypeError):
        device.bundle_adjust(**good)
    scaled = eye.copy()
    scaled[:, :3] *= 1 + 1e-5
    badK = bc.K0.copy()
    badK[1, 0] = 1e-3
    common = (("K shape", dict(K=np.eye(4))), ("K count", dict(K=np.stack([bc.K0] * 3))), ("K lower entry", dict(K=badK)),
              ("K[2,2]", dict(K=bc.K0 * 2)), ("K NaN", dict(K=bc.K0 * np.nan)), ("poses count", dict(poses=[eye])),
              ("pose shape", dict(poses=[eye, np.eye(4)])), ("pose no rotation", dict(poses=[eye, scaled])),
              ("pose NaN", dict(poses=[eye, eye * np.nan])), ("fixed count", dict(fixed=[1])), ("huber", dict(huber=0.)),
              ("huber NaN", dict(huber=float("nan"))), ("lambda0", dict(lambda0=-1.)), ("ftol", dict(ftol=float("nan"))),
              ("gtol", dict(gtol=-1.)), ("cg_tol", dict(cg_tol=-1.)), ("max_steps", dict(max_steps=-1)), ("cg_max", dict(cg_max=-1)),
              ("track_off start", dict(track_off=[1, 2, 5])), ("track_off end", dict(track_off=[0, 2, 4])))
    for what, over in common + (
            ("geom shape", dict(geom=torch.zeros((6, 3), dtype=torch.float32))),
            ("geom dtype", dict(geom=torch.zeros((6, 4), dtype=torch.float64))),
            ("geom numpy", dict(geom=np.zeros((6, 4), np.float32))),
            ("geom rows", dict(geom=torch.zeros((5, 4), dtype=torch.float32))),
            ("members shape", dict(members=torch.zeros((5, 3), dtype=torch.int32))),
            ("members dtype", dict(members=torch.zeros((5, 2), dtype=torch.int64))),
            ("seg_off order", dict(seg_off=[0, 7, 6])),
            ("X shape", dict(X=torch.ones((3, 4), dtype=torch.float64))),
            ("X dtype", dict(X=torch.ones((2, 4), dtype=torch.float32))),
            ("use dtype", dict(use=torch.ones(2, dtype=torch.int32))),
            ("use count", dict(use=torch.ones(3, dtype=torch.uint8)))):
        with pytest.raises(ValueError):
            device.bundle_adjust(**dict(good, **over))
    hgood = dict(coords=[np.zeros((2, 2)), np.zeros((4, 3))], sizes=[2, 4], K=bc.K0, poses=[eye, eye], track_off=[0, 2, 5],
                 members=np.zeros((5, 2), np.int32), X=np.ones((2, 4)))
    for what, over in common + (
            ("coords columns", dict(coords=[np.zeros((2, 1)), np.zeros((4, 3))])),
            ("coords rows", dict(coords=[np.zeros((3, 2)), np.zeros((4, 3))])),
            ("sizes negative", dict(sizes=[2, -4])),
            ("members shape", dict(members=np.zeros((5, 3), np.int32))),
            ("members dtype", dict(members=np.zeros((5, 2)))),
            ("X shape", dict(X=np.ones((2, 3)))),
            ("use count", dict(use=[1]))):
        with pytest.raises(ValueError):
            mvg.bundle_adjust(**dict(hgood, **over))
    # nothing to do: no device is needed, and the inputs come back
    P, Xo, info = mvg.bundle_adjust(hgood["coords"], [2, 4], bc.K0, [eye, None], [0], np.zeros((0, 2), np.int32), np.zeros((0, 4)))
    assert P.shape == (2, 3, 4) and np.array_equal(P[0], eye) and not P[1].any() and Xo.shape == (0, 4)
    assert info["steps"] == 0 and info["tracks"] == 0 and info["stop"] == "max_steps" and info["trace"].shape == (0, 6)
    P, Xo, info = mvg.bundle_adjust(hgood["coords"], [2, 4], bc.K0, [None, None], [0, 2, 5], np.zeros((5, 2), np.int32),
                                    np.ones((2, 4)))
    assert not P.any() and np.all(Xo == 1) and not info["active"].any() and np.all(np.isnan(info["err"]))


@pytest.mark.parametrize("what", ["missing", "short", "misaligned"])
def test_device_form_refuses_its_workspace_before_it_writes(what):
    """Valid arguments with work to do and a workspace that is NULL, a byte short or not aligned to 256: SPV_ERR_INVALID
    before a device is touched, and trace, info and every other array as they came."""
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    a = raw_args()
    need = clib.spv_bundle_adjust_workspace_bytes(a["nseg"], a["nt"], a["nm"])
    room = np.zeros(need // 8 + 64)
    base = (room.ctypes.data + 255) // 256 * 256
    ws, nbytes = {"missing": (None, need), "short": (base, need - 1), "misaligned": (base + 8, need)}[what]
    before = {k: v.copy() for k, v in a.items() if isinstance(v, np.ndarray)}
    args = [ptr(a["geom"]), ptr(a["seg"]), a["nseg"], ptr(a["K"]), ptr(a["poses"]), ptr(a["mode"]), ptr(a["off"]), a["nt"],
            ptr(a["mem"]), a["nm"], ptr(a["X"]), ptr(a["use"]), a["huber"], a["max_steps"], a["lambda0"], a["ftol"], a["gtol"],
            a["cg_tol"], a["cg_max"], ptr(a["err"]), ptr(a["active"]), ptr(a["trace"]), ptr(a["info"])]
    assert clib.spv_bundle_adjust_device(*args, ws, nbytes, None) == SPV_ERR_INVALID
    assert b"workspace" in clib.spv_last_error()
    for k, v in before.items():
        assert a[k].tobytes() == v.tobytes(), "nothing is written (%s)" % k
    assert not room.any()
