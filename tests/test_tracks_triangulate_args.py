"""triangulate_tracks without a GPU: the model of tests/tracks_triangulate_model.py recovers planted points, the plan
entry counts the two forms around the threshold, the setter round-trips, and every argument the entry points reject
is rejected before a device is touched."""
import ctypes as ct

import numpy as np
import pytest

from tests import tracks_triangulate_model as ttm


@pytest.fixture
def default_long():
    from spectavi_amd import device
    before = device.tracks_triangulate_get_long()
    yield before
    device.tracks_triangulate_set_long(before)


def test_model_recovers_planted_points():
    rng = np.random.default_rng(11)
    cams = ttm.wide_cameras(rng, 40)
    lengths = [2, 3, 4, 5, 8, 12] * 20
    Xw = ttm.points(rng, len(lengths))
    geom, seg = ttm.observe(rng, cams, Xw, 0.0)
    off, mem = ttm.make_tracks(rng, lengths, len(cams))
    mo = ttm.model(geom, seg, cams, off, mem, max_error=1e-2)
    assert mo["solved"].all() and np.array_equal(mo["nused"], lengths) and mo["ok"].all()
    got = mo["X"] / mo["X"][:, 3:4]
    assert np.max(np.abs(got - Xw)) < 1e-3          # float32 pixels: 6e-5 px at 1000 px
    assert np.nanmax(mo["err"]) < 1e-3
    # half a pixel of noise: still close, residuals of the noise's size, and the model is its own definition
    geom, seg = ttm.observe(rng, cams, Xw, 0.5)
    mo = ttm.model(geom, seg, cams, off, mem, max_error=5.0, qr_route=True)
    got = mo["X"] / mo["X"][:, 3:4]
    assert np.max(np.abs(got - Xw)) < 0.1 and 0.05 < np.nanmedian(mo["err"]) < 2.0 and mo["ok"].all()
    st = ttm.check_definition(mo["X"], mo["err"], mo, geom, seg, off, mem, what="the model")
    assert st["tracks"] == len(lengths) == st["well_separated"]
    assert ttm.check_verdict(mo["ok"], mo["nused"], mo, geom, seg, off, mem, 5.0) == 0
    # one observation moved by 20 px: its track fails max_error = 3, its residual exceeds it
    geom2 = geom.copy()
    row = seg[mem[off[7], 0]] + mem[off[7], 1]
    geom2[row, 0] += 20
    mo2 = ttm.model(geom2, seg, cams, off, mem, max_error=3.0)
    assert mo2["ok"][7] == 0 and mo2["err"][off[7]] > 3 and mo2["ok"].sum() == len(lengths) - 1


def test_model_conventions():
    rng = np.random.default_rng(12)
    cams = ttm.wide_cameras(rng, 5)
    Xw = ttm.points(rng, 4)
    geom, seg = ttm.observe(rng, cams, Xw, 0.0)
    off = np.array([0, 3, 5, 5, 8], np.int64)
    mem = np.array([[0, 0], [1, 0], [2, 0], [-1, 1], [3, 1], [4, 3], [5, 3], [2, 4]], np.int32)
    mo = ttm.model(geom, seg, cams, off, mem, use=[1, 0, 1, 1, 1])
    assert mo["nused"].tolist() == [2, 1, 0, 1] and mo["solved"].tolist() == [True, False, False, False]
    assert mo["ok"].tolist() == [1, 0, 0, 0] and np.all(mo["X"][1:] == 0)
    assert np.isnan(mo["err"]).tolist() == [False, True, False, True, True, True, True, True]


def test_plan_counts(default_long):
    from spectavi_amd import device
    assert default_long == 16

    def plan_of(lengths):
        return device.triangulate_tracks_plan(np.concatenate([[0], np.cumsum(lengths)]))
    for setting, L in ((None, 16), (5, 5), (32, 32), (0, 0), (10 ** 9, 10 ** 9)):
        if setting is not None:
            device.tracks_triangulate_set_long(setting)
        assert device.tracks_triangulate_get_long() == L
        lengths = [max(L - 1, 0), L, L + 1, 2, 0, 1, 3, 300, 70]
        lengths = [min(n, 5000) for n in lengths]
        wave = sum(1 for n in lengths if n >= 3 and n > L)
        p = plan_of(lengths)
        assert p == dict(lane_tracks=len(lengths) - wave, wave_tracks=wave, lane_groups=1, longest=max(lengths)), (L, p)
        for n in (max(L - 1, 2), L, L + 1):
            n = min(n, 5000)
            p = plan_of([n])
            want_wave = 1 if (n >= 3 and n > L) else 0
            assert (p["lane_tracks"], p["wave_tracks"], p["lane_groups"], p["longest"]) == (1 - want_wave, want_wave,
                                                                                         1 - want_wave, n), (L, n, p)
    device.tracks_triangulate_set_long(16)
    # workgroups of the lane launch: one lane per track of the call
    for nt, groups in ((255, 1), (256, 1), (257, 2), (513, 3)):
        assert plan_of([2] * nt)["lane_groups"] == groups
    assert plan_of([40] * 300) == dict(lane_tracks=0, wave_tracks=300, lane_groups=0, longest=40)
    assert plan_of([40] * 300 + [2])["lane_groups"] == 2
    assert device.triangulate_tracks_plan([0]) == dict(lane_tracks=0, wave_tracks=0, lane_groups=0, longest=0)
    assert device.triangulate_tracks_plan([0, 7]) == dict(lane_tracks=1, wave_tracks=0, lane_groups=1, longest=7)
    for bad in ([], [1, 2], [0, 3, 2], [0, 2 ** 31]):
        with pytest.raises(ValueError):
            device.triangulate_tracks_plan(bad)


def test_setter_round_trips(default_long):
    from spectavi_amd import device
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    for L in (0, 1, 7, 64, 2 ** 31 - 1, 16):
        device.tracks_triangulate_set_long(L)
        assert device.tracks_triangulate_get_long() == L == clib.spv_tracks_triangulate_get_long()
    assert clib.spv_tracks_triangulate_set_long(-1) == SPV_ERR_INVALID and clib.spv_last_error()
    assert device.tracks_triangulate_get_long() == 16
    for bad in (-1, 2.5):
        with pytest.raises(ValueError):
            device.tracks_triangulate_set_long(bad)


def raw_args(**over):
    """Valid arguments of the raw entry points on host arrays (the device entry checks before it launches)."""
    a = dict(geom=np.zeros((6, 4), np.float32), seg=np.array([0, 2, 6], np.int64), nseg=2, cams=np.zeros((2, 12)),
             use=None, off=np.array([0, 2, 5], np.int64), nt=2, mem=np.zeros((5, 2), np.int32), nm=5, max_error=1.0,
             X=np.zeros((2, 4)), err=np.zeros(5), ok=np.zeros(2, np.uint8), nused=np.zeros(2, np.int32))
    a.update(over)
    return a


def ptr(x):
    if x is None or isinstance(x, int):
        return x
    return x.ctypes.data


def call_raw(a, device_form):
    from spectavi_amd._lib import clib
    args = [ptr(a["geom"]), ptr(a["seg"]), a["nseg"], ptr(a["cams"]), ptr(a["use"]), ptr(a["off"]), a["nt"], ptr(a["mem"]),
            a["nm"], a["max_error"], ptr(a["X"]), ptr(a["err"]), ptr(a["ok"]), ptr(a["nused"])]
    if device_form:
        return clib.spv_tracks_triangulate_device(*args, None)
    return clib.spv_tracks_triangulate(*args)


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
    "null seg_off": dict(seg=None),
    "null track_off": dict(off=None),
    "null cams": dict(cams=None),
    "null members": dict(mem=None),
    "null geom": dict(geom=None),
    "null X": dict(X=None),
    "NaN max_error": dict(max_error=float("nan")),
    "misaligned X": dict(X="off by 4"),
    "misaligned err": dict(err="off by 4"),
    "misaligned nused": dict(nused="off by 2"),
}


@pytest.mark.parametrize("device_form", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("what", sorted(BAD))
def test_raw_calls_reject(what, device_form):
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    room = np.zeros(16)
    over = {k: room.ctypes.data + int(v.split()[-1]) if isinstance(v, str) else v for k, v in BAD[what].items()}
    a = raw_args(**over)
    a["X"] = a["X"] if a["X"] is None or isinstance(a["X"], int) else np.full((2, 4), 5.0)
    assert call_raw(a, device_form) == SPV_ERR_INVALID, what
    assert clib.spv_last_error(), what
    if isinstance(a["X"], np.ndarray):
        assert np.all(a["X"] == 5.0), "nothing is written"


def test_raw_calls_accept_nothing_to_do():
    """No track: SPV_OK without a device, whatever else is empty or NULL."""
    a = raw_args(off=np.array([0], np.int64), nt=0, nm=0, mem=None, X=None, err=None, ok=None, nused=None)
    assert call_raw(a, True) == 0 and call_raw(a, False) == 0
    a = raw_args(off=np.array([0], np.int64), nt=0, nm=0, mem=None, X=None, err=None, ok=None, nused=None,
                 seg=np.array([0], np.int64), nseg=0, cams=None, geom=None)
    assert call_raw(a, True) == 0 and call_raw(a, False) == 0


def test_plan_entry_rejects():
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    out = (ct.c_longlong * 4)(-7, -7, -7, -7)
    ok = np.array([0, 2, 5], np.int64)
    for off, nt, o in ((None, 2, out), (ok, -1, out), (ok, 2, None), (np.array([1, 2, 5], np.int64), 2, out),
                       (np.array([0, 5, 2], np.int64), 2, out), (np.array([0, 2, 2 ** 31], np.int64), 2, out)):
        assert clib.spv_tracks_triangulate_plan(ptr(off), nt, o) == SPV_ERR_INVALID
        assert list(out) == [-7] * 4
    assert clib.spv_tracks_triangulate_plan(ptr(ok), 2, out) == 0 and list(out) == [2, 0, 1, 3]


def test_python_forms_raise_value_error_before_a_device():
    import torch
    from spectavi_amd import device, mvg
    geom = torch.zeros((6, 4), dtype=torch.float32)      # CPU tensors: a call that got past its checks would raise
    mem = torch.zeros((5, 2), dtype=torch.int32)         # TypeError ("on the GPU"), never ValueError
    seg, off = [0, 2, 6], [0, 2, 5]
    cams = np.zeros((2, 3, 4))
    good = dict(geom=geom, seg_off=seg, cameras=cams, track_off=off, members=mem)
    with pytest.raises(TypeError):
        device.triangulate_tracks(**good)
    for what, over in (
            ("geom shape", dict(geom=torch.zeros((6, 3), dtype=torch.float32))),
            ("geom dtype", dict(geom=torch.zeros((6, 4), dtype=torch.float64))),
            ("geom numpy", dict(geom=np.zeros((6, 4), np.float32))),
            ("geom rows", dict(geom=torch.zeros((5, 4), dtype=torch.float32))),
            ("members shape", dict(members=torch.zeros((5, 3), dtype=torch.int32))),
            ("members dtype", dict(members=torch.zeros((5, 2), dtype=torch.int64))),
            ("members rows", dict(members=torch.zeros((4, 2), dtype=torch.int32))),
            ("seg_off start", dict(seg_off=[1, 2, 6])),
            ("seg_off order", dict(seg_off=[0, 7, 6])),
            ("track_off start", dict(track_off=[1, 2, 5])),
            ("track_off order", dict(track_off=[0, 6, 5])),
            ("track_off empty", dict(track_off=[])),
            ("cameras count", dict(cameras=np.zeros((3, 3, 4)))),
            ("cameras shape", dict(cameras=np.zeros((2, 3, 3)))),
            ("cameras list count", dict(cameras=[None, np.zeros((3, 4)), None])),
            ("use count", dict(use=[1, 1, 1])),
            ("max_error", dict(max_error=float("nan")))):
        with pytest.raises(ValueError):
            device.triangulate_tracks(**dict(good, **over))
    coords = [np.zeros((2, 2)), np.zeros((4, 3))]
    hgood = dict(coords=coords, sizes=[2, 4], cameras=[np.zeros((3, 4)), None], track_off=off, members=np.zeros((5, 2), np.int32))
    for what, over in (
            ("coords columns", dict(coords=[np.zeros((2, 1)), np.zeros((4, 3))])),
            ("coords rows", dict(coords=[np.zeros((3, 2)), np.zeros((4, 3))])),
            ("sizes negative", dict(sizes=[2, -4])),
            ("cameras count", dict(cameras=[None])),
            ("camera shape", dict(cameras=[np.zeros((4, 4)), None])),
            ("use count", dict(use=[1])),
            ("track_off start", dict(track_off=[1, 2, 5])),
            ("track_off end", dict(track_off=[0, 2, 4])),
            ("members shape", dict(members=np.zeros((5, 3), np.int32))),
            ("members dtype", dict(members=np.zeros((5, 2)))),
            ("max_error", dict(max_error=float("nan")))):
        with pytest.raises(ValueError):
            mvg.triangulate_tracks(**dict(hgood, **over))
    # nothing to do: no device is needed
    X, err, ok, nused = mvg.triangulate_tracks(coords, [2, 4], [np.zeros((3, 4)), None], [0], np.zeros((0, 2), np.int32))
    assert X.shape == (0, 4) and err.shape == (0,) and ok.shape == (0,) and nused.shape == (0,)
