"""triangulate_tracks on the GPU against tests/tracks_triangulate_model.py (numpy.linalg.svd of the 2m x 4 matrix).

The scenes are the model file's: K with f = 1000, 40 cameras with rotations of 0.05-0.25 rad at distance 1 (`wide`),
12 cameras K [I | t] with |t| = 2e-3 (`narrow`, the set on which a Gram-matrix solver leaves ||A X|| above sigma4 +
1e-13 sigma1), points x in +-2.5, y in +-1.8, z in 4-8, observations rounded to float32.

The two forms of the kernel (one lane per track up to L = 16 members, one wave per longer track) are driven on the
same input through tracks_triangulate_set_long.  For tracks of more than 64 members the residual criterion's 1e-13
sigma1 becomes max(1e-13, 8 c m eps) sigma1, c being the worst excess of the model's own float64 QR route
(numpy.linalg.qr, then the SVD of R) in units of m eps sigma1 on the same tracks.  Measured on the tracks of
`edges` (65, 129 and 1000 members, 0.5 px noise): c = 0 -- the QR route stays inside sigma4 (1 + 1e-9) + 2 formation on
every one of them -- so the floor 1e-13 sigma1 is the bound in force for every length tested here."""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import tracks_triangulate_model as ttm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANTIATED = {"tracks_triangulate_lane_kernel", "tracks_triangulate_wave_kernel"}
PROFILE_NAMES = ("tracks_triangulate", "tracks_triangulate_long")
INF = float("inf")
L0 = 16          # the default of tracks_triangulate_set_long


def run(geom, seg, cams, off, mem, max_error=INF, use=None):
    """device.triangulate_tracks on host arrays -> (X, err, ok, nused) as numpy arrays."""
    import torch
    from spectavi_amd import device
    out = device.triangulate_tracks(torch.from_numpy(np.ascontiguousarray(geom)).cuda(), seg, cams, off,
                                    torch.from_numpy(np.ascontiguousarray(mem, np.int32).reshape(-1, 2)).cuda(),
                                    max_error=max_error, use=use)
    return tuple(t.cpu().numpy() for t in out)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture
def long_setting():
    from spectavi_amd import device
    before = device.tracks_triangulate_get_long()
    assert before == L0
    yield device.tracks_triangulate_set_long
    device.tracks_triangulate_set_long(before)


def scene(seed, cams_kind, noise, lengths, distinct=True):
    rng = np.random.default_rng(seed)
    cams = ttm.wide_cameras(rng, 40) if cams_kind == "wide" else ttm.narrow_cameras(rng, 12)
    Xw = ttm.points(rng, len(lengths))
    geom, seg = ttm.observe(rng, cams, Xw, noise)
    off, mem = ttm.make_tracks(rng, lengths, len(cams), distinct)
    return dict(cams=cams, geom=geom, seg=seg, off=off, mem=mem, Xw=Xw)


def anchor_reference(sc, a, b):
    """device.dlt_triangulate_batch on the observations members[a], members[b] of every track (w = 1), each track a
    set of one row with P0 = the first member's camera and P1 = the second's: (X, err)."""
    import torch
    from spectavi_amd import device
    mem, seg, geom, cams = sc["mem"], sc["seg"], sc["geom"], sc["cams"]
    n = len(a)
    x0 = np.ones((n, 3))
    x1 = np.ones((n, 3))
    x0[:, :2] = geom[seg[mem[a, 0]] + mem[a, 1], :2]
    x1[:, :2] = geom[seg[mem[b, 0]] + mem[b, 1], :2]
    X, err, _ = device.dlt_triangulate_batch(torch.from_numpy(x0).cuda(), torch.from_numpy(x1).cuda(), np.arange(n + 1),
                                             cams[mem[b, 0]].reshape(n, 12), P0s=cams[mem[a, 0]].reshape(n, 12),
                                             want_error=True)
    return X.cpu().numpy(), err.cpu().numpy()


@pytest.mark.parametrize("calibrated", [False, True], ids=["pixel", "calibrated"])
def test_two_member_anchor(calibrated):
    sc = scene(21, "wide", 0.5, [2] * 3000)
    if calibrated:
        sc["cams"], sc["geom"] = ttm.calibrate(ttm.intrinsics(), sc["cams"], sc["geom"])
    X, err, ok, nused = run(sc["geom"], sc["seg"], sc["cams"], sc["off"], sc["mem"])
    a = sc["off"][:-1]
    rX, rerr = anchor_reference(sc, a, a + 1)
    assert same_bits(X, rX), np.flatnonzero((bits(X) != bits(rX)).any(1))[:8]
    assert same_bits(err[a] + err[a + 1], rerr)
    assert np.all(nused == 2) and ok.dtype == np.uint8 and nused.dtype == np.int32


DEFINITION_CASES = {
    # name: (cameras, noise px, calibrated, max_error: between the residuals of the noise and a planted outlier)
    "wide-exact": ("wide", 0.0, False, 1e-2),
    "wide-noise": ("wide", 0.5, False, 6.0),
    "narrow-exact": ("narrow", 0.0, False, 1e-2),
    "narrow-noise": ("narrow", 0.5, False, 6.0),
    "wide-noise-calibrated": ("wide", 0.5, True, 6.0e-3),
}


@pytest.mark.parametrize("case", sorted(DEFINITION_CASES))
def test_definition(case):
    kind, noise, calibrated, max_error = DEFINITION_CASES[case]
    sc = scene(22, kind, noise, [2, 3, 4, 5, 8, 12] * 100)
    if calibrated:
        sc["cams"], sc["geom"] = ttm.calibrate(ttm.intrinsics(), sc["cams"], sc["geom"])
    args = (sc["geom"], sc["seg"], sc["cams"], sc["off"], sc["mem"])
    mo = ttm.model(*args, max_error=max_error)
    X, err, ok, nused = run(*args, max_error=max_error)
    st = ttm.check_definition(X, err, mo, sc["geom"], sc["seg"], sc["off"], sc["mem"], what=case)
    und = ttm.check_verdict(ok, nused, mo, sc["geom"], sc["seg"], sc["off"], sc["mem"], max_error, what=case)
    print(case, st, "undecided", und, "ok", int(ok.sum()))
    assert st["tracks"] == st["well_separated"] == 600, "every track of these scenes is well separated"


# ---- length edges -----------------------------------------------------------------------------------------------------
EDGE_LONG = [L0 - 1, L0, L0 + 1, 63, 64, 65, 129, 1000]     # L - 1, L, L + 1 for the default L, the wave's edges, long ones


@pytest.fixture(scope="module")
def edges():
    """8 edge-length tracks, then 255 tracks of 2-5 members; members drawn with repetition from the 40 sets.  The
    model, with its float64 QR route, once."""
    lengths = EDGE_LONG + [2, 3, 4, 5] * 63 + [2, 3, 4]
    sc = scene(23, "wide", 0.5, lengths, distinct=False)
    sc["lengths"] = np.array(lengths)
    sc["mo"] = ttm.model(sc["geom"], sc["seg"], sc["cams"], sc["off"], sc["mem"], max_error=6.0, qr_route=True)
    sc["long_c"] = float(sc["mo"]["qr_excess"][sc["lengths"] > 64].max())
    return sc


def prefix(sc, nt):
    """The first nt tracks of a scene and of its model."""
    nm = int(sc["off"][nt])
    mo = {k: (v[:nt] if len(v) == len(sc["off"]) - 1 else v[:nm]) for k, v in sc["mo"].items()}
    return dict(sc, off=sc["off"][:nt + 1], mem=sc["mem"][:nm], lengths=sc["lengths"][:nt], mo=mo)


@pytest.mark.parametrize("lane_tracks", [249, 250, 251, 255, 256, 257])
def test_length_edges(edges, long_setting, lane_tracks):
    """lane_tracks tracks in the lane form under the default L, 6 in the wave form: 255, 256 and 257 lane-form tracks,
    and 255, 256 and 257 tracks in all (the lane launch has one lane per track of the call); then all of 3 or more
    members in the wave form, then none."""
    from spectavi_amd import device
    sc = prefix(edges, lane_tracks + 6)
    args = (sc["geom"], sc["seg"], sc["cams"], sc["off"], sc["mem"])
    mo, lengths = sc["mo"], sc["lengths"]
    print("float64 QR route: worst excess %.3g m eps sigma1" % sc["long_c"])
    res = {}
    for setting, waves in ((L0, 6), (0, int((lengths >= 3).sum())), (10 ** 9, 0)):
        long_setting(setting)
        plan = device.triangulate_tracks_plan(sc["off"])
        assert (plan["lane_tracks"], plan["wave_tracks"]) == (len(lengths) - waves, waves)
        if setting == L0:
            assert plan["lane_tracks"] == lane_tracks and plan["lane_groups"] == (lane_tracks + 6 + 255) // 256
        res[setting] = run(*args, max_error=6.0)
        X, err, ok, nused = res[setting]
        st = ttm.check_definition(X, err, mo, sc["geom"], sc["seg"], sc["off"], sc["mem"], long_c=sc["long_c"],
                                  what="L = %d" % setting)
        ttm.check_verdict(ok, nused, mo, sc["geom"], sc["seg"], sc["off"], sc["mem"], 6.0, what="L = %d" % setting)
        print("L = %d" % setting, st)
    S = mo["S"]
    tol = (64 * ttm.EPS * S[:, 0] * lengths / 2) / (S[:, 2] - S[:, 3]) + 1e-15
    for other in (0, 10 ** 9):
        diff = np.abs(res[L0][0] - res[other][0]).max(axis=1)
        assert np.all(diff <= tol), (other, np.flatnonzero(diff > tol)[:8], diff.max())
    two = np.flatnonzero(lengths == 2)
    mtwo = np.repeat(lengths == 2, lengths)
    for other in (0, 10 ** 9):
        assert same_bits(res[L0][0][two], res[other][0][two]) and same_bits(res[L0][1][mtwo], res[other][1][mtwo])
        assert np.array_equal(res[L0][2], res[other][2]) and np.array_equal(res[L0][3], res[other][3])
    # the lane form is one code path whatever L: identical bits for the tracks that stayed in it
    lane = np.flatnonzero(lengths <= L0)
    assert same_bits(res[L0][0][lane], res[10 ** 9][0][lane])


# ---- determinism ------------------------------------------------------------------------------------------------------
def select(sc, order):
    """The tracks `order` of a scene as a call of their own: (off, mem, member index of every new member)."""
    off = sc["off"]
    idx = np.concatenate([np.arange(off[t], off[t + 1]) for t in order]) if len(order) else np.zeros(0, np.int64)
    noff = np.concatenate([[0], np.cumsum([off[t + 1] - off[t] for t in order])]).astype(np.int64)
    return noff, sc["mem"][idx], idx


def test_determinism(edges):
    sc = edges
    args = (sc["geom"], sc["seg"], sc["cams"])
    nt = len(sc["off"]) - 1
    base = run(*args, sc["off"], sc["mem"], max_error=6.0)
    for _ in range(4):
        again = run(*args, sc["off"], sc["mem"], max_error=6.0)
        assert all(same_bits(a, b) for a, b in zip(base, again))
    rng = np.random.default_rng(5)

    def check(order, got, idx):
        assert same_bits(got[0], base[0][order]) and same_bits(got[1], base[1][idx])
        assert np.array_equal(got[2], base[2][order]) and np.array_equal(got[3], base[3][order])
    order = rng.permutation(nt)
    off, mem, idx = select(sc, order)
    check(order, run(*args, off, mem, max_error=6.0), idx)
    for order in (np.arange(0, 100), np.arange(100, nt)):          # split over two calls
        off, mem, idx = select(sc, order)
        check(order, run(*args, off, mem, max_error=6.0), idx)
    # embedded among other tracks: every track twice over, the copies reversed, in between
    order = np.concatenate([[t, nt - 1 - t] for t in range(nt)])
    off, mem, idx = select(sc, order)
    got = run(*args, off, mem, max_error=6.0)
    check(order, got, idx)


# ---- unusable input ---------------------------------------------------------------------------------------------------
def test_unusable_input(long_setting):
    rng = np.random.default_rng(24)
    cams = list(ttm.wide_cameras(rng, 40))
    nt = 320
    Xw = ttm.points(rng, nt)
    geom, seg = ttm.observe(rng, np.array(cams), Xw, 0.5)
    # an empty set between sets 1 and 2: 41 sets, the camera of the empty one is never used
    seg = np.concatenate([seg[:2], seg[1:]]).astype(np.int64)
    cams.insert(1, np.full((3, 4), np.nan))
    nseg = 41
    off, mem = ttm.make_tracks(rng, [5] * nt, 40)
    mem[:, 0] += mem[:, 0] >= 1                       # the sets behind the empty one move up
    use = np.ones(nseg, np.int32)
    use[7] = 0
    cams[11] = None
    npts = nt
    for t in range(nt):
        m = mem[off[t]:off[t + 1]]
        k = t % 8
        if k == 1:
            m[2, 0] = -1
        elif k == 2:
            m[0, 0], m[4, 0] = nseg, 2 ** 31 - 1
        elif k == 3:
            m[0, 1], m[2, 1], m[3, 1] = -1, npts, 2 ** 31 - 1       # 2 usable of 5 (unless a set is switched off)
        elif k == 4:
            m[:4, 0] = [-1, nseg, -2 ** 31, 1]                       # set 1 is the empty one: row t is outside it
        elif k == 5:
            m[:, 0] = [-5, nseg + 3, 1, 7, 11]                       # none usable
        elif k == 6:
            m[1, 0], m[3, 0] = 7, 11                                 # a set switched off, a set without a camera
    mcams = np.array([np.zeros((3, 4)) if P is None else P for P in cams])
    muse = use.copy()
    muse[11] = 0
    mo = ttm.model(geom, seg, mcams, off, mem, max_error=6.0, use=muse)
    assert set(mo["nused"].tolist()) >= {0, 1, 2, 3, 4, 5}
    res = {}
    for setting in (L0, 0):
        long_setting(setting)
        X, err, ok, nused = res[setting] = run(geom, seg, cams, off, mem, max_error=6.0, use=use)
        ttm.check_definition(X, err, mo, geom, seg, off, mem, what="unusable, L = %d" % setting)
        ttm.check_verdict(ok, nused, mo, geom, seg, off, mem, 6.0, what="unusable, L = %d" % setting)
        assert np.all(X[nused < 2] == 0) and np.all(ok[nused < 2] == 0)
        assert np.all(np.isnan(err[np.repeat(nused < 2, 5)]))
    long_setting(L0)
    # exactly 2 usable of 5: the two-member anchor's bits, in both forms
    two = np.flatnonzero(mo["nused"] == 2)
    assert len(two) >= 30
    first = np.array([off[t] + np.flatnonzero(mo["usable"][off[t]:off[t + 1]])[0] for t in two])
    second = np.array([off[t] + np.flatnonzero(mo["usable"][off[t]:off[t + 1]])[1] for t in two])
    sc = dict(mem=mem, seg=seg, geom=geom, cams=mcams)
    rX, rerr = anchor_reference(sc, first, second)
    for setting in (L0, 0):
        X, err = res[setting][:2]
        assert same_bits(X[two], rX) and same_bits(err[first] + err[second], rerr), setting
    # nothing to do, and tracks without members
    X, err, ok, nused = run(geom, seg, cams, [0], np.zeros((0, 2), np.int32), use=use)
    assert X.shape == (0, 4) and err.shape == (0,) and ok.shape == (0,) and nused.shape == (0,)
    X, err, ok, nused = run(geom, seg, cams, [0, 0, 0, 0], np.zeros((0, 2), np.int32), use=use)
    assert np.all(X == 0) and X.shape == (3, 4) and err.shape == (0,) and not ok.any() and not nused.any()
    X, err, ok, nused = run(np.zeros((0, 4), np.float32), [0], np.zeros((0, 3, 4)), [0, 2], [[0, 0], [3, 1]])
    assert np.all(X == 0) and np.isnan(err).all() and not ok.any() and not nused.any()


# ---- the verdict ------------------------------------------------------------------------------------------------------
def test_verdict():
    rng = np.random.default_rng(25)
    K = ttm.intrinsics()
    cams = list(ttm.wide_cameras(rng, 40))
    C = np.array([0.1, -0.2, 0.3])
    behind = K @ np.diag([-1.0, 1.0, -1.0]) @ np.hstack([np.eye(3), -C[:, None]])   # looks away from the scene
    cams += [behind, -cams[3]]                                                       # set 40; set 41 has det < 0
    cams = np.array(cams)
    assert np.linalg.det(cams[41][:, :3]) < 0 < np.linalg.det(cams[40][:, :3])
    nt = 400
    Xw = ttm.points(rng, nt)
    geom, seg = ttm.observe(rng, cams, Xw, 0.5)
    off, mem = ttm.make_tracks(rng, [4] * nt, 40)
    moved = np.arange(0, nt, 4)
    rows = seg[mem[off[moved] + 1, 0]] + mem[off[moved] + 1, 1]
    geom[rows, 0] += 20                                  # one observation of every fourth track, 20 px away
    mem[off[np.arange(1, nt, 4)] + 2, 0] = 40            # one observation from behind the camera
    mem[off[np.arange(2, nt, 4)] + 3, 0] = 41            # one observation through the camera of negative determinant
    kind = np.arange(nt) % 4
    for max_error in (3.0, INF):
        mo = ttm.model(geom, seg, cams, off, mem, max_error=max_error)
        X, err, ok, nused = run(geom, seg, cams, off, mem, max_error=max_error)
        ttm.check_definition(X, err, mo, geom, seg, off, mem, what="verdict")
        und = ttm.check_verdict(ok, nused, mo, geom, seg, off, mem, max_error, what="verdict")
        assert und == 0 and np.array_equal(ok, mo["ok"])
        assert not ok[kind == 1].any(), "a point behind one of its cameras"
        if max_error == 3.0:
            assert not ok[kind == 0].any() and np.all(err[off[moved] + 1] > 3)
            assert ok[kind >= 2].mean() > 0.95, "noise of 0.5 px stays under 3 px; a negative determinant is no fault"
        else:
            assert ok[kind != 1].all(), "without a residual bound only cheirality is left"


# ---- the raw call -----------------------------------------------------------------------------------------------------
def test_guards(edges, long_setting):
    """64 sentinel elements either side of X, err, ok and nused stay untouched, in both forms."""
    import torch
    from spectavi_amd._lib import clib, check
    sc = edges
    nt, nm, G = len(sc["off"]) - 1, len(sc["mem"]), 64

    def guarded(count, dtype, fill):
        t = torch.full((count + 2 * G,), fill, dtype=dtype, device="cuda")
        return t, t[G:G + count]
    geom = torch.from_numpy(sc["geom"]).cuda()
    mem = torch.from_numpy(sc["mem"]).cuda()
    cams = np.ascontiguousarray(sc["cams"].reshape(-1, 12))
    for setting in (L0, 0):
        long_setting(setting)
        bufs = {"X": guarded(4 * nt, torch.float64, -77.0), "err": guarded(nm, torch.float64, -77.0),
                "ok": guarded(nt, torch.uint8, 0xEE), "nused": guarded(nt, torch.int32, -77)}
        check(clib.spv_tracks_triangulate_device(geom.data_ptr(), sc["seg"].ctypes.data, len(sc["seg"]) - 1, cams.ctypes.data,
                                                 None, sc["off"].ctypes.data, nt, mem.data_ptr(), nm, 6.0,
                                                 *[bufs[k][1].data_ptr() for k in ("X", "err", "ok", "nused")],
                                                 ct.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        for name, (whole, inner) in bufs.items():
            fill = 0xEE if name == "ok" else -77
            assert bool((whole[:G] == fill).all()) and bool((whole[G + inner.numel():] == fill).all()), name
        assert np.array_equal(bufs["nused"][1].cpu().numpy(), sc["mo"]["nused"])
        assert bool((bufs["ok"][1] <= 1).all()) and not bool((bufs["X"][1] == -77.0).any())
    # err, ok and nused may be NULL
    X = torch.full((nt, 4), -77.0, dtype=torch.float64, device="cuda")
    check(clib.spv_tracks_triangulate_device(geom.data_ptr(), sc["seg"].ctypes.data, len(sc["seg"]) - 1, cams.ctypes.data, None,
                                             sc["off"].ctypes.data, nt, mem.data_ptr(), nm, 6.0, X.data_ptr(), None, None, None,
                                             ct.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert same_bits(X.cpu().numpy(), bufs["X"][1].cpu().numpy().reshape(nt, 4))


def test_host_form_equals_device_form(edges):
    from spectavi_amd import mvg
    sc = edges
    nseg = len(sc["seg"]) - 1
    coords = [sc["geom"][sc["seg"][s]:sc["seg"][s + 1], :3] for s in range(nseg)]
    cams = [None if s == 4 else sc["cams"][s] for s in range(nseg)]
    use = np.ones(nseg, np.int32)
    use[9] = 0
    host = mvg.triangulate_tracks(coords, None, cams, sc["off"], sc["mem"], max_error=6.0, use=use)
    dev = run(sc["geom"], sc["seg"], cams, sc["off"], sc["mem"], max_error=6.0, use=use)
    for h, d in zip(host, dev):
        assert h.dtype == d.dtype and same_bits(h, d)
    assert host[2].any() and (host[3] < sc["lengths"]).any()


# ---- the example's pipeline -------------------------------------------------------------------------------------------
def test_pipeline_track_points():
    from examples.multiview_from_sift_tables import multiview_pipeline, synthetic_sift_views
    tables, K, cameras = synthetic_sift_views(seed=3, n_views=4, n_points=300, return_cameras=True)
    out = multiview_pipeline(tables, K, tracks=True, triangulate=cameras)
    X, err, ok, nused = (t.cpu().numpy() for t in out["track_points"])
    track_off, members = out["tracks"][0], out["tracks"][1].cpu().numpy()
    assert len(track_off) - 1 > 100
    geom = np.concatenate(tables)[:, :4].copy()
    seg = out["track_inputs"]["seg_off"]
    mo = ttm.model(geom, seg, cameras, track_off, members)
    st = ttm.check_definition(X, err, mo, geom, seg, track_off, members, what="pipeline")
    ttm.check_verdict(ok, nused, mo, geom, seg, track_off, members, INF, what="pipeline")
    assert st["tracks"] == len(track_off) - 1 and np.array_equal(nused, np.diff(track_off))
    # the scene's own cameras and the scene's own points: the consistent tracks reproject within the float32 rounding
    assert np.nanmedian(err) < 1e-2


# ---- names ------------------------------------------------------------------------------------------------------------
def test_profile_names(edges, long_setting):
    from spectavi_amd import device
    sc = edges
    counts = {}
    device.profile_enable(True)
    try:
        for what, setting in (("both", L0), ("wave only", 0), ("lane only", 10 ** 9)):
            long_setting(setting)
            off = sc["off"]
            mem = sc["mem"]
            if what == "wave only":                       # no track of fewer than 3 members: no lane launch
                keep = np.flatnonzero(sc["lengths"] >= 3)
                off, mem, _ = select(sc, keep)
            device.profile_reset()
            run(sc["geom"], sc["seg"], sc["cams"], off, mem)
            counts[what] = [device.profile_read(k)[0] for k in PROFILE_NAMES]
    finally:
        device.profile_enable(False)
        device.profile_reset()
    assert counts == {"both": [1, 1], "wave only": [0, 1], "lane only": [1, 0]}


def test_kernel_coverage_lists_the_instantiations():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_coverage.py"), "--list",
                          "--files", "tracks_triangulate.hip"], check=True, capture_output=True, text=True).stdout
    listed = {ln.strip() for ln in out.splitlines() if ln.startswith("  ")}
    assert listed == INSTANTIATED, out
