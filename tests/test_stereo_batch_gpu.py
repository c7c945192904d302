"""stereo_batch, stereo_keep_batch and stereo_matches_batch on the GPU against tests/stereo_model.py: every output
element equal to the numpy statement of the contract, with the outputs pre-filled with garbage so that an element
the kernel leaves unwritten shows.  One collection of windows serves all cases; the model's results are computed
once per (radius, ranges, direction) and shared."""
import ctypes as ct
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests import stereo_model as sm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 128  # disparities per staging of the other image's rows (spectavi_amd/csrc/stereo_batch.hip)
TILE = 64    # columns of an item

# The kernel instantiations stereo_batch.hip launches: the cost kernel per radius, the fill of the pairs that are not
# used, the keep kernel and the four kernels of the compaction.  The set is held against the built library's code
# objects; that the cases below launch each of them is by construction, not traced: test_every_radius runs radii 0..7
# over a collection with a pair that is not used (stereo_none_kernel), test_keep the keep kernel, and
# test_matches_equal_the_model the count, scan, offsets and -- with kept samples -- fill kernels.
INSTANTIATED = {"stereo_batch_kernel<%d>" % r for r in range(8)} | {
    "stereo_none_kernel", "stereo_keep_kernel", "stereo_matches_count_kernel", "stereo_matches_scan_kernel",
    "stereo_matches_offsets_kernel", "stereo_matches_fill_kernel"}


def synthetic(a, b):
    idx = np.arange(a.size, dtype=np.int32).reshape(a.shape)
    return np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8), idx, idx.copy()


def seam_window():
    """Radius 0: the reference is 100 everywhere, the other image 200 but for two columns per row pair, one of
    value 100 (cost 0) and one of 101 (cost 1), 1, 2 or 3 columns apart in either order.  Over the reference
    columns of a row the two disparities c - x sweep the whole range, so for some x the best and the second best
    sit on either side of every chunk seam."""
    R, C = 12, 200
    a = np.full((R, C), 100, np.uint8)
    b = np.full((R, C), 200, np.uint8)
    for k, (dist, flip) in enumerate((d, f) for d in (1, 2, 3) for f in (0, 1)):
        for y, c in ((2 * k, 90), (2 * k + 1, 140)):
            b[y, c], b[y, c + dist] = (101, 100) if flip else (100, 101)
    return synthetic(a, b)


@functools.lru_cache(maxsize=None)
def collection():
    rng = np.random.default_rng(2024)
    scene = sm.plane_window(1)[:4]
    wide = sm.plane_window(2, 300, 40)[:4]
    assert scene[0].shape == (68, 115) and wide[0].shape[1] == 360  # 360: more than one tile, no multiple of 64
    holes = [a.copy() for a in scene]
    for v, ri in ((holes[0], holes[2]), (holes[1], holes[3])):
        m = rng.random(ri.shape) < 0.05
        m[:8], m[-8:], m[:, :8], m[:, -8:] = False, False, False, False  # the interior
        ri[m], v[m] = -1, 0

    def noise(R, C):
        return synthetic(rng.integers(0, 256, (R, C)), rng.integers(0, 256, (R, C)))
    table = [
        ("scene", scene, (-24, 8), 1),                                              # 0: 33 disparities
        ("wide", wide, (-100, 29), 1),                                              # 1: 130, the chunk seam is crossed
        ("holes", holes, (-24, 8), 1),                                              # 2
        ("constant", synthetic(np.full((12, 40), 77), np.full((12, 40), 77)), (-500, 500), 1),   # 3: past both edges
        ("black-white", synthetic(np.zeros((20, 40)), np.full((20, 40), 255)), (-3, 3), 1),       # 4
        ("noise", noise(30, 70), (-1, 1), 1),                                       # 5: 3 disparities
        ("1x1", noise(1, 1), (-2, 2), 1),                                           # 6
        ("5x9", noise(5, 9), (-2, 2), 1),                                           # 7
        ("9x14", noise(9, 14), (-2, 2), 1),                                         # 8: width 2r at r = 7
        ("9x6", noise(9, 6), (-2, 2), 1),                                           # 9: ... at r = 3
        ("9x2", noise(9, 2), (-2, 2), 1),                                           # 10: ... at r = 1
        ("unused", noise(6, 50), (-2, 2), 0),                                       # 11
        ("empty", None, (0, 0), 1),                                                 # 12
        ("scene again", scene, (-24, 8), 1),                                        # 13
        ("seam", seam_window(), (-150, 150), 1),                                    # 14: 301, three chunks
        ("noise wide range", noise(9, 150), (-32767, 32767), 1),                    # 15
    ]
    box, flats = [], [[], [], [], []]
    for k, (_, w, _, _) in enumerate(table):
        if w is None:
            box.append((3, 3, 5, 9))
            continue
        R, C = w[0].shape
        box.append((k, k + R, 2 * k, 2 * k + C))
        for f, a in zip(flats, w):
            f.append(a.ravel())
    flats = [np.concatenate(f) for f in flats]
    return SimpleNamespace(names=[t[0] for t in table], box=np.array(box, np.int32), flats=flats,
                           drange=[t[2] for t in table], use=[t[3] for t in table], off=sm.out_offsets(box))


@functools.lru_cache(maxsize=None)
def want(radius, drange=None, swap=0):
    col = collection()
    dr = col.drange if drange is None else [drange] * len(col.box)
    out = sm.stereo_batch(*col.flats, col.box, col.use, radius, dr, swap)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def on_device():
    import torch
    return [torch.from_numpy(f).cuda() for f in collection().flats]


def run(radius, drange=None, swap=0, garbage=0x1234):
    """spv_stereo_batch_device into outputs full of garbage -> (disp, cost, cost2) as numpy arrays."""
    import torch
    from spectavi_amd import device
    col = collection()
    n = int(col.off[-1])
    disp = torch.full((n,), 1000000 + garbage, dtype=torch.int32, device="cuda")
    cost = torch.from_numpy(np.full(n, garbage, np.uint16)).cuda()
    cost2 = torch.from_numpy(np.full(n, garbage + 1, np.uint16)).cuda()
    device.stereo_batch_into(*on_device(), col.box, col.use, radius, col.drange if drange is None else drange, swap,
                             disp, cost, cost2)
    torch.cuda.synchronize()
    return disp.cpu().numpy(), cost.cpu().numpy(), cost2.cpu().numpy()


def same(got, exp, what):
    col = collection()
    for name, g, w in zip(("disp", "cost", "cost2"), got, exp):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype)
        bad = np.flatnonzero(g != w)
        if bad.size:
            p = int(np.searchsorted(col.off, bad[0], "right")) - 1
            y, x = divmod(int(bad[0] - col.off[p]), int(col.box[p][3] - col.box[p][2]))
            raise AssertionError("%s: %s differs at %d samples, first in window %d (%s) at (%d, %d): got %d, want %d"
                                 % (what, name, bad.size, p, col.names[p], y, x, g[bad[0]], w[bad[0]]))


def test_kernel_coverage_lists_the_instantiations():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_coverage.py"), "--list",
                          "--files", "stereo_batch.hip"], check=True, capture_output=True, text=True).stdout
    listed = {ln.strip() for ln in out.splitlines() if ln.startswith("  ")}
    assert listed == INSTANTIATED, out


@pytest.mark.parametrize("radius", range(8))
def test_every_radius(radius):
    """The whole collection with its own ranges: the scene, 360 columns, holes, constant images, 0 against 255,
    noise, the tiny windows, the window of width 2r, a pair that is not used, an empty box, a pair twice."""
    col = collection()
    exp = want(radius)
    same(run(radius), exp, "radius %d" % radius)
    off = col.off
    w = {n: p for p, n in enumerate(col.names)}
    narrow = {7: "9x14", 3: "9x6", 1: "9x2"}.get(radius)
    if narrow:
        assert (exp[0][off[w[narrow]]:off[w[narrow] + 1]] == sm.NONE).all()
    assert (exp[0][off[w["unused"]]:off[w["unused"] + 1]] == sm.NONE).all() and off[w["empty"]] == off[w["empty"] + 1]
    assert np.array_equal(exp[0][off[0]:off[1]], exp[0][off[w["scene again"]]:off[w["scene again"] + 1]])
    const = sm.window(exp[0], w["constant"], col.box, off)
    if radius <= 5:  # every cost ties: the smallest admissible d, which the window's edge sets
        assert const[6, 20] == radius - 20 and sm.window(exp[1], w["constant"], col.box, off)[6, 20] == 0
    bw = sm.window(exp[1], w["black-white"], col.box, off)
    assert bw[10, 20] == (2 * radius + 1) ** 2 * 255 and (radius < 7 or bw[10, 20] == 57375)
    if radius == 0:
        nz = slice(off[w["noise wide range"]], off[w["noise wide range"] + 1])
        assert int((exp[1][nz] == exp[2][nz]).sum()) > 100  # best and second best tie: the tie rule decides


RANGES = [(-6, -6), (2, 9), (-20, -3), (-1, 1), (-24, 8), (-100, 29), (-500, 500)]


@pytest.mark.parametrize("drange", RANGES, ids=["%d..%d" % r for r in RANGES])
@pytest.mark.parametrize("radius", [0, 3])
def test_disparity_ranges(radius, drange):
    """One value, all positive, all negative, 3, 33 and 130 wide, past both edges of every window -- the same range
    for every pair."""
    same(run(radius, drange), want(radius, drange), "range %s" % (drange,))


def test_seam_case_crosses_the_chunk_seams():
    """The seam window puts best and second best on either side of a seam of the kernel's chunks, at distances 1, 2
    and 3 in both orders; at distance 1 the neighbour is excluded (cost2 = 100), at 2 and 3 it is the second best."""
    col = collection()
    p = col.names.index("seam")
    disp, cost, cost2 = (sm.window(a, p, col.box, col.off) for a in want(0))
    R, C = disp.shape
    lo_tile = np.array([max(-150, 0 - (min(c0 + TILE, C) - 1)) for c0 in range(0, C, TILE)])
    crossed = set()
    for k, (dist, flip) in enumerate((d, f) for d in (1, 2, 3) for f in (0, 1)):
        for y, c in ((2 * k, 90), (2 * k + 1, 140)):
            x = np.arange(C)
            best, second = (c + dist - x, c - x) if flip else (c - x, c + dist - x)
            assert np.array_equal(disp[y], best) and (cost[y] == 0).all()
            assert (cost2[y][second + x < C] == (100 if dist == 1 else 1)).all()
            lo = lo_tile[x // TILE]
            if (((best - lo) // CHUNK != (second - lo) // CHUNK) & (second + x < C)).any():
                crossed.add((dist, flip))
    assert crossed == {(d, f) for d in (1, 2, 3) for f in (0, 1)}
    same(run(0), want(0), "seam")


def test_swap_is_the_exchanged_call():
    import torch
    from spectavi_amd import device
    col = collection()
    r0, r1, ri0, ri1 = on_device()
    got = run(3, swap=1)
    same(got, want(3, swap=1), "swap")
    ex = device.stereo_batch(r1, r0, ri1, ri0, col.box, col.drange, radius=3, use=col.use)
    torch.cuda.synchronize()
    same([t.cpu().numpy() for t in ex], got, "exchanged inputs")
    (a, b) = device.stereo_batch(r0, r1, ri0, ri1, col.box, col.drange, radius=3, use=col.use, both=True)
    torch.cuda.synchronize()
    same([t.cpu().numpy() for t in a], want(3), "both: direction 0")
    back = sm.stereo_batch(*col.flats, col.box, col.use, 3, [(-h, -l) for l, h in col.drange], 1)
    same([t.cpu().numpy() for t in b], back, "both: direction 1")


def test_two_runs_give_the_same_bits():
    a, b = run(5, garbage=0x1111), run(5, garbage=0x2222)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_a_stream_and_the_tables_of_earlier_calls():
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for radius, rng in ((2, None), (0, (-1, 1)), (2, None)):
            same(run(radius, rng), want(radius, rng), "stream")
    s.synchronize()


@functools.lru_cache(maxsize=None)
def both_directions():
    col = collection()
    d0 = want(3)
    d1 = sm.stereo_batch(*col.flats, col.box, col.use, 3, [(-h, -l) for l, h in col.drange], 1)
    return d0, d1


@pytest.mark.parametrize("with_back", [False, True])
@pytest.mark.parametrize("lr_tol,uniqueness", [(0, 0), (2, 10), (0, 100), (2, 0), (1, 10)])
def test_keep(with_back, lr_tol, uniqueness):
    import torch
    from spectavi_amd import device
    col = collection()
    (disp0, cost0, cost20), (disp1, _, _) = both_directions()
    exp = sm.keep_batch(col.box, disp0, cost0, cost20, disp1 if with_back else None, lr_tol, uniqueness)
    t = [torch.from_numpy(np.array(a)).cuda() for a in (disp0, cost0, cost20, disp1)]
    got = device.stereo_keep_batch(col.box, t[0], t[1], t[2], t[3] if with_back else None, lr_tol, uniqueness)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, exp), np.flatnonzero(got != exp)[:5]
    assert 0 < int(exp.sum()) <= int((disp0 != sm.NONE).sum())
    assert (uniqueness, with_back) == (0, False) or int(exp.sum()) < int((disp0 != sm.NONE).sum())


@functools.lru_cache(maxsize=None)
def kept_case():
    col = collection()
    (disp0, cost0, cost20), (disp1, _, _) = both_directions()
    kept = sm.keep_batch(col.box, disp0, cost0, cost20, disp1, 1, 10)
    n = len(col.box)
    sizes = [(96, 64), (300, 40), (101, 77)]  # the images of a pair may differ in width
    pairs = [(0, 0), (1, 1)] + [(0, 2)] * (n - 2)
    return kept, sizes, pairs, sm.matches_batch(col.box, sizes, pairs, disp0, kept, col.flats[2], col.flats[3])


def test_matches_equal_the_model():
    import torch
    from spectavi_amd import device
    col = collection()
    disp0 = both_directions()[0][0]
    kept, sizes, pairs, (x0, x1, rows, pair_off) = kept_case()
    assert len(rows) > 5000 and len(set(np.diff(pair_off).tolist())) > 4
    _, _, ri0, ri1 = on_device()
    got = device.stereo_matches_batch(col.box, sizes, pairs, torch.from_numpy(np.array(disp0)).cuda(),
                                      torch.from_numpy(kept).cuda(), ri0, ri1)
    torch.cuda.synchronize()
    assert np.array_equal(got[3], pair_off) and got[3].dtype == np.int64
    assert np.array_equal(got[0].cpu().numpy(), x0) and np.array_equal(got[1].cpu().numpy(), x1)
    assert np.array_equal(got[2].cpu().numpy(), rows) and got[2].dtype == torch.int32
    # nothing kept at all
    none = device.stereo_matches_batch(col.box, sizes, pairs, torch.from_numpy(np.array(disp0)).cuda(),
                                       torch.zeros(len(kept), dtype=torch.uint8, device="cuda"), ri0, ri1)
    assert none[0].shape == (0, 3) and none[2].shape == (0,) and not none[3].any() and len(none[3]) == len(col.box) + 1


@pytest.mark.parametrize("capacity", [0, 1, 1025, 4000])
def test_matches_capacity(capacity):
    """A capacity below the count: the first `capacity` matches are written, nothing past them, and pair_off still
    holds the true counts."""
    import torch
    from spectavi_amd._lib import check, clib
    col = collection()
    disp0 = both_directions()[0][0]
    kept, sizes, pairs, (x0, x1, rows, pair_off) = kept_case()
    assert capacity < len(rows)
    _, _, ri0, ri1 = on_device()
    G = 64
    d_x0 = torch.full((capacity + G, 3), -7., dtype=torch.float64, device="cuda")
    d_x1 = torch.full((capacity + G, 3), -8., dtype=torch.float64, device="cuda")
    d_rows = torch.full((capacity + G,), -9, dtype=torch.int32, device="cuda")
    d_off = torch.full((len(col.box) + 1,), -1, dtype=torch.int64, device="cuda")
    d_disp, d_keep = torch.from_numpy(np.array(disp0)).cuda(), torch.from_numpy(kept).cuda()
    sz, pr = np.array(sizes, np.int32), np.array(pairs, np.int32)
    check(clib.spv_stereo_matches_batch_device(col.box.ctypes.data, len(col.box), sz.ctypes.data, len(sz), pr.ctypes.data,
                                               d_disp.data_ptr(), d_keep.data_ptr(), ri0.data_ptr(), ri1.data_ptr(),
                                               capacity, d_x0.data_ptr(), d_x1.data_ptr(), d_rows.data_ptr(),
                                               d_off.data_ptr(), ct.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(d_off.cpu().numpy(), pair_off)
    assert np.array_equal(d_x0.cpu().numpy()[:capacity], x0[:capacity]) and (d_x0.cpu().numpy()[capacity:] == -7.).all()
    assert np.array_equal(d_x1.cpu().numpy()[:capacity], x1[:capacity]) and (d_x1.cpu().numpy()[capacity:] == -8.).all()
    assert np.array_equal(d_rows.cpu().numpy()[:capacity], rows[:capacity]) and (d_rows.cpu().numpy()[capacity:] == -9).all()


def test_chain_from_rectify_batch_to_points():
    """The plane scene through the device chain, rectify_batch -> stereo_batch(both) -> stereo_keep_batch ->
    stereo_matches_batch -> dlt_triangulate_batch: every step equals the model run on the device's own rectified
    windows, and the cloud meets the two conditions of tests/test_stereo_model.py."""
    import torch
    from spectavi_amd.scenes import plane_distance, plane_scene
    from spectavi_amd import device
    im0, im1, P0, P1 = plane_scene(96, 64, 1)
    ims = [torch.from_numpy(im0).cuda(), torch.from_numpy(im1).cuda()]
    pairs, sizes = [(0, 1), (0, 1)], [(96, 64), (96, 64)]
    r0, r1, ri0, ri1, box, out_off = device.rectify_batch(ims, None, pairs, [P1, P1], [P0, P0])
    oracle = sm.plane_window(1)
    flats = [t.cpu().numpy() for t in (r0, r1, ri0, ri1)]
    for f, w in zip(flats, oracle[:4]):  # the windows of rectify_batch are the oracle's crop, twice
        assert np.array_equal(f, np.concatenate([w.ravel(), w.ravel()]))
    (d0, c0, c20), (d1, _, _) = device.stereo_batch(r0, r1, ri0, ri1, box, (-24, 8), radius=7, both=True)
    kept = device.stereo_keep_batch(box, d0, c0, c20, d1, lr_tol=1, uniqueness=10)
    x0, x1, rows, pair_off = device.stereo_matches_batch(box, sizes, pairs, d0, kept, ri0, ri1)
    X, x_off = device.dlt_triangulate_batch(x0, x1, pair_off, [P1, P1], [P0, P0])
    torch.cuda.synchronize()
    m0 = sm.stereo_batch(*flats, box, None, 7, [(-24, 8)] * 2)
    m1 = sm.stereo_batch(*flats, box, None, 7, [(-8, 24)] * 2, swap=1)
    same([t.cpu().numpy() for t in (d0, c0, c20)], m0, "chain, direction 0")
    assert np.array_equal(d1.cpu().numpy(), m1[0])
    mk = sm.keep_batch(box, *m0, m1[0], 1, 10)
    assert np.array_equal(kept.cpu().numpy(), mk)
    mx0, mx1, mrows, moff = sm.matches_batch(box, sizes, pairs, m0[0], mk, flats[2], flats[3])
    assert np.array_equal(pair_off, moff) and np.array_equal(x_off, moff) and np.array_equal(rows.cpu().numpy(), mrows)
    assert np.array_equal(x0.cpu().numpy(), mx0) and np.array_equal(x1.cpu().numpy(), mx1)
    X = X.cpu().numpy()
    dist = plane_distance(X[:, :3] / X[:, 3:4])
    share = float(mk.sum()) / int((m0[0] != sm.NONE).sum())
    print("kept share %.4f, largest distance from the plane %.4f, median %.4f" % (share, dist.max(), np.median(dist)))
    assert share >= 0.9 and dist.max() <= 1.0
    n = int(moff[1])
    assert n > 4000 and np.array_equal(X[:n], X[n:])  # the same pair twice: the same points


def test_profile_names():
    import torch
    from spectavi_amd import device
    col = collection()
    kept, sizes, pairs, _ = kept_case()
    (disp0, cost0, cost20), _ = both_directions()
    t = [torch.from_numpy(np.array(a)).cuda() for a in (disp0, cost0, cost20)]
    device.profile_reset()
    device.profile_enable(True)
    run(1)
    device.stereo_keep_batch(col.box, *t)
    device.stereo_matches_batch(col.box, sizes, pairs, t[0], torch.from_numpy(kept).cuda(), *on_device()[2:])
    device.profile_enable(False)
    for name, calls in (("stereo_batch", 1), ("stereo_keep_batch", 1), ("stereo_matches_count", 2), ("stereo_matches_fill", 1)):
        n, ms = device.profile_read(name)
        assert n == calls and ms > 0, name
