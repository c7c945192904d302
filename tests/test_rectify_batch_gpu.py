"""rectify_batch on the GPU (device.rectify_batch_bounds / rectify_batch, spv_rectify_batch through
mvg.image_pair_rectification_batch) against the numpy statement of the contract, tests/rectify_oracle.py, driven by
the library's own F, and against the single calls: values compared bit for bit (float64 as uint64, float32 as
uint32), indices and boxes exactly."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from tests import rectify_oracle as ro
from tests import test_rectify_gpu as trg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF = 1.2
BOUNDS_ROWS = 16  # frame rows per item of the bounds step (include/spectavi_amd.h)
GROUPS_PER_CU = 32  # the grid cap of both steps

# The kernel instantiations rectify_batch.hip launches: the resampling kernel per element width, and the two kernels
# of the bounds step.
INSTANTIATED = {"rectify_batch_kernel<unsigned long>", "rectify_batch_kernel<unsigned int>",
                "rectify_batch_kernel<unsigned char>", "rectify_batch_bounds_kernel", "rectify_batch_box_kernel"}

DTYPES = [np.float64, np.float32, np.uint8]


def bits(a):
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def make_image(rng, hgt, wid, nchan, dtype):
    """test_rectify_gpu.image, and its float32 counterpart: NaN payloads, -0.0 and -inf planted, never computed."""
    if dtype != np.float32:
        return trg.image(rng, hgt, wid, nchan, dtype)
    shp = (hgt, wid) if nchan == 1 else (hgt, wid, nchan)
    im = (rng.standard_normal(shp) * 100).astype(np.float32)
    b = im.reshape(-1).view(np.uint32)
    b[::5] = 0x7FC0BEEF
    b[1::7] = 0xFFC00F0F
    b[2::11] = 0x80000000
    b[3::13] = 0xFF800000
    return im


def oracle_box(want):
    m = (want[2] != -1) | (want[3] != -1)
    if not m.any():
        return (0, 0, 0, 0)
    y, x = np.where(m)
    return (int(y.min()), int(y.max()) + 1, int(x.min()), int(x.max()) + 1)


def window(full, box):
    ys, xs = slice(box[0], box[1]), slice(box[2], box[3])
    return tuple(a[ys, xs, ...] for a in full)


def build(ims, pairs, P0s, P1s, use, sf=SF):
    """A collection with its oracle: want[p] the uncropped single-pair result (None where the pair is not used),
    box[p] the oracle's bounding box of the valid samples."""
    from spectavi_amd import mvg
    want, box = [], []
    for (a, b), P0, P1, u in zip(pairs, P0s, P1s, use):
        if not u:
            want.append(None)
            box.append((0, 0, 0, 0))
            continue
        want.append(ro.rectify(mvg.rectification_fundamental(P0, P1), ims[a], ims[b], sf))
        box.append(oracle_box(want[-1]))
    nchan = ro.dims(ims[0])[2]
    return SimpleNamespace(ims=ims, pairs=list(pairs), P0s=list(P0s), P1s=list(P1s), use=list(use), sf=sf, want=want,
                           box=np.array(box, np.int32).reshape(-1, 4), nchan=nchan)


# (wid, hgt): three sizes; 300 wide gives 360 output columns, more than one 256-lane stride and no multiple of it
SIZES = [(300, 40)] * 3 + [(96, 64)] * 2 + [(1, 9)]
EMPTY = (3, 4, 5, 7)  # not used, identical cameras, rank-deficient P0, rnx = 1
STEREO = (0, 1, 2, 8, 9)  # (the vertical-baseline pair 6 keeps column 0 of some rows, or nothing)


@functools.lru_cache(maxsize=None)
def mixed(dtype_name, nchan):
    dtype = np.dtype(dtype_name).type
    rng = np.random.default_rng([nchan, np.dtype(dtype).itemsize, 77])
    ims = [make_image(rng, h, w, nchan, dtype) for w, h in SIZES]
    rng = np.random.default_rng(77)  # the cameras are the same for every dtype and nchan
    A, A2, B = trg.pair(rng, 40, 300), trg.pair(rng, 40, 300, baseline=(-0.3, 0.02, 0.01)), trg.pair(rng, 64, 96)
    Bv = trg.pair(rng, 64, 96, baseline=(0., -0.3, 0.))   # vertical baseline: y huge, inf or NaN
    Av = trg.pair(rng, 40, 300, baseline=(0.02, -0.3, 0.))
    C = trg.pair(rng, 9, 1)
    table = [
        ((0, 1), A, 1),                                      # 0 stereo
        ((0, 2), A2, 1),                                     # 1 shares image 0
        ((0, 1), A, 1),                                      # 2 pair 0 again
        ((1, 2), A, 0),                                      # 3 not used
        ((3, 4), (B[0], B[0].copy()), 1),                    # 4 identical cameras: F = 0
        ((3, 4), (np.vstack([B[0][:2], B[0][:1] * 2.]), B[1]), 1),  # 5 rank-deficient P0: F = NaN
        ((3, 4), Bv, 1),                                     # 6 vertical baseline
        ((5, 5), C, 1),                                      # 7 wid = 1: rnx = 1
        ((4, 3), B, 1),                                      # 8 stereo on the second size
        ((2, 0), Av, 1),                                     # 9 steep lines on the wide size
    ]
    col = build(ims, [t[0] for t in table], [t[1][0] for t in table], [t[1][1] for t in table], [t[2] for t in table])
    for p in EMPTY + STEREO:
        assert (tuple(col.box[p]) == (0, 0, 0, 0)) == (p in EMPTY), (p, col.box[p])
    assert col.want[0][2].shape[1] == 360
    return col


def run(col, ims=None, **kw):
    """device.rectify_batch of a collection -> ([r0, r1, ri0, ri1] as flat numpy arrays, box, out_off)."""
    import torch
    from spectavi_amd import device
    t = [torch.from_numpy(im).cuda() for im in (ims or col.ims)]
    out = device.rectify_batch(t, None, col.pairs, col.P1s, col.P0s, col.use, sampling_factor=col.sf, **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out[:4]], out[4], out[5]


def pair_window(flats, box, off, p, nchan):
    rows, cols = int(box[p][1] - box[p][0]), int(box[p][3] - box[p][2])
    lo, hi = int(off[p]), int(off[p + 1])
    assert hi - lo == rows * cols
    vshape = (rows, cols) if nchan == 1 else (rows, cols, nchan)
    return (flats[0][lo * nchan:hi * nchan].reshape(vshape), flats[1][lo * nchan:hi * nchan].reshape(vshape),
            flats[2][lo:hi].reshape(rows, cols), flats[3][lo:hi].reshape(rows, cols))


def same(got, want, what=""):
    for name, g, w in zip(("r0", "r1", "ri0", "ri1"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.argwhere(bits(np.ascontiguousarray(g)) != bits(np.ascontiguousarray(w)))
        assert bad.size == 0, "%s %s differs at %s" % (what, name, bad[:3].tolist())


def self_check(im, r, ri):
    """Every valid sample is the pixel its index names, every other one zero bits."""
    nchan = ro.dims(im)[2]
    ok = (ri >= 0).reshape(-1)
    assert np.array_equal(bits(r).reshape(-1, nchan)[ok], bits(im).reshape(-1, nchan)[ri.reshape(-1)[ok]])
    assert not bits(r).reshape(-1, nchan)[~ok].any()


def check_against_oracle(col, flats, box, off, want_box):
    """box and out_off as stated, and every pair's window the slice of the oracle's uncropped result."""
    want_box = np.asarray(want_box, np.int32).reshape(-1, 4)
    assert np.array_equal(box, want_box), (box.tolist(), want_box.tolist())
    sizes = (want_box[:, 1] - want_box[:, 0]).astype(np.int64) * (want_box[:, 3] - want_box[:, 2])
    assert off.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert flats[2].size == flats[3].size == off[-1] and flats[0].size == flats[1].size == off[-1] * col.nchan
    for p, w in enumerate(col.want):
        if w is not None and sizes[p]:
            same(pair_window(flats, box, off, p, col.nchan), window(w, want_box[p]), "pair %d" % p)


def test_kernel_coverage_lists_the_instantiations():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_coverage.py"), "--list",
                          "--files", "rectify_batch.hip"], check=True, capture_output=True, text=True).stdout
    listed = {ln.strip() for ln in out.splitlines() if ln.startswith("  ")}
    assert listed == INSTANTIATED, out


@pytest.mark.parametrize("nchan", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=[np.dtype(d).name for d in DTYPES])
def test_mixed_collection(dtype, nchan):
    """Cropped on the device: the boxes are the oracle's, the windows ro.crop of the oracle's result and, for the
    dtypes the single call takes, the same windows of device.image_pair_rectification."""
    from spectavi_amd import device
    col = mixed(np.dtype(dtype).name, nchan)
    flats, box, off = run(col)
    check_against_oracle(col, flats, box, off, col.box)
    for p, w in enumerate(col.want):
        if off[p] == off[p + 1]:
            assert p not in STEREO
            continue
        got = pair_window(flats, box, off, p, nchan)
        same(got, ro.crop(*w), "crop of pair %d" % p)
        assert np.array_equal(bits(device.rectify_batch_view(flats[1], p, box, off, nchan)), bits(got[1]))
        self_check(col.ims[col.pairs[p][0]], got[0], got[2])
        self_check(col.ims[col.pairs[p][1]], got[1], got[3])
        if dtype != np.float32:
            a, b = col.pairs[p]
            single = trg.device_run(col.P0s[p], col.P1s[p], col.ims[a], col.ims[b], SF)
            same(got, window(single, box[p]), "single call of pair %d" % p)


@pytest.mark.parametrize("nchan,sf", [(1, 1.2), (3, 1.2), (1, 0.5), (2, 2.2)])
def test_bounds_agree_with_the_oracle(nchan, sf):
    from spectavi_amd import device
    base = mixed("uint8", nchan)
    if sf == SF:
        col = base
    else:  # 2 wide in place of 1 wide: rnx = 1 with an infinite delta at sf = 0.5, where 1 wide has no sample at all
        ims = base.ims[:5] + [trg.image(np.random.default_rng(2), 9, 2, nchan, np.uint8)]
        col = build(ims, base.pairs, base.P0s, base.P1s, base.use, sf)
        assert (ro.shape(2, 9, nchan, sf)[2] == 1) == (sf == 0.5) and (sf != 0.5 or tuple(col.box[7]) == (0, 0, 0, 0))
    sizes = [(im.shape[1], im.shape[0]) for im in col.ims]
    d_box = device.rectify_batch_bounds(sizes, col.pairs, col.P1s, col.P0s, col.use, nchan, sf)
    assert np.array_equal(d_box.cpu().numpy(), col.box), (d_box.cpu().numpy().tolist(), col.box.tolist())
    assert sum(1 for b in col.box if b[1] > b[0]) >= 3


def test_caller_boxes_and_whole_frames():
    col = mixed("float64", 1)
    frames = [(0, 0) if w is None else w[2].shape for w in col.want]
    whole = np.array([(0, r, 0, c) for r, c in frames], np.int32)
    flats, box, off = run(col, crop_invalid=False)
    check_against_oracle(col, flats, box, off, whole)
    for p in (0, 8):  # the whole frame is the single call
        a, b = col.pairs[p]
        same(pair_window(flats, box, off, p, 1), trg.device_run(col.P0s[p], col.P1s[p], col.ims[a], col.ims[b], SF))
    given = whole.copy()
    given[0] = (120, 230, 7, 300)                   # col_lo > 0, col_hi between rnx's strides
    given[1] = (170, 171, 0, 360)                # a single row
    given[2] = (339, 340, 359, 360)              # the frame's last sample alone
    given[4] = (10, 10, 0, 50)                   # no rows
    given[6] = (0, frames[6][0], 40, 41)         # a single column
    given[9] = (100, 260, 256, 257)              # the first column of the second stride
    flats, box, off = run(col, crop_invalid=False, box=given)
    given[3] = 0                                 # a pair that is not used reports an empty box
    check_against_oracle(col, flats, box, off, given)
    from spectavi_amd import device
    for p in (0, 1, 9):  # the front-end's helper shows the same windows
        same([device.rectify_batch_view(f, p, box, off) for f in flats], pair_window(flats, box, off, p, 1))
    # a caller's box takes precedence over crop_invalid
    flats2, box2, off2 = run(col, crop_invalid=True, box=given)
    assert np.array_equal(box2, box) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(flats, flats2))


@pytest.mark.parametrize("wid", [30, 90])
def test_padding_and_dropped_columns(wid):
    """sf = 0.7 on 3 channels: rnx = cols + 1 at 30 wide (the last sample is dropped), rnx = cols - 1 at 90 wide
    (the last column is padding, 0 / -1, and is written)."""
    rows, cols, rnx = ro.shape(wid, 20, 3, 0.7)
    assert rnx - cols == (1 if wid == 30 else -1)
    rng = np.random.default_rng(wid)
    ims = [trg.image(rng, 20, wid, 3), trg.image(rng, 20, wid, 3)]
    P0, P1 = trg.pair(rng, 20, wid)
    col = build(ims, [(0, 1), (1, 0)], [P0, P0], [P1, P1], [1, 1], sf=0.7)
    flats, box, off = run(col, crop_invalid=False)
    check_against_oracle(col, flats, box, off, [(0, rows, 0, cols)] * 2)
    assert (pair_window(flats, box, off, 0, 3)[2][:, rnx:] == -1).all()
    flats, box, off = run(col)
    check_against_oracle(col, flats, box, off, col.box)


def test_a_window_does_not_depend_on_the_collection():
    col = mixed("float32", 3)
    flats, box, off = run(col)
    order = [9, 8, 7, 6, 5, 4, 3, 2, 1, 0]
    rev = SimpleNamespace(**vars(col))
    rev.pairs, rev.P0s, rev.P1s, rev.use = ([seq[p] for p in order] for seq in (col.pairs, col.P0s, col.P1s, col.use))
    rflats, rbox, roff = run(rev)
    for q, p in enumerate(order):
        assert tuple(rbox[q]) == tuple(box[p])
        same(pair_window(rflats, rbox, roff, q, 3), pair_window(flats, box, off, p, 3), "permuted pair %d" % p)
    for p in (0, 6, 9):
        one = SimpleNamespace(**vars(col))
        one.pairs, one.P0s, one.P1s, one.use = [col.pairs[p]], [col.P0s[p]], [col.P1s[p]], [1]
        oflats, obox, ooff = run(one)
        assert tuple(obox[0]) == tuple(box[p])
        same(pair_window(oflats, obox, ooff, 0, 3), pair_window(flats, box, off, p, 3), "pair %d alone" % p)


def test_two_runs_give_the_same_bits():
    col = mixed("float64", 3)
    a, abox, aoff = run(col)
    b, bbox, boff = run(col)
    assert np.array_equal(abox, bbox) and np.array_equal(aoff, boff)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", [np.float64, np.uint8], ids=["float64", "uint8"])
def test_only_the_windows_are_written(dtype):
    """Outputs pre-filled with a sentinel, guard elements before and behind: the windows are packed, so everything in
    [0, out_off[npairs]) is written -- the same bits whatever the sentinel was -- and the guards keep theirs."""
    import torch
    from spectavi_amd import device
    col = mixed(np.dtype(dtype).name, 3)
    tdt = torch.from_numpy(np.zeros(1, dtype)).dtype
    packed = torch.cat([torch.from_numpy(im).reshape(-1) for im in col.ims]).cuda()
    sizes = [(im.shape[1], im.shape[0]) for im in col.ims]
    box = col.box.copy()
    box[0] = (120, 230, 7, 300)
    plan = device.rectify_batch_plan(sizes, col.pairs, 3, SF, col.use, box)
    n, G = plan["samples"], 64
    short = [torch.empty(n * 3 - 1, dtype=tdt, device="cuda"), torch.empty(n * 3, dtype=tdt, device="cuda"),
             torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")]
    with pytest.raises(ValueError):  # outputs shorter than the windows are refused before anything is launched
        device.rectify_batch_into(packed, sizes, col.pairs, col.P1s, col.P0s, col.use, SF, box, 3, *short)
    results = []
    for sentinel in (77, 99):
        vals = [torch.full((G + n * 3 + G,), sentinel, dtype=tdt, device="cuda") for _ in range(2)]
        idxs = [torch.full((G + n + G,), -1000 - sentinel, dtype=torch.int32, device="cuda") for _ in range(2)]
        device.rectify_batch_into(packed, sizes, col.pairs, col.P1s, col.P0s, col.use, SF, box, 3,
                                  vals[0][G:G + n * 3], vals[1][G:G + n * 3], idxs[0][G:G + n], idxs[1][G:G + n])
        torch.cuda.synchronize()
        vals, idxs = [v.cpu().numpy() for v in vals], [i.cpu().numpy() for i in idxs]
        fill = np.array([sentinel]).astype(dtype)[0]
        for v in vals:
            assert (v[:G] == fill).all() and (v[G + n * 3:] == fill).all(), "a value guard was written"
        for i in idxs:
            assert (i[:G] == -1000 - sentinel).all() and (i[G + n:] == -1000 - sentinel).all(), "an index guard was written"
            assert (i[G:G + n] >= -1).all(), "a window element was left unwritten"
        results.append([v[G:G + n * 3] for v in vals] + [i[G:G + n] for i in idxs])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(*results)), "a window element was left unwritten"
    want_box = box.copy()
    want_box[3] = 0
    check_against_oracle(col, results[0], want_box, plan["out_off"], want_box)


@pytest.mark.parametrize("nchan", [1, 3])
def test_float32_is_the_float64_run_of_the_widened_images(nchan):
    col = mixed("float32", nchan)
    f32, box32, off32 = run(col)
    f64, box64, off64 = run(col, ims=[im.astype(np.float64) for im in col.ims])
    assert np.array_equal(box32, box64) and np.array_equal(off32, off64)
    assert np.array_equal(f32[2], f64[2]) and np.array_equal(f32[3], f64[3])
    for a, b in zip(f32[:2], f64[:2]):
        assert a.dtype == np.float32 and b.dtype == np.float64
        assert np.array_equal(a.astype(np.float64).view(np.uint64), b.view(np.uint64))


def test_more_items_than_the_grid_cap():
    """Tall images two pixels wide: enough pairs that both steps' work items exceed their grid of 32 workgroups per
    compute unit, so every workgroup walks several items."""
    import torch
    from spectavi_amd import device
    cap = GROUPS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    hgt, wid = 400, 2
    rows = ro.shape(wid, hgt, 1, SF)[0]
    per_pair = -(-rows // BOUNDS_ROWS)
    npairs = cap // per_pair + 2
    rng = np.random.default_rng(400)
    ims = [trg.image(rng, hgt, wid, 1, np.uint8) for _ in range(3)]
    pairs = [(p % 3, (p + 1) % 3) for p in range(npairs)]
    cams = [trg.pair(rng, hgt, wid, baseline=(-0.25 - 0.001 * p, 0.01, 0.02)) for p in range(npairs)]
    col = build(ims, pairs, [c[0] for c in cams], [c[1] for c in cams], [1] * npairs)
    assert npairs * per_pair > cap
    plan = device.rectify_batch_plan([(wid, hgt)] * 3, pairs, 1, SF, box=col.box)
    assert plan["items"] > cap, (plan["items"], cap)
    assert sum(1 for b in col.box if b[1] - b[0] > BOUNDS_ROWS) > npairs // 2
    flats, box, off = run(col)
    check_against_oracle(col, flats, box, off, col.box)


def test_stream_and_cache_reuse():
    """A non-default stream; and the cached tables of one call reused by calls of other shapes."""
    import torch
    big, small = mixed("uint8", 1), mixed("uint8", 3)
    one = SimpleNamespace(**vars(small))
    one.pairs, one.P0s, one.P1s, one.use = [small.pairs[8]], [small.P0s[8]], [small.P1s[8]], [1]
    one.want, one.box = [small.want[8]], small.box[8:9]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for col in (big, one, big, small):
            flats, box, off = run(col)
            check_against_oracle(col, flats, box, off, col.box)
    s.synchronize()


@pytest.mark.parametrize("dtype", DTYPES, ids=[np.dtype(d).name for d in DTYPES])
def test_host_form_and_front_end(dtype):
    """spv_rectify_batch through mvg.image_pair_rectification_batch: the single front-end call per pair, None where
    that raises (or the pair is skipped)."""
    from spectavi_amd import mvg
    col = mixed(np.dtype(dtype).name, 1)
    P1s = [P if u else None for P, u in zip(col.P1s, col.use)]
    got = mvg.image_pair_rectification_batch(col.ims, col.pairs, P1s, col.P0s, sampling_factor=SF)
    assert len(got) == len(col.pairs)
    for p, g in enumerate(got):
        if tuple(col.box[p]) == (0, 0, 0, 0):
            assert g is None and p not in STEREO
            if col.use[p] and dtype == np.float64:
                with pytest.raises(ValueError):
                    mvg.image_pair_rectification(col.P0s[p], col.P1s[p], col.ims[col.pairs[p][0]],
                                                 col.ims[col.pairs[p][1]], sampling_factor=SF)
            continue
        same(g, ro.crop(*col.want[p]), "pair %d" % p)
        if dtype == np.float64:
            a, b = col.pairs[p]
            same(g, mvg.image_pair_rectification(col.P0s[p], col.P1s[p], col.ims[a], col.ims[b], sampling_factor=SF),
                 "front end, pair %d" % p)
    # whole frames: nothing is None but the skipped pair
    full = mvg.image_pair_rectification_batch(col.ims, col.pairs, P1s, col.P0s, sampling_factor=SF, crop_invalid=False)
    for p, g in enumerate(full):
        if col.use[p]:
            same(g, col.want[p], "whole frame of pair %d" % p)
        else:
            assert g is None


def test_default_first_camera():
    """P0s = None is [I | 0] for every pair."""
    from spectavi_amd import mvg
    rng = np.random.default_rng(11)
    ims = [trg.image(rng, 48, 64, 1) for _ in range(2)]
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    P1s = [np.hstack([trg.rot(rng, 0.01), np.array([[-0.25], [0.01 * k], [0.02]])]) for k in (1, 2)]
    got = mvg.image_pair_rectification_batch(ims, [(0, 1), (1, 0)], P1s, None, sampling_factor=SF)
    for g, P1, (a, b) in zip(got, P1s, [(0, 1), (1, 0)]):
        want = ro.rectify(mvg.rectification_fundamental(P0, P1), ims[a], ims[b], SF)
        assert oracle_box(want) != (0, 0, 0, 0)
        same(g, ro.crop(*want))


def test_profile_names():
    from spectavi_amd import device
    col = mixed("float64", 1)
    device.profile_reset()
    device.profile_enable(True)
    run(col)
    device.profile_enable(False)
    for name in ("rectify_batch_bounds", "rectify_batch_box", "rectify_batch"):
        n, ms = device.profile_read(name)
        assert n == 1 and ms > 0, name
    assert device.profile_read("rectify")[0] == 0
