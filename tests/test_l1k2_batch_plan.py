"""Host only: spv_l1k2_batch_plan cuts a collection of (query set, database set) pairs into work items that tile
every pair's query x database rectangle exactly once, reports what the device call will launch, and refuses
everything outside the contract of include/spectavi_amd.h with `out` untouched."""
import ctypes as ct

import numpy as np
import pytest

from tests import l1k2_batch_cases as bc


def raw_plan(seg, nseg, dim, pairs, npairs, items_cap=0):
    """spv_l1k2_batch_plan itself: (status, out[6] as a list, items or None); out starts as -7s."""
    from spectavi_amd._lib import clib
    out = (ct.c_longlong * 6)(*([-7] * 6))
    items = np.full((items_cap, 5), -7, np.int32) if items_cap else None
    st = clib.spv_l1k2_batch_plan(None if seg is None else seg.ctypes.data, nseg, dim,
                                  None if pairs is None else pairs.ctypes.data, npairs, out,
                                  None if items is None else items.ctypes.data, items_cap)
    return st, list(out), items


def plan_of(rows, pairs, dim):
    from spectavi_amd import device
    return device.l1k2_batch_plan(bc.seg_of(rows), pairs, dim, want_items=True)


def check_tiling(rows, pairs, plan, items):
    """No gap, no overlap, item limits, launch order; returns the slice count of every pair with queries."""
    assert len(items) == plan["items"]
    cover = {}
    for p, y0, yr, x0, xr in items.tolist():
        n, m = rows[pairs[p][0]], rows[pairs[p][1]]
        assert n > 0, "an item for an empty query set"
        assert 0 < yr <= 256 * plan["q"] and y0 % (256 * plan["q"]) == 0 and y0 + yr <= n
        assert 0 <= xr <= 65536 and x0 % 64 == 0 and x0 + xr <= m and (xr > 0 or m == 0)
        cover.setdefault(p, []).append((y0, yr, x0, xr))
    slices = {}
    for p, (a, b) in enumerate(pairs):
        n, m = rows[a], rows[b]
        if n == 0:
            assert p not in cover
            continue
        assert p in cover, "a pair with queries must get items, even against an empty database set"
        # exactly once: the items are distinct, they are the product of their query and database intervals, and
        # each family of intervals tiles its axis without gap or overlap
        ys, xs = sorted({(y0, yr) for y0, yr, _, _ in cover[p]}), sorted({(x0, xr) for _, _, x0, xr in cover[p]})
        assert len(cover[p]) == len(set(cover[p])) == len(ys) * len(xs), p
        for ivals, end in ((ys, n), (xs, m)):
            at = 0
            for lo, cnt in ivals:
                assert lo == at, ("gap or overlap in pair %d" % p)
                at += cnt
            assert at == end, p
        slices[p] = len(xs)
    work = [int(yr) * int(xr) for _, _, yr, _, xr in items.tolist()]
    assert work == sorted(work, reverse=True), "longest item first"
    assert plan["max_slices"] == max(slices.values(), default=0)
    return slices


def check_totals(rows, pairs, dim, plan):
    from spectavi_amd._lib import clib
    seg, prs = bc.seg_of(rows), np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    want_off = np.concatenate([[0], np.cumsum([rows[a] for a, _ in pairs])]).astype(np.int64)
    assert plan["out_rows"] == want_off[-1] and np.array_equal(plan["out_off"], want_off)
    assert plan["workspace_bytes"] == clib.spv_l1k2_batch_workspace_bytes(seg.ctypes.data, len(rows), dim,
                                                                         prs.ctypes.data, len(prs))
    # 16 bytes per out row, 32 per item, the padded desc: nothing that grows with the slice count alone
    pad = sum(rows) * plan["dim_pad"] if plan["dim_pad"] != dim else 0
    assert plan["workspace_bytes"] <= 16 * plan["out_rows"] + 32 * plan["items"] + pad + 3 * 256


def test_nine_sets_all_ordered_pairs():
    plan, items = plan_of(bc.NINE, bc.ALL81, 128)
    check_tiling(bc.NINE, bc.ALL81, plan, items)
    check_totals(bc.NINE, bc.ALL81, 128, plan)
    assert plan["out_rows"] == 9 * sum(bc.NINE)


def test_long_database_crosses_the_16_bit_slice_limit():
    rows, pairs = [70000, 257], [(1, 0)]
    plan, items = plan_of(rows, pairs, 128)
    assert check_tiling(rows, pairs, plan, items)[0] >= 2 and plan["max_slices"] >= 2
    check_totals(rows, pairs, 128, plan)


def test_a_lone_pair_is_sliced_to_fill_the_chip():
    rows, pairs = [20000, 600], [(1, 0)]
    plan, items = plan_of(rows, pairs, 128)
    assert check_tiling(rows, pairs, plan, items)[0] > 1 and plan["items"] >= 256
    check_totals(rows, pairs, 128, plan)


def test_many_short_pairs_are_not_sliced():
    rows = [3000] * 40
    pairs = [(j, i) for i in range(40) for j in range(i + 1, 40)]
    plan, items = plan_of(rows, pairs, 128)
    assert set(check_tiling(rows, pairs, plan, items).values()) == {1} and plan["max_slices"] == 1
    assert plan["q"] == 2 and plan["items"] == 780 * 6
    check_totals(rows, pairs, 128, plan)


@pytest.mark.parametrize("seed", range(6))
def test_random_collections(seed):
    rng = np.random.default_rng(seed)
    nseg = int(rng.integers(1, 12))
    rows = [int(r) for r in rng.choice([0, 1, 5, 64, 100, 255, 256, 257, 700, 1500, 5000, 66000], nseg)]
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, nseg, (int(rng.integers(0, 30)), 2))]
    dim = int(rng.choice([16, 64, 128, 176, 256]))
    plan, items = plan_of(rows, pairs, dim)
    check_tiling(rows, pairs, plan, items)
    check_totals(rows, pairs, dim, plan)


def test_empty_collections():
    for rows, pairs in (([], []), ([5, 0], []), ([0, 0], [(0, 1)]), ([0, 9], [(0, 1), (0, 0)])):
        plan, items = plan_of(rows, pairs, 128)
        assert plan["items"] == 0 and plan["out_rows"] == 0 and len(items) == 0
    st, out, _ = raw_plan(None, 0, 128, None, 0)   # no sets at all: seg_off may be NULL
    assert st == 0 and out[2:5] == [0, 0, 0]


@pytest.mark.parametrize("dim", [16, 32, 48, 128, 176, 256])
def test_width_and_q_follow_the_single_pair_rule(dim):
    """The kernel row width is l1k2_plan's; so is q wherever the shape alone fills the chip."""
    from spectavi_amd import device
    single = device.l1k2_plan(70000, 70000, dim)
    assert not single["wide"]
    plan = device.l1k2_batch_plan(bc.seg_of([70000, 70000]), [(1, 0)], dim)
    assert (plan["dim_pad"], plan["q"]) == (single["dim_pad"], single["q"])


def test_q_cases_reach_every_instantiation():
    """The cases tests/test_l1k2_batch_gpu.py runs get the queries per lane and the longest item they are written for,
    and together reach every instantiation of l1k2_batch_kernel (asked of the library: a new width or Q without a
    case fails here), each of them also with items of 64 tiles (tiles-*; at the planner's largest q here, at the
    smaller ones in the child process below).  A retuned planner that takes the many-tile items away fails here."""
    from tests.l1k2_batch_child import longest_item
    shipped = bc.library_instantiations()
    assert {w for w, _ in shipped} == {bc.width_of(d) for d in bc.DIMS} and len(shipped) > 20
    reached, many_tiles = set(), set()
    for name, rows, pairs, dim, q, xrows in bc.Q_CASES:
        assert longest_item(rows, pairs, dim) == (q, xrows), name
        reached.add((bc.width_of(dim), q))
        if xrows >= 4096:
            many_tiles.add((bc.width_of(dim), q))
    assert reached == shipped
    assert many_tiles == {(w, q) for w, q in shipped if (w, 2 * q) not in shipped}
    assert max(c[5] for c in bc.Q_CASES) == 65536


@pytest.mark.parametrize("q", [1, 2])
def test_tile_cases_keep_their_long_items_under_a_forced_q(q):
    """What the GPU child of tests/test_l1k2_batch_gpu.py asserts before it runs, without a GPU: under
    SPECTAVI_L1K2_Q (read once per process, hence the child) the tiles-* cases run at that q on 4096-row items."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(root, "tests", "l1k2_batch_child.py"), str(q), "--plan-only"]
    r = subprocess.run(cmd, cwd=root, env=dict(os.environ, SPECTAVI_L1K2_Q=str(q)), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok q=%d" % q), r.stdout[-2000:] + r.stderr[-2000:]


def test_items_cap_limits_what_is_written():
    seg, prs = bc.seg_of(bc.NINE), np.array(bc.ALL81, np.int32)
    st, out, items = raw_plan(seg, 9, 128, prs, 81, items_cap=5)
    assert st == 0 and out[2] > 5 and (items != -7).all()
    st, out2, more = raw_plan(seg, 9, 128, prs, 81, items_cap=int(out[2]) + 3)
    assert st == 0 and out2 == out and np.array_equal(more[:5], items)
    assert (more[:out[2]] != -7).any(axis=1).all() and (more[out[2]:] == -7).all()


def test_invalid_arguments_leave_out_untouched():
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    seg, prs = bc.seg_of([10, 20, 30]), np.array([[0, 1], [2, 0]], np.int32)
    bad = [
        (seg, 3, 24, prs, 2),                                       # dim no multiple of 16
        (seg, 3, 272, prs, 2),                                      # above the tile widths
        (seg, 3, 0, prs, 2),
        (np.array([1, 10, 30, 60], np.int64), 3, 128, prs, 2),      # seg_off[0] != 0
        (np.array([0, 30, 10, 60], np.int64), 3, 128, prs, 2),      # decreasing
        (np.array([0, 10, 30, 2 ** 31], np.int64), 3, 128, prs, 2),  # 2^31 rows
        (seg, 3, 128, np.array([[0, 1], [-1, 0]], np.int32), 2),    # set -1
        (seg, 3, 128, np.array([[0, 1], [2, 3]], np.int32), 2),     # set nseg
        (None, 3, 128, prs, 2),                                     # NULL seg_off with nseg > 0
        (seg, 3, 128, None, 2),                                     # NULL pairs with npairs > 0
        (seg, -1, 128, prs, 2),
        (seg, 3, 128, prs, -1),
    ]
    for k, (s, nseg, dim, p, npairs) in enumerate(bad):
        st, out, items = raw_plan(s, nseg, dim, p, npairs, items_cap=4)
        assert st == SPV_ERR_INVALID and clib.spv_last_error(), k
        assert out == [-7] * 6 and (items == -7).all(), k
        assert clib.spv_l1k2_batch_workspace_bytes(None if s is None else s.ctypes.data, nseg, dim,
                                                   None if p is None else p.ctypes.data, npairs) == 0, k
    out = (ct.c_longlong * 6)()
    assert clib.spv_l1k2_batch_plan(seg.ctypes.data, 3, 128, prs.ctypes.data, 2, None, None, 0) == SPV_ERR_INVALID
    assert clib.spv_l1k2_batch_plan(seg.ctypes.data, 3, 128, prs.ctypes.data, 2, out, prs.ctypes.data, -1) == SPV_ERR_INVALID


def test_python_argument_checks_are_value_errors():
    """device.l1k2_batch_plan (and l1k2_batch, through the same helper) refuse a mis-shaped input in Python."""
    from spectavi_amd import device, feature
    seg = bc.seg_of([10, 20])
    for s, p, dim in ((seg, [(0, 2)], 128), (seg, [(-1, 0)], 128), (seg, [(0, 1, 1)], 128), (seg, [(0, 1)], 24),
                      (seg, [(0, 1)], 272), (seg[1:], [(0, 0)], 128), (seg[::-1].copy(), [(0, 0)], 128),
                      (seg, [(0.5, 1)], 128)):
        with pytest.raises(ValueError):
            device.l1k2_batch_plan(s, p, dim)
    t = np.zeros((4, 16), np.uint8)
    for tables, pairs in (([], None), ([t, np.zeros((4, 32), np.uint8)], None), ([t.astype(np.int32)], None),
                          ([t, t], [(0, 2)]), ([np.zeros((4, 24), np.uint8)], None), ([np.zeros((1, 272), np.uint8)], None),
                          ([t, t], [(0.0, 1.0)]), ([t, t], [(0, 1, 1), (1, 0, 0)]), ([t, t], [0, 1]),
                          ([np.zeros((4, 0), np.uint8)], None)):
        with pytest.raises(ValueError):
            feature.nn_bruteforcel1k2_batch(tables, pairs)


def test_no_gpu_is_a_loud_error():
    """Without a device both forms fail with SPV_ERR_HIP, never with a host computation."""
    from spectavi_amd import _lib, feature
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    seg, prs = bc.seg_of([4, 4]), np.array([[1, 0]], np.int32)
    desc = np.zeros((8, 16), np.uint8)
    idx, dist = np.zeros((4, 2), np.uint64), np.zeros((4, 2), np.int32)
    st = _lib.clib.spv_nn_bruteforcel1k2_batch(desc.ctypes.data, seg.ctypes.data, 2, 16, prs.ctypes.data, 1,
                                               idx.ctypes.data, dist.ctypes.data)
    assert st == _lib.SPV_ERR_HIP and _lib.clib.spv_last_error()
    # never dereferenced: there is no device to launch on
    fake = 1 << 20
    st = _lib.clib.spv_l1k2_batch_device(fake, seg.ctypes.data, 2, 16, prs.ctypes.data, 1, fake, fake, fake, 1 << 20, None)
    assert st == _lib.SPV_ERR_HIP and _lib.clib.spv_last_error()
    with pytest.raises(_lib.SpectaviError):
        feature.nn_bruteforcel1k2_batch([desc[:4], desc[4:]])
