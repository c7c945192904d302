"""Host only: spv_l1k2_guided_batch_plan cuts a collection of (query set, database set) pairs into work items that
cover every (out row, database row) exactly once, the collections of tests/test_l1k2_guided_gpu.py get the items
their cases are written for, and mis-shaped arguments are refused before any device is touched."""
import ctypes as ct

import numpy as np
import pytest

from tests import l1k2_guided_cases as gc

SPV_ERR_INVALID = 1


def plan_c(seg, nseg, dim, pairs):
    """spv_l1k2_guided_batch_plan itself: (status, out[4] as a list); out starts as -7s."""
    from spectavi_amd._lib import clib
    prs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    out = (ct.c_longlong * 4)(-7, -7, -7, -7)
    st = clib.spv_l1k2_guided_batch_plan(None if seg is None else seg.ctypes.data, nseg, dim, prs.ctypes.data, len(prs),
                                         out, None, 0)
    return st, list(out)


COLLECTIONS = [(gc.NINE, gc.FEW), gc.LONE, gc.TILES, gc.LONG, ([0, 0, 5], [(0, 1), (2, 0), (0, 2)]), ([300], []),
               ([256, 257, 64], [(0, 1), (1, 0), (2, 2)] * 200)]


@pytest.mark.parametrize("rows,pairs", COLLECTIONS)
def test_items_cover_every_pair_of_rows_once(rows, pairs):
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    plan, items = device.l1k2_guided_batch_plan(gc.seg_of(rows), pairs, 128, want_items=True)
    assert plan["items"] == len(items) and plan["out_rows"] == sum(rows[q] for q, _ in pairs)
    assert np.array_equal(plan["out_off"], np.concatenate([[0], np.cumsum([rows[q] for q, _ in pairs])]))
    work = (items[:, 2].astype(np.int64) * items[:, 4]).tolist()
    assert work == sorted(work, reverse=True), "longest item first"
    slices = 0
    for p, (q, d) in enumerate(pairs):
        mine = items[items[:, 0] == p]
        # query blocks of at most 256 rows tile the query set; each block's slices tile the database set
        blocks = sorted(set(map(tuple, mine[:, 1:3])))
        assert [b[0] for b in blocks] == list(range(0, rows[q], 256))
        assert all(0 < n <= 256 for _, n in blocks) and sum(n for _, n in blocks) == rows[q]
        for y0, _ in blocks:
            sl = mine[mine[:, 1] == y0][:, 3:5]
            sl = sl[np.argsort(sl[:, 0], kind="stable")]
            assert sl[0, 0] == 0 and np.array_equal(sl[1:, 0], np.cumsum(sl[:-1, 1])) and sl[:, 1].sum() == rows[d]
            assert rows[d] == 0 and len(sl) == 1 or (sl[:, 1] > 0).all()
            slices = max(slices, len(sl))
    assert plan["max_slices"] == slices
    seg, prs = gc.seg_of(rows), np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    assert plan["workspace_bytes"] == clib.spv_l1k2_guided_batch_workspace_bytes(seg.ctypes.data, len(rows), 128,
                                                                                prs.ctypes.data, len(prs))
    assert plan["workspace_bytes"] >= 16 * plan["out_rows"] + 32 * plan["items"]


def test_the_gpu_cases_are_what_they_claim():
    from spectavi_amd import device
    plan, items = device.l1k2_guided_batch_plan(gc.seg_of(gc.LONE[0]), gc.LONE[1], 128, want_items=True)
    assert plan["max_slices"] > 1 and (items[:, 4] < 5000).all(), "the lone pair is cut: the global merge decides"
    plan, items = device.l1k2_guided_batch_plan(gc.seg_of(gc.TILES[0]), gc.TILES[1], 128, want_items=True)
    assert plan["max_slices"] == 1 and (items[:, 4] == 5000).all(), "whole sets of 79 tiles: the double buffer swaps"
    assert len(items) == 2 * 1024 and 5000 > 2 * 64
    plan, items = device.l1k2_guided_batch_plan(gc.seg_of(gc.LONG[0]), gc.LONG[1], 128, want_items=True)
    assert plan["max_slices"] > 1 and (items[:, 3] > 65536).any(), "slices that begin past row 65536"
    plan, items = device.l1k2_guided_batch_plan(gc.seg_of(gc.NINE), gc.FEW, 128, want_items=True)
    assert (items[:, 4] == 0).any() and (items[:, 4] > 64).any() and plan["max_slices"] > 1


@pytest.mark.parametrize("dim", [64, 144, 0, 16, 256])
def test_only_dim_128(dim):
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    seg = gc.seg_of([4, 4])
    st, out = plan_c(seg, 2, dim, [(1, 0)])
    assert st == SPV_ERR_INVALID and out == [-7] * 4
    prs = np.array([[1, 0]], np.int32)
    assert clib.spv_l1k2_guided_batch_workspace_bytes(seg.ctypes.data, 2, dim, prs.ctypes.data, 1) == 0
    with pytest.raises(ValueError):
        device.l1k2_guided_batch_plan(seg, [(1, 0)], dim)
    # the device call refuses before it looks at a pointer
    fake = 1 << 20
    st = clib.spv_l1k2_guided_batch_device(fake, fake, seg.ctypes.data, 2, dim, prs.ctypes.data, 1, fake, 1.0, fake, fake,
                                           fake, fake, 1 << 20, None)
    assert st == SPV_ERR_INVALID
    st = clib.spv_nn_bruteforcel1k2_guided_batch(fake, fake, seg.ctypes.data, 2, dim, prs.ctypes.data, 1, fake, 1.0, fake,
                                                 fake, fake)
    assert st == SPV_ERR_INVALID


@pytest.mark.parametrize("seg,pairs", [
    (np.array([1, 4, 8], np.int64), [(1, 0)]),          # does not start at 0
    (np.array([0, 5, 4], np.int64), [(1, 0)]),          # decreases
    (np.array([0, 4, 2 ** 31], np.int64), [(1, 0)]),    # too many rows
    (np.array([0, 4, 8], np.int64), [(2, 0)]),          # a set outside [0, nseg)
    (np.array([0, 4, 8], np.int64), [(0, -1)]),
])
def test_collections_outside_the_rules(seg, pairs):
    from spectavi_amd import device
    st, out = plan_c(seg, len(seg) - 1, 128, pairs)
    assert st == SPV_ERR_INVALID and out == [-7] * 4
    with pytest.raises(ValueError):
        device.l1k2_guided_batch_plan(seg, pairs, 128)


def test_plan_refuses_null_output_and_negative_cap():
    from spectavi_amd._lib import clib
    seg, prs = gc.seg_of([4, 4]), np.array([[1, 0]], np.int32)
    out = (ct.c_longlong * 4)()
    assert clib.spv_l1k2_guided_batch_plan(seg.ctypes.data, 2, 128, prs.ctypes.data, 1, None, None, 0) == SPV_ERR_INVALID
    assert clib.spv_l1k2_guided_batch_plan(seg.ctypes.data, 2, 128, prs.ctypes.data, 1, out, prs.ctypes.data, -1) == SPV_ERR_INVALID


def test_host_form_refuses_mis_shaped_inputs():
    """feature.nn_bruteforcel1k2_guided_batch checks its arrays in Python, lines with the wrong row count among them."""
    from spectavi_amd import feature
    tables, geoms, lines = gc.collection([5, 3], [(1, 0)], 1)
    bad = [
        (tables, geoms, lines[:2], [(1, 0)]),                                   # lines: wrong row count
        (tables, geoms, lines.astype(np.float32), [(1, 0)]),                    # lines: wrong dtype
        (tables, geoms, np.zeros((3, 2)), [(1, 0)]),                            # lines: wrong width
        (tables, [geoms[0][:, :3], geoms[1]], lines, [(1, 0)]),                 # geom: wrong width
        (tables, [g.astype(np.float64) for g in geoms], lines, [(1, 0)]),       # geom: wrong dtype
        (tables, geoms[:1], lines, [(1, 0)]),                                   # geom: one per table
        ([t[:, :64] for t in tables], geoms, lines, [(1, 0)]),                  # dim 64
        ([np.tile(t, (1, 2))[:, :144] for t in tables], geoms, lines, [(1, 0)]),  # dim 144
        (tables, geoms, lines, [(2, 0)]),                                       # a table outside [0, n)
    ]
    for t, g, l, p in bad:
        with pytest.raises(ValueError):
            feature.nn_bruteforcel1k2_guided_batch(t, g, l, 1.0, p)


def test_the_ragged_case_meets_its_conditions():
    """What test_ragged_collection asserts before it consults the GPU, checked here where no GPU is needed."""
    tables, geoms, lines = gc.ragged()
    assert gc.is_dyadic(geoms, lines, gc.RAGGED_DIST)
    _, _, ncand = gc.oracle(tables, geoms, gc.FEW, lines, gc.RAGGED_DIST)
    assert gc.ragged_counts_ok(ncand)
