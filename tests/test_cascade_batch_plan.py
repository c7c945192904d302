"""Host only: spv_cascade_batch_plan cuts the out rows of a collection of (query set, database set) pairs into
work items that cover every out row exactly once, reports what the device call will launch, and refuses everything
outside the contract of include/spectavi_amd.h with `out` untouched; the device and host forms refuse the same,
and a misaligned pointer or a short workspace, before anything is enqueued."""
import ctypes as ct

import numpy as np
import pytest

from tests import cascade_batch_cases as cb

ITEM_ROWS = 64


def raw_plan(seg, nseg, dim, m, n, g, pairs, npairs, items_cap=0):
    """spv_cascade_batch_plan itself: (status, out[4] as a list, items or None); out starts as -7s."""
    from spectavi_amd._lib import clib
    out = (ct.c_longlong * 4)(*([-7] * 4))
    items = np.full((items_cap, 3), -7, np.int32) if items_cap else None
    st = clib.spv_cascade_batch_plan(None if seg is None else seg.ctypes.data, nseg, dim, m, n, g,
                                     None if pairs is None else pairs.ctypes.data, npairs, out,
                                     None if items is None else items.ctypes.data, items_cap)
    return st, list(out), items


def plan_of(rows, pairs, dim, m, n, g):
    from spectavi_amd import device
    return device.cascade_batch_plan(cb.seg_of(rows), pairs, dim, m, n, g, want_items=True)


def check_plan(rows, pairs, dim, m, n, g):
    """out_off, the items and the workspace bytes of a collection agree with each other and with the contract."""
    from spectavi_amd._lib import clib
    plan, items = plan_of(rows, pairs, dim, m, n, g)
    want_off = np.concatenate([[0], np.cumsum([rows[a] for a, _ in pairs])]).astype(np.int64)
    assert plan["out_rows"] == want_off[-1] and np.array_equal(plan["out_off"], want_off)
    assert len(items) == plan["items"]
    # every out row exactly once, in pair order, no item for an empty query set, none across two pairs
    covered = np.zeros(plan["out_rows"], np.int64)
    last = (-1, 0)
    for p, y0, yr in items.tolist():
        nq = rows[pairs[p][0]]
        assert nq > 0 and 0 < yr <= ITEM_ROWS and y0 % ITEM_ROWS == 0 and y0 + yr <= nq, (p, y0, yr)
        assert (p, y0) > last, "launch order: by pair, then by query row"
        last = (p, y0)
        covered[want_off[p] + y0:want_off[p] + y0 + yr] += 1
    assert (covered == 1).all()
    assert plan["items"] == sum(-(-rows[a] // ITEM_ROWS) for a, _ in pairs)
    # bucket bits: never above m or 22, at least min(m, 12), and the tables within 1 GiB
    assert min(m, 12) <= plan["hb"] <= min(m, 22) or len(rows) * n * (2 ** min(m, 12) + 1) * 4 > 2 ** 30
    assert len(rows) * n * (2 ** plan["hb"] + 1) * 4 <= 2 ** 30
    seg, prs = cb.seg_of(rows), np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    assert plan["workspace_bytes"] == clib.spv_cascade_batch_workspace_bytes(seg.ctypes.data, len(rows), dim, m, n, g,
                                                                            prs.ctypes.data, len(prs))
    # the pieces of the workspace: tables, dictionary, image, four [n][total] arrays, bucket offsets, segment sums
    total, ntab, nb1 = sum(rows), len(rows) * n, 2 ** plan["hb"] + 1
    pieces = [32 * plan["items"] + 4 * (len(rows) + 1), 4 * max(n * dim * ((m + 3) // 4 * 4), (dim + 16) * 64),
              total * dim] + [4 * n * total] * 4 + [4 * ntab * nb1, 4 * ntab * -(-nb1 // 1024)]
    assert plan["workspace_bytes"] == sum(-(-max(b, 16) // 256) * 256 for b in pieces)
    return plan, items


def test_nine_sets_all_ordered_pairs():
    plan, _ = check_plan(cb.NINE, cb.ALL81, *cb.NINE_SHAPE)
    assert plan["out_rows"] == 9 * sum(cb.NINE) and plan["hb"] == 6


@pytest.mark.parametrize("shape", cb.EDGES, ids=lambda s: "-".join(map(str, s)))
def test_edge_collections(shape):
    plan, _ = check_plan(cb.FEW_ROWS, cb.FEW, *shape)
    assert plan["hb"] == min(shape[1], 12)   # sets of at most 130 rows: the floor of 12 bits, or m


def test_bookkeeping_collections():
    check_plan(cb.BOOK_ROWS, cb.BOOK, *cb.NINE_SHAPE)
    check_plan(cb.BOOK_ROWS, cb.DESCENDING, *cb.NINE_SHAPE)


def test_bucket_bits_follow_the_largest_set_and_the_memory_cap():
    from spectavi_amd import device
    hb = lambda rows, m, n=2: device.cascade_batch_plan(cb.seg_of(rows), [(0, 0)], 128, m, n, 2)["hb"]
    assert hb([15000] * 12, 11) == 11                    # m from auto_hash_bit_rate: a bucket is one code
    assert hb([15000] * 12, 20) == 14                    # no more bits than the largest set can spread over
    assert hb([5000, 70000], 31) == 17
    assert hb([3000000], 31) == 22                       # the single call's cap
    assert hb([100] * 1000, 31) == 12                    # the floor
    assert hb([100] * 30000, 31) == 12                   # 60000 tables of 4097 words: 0.98e9 bytes
    assert hb([100] * 32767, 31) == 11                   # 65534 of them pass 1 GiB: one bit less


@pytest.mark.parametrize("seed", range(6))
def test_random_collections(seed):
    rng = np.random.default_rng(seed)
    nseg = int(rng.integers(1, 12))
    rows = [int(r) for r in rng.choice([0, 1, 5, 63, 64, 65, 100, 128, 257, 700, 5000, 66000], nseg)]
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, nseg, (int(rng.integers(0, 30)), 2))]
    dim, m, n, g = cb.EDGES[seed % len(cb.EDGES)]
    check_plan(rows, pairs, dim, m, n, g)


def test_empty_collections():
    """pairs = [] and total_rows = 0 are accepted: no items, no out rows; the device and host forms return at once."""
    from spectavi_amd import feature
    from spectavi_amd._lib import clib
    for rows, pairs in (([], []), ([5, 0], []), ([0, 0], [(0, 1)]), ([0, 9], [(0, 1), (0, 0)])):
        plan, items = plan_of(rows, pairs, *cb.NINE_SHAPE)
        assert plan["items"] == 0 and plan["out_rows"] == 0 and len(items) == 0
        seg, prs = cb.seg_of(rows), np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        # nothing to write: no pointer is looked at, no device is touched
        assert clib.spv_cascade_batch_device(None, seg.ctypes.data, len(rows), 128, 6, 2, 2, prs.ctypes.data, len(prs),
                                             None, None, None, None, None, 0, None) == 0
        assert clib.spv_nn_cascading_hash_batch(None, seg.ctypes.data, len(rows), 128, 6, 2, 2, prs.ctypes.data,
                                                len(prs), None, None, None, None) == 0
    st, out, _ = raw_plan(None, 0, 128, 6, 2, 2, None, 0)   # no sets at all: seg_off may be NULL
    assert st == 0 and out[:2] == [0, 0]
    d = cb.hash_dict(*cb.NINE_SHAPE)
    empty = np.zeros((0, 128), np.float32)
    assert feature.nn_cascading_hash_batch([empty, empty], d, pairs=[]) == []
    got = feature.nn_cascading_hash_batch([empty, np.ones((3, 128), np.float32)], d, pairs=[(0, 1), (0, 0)], return_ncand=True)
    assert [tuple(a.shape for a in r) for r in got] == [((0, 2), (0, 2), (0,))] * 2


def test_items_cap_limits_what_is_written():
    seg, prs = cb.seg_of(cb.NINE), np.array(cb.ALL81, np.int32)
    st, out, items = raw_plan(seg, 9, 128, 6, 2, 2, prs, 81, items_cap=5)
    assert st == 0 and out[0] > 5 and (items != -7).all()
    st, out2, more = raw_plan(seg, 9, 128, 6, 2, 2, prs, 81, items_cap=int(out[0]) + 3)
    assert st == 0 and out2 == out and np.array_equal(more[:5], items)
    assert (more[:out[0]] != -7).any(axis=1).all() and (more[out[0]:] == -7).all()


SEG3 = cb.seg_of([10, 20, 30])
PRS2 = np.array([[0, 1], [2, 0]], np.int32)
# (seg_off, nseg, dim, m, n, g, pairs, npairs)
BAD = [
    (SEG3, 3, 24, 6, 2, 2, PRS2, 2),                                        # dim no multiple of 16
    (SEG3, 3, 272, 6, 2, 2, PRS2, 2),                                       # dim above 256
    (SEG3, 3, 0, 6, 2, 2, PRS2, 2),
    (SEG3, 3, 128, 0, 2, 0, PRS2, 2),                                       # m outside [1, 31]
    (SEG3, 3, 128, 32, 2, 2, PRS2, 2),
    (SEG3, 3, 128, 6, 0, 2, PRS2, 2),                                       # n < 1
    (SEG3, 3, 128, 6, 2, -1, PRS2, 2),                                      # g outside [0, min(m, 16)]
    (SEG3, 3, 128, 4, 2, 5, PRS2, 2),
    (SEG3, 3, 128, 20, 2, 17, PRS2, 2),
    (np.array([1, 10, 30, 60], np.int64), 3, 128, 6, 2, 2, PRS2, 2),        # seg_off[0] != 0
    (np.array([0, 30, 10, 60], np.int64), 3, 128, 6, 2, 2, PRS2, 2),        # non-monotone
    (np.array([0, 10, 30, 2 ** 31], np.int64), 3, 128, 6, 2, 2, PRS2, 2),   # 2^31 rows
    (SEG3, 3, 128, 6, 2, 2, np.array([[0, 1], [-1, 0]], np.int32), 2),      # set -1
    (SEG3, 3, 128, 6, 2, 2, np.array([[0, 1], [2, 3]], np.int32), 2),       # set nseg
    (SEG3, 3, 128, 6, 21846, 2, PRS2, 2),                                   # nseg * n = 65538 bucket tables
    (None, 3, 128, 6, 2, 2, PRS2, 2),                                       # NULL seg_off with nseg > 0
    (SEG3, 3, 128, 6, 2, 2, None, 2),                                       # NULL pairs with npairs > 0
    (SEG3, -1, 128, 6, 2, 2, PRS2, 2),
    (SEG3, 3, 128, 6, 2, 2, PRS2, -1),
]
FAKE = 1 << 20   # a pointer that is never dereferenced: every call below is refused before the first HIP call


def test_invalid_arguments_leave_out_untouched():
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    ptr = lambda a: None if a is None else a.ctypes.data
    for k, (s, nseg, dim, m, n, g, p, npairs) in enumerate(BAD):
        st, out, items = raw_plan(s, nseg, dim, m, n, g, p, npairs, items_cap=4)
        assert st == SPV_ERR_INVALID and clib.spv_last_error(), k
        assert out == [-7] * 4 and (items == -7).all(), k
        assert clib.spv_cascade_batch_workspace_bytes(ptr(s), nseg, dim, m, n, g, ptr(p), npairs) == 0, k
        # the device form and the host form refuse the same, whatever the device count: nothing is enqueued
        assert clib.spv_cascade_batch_device(FAKE, ptr(s), nseg, dim, m, n, g, ptr(p), npairs, FAKE, FAKE, FAKE, FAKE,
                                             FAKE, 1 << 40, None) == SPV_ERR_INVALID, k
        idx, dist, nc = np.full((64, 2), 7, np.uint64), np.full((64, 2), 7, np.float32), np.full(64, 7, np.int32)
        rows = np.zeros((60, max(dim, 16)), np.float32)
        d = np.zeros(max(n, 1) * max(dim, 16) * max(m, 1), np.float32) if n < 100 else np.zeros(16, np.float32)
        assert clib.spv_nn_cascading_hash_batch(rows.ctypes.data, ptr(s), nseg, dim, m, n, g, ptr(p), npairs,
                                                d.ctypes.data, idx.ctypes.data, dist.ctypes.data,
                                                nc.ctypes.data) == SPV_ERR_INVALID, k
        assert (idx == 7).all() and (dist == 7).all() and (nc == 7).all(), k
    out = (ct.c_longlong * 4)()
    args = (SEG3.ctypes.data, 3, 128, 6, 2, 2, PRS2.ctypes.data, 2)
    assert clib.spv_cascade_batch_plan(*args, None, None, 0) == SPV_ERR_INVALID
    assert clib.spv_cascade_batch_plan(*args, out, PRS2.ctypes.data, -1) == SPV_ERR_INVALID


def test_misaligned_pointers_and_a_short_workspace_are_refused_before_any_launch():
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    need = clib.spv_cascade_batch_workspace_bytes(SEG3.ctypes.data, 3, 128, 6, 2, 2, PRS2.ctypes.data, 2)
    assert need > 0
    good = dict(rows=FAKE, dict=FAKE, idx=FAKE, dist=FAKE, ncand=FAKE, ws=FAKE, ws_bytes=need)
    for change in (dict(rows=FAKE + 4), dict(dict=FAKE + 8), dict(ws=FAKE + 4), dict(idx=FAKE + 4), dict(dist=FAKE + 2),
                   dict(ncand=FAKE + 1), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(rows=None), dict(dict=None),
                   dict(idx=None), dict(dist=None), dict(ws=None)):
        a = dict(good, **change)
        st = clib.spv_cascade_batch_device(a["rows"], SEG3.ctypes.data, 3, 128, 6, 2, 2, PRS2.ctypes.data, 2, a["dict"],
                                           a["idx"], a["dist"], a["ncand"], a["ws"], a["ws_bytes"], None)
        assert st == SPV_ERR_INVALID and clib.spv_last_error(), change


def test_python_argument_checks_are_value_errors():
    """device.cascade_batch_plan (and cascade_batch, through the same helper) and feature.nn_cascading_hash_batch
    refuse a mis-shaped input in Python."""
    from spectavi_amd import device, feature
    seg = cb.seg_of([10, 20])
    for s, p, dim, m, n, g in ((seg, [(0, 2)], 128, 6, 2, 2), (seg, [(-1, 0)], 128, 6, 2, 2), (seg, [(0, 1, 1)], 128, 6, 2, 2),
                               (seg, [(0, 1)], 24, 6, 2, 2), (seg, [(0, 1)], 272, 6, 2, 2), (seg[1:], [(0, 0)], 128, 6, 2, 2),
                               (seg[::-1].copy(), [(0, 0)], 128, 6, 2, 2), (seg, [(0, 1)], 128, 32, 2, 2),
                               (seg, [(0, 1)], 128, 6, 0, 2), (seg, [(0, 1)], 128, 4, 2, 5), (seg, [(0, 1)], 128, 20, 2, 17),
                               (seg, [(0, 1)], 128, 6, 32768, 2)):
        with pytest.raises(ValueError):
            device.cascade_batch_plan(s, p, dim, m, n, g)
    t, d = np.zeros((4, 16), np.float32), np.zeros((2, 16, 6), np.float32)
    for tables, hd, pairs, g in (([], d, None, 2), ([t, np.zeros((4, 32), np.float32)], d, None, 2), ([t, t], d, [(0, 2)], 2),
                                 ([t, t], np.zeros((2, 32, 6), np.float32), None, 2), ([t, t], d, [(0.0, 1.0)], 2),
                                 ([t, t], d, [0, 1], 2), ([t, t], d, None, 7), ([t, t], np.zeros((2, 16, 32), np.float32), None, 2),
                                 ([np.zeros((4, 24), np.float32)], np.zeros((2, 24, 6), np.float32), None, 2),
                                 ([np.zeros((1, 272), np.float32)], np.zeros((2, 272, 6), np.float32), None, 2)):
        with pytest.raises(ValueError):
            feature.nn_cascading_hash_batch(tables, hd, pairs, g=g)


def test_no_gpu_is_a_loud_error():
    """Without a device both forms fail with SPV_ERR_HIP, never with a host computation."""
    from spectavi_amd import _lib, feature
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    x, seg, d = cb.collection([4, 4], 16, 6, 2, 2)
    with pytest.raises(_lib.SpectaviError):
        feature.nn_cascading_hash_batch([x[:4], x[4:]], d)
    need = _lib.clib.spv_cascade_batch_workspace_bytes(seg.ctypes.data, 2, 16, 6, 2, 2, PRS2[:1].ctypes.data, 1)
    st = _lib.clib.spv_cascade_batch_device(FAKE, seg.ctypes.data, 2, 16, 6, 2, 2, PRS2[:1].ctypes.data, 1, FAKE, FAKE, FAKE,
                                            FAKE, FAKE, need, None)
    assert st == _lib.SPV_ERR_HIP and _lib.clib.spv_last_error()
