"""Host only: the collections of tests/test_cascade_batch_edges_gpu.py reach the paths of cascade_batch.hip they are
named after.  The CPU oracle's codes, signs and masks (debug=True) and the library's own plan (device.cascade_batch_plan)
show the bucket bits, the composition of the buckets, the candidate counts and where the neighbours lie, so the GPU
tests cannot pass by missing their path."""
import numpy as np
import pytest

from tests import cascade_batch_cases as cb


def plan_of(case):
    from spectavi_amd import device
    x, seg, d, pairs, g = case
    n, dim, m = d.shape
    assert len(x) == seg[-1] and x.shape[1] == dim
    return device.cascade_batch_plan(seg, pairs, dim, m, n, g)


def oracle_debug(case, a, b):
    """(idx, dist, ncand, nset, xcodes [n, rows of b], ysign, ymask [n, rows of a]) of the pair (query a, database b)."""
    from oracle import oracle as o
    x, seg, d, _, g = case
    n, _, m = d.shape
    return o.nn_cascading_hash(x[seg[b]:seg[b + 1]], x[seg[a]:seg[a + 1]], m, n, g, d, debug=True)


def probe_codes(sign, mask, g):
    """The 2^g probe codes of one query and table: the sign code with every subset of the mask's bits."""
    bits = [b for b in range(32) if (int(mask) >> b) & 1]
    assert len(bits) == g
    base = int(sign) & ~int(mask)
    return [base | sum(1 << b for k, b in enumerate(bits) if (var >> k) & 1) for var in range(1 << g)]


@pytest.mark.parametrize("big,m,hb", cb.BITS_EDGE)
def test_bucket_bits_change_between_4096_and_4097_rows(big, m, hb):
    case = cb.bits_edge(big, m)
    plan = plan_of(case)
    assert plan["hb"] == hb and (hb < m) == (m == 20)
    assert list(np.diff(case[1])) == [257, 513, big]
    assert -(-((1 << hb) + 1) // 1024) == (5 if hb == 12 else 9)   # scan segments of 1024 entries per table
    pairs = set(case[3])
    assert all((a, b) in pairs for a in range(3) for b in range(3) if a != b) and (2, 2) in pairs


def test_bystander_sets_change_the_bucket_bits_and_nothing_else():
    small = None
    for rows, hb in cb.BYSTANDERS:
        x, seg, d, pairs, g = case = cb.invariance(rows)
        assert plan_of(case)["hb"] == hb < cb.INVARIANCE_SHAPE[1]
        assert seg[3] - seg[2] == rows and all(2 not in p for p in pairs)
        if small is None:
            small = x[:seg[2]].copy()
        assert np.array_equal(x[:seg[2]], small) and np.array_equal(seg[:3], [0, 257, 387])
    # the pair has something to find in both directions: dozens of queries meet candidates, in differing numbers
    for a, b in ((0, 1), (1, 0)):
        ncand = oracle_debug(case, a, b)[2]
        assert (ncand >= 1).sum() >= 30 and len(np.unique(ncand)) > 2


def test_the_cap_collection_takes_the_cap():
    x, seg, d, pairs, g = case = cb.cap()
    dim, m, n, _ = cb.CAP_SHAPE
    plan = plan_of(case)
    nseg = len(seg) - 1
    assert nseg == cb.CAP_SETS and 65520 < nseg * n <= 65535
    assert nseg * n * (2 ** 12 + 1) * 4 > 2 ** 30 >= nseg * n * (2 ** 11 + 1) * 4
    assert plan["hb"] == 11 and plan["workspace_bytes"] < 2 ** 30
    rows = np.diff(seg)
    for s, r in cb.CAP_BIG.items():
        assert rows[s] == r and 100 <= r <= 300
    assert sorted(cb.CAP_BIG) == [0, 1, 16383, 32765, 32766]
    small = np.delete(rows, sorted(cb.CAP_BIG))
    assert set(small) == {0, 1, 2} and min(np.bincount(small)) > 5000
    empty_runs = np.diff(np.nonzero(np.concatenate([[1], rows, [1]]))[0]) - 1
    assert empty_runs.max() >= 20 and (empty_runs >= 2).sum() > 1000   # runs of consecutive empty sets
    # every ordered pair of the five; tiny and empty sets as query and as database
    assert all((a, b) in pairs for a in cb.CAP_BIG for b in cb.CAP_BIG)
    others = [(a, b) for a, b in pairs if not (a in cb.CAP_BIG and b in cb.CAP_BIG)]
    assert len(others) >= 24
    for k in (0, 1):
        assert {0, 1, 2} <= {int(rows[p[k]]) for p in others}
    # the planted near-copies: pairs of neighbouring big sets share candidates, and so do one-row sets with set 0
    big = sorted(cb.CAP_BIG)
    for a, b in zip(big[1:], big[:-1]):
        assert (oracle_debug(case, a, b)[2] >= 1).sum() >= cb.CAP_BIG[a] // 4
    assert sum(int(oracle_debug(case, a, b)[2].sum() > 0) for a, b in others if rows[a] == 1 and b == 0) >= 5
    # m > hb: the full-code filter runs with 11-bit buckets
    assert m > plan["hb"]


@pytest.mark.parametrize("n", cb.FILTER_TABLES)
def test_the_mixed_bucket_holds_two_full_codes_interleaved(n):
    x, seg, d, pairs, g = case = cb.mixed_bucket(n)
    dim, m = cb.FILTER_SHAPE[:2]
    assert d.shape == (n, dim, m)
    hb = plan_of(case)["hb"]
    assert hb == 12 < m and list(np.diff(seg)) == cb.FILTER_ROWS and pairs == [(2, 1), (1, 2)]
    _, _, ncand, _, xcodes, ysign, ymask = oracle_debug(case, 2, 1)
    low = xcodes[0] & ((1 << hb) - 1)
    assert (low == low[0]).all(), "table 0: one bucket of 300 entries, five 64-entry steps of the probe"
    codes, counts = np.unique(xcodes[0], return_counts=True)
    assert len(codes) == 2 and list(counts) == [150, 150] and (counts >= 128).all()
    assert (xcodes[0][0::2] == xcodes[0][0]).all() and (xcodes[0][1::2] == xcodes[0][1]).all(), "interleaved row by row"
    assert xcodes[0][0] != xcodes[0][1]
    # rows are not bucket entries: the fill order is atomic.  But whatever the order, both codes are in the bucket,
    # and each of the five steps of 64 can hold entries of both
    assert (ncand == 150 * n).all(), "150 of table 0 and, with two tables, 150 of table 1: 300"
    for j in range(1, n):   # the second table holds every copy of a parent under one code: it alone finds them all
        assert len(np.unique(xcodes[j][0::2])) == len(np.unique(xcodes[j][1::2])) == 1
    unfiltered = np.zeros(len(ncand), np.int64)
    for q in range(len(ncand)):
        for j in range(n):
            lowx = xcodes[j] & ((1 << hb) - 1)
            unfiltered[q] += sum(int((lowx == (c & ((1 << hb) - 1))).sum()) for c in probe_codes(ysign[j, q], ymask[j, q], g))
    assert (unfiltered >= 150 * n + 150).all(), "without the full-code filter every query would count the other code's 150 too"
    # the reverse pair: 40 database rows, one bucket of two codes in a single step
    back = oracle_debug(case, 1, 2)
    assert (back[2] == 20 * n).all() and len(np.unique(back[4][0])) == 2 and len(np.unique(back[4][0] & 4095)) == 1


def test_the_long_bucket_with_the_filter_on():
    x, seg, d, pairs, g = case = cb.long_bucket(cb.FILTER_SHAPE)
    assert plan_of(case)["hb"] == 12 < cb.FILTER_SHAPE[1]
    ncand, xcodes = oracle_debug(case, 2, 1)[2], oracle_debug(case, 2, 1)[4]
    assert xcodes.shape == (2, 1500) and (xcodes == xcodes[:, :1]).all(), "one code per table: 24 steps of 64"
    assert (ncand[cb.LONG_HIT] == 3000).all()
    # the pair (1, 0): 1500 equal queries against a normal set
    assert plan_of(cb.long_bucket(cb.NINE_SHAPE))["hb"] == 6 == cb.NINE_SHAPE[1]


def test_the_buckets_fit_the_list_one_by_one_but_not_together():
    x, seg, d, pairs, g = case = cb.bucket_sum()
    dim, m, n, _ = cb.SUM_SHAPE
    assert plan_of(case)["hb"] == m == 4, "hb = m: no filter, the fast path is tried first"
    assert n << g <= 64, "all probes of a query in one pass of the wave: the pass's total is the candidate count"
    _, _, ncand, _, xcodes, ysign, ymask = oracle_debug(case, 1, 0)
    largest = max(int(np.bincount(xcodes[j], minlength=16).max()) for j in range(n))
    assert largest == 243 < cb.LIST_CAP
    assert ncand.min() == 836 > cb.LIST_CAP and ncand.max() == 1286
    for q in (0, 50, 99):   # the count is the sum of the probed buckets
        assert ncand[q] == sum(int((xcodes[j] == c).sum()) for j in range(n) for c in probe_codes(ysign[j, q], ymask[j, q], g))
    # the reverse pair stays on the fast path: every query's buckets fit together
    back = oracle_debug(case, 0, 1)[2]
    assert 0 < back.min() and back.max() <= cb.LIST_CAP


def test_the_stride_collection_passes_one_grid_of_rows():
    x, seg, d, pairs, g = case = cb.stride()
    dim, m, n, _ = cb.STRIDE_SHAPE
    plan = plan_of(case)
    assert plan["hb"] == 19 < m
    assert cb.GRID_ROWS == 524288 and list(seg) == [0, 524238, 524938, 525238]
    assert seg[1] + 50 == cb.GRID_ROWS and seg[2] > cb.GRID_ROWS, "set 1 straddles the boundary, set 2 lies past it"
    assert pairs == [(2, 1), (1, 2), (2, 2), (1, 1), (2, 0)]
    idx, _, ncand = oracle_debug(case, 2, 1)[:3]
    assert (ncand >= 1).all()
    assert (idx[:, 0] != np.uint64(2 ** 64 - 1)).all() and (idx[:, 0] >= 50).mean() >= 0.9, \
        "the first neighbour is a row the second trip of the loops ranked and filled"
    assert (idx[:, 0] < 50).any(), "... and some lie before the boundary"
    big = oracle_debug(case, 2, 0)[2]
    assert (big >= 1).mean() > 0.9 and big.max() > 64


def test_the_form_cases_are_the_variant_table_below_the_batch_limit():
    from tests import cascade_variant_cases as cv
    cases = [c for c in cv.CASES if c[0] <= 256]
    assert len(cv.CASES) == 55 and len(cases) == 54
    assert sum(cb.FORMS_ROWS) == 528 and len(cb.FORMS_PAIRS) == 7
    seg = cb.seg_of(cb.FORMS_ROWS)
    assert all(seg[s] % 256 for s in (1, 2, 3)), "no set starts at a projection tile"
