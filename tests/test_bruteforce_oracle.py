"""CPU only: the numpy oracle of the p-norm k-NN contract (tests/bruteforce_oracle.py) against a
literal pure-Python streaming scan, and its tie, sentinel and int-truncation rules."""
import heapq
import math
import struct

import numpy as np
import pytest

from tests import bruteforce_oracle as bo


def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def scalar_term(d, p, is_int):
    pd = float(np.float32(p))
    if pd == 1:
        t = abs(d)
    elif pd == 2:
        t = f32(d * d)
    elif pd == 0.5:
        t = f32(math.sqrt(abs(d)))  # sqrt of a float32 rounded once to float32: correctly rounded
    else:
        t = math.pow(abs(d), pd)
        if not is_int:
            t = f32(t)
    return int(t) if is_int else t


def scan(x, y, p, k, is_int):
    """One query at a time, rows in ascending order, a bounded max-heap of (dist, idx)."""
    out_i, out_d = [], []
    for q in y:
        heap = []
        for j, row in enumerate(x):
            s = 0
            for a, b in zip(row, q):
                d = float(int(a) - int(b)) if is_int else f32(float(a) - float(b))
                s = (s + scalar_term(d, p, is_int)) if is_int else f32(s + scalar_term(d, p, is_int))
            item = (-s, -j)
            if len(heap) < k:
                heapq.heappush(heap, item)
            elif item > heap[0]:  # (s, j) < the current k-th, lexicographically
                heapq.heapreplace(heap, item)
        best = sorted((-a, -b) for a, b in heap)
        out_i.append([j for _, j in best])
        out_d.append([s for s, _ in best])
    return out_i, out_d


@pytest.mark.parametrize("is_int", [False, True])
@pytest.mark.parametrize("p", [1.0, 2.0, 0.5, 1.5, 3.0])
def test_oracle_matches_streaming_scan(p, is_int):
    rng = np.random.default_rng([int(p * 10), is_int])
    if is_int:
        x = rng.integers(-300, 300, (40, 7)).astype(np.int32)
        y = rng.integers(-300, 300, (6, 7)).astype(np.int32)
    else:
        x = rng.standard_normal((40, 7)).astype(np.float32)
        y = rng.standard_normal((6, 7)).astype(np.float32)
    k = 5
    idx, dist = bo.nn_bruteforce(x, y, p, k, is_int)
    si, sd = scan(x, y, p, k, is_int)
    assert idx.tolist() == si
    if is_int:
        assert dist.tolist() == sd
    else:
        assert np.array_equal(dist, np.array(sd, np.float32))


def test_ties_are_broken_by_the_lower_index():
    x = np.array([[1], [0], [1], [-1], [0]], np.float32)
    y = np.array([[0]], np.float32)
    idx, dist = bo.nn_bruteforce(x, y, 2.0, 4)
    assert idx.tolist() == [[1, 4, 0, 2]] and dist.tolist() == [[0, 0, 1, 1]]


def test_missing_neighbours_are_sentinels():
    x = np.zeros((2, 3), np.float32)
    y = np.ones((2, 3), np.float32)
    idx, dist = bo.nn_bruteforce(x, y, 1.0, 4)
    assert idx[:, 2:].tolist() == [[2**64 - 1] * 2] * 2 and np.all(np.isinf(dist[:, 2:]))
    assert dist[:, :2].tolist() == [[3, 3]] * 2 and idx[:, :2].tolist() == [[0, 1]] * 2
    idx, dist = bo.nn_bruteforce(x.astype(np.int32), y.astype(np.int32), 1.0, 3, is_int=True)
    assert idx[:, 2].tolist() == [2**64 - 1] * 2 and dist[:, 2].tolist() == [2**31 - 1] * 2
    idx, dist = bo.nn_bruteforce(np.zeros((0, 3), np.float32), y, 2.0, 2)
    assert np.all(idx == bo.NONE_IDX) and np.all(np.isinf(dist))


def test_int_terms_truncate():
    # int(sqrtf(2)) == 1, int(sqrtf(8)) == 2
    assert bo.term(np.float32([2, 8, 9]), 0.5, True).tolist() == [1, 2, 3]
    # pow truncated from the double: 3^1.5 = 5.196..., 2^3 = 8
    assert bo.term(np.float32([3, 2, -2]), 1.5, True).tolist() == [5, 2, 2]
    assert bo.term(np.float32([2, -3]), 3.0, True).tolist() == [8, 27]
    x = np.array([[2, 0], [0, 0]], np.int32)
    y = np.array([[0, 2]], np.int32)
    _, dist = bo.nn_bruteforce(x, y, 0.5, 2, is_int=True)
    assert dist.tolist() == [[1, 2]]  # row 1: int(sqrt 2) = 1; row 0: 1 + 1


def test_p_branches_follow_the_float_argument():
    assert bo.p_kind(0.5) == 0.5 and bo.p_kind(1) == 1 and bo.p_kind(2.0) == 2
    assert bo.p_kind(1.5) is None and bo.p_kind(0.1) is None  # 0.1f widened is not 0.5, 1 or 2


def test_float_sum_is_sequential():
    # 1e8 + 1 + 1 ... in float32 stays 1e8 when added one at a time (a pairwise sum would not)
    x = np.array([[1e4] + [1.0] * 16], np.float32)
    y = np.zeros((1, 17), np.float32)
    d = bo.distances(x, y, 2.0)
    assert d[0, 0] == np.float32(1e8)


# ---- the value classes of tests/bruteforce_value_cases.py reach what they were chosen for, and three
# ---- wrong kernels that today's randn / +-50 data lets through would not pass on them ----------------
from functools import lru_cache  # noqa: E402

from tests import bruteforce_value_cases as vc  # noqa: E402
from tests.test_bruteforce_gpu import data  # noqa: E402  (the data of the existing GPU tests)

TINY = np.float32(2.0 ** -126)


@lru_cache(maxsize=None)
def class_distances(cls, dim, p):
    x, y = vc.make(cls, dim)
    return bo.distances(x, y, p, vc.BY_NAME[cls].is_int)


def exact_int_distances(x, y, p):
    """Wrong kernel 1: int rows in exact integer arithmetic (|d|, d*d, isqrt |d|), not through float32."""
    x, y = x.astype(np.int64), y.astype(np.int64)
    out = np.zeros((y.shape[0], x.shape[0]), np.int64)
    for c in range(x.shape[1]):
        a = np.abs(x[None, :, c] - y[:, None, c])
        if p == 0.5:
            r = np.floor(np.sqrt(a.astype(np.float64))).astype(np.int64)
            a = r - (r * r > a)
        elif p == 2.0:
            a = a * a
        out += a
    return out.astype(np.int32)


def ftz(a):
    return np.where(np.abs(a) < TINY, np.copysign(np.float32(0), a), a).astype(np.float32)


def ftz_distances(x, y, p):
    """Wrong kernel 2: float32 subnormals flushed to zero in the inputs, the terms and the partial sums."""
    x, y = ftz(x), ftz(y)
    out = np.zeros((y.shape[0], x.shape[0]), np.float32)
    for c in range(x.shape[1]):
        with np.errstate(over="ignore", invalid="ignore"):
            d = ftz(x[None, :, c] - y[:, None, c])
            out = ftz(out + ftz(bo.term(d, p, False)))
    return out


def inf_is_none_select(dist, k):
    """Wrong kernel 3: a distance of +inf taken for "no neighbour"."""
    idx, out = bo.select(dist, k)
    idx[np.isposinf(out)] = bo.NONE_IDX
    return idx, out


def differ(a, b):
    return float((a.view(np.uint32) != b.view(np.uint32)).mean())


def test_value_case_table_reaches_every_exact_instantiation():
    assert vc.REACHED == vc.EXACT_INSTANTIATIONS and len(vc.REACHED) == 18
    assert len({vc.case_id(c) for c in vc.CASES}) == len(vc.CASES)
    for c in vc.CASES:
        assert c.p in vc.BY_NAME[c.cls].ps and c.dim in vc.BY_NAME[c.cls].dims and c.k in vc.KS
        x, y = vc.case_data(c)
        assert x.shape == (97, c.dim) and y.shape == (70, c.dim)
        assert x.dtype == y.dtype == (np.int32 if c.is_int else np.float32)
        assert c.is_int or (np.isfinite(x).all() and np.isfinite(y).all())


def test_int_cases_are_inside_the_domain():
    for c in vc.CASES:
        if c.is_int:
            x, y = vc.case_data(c)
            assert vc.int_domain_ok(x, y, c.p) and vc.int_domain_bound_ok(x, y, c.p), vc.case_id(c)
    # and the check itself sees each way out of the domain: x - y, a term, a partial sum
    a, b = np.array([[2 ** 30]], np.int32), np.array([[-2 ** 30]], np.int32)
    assert not vc.int_domain_ok(a, b, 1.0) and not vc.int_domain_bound_ok(a, b, 1.0)
    a, b = np.array([[46341]], np.int32), np.array([[0]], np.int32)
    assert not vc.int_domain_ok(a, b, 2.0) and vc.int_domain_ok(a - 1, b, 2.0)
    a, b = np.full((1, 3), 2 ** 29, np.int32), np.full((1, 3), -2 ** 29 + 1, np.int32)
    assert not vc.int_domain_ok(a, b, 1.0) and vc.int_domain_ok(a[:, :1], b[:, :1], 1.0)


def test_exact_integer_mutant_passes_on_small_ints_and_fails_on_the_big_classes():
    rng = np.random.default_rng(5)
    x, y = data(rng, 97, 40, True), data(rng, 70, 40, True)
    for p in (1.0, 2.0, 0.5):
        assert differ(exact_int_distances(x, y, p), bo.distances(x, y, p, True)) == 0
    seen = set()
    for c in vc.CASES:
        if not c.is_int or (c.cls, c.dim) in seen:
            continue
        seen.add((c.cls, c.dim))
        x, y = vc.case_data(c)
        share = differ(exact_int_distances(x, y, c.p), class_distances(c.cls, c.dim, c.p))
        if c.cls == "i_big_half":
            assert share > 0, vc.case_id(c)
        else:
            assert share >= 0.25, (vc.case_id(c), share)
    assert len(seen) == 6


def test_flush_to_zero_mutant_passes_on_randn_and_fails_on_subn_and_under():
    rng = np.random.default_rng(6)
    x, y = data(rng, 97, 40, False), data(rng, 70, 40, False)
    for p in (1.0, 2.0, 0.5):
        assert differ(ftz_distances(x, y, p), bo.distances(x, y, p)) == 0
    for cls, p, dims, least in (("subn", 1.0, (7, 40), 1.0), ("subn", 0.5, (7, 40), 1.0),
                                ("under", 2.0, (7,), 1.0), ("under", 2.0, (40,), 0.9)):
        for dim in dims:
            x, y = vc.make(cls, dim)
            want = class_distances(cls, dim, p)
            assert differ(ftz_distances(x, y, p), want) >= least, (cls, p, dim)
            if least == 1.0 and p != 0.5:   # because every one of them is a non-zero subnormal
                assert vc.describe(want, 2)["subnormal"] == 1.0


def test_overflow_and_underflow_classes_reach_inf_zero_and_ties():
    for c in vc.CASES:
        if c.is_int:
            continue
        d = class_distances(c.cls, c.dim, c.p)
        got = vc.describe(d, c.k)
        assert got["nan"] == 0 and not np.signbit(d).any(), vc.case_id(c)
        idx, dist = bo.nn_bruteforce(*vc.case_data(c), c.p, c.k)
        if c.cls == "max" or (c.cls == "huge" and c.p == 2.0):
            assert got["inf"] >= 0.9, (vc.case_id(c), got)
        if c.cls == "zeros" or (c.cls == "subn" and c.p == 2.0):
            # all distances +0: every query's k-th place is a tie, the k lowest indices win
            assert got["zero"] == 1.0 and got["kth_tie"] == 1.0
            assert np.array_equal(idx, np.tile(np.arange(c.k, dtype=np.uint64), (70, 1)))
            assert not dist.view(np.uint32).any()
        if c.cls == "max" and c.p == 2.0:
            # all distances +inf (|x - y| >= 1e38 squared, or inf squared): the same tie at +inf
            assert got["inf"] == 1.0 and got["kth_tie"] == 1.0
            assert np.array_equal(idx, np.tile(np.arange(c.k, dtype=np.uint64), (70, 1)))
            assert (dist.view(np.uint32) == 0x7F800000).all()
    # finite where the class says so
    assert vc.describe(class_distances("huge", 40, 1.0), 2)["inf"] == 0
    assert vc.describe(class_distances("huge", 40, 0.5), 2)["inf"] == 0


@pytest.mark.parametrize("k", [2, 17])
def test_real_neighbour_at_inf_precedes_a_missing_one(k):
    for xrows in sorted({1, k - 1}):
        x, y = vc.make("max", 7, xrows=xrows)
        idx, dist = bo.nn_bruteforce(x, y, 2.0, k)
        assert np.array_equal(idx[:, :xrows], np.tile(np.arange(xrows, dtype=np.uint64), (70, 1)))
        assert (idx[:, xrows:] == bo.NONE_IDX).all()
        assert (dist.view(np.uint32) == 0x7F800000).all()   # real and missing alike: only idx tells them apart
        # the third wrong kernel loses the real ones
        mi, _ = inf_is_none_select(bo.distances(x, y, 2.0), k)
        assert (mi == bo.NONE_IDX).all()


def test_inf_is_none_mutant_passes_on_randn_and_fails_on_huge_and_max():
    rng = np.random.default_rng(7)
    x, y = data(rng, 97, 40, False), data(rng, 70, 40, False)
    d = bo.distances(x, y, 2.0)
    assert np.array_equal(inf_is_none_select(d, 8)[0], bo.select(d, 8)[0])
    for cls, p, dim in (("huge", 2.0, 40), ("max", 1.0, 40), ("max", 2.0, 7), ("max", 0.5, 7)):
        d = class_distances(cls, dim, p)
        wrong = (inf_is_none_select(d, 8)[0] != bo.select(d, 8)[0]).any(1)
        assert wrong.mean() >= 0.9, (cls, p, dim)
