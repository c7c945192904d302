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
