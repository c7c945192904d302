"""CPU-only: every function of spectavi_amd._collection at the edges of its rule, with the dtype, shape and
contiguity of what it hands to the library.  The module needs numpy alone."""
import subprocess
import sys

import numpy as np
import pytest

from spectavi_amd import _collection as col

B31 = 2 ** 31


def is_array(a, dtype, shape):
    assert isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == shape and a.flags.c_contiguous, (a.dtype, a.shape)
    return a


def test_needs_numpy_alone():
    # (importing the package itself loads the library: the module file is imported on its own)
    code = ("import importlib.util, sys; s = importlib.util.spec_from_file_location('c', %r); m = importlib.util.module_from_spec(s); "
            "s.loader.exec_module(m); bad = [n for n in ('torch', 'spectavi_amd', 'spectavi_amd._lib') if n in sys.modules]; "
            "assert not bad, bad; assert m.offsets([0, 2], 'o').tolist() == [0, 2]" % col.__file__)
    subprocess.run([sys.executable, "-c", code], check=True)


def test_offsets():
    assert is_array(col.offsets([0], "o"), np.int64, (1,)).tolist() == [0]
    assert is_array(col.offsets([0, 3, 3, 10], "o", 10, "t"), np.int64, (4,)).tolist() == [0, 3, 3, 10]
    strided = np.array([[0, 9], [4, 9], [7, 9]], np.int32)[:, 0]
    assert is_array(col.offsets(strided, "o"), np.int64, (3,)).tolist() == [0, 4, 7]
    assert is_array(col.offsets([[0, 2], [2, 5]], "o"), np.int64, (4,)).tolist() == [0, 2, 2, 5]       # flattened
    same = np.array([0, 2], np.int64)
    assert col.offsets(same, "o") is same or np.shares_memory(col.offsets(same, "o"), same)             # nothing copied
    assert col.offsets([0, B31 - 1], "o")[-1] == B31 - 1
    assert col.offsets([0, 5], "o", count=1).size == 2 and col.offsets([0], "o", count=0).size == 1
    for bad, kw in (([], {}), ([1, 2], {}), ([0, 3, 2], {}), ([0, -1], {}), ([0, B31], {}), ([0, B31 + 5, B31 + 5], {}),
                    ([0, 4], dict(rows=5, rows_of="t")), ([0, 6], dict(rows=5, rows_of="t")), ([0], dict(rows=1, rows_of="t")),
                    ([0, 4], dict(count=2)), ([0, 4], dict(count=0)), ([], dict(count=-1)), ([0, B31], dict(rows=B31, rows_of="t"))):
        with pytest.raises(ValueError) as info:
            col.offsets(bad, "the_name", **kw)
        assert "the_name" in str(info.value)
    with pytest.raises(ValueError, match="the_table has 5 rows"):
        col.offsets([0, 4], "o", 5, "the_table")


def test_offsets_unchecked_checks_emptiness_alone():
    for seq in ([1, 2], [0, 3, 2], [0, B31], [7]):
        assert is_array(col.offsets_unchecked(seq, "o"), np.int64, (len(seq),)).tolist() == seq
    with pytest.raises(ValueError, match="the_name"):
        col.offsets_unchecked([], "the_name")


def test_offsets_of():
    assert is_array(col.offsets_of([]), np.int64, (1,)).tolist() == [0]
    assert is_array(col.offsets_of([3, 0, 7]), np.int64, (4,)).tolist() == [0, 3, 3, 10]
    assert is_array(col.offsets_of(np.array([2, 5], np.int32)), np.int64, (3,)).tolist() == [0, 2, 7]
    assert col.offsets_of([2 ** 30] * 4)[-1] == 2 ** 32                      # summed in int64; no rule of its own
    assert is_array(col.offsets_of(np.array([B31 - 1, 1], np.int32)), np.int64, (3,))[-1] == B31


def test_offsets_of_sizes():
    n, seg = col.offsets_of_sizes([], "table")
    assert n == 0 and is_array(seg, np.int64, (1,)).tolist() == [0]
    n, seg = col.offsets_of_sizes([3, 0, 7], "table")
    assert n == 3 and is_array(seg, np.int64, (4,)).tolist() == [0, 3, 3, 10]
    assert col.offsets_of_sizes(np.array([4], np.uint8), "table")[1].tolist() == [0, 4]
    assert col.offsets_of_sizes([2 ** 30, 2 ** 30 - 1], "table")[1][-1] == B31 - 1
    for bad in ([3, -1], [3.0, 4.0], [[3, 4]], 3, [2 ** 30, 2 ** 30]):
        with pytest.raises(ValueError):
            col.offsets_of_sizes(bad, "table")
    with pytest.raises(ValueError, match="one per view"):
        col.offsets_of_sizes([-1], "view")


def test_check_set_count():
    assert col.MAX_SETS == 2 ** 20
    col.check_set_count(0)
    col.check_set_count(2 ** 20)
    with pytest.raises(ValueError):
        col.check_set_count(2 ** 20 + 1)


def test_all_pairs():
    assert col.all_pairs(0) == [] and col.all_pairs(1) == []
    assert col.all_pairs(2) == [(1, 0)]
    assert col.all_pairs(4) == [(1, 0), (2, 0), (3, 0), (2, 1), (3, 1), (3, 2)]       # (query j, database i), i < j
    assert is_array(col.pair_table(col.all_pairs(3), 3), np.int32, (3, 2)).tolist() == [[1, 0], [2, 0], [2, 1]]


def test_pair_table():
    for empty in ([], (), np.zeros((0, 2), np.int64), np.zeros(0), np.zeros((0, 5))):
        is_array(col.pair_table(empty, 0), np.int32, (0, 2))
    got = col.pair_table([[2, 0], [1, 1], [2, 0]], 3)                               # self and duplicate pairs
    assert is_array(got, np.int32, (3, 2)).tolist() == [[2, 0], [1, 1], [2, 0]]
    assert is_array(col.pair_table(np.array([[1, 0]], np.uint64), 2), np.int32, (1, 2)).tolist() == [[1, 0]]
    strided = np.array([[1, 0, 9], [0, 1, 9]], np.int64)[:, :2]
    assert is_array(col.pair_table(strided, 2), np.int32, (2, 2)).tolist() == [[1, 0], [0, 1]]
    assert col.pair_table([[2 ** 20, 0]], 2 ** 20 + 1).tolist() == [[2 ** 20, 0]]
    for bad, nseg in (([[0, 2]], 2), ([[2, 0]], 2), ([[-1, 0]], 2), ([[0, 0]], 0), ([0, 1], 2), ([[0, 1, 0]], 2),
                      ([[0.0, 1.0]], 2), ([[True, False]], 2), (None, 2), ([[[0, 1]]], 2), ([[2 ** 40, 0]], 2)):
        with pytest.raises(ValueError):
            col.pair_table(bad, nseg)
    with pytest.raises(ValueError, match=r"pairs name tables outside \[0, 2\)"):
        col.pair_table([[0, 2]], 2, "tables")


def test_out_offsets():
    seg = col.offsets([0, 3, 3, 10], "o")
    prs = col.pair_table([[2, 0], [1, 0], [0, 2], [2, 2]], 3)
    assert is_array(col.out_offsets(seg, prs), np.int64, (5,)).tolist() == [0, 7, 7, 10, 17]    # rows of the QUERY set
    assert is_array(col.out_offsets(seg, col.pair_table([], 3)), np.int64, (1,)).tolist() == [0]
    assert is_array(col.out_offsets(col.offsets([0], "o"), col.pair_table([], 0)), np.int64, (1,)).tolist() == [0]
    big = col.offsets([0, 2 ** 30, B31 - 1], "o")
    two = col.pair_table([[0, 0], [1, 1]], 2)
    assert col.out_offsets(big, two, below_2_31=True)[-1] == B31 - 1
    twice = col.pair_table([[0, 0], [0, 0]], 2)
    assert col.out_offsets(big, twice)[-1] == B31                                   # no rule unless asked for
    with pytest.raises(ValueError):
        col.out_offsets(big, twice, below_2_31=True)


def test_per_pair():
    idx, dist = np.arange(10).reshape(5, 2), np.arange(5.0)
    got = col.per_pair(np.array([0, 2, 2, 5]), idx, dist)
    assert [(a.tolist(), b.tolist()) for a, b in got] == [([[0, 1], [2, 3]], [0, 1]), ([], []), ([[4, 5], [6, 7], [8, 9]], [2, 3, 4])]
    assert all(np.shares_memory(a, idx) and np.shares_memory(b, dist) for a, b in got if len(a))   # views, not copies
    assert col.per_pair(np.array([0]), idx) == []
    assert [t[0].tolist() for t in col.per_pair([0, 1], dist)] == [[0.0]] and isinstance(col.per_pair([0, 1], dist)[0], tuple)


def test_check_matcher_dim():
    for dim in (16, 32, 128, 240, 256):
        col.check_matcher_dim(dim)
    for dim in (0, -16, 1, 8, 15, 17, 24, 255, 257, 272, 2048):
        with pytest.raises(ValueError):
            col.check_matcher_dim(dim)


def test_use_flags():
    assert col.use_flags(None, 3) is None
    assert is_array(col.use_flags([], 0), np.int32, (0,)).size == 0
    assert is_array(col.use_flags([1, 0, -3, 0.5, 0.0, True, False, float("nan")], 8), np.int32, (8,)).tolist() == [1, 0, 1, 1, 0, 1, 0, 1]
    assert is_array(col.use_flags(np.array([[2], [0]], np.uint8), 2), np.int32, (2,)).tolist() == [1, 0]
    assert is_array(col.use_flags(np.array([0, 7, 0, 7], np.int64)[::2], 2), np.int32, (2,)).tolist() == [0, 0]
    for bad, n in (([1], 2), ([1, 1, 1], 2), ([], 1), (1, 2)):
        with pytest.raises(ValueError, match="one value per pair"):
            col.use_flags(bad, n, "pair")


P = np.arange(12.0).reshape(3, 4)


def test_packed_cameras():
    assert is_array(col.packed_cameras([P, 2 * P], 2, "P1s"), np.float64, (2, 12))[1].tolist() == (2 * P).reshape(-1).tolist()
    assert is_array(col.packed_cameras(np.stack([P, P]).astype(np.float32), 2, "P1s"), np.float64, (2, 12))[0].tolist() == list(range(12))
    assert not is_array(col.packed_cameras(np.zeros((2, 12)), 2, "P1s"), np.float64, (2, 12)).any()
    assert is_array(col.packed_cameras(np.zeros((4, 3, 4))[::2], 2, "P1s"), np.float64, (2, 12)).shape == (2, 12)   # made contiguous
    is_array(col.packed_cameras([], 0, "P1s"), np.float64, (0, 12))
    is_array(col.packed_cameras("not looked at", 0, "P1s"), np.float64, (0, 12))       # no set: nothing to read
    for bad, n in (([P], 2), ([P, P, P], 2), (np.zeros((2, 3, 3)), 2), ([], 1)):
        with pytest.raises(ValueError):
            col.packed_cameras(bad, n, "P1s")
    with pytest.raises(ValueError, match="P0s must hold one .* per pair"):
        col.packed_cameras([P], 2, "P0s", "pair")


def test_none_cameras_skip():
    Ps, use = col.none_cameras_skip([P, None, P], 3, "P1s", None)
    assert is_array(use, np.int32, (3,)).tolist() == [1, 0, 1] and not Ps[1].any() and Ps[1].shape == (3, 4) and Ps[0] is P
    Ps, use = col.none_cameras_skip([P, None, P], 3, "P1s", col.use_flags([0, 1, 5], 3))
    assert is_array(use, np.int32, (3,)).tolist() == [0, 0, 1]
    assert is_array(col.packed_cameras(Ps, 3, "P1s"), np.float64, (3, 12))[1].tolist() == [0.0] * 12
    # nothing is None: both come back as they went in, a use of None stays None
    listed, arr, flags = [P, P], np.zeros((2, 3, 4)), col.use_flags([1, 0], 2)
    assert col.none_cameras_skip(listed, 2, "P1s", None) == (listed, None)
    got = col.none_cameras_skip(arr, 2, "P1s", flags)
    assert got[0] is arr and got[1] is flags
    assert col.none_cameras_skip([], 0, "P1s", None) == ([], None)
    for bad, n in (([None], 2), ([P, None, None], 2)):
        with pytest.raises(ValueError, match="cameras must hold one .* per view"):
            col.none_cameras_skip(bad, n, "cameras", None, "view")


@pytest.mark.parametrize("exc", [TypeError, ValueError])
def test_listed_cameras(exc):
    cams, have = col.listed_cameras([P, None, 2 * P], 3, "P1s", exc)
    assert is_array(cams, np.float64, (3, 12)).tolist() == [P.reshape(-1).tolist(), [0.0] * 12, (2 * P).reshape(-1).tolist()]
    assert is_array(have, np.int32, (3,)).tolist() == [1, 0, 1]
    cams, have = col.listed_cameras([], 0, "P1s", exc)
    is_array(cams, np.float64, (0, 12))
    is_array(have, np.int32, (0,))
    assert col.listed_cameras([P.astype(np.float32).tolist()], 1, "P1s", exc)[0].tolist() == [P.reshape(-1).tolist()]
    # a None entry is refused only where it is needed
    cams, have = col.listed_cameras([None, P], 2, "P0s", exc, needed=[0, 1])
    assert have.tolist() == [0, 1] and not cams[0].any()
    for bad, kw in (([np.zeros((4, 4))], {}), ([np.zeros(12)], {}), ([np.zeros((3, 3))], {}), ([None], dict(needed=[1])),
                    ([None], dict(needed=np.array([5], np.int32))), ([np.zeros((2, 2))], dict(needed=[0]))):
        with pytest.raises(exc) as info:
            col.listed_cameras(bad, 1, "the_name", exc, **kw)
        assert info.type is exc and "the_name" in str(info.value)


def test_seeds_and_tries():
    seeds, tries = col.seeds_and_tries(None, None, 500, 3)
    assert is_array(seeds, np.uint64, (3,)).tolist() == [0, 0, 0] and tries == 500 and type(tries) is int
    seeds, tries = col.seeds_and_tries([[1], [2 ** 63]], None, 0.0, 2)
    assert is_array(seeds, np.uint64, (2,)).tolist() == [1, 2 ** 63] and tries == 0 and type(tries) is int
    assert col.seeds_and_tries(None, None, 700000000, 0)[1] == 700000000
    assert is_array(col.seeds_and_tries([], None, 1, 0)[0], np.uint64, (0,)).size == 0
    # samples decide the tries; neither seeds nor maximum_tries is looked at
    samples = np.zeros((2, 5, 7), np.int32)
    assert col.seeds_and_tries("anything", samples, -1, 2) == ("anything", 5)
    assert col.seeds_and_tries(None, np.zeros((0, 0, 7), np.int32), 10 ** 12, 0) == (None, 0)
    for seeds, tries, n in (([1], 5, 2), ([1, 2, 3], 5, 2), (None, -1, 2), (None, 700000001, 2)):
        with pytest.raises(ValueError):
            col.seeds_and_tries(seeds, None, tries, n)


def test_fit_dicts():
    off = np.array([0, 3, 3, 8], np.int64)
    ok, n = np.array([1, 0, 0], np.int32), np.array([2, 0, 4], np.int32)
    bt, br, ran = np.array([4, -1, 0], np.int32), np.array([1, -1, 2], np.int32), np.array([9, 0, 9], np.int32)
    F, Pm, pct = np.arange(27.0).reshape(3, 9), np.arange(36.0).reshape(3, 12), np.array([0.5, 0.0, 0.25])
    idx = np.arange(100, 108, dtype=np.int32)
    rows = col.fit_dicts(off, ok, F, Pm, pct, idx, n, bt, br, ran)
    assert len(rows) == 3 and [set(r) for r in rows] == [{'success', 'essential', 'camera', 'inlier_percent', 'inlier_idx',
                                                          'best_try', 'best_root', 'tries_run'}] * 3
    a, b, c = rows
    assert a['success'] is True and b['success'] is False and c['success'] is False
    assert a['essential'].shape == (3, 3) and a['camera'].shape == (3, 4) and a['essential'].tolist() == F[0].reshape(3, 3).tolist()
    assert b['essential'] is None and b['camera'] is None                            # best_try -1: no model kept
    assert c['essential'] is not None and c['camera'][2, 3] == 35.0                  # a model that did not succeed is still returned
    assert [r['inlier_idx'].tolist() for r in rows] == [[100, 101], [], [103, 104, 105, 106]]
    assert [type(r[k]) for r in rows for k in ('best_try', 'best_root', 'tries_run')] == [int] * 9
    assert [type(r['inlier_percent']) for r in rows] == [float] * 3 and a['inlier_percent'] == 0.5
    # copies: the call's buffers may be reused
    F[0, 0], Pm[0, 0], idx[0] = -1, -1, -1
    assert a['essential'][0, 0] == 0.0 and a['camera'][0, 0] == 0.0 and a['inlier_idx'][0] == 100
    assert col.fit_dicts(np.array([0], np.int64), *[np.zeros(0)] * 9) == []
