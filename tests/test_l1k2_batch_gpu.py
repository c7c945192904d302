"""GPU: the many-pairs L1 2-NN (spv_l1k2_batch_device, spv_nn_bruteforcel1k2_batch) is bit for bit
oracle.nn_bruteforcel1k2(database set, query set) for every pair, at the smallest shapes at which the kernel
can go wrong: empty and one-row sets, ragged tiles and query blocks, every shipped instantiation, a database set
past the 16-bit slice limit with ties across slice boundaries, items of one, 15, 47, 64 and 1024 LDS tiles, a sliced
lone pair and an unsliced collection."""
import numpy as np
import pytest

from tests import l1k2_batch_cases as bc
from tests.l1k2_batch_child import case_tables, check_pairs, longest_item, run_device, sets_u8

pytestmark = pytest.mark.gpu

NONE = np.iinfo(np.uint64).max


@pytest.fixture(scope="module")
def nine128():
    return sets_u8(11, bc.NINE, 128)


def test_nine_sets_all_pairs_device_form(oracle, nine128):
    idx, dist, off = run_device(nine128, bc.ALL81)
    check_pairs(oracle, nine128, bc.ALL81, idx, dist, off)
    # what the shapes are there for: an empty database gives two sentinels, a one-row database one
    p0, p1 = bc.ALL81.index((8, 0)), bc.ALL81.index((8, 1))
    assert (idx[off[p0]:off[p0 + 1]] == NONE).all() and (dist[off[p0]:off[p0 + 1]] == 2 ** 31 - 1).all()
    assert (idx[off[p1]:off[p1 + 1], 0] == 0).all() and (idx[off[p1]:off[p1 + 1], 1] == NONE).all()
    ps = bc.ALL81.index((8, 8))   # a set against itself: every row finds itself first
    assert np.array_equal(idx[off[ps]:off[ps + 1], 0], np.arange(1000, dtype=np.uint64)) and (dist[off[ps]:off[ps + 1], 0] == 0).all()


def test_nine_sets_all_pairs_host_form(oracle, nine128):
    from spectavi_amd import feature
    res = feature.nn_bruteforcel1k2_batch(nine128, bc.ALL81)
    assert len(res) == 81
    off = np.concatenate([[0], np.cumsum([len(i) for i, _ in res])])
    idx = np.concatenate([i for i, _ in res])
    dist = np.concatenate([d for _, d in res])
    assert idx.dtype == np.uint64 and dist.dtype == np.int32
    check_pairs(oracle, nine128, bc.ALL81, idx, dist, off)


@pytest.mark.parametrize("case", [c for c in bc.Q_CASES if c[0] not in ("nine-128", "maxslice-16")], ids=lambda c: c[0])
def test_every_instantiation(oracle, case):
    """Each (row width, queries per lane) that ships, on one-tile items (nine-*, mid-*, long-*) and, at the planner's
    largest q, on items of 64 and 15 tiles (tiles-*: the double buffer, tile-local bases up to 4032, a ragged last
    tile, every staging width); tests/test_l1k2_batch_plan.py asserts which case gets which."""
    name, rows, pairs, dim, q, xrows = case
    assert longest_item(rows, pairs, dim) == (q, xrows)
    tables = case_tables(case)
    idx, dist, off = run_device(tables, pairs)
    check_pairs(oracle, tables, pairs, idx, dist, off)


@pytest.mark.parametrize("q", [1, 2])
def test_many_tile_items_at_the_smaller_q(q):
    """The tiles-* cases under SPECTAVI_L1K2_Q, in a child process (tests/l1k2_batch_child.py says why)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(root, "tests", "l1k2_batch_child.py"), str(q)]
    r = subprocess.run(cmd, cwd=root, env=dict(os.environ, SPECTAVI_L1K2_Q=str(q)), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok q=%d" % q), r.stdout[-2000:] + r.stderr[-2000:]


@pytest.fixture(scope="module")
def max_slice():
    case = next(c for c in bc.Q_CASES if c[0] == "maxslice-16")
    assert longest_item(*case[1:4]) == (case[4], 65536)
    return case, sets_u8(17, case[1], case[3])


def test_an_item_of_65536_rows(oracle, max_slice):
    """One item holds database rows 0..65535, the whole range of the 16-bit local index, the next one the rest.  Rows
    65535, 65536 and 65537 are the only exact copies of query 1: the answer is the last row of the first item and the
    first row of the second."""
    (name, rows, pairs, dim, q, xrows), (db, qs) = max_slice
    db = db.copy()
    db[[65535, 65536, 65537]] = qs[1]
    idx, dist, off = run_device([db, qs], pairs)
    assert idx[1].tolist() == [65535, 65536] and dist[1].tolist() == [0, 0]
    check_pairs(oracle, [db, qs], pairs, idx, dist, off)


def test_identical_rows_across_the_two_items(max_slice):
    """Every database row the same: 70000 distances tie, 65536 of them inside one item, so rows (0, 1) must win over
    every key of the second item and over every later tile of the first."""
    (name, rows, pairs, dim, q, xrows), (db, qs) = max_slice
    same = np.repeat(db[:1], 70000, axis=0)
    idx, dist, off = run_device([same, qs], pairs)
    assert (idx[:, 0] == 0).all() and (idx[:, 1] == 1).all()
    want = np.tile(np.abs(qs.astype(np.int32) - same[0].astype(np.int32)).sum(1), len(pairs))
    assert np.array_equal(dist[:, 0], want) and np.array_equal(dist[:, 1], want)


@pytest.fixture(scope="module")
def long_pair():
    return sets_u8(12, [70000, 257], 128)


def test_identical_database_rows_across_slices(long_pair):
    """Every database row the same: all 70000 distances tie, so the answer is rows (0, 1) for every query.  This
    lone pair is cut into 1094 one-tile items: it checks the item's base row (x_local0) and the merge of 1094 key
    pairs per out row; test_identical_rows_across_the_two_items has the long items."""
    db = np.repeat(long_pair[0][:1], 70000, axis=0)
    idx, dist, off = run_device([db, long_pair[1]], [(1, 0)])
    assert (idx[:, 0] == 0).all() and (idx[:, 1] == 1).all()
    want = np.abs(long_pair[1].astype(np.int32) - db[0].astype(np.int32)).sum(1)
    assert np.array_equal(dist[:, 0], want) and np.array_equal(dist[:, 1], want)


def test_duplicates_at_the_16_bit_boundary(oracle, long_pair):
    """Rows 65535, 65536 and 65537 are the only exact copies of query 5, in three of the 1094 one-tile items this lone
    pair is cut into: the two smallest set-local indices win, on either side of 2^16 (test_an_item_of_65536_rows puts
    that boundary between two items)."""
    db, qs = long_pair[0].copy(), long_pair[1]
    db[[65535, 65536, 65537]] = qs[5]
    idx, dist, off = run_device([db, qs], [(1, 0)])
    assert idx[5].tolist() == [65535, 65536] and dist[5].tolist() == [0, 0]
    check_pairs(oracle, [db, qs], [(1, 0)], idx, dist, off)


def test_lone_pair_sliced_by_the_planner(oracle):
    from spectavi_amd import device
    rows, pairs = [20000, 600], [(1, 0)]
    assert device.l1k2_batch_plan(bc.seg_of(rows), pairs, 128)["max_slices"] > 1
    tables = sets_u8(13, rows, 128)
    idx, dist, off = run_device(tables, pairs)
    check_pairs(oracle, tables, pairs, idx, dist, off)


def test_unsliced_collection_against_the_single_pair_kernels(oracle):
    """40 sets of 3000 rows, all 780 pairs i < j: each pair against device.l1k2 (GPU against GPU), three of them
    against the oracle."""
    import torch
    from spectavi_amd import device
    rows = [3000] * 40
    pairs = [(j, i) for i in range(40) for j in range(i + 1, 40)]
    assert device.l1k2_batch_plan(bc.seg_of(rows), pairs, 128)["max_slices"] == 1
    tables = sets_u8(14, rows, 128)
    desc = torch.from_numpy(np.concatenate(tables)).cuda()
    idx, dist, off = device.l1k2_batch(desc, bc.seg_of(rows), pairs)
    differs = torch.zeros(len(pairs), dtype=torch.bool, device="cuda")   # compared on the device: one wait for 780 pairs
    for p, (a, b) in enumerate(pairs):
        si, sd = device.l1k2(desc[3000 * b:3000 * (b + 1)], desc[3000 * a:3000 * (a + 1)])
        differs[p] = (si != idx[off[p]:off[p + 1]]).any() | (sd != dist[off[p]:off[p + 1]]).any()
    assert not bool(differs.any()), differs.nonzero().flatten().tolist()
    check_pairs(oracle, tables, pairs, idx.cpu().numpy().view(np.uint64), dist.cpu().numpy(), off, which=(0, 391, 779))


@pytest.mark.parametrize("name", ["l1k2_ties_300x500_64.npz", "l1k2_dups_257x5_128.npz"])
def test_goldens_as_two_set_collections(golden, name):
    g = golden(name)
    idx, dist, off = run_device([g["x"], g["y"]], [(1, 0)])
    assert np.array_equal(idx, g["idx"]) and np.array_equal(dist, g["dist"])


def test_repeated_pairs_and_pair_order(nine128):
    pairs = [(8, 7), (6, 8), (8, 7), (7, 7), (2, 8), (8, 7)]
    idx, dist, off = run_device(nine128, pairs)
    first = slice(off[0], off[1])
    for p in (2, 5):
        assert np.array_equal(idx[off[p]:off[p + 1]], idx[first]) and np.array_equal(dist[off[p]:off[p + 1]], dist[first])
    order = [4, 0, 5, 3, 1, 2]
    idx2, dist2, off2 = run_device(nine128, [pairs[k] for k in order])
    for at, k in enumerate(order):
        assert np.array_equal(idx2[off2[at]:off2[at + 1]], idx[off[k]:off[k + 1]])
        assert np.array_equal(dist2[off2[at]:off2[at + 1]], dist[off[k]:off[k + 1]])


def test_exact_size_buffers_and_short_workspace(nine128):
    """idx, dist and the workspace at exactly their sizes, each with a canary region behind it that must stay
    intact; a workspace one byte short is refused before anything is launched."""
    import ctypes as ct
    import torch
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    tables = sets_u8(15, bc.NINE, 176)      # padded to 192: every piece of the workspace is in use
    pairs = np.array(bc.FEW, np.int32)
    seg = bc.seg_of(bc.NINE)
    desc = torch.from_numpy(np.concatenate(tables)).cuda()
    out = (ct.c_longlong * 6)()
    assert clib.spv_l1k2_batch_plan(seg.ctypes.data, 9, 176, pairs.ctypes.data, len(pairs), out, None, 0) == 0
    out_rows, wsb = int(out[3]), int(out[5])
    TAIL, FILL = 4096, 0xA5
    sizes = dict(idx=out_rows * 16, dist=out_rows * 8, ws=wsb)

    def buffers():
        return {k: torch.full((n + TAIL,), FILL, dtype=torch.uint8, device="cuda") for k, n in sizes.items()}

    def call(b, ws_bytes):
        st = clib.spv_l1k2_batch_device(desc.data_ptr(), seg.ctypes.data, 9, 176, pairs.ctypes.data, len(pairs),
                                        b["idx"].data_ptr(), b["dist"].data_ptr(), b["ws"].data_ptr(), ws_bytes,
                                        ct.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return st

    b = buffers()
    assert call(b, wsb) == 0
    for k, n in sizes.items():
        assert bool((b[k][n:] == FILL).all()), "the call wrote past the end of " + k
    idx = b["idx"][:sizes["idx"]].cpu().numpy().view(np.uint64).reshape(-1, 2)
    dist = b["dist"][:sizes["dist"]].cpu().numpy().view(np.int32).reshape(-1, 2)
    want = run_device(tables, bc.FEW)
    assert np.array_equal(idx, want[0]) and np.array_equal(dist, want[1])
    b = buffers()
    assert call(b, wsb - 1) == SPV_ERR_INVALID
    assert all(bool((t == FILL).all()) for t in b.values()), "a refused call has launched something"


def test_non_default_stream(nine128):
    import torch
    want = run_device(nine128, bc.FEW)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = run_device(nine128, bc.FEW)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_feature_form_equals_single_pair_calls():
    from spectavi_amd import feature
    tables = sets_u8(16, [300, 1, 700], 128)
    res = feature.nn_bruteforcel1k2_batch(tables)          # (1, 0), (2, 0), (2, 1)
    assert len(res) == 3
    for (q, d), (idx, dist) in zip([(1, 0), (2, 0), (2, 1)], res):
        si, sd = feature.nn_bruteforcel1k2(tables[d], tables[q])
        assert np.array_equal(idx, si) and np.array_equal(dist, sd)


def test_one_main_launch_per_call(nine128):
    from spectavi_amd import device
    device.profile_reset()
    device.profile_enable(True)
    try:
        run_device(nine128, bc.FEW)
        run_device(nine128, bc.ALL81)
        assert device.profile_read("l1k2_batch")[0] == 2
        assert device.profile_read("l1k2_batch_merge")[0] == 2
    finally:
        device.profile_enable(False)
        device.profile_reset()
