"""GPU parity of the many-pairs cascade (cascade_batch.hip): every pair's slice of the concatenated result equals
oracle.nn_cascading_hash(database set, query set) -- candidate counts, distances and indices with array_equal, no
tolerance -- and, where stated, device.cascade of that pair alone, bit for bit."""
import functools

import numpy as np
import pytest

from tests import cascade_batch_cases as cb

pytestmark = pytest.mark.gpu

NONE_DIST = np.float32(2147483648.0)
NONE_IDX = np.uint64(2 ** 64 - 1)


def oracle_pairs(x, seg, d, pairs, g):
    """{(query set, database set): (idx, dist, ncand)} of the distinct pairs, from the CPU oracle."""
    from oracle import oracle as o
    n, _, m = d.shape
    return {(a, b): o.nn_cascading_hash(x[seg[b]:seg[b + 1]], x[seg[a]:seg[a + 1]], m, n, g, d)[:3]
            for a, b in sorted(set(map(tuple, pairs)))}


def device_batch(x, seg, d, pairs, g):
    """device.cascade_batch on numpy inputs -> numpy (idx uint64, dist, ncand, out_off)."""
    import torch
    from spectavi_amd import device
    idx, dist, out_off, ncand = device.cascade_batch(torch.from_numpy(x).cuda(), seg, pairs, torch.from_numpy(d).cuda(), g=g,
                                                     want_ncand=True)
    return idx.cpu().numpy().view(np.uint64), dist.cpu().numpy(), ncand.cpu().numpy(), out_off


def host_batch(x, seg, d, pairs, g):
    """feature.nn_cascading_hash_batch, concatenated again -> the same four."""
    from spectavi_amd import feature
    res = feature.nn_cascading_hash_batch([x[a:b] for a, b in zip(seg[:-1], seg[1:])], d, pairs, g=g, return_ncand=True)
    assert len(res) == len(pairs)
    cat = lambda k, shape, t: np.concatenate([r[k] for r in res]) if res else np.zeros(shape, t)
    out_off = np.concatenate([[0], np.cumsum([len(r[0]) for r in res])]).astype(np.int64)
    return cat(0, (0, 2), np.uint64), cat(1, (0, 2), np.float32), cat(2, (0,), np.int32), out_off


def assert_pairs_equal(got, want, seg, pairs, what):
    idx, dist, ncand, out_off = got
    assert np.array_equal(out_off, np.concatenate([[0], np.cumsum([seg[a + 1] - seg[a] for a, _ in pairs])]))
    assert len(idx) == len(dist) == len(ncand) == out_off[-1]
    for p, (a, b) in enumerate(pairs):
        lo, hi = out_off[p], out_off[p + 1]
        oidx, odist, oncand = want[(a, b)]
        assert np.array_equal(ncand[lo:hi], oncand), (what, "ncand", p, a, b)
        assert np.array_equal(dist[lo:hi], odist), (what, "dist", p, a, b)
        assert np.array_equal(idx[lo:hi], oidx), (what, "idx", p, a, b)


def check_collection(x, seg, d, pairs, g, forms=("device",)):
    want = oracle_pairs(x, seg, d, pairs, g)
    got = {}
    for form in forms:
        got[form] = (device_batch if form == "device" else host_batch)(x, seg, d, pairs, g)
        assert_pairs_equal(got[form], want, seg, pairs, form)
    return got[forms[0]], want


@functools.lru_cache(maxsize=None)
def nine():
    """The nine-set collection, its oracle results and the device form's, computed once."""
    x, seg, d = cb.collection(cb.NINE, *cb.NINE_SHAPE)
    got, want = check_collection(x, seg, d, cb.ALL81, cb.NINE_SHAPE[3], forms=("device", "host"))
    for a in (x, seg, d) + got:
        a.setflags(write=False)
    return x, seg, d, got, want


def test_nine_sets_all_ordered_pairs_match_the_oracle_in_both_forms():
    nine()


def test_nine_sets_every_pair_is_the_single_call_bit_for_bit():
    import torch
    from spectavi_amd import device
    x, seg, d, (idx, dist, ncand, out_off), _ = nine()
    dx, dd = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(d.copy()).cuda()
    for p, (a, b) in enumerate(cb.ALL81):
        sidx, sdist, sncand = device.cascade(dx[seg[b]:seg[b + 1]], dx[seg[a]:seg[a + 1]], dd, g=cb.NINE_SHAPE[3],
                                             want_ncand=True)
        lo, hi = out_off[p], out_off[p + 1]
        assert np.array_equal(ncand[lo:hi], sncand.cpu().numpy()), (a, b)
        assert np.array_equal(dist[lo:hi].view(np.uint32), sdist.cpu().numpy().view(np.uint32)), (a, b)
        assert np.array_equal(idx[lo:hi], sidx.cpu().numpy().view(np.uint64)), (a, b)


def test_nine_sets_empty_database_and_self_pair():
    x, seg, d, (idx, dist, ncand, out_off), _ = nine()
    for a in range(9):   # database set 0 is empty: sentinels, no candidate
        p = cb.ALL81.index((a, 0))
        lo, hi = out_off[p], out_off[p + 1]
        assert hi - lo == cb.NINE[a]
        assert (idx[lo:hi] == NONE_IDX).all() and (dist[lo:hi] == NONE_DIST).all() and (ncand[lo:hi] == 0).all()
    for b in range(9):   # query set 0 is empty: it owns no rows
        p = cb.ALL81.index((0, b))
        assert out_off[p] == out_off[p + 1]
    # (8, 8): every row finds itself first, at distance 0 (a row whose uint8 image occurs twice in the set, like the
    # all-zero rows, may find its twin's lower number: the smallest (dist, idx))
    p = cb.ALL81.index((8, 8))
    lo, hi = out_off[p], out_off[p + 1]
    assert (dist[lo:hi, 0] == 0).all() and (ncand[lo:hi] >= 1).all()
    _, first, inverse, counts = np.unique(cb.image(x[seg[8]:seg[9]]), axis=0, return_index=True, return_inverse=True,
                                          return_counts=True)
    once = counts[inverse.reshape(-1)] == 1
    assert once.sum() > 900
    assert np.array_equal(idx[lo:hi, 0][once], np.arange(hi - lo, dtype=np.uint64)[once])
    assert (idx[lo:hi, 0] <= np.arange(hi - lo, dtype=np.uint64)).all()


@pytest.mark.parametrize("shape", cb.EDGES, ids=lambda s: "-".join(map(str, s)))
def test_parameter_edges(shape):
    dim, m, n, g = shape
    x, seg, d = cb.collection(cb.FEW_ROWS, dim, m, n, g)
    check_collection(x, seg, d, cb.FEW, g, forms=("device", "host") if shape == cb.EDGES[1] else ("device",))


def test_a_bucket_longer_than_the_lds_list():
    """1500 copies of one row are one bucket per table, three times the 512 entries of the probe's LDS list: the
    probe takes them 64 at a time.  The same set is also a query set against a normal one."""
    dim, m, n, g = cb.NINE_SHAPE
    x, seg, d = cb.collection([300, 1500, 257], dim, m, n, g)
    x[seg[1]:seg[2]] = x[seg[1]]
    hit = np.arange(10) * 25 + 3
    x[seg[2] + hit] = x[seg[1]]
    pairs = [(2, 1), (1, 0)]
    (idx, dist, ncand, out_off), _ = check_collection(x, seg, d, pairs, g)
    assert np.array_equal(idx[hit], np.tile(np.array([0, 1], np.uint64), (10, 1)))
    assert (dist[hit] == 0).all() and (ncand[hit] == 3000).all()
    others = np.setdiff1d(np.arange(257), hit)
    assert set(np.unique(ncand[others])) <= {0, 1500, 3000}   # all of the bucket or none of it, per table


def test_set_isolation():
    """Two database sets next to each other in the packed table, identical but for the planted near-copies of the
    queries, which only the first holds: candidates come from the pair's own database set alone."""
    dim, m, n, g = cb.NINE_SHAPE
    rng = np.random.default_rng(11)
    x, seg, d = cb.collection([400, 400, 200], dim, m, n, g)
    x[seg[1]:seg[2]] = x[seg[0]:seg[1]]
    planted = rng.choice(400, 200, replace=False)
    x[seg[0] + planted] = np.clip(x[seg[2]:seg[3]] + rng.integers(-1, 2, (200, dim)), -128, 127)
    pairs = [(2, 0), (2, 1)]
    (idx, dist, ncand, out_off), want = check_collection(x, seg, d, pairs, g)
    with_copies, without = dist[out_off[0]:out_off[1]], dist[out_off[1]:out_off[2]]
    found = idx[out_off[0]:out_off[1], 0] == planted.astype(np.uint64)
    assert found.sum() > 100, "the planted neighbours are found in the set that holds them"
    assert (without[found, 0] > with_copies[found, 0]).all(), "... and nothing as near in the set that does not"
    assert np.array_equal(with_copies != without, want[(2, 0)][1] != want[(2, 1)][1])


@pytest.mark.parametrize("pairs", [cb.BOOK, cb.DESCENDING], ids=["repeats", "descending"])
def test_pair_bookkeeping(pairs):
    x, seg, d = cb.collection(cb.BOOK_ROWS, *cb.NINE_SHAPE)
    (idx, dist, ncand, out_off), _ = check_collection(x, seg, d, pairs, cb.NINE_SHAPE[3], forms=("device", "host"))
    for p, q in ((p, q) for p in range(len(pairs)) for q in range(p)):
        if pairs[p] == pairs[q]:   # a repeated pair repeats its rows
            assert np.array_equal(idx[out_off[p]:out_off[p + 1]], idx[out_off[q]:out_off[q + 1]])


def test_ratio_test_applies_to_the_concatenated_output():
    import torch
    from spectavi_amd import device
    x, seg, d = cb.collection(cb.BOOK_ROWS, *cb.NINE_SHAPE)
    idx, dist, out_off = device.cascade_batch(torch.from_numpy(x).cuda(), seg, cb.BOOK, torch.from_numpy(d).cuda(), g=2)
    matches, count = device.ratio_test(idx, dist, 1.5)
    k = int(count.item())
    hi, hd = idx.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        keep = (hi[:, 0] >= 0) & (hd[:, 1] / hd[:, 0] >= 1.5)
    assert k == keep.sum() and 0 < k < len(hi)
    assert np.array_equal(matches[:k].cpu().numpy(), np.stack([np.nonzero(keep)[0], hi[keep, 0]], 1))


def test_a_non_default_stream_gives_the_default_stream_result():
    import torch
    from spectavi_amd import device
    dim, m, n, g = cb.EDGES[3]
    x, seg, d = cb.collection(cb.FEW_ROWS, dim, m, n, g)
    want, _ = check_collection(x, seg, d, cb.FEW, g)   # on the default stream
    dx, dd = torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side != torch.cuda.default_stream()
    with torch.cuda.stream(side):
        idx, dist, out_off, ncand = device.cascade_batch(dx, seg, cb.FEW, dd, g=g, workspace=device.Workspace(), want_ncand=True)
    side.synchronize()
    got = (idx.cpu().numpy().view(np.uint64), dist.cpu().numpy(), ncand.cpu().numpy(), out_off)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_a_workspace_reused_by_a_smaller_collection():
    """Large then small on one device.Workspace: the second call finds the order, ranks and segment sums of the first
    in its workspace, which no call zeroes, and still matches its oracle."""
    import torch
    from spectavi_amd import device
    ws = device.Workspace()
    first = None
    for rows, pairs in ((cb.NINE, [(8, 7), (7, 8), (6, 8), (8, 8)]), (cb.FEW_ROWS, cb.FEW)):
        x, seg, d = cb.collection(rows, *cb.NINE_SHAPE)
        idx, dist, out_off, ncand = device.cascade_batch(torch.from_numpy(x).cuda(), seg, pairs, torch.from_numpy(d).cuda(),
                                                         g=cb.NINE_SHAPE[3], workspace=ws, want_ncand=True)
        got = (idx.cpu().numpy().view(np.uint64), dist.cpu().numpy(), ncand.cpu().numpy(), out_off)
        assert_pairs_equal(got, oracle_pairs(x, seg, d, pairs, cb.NINE_SHAPE[3]), seg, pairs, str(rows))
        buf = ws.get(0, idx.device)
        first = first or (buf.data_ptr(), buf.numel())
    assert (buf.data_ptr(), buf.numel()) == first, "the smaller call ran on the larger call's buffer"


def test_launch_count_does_not_depend_on_the_number_of_pairs():
    import torch
    from spectavi_amd import device
    x, seg, d = cb.collection(cb.NINE, *cb.NINE_SHAPE)
    dx, dd = torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda()
    names = ("cascade_batch_project", "cascade_batch_buckets", "cascade_batch_probe")
    counts = []
    device.profile_enable(True)
    try:
        for pairs in ([(8, 7)], cb.ALL81):
            device.profile_reset()
            device.cascade_batch(dx, seg, pairs, dd, g=2)
            torch.cuda.synchronize()
            counts.append([device.profile_read(k)[0] for k in names])
    finally:
        device.profile_enable(False)
        device.profile_reset()
    assert counts[0] == counts[1] == [1, 1, 1]
