"""GPU parity of the many-sets RANSAC (spv_ransac_fit_batch / _device) and of the batch gather
(spv_gather_match_coords_batch_device).  Every fit is compared with `mvg.ransac_fit(samples=...)` on that set
alone -- unchanged code -- bit for bit on everything but tries_run, which stays within its stated bounds; the
gather with the per-pair loop over l1k2 / ratio_test / match_coordinates."""
import ctypes as ct

import numpy as np
import pytest

from tests import ransac_batch_cases as rc

pytestmark = pytest.mark.gpu


def _kw(req, find_best):
    return dict(required_percent_inliers=req, reprojection_error_allowed=rc.THRESHOLD,
                find_best_even_in_failure=find_best, singular_value_ratio_allowed=3e-2)


def _singles(x0s, x1s, smp, **kw):
    from spectavi_amd import mvg
    return [mvg.ransac_fit(a, b, samples=s, **kw) if len(a) >= 10 else None for a, b, s in zip(x0s, x1s, smp)]


def _compare(rows, singles, ntries, what):
    assert len(rows) == len(singles)
    for p, (row, one) in enumerate(zip(rows, singles)):
        if one is None:
            rc.assert_skipped(row, (what, p))
        else:
            rc.assert_same_fit(row, one, ntries, (what, p))


def _device_batch(x0s, x1s, smp, **kw):
    import torch
    from spectavi_amd import device as spv
    cat0 = torch.from_numpy(np.concatenate(x0s)).cuda()
    cat1 = torch.from_numpy(np.concatenate(x1s)).cuda()
    return spv.ransac_fit_batch(cat0, cat1, rc.offsets(x0s), samples=np.stack(smp), **kw)


@pytest.fixture(scope="module")
def edge():
    return rc.collection(rc.EDGE_SIZES, rc.EDGE_OUTLIERS, 60, 100)


@pytest.mark.parametrize("req,find_best", rc.SETTINGS)
def test_edge_sizes_equal_the_single_fits(edge, req, find_best):
    """0, 9 (skipped), 10, 255 / 256 / 257 and 2 500 rows in one collection, each set with its own outlier share
    and subsets: success, best-on-failure and no model at all."""
    x0s, x1s, smp, inl = edge
    kw = _kw(req, find_best)
    singles = _singles(x0s, x1s, smp, **kw)
    rows = _device_batch(x0s, x1s, smp, **kw)
    _compare(rows, singles, 60, (req, find_best))
    for p, row in enumerate(rows):
        if len(x0s[p]) < 10:
            continue
        if req < 0.6 and len(x0s[p]) > 10 and row['success']:  # above the share in a noise-free scene: the planted model
            assert np.array_equal(row['inlier_idx'], inl[p]), p
        elif req > 0.9:  # no set is that clean
            assert not row['success'] and (find_best or row['best_try'] == -1), p
    # the host-pointer entry: the same rows
    from spectavi_amd import mvg
    host = mvg.ransac_fit_batch(x0s, x1s, samples=smp, **kw)
    _compare(host, singles, 60, ("host", req, find_best))


@pytest.fixture(scope="module")
def mixed():
    """Easy sets that end in the first round, the 300-point 60 %-outlier scene of
    test_ransac_fit_late_success_crosses_batches (winner beyond try 256) and a pure-outlier set that runs all
    6 000 tries: the sets leave in different rounds."""
    from spectavi_amd import mvg
    from tests import mvg_checks as mc
    x0s, x1s, smp, _ = rc.collection([200, 150, 400], [0.2, 0.1, 0.25], 6000, 300)
    x0, x1, _, out_idx = mc.two_view_scene(np.random.default_rng(99), npt=300, outlier_fraction=0.6)
    x0s.insert(1, x0)
    x1s.insert(1, x1)
    smp.insert(1, mvg.ransac_sample(77, 300, 6000))
    a, b, _ = rc.scene(555, 120, 1.0)
    x0s.append(a)
    x1s.append(b)
    smp.append(mvg.ransac_sample(556, 120, 6000))
    return x0s, x1s, smp, np.setdiff1d(np.arange(300), out_idx)


def test_sets_that_leave_in_different_rounds(mixed):
    x0s, x1s, smp, late_inliers = mixed
    kw = _kw(0.35, True)
    singles = _singles(x0s, x1s, smp, **kw)
    rows = _device_batch(x0s, x1s, smp, **kw)
    _compare(rows, singles, 6000, "mixed")
    assert [r['success'] for r in rows] == [True, True, True, True, False]
    assert all(rows[p]['tries_run'] <= 256 for p in (0, 2, 3))       # easy: the first round
    assert rows[1]['best_try'] >= 256 and rows[1]['tries_run'] > 256  # late: still the first success in try order
    assert np.array_equal(rows[1]['inlier_idx'], late_inliers)
    assert rows[4]['tries_run'] == 6000  # pure outliers: every try


def test_candidates_cut_over_several_items_and_repeated_sets():
    """Few row blocks for the chip: the plan cuts every set's candidates over several work items (asserted from
    the plan).  The same set listed several times: identical rows with the same subsets, its own single fit with
    different ones."""
    import torch
    from spectavi_amd import device as spv
    x0s, x1s, smp, _ = rc.collection([300, 700, 64], [0.25, 0.3, 0.1], 150, 400)
    x0s += [x0s[0], x0s[0], x0s[1]]
    x1s += [x1s[0], x1s[0], x1s[1]]
    smp += [smp[0], rc.subsets(9001, 300, 150), smp[1]]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan, items = spv.ransac_fit_batch_plan(rc.offsets(x0s), 150, cus, want_items=True)
    assert plan['items'] > plan['row_blocks'] and len({tuple(i[3:]) for i in items if i[0] == 0}) > 1
    kw = _kw(0.55, True)
    singles = _singles(x0s, x1s, smp, **kw)
    rows = _device_batch(x0s, x1s, smp, **kw)
    _compare(rows, singles, 150, "cut")
    for a, b in ((0, 3), (1, 5)):
        rc.assert_same_fit(rows[a], rows[b], 150, ("repeat", a, b))
        assert rows[a]['tries_run'] == rows[b]['tries_run']


def test_seeds_path_equals_the_sampled_subsets_and_the_single_seeded_fit():
    import torch
    from spectavi_amd import device as spv
    from spectavi_amd import mvg
    sizes, ntries = [120, 9, 333, 1000], 200
    x0s, x1s, _, _ = rc.collection(sizes, [0.3, 0.0, 0.2, 0.35], 1, 500)
    seeds = [41, 42, 43, 2 ** 40 + 5]
    kw = _kw(0.6, True)
    rows = mvg.ransac_fit_batch(x0s, x1s, maximum_tries=ntries, seeds=seeds, **kw)
    smp = [mvg.ransac_sample(s, n, ntries) if n >= 10 else np.zeros((ntries, 7), np.int32) for s, n in zip(seeds, sizes)]
    _compare(rows, _singles(x0s, x1s, smp, **kw), ntries, "seeds vs samples")
    seeded = [mvg.ransac_fit(a, b, maximum_tries=ntries, seed=s, **kw) if len(a) >= 10 else None
              for a, b, s in zip(x0s, x1s, seeds)]
    _compare(rows, seeded, ntries, "seeds vs seeded single fit")
    dev = spv.ransac_fit_batch(torch.from_numpy(np.concatenate(x0s)).cuda(), torch.from_numpy(np.concatenate(x1s)).cuda(),
                               rc.offsets(x0s), maximum_tries=ntries, seeds=seeds, **kw)
    _compare(dev, seeded, ntries, "device entry, seeds")


def test_noise_free_sets_against_the_oracle_and_single_path_afterwards(oracle):
    """The 200-point and 64-point scenes of test_ransac_fit_matches_oracle_given_the_same_subsets, in one
    collection, against the oracle by that test's rule; then one single fit in the same process."""
    from spectavi_amd import mvg
    from tests import mvg_checks as mc
    from tests.test_ransac_fit_gpu import _same_model
    x0s, x1s, smp, inl = [], [], [], []
    for npt, outliers in ((200, 0.25), (64, 0.1)):
        x0, x1, _, out_idx = mc.two_view_scene(np.random.default_rng(npt), npt=npt, outlier_fraction=outliers)
        x0s.append(x0)
        x1s.append(x1)
        smp.append(mvg.ransac_sample(1234 + npt, npt, 150))
        inl.append(np.setdiff1d(np.arange(npt), out_idx))
    for req, find_best in ((0.65, False), (0.995, True), (0.995, False)):
        kw = _kw(req, find_best)
        rows = mvg.ransac_fit_batch(x0s, x1s, samples=smp, **kw)
        for p, row in enumerate(rows):
            _same_model(row, oracle.ransac_fit(x0s[p], x1s[p], smp[p], **kw))
            if req < 0.7:
                assert row['success'] and np.array_equal(row['inlier_idx'], inl[p])
    kw = _kw(0.65, False)
    _same_model(mvg.ransac_fit(x0s[0], x1s[0], samples=smp[0], **kw), oracle.ransac_fit(x0s[0], x1s[0], smp[0], **kw))


def test_inlier_mask_is_the_inlier_lists_and_every_byte_is_written(edge):
    import torch
    from spectavi_amd._lib import clib, check
    x0s, x1s, smp, _ = edge
    off = rc.offsets(x0s)
    npairs, total = len(x0s), int(off[-1])
    cat0 = torch.from_numpy(np.concatenate(x0s)).cuda()
    cat1 = torch.from_numpy(np.concatenate(x1s)).cuda()
    samples = np.ascontiguousarray(np.stack(smp), dtype=np.int32)
    for req, find_best in ((0.55, True), (0.995, False)):  # models for all running sets; no model anywhere
        mask = torch.full((total,), 0xAB, dtype=torch.uint8, device="cuda")
        ok, n = np.zeros(npairs, np.int32), np.zeros(npairs, np.int32)
        F, P, pct, idx = np.zeros((npairs, 9)), np.zeros((npairs, 12)), np.zeros(npairs), np.zeros(total, np.int32)
        stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(clib.spv_ransac_fit_batch_device(cat0.data_ptr(), cat1.data_ptr(), off.ctypes.data, npairs, req, rc.THRESHOLD,
                                               60, int(find_best), 3e-2, samples.ctypes.data, None, ok.ctypes.data,
                                               F.ctypes.data, P.ctypes.data, pct.ctypes.data, idx.ctypes.data,
                                               n.ctypes.data, None, None, None, mask.data_ptr(), stream))
        torch.cuda.synchronize()
        got = mask.cpu().numpy()
        want = np.zeros(total, np.uint8)
        for p in range(npairs):
            want[off[p] + idx[off[p]:off[p] + n[p]]] = 1
        assert np.array_equal(got, want)
        assert (n.sum() > 0) == find_best and np.all(n[[0, 1]] == 0)
    # the Python form returns the same tensor
    from spectavi_amd import device as spv
    rows, m = spv.ransac_fit_batch(cat0, cat1, off, samples=samples, want_mask=True, **_kw(0.55, True))
    for p, row in enumerate(rows):
        assert np.array_equal(np.flatnonzero(m[off[p]:off[p + 1]].cpu().numpy()), row['inlier_idx'])


# ---- the gather ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def matched():
    """Tables of 0, 1, 300 and 1 000 rows (the 300 are noisy copies of rows of the 1 000, so the ratio test keeps
    them), pairs in arbitrary order with a repeat and a self-pair."""
    import torch
    rng = np.random.default_rng(7)
    rows = [0, 1, 300, 1000]
    big = rng.integers(0, 256, (1000, 128)).astype(np.int16)
    small = np.clip(big[rng.permutation(1000)[:300]] + rng.integers(-3, 4, (300, 128)), 0, 255)
    desc = np.concatenate([np.zeros((0, 128)), big[:1], small, big]).astype(np.uint8)
    geom = rng.uniform(-1, 1, (sum(rows), 4)).astype(np.float32)
    seg = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    pairs = np.array([[2, 3], [3, 2], [0, 3], [2, 3], [3, 3], [1, 3], [2, 2], [1, 1]], np.int32)
    return torch.from_numpy(desc).cuda(), torch.from_numpy(geom).cuda(), seg, pairs


def _per_pair_loop(desc, geom, seg, pairs, ratio):
    """(x0, x1) per pair through the single-pair entry points."""
    import torch
    from spectavi_amd import device as spv
    out = []
    for q, d in pairs:
        dq, dd = desc[seg[q]:seg[q + 1]], desc[seg[d]:seg[d + 1]]
        if len(dq) == 0:
            out.append((np.zeros((0, 3)), np.zeros((0, 3))))
            continue
        idx, dist = spv.l1k2(dd.contiguous(), dq.contiguous())
        m, c = spv.ratio_test(idx, dist, ratio)
        x0, x1 = spv.match_coordinates(geom[seg[d]:seg[d + 1]].contiguous(), geom[seg[q]:seg[q + 1]].contiguous(), m, c)
        k = int(c.item())
        out.append((x0[:k].cpu().numpy(), x1[:k].cpu().numpy()))
    return out


@pytest.mark.parametrize("ratio,npairs", [(1.5, 8), (1e30, 4)])
def test_gather_equals_the_per_pair_loop(matched, ratio, npairs):
    """min_ratio 1.5 over all pairs; 1e30 over the first four, none of which holds an exact copy: no match at all
    (count = 0)."""
    from spectavi_amd import device as spv
    desc, geom, seg, pairs = matched
    pairs = pairs[:npairs]
    idx, dist, out_off = spv.l1k2_batch(desc, seg, pairs)
    m, c = spv.ratio_test(idx, dist, ratio)
    x0, x1, pair_off = spv.match_coordinates_batch(geom, seg, pairs, m, c)
    loop = _per_pair_loop(desc, geom, seg, pairs, ratio)
    want_off = np.concatenate([[0], np.cumsum([len(a) for a, _ in loop])])
    assert pair_off.dtype == np.int64 and np.array_equal(pair_off, want_off) and pair_off[-1] == int(c.item())
    n = int(c.item())
    assert (n == 0) == (npairs == 4)
    if n:
        assert x0[:n].cpu().numpy().tobytes() == np.concatenate([a for a, _ in loop]).tobytes()
        assert x1[:n].cpu().numpy().tobytes() == np.concatenate([b for _, b in loop]).tobytes()
        assert want_off[3] == want_off[2] and want_off[5] == want_off[4] + 1000  # a pair with no match; the self-pair
    # rows at and beyond count stay as they were
    assert not x0[n:].any().item() and not x1[n:].any().item()


def _gather_raw(geom, seg, pairs, m, c, cap, x0, x1, pair_off, stream):
    """spv_gather_match_coords_batch_device into the caller's tensors on `stream`, without waiting for it."""
    from spectavi_amd._lib import clib, check
    seg = np.ascontiguousarray(seg, np.int64)
    prs = np.ascontiguousarray(pairs, np.int32)
    check(clib.spv_gather_match_coords_batch_device(geom.data_ptr(), seg.ctypes.data, len(seg) - 1, prs.ctypes.data, len(prs),
                                                    m.data_ptr(), c.data_ptr(), cap, x0.data_ptr(), x1.data_ptr(),
                                                    pair_off.data_ptr(), ct.c_void_p(stream.cuda_stream)))


def test_gather_with_a_capacity_below_the_count(matched):
    """matches[:cap] with cap inside a pair's matches, and cap = 0: the first cap matches are gathered, the pair is
    cut short, later pairs are empty and no row at or beyond cap is written."""
    import torch
    from spectavi_amd import device as spv
    desc, geom, seg, pairs = matched
    idx, dist, _ = spv.l1k2_batch(desc, seg, pairs)
    m, c = spv.ratio_test(idx, dist, 1.5)
    loop = _per_pair_loop(desc, geom, seg, pairs, 1.5)
    want_off = np.concatenate([[0], np.cumsum([len(a) for a, _ in loop])])
    want0, want1 = np.concatenate([a for a, _ in loop]), np.concatenate([b for _, b in loop])
    n = int(c.item())
    assert n == want_off[-1] and want_off[4] - want_off[3] > 20
    for cap in (int(want_off[3]) + 7, 0):
        x0, x1, pair_off = spv.match_coordinates_batch(geom, seg, pairs, m[:cap], c)
        assert pair_off[-1] == cap and np.array_equal(pair_off, np.minimum(want_off, cap))
        assert x0.shape == (cap, 3) and x0.cpu().numpy().tobytes() == want0[:cap].tobytes()
        assert x1.cpu().numpy().tobytes() == want1[:cap].tobytes()
        # the same with room behind the capacity: rows from cap on stay as they were
        big0, big1 = (torch.zeros((n, 3), dtype=torch.float64, device="cuda") for _ in range(2))
        off = torch.full((len(pairs) + 1,), -1, dtype=torch.int64, device="cuda")
        _gather_raw(geom, seg, pairs, m[:cap], c, cap, big0, big1, off, torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert np.array_equal(off.cpu().numpy(), np.minimum(want_off, cap))
        assert big0[:cap].cpu().numpy().tobytes() == want0[:cap].tobytes()
        assert big1[:cap].cpu().numpy().tobytes() == want1[:cap].tobytes()
        assert not big0[cap:].any().item() and not big1[cap:].any().item()


def test_gather_table_regrows_between_calls_on_two_streams(matched):
    """2 pairs, 8 pairs, 2 pairs, alternating between the current stream and a second one with no wait in between:
    the calling thread's pair table grows for the second call, and each call waits for the kernel that read the
    table last before it overwrites it.  Then 24 pairs and 2 again: more pairs than any other test of this
    process has gathered, so the table grows here wherever in the suite this runs.  Each result is its per-pair
    loop's."""
    import torch
    from spectavi_amd import device as spv
    desc, geom, seg, pairs = matched
    calls = []
    for prs in (pairs[:2], pairs, pairs[3:5], np.tile(pairs, (3, 1)), pairs[5:7]):
        idx, dist, _ = spv.l1k2_batch(desc, seg, prs)
        m, c = spv.ratio_test(idx, dist, 1.5)
        cap = m.shape[0]
        outs = (torch.zeros((cap, 3), dtype=torch.float64, device="cuda"), torch.zeros((cap, 3), dtype=torch.float64, device="cuda"),
                torch.full((len(prs) + 1,), -1, dtype=torch.int64, device="cuda"))
        calls.append((prs, m, c, cap, outs, _per_pair_loop(desc, geom, seg, prs, 1.5)))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()  # inputs and zeroed outputs are there for both streams
    for k, (prs, m, c, cap, outs, _) in enumerate(calls):
        _gather_raw(geom, seg, prs, m, c, cap, *outs, side if k % 2 else torch.cuda.current_stream())
    torch.cuda.synchronize()
    for prs, m, c, cap, (x0, x1, pair_off), loop in calls:
        want_off = np.concatenate([[0], np.cumsum([len(a) for a, _ in loop])])
        n = int(want_off[-1])
        assert n > 0 and n == int(c.item()) and np.array_equal(pair_off.cpu().numpy(), want_off), len(prs)
        assert x0[:n].cpu().numpy().tobytes() == np.concatenate([a for a, _ in loop]).tobytes(), len(prs)
        assert x1[:n].cpu().numpy().tobytes() == np.concatenate([b for _, b in loop]).tobytes(), len(prs)
        assert not x0[n:].any().item() and not x1[n:].any().item()


def test_matches_to_fits_end_to_end(matched):
    """l1k2_batch -> ratio_test -> match_coordinates_batch -> ransac_fit_batch against the per-pair loop."""
    from spectavi_amd import device as spv
    from spectavi_amd import mvg
    desc, geom, seg, pairs = matched
    idx, dist, _ = spv.l1k2_batch(desc, seg, pairs)
    m, c = spv.ratio_test(idx, dist, 1.5)
    x0, x1, pair_off = spv.match_coordinates_batch(geom, seg, pairs, m, c)
    n = int(pair_off[-1])
    sizes = np.diff(pair_off)
    smp = [rc.subsets(70 + p, int(k), 40) for p, k in enumerate(sizes)]
    kw = dict(required_percent_inliers=0.5, reprojection_error_allowed=0.05, find_best_even_in_failure=True)
    rows = spv.ransac_fit_batch(x0[:n].contiguous(), x1[:n].contiguous(), pair_off, samples=np.stack(smp), **kw)
    loop = _per_pair_loop(desc, geom, seg, pairs, 1.5)
    singles = [mvg.ransac_fit(a, b, samples=s, **kw) if len(a) >= 10 else None for (a, b), s in zip(loop, smp)]
    _compare(rows, singles, 40, "end to end")
    assert sum(one is not None for one in singles) >= 4
