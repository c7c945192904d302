"""The many-sets RANSAC (spv_ransac_fit_batch_device) where rounds fill up and where sets are not clean.

Rounds: collection A fills rounds to the tries cap, collection B to the work cap (tests/ransac_batch_cases.py;
tests/test_ransac_batch_schedule.py asserts on the host model that they do).  Every row is the single fit's, bit for
bit; tries_run of every set and the number of rounds (= launches of the reduction) are the model's, fed with the
single fits' first successes.

Sets that are not clean: noisy scenes, the inf / nan / overflow class table of the DLT edge tests, repeated and
identical correspondences, single NaN / inf rows and a rescaled set, with clean sets between them.  Every row is
its single fit's, the clean rows are what they are without such neighbours, every mask byte is written."""
import ctypes as ct

import numpy as np
import pytest

from tests import ransac_batch_cases as rc

pytestmark = pytest.mark.gpu


def _cat(xs):
    import torch
    return torch.from_numpy(np.concatenate(xs)).cuda()


def _compare(rows, singles, ntries, what):
    assert len(rows) == len(singles)
    for p, (row, one) in enumerate(zip(rows, singles)):
        rc.assert_same_fit(row, one, ntries, (what, p))


def _counted_rounds(call):
    """call() with profiling on: (its result, launches of the reduction = rounds)."""
    from spectavi_amd import device
    device.profile_reset()
    device.profile_enable(True)
    try:
        out = call()
        return out, device.profile_read("ransac_batch_reduce")[0]
    finally:
        device.profile_enable(False)
        device.profile_reset()


def _check_schedule(rows, singles, sizes, ntries, nrounds, what):
    firsts = [one['best_try'] if one['success'] else None for one in singles]
    rounds, tries_run = rc.schedule(sizes, ntries, firsts)
    got = [row['tries_run'] for row in rows]
    assert got == tries_run, (what, [(p, g, w) for p, (g, w) in enumerate(zip(got, tries_run)) if g != w][:8])
    assert nrounds == len(rounds), (what, nrounds, len(rounds))


@pytest.fixture(scope="module")
def coll_a():
    x0s, x1s, smp, seeds = rc.collection_a()
    return x0s, x1s, smp, seeds, _cat(x0s), _cat(x1s)


def _a_success_is_the_clean_sets(singles):
    assert [one['success'] for one in singles] == rc.collection_a_shape()[1]


def test_tries_cap_with_samples_equals_the_single_fits_and_the_model(coll_a):
    from spectavi_amd import device as spv
    from spectavi_amd import mvg
    x0s, x1s, smp, _, cat0, cat1 = coll_a
    singles = [mvg.ransac_fit(a, b, samples=s, **rc.A_SETTINGS) for a, b, s in zip(x0s, x1s, smp)]
    _a_success_is_the_clean_sets(singles)
    off, samples = rc.offsets(x0s), np.stack(smp)
    rows, nrounds = _counted_rounds(lambda: spv.ransac_fit_batch(cat0, cat1, off, samples=samples, **rc.A_SETTINGS))
    _compare(rows, singles, rc.A_TRIES, "A, samples")
    _check_schedule(rows, singles, [len(a) for a in x0s], rc.A_TRIES, nrounds, "A, samples")
    # the mask of the same call: the inlier lists
    again, mask = spv.ransac_fit_batch(cat0, cat1, off, samples=samples, want_mask=True, **rc.A_SETTINGS)
    _compare(again, singles, rc.A_TRIES, "A, samples, with mask")
    mask = mask.cpu().numpy()
    assert mask.dtype == np.uint8 and mask.max() == 1
    for p, one in enumerate(singles):
        assert np.array_equal(np.flatnonzero(mask[off[p]:off[p + 1]]), one['inlier_idx']), p


def test_tries_cap_with_seeds_equals_the_seeded_single_fits_and_the_model(coll_a):
    """Sets wait for a round and leave between others: every set's generator must stay its own and must not be
    advanced while the set waits."""
    from spectavi_amd import device as spv
    from spectavi_amd import mvg
    x0s, x1s, _, seeds, cat0, cat1 = coll_a
    singles = [mvg.ransac_fit(a, b, maximum_tries=rc.A_TRIES, seed=s, **rc.A_SETTINGS) for a, b, s in zip(x0s, x1s, seeds)]
    _a_success_is_the_clean_sets(singles)
    rows, nrounds = _counted_rounds(lambda: spv.ransac_fit_batch(cat0, cat1, rc.offsets(x0s), maximum_tries=rc.A_TRIES,
                                                                 seeds=seeds, **rc.A_SETTINGS))
    _compare(rows, singles, rc.A_TRIES, "A, seeds")
    _check_schedule(rows, singles, [len(a) for a in x0s], rc.A_TRIES, nrounds, "A, seeds")


def test_work_cap_equals_the_single_fits_and_the_model():
    from spectavi_amd import device as spv
    from spectavi_amd import mvg
    x0s, x1s, smp = rc.collection_b()
    singles = [mvg.ransac_fit(a, b, samples=s, **rc.B_SETTINGS) for a, b, s in zip(x0s, x1s, smp)]
    # the late sets succeed on their first clean subset, nothing else does: one first success inside the slot that
    # the work cap cuts, one on the first try that a set kept waiting by the cap has not run
    assert [one['best_try'] if one['success'] else None for one in singles] == rc.collection_b_firsts()
    assert all(one['best_try'] >= 0 for one in singles)
    cat0, cat1 = _cat(x0s), _cat(x1s)
    rows, nrounds = _counted_rounds(lambda: spv.ransac_fit_batch(cat0, cat1, rc.offsets(x0s), samples=np.stack(smp),
                                                                 **rc.B_SETTINGS))
    _compare(rows, singles, rc.B_TRIES, "B")
    _check_schedule(rows, singles, rc.B_SIZES, rc.B_TRIES, nrounds, "B")


# ---- sets that are not clean ------------------------------------------------------------------------------------

UNCLEAN_TRIES = 150
NOISY = [(777, 0.3, 2e-4), (2500, 0.35, 1e-4)]  # test_ransac_fit_matches_oracle_given_the_same_subsets' noisy scenes
# One call has one threshold, and each noisy scene is meant at 6 x its noise: the collection runs at both.
THRESHOLDS = [6 * 2e-4, 6 * 1e-4]


@pytest.fixture(scope="module")
def unclean():
    """names, x0s, x1s, samples; every second set is a clean (noise-free) one of rc.collection."""
    from spectavi_amd import mvg
    from tests import dlt_edge_cases as ec
    from tests import mvg_checks as mc
    sets = []
    for npt, outliers, noise in NOISY:
        x0, x1, _, _ = mc.two_view_scene(np.random.default_rng(npt), npt=npt, outlier_fraction=outliers, noise=noise)
        sets.append(("noisy %d" % npt, x0, x1, mvg.ransac_sample(1234 + npt, npt, UNCLEAN_TRIES)))
    _, _, x, xp = ec.class_table(31, npt=257)
    sets.append(("class table", x, xp, None))
    a, b, _ = rc.scene(601, 300, 0.0)
    sets.append(("300 copies", np.repeat(a[:1], 300, axis=0), np.repeat(b[:1], 300, axis=0), None))
    sets.append(("x1 == x0", a, a.copy(), None))
    for name, seed, bad in (("one nan row", 602, np.nan), ("one inf row", 603, np.inf)):
        a, b, _ = rc.scene(seed, 300, 0.25)
        b = b.copy()
        b[123] = bad
        sets.append((name, a, b, None))
    a, b, _ = rc.scene(604, 300, 0.25)
    sets.append(("scaled by 1e150", a * 1e150, b * 1e150, None))
    cx0, cx1, csmp, _ = rc.collection([300, 64, 257, 500, 120, 300, 256, 200, 333], [0.25, 0.1, 0.3, 0.2, 0.15, 0.3, 0.2, 0.35, 0.25],
                                      UNCLEAN_TRIES, 650)
    names, x0s, x1s, smp = [], [], [], []
    for k, (cl0, cl1, cls) in enumerate(zip(cx0, cx1, csmp)):  # clean, unclean, clean, ..., clean
        names.append("clean %d" % k)
        x0s.append(cl0)
        x1s.append(cl1)
        smp.append(cls)
        if k < len(sets):
            name, a, b, s = sets[k]
            names.append(name)
            x0s.append(np.ascontiguousarray(a))
            x1s.append(np.ascontiguousarray(b))
            smp.append(s if s is not None else mvg.ransac_sample(700 + k, len(a), UNCLEAN_TRIES))
    assert len(sets) == 8 and len(names) == 17 and max(len(a) for a in x0s) == 2500
    return names, x0s, x1s, smp


def _call_with_filled_mask(x0s, x1s, smp, kw, fill=0xAB):
    """spv_ransac_fit_batch_device with a caller's mask that starts as `fill`: (rows, mask as numpy)."""
    import torch
    from spectavi_amd import device as spv
    from spectavi_amd._lib import clib, check
    off = rc.offsets(x0s)
    npairs, total = len(x0s), int(off[-1])
    cat0, cat1 = _cat(x0s), _cat(x1s)
    samples = np.ascontiguousarray(np.stack(smp), dtype=np.int32)
    mask = torch.full((total,), fill, dtype=torch.uint8, device="cuda")
    ok, n, bt, br, ran = (np.zeros(npairs, np.int32) for _ in range(5))
    F, P, pct, idx = np.zeros((npairs, 9)), np.zeros((npairs, 12)), np.zeros(npairs), np.zeros(total, np.int32)
    stream = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(clib.spv_ransac_fit_batch_device(
        cat0.data_ptr(), cat1.data_ptr(), off.ctypes.data, npairs, kw['required_percent_inliers'],
        kw['reprojection_error_allowed'], samples.shape[1], int(kw['find_best_even_in_failure']),
        kw['singular_value_ratio_allowed'], samples.ctypes.data, None, ok.ctypes.data, F.ctypes.data, P.ctypes.data,
        pct.ctypes.data, idx.ctypes.data, n.ctypes.data, bt.ctypes.data, br.ctypes.data, ran.ctypes.data, mask.data_ptr(),
        stream))
    torch.cuda.synchronize()
    return spv._fit_batch_dicts(off, ok, F, P, pct, idx, n, bt, br, ran), mask.cpu().numpy()


@pytest.mark.parametrize("thr", THRESHOLDS, ids=["thr6x2e-4", "thr6x1e-4"])
@pytest.mark.parametrize("req,find_best", rc.SETTINGS)
def test_unclean_sets_equal_their_single_fits_and_leave_their_neighbours_alone(unclean, oracle, req, find_best, thr):
    from spectavi_amd import mvg
    from tests.test_ransac_fit_gpu import _same_model
    names, x0s, x1s, smp = unclean
    kw = dict(required_percent_inliers=req, reprojection_error_allowed=thr, find_best_even_in_failure=find_best,
              singular_value_ratio_allowed=3e-2)
    singles = [mvg.ransac_fit(a, b, samples=s, **kw) for a, b, s in zip(x0s, x1s, smp)]
    rows, mask = _call_with_filled_mask(x0s, x1s, smp, kw)
    for p, (row, one) in enumerate(zip(rows, singles)):
        rc.assert_same_fit(row, one, UNCLEAN_TRIES, (names[p], req, find_best, thr))
    # every mask byte is written, and is the inlier list
    off = rc.offsets(x0s)
    want = np.zeros(int(off[-1]), np.uint8)
    for p, one in enumerate(singles):
        want[off[p] + one['inlier_idx']] = 1
    assert np.array_equal(mask, want)
    # the clean sets: the rows of a collection that holds nothing else (one round either way: the same tries_run)
    keep = [p for p, name in enumerate(names) if name.startswith("clean")]
    alone, mask_alone = _call_with_filled_mask([x0s[p] for p in keep], [x1s[p] for p in keep], [smp[p] for p in keep], kw)
    for p, row in zip(keep, alone):
        rc.assert_same_fit(rows[p], row, UNCLEAN_TRIES, ("clean alone", names[p], req, find_best, thr))
        assert rows[p]['tries_run'] == row['tries_run']
        assert np.array_equal(mask[off[p]:off[p + 1]], mask_alone[:len(x0s[p])])
        mask_alone = mask_alone[len(x0s[p]):]
    # the 777-row noisy scene at its own threshold against the oracle, by the single test's rule
    if thr == 6 * NOISY[0][2]:
        p = names.index("noisy 777")
        o = oracle.ransac_fit(x0s[p], x1s[p], smp[p], **kw)
        _same_model(rows[p], o, exact_inliers=False)
        assert len(np.setxor1d(rows[p]['inlier_idx'], o['inlier_idx'])) <= 2
