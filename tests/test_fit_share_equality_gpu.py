"""The share test of the best-model rule at the equality point: a try whose inlier share is exactly the required one.

The two-view fits (ransac_fit, ransac_fit_batch) take a candidate as a success when its share is ABOVE the required
share (src/RansacFitter.h:196-214); resection (resect_fit_batch) when it REACHES it (include/spectavi_amd.h).  The
three reductions share one statement of the rule, so this difference is pinned here: three sets of 64 rows and 32 fixed
subsets each; a first run with a share no try reaches and find_best_even_in_failure gives each set's best count c, and
the required share is then c / 64 -- exact in binary, and the double the kernels form from the count and the set size."""
import numpy as np
import pytest

from tests import ransac_batch_cases as rbc
from tests import resect_model as rm

pytestmark = pytest.mark.gpu

ROWS, TRIES, NSETS = 64, 32, 3
TWO_VIEW = dict(reprojection_error_allowed=rbc.THRESHOLD, singular_value_ratio_allowed=3e-2)


def same_model(a, b):
    if any(a[k] != b[k] for k in ("best_try", "best_root", "inlier_percent")):
        return False
    return (a["essential"].tobytes() == b["essential"].tobytes() and a["camera"].tobytes() == b["camera"].tobytes()
            and np.array_equal(a["inlier_idx"], b["inlier_idx"]))


@pytest.fixture(scope="module")
def two_view():
    """The collection and, per set, the best-on-failure fit under a share that no try reaches."""
    from spectavi_amd import mvg
    x0s, x1s, smp, _ = rbc.collection([ROWS] * NSETS, [0.2, 0.3, 0.4], TRIES, 6100)
    best = mvg.ransac_fit_batch(x0s, x1s, required_percent_inliers=2.0, find_best_even_in_failure=True, samples=smp,
                                **TWO_VIEW)
    for f in best:
        assert not f["success"] and f["best_try"] >= 0 and f["tries_run"] == TRIES
        assert len(f["inlier_idx"]) >= 7 and f["inlier_percent"] == len(f["inlier_idx"]) / ROWS
    return x0s, x1s, smp, best


@pytest.mark.parametrize("p", range(NSETS))
def test_two_view_share_equal_to_the_best_is_no_success(two_view, p):
    from spectavi_amd import mvg
    x0s, x1s, smp, best = two_view
    share = len(best[p]["inlier_idx"]) / ROWS
    assert share == best[p]["inlier_percent"]
    for find_best in (True, False):
        kw = dict(required_percent_inliers=share, find_best_even_in_failure=find_best, **TWO_VIEW)
        row = mvg.ransac_fit_batch(x0s, x1s, samples=smp, **kw)[p]
        single = mvg.ransac_fit(x0s[p], x1s[p], samples=smp[p], **kw)
        for what, f in (("ransac_fit_batch", row), ("ransac_fit", single)):
            print("set %d, find_best %d, %s: success %d, best_try %d, inliers %d of %d" % (
                p, find_best, what, f["success"], f["best_try"], len(f["inlier_idx"]), ROWS))
            assert not f["success"] and f["tries_run"] == TRIES, what
            if find_best:
                assert same_model(f, best[p]), what
            else:
                assert f["best_try"] == -1 and f["best_root"] == -1 and f["essential"] is None and f["camera"] is None, what
                assert len(f["inlier_idx"]) == 0 and f["inlier_percent"] == 0.0, what


@pytest.fixture(scope="module")
def resection():
    """The collection, its subsets and every try's count, from a run whose share no try reaches."""
    import torch
    from spectavi_amd import device
    rng = np.random.default_rng(6200)
    col = rm.collection(rng, [ROWS] * NSETS, noise=0.0, outliers=0.3)
    smp = rm.draw_samples(rng, col["off"], TRIES, col["planted"], clean_every=8)
    x, Xw = torch.from_numpy(col["x"]).cuda(), torch.from_numpy(col["Xw"]).cuda()
    fits, _, inl = device.resect_fit_batch(x, Xw, col["off"], required_percent_inliers=2.0, max_error=1.0,
                                           find_best_even_in_failure=True, samples=smp, want_tries=True)
    inl = inl.cpu().numpy()
    for p, f in enumerate(fits):
        assert not f["success"] and f["tries_run"] == TRIES and len(f["inlier_idx"]) == inl[p].max() >= 6
        assert f["best_try"] == int(np.argmax(inl[p]))
    return x, Xw, col["off"], smp, inl


@pytest.mark.parametrize("p", range(NSETS))
def test_resection_share_equal_to_the_best_is_a_success(resection, p):
    from spectavi_amd import device
    x, Xw, off, smp, inl = resection
    c = int(inl[p].max())
    first = int(np.flatnonzero(inl[p] == c)[0])
    for find_best in (True, False):
        f = device.resect_fit_batch(x, Xw, off, required_percent_inliers=c / ROWS, max_error=1.0,
                                    find_best_even_in_failure=find_best, samples=smp)[p]
        print("set %d, find_best %d: success %d, best_try %d (first try with %d inliers: %d)" % (
            p, find_best, f["success"], f["best_try"], c, first))
        assert f["success"] and f["best_try"] == first and len(f["inlier_idx"]) == c
        assert f["inlier_percent"] == c / ROWS and f["tries_run"] == TRIES
