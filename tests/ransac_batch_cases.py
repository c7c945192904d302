"""Collections of correspondence sets for the many-sets RANSAC tests (tests/test_ransac_batch_args.py,
tests/test_ransac_batch_gpu.py): scenes from tests/mvg_checks.two_view_scene with fixed seeds, as the single-fit
tests draw them, and the comparison of a batch row with a single fit."""
import numpy as np

from tests import mvg_checks as mc

THRESHOLD = 1e-3  # noise-free scenes: the reprojection error that separates planted inliers from outliers

# (required share, find_best) of test_ransac_fit_matches_oracle_given_the_same_subsets, with `clean` the clean
# share of the most contaminated set (0.65): success, best-on-failure and no model at all
SETTINGS = [(0.55, False), (0.55, True), (0.995, False), (0.995, True)]

# the sizes every collection of the edge test holds: empty, skipped, the minimum, the row-block edge, many row blocks
EDGE_SIZES = [0, 9, 10, 255, 256, 257, 2500]
EDGE_OUTLIERS = [0.0, 0.0, 0.1, 0.15, 0.2, 0.3, 0.35]


def scene(seed, npt, outliers):
    """x0, x1 float64 [npt,3] and the planted inlier rows."""
    if npt == 0:
        return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int64)
    x0, x1, _, out_idx = mc.two_view_scene(np.random.default_rng(seed), npt=npt, outlier_fraction=outliers)
    return x0, x1, np.setdiff1d(np.arange(npt), out_idx)


def subsets(seed, npt, ntries):
    """int32 [ntries,7] as spv_ransac_sample draws them; a set too small to run gets rows no set holds (its
    subsets must not be read)."""
    from spectavi_amd import mvg
    if npt < 10:
        return np.full((ntries, 7), -7, np.int32)
    return mvg.ransac_sample(seed, npt, ntries)


def collection(sizes, outliers, ntries, seed0):
    """Lists x0s, x1s, samples, planted inliers: set p from seed seed0 + p."""
    x0s, x1s, smp, inl = [], [], [], []
    for p, (n, f) in enumerate(zip(sizes, outliers)):
        a, b, keep = scene(seed0 + p, n, f)
        x0s.append(a)
        x1s.append(b)
        inl.append(keep)
        smp.append(subsets(1000 + seed0 + p, n, ntries))
    return x0s, x1s, smp, inl


def offsets(x0s):
    return np.concatenate([[0], np.cumsum([len(x) for x in x0s])]).astype(np.int64)


def skipped_row():
    return {'success': False, 'essential': None, 'camera': None, 'inlier_percent': 0.0, 'n_inliers': 0,
            'best_try': -1, 'best_root': -1, 'tries_run': 0}


def assert_same_fit(row, single, ntries, what):
    """A batch row against the single fit of the same set with the same subsets: bit for bit on everything but
    tries_run, which stays within its bounds."""
    for k in ('success', 'best_try', 'best_root', 'inlier_percent'):
        assert row[k] == single[k], (what, k, row[k], single[k])
    assert np.array_equal(row['inlier_idx'], single['inlier_idx']), what
    assert row['inlier_idx'].dtype == np.int32
    for k in ('essential', 'camera'):
        if single[k] is None:
            assert row[k] is None, (what, k)
        else:
            assert row[k] is not None and row[k].tobytes() == single[k].tobytes(), (what, k)
    if row['success']:
        assert row['best_try'] < row['tries_run'] <= ntries, (what, row['tries_run'])
    else:
        assert row['tries_run'] == ntries, (what, row['tries_run'])


def assert_skipped(row, what):
    want = skipped_row()
    for k in ('success', 'essential', 'camera', 'inlier_percent', 'best_try', 'best_root', 'tries_run'):
        assert row[k] == want[k] or (row[k] is None and want[k] is None), (what, k, row[k])
    assert len(row['inlier_idx']) == 0, what
