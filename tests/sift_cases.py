"""Shared inputs and the table comparison of the SIFT tests."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sur_ogre():
    """(image float32 [233, 310], vlfeat's table float32 [1168, 132])."""
    im = np.load(os.path.join(GOLDEN, "sift_sur_ogre_image.npz"))["im"].astype(np.float32)
    table = np.load(os.path.join(GOLDEN, "sift_sur_ogre_table.npz"))["table"]
    return im, table


def smooth_random(seed, h, w, passes=3):
    """Uniform noise in [0, 255) smoothed by `passes` circular [1 1 1]/3 passes along each axis."""
    r = np.random.default_rng(seed).random((h, w)) * 255
    for _ in range(passes):
        r = (r + np.roll(r, 1, 0) + np.roll(r, -1, 0)) / 3
        r = (r + np.roll(r, 1, 1) + np.roll(r, -1, 1)) / 3
    return r.astype(np.float32)


def ulp_diff(a, b):
    """Distance in float32 units in the last place (both finite, same sign assumed by the caller)."""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def assert_tables_match(got, want, what="", ulp=0):
    """The same rows; x, y, sigma, angle at most `ulp` float32 units apart (0: bit-equal); descriptors
    equal."""
    assert got.dtype == np.float32 and got.ndim == 2 and got.shape[1] == 132, (what, got.shape, got.dtype)
    assert got.shape == want.shape, "%s: %d rows, expected %d" % (what, got.shape[0], want.shape[0])
    if got.shape[0] == 0:
        return
    d = ulp_diff(got[:, :4], want[:, :4])
    assert d.max() <= ulp, "%s: frame rows %s differ by up to %d ulp" % (what, np.nonzero(d.max(1) > ulp)[0][:8], d.max())
    bad = np.nonzero(~np.all(got[:, 4:] == want[:, 4:], axis=1))[0]
    assert bad.size == 0, "%s: descriptor rows %s differ" % (what, bad[:8])


def orientation_counts(table):
    """Rows per keypoint (x, y, sigma)."""
    if len(table) == 0:
        return np.zeros(0, np.int64)
    _, counts = np.unique(table[:, :3], axis=0, return_counts=True)
    return counts
