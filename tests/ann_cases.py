"""Inputs of tests/test_ann_gpu.py and their oracle results (tests/bruteforce_oracle.py, p = 2), each
computed once per session and shared."""
import functools
import os

import numpy as np

from tests import bruteforce_oracle as bo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

GOLDEN_CASES = ("ties", "dups", "sift")
GOLDEN_K = (1, 2, 8)
EDGE_K = 8                       # edges run at ncand = k = 8: no slack
EDGE_DIMS = (1, 31, 32, 33, 100, 128, 132, 2048)
FORCED_SLICES = (1, 2, 3, 7)
SMALL_SCALES = (1e-20, 1.0, 1e15)
PROPERTY_SETS = ("randn", "clusters", "offset")
PROPERTY_K = 4
PROPERTY_NCAND = (PROPERTY_K, 16, 64, 256)


@functools.lru_cache(maxsize=None)
def golden_rows(name):
    """(x, y) float32 of a stored byte-valued case: every value an integer in [0, 255]."""
    if name == "ties":
        d = np.load(os.path.join(GOLDEN, "l1k2_ties_300x500_64.npz"))
        x, y = d["x"], d["y"]
    elif name == "dups":
        d = np.load(os.path.join(GOLDEN, "l1k2_dups_257x5_128.npz"))
        x, y = d["x"], d["y"]
    else:
        x = np.load(os.path.join(GOLDEN, "sift_sur_ogre_table.npz"))["table"][:, 4:]
        y = x[np.random.default_rng(1168).choice(x.shape[0], 300, replace=False)]
    x, y = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32)
    for a in (x, y):
        assert np.array_equal(a, np.rint(a)) and a.min() >= 0 and a.max() <= 255
    return x, y


@functools.lru_cache(maxsize=None)
def golden_oracle(name):
    """The oracle's 8 nearest of a stored case; its first k columns are the k nearest."""
    x, y = golden_rows(name)
    return bo.nn_bruteforce(x, y, 2.0, max(GOLDEN_K))


def edge_rows(xrows, yrows, dim, seed=0):
    """Integers in [0, 15]: many equal distances, so the (score, idx) order decides."""
    rng = np.random.default_rng([xrows, yrows, dim, seed])
    return (rng.integers(0, 16, (xrows, dim)).astype(np.float32),
            rng.integers(0, 16, (yrows, dim)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def property_rows(name):
    """2000 x 64 database, 300 queries."""
    rng = np.random.default_rng(sorted(PROPERTY_SETS).index(name) + 50)
    if name == "clusters":   # 40 centres, members 1e-3 apart: far below what bf16 resolves
        c = rng.standard_normal((40, 64))
        x = c[rng.integers(0, 40, 2000)] + 1e-3 * rng.standard_normal((2000, 64))
        y = c[rng.integers(0, 40, 300)] + 1e-3 * rng.standard_normal((300, 64))
    else:
        off = 100.0 if name == "offset" else 0.0
        x = rng.standard_normal((2000, 64)) + off
        y = rng.standard_normal((300, 64)) + off
    return x.astype(np.float32), y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def property_distances(name):
    x, y = property_rows(name)
    d = bo.distances(x, y, 2.0)
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def property_oracle(name):
    return bo.select(property_distances(name), PROPERTY_K)


@functools.lru_cache(maxsize=None)
def reference_rows():
    """The reference's own case (test/test_feature.py:49-65): randn 1000 x 132 on both sides."""
    rng = np.random.default_rng(49)
    return (rng.standard_normal((1000, 132)).astype(np.float32),
            rng.standard_normal((1000, 132)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def reference_oracle():
    x, y = reference_rows()
    return bo.nn_bruteforce(x, y, 2.0, 2)
