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

# One dim per staged width of ann_coarse_kernel<SHAPE, KG> (KG = kpad / 32 up to 128 columns, 0 beyond), for
# both MFMA shapes: the default one in process, the other under SPECTAVI_ANN_MFMA=16 in tests/knob_child.py.
COARSE_CASES = (32, 64, 65, 96, 128, 160)
COARSE_SHAPES = (32, 16)
COARSE_SLICES = (0, 1, 3)
RERANK_CASES = (64, 65)          # ncand: ann_rerank_kernel<1> up to 64, <4> beyond
# (k, ncand) on both sides of every step of the survivor buffer length (128, 192, 256, 320, 384 keys)
LARGE_DIMS = (33, 132)
LARGE_PAIRS = ((32, 32), (33, 33), (64, 64), (64, 65), (8, 160), (8, 161), (8, 224), (8, 225), (64, 256))
LARGE_SLICES = (0, 7)
MODEL_SETS = ("randn", "offset", "scaled")
MODEL_NCAND = (4, 16, 64)
MODEL_SLICES = (0, 3)
SCALED_SEED = 0
WINDOW_DIMS = (100, 128)
WINDOW_BASES = (0, -255, 100000)
WINDOW_K = (2, 8)


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
    if name == "scaled":     # column scales log-uniform in [1e-3, 1e3], column offsets up to +-1e4
        rng = np.random.default_rng(SCALED_SEED)
        scale = 10.0 ** rng.uniform(-3, 3, 64)
        off = rng.uniform(-1e4, 1e4, 64)
        off[:2] = (-1e4, 1e4)
        return ((rng.standard_normal((2000, 64)) * scale + off).astype(np.float32),
                (rng.standard_normal((300, 64)) * scale + off).astype(np.float32))
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


# ---- the variant cases of tests/test_ann_variants_gpu.py and of the "ann_mfma16" child -----------------
def coarse_kg(kpad):
    """KG of the ann_coarse_kernel<SHAPE, KG> that ann_run launches at this padded width."""
    return kpad // 32 if kpad <= 128 else 0


def rerank_per(ncand):
    """PER of the ann_rerank_kernel<PER> that ann_run launches at this candidate count."""
    return 1 if ncand <= 64 else 4


@functools.lru_cache(maxsize=None)
def coarse_case(dim):
    """(x, y, oracle) of a COARSE_CASES dim: 1000 rows are several compactions per slice, 150 queries one
    full block of 128 and a ragged one."""
    x, y = edge_rows(1000, 150, dim)
    return x, y, bo.nn_bruteforce(x, y, 2.0, EDGE_K)


@functools.lru_cache(maxsize=None)
def large_case(dim):
    """(x, y, the oracle's 64 nearest) of a LARGE_DIMS dim; values in [0, 15]: ties at every k-th place."""
    x, y = edge_rows(1500, 150, dim)
    return x, y, bo.nn_bruteforce(x, y, 2.0, 64)


def window_rows(dim, a, xrows=700, yrows=150):
    """The corner of the exact domain: integers of {a, a+1, a+254, a+255}, whole rows of a and of a+255.
    The database leans on the low pair, so that every column's centre is within 8 of a and the centred
    values reach 247 and more: with two rows of a+255 the sum of products is at least 247^2 dim.  The
    asserts keep the case inside the header's contract by construction."""
    from tests import ann_coarse_model as cm
    rng = np.random.default_rng([dim, abs(a), int(a < 0)])
    vals = np.array([0, 1, 254, 255], np.int64) + a
    x = vals[rng.choice(4, (xrows, dim), p=(0.7, 0.296, 0.002, 0.002))]
    y = vals[rng.integers(0, 4, (yrows, dim))]
    x[::50], x[25::233] = a, a + 255
    y[::30], y[15::30] = a, a + 255
    x, y = x.astype(np.float32), y.astype(np.float32)
    m = cm.centre(x)
    assert np.array_equal(x.astype(np.int64), np.rint(x)) and (np.abs(m - a) <= 8).all()
    assert np.abs(x - m).max() <= 255 and np.abs(y - m).max() <= 255 and 255 * 255 * dim < 2 ** 24
    assert np.abs(x - m).max() >= 247 and np.abs(y - m).max() >= 247
    return x, y


@functools.lru_cache(maxsize=None)
def window_case(dim, a):
    x, y = window_rows(dim, a)
    return x, y, bo.nn_bruteforce(x, y, 2.0, max(WINDOW_K))


@functools.lru_cache(maxsize=None)
def model_case(name):
    """(s*, eps) of tests/ann_coarse_model.py for a MODEL_SETS data set, read-only."""
    from tests import ann_coarse_model as cm
    s, eps = cm.scores(*property_rows(name))
    s.setflags(write=False)
    eps.setflags(write=False)
    return s, eps


@functools.lru_cache(maxsize=None)
def model_rules(name, ncand):
    from tests import ann_coarse_model as cm
    return cm.rules(*model_case(name), ncand)


def device_run(x, y, k, ncand=0, slices=0):
    import torch
    from spectavi_amd import device
    i, d = device.ann_l2(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), k=k, ncand=ncand, slices=slices)
    torch.cuda.synchronize()
    return i.cpu().numpy().view(np.uint64), d.cpu().numpy()


def assert_bits(got, want, what=""):
    gi, gd = got
    wi, wd = want
    assert gi.dtype == np.uint64 and gd.dtype == np.float32 and gi.shape == wi.shape and gd.shape == wd.shape, what
    bad = np.flatnonzero((gi != wi).any(1) | (gd.view(np.uint32) != wd.view(np.uint32)).any(1))
    assert bad.size == 0, "%s: %d rows differ, first %s: got %s / %s, want %s / %s" % (
        what, bad.size, bad[:5], gi[bad[:2]], gd[bad[:2]], wi[bad[:2]], wd[bad[:2]])


def check_coarse_case(dim, slices, mfma):
    """A COARSE_CASES dim at ncand = k = 8 against the oracle, on the coarse kernel the plan names."""
    from spectavi_amd import device
    x, y, want = coarse_case(dim)
    p = device.ann_l2_plan(x.shape[0], y.shape[0], dim, EDGE_K, EDGE_K, slices)
    assert p["mfma"] == mfma and p["kpad"] == (dim + 31) // 32 * 32 and (slices == 0 or p["slices"] == slices), p
    assert_bits(device_run(x, y, EDGE_K, EDGE_K, slices), want, "coarse dim=%d slices=%d mfma=%d" % (dim, slices, mfma))


def check_large_case(dim, k, ncand, mfma):
    """A LARGE_PAIRS pair against the oracle, with the plan's slices and with 7 forced ones (the merge
    kernel then folds part-filled buffers)."""
    from spectavi_amd import device
    x, y, (oi, od) = large_case(dim)
    for slices in LARGE_SLICES:
        p = device.ann_l2_plan(x.shape[0], y.shape[0], dim, k, ncand, slices)
        assert p["mfma"] == mfma and p["ncand"] == ncand and p["buflen"] == (ncand + 96 + 63) // 64 * 64, p
        assert slices == 0 or p["slices"] == slices, p
        assert_bits(device_run(x, y, k, ncand, slices), (oi[:, :k], od[:, :k]),
                    "large dim=%d k=%d ncand=%d slices=%d mfma=%d" % (dim, k, ncand, slices, mfma))


def check_model_case(name, ncand, mfma):
    """The candidate set (the result at k = ncand) of a MODEL_SETS data set against both rules of
    tests/ann_coarse_model.py, for every query; returns the line that the tests print."""
    from spectavi_amd import device
    from tests import ann_coarse_model as cm
    x, y = property_rows(name)
    must, must_not = model_rules(name, ncand)
    for slices in MODEL_SLICES:
        assert device.ann_l2_plan(x.shape[0], y.shape[0], x.shape[1], ncand, ncand, slices)["mfma"] == mfma
        gi, _ = device_run(x, y, ncand, ncand, slices)
        bad = np.flatnonzero(cm.violations(must, must_not, gi.astype(np.int64)))
        assert bad.size == 0, "model %s ncand=%d slices=%d mfma=%d: %d queries break a rule, first %s" % (
            name, ncand, slices, mfma, bad.size, bad[:5])
    free = cm.open_rows(must, must_not, ncand)
    return "ann coarse model: %s 2000x300x64 ncand=%d: %d open rows, %d of %d queries have one" % (
        name, ncand, int(free.sum()), int((free > 0).sum()), free.size)
