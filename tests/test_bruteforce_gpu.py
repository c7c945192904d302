"""Exact p-norm k-NN on the GPU (nn_bruteforce / nn_bruteforcei, device.bruteforce) against the
numpy statement of the contract, tests/bruteforce_oracle.py: indices and distance bits equal for
p in {1, 2, 0.5}, a stated tolerance for other p."""
import ctypes as ct

import numpy as np
import pytest

from tests import bruteforce_oracle as bo

pytestmark = pytest.mark.gpu

# The tile-kernel instantiations bruteforce_run launches (spectavi_amd/csrc/bruteforce.hip):
# bf_tile_kernel<INT, PK, KB> with the row type, the p branch (0: p = 1, 1: p = 2, 2: p = 0.5,
# 3: other p) and the list length KB = 2 (k <= 2), 8 (k <= 8), 64 (k <= 64); bf_merge_kernel<KB>.
K_BUCKET = {1: 2, 2: 2, 3: 8, 5: 8, 8: 8, 17: 64, 20: 64, 64: 64}
P_KIND = {1.0: 0, 2.0: 1, 0.5: 2, 1.5: 3, 3.0: 3}
INSTANTIATED = {(i, pk, kb) for i in (False, True) for pk in range(4) for kb in (2, 8, 64)}

MATRIX_P = (1.0, 2.0, 0.5)
MATRIX_K = (1, 2, 3, 8, 17, 64)
MATRIX_DIM = (1, 3, 16, 128, 132, 257, 2048)
GENERAL_CASES = [(p, is_int, k) for p in (1.5, 3.0) for is_int in (False, True) for k in (2, 5, 20)]


def test_case_table_reaches_every_instantiation():
    reached = {(i, P_KIND[p], K_BUCKET[k]) for p in MATRIX_P for i in (False, True) for k in MATRIX_K}
    reached |= {(i, P_KIND[p], K_BUCKET[k]) for p, i, k in GENERAL_CASES}
    assert reached == INSTANTIATED


def data(rng, rows, dim, is_int, lo=-50, hi=50):
    if is_int:
        return rng.integers(lo, hi, (rows, dim)).astype(np.int32)
    return rng.standard_normal((rows, dim)).astype(np.float32)


def host(x, y, p, k):
    """spv_nn_bruteforce: the raw rows through the host-pointer entry point."""
    from spectavi_amd import feature
    is_int = x.dtype == np.int32
    if is_int:
        oi, od = feature.NdArray(dtype="uint64"), feature.NdArray(dtype="int32")
        feature._nn_bruteforcei(x, y, x.shape[0], y.shape[0], x.shape[1], k, p, 0.0, ct.byref(oi), ct.byref(od))
    else:
        oi, od = feature.NdArray(dtype="uint64"), feature.NdArray(dtype="float32")
        feature._nn_bruteforce(x, y, x.shape[0], y.shape[0], x.shape[1], k, p, 0.0, ct.byref(oi), ct.byref(od))
    feature.check()
    return oi.asarray(), od.asarray()


def assert_bits(got, want):
    gi, gd = got
    wi, wd = want
    assert gi.dtype == np.uint64 and gd.dtype == wd.dtype and gd.shape == wd.shape
    bad = np.flatnonzero((gi != wi).any(1) | (gd.view(np.uint32) != wd.view(np.uint32)).any(1))
    assert bad.size == 0, "rows %s: got %s / %s, want %s / %s" % (
        bad[:5], gi[bad[:2]], gd[bad[:2]], wi[bad[:2]], wd[bad[:2]])


def test_reference_test_case():
    """The reference's own test (test/test_feature.py:67-81): 1000 x 1000 x 132 randn, p = 2, k = 2."""
    from spectavi_amd import feature
    rng = np.random.default_rng(67)
    x = rng.standard_normal((1000, 132)).astype(np.float32)
    y = rng.standard_normal((1000, 132)).astype(np.float32)
    got = feature.nn_bruteforce(x, y, p=2, k=2)
    assert_bits(got, bo.nn_bruteforce(x, y, 2.0, 2))


@pytest.mark.parametrize("dim", MATRIX_DIM)
@pytest.mark.parametrize("k", MATRIX_K)
@pytest.mark.parametrize("is_int", [False, True])
@pytest.mark.parametrize("p", MATRIX_P)
def test_matrix(p, is_int, k, dim):
    # 333 database rows: a ragged last 32-row group; 300 queries: a ragged second query block
    rng = np.random.default_rng([int(p * 2), is_int, k, dim])
    x, y = data(rng, 333, dim, is_int), data(rng, 300, dim, is_int)
    assert_bits(host(x, y, p, k), bo.nn_bruteforce(x, y, p, k, is_int))


@pytest.mark.parametrize("is_int", [False, True])
@pytest.mark.parametrize("k", [2, 8, 17])
def test_ties(is_int, k):
    """Values in {0, 1, 2} over 5 columns and repeated rows: most distances tie, many at the k-th
    place; the lower index must win."""
    rng = np.random.default_rng([k, is_int])
    base = rng.integers(0, 3, (50, 5))
    x = base[rng.integers(0, 50, 700)]
    y = base[rng.integers(0, 50, 90)]
    x, y = (x.astype(np.int32), y.astype(np.int32)) if is_int else (x.astype(np.float32), y.astype(np.float32))
    for p in (1.0, 2.0, 0.5):
        assert_bits(host(x, y, p, k), bo.nn_bruteforce(x, y, p, k, is_int))


@pytest.mark.parametrize("is_int", [False, True])
@pytest.mark.parametrize("k", [1, 2, 5, 64])
def test_edges(is_int, k):
    rng = np.random.default_rng([k, is_int, 7])
    for xrows in sorted({0, 1, max(k - 1, 0), k, k + 33}):
        for yrows in (0, 1, 257):
            x, y = data(rng, xrows, 19, is_int), data(rng, yrows, 19, is_int)
            gi, gd = host(x, y, 2.0, k)
            assert gi.shape == (yrows, k)
            assert_bits((gi, gd), bo.nn_bruteforce(x, y, 2.0, k, is_int))


def test_slice_merge_path():
    """~300k database rows x 2k queries: the automatic plan cuts the database into hundreds of
    slices, and the merge kernel selects among them."""
    from spectavi_amd import feature
    rng = np.random.default_rng(300)
    x = rng.integers(-8, 8, (300_007, 6)).astype(np.float32)
    y = rng.integers(-8, 8, (2048, 6)).astype(np.float32)
    for p, k in ((2.0, 3), (1.0, 8)):
        got = feature.nn_bruteforce(x, y, p=p, k=k)
        assert_bits(got, bo.nn_bruteforce(x, y, p, k, chunk=64))


@pytest.mark.parametrize("p, is_int, k", GENERAL_CASES)
def test_general_p(p, is_int, k):
    """Device pow vs glibc pow may differ by an ulp of the double: distances within a relative
    1e-6 * dim (int rows: plus one unit per column, where the truncation of a pow result an ulp
    below an integer drops it by one); indices equal except where neighbouring oracle distances are
    that close."""
    dim = 40
    rng = np.random.default_rng([int(p * 2), is_int, k])
    x, y = data(rng, 500, dim, is_int, -20, 20), data(rng, 200, dim, is_int, -20, 20)
    gi, gd = host(x, y, p, k)
    wi, wd = bo.nn_bruteforce(x, y, p, k + 1, is_int)
    tol, units = 1e-6 * dim, (dim if is_int else 0)
    wd64 = wd.astype(np.float64)
    close = np.abs(gd.astype(np.float64) - wd64[:, :k]) <= tol * np.maximum(np.abs(wd64[:, :k]), 1) + units
    assert close.all()
    ambiguous = np.abs(wd64[:, k - 1] - wd64[:, k]) <= 2 * (tol * np.maximum(np.abs(wd64[:, k]), 1) + units)
    # a near tie anywhere in the first k can swap two entries; compare the sets there, exactly elsewhere
    near = np.zeros(len(gi), bool)
    for j in range(k):
        near |= np.abs(wd64[:, j] - wd64[:, j + 1]) <= 2 * (tol * np.maximum(np.abs(wd64[:, j + 1]), 1) + units)
    exact = ~near
    assert np.array_equal(gi[exact], wi[exact, :k])
    for i in np.flatnonzero(near & ~ambiguous):
        assert set(gi[i].tolist()) == set(wi[i, :k].tolist())


def test_use_int_frontend():
    from spectavi_amd import feature
    rng = np.random.default_rng(11)
    x = rng.standard_normal((400, 33)).astype(np.float32)
    y = rng.standard_normal((150, 33)).astype(np.float32)
    xi, yi = np.round(100 * x).astype("int32"), np.round(100 * y).astype("int32")
    for p in (1.0, 2.0, 0.5):
        got = feature.nn_bruteforce(x, y, p=p, k=4, use_int=True)
        assert got[1].dtype == np.int32
        assert_bits(got, bo.nn_bruteforce(xi, yi, p, 4, is_int=True))


def test_mu_is_ignored():
    from spectavi_amd import feature
    rng = np.random.default_rng(12)
    x = rng.standard_normal((500, 20)).astype(np.float32)
    y = rng.standard_normal((100, 20)).astype(np.float32)
    ref = feature.nn_bruteforce(x, y, p=2, mu=0.0, k=5)
    for mu in (0.5, -1.0):
        assert_bits(feature.nn_bruteforce(x, y, p=2, mu=mu, k=5), ref)


@pytest.mark.parametrize("is_int", [False, True])
def test_device_path_and_plan_independence(is_int):
    import torch
    from spectavi_amd import device
    rng = np.random.default_rng([13, is_int])
    x, y = data(rng, 5000, 37, is_int), data(rng, 700, 37, is_int)
    want = host(x, y, 2.0, 6)
    tx, ty = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for slices in (0, 1, 2, 7, 300):
        i, d = device.bruteforce(tx, ty, k=6, p=2.0, slices=slices)
        torch.cuda.synchronize()
        assert_bits((i.cpu().numpy().view(np.uint64), d.cpu().numpy()), want)


def test_bad_arguments_through_the_c_abi():
    import torch
    from spectavi_amd import feature
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    from spectavi_amd.ndarray import NdArray
    x = np.zeros((8, 4), np.float32)
    xi = np.zeros((8, 4), np.int32)
    for (k, p, dim) in ((0, 2.0, 4), (65, 2.0, 4), (2, 0.0, 4), (2, float("nan"), 4), (2, 2.0, 2049), (2, 2.0, 0)):
        oi, od = NdArray(dtype="uint64"), NdArray(dtype="float32")
        feature._nn_bruteforce(x, x, 8, 8, dim, k, p, 0.0, ct.byref(oi), ct.byref(od))
        assert clib.spv_last_status() == SPV_ERR_INVALID and not oi.m_data
        oi, od = NdArray(dtype="uint64"), NdArray(dtype="int32")
        feature._nn_bruteforcei(xi, xi, 8, 8, dim, k, p, 0.0, ct.byref(oi), ct.byref(od))
        assert clib.spv_last_status() == SPV_ERR_INVALID and not oi.m_data
    dev = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    idx = torch.zeros((64, 2), dtype=torch.int64, device="cuda")
    dist = torch.zeros((64, 2), dtype=torch.float32, device="cuda")
    f = clib.spv_bruteforce_device
    s = ct.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.zeros(8, dtype=torch.uint8, device="cuda")
    # workspace too small, misaligned idx, negative slices, absurd forced slices
    assert f(dev.data_ptr(), dev.data_ptr(), 0, 64, 64, 4, 2, 2.0, 0, idx.data_ptr(), dist.data_ptr(),
             ws.data_ptr(), 8, s) == SPV_ERR_INVALID
    big = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    assert f(dev.data_ptr(), dev.data_ptr(), 0, 64, 64, 4, 2, 2.0, 0, idx.data_ptr() + 4, dist.data_ptr(),
             big.data_ptr(), big.numel(), s) == SPV_ERR_INVALID
    assert f(dev.data_ptr(), dev.data_ptr(), 0, 64, 64, 4, 2, 2.0, -1, idx.data_ptr(), dist.data_ptr(),
             big.data_ptr(), big.numel(), s) == SPV_ERR_INVALID
    assert f(dev.data_ptr(), dev.data_ptr(), 0, 64, 64, 4, 2, 2.0, 64, idx.data_ptr(), dist.data_ptr(),
             big.data_ptr(), 64 * 64 * 2 * 8 - 8, s) == SPV_ERR_INVALID
    torch.cuda.synchronize()
    # and a good call still works afterwards
    assert f(dev.data_ptr(), dev.data_ptr(), 0, 64, 64, 4, 2, 2.0, 0, idx.data_ptr(), dist.data_ptr(),
             big.data_ptr(), big.numel(), s) == 0
    torch.cuda.synchronize()
    assert (dist == 0).all()
