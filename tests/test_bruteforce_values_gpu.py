"""nn_bruteforce / nn_bruteforcei on the GPU over the whole finite float32 and int32 value domain of the
contract: the named classes of tests/bruteforce_value_cases.py (overflow to +inf, subnormal differences
and products, absorbed terms, signed zeros, int differences and terms past 2**24) through the host entry
and the device entry at several slice counts, indices and distance bits equal to
tests/bruteforce_oracle.py.  tests/test_bruteforce_oracle.py shows on the CPU that these classes tell
exact-integer int terms, flushed subnormals and "+inf means none" apart from the contract."""
import numpy as np
import pytest

from tests import bruteforce_oracle as bo
from tests import bruteforce_value_cases as vc
from tests.test_bruteforce_gpu import assert_bits, host

pytestmark = pytest.mark.gpu

INF_BITS = 0x7F800000


def device_entry(x, y, p, k, slices):
    import torch
    from spectavi_amd import device
    # a workspace of its own: exactly the bytes the header asks for, not what an earlier call left behind
    i, d = device.bruteforce(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), k=k, p=p, slices=slices,
                             workspace=device.Workspace())
    torch.cuda.synchronize()
    return i.cpu().numpy().view(np.uint64), d.cpu().numpy()


def test_case_table_reaches_every_instantiation():
    assert vc.REACHED == vc.EXACT_INSTANTIATIONS


@pytest.mark.parametrize("case", vc.CASES, ids=vc.case_id)
def test_value_case(case):
    x, y = vc.case_data(case)
    want = bo.nn_bruteforce(x, y, case.p, case.k, case.is_int)
    assert_bits(host(x, y, case.p, case.k), want)
    first = None
    for slices in (0, 1, 3):
        got = device_entry(x, y, case.p, case.k, slices)
        assert_bits(got, want)
        both = got[0].tobytes() + got[1].tobytes()
        first = first or both
        assert both == first   # the slice count changes no byte


@pytest.mark.parametrize("k", [2, 17])
@pytest.mark.parametrize("cls", ["max", "zeros"])
def test_short_database(cls, k):
    """Fewer database rows than k on `max` (every real neighbour at +inf, ahead of the missing ones, which
    differ from them in idx alone) and on `zeros` (all tied at +0)."""
    dim = vc.BY_NAME[cls].dims[0]
    for xrows in sorted({0, 1, k - 1, k}):
        x, y = vc.make(cls, dim, xrows=xrows)
        for p in (2.0, 1.0):
            wi, wd = bo.nn_bruteforce(x, y, p, k)
            n = min(xrows, k)
            assert (wi[:, n:] == bo.NONE_IDX).all() and (wd[:, n:].view(np.uint32) == INF_BITS).all()
            if cls == "zeros" or p == 2.0:   # all real neighbours tied, at +0 or at +inf: ascending idx
                assert np.array_equal(wi[:, :n], np.tile(np.arange(n, dtype=np.uint64), (len(y), 1)))
                assert (wd[:, :n].view(np.uint32) == (INF_BITS if cls == "max" else 0)).all()
            assert_bits(host(x, y, p, k), (wi, wd))
            for slices in (0, 3):
                assert_bits(device_entry(x, y, p, k, slices), (wi, wd))


def zeros_heavy(rng, rows_x, rows_y, dim, is_int):
    """randn (ints in [-20, 20)) with half of the coordinates made equal between every query and every
    database row: a random half of the columns is constant, so pow(0, p) = 0 terms occur in every sum, and
    some queries are copies of database rows, so distances of exactly 0 occur."""
    if is_int:
        a = rng.integers(-20, 20, (rows_x + rows_y, dim)).astype(np.int32)
    else:
        a = rng.standard_normal((rows_x + rows_y, dim)).astype(np.float32)
    same = rng.random(dim) < 0.5
    a[:, same] = a[0, same]
    x, y = np.ascontiguousarray(a[:rows_x]), np.ascontiguousarray(a[rows_x:])
    y[::5] = x[rng.integers(0, rows_x, len(y[::5]))]
    return x, y


def check_general_p(x, y, p, k, is_int):
    """The rule of test_bruteforce_gpu.py::test_general_p, unchanged, plus: where the oracle's distance is
    exactly 0 or +inf the device's has the same bits."""
    dim = x.shape[1]
    gi, gd = host(x, y, p, k)
    wi, wd = bo.nn_bruteforce(x, y, p, k + 1, is_int)
    pinned = (wd[:, :k] == 0) if is_int else ((wd[:, :k] == 0) | np.isposinf(wd[:, :k]))
    assert np.array_equal(gd.view(np.uint32)[pinned], wd[:, :k].view(np.uint32)[pinned])
    tol, units = 1e-6 * dim, (dim if is_int else 0)
    wd64 = wd.astype(np.float64)
    with np.errstate(invalid="ignore"):   # inf - inf = nan compares false: such rows count as exact below
        close = np.abs(gd.astype(np.float64) - wd64[:, :k]) <= tol * np.maximum(np.abs(wd64[:, :k]), 1) + units
        assert (close | pinned).all()
        ambiguous = np.abs(wd64[:, k - 1] - wd64[:, k]) <= 2 * (tol * np.maximum(np.abs(wd64[:, k]), 1) + units)
        near = np.zeros(len(gi), bool)
        for j in range(k):
            near |= np.abs(wd64[:, j] - wd64[:, j + 1]) <= 2 * (tol * np.maximum(np.abs(wd64[:, j + 1]), 1) + units)
    exact = ~near
    assert np.array_equal(gi[exact], wi[exact, :k])
    for i in np.flatnonzero(near & ~ambiguous):
        assert set(gi[i].tolist()) == set(wi[i, :k].tolist())
    return int(pinned.sum()), int(exact.sum())


@pytest.mark.parametrize("k", [2, 5, 20])
@pytest.mark.parametrize("is_int", [False, True])
@pytest.mark.parametrize("p", [1.5, 3.0])
def test_general_p_on_zero_terms(p, is_int, k):
    rng = np.random.default_rng([int(p * 2), is_int, k, 3])
    x, y = zeros_heavy(rng, vc.XROWS, vc.YROWS, 40, is_int)
    pinned, exact = check_general_p(x, y, p, k, is_int)
    assert pinned >= len(y[::5])   # the copied rows are found at distance 0


@pytest.mark.parametrize("k", [2, 5, 20])
@pytest.mark.parametrize("p", [1.5, 3.0])
def test_general_p_on_huge(p, k):
    """|d| ~ 1e19: at p = 3 every term is float(1e57) = +inf; at p = 1.5 the terms are ~ 1e28 and finite."""
    x, y = vc.make("huge", 40)
    pinned, exact = check_general_p(x, y, p, k, False)
    assert pinned == (len(y) * k if p == 3.0 else 0)
    if p == 3.0:   # all tied at +inf: equal bits, so the lower index wins
        assert exact == len(y)


def test_forced_slices_need_only_the_documented_workspace():
    """spv_bruteforce_device with slices > 0 asks for max(spv_bruteforce_workspace_bytes, yrows * slices * k * 8)
    bytes (include/spectavi_amd.h): a buffer of exactly that size, here not a multiple of 256, is accepted."""
    import torch
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    x, y = vc.make("offset", 4)
    k, slices = 17, 3
    need = max(clib.spv_bruteforce_workspace_bytes(len(x), len(y), 4, k), len(y) * slices * k * 8)
    assert need == len(y) * slices * k * 8 and need % 256
    ws = device.Workspace()
    i, d = device.bruteforce(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), k=k, p=2.0, slices=slices, workspace=ws)
    torch.cuda.synchronize()
    assert ws.get(0, i.device).numel() == need
    assert_bits((i.cpu().numpy().view(np.uint64), d.cpu().numpy()), bo.nn_bruteforce(x, y, 2.0, k))
