"""CPU only: the exact p-norm k-NN entry points exist with the reference's signatures, and every
limit of the contract is refused before a device is touched."""
import ctypes as ct
import inspect
import math

import numpy as np
import pytest


def test_symbols_are_exported():
    from spectavi_amd._lib import clib
    for name in ("nn_bruteforce", "nn_bruteforcei", "spv_nn_bruteforce", "spv_bruteforce_device",
                 "spv_bruteforce_workspace_bytes"):
        assert hasattr(clib, name), name


def test_reference_argtypes_and_signature():
    from spectavi_amd import feature
    assert len(feature._nn_bruteforce.argtypes) == 10
    assert len(feature._nn_bruteforcei.argtypes) == 10
    assert feature._nn_bruteforce.argtypes[6] is ct.c_float and feature._nn_bruteforce.argtypes[7] is ct.c_float
    sig = inspect.signature(feature.nn_bruteforce)
    assert [(n, q.default) for n, q in sig.parameters.items()] == [
        ("x", inspect._empty), ("y", inspect._empty), ("p", 0.5), ("mu", 0.0), ("k", 2), ("use_int", False)]


@pytest.mark.parametrize("kw, shapes", [
    (dict(k=0), ((4, 8), (3, 8))),
    (dict(k=65), ((4, 8), (3, 8))),
    (dict(p=0.0), ((4, 8), (3, 8))),
    (dict(p=-1.0), ((4, 8), (3, 8))),
    (dict(p=math.nan), ((4, 8), (3, 8))),
    (dict(p=math.inf), ((4, 8), (3, 8))),
    (dict(p=1e-50), ((4, 8), (3, 8))),  # 0 as the C float the library receives
    (dict(), ((4, 2049), (3, 2049))),
    (dict(), ((4, 0), (3, 0))),
    (dict(), ((4, 8), (3, 9))),
    (dict(use_int=True, k=0), ((4, 8), (3, 8))),
])
def test_frontend_limits_raise_value_error(kw, shapes):
    from spectavi_amd import feature
    x = np.zeros(shapes[0], np.float32)
    y = np.zeros(shapes[1], np.float32)
    with pytest.raises(ValueError):
        feature.nn_bruteforce(x, y, **kw)


def test_c_abi_refuses_bad_arguments_without_a_device():
    """spv_nn_bruteforce checks the limits before it selects a device: SPV_ERR_INVALID here even
    without a GPU; the workspace query answers 0 for a refused shape."""
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    f = clib.spv_nn_bruteforce
    x = np.zeros((4, 8), np.float32)
    idx = np.zeros((4, 64), np.uint64)
    dist = np.zeros((4, 64), np.float32)
    for (xr, yr, dim, k, p) in ((4, 4, 8, 0, 2.0), (4, 4, 8, 65, 2.0), (4, 4, 0, 2, 2.0), (4, 4, 2049, 2, 2.0),
                                (4, 4, 8, 2, 0.0), (4, 4, 8, 2, -2.0), (4, 4, 8, 2, math.nan),
                                (4, 4, 8, 2, math.inf), (-1, 4, 8, 2, 2.0), (4, -1, 8, 2, 2.0)):
        for is_int in (0, 1):
            assert f(x.ctypes.data, x.ctypes.data, is_int, xr, yr, dim, k, p, idx.ctypes.data,
                     dist.ctypes.data) == SPV_ERR_INVALID, (xr, yr, dim, k, p)
    assert f(x.ctypes.data, None, 0, 4, 4, 8, 2, 2.0, idx.ctypes.data, dist.ctypes.data) == SPV_ERR_INVALID
    # yrows = 0 is a valid empty call: nothing to compute, no device needed
    assert f(None, None, 0, 0, 0, 8, 2, 2.0, None, None) == 0
    ws = clib.spv_bruteforce_workspace_bytes
    assert ws(100, 100, 8, 0) == 0 and ws(100, 100, 2049, 2) == 0
    assert ws(100, 100, 8, 2) >= 100 * 2 * 8


def test_reference_symbol_leaves_outputs_unallocated_on_bad_arguments():
    from spectavi_amd import feature
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    from spectavi_amd.ndarray import NdArray
    x = np.zeros((4, 8), np.float32)
    oi, od = NdArray(dtype="uint64"), NdArray(dtype="float32")
    feature._nn_bruteforce(x, x, 4, 4, 8, 0, 2.0, 0.0, ct.byref(oi), ct.byref(od))
    assert clib.spv_last_status() == SPV_ERR_INVALID and not oi.m_data and not od.m_data
