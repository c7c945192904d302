"""CPU-only: the approximate L2 k-NN (ann_hnswlib / spv_ann_l2*) and the k-medians exports are declared,
exported and prototyped; the reference's front-end signatures hold; spv_ann_l2_plan answers without a
device and rejects what the header rejects; the Python argument checks raise before any device work."""
import ctypes as ct
import inspect

import numpy as np
import pytest

NEW_SYMBOLS = ("ann_hnswlib", "nn_kmedians", "kmedians", "spv_ann_l2", "spv_ann_l2_workspace_bytes",
               "spv_ann_l2_plan", "spv_ann_l2_device")


def plan(xrows, yrows, dim, k, ncand=0, slices=0, fill=-7):
    from spectavi_amd._lib import clib
    out = (ct.c_int * 8)(*([fill] * 8))
    return clib.spv_ann_l2_plan(xrows, yrows, dim, k, ncand, slices, out), list(out)


def test_symbols_are_declared_exported_and_prototyped():
    from spectavi_amd._lib import clib
    from spectavi_amd._proto import PROTOTYPES
    from tests.test_abi import declared_prototypes, mismatches
    decls = declared_prototypes()
    for name in NEW_SYMBOLS:
        assert name in decls, "%s is not declared in include/spectavi_amd.h" % name
        assert name in PROTOTYPES and not mismatches(PROTOTYPES[name], decls[name]), name
        assert hasattr(clib, name), "libspectavi.so does not export %s" % name


def test_frontend_signatures_are_the_references():
    from spectavi_amd import feature

    def sig(fn):
        ps = inspect.signature(fn).parameters
        return list(ps), [p.default for p in ps.values() if p.default is not inspect._empty]

    assert sig(feature.ann_hnswlib) == (["x", "y", "k"], [2])              # reference spectavi/feature.py:172
    assert sig(feature.nn_kmedians) == (["x", "y", "k", "c"], [5])         # reference spectavi/feature.py:328
    assert sig(feature.ann_l2) == (["x", "y", "k", "ncand", "return_dist"], [2, 0, False])
    assert len(feature._ann_hnswlib.argtypes) == 7 and len(feature._nn_kmedians.argtypes) == 11


def test_plan_is_host_only_and_reports_the_launch():
    from spectavi_amd import device
    st, out = plan(131072, 131072, 128, 2)
    assert st == 0
    kpad, qtile, rtile, slices, slice_rows, ncand, buflen, mfma = out
    assert kpad == 128 and ncand == 16 and mfma in (16, 32)
    assert qtile > 0 and rtile > 0 and slice_rows % rtile == 0 and slices * slice_rows >= 131072
    assert buflen >= ncand + 32    # room for the survivors of one sub-tile past the kept keys
    assert plan(1000, 10, 33, 2)[1][0] == 64 and plan(1000, 10, 2048, 2)[1][0] == 2048   # K padded to the MFMA's
    assert plan(1000, 10, 16, 2, slices=7)[1][3:5] == [7, 143]
    assert device.ann_l2_plan(1000, 10, 16, slices=7)["slices"] == 7


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 16, 64])
def test_default_ncand_is_max_16_4k(k):
    assert plan(1000, 10, 16, k)[1][5] == max(16, 4 * k)
    assert plan(1000, 10, 16, k, ncand=k)[1][5] == k and plan(1000, 10, 16, k, ncand=256)[1][5] == 256


@pytest.mark.parametrize("args", [dict(k=0), dict(k=65), dict(k=8, ncand=7), dict(k=8, ncand=257), dict(dim=0),
                                  dict(dim=2049), dict(xrows=-1), dict(yrows=-1), dict(slices=-1)])
def test_plan_rejects_what_the_header_rejects(args):
    from spectavi_amd._lib import clib
    a = dict(xrows=1000, yrows=10, dim=16, k=2, ncand=0, slices=0)
    a.update(args)
    st, out = plan(**a)
    assert st == 1 and out == [-7] * 8          # SPV_ERR_INVALID, out untouched
    assert clib.spv_last_status() == 1
    if "slices" not in args:
        assert clib.spv_ann_l2_workspace_bytes(a["xrows"], a["yrows"], a["dim"], a["k"], a["ncand"]) == 0


def test_workspace_covers_the_plan():
    from spectavi_amd._lib import clib
    kpad, _, _, slices, _, ncand, buflen, _ = plan(5000, 300, 100, 2)[1]
    need = 5000 * kpad * 2 + 300 * kpad * 2 + 5000 * 4 + 300 * slices * (buflen * 8 + 4) + 300 * ncand * 4
    assert clib.spv_ann_l2_workspace_bytes(5000, 300, 100, 2, 0) >= need
    assert clib.spv_ann_l2_workspace_bytes(16, 300, 100, 2, 0) == 0   # every row is a candidate: the re-rank alone


def test_python_checks_raise_before_any_device_work():
    from spectavi_amd import feature
    x, y = np.zeros((40, 8), np.float32), np.zeros((4, 8), np.float32)
    for bad in (dict(k=0), dict(k=65), dict(k=2.5)):
        with pytest.raises(ValueError):
            feature.ann_hnswlib(x, y, **bad)
    for bad in (dict(k=8, ncand=7), dict(k=2, ncand=257), dict(k=2, ncand=-1), dict(k=2, ncand=16.5)):
        with pytest.raises(ValueError):
            feature.ann_l2(x, y, **bad)
    for xs, ys in (((40, 8), (4, 9)), ((40,), (4, 8)), ((40, 0), (4, 0)), ((40, 2049), (4, 2049))):
        with pytest.raises(ValueError):
            feature.check_ann_args(xs, ys, 2)
        with pytest.raises(ValueError):
            feature.ann_hnswlib(np.zeros(xs, np.float32), np.zeros(ys, np.float32))
    with pytest.raises(ValueError):
        feature.nn_kmedians(x, y, 65)
    with pytest.raises(ValueError):
        feature.nn_kmedians(x, np.zeros((4, 9), np.float32), 2)
    feature.check_ann_args((40, 8), (4, 8), 2, 0)
    feature.check_ann_args((40, 8), (4, 8), 64, 256)


def test_device_front_end_checks_raise_before_any_device_work():
    import torch
    from spectavi_amd import device
    x = torch.zeros((40, 8), dtype=torch.float32)
    with pytest.raises(TypeError):      # not on a GPU
        device.ann_l2(x, x)


def test_kmedians_validates_and_returns():
    from spectavi_amd._lib import clib
    x = np.zeros((10, 4), np.float32)
    clib.kmedians(x, 10, 4, 3)
    assert clib.spv_last_status() == 0
    for bad in ((-1, 4, 3), (10, 0, 3), (10, 4, 0)):
        clib.kmedians(x, *bad)
        assert clib.spv_last_status() == 1
    clib.kmedians(x, 10, 4, 3)
    assert clib.spv_last_status() == 0
