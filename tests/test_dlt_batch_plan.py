"""Host only: the work items of dlt_triangulate_batch (spv_dlt_triangulate_batch_plan) and the argument checks of its
entry points that run before any device is touched.  No GPU involved."""
import ctypes as ct

import numpy as np
import pytest

SIZES = [0, 1, 255, 256, 257, 0, 600]
USE = [1, 1, 1, 0, 1, 1, 1]


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def test_items_cover_every_used_row_once_in_order():
    from spectavi_amd import device
    off = _off(SIZES)
    plan, items = device.dlt_triangulate_batch_plan(off, USE, want_items=True)
    used_rows = sum(n for n, u in zip(SIZES, USE) if u)
    assert plan == dict(sets=6, items=len(items), bound=used_rows)
    assert items.dtype == np.int32 and items.shape[1] == 4
    # blocks of 256 per used set: 0, 1, 1, (skipped), 2, 0, 3
    assert [int((items[:, 0] == p).sum()) for p in range(len(SIZES))] == [0, 1, 1, 0, 2, 0, 3]
    covered, base = [], 0
    for s, row0, rows, out in items.tolist():
        assert USE[s] and 1 <= rows <= 256
        assert off[s] <= row0 and row0 + rows <= off[s + 1], "an item spans two sets"
        assert out == base, "the out bases are the running sum"
        base += rows
        covered.extend(range(row0, row0 + rows))
    want = [r for p, u in enumerate(USE) if u for r in range(off[p], off[p + 1])]
    assert covered == want
    assert base == used_rows
    # the items do not depend on the compute units; use = None takes every set
    _, again = device.dlt_triangulate_batch_plan(off, USE, compute_units=3, want_items=True)
    assert np.array_equal(items, again)
    plan_all, items_all = device.dlt_triangulate_batch_plan(off, want_items=True)
    assert plan_all == dict(sets=7, items=8, bound=sum(SIZES))
    assert int((items_all[:, 0] == 3).sum()) == 1 and items_all[-1].tolist() == [6, int(off[6]) + 512, 88, sum(SIZES) - 88]
    # a short items buffer receives the first items only
    from spectavi_amd._lib import clib
    out = (ct.c_longlong * 3)()
    few = np.full((3, 4), -5, np.int32)
    use = np.array(USE, np.int32)
    assert clib.spv_dlt_triangulate_batch_plan(off.ctypes.data, len(SIZES), use.ctypes.data, 256, out, few.ctypes.data, 2) == 0
    assert np.array_equal(few[:2], items[:2]) and few[2].tolist() == [-5] * 4


def test_empty_collections_are_valid():
    from spectavi_amd import device
    assert device.dlt_triangulate_batch_plan([0]) == dict(sets=0, items=0, bound=0)
    assert device.dlt_triangulate_batch_plan([0, 0, 0]) == dict(sets=2, items=0, bound=0)
    assert device.dlt_triangulate_batch_plan(_off(SIZES), [0] * len(SIZES)) == dict(sets=0, items=0, bound=0)


def test_plan_rejects_bad_arguments_and_leaves_out_untouched():
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    good = _off(SIZES)
    cases = [
        (good + 1, len(SIZES), 256, True, 0),                                      # does not start at 0
        (np.array([0, 5, 4, 9], np.int64), 3, 256, True, 0),                       # decreases
        (np.array([0, 2 ** 31], np.int64), 1, 256, True, 0),                       # 2^31 rows
        (good, -1, 256, True, 0),                                                  # negative set count
        (good, 2 ** 20 + 1, 256, True, 0),                                         # too many sets (pair_off is not read)
        (None, 1, 256, True, 0),                                                   # no pair_off
        (good, len(SIZES), 0, True, 0),                                            # no compute unit
        (good, len(SIZES), 256, False, 0),                                         # no out
        (good, len(SIZES), 256, True, -1),                                         # negative items_cap
    ]
    for off, npairs, cus, with_out, cap in cases:
        out = (ct.c_longlong * 3)(-7, -7, -7)
        items = np.full((4, 4), -5, np.int32)
        st = clib.spv_dlt_triangulate_batch_plan(off.ctypes.data if off is not None else None, npairs, None, cus,
                                                 out if with_out else None, items.ctypes.data, cap)
        assert st == SPV_ERR_INVALID, (npairs, cus, with_out, cap)
        assert clib.spv_last_error()
        assert list(out) == [-7] * 3 and np.all(items == -5)


def test_call_rejects_bad_arguments_before_any_device():
    """The host and the device form: SPV_ERR_INVALID with the outputs untouched, on a machine with or without a
    GPU -- the checks come first."""
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    off = _off([3, 2])
    x = np.zeros((5, 3))
    P = np.zeros((2, 12))
    X = np.full((5, 4), -3.0)
    err = np.full(5, -3.0)
    oo = np.full(3, -9, np.int64)
    cnt = ct.c_longlong(-9)

    def host(x0=x, x1=x, off=off, npairs=2, P1s=P, X=X, err=err, cap=5):
        return clib.spv_dlt_triangulate_batch(
            x0.ctypes.data if x0 is not None else None, x1.ctypes.data if x1 is not None else None,
            off.ctypes.data if off is not None else None, npairs, None, P1s.ctypes.data if P1s is not None else None,
            None, None, X.ctypes.data if X is not None else None, err.ctypes.data if err is not None else None, None, cap,
            oo.ctypes.data, ct.addressof(cnt))

    def dev(x0=x, x1=x, off=off, npairs=2, P1s=P, X=X, err=err, cap=5):
        # (host arrays stand in for device memory: the call must not get as far as touching them)
        return clib.spv_dlt_triangulate_batch_device(
            x0.ctypes.data if x0 is not None else None, x1.ctypes.data if x1 is not None else None,
            off.ctypes.data if off is not None else None, npairs, None, P1s.ctypes.data if P1s is not None else None,
            None, None, X.ctypes.data if X is not None else None, err.ctypes.data if err is not None else None, None, cap,
            None, None, None)

    for call in (host, dev):
        for kw in (dict(x0=None), dict(x1=None), dict(off=None), dict(P1s=None), dict(X=None, err=None), dict(cap=-1),
                   dict(npairs=-1), dict(off=off + 1), dict(off=np.array([0, 4, 3], np.int64)),
                   dict(off=np.array([0, 1, 2 ** 31], np.int64))):
            assert call(**kw) == SPV_ERR_INVALID, (call.__name__, sorted(kw))
            assert clib.spv_last_error()
    assert np.all(X == -3.0) and np.all(err == -3.0) and np.all(oo == -9) and cnt.value == -9


def test_python_wrappers_mirror_the_checks():
    from spectavi_amd import device, mvg
    P = np.zeros((3, 4))
    x = np.zeros((4, 3))
    with pytest.raises(ValueError):
        mvg.dlt_triangulate_batch([P], [x, x], [x, x])
    with pytest.raises(TypeError):
        mvg.dlt_triangulate_batch([P], [x], [np.zeros((5, 3))])
    with pytest.raises(TypeError):
        mvg.dlt_triangulate_batch([P], [np.zeros((4, 2))], [np.zeros((4, 2))])
    with pytest.raises(TypeError):
        mvg.dlt_triangulate_batch([np.zeros((4, 4))], [x], [x])
    with pytest.raises(ValueError):
        mvg.dlt_triangulate_batch([P], [x], [x], masks=[np.ones(3)])
    with pytest.raises(ValueError):
        mvg.dlt_triangulate_batch([P], [x], [x], P0s=[P, P])
    # nothing to solve: no device is touched, one empty array per set
    Xs, Es = mvg.dlt_triangulate_batch([None, P], [x, x[:0]], [x, x[:0]], ret_error=True)
    assert [a.shape for a in Xs] == [(0, 4), (0, 4)] and [e.shape for e in Es] == [(0, 1), (0, 1)]
    assert mvg.dlt_triangulate_batch([], [], []) == []
    from spectavi_amd._lib import SpectaviError
    with pytest.raises(SpectaviError):
        device.dlt_triangulate_batch_plan([1, 2])
    with pytest.raises(ValueError):
        device.dlt_triangulate_batch_plan([0, 2], use=[1, 1])
