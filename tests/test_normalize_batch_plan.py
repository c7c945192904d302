"""Host only: the work items and the workspace of normalize_batch (spv_normalize_batch_plan,
spv_normalize_batch_workspace_bytes) and the argument checks of its entry points that run before any device is
touched.  No GPU involved."""
import ctypes as ct

import numpy as np
import pytest

F32, U8 = 0, 1
ITEM_ROWS = 256  # rows per work item (include/spectavi_amd.h)
SIZES = [0, 0, 1, 255, 256, 257, 0, 0, 1500, 3, 0]  # empty sets at the start, in the middle and at the end


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _r256(n):
    return (n + 255) // 256 * 256


def layout_bytes(sizes, dim, dtype):
    """The layout the header states: 12 bytes per item, 4 + 4 per set (+ 1), float32[nseg, 2, dim], and for uint8
    4 bytes per item and column; each piece rounded up to 256."""
    nseg, nitems = len(sizes), sum((n + ITEM_ROWS - 1) // ITEM_ROWS for n in sizes)
    return (_r256(12 * nitems) + 2 * _r256(4 * (nseg + 1)) + _r256(8 * nseg * dim)
            + (_r256(4 * nitems * dim) if dtype == U8 else 0))


@pytest.mark.parametrize("dtype", [F32, U8])
def test_items_cover_every_row_once_in_order(dtype):
    from spectavi_amd import device
    off = _off(SIZES)
    name = ("float32", "uint8")[dtype]
    plan, items = device.normalize_batch_plan(off, 128, name, want_items=True)
    assert plan == dict(sets=sum(n > 0 for n in SIZES), items=len(items), workspace_bytes=layout_bytes(SIZES, 128, dtype),
                        rows=sum(SIZES))
    assert items.dtype == np.int32 and items.shape[1] == 3
    assert [int((items[:, 0] == s).sum()) for s in range(len(SIZES))] == [(n + ITEM_ROWS - 1) // ITEM_ROWS for n in SIZES]
    covered = []
    for s, row0, rows in items.tolist():
        assert 1 <= rows <= ITEM_ROWS and 0 <= row0 and row0 + rows <= SIZES[s], "an item leaves its set"
        covered.extend(range(off[s] + row0, off[s] + row0 + rows))
    assert covered == list(range(sum(SIZES))), "every row once, in order"
    # the compute units cap the grid only
    for cus in (1, 3, 304):
        plan_c, again = device.normalize_batch_plan(off, 128, name, compute_units=cus, want_items=True)
        assert plan_c == plan and np.array_equal(items, again)
    # a short items buffer receives the first items only
    from spectavi_amd._lib import clib
    out = (ct.c_longlong * 4)()
    few = np.full((3, 3), -5, np.int32)
    assert clib.spv_normalize_batch_plan(off.ctypes.data, len(SIZES), 128, dtype, 256, out, few.ctypes.data, 2) == 0
    assert np.array_equal(few[:2], items[:2]) and few[2].tolist() == [-5] * 3


def test_empty_collections_are_valid():
    from spectavi_amd import device
    for dtype, code in (("float32", F32), ("uint8", U8)):
        assert device.normalize_batch_plan([0], 128, dtype) == dict(sets=0, items=0, workspace_bytes=layout_bytes([], 128, code), rows=0)
        assert device.normalize_batch_plan([0, 0, 0], 20, dtype) == dict(sets=0, items=0, workspace_bytes=layout_bytes([0, 0], 20, code), rows=0)
    # one-row sets are the only sets a single column may have
    assert device.normalize_batch_plan([0, 1, 1, 2], 1, "uint8")["items"] == 2


def test_workspace_query_is_the_plans_and_never_shrinks():
    from spectavi_amd._lib import clib
    for dtype in (F32, U8):
        for dim in (1, 20, 128, 129, 2048):
            sizes = [1] * 5 if dim == 1 else SIZES
            off = _off(sizes)
            out = (ct.c_longlong * 4)()
            assert clib.spv_normalize_batch_plan(off.ctypes.data, len(sizes), dim, dtype, 256, out, None, 0) == 0
            got = clib.spv_normalize_batch_workspace_bytes(off.ctypes.data, len(sizes), dim, dtype)
            assert got == out[2] == layout_bytes(sizes, dim, dtype), (dtype, dim)
        # a set that grows never shrinks the workspace
        last = 0
        for n in (0, 1, 255, 256, 257, 1000, 65793, 65800, 140000):
            off = _off([3, n, 300])
            got = clib.spv_normalize_batch_workspace_bytes(off.ctypes.data, 3, 16, dtype)
            assert got >= last and got == layout_bytes([3, n, 300], 16, dtype)
            last = got
    # 0 for what the plan rejects, and no error left behind
    good = _off(SIZES)
    bad = np.array([0, 5, 4], np.int64)
    for args in ((bad.ctypes.data, 2, 128, U8), (good.ctypes.data, len(SIZES), 0, U8), (good.ctypes.data, len(SIZES), 2049, F32),
                 (good.ctypes.data, len(SIZES), 1, U8), (good.ctypes.data, len(SIZES), 128, 2), (None, 1, 128, U8),
                 (good.ctypes.data, -1, 128, F32)):
        assert clib.spv_normalize_batch_workspace_bytes(*args) == 0, args[1:]


def rejected_shapes():
    good = _off(SIZES)
    return [
        dict(off=good + 1),                                   # does not start at 0
        dict(off=np.array([0, 5, 4, 9], np.int64), nseg=3),   # decreases
        dict(off=np.array([0, 2 ** 31], np.int64), nseg=1),   # 2^31 rows
        dict(nseg=-1),                                        # negative set count
        dict(off=None, nseg=1),                               # no seg_off
        dict(dim=0), dict(dim=-3), dict(dim=2049),            # dim outside [1, 2048]
        dict(dim=1),                                          # one column, sets of more than one row
        dict(dtype=2), dict(dtype=-1),                        # unknown dtype
    ]


def test_plan_rejects_bad_arguments_and_leaves_out_untouched():
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    good = _off(SIZES)
    cases = rejected_shapes() + [dict(cus=0), dict(with_out=False), dict(cap=-1)]
    for kw in cases:
        a = dict(off=good, nseg=len(SIZES), dim=128, dtype=U8, cus=256, with_out=True, cap=0)
        a.update(kw)
        out = (ct.c_longlong * 4)(-7, -7, -7, -7)
        items = np.full((4, 3), -5, np.int32)
        st = clib.spv_normalize_batch_plan(a["off"].ctypes.data if a["off"] is not None else None, a["nseg"], a["dim"],
                                           a["dtype"], a["cus"], out if a["with_out"] else None, items.ctypes.data, a["cap"])
        assert st == SPV_ERR_INVALID, sorted(kw)
        assert clib.spv_last_error()
        assert list(out) == [-7] * 4 and np.all(items == -5)


def test_call_rejects_bad_arguments_before_any_device():
    """The host and the device form: SPV_ERR_INVALID with the outputs untouched, on a machine with or without a
    GPU -- the checks come first."""
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    sizes = [3, 0, 2]
    good = _off(sizes)
    x = np.zeros((5, 128), np.uint8)
    of = np.full((5, 128), -3.0, np.float32)
    ou = np.full((5, 128), 7, np.uint8)
    ws = np.zeros(1 << 16, np.uint8)
    assert len(ws) >= layout_bytes(sizes, 128, U8)

    def ptr(a):
        return a.ctypes.data if a is not None else None

    def host(x=x, off=good, nseg=3, dim=128, dtype=U8, of=of, ou=ou, **_):
        return clib.spv_normalize_batch(ptr(x), dtype, ptr(off), nseg, dim, ptr(of), ptr(ou))

    def dev(x=x, off=good, nseg=3, dim=128, dtype=U8, of=of, ou=ou, ws=ws, ws_bytes=len(ws), x_shift=0):
        # (host arrays stand in for device memory: the call must not get as far as touching them)
        return clib.spv_normalize_batch_device(ptr(x) + x_shift if x is not None else None, dtype, ptr(off), nseg, dim,
                                               ptr(of), ptr(ou), ptr(ws), ws_bytes, None)

    shapes = [kw for kw in rejected_shapes() if kw != dict(dim=1)] + [dict(dim=1, off=_off([1, 2, 1]))]
    for call in (host, dev):
        for kw in shapes + [dict(x=None), dict(of=None, ou=None)]:
            assert call(**kw) == SPV_ERR_INVALID, (call.__name__, sorted(kw))
            assert clib.spv_last_error()
    for kw in (dict(ws=None), dict(ws_bytes=layout_bytes(sizes, 128, U8) - 1), dict(ws_bytes=0),
               dict(dtype=F32, x_shift=2),                                       # float32 rows at an odd half-word
               dict(dtype=F32, ws_bytes=layout_bytes(sizes, 128, F32) - 1)):
        assert dev(**kw) == SPV_ERR_INVALID, sorted(kw)
        assert clib.spv_last_error()
    assert np.all(of == -3.0) and np.all(ou == 7) and not ws.any()
    # nothing to do is valid, device or not: no set, and sets without a row (x and the workspace may then be NULL)
    for call in (host, dev):
        assert call(off=_off([]), nseg=0) == 0
        assert call(off=_off([0, 0]), nseg=2, x=None, ws=None, ws_bytes=0) == 0
    assert np.all(of == -3.0) and np.all(ou == 7)


def test_python_wrappers_mirror_the_checks():
    from spectavi_amd import device, feature
    for bad in ([1, 2], [0, 3, 2], [0, 2 ** 31]):
        with pytest.raises(ValueError):
            device.normalize_batch_plan(bad, 128, "uint8")
    for dim in (0, 2049):
        with pytest.raises(ValueError):
            device.normalize_batch_plan([0, 4], dim, "uint8")
    with pytest.raises(ValueError):
        device.normalize_batch_plan([0, 1, 3], 1, "float32")
    with pytest.raises(TypeError):
        device.normalize_batch_plan([0, 4], 128, "float64")
    with pytest.raises(TypeError):
        device.normalize_batch(np.zeros((4, 16), np.uint8), [0, 4])  # not a CUDA tensor
    with pytest.raises(ValueError):
        feature.normalize_to_ubyte_and_multiple_16_dim_batch([np.zeros((2, 16), np.uint8), np.zeros((2, 16), np.float32)])
    with pytest.raises(ValueError):
        feature.normalize_to_ubyte_and_multiple_16_dim_batch([np.zeros((2, 16), np.float64)])
    with pytest.raises(ValueError):
        feature.normalize_to_ubyte_and_multiple_16_dim_batch([np.zeros((2, 16), np.uint8), np.zeros((2, 32), np.uint8)])
    # nothing to normalise: no device is touched, one empty table per set
    assert feature.normalize_to_ubyte_and_multiple_16_dim_batch([]) == []
    out = feature.normalize_to_ubyte_and_multiple_16_dim_batch([np.zeros((0, 20), np.uint8)] * 2, want_ubyte=True)
    assert [(f.shape, u.shape, f.dtype, u.dtype) for f, u in out] == [((0, 32), (0, 32), np.float32, np.uint8)] * 2
