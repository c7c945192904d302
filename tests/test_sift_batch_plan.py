"""Host only: how sift_batch cuts its images into groups (spv_sift_batch_plan), its workspace sizes and the
argument checks that run before any device is touched.  No GPU involved."""
import ctypes as ct
import os

import numpy as np
import pytest

from spectavi_amd._lib import SPV_ERR_INVALID, SPV_OK

# (wid, hgt): ragged, the most demanding image in the middle
SIZES = [(21, 15), (310, 233), (32, 45), (640, 480), (40, 1), (3, 2), (128, 96), (129, 127)]
NEW = ["spv_sift_batch_plan", "spv_sift_batch_workspace_bytes", "spv_sift_batch_device", "spv_sift_batch_pack_device",
       "spv_sift_tables"]


@pytest.fixture(scope="module")
def clib():
    from spectavi_amd._lib import clib
    return clib


def _sizes(sizes):
    return np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(-1, 2))


def _plan(clib, sizes, ws_bytes=0):
    """(status, out[4], groups int32[groups, 2])."""
    sz = _sizes(sizes)
    out = (ct.c_longlong * 4)(-7, -7, -7, -7)
    st = clib.spv_sift_batch_plan(sz.ctypes.data, len(sz), ws_bytes, out, None, 0)
    if st != SPV_OK:
        return st, list(out), None
    groups = np.full((out[0], 2), -5, np.int32)
    assert clib.spv_sift_batch_plan(sz.ctypes.data, len(sz), ws_bytes, out, groups.ctypes.data, len(groups)) == SPV_OK
    return st, list(out), groups


def _single(clib, sizes):
    return [clib.spv_sift_workspace_bytes(w, h) for w, h in sizes]


def test_workspace_bytes(clib):
    st, out, groups = _plan(clib, SIZES)
    single = _single(clib, SIZES)
    assert st == SPV_OK and all(single)
    assert out[1] >= sum(single) and out[2] >= max(single)
    assert out[3] == sum(w * h for w, h in SIZES)
    sz = _sizes(SIZES)
    assert clib.spv_sift_batch_workspace_bytes(sz.ctypes.data, len(sz)) == out[1]
    assert out[0] == 1 and groups.tolist() == [[0, len(SIZES)]]


def _assert_tiles(groups, nimg):
    at = 0
    for first, n in groups.tolist():
        assert first == at and n >= 1
        at += n
    assert at == nimg


def test_groups_tile_the_images_in_order(clib):
    _, out, _ = _plan(clib, SIZES)
    single = _single(clib, SIZES)
    big = int(np.argmax(single))
    # the least workspace: an image that needs all of it sits alone
    st, o, groups = _plan(clib, SIZES, out[2])
    assert st == SPV_OK and o[0] == len(groups) > 1 and o[1:] == out[1:]
    _assert_tiles(groups, len(SIZES))
    assert [big, 1] in groups.tolist()
    # all of it: one group
    st, o, groups = _plan(clib, SIZES, out[1])
    assert st == SPV_OK and groups.tolist() == [[0, len(SIZES)]]
    # in between: the group count never grows with the workspace, and every plan tiles
    counts = []
    for ws in np.linspace(out[2], out[1], 23).astype(np.int64).tolist() + [out[1] + 1, 4 * out[1]]:
        st, o, groups = _plan(clib, SIZES, ws)
        assert st == SPV_OK
        _assert_tiles(groups, len(SIZES))
        for first, n in groups.tolist():
            assert sum(single[first:first + n]) <= ws, "a group's slices exceed the workspace"
        counts.append(o[0])
    assert counts == sorted(counts, reverse=True) and counts[0] > 1 and counts[-1] == 1


def test_a_short_groups_buffer_receives_the_first_groups_only(clib):
    _, out, _ = _plan(clib, SIZES)
    _, o, groups = _plan(clib, SIZES, out[2])
    sz = _sizes(SIZES)
    few = np.full((3, 2), -5, np.int32)
    res = (ct.c_longlong * 4)()
    assert clib.spv_sift_batch_plan(sz.ctypes.data, len(sz), out[2], res, few.ctypes.data, 2) == SPV_OK
    assert np.array_equal(few[:2], groups[:2]) and few[2].tolist() == [-5, -5]


def test_group_cap_of_65535_images(clib):
    sizes = np.ones((70000, 2), np.int32)
    st, out, groups = _plan(clib, sizes)
    assert st == SPV_OK and out[0] == len(groups) >= 2
    _assert_tiles(groups, 70000)
    assert groups[:, 1].max() <= 65535
    assert out[1] >= 65535 * clib.spv_sift_workspace_bytes(1, 1) and out[3] == 70000


@pytest.mark.parametrize("what", ["side 0", "side 8193", "nimg -1", "ws_bytes below the least", "null sizes"])
def test_rejections_leave_the_outputs_untouched(clib, what):
    sizes, nimg, ws = list(SIZES), len(SIZES), 0
    if what == "side 0":
        sizes[2] = (0, 45)
    elif what == "side 8193":
        sizes[5] = (3, 8193)
    elif what == "nimg -1":
        nimg = -1
    elif what == "ws_bytes below the least":
        ws = _plan(clib, SIZES)[1][2] - 1
    sz = _sizes(sizes)
    out = (ct.c_longlong * 4)(-7, -7, -7, -7)
    groups = np.full((len(SIZES), 2), -5, np.int32)
    ptr = None if what == "null sizes" else sz.ctypes.data
    assert clib.spv_sift_batch_plan(ptr, nimg, ws, out, groups.ctypes.data, len(groups)) == SPV_ERR_INVALID
    assert list(out) == [-7] * 4 and (groups == -5).all()
    assert clib.spv_last_error()
    if ws == 0:
        assert clib.spv_sift_batch_workspace_bytes(ptr, nimg) == 0


def test_no_images(clib):
    st, out, groups = _plan(clib, np.zeros((0, 2), np.int32))
    assert st == SPV_OK and out == [0, 0, 0, 0] and len(groups) == 0
    assert clib.spv_sift_batch_workspace_bytes(None, 0) == 0
    from spectavi_amd import device
    assert device.sift_batch_plan([]) == dict(groups=0, workspace_bytes=0, min_workspace_bytes=0, pixels=0)


def test_python_plan_agrees(clib):
    from spectavi_amd import device
    _, out, _ = _plan(clib, SIZES)
    plan, groups = device.sift_batch_plan(SIZES, ws_bytes=out[2], want_groups=True)
    _, o, want = _plan(clib, SIZES, out[2])
    assert plan == dict(groups=o[0], workspace_bytes=o[1], min_workspace_bytes=o[2], pixels=o[3])
    assert np.array_equal(groups, want)
    with pytest.raises(ValueError):
        device.sift_batch_plan([(0, 4)])


def test_entry_points_reject_bad_arguments_before_any_device(clib):
    """cap_off outside the rules, NULL required pointers and sizes the plan rejects: SPV_ERR_INVALID from the device
    and host forms, which then touch no device (this test runs without one)."""
    sz = _sizes(SIZES[:3])
    good = np.array([0, 5, 5, 9], np.int64)
    one = 0x1000  # a non-null address that is never dereferenced: every call below is rejected first
    for cap in ([1, 5, 5, 9], [0, 5, 4, 9], [0, 5, 5, 2 ** 31]):
        cap = np.array(cap, np.int64)
        assert clib.spv_sift_batch_device(one, sz.ctypes.data, 3, one, 1 << 40, one, cap.ctypes.data, one, None) == SPV_ERR_INVALID
        assert clib.spv_sift_tables(one, sz.ctypes.data, 3, one, cap.ctypes.data, one) == SPV_ERR_INVALID
    for args in ((None, sz.ctypes.data, 3, one, 1 << 40, one, good.ctypes.data, one, None),
                 (one, None, 3, one, 1 << 40, one, good.ctypes.data, one, None),
                 (one, sz.ctypes.data, 3, None, 1 << 40, one, good.ctypes.data, one, None),
                 (one, sz.ctypes.data, 3, one, 1 << 40, None, good.ctypes.data, one, None),
                 (one, sz.ctypes.data, 3, one, 1 << 40, one, None, one, None),
                 (one, sz.ctypes.data, 3, one, 1 << 40, one, good.ctypes.data, None, None),
                 (one, sz.ctypes.data, 3, one, 255, one, good.ctypes.data, one, None),
                 (one, sz.ctypes.data, -1, one, 1 << 40, one, good.ctypes.data, one, None)):
        assert clib.spv_sift_batch_device(*args) == SPV_ERR_INVALID, args
    # pack: a segment longer than its capacity, a seg_off outside the rules, no output wanted
    for seg in ([0, 5, 5, 10], [0, 6, 6, 9], [1, 5, 5, 9], [0, 5, 4, 8]):
        seg = np.array(seg, np.int64)
        assert clib.spv_sift_batch_pack_device(one, good.ctypes.data, seg.ctypes.data, 3, one, one, one, None) == SPV_ERR_INVALID, seg
    assert clib.spv_sift_batch_pack_device(one, good.ctypes.data, good.ctypes.data, 3, None, None, None, None) == SPV_ERR_INVALID
    assert clib.spv_sift_batch_pack_device(None, good.ctypes.data, good.ctypes.data, 3, one, None, None, None) == SPV_ERR_INVALID
    assert clib.spv_sift_batch_pack_device(one, good.ctypes.data, good.ctypes.data, -1, one, None, None, None) == SPV_ERR_INVALID


def test_new_names_are_declared_and_exported(clib):
    from spectavi_amd import _proto
    for name in NEW:
        assert name in _proto.PROTOTYPES, name
        assert getattr(clib, name) is not None, name
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "spectavi_amd.h")).read()
    for name in ("sift_batch_pyramid", "sift_batch_detect", "sift_batch_describe", "sift_batch_pack"):
        assert '"%s"' % name in header, name
