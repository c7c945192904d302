"""spv_stereo_batch_plan and the argument rules of the stereo_batch ops: host only, no GPU.  The items cover every
sample of every used window once, out_off is the running area of all boxes, and everything include/spectavi_amd.h
lists is refused before a device is touched."""
import ctypes as ct
import os

import numpy as np
import pytest

ROWS, COLS = 4, 64  # the band and the tile of an item (include/spectavi_amd.h)

BOXES = np.array([(3, 71, 2, 117),    # 68 x 115: two tiles, the second ragged; 17 bands
                  (0, 0, 0, 0),       # empty
                  (5, 5, 0, 40),      # no rows
                  (0, 9, 7, 7),       # no columns
                  (10, 16, 0, 64),    # one tile exactly, a ragged last band
                  (0, 1, 0, 1),       # one sample
                  (0, 130, 100, 293),  # 130 x 193
                  (3, 71, 2, 117)], np.int32)
USE = [1, 1, 1, 1, 0, 1, 1, 1]


def test_out_off_and_item_cover():
    from spectavi_amd import device
    plan, items = device.stereo_batch_plan(BOXES, USE, radius=3, drange=(-5, 5), want_items=True)
    areas = (BOXES[:, 1] - BOXES[:, 0]).astype(np.int64) * (BOXES[:, 3] - BOXES[:, 2])
    assert plan["out_off"].dtype == np.int64
    assert plan["out_off"].tolist() == np.concatenate([[0], np.cumsum(areas)]).tolist()
    assert plan["samples"] == int(areas.sum()) and plan["pairs"] == 7 and plan["items"] == len(items)
    assert items.dtype == np.int32 and items.shape[1] == 4
    seen = {p: np.zeros((b[1] - b[0], b[3] - b[2]), np.int32) for p, b in enumerate(BOXES)}
    for p, row0, rows, col0 in items.tolist():
        R, C = seen[p].shape
        assert 1 <= rows <= ROWS and row0 % ROWS == 0 and col0 % COLS == 0 and row0 + rows <= R and col0 < C
        seen[p][row0:row0 + rows, col0:col0 + COLS] += 1
    for p, s in seen.items():
        want = 1 if USE[p] else 0
        assert (s == want).all(), p  # unused and empty pairs own no item
    assert set(items[:, 0].tolist()) == {0, 5, 6, 7}
    assert sorted(items[:, 0].tolist()) == items[:, 0].tolist()  # pair by pair
    # the plan is a function of the boxes and use alone
    again = device.stereo_batch_plan(BOXES, USE, radius=0, drange=None, want_items=True)[1]
    assert np.array_equal(again, items)
    assert device.stereo_batch_plan(BOXES)["pairs"] == 8
    none = device.stereo_batch_plan(np.zeros((0, 4), np.int32))
    assert none["pairs"] == 0 and none["items"] == 0 and none["samples"] == 0 and none["out_off"].tolist() == [0]


def plan_status(box, use=None, radius=0, drange=None):
    from spectavi_amd._lib import clib
    box = np.ascontiguousarray(box, np.int32).reshape(-1, 4)
    use = None if use is None else np.ascontiguousarray(use, np.int32)
    drange = None if drange is None else np.ascontiguousarray(drange, np.int32).reshape(-1, 2)
    out = (ct.c_longlong * 3)(-7, -7, -7)
    off = np.full(len(box) + 1, -7, np.int64)
    st = clib.spv_stereo_batch_plan(box.ctypes.data, len(box), None if use is None else use.ctypes.data, radius,
                                    None if drange is None else drange.ctypes.data, out, off.ctypes.data, None, 0)
    if st != 0:
        assert list(out) == [-7] * 3 and (off == -7).all() and clib.spv_last_error()
    return st


BAD = [
    ("radius -1", dict(box=[(0, 4, 0, 4)], radius=-1)),
    ("radius 8", dict(box=[(0, 4, 0, 4)], radius=8)),
    ("d_lo > d_hi", dict(box=[(0, 4, 0, 4)], drange=[(3, 2)])),
    ("d_lo below -32767", dict(box=[(0, 4, 0, 4)], drange=[(-32768, 0)])),
    ("d_hi above 32767", dict(box=[(0, 4, 0, 4)], drange=[(0, 32768)])),
    ("d_lo above 32767", dict(box=[(0, 4, 0, 4)], drange=[(40000, 40001)])),
    ("negative row_lo", dict(box=[(-1, 4, 0, 4)])),
    ("negative col_lo", dict(box=[(0, 4, -2, 4)])),
    ("inverted rows", dict(box=[(5, 4, 0, 4)])),
    ("inverted columns", dict(box=[(0, 4, 5, 4)])),
    ("inverted box of a pair that is not used", dict(box=[(0, 4, 0, 4), (0, 4, 5, 4)], use=[1, 0])),
    ("2^31 samples in one box", dict(box=[(0, 46341, 0, 46341)])),
    ("2^31 samples in all", dict(box=[(0, 32768, 0, 32768)] * 2)),
]


@pytest.mark.parametrize("what,kw", BAD, ids=[b[0] for b in BAD])
def test_plan_refusals(what, kw):
    from spectavi_amd import device
    from spectavi_amd._lib import SPV_ERR_INVALID, SpectaviError
    assert plan_status(**kw) == SPV_ERR_INVALID, what
    with pytest.raises(SpectaviError):
        device.stereo_batch_plan(kw["box"], kw.get("use"), kw.get("radius", 0), kw.get("drange"))


def test_plan_accepts_the_edges():
    assert plan_status([(0, 4, 0, 4)], radius=7, drange=[(-32767, 32767)]) == 0
    assert plan_status([(0, 4, 0, 4)], radius=0, drange=[(5, 5)]) == 0
    assert plan_status([(0, 32768, 0, 32768), (0, 32768, 0, 32767)], use=[0, 0]) == 0  # 2^31 - 32768 samples
    assert plan_status([(0, 4, 0, 4), (0, 4, 0, 4)], use=[1, 0], drange=[(0, 0), (9, -9)]) == 0  # a range that is not used


def test_device_entries_refuse_before_touching_a_device():
    """The C entries check their host arguments first: with null device pointers nothing can have been launched."""
    from spectavi_amd._lib import SPV_ERR_INVALID, clib
    box = np.array([(0, 4, 0, 4)], np.int32)
    dr = np.array([(0, 0)], np.int32)
    bad_dr = np.array([(1, 0)], np.int32)
    bad_box = np.array([(0, 4, 5, 4)], np.int32)
    sizes, pairs = np.array([(4, 4)], np.int32), np.array([(0, 0)], np.int32)

    def stereo(b, radius, d, swap=0):
        return clib.spv_stereo_batch_device(None, None, None, None, b.ctypes.data, 1, None, radius, d.ctypes.data, swap,
                                            None, None, None, None)
    assert stereo(box, 8, dr) == SPV_ERR_INVALID
    assert stereo(box, 0, bad_dr) == SPV_ERR_INVALID
    assert stereo(bad_box, 0, dr) == SPV_ERR_INVALID
    assert stereo(box, 0, dr, swap=2) == SPV_ERR_INVALID
    assert stereo(box, 0, dr) == SPV_ERR_INVALID  # null device pointers with samples to write
    keep = lambda b, tol, u: clib.spv_stereo_keep_batch_device(b.ctypes.data, 1, None, None, None, None, tol, u, None, None)
    assert keep(box, -1, 10) == SPV_ERR_INVALID
    assert keep(box, 1, 101) == SPV_ERR_INVALID
    assert keep(box, 1, -1) == SPV_ERR_INVALID
    assert keep(bad_box, 1, 10) == SPV_ERR_INVALID
    assert keep(box, 1, 10) == SPV_ERR_INVALID

    def matches(b, prs, cap=0, nimg=1):
        return clib.spv_stereo_matches_batch_device(b.ctypes.data, 1, sizes.ctypes.data, nimg, prs.ctypes.data, None, None,
                                                    None, None, cap, None, None, None, None, None)
    assert matches(box, pairs) == SPV_ERR_INVALID  # null d_pair_off
    assert matches(box, pairs, cap=-1) == SPV_ERR_INVALID
    assert matches(bad_box, pairs) == SPV_ERR_INVALID
    assert matches(box, np.array([(0, 1)], np.int32)) == SPV_ERR_INVALID


def test_wrapper_refusals():
    """What the Python wrappers refuse on their own, with tensors that never reach a device."""
    import torch
    from spectavi_amd import device
    box = [(0, 4, 0, 6)]
    u8, i32, u16 = (torch.zeros(24, dtype=t) for t in (torch.uint8, torch.int32, torch.uint16))
    with pytest.raises(ValueError):  # counts that disagree
        device._stereo_batch_args(box * 2, use=[1])
    with pytest.raises(ValueError):
        device._stereo_batch_args(box * 2, drange=[(0, 1)] * 3)
    with pytest.raises(ValueError):
        device._stereo_batch_args(box, radius=8)
    with pytest.raises(ValueError):  # no range
        device.stereo_batch(u8, u8, i32, i32, box, None)
    b, use, dr = device._stereo_batch_args(box * 3, use=[1, 0, 2], drange=(-2, 5))
    assert b.shape == (3, 4) and b.dtype == np.int32 and use.dtype == np.int32 and dr.tolist() == [[-2, 5]] * 3
    # tensors that are not on a GPU are a TypeError naming the first of them (the dtype and channel refusals need
    # tensors that are otherwise valid: test_wrappers_refuse_one_wrong_argument_at_a_time, on the GPU)
    with pytest.raises(TypeError, match="^r0 must be"):
        device.stereo_batch(u8, u8, i32, i32, box, (0, 1), radius=1)
    with pytest.raises(TypeError, match="^disp0 must be"):
        device.stereo_keep_batch(box, i32, u16, u16)
    with pytest.raises(TypeError, match="^disp0 must be"):
        device.stereo_matches_batch(box, [(6, 4)], [(0, 0)], i32, u8, i32, i32)
    with pytest.raises(ValueError):
        device.stereo_matches_batch(box, [(6, 4)], [(0, 0), (0, 0)], i32, u8, i32, i32)
    with pytest.raises(ValueError):
        device.stereo_keep_batch(box, i32, u16, u16, lr_tol=-1)
    with pytest.raises(ValueError):
        device.stereo_keep_batch(box, i32, u16, u16, uniqueness=101)


@pytest.mark.gpu
def test_wrappers_refuse_one_wrong_argument_at_a_time():
    """CUDA tensors that are valid -- the calls with them succeed -- and then one argument wrong at a time: a wrong
    dtype or a tensor that is not contiguous is a TypeError, a wrong length a ValueError, each naming the argument.
    A uint8 tensor of `samples` elements in place of the uint16 cost would be written past its end if it got through."""
    import torch
    from spectavi_amd import device
    box, n = [(0, 4, 0, 6)], 24

    def z(dt, k=n):
        return torch.zeros(k, dtype=dt, device="cuda")
    u8, i32, u16, i64, f32 = torch.uint8, torch.int32, torch.uint16, torch.int64, torch.float32

    def into(**kw):
        a = dict(r0=z(u8), r1=z(u8), ri0=z(i32), ri1=z(i32), disp=z(i32), cost=z(u16), cost2=z(u16))
        a.update(kw)
        device.stereo_batch_into(a["r0"], a["r1"], a["ri0"], a["ri1"], box, None, 1, (0, 1), 0, a["disp"], a["cost"], a["cost2"])

    def cost(**kw):
        a = dict(r0=z(u8), r1=z(u8), ri0=z(i32), ri1=z(i32))
        a.update(kw)
        return device.stereo_batch(a["r0"], a["r1"], a["ri0"], a["ri1"], box, (0, 1), radius=1)

    def keep(**kw):
        a = dict(disp0=z(i32), cost0=z(u16), cost20=z(u16), disp1=z(i32))
        a.update(kw)
        return device.stereo_keep_batch(box, a["disp0"], a["cost0"], a["cost20"], a["disp1"])

    def matches(**kw):
        a = dict(disp0=z(i32), keep=z(u8), ri0=z(i32), ri1=z(i32))
        a.update(kw)
        return device.stereo_matches_batch(box, [(6, 4)], [(0, 0)], a["disp0"], a["keep"], a["ri0"], a["ri1"])
    into()
    cost()
    keep()
    matches()
    torch.cuda.synchronize()
    strided = torch.zeros(2 * n, dtype=u8, device="cuda")[::2]
    for fn, wrong in ((into, dict(r0=z(f32), r1=z(i32), ri0=z(i64), ri1=z(u8), disp=z(i64), cost=z(u8), cost2=z(i32))),
                      (into, dict(r0=strided, cost=z(u16, 2 * n)[::2])),
                      (cost, dict(r0=z(u16), r1=z(f32), ri0=z(u8), ri1=z(i64))),
                      (keep, dict(disp0=z(i64), cost0=z(u8), cost20=z(i32), disp1=z(u16))),
                      (matches, dict(disp0=z(u8), keep=z(i32), ri0=z(i64), ri1=z(u16)))):
        for name, t in wrong.items():
            with pytest.raises(TypeError, match="^%s must be" % name):
                fn(**{name: t})
    # lengths: the rectified inputs hold one element per sample exactly, the outputs and results at least that
    for fn, names, k in ((into, ("r0", "r1"), n - 1), (into, ("r0", "r1"), n + 1), (into, ("r0", "r1"), 3 * n),
                         (cost, ("r0", "r1"), 3 * n), (cost, ("r0", "r1"), n - 1)):
        for name in names:
            with pytest.raises(ValueError, match="^%s must hold exactly" % name):
                fn(**{name: z(u8, k)})
    for fn, names, dt, k in ((into, ("ri0", "ri1"), i32, n + 1), (cost, ("ri0", "ri1"), i32, n - 1),
                             (matches, ("ri0", "ri1"), i32, n - 1), (matches, ("ri0", "ri1"), i32, n + 1)):
        for name in names:
            with pytest.raises(ValueError, match="^%s must hold exactly" % name):
                fn(**{name: z(dt, k)})
    for fn, name, dt in ((into, "disp", i32), (into, "cost", u16), (into, "cost2", u16), (keep, "disp0", i32),
                         (keep, "cost0", u16), (keep, "cost20", u16), (keep, "disp1", i32), (matches, "disp0", i32),
                         (matches, "keep", u8)):
        with pytest.raises(ValueError, match="^%s is too short" % name):
            fn(**{name: z(dt, n - 1)})
    into(disp=z(i32, n + 5), cost=z(u16, n + 1))  # longer outputs are the caller's business


@pytest.mark.gpu
def test_colour_rectification_is_refused():
    """Gray uint8 only: what rectify_batch returns for 3-channel images -- flat contiguous uint8 of samples * 3
    elements, which no dtype check can tell from gray -- is refused by its length, in both forms of the call."""
    import torch
    from spectavi_amd import device
    from spectavi_amd.scenes import plane_scene
    im0, im1, P0, P1 = plane_scene(96, 64, 1)
    rgb = [torch.from_numpy(np.ascontiguousarray(np.stack([im, im, im], 2))).cuda() for im in (im0, im1)]
    r0, r1, ri0, ri1, box, off = device.rectify_batch(rgb, None, [(0, 1)], [P1], [P0])
    n = int(off[-1])
    assert n > 0 and r0.numel() == r1.numel() == 3 * n and ri0.numel() == n and r0.dtype == torch.uint8 and r0.is_contiguous()
    with pytest.raises(ValueError, match="^r0 must hold exactly .*nchan == 1"):
        device.stereo_batch(r0, r1, ri0, ri1, box, (-24, 8), radius=3)
    gray = r0.reshape(n, 3)[:, 0].contiguous()
    with pytest.raises(ValueError, match="^r1 must hold exactly .*nchan == 1"):
        device.stereo_batch(gray, r1, ri0, ri1, box, (-24, 8), radius=3, both=True)
    out = [torch.empty(n, dtype=torch.int32, device="cuda")] + [torch.empty(n, dtype=torch.uint16, device="cuda") for _ in range(2)]
    with pytest.raises(ValueError, match="^r0 must hold exactly"):
        device.stereo_batch_into(r0, r1, ri0, ri1, box, None, 3, (-24, 8), 0, *out)
    # one channel of it is a gray window and is taken
    device.stereo_batch(gray, r1.reshape(n, 3)[:, 0].contiguous(), ri0, ri1, box, (-24, 8), radius=3)
    torch.cuda.synchronize()


def test_names_are_declared_exported_and_prototyped():
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    from spectavi_amd._proto import PROTOTYPES
    from tests.test_abi import declared_prototypes
    decls = declared_prototypes()
    for n in ("spv_stereo_batch_plan", "spv_stereo_batch_device", "spv_stereo_keep_batch_device",
              "spv_stereo_matches_batch_device"):
        assert n in decls and n in PROTOTYPES and hasattr(clib, n), n
    hdr = open(os.path.join(os.path.dirname(device.__file__), "..", "include", "spectavi_amd.h")).read()
    assert "#define SPV_STEREO_NONE (-2147483647 - 1)" in hdr and device.STEREO_NONE == -2**31
    for name in ("stereo_batch", "stereo_keep_batch", "stereo_matches_count", "stereo_matches_fill"):
        assert '"%s"' % name in hdr
    for fn in ("stereo_batch_plan", "stereo_batch", "stereo_batch_into", "stereo_keep_batch", "stereo_matches_batch"):
        assert callable(getattr(device, fn))
