"""resect_gather and resect_fit_batch without a GPU: every argument the entry points reject is rejected before a device
is touched and before anything is written, calls with nothing to run return without a device, and the Python forms raise
ValueError for the same arguments."""
import ctypes as ct

import numpy as np
import pytest

from spectavi_amd._lib import clib, SPV_ERR_INVALID


def ptr(x):
    if x is None or isinstance(x, int):
        return x
    return x.ctypes.data


# ---- the fit ----------------------------------------------------------------------------------------------------------
def fit_args(**over):
    """Valid arguments on host arrays: two sets of 7 and 3 rows, 4 tries."""
    smp = np.tile(np.arange(6, dtype=np.int32), (2, 4, 1))
    a = dict(x=np.ones((10, 3)), Xw=np.ones((10, 4)), off=np.array([0, 7, 10], np.int64), nviews=2, share=0.5,
             max_error=1.0, tries=4, find_best=0, samples=smp, seeds=None, ok=np.full(2, 7, np.int32),
             P=np.full((2, 12), 7.0), pct=np.full(2, 7.0), n=np.full(2, 7, np.int32), bt=np.full(2, 7, np.int32),
             ran=np.full(2, 7, np.int32), mask=None, cams=None, inl=None)
    a.update(over)
    return a


def call_fit(a, device_form):
    args = [ptr(a["x"]), ptr(a["Xw"]), ptr(a["off"]), a["nviews"], a["share"], a["max_error"], a["tries"], a["find_best"],
            ptr(a["samples"]), ptr(a["seeds"]), ptr(a["ok"]), ptr(a["P"]), ptr(a["pct"]), ptr(a["n"]), ptr(a["bt"]),
            ptr(a["ran"]), ptr(a["mask"]), ptr(a["cams"]), ptr(a["inl"])]
    if device_form:
        return clib.spv_resect_fit_batch_device(*args, None)
    return clib.spv_resect_fit_batch(*args)


def _bad_sample(value):
    smp = np.tile(np.arange(6, dtype=np.int32), (2, 4, 1))
    smp[0, 3, 5] = value
    return smp


FIT_BAD = {
    "null view_off": dict(off=None),
    "view_off starts at 1": dict(off=np.array([1, 7, 10], np.int64)),
    "view_off decreases": dict(off=np.array([0, 11, 10], np.int64)),
    "view_off ends at 2^31": dict(off=np.array([0, 7, 2 ** 31], np.int64)),
    "NaN max_error": dict(max_error=float("nan")),
    "NaN share": dict(share=float("nan")),
    "negative nviews": dict(nviews=-1),
    "more than 2^20 sets": dict(nviews=2 ** 20 + 1),
    "negative maximum_tries": dict(tries=-1),
    "maximum_tries above 7e8": dict(tries=700000001, samples=None, seeds=np.zeros(2, np.uint64)),
    "null success": dict(ok=None),
    "null camera": dict(P=None),
    "null inlier_percent": dict(pct=None),
    "null n_inliers": dict(n=None),
    "null x": dict(x=None),
    "null Xw": dict(Xw=None),
    "neither samples nor seeds": dict(samples=None, seeds=None),
    "sample below 0": dict(samples=_bad_sample(-1)),
    "sample at rows": dict(samples=_bad_sample(7)),
}
FIT_BAD_DEVICE = {   # the device form's own: what it is handed is dereferenced by kernels
    "misaligned x": dict(x="off by 4"),
    "misaligned Xw": dict(Xw="off by 4"),
    "misaligned try_cameras": dict(cams="off by 4"),
    "misaligned try_inliers": dict(inl="off by 2"),
}


def _reject_fit(what, over, device_form):
    room = np.zeros(64)
    over = {k: room.ctypes.data + int(v.split()[-1]) if isinstance(v, str) else v for k, v in over.items()}
    a = fit_args(**over)
    assert call_fit(a, device_form) == SPV_ERR_INVALID, what
    assert clib.spv_last_error(), what
    for k in ("ok", "P", "pct", "n", "bt", "ran"):
        if isinstance(a[k], np.ndarray):
            assert np.all(a[k] == 7), "%s: %s was written" % (what, k)


@pytest.mark.parametrize("device_form", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("what", sorted(FIT_BAD))
def test_fit_rejects(what, device_form):
    _reject_fit(what, FIT_BAD[what], device_form)


@pytest.mark.parametrize("what", sorted(FIT_BAD_DEVICE))
def test_fit_device_form_rejects(what):
    _reject_fit(what, FIT_BAD_DEVICE[what], True)


@pytest.mark.parametrize("device_form", [True, False], ids=["device", "host"])
def test_fit_with_nothing_to_run_touches_no_device(device_form):
    """No set of 6 rows, or no tries: SPV_OK on a machine without a GPU, every set reports what a skipped set does."""
    for over in (dict(off=np.array([0, 5, 10], np.int64)),                      # 5 and 5 rows
                 dict(off=np.array([0, 5, 10], np.int64), samples=None, seeds=None),   # ... and then no subsets are needed
                 dict(off=np.array([0, 5, 10], np.int64), samples=_bad_sample(99)),    # ... nor looked at
                 dict(tries=0, samples=None, seeds=None),
                 dict(off=np.array([0], np.int64), nviews=0, x=None, Xw=None, ok=None, P=None, pct=None, n=None),
                 dict(off=np.array([0, 0, 0], np.int64), x=None, Xw=None)):
        a = fit_args(**over)
        host_out = {}
        if not device_form and a["nviews"] == 2:   # the host form's optional outputs are filled on the host
            host_out = dict(mask=np.full(10, 9, np.uint8), cams=np.zeros((2, max(a["tries"], 1), 12)),
                            inl=np.full((2, max(a["tries"], 1)), 9, np.int32))
            a.update(host_out)
        assert call_fit(a, device_form) == 0, (over, clib.spv_last_error())
        if a["nviews"] == 2:
            assert a["ok"].tolist() == [0, 0] and a["n"].tolist() == [0, 0] and a["pct"].tolist() == [0.0, 0.0]
            assert a["bt"].tolist() == [-1, -1] and a["ran"].tolist() == [0, 0]
            assert np.all(a["P"] == 7.0), "a skipped set's camera row stays untouched"
        if host_out:
            total = int(a["off"][-1])
            assert np.all(host_out["mask"][:total] == 0)
            if a["tries"] > 0:
                assert np.all(host_out["inl"] == 0) and np.all(np.isnan(host_out["cams"]))


def test_fit_optional_outputs_may_be_null():
    a = fit_args(off=np.array([0, 5, 10], np.int64), bt=None, ran=None)
    assert call_fit(a, True) == 0 and call_fit(a, False) == 0


def test_fit_plan_entry_rejects():
    out = (ct.c_longlong * 4)(-7, -7, -7, -7)
    ok = np.array([0, 7, 10], np.int64)
    for off, nv, tries, cus, o, cap in ((None, 2, 4, 256, out, 0), (ok, -1, 4, 256, out, 0), (ok, 2, -1, 256, out, 0),
                                        (ok, 2, 4, 0, out, 0), (ok, 2, 4, 256, None, 0), (ok, 2, 4, 256, out, -1),
                                        (np.array([1, 7, 10], np.int64), 2, 4, 256, out, 0),
                                        (np.array([0, 7, 2 ** 31], np.int64), 2, 4, 256, out, 0)):
        assert clib.spv_resect_fit_batch_plan(ptr(off), nv, tries, cus, o, None, cap) == SPV_ERR_INVALID
        assert list(out) == [-7] * 4
    assert clib.spv_resect_fit_batch_plan(ptr(ok), 2, 4, 256, out, None, 0) == 0 and list(out) == [1, 4, 1, 1]


# ---- the gather -------------------------------------------------------------------------------------------------------
def gather_args(**over):
    """Valid arguments on host arrays (the entry checks before it launches): two sets of 2 and 4 rows, 3 tracks."""
    a = dict(geom=np.zeros((6, 4), np.float32), track=np.zeros(6, np.int32), seg=np.array([0, 2, 6], np.int64), nseg=2,
             views=np.array([1, 0], np.int32), nviews=2, X=np.zeros((3, 4)), ok=None, ntracks=3, capacity=6,
             x=np.full((6, 3), 5.0), Xw=np.full((6, 4), 5.0), rows=np.full(6, 5, np.int32), d_off=None,
             off=np.full(3, 5, np.int64))
    a.update(over)
    return a


def call_gather(a):
    return clib.spv_resect_gather_device(ptr(a["geom"]), ptr(a["track"]), ptr(a["seg"]), a["nseg"], ptr(a["views"]),
                                         a["nviews"], ptr(a["X"]), ptr(a["ok"]), a["ntracks"], a["capacity"], ptr(a["x"]),
                                         ptr(a["Xw"]), ptr(a["rows"]), ptr(a["d_off"]), ptr(a["off"]), None)


GATHER_BAD = {
    "negative nseg": dict(nseg=-1),
    "negative nviews": dict(nviews=-1),
    "negative ntracks": dict(ntracks=-1),
    "negative capacity": dict(capacity=-1),
    "more than 2^20 views": dict(nviews=2 ** 20 + 1),
    "null seg_off": dict(seg=None),
    "seg_off starts at 1": dict(seg=np.array([1, 2, 6], np.int64)),
    "seg_off decreases": dict(seg=np.array([0, 7, 6], np.int64)),
    "seg_off ends at 2^31": dict(seg=np.array([0, 2, 2 ** 31], np.int64)),
    "null views": dict(views=None),
    "view below 0": dict(views=np.array([1, -1], np.int32)),
    "view at nseg": dict(views=np.array([2, 0], np.int32)),
    "null geom": dict(geom=None),
    "null track": dict(track=None),
    "null X": dict(X=None),
    "null x": dict(x=None),
    "null Xw": dict(Xw=None),
    "misaligned X": dict(X="off by 4"),
    "misaligned x": dict(x="off by 4"),
    "misaligned Xw": dict(Xw="off by 4"),
    "misaligned rows": dict(rows="off by 2"),
    "misaligned d_view_off": dict(d_off="off by 4"),
    "misaligned geom": dict(geom="off by 2"),
    "misaligned track": dict(track="off by 2"),
}


@pytest.mark.parametrize("what", sorted(GATHER_BAD))
def test_gather_rejects(what):
    room = np.zeros(64)
    over = {k: room.ctypes.data + int(v.split()[-1]) if isinstance(v, str) else v for k, v in GATHER_BAD[what].items()}
    a = gather_args(**over)
    assert call_gather(a) == SPV_ERR_INVALID, what
    assert clib.spv_last_error(), what
    assert np.all(a["off"] == 5), "nothing is written"
    for k in ("x", "Xw", "rows"):
        if isinstance(a[k], np.ndarray):
            assert np.all(a[k] == 5), "nothing is written"


def test_gather_rejects_2_31_listed_rows():
    """Repeats make the listed rows exceed the table's: 3 x 2^30 rows."""
    a = gather_args(seg=np.array([0, 2 ** 30, 2 ** 30 + 4], np.int64), views=np.array([0, 0, 0], np.int32), nviews=3,
                    off=np.full(4, 5, np.int64))
    assert call_gather(a) == SPV_ERR_INVALID and np.all(a["off"] == 5)


def test_gather_with_nothing_to_take_touches_no_device():
    for over, n in ((dict(nviews=0, views=None, off=np.full(1, 5, np.int64)), 1),
                    (dict(seg=np.array([0, 0, 6], np.int64), views=np.array([0, 0], np.int32), geom=None, track=None), 3),
                    (dict(ntracks=0, X=None), 3),
                    (dict(seg=np.array([0], np.int64), nseg=0, nviews=0, views=None, geom=None, track=None, X=None,
                          ntracks=0, x=None, Xw=None, rows=None, off=np.full(1, 5, np.int64)), 1)):
        a = gather_args(**over)
        assert call_gather(a) == 0, (over, clib.spv_last_error())
        assert a["off"].tolist() == [0] * n


# ---- the Python forms -------------------------------------------------------------------------------------------------
def test_python_forms_raise_value_error_before_a_device():
    import torch
    from spectavi_amd import device, mvg
    x, Xw = torch.ones((10, 3), dtype=torch.float64), torch.ones((10, 4), dtype=torch.float64)   # CPU tensors: a call
    good = dict(x=x, Xw=Xw, view_off=[0, 7, 10], maximum_tries=4)   # that got past its checks raises TypeError
    with pytest.raises(TypeError):
        device.resect_fit_batch(**good)
    smp = np.tile(np.arange(6), (2, 4, 1))
    for what, over in (
            ("x shape", dict(x=torch.ones((10, 2), dtype=torch.float64))),
            ("Xw shape", dict(Xw=torch.ones((10, 3), dtype=torch.float64))),
            ("rows differ", dict(Xw=torch.ones((9, 4), dtype=torch.float64))),
            ("view_off start", dict(view_off=[1, 7, 10])),
            ("view_off order", dict(view_off=[0, 11, 10])),
            ("view_off end", dict(view_off=[0, 7, 9])),
            ("view_off empty", dict(view_off=[])),
            ("samples width", dict(samples=np.zeros((2, 4, 7), np.int32))),
            ("samples sets", dict(samples=np.zeros((3, 4, 6), np.int32))),
            ("samples dtype", dict(samples=np.zeros((2, 4, 6)))),
            ("sample below 0", dict(samples=np.where(smp == 5, -1, smp))),
            ("sample at rows", dict(samples=np.where(smp == 5, 7, smp))),
            ("seeds count", dict(seeds=[1, 2, 3])),
            ("negative tries", dict(maximum_tries=-1)),
            ("NaN max_error", dict(max_error=float("nan"))),
            ("NaN share", dict(required_percent_inliers=float("nan")))):
        with pytest.raises(ValueError):
            device.resect_fit_batch(**dict(good, **over))
    geom, track = torch.zeros((6, 4), dtype=torch.float32), torch.zeros(6, dtype=torch.int32)
    X, ok = torch.zeros((3, 4), dtype=torch.float64), torch.ones(3, dtype=torch.uint8)
    ggood = dict(geom=geom, track=track, seg_off=[0, 2, 6], views=[1, 0], X=X, ok=ok)
    with pytest.raises(TypeError):
        device.resect_gather(**ggood)
    for what, over in (
            ("geom shape", dict(geom=torch.zeros((6, 3), dtype=torch.float32))),
            ("geom dtype", dict(geom=torch.zeros((6, 4), dtype=torch.float64))),
            ("geom rows", dict(geom=torch.zeros((5, 4), dtype=torch.float32))),
            ("track rows", dict(track=torch.zeros(5, dtype=torch.int32))),
            ("X shape", dict(X=torch.zeros((3, 3), dtype=torch.float64))),
            ("ok rows", dict(ok=torch.ones(2, dtype=torch.uint8))),
            ("seg_off start", dict(seg_off=[1, 2, 6])),
            ("view below 0", dict(views=[-1])),
            ("view at nseg", dict(views=[2])),
            ("views not integers", dict(views=[0.5])),
            ("views shape", dict(views=[[0, 1]])),
            ("negative capacity", dict(capacity=-1))):
        with pytest.raises(ValueError):
            device.resect_gather(**dict(ggood, **over))
    # the host-list form
    xs, Xws = [np.ones((7, 2)), np.ones((3, 3))], [np.ones((7, 4)), np.ones((3, 4))]
    for what, over, exc in (
            ("lists differ", dict(Xws=Xws[:1]), ValueError),
            ("x columns", dict(xs=[np.ones((7, 4)), np.ones((3, 3))]), TypeError),
            ("Xw columns", dict(Xws=[np.ones((7, 3)), np.ones((3, 4))]), TypeError),
            ("rows differ", dict(Xws=[np.ones((6, 4)), np.ones((3, 4))]), TypeError),
            ("samples count", dict(samples=[np.zeros((4, 6), np.int32)]), ValueError),
            ("samples width", dict(samples=[np.zeros((4, 7), np.int32)] * 2), ValueError),
            ("samples of two ntries", dict(samples=[np.zeros((4, 6), np.int32), np.zeros((5, 6), np.int32)]), ValueError),
            ("sample at rows", dict(samples=[np.full((4, 6), 7, np.int32), np.zeros((4, 6), np.int32)]), ValueError),
            ("seeds count", dict(seeds=[1]), ValueError),
            ("NaN max_error", dict(max_error=float("nan")), ValueError)):
        with pytest.raises(exc):
            mvg.resect_batch(**dict(dict(xs=xs, Xws=Xws, maximum_tries=4), **over))
    # nothing to run: no device is needed
    fits = mvg.resect_batch([np.ones((5, 2)), np.ones((0, 2))], [np.ones((5, 4)), np.ones((0, 4))], maximum_tries=4)
    assert [f["success"] for f in fits] == [False, False] and all(f["camera"] is None and f["best_try"] == -1 and
                                                                   f["tries_run"] == 0 and f["inlier_idx"].size == 0 for f in fits)
    fits, cams, inl = mvg.resect_batch([np.ones((7, 2))], [np.ones((7, 4))], maximum_tries=0, want_tries=True)
    assert fits[0]["camera"] is None and cams.shape == (1, 0, 12) and inl.shape == (1, 0)
    assert mvg.resect_batch([], []) == []
