"""resect_gather and resect_fit_batch on the GPU (spv_resect_*), against tests/resect_model.py.

The gather is compared to a numpy loop bit for bit.  The fit is held to its definition try by try (want_tries): every
try camera of unit norm within 1e-12 and ||A p|| <= 1e-13 sigma1(A) + 2 formation (A is 11 x 12: its null vector is
exact, there is no smallest singular value to allow for); every try's count between the model's counts at max_error -/+ tol (tol = 1e-6 max_error + 8 x
the difference of the model's two routes on that row; tests/test_resect_model.py records what it measures); the winner
from the device's own counts by the stated rule, exactly; and, without the per-try outputs, the same bits across
rounds and early leaving.

Measured on one MI355X over the tries without a repeated sample row (test_every_try_meets_the_definition prints them
with -s), worst ||A p|| / sigma1 and worst | ||p|| - 1 | per case: calibrated-clean 1.02e-16 and 2.22e-16,
calibrated-noisy 8.52e-17 and 2.22e-16, pixel-clean 6.44e-19 and 3.33e-16, pixel-noisy 2.31e-19 and 2.22e-16 -- three
orders inside the 1e-13 floor and four inside 1e-12.  Every count lay inside the model's bounds, which coincide on
these cases (tests/test_resect_model.py: no undecided row)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import resect_model as rm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANTIATED = {"resect_gather_count_kernel", "resect_gather_scan_kernel", "resect_gather_place_kernel",
                "resect_solve_kernel", "resect_score_kernel", "resect_reduce_kernel", "resect_mask_kernel"}
PROFILE_NAMES = ("resect_gather", "resect_solve", "resect_score", "resect_reduce")
INT_MAX = 2 ** 31 - 1


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fit(col, **kw):
    from spectavi_amd import device
    return device.resect_fit_batch(cuda(col["x"]), cuda(col["Xw"]), col["off"], **kw)


def same_fit(a, b, tries_run=True):
    keys = ["success", "inlier_percent", "best_try"] + (["tries_run"] if tries_run else [])
    if any(a[k] != b[k] for k in keys) or not np.array_equal(a["inlier_idx"], b["inlier_idx"]):
        return False
    if (a["camera"] is None) != (b["camera"] is None):
        return False
    return a["camera"] is None or np.array_equal(a["camera"].view(np.uint64), b["camera"].view(np.uint64))


# ---- gather -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gather_case():
    rng = np.random.default_rng(77)
    sizes = [0, 1, 255, 256, 257]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total, nt = int(seg[-1]), 300
    geom = rng.uniform(-50, 1500, (total, 4)).astype(np.float32)
    track = rng.integers(0, nt, total).astype(np.int32)
    track[rng.choice(total, 90, replace=False)] = np.tile(np.array([-7, nt, INT_MAX, -1, nt + 5, -INT_MAX - 1], np.int32), 15)
    track[0] = 17                                    # the one row of set 1 is taken
    X = rng.standard_normal((nt, 4))
    X[3, 2], X[40, 0], X[41, 3], X[200, 1] = np.nan, np.inf, -np.inf, np.nan
    ok = (rng.uniform(size=nt) < 0.8).astype(np.uint8)
    ok[17], ok[5] = 1, 0
    return dict(seg=seg, geom=geom, track=track, X=X, ok=ok, nt=nt, views=[4, 2, 0, 2, 1, 3])


def gather_numpy(c, views, ok):
    x, Xw, rows, off = [], [], [], [0]
    for s in views:
        for r in range(int(c["seg"][s + 1] - c["seg"][s])):
            g = int(c["seg"][s]) + r
            t = int(c["track"][g])
            if 0 <= t < c["nt"] and (ok is None or ok[t] != 0) and np.isfinite(c["X"][t]).all():
                x.append([np.float64(c["geom"][g, 0]), np.float64(c["geom"][g, 1]), 1.0])
                Xw.append(c["X"][t])
                rows.append(r)
        off.append(len(rows))
    return (np.array(x, np.float64).reshape(-1, 3), np.array(Xw, np.float64).reshape(-1, 4), np.array(rows, np.int32),
            np.array(off, np.int64))


@pytest.mark.parametrize("with_ok", [False, True], ids=["ok NULL", "ok given"])
def test_gather_is_the_numpy_loop(gather_case, with_ok):
    from spectavi_amd import device
    c = gather_case
    ok = c["ok"] if with_ok else None
    wx, wX, wrows, woff = gather_numpy(c, c["views"], ok)
    assert woff[-1] > 600 and woff[3] == woff[2] and woff[5] - woff[4] == 1     # an empty view, the one-row view
    args = (cuda(c["geom"]), cuda(c["track"]), c["seg"], c["views"], cuda(c["X"]), cuda(ok) if with_ok else None)
    for _ in range(2):                                                           # the same bits from run to run
        x, Xw, rows, off = device.resect_gather(*args)
        n = int(off[-1])
        assert np.array_equal(off, woff)
        assert np.array_equal(x.cpu().numpy()[:n].view(np.uint64), wx.view(np.uint64))
        assert np.array_equal(Xw.cpu().numpy()[:n].view(np.uint64), wX.view(np.uint64))
        assert np.array_equal(rows.cpu().numpy()[:n], wrows)
    # the repeated view owns two blocks of its own with the same rows
    a, b = slice(woff[1], woff[2]), slice(woff[3], woff[4])
    assert np.array_equal(rows.cpu().numpy()[a], rows.cpu().numpy()[b]) and woff[2] - woff[1] > 100


def test_gather_capacity_short_of_the_count(gather_case):
    import torch
    from spectavi_amd._lib import clib, check
    c = gather_case
    wx, wX, wrows, woff = gather_numpy(c, c["views"], c["ok"])
    count = int(woff[-1])
    views = np.array(c["views"], np.int32)
    geom, track, X, ok = cuda(c["geom"]), cuda(c["track"]), cuda(c["X"]), cuda(c["ok"])
    for cap in (count - 301, 1, 0):
        x = torch.full((count, 3), 7.0, dtype=torch.float64, device="cuda")
        Xw = torch.full((count, 4), 7.0, dtype=torch.float64, device="cuda")
        rows = torch.full((count,), 7, dtype=torch.int32, device="cuda")
        d_off = torch.full((len(views) + 1,), -1, dtype=torch.int64, device="cuda")
        off = np.full(len(views) + 1, -1, np.int64)
        stream = torch.cuda.current_stream().cuda_stream
        check(clib.spv_resect_gather_device(geom.data_ptr(), track.data_ptr(), c["seg"].ctypes.data, len(c["seg"]) - 1,
                                            views.ctypes.data, len(views), X.data_ptr(), ok.data_ptr(), c["nt"], cap,
                                            x.data_ptr(), Xw.data_ptr(), rows.data_ptr(), d_off.data_ptr(), off.ctypes.data,
                                            stream))
        torch.cuda.synchronize()
        assert np.array_equal(off, woff) and np.array_equal(d_off.cpu().numpy(), woff), "view_off counts every taken row"
        assert np.array_equal(x.cpu().numpy()[:cap], wx[:cap]) and np.array_equal(Xw.cpu().numpy()[:cap], wX[:cap])
        assert np.array_equal(rows.cpu().numpy()[:cap], wrows[:cap])
        assert torch.all(x[cap:] == 7.0) and torch.all(Xw[cap:] == 7.0) and torch.all(rows[cap:] == 7), "nothing beyond capacity"


# ---- the per-try definition -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    """Every case run once with the per-try outputs and the mask."""
    out = {}

    def get(name):
        if name not in out:
            c = rm.case(name)
            fits, mask, cams, inl = fit(c["col"], required_percent_inliers=rm.SHARE, max_error=c["max_error"],
                                        samples=c["samples"], want_mask=True, want_tries=True)
            out[name] = dict(fits=fits, mask=mask.cpu().numpy(), cams=cams.cpu().numpy(), inl=inl.cpu().numpy())
        return out[name]
    return get


@pytest.mark.parametrize("name", sorted(rm.CASES))
def test_every_try_meets_the_definition(runs, name):
    c, r = rm.case(name), runs(name)
    off = c["col"]["off"]
    worst_res = worst_norm = 0.0
    for p, m in enumerate(c["model"]):
        rows = int(off[p + 1] - off[p])
        f = r["fits"][p]
        if m is None:
            assert rows < rm.MIN_ROWS and not f["success"] and f["camera"] is None and f["best_try"] == -1
            assert f["tries_run"] == 0 and f["inlier_idx"].size == 0 and f["inlier_percent"] == 0.0
            assert np.all(r["inl"][p] == 0) and np.all(np.isnan(r["cams"][p])) and not r["mask"][off[p]:off[p + 1]].any()
            continue
        assert f["tries_run"] == rm.TRIES
        cnt = r["inl"][p]
        assert np.all((cnt >= 0) & (cnt <= rows)), (name, p)
        for t in range(rm.TRIES):
            P = r["cams"][p, t]
            if t == rm.REPEATED_TRY:        # a repeated sample row: a count of 0 or finite garbage, nothing more is asked
                continue
            assert np.isfinite(P).all(), (name, p, t)
            worst_norm = max(worst_norm, abs(np.linalg.norm(P) - 1))
            assert abs(np.linalg.norm(P) - 1) <= 1e-12, (name, p, t)
            assert P[np.flatnonzero(P)[-1]] > 0, "the last non-zero entry is positive"
            A, s = m["A"][t], m["S"][t]
            res = np.linalg.norm(A @ P)
            worst_res = max(worst_res, res / s[0])
            assert res <= 1e-13 * s[0] + 2 * m["formation"][t], (name, p, t, res, s[0])
            assert m["count_lo"][t] <= cnt[t] <= m["count_hi"][t], (name, p, t, cnt[t], m["count_lo"][t], m["count_hi"][t])
    print("%s: worst ||A p|| / sigma1 %.2e, worst | ||p|| - 1 | %.2e" % (name, worst_res, worst_norm))


@pytest.mark.parametrize("name", sorted(rm.CASES))
def test_winner_follows_the_rule_on_the_devices_counts(runs, name):
    c, r = rm.case(name), runs(name)
    off = c["col"]["off"]
    for p, m in enumerate(c["model"]):
        if m is None:
            continue
        rows = int(off[p + 1] - off[p])
        f, cnt = r["fits"][p], r["inl"][p]
        bt, ok = rm.select(cnt, rows, rm.SHARE, False)
        assert (f["best_try"], f["success"]) == (bt, ok), (name, p)
        if bt < 0:
            assert f["camera"] is None and f["inlier_idx"].size == 0 and f["inlier_percent"] == 0.0
            continue
        assert len(f["inlier_idx"]) == cnt[bt] and f["inlier_percent"] == cnt[bt] / float(rows)
        assert np.array_equal(f["camera"].reshape(12).view(np.uint64), r["cams"][p, bt].view(np.uint64))
        # the mask is numpy's verdict under the returned camera.  A departure from "equals", on the noisy cases only: the
        # scorer compares squares and divides by a Newton reciprocal, so a row whose residual lies within 1e-9 relative
        # of max_error may fall either way; at most one such row a set is let differ.  The clean cases have none.
        x, Xw = c["col"]["x"][off[p]:off[p + 1]], c["col"]["Xw"][off[p]:off[p + 1]]
        err, dc = rm.verdict_terms(f["camera"][None], x, Xw)
        edge = (np.abs(err[0] - c["max_error"]) <= 1e-9 * c["max_error"]) | (np.abs(dc[0]) <= 1e-12 * np.abs(dc[0]).max())
        want = rm.inliers(err[0], dc[0], c["max_error"])
        got = r["mask"][off[p]:off[p + 1]] != 0
        assert np.array_equal(got[~edge], want[~edge]) and edge.sum() <= (1 if c["noisy"] else 0), (name, p)
        assert np.array_equal(np.flatnonzero(got), f["inlier_idx"])


@pytest.mark.parametrize("name", [n for n in sorted(rm.CASES) if n.endswith("clean")])
def test_clean_cases_recover_the_planted_inliers(runs, name):
    c, r = rm.case(name), runs(name)
    off = c["col"]["off"]
    for p, m in enumerate(c["model"]):
        if m is None:
            continue
        f = r["fits"][p]
        assert f["success"], (name, p)
        assert np.array_equal(f["inlier_idx"], np.flatnonzero(c["col"]["planted"][off[p]:off[p + 1]])), (name, p)
        assert f["best_try"] == m["best_try"]


def test_rule_variants_on_the_devices_counts(runs):
    """First above the share, best on failure with the earliest among equals, no model -- and the bound's edges."""
    name = "pixel-noisy"
    c, r = rm.case(name), runs(name)
    off = c["col"]["off"]
    for share, find_best in ((0.6, True), (2.0, True), (2.0, False), (0.0, False), (0.4, False), (1.0, True)):
        fits = fit(c["col"], required_percent_inliers=share, max_error=c["max_error"], samples=c["samples"],
                   find_best_even_in_failure=find_best)
        for p, m in enumerate(c["model"]):
            if m is None:
                assert fits[p]["best_try"] == -1 and fits[p]["tries_run"] == 0
                continue
            rows = int(off[p + 1] - off[p])
            cnt = r["inl"][p]
            bt, ok = rm.select(cnt, rows, share, find_best)
            f = fits[p]
            assert (f["best_try"], f["success"]) == (bt, ok), (share, find_best, p)
            assert len(f["inlier_idx"]) == (cnt[bt] if bt >= 0 else 0)
            assert (f["camera"] is None) == (bt < 0)
            if bt >= 0:
                assert np.array_equal(f["camera"].reshape(12).view(np.uint64), r["cams"][p, bt].view(np.uint64))
                assert bt + 1 <= f["tries_run"] <= rm.TRIES
        if share == 2.0 and find_best:      # the 6-row set: many tries with the same count, the earliest wins
            cnt = r["inl"][2]
            assert np.sum(cnt == cnt.max()) > 1 and fits[2]["best_try"] == int(np.argmax(cnt))
    # a negative bound takes no row, an infinite one every row in front of the camera
    _, _, inl = fit(c["col"], max_error=-1.0, samples=c["samples"], want_tries=True)
    assert not inl.cpu().numpy().any()
    fits, cams, inl = fit(c["col"], max_error=float("inf"), samples=c["samples"], want_tries=True, required_percent_inliers=2.0)
    p = 6
    x, Xw = c["col"]["x"][off[p]:off[p + 1]], c["col"]["Xw"][off[p]:off[p + 1]]
    keep = np.arange(rm.TRIES) != rm.REPEATED_TRY
    err, dc = rm.verdict_terms(cams.cpu().numpy()[p].reshape(-1, 3, 4)[keep], x, Xw)
    with np.errstate(invalid="ignore"):
        sure, maybe = (dc > 1e-9).sum(1), (dc > -1e-9).sum(1)
    got = inl.cpu().numpy()[p][keep]
    assert np.all((sure <= got) & (got <= maybe))


# ---- rounds, early leaving, seeds -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed():
    """Easy sets that leave in round one, a pure-outlier set that runs every try, small sets; 600 tries from seeds."""
    rng = np.random.default_rng(2024)
    col = rm.collection(rng, [300, 5, 700, 500, 40, 60], noise=0.0, outliers=0.3)
    lo, hi = col["off"][3], col["off"][4]
    col["x"][lo:hi, 0] = rng.uniform(0, 1280, hi - lo)        # set 3: no row agrees with its point
    col["x"][lo:hi, 1] = rng.uniform(0, 960, hi - lo)
    col["planted"][lo:hi] = False
    return col, np.array([11, 12, 13, 14, 15, 16], np.uint64), 600


def test_rounds_and_early_leaving_give_the_same_bits(mixed):
    from spectavi_amd import mvg
    col, seeds, tries = mixed
    kw = dict(required_percent_inliers=0.6, max_error=1.0, maximum_tries=tries, seeds=seeds)
    all_tries, cams, inl = fit(col, want_tries=True, **kw)
    early = fit(col, **kw)
    inl = inl.cpu().numpy()
    sizes = np.diff(col["off"])
    for p, (a, b) in enumerate(zip(all_tries, early)):
        assert same_fit(a, b, tries_run=False), p
        if sizes[p] < rm.MIN_ROWS:
            assert a["tries_run"] == b["tries_run"] == 0
            continue
        assert a["tries_run"] == tries
        assert (a["best_try"], a["success"]) == rm.select(inl[p], sizes[p], 0.6, False)
        if b["success"]:
            assert b["best_try"] + 1 <= b["tries_run"] <= tries
        else:
            assert b["tries_run"] == tries
    assert [f["success"] for f in early] == [True, False, True, False, True, True]
    assert early[3]["best_try"] == -1 and early[3]["camera"] is None and early[3]["tries_run"] == tries
    assert all(early[p]["best_try"] < 256 and early[p]["tries_run"] == 256 for p in (0, 2, 4, 5)), "easy sets leave in round one"
    for p in (0, 2, 4, 5):      # no redrawn row comes within a pixel of its point by chance
        assert col["planted"][col["off"][p]:col["off"][p + 1]][early[p]["inlier_idx"]].all()
    # the subsets of a seed are the first six columns of ransac_sample's
    smp = np.zeros((len(sizes), tries, 6), np.int32)
    for p in range(len(sizes)):
        if sizes[p] >= 10:
            smp[p] = mvg.ransac_sample(int(seeds[p]), int(sizes[p]), tries)[:, :6]
    sampled = fit(col, required_percent_inliers=0.6, max_error=1.0, samples=smp)
    assert all(same_fit(a, b) for a, b in zip(early, sampled))
    # best on failure across rounds: the pure-outlier set keeps the earliest of its best tries
    best = fit(col, find_best_even_in_failure=True, **kw)
    bt, ok = rm.select(inl[3], sizes[3], 0.6, True)
    assert (best[3]["best_try"], best[3]["success"]) == (bt, ok) and bt >= 0 and len(best[3]["inlier_idx"]) == inl[3][bt]


def test_small_sets_under_seeds():
    """Sets of 6 to 9 rows, which ransac_sample does not take, draw their subsets from the same generator."""
    rng = np.random.default_rng(5)
    col = rm.collection(rng, [6, 7, 9, 10, 3], noise=0.0, outliers=0.0)
    seeds = np.array([3, 4, 5, 6, 7], np.uint64)
    a, cams, inl = fit(col, required_percent_inliers=0.9, max_error=1.0, maximum_tries=20, seeds=seeds, want_tries=True)
    b = fit(col, required_percent_inliers=0.9, max_error=1.0, maximum_tries=20, seeds=seeds)
    inl = inl.cpu().numpy()
    for p, n in enumerate([6, 7, 9, 10, 3]):
        assert same_fit(a[p], b[p], tries_run=False)
        if n < rm.MIN_ROWS:
            assert a[p]["best_try"] == -1
            continue
        assert (a[p]["best_try"], a[p]["success"]) == rm.select(inl[p], n, 0.9, False)
        assert np.isfinite(cams.cpu().numpy()[p]).all(), "six different rows a try: no degenerate hypothesis"
    assert a[0]["success"] and len(a[0]["inlier_idx"]) == 6


# ---- cuts -------------------------------------------------------------------------------------------------------------
def test_cut_tries_repeated_sets_and_the_host_form():
    import torch
    from spectavi_amd import device, mvg
    rng = np.random.default_rng(31)
    base = rm.collection(rng, [300, 40], noise=0.0, outliers=0.3)
    tries = 200
    smp = rm.draw_samples(rng, base["off"], tries, base["planted"], clean_every=50)
    other = rm.draw_samples(rng, base["off"], tries, base["planted"], clean_every=50)[0]
    S = (base["x"][:300], base["Xw"][:300])
    T = (base["x"][300:], base["Xw"][300:])
    order = [S, T, S, S, S]
    col = dict(x=np.concatenate([s[0] for s in order]), Xw=np.concatenate([s[1] for s in order]),
               off=np.concatenate([[0], np.cumsum([len(s[0]) for s in order])]).astype(np.int64))
    samples = np.stack([smp[0], smp[1], smp[0], smp[0], other])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    plan, items = device.resect_fit_batch_plan(col["off"], tries, cus, want_items=True)
    assert plan["items"] > plan["row_blocks"] == 9 and len(set(items[items[:, 0] == 0][:, 3].tolist())) > 1, "tries are cut"
    # share 2: every try runs; find_best keeps the best
    kw = dict(required_percent_inliers=2.0, max_error=1.0, find_best_even_in_failure=True)
    fits, cams, inl = fit(col, samples=samples, want_tries=True, **kw)
    cams, inl = cams.cpu().numpy(), inl.cpu().numpy()
    for p in (2, 3):
        assert same_fit(fits[0], fits[p])
        assert np.array_equal(inl[0], inl[p]) and np.array_equal(cams[0].view(np.uint64), cams[p].view(np.uint64))
    single = fit(dict(x=S[0], Xw=S[1], off=np.array([0, 300], np.int64)), samples=other[None], **kw)
    assert same_fit(fits[4], single[0])
    plain = fit(col, samples=samples, **kw)
    assert all(same_fit(a, b) for a, b in zip(fits, plain))
    host, hcams, hinl = mvg.resect_batch([s[0] for s in order], [s[1] for s in order], samples=list(samples),
                                         want_tries=True, **kw)
    assert all(same_fit(a, b) for a, b in zip(fits, host))
    assert np.array_equal(hinl, inl) and np.array_equal(hcams.view(np.uint64), cams.view(np.uint64))


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_example_registers_every_view():
    """The example's --resect step on a small scene: every view is registered from the best fitted pair on, and the
    resected cameras are the scene's in the seed's gauge.  The bounds are what the inlier bound allows, not what the
    run gives: 2 px at f = 1000 px subtend atan(2 / 1000) = 0.115 degrees, and a centre moved by d baselines moves the
    image of a point at depth z (4 to 8 baselines here) by f d / z px, so 2 px allow d <= 2 x 8 / 1000."""
    from examples.multiview_from_sift_tables import camera_parts, multiview_pipeline, resect_views, synthetic_sift_views
    tables, K, scene = synthetic_sift_views(0, 5, 600, return_cameras=True)
    out = multiview_pipeline(tables, K, tracks=True)
    reg = resect_views(out, K, 2.0)
    d, q = reg["seed"]
    assert sorted(reg["views"] + [d, q]) == list(range(5)) and all(c is not None for c in reg["cameras"])
    Rd, Cd = camera_parts(scene[d], K)
    scale = np.linalg.norm(camera_parts(reg["cameras"][q], K)[1]) / np.linalg.norm(Rd @ (camera_parts(scene[q], K)[1] - Cd))
    for i, (v, f) in enumerate(zip(reg["views"], reg["fits"])):
        rows = int(reg["view_off"][i + 1] - reg["view_off"][i])
        assert f["success"] and rows > 300 and len(f["inlier_idx"]) >= 0.6 * rows, (v, rows)
        R, C = camera_parts(f["camera"], K)
        Rs, Cs = camera_parts(scene[v], K)
        Rs, Cs = Rs @ Rd.T, scale * (Rd @ (Cs - Cd))
        angle = np.degrees(np.arccos(np.clip((np.trace(R @ Rs.T) - 1) / 2, -1, 1)))
        print("view %d: %d rows, %d inliers, rotation off by %.2e deg, centre by %.2e baselines" % (
            v, rows, len(f["inlier_idx"]), angle, np.linalg.norm(C - Cs)))
        assert angle <= 0.115 and np.linalg.norm(C - Cs) <= 0.016, (v, angle, np.linalg.norm(C - Cs))
    X, err, ok, nused = reg["points"]
    assert int(ok.sum()) >= 0.9 * len(ok) and int(nused.max()) == 5


# ---- names ------------------------------------------------------------------------------------------------------------
def test_profile_names(gather_case, mixed):
    from spectavi_amd import device
    c = gather_case
    col, seeds, tries = mixed
    device.profile_enable(True)
    try:
        device.profile_reset()
        device.resect_gather(cuda(c["geom"]), cuda(c["track"]), c["seg"], c["views"], cuda(c["X"]))
        fit(col, required_percent_inliers=0.6, max_error=1.0, maximum_tries=tries, seeds=seeds)
        counts = [device.profile_read(k)[0] for k in PROFILE_NAMES]
    finally:
        device.profile_enable(False)
        device.profile_reset()
    assert counts == [1, 2, 2, 2], counts        # one gather; two rounds: 256 tries, then the pure-outlier set's other 344


def test_kernel_coverage_lists_the_instantiations():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_coverage.py"), "--list",
                          "--files", "resect_batch.hip"], check=True, capture_output=True, text=True).stdout
    listed = {ln.strip() for ln in out.splitlines() if ln.startswith("  ")}
    assert listed == INSTANTIATED, out
