"""dlt_triangulate_batch on the GPU: every selected row of every set is bit for bit what the single calls
(device.dlt_triangulate, device.dlt_reprojection_error) return for that row with its set's cameras, whatever the
sizes, the mask, the skipped sets and the capacity.  Bits are compared through .view(int64): NaNs compare equal."""
import ctypes as ct
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import dlt_checks as dc
from tests import ransac_batch_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 513]
P0_EYE = np.hstack([np.eye(3), np.zeros((3, 1))])


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def make_collection(sizes, seed, p0_eye=False):
    """Per set a random camera pair and points seen by both; rows 0, 2, 5, ... of a set get w = 0 or NaN entries."""
    rng = np.random.default_rng(seed)
    P0s, P1s, x0s, x1s = [], [], [], []
    for k, n in enumerate(sizes):
        P0 = P0_EYE.copy() if p0_eye else rng.standard_normal((3, 4))
        P1 = rng.standard_normal((3, 4))
        Xw = np.hstack([rng.standard_normal((n, 3)) + [0, 0, 5], np.ones((n, 1))])
        x0, x1 = Xw @ P0.T, Xw @ P1.T
        x1[:, :2] += 1e-3 * rng.standard_normal((n, 2))
        if n > 0:
            x0[0, 2] = 0.0            # a point at infinity in the first view
        if n > 2:
            x1[2, 1] = np.nan
        if n > 5:
            x0[5] = np.nan
            x1[n - 1, 2] = 0.0
        if n > 70:
            x0[67, 0] = np.inf
        P0s.append(P0)
        P1s.append(P1)
        x0s.append(x0)
        x1s.append(x1)
    return P0s, P1s, x0s, x1s


@pytest.fixture(scope="module")
def edge():
    """The edge-size collection on the device with its single-call results per set, computed once."""
    import torch
    from spectavi_amd import device as spv
    P0s, P1s, x0s, x1s = make_collection(EDGE_SIZES, 11)
    off = rc.offsets(x0s)
    x0, x1 = torch.from_numpy(np.concatenate(x0s)).cuda(), torch.from_numpy(np.concatenate(x1s)).cuda()
    X, E = [], []
    for p in range(len(EDGE_SIZES)):
        a, b = x0[off[p]:off[p + 1]].contiguous(), x1[off[p]:off[p + 1]].contiguous()
        X.append(spv.dlt_triangulate(P0s[p], P1s[p], a, b).cpu().numpy())
        E.append(spv.dlt_reprojection_error(P0s[p], P1s[p], a, b).cpu().numpy().reshape(-1))
    assert np.isnan(np.concatenate(E)).any() and np.isfinite(np.concatenate(E)).sum() > 1400   # of 1474 rows
    return dict(P0s=P0s, P1s=P1s, x0=x0, x1=x1, off=off, X=X, E=E)


def single_results(P0s, P1s, x0, x1, off, sel):
    """The single calls on the gathered rows sel[p] (index arrays) of every set; None entries are skipped sets."""
    import torch
    from spectavi_amd import device as spv
    X, E = [], []
    for p, idx in enumerate(sel):
        if idx is None or len(idx) == 0:
            X.append(np.zeros((0, 4)))
            E.append(np.zeros(0))
            continue
        rows = torch.from_numpy(np.asarray(idx, np.int64) + int(off[p])).cuda()
        a, b = x0[rows].contiguous(), x1[rows].contiguous()
        X.append(spv.dlt_triangulate(P0s[p], P1s[p], a, b).cpu().numpy())
        E.append(spv.dlt_reprojection_error(P0s[p], P1s[p], a, b).cpu().numpy().reshape(-1))
    return X, E


def assert_same(X, E, out_off, wantX, wantE, what):
    n = int(out_off[-1])
    assert n == sum(len(a) for a in wantX), what
    assert np.array_equal(bits(X[:n]), bits(np.concatenate(wantX))), what
    assert np.array_equal(bits(E[:n]), bits(np.concatenate(wantE))), what


def test_edge_sizes_without_a_mask(edge):
    from spectavi_amd import device as spv
    X, E, rows, out_off = spv.dlt_triangulate_batch(edge["x0"], edge["x1"], edge["off"], edge["P1s"], P0s=edge["P0s"],
                                                    want_error=True, want_rows=True)
    assert out_off.dtype == np.int64 and np.array_equal(out_off, edge["off"])
    assert_same(X, E, out_off, edge["X"], edge["E"], "edge sizes")
    assert np.array_equal(rows.cpu().numpy(), np.concatenate([np.arange(n) for n in EDGE_SIZES]))
    # X alone and the error alone are the same bits
    X2, off2 = spv.dlt_triangulate_batch(edge["x0"], edge["x1"], edge["off"], edge["P1s"], P0s=edge["P0s"])
    assert np.array_equal(bits(X2), bits(X)) and np.array_equal(off2, out_off)


def test_no_first_cameras_means_identity():
    import torch
    from spectavi_amd import device as spv
    P0s, P1s, x0s, x1s = make_collection(EDGE_SIZES, 12, p0_eye=True)
    off = rc.offsets(x0s)
    x0, x1 = torch.from_numpy(np.concatenate(x0s)).cuda(), torch.from_numpy(np.concatenate(x1s)).cuda()
    X, E, out_off = spv.dlt_triangulate_batch(x0, x1, off, P1s, want_error=True)
    Xe, Ee, _ = spv.dlt_triangulate_batch(x0, x1, off, P1s, P0s=P0s, want_error=True)
    assert np.array_equal(bits(X), bits(Xe)) and np.array_equal(bits(E), bits(Ee))
    wantX, wantE = single_results(P0s, P1s, x0, x1, off, [np.arange(n) for n in EDGE_SIZES])
    assert_same(X, E, out_off, wantX, wantE, "P0s=None")


def _run_masked(edge, mask, use=None, P1s=None):
    import torch
    from spectavi_amd import device as spv
    m = torch.from_numpy(mask.astype(np.uint8)).cuda()
    return spv.dlt_triangulate_batch(edge["x0"], edge["x1"], edge["off"], edge["P1s"] if P1s is None else P1s,
                                     P0s=edge["P0s"], use=use, mask=m, want_error=True, want_rows=True)


@pytest.mark.parametrize("density", [0.0, 0.5, 1.0])
def test_mask_densities(edge, density):
    off = edge["off"]
    mask = (np.random.default_rng(5).random(int(off[-1])) < density).astype(np.uint8) * 7   # any non-zero byte selects
    X, E, rows, out_off = _run_masked(edge, mask)
    sel = [np.flatnonzero(mask[off[p]:off[p + 1]]) for p in range(len(EDGE_SIZES))]
    assert np.array_equal(out_off, np.concatenate([[0], np.cumsum([len(s) for s in sel])]))
    n = int(out_off[-1])
    assert n == int((mask != 0).sum()) and (density > 0) == (n > 0)
    assert np.array_equal(rows[:n].cpu().numpy(), np.concatenate(sel))
    wantX = [edge["X"][p][sel[p]] for p in range(len(EDGE_SIZES))]
    wantE = [edge["E"][p][sel[p]] for p in range(len(EDGE_SIZES))]
    assert_same(X, E, out_off, wantX, wantE, "density %g" % density)
    if density == 0.5:   # ... which are the single calls' bits on the gathered rows, too
        gX, gE = single_results(edge["P0s"], edge["P1s"], edge["x0"], edge["x1"], off, sel)
        assert_same(X, E, out_off, gX, gE, "gathered rows")


@pytest.mark.parametrize("row", [0, 63, 64, 255, 256])
def test_a_single_selected_row_of_a_257_row_set(edge, row):
    off = edge["off"]
    p = EDGE_SIZES.index(257)
    mask = np.zeros(int(off[-1]), np.uint8)
    mask[off[p] + row] = 1
    X, E, rows, out_off = _run_masked(edge, mask)
    assert np.array_equal(out_off, (np.arange(len(off)) > p).astype(np.int64))
    assert rows[:1].cpu().numpy().tolist() == [row]
    assert np.array_equal(bits(X[:1]), bits(edge["X"][p][row:row + 1]))
    assert np.array_equal(bits(E[:1]), bits(edge["E"][p][row:row + 1]))


def test_an_all_zero_set_between_two_full_ones(edge):
    off = edge["off"]
    a, z, b = (EDGE_SIZES.index(n) for n in (255, 256, 257))
    mask = np.zeros(int(off[-1]), np.uint8)
    mask[off[a]:off[a + 1]] = 1
    mask[off[b]:off[b + 1]] = 255
    X, E, rows, out_off = _run_masked(edge, mask)
    assert out_off[z] == out_off[z + 1] == 255 and out_off[-1] == 255 + 257
    assert np.array_equal(rows[:512].cpu().numpy(), np.concatenate([np.arange(255), np.arange(257)]))
    assert_same(X, E, out_off, [edge["X"][a], edge["X"][b]], [edge["E"][a], edge["E"][b]], "zero set between full ones")


def test_skipped_sets_own_no_rows_and_their_cameras_are_not_read(edge):
    from spectavi_amd import device as spv
    off = edge["off"]
    use = np.array([1, 1, 0, 1, 1, 0, 1, 0, 1], np.int32)
    nan_cams = [P if u else np.full((3, 4), np.nan) for P, u in zip(edge["P1s"], use)]
    keep = [p for p in range(len(use)) if use[p]]
    want_off = np.concatenate([[0], np.cumsum(np.array(EDGE_SIZES) * use)])
    results = []
    for P1s in (edge["P1s"], nan_cams):
        X, E, rows, out_off = spv.dlt_triangulate_batch(edge["x0"], edge["x1"], off, P1s, P0s=edge["P0s"], use=use,
                                                        want_error=True, want_rows=True)
        assert np.array_equal(out_off, want_off)
        for p in np.flatnonzero(use == 0):
            assert out_off[p] == out_off[p + 1]
        assert_same(X, E, out_off, [edge["X"][p] for p in keep], [edge["E"][p] for p in keep], "use")
        assert np.array_equal(rows[:out_off[-1]].cpu().numpy(), np.concatenate([np.arange(EDGE_SIZES[p]) for p in keep]))
        results.append((bits(X[:out_off[-1]]), bits(E[:out_off[-1]])))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1])
    # a None entry of the camera list is a skipped set; with a mask on top
    listed = [P if u else None for P, u in zip(edge["P1s"], use)]
    mask = (np.random.default_rng(8).random(int(off[-1])) < 0.5).astype(np.uint8)
    X, E, rows, out_off = _run_masked(edge, mask, P1s=listed)
    sel = [np.flatnonzero(mask[off[p]:off[p + 1]]) if use[p] else np.zeros(0, np.int64) for p in range(len(use))]
    assert np.array_equal(out_off, np.concatenate([[0], np.cumsum([len(s) for s in sel])]))
    assert_same(X, E, out_off, [edge["X"][p][sel[p]] for p in range(len(use))],
                [edge["E"][p][sel[p]] for p in range(len(use))], "use and mask")


def test_a_set_gives_the_same_bits_wherever_it_stands(edge):
    import torch
    from spectavi_amd import device as spv
    off = edge["off"]
    p = EDGE_SIZES.index(513)
    other = [EDGE_SIZES.index(65), EDGE_SIZES.index(257)]
    mask_p = (np.random.default_rng(9).random(513) < 0.6).astype(np.uint8)
    for place in (0, 1, 2):
        order = other[:place] + [p] + other[place:]
        x0 = torch.cat([edge["x0"][off[q]:off[q + 1]] for q in order]).contiguous()
        x1 = torch.cat([edge["x1"][off[q]:off[q + 1]] for q in order]).contiguous()
        sizes = [EDGE_SIZES[q] for q in order]
        o = np.concatenate([[0], np.cumsum(sizes)])
        mask = np.concatenate([mask_p if q == p else np.ones(EDGE_SIZES[q], np.uint8) for q in order])
        X, E, out_off = spv.dlt_triangulate_batch(x0, x1, o, [edge["P1s"][q] for q in order],
                                                  P0s=[edge["P0s"][q] for q in order],
                                                  mask=torch.from_numpy(mask).cuda(), want_error=True)
        got = slice(int(out_off[place]), int(out_off[place + 1]))
        assert np.array_equal(bits(X[got]), bits(edge["X"][p][mask_p != 0])), place
        assert np.array_equal(bits(E[got]), bits(edge["E"][p][mask_p != 0])), place


def _raw(edge, mask, capacity, X, E, rows, d_off, d_count, stream=None):
    """spv_dlt_triangulate_batch_device into the caller's tensors; on `stream` without waiting for it, else on the
    current stream and waited for."""
    import torch
    from spectavi_amd._lib import clib
    off = edge["off"]
    P0 = np.ascontiguousarray(np.stack(edge["P0s"]).reshape(-1, 12))
    P1 = np.ascontiguousarray(np.stack(edge["P1s"]).reshape(-1, 12))
    st = clib.spv_dlt_triangulate_batch_device(
        edge["x0"].data_ptr(), edge["x1"].data_ptr(), off.ctypes.data, len(off) - 1, P0.ctypes.data, P1.ctypes.data, None,
        mask.data_ptr() if mask is not None else None, X.data_ptr(), E.data_ptr(), rows.data_ptr(), capacity,
        d_off.data_ptr(), d_count.data_ptr(), ct.c_void_p((torch.cuda.current_stream() if stream is None else stream).cuda_stream))
    if stream is None:
        torch.cuda.synchronize()
    return st


def test_calls_in_flight_on_two_streams_keep_their_scratch(edge):
    """Six calls alternating between the current stream and a second one with no wait in between, masks of
    different densities: a call's scratch (its tables and out bases, from the library's cache) must not reach a
    later call while its own kernels are still queued.  Releasing the cache afterwards waits for all of them."""
    import torch
    from spectavi_amd._lib import clib
    off = edge["off"]
    total = int(off[-1])
    side = torch.cuda.Stream()
    calls = []
    for k, density in enumerate((0.5, 0.9, 0.1, 1.0, 0.3, 0.7)):
        mask_h = (np.random.default_rng(40 + k).random(total) < density).astype(np.uint8)
        outs = (torch.full((total, 4), -77.0, dtype=torch.float64, device="cuda"),
                torch.full((total,), -77.0, dtype=torch.float64, device="cuda"),
                torch.full((total,), -77, dtype=torch.int32, device="cuda"),
                torch.full((len(off),), -1, dtype=torch.int64, device="cuda"),
                torch.full((1,), -1, dtype=torch.int64, device="cuda"))
        calls.append((mask_h, torch.from_numpy(mask_h).cuda(), outs))
    torch.cuda.synchronize()   # inputs and sentinels are there for both streams
    for k, (_, mask, outs) in enumerate(calls):
        assert _raw(edge, mask, total, *outs, stream=side if k % 2 else torch.cuda.current_stream()) == 0
    clib.spv_release_cached_memory()
    torch.cuda.synchronize()
    for mask_h, _, (X, E, rows, d_off, d_count) in calls:
        sel = [np.flatnonzero(mask_h[off[p]:off[p + 1]]) for p in range(len(EDGE_SIZES))]
        n = int(mask_h.sum())
        assert int(d_count.item()) == n
        assert np.array_equal(d_off.cpu().numpy(), np.concatenate([[0], np.cumsum([len(s) for s in sel])]))
        assert np.array_equal(rows[:n].cpu().numpy(), np.concatenate(sel))
        assert_same(X, E, d_off.cpu().numpy(), [edge["X"][p][sel[p]] for p in range(len(EDGE_SIZES))],
                    [edge["E"][p][sel[p]] for p in range(len(EDGE_SIZES))], "two streams")
        assert bool((X[n:] == -77.0).all()) and bool((rows[n:] == -77).all())


@pytest.mark.parametrize("masked", [False, True])
def test_capacity_below_and_at_the_count(edge, masked):
    """Rows at and beyond min(count, capacity) keep a sentinel; d_count and d_out_off hold the true numbers."""
    import torch
    off = edge["off"]
    total = int(off[-1])
    mask_h = (np.random.default_rng(6).random(total) < 0.5).astype(np.uint8) if masked else np.ones(total, np.uint8)
    mask = torch.from_numpy(mask_h).cuda() if masked else None
    sel = [np.flatnonzero(mask_h[off[p]:off[p + 1]]) for p in range(len(EDGE_SIZES))]
    count = int(mask_h.sum())
    wantX = np.concatenate([edge["X"][p][sel[p]] for p in range(len(EDGE_SIZES))])
    wantE = np.concatenate([edge["E"][p][sel[p]] for p in range(len(EDGE_SIZES))])
    want_off = np.concatenate([[0], np.cumsum([len(s) for s in sel])])
    for capacity in (count - 300, count, 0):
        X = torch.full((total + 8, 4), -77.0, dtype=torch.float64, device="cuda")
        E = torch.full((total + 8,), -77.0, dtype=torch.float64, device="cuda")
        rows = torch.full((total + 8,), -77, dtype=torch.int32, device="cuda")
        d_off = torch.full((len(off),), -1, dtype=torch.int64, device="cuda")
        d_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        assert _raw(edge, mask, capacity, X, E, rows, d_off, d_count) == 0
        assert int(d_count.item()) == count and np.array_equal(d_off.cpu().numpy(), want_off)
        assert np.array_equal(bits(X[:capacity]), bits(wantX[:capacity])), capacity
        assert np.array_equal(bits(E[:capacity]), bits(wantE[:capacity])), capacity
        assert np.array_equal(rows[:capacity].cpu().numpy(), np.concatenate(sel)[:capacity])
        assert bool((X[capacity:] == -77.0).all()) and bool((E[capacity:] == -77.0).all()) and bool((rows[capacity:] == -77).all())


def test_host_form_and_mvg_wrapper_equal_the_device_form(edge):
    from spectavi_amd import mvg
    from spectavi_amd._lib import clib, SPV_ERR_INVALID, SPV_ERR_OVERFLOW
    off = edge["off"]
    total = int(off[-1])
    x0, x1 = edge["x0"].cpu().numpy(), edge["x1"].cpu().numpy()
    mask = (np.random.default_rng(4).random(total) < 0.5).astype(np.uint8)
    use = np.array([1, 1, 1, 1, 0, 1, 1, 1, 1], np.int32)
    X, E, rows, out_off = _run_masked(edge, mask, use=use)
    n = int(out_off[-1])
    P0 = np.ascontiguousarray(np.stack(edge["P0s"]).reshape(-1, 12))
    P1 = np.ascontiguousarray(np.stack(edge["P1s"]).reshape(-1, 12))

    def host(capacity, npairs=len(EDGE_SIZES)):
        hX, hE, hr = np.full((total, 4), -77.0), np.full(total, -77.0), np.full(total, -77, np.int32)
        ho, hc = np.full(len(off), -1, np.int64), ct.c_longlong(-1)
        st = clib.spv_dlt_triangulate_batch(x0.ctypes.data, x1.ctypes.data, off.ctypes.data, npairs, P0.ctypes.data,
                                            P1.ctypes.data, use.ctypes.data, mask.ctypes.data, hX.ctypes.data, hE.ctypes.data,
                                            hr.ctypes.data, capacity, ho.ctypes.data, ct.addressof(hc))
        return st, hX, hE, hr, ho, hc.value

    st, hX, hE, hr, ho, hc = host(total)
    assert st == 0 and hc == n and np.array_equal(ho, out_off)
    assert np.array_equal(bits(hX[:n]), bits(X[:n])) and np.array_equal(bits(hE[:n]), bits(E[:n]))
    assert np.array_equal(hr[:n], rows[:n].cpu().numpy())
    assert np.all(hX[n:] == -77.0) and np.all(hE[n:] == -77.0) and np.all(hr[n:] == -77)
    # a capacity below the count: the rows that fit, the true count, SPV_ERR_OVERFLOW
    st, hX, hE, hr, ho, hc = host(n - 100)
    assert st == SPV_ERR_OVERFLOW and hc == n and np.array_equal(ho, out_off)
    assert np.array_equal(bits(hX[:n - 100]), bits(X[:n - 100])) and np.all(hX[n - 100:] == -77.0) and np.all(hr[n - 100:] == -77)
    # invalid arguments leave every output as it was
    for bad in (dict(capacity=-1), dict(capacity=total, npairs=-2)):
        st, hX, hE, hr, ho, hc = host(**bad)
        assert st == SPV_ERR_INVALID and hc == -1 and np.all(ho == -1)
        assert np.all(hX == -77.0) and np.all(hE == -77.0) and np.all(hr == -77)
    # the list front-end
    cams = [P if u else None for P, u in zip(edge["P1s"], use)]
    x0s = [x0[off[p]:off[p + 1]] for p in range(len(use))]
    x1s = [x1[off[p]:off[p + 1]] for p in range(len(use))]
    masks = [mask[off[p]:off[p + 1]] for p in range(len(use))]
    Xs, Es = mvg.dlt_triangulate_batch(cams, x0s, x1s, P0s=edge["P0s"], masks=masks, ret_error=True)
    assert [len(a) for a in Xs] == np.diff(out_off).tolist() and len(Xs[4]) == 0 and Xs[4].shape == (0, 4)
    assert all(e.shape == (len(a), 1) for a, e in zip(Xs, Es))
    assert np.array_equal(bits(np.concatenate(Xs)), bits(X[:n]))
    assert np.array_equal(bits(np.concatenate(Es).reshape(-1)), bits(E[:n]))
    assert np.array_equal(bits(np.concatenate(mvg.dlt_triangulate_batch(cams, x0s, x1s, P0s=edge["P0s"], masks=masks))), bits(X[:n]))


def test_after_ransac_fit_batch_end_to_end():
    """ransac_fit_batch(want_mask=True), then every set's inliers with that set's camera: the rows are the fits'
    inlier lists, X is mvg.dlt_triangulate on the gathered rows bit for bit, the noise-free errors sit far below the
    threshold, and the points meet the definition check of the single-call tests."""
    import torch
    from spectavi_amd import device as spv
    from spectavi_amd import mvg
    sizes = [9, 10, 257, 2500]
    x0s, x1s, smp, _ = rc.collection(sizes, [0.0, 0.0, 0.2, 0.3], 300, 4100)
    off = rc.offsets(x0s)
    x0, x1 = torch.from_numpy(np.concatenate(x0s)).cuda(), torch.from_numpy(np.concatenate(x1s)).cuda()
    fits, mask = spv.ransac_fit_batch(x0, x1, off, required_percent_inliers=0.6, reprojection_error_allowed=rc.THRESHOLD,
                                      samples=np.stack(smp), want_mask=True)
    use = [f['best_try'] >= 0 for f in fits]
    assert use == [False, True, True, True]
    X, E, rows, out_off = spv.dlt_triangulate_batch(x0, x1, off, [f['camera'] for f in fits], use=use, mask=mask,
                                                    want_error=True, want_rows=True)
    assert np.array_equal(np.diff(out_off), [len(f['inlier_idx']) for f in fits]) and out_off[1] == 0
    n = int(out_off[-1])
    assert n > 0.6 * 2500
    assert bool((E[:n] < rc.THRESHOLD).all()) and float(E[:n].median()) < 1e-9   # planted inliers reproject to ~1e-15
    for p, f in enumerate(fits):
        idx = f['inlier_idx']
        got = slice(int(out_off[p]), int(out_off[p + 1]))
        assert np.array_equal(rows[got].cpu().numpy(), idx), p
        if not use[p]:
            continue
        want = mvg.dlt_triangulate(P0_EYE, f['camera'], x0s[p][idx], x1s[p][idx])
        assert np.array_equal(bits(X[got]), bits(want)), p
        st = dc.check_definition(X[got].cpu().numpy(), P0_EYE, f['camera'], x0s[p][idx], x1s[p][idx],
                                 err=E[got].cpu().numpy(), what="set %d" % p)
        assert st["points"] == len(idx)


def test_example_script_runs_in_a_fresh_process():
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "examples", "multiview_from_sift_tables.py"), "--images", "4", "--points", "300"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^pair (\d+)-(\d+): matches (\d+) model (yes|no) inliers (\d+) points (\d+)$", r.stdout, flags=re.M)
    assert len(lines) == 6, r.stdout
    fitted = [ln for ln in lines if ln[3] == "yes"]
    assert len(fitted) >= 4, r.stdout
    for _, _, matches, model, inliers, points in lines:
        assert int(points) == (int(inliers) if model == "yes" else 0), r.stdout
        if model == "yes":
            assert 150 <= int(inliers) <= int(matches), r.stdout
    total = re.search(r"^pairs 6 fitted (\d+) inliers (\d+) points (\d+)$", r.stdout, flags=re.M)
    assert total and int(total.group(1)) == len(fitted), r.stdout
