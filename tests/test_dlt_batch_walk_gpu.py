"""dlt_triangulate_batch on the GPU with more work items than the launch has workgroups.  The collection of
tests/test_dlt_batch_gpu.py has about 12 items; here the sizes of the sets cycle through CYCLE, and there are enough
sets for more than cap items (cap = 32 * compute units, the grid's limit in dlt_batch_run) even where `use` skips
every third set.  An empty set has no item, so a cycle of nine sets gives seven items, five with `use`: cap + 300
sets would stay below the cap, and the number of sets is raised from there until the items pass it.  Then

  dlt_batch_kernel<false, ...>   every workgroup walks b, b + cap, ...: X and err, X alone, err alone
  dlt_batch_count_kernel         walks the same way, s_wsum reused behind its second barrier
  dlt_batch_scan_kernel          scans more than 1024 counts: the carry loop of block_scan_inplace takes several turns,
                                 the last one partial; out_off is read through set_item0 behind runs of sets without
                                 an item (two empty sets in every cycle, with `use` up to four, and one run of 300)
  dlt_batch_kernel<true, ...>    reuses s_wsum and s_list for its next item; lanes beyond an item's selected rows, and
                                 with a small capacity the lanes beyond the capacity, have left through `continue` and
                                 meet the others again at the next item's barrier.  The neighbours of an item in the
                                 walk are items of other sizes (1, 2, 3, 5 and 256 + 1 rows) and other cameras.

Two references, both independent of the batch kernel.  The single calls (device.dlt_triangulate and
device.dlt_reprojection_error, one of each per camera pair on the gathered rows of all its sets), bit for bit and
row by row: a row's arithmetic depends only on the row and its cameras, which is the contract dlt_batch.hip states.
And tests/dlt_checks.py's check_definition per camera pair, the LAPACK statement of what a triangulation is.  Bits
are compared through .view(int64)."""
import ctypes as ct

import numpy as np
import pytest

from tests import dlt_checks as dc

pytestmark = pytest.mark.gpu

CYCLE = [1, 2, 0, 3, 257, 1, 0, 0, 5]
NCAMS = 4
ZERO_TAIL = 200  # the last sets whose mask is all zero


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def sizes_of(npairs):
    return np.array([CYCLE[p % len(CYCLE)] for p in range(npairs)], np.int64)


def use_of(npairs):
    """use = 0 for every third set, and for 300 sets in a row a quarter of the way in."""
    use = (np.arange(npairs) % 3 != 2).astype(np.int32)
    use[npairs // 4:npairs // 4 + 300] = 0
    return use


def used_items(sizes, use):
    return int((-(-sizes // 256) * (use != 0)).sum())


@pytest.fixture(scope="module")
def walk():
    """The collection on the device, the single calls' results for every row, and the plan's numbers; computed once."""
    import torch
    from spectavi_amd import device as spv
    cap = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    npairs = cap + 300
    while used_items(sizes_of(npairs), use_of(npairs)) <= cap:
        npairs += len(CYCLE)
    sizes = sizes_of(npairs)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(off[-1])
    set_of = np.repeat(np.arange(npairs), sizes)
    cam_of = set_of % NCAMS
    rng = np.random.default_rng(31)
    P0c, P1c = rng.standard_normal((NCAMS, 3, 4)), rng.standard_normal((NCAMS, 3, 4))
    # make_collection's recipe (tests/test_dlt_batch_gpu.py) without its planted non-finite rows
    Xw = np.hstack([rng.standard_normal((total, 3)) + [0, 0, 5], np.ones((total, 1))])
    x0 = np.einsum("nj,nij->ni", Xw, P0c[cam_of])
    x1 = np.einsum("nj,nij->ni", Xw, P1c[cam_of])
    x1[:, :2] += 1e-3 * rng.standard_normal((total, 2))
    d_x0, d_x1 = torch.from_numpy(x0).cuda(), torch.from_numpy(x1).cuda()
    X, E = np.empty((total, 4)), np.empty(total)
    for c in range(NCAMS):
        idx = np.flatnonzero(cam_of == c)
        rows = torch.from_numpy(idx).cuda()
        a, b = d_x0[rows].contiguous(), d_x1[rows].contiguous()
        X[idx] = spv.dlt_triangulate(P0c[c], P1c[c], a, b).cpu().numpy()
        E[idx] = spv.dlt_reprojection_error(P0c[c], P1c[c], a, b).cpu().numpy().reshape(-1)
    assert np.isfinite(X).all() and np.isfinite(E).all()
    mask = np.random.default_rng(32).integers(1, 256, total).astype(np.uint8) * (np.random.default_rng(33).random(total) < 0.5)
    mask[off[npairs - ZERO_TAIL]:] = 0
    return dict(cap=cap, npairs=npairs, sizes=sizes, off=off, total=total, set_of=set_of, cam_of=cam_of,
                row_in_set=np.arange(total) - off[set_of], P0c=P0c, P1c=P1c, P0s=P0c[np.arange(npairs) % NCAMS],
                P1s=P1c[np.arange(npairs) % NCAMS], x0=x0, x1=x1, d_x0=d_x0, d_x1=d_x1, X=X, E=E, mask=mask.astype(np.uint8))


def selected(w, mask, use=None):
    """numpy's statement of the selection: (the selected rows in input order, out_off)."""
    keep = mask != 0 if use is None else (mask != 0) & (np.asarray(use)[w["set_of"]] != 0)
    per_set = np.bincount(w["set_of"][keep], minlength=w["npairs"])
    return np.flatnonzero(keep), np.concatenate([[0], np.cumsum(per_set)]).astype(np.int64)


def raw(w, mask, use, P1s, capacity, X, E, rows, d_off, d_count):
    """spv_dlt_triangulate_batch_device into the caller's tensors (None: not wanted), waited for."""
    import torch
    from spectavi_amd._lib import clib
    P0 = np.ascontiguousarray(w["P0s"].reshape(-1, 12))
    P1 = np.ascontiguousarray(np.asarray(P1s).reshape(-1, 12))
    use = None if use is None else np.ascontiguousarray(use, dtype=np.int32)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    st = clib.spv_dlt_triangulate_batch_device(
        w["d_x0"].data_ptr(), w["d_x1"].data_ptr(), w["off"].ctypes.data, w["npairs"], P0.ctypes.data, P1.ctypes.data,
        None if use is None else use.ctypes.data, ptr(mask), ptr(X), ptr(E), ptr(rows), capacity, ptr(d_off), ptr(d_count),
        ct.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st


def test_the_collection_is_past_the_caps(walk):
    """What the other tests of this module rely on, from the plan and the device's compute units."""
    from spectavi_amd import device as spv
    plan = spv.dlt_triangulate_batch_plan(walk["off"])
    assert walk["npairs"] >= walk["cap"] + 300
    assert plan["items"] == int((-(-walk["sizes"] // 256)).sum()) and plan["bound"] == walk["total"]
    assert plan["items"] > walk["cap"], "every workgroup walks a second item"
    assert walk["cap"] > 1024 and plan["items"] > 1024, "the scan takes a second turn"
    assert plan["items"] % 1024 != 0, "... and its last turn is partial"
    assert walk["total"] <= 1100000
    # every size of the cycle meets every camera pair
    assert len({(int(n), p % NCAMS) for p, n in enumerate(walk["sizes"])}) == len(set(CYCLE)) * NCAMS


def test_no_mask(walk):
    """X and err together, X alone, err alone: the three dlt_batch_kernel<false, ...> forms."""
    import torch
    from spectavi_amd import device as spv
    w = walk
    X, E, rows, out_off = spv.dlt_triangulate_batch(w["d_x0"], w["d_x1"], w["off"], w["P1s"], P0s=w["P0s"],
                                                    want_error=True, want_rows=True)
    assert np.array_equal(out_off, w["off"])
    assert np.array_equal(bits(X), bits(w["X"])), "X, with err"
    assert np.array_equal(bits(E), bits(w["E"])), "err, with X"
    assert np.array_equal(rows.cpu().numpy(), w["row_in_set"])
    X2, off2 = spv.dlt_triangulate_batch(w["d_x0"], w["d_x1"], w["off"], w["P1s"], P0s=w["P0s"])
    assert np.array_equal(bits(X2), bits(w["X"])) and np.array_equal(off2, w["off"]), "X alone"
    E3 = torch.full((w["total"] + 8,), -77.0, dtype=torch.float64, device="cuda")
    assert raw(w, None, None, w["P1s"], w["total"], None, E3, None, None, None) == 0
    assert np.array_equal(bits(E3[:w["total"]]), bits(w["E"])) and bool((E3[w["total"]:] == -77.0).all()), "err alone"
    # the LAPACK statement, on the batch call's own output
    Xh, Eh = X.cpu().numpy(), E.cpu().numpy()
    points = 0
    for c in range(NCAMS):
        idx = np.flatnonzero(w["cam_of"] == c)
        st = dc.check_definition(Xh[idx], w["P0c"][c], w["P1c"][c], w["x0"][idx], w["x1"][idx], err=Eh[idx],
                                 what="camera pair %d" % c)
        points += st["points"]
    assert points == w["total"]


def check_masked(w, got, mask, use, what):
    X, E, rows, out_off = got
    sel, want_off = selected(w, mask, use)
    assert np.array_equal(out_off, want_off), "%s: out_off" % what
    n = len(sel)
    assert int(out_off[-1]) == n
    assert np.array_equal(rows[:n].cpu().numpy(), w["row_in_set"][sel]), "%s: rows" % what
    assert np.array_equal(bits(X[:n]), bits(w["X"][sel])), "%s: X" % what
    assert np.array_equal(bits(E[:n]), bits(w["E"][sel])), "%s: err" % what
    return sel, want_off


def test_random_mask(walk):
    """Density 0.5, any non-zero byte selects; the last 200 sets select nothing, so out_off ends in a long flat run."""
    import torch
    from spectavi_amd import device as spv
    w = walk
    mask = w["mask"]
    assert 0.45 < (mask != 0).mean() < 0.55 and len(np.unique(mask)) > 200
    got = spv.dlt_triangulate_batch(w["d_x0"], w["d_x1"], w["off"], w["P1s"], P0s=w["P0s"],
                                    mask=torch.from_numpy(mask).cuda(), want_error=True, want_rows=True)
    sel, want_off = check_masked(w, got, mask, None, "mask")
    assert (want_off[-ZERO_TAIL - 1:] == len(sel)).all() and want_off[-ZERO_TAIL - 1 - len(CYCLE)] < len(sel)


def test_skipped_sets(walk):
    """The mask plus use = 0 for every third set and for 300 sets in a row; their second cameras are NaN and must not
    be read.  out_off of a skipped set is read through set_item0 from the first item behind it."""
    import torch
    from spectavi_amd import device as spv
    w = walk
    use = use_of(w["npairs"])
    a, b = w["npairs"] // 4, w["npairs"] // 4 + 300
    assert not use[a:b].any() and not use[2::3].any() and use[0::3].sum() + use[1::3].sum() == use.sum()
    P1s = np.where(use[:, None, None] != 0, w["P1s"], np.nan)
    plan = spv.dlt_triangulate_batch_plan(w["off"], use=use)
    assert plan["sets"] == int(use.sum()) and plan["items"] == used_items(w["sizes"], use)
    assert plan["items"] > w["cap"] > 1024
    got = spv.dlt_triangulate_batch(w["d_x0"], w["d_x1"], w["off"], P1s, P0s=w["P0s"], use=use,
                                    mask=torch.from_numpy(w["mask"]).cuda(), want_error=True, want_rows=True)
    sel, want_off = check_masked(w, got, w["mask"], use, "use and mask")
    assert want_off[a] == want_off[b] and 0 < want_off[a] < want_off[b + len(CYCLE)]
    assert np.isfinite(got[0][:len(sel)].cpu().numpy()).all()
    # without a mask the host states out_off; the kernel still walks past the skipped sets
    X, E, out_off = spv.dlt_triangulate_batch(w["d_x0"], w["d_x1"], w["off"], P1s, P0s=w["P0s"], use=use, want_error=True)
    keep = np.flatnonzero(use[w["set_of"]] != 0)
    assert np.array_equal(out_off, np.concatenate([[0], np.cumsum(w["sizes"] * use)]))
    assert np.array_equal(bits(X[:len(keep)]), bits(w["X"][keep])) and np.array_equal(bits(E[:len(keep)]), bits(w["E"][keep]))


def test_small_capacity(walk):
    """Capacity 1000 below the count: rows from the capacity on keep their sentinel, everything before is unchanged,
    the count and out_off are the true ones."""
    import torch
    w = walk
    sel, want_off = selected(w, w["mask"])
    count = len(sel)
    capacity = count - 1000
    assert capacity > 0
    n = w["total"] + 8
    X = torch.full((n, 4), -77.0, dtype=torch.float64, device="cuda")
    E = torch.full((n,), -77.0, dtype=torch.float64, device="cuda")
    rows = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    d_off = torch.full((w["npairs"] + 1,), -1, dtype=torch.int64, device="cuda")
    d_count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    assert raw(w, torch.from_numpy(w["mask"]).cuda(), None, w["P1s"], capacity, X, E, rows, d_off, d_count) == 0
    assert int(d_count.item()) == count and np.array_equal(d_off.cpu().numpy(), want_off)
    assert np.array_equal(bits(X[:capacity]), bits(w["X"][sel[:capacity]]))
    assert np.array_equal(bits(E[:capacity]), bits(w["E"][sel[:capacity]]))
    assert np.array_equal(rows[:capacity].cpu().numpy(), w["row_in_set"][sel[:capacity]])
    assert bool((X[capacity:] == -77.0).all()) and bool((E[capacity:] == -77.0).all()) and bool((rows[capacity:] == -77).all())
