"""GPU: the guided many-pairs L1 2-NN (spv_l1k2_guided_batch_device, spv_nn_bruteforcel1k2_guided_batch) equals the
numpy oracle of tests/l1k2_guided_cases.py in idx, dist and ncand, elementwise, on inputs whose candidate decision
is exact under any evaluation order; and spv_epipolar_lines_batch_device equals numpy within the rounding of its
operations -- also past its caps: more pairs than one launch takes as kernel arguments (kLinesChunk = 32: the host loop
of epipolar_lines_run takes three turns, one of them skipped for having no query row) and a query set longer than
the 4096 x 256 rows one pass of the capped grid covers (the kernel's grid-stride loop).  tests/test_l1k2_guided_plan.py shows without a GPU that the collections get the items these cases are
written for."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import l1k2_guided_cases as gc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANTIATED = {"l1k2_guided_kernel", "epipolar_lines_kernel"}   # the finish kernel is l1k2_batch.hip's l1k2_finish_kernel


def run_device(tables, geoms, pairs, lines, max_dist):
    """device.l1k2_guided_batch on the concatenated tables -> (idx uint64, dist int32, ncand int32) on the host."""
    import torch
    from spectavi_amd import device
    rows = [len(t) for t in tables]
    desc = torch.from_numpy(np.concatenate(tables)).cuda() if sum(rows) else torch.zeros((0, 128), dtype=torch.uint8, device="cuda")
    geom = torch.from_numpy(np.concatenate(geoms)).cuda() if sum(rows) else torch.zeros((0, 4), dtype=torch.float32, device="cuda")
    ln = torch.from_numpy(np.array(lines, dtype=np.float64)).cuda()
    idx, dist, ncand, off = device.l1k2_guided_batch(desc, geom, gc.seg_of(rows), pairs, ln, max_dist, want_ncand=True)
    torch.cuda.synchronize()
    assert np.array_equal(off, np.concatenate([[0], np.cumsum([rows[q] for q, _ in pairs])]))
    return idx.cpu().numpy().view(np.uint64), dist.cpu().numpy(), ncand.cpu().numpy()


def assert_equal(got, want, what):
    for name, g, w in zip(("idx", "dist", "ncand"), got, want):
        bad = np.flatnonzero((g != w).reshape(len(w), -1).any(axis=1))
        assert bad.size == 0, "%s: %s differs in %d out rows, first %d: got %s, oracle %s" % (
            what, name, bad.size, bad[0], g[bad[0]], w[bad[0]])


@functools.lru_cache(maxsize=None)
def ragged_reference():
    tables, geoms, lines = gc.ragged()
    for a in tables + geoms + [lines]:
        a.setflags(write=False)
    return tables, geoms, lines, gc.oracle(tables, geoms, gc.FEW, lines, gc.RAGGED_DIST)


def out_rows_of(pair_number):
    o = sum(gc.NINE[q] for q, _ in gc.FEW[:pair_number])
    return slice(o, o + gc.NINE[gc.FEW[pair_number][0]])


def test_ragged_collection():
    tables, geoms, lines, want = ragged_reference()
    assert gc.is_dyadic(geoms, lines, gc.RAGGED_DIST)
    assert gc.ragged_counts_ok(want[2]), "candidate counts 0, 1 and 2 occur and a tenth of the rows have 3 or more"
    got = run_device(tables, geoms, gc.FEW, lines, gc.RAGGED_DIST)
    assert_equal(got, want, "ragged")
    # an empty database set: two sentinels, no candidates
    empty = out_rows_of(gc.FEW.index((8, 0)))
    assert (got[0][empty] == gc.NONE_IDX).all() and (got[1][empty] == gc.NONE_DIST).all() and not got[2][empty].any()


def test_one_row_database_inside_the_band():
    tables, geoms, lines, _ = ragged_reference()
    lines = lines.copy()
    one = out_rows_of(gc.FEW.index((8, 1)))
    u, v = (float(c) for c in geoms[1][0, :2])
    lines[one, 2] = -(lines[one, 0] * u + lines[one, 1] * v)      # every query's line through the one keypoint
    got = run_device(tables, geoms, gc.FEW, lines, gc.RAGGED_DIST)
    assert_equal(got, gc.oracle(tables, geoms, gc.FEW, lines, gc.RAGGED_DIST), "one-row database")
    assert (got[0][one] == np.array([0, gc.NONE_IDX], np.uint64)).all() and (got[2][one] == 1).all()
    assert (got[1][one, 1] == gc.NONE_DIST).all() and (got[1][one, 0] < gc.NONE_DIST).all()


def test_the_boundary_is_closed():
    rng = np.random.default_rng(21)
    nq, nd, md = 8, 300, 3.0
    tables = [rng.integers(0, 256, (nd, 128), dtype=np.uint8), rng.integers(0, 256, (nq, 128), dtype=np.uint8)]
    geoms = [gc.dyadic_geom(rng, nd), gc.dyadic_geom(rng, nq)]
    lines = np.zeros((nq, 3))
    for q in range(nq):
        # rows 2q and 2q + 1 are one step of the grid apart in u: with l0 = 2^-12 their s differ by 2^-16
        j, k, sign = 2 * q, 2 * q + 1, 1.0 if q % 2 == 0 else -1.0
        u, v = 100.0 + 16 * q, 50.0 + q
        geoms[0][j, :2] = (u, v)
        geoms[0][k, :2] = (u + sign / 16.0, v)
        l0, l1 = 1.0 / 4096, (q - 3) / 4096.0
        lines[q] = (l0, l1, sign * md - (l0 * u + l1 * v))   # s_j = +-md exactly, s_k = +-(md + 2^-16)
        tables[0][j] = tables[0][k] = tables[1][q]            # both at distance 0: only the band tells them apart
    assert gc.is_dyadic(geoms, lines, md)
    s = lines[:, 0:1] * geoms[0][:, 0].astype(np.float64) + lines[:, 1:2] * geoms[0][:, 1].astype(np.float64) + lines[:, 2:3]
    q = np.arange(nq)
    assert (np.abs(s[q, 2 * q]) == md).all() and (np.abs(s[q, 2 * q + 1]) == md + 2.0 ** -16).all()
    want = gc.oracle(tables, geoms, [(1, 0)], lines, md)
    mask = gc.candidate_mask(geoms[0], lines, md)
    assert mask[q, 2 * q].all() and not mask[q, 2 * q + 1].any()
    got = run_device(tables, geoms, [(1, 0)], lines, md)
    assert_equal(got, want, "boundary")
    assert (got[0][:, 0] == 2 * q).all() and (got[1][:, 0] == 0).all() and (got[2] == mask.sum(axis=1)).all()
    assert not (got[0] == (2 * q + 1)[:, None].astype(np.uint64)).any(), "the row just outside is never returned"


def test_ties_go_to_the_lower_row():
    rng = np.random.default_rng(22)
    tables = [np.tile(rng.integers(0, 256, (1, 128), dtype=np.uint8), (1000, 1)), rng.integers(0, 256, (2, 128), dtype=np.uint8)]
    geoms = [gc.dyadic_geom(rng, 1000), gc.dyadic_geom(rng, 2)]
    geoms[0][:, 1] = 200.0 + (np.arange(1000) % 3000)          # nobody near the two scan lines
    geoms[0][[5, 64, 65], 1] = 100.0
    geoms[0][999, 1] = 101.0
    lines = np.array([[0.0, 1.0, -100.0], [0.0, 1.0, -102.0]])  # scan lines v = 100 and v = 102, one pixel either side
    want = gc.oracle(tables, geoms, [(1, 0)], lines, 1.0)
    assert want[2].tolist() == [4, 1]
    got = run_device(tables, geoms, [(1, 0)], lines, 1.0)
    assert_equal(got, want, "ties")
    assert got[0].tolist() == [[5, 64], [999, int(gc.NONE_IDX)]]
    assert got[1][0, 0] == got[1][0, 1] and got[1][1, 1] == gc.NONE_DIST


def test_everything_a_candidate():
    """max_dist = 1e30: the queue fills once per database row, and the result is l1k2_batch's bit for bit."""
    import torch
    from spectavi_amd import device
    tables, geoms, lines, _ = ragged_reference()
    got = run_device(tables, geoms, gc.FEW, lines, 1e30)
    desc = torch.from_numpy(np.concatenate(tables)).cuda()
    bi, bd, _ = device.l1k2_batch(desc, gc.seg_of(gc.NINE), gc.FEW)
    assert np.array_equal(got[0], bi.cpu().numpy().view(np.uint64)) and np.array_equal(got[1], bd.cpu().numpy())
    assert np.array_equal(got[2], np.concatenate([np.full(gc.NINE[q], gc.NINE[d], np.int32) for q, d in gc.FEW]))


@pytest.mark.parametrize("what", ["negative max_dist", "nan lines", "nan keypoints"])
def test_nothing_a_candidate(what):
    tables, geoms, lines, _ = ragged_reference()
    max_dist = 1e30
    if what == "negative max_dist":
        max_dist = -1.0
    elif what == "nan lines":
        lines = np.full_like(lines, np.nan)
    else:
        geoms = [g.copy() for g in geoms]
        for g in geoms:
            g[:, 0] = np.nan
    idx, dist, ncand = run_device(tables, geoms, gc.FEW, lines, max_dist)
    assert (idx == gc.NONE_IDX).all() and (dist == gc.NONE_DIST).all() and not ncand.any()


def test_a_nan_keypoint_is_never_returned():
    rng = np.random.default_rng(23)
    tables, geoms, lines = gc.collection([200, 70], [(1, 0)], 23)
    for nan_col in (0, 1):
        g = [geoms[0].copy(), geoms[1]]
        t = [tables[0].copy(), tables[1]]
        bad = int(rng.integers(0, 200))
        g[0][bad, nan_col] = np.nan
        t[0][bad] = t[1][3]                                  # the best match of query 3, were it a candidate
        want = gc.oracle(t, g, [(1, 0)], lines, 1e30)
        assert (want[2] == 199).all()
        got = run_device(t, g, [(1, 0)], lines, 1e30)
        assert_equal(got, want, "one NaN keypoint")
        assert not (got[0] == np.uint64(bad)).any()


@functools.lru_cache(maxsize=None)
def lone_reference():
    tables, geoms, lines = gc.collection(gc.LONE[0], gc.LONE[1], 31)
    for a in tables + geoms + [lines]:
        a.setflags(write=False)
    return tables, geoms, lines, gc.oracle(tables, geoms, gc.LONE[1], lines, gc.RAGGED_DIST)


def test_slices_of_a_lone_pair():
    tables, geoms, lines, want = lone_reference()
    assert 0.01 < want[2].mean() / 5000 < 0.04
    assert_equal(run_device(tables, geoms, gc.LONE[1], lines, gc.RAGGED_DIST), want, "lone pair")


def test_whole_sets_of_many_tiles():
    tables, geoms, lines, want = lone_reference()
    copies = len(gc.TILES[1])
    got = run_device(tables, geoms, gc.TILES[1], np.tile(lines, (copies, 1)), gc.RAGGED_DIST)
    n = len(lines)
    assert_equal(tuple(g[:n] for g in got), want, "first copy")
    for name, g in zip(("idx", "dist", "ncand"), got):
        g = g.reshape((copies, n) + g.shape[1:])
        assert (g == g[0]).all(), "%s: a later copy differs from the first" % name


def test_row_numbers_past_16_bits():
    rows, pairs = gc.LONG
    tables, geoms, lines = gc.collection(rows, pairs, 41)
    geoms[0][:, 1] = np.minimum(geoms[0][:, 1], 4000.0)        # nobody else near the three scan lines below
    geoms[0][[65535, 65536], 1] = 4050.0
    geoms[0][69999, 1] = 4090.0
    lines[0] = (0.0, 1.0, -4050.0)                             # with max_dist 8: rows 65535 and 65536
    lines[1] = (0.0, 1.0, -4090.0)                             # row 69999
    lines[2] = (0.0, 0.25, -4070.0 / 4)                        # |v - 4070| <= 32: all three
    tables[0][[65535, 65536]] = tables[1][0]
    tables[0][69999] = tables[1][1]
    max_dist = 8.0   # a band of about 0.5 % for the other queries; the three lines are exact scan lines
    assert gc.is_dyadic(geoms, lines, max_dist)
    want = gc.oracle(tables, geoms, pairs, lines, max_dist)
    assert want[0][:2].tolist() == [[65535, 65536], [69999, int(gc.NONE_IDX)]]
    assert want[2][:3].tolist() == [2, 1, 3] and want[1][0].tolist() == [0, 0] and want[1][1, 0] == 0
    assert set(want[0][2].tolist()) < {65535, 65536, 69999}
    assert 0.002 < want[2][3:].mean() / rows[0] < 0.01
    assert_equal(run_device(tables, geoms, pairs, lines, max_dist), want, "70000 rows")


def test_host_form_equals_the_device_form():
    from spectavi_amd import feature
    tables, geoms, lines, want = ragged_reference()
    res = feature.nn_bruteforcel1k2_guided_batch(tables, geoms, lines, gc.RAGGED_DIST, gc.FEW)
    assert len(res) == len(gc.FEW)
    got = run_device(tables, geoms, gc.FEW, lines, gc.RAGGED_DIST)
    for p in range(len(gc.FEW)):
        sl = out_rows_of(p)
        for g, r in zip(got, res[p]):
            assert r.dtype == g.dtype and np.array_equal(r, g[sl]), "pair %d" % p
    assert_equal(tuple(np.concatenate([r[k] for r in res]) for k in range(3)), want, "host form")


def random_geoms(rng, rows):
    return [np.c_[rng.uniform(0, 1280, n), rng.uniform(0, 960, n), rng.uniform(1, 8, (n, 2))].astype(np.float32) for n in rows]


def check_lines(got, geom_q, G, used, what):
    """The out rows `got` of one pair against numpy: three NaNs where the pair is not used or the norm is zero or not
    finite, else G (u, v, 1)^T / hypot(l0, l1) within 16 eps sum_j |g_ij x_j| / n.  Returns the NaN rows."""
    eps, rows = np.finfo(np.float64).eps, len(geom_q)
    assert got.shape == (rows, 3), what
    x = np.c_[geom_q[:, :2].astype(np.float64), np.ones(rows)]
    l = x @ G.T
    n = np.hypot(l[:, 0], l[:, 1])
    nan = np.full(rows, not used) | ~(n > 0) | ~np.isfinite(n)
    assert np.array_equal(np.isnan(got), np.repeat(nan[:, None], 3, axis=1)), "%s: the NaN rows" % what
    # three products, two sums, a hypot and a division, each good to an ulp
    ok = ~nan
    bound = 16 * eps * (np.abs(x[:, None, :] * G[None, :, :]).sum(axis=2)) / np.where(ok, n, 1.0)[:, None]
    diff = np.abs(got[ok] - l[ok] / n[ok, None])
    if ok.any():
        print("%s: worst |difference| / bound %.3f over %d rows" % (what, (diff / bound[ok]).max(), ok.sum()))
    assert (diff <= bound[ok]).all(), what
    return nan


def test_epipolar_lines_against_numpy():
    import torch
    from spectavi_amd import device
    rng = np.random.default_rng(51)
    rows, pairs = [40, 0, 300, 7], [(2, 0), (0, 3), (3, 2)]
    geoms = random_geoms(rng, rows)
    G = rng.standard_normal((3, 3, 3))
    G[0, 0] = (1.0, -1.0, 3.0)       # with the keypoint below, l0 = l1 = 0 exactly for one row of pair 0
    G[0, 1] = (2.0, 0.5, -6.5)
    geoms[2][17, :2] = (2.0, 5.0)
    use = [1, 0, 1]
    geom = torch.from_numpy(np.concatenate(geoms)).cuda()
    lines = device.epipolar_lines_batch(geom, gc.seg_of(rows), pairs, G, use=use).cpu().numpy()
    assert lines.shape == (sum(rows[q] for q, _ in pairs), 3) and lines.dtype == np.float64
    o = 0
    for p, (q, _) in enumerate(pairs):
        nan = check_lines(lines[o:o + rows[q]], geoms[q], G[p], use[p], "pair %d" % p)
        if p == 0:
            assert nan[17] and nan.sum() == 1
        o += rows[q]
    # without `use` every pair has a model
    lines = device.epipolar_lines_batch(geom, gc.seg_of(rows), pairs, G).cpu().numpy()
    assert np.isnan(lines).any(axis=1).sum() == 1


LINES_CHUNK = 32          # kLinesChunk of l1k2_guided.hip: the pairs one launch takes as kernel arguments
LINES_GRID = 4096 * 256   # rows of a set that one pass of the capped grid covers


def test_epipolar_lines_across_chunks():
    """70 pairs are three chunks of kernel arguments: out_row and G[9 * i] are carried from chunk to chunk and use[i] is
    read beyond the first; the second chunk's query sets are all empty (most == 0, no launch), so the third chunk's
    out rows start where the first one's end."""
    import torch
    from spectavi_amd import device
    rng = np.random.default_rng(52)
    rows = [40, 0, 300, 7, 257]
    filled = [0, 2, 3, 4]
    query = [filled[k] for k in rng.integers(0, 4, 32)] + [1] * 32 + [4, 0, 2, 3, 2, 4]
    query[5] = 1                     # an empty query set inside a chunk that is launched
    pairs = [(q, int(d)) for q, d in zip(query, rng.integers(0, 5, 70))]
    npairs = len(pairs)
    assert npairs > 2 * LINES_CHUNK and all(rows[q] == 0 for q, _ in pairs[LINES_CHUNK:2 * LINES_CHUNK])
    assert all(rows[q] > 0 for q, _ in pairs[2 * LINES_CHUNK:])
    geoms = random_geoms(rng, rows)
    G = rng.standard_normal((npairs, 3, 3))
    use = np.ones(npairs, np.int32)
    use[[3, 40, 65, 69]] = 0
    seg = gc.seg_of(rows)
    out_off = device.l1k2_guided_batch_plan(seg, pairs)["out_off"]
    assert np.array_equal(np.diff(out_off), [rows[q] for q, _ in pairs])
    assert out_off[2 * LINES_CHUNK] == out_off[LINES_CHUNK] > 0 and out_off[-1] > out_off[2 * LINES_CHUNK]
    geom = torch.from_numpy(np.concatenate(geoms)).cuda()
    lines = device.epipolar_lines_batch(geom, seg, pairs, G, use=use).cpu().numpy()
    assert lines.shape == (out_off[-1], 3)
    for p, (q, _) in enumerate(pairs):
        nan = check_lines(lines[out_off[p]:out_off[p + 1]], geoms[q], G[p], use[p], "pair %d" % p)
        assert nan.all() == (not use[p]) or rows[q] == 0
    # the last six pairs as a call of their own: the same bits
    tail = slice(2 * LINES_CHUNK, npairs)
    alone = device.epipolar_lines_batch(geom, seg, pairs[tail], G[tail], use=use[tail]).cpu().numpy()
    assert alone.shape == (out_off[-1] - out_off[2 * LINES_CHUNK], 3)
    assert np.array_equal(alone.view(np.int64), lines[out_off[2 * LINES_CHUNK]:].view(np.int64))


def test_epipolar_lines_grid_stride():
    """One query set of 4096 * 256 + 300 rows: grid.x is capped at 4096 workgroups of 256 lanes, so the last 300 rows
    are the second turn of 300 lanes' loops."""
    import torch
    from spectavi_amd import device
    rng = np.random.default_rng(53)
    rows = [LINES_GRID + 300, 1]
    assert rows[0] > LINES_GRID
    geoms = random_geoms(rng, rows)
    G = rng.standard_normal((1, 3, 3))
    geom = torch.from_numpy(np.concatenate(geoms)).cuda()
    lines = device.epipolar_lines_batch(geom, gc.seg_of(rows), [(0, 1)], G).cpu().numpy()
    assert lines.shape == (rows[0], 3)
    nan = check_lines(lines, geoms[0], G[0], True, "all rows")
    assert not nan.any()
    # the last 300 rows as the query set of a collection of their own: the same bits
    last = torch.from_numpy(np.concatenate([geoms[0][LINES_GRID:], geoms[1]])).cuda()
    alone = device.epipolar_lines_batch(last, gc.seg_of([300, 1]), [(0, 1)], G).cpu().numpy()
    assert np.array_equal(alone.view(np.int64), lines[LINES_GRID:].view(np.int64))


def test_the_point_of_it_all():
    """The scene of the multiview example at desc_noise 20: inside a 2-pixel band around the true epipolar lines the
    same ratio test holds at least 1.5 times the correct correspondences of the blind one, and the kernel equals the
    oracle on these inexact inputs because no pair lies within 1e-6 of the band's edge."""
    import torch
    from spectavi_amd import device
    tables, K, cams, ids = gc.synthetic_sift_views(0, 3, 400, desc_noise=20.0)
    pairs = [(q, d) for d in range(3) for q in range(d + 1, 3)]
    descs = [t[:, 4:].astype(np.uint8) for t in tables]
    geoms = [np.ascontiguousarray(t[:, :4]) for t in tables]
    rows = [len(t) for t in tables]
    G = np.stack([gc.true_line_matrix(K, cams[q], cams[d]) for q, d in pairs])
    geom = torch.from_numpy(np.concatenate(geoms)).cuda()
    lines = device.epipolar_lines_batch(geom, gc.seg_of(rows), pairs, G).cpu().numpy()
    assert np.isfinite(lines).all()
    o = 0
    for q, d in pairs:
        ln = lines[o:o + rows[q]]
        s = ln[:, 0:1] * geoms[d][:, 0].astype(np.float64) + ln[:, 1:2] * geoms[d][:, 1].astype(np.float64) + ln[:, 2:3]
        assert np.abs(np.abs(s) - 2.0).min() >= 1e-6, "a pair on the band's edge: the decision is not pinned"
        o += rows[q]
    want = gc.oracle(descs, geoms, pairs, lines, 2.0)
    assert_equal(run_device(descs, geoms, pairs, lines, 2.0), want, "scene")
    blind = gc.oracle(descs, geoms, pairs, lines, np.inf)
    o = 0
    for q, d in pairs:
        sl = slice(o, o + rows[q])

        def correct(res):
            keep = gc.ratio_passes(res[0][sl], res[1][sl], 1.75) & (ids[q] >= 0)
            return int((ids[d][res[0][sl][keep, 0].astype(np.int64)] == ids[q][keep]).sum())
        g, b = correct(want), correct(blind)
        print("pair %d-%d: correct correspondences guided %d, blind %d" % (d, q, g, b))
        assert g >= 1.5 * b and b > 0
        o += rows[q]


def test_kernel_coverage_lists_the_instantiations():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_coverage.py"), "--list",
                          "--files", "l1k2_guided.hip"], check=True, capture_output=True, text=True).stdout
    listed = {ln.strip() for ln in out.splitlines() if ln.startswith("  ")}
    assert listed == INSTANTIATED, out
