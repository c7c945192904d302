"""The conditions the GPU tests of tests/test_resect_edges_gpu.py rest on, checked without a GPU: the planner's cuts
for the repeated set at 256 compute units, an empty band under the model's cameras, and what count_band returns."""
import numpy as np

from spectavi_amd import device
from tests import resect_edge_cases as rec
from tests import resect_model as rm

CUS = 256


def first_round_items(c, tries, cus):
    off = (np.arange(c + 1) * rec.ROWS_A).astype(np.int64)
    plan, items = device.resect_fit_batch_plan(off, tries, cus, want_items=True)
    return plan, items


def test_planner_gives_the_intended_items():
    one, two = rec.copies_for(1, CUS), rec.copies_for(2, CUS)
    assert (one, two) == (64, 32)
    for pieces, c, all_tries in ((1, one, rec.ONE_PIECE_TRIES + (rec.LONG_TRIES,)), (2, two, rec.TWO_PIECE_TRIES)):
        for tries in all_tries:
            plan, items = first_round_items(c, tries, CUS)
            want = rec.expected_items(tries, pieces)
            assert plan["sets"] == c and plan["row_blocks"] == c * rec.BLOCKS_A
            for p in range(c):
                mine = items[(items[:, 0] == p) & (items[:, 1] == p * rec.ROWS_A)]
                assert mine[:, 4].tolist() == want, (pieces, tries, p)
                assert mine[:, 3].tolist() == (p * min(tries, 256) + np.cumsum([0] + want[:-1])).tolist()
    assert rec.expected_items(129, 2) == [65, 64] and rec.expected_items(255, 2) == [128, 127]
    assert rec.expected_items(256, 1) == [256] and rec.expected_items(64, 1) == [64]


def test_later_rounds_bring_an_uncut_item_of_1024():
    """The restated rounds agree with the planner on the first round, and the long call runs items of 1024 tries."""
    c = rec.copies_for(1, CUS)
    rounds = rec.later_rounds(c, rec.LONG_TRIES, CUS)
    plan, items = first_round_items(c, rec.LONG_TRIES, CUS)
    assert [(p, n, cuts) for p, _, n, cuts in rounds[0]] == [(p, 256, [256]) for p in range(c)] and plan["tries"] == 256 * c
    assert sum(n for rnd in rounds for p, _, n, _ in rnd if p == 0) == rec.LONG_TRIES
    sizes = sorted({k for rnd in rounds[1:] for _, _, _, cuts in rnd for k in cuts})
    assert 1024 in sizes and 512 in sizes, sizes
    # an item of 1024 starts at try 256 of its set: its flushes at 64 tries fall on tries 319, 383, ...
    assert any(t0 == 256 and cuts == [1024] for rnd in rounds[1:] for _, t0, _, cuts in rnd)


def test_band_is_empty_under_the_models_cameras():
    it = rec.item_set()
    col, smp = it["col"], it["samples"][0]
    P = np.stack([rm.hypothesis(rm.try_matrix(col["x"], col["Xw"], s)[0])[0].reshape(12) for s in smp])
    lo, hi, band = rec.count_band(P, col["x"], col["Xw"], it["max_error"])
    print("band pairs %d of %d, worst hi - lo %d" % (band.sum(), band.size, (hi - lo).max()))
    assert band.size == rec.LONG_TRIES * rec.ROWS_A and band.sum() == 0 and np.array_equal(lo, hi)
    clean = lo[7::8]                       # every eighth try is drawn among the planted rows
    assert np.all(clean >= 0.69 * rec.ROWS_A), "the clean tries recover the planted rows"
    assert np.all(lo[64::64] >= 0.69 * rec.ROWS_A), "and so does the first try behind each of the scorer's flushes"

def test_count_band_on_known_cameras():
    it = rec.item_set()
    col = it["col"]
    x, Xw = col["x"][:500], col["Xw"][:500]
    planted = col["planted"][:500]
    P = col["cams"][0].reshape(12)
    bad = P.copy()
    bad[3] = np.nan
    inf = P.copy()
    inf[0] = np.inf
    lo, hi, band = rec.count_band(np.stack([P, bad, inf, -P]), x, Xw, 1.0)
    assert lo[0] == hi[0] == planted.sum() and not band.any(), "float32 rounding is far inside one pixel"
    assert lo[1] == hi[1] == lo[2] == hi[2] == 0, "a camera that is not finite counts 0"
    assert lo[3] == lo[0], "the sign of the camera does not enter the verdict"
    # a row on the bound is in the band; rows that are not finite are neither inliers nor band
    err, _ = rm.verdict_terms(P.reshape(1, 3, 4), x, Xw)
    k = int(np.flatnonzero(~planted)[0])
    lo, hi, band = rec.count_band(P[None], x, Xw, float(err[0, k]))
    assert band[0, k] and hi[0] - lo[0] == band.sum() == 1
    x2, X2 = x.copy(), Xw.copy()
    good = np.flatnonzero(planted)[:4]
    x2[good[0], 2], x2[good[1], 0], X2[good[2], 1], X2[good[3]] = 0.0, np.nan, np.nan, 0.0
    lo, hi, band = rec.count_band(P[None], x2, X2, 1.0)
    assert lo[0] == hi[0] == planted.sum() - 4 and not band.any()


def test_input_forms_are_what_they_claim():
    c = rm.case(rec.BASE)
    col = c["col"]
    rng = np.random.default_rng(9)
    sx = rec.scaled_x(col, rng)
    assert np.array_equal(sx["x"][:, 0] / sx["x"][:, 2], col["x"][:, 0]) and np.array_equal(sx["x"][:, 1] / sx["x"][:, 2], col["x"][:, 1])
    assert len(np.unique(np.abs(sx["x"][:, 2]))) == 41 and (sx["x"][:, 2] < 0).any()
    pc, smp, rows = rec.poisoned(col, c["samples"], rng)
    sizes = np.diff(col["off"])
    for p, n in enumerate(sizes):
        assert (rows[p] >= 0).all() == (n >= 255)
        if n < 255:
            continue
        local = rows[p] - col["off"][p]
        hit = np.isin(smp[p], local[:5]).any(axis=1)
        assert hit.sum() >= rec.POISON_TRIES
        assert all(len(set(s.tolist())) == 6 for t, s in enumerate(smp[p]) if t != rm.REPEATED_TRY)
    g = rows[3]
    assert pc["Xw"][g[0], 3] == 0 and pc["x"][g[1], 2] == 0 and np.isnan(pc["x"][g[2]]).any() and np.isnan(pc["Xw"][g[3]]).any()
    assert not pc["Xw"][g[4]].any() and pc["x"][g[5], 2] == -1 and np.array_equal(pc["x"][g[5]], -col["x"][g[5]])


def test_degenerate_subsets_are_degenerate():
    d = rec.degenerate()
    col, smp = d["col"], d["samples"][0]
    x, Xw = col["x"][:300], col["Xw"][:300]

    def rank_gap(rows):
        return rm.try_matrix(x, Xw, rows)[0]
    for name, t in rec.DEGENERATE.items():
        s = np.linalg.svd(rank_gap(smp[t]), compute_uv=False)
        ordinary = np.linalg.svd(rank_gap(d["plain"][0][t]), compute_uv=False)
        print("%s: sigma11 / sigma1 = %.2e (the try it replaces: %.2e)" % (name, s[10] / s[0], ordinary[10] / ordinary[0]))
        if name in ("coplanar", "collinear"):   # the six points span no more than a plane through the origin of R^4
            assert np.linalg.svd(Xw[smp[t]], compute_uv=False)[3] <= 1e-12, name
        else:
            assert s[10] <= 1e-12 * s[0], name
    Xb = col["Xw"][300:600]
    assert np.linalg.svd(Xb, compute_uv=False)[3] <= 1e-12, "set 1 is coplanar"
    keep = np.ones(rec.TRIES_C, bool)
    keep[list(rec.DEGENERATE.values())] = False
    assert np.array_equal(d["samples"][0][keep], d["plain"][0][keep]) and np.array_equal(d["samples"][1:], d["plain"][1:])
