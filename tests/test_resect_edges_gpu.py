"""resect_fit_batch off its well-posed inputs, on the GPU (cases: tests/resect_edge_cases.py).

The scorer is judged on its own: a try's count against numpy's verdicts under the device's camera of that try
(count_band), so that a count which is wrong at some place of a work item cannot hide behind another device run.

Measured on one MI355X, 256 compute units (the tests print these with -s; profiles/resect_tracks_edges.md has all):
item sizes -- no band pair and hi - lo = 0 in each of the ten calls (up to 5 328 896 pairs a call); x rows times +-2^k
and Xw times 2^+-30 -- every output bit for bit; negated rows -- worst ||A p|| / sigma1 6.44e-19, worst | ||p|| - 1 |
3.33e-16; poisoned rows -- 59 tries on one, 45 with a camera that is not finite and 14 with a finite one, no band pair;
degenerate subsets -- every camera finite, 45 band pairs in set 0 (worst hi - lo 40, the coplanar try) and 718 in the
coplanar set (worst hi - lo 97).  A scorer that never flushes inside its loop, and one that adds every count to
counts[c0 + lane], fail test_counts_at_every_item_size from 65 tries on and nothing in tests/test_resect_gpu.py."""
import numpy as np
import pytest

from tests import resect_edge_cases as rec
from tests import resect_model as rm

pytestmark = pytest.mark.gpu


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def on_device(col):
    return dict(col, dx=cuda(col["x"]), dX=cuda(col["Xw"]))


def fit(col, **kw):
    from spectavi_amd import device
    if "dx" not in col:
        col = on_device(col)
    return device.resect_fit_batch(col["dx"], col["dX"], col["off"], **kw)


def tries_of(col, **kw):
    """(fits, mask, try_cameras, try_inliers) as numpy arrays."""
    fits, mask, cams, inl = fit(col, want_mask=True, want_tries=True, **kw)
    return fits, mask.cpu().numpy() != 0, cams.cpu().numpy(), inl.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_fit(a, b):
    if any(a[k] != b[k] for k in ("success", "inlier_percent", "best_try", "tries_run")):
        return False
    if not np.array_equal(a["inlier_idx"], b["inlier_idx"]) or (a["camera"] is None) != (b["camera"] is None):
        return False
    return a["camera"] is None or np.array_equal(bits(a["camera"]), bits(b["camera"]))


def follows_the_rule(f, cnt, cams, rows, share, find_best, mask, x, Xw, max_error, edge_rows=0):
    """best_try, success, camera and the mask of a set from the device's own counts and cameras."""
    bt, ok = rm.select(cnt, rows, share, find_best)
    assert (f["best_try"], f["success"]) == (bt, ok)
    if bt < 0:
        assert f["camera"] is None and f["inlier_idx"].size == 0 and f["inlier_percent"] == 0.0 and not mask.any()
        return
    assert np.array_equal(bits(f["camera"].reshape(12)), bits(cams[bt]))
    assert len(f["inlier_idx"]) == cnt[bt] == mask.sum() and f["inlier_percent"] == cnt[bt] / float(rows)
    assert np.array_equal(np.flatnonzero(mask), f["inlier_idx"])
    lo, hi, band = rec.count_band(cams[bt][None], x, Xw, max_error)
    err, dc = rm.verdict_terms(cams[bt].reshape(1, 3, 4), x, Xw)
    want = rm.inliers(err[0], dc[0], max_error)
    assert np.array_equal(mask[~band[0]], want[~band[0]]) and band.sum() <= edge_rows


# ---- (a) item sizes ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def repeated_sets(cus):
    """The repeated set on the device, once per number of copies."""
    made = {}

    def get(pieces):
        c = rec.copies_for(pieces, cus)
        if c not in made:
            made[c] = on_device(rec.repeated(c, rec.LONG_TRIES)[0])
        return c, made[c]
    return get


ITEM_CALLS = [(1, t) for t in rec.ONE_PIECE_TRIES] + [(2, t) for t in rec.TWO_PIECE_TRIES] + [(1, rec.LONG_TRIES)]


@pytest.mark.parametrize("pieces,tries", ITEM_CALLS, ids=["%d tries in %d" % (t, p) for p, t in ITEM_CALLS])
def test_counts_at_every_item_size(repeated_sets, cus, pieces, tries):
    """An item of 64 .. 256 tries whole, items of 65 + 64 and 128 + 127 tries, and 1301 tries whose later rounds bring
    items of 512 and of 1024: every copy's counts and cameras are copy 0's bits, copy 0's counts are numpy's under
    the device's cameras, and the winner follows the rule.  Measured on one MI355X (256 compute units): no band pair
    in any of the ten calls, hi - lo = 0 throughout."""
    from spectavi_amd import device
    it = rec.item_set()
    c, col = repeated_sets(pieces)
    samples = np.ascontiguousarray(np.broadcast_to(it["samples"][:, :tries], (c, tries, 6)))
    plan, items = device.resect_fit_batch_plan(col["off"], tries, cus, want_items=True)
    want = rec.expected_items(tries, pieces)
    assert plan["sets"] == c
    for p in (0, c - 1):
        assert items[(items[:, 0] == p) & (items[:, 1] == p * rec.ROWS_A)][:, 4].tolist() == want, (p, want)
    if tries == rec.LONG_TRIES:
        later = {k for rnd in rec.later_rounds(c, tries, cus)[1:] for _, _, _, cuts in rnd for k in cuts}
        assert 1024 in later, later
    kw = dict(required_percent_inliers=2.0, max_error=it["max_error"], find_best_even_in_failure=True, samples=samples)
    fits, mask, cams, inl = tries_of(col, **kw)
    assert cams.shape == (c, tries, 12) and inl.shape == (c, tries)
    for p in range(1, c):
        assert np.array_equal(inl[p], inl[0]), (p, np.flatnonzero(inl[p] != inl[0])[:8])
        assert np.array_equal(bits(cams[p]), bits(cams[0])), p
        assert same_fit(fits[p], fits[0]), p
    x, Xw = it["col"]["x"], it["col"]["Xw"]
    assert np.isfinite(cams[0]).all()
    lo, hi, band = rec.count_band(cams[0], x, Xw, it["max_error"])
    print("%d tries, %d pieces: band pairs %d of %d, worst hi - lo %d" % (tries, pieces, band.sum(), band.size, (hi - lo).max()))
    assert band.sum() <= 1
    wrong = np.flatnonzero((inl[0] < lo) | (inl[0] > hi))
    assert wrong.size == 0, (wrong[:8], inl[0][wrong[:8]], lo[wrong[:8]], hi[wrong[:8]])
    assert all(f["tries_run"] == tries for f in fits)
    follows_the_rule(fits[0], inl[0], cams[0], rec.ROWS_A, 2.0, True, mask[:rec.ROWS_A], x, Xw, it["max_error"], edge_rows=1)
    assert fits[0]["best_try"] >= 0 and not fits[0]["success"] and inl[0].max() >= 0.69 * rec.ROWS_A


# ---- (b) input forms --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    c = rm.case(rec.BASE)
    kw = dict(required_percent_inliers=rm.SHARE, max_error=c["max_error"], samples=c["samples"])
    return c, kw, tries_of(c["col"], **kw)


def assert_same_run(a, b, what):
    fa, ma, ca, ia = a
    fb, mb, cb, ib = b
    diff = np.flatnonzero((bits(ca) != bits(cb)).any(axis=2))
    assert diff.size == 0, (what, "cameras differ at %d tries, first %d" % (diff.size, diff[0]))
    assert np.array_equal(ia, ib), (what, np.argwhere(ia != ib)[:8])
    assert np.array_equal(ma, mb), what
    assert all(same_fit(p, q) for p, q in zip(fa, fb)), what


def test_scaled_x_rows_give_the_same_bits(plain):
    """(u, v) = x[0..1] / x[2] by IEEE division: a row times +-2^k is the same row.  Held on one MI355X."""
    c, kw, base = plain
    assert_same_run(tries_of(rec.scaled_x(c["col"], np.random.default_rng(41)), **kw), base, "x rows times +-2^k")


@pytest.mark.parametrize("k", [30, -30])
def test_scaled_points_give_the_same_bits(plain, k):
    """All of Xw times 2^k: every operation of the solve and of the verdict commutes with it.  Held on one MI355X."""
    c, kw, base = plain
    assert_same_run(tries_of(rec.scaled_Xw(c["col"], k), **kw), base, "Xw times 2^%d" % k)


def test_negated_rows_meet_the_definition(plain):
    """Half of the Xw rows negated (w < 0): the criteria of test_resect_gpu.test_every_try_meets_the_definition against
    the model of the negated input, and the planted inliers recovered."""
    c, kw, _ = plain
    col, neg = rec.negated_rows(c["col"], np.random.default_rng(42))
    assert 0.4 < neg.mean() < 0.6
    model = rm.model(col, c["samples"], rm.SHARE, c["max_error"])
    fits, mask, cams, inl = tries_of(col, **kw)
    off = col["off"]
    worst_res = worst_norm = 0.0
    for p, m in enumerate(model):
        if m is None:
            assert fits[p]["best_try"] == -1 and fits[p]["tries_run"] == 0
            continue
        for t in range(rm.TRIES):
            if t == rm.REPEATED_TRY:
                continue
            P = cams[p, t]
            assert np.isfinite(P).all(), (p, t)
            worst_norm = max(worst_norm, abs(np.linalg.norm(P) - 1))
            assert abs(np.linalg.norm(P) - 1) <= 1e-12 and P[np.flatnonzero(P)[-1]] > 0, (p, t)
            res = np.linalg.norm(m["A"][t] @ P)
            worst_res = max(worst_res, res / m["S"][t][0])
            assert res <= 1e-13 * m["S"][t][0] + 2 * m["formation"][t], (p, t, res)
            assert m["count_lo"][t] <= inl[p, t] <= m["count_hi"][t], (p, t, inl[p, t], m["count_lo"][t], m["count_hi"][t])
        f = fits[p]
        assert f["success"] and f["best_try"] == m["best_try"], p
        assert np.array_equal(f["inlier_idx"], np.flatnonzero(col["planted"][off[p]:off[p + 1]])), p
    print("negated rows: worst ||A p|| / sigma1 %.2e, worst | ||p|| - 1 | %.2e" % (worst_res, worst_norm))


def test_poisoned_rows(plain):
    """Six rows a set that are no correspondence (and one that is, written with x[2] = -1): the tries that sample none
    keep their cameras' bits and their counts move by those rows' verdicts alone; a try that samples one has a camera
    that is not finite and counts 0, or a finite one that counts what numpy counts under it."""
    c, kw, base = plain
    col, smp, rows = rec.poisoned(c["col"], c["samples"], np.random.default_rng(43))
    kw = dict(kw, samples=smp)
    fits, mask, cams, inl = tries_of(col, **kw)
    _, bmask, bcams, binl = base
    off, me = col["off"], c["max_error"]
    checked_legal = nonfinite = finite = 0
    for p in range(len(off) - 1):
        n = int(off[p + 1] - off[p])
        if n < rm.MIN_ROWS:
            continue
        sl = slice(off[p], off[p + 1])
        x, Xw = col["x"][sl], col["Xw"][sl]
        if rows[p, 0] < 0:          # an untouched set: the plain run's bits
            assert np.array_equal(bits(cams[p]), bits(bcams[p])) and np.array_equal(inl[p], binl[p])
            assert np.array_equal(mask[sl], bmask[sl])
            continue
        local = rows[p] - off[p]
        hit = np.isin(smp[p], local[:5]).any(axis=1)
        moved = (smp[p] != c["samples"][p]).any(axis=1)
        assert hit.sum() >= rec.POISON_TRIES
        clean = ~hit & ~moved
        assert np.array_equal(bits(cams[p][clean]), bits(bcams[p][clean])), p
        # the six rows' own verdicts, before and after: the other rows' are the same bits
        ok = np.isfinite(cams[p]).all(axis=1)
        alo, ahi, _ = rec.count_band(cams[p], c["col"]["x"][sl][local], c["col"]["Xw"][sl][local], me)
        blo, bhi, _ = rec.count_band(cams[p], x[local], Xw[local], me)
        d = inl[p] - binl[p]
        t = np.flatnonzero(clean & ok)
        assert np.all((blo[t] - ahi[t] <= d[t]) & (d[t] <= bhi[t] - alo[t])), (p, t[(blo[t] - ahi[t] > d[t]) | (d[t] > bhi[t] - alo[t])][:8])
        # every try, the poisoned ones among them
        lo, hi, band = rec.count_band(cams[p], x, Xw, me)
        assert np.all(inl[p][~ok] == 0), (p, "a camera that is not finite counts 0")
        assert np.all((lo <= inl[p]) & (inl[p] <= hi)), (p, np.flatnonzero((lo > inl[p]) | (inl[p] > hi))[:8])
        nonfinite += int((~ok & hit).sum())
        finite += int((ok & hit).sum())
        print("set %d: %d tries on a poisoned row, %d of them with a finite camera; band pairs %d, worst hi - lo %d" % (
            p, hit.sum(), (ok & hit).sum(), band.sum(), (hi - lo).max()))
        for name in rec.NEVER_IN_MASK:
            assert not mask[sl][local[rec.POISONS.index(name)]], (p, name)
        f = fits[p]
        follows_the_rule(f, inl[p], cams[p], n, rm.SHARE, False, mask[sl], x, Xw, me)
        if f["camera"] is not None and base[0][p]["camera"] is not None and np.array_equal(bits(f["camera"]), bits(base[0][p]["camera"])):
            assert mask[sl][local[5]] == bmask[sl][local[5]], (p, "x2 = -1 is the same row")
            checked_legal += 1
    assert checked_legal >= 1 and nonfinite + finite >= 4 * rec.POISON_TRIES
    print("poisoned tries: %d with a camera that is not finite, %d with a finite one" % (nonfinite, finite))


# ---- (c) degenerate subsets -------------------------------------------------------------------------------------------
def test_degenerate_subsets():
    """Coplanar, collinear, repeated and equal sample rows, and a set of coplanar points: a camera that is not finite
    counts 0, a finite one counts what numpy counts under it; the tries next to them do not notice; the winner follows
    the rule on the device's counts.  Nothing is asked of which camera a degenerate try yields."""
    d = rec.degenerate()
    col = on_device(d["col"])
    off, me = col["off"], d["max_error"]
    for share, find_best in ((rm.SHARE, False), (2.0, True)):
        kw = dict(required_percent_inliers=share, max_error=me, find_best_even_in_failure=find_best)
        fits, mask, cams, inl = tries_of(col, samples=d["samples"], **kw)
        bfits, bmask, bcams, binl = tries_of(col, samples=d["plain"], **kw)
        keep = np.ones(rec.TRIES_C, bool)
        keep[list(rec.DEGENERATE.values())] = False
        assert np.array_equal(bits(cams[0][keep]), bits(bcams[0][keep])) and np.array_equal(inl[0][keep], binl[0][keep])
        assert np.array_equal(bits(cams[1:]), bits(bcams[1:])) and np.array_equal(inl[1:], binl[1:])
        assert np.isfinite(bcams[0]).all() and np.isfinite(bcams[2]).all(), "ordinary subsets of ordinary sets"
        for p in range(3):
            sl = slice(off[p], off[p + 1])
            x, Xw = col["x"][sl], col["Xw"][sl]
            ok = np.isfinite(cams[p]).all(axis=1)
            lo, hi, band = rec.count_band(cams[p], x, Xw, me)
            assert np.all(inl[p][~ok] == 0), p
            wrong = np.flatnonzero((lo > inl[p]) | (inl[p] > hi))
            assert wrong.size == 0, (p, wrong[:8], inl[p][wrong[:8]], lo[wrong[:8]], hi[wrong[:8]])
            if share == 2.0:
                print("set %d: %d of %d cameras finite, band pairs %d, worst hi - lo %d" % (p, ok.sum(), len(ok), band.sum(), (hi - lo).max()))
                if p == 0:
                    for name, t in rec.DEGENERATE.items():
                        print("  %s: camera %s, count %d" % (name, "finite" if ok[t] else "not finite", inl[0][t]))
            f = fits[p]
            assert f["tries_run"] == rec.TRIES_C
            follows_the_rule(f, inl[p], cams[p], int(off[p + 1] - off[p]), share, find_best, mask[sl], x, Xw, me,
                             edge_rows=int(band.sum()))
        # without the per-try outputs a set may leave early: the same winner, and the coplanar set returns
        early = fit(col, samples=d["samples"], **kw)
        for p in range(3):
            a, b = fits[p], early[p]
            assert (a["best_try"], a["success"]) == (b["best_try"], b["success"]) and np.array_equal(a["inlier_idx"], b["inlier_idx"])
            assert b["tries_run"] == rec.TRIES_C or (b["success"] and rm.select(inl[p], int(off[p + 1] - off[p]), share, find_best)[1])
