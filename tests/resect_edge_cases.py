"""Inputs of resect_fit_batch that tests/resect_model.py's cases never form, and the helper that judges the scorer on
its own: numpy only.

count_band holds a try's count against numpy's verdicts under the *device's* camera of that try, so the solver's
rounding does not enter: what is left open is the band test_winner_follows_the_rule_on_the_devices_counts already
uses (a residual within 1e-9 relative of max_error, a depth term within 1e-12 of the try's largest).

(a) item_sizes: one clean set of 4096 rows repeated c times, so that the planner's cut of a slot's tries is chosen by
    c alone (ransac_batch_items: ceil(4 cus / row blocks) pieces of at least 48 tries; 16 row blocks a copy).
(b) input forms on rm.case("pixel-clean"): rows of x rescaled by +-2^k, Xw rescaled by 2^+-30, negated Xw rows, and six
    poisoned rows a set.
(c) degenerate subsets: coplanar, five collinear plus one, repeats at three pairs of positions, six equal rows, and a
    set whose 300 points are all coplanar."""
import numpy as np

from tests import resect_model as rm
from tests import tracks_triangulate_model as tm

ROWS_A, BLOCKS_A = 4096, 16
MIN_PIECE, FIRST_STEP, LAST_STEP, ROUND_TRIES = 48, 256, 4096, 32768
ONE_PIECE_TRIES = (64, 65, 127, 128, 129, 255, 256)
TWO_PIECE_TRIES = (129, 255)
LONG_TRIES = 256 + 1024 + 21


def count_band(P, x, Xw, max_error):
    """(lo int64 [T], hi int64 [T], band bool [T, n]) for cameras P [T, 12] over the rows (x, Xw): band marks the (try,
    row) pairs whose verdict is open -- |err - max_error| <= 1e-9 max_error or |dc| <= 1e-12 of the try's largest
    finite |dc| --, lo counts the inliers outside it, hi the inliers and the band.  A try whose camera is not finite
    has lo = hi = 0 and no band."""
    P = np.asarray(P, np.float64).reshape(-1, 3, 4)
    finite = np.isfinite(P).all(axis=(1, 2))
    err, dc = rm.verdict_terms(np.where(finite[:, None, None], P, 0.0), x, Xw)
    with np.errstate(invalid="ignore"):
        adc = np.abs(dc)
        top = np.where(np.isfinite(adc), adc, 0.0).max(axis=1, initial=0.0)
        band = (np.abs(err - max_error) <= 1e-9 * max_error) | (adc <= 1e-12 * top[:, None])
    inl = rm.inliers(err, dc, max_error)
    band &= finite[:, None]
    inl &= finite[:, None]
    return (inl & ~band).sum(1), (inl | band).sum(1), band


# ---- (a) item sizes -------------------------------------------------------------------------------------------------
_item = {}


def item_set():
    """The clean set of (a) and its LONG_TRIES subsets, once: dict(col, samples [1, LONG_TRIES, 6], max_error)."""
    if not _item:
        rng = np.random.default_rng(4096)
        col = rm.collection(rng, [ROWS_A], noise=0.0, outliers=0.3)
        smp = rm.draw_samples(rng, col["off"], LONG_TRIES, col["planted"], clean_every=8)
        # the first try behind each of the scorer's flushes is drawn among the planted rows as well: a count of a few
        # rows there (try 64 of the plain draw counts none) would let a count that lands in another try's place pass
        good = np.flatnonzero(col["planted"])
        for t in range(64, LONG_TRIES, 64):
            smp[0, t] = rng.choice(good, 6, replace=False)
        _item.update(col=col, samples=smp, max_error=1.0)
    return _item


def copies_for(pieces, cus):
    """How many copies of the 16-row-block set make the planner cut a slot's tries into `pieces`."""
    return -(-4 * cus // (BLOCKS_A * pieces))


def repeated(c, tries):
    """The set c times back to back with the first `tries` subsets for every copy: (col, samples [c, tries, 6])."""
    it = item_set()
    col = it["col"]
    rep = dict(x=np.ascontiguousarray(np.tile(col["x"], (c, 1))), Xw=np.ascontiguousarray(np.tile(col["Xw"], (c, 1))),
               off=(np.arange(c + 1) * ROWS_A).astype(np.int64))
    return rep, np.ascontiguousarray(np.broadcast_to(it["samples"][:, :tries], (c, tries, 6)))


def expected_items(tries, pieces):
    """The try counts of a slot's items under the planner's rule, for a first round of min(256, tries) tries."""
    k = min(FIRST_STEP, tries)
    cut = max(1, min(pieces, k // MIN_PIECE))
    chunk = -(-k // cut)
    return [min(chunk, k - c) for c in range(0, k, chunk)]


def later_rounds(c, tries, cus):
    """The rounds of a call over c equal sets of ROWS_A rows, restated from the contract (every running set brings
    its next step -- 256, then fourfold up to 4096 -- while the round has room for ROUND_TRIES tries; the verdict cap
    is not reached at these sizes): a list of rounds, each a list of (set, first try, tries, item try counts)."""
    done, step = [0] * c, [min(FIRST_STEP, tries)] * c
    rounds = []
    while any(d < tries for d in done):
        room, slots = ROUND_TRIES, []
        for p in range(c):
            if done[p] >= tries:
                continue
            if room <= 0:
                break
            n = min(step[p], tries - done[p], room)
            slots.append((p, done[p], n))
            room -= n
        pieces = min(-(-4 * cus // (BLOCKS_A * len(slots))), 1 << 16)
        rnd = []
        for p, t0, n in slots:
            cut = max(1, min(pieces, n // MIN_PIECE))
            chunk = -(-n // cut)
            rnd.append((p, t0, n, [min(chunk, n - k) for k in range(0, n, chunk)]))
            if n == step[p]:
                step[p] = min(LAST_STEP, 4 * step[p])
            done[p] += n
        rounds.append(rnd)
    return rounds


# ---- (b) input forms ------------------------------------------------------------------------------------------------
BASE = "pixel-clean"
POISONS = ("Xw3 = 0", "x2 = 0", "nan x", "nan Xw", "zero Xw", "x2 = -1")
NEVER_IN_MASK = ("x2 = 0", "nan x", "nan Xw", "zero Xw")
POISON_TRIES = 8


def scaled_x(col, rng):
    """Every x row times +-2^k, k in [-20, 20]: (u, v) = x[0..1] / x[2] keep their bits."""
    k = rng.integers(-20, 21, len(col["x"]))
    f = np.ldexp(np.where(rng.uniform(size=len(k)) < 0.5, -1.0, 1.0), k)
    return dict(col, x=np.ascontiguousarray(col["x"] * f[:, None]))


def scaled_Xw(col, k):
    return dict(col, Xw=np.ascontiguousarray(np.ldexp(col["Xw"], k)))


def negated_rows(col, rng):
    """A random half of the Xw rows negated: the same points, w < 0."""
    neg = rng.uniform(size=len(col["Xw"])) < 0.5
    return dict(col, Xw=np.ascontiguousarray(np.where(neg[:, None], -col["Xw"], col["Xw"]))), neg


def poisoned(col, samples, rng):
    """Six poisoned rows (POISONS, in that order) in every set of 255 rows and more, and POISON_TRIES tries of each
    such set moved onto one of them: (col, samples, rows int64 [nsets, 6] of the concatenated arrays or -1)."""
    x, Xw, smp = col["x"].copy(), col["Xw"].copy(), samples.copy()
    off = col["off"]
    rows = np.full((len(off) - 1, 6), -1, np.int64)
    for p in range(len(off) - 1):
        n = int(off[p + 1] - off[p])
        if n < 255:
            continue
        local = rng.choice(n, 6, replace=False)
        rows[p] = off[p] + local
        g = rows[p]
        Xw[g[0], 3] = 0.0
        x[g[1], 2] = 0.0
        x[g[2], 1] = np.nan
        Xw[g[3], 0] = np.nan
        Xw[g[4]] = 0.0
        x[g[5]] = -x[g[5]]
        for i, t in enumerate(range(20, 20 + POISON_TRIES)):     # the five rows that are no correspondence, in turn;
            if local[i % 5] not in smp[p, t]:                    # the position moves along
                smp[p, t, i % 6] = local[i % 5]
        if local[5] not in smp[p, 30]:
            smp[p, 30, 2] = local[5]                             # and one try on the row written with x[2] = -1
    return dict(col, x=x, Xw=Xw), smp, rows


# ---- (c) degenerate subsets -----------------------------------------------------------------------------------------
DEGENERATE = {"coplanar": 3, "collinear": 7, "repeat 0,5": 11, "repeat 4,5": 13, "repeat 2,3": 17, "six equal": 19}
SIZES_C = (300, 300, 6)
TRIES_C = 60
_deg = {}


def built(rng, clouds, outliers=0.3):
    """rm.collection for given point clouds [n, 4] (w = 1): one wide camera a set, float32 observations, 30 % of the
    rows of a set of more than 6 redrawn in the frame, points scaled to unit norm."""
    cams = tm.wide_cameras(rng, len(clouds))
    xs, Xs, planted = [], [], []
    for P, Xw in zip(cams, clouds):
        n = len(Xw)
        geom, _ = tm.observe(rng, P[None], Xw, 0.0)
        good = np.ones(n, bool)
        if outliers and n > rm.MIN_ROWS:
            bad = rng.choice(n, int(round(outliers * n)), replace=False)
            good[bad] = False
            geom[bad, 0] = rng.uniform(0, 1280, len(bad))
            geom[bad, 1] = rng.uniform(0, 960, len(bad))
        xs.append(np.concatenate([geom[:, :2].astype(np.float64), np.ones((n, 1))], 1))
        Xs.append(Xw / np.linalg.norm(Xw, axis=1, keepdims=True))
        planted.append(good)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    return dict(x=np.ascontiguousarray(np.concatenate(xs)), Xw=np.ascontiguousarray(np.concatenate(Xs)), off=off,
                cams=cams, planted=np.concatenate(planted))


def degenerate():
    """dict(col, plain [3, TRIES_C, 6], samples the same with the DEGENERATE tries of set 0 replaced, max_error).
    Set 0: 300 points of which rows 0..39 lie on the plane z = 5 and rows 40..44 on a line; set 1: 300 points on the
    plane z = 5; set 2: six points."""
    if not _deg:
        rng = np.random.default_rng(606)
        a = tm.points(rng, SIZES_C[0])
        a[:40, 2] = 5.0
        a[40:45, :3] = np.array([-1.0, 0.5, 4.5]) + np.linspace(0, 1, 5)[:, None] * np.array([2.0, -1.0, 3.0])
        b = tm.points(rng, SIZES_C[1])
        b[:, 2] = 5.0
        col = built(rng, [a, b, tm.points(rng, SIZES_C[2])])
        plain = rm.draw_samples(rng, col["off"], TRIES_C, col["planted"], clean_every=8)
        smp = plain.copy()
        s = smp[0]
        s[DEGENERATE["coplanar"]] = rng.choice(40, 6, replace=False)
        s[DEGENERATE["collinear"]] = [40, 41, 42, 43, 44, 200]
        for name, (i, j) in (("repeat 0,5", (0, 5)), ("repeat 4,5", (4, 5)), ("repeat 2,3", (2, 3))):
            s[DEGENERATE[name], j] = s[DEGENERATE[name], i]
        s[DEGENERATE["six equal"]] = s[DEGENERATE["six equal"], 0]
        _deg.update(col=col, plain=plain, samples=smp, max_error=1.0)
    return _deg
