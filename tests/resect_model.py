"""The judge of resect_fit_batch and resect_gather (spv_resect_*): a plain numpy restatement of the contract in
include/spectavi_amd.h that shares no code and no algorithm with the kernels, and the synthetic collections of the
tests.  The scenes are tests/tracks_triangulate_model.py's: wide_cameras, points (scaled to unit norm, as
triangulate_tracks returns them), observe (float32 rounding) and calibrate.

Per try the model forms the 11 x 12 matrix A of the six sampled rows in np.longdouble and rounds once, takes P as the
last right singular vector of numpy.linalg.svd (sign: the last non-zero entry positive) and computes every row's
reprojection residual and depth term, the counts, the winner and its mask.  A second float64 route of its own
(numpy.linalg.qr of A, then the null vector of R) gives the same quantities; the per-row tolerance on a residual is

    tol = 1e-6 max_error + 8 |err_svd - err_qr|

and a row whose residual lies within tol of max_error, or whose depth term within tol of 0 while its residual is not
beyond max_error + tol, is undecided.  (The second condition without its rider -- `undecided_literal` -- also counts
rows next to a try's principal plane, whose residual is 1e5 px and more and whose tolerance, eight times the routes'
difference of that residual, then exceeds any depth term: outliers under either route, so their verdict is not open.)
The bounds of a try's count do not use the notion: count_lo counts the rows inside max_error - tol with a depth term
above tol, count_hi those inside max_error + tol with a depth term above -tol."""
import numpy as np

from tests import tracks_triangulate_model as tm

EPS = np.finfo(np.float64).eps
MIN_ROWS = 6


# ---- collections ------------------------------------------------------------------------------------------------------
def collection(rng, sizes, noise=0.0, outliers=0.3, calibrated=False):
    """One camera and one point cloud per set: x float64 [total, 3] = (u, v, 1) widened from float32, Xw float64
    [total, 4] of unit norm, off int64, cams [nsets, 3, 4], planted bool [total] (False: the row's (u, v) was redrawn
    uniformly in the frame)."""
    K = tm.intrinsics()
    cams = tm.wide_cameras(rng, max(len(sizes), 1), K)[:len(sizes)]
    xs, Xs, planted = [], [], []
    for P, n in zip(cams, sizes):
        Xw = tm.points(rng, n)
        geom, _ = tm.observe(rng, P[None], Xw, noise)
        good = np.ones(n, bool)
        if outliers and n > MIN_ROWS:
            bad = rng.choice(n, int(round(outliers * n)), replace=False)
            good[bad] = False
            geom[bad, 0] = rng.uniform(0, 1280, len(bad))
            geom[bad, 1] = rng.uniform(0, 960, len(bad))
        xs.append(geom)
        Xs.append(Xw / np.linalg.norm(Xw, axis=1, keepdims=True))
        planted.append(good)
    geom = np.concatenate(xs) if xs else np.zeros((0, 4), np.float32)
    if calibrated and len(geom):
        cams, geom = tm.calibrate(K, cams, geom)
    x = np.concatenate([geom[:, :2].astype(np.float64), np.ones((len(geom), 1))], 1)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return dict(x=np.ascontiguousarray(x), Xw=np.ascontiguousarray(np.concatenate(Xs) if Xs else np.zeros((0, 4))),
                off=off, cams=np.asarray(cams), planted=np.concatenate(planted) if planted else np.zeros(0, bool))


def draw_samples(rng, off, ntries, planted=None, clean_every=0):
    """int32 [nsets, ntries, 6]: six different rows per try; every clean_every-th try of a set is drawn among its
    planted rows (so that a model exists whatever the luck of the draw).  Sets under 6 rows get zeros."""
    nsets = len(off) - 1
    s = np.zeros((nsets, ntries, 6), np.int32)
    for p in range(nsets):
        n = int(off[p + 1] - off[p])
        if n < MIN_ROWS:
            continue
        good = np.flatnonzero(planted[off[p]:off[p + 1]]) if planted is not None else np.arange(n)
        for t in range(ntries):
            pool = good if clean_every and t % clean_every == clean_every - 1 and len(good) >= 6 else np.arange(n)
            s[p, t] = rng.choice(pool, 6, replace=False)
    return s


# The cases of the per-try tests: name -> (calibrated, noise in px, max_error in px).  Calibrated coordinates are the
# pixel ones divided by the focal length, 1000.
SIZES = (0, 5, 6, 255, 256, 257, 2500)
TRIES = 60
SHARE = 0.6
FOCAL = 1000.0
CASES = {"pixel-clean": (False, 0.0, 1.0), "pixel-noisy": (False, 0.5, 3.0),
         "calibrated-clean": (True, 0.0, 1.0), "calibrated-noisy": (True, 0.5, 3.0)}
REPEATED_TRY = 5   # the try of every set whose second sample row repeats the first
_cache = {}


def case(name):
    """The collection, subsets and model of a case, computed once: dict(col, samples, max_error, model, repeated).
    30 % of the rows of every set of more than 6 are outliers; every eighth try is drawn among the planted rows."""
    if name not in _cache:
        calibrated, noise, px = CASES[name]
        rng = np.random.default_rng(1000 + sorted(CASES).index(name))
        col = collection(rng, SIZES, noise=noise, outliers=0.3, calibrated=calibrated)
        smp = draw_samples(rng, col["off"], TRIES, col["planted"], clean_every=8)
        smp[:, REPEATED_TRY, 1] = smp[:, REPEATED_TRY, 0]
        me = px / FOCAL if calibrated else px
        _cache[name] = dict(col=col, samples=smp, max_error=me, model=model(col, smp, SHARE, me), noisy=noise > 0)
    return _cache[name]


# ---- the model --------------------------------------------------------------------------------------------------------
def try_matrix(x, Xw, rows):
    """A [11, 12] of six rows (u, v, 1), X in extended precision rounded once, and the formation bound."""
    L = np.longdouble
    u = (x[rows, 0].astype(L) / x[rows, 2].astype(L))
    v = (x[rows, 1].astype(L) / x[rows, 2].astype(L))
    X = Xw[rows].astype(L)
    A = np.zeros((12, 12), L)
    A[0::2, 0:4] = X
    A[0::2, 8:12] = -u[:, None] * X
    A[1::2, 4:8] = X
    A[1::2, 8:12] = -v[:, None] * X
    A = A[:11].astype(np.float64)
    mags = np.concatenate([np.abs(np.float64(u))[:, None] * np.abs(Xw[rows]), np.abs(np.float64(v))[:5, None] * np.abs(Xw[rows[:5]])])
    return A, EPS * np.linalg.norm(mags)


def canonical(p):
    nz = np.flatnonzero(p != 0)
    return -p if nz.size and p[nz[-1]] < 0 else p


def hypothesis(A, route="svd"):
    """The unit null vector of A as a [3, 4] camera; (P, singular values of A)."""
    if route == "svd":
        _, s, vt = np.linalg.svd(A)
        return canonical(vt[-1]).reshape(3, 4), s
    R = np.linalg.qr(A, mode="r")
    _, s, vt = np.linalg.svd(R)
    return canonical(vt[-1]).reshape(3, 4), s


def verdict_terms(Ps, x, Xw):
    """Per (try, row): the residual |proj(P Xw) - (u, v)| and the depth term; NaN stays NaN."""
    with np.errstate(all="ignore"):
        h = np.einsum("tij,nj->tni", Ps, Xw)
        u, v = x[:, 0] / x[:, 2], x[:, 1] / x[:, 2]
        err = np.hypot(h[:, :, 0] / h[:, :, 2] - u[None], h[:, :, 1] / h[:, :, 2] - v[None])
        sgn = np.where(np.linalg.det(Ps[:, :, :3]) < 0, -1.0, 1.0)
        dc = (sgn / np.sum(Ps[:, 2, :3] ** 2, axis=1))[:, None] * h[:, :, 2] / Xw[None, :, 3]
    return err, dc


def inliers(err, dc, max_error):
    with np.errstate(invalid="ignore"):
        return (err <= max_error) & (dc > 0)


def select(counts, rows, share, find_best):
    """The best-model rule on try order: (best_try or -1, success).  First try with count / rows >= share; failing
    that and with find_best the try with the most inliers (at least one), the earliest among equals."""
    counts = np.asarray(counts, np.int64)
    above = np.flatnonzero(counts / float(rows) >= share) if rows > 0 else np.zeros(0, int)
    if above.size:
        return int(above[0]), True
    if find_best and counts.size and counts.max() > 0:
        return int(np.argmax(counts)), False
    return -1, False


def model_set(x, Xw, samples, max_error, route="svd"):
    """One set: the cameras of its tries [T, 3, 4], err and dc [T, n], the matrices and their singular values."""
    T = len(samples)
    Ps = np.full((T, 3, 4), np.nan)
    As, Ss, Fs = [], [], []
    for t in range(T):
        A, formation = try_matrix(x, Xw, samples[t])
        P, s = hypothesis(A, route)
        Ps[t] = P
        As.append(A)
        Ss.append(s)
        Fs.append(formation)
    err, dc = verdict_terms(Ps, x, Xw)
    return dict(P=Ps, err=err, dc=dc, A=As, S=Ss, formation=Fs)


def model(col, samples, share, max_error, find_best=False):
    """The whole contract for a collection: per set None (under 6 rows) or a dict with the SVD route's cameras, err,
    dc, counts, the tolerance and the undecided rows, the count bounds, the winner and its mask, and the QR route's
    winner and mask."""
    off = col["off"]
    out = []
    for p in range(len(off) - 1):
        lo, hi = int(off[p]), int(off[p + 1])
        if hi - lo < MIN_ROWS:
            out.append(None)
            continue
        x, Xw = col["x"][lo:hi], col["Xw"][lo:hi]
        a = model_set(x, Xw, samples[p], max_error, "svd")
        b = model_set(x, Xw, samples[p], max_error, "qr")
        with np.errstate(invalid="ignore"):
            tol = 1e-6 * max_error + 8 * np.abs(a["err"] - b["err"])
            tol = np.where(np.isfinite(tol), tol, np.inf)
            und_literal = (np.abs(a["err"] - max_error) <= tol) | (np.abs(a["dc"]) <= tol)
            # a row beyond max_error + tol is an outlier whatever its depth term: its verdict is not open
            und = (np.abs(a["err"] - max_error) <= tol) | ((np.abs(a["dc"]) <= tol) & (a["err"] <= max_error + tol))
            sure_in = (a["err"] <= max_error - tol) & (a["dc"] > tol)
            maybe_in = (a["err"] <= max_error + tol) & (a["dc"] > -tol)
        m = dict(a, tol=tol, undecided=und, undecided_literal=und_literal, count_lo=sure_in.sum(1), count_hi=maybe_in.sum(1))
        for name, r in (("", a), ("qr_", b)):
            inl = inliers(r["err"], r["dc"], max_error)
            m[name + "counts"] = inl.sum(1)
            bt, ok = select(m[name + "counts"], hi - lo, share, find_best)
            m[name + "best_try"], m[name + "success"] = bt, ok
            m[name + "mask"] = inl[bt] if bt >= 0 else np.zeros(hi - lo, bool)
        out.append(m)
    return out
