"""Inputs and reference statements for the DLT edge tests: power-of-two rescaling and error classes.

In IEEE arithmetic the perspective division u = x0 / x2 does not change by a single bit when x0 and
x2 are both multiplied by 2^k (as long as both stay exact), and the DLT matrix A, hence X and the
reprojection error, depend on the observations only through u, v, u', v'.  Negating x or xp does
not change them either, and multiplying both cameras by the same 2^k scales A by 2^k, which leaves X
and the error as they are while nothing over- or underflows.  These invariances give a bit-exact
reference that needs no second implementation, and they probe exactly the edges where the HIP
kernel's fast reciprocals (v_rcp_f64 / v_rsq_f64 + Newton steps) leave the IEEE results: |w| near
the top of the range (1 / w subnormal) and subnormal entries.

The error classes (finite / +inf / -inf / nan) are judged against a plain numpy restatement of the
reference's reprojection error (src/DltTriangulator.h:67-74: sqrt of the summed squared difference of
hnormalized(P X) and the hnormalized observation, per view, the two views added).

Used by tests/test_dlt_invariance_oracle.py (CPU: the oracle and the host mirror) and
tests/test_dlt_edges_gpu.py (the HIP entry points)."""
import numpy as np

DBL_MAX = np.finfo(np.float64).max
FINITE, POS_INF, NEG_INF, NAN = 0, 1, 2, 3


def error_class(e):
    """0 finite, 1 +inf, 2 -inf, 3 nan, elementwise."""
    e = np.asarray(e, np.float64)
    return np.select([np.isnan(e), np.isposinf(e), np.isneginf(e)], [NAN, POS_INF, NEG_INF], FINITE)


def same_bits(a, b):
    """Elementwise: the same float64 bits, or both nan (a nan's payload is not part of the contract)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def scene(rng, npt, P0=None, P1=None):
    """A RANSAC-like mix (tests/test_ransac_gpu.py::_scene): points 4..8 in front of P0 = [I|0] and
    P1 = [R|t], noise-free rows, rows with 2e-3 pixel noise, and every 7th row an unrelated xp."""
    if P0 is None:
        P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    if P1 is None:
        a = rng.standard_normal(3)
        a /= np.linalg.norm(a)
        th = rng.uniform(-0.3, 0.3)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
        t = rng.standard_normal(3)
        P1 = np.hstack([R, (t / np.linalg.norm(t))[:, None]])
    Xw = np.hstack([rng.standard_normal((npt, 2)), rng.uniform(4, 8, (npt, 1)), np.ones((npt, 1))])
    x, xp = Xw @ P0.T, Xw @ P1.T
    noisy = rng.random(npt) < 0.6
    x[noisy, :2] += rng.normal(0, 2e-3, (noisy.sum(), 2)) * x[noisy, 2:3]
    xp[noisy, :2] += rng.normal(0, 2e-3, (noisy.sum(), 2)) * xp[noisy, 2:3]
    xp[::7] = rng.standard_normal((len(xp[::7]), 3))
    return P0, P1, x, xp


def quantise(x, bits=20):
    """x rounded to `bits` significant bits per entry: such a row can be scaled deep into the
    subnormal range and still round-trip exactly."""
    m, e = np.frexp(x)
    return np.ldexp(np.round(np.ldexp(m, bits)), e - bits)


def row_scales(rng, x):
    """A power-of-two exponent k and a sign per row of x, drawn so that the scaled rows cover the whole
    exact range: a quarter anywhere in k in [-1000, 1000], a quarter with |w| landing in
    [2^1021, 2^1023), a quarter with w at the subnormal boundary (ilogb(w) in [-1030, -1018]) and a
    quarter with the largest entry deep in the subnormal range (ilogb in [-1050, -1030])."""
    n = x.shape[0]
    with np.errstate(all="ignore"):
        ew = np.frexp(x[:, 2])[1] - 1                                # ilogb(w) (garbage for 0 / inf / nan)
        emax = np.frexp(np.max(np.abs(x), axis=1))[1] - 1
    kind = rng.integers(0, 4, n)
    k = np.select([kind == 0, kind == 1, kind == 2],
                  [rng.integers(-1000, 1001, n), rng.integers(1021, 1023, n) - ew, rng.integers(-1030, -1017, n) - ew],
                  rng.integers(-1050, -1029, n) - emax)
    sign = rng.choice([-1.0, 1.0], n)
    return k.astype(np.int64), sign


def apply_row_scales(x, k, sign):
    """(scaled x, ok): rows scaled by sign * 2^k where that is exact (round trip), left as they are
    elsewhere; ok marks the rows that were scaled."""
    with np.errstate(all="ignore"):
        xs = sign[:, None] * np.ldexp(x, k[:, None])
        back = sign[:, None] * np.ldexp(xs, -k[:, None])
    ok = np.all(back == x, axis=1) & np.all(np.isfinite(xs), axis=1) & np.all(np.isfinite(x), axis=1)
    return np.where(ok[:, None], xs, x), ok


def invariance_inputs(seed, npt=6000):
    """(P0, P1, x, xp, variants): a scene (a fifth of its rows quantised so that they survive deep
    subnormal scaling) and the rescaled copies to compare it with.  variants is a list of
    (name, P0', P1', x', xp', ok) where ok marks the rows that were actually rescaled."""
    rng = np.random.default_rng(seed)
    P0, P1, x, xp = scene(rng, npt)
    q = rng.random(npt) < 0.2
    x[q], xp[q] = quantise(x[q]), quantise(xp[q])
    k, s = row_scales(rng, x)
    xs, okx = apply_row_scales(x, k, s)
    k, s = row_scales(rng, xp)
    xps, okp = apply_row_scales(xp, k, s)
    kc = int(rng.integers(-200, 201))
    variants = [("rows of x", P0, P1, xs, xp, okx),
                ("rows of xp", P0, P1, x, xps, okp),
                ("rows of x and xp", P0, P1, xs, xps, okx | okp),
                ("negated", P0, P1, -x, -xp, np.ones(npt, bool)),
                ("cameras x 2^%d" % kc, np.ldexp(P0, kc), np.ldexp(P1, kc), x, xp, np.ones(npt, bool)),
                ("cameras x 2^200", np.ldexp(P0, 200), np.ldexp(P1, 200), x, xp, np.ones(npt, bool)),
                ("cameras x 2^-200", np.ldexp(P0, -200), np.ldexp(P1, -200), x, xp, np.ones(npt, bool))]
    return P0, P1, x, xp, variants


def extreme_rows(x, ok):
    """Row masks of the rescaled rows at the edges: |w| >= 2^1021, and a subnormal entry."""
    tiny = np.finfo(np.float64).tiny
    big = ok & (np.abs(x[:, 2]) >= 2.0 ** 1021)
    sub = ok & np.any((x != 0) & (np.abs(x) < tiny), axis=1)
    return big, sub


def class_table(seed, npt=20000):
    """Rows whose reprojection error is +inf or nan under IEEE arithmetic, and rows around them:
      * overflow rows: one homogeneous component of view 0 multiplied by 10^100 .. 10^200;
      * w = 0 observations (either view), inf and nan observations;
      * a point at the centre of camera 0 (x = P0 C = 0: u = 0 / 0);
      * noise-free rows on integer points (error exactly 0 or a few ulps);
      * the plain scene rows.
    Returns (P0, P1, x, xp)."""
    rng = np.random.default_rng(seed)
    P0, P1, x, xp = scene(rng, npt)
    n = npt // 8
    rows = rng.permutation(npt)
    over, w0, nonfin, centre, exact = (rows[i * n:(i + 1) * n] for i in range(5))
    comp = rng.integers(0, 3, len(over))
    x[over, comp] *= 10.0 ** rng.uniform(100, 200, len(over))
    half = len(w0) // 2
    x[w0[:half], 2] = 0.0
    xp[w0[half:], 2] = 0.0
    vals = np.array([np.inf, -np.inf, np.nan])
    x[nonfin, rng.integers(0, 3, len(nonfin))] = vals[rng.integers(0, 3, len(nonfin))]
    x[centre] = 0.0
    # noise-free rows on integer points: x = P0 X is exact (P0 = [I|0]), xp = P1 X one rounding off
    Xi = np.hstack([rng.integers(-8, 9, (len(exact), 2)), rng.integers(4, 9, (len(exact), 1)), np.ones((len(exact), 1))])
    x[exact], xp[exact] = Xi @ P0.T, Xi @ P1.T
    return P0, P1, x, xp


def ieee_error(P0, P1, X, x, xp):
    """The reference's reprojection error (src/DltTriangulator.h:67-74) in plain IEEE float64 for rows
    of X, and the two squared residuals in extended precision (to tell the rows whose square sits
    at the overflow threshold)."""
    P0, P1, X = np.asarray(P0, np.float64), np.asarray(P1, np.float64), np.asarray(X, np.float64)
    out, sq = [], []
    with np.errstate(all="ignore"):
        for P, o in ((P0, x), (P1, xp)):
            r = X @ P.T
            d0 = r[:, 0] / r[:, 2] - o[:, 0] / o[:, 2]
            d1 = r[:, 1] / r[:, 2] - o[:, 1] / o[:, 2]
            out.append(np.sqrt(d0 * d0 + d1 * d1))
            L = np.longdouble
            sq.append(d0.astype(L) ** 2 + d1.astype(L) ** 2)
        return out[0] + out[1], sq


def clear_of_overflow(sq):
    """Rows whose squared residuals (both views) are not within a factor of 4 of DBL_MAX."""
    ok = np.ones(sq[0].shape, bool)
    lo, hi = np.longdouble(DBL_MAX) / 4, np.longdouble(DBL_MAX) * 4
    with np.errstate(all="ignore"):
        for s in sq:
            ok &= ~((s >= lo) & (s <= hi))
    return ok
