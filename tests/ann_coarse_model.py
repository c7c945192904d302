"""float64 model of the coarse stage of ann_hnswlib / spv_ann_l2 (steps 1-2 of the contract in
include/spectavi_amd.h), numpy only, and the two rules it gives for the candidate set of step 3.

The model
    m_c   = rintf(float(mean of column c of x)), the mean from float64 column sums;
    x'    = bf16(x - m), y' = bf16(y - m): the float32 difference, rounded to nearest even by integer
            arithmetic on its bits;
    s*(i,j) = n_j - 2 y'_i . x'_j,  n_j = sum_c x'_jc^2,  in float64.
A bf16 value has 8 significant bits, so every product of two of them has at most 16 and is exact in
float32 and in float64; the float64 sums of at most 2048 such products are off by a relative 2^-42 at the
most, which the bound below does not notice.  The mean is taken from numpy's float64 sum, not from the
library's chunk order: the two agree to about 1e-12, and the data sets used with this model keep every
column mean at least 1e-3 from a half-integer (means_are_unambiguous), which also covers the rounding
of the mean to float32 for |mean| < 16384 (spacing 2^-10), so rintf gives the same integer either way.

The bound.  Let u = 2^-24 and K = kpad, the padded row width.  The library computes in float32
    n~_j   : K exact non-negative products added one by one:   |n~ - n|     <= (K - 1) u n (1 + O(Ku)),
    acc~   : K exact products added in SOME order, each add rounded once, whatever the order and
             however the matrix core groups them:              |acc~ - acc| <= (K - 1) u A (1 + O(Ku)),
             A(i,j) = sum_c |y'_ic x'_jc|,
    s~     = fma(-2, acc~, n~), one rounding of n~ - 2 acc~:   |s~ - (n~ - 2 acc~)| <= u |n~ - 2 acc~|
                                                                             <= u (n + 2 A)(1 + O(Ku)).
Together |s~ - s*| <= K u (n + 2A)(1 + O(Ku)) <= eps(i,j) = (K + 2) u (n_j + 2 A(i,j)): the two spare units
pay for the O(Ku) terms (K <= 2048, Ku <= 2^-13) many times over.  The rules use the margin 2 E_i with
E_i = max_j eps(i,j), so that they also hold for adds that truncate instead of rounding (u -> 2u).

The rules.  Let tau_i be the ncand-th smallest s*(i, .).  The library keeps the ncand smallest keys
(s~, j).  With |s~ - s*| <= E for every row of the query:
  * a row with s* < tau - 2E MUST be kept: if it were not, ncand other rows l had s~_l <= s~_j, hence
    s*_l <= s*_j + 2E < tau; with j itself that makes ncand + 1 rows below tau, but only ncand - 1 are;
  * a row with s* > tau + 2E MUST NOT be kept: the ncand rows with s* <= tau have
    s~ <= tau + E < s*_j - E <= s~_j, so ncand keys are smaller than this one;
  * the rows in between (the band) are left open, unless the band and the MUST rows together are exactly
    ncand rows: the candidate set has ncand distinct rows, so it is then that set (open_rows() counts
    the band of such a query as 0).  The ncand-th row of the model itself always lies in the band.
"""
import numpy as np

U = 2.0 ** -24


def kpad_of(dim):
    return (dim + 31) // 32 * 32


def column_means(x):
    return np.asarray(x, np.float64).sum(0) / x.shape[0]


def means_are_unambiguous(x, gap=1e-3):
    """No column mean within `gap` of a half-integer, and small enough for the float32 rounding of the
    mean to stay inside the gap."""
    mean = column_means(x)
    return bool((np.abs(mean - np.floor(mean) - 0.5) > gap).all() and (np.abs(mean) < 16384).all())


def centre(x):
    """m_c = rintf(mean), float32 (np.rint rounds halves to even, as rintf does)."""
    return np.rint(column_means(x).astype(np.float32))


def bf16_rne(a):
    """float32 -> the nearest bf16 (ties to even), returned as float32; finite values only."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return (u & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def bf16_trunc(a):
    """The wrong rounding: the low 16 bits dropped."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32)


def images(x, y, rounding=bf16_rne, centre_y=True):
    """(x', y') as float32 arrays of bf16 values.  `rounding` and `centre_y` exist for the mutants of
    tests/test_ann_coarse_model.py."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    assert np.isfinite(x).all() and np.isfinite(y).all()
    m = centre(x)
    return rounding(x - m), rounding(y - m if centre_y else y)


def scores(x, y):
    """(s*, eps), both float64 [yrows, xrows]."""
    xp, yp = (a.astype(np.float64) for a in images(x, y))
    n = (xp * xp).sum(1)
    s = n[None, :] - 2.0 * (yp @ xp.T)
    eps = (kpad_of(x.shape[1]) + 2) * U * (n[None, :] + 2.0 * (np.abs(yp) @ np.abs(xp).T))
    return s, eps


def rules(s, eps, ncand):
    """(must, must_not): bool [yrows, xrows]."""
    assert 1 <= ncand < s.shape[1]
    margin = 2.0 * eps.max(1, keepdims=True)
    tau = np.partition(s, ncand - 1, axis=1)[:, ncand - 1:ncand]
    return s < tau - margin, s > tau + margin


def open_rows(must, must_not, ncand):
    """Per query, the rows whose membership the rules leave open."""
    band = (~must & ~must_not).sum(1)
    return np.where(must.sum(1) + band > ncand, band, 0)


def violations(must, must_not, idx):
    """Per query, whether the selection idx [yrows, ncand] breaks a rule or is no set of ncand rows."""
    idx = np.asarray(idx).astype(np.int64)
    yrows, xrows = must.shape
    bad = ((idx < 0) | (idx >= xrows)).any(1)
    sel = np.zeros((yrows, xrows), bool)
    sel[np.arange(yrows)[:, None], np.clip(idx, 0, xrows - 1)] = True
    return bad | (sel.sum(1) != idx.shape[1]) | (must & ~sel).any(1) | (must_not & sel).any(1)


def select(s, ncand):
    """The ncand smallest (s, idx) of every query: what step 3 does with the scores s."""
    order = np.lexsort((np.broadcast_to(np.arange(s.shape[1]), s.shape), s), axis=1)
    return order[:, :ncand]


def float32_scores(xp, yp):
    """Step 2 in plain float32 numpy arithmetic on the images (one order among the many the bound covers)."""
    xp, yp = np.asarray(xp, np.float32), np.asarray(yp, np.float32)
    n = np.zeros(xp.shape[0], np.float32)
    for c in range(xp.shape[1]):
        n = n + xp[:, c] * xp[:, c]
    return n[None, :] - np.float32(2.0) * (yp @ xp.T)
