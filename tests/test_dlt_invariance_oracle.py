"""CPU: the DLT references themselves under power-of-two rescaling and at the inf / nan edges of the
reprojection error (tests/dlt_edge_cases.py).  tests/test_dlt_edges_gpu.py judges the HIP kernel by
the same invariances and classes; these tests make sure a failure there can only be the kernel's.

  * the host mirror of the kernel's operation sequence (oracle_dlt_mirror.cpp) and the JacobiSVD
    oracle (oracle_jacobisvd.cpp) give the same bits after each row of x or xp is multiplied by
    +-2^k (over the whole exact range, |w| up to 2^1023 and subnormal entries included), after x and
    xp are negated, and after both cameras are multiplied by the same 2^k, |k| <= 200;
  * the mirror's error class (finite / +inf / -inf / nan) on every row equals the class of the
    reference's formula (src/DltTriangulator.h:67-74) restated in numpy on the mirror's own X."""
import numpy as np

from tests import dlt_edge_cases as ec


def _check_variants(tri, rep, seed):
    P0, P1, x, xp, variants = ec.invariance_inputs(seed)
    X0, E0 = tri(P0, P1, x, xp), rep(P0, P1, x, xp)
    npt = x.shape[0]
    for name, a, b, xs, xps, ok in variants:
        # the filter must leave most rows rescaled (it drops rows that would not round-trip exactly)
        assert ok.sum() >= 0.5 * npt, (name, ok.sum())
        if name.startswith("rows"):
            big, sub = ec.extreme_rows(xps if name == "rows of xp" else xs, ok)
            assert big.sum() >= 0.1 * npt and sub.sum() >= 0.05 * npt, (name, big.sum(), sub.sum())
        X1, E1 = tri(a, b, xs, xps), rep(a, b, xs, xps)
        bad = np.flatnonzero(~ec.same_bits(X1, X0).all(axis=1))
        assert bad.size == 0, "%s: X changed at %d rows, first %d: %r -> %r" % (name, bad.size, bad[0], X0[bad[0]], X1[bad[0]])
        bad = np.flatnonzero(~ec.same_bits(E1, E0).all(axis=1))
        assert bad.size == 0, "%s: error changed at %d rows, first %d: %r -> %r" % (name, bad.size, bad[0], E0[bad[0]], E1[bad[0]])


def test_mirror_is_bit_invariant_under_power_of_two_rescaling(oracle):
    for seed in (1, 2):
        _check_variants(oracle.dlt_mirror_triangulate, oracle.dlt_mirror_reprojection_error, seed)


def test_oracle_is_bit_invariant_under_power_of_two_rescaling(oracle):
    _check_variants(oracle.dlt_triangulate, oracle.dlt_reprojection_error, 3)


def test_mirror_scorer_is_bit_invariant_under_power_of_two_rescaling(oracle):
    """dlt_mirror_score_hypotheses: counts and masks unchanged (rows rescaled; cameras rescaled with
    the hypotheses rescaled alike)."""
    P0, P1, x, xp, variants = ec.invariance_inputs(4, npt=3000)
    rng = np.random.default_rng(4)
    P1s = np.stack([P1, P1 + 0.05 * rng.standard_normal((3, 4)), rng.standard_normal((3, 4))])
    c0, m0 = oracle.dlt_mirror_score_hypotheses(P0, P1s, x, xp, 1e-2)
    assert c0[0] > 0.5 * x.shape[0]
    for name, a, b, xs, xps, _ in variants:
        s = b[0, 0] / P1[0, 0]                                   # the camera scale of the variant (a power of two)
        c1, m1 = oracle.dlt_mirror_score_hypotheses(a, P1s * s, xs, xps, 1e-2)
        assert np.array_equal(c0, c1) and np.array_equal(m0, m1), name


def _class_check(X, E, P0, P1, x, xp, what):
    e, sq = ec.ieee_error(P0, P1, X, x, xp)
    clear = ec.clear_of_overflow(sq)
    assert clear.mean() > 0.99, what
    cm, cn = ec.error_class(E), ec.error_class(e)
    bad = np.flatnonzero((cm != cn) & clear)
    assert bad.size == 0, "%s: error class differs from the IEEE restatement at %d rows, first %d: %r vs %r" % (
        what, bad.size, bad[0], E[bad[0]], e[bad[0]])
    return cm


def test_mirror_error_classes_match_ieee_restatement(oracle):
    for seed in (5, 6):
        P0, P1, x, xp = ec.class_table(seed)
        mX = oracle.dlt_mirror_triangulate(P0, P1, x, xp)
        mE = oracle.dlt_mirror_reprojection_error(P0, P1, x, xp)[:, 0]
        cm = _class_check(mX, mE, P0, P1, x, xp, "mirror, table %d" % seed)
        n = np.bincount(cm, minlength=4)
        # the table really holds overflow rows (+inf) and nan rows, next to finite ones
        assert n[ec.POS_INF] > 500 and n[ec.NAN] > 2000 and n[ec.FINITE] > 8000, n
        # ... and the noise-free rows, whose error is zero or a few ulps
        assert (mE < 1e-12).sum() > 2000


def test_oracle_error_classes_match_ieee_restatement(oracle):
    P0, P1, x, xp = ec.class_table(7)
    oX = oracle.dlt_triangulate(P0, P1, x, xp)
    oE = oracle.dlt_reprojection_error(P0, P1, x, xp)[:, 0]
    n = np.bincount(_class_check(oX, oE, P0, P1, x, xp, "oracle"), minlength=4)
    assert n[ec.POS_INF] > 0 and n[ec.NAN] > 0, n
