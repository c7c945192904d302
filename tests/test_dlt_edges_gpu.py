"""GPU: the HIP DLT paths (dlt_triangulate, dlt_reprojection_error, the RANSAC scorer and everything built
on it) under power-of-two rescaling, reordering and batch-size changes, and at the inf / nan edges of
the reprojection error.  Everything is compared bit for bit, except the finite values against the host
mirror (dlt_checks.check_against_mirror's tolerance).

The references need no second implementation (tests/dlt_edge_cases.py): the perspective division is
invariant under multiplying a homogeneous row by +-2^k, and A (hence X and the error) under
multiplying both cameras by 2^k; a point's result must not depend on where it sits in the batch or on
how many points the batch has.  tests/test_dlt_invariance_oracle.py holds the host mirror and the
JacobiSVD oracle to the same invariances and classes on the CPU.  The rescaled rows include |w| in
[2^1021, 2^1023) and subnormal entries: the ranges where a bare v_rcp_f64 + Newton reciprocal leaves
the IEEE quotient."""
import numpy as np
import pytest

from tests import dlt_checks as dc
from tests import dlt_edge_cases as ec

pytestmark = pytest.mark.gpu


def _diff_report(a, b, x, ok):
    """The rows where a and b differ, split by where the rescaled input x sits."""
    bad = ~ec.same_bits(a, b).reshape(len(x), -1).all(axis=1)
    big, sub = ec.extreme_rows(x, ok)
    ca, cb = ec.error_class(a).reshape(len(x), -1), ec.error_class(b).reshape(len(x), -1)
    nan_inf = ((ca == ec.NAN) & (cb == ec.POS_INF)) | ((ca == ec.POS_INF) & (cb == ec.NAN))
    return bad, "%d rows differ (%d with |w| >= 2^1021, %d with a subnormal entry, %d nan vs +inf)" % (
        bad.sum(), (bad & big).sum(), (bad & sub).sum(), nan_inf.any(axis=1).sum())


def _hip_paths():
    import torch
    from spectavi_amd import device, mvg

    def dev(fn):
        return lambda P0, P1, x, xp: fn(P0, P1, torch.from_numpy(x).cuda(), torch.from_numpy(xp).cuda()).cpu().numpy()
    return (("host ABI", mvg.dlt_triangulate, mvg.dlt_reprojection_error),
            ("device", dev(device.dlt_triangulate), dev(device.dlt_reprojection_error)))


@pytest.mark.parametrize("seed", [11, 12])
def test_triangulate_and_error_invariant_under_rescaling(seed):
    P0, P1, x, xp, variants = ec.invariance_inputs(seed)
    for path, tri, rep in _hip_paths():
        X0, E0 = tri(P0, P1, x, xp), rep(P0, P1, x, xp)
        assert np.isfinite(X0).all() and np.isfinite(E0).all()
        for name, a, b, xs, xps, ok in variants:
            assert ok.sum() >= 0.5 * len(x), name
            probe = xps if name == "rows of xp" else xs
            X1, E1 = tri(a, b, xs, xps), rep(a, b, xs, xps)
            bad, msg = _diff_report(X1, X0, probe, ok)
            assert not bad.any(), "%s, %s: X: %s" % (path, name, msg)
            bad, msg = _diff_report(E1, E0, probe, ok)
            assert not bad.any(), "%s, %s: error: %s" % (path, name, msg)


def test_scorer_invariant_under_rescaling():
    """device.dlt_score_hypotheses: counts and mask (the cameras of a variant rescaled alike)."""
    import torch
    from spectavi_amd import device
    P0, P1, x, xp, variants = ec.invariance_inputs(13)
    rng = np.random.default_rng(13)
    P1s = np.stack([P1, P1 + 0.05 * rng.standard_normal((3, 4)), P1 + 1e-3 * rng.standard_normal((3, 4)),
                    rng.standard_normal((3, 4))])

    def score(P0, P1s, x, xp):
        c, m = device.dlt_score_hypotheses(P0, torch.from_numpy(P1s).cuda(), torch.from_numpy(x).cuda(),
                                           torch.from_numpy(xp).cuda(), 1e-2, want_mask=True)
        return c.cpu().numpy(), m.cpu().numpy()
    c0, m0 = score(P0, P1s, x, xp)
    assert c0[0] > 0.5 * len(x)
    for name, a, b, xs, xps, ok in variants:
        c1, m1 = score(a, P1s * (b[0, 0] / P1[0, 0]), xs, xps)
        cols = np.flatnonzero((m1 != m0).any(axis=0))
        big, sub = ec.extreme_rows(xps if name == "rows of xp" else xs, ok)
        assert cols.size == 0 and np.array_equal(c1, c0), (
            "%s: mask differs at %d points (%d with |w| >= 2^1021, %d subnormal); counts %s vs %s"
            % (name, cols.size, big[cols].sum(), sub[cols].sum(), c1, c0))


def _row_variants(variants):
    return [v for v in variants if not v[0].startswith("cameras")]


def test_ransac_process_candidates_invariant_under_rescaling():
    """device.ransac_process_candidates (gate, E, four cameras, scoring, best camera, inlier mask):
    every output the same bits after rows of x0 / x1 are rescaled or negated."""
    import torch
    from spectavi_amd import device
    P0, P1, x, xp, variants = ec.invariance_inputs(14)
    rng = np.random.default_rng(14)
    R, t = P1[:, :3], P1[:, 3]
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    Fs = np.stack([E * rng.uniform(0.1, 10), -E, E + 1e-4 * rng.standard_normal((3, 3)),
                   E + 1e-2 * rng.standard_normal((3, 3)), rng.standard_normal((3, 3))])

    def run(x0, x1):
        out = device.ransac_process_candidates(torch.from_numpy(Fs).cuda(), torch.from_numpy(x0).cuda(),
                                               torch.from_numpy(x1).cuda(), required_percent_inliers=.5,
                                               reprojection_error_allowed=1e-2, find_best_even_in_failure=False,
                                               want_mask=True)
        return {k: v.cpu().numpy() for k, v in out.items()}
    want = run(x, xp)
    assert want["success"][0] and want["inlier_count"][0] > 0.5 * len(x)
    for name, _, _, xs, xps, _ in _row_variants(variants):
        got = run(xs, xps)
        for k in want:
            assert ec.same_bits(got[k].astype(np.float64), want[k].astype(np.float64)).all(), (name, k)


def test_ransac_fit_invariant_under_rescaling():
    """mvg.ransac_fit over fixed 7-subsets: the seven-point kernel normalises with the IEEE division,
    the scorer with the kernel's reciprocal -- the whole fit must come out the same."""
    from spectavi_amd import mvg
    P0, P1, x, xp, variants = ec.invariance_inputs(15, npt=3000)
    samples = mvg.ransac_sample(15, len(x), 300)
    opts = dict(required_percent_inliers=0.99, reprojection_error_allowed=1e-2, find_best_even_in_failure=True)
    want = mvg.ransac_fit(x, xp, samples=samples, **opts)
    assert want["best_try"] >= 0 and len(want["inlier_idx"]) > 0.5 * len(x)
    for name, _, _, xs, xps, _ in _row_variants(variants):
        got = mvg.ransac_fit(xs, xps, samples=samples, **opts)
        assert got["success"] == want["success"] and got["inlier_percent"] == want["inlier_percent"], name
        assert got["best_try"] == want["best_try"] and got["best_root"] == want["best_root"], name
        assert ec.same_bits(got["essential"], want["essential"]).all(), name
        assert ec.same_bits(got["camera"], want["camera"]).all(), name
        assert np.array_equal(got["inlier_idx"], want["inlier_idx"]), name


def test_result_independent_of_position():
    """A random permutation of the points gives the permuted bits (triangulation, errors) and, for the
    scorer, the same counts with the mask columns permuted.  Edge rows (class table) included."""
    import torch
    from spectavi_amd import device
    P0, P1, x, xp = ec.class_table(16, npt=8000)
    rng = np.random.default_rng(16)
    perm = rng.permutation(len(x))
    for path, tri, rep in _hip_paths():
        X, E = tri(P0, P1, x, xp), rep(P0, P1, x, xp)
        Xp, Ep = tri(P0, P1, x[perm], xp[perm]), rep(P0, P1, x[perm], xp[perm])
        assert ec.same_bits(Xp, X[perm]).all(), path
        assert ec.same_bits(Ep, E[perm]).all(), path
    P1s = torch.from_numpy(np.stack([P1, P1 + 0.05 * rng.standard_normal((3, 4)), rng.standard_normal((3, 4))])).cuda()
    c0, m0 = device.dlt_score_hypotheses(P0, P1s, torch.from_numpy(x).cuda(), torch.from_numpy(xp).cuda(), 1e-2, want_mask=True)
    c1, m1 = device.dlt_score_hypotheses(P0, P1s, torch.from_numpy(x[perm]).cuda(), torch.from_numpy(xp[perm]).cuda(), 1e-2,
                                         want_mask=True)
    assert np.array_equal(c1.cpu().numpy(), c0.cpu().numpy())
    assert np.array_equal(m1.cpu().numpy(), m0.cpu().numpy()[:, perm])


def test_batch_size_around_the_persistent_grid_stride():
    """dlt_run's persistent grid walks p, p + stride, ... with stride = CUs x 32 x 256 and prefetches the
    next point under `q < npt`.  npt = 1, 63, 64, 65, 257, stride - 1, stride, stride + 1, 2 stride + 1
    must give, point for point, the bits of one launch over a superset (2 stride + 4098 points), edge
    rows (class table) placed across the stride boundaries."""
    import torch
    from spectavi_amd import device
    stride = torch.cuda.get_device_properties(0).multi_processor_count * 32 * 256
    total = 2 * stride + 4098
    rng = np.random.default_rng(17)
    P0, P1, x, xp = ec.scene(rng, total)
    _, _, ex, exp_ = ec.class_table(17, npt=2000)          # edge rows (made for other cameras: just inputs here)
    for at in (0, stride - 1000, 2 * stride - 1000, total - 2000):
        x[at:at + 2000], xp[at:at + 2000] = ex, exp_
    dx, dxp = torch.from_numpy(x).cuda(), torch.from_numpy(xp).cuda()
    refX, refE = device.dlt_triangulate(P0, P1, dx, dxp), device.dlt_reprojection_error(P0, P1, dx, dxp)

    def same(a, b):
        return bool(((a.view(torch.int64) == b.view(torch.int64)) | (torch.isnan(a) & torch.isnan(b))).all())
    for npt in (1, 63, 64, 65, 257, stride - 1, stride, stride + 1, 2 * stride + 1):
        X = device.dlt_triangulate(P0, P1, dx[:npt], dxp[:npt])
        E = device.dlt_reprojection_error(P0, P1, dx[:npt], dxp[:npt])
        assert same(X, refX[:npt]) and same(E, refE[:npt]), npt
    torch.cuda.synchronize()
    # the superset really holds the edge rows
    assert int(torch.isnan(refE).sum()) > 1000 and int(torch.isposinf(refE).sum()) > 100


@pytest.mark.parametrize("seed", [5, 6])
def test_error_classes_match_the_mirror(oracle, seed):
    """On the class tables: the kernel's error class per row (finite / +inf / -inf / nan) equals the
    mirror's, which tests/test_dlt_invariance_oracle.py holds to the reference's IEEE formula -- in
    particular an overflowing squared residual comes out +inf, not nan.  The finite values stay
    within check_against_mirror's tolerance, and the RANSAC scorer counts none of the non-finite rows
    as an inlier."""
    import torch
    from spectavi_amd import device
    P0, P1, x, xp = ec.class_table(seed)
    mX = oracle.dlt_mirror_triangulate(P0, P1, x, xp)
    mE = oracle.dlt_mirror_reprojection_error(P0, P1, x, xp)[:, 0]
    cm = ec.error_class(mE)
    assert (cm == ec.POS_INF).sum() > 500 and (cm == ec.NAN).sum() > 2000
    for path, tri, rep in _hip_paths():
        X, E = tri(P0, P1, x, xp), rep(P0, P1, x, xp)[:, 0]
        ck = ec.error_class(E)
        wrong = ck != cm
        nan_for_inf = (ck == ec.NAN) & (cm == ec.POS_INF)
        assert not wrong.any(), "%s: error class differs from the mirror's at %d rows (%d nan where +inf)" % (
            path, wrong.sum(), nan_for_inf.sum())
        dc.check_against_mirror(X, mX, P0, P1, x, xp, E=E, mE=mE, what="%s, table %d" % (path, seed))
    rng = np.random.default_rng(seed)
    P1s = np.stack([P1, P1 + 1e-3 * rng.standard_normal((3, 4))])
    counts, mask = device.dlt_score_hypotheses(P0, torch.from_numpy(P1s).cuda(), torch.from_numpy(x).cuda(),
                                               torch.from_numpy(xp).cuda(), 1e-2, want_mask=True)
    mask = mask.cpu().numpy().astype(bool)
    assert not mask[:, cm != ec.FINITE].any()
    mc, mm = oracle.dlt_mirror_score_hypotheses(P0, P1s, x, xp, 1e-2)
    assert not mm[:, cm != ec.FINITE].any()
    assert counts.cpu().numpy()[0] > 0.2 * len(x)
