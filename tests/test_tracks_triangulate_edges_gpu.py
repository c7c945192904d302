"""triangulate_tracks off its well-posed inputs, on the GPU (cases: tests/tracks_triangulate_edge_cases.py), in
both forms of the kernel: every case runs with all tracks of 3 and more members in the wave form, with none, and
under the default L = 16.

Measured on one MI355X (the tests print these with -s; profiles/resect_tracks_edges.md has all), the same under the
three settings unless said: mismatched tracks -- worst residual excess -1.055e-11 sigma1, direction 6.66e-16, err 3.88e-7
of its tolerance (3.75e-7 with no track in the wave form), 1 of 360 undecided, |X - X'| between the forms up to 1.1e-2
of its bound; rank deficiency -- residual excess -1.0e-13 sigma1, direction 1.1e-16; cameras times 2^-40, 2^-1, 2^3,
2^40 and -1 -- X and err bit for bit, ok and nused equal; times 2^+-445 -- residual excess -1.036e-13 sigma1, direction
4.4e-16, err 7.1e-5 of its tolerance; members that are not finite -- ok 0 on all, X finite on all, every other track the
clean call's bits.  A solve_matrix without its null_jacobi call fails test_mismatched_tracks and
test_rank_deficient_tracks."""
import numpy as np
import pytest

from tests import tracks_triangulate_edge_cases as tec
from tests import tracks_triangulate_model as ttm

pytestmark = pytest.mark.gpu


def run(sc, max_error=float("inf")):
    import torch
    from spectavi_amd import device
    out = device.triangulate_tracks(torch.from_numpy(np.ascontiguousarray(sc["geom"])).cuda(), sc["seg"], sc["cams"], sc["off"],
                                    torch.from_numpy(np.ascontiguousarray(sc["mem"], np.int32).reshape(-1, 2)).cuda(),
                                    max_error=max_error)
    return tuple(t.cpu().numpy() for t in out)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture
def settings():
    """Runs a function under the three settings and restores the default."""
    from spectavi_amd import device
    before = device.tracks_triangulate_get_long()
    assert before == tec.L0

    def each(fn):
        out = {}
        for L in tec.SETTINGS:
            device.tracks_triangulate_set_long(L)
            out[L] = fn(L)
        return out
    yield each
    device.tracks_triangulate_set_long(before)


def forms(sc, L):
    from spectavi_amd import device
    plan = device.triangulate_tracks_plan(sc["off"])
    waves = int(((sc["lengths"] >= 3) & (sc["lengths"] > L)).sum())
    assert (plan["wave_tracks"], plan["lane_tracks"]) == (waves, len(sc["lengths"]) - waves)
    return waves


# ---- (a) ----------------------------------------------------------------------------------------------------------------
def test_mismatched_tracks(settings):
    """360 tracks whose observations agree on no point: the inverse iteration does not converge (tests/
    test_tracks_triangulate_edge_cases.py) and the Jacobi solves the Givens triangle, per lane and per wave."""
    sc = tec.mismatched()
    mo = sc["mo"]

    def one(L):
        waves = forms(sc, L)
        X, err, ok, nused = res = run(sc)
        st = ttm.check_definition(X, err, mo, sc["geom"], sc["seg"], sc["off"], sc["mem"], long_c=sc["long_c"], what="L = %d" % L)
        und = ttm.check_verdict(ok, nused, mo, sc["geom"], sc["seg"], sc["off"], sc["mem"], np.inf, what="L = %d" % L)
        print("L = %d (%d tracks in the wave form): worst residual excess %.3e sigma1, direction %.3e, err ratio %.3e, undecided %d" % (
            L, waves, st["worst_residual_excess"], st["worst_direction"], st["worst_err_rel"], und))
        assert st["tracks"] == st["well_separated"] == 360
        return res
    res = settings(one)
    tol = tec.form_tolerance(sc)
    for other in (0, 10 ** 9):
        diff = np.abs(res[tec.L0][0] - res[other][0]).max(axis=1)
        print("L = %d against the default: worst |X - X'| / bound %.3e" % (other, (diff / tol).max()))
        assert np.all(diff <= tol), (other, np.flatnonzero(diff > tol)[:8], diff.max())
        assert np.array_equal(res[tec.L0][3], res[other][3])


# ---- (b) ----------------------------------------------------------------------------------------------------------------
def test_rank_deficient_tracks(settings):
    sc = tec.rank_deficient()
    mo = sc["mo"]
    # err is held to the model on the ordinary tracks alone: tracks 3-5 divide by a depth that is a rounding of 0
    ordinary = np.repeat(np.arange(len(sc["lengths"])) >= 6, sc["lengths"])

    def one(L):
        forms(sc, L)
        X, err, ok, nused = run(sc)
        st = ttm.check_definition(X, None, mo, sc["geom"], sc["seg"], sc["off"], sc["mem"], long_c=sc["long_c"], what="L = %d" % L)
        assert st["tracks"] == 10 and st["well_separated"] == 7, "the repeated observation alone is not separated"
        assert np.array_equal(nused, mo["nused"]) and np.array_equal(nused, sc["lengths"])
        for t in range(3, 6):
            C = tec.camera_centre(sc["cams"][int(sc["mem"][sc["off"][t], 0])])
            assert abs(abs(C @ X[t]) - 1) <= 1e-9, (L, t)
        sub = dict(mo, err=np.where(ordinary, mo["err"], np.nan))
        ttm.check_definition(X, np.where(ordinary, err, np.nan), sub, sc["geom"], sc["seg"], sc["off"], sc["mem"],
                             long_c=sc["long_c"], what="L = %d" % L)
        assert np.all(np.isfinite(err[ordinary])) and np.all(ok[6:] == 1) and np.array_equal(ok[6:], mo["ok"][6:])
        for t, two in ((6, 8), (7, 9)):
            S, slack = mo["S"][two], 2 * mo["formation"][two]
            d = 1 - abs(X[t] @ X[two])
            assert d <= 1e-9 + 2 * (slack / (S[2] - S[3])) ** 2, (L, t, d)
        print("L = %d: worst residual excess %.3e sigma1, direction %.3e; ok of the deficient tracks %s" % (
            L, st["worst_residual_excess"], st["worst_direction"], ok[:6].tolist()))
        return X
    settings(one)


# ---- (c) ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unscaled():
    """The `edges` scene under the three settings, once."""
    from spectavi_amd import device
    sc = tec.edges()
    out = {}
    try:
        for L in tec.SETTINGS:
            device.tracks_triangulate_set_long(L)
            out[L] = run(sc, 6.0)
    finally:
        device.tracks_triangulate_set_long(tec.L0)
    return out


@pytest.mark.parametrize("k,sign", [(k, 1.0) for k in tec.SCALES] + [(0, -1.0)], ids=["2^%d" % k for k in tec.SCALES] + ["-1"])
def test_rescaled_cameras_give_the_same_bits(settings, unscaled, k, sign):
    """All cameras times 2^k or -1: every Givens step, the butterfly merge, the solver and the residuals commute with
    it, so X and err keep their bits and ok and nused their values.  Held on one MI355X for the five factors under
    the three settings."""
    sc = tec.scaled_cameras(tec.edges(), k, sign)

    def one(L):
        forms(sc, L)
        X, err, ok, nused = run(sc, 6.0)
        bX, berr, bok, bnused = unscaled[L]
        dX = np.flatnonzero((bits(X) != bits(bX)).any(axis=1))
        assert dX.size == 0, (L, "X differs at %d tracks, first %d of %d members" % (dX.size, dX[0], sc["lengths"][dX[0]]))
        de = np.flatnonzero(bits(err) != bits(berr))
        assert de.size == 0, (L, "err differs at %d members" % de.size)
        assert np.array_equal(ok, bok) and np.array_equal(nused, bnused)
    settings(one)


@pytest.mark.parametrize("k", tec.FAR_SCALES)
def test_cameras_at_the_far_scales(settings, k):
    """All cameras times 2^+-445: the Givens stage's h = a^2 + b^2 leaves [2^-900, 2^900] and rsqrt_guarded divides.
    The definition is held against the model of the scaled cameras; ok is not (the determinant of the left 3 x 3 block
    leaves the double range, in numpy as on the device)."""
    sc = tec.scaled_cameras(tec.edges(), k)
    mo = ttm.model(*tec.args(sc), max_error=6.0)
    # a residual does not change with the cameras' scale, so its tolerance is the unscaled problem's: the criterion
    # reads the depth in the scene's units
    mo["depth"] = np.ldexp(mo["depth"], -k)

    def one(L):
        forms(sc, L)
        X, err, ok, nused = run(sc, 6.0)
        st = ttm.check_definition(X, err, mo, sc["geom"], sc["seg"], sc["off"], sc["mem"], long_c=sc["long_c"], what="2^%d, L = %d" % (k, L))
        assert np.array_equal(nused, mo["nused"]) and st["tracks"] == st["well_separated"] == len(sc["lengths"])
        print("2^%d, L = %d: worst residual excess %.3e sigma1, direction %.3e, err ratio %.3e" % (
            k, L, st["worst_residual_excess"], st["worst_direction"], st["worst_err_rel"]))
    settings(one)


# ---- (d) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", tec.POISON_KINDS)
def test_members_that_are_not_finite(settings, kind):
    """A NaN or +inf observation, or a camera with a NaN entry, in one usable member of tracks of 2, 3, 5, 17, 65 and
    129 members: those tracks are not ok and count the member; every other track keeps the clean call's bits."""
    clean, dirty, tracks = tec.poisoned(kind)
    want_nused = tec.nused_of(dirty)
    other = np.ones(len(clean["lengths"]), bool)
    other[tracks] = False
    mother = np.repeat(other, clean["lengths"])

    def one(L):
        forms(dirty, L)
        bX, berr, bok, bnused = run(clean, 6.0)
        X, err, ok, nused = run(dirty, 6.0)
        assert np.array_equal(nused, want_nused) and np.array_equal(bnused, want_nused)
        assert not ok[tracks].any(), (L, ok[tracks])
        assert same_bits(X[other], bX[other]) and same_bits(err[mother], berr[mother]) and np.array_equal(ok[other], bok[other])
        print("%s, L = %d: X finite at %s of the tracks of %s members" % (
            kind, L, np.isfinite(X[tracks]).all(axis=1).astype(int).tolist(), clean["lengths"][tracks].tolist()))
    settings(one)
