"""CPU-only: the yardstick of the bundle adjustment tests, tests/bundle_model.py, checked against
scipy.optimize.least_squares on the same residual function and against central differences."""
import numpy as np
import pytest

from tests import bundle_cases as bc
from tests import bundle_model as bm


@pytest.fixture(scope="module")
def problem():
    sc = bc.scene(4, 30, seed=11, min_len=2, max_len=4)
    poses, X, mode = bc.perturbed(sc, seed=12)
    return sc, bm.Problem(sc["geom"], sc["seg"], sc["K"], poses, mode, sc["track_off"], sc["members"], X)


def unpack(pb, x):
    return pb.moved(pb.poses0, pb.Xe0, x)


def test_every_track_takes_part(problem):
    sc, pb = problem
    assert pb.active.all() and len(pb.obs_member) == len(sc["members"]) and list(pb.free) == [2, 3]


def test_analytic_jacobian_matches_central_differences(problem):
    _, pb = problem
    _, J, _ = pb.linearise(pb.poses0, pb.Xe0)
    h = 1e-6
    for k in range(pb.nunknowns):
        e = np.zeros(pb.nunknowns)
        e[k] = h
        rp, _ = pb.residuals(*unpack(pb, e))
        rm, _ = pb.residuals(*unpack(pb, -e))
        num = ((rp - rm) / (2 * h)).reshape(-1)
        # second differences of a projection at 1 % from the solution: |error| ~ h^2 |r'''| + eps |r| / h
        assert np.max(np.abs(num - J[:, k])) <= 1e-5 * max(1., np.max(np.abs(J[:, k]))), k


def test_huber_weights_scale_rows_and_residuals():
    sc = bc.scene(4, 30, seed=13, noise=0.5, outliers=0.1)
    poses, X, mode = bc.perturbed(sc, seed=14)
    plain = bm.Problem(sc["geom"], sc["seg"], sc["K"], poses, mode, sc["track_off"], sc["members"], X)
    robust = bm.Problem(sc["geom"], sc["seg"], sc["K"], poses, mode, sc["track_off"], sc["members"], X, huber=2.)
    r0, J0, F0 = plain.linearise(plain.poses0, plain.Xe0)
    r1, J1, F1 = robust.linearise(robust.poses0, robust.Xe0)
    n = np.hypot(r0[0::2], r0[1::2])
    sw = np.sqrt(np.minimum(1., 2. / n))
    assert np.any(sw < 1)
    assert np.allclose(r1, r0 * np.repeat(sw, 2), rtol=1e-14) and np.allclose(J1, J0 * np.repeat(sw, 2)[:, None], rtol=1e-14)
    assert np.isclose(F1, np.sum(np.where(n <= 2, n * n / 2, 2 * (n - 1))), rtol=1e-14) and F1 < F0


def test_loop_agrees_with_scipy_least_squares(problem):
    import scipy.optimize as scipy_optimize
    sc, pb = problem

    def fun(x):
        r, _ = pb.residuals(*unpack(pb, x))
        return r.reshape(-1)

    ref = scipy_optimize.least_squares(fun, np.zeros(pb.nunknowns), method="trf", x_scale="jac", xtol=1e-15, ftol=1e-15,
                                       gtol=1e-15, max_nfev=200)
    poses, X, info = pb.run(max_steps=50)
    # float32 pixels leave a residual floor; both minimisers must sit on it
    assert info["stop"] in ("cost", "gradient") and info["last_cost"] < info["first_cost"] * 1e-6
    assert abs(info["last_cost"] - ref.cost) <= 1e-6 * ref.cost
    rposes, rXe = unpack(pb, ref.x)
    # at the minimum |dx| ~ sqrt(2 dF / lambda_min(H)); with dF <= 1e-6 F and F ~ 1e-7 px^2 that is far below 1e-6
    for s in pb.free:
        assert bc.rotation_angle(poses[s][:, :3], rposes[s][:, :3]) <= 1e-6
        assert np.max(np.abs(bc.centre(poses[s]) - bc.centre(rposes[s]))) <= 1e-6
    assert np.max(np.abs(X[:, :3] - rXe)) <= 1e-6
    # and both found the scene
    for s in pb.free:
        assert np.max(np.abs(bc.centre(poses[s]) - bc.centre(sc["poses"][s]))) <= 1e-4


def test_trace_and_stops():
    sc = bc.scene(4, 30, seed=15)
    poses, X, mode = bc.perturbed(sc, seed=16)
    pb = bm.Problem(sc["geom"], sc["seg"], sc["K"], poses, mode, sc["track_off"], sc["members"], X)
    _, _, info = pb.run(max_steps=3, ftol=0., gtol=0.)
    assert info["stop"] == "max_steps" and info["steps"] == 3
    acc = info["trace"][info["trace"][:, 4] == 1]
    assert np.all(np.diff(acc[:, 1]) < 0) and np.all(acc[:, 1] < acc[:, 0])
    _, _, info = pb.run(max_steps=3, gtol=1e30)
    assert info["stop"] == "gradient" and info["steps"] == 0
