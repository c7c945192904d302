"""GPU: spv_bundle_adjust_device against tests/bundle_model.py (dense normal equations, numpy.linalg.solve) on the
scenes of tests/bundle_cases.py.  The bounds marked "measured" are ten times the largest figure one MI355X gave
(profiles/bundle_adjust.jsonl has the figures); `pytest -s` prints each figure before it is asserted."""
import numpy as np
import pytest

from tests import bundle_cases as bc
from tests import bundle_model as bm

pytestmark = pytest.mark.gpu

# Measured on one MI355X against the model on the host (profiles/bundle_adjust.jsonl); every bound is ten times the
# largest figure, because CG stops on a preconditioned residual and not on the error, and none is beyond 1e-6.
# One step, lambda0 in {1e-6, 1e-2, 1e2}: |delta_gpu - delta_model| / |delta_model| = 4.627e-13, 2.956e-14, 1.246e-13.
ONE_STEP_DELTA = 4.7e-12
# One step: |F - F_model| / F_model = 3.835e-16 in all three; |F' - F'_model| / F'_model = 1.028e-13, 4.729e-14,
# 4.002e-16 (at lambda0 = 1e-6 F' is 5.6e-5 of F and feels delta's error that much more).
ONE_STEP_COST, ONE_STEP_COST_NEW = 3.9e-15, 1.1e-12
# Whole loop against the model's: the largest rotation angle between the two (rad) 6.083e-15, centre offset 3.642e-14
# and point offset 4.796e-14 (scene units; the scene is about 6 deep).  All cameras fixed, three steps: 8.882e-15.
LOOP_ROTATION, LOOP_CENTRE, LOOP_POINT, FIXED_POINT = 6.1e-14, 3.7e-13, 4.8e-13, 8.9e-14


run, recovered_delta = bc.run_gpu, bc.recovered_delta


@pytest.fixture(scope="module")
def small():
    sc = bc.scene(4, 60, seed=21, min_len=2, max_len=4)
    poses, X, mode = bc.perturbed(sc, seed=22)
    return sc, poses, X, mode, bm.Problem(sc["geom"], sc["seg"], sc["K"], poses, mode, sc["track_off"], sc["members"], X)


@pytest.fixture(scope="module")
def loop_scene():
    sc = bc.scene(5, 200, seed=31, min_len=2, max_len=5)
    poses, X, mode = bc.perturbed(sc, seed=32)
    pb = bm.Problem(sc["geom"], sc["seg"], sc["K"], poses, mode, sc["track_off"], sc["members"], X)
    return sc, poses, X, mode, pb, pb.run(max_steps=50)


@pytest.mark.parametrize("lambda0", [1e-6, 1e-2, 1e2])
def test_one_step_is_the_dense_solve(small, lambda0):
    sc, poses, X, mode, pb = small
    nfree = len(pb.free)
    P, Xo, info = run(sc, poses, X, mode, max_steps=1, lambda0=lambda0, cg_tol=1e-14, cg_max=10 * 6 * nfree, ftol=0., gtol=0.)
    delta, Fn, gmax, F = pb.step(pb.poses0, pb.Xe0, lambda0)
    row = info["trace"][0]
    assert info["steps"] == 1 and row[4] == 1 and row[2] == lambda0 and Fn < F
    got = recovered_delta(pb, poses, X, P, Xo)
    rel = np.linalg.norm(got - delta) / np.linalg.norm(delta)
    relF, relFn, relg = abs(row[0] - F) / F, abs(row[1] - Fn) / Fn, abs(row[5] - gmax) / gmax
    print("one step lambda0=%g: delta rel %.3e, F rel %.3e, F' rel %.3e (F'/F %.3e), max|g| rel %.3e, cg %d"
          % (lambda0, rel, relF, relFn, Fn / F, relg, row[3]))
    assert rel <= min(ONE_STEP_DELTA, 1e-6)
    assert relF <= ONE_STEP_COST and relFn <= ONE_STEP_COST_NEW
    assert relg <= 1e-12      # a sum of a few hundred products of one sign pattern: n eps, not measured into a bound
    assert info["first_cost"] == row[0] and info["last_cost"] == row[1]
    assert info["tracks"] == len(pb.pts) and info["observations"] == len(pb.obs_member)


def test_whole_loop_noise_free(loop_scene):
    sc, poses, X, mode, pb, (mposes, mX, minfo) = loop_scene
    P, Xo, info = run(sc, poses, X, mode, max_steps=50, want_err=True)
    tr = info["trace"]
    rot = max(bc.rotation_angle(P[s][:, :3], mposes[s][:, :3]) for s in pb.free)
    cen = max(np.max(np.abs(bc.centre(P[s]) - bc.centre(mposes[s]))) for s in pb.free)
    pts = np.max(np.abs(Xo[:, :3] - mX[:, :3]))
    print("loop: F %.6e model %.6e (first %.3e), steps %d/%d model %d, stop %s/%s, rot %.3e centre %.3e point %.3e"
          % (info["last_cost"], minfo["last_cost"], info["first_cost"], info["accepted"], info["steps"], minfo["steps"],
             info["stop"], minfo["stop"], rot, cen, pts))
    assert info["last_cost"] <= (1 + 1e-6) * minfo["last_cost"]
    assert rot <= LOOP_ROTATION and cen <= LOOP_CENTRE and pts <= LOOP_POINT
    acc = tr[tr[:, 4] == 1]
    assert len(acc) >= 3 and np.all(np.diff(acc[:, 1]) < 0) and np.all(acc[:, 1] < acc[:, 0])
    assert np.all(Xo[:, 3] == 1) and info["active"].all()
    # err is the residual norm at the returned parameters
    want = pb.err(P, Xo)
    assert np.allclose(info["err"], want, rtol=0, atol=1e-9) and np.isclose(np.sum(want ** 2) / 2, info["last_cost"], rtol=1e-9)


def test_outliers_huber_beats_least_squares():
    sc = bc.scene(5, 200, seed=31, min_len=2, max_len=5, noise=0.5, outliers=0.05)
    poses, X, mode = bc.perturbed(sc, seed=32)
    pb = bm.Problem(sc["geom"], sc["seg"], sc["K"], poses, mode, sc["track_off"], sc["members"], X, huber=2.)
    _, _, minfo = pb.run(max_steps=50)
    P, _, info = run(sc, poses, X, mode, max_steps=50, huber=2.)
    Pl, _, linfo = run(sc, poses, X, mode, max_steps=50)
    off = sum(np.linalg.norm(bc.centre(P[s]) - bc.centre(sc["poses"][s])) for s in pb.free)
    offl = sum(np.linalg.norm(bc.centre(Pl[s]) - bc.centre(sc["poses"][s])) for s in pb.free)
    rot = sum(bc.rotation_angle(P[s][:, :3], sc["poses"][s][:, :3]) for s in pb.free)
    rotl = sum(bc.rotation_angle(Pl[s][:, :3], sc["poses"][s][:, :3]) for s in pb.free)
    print("outliers: F %.9e model %.9e; centre offsets huber %.3e inf %.3e; rotations %.3e %.3e; steps %d %d"
          % (info["last_cost"], minfo["last_cost"], off, offl, rot, rotl, info["steps"], linfo["steps"]))
    assert info["last_cost"] <= (1 + 1e-6) * minfo["last_cost"]
    assert off < offl and rot < rotl


def test_same_bits_from_run_to_run(loop_scene):
    sc, poses, X, mode, pb, _ = loop_scene
    a = run(sc, poses, X, mode, max_steps=8, huber=2., want_err=True)
    b = run(sc, poses, X, mode, max_steps=8, huber=2., want_err=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert a[2]["err"].tobytes() == b[2]["err"].tobytes() and a[2]["trace"].tobytes() == b[2]["trace"].tobytes()
    assert a[2]["steps"] == 8 or a[2]["stop"] != "max_steps"


def test_all_cameras_fixed_moves_points_alone(loop_scene):
    sc, poses, X, _, _, _ = loop_scene
    mode = np.full(sc["nviews"], 2, np.int32)
    pb = bm.Problem(sc["geom"], sc["seg"], sc["K"], poses, mode, sc["track_off"], sc["members"], X)
    mposes, mX, minfo = pb.run(max_steps=3, ftol=0., gtol=0.)
    P, Xo, info = run(sc, poses, X, mode, max_steps=3, ftol=0., gtol=0.)
    assert P.tobytes() == np.ascontiguousarray(poses).tobytes()
    assert np.all(info["trace"][:, 4] == 1) and np.all(info["trace"][:, 3] == 0)
    diff = np.max(np.abs(Xo - mX))
    print("all fixed: point offset %.3e, F %.6e model %.6e" % (diff, info["last_cost"], minfo["last_cost"]))
    assert diff <= FIXED_POINT
    # the points decouple: while every step is accepted (as here, in both calls), a track's result is its own
    keep = np.arange(0, 200, 3)
    off = sc["track_off"]
    sub = dict(sc, track_off=np.concatenate([[0], np.cumsum(np.diff(off)[keep])]),
               members=np.concatenate([sc["members"][off[t]:off[t + 1]] for t in keep]))
    Ps, Xs, sinfo = run(sub, poses, np.ascontiguousarray(X[keep]), mode, max_steps=3, ftol=0., gtol=0.)
    assert np.all(sinfo["trace"][:, 4] == 1)
    assert Xs.tobytes() == np.ascontiguousarray(Xo[keep]).tobytes()


def test_no_point_moves_a_fixed_or_absent_camera(loop_scene):
    sc, poses, X, _, _, _ = loop_scene
    mode = np.array([2, 1, 0, 1, 2], np.int32)
    P, Xo, info = run(sc, poses, X, mode, max_steps=10)
    assert info["accepted"] >= 2
    for s in (0, 4):
        assert P[s].tobytes() == poses[s].tobytes()
    assert not P[2].any()
    for s in (1, 3):
        assert np.abs(P[s] - poses[s]).max() > 1e-6
    # set 2 has no camera: its members are ignored, tracks left with fewer than two do not take part
    pb = bm.Problem(sc["geom"], sc["seg"], sc["K"], np.where(mode[:, None, None] == 0, 0., poses), mode, sc["track_off"],
                    sc["members"], X)
    assert np.array_equal(info["active"] != 0, pb.active) and 0 < pb.active.sum() < len(pb.active)
    assert Xo[~pb.active].tobytes() == X[~pb.active].tobytes()
    assert info["tracks"] == pb.active.sum() and info["observations"] == len(pb.obs_member)


def test_every_kernel_has_a_profile_name(small):
    """The names include/spectavi_amd.h lists for spv_profile_read, on a call with lane-form tracks only (the scene has
    no track beyond four members) and CG iterations that end before cg_max."""
    from spectavi_amd import device
    sc, poses, X, mode, pb = small
    names = ("bundle_mark", "bundle_sort", "bundle_linearise", "bundle_cam_sum", "bundle_gradient_max", "bundle_cost_sum",
             "bundle_point_blocks", "bundle_precondition", "bundle_cg_start", "bundle_cg_track", "bundle_cg_cam",
             "bundle_cg_step", "bundle_move", "bundle_cost", "bundle_commit", "bundle_finish")
    device.profile_enable(True)
    device.profile_reset()
    try:
        _, _, info = run(sc, poses, X, mode, max_steps=2, ftol=0., gtol=0., cg_max=20)
        got = {n: device.profile_read(n)[0] for n in names}
    finally:
        device.profile_enable(False)
        device.profile_reset()
    assert info["steps"] == 2 and np.all(info["trace"][:, 3] < 20)
    once = dict(bundle_mark=1, bundle_sort=1, bundle_finish=1)
    per_step = dict(bundle_point_blocks=1, bundle_precondition=1, bundle_cg_start=1, bundle_cg_step=20, bundle_move=1,
                    bundle_cost=1, bundle_commit=1, bundle_cg_track=21, bundle_cg_cam=21)
    want = dict(once, **{n: 2 * k for n, k in per_step.items()})
    want.update(bundle_linearise=3, bundle_cam_sum=3, bundle_gradient_max=3, bundle_cost_sum=3)
    assert got == want
