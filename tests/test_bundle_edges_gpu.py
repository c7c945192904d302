"""GPU: spv_bundle_adjust_device at the edges of its two orders and of "who takes part".  The shapes come from
spv_bundle_adjust_plan (the lane/wave boundary L, the view-major chunk size C), not from constants copied here.
`pytest -s` prints each measured figure before it is asserted (profiles/bundle_adjust.jsonl has them)."""
import numpy as np
import pytest

from tests import bundle_cases as bc
from tests import bundle_model as bm

pytestmark = pytest.mark.gpu

# Measured on one MI355X against the model on the host (profiles/bundle_adjust.jsonl), one step at lambda0 = 1e-2 with
# cg_tol = 1e-14; every bound is ten times the figure and none is beyond 1e-6.
# Lane/wave boundary: |delta_gpu - delta_model| / |delta_model| = 3.737e-13 (47 CG iterations, 68 free cameras), the
# points of the five boundary tracks within 3.268e-15.
BOUNDARY_DELTA, BOUNDARY_POINT = 3.8e-12, 3.3e-14
# Chunk boundaries: 2.420e-12 (against the sparse factorisation of the same normal equations), the 18 camera entries
# within 1.794e-14.  Two members of one set: 2.298e-14.
CHUNK_DELTA, CHUNK_CAMERA = 2.5e-11, 1.8e-13
DUPLICATE_DELTA = 2.3e-13

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def plan(*a, **kw):
    from spectavi_amd import device
    return device.bundle_adjust_plan(*a, **kw)


def lane_max():
    """L: the longest track the plan gives to one lane."""
    n = 1
    while plan([0, n + 1])["wave_tracks"] == 0:
        n += 1
        assert n < 4096
    return n


def one_step(sc, poses, X, mode, lambda0=1e-2, **kw):
    pb = bm.Problem(sc["geom"], sc["seg"], sc["K"], poses, mode, sc["track_off"], sc["members"], X, **kw)
    P, Xo, info = bc.run_gpu(sc, poses, X, mode, max_steps=1, lambda0=lambda0, cg_tol=1e-14, cg_max=10 * 6 * max(len(pb.free), 1),
                             ftol=0., gtol=0., **kw)
    delta, Fn, gmax, F = pb.step(pb.poses0, pb.Xe0, lambda0)
    assert info["trace"][0, 4] == 1 and Fn < F
    got = bc.recovered_delta(pb, poses, X, P, Xo)
    return pb, got, delta, info


def test_tracks_at_the_lane_wave_boundary():
    L = lane_max()
    lengths = np.concatenate([[L - 1, L, L + 1, 64, 65], np.random.default_rng(40).integers(2, 6, 300)])
    sc = bc.scene(70, len(lengths), seed=41, lengths=lengths)
    poses, X, mode = bc.perturbed(sc, seed=42)
    pl = plan(sc["track_off"])
    assert pl["wave_tracks"] == 3 and pl["lane_tracks"] == len(lengths) - 3 and pl["longest"] == 65
    pb, got, delta, info = one_step(sc, poses, X, mode)
    assert pb.active.all() and info["tracks"] == len(lengths) and info["observations"] == lengths.sum()
    rel = np.linalg.norm(got - delta) / np.linalg.norm(delta)
    first = np.max(np.abs(got[6 * len(pb.free):][:15] - delta[6 * len(pb.free):][:15]))
    print("boundary (L = %d): delta rel %.3e, the five boundary points' offset %.3e, cg %d" % (L, rel, first, info["trace"][0, 3]))
    assert rel <= min(BOUNDARY_DELTA, 1e-6) and first <= BOUNDARY_POINT


def test_cameras_at_the_chunk_boundaries():
    C = plan([0, 2])["chunk"]
    n = 2 * C + 1
    visible = np.ones((n, 5), bool)           # views 0 and 4 (fixed) see everything; 1, 2, 3 see C, C + 1 and 2 C + 1
    visible[C:, 1] = False
    visible[C + 1:, 2] = False
    sc = bc.scene(5, n, seed=43, visible=visible)
    poses, X, mode = bc.perturbed(sc, seed=44, fixed=(0, 4))
    pl = plan(sc["track_off"], sc["members"], sc["seg"], mode)
    assert pl["chunks"] == 1 + 2 + 3 and pl["chunk"] == C
    assert plan(sc["track_off"], sc["members"], sc["seg"])["chunks"] == 6 + 2 * 3
    pb, got, delta, info = one_step(sc, poses, X, mode)
    assert list(np.bincount(pb.obs_set)[1:4]) == [C, C + 1, 2 * C + 1]
    rel = np.linalg.norm(got - delta) / np.linalg.norm(delta)
    cam = np.max(np.abs(got[:18] - delta[:18]))
    print("chunks (C = %d): delta rel %.3e, camera entries' offset %.3e, cg %d" % (C, rel, cam, info["trace"][0, 3]))
    assert rel <= min(CHUNK_DELTA, 1e-6) and cam <= CHUNK_CAMERA


def test_free_camera_without_observations_stays():
    sc = bc.scene(5, 120, seed=45, min_len=2, max_len=4)
    poses, X, mode = bc.perturbed(sc, seed=46)
    off = sc["track_off"]
    sees3 = np.array([np.any(sc["members"][off[t]:off[t + 1], 0] == 3) for t in range(120)])
    assert 10 < sees3.sum() < 110
    use = (~sees3).astype(np.uint8)
    P, Xo, info = bc.run_gpu(sc, poses, X, mode, use=use, max_steps=6)
    assert info["accepted"] >= 2 and P[3].tobytes() == poses[3].tobytes() and np.abs(P[2] - poses[2]).max() > 1e-6
    assert np.array_equal(info["active"], use) and Xo[sees3].tobytes() == X[sees3].tobytes()
    # the same call with view 3 absent: the same bits everywhere else
    mode0 = mode.copy()
    mode0[3] = 0
    P0, X0, info0 = bc.run_gpu(sc, poses, X, mode0, use=use, max_steps=6)
    assert P0[[0, 1, 2, 4]].tobytes() == P[[0, 1, 2, 4]].tobytes() and X0.tobytes() == Xo.tobytes()
    assert info0["trace"].tobytes() == info["trace"].tobytes()


def test_tracks_that_do_not_take_part_leave_the_others_alone():
    """Switched-off tracks, rows of X that are not finite or have w = 0, tracks with one usable member and tracks that
    start behind a camera, and garbage members inside good tracks: the bad tracks come back untouched with d_active 0,
    and every other track and every camera has the bits of a call that never had them.  (F is summed over the call's
    tracks in track order, so its own last bits may differ between the two calls; the steps here are all accepted in
    both, and the parameters then agree bit for bit.)"""
    sc = bc.scene(6, 150, seed=47, min_len=2, max_len=4)
    poses, X, mode = bc.perturbed(sc, seed=48)
    mode[5] = 0                                   # a set without a camera: its members are ignored in both calls
    nseg, off, mem = 6, sc["track_off"], sc["members"]
    rows0 = int(sc["seg"][1] - sc["seg"][0])
    garbage = np.array([[I32_MIN, I32_MIN], [I32_MAX, I32_MAX], [nseg, 0], [-1, 0], [0, I32_MAX], [0, rows0], [1, -1], [5, 0]])
    tracks, Xs, use, kind = [], [], [], []
    for t in range(150):
        m = mem[off[t]:off[t + 1]]
        if t % 15 == 7:                           # garbage members inside a good track
            m = np.concatenate([m[:1], garbage[(t // 15) % 4 * 2:][:2], m[1:], garbage[-1:]])
        tracks.append(m), Xs.append(X[t]), use.append(1), kind.append("good")
        if t % 10 != 3:
            continue
        k = ("off", "nan", "inf", "w0", "single", "behind", "none")[(t // 10) % 7]
        bad_m, bad_X, bad_use = m.copy(), X[t].copy(), 1
        if k == "off":
            bad_use = 0
        elif k == "nan":
            bad_X[1] = np.nan
        elif k == "inf":
            bad_X[3] = np.inf
        elif k == "w0":
            bad_X[3] = 0.
        elif k == "single":
            bad_m[1:] = garbage[:len(bad_m) - 1]
        elif k == "behind":
            bad_X[2] = -bad_X[2]
        elif k == "none":
            bad_m[:] = garbage[2:3]
        tracks.append(bad_m), Xs.append(bad_X), use.append(bad_use), kind.append(k)
    kind = np.array(kind)
    assert set(kind) == {"good", "off", "nan", "inf", "w0", "single", "behind", "none"}
    ext = dict(sc, members=np.concatenate(tracks).astype(np.int32),
               track_off=np.concatenate([[0], np.cumsum([len(m) for m in tracks])]).astype(np.int64))
    Xe, use = np.array(Xs), np.array(use, np.uint8)
    kw = dict(max_steps=4, ftol=0., gtol=0., want_err=True)
    P, Xo, info = bc.run_gpu(ext, poses, Xe, mode, use=use, **kw)
    good = kind == "good"
    # (a good track whose other members all lie in the set without a camera does not take part in either call)
    pbb = bm.Problem(sc["geom"], sc["seg"], sc["K"], np.where(mode[:, None, None] == 0, 0., poses), mode, off, mem, X)
    assert 100 < pbb.active.sum() < 150
    assert np.array_equal(info["active"][good] != 0, pbb.active) and not info["active"][~good].any()
    assert info["tracks"] == pbb.active.sum()
    assert Xo[~good].tobytes() == Xe[~good].tobytes()
    track_of = np.repeat(np.arange(len(tracks)), [len(m) for m in tracks])
    assert np.all(np.isnan(info["err"][~good[track_of]]))
    # the call that never had them
    Pb, Xb, infob = bc.run_gpu(sc, poses, X, mode, **kw)
    assert np.all(info["trace"][:, 4] == 1) and np.all(infob["trace"][:, 4] == 1)
    assert infob["tracks"] == info["tracks"] and infob["observations"] == info["observations"]
    assert P.tobytes() == Pb.tobytes() and Xo[good].tobytes() == Xb.tobytes()
    assert np.allclose(info["trace"], infob["trace"], rtol=1e-12, atol=0)
    # the model agrees on who takes part
    pb = bm.Problem(ext["geom"], ext["seg"], ext["K"], np.where(mode[:, None, None] == 0, 0., poses), mode, ext["track_off"],
                    ext["members"], Xe, use=use)
    assert np.array_equal(pb.active, info["active"] != 0) and len(pb.obs_member) == info["observations"]
    assert np.array_equal(np.isfinite(info["err"]), np.isin(np.arange(len(track_of)), pb.obs_member))


def test_two_members_of_one_set_both_count():
    sc = bc.scene(4, 60, seed=49, min_len=2, max_len=4)
    poses, X, mode = bc.perturbed(sc, seed=50)
    off, mem = sc["track_off"], sc["members"]
    tracks = [mem[off[t]:off[t + 1]] for t in range(60)]
    for t in (0, 7, 30):        # the first member once more; in track 7 another row of the same set instead
        extra = tracks[t][:1].copy()
        if t == 7:
            extra[0, 1] = (extra[0, 1] + 1) % (sc["seg"][extra[0, 0] + 1] - sc["seg"][extra[0, 0]])
        tracks[t] = np.concatenate([tracks[t], extra])
    dup = dict(sc, members=np.concatenate(tracks).astype(np.int32),
               track_off=np.concatenate([[0], np.cumsum([len(m) for m in tracks])]).astype(np.int64))
    pb, got, delta, info = one_step(dup, poses, X, mode, huber=30.)
    assert info["observations"] == len(mem) + 3 == len(pb.obs_member)
    rel = np.linalg.norm(got - delta) / np.linalg.norm(delta)
    print("duplicates: delta rel %.3e, cg %d" % (rel, info["trace"][0, 3]))
    assert rel <= min(DUPLICATE_DELTA, 1e-6)


def test_a_step_behind_a_camera_is_rejected():
    """Gauss-Newton on a point four times too deep along the first camera's ray steps through the cameras' planes
    (the parallax is linear in 1 / depth): with a tiny lambda0 the first F' is +inf and the step is rejected."""
    sc = bc.scene(3, 40, seed=51, lengths=np.full(40, 3))
    mode = np.full(3, 2, np.int32)
    X = sc["X"].copy()
    X[5, :3] *= 4.
    pb = bm.Problem(sc["geom"], sc["seg"], sc["K"], sc["poses"], mode, sc["track_off"], sc["members"], X)
    assert pb.active.all() and pb.step(pb.poses0, pb.Xe0, 1e-12)[1] == np.inf
    P, Xo, info = bc.run_gpu(sc, sc["poses"], X, mode, max_steps=30, lambda0=1e-12)
    tr = info["trace"]
    assert tr[0, 1] == np.inf and tr[0, 4] == 0 and tr[1, 2] == 1e-12 * 10 and tr[1, 0] == tr[0, 0]
    assert tr[:, 4].sum() >= 1 and info["last_cost"] < info["first_cost"]
    assert np.all(np.isfinite(Xo)) and P.tobytes() == np.ascontiguousarray(sc["poses"]).tobytes()


def test_calls_in_which_no_track_takes_part():
    """No members at all, tracks without members, and every track switched off: nothing moves, d_active is 0, the
    trace stays NaN and info counts nothing."""
    sc = bc.scene(3, 20, seed=52, lengths=np.full(20, 3))
    poses, X, mode = bc.perturbed(sc, seed=53)
    empty = dict(sc, members=np.zeros((0, 2), np.int32), track_off=np.zeros(4, np.int64))
    for call, Xin, use in ((empty, X[:3], None), (sc, X, np.zeros(20, np.uint8))):
        P, Xo, info = bc.run_gpu(call, poses, Xin, mode, use=use, max_steps=5, want_err=True)
        assert P.tobytes() == np.ascontiguousarray(poses).tobytes() and Xo.tobytes() == np.ascontiguousarray(Xin).tobytes()
        assert not info["active"].any() and np.all(np.isnan(info["err"])) and info["trace"].shape == (0, 6)
        assert (info["steps"], info["tracks"], info["observations"], info["first_cost"], info["last_cost"]) == (0, 0, 0, 0., 0.)
    # tracks without members among the others: the others' results are those of a call without them
    lengths = np.full(20, 3)
    lengths2 = np.insert(lengths, [0, 7, 20], 0)
    X2 = np.insert(X, [0, 7, 20], np.full(4, 9.0), axis=0)
    holes = dict(sc, track_off=np.concatenate([[0], np.cumsum(lengths2)]).astype(np.int64))
    kw = dict(max_steps=3, ftol=0., gtol=0.)
    Pa, Xa, ia = bc.run_gpu(sc, poses, X, mode, **kw)
    Pb, Xb, ib = bc.run_gpu(holes, poses, X2, mode, **kw)
    real = lengths2 > 0
    assert np.array_equal(ib["active"] != 0, real) and np.all(Xb[~real] == 9.0)
    assert Pa.tobytes() == Pb.tobytes() and Xa.tobytes() == np.ascontiguousarray(Xb[real]).tobytes()
