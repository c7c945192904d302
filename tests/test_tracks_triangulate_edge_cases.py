"""The conditions the GPU tests of tests/test_tracks_triangulate_edges_gpu.py rest on, checked on the numpy model
without a GPU."""
import numpy as np

from tests import tracks_triangulate_edge_cases as tec
from tests import tracks_triangulate_model as ttm


def test_mismatched_tracks_defeat_the_inverse_iteration():
    """rho = (sigma4 / sigma3)^2 is the contraction of a step; a direction error that starts at O(1) and shrinks by
    rho >= 0.1 a step is above 1e-13 after 8 steps, so such a track takes the Jacobi route."""
    sc = tec.mismatched()
    mo, lengths = sc["mo"], sc["lengths"]
    rho = tec.contraction(mo)
    assert mo["solved"].all() and len(lengths) == 360 and np.array_equal(mo["nused"], lengths)
    for m in tec.MISMATCH_LENGTHS:
        share = float((rho[lengths == m] >= 0.1).mean())
        print("length %3d: rho >= 0.1 on %3.0f %%, least rho %.3f" % (m, 100 * share, rho[lengths == m].min()))
        assert share >= 0.7, m
        if m >= 8:
            assert share == 1.0, m
    gap = (mo["S"][:, 2] - mo["S"][:, 3]) / mo["S"][:, 0]
    print("least (sigma3 - sigma4) / sigma1 %.2e" % gap.min())
    assert gap.min() > 1e-3 > ttm.GAP, "every track is well separated"
    und = ttm.verdict_undecided(mo, sc["geom"], sc["seg"], sc["off"], sc["mem"], np.inf)
    print("undecided %d of %d" % (und.sum(), len(und)))
    assert und.sum() <= 0.01 * len(und)
    assert sc["long_c"] == 0.0, "the float64 QR route stays inside the floor on the long tracks"


def test_rank_deficient_tracks_are_what_they_claim():
    sc = tec.rank_deficient()
    mo, off, mem = sc["mo"], sc["off"], sc["mem"]
    S = mo["S"]
    assert sc["lengths"].tolist() == [3, 17, 65, 3, 17, 65, 17, 65, 2, 2] and mo["solved"].all()
    for t in range(3):      # rank 2
        assert S[t, 2] <= 1e-12 * S[t, 0] and len(set(map(tuple, mem[off[t]:off[t + 1]]))) == 1
    for t in range(3, 6):   # rank 3, well separated: the camera centre
        s = int(mem[off[t], 0])
        assert S[t, 3] <= 1e-12 * S[t, 0] and S[t, 2] - S[t, 3] > 1e-3 * S[t, 0] and np.all(mem[off[t]:off[t + 1], 0] == s)
        C = tec.camera_centre(sc["cams"][s])
        assert abs(abs(C @ mo["X"][t]) - 1) <= 1e-9, t
        assert np.all(np.abs(mo["depth"][off[t]:off[t + 1]]) < 1e-9), "the depth term is a rounding of 0"
    for t, two in ((6, 8), (7, 9)):
        assert S[t, 2] - S[t, 3] > 1e-3 * S[t, 0] and mo["ok"][t] == mo["ok"][two] == 1
        assert set(map(tuple, mem[off[t]:off[t + 1]])) == set(map(tuple, mem[off[two]:off[two + 1]]))
        d = 1 - abs(mo["X"][t] @ mo["X"][two])
        print("track %d against its two-member track: 1 - |<X, X'>| = %.2e" % (t, d))
        assert d <= 1e-10, "the unequal weights of the two observations stay inside the direction tolerance"


def test_edges_scene_is_the_gpu_tests_scene():
    sc = tec.edges()
    assert sc["lengths"][:8].tolist() == tec.EDGE_LONG and len(sc["lengths"]) == 263 and sc["geom"].dtype == np.float32
    mo = sc["mo"]
    assert mo["solved"].all() and np.all(mo["S"][:, 2] - mo["S"][:, 3] > ttm.GAP * mo["S"][:, 0]) and sc["long_c"] == 0.0
    # rescaled cameras are exact, and the far scales take the Givens stage's h = a^2 + b^2 beyond 2^900
    for k in tec.SCALES + tec.FAR_SCALES:
        cams = tec.scaled_cameras(sc, k)["cams"]
        assert np.array_equal(np.ldexp(cams, -k), sc["cams"]) and np.isfinite(cams).all() and np.all(cams[sc["cams"] != 0] != 0)
    far = ttm.model(*tec.args(tec.scaled_cameras(sc, 445)))
    assert np.all(far["S"][:, 0] ** 2 > 2.0 ** 900) and np.isfinite(far["S"]).all()
    near = ttm.model(*tec.args(tec.scaled_cameras(sc, -445)))
    assert np.all(near["S"][:, 3] ** 2 < 2.0 ** -850) and np.all(near["S"][:, 3] > 0)
    for mo2, k in ((far, 445), (near, -445)):      # the model itself commutes with the scale
        assert np.allclose(np.ldexp(mo2["S"], -k), mo["S"], rtol=1e-12) and np.all(np.abs(np.sum(mo2["X"] * mo["X"], 1)) > 1 - 1e-12)
        assert np.allclose(mo2["err"], mo["err"], rtol=1e-9, atol=1e-12)


def test_poisoned_members_stay_usable():
    sc = tec.edges()
    for kind in tec.POISON_KINDS:
        clean, dirty, tracks = tec.poisoned(kind)
        assert sc["lengths"][tracks].tolist() == list(tec.POISON_LANE + tec.POISON_WAVE)
        assert np.array_equal(tec.nused_of(dirty), sc["lengths"]), "a member that is not finite is usable by the contract"
        assert np.isfinite(clean["geom"][:, :2]).all() and np.isfinite(clean["cams"]).all()
        bad_rows = np.flatnonzero(~np.isfinite(dirty["geom"][:, :2]).all(axis=1))
        if kind == "nan camera":
            assert bad_rows.size == 0 and np.isnan(dirty["cams"][40]).sum() == 1 and np.isfinite(dirty["cams"][:40]).all()
            uses = np.flatnonzero(dirty["mem"][:, 0] == 40)
            assert (np.searchsorted(sc["off"], uses, "right") - 1).tolist() == sorted(tracks)
        else:
            assert bad_rows.size == 6 and np.array_equal(dirty["cams"], clean["cams"])
            rows = dirty["seg"][dirty["mem"][:, 0]] + dirty["mem"][:, 1]
            hit = np.flatnonzero(np.isin(rows, bad_rows))
            assert sorted(set((np.searchsorted(sc["off"], hit, "right") - 1).tolist())) == sorted(tracks)
