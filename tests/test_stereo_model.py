"""tests/stereo_model.py against its own literal transcription, and the geometric sanity of the stereo_batch
contract on the plane scene.  No GPU: the device ops are held to this model in tests/test_stereo_batch_gpu.py."""
import functools

import numpy as np
import pytest

from tests import stereo_model as sm


def window_case(rng, R, C, kind):
    if kind == "equal":
        a = np.full((R, C), 77, np.uint8)
        b = a.copy()
    elif kind == "coarse":  # few grey levels: many ties between disparities
        a = rng.integers(0, 3, (R, C)).astype(np.uint8)
        b = rng.integers(0, 3, (R, C)).astype(np.uint8)
    else:
        a = rng.integers(0, 256, (R, C), dtype=np.uint8)
        b = np.roll(a, 2, 1) if kind == "shift" else rng.integers(0, 256, (R, C), dtype=np.uint8)
    ri0 = np.arange(R * C, dtype=np.int32).reshape(R, C)
    ri1 = ri0.copy()
    ri0[rng.random((R, C)) < 0.1] = -1
    ri1[rng.random((R, C)) < 0.1] = -1
    a[ri0 == -1] = 0
    b[ri1 == -1] = 0
    return a, b, ri0, ri1


@pytest.mark.parametrize("radius", [0, 1, 3])
@pytest.mark.parametrize("kind", ["equal", "coarse", "noise", "shift"])
def test_model_is_the_literal_form(radius, kind):
    rng = np.random.default_rng([radius, len(kind)])
    for R, C, (lo, hi) in ((12, 20, (-5, 4)), (7, 9, (-30, 30)), (1, 1, (0, 0)), (8, 2 * radius, (-3, 3)), (9, 13, (2, 2)),
                           (9, 13, (-4, -1))):
        if C == 0:
            continue
        w = window_case(rng, R, C, kind)
        got, want = sm.stereo(*w, radius, lo, hi), sm.literal_stereo(*w, radius, lo, hi)
        for name, g, x in zip(("disp", "cost", "cost2"), got, want):
            assert g.dtype == x.dtype and np.array_equal(g, x), (name, R, C, lo, hi)
        back = sm.stereo(w[1], w[0], w[3], w[2], radius, -hi, -lo)
        for d1 in (None, back[0]):
            for tol, uniq in ((0, 0), (1, 10), (2, 100)):
                assert np.array_equal(sm.keep(*got, d1, tol, uniq), sm.literal_keep(*got, d1, tol, uniq)), (R, C, tol, uniq)
    if kind == "equal" and radius == 1:  # every cost ties at 0: the smallest admissible d
        a, z = np.full((12, 20), 77, np.uint8), np.zeros((12, 20), np.int32)
        d, c, c2 = sm.stereo(a, a, z, z, 1, -5, 4)
        assert d[5, 10] == -5 and d[5, 3] == -2 and d[0, 0] == sm.NONE and c[5, 10] == 0 and c2[5, 10] == 0


def test_ties_reach_the_tie_rule():
    """Radius 0 on noise: hundreds of samples whose best and second-best cost are equal."""
    r0, r1, ri0, ri1, _, _ = plane(1)
    disp, cost, cost2 = sm.stereo(r0, r1, ri0, ri1, 0, -24, 8)
    assert int(((cost == cost2) & (disp != sm.NONE)).sum()) > 100


@functools.lru_cache(maxsize=None)
def plane(seed):
    return sm.plane_window(seed)


def test_plane_scene_meets_the_two_conditions():
    """wid 96, hgt 64, the plane z = 4 + 0.25 x, sf 1.2, cropped; r = 7, drange (-24, 8), both directions, lr_tol 1,
    uniqueness 10, seed 1: at least 0.9 of the samples with a disparity are kept, and every kept sample triangulates
    within 1.0 of the plane.  These are conditions on the inputs and the contract, not tolerances on a kernel.  With
    this renderer the model gives (kept share, largest distance) = (0.932, 0.728) for seed 1, (0.938, 1.0009) for
    seed 2 -- one sample past the second condition, so seed 2 is not a scene of the tests -- and (0.930, 0.726) for
    seed 3."""
    r0, r1, ri0, ri1, P0, P1 = plane(1)
    assert r0.shape == (68, 115)
    d0, c0, c20 = sm.stereo(r0, r1, ri0, ri1, 7, -24, 8)
    d1, _, _ = sm.stereo(r1, r0, ri1, ri0, 7, -8, 24)
    kept = sm.keep(d0, c0, c20, d1, 1, 10)
    x0, x1, rows = sm.matches(d0, kept, ri0, ri1, 96, 96)
    share, worst = sm.plane_conditions(d0, kept, x0, x1, P0, P1)
    print("kept share %.4f, largest distance from the plane %.4f" % (share, worst))
    assert share >= 0.9
    assert worst <= 1.0
    assert len(rows) == int(kept.sum()) > 4000


def test_flat_forms_are_the_windows():
    rng = np.random.default_rng(3)
    wins = [window_case(rng, R, C, "noise") for R, C in ((6, 9), (4, 7), (5, 5))]
    box = np.array([(2, 8, 1, 10), (0, 0, 3, 3), (1, 5, 0, 7), (0, 5, 2, 7)], np.int32)
    order = [0, None, 1, 2]
    flat = [np.concatenate([wins[k][j].ravel() for k in order if k is not None]) for j in range(4)]
    use = [1, 1, 0, 1]
    drange = [(-3, 3)] * 4
    disp, cost, cost2 = sm.stereo_batch(*flat, box, use, 1, drange)
    off = sm.out_offsets(box)
    assert off.tolist() == [0, 54, 54, 82, 107]
    assert (disp[54:82] == sm.NONE).all() and (cost[54:82] == 0xFFFF).all() and (cost2[54:82] == 0xFFFF).all()
    assert np.array_equal(sm.window(disp, 3, box, off), sm.stereo(*wins[2], 1, -3, 3)[0])
    sw = sm.stereo_batch(*flat, box, use, 1, drange, swap=1)
    assert np.array_equal(sm.window(sw[1], 0, box, off), sm.stereo(wins[0][1], wins[0][0], wins[0][3], wins[0][2], 1, -3, 3)[1])
    kept = sm.keep_batch(box, disp, cost, cost2, None, 1, 0)
    x0, x1, rows, pair_off = sm.matches_batch(box, [(9, 9), (7, 5)], [(0, 1)] * 4, disp, kept, flat[2], flat[3])
    assert pair_off[0] == 0 and pair_off[1] == pair_off[2] == pair_off[3] and pair_off[4] == len(rows) == int(kept.sum())
    assert pair_off[1] > 0 and pair_off[4] > pair_off[3]
    y, x = divmod(int(rows[0]), 9)
    s1 = int(wins[0][3][y, x + sm.window(disp, 0, box, off)[y, x]])
    assert x1[0].tolist() == [s1 % 7, s1 // 7, 1.] and x0[0].tolist() == [wins[0][2][y, x] % 9, wins[0][2][y, x] // 9, 1.]
