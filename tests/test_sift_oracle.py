"""CPU checks of the SIFT oracle (tests/sift_oracle.py) and of the SIFT front-end's argument rules.

The oracle is anchored to vlfeat: on the reference's test image it reproduces vlfeat's recorded table
(tests/golden/sift_sur_ogre_table.npz) row for row, the reference's own allclose on the frames
(reference test/test_feature.py:33-47) and every descriptor value equal."""
import numpy as np
import pytest

from tests import sift_oracle as so
from tests import sift_cases as sc
from tests.sift_cases import orientation_counts, smooth_random, sur_ogre


@pytest.fixture(scope="module")
def ogre():
    im, golden = sur_ogre()
    return im, golden, so.sift(im)


def test_oracle_matches_vlfeat_rows(ogre):
    _, golden, table = ogre
    assert table.shape == golden.shape == (1168, 132)
    assert np.allclose(table[:, :4], golden[:, :4])
    assert np.array_equal(table[:, 4:], golden[:, 4:])


def test_oracle_golden_has_four_orientations(ogre):
    _, _, table = ogre
    assert orientation_counts(table).max() == 4


def test_oracle_constant_image_has_no_rows():
    assert so.sift(np.full((40, 50), 7, np.float32)).shape == (0, 132)


def test_oracle_octave_count():
    assert so.noctaves(310, 233) == 5
    assert so.noctaves(15, 12) == 1
    assert so.noctaves(1, 1) == 1
    assert so.noctaves(64, 64) == 4


def test_oracle_descriptor_values_are_quantised():
    t = so.sift(smooth_random(1, 64, 64))
    d = t[:, 4:]
    assert len(t) > 0 and np.all(d == np.floor(d)) and d.min() >= 0 and d.max() <= 255


def test_fast_sqrt_and_atan2_match_references():
    x = np.array([0, 1e-9, 2e-8, 2.0, 1e4], np.float32)
    r = so.fast_sqrt(x)
    assert r[0] == 0 and r[1] == 0
    assert np.allclose(r[2:], np.sqrt(x[2:]), rtol=1e-5)
    y, xx = np.float32([1, -1, 0.5, -2]), np.float32([1, 1, -3, -0.25])
    assert np.allclose(so.fast_atan2(y, xx), np.arctan2(y, xx), atol=1e-2)


def test_taps_are_symmetric_and_normalised():
    for sigma in (1.2489995996796797, 1.2262735, 3.0897):
        W, t = so.gauss_taps(sigma)
        assert len(t) == 2 * W + 1 and np.array_equal(t, t[::-1])
        assert abs(float(t.astype(np.float64).sum()) - 1) < 1e-6


# ---- the case table of tests/sift_cases.py is not vacuous: every case reaches what it was chosen for ----
def detection(im):
    """Yields (o, L [6, h, w], D [5, h, w], [(report, refined or None) per candidate in scan order])."""
    for o, L in so.octaves(np.ascontiguousarray(im, np.float32)):
        h, w = L.shape[1:]
        D = L[1:] - L[:-1]
        out = []
        for s, y, x in zip(*so.extrema(D)):
            rep = {}
            out.append((rep, so.refine(D, int(s), int(x), int(y), w, h, report=rep)))
        yield o, L, D, out


def first_row_exists(im):
    """The first keypoint that has an orientation: the table has a row."""
    grads = {}
    for o, L, (kx, ky, ks), si in so.keypoints(np.ascontiguousarray(im, np.float32)):
        if (o, si) not in grads:
            grads[(o, si)] = so.gradient(L[si + 1])
        if so.orientations(*grads[(o, si)], kx, ky, ks, o):
            return True
    return False


@pytest.mark.parametrize("name", [n for n in sc.CASE_NAMES if n not in sc.NO_ROWS])
def test_case_gives_rows(name):
    assert first_row_exists(sc.case_image(name))


@pytest.mark.parametrize("name", sorted(sc.NO_ROWS))
def test_case_gives_no_rows(name):
    """The one-pixel-wide images have no octave with a DoG interior (the path that skips detection); the
    three-pixel-wide ones have one (6 rows in octave -1), candidates or not, and still no row."""
    im = sc.case_image(name)
    assert so.sift(im).shape == (0, 132)
    shapes = [L.shape[1:] for _, L in so.octaves(im)]
    assert len(shapes) == 1
    assert (min(shapes[0]) < 3) == name.startswith("no-interior"), shapes


@pytest.mark.parametrize("name", sc.SMALL_RANGE)
def test_small_range_cases_reach_the_zero_branch_of_fast_sqrt(name):
    """Pixels of the gradient levels with 0 < gx^2 + gy^2 < 1e-8: fast_sqrt returns 0 for them."""
    n = 0
    for _, L in so.octaves(sc.case_image(name)):
        for s in range(3):
            gx, gy = so.gradient_xy(L[s + 1])
            m2 = (gx * gx + gy * gy).astype(np.float64)
            n += int(((m2 > 0) & (m2 < 1e-8)).sum())
    assert n > 0


def test_plain_range_does_not_reach_the_zero_branch():
    """The contrast: on sur-ogre as it is (0..255) only exactly flat pixels take that branch."""
    for _, L in so.octaves(sur_ogre()[0]):
        for s in range(3):
            gx, gy = so.gradient_xy(L[s + 1])
            m2 = (gx * gx + gy * gy).astype(np.float64)
            assert not ((m2 > 0) & (m2 < 1e-8)).any()


def dog_ties(D):
    """(values of the scan region equal to one of their 26 neighbours, values exactly 0)."""
    _, h, w = D.shape
    c = D[1:4, 1:h - 1, 1:w - 1]
    tie = np.zeros(c.shape, bool)
    for ds in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if not ds == dy == dx == 0:
                    tie |= c == D[1 + ds:4 + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    return int(tie.sum()), int((c == 0).sum())


@pytest.mark.parametrize("name", sc.PLATEAU)
def test_plateau_cases_hold_dog_ties_or_zeros(name):
    ties = zeros = 0
    for _, L in so.octaves(sc.case_image(name)):
        t, z = dog_ties(L[1:] - L[:-1])
        ties, zeros = ties + t, zeros + z
    print("%s: %d DoG values equal a neighbour, %d are exactly 0" % (name, ties, zeros))
    assert ties > 0 or zeros > 0


def extrema_with_ties(D):
    """so.extrema with the neighbour comparisons made non-strict: what a wrong tie rule would accept."""
    _, h, w = D.shape
    c = D[1:4, 1:h - 1, 1:w - 1]
    gt, lt = c >= 0, c <= 0
    for ds in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if not ds == dy == dx == 0:
                    n = D[1 + ds:4 + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                    gt &= c >= n
                    lt &= c <= n
    return np.nonzero(gt | lt)


@pytest.mark.parametrize("name", ["ogre-stretch-clip", "ogre-4-levels", "castle-01", "castle-02"])
def test_plateau_cases_tell_a_wrong_tie_rule(name):
    """On the saturated and few-level images the ties sit on plateau tops: a non-strict neighbour rule
    finds candidates that the strict one refuses, so a kernel with the wrong rule gives another table (the
    full tables differ in their row counts: 1126 / 1123, 1209 / 1056, 1101 / 976, 1164 / 1035).  The two noise
    images hold ties too, but none at an extremum."""
    strict = loose = 0
    for _, L in so.octaves(sc.case_image(name)):
        D = L[1:] - L[:-1]
        strict += len(so.extrema(D)[0])
        loose += len(extrema_with_ties(D)[0])
    print("%s: %d candidates, %d with a non-strict rule" % (name, strict, loose))
    assert loose > strict


def test_small_range_table_depends_on_the_zero_branch(monkeypatch):
    """sur-ogre x 1e-3 through the oracle with and without fast_sqrt's x < 1e-8 -> 0 branch: rows differ
    (142 of 1169), so a kernel without the branch fails the case."""
    im = sc.case_image("ogre*1e-3")
    want = so.sift(im)
    monkeypatch.setattr(so, "fast_sqrt", lambda x: (np.asarray(x, np.float32) * so.fast_resqrt(x)).astype(np.float32))
    got = so.sift(im)
    assert got.shape == want.shape and (got != want).any(1).sum() > 0


def test_negative_cases_hold_negative_pixels():
    assert (sc.case_image("-ogre") < 0).all()
    im = sc.case_image("ogre-128")
    assert (im < 0).any() and (im > 0).any()


@pytest.mark.parametrize("name", sorted(sc.THIN))
def test_thin_cases_reach_the_far_end_of_the_candidate_packing(name):
    """A keypoint of octave -1 whose octave coordinate along the long side exceeds 8191 (more than 13 bits
    of the 15-bit field), and a keypoint within 4 px of the far end of the image."""
    h, w = sc.THIN[name]
    axis, side = (0, w) if w > h else (1, h)
    far = [k[axis] for o, _, k, _ in so.keypoints(sc.case_image(name)) if o == -1]
    assert len(far) > 0 and 2 * max(far) > 8191
    assert max(far) > side - 1 - 4


@pytest.fixture(scope="module")
def structure_reports():
    return {name: [c for _, _, _, cands in detection(sc.case_image(name)) for c in cands] for name in sc.STRUCTURE}


def test_structure_cases_reach_edge_rejection_and_refinement_moves(structure_reports):
    edge = {n: sum(1 for rep, r in c if r is None and rep["edge"]) for n, c in structure_reports.items()}
    moved = {n: sum(1 for rep, _ in c if rep["moved"]) for n, c in structure_reports.items()}
    kept_moved = {n: sum(1 for rep, r in c if rep["moved"] and r is not None) for n, c in structure_reports.items()}
    print("rejected by the edge score %s, moved %s, moved and kept %s" % (edge, moved, kept_moved))
    assert sum(edge.values()) > 0 and sum(moved.values()) > 0
    # the step edge is what the score is there for
    assert edge["edge-corner"] > 0


def test_a_case_has_a_keypoint_with_four_orientations():
    im = sc.case_image("-ogre")
    grads = {}
    for o, L, (kx, ky, ks), si in so.keypoints(im):
        if (o, si) not in grads:
            grads[(o, si)] = so.gradient(L[si + 1])
        if len(so.orientations(*grads[(o, si)], kx, ky, ks, o)) == 4:
            return
    pytest.fail("no keypoint of -ogre has four orientations")


def test_seam_cases_give_the_octave_widths_they_were_chosen_for():
    for w, widths in sc.SEAM_OCTAVE_WIDTHS.items():
        shapes = [L.shape[1:] for _, L in so.octaves(sc.case_image("seam-%dx%d" % (sc.SEAM_HEIGHT, w)))]
        assert tuple(s[1] for s in shapes) == widths, (w, shapes)
    seams = {ow for widths in sc.SEAM_OCTAVE_WIDTHS.values() for ow in widths}
    # 256 columns per block: one block, exactly full, one over; 64 columns per wave step from column 1
    assert {255, 256, 257, 258, 510, 512, 514} <= seams
    assert {64 * k + 2 + d for k in (1, 2, 4, 8) for d in (-2, 0)} <= seams   # the last step full: w - 2 = 64 k
    assert {33, 63, 65, 127, 129, 255, 257} <= set(sc.SEAM_OCTAVE_WIDTHS)     # odd sizes: wid >> o floors


def test_min_side_cases_step_the_octave_count():
    for (h, w), n in sc.OCTAVE_STEP_SHAPES.items():
        im = sc.case_image("min-side-%dx%d" % (h, w))
        assert im.shape == (h, w) and len(list(so.octaves(im))) == n == so.noctaves(w, h)
    assert sorted(set(sc.OCTAVE_STEP_SHAPES.values())) == [1, 2, 3]


def test_blobs_are_found_where_they_are_by_the_oracle():
    """The check of tests/test_sift_classes_gpu.py that leans on no oracle, held to the oracle itself."""
    sc.assert_blobs_found(so.sift(sc.case_image("blobs")), "oracle")


# ---- front-end rules that need no GPU -------------------------------------------------------------
def test_sift_filter_rejects_non_2d():
    from spectavi_amd import feature
    for bad in (np.zeros(5, np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(TypeError):
            feature.sift_filter(bad)
        with pytest.raises(TypeError):
            feature.sift_filter_batch([bad])
        with pytest.raises(TypeError):
            feature.sift_filter_striped(bad)


def test_sift_workspace_bytes_rules():
    from spectavi_amd._lib import clib
    f = clib.spv_sift_workspace_bytes
    assert f(0, 10) == 0 and f(10, -1) == 0 and f(8193, 10) == 0
    assert f(310, 233) > 4 * 620 * 466 * 6
    assert f(8192, 8192) > 0


def test_device_expn_table_is_the_host_exp():
    """sift.hip carries vlfeat's fast_expn table as constant data: every entry must be the C library's
    exp(-k * 25/256), the oracle's table."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "spectavi_amd", "csrc", "sift.hip")).read()
    body = re.search(r"kExpn\[257\] = \{(.*?)\};", src, re.S).group(1)
    vals = [float.fromhex(t) for t in body.replace("\n", " ").split(",") if t.strip()]
    assert len(vals) == 257
    assert np.array_equal(np.array(vals), so.EXPN_TAB)
