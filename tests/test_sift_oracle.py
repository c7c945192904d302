"""CPU checks of the SIFT oracle (tests/sift_oracle.py) and of the SIFT front-end's argument rules.

The oracle is anchored to vlfeat: on the reference's test image it reproduces vlfeat's recorded table
(tests/golden/sift_sur_ogre_table.npz) row for row, the reference's own allclose on the frames
(reference test/test_feature.py:33-47) and every descriptor value equal."""
import numpy as np
import pytest

from tests import sift_oracle as so
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
