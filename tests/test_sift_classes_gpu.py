"""SIFT on the GPU over the named case table of tests/sift_cases.py: image classes (value range and sign,
ties and plateaus, structure) and shapes (thin images up to the 8192 limit, block and wave seams, steps of
the octave count) that the fixed images of tests/test_sift_gpu.py never reach.

Bar, as there: the same rows in the same order, x, y, sigma, angle and descriptors bit-equal to the numpy
oracle (ulp=0).  tests/test_sift_oracle.py shows on the CPU that each case reaches the branch it was
chosen for.  The blob test leans on no oracle: it knows where the keypoints must be."""
import numpy as np
import pytest

from tests import sift_oracle as so
from tests.sift_cases import CASE_NAMES, NO_ROWS, assert_blobs_found, assert_tables_match, case_image

pytestmark = pytest.mark.gpu

# Cases that need the contract's one float32 ulp on a frame value (the device's pow / sin / cos against the
# C library's): none.  An entry here names the case, and its comment the column and row.
ULP1 = {}
assert len(ULP1) * 10 <= len(CASE_NAMES)

_oracle = {}


def oracle_table(name):
    """so.sift of a case, computed once per module run."""
    if name not in _oracle:
        _oracle[name] = so.sift(case_image(name))
    return _oracle[name]


@pytest.fixture(scope="module")
def feature():
    from spectavi_amd import feature
    return feature


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_matches_oracle(feature, name):
    im = case_image(name)
    want = oracle_table(name)
    got = feature.sift_filter(im)
    print("%s: %d x %d, %d rows (oracle %d)" % (name, im.shape[0], im.shape[1], len(got), len(want)))
    if name in NO_ROWS:
        assert want.shape == (0, 132) and got.shape == (0, 132) and got.dtype == np.float32
    else:
        assert len(want) > 0
    assert_tables_match(got, want, name, ulp=ULP1.get(name, 0))


def test_blobs_are_found_where_they_are(feature):
    assert_blobs_found(feature.sift_filter(case_image("blobs")), "gpu")
