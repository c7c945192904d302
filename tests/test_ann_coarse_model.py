"""The float64 coarse-stage model of tests/ann_coarse_model.py on its own, no GPU: that its rules decide
nearly every query of the data sets they are used on, that rintf of the column means is unambiguous
there, and that the check passes a correct selection and fails two wrong ones -- which is what shows
that the GPU test of tests/test_ann_variants_gpu.py can fail."""
import numpy as np
import pytest

from tests import ann_cases as ac
from tests import ann_coarse_model as cm

UNDECIDED_CAP = 0.05     # share of queries that may have an open row


def test_bf16_rounding_on_known_bits():
    a = np.array([0x3F800000, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000,
                  0x00000000, 0x80000000, 0x437F0000, 0x477FFFFF], np.uint32).view(np.float32)
    want = np.array([0x3F800000, 0x3F800000, 0x3F820000, 0x3F800000, 0x3F810000, 0xBF800000, 0xBF820000,
                     0x00000000, 0x80000000, 0x437F0000, 0x47800000], np.uint32)
    assert np.array_equal(cm.bf16_rne(a).view(np.uint32), want)
    assert np.array_equal(cm.bf16_trunc(a).view(np.uint32), a.view(np.uint32) & np.uint32(0xFFFF0000))
    ints = np.arange(-256, 257, dtype=np.float32)          # what the exact domain rests on
    assert np.array_equal(cm.bf16_rne(ints), ints)


def test_rules_on_a_hand_made_query():
    s = np.array([[0.0, 1.0, 2.0, 2.5, 10.0, 11.0]])
    eps = np.full_like(s, 0.5)                              # margin 1
    must, must_not = cm.rules(s, eps, 3)                    # tau = 2
    assert must.tolist() == [[True, False, False, False, False, False]]
    assert must_not.tolist() == [[False, False, False, False, True, True]]
    assert cm.open_rows(must, must_not, 3).tolist() == [3]  # rows 1, 2, 3 for two places
    assert not cm.violations(must, must_not, np.array([[0, 1, 3]]))[0]
    assert cm.violations(must, must_not, np.array([[1, 2, 3]]))[0]      # a MUST row lost
    assert cm.violations(must, must_not, np.array([[0, 1, 4]]))[0]      # a MUST NOT row kept
    assert cm.violations(must, must_not, np.array([[0, 1, 1]]))[0]      # a row twice
    assert cm.violations(must, must_not, np.array([[0, 1, 6]]))[0]      # no row
    must, must_not = cm.rules(s, eps, 4)                    # tau = 2.5: rows 2 and 3 fill the two places left
    assert cm.open_rows(must, must_not, 4).tolist() == [0]


@pytest.mark.parametrize("name", ac.MODEL_SETS)
def test_means(name):
    x, _ = ac.property_rows(name)
    assert x.shape == (2000, 64) and cm.means_are_unambiguous(x)
    if name == "scaled":
        sd, mean = x.astype(np.float64).std(0), cm.column_means(x)
        assert sd.min() < 1e-2 and sd.max() > 100 and np.abs(mean).max() > 9e3


@pytest.mark.parametrize("ncand", ac.MODEL_NCAND)
@pytest.mark.parametrize("name", ac.MODEL_SETS)
def test_undecided_cap(name, ncand):
    must, must_not = ac.model_rules(name, ncand)
    free = cm.open_rows(must, must_not, ncand)
    share = (free > 0).mean()
    print("ann coarse model: %s 2000x300x64 ncand=%d: %d open rows, %d of %d queries have one"
          % (name, ncand, int(free.sum()), int((free > 0).sum()), free.size))
    assert share <= UNDECIDED_CAP
    assert (must.sum(1) <= ncand - 1).all() and ((~must_not).sum(1) >= ncand).all()


def violating(name, ncand, idx):
    return int(cm.violations(*ac.model_rules(name, ncand), idx).sum())


@pytest.mark.parametrize("ncand", ac.MODEL_NCAND)
@pytest.mark.parametrize("name", ac.MODEL_SETS)
def test_sensitivity_float32_arithmetic_passes(name, ncand):
    x, y = ac.property_rows(name)
    assert violating(name, ncand, cm.select(cm.float32_scores(*cm.images(x, y)), ncand)) == 0
    assert violating(name, ncand, cm.select(ac.model_case(name)[0], ncand)) == 0


@pytest.mark.parametrize("ncand", ac.MODEL_NCAND)
@pytest.mark.parametrize("name", ac.MODEL_SETS)
def test_sensitivity_truncation_fails(name, ncand):
    x, y = ac.property_rows(name)
    n = violating(name, ncand, cm.select(cm.float32_scores(*cm.images(x, y, rounding=cm.bf16_trunc)), ncand))
    print("ann coarse model: %s ncand=%d: bf16 by truncation breaks a rule in %d of %d queries" % (name, ncand, n, len(y)))
    assert n > 0


@pytest.mark.parametrize("ncand", ac.MODEL_NCAND)
def test_sensitivity_uncentred_queries_fail(ncand):
    x, y = ac.property_rows("offset")
    n = violating("offset", ncand, cm.select(cm.float32_scores(*cm.images(x, y, centre_y=False)), ncand))
    print("ann coarse model: offset ncand=%d: y left uncentred breaks a rule in %d of %d queries" % (ncand, n, len(y)))
    assert n == len(y)
