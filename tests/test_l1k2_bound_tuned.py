"""The tuned rank-4 int8 table of the dim-128 L1 2-NN bound path (spectavi_amd/csrc/l1k2_bound_tuned.h, produced by
tools/l1k2_bound_tune.py), read through spv_l1k2_bound_table_of and checked on the CPU in int64 exactly as
tests/test_l1k2_bound_table.py checks the recipe: the inequality holds on every byte pair, m is attained, nothing can
leave int8 / int32, whole rows are bounded from below.  On top of that: it is tighter than the recipe on average, table
0 is the recipe, and the numpy model of the path (tests/l1k2_prune_model.py) gives the oracle's bytes with it while
fewer pairs survive."""
import ctypes as ct

import numpy as np
import pytest

from tests import l1k2_prune_model as pm
from tests.test_l1k2_bound_table import _table

RECIPE, TUNED = 0, 1


def table_of(which):
    from spectavi_amd._lib import clib
    phi = np.zeros((256, 4), np.int8)
    p, m = ct.c_int(0), ct.c_int(0)
    assert clib.spv_l1k2_bound_table_of(which, phi.ctypes.data, ct.byref(p), ct.byref(m)) == 0
    return phi.astype(np.int64), int(p.value), int(m.value)


def mean_bound(table):
    """Mean over all byte pairs of (m - G(a, b)) / p: the bound per dimension (the true mean of |a - b| is 85.33)."""
    phi, p, m = table
    return float((m - (phi @ phi.T).mean()) / p)


def test_table_0_is_the_recipe_and_1_is_not():
    for got, want in zip(table_of(RECIPE), _table()):
        assert np.array_equal(got, want)
    assert not np.array_equal(table_of(TUNED)[0], _table()[0])   # the tuned table passed its check and did not yield


def test_which_is_validated():
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    phi = np.zeros((256, 4), np.int8)
    p, m = ct.c_int(0), ct.c_int(0)
    for bad in (-1, 2):
        assert clib.spv_l1k2_bound_table_of(bad, phi.ctypes.data, ct.byref(p), ct.byref(m)) == SPV_ERR_INVALID
    assert clib.spv_l1k2_set_bound(2) == SPV_ERR_INVALID and clib.spv_l1k2_set_bound(-2) == SPV_ERR_INVALID


def test_setter_round_trip():
    from spectavi_amd import device
    before = device.l1k2_get_bound()
    try:
        for name, value in (("tuned", 1), ("recipe", 0), ("default", -1), (1, 1), (0, 0)):
            device.l1k2_set_bound(name)
            assert device.l1k2_get_bound() == value
        for bad in (2, "best", None, 1.0, True):
            with pytest.raises(ValueError):
                device.l1k2_set_bound(bad)
    finally:
        device.l1k2_set_bound(before)
    assert device.l1k2_get_bound() == before


def test_bound_holds_on_every_byte_pair_and_is_attained():
    phi, p, m = table_of(TUNED)
    a = np.arange(256, dtype=np.int64)
    G = phi @ phi.T
    slack = p * np.abs(a[:, None] - a[None, :]) - (m - G)
    assert slack.min() >= 0          # p |a-b| >= m - phi(a).phi(b) everywhere
    assert (slack == 0).any()        # and m is the minimum itself, not merely a bound


def test_ranges():
    phi, p, m = table_of(TUNED)
    G = phi @ phi.T
    assert np.abs(phi).max() <= 127
    assert 128 * int(np.abs(G).max()) < 2 ** 31
    assert p * 128 * 255 + 128 * abs(m) < 2 ** 31   # the lane threshold 128 m - p thr stays in int32


def test_rows_are_bounded_from_below():
    """p L1(x, y) >= 128 m - sum_d G(x_d, y_d) on random and on adversarial rows."""
    phi, p, m = table_of(TUNED)
    rng = np.random.default_rng(7)
    x = rng.integers(0, 256, (2000, 128))
    y = rng.integers(0, 256, (2000, 128))
    x[:50] = y[:50]
    x[50:60], y[50:60] = 0, 255
    l1 = np.abs(x - y).sum(axis=1)
    g = np.einsum("ndf,ndf->n", phi[x], phi[y])
    assert np.all(p * l1 >= 128 * m - g)


def test_mean_bound_is_above_the_recipe_s():
    recipe, tuned = mean_bound(table_of(RECIPE)), mean_bound(table_of(TUNED))
    print("mean bound per dimension: recipe %.3f, tuned %.3f (true mean 85.33)" % (recipe, tuned))
    assert tuned > recipe


@pytest.fixture(scope="module")
def uniform_case(oracle):
    """512 x 100 uniform bytes: with two wanted blocks, two slices of eight tiles each."""
    rng = np.random.default_rng(16)
    x = rng.integers(0, 256, (512, 128), dtype=np.uint8)
    y = rng.integers(0, 256, (100, 128), dtype=np.uint8)
    return x, y, oracle.nn_bruteforcel1k2(x, y)


@pytest.mark.parametrize("schedule", pm.SCHEDULES)
def test_model_with_the_tuned_table(uniform_case, schedule):
    """The oracle's bytes with either table, strictly fewer survivors with the tuned one (hand-over off, so that
    both runs put every pair to the bound)."""
    x, y, (oidx, odist) = uniform_case
    survivors = {}
    for which in (RECIPE, TUNED):
        idx, dist, stats = pm.run(x, y, table_of(which), 2, 1024, schedule)
        assert np.array_equal(idx[:len(y)], oidx) and np.array_equal(dist[:len(y)], odist), which
        assert bool((idx[len(y):] == pm.NONE).all())
        assert stats[0] == 512 * 256 and stats[2] == 0, stats
        survivors[which] = stats[1]
    print("%s: survivors recipe %d, tuned %d of %d" % (schedule, survivors[RECIPE], survivors[TUNED], 512 * 256))
    assert survivors[TUNED] < survivors[RECIPE]
