"""The rank-4 int8 minorant of |a - b| behind the dim-128 L1 2-NN bound path (l1k2_prune.hip), checked
on the CPU in int64: the table is the published recipe, the inequality holds on every byte pair, m is
attained, and nothing can leave int8 / int32."""
import ctypes as ct

import numpy as np


def _table():
    from spectavi_amd._lib import clib
    phi = np.zeros((256, 4), np.int8)
    p, m = ct.c_int(0), ct.c_int(0)
    assert clib.spv_l1k2_bound_table(phi.ctypes.data, ct.byref(p), ct.byref(m)) == 0
    return phi.astype(np.int64), int(p.value), int(m.value)


def test_table_is_the_recipe():
    phi, p, m = _table()
    a = np.arange(256, dtype=np.float64)
    want = np.stack([np.rint(127 * np.cos(np.pi * a / 255)), np.rint(127 * np.sin(np.pi * a / 255)),
                     np.rint(127 * np.cos(3 * np.pi * a / 255) / 3), np.rint(127 * np.sin(3 * np.pi * a / 255) / 3)],
                    axis=1).astype(np.int64)
    assert np.array_equal(phi, want)
    assert 100 <= p < 260


def test_bound_holds_on_every_byte_pair_and_is_attained():
    phi, p, m = _table()
    a = np.arange(256, dtype=np.int64)
    G = phi @ phi.T
    slack = p * np.abs(a[:, None] - a[None, :]) - (m - G)
    assert slack.min() >= 0          # p |a-b| >= m - phi(a).phi(b) everywhere
    assert (slack == 0).any()        # and m is the minimum itself, not merely a bound


def test_ranges():
    phi, p, m = _table()
    G = phi @ phi.T
    assert np.abs(phi).max() <= 127
    assert 128 * int(np.abs(G).max()) < 2 ** 31
    assert p * 128 * 255 + 128 * abs(m) < 2 ** 31   # the lane threshold 128 m - p thr stays in int32


def test_rows_are_bounded_from_below():
    """p L1(x, y) >= 128 m - sum_d G(x_d, y_d) on random and on adversarial rows."""
    phi, p, m = _table()
    rng = np.random.default_rng(7)
    x = rng.integers(0, 256, (2000, 128))
    y = rng.integers(0, 256, (2000, 128))
    x[:50] = y[:50]
    x[50:60], y[50:60] = 0, 255
    l1 = np.abs(x - y).sum(axis=1)
    g = np.einsum("ndf,ndf->n", phi[x], phi[y])
    assert np.all(p * l1 >= 128 * m - g)
