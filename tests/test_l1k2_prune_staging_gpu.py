"""The direct-to-LDS staging of the dim-128 bound path of the L1 2-NN (l1k2_prune.hip), prune forced on,
bit for bit against the CPU oracle, at the two places where it differs from staging through registers.

Clamped tail rows.  The loads into LDS run with every lane on, so the rows past the end of a ragged last
tile are copies of the database's last row where they used to be zeros.  The last row is planted as the
nearest neighbour of some queries (so its copies pass the bound for them), once with a byte-identical copy
of it in an earlier tile and once without: with the copy the last row and its phantoms sit exactly at the
queries' threshold, without it a phantom that got through would be the second neighbour.  Default knobs:
slices of 64 rows, so 33 and 63 rows are one slice with a tail of 1 and 31 rows, 161 rows two full slices
and one of 33.

Swizzle.  The feature tile lies in LDS unpadded, piece j of row r in slot j ^ (r & 15), and is read back
through the same XOR.  One workgroup and one slice of one, two and three tiles (no prefetch, one, and the
first buffer used again), on rows whose every 4-byte group (one 16-byte feature piece) is different: near
rows, which the bound must keep, and rows that are the near pattern with its groups permuted by an XOR,
which it must rule out and which look near exactly when slots are mixed up.  Results must be the oracle's
and (bounded, survived) the numpy model's (tests/l1k2_prune_model.py), exactly: with one workgroup and one
slice no timing is involved, so a bound loosened by a wrong operand shows even where the results stay
right.  One slice of three tiles needs SPECTAVI_L1K2_BLOCKS=1, which the library reads once per process:
the three shapes run in one child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # run as the child of test_swizzle_one_slice_in_a_child_process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import l1k2_prune_cases as pc  # noqa: E402
from tests import l1k2_prune_model as pm  # noqa: E402
from tests.test_l1k2_bound_table import _table  # noqa: E402
from tests.test_l1k2_prune_gpu import _run  # noqa: E402

TAIL_XROWS = (33, 63, 32 * 5 + 1)
TAIL_YROWS = (1, 257)
COPY_ROW = 7
SWIZZLE_XROWS = (32, 64, 96)
SWIZZLE_YROWS = 200
CHILD_ENV = {"SPECTAVI_L1K2_BLOCKS": "1"}
CHILD_TIMEOUT = 120


def tail_case(xrows, yrows, with_copy):
    """(x, y, planted queries): uniform bytes; the planted queries are the last row, a few bytes one off."""
    rng = np.random.default_rng([xrows, yrows, int(with_copy)])
    x = rng.integers(0, 256, (xrows, 128), dtype=np.uint8)
    y = rng.integers(0, 256, (yrows, 128), dtype=np.uint8)
    x[-1] = np.clip(x[-1], 1, 254)
    if with_copy:
        x[COPY_ROW] = x[-1]
    planted = sorted({0, yrows // 2, yrows - 1})
    for n, k in enumerate(planted):
        y[k] = x[-1]
        y[k, 5 * n:5 * n + 3] += 1
    return x, y, planted


def swizzle_case(xrows, yrows=SWIZZLE_YROWS):
    """(x, y).  P: a pattern whose 32 groups of 4 bytes take 32 values 7 apart, in a seeded order.  Queries
    and near rows are P with noise seeded per row; row r of the others is P with group j holding group
    j ^ k of it, k = 1 + r % 31, and noise.  Two near rows head the slice, every other row after them is near."""
    rng = np.random.default_rng(20)
    groups = 16 + 7 * rng.permutation(32)

    def rows(n, perm_of_row):
        out = np.empty((n, 128), np.int16)
        for r in range(n):
            out[r] = np.repeat(groups[np.arange(32) ^ perm_of_row(r)], 4)
            out[r] += rng.integers(-2, 3, 128)
        return out.astype(np.uint8)

    near = (np.arange(xrows) % 2 == 0) | (np.arange(xrows) < 2)
    x = rows(xrows, lambda r: 0 if near[r] else 1 + r % 31)
    y = rows(yrows, lambda r: 0)
    assert len({x[r, 16 * j:16 * j + 16].tobytes() for r in range(xrows) for j in range(8)}) == 8 * xrows
    return x, y


def mixed_up(table, x, y):
    """The model's precomputation with the feature pieces of row r read from slot j ^ (r & 15): what a
    swizzle applied on one side only computes."""
    dist, _, ysum = pm.prepare(x, y, table)
    fx = pm.features(table, x).reshape(len(x), 32, 16)
    slot = np.arange(32)[None, :] ^ (np.arange(len(x)) & 15)[:, None]
    fx = np.take_along_axis(fx, slot[:, :, None], axis=1).reshape(len(x), 512)
    return dist, fx @ pm.features(table, y).T, ysum


def test_swizzle_model_numbers_are_fixed_and_have_teeth():
    """CPU only.  One slice: the model's statistics are the same under every schedule and from run to run,
    it gives a share strictly between none and all from the second tile on, and mixing the slots up moves it."""
    table = _table()
    for xrows in SWIZZLE_XROWS:
        x, y = swizzle_case(xrows)
        assert pc.plan_of(xrows, len(y), 1)[0] == 1
        stats = {s: pm.run(x, y, table, 1, pc.BREAK_EVEN_SHARE, s)[2] for s in pm.SCHEDULES}
        again = pm.run(*swizzle_case(xrows), table, 1, pc.BREAK_EVEN_SHARE, "up")[2]
        assert len(set(stats.values())) == 1 and again == stats["up"], (xrows, stats, again)
        bounded, survived, fallback = stats["up"]
        assert bounded == xrows * 256 and fallback == 0
        wrong = pm.run(x, y, table, 1, pc.BREAK_EVEN_SHARE, "up", pre=mixed_up(table, x, y))[2]
        if xrows == 32:     # a first tile has no threshold yet: everything survives, whatever the operand
            assert survived == bounded == wrong[1]
        else:
            near = 32 * 256 + (xrows - 32) // 2 * 256
            assert survived == near, (xrows, stats)      # tile 0, then exactly the near rows
            assert wrong[1] != survived, (xrows, wrong)


@pytest.mark.gpu
@pytest.mark.parametrize("with_copy", [True, False], ids=["copy", "nocopy"])
@pytest.mark.parametrize("yrows", TAIL_YROWS)
@pytest.mark.parametrize("xrows", TAIL_XROWS)
def test_clamped_tail_rows(oracle, xrows, yrows, with_copy):
    from spectavi_amd import device
    plan = device.l1k2_plan(xrows, yrows, 128)
    assert (plan["slices"], plan["slice_rows"]) == (-(-xrows // 64), 64), plan
    x, y, planted = tail_case(xrows, yrows, with_copy)
    oidx, odist = oracle.nn_bruteforcel1k2(x, y)
    idx, dist, stats = _run(x, y, 1)
    print("tail %d x %d copy %d: statistics %r" % (xrows, yrows, with_copy, stats))
    assert stats[0] > 0 and stats[2] == 0, stats          # the bound kernel ran and kept its slices
    assert (idx < xrows).all(), idx[(idx >= xrows).any(axis=1)][:4]
    assert ((idx == xrows - 1).sum(axis=1) <= 1).all()
    assert np.array_equal(idx, oidx) and np.array_equal(dist, odist)
    assert idx.tobytes() == np.ascontiguousarray(oidx).view(np.uint64).tobytes() and dist.tobytes() == odist.tobytes()
    for k in planted:
        if with_copy:
            assert tuple(int(v) for v in idx[k]) == (COPY_ROW, xrows - 1) and dist[k, 0] == dist[k, 1] == 3
        else:
            assert int(idx[k, 0]) == xrows - 1 and dist[k, 0] == 3 and dist[k, 1] > 3


def run_swizzle(oracle_fn):
    """In a process with CHILD_ENV: the three shapes, each against the oracle and the model."""
    from spectavi_amd import device
    table = _table()
    for xrows in SWIZZLE_XROWS:
        x, y = swizzle_case(xrows)
        plan = device.l1k2_plan(xrows, len(y), 128)
        assert plan["slices"] == 1 and plan["slice_rows"] >= xrows, plan
        oidx, odist = oracle_fn(x, y)
        want = pm.run(x, y, table, 1, pc.BREAK_EVEN_SHARE, "up")[2]
        for attempt in range(2):
            idx, dist, stats = _run(x, y, 1)
            print("swizzle %d x %d run %d: statistics %r, the model's %r" % (xrows, len(y), attempt, stats, want), flush=True)
            assert np.array_equal(idx, oidx) and np.array_equal(dist, odist), "results differ from the oracle"
            assert tuple(stats) == tuple(want), "statistics differ from the model"
        off_idx, off_dist, off_stats = _run(x, y, 0)
        assert np.array_equal(off_idx, oidx) and np.array_equal(off_dist, odist) and off_stats == (0, 0, 0)


@pytest.mark.gpu
def test_swizzle_one_slice_in_a_child_process():
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPECTAVI_L1K2_")}
    env.update(CHILD_ENV)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    print(r.stdout)
    assert r.returncode == 0 and "swizzle ok: %d shapes" % len(SWIZZLE_XROWS) in r.stdout, r.stdout


if __name__ == "__main__":
    from oracle import oracle as _oracle
    run_swizzle(_oracle.nn_bruteforcel1k2)
    print("swizzle ok: %d shapes" % len(SWIZZLE_XROWS))
