"""The dim-128 bound path of the L1 2-NN (l1k2_prune.hip) at its slice, tile and tie edges: every case of
tests/l1k2_prune_cases.py, prune forced on (twice) and off, bit for bit against the CPU oracle, after
the plan of the case (slices, tiles of every slice, live rows of the last tile) has been asserted through
device.l1k2_plan(), and with the statistics the table pins.

The settings other than "default" need SPECTAVI_L1K2_BLOCKS / SPECTAVI_L1K2_PRUNE_SHARE, which the
library reads once per process: one fresh child per setting runs all of its cases and stops at the first
that fails.  A child that ends by a signal, an abort or the time limit fails its test and makes the rest
of this module skip: nothing more is started on the GPU from here.

The tight-tie case ("two-4096x40-tight"): a correct kernel passes under every interleaving of the two
slices.  A kernel that skips a pair on equality (128 m - sum >= p thr) fails whenever slice 1, which
begins with tight rows, has published the tight distance before slice 0 reaches the tight rows in its
last two of 64 tiles; slice 1 publishes at its tile 4 and both start together, so that is the normal
order.  The power of the test depends on timing, its verdict on a correct kernel does not."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

if __name__ == "__main__":   # run as the child of test_setting_in_a_child_process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import l1k2_prune_cases as pc  # noqa: E402
from tests.test_l1k2_bound_table import _table  # noqa: E402
from tests.test_l1k2_prune_gpu import _run  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120
_gpu_lost = []   # why nothing more may be started on the GPU from this module


class CaseFailed(AssertionError):
    pass


def assert_plan(c):
    from spectavi_amd import device
    plan = device.l1k2_plan(c.xrows, c.yrows, 128)
    got = (plan["slices"], pc.shape_of(c.xrows, plan["slices"], plan["slice_rows"]))
    if got != (c.slices, (c.tiles, c.last_rows)):
        raise CaseFailed("%s: plan %r gives (slices, (tiles, last rows)) = %r, the case needs %r"
                         % (c.id, plan, got, (c.slices, (c.tiles, c.last_rows))))


def _first_difference(name, idx, dist, oidx, odist):
    bad = np.flatnonzero((idx != oidx).any(axis=1) | (dist != odist).any(axis=1))
    if not len(bad):
        return None
    k = int(bad[0])
    return "%s: %d of %d queries differ, first query %d: got idx %s dist %s, want idx %s dist %s" % (
        name, len(bad), len(oidx), k, idx[k].tolist(), dist[k].tolist(), oidx[k].tolist(), odist[k].tolist())


def check_case(c, oracle_fn, table):
    """Returns the statistics of the forced run; raises CaseFailed with the first differing query."""
    x, y, expect = pc.make_case(c, table)
    oidx, odist = oracle_fn(x, y)
    on_idx, on_dist, on_stats = _run(x, y, 1)
    again_idx, again_dist, again_stats = _run(x, y, 1)
    off_idx, off_dist, off_stats = _run(x, y, 0)
    problems = [_first_difference("prune on", on_idx, on_dist, oidx, odist),
                _first_difference("prune on, second run", again_idx, again_dist, oidx, odist),
                _first_difference("prune off", off_idx, off_dist, oidx, odist)]
    for k, rows in expect.items():
        if tuple(int(v) for v in on_idx[k]) != rows:
            problems.append("query %d: got rows %s, planted %s" % (k, on_idx[k].tolist(), rows))
    for name, stats in (("first", on_stats), ("second", again_stats)):
        if not all(e is None or e == g for e, g in zip(c.stats, stats)):
            problems.append("statistics of the %s forced run %r, the case pins %r" % (name, stats, c.stats))
        if c.path and not 0 < stats[1] <= stats[0]:
            problems.append("the %s forced run did not go through the bound kernel: %r" % (name, stats))
    if off_stats != (0, 0, 0):
        problems.append("statistics with prune off %r" % (off_stats,))
    problems = [p for p in problems if p]
    if problems:
        raise CaseFailed("%s (slices %d, tiles %s, last rows %d; statistics on %r / %r, off %r):\n  %s" % (
            c.id, c.slices, c.tiles, c.last_rows, on_stats, again_stats, off_stats, "\n  ".join(problems)))
    return on_stats


def run_case(c, oracle_fn, table):
    t0 = time.perf_counter()
    stats = check_case(c, oracle_fn, table)
    print("ok %s slices %d tiles %s last rows %d bounded %d survivors %d fallback %d (%.2f s)" % (
        (c.id, c.slices, "/".join(map(str, c.tiles)), c.last_rows) + stats + (time.perf_counter() - t0,)), flush=True)


def run_setting(setting, oracle_fn):
    """All cases of a setting, in this process: the plans first, then case by case to the first failure."""
    table = _table()
    cases = pc.cases_of(setting)
    for c in cases:
        assert_plan(c)
    for c in cases:
        run_case(c, oracle_fn, table)


def _skip_if_gpu_lost():
    if _gpu_lost:
        pytest.skip("nothing more is started on the GPU from this module: %s" % _gpu_lost[0])


@pytest.mark.parametrize("setting", [s for s in pc.SETTINGS if s != "default"])
def test_setting_in_a_child_process(setting):
    _skip_if_gpu_lost()
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPECTAVI_L1K2_")}
    env.update(pc.SETTINGS[setting])
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), setting]
    t0 = time.perf_counter()
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _gpu_lost.append("the child of setting %r ran into its time limit" % setting)
        pytest.fail("%s\n%s" % (_gpu_lost[0], e.stdout))
    print(r.stdout)
    print("setting %s: %.1f s in its child process" % (setting, time.perf_counter() - t0))
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _gpu_lost.append("the child of setting %r ended with status %d" % (setting, r.returncode))
        pytest.fail("%s\n%s" % (_gpu_lost[0], r.stdout))
    assert r.returncode == 0 and ("all ok: %s, %d cases" % (setting, len(pc.cases_of(setting)))) in r.stdout, r.stdout


@pytest.fixture(scope="module")
def table():
    return _table()


@pytest.mark.parametrize("case", pc.cases_of("default"), ids=lambda c: c.id)
def test_one_tile_slices_in_this_process(oracle, table, case):
    """Query tails against slices of a single tile, a last slice of one row, and a shape below the path
    (31 rows: statistics (0, 0, 0) with prune forced)."""
    _skip_if_gpu_lost()
    assert_plan(case)
    run_case(case, oracle.nn_bruteforcel1k2, table)


if __name__ == "__main__":
    from oracle import oracle as _oracle
    try:
        run_setting(sys.argv[1], _oracle.nn_bruteforcel1k2)
    except CaseFailed as e:
        print("FAILED %s" % e, flush=True)
        sys.exit(1)
    print("all ok: %s, %d cases" % (sys.argv[1], len(pc.cases_of(sys.argv[1]))))
