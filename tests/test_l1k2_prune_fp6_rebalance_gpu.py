"""l1k2_prune_wide6_kernel arms a tile's accumulators in the tile's own top, no longer at the end of the compare of the tile
before.  That changes no decision, so every case here is compared bit for bit with the CPU oracle and, with one slice, its
survivor statistics exactly with tests/l1k2_prune_fp6_model.py, through the checks of tests/test_l1k2_prune_fp6_gpu.py
(check_data, check_case: the FP6 form forced on for the call).  The cases are the smallest at which the move could go wrong
(tests/l1k2_prune_fp6_rebalance_cases.py has the recipes and checks on the CPU that each does what it is named for):

  * one 64-row tile alone, armed once at tile 0; two and three tiles, ragged in either row half;
  * a second best that tile t's drain lowers so that rows of tile t + 1 kept under the old threshold are ruled out under the
    new one, t odd and even, all eight waves: an arming that reads a stale k2s[] shows as survivors above the model's;
  * three and four slices of 4 to 5 tiles with inherited thresholds (publication at tiles 0, 2, 4); their survivors depend
    on timing, so the oracle and the plan are what is checked;
  * the share rule fired at tiles 3 and 4 by one wave of either half: the workgroup leaves with the next tile's loads in
    flight and armed or not, and the tile kernel finishes the slice;
  * the lowering and ragged cases with the end-of-tile pass by lanes only (octet_max 0).

Settings are SPECTAVI_L1K2_* variables that the library reads once per process: one fresh child per setting runs all of its
cases and stops at the first that fails.  A child that ends by a signal, an abort or the time limit fails its test and makes
the rest of this module skip: nothing more is started on the GPU from here."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # run as the child of test_setting_in_a_child_process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import l1k2_prune_fp6_rebalance_cases as rc  # noqa: E402
from tests import test_l1k2_prune_fp6_gpu as fp6  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120
TILE = rc.TILE
SETTINGS = ("one", "three", "four", "octet0")   # of tests/test_l1k2_prune_fp6_gpu.SETTINGS
# slices of 4 and 5 tiles, the last one ragged: setting -> ((database rows, queries), ...); up to 256 queries are one query
# block of the plan, which then cuts as many slices as the setting names
SLICED = {"three": ((3 * 5 * TILE - 63, 200), (3 * 4 * TILE - 1, 256)), "four": ((4 * 4 * TILE - 31, 256), (4 * 5 * TILE - 1, 130))}
_gpu_lost = []   # why nothing more may be started on the GPU from this module


def check_lowering(setting, oracle_fn):
    from spectavi_amd import device
    table = device.l1k2_bound6_table()
    for t in rc.LOWERING:
        x, y, _ = rc.lowering(table, t)
        fp6.check_data("lowering-tile%d" % t, setting, x, y, oracle_fn, slices_wanted=1)


def check_leaving(oracle_fn):
    from spectavi_amd import device
    table = device.l1k2_bound6_table()
    for wave, tile in rc.LEAVING:
        x, y, _ = rc.leaving(table, wave, tile)
        stats, want = fp6.check_data("leaving-wave%d-tile%d" % (wave, tile), "one", x, y, oracle_fn, slices_wanted=1)
        if not (want[0] == (tile + 1) * TILE * 512 and want[2] == len(x) * 512):
            raise fp6.CaseFailed("leaving-wave%d-tile%d: the model does not leave at tile %d: %r" % (wave, tile, tile, want))


def check_sliced(setting, oracle_fn):
    slices = {"three": 3, "four": 4}[setting]
    for xrows, yrows in SLICED[setting]:
        rng = np.random.default_rng([xrows, yrows, slices])
        # clustered rows, as check_four of tests/test_l1k2_prune_fp6_gpu.py: thresholds fall and pass from slice to slice
        x = rng.integers(0, 256, (xrows, 128), dtype=np.uint8)
        y = x[rng.integers(0, xrows, yrows)].copy()
        y[np.arange(yrows), rng.integers(0, 128, yrows)] ^= 1
        y[::7] = rng.integers(0, 256, (len(y[::7]), 128), dtype=np.uint8)
        fp6.check_data("sliced-%dx%d" % (xrows, yrows), setting, x, y, oracle_fn, slices_wanted=slices)


def run_setting(setting, oracle_fn):
    """Everything of one setting; returns the number of checks made."""
    if setting in SLICED:
        check_sliced(setting, oracle_fn)
        return len(SLICED[setting])
    shapes = rc.shape_cases()
    if setting == "octet0":
        shapes = shapes[1::2]         # a ragged row half 0 and a ragged row half 1
    for c in shapes:
        fp6.check_case(c, oracle_fn, setting)
    check_lowering(setting, oracle_fn)
    if setting == "one":
        check_leaving(oracle_fn)
    return len(shapes) + len(rc.LOWERING) + (len(rc.LEAVING) if setting == "one" else 0)


@pytest.mark.parametrize("setting", SETTINGS)
def test_setting_in_a_child_process(setting):
    if _gpu_lost:
        pytest.skip("nothing more is started on the GPU from this module: %s" % _gpu_lost[0])
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPECTAVI_L1K2_")}
    env.update(fp6.SETTINGS[setting])
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), setting]
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _gpu_lost.append("the child of setting %r ran into its time limit" % setting)
        pytest.fail("%s\n%s" % (_gpu_lost[0], e.stdout))
    print(r.stdout)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _gpu_lost.append("the child of setting %r ended with status %d" % (setting, r.returncode))
        pytest.fail("%s\n%s" % (_gpu_lost[0], r.stdout))
    assert r.returncode == 0 and ("all ok: %s," % setting) in r.stdout, r.stdout


if __name__ == "__main__":
    from oracle import oracle as _oracle
    try:
        _n = run_setting(sys.argv[1], _oracle.nn_bruteforcel1k2)
    except fp6.CaseFailed as e:
        print("FAILED %s" % e, flush=True)
        sys.exit(1)
    print("all ok: %s, %d checks" % (sys.argv[1], _n))
