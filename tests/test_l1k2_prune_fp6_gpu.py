"""The FP6 form of the wide bound kernel (l1k2_prune_wide6_kernel: 40 scaled FP6 MFMAs per 64-row tile over the rank-5 e2m3
table) forced on through spv_l1k2_set_prune(1), spv_l1k2_set_prune_form(1) and spv_l1k2_set_prune_matrix(1): every case bit
for bit against the CPU oracle, and against the statistics of tests/l1k2_prune_fp6_model.py where a single slice makes them
independent of timing.  The cases are those of tests/l1k2_prune_wide_cases.py, built from the FP6 table's own tight pairs
(ragged tiles in either row half at even and odd tiles, the query counts, two and three slices, the planted survivor
counts with two survivors in one lane, duplicates and ties, a pair on the threshold, workgroups that leave, all 4096
surviving), and what is added here: four slices, bytes in [0, 128) with one and with two query blocks on the work list,
the end-of-tile pass with one pair per lane only, the feature rows themselves, and the default selection.

Settings other than "default" need SPECTAVI_L1K2_* variables that the library reads once per process: one fresh child per
setting runs all of its cases and stops at the first that fails.  A child that ends by a signal, an abort or the time limit
fails its test and makes the rest of this module skip: nothing more is started on the GPU from here."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # run as the child of test_setting_in_a_child_process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import l1k2_prune_cases as pc  # noqa: E402
from tests import l1k2_prune_fp6_model as fm  # noqa: E402
from tests import l1k2_prune_wide_cases as wc  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120
WIDE, I8, FP6 = 1, 0, 1
TILE = wc.TILE
# the environment of a child: the settings of tests/l1k2_prune_cases.py, four slices, and the drains by lanes only
SETTINGS = dict(pc.SETTINGS)
SETTINGS["four"] = {"SPECTAVI_L1K2_BLOCKS": "4"}
SETTINGS["octet0"] = {"SPECTAVI_L1K2_BLOCKS": "1", "SPECTAVI_L1K2_PRUNE_OCTET": "0"}
BLOCKS = {name: int(env.get("SPECTAVI_L1K2_BLOCKS", 16384)) for name, env in SETTINGS.items()}
SHARE = {name: int(env.get("SPECTAVI_L1K2_PRUNE_SHARE", pc.BREAK_EVEN_SHARE)) for name, env in SETTINGS.items()}
# four slices of 2 .. 5 tiles (the last one ragged): (database rows, queries); up to 256 queries make one query block of the plan
FOUR = ((4 * 2 * TILE, 200), (4 * 3 * TILE - 31, 255), (4 * 4 * TILE - 63, 65), (4 * 5 * TILE - 1, 256))
# bytes in [0, 128): (database rows, queries); 200 queries list one query block of 256 when the workgroup leaves, 300 two
LEAVING = ((10 * TILE + 5, 200), (10 * TILE + 5, 300))
# the feature rows: (database rows, queries); a database of fewer than 32 rows has no bound path, the single row is a query's
FEATURE_ROWS = ((63, 1), (64, 63), (65, 65), (64, 64))
_gpu_lost = []   # why nothing more may be started on the GPU from this module


class CaseFailed(AssertionError):
    pass


def _run(x, y, mode=1, form=WIDE, matrix=FP6, workspace=None):
    """(idx, dist, (bounded, survivors, fallback pairs)) with mode, form and matrix format set for this call only."""
    import torch
    from spectavi_amd import device
    before = device.l1k2_get_prune(), device.l1k2_get_prune_form(), device.l1k2_get_prune_matrix(), device.l1k2_get_bound()
    device.l1k2_set_prune(mode)
    device.l1k2_set_prune_form(form)
    device.l1k2_set_prune_matrix(matrix)
    device.l1k2_set_bound("default")
    try:
        idx, dist = device.l1k2(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), workspace=workspace)
        stats = device.l1k2_prune_stats()
        return idx.cpu().numpy().view(np.uint64), dist.cpu().numpy(), stats
    finally:
        device.l1k2_set_prune(before[0])
        device.l1k2_set_prune_form(before[1])
        device.l1k2_set_prune_matrix(before[2])
        device.l1k2_set_bound(before[3])


def check_data(name, setting, x, y, oracle_fn, expect=None, slices_wanted=None):
    """One FP6 run of (x, y) against the oracle and, with one slice, the model's statistics; returns (got, model's)."""
    from spectavi_amd import device
    table = device.l1k2_bound6_table()
    slices, slice_rows, _ = pc.plan_of(len(x), len(y), BLOCKS[setting])
    got = device.l1k2_plan(len(x), len(y), 128)
    if (got["slices"], got["slice_rows"]) != (slices, slice_rows) or slices_wanted not in (None, slices):
        raise CaseFailed("%s: plan %r, the case needs %s slices (%d of %d rows by the model)" % (name, got, slices_wanted, slices, slice_rows))
    oidx, odist = oracle_fn(x, y)
    want = fm.run(x, y, table, BLOCKS[setting], SHARE[setting])[2]
    idx, dist, stats = _run(x, y)
    problems = []
    bad = np.flatnonzero((idx != oidx).any(axis=1) | (dist != odist).any(axis=1))
    if len(bad):
        k = int(bad[0])
        problems.append("%d of %d queries differ from the oracle, first query %d: got idx %s dist %s, want idx %s dist %s" % (
            len(bad), len(oidx), k, idx[k].tolist(), dist[k].tolist(), oidx[k].tolist(), odist[k].tolist()))
    if idx.tobytes() != oidx.tobytes() or dist.tobytes() != odist.tobytes():
        problems.append("bytes differ from the oracle's")
    if not 0 < stats[1] <= stats[0]:
        problems.append("did not go through the bound kernel: %r" % (stats,))
    if stats[0] % (64 * 8) or stats[2] % 512:
        problems.append("statistics %r are not those of 512-query workgroups" % (stats,))
    if slices == 1 and stats != want:
        problems.append("statistics %r, the model's %r" % (stats, want))
    for k, rows in (expect or {}).items():
        if tuple(int(v) for v in idx[k]) != rows:
            problems.append("query %d: got rows %s, planted %s" % (k, idx[k].tolist(), rows))
    if problems:
        raise CaseFailed("%s (slices %d):\n  %s" % (name, slices, "\n  ".join(problems)))
    print("ok %s slices %d %s" % (name, slices, stats), flush=True)
    return stats, want


def check_case(c, oracle_fn, setting=None):
    from spectavi_amd import device
    x, y, expect = wc.make_case(c, device.l1k2_bound6_table())
    stats, _ = check_data(c.id, setting or c.setting, x, y, oracle_fn, expect)
    groups = wc.plan(c)[3]
    if c.kind == "constant" and SHARE[setting or c.setting] != 1024 and stats[2] != c.xrows * 512 * groups:
        raise CaseFailed("%s: fallback %d, every workgroup leaves every slice: %d" % (c.id, stats[2], c.xrows * 512 * groups))


def check_four(oracle_fn):
    for xrows, yrows in FOUR:
        rng = np.random.default_rng([xrows, yrows, 4])
        # clustered rows: queries near a few database rows, so that thresholds fall and are handed from slice to slice
        x = rng.integers(0, 256, (xrows, 128), dtype=np.uint8)
        y = x[rng.integers(0, xrows, yrows)].copy()
        y[np.arange(yrows), rng.integers(0, 128, yrows)] ^= 1
        y[::7] = rng.integers(0, 256, (len(y[::7]), 128), dtype=np.uint8)
        check_data("four-%dx%d" % (xrows, yrows), "four", x, y, oracle_fn, slices_wanted=4)


def check_leaving(oracle_fn):
    """Bytes in [0, 128): the bound rules little out, the workgroup leaves at the tile the model names, and the exact kernel
    computes the slice for the one or two query blocks of 256 that hold a query."""
    for xrows, yrows in LEAVING:
        rng = np.random.default_rng([xrows, yrows, 128])
        x = rng.integers(0, 128, (xrows, 128), dtype=np.uint8)
        y = rng.integers(0, 128, (yrows, 128), dtype=np.uint8)
        stats, want = check_data("leaving-%dx%d" % (xrows, yrows), "one", x, y, oracle_fn, slices_wanted=1)
        # by the model it left, and before its last tile: fewer tiles were bounded than the slice has, and the whole slice
        # went to the exact kernel (counted for the workgroup's 512 query slots)
        if not (want[2] == xrows * 512 and 0 < want[0] < (xrows // TILE) * TILE * 512 and want[0] % (TILE * 512) == 0):
            raise CaseFailed("leaving-%dx%d: the model does not leave early: %r" % (xrows, yrows, want))
        print("ok leaving after %d tiles" % (want[0] // (TILE * 512)), flush=True)


def check_feature_rows(oracle_fn):
    """The feature rows in the workspace after a run, against the model's packing, and the run itself."""
    import torch
    from spectavi_amd import device
    k = device.l1k2_bound6_table()[0]
    for xrows, yrows in FEATURE_ROWS:
        rng = np.random.default_rng([xrows, yrows, 6])
        x = rng.integers(0, 256, (xrows, 128), dtype=np.uint8)
        y = rng.integers(0, 256, (yrows, 128), dtype=np.uint8)
        x[0], x[-1], y[-1] = 0, 255, np.arange(128) * 2 + 1
        ws = device.Workspace()
        idx, dist, stats = _run(x, y, workspace=ws)
        oidx, odist = oracle_fn(x, y)
        if idx.tobytes() != oidx.tobytes() or dist.tobytes() != odist.tobytes() or not stats[0]:
            raise CaseFailed("features %dx%d: the run itself differs from the oracle (%r)" % (xrows, yrows, stats))
        torch.cuda.synchronize()
        raw = ws.get(0, torch.device("cuda", torch.cuda.current_device())).cpu().numpy()
        off_x, off_y = fm.feature_offsets(xrows, yrows, device.l1k2_plan(xrows, yrows, 128)["slices"])
        for name, off, rows in (("database", off_x, x), ("query", off_y, y)):
            got = raw[off:off + 512 * len(rows)].reshape(len(rows), 512)
            want = fm.pack_rows(rows, k)
            if not np.array_equal(got, want):
                r = int(np.flatnonzero((got != want).any(axis=1))[0])
                raise CaseFailed("features %dx%d: %s row %d differs from the model's packing at bytes %s" % (
                    xrows, yrows, name, r, np.flatnonzero(got[r] != want[r])[:8].tolist()))
        print("ok features %dx%d" % (xrows, yrows), flush=True)


def run_setting(setting, oracle_fn):
    """Everything of one setting; returns the number of checks made."""
    if setting == "four":
        check_four(oracle_fn)
        return len(FOUR)
    if setting == "octet0":   # the end-of-tile pass with one pair per lane: few survivors, many, ties and a ragged tile
        picked = [c for c in wc.cases_of("one") if c.kind in ("planted", "ties", "second") or c.xrows in (65, 3 * TILE + 31)]
        for c in picked:
            check_case(c, oracle_fn, "octet0")
        return len(picked)
    for c in wc.cases_of(setting):
        check_case(c, oracle_fn)
    n = len(wc.cases_of(setting))
    if setting == "one":
        check_leaving(oracle_fn)
        check_feature_rows(oracle_fn)
        n += len(LEAVING) + len(FEATURE_ROWS)
    return n


def _skip_if_gpu_lost():
    if _gpu_lost:
        pytest.skip("nothing more is started on the GPU from this module: %s" % _gpu_lost[0])


@pytest.mark.parametrize("setting", sorted(set(SETTINGS) - {"default"}))
def test_setting_in_a_child_process(setting):
    _skip_if_gpu_lost()
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPECTAVI_L1K2_")}
    env.update(SETTINGS[setting])
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


@pytest.mark.parametrize("case", wc.cases_of("default"), ids=lambda c: c.id)
def test_several_one_tile_slices_in_this_process(oracle, case):
    _skip_if_gpu_lost()
    check_case(case, oracle.nn_bruteforcel1k2)


def test_the_default_selection_runs_fp6_where_auto_takes_the_wide_form():
    """The smallest shape at which `auto` takes the wide form, found through spv_l1k2_prune_form_of.  It is far too large
    for the CPU oracle in a test (over 10^11 pairs), so the plan's choice is asserted through spv_l1k2_prune_matrix_of, and
    the run under the default selection is compared with the int8 kernel's and the tile kernel's on the same data."""
    _skip_if_gpu_lost()
    from spectavi_amd import device
    before = device.l1k2_get_prune(), device.l1k2_get_prune_form(), device.l1k2_get_prune_matrix(), device.l1k2_get_bound()
    try:
        for setter in (device.l1k2_set_prune, device.l1k2_set_prune_form, device.l1k2_set_prune_matrix, device.l1k2_set_bound):
            setter(-1)
        shapes = [(x, y) for x in range(1 << 18, (1 << 20) + 1, 1 << 16) for y in range(1 << 16, (1 << 20) + 1, 1 << 16)
                  if device.l1k2_prune_form_of(x, y) == WIDE]
        assert shapes
        xrows, yrows = min(shapes, key=lambda s: (s[0] * s[1], s[0]))
        assert device.l1k2_prune_matrix_of(xrows, yrows) == FP6
        assert device.l1k2_prune_matrix_of(1 << 20, 1 << 20) == FP6
    finally:
        for setter, value in zip((device.l1k2_set_prune, device.l1k2_set_prune_form, device.l1k2_set_prune_matrix, device.l1k2_set_bound), before):
            setter(value)
    rng = np.random.default_rng(20)
    x = rng.integers(0, 256, (xrows, 128), dtype=np.uint8)
    y = rng.integers(0, 256, (yrows, 128), dtype=np.uint8)
    idx6, dist6, stats6 = _run(x, y, mode=-1, form=-1, matrix=-1)
    idx8, dist8, stats8 = _run(x, y, mode=-1, form=-1, matrix=I8)
    idx0, dist0, stats0 = _run(x, y, mode=0, form=-1, matrix=-1)
    print("default selection at %d x %d: FP6 %r, int8 %r" % (xrows, yrows, stats6, stats8))
    assert stats0 == (0, 0, 0) and 0 < stats6[1] < stats6[0] and 0 < stats8[1] < stats8[0]   # both went through a bound kernel
    assert idx6.tobytes() == idx0.tobytes() and dist6.tobytes() == dist0.tobytes()
    assert idx8.tobytes() == idx0.tobytes() and dist8.tobytes() == dist0.tobytes()


if __name__ == "__main__":
    from oracle import oracle as _oracle
    try:
        _n = run_setting(sys.argv[1], _oracle.nn_bruteforcel1k2)
    except CaseFailed as e:
        print("FAILED %s" % e, flush=True)
        sys.exit(1)
    print("all ok: %s, %d checks" % (sys.argv[1], _n))
