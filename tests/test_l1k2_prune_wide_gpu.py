"""The wide form of the bound kernel (l1k2_prune_wide_kernel: 64-row tiles, 512-query workgroups) forced on through
spv_l1k2_set_prune(1) and spv_l1k2_set_prune_form(1), with both bound tables, on every case of
tests/l1k2_prune_wide_cases.py: bit for bit against the CPU oracle, against the tile kernel (mode 0) and against the
narrow form, and with the statistics of tests/l1k2_prune_wide_model.py where a single slice makes them independent of
timing (workgroups have queries of their own, so one slice is all it takes).

The settings other than "default" need SPECTAVI_L1K2_BLOCKS / SPECTAVI_L1K2_PRUNE_SHARE, which the library reads once
per process: one fresh child per setting runs all of its cases and stops at the first that fails.  A child that ends
by a signal, an abort or the time limit fails its test and makes the rest of this module skip: nothing more is
started on the GPU from here."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # run as the child of test_setting_in_a_child_process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import l1k2_prune_cases as pc  # noqa: E402
from tests import l1k2_prune_wide_cases as wc  # noqa: E402
from tests import l1k2_prune_wide_model as wm  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120
NARROW, WIDE = 0, 1
_gpu_lost = []   # why nothing more may be started on the GPU from this module


class CaseFailed(AssertionError):
    pass


def _run(x, y, mode, form, bound):
    """(idx, dist, (bounded, survivors, fallback pairs)) with mode, form and table set for this call only."""
    import torch
    from spectavi_amd import device
    before = device.l1k2_get_prune(), device.l1k2_get_prune_form(), device.l1k2_get_bound()
    device.l1k2_set_prune(mode)
    device.l1k2_set_prune_form(form)
    device.l1k2_set_bound(bound)
    try:
        idx, dist = device.l1k2(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
        stats = device.l1k2_prune_stats()
        return idx.cpu().numpy().view(np.uint64), dist.cpu().numpy(), stats
    finally:
        device.l1k2_set_prune(before[0])
        device.l1k2_set_prune_form(before[1])
        device.l1k2_set_bound(before[2])


def check_case(c, oracle_fn):
    from spectavi_amd import device
    slices, slice_rows, tiles, groups = wc.plan(c)
    got = device.l1k2_plan(c.xrows, c.yrows, 128)
    if (got["slices"], got["slice_rows"]) != (slices, slice_rows):
        raise CaseFailed("%s: plan %r, the case needs %d slices of %d rows" % (c.id, got, slices, slice_rows))
    tables = {which: device.l1k2_bound_table(which) for which in (0, 1)}
    x, y, expect = wc.make_case(c, tables[0])
    oidx, odist = oracle_fn(x, y)
    problems = []

    def compare(name, idx, dist):
        bad = np.flatnonzero((idx != oidx).any(axis=1) | (dist != odist).any(axis=1))
        if len(bad):
            k = int(bad[0])
            problems.append("%s: %d of %d queries differ from the oracle, first query %d: got idx %s dist %s, want idx %s dist %s" % (
                name, len(bad), len(oidx), k, idx[k].tolist(), dist[k].tolist(), oidx[k].tolist(), odist[k].tolist()))

    off_idx, off_dist, off_stats = _run(x, y, 0, WIDE, -1)
    compare("tile kernel", off_idx, off_dist)
    if off_stats != (0, 0, 0):
        problems.append("statistics with prune off %r" % (off_stats,))
    seen = {}
    for which in (0, 1):
        pre = wm.prepare(x, y, tables[which])
        want = wm.run(x, y, tables[which], pc.blocks_of(c.setting), pc.share_of(c.setting), "up", pre)[2]
        for form in (WIDE, NARROW):
            idx, dist, stats = _run(x, y, 1, form, which)
            name = "%s form, table %d" % ("wide" if form == WIDE else "narrow", which)
            compare(name, idx, dist)
            if idx.tobytes() != off_idx.tobytes() or dist.tobytes() != off_dist.tobytes():
                problems.append("%s: bytes differ from the tile kernel's" % name)
            if not 0 < stats[1] <= stats[0]:
                problems.append("%s did not go through the bound kernel: %r" % (name, stats))
            seen[name] = stats
            if form != WIDE:
                continue
            if stats[0] % (64 * 8) or stats[2] % 512:
                problems.append("%s: statistics %r are not those of 512-query workgroups" % (name, stats))
            if slices == 1 and stats != want:
                problems.append("%s: statistics %r, the model's %r" % (name, stats, want))
            if c.kind == "constant" and pc.share_of(c.setting) != 1024 and stats[2] != c.xrows * 512 * groups:
                problems.append("%s: fallback %d, every workgroup leaves every slice: %d" % (name, stats[2], c.xrows * 512 * groups))
            for k, rows in expect.items():
                if tuple(int(v) for v in idx[k]) != rows:
                    problems.append("%s, query %d: got rows %s, planted %s" % (name, k, idx[k].tolist(), rows))
    if problems:
        raise CaseFailed("%s (slices %d, wide tiles %s):\n  %s" % (c.id, slices, tiles, "\n  ".join(problems)))
    print("ok %s slices %d wide tiles %s %s" % (c.id, slices, "/".join(map(str, tiles)), seen["wide form, table 0"]), flush=True)


def _skip_if_gpu_lost():
    if _gpu_lost:
        pytest.skip("nothing more is started on the GPU from this module: %s" % _gpu_lost[0])


@pytest.mark.parametrize("setting", sorted({c.setting for c in wc.CASES} - {"default"}))
def test_setting_in_a_child_process(setting):
    _skip_if_gpu_lost()
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPECTAVI_L1K2_")}
    env.update(pc.SETTINGS[setting])
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
    assert r.returncode == 0 and ("all ok: %s, %d cases" % (setting, len(wc.cases_of(setting)))) in r.stdout, r.stdout


@pytest.mark.parametrize("case", wc.cases_of("default"), ids=lambda c: c.id)
def test_several_one_tile_slices_in_this_process(oracle, case):
    _skip_if_gpu_lost()
    check_case(case, oracle.nn_bruteforcel1k2)


def test_auto_chooses_the_form_by_the_plan():
    """Host only: where `auto` takes the path and the wide grid fills the chip it is the wide form; below that, and
    wherever the path is forced (what the case tables of the narrow kernel run under), the narrow one."""
    from spectavi_amd import device
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    before = device.l1k2_get_prune(), device.l1k2_get_prune_form()
    try:
        device.l1k2_set_prune("auto")
        device.l1k2_set_prune_form("default")
        assert device.l1k2_prune_form_of(1 << 20, 1 << 20) == WIDE
        assert device.l1k2_prune_form_of(4000000, 500000) == WIDE
        assert device.l1k2_prune_form_of(262144, 262144) == -1          # the tile kernel: no form at all
        device.l1k2_set_prune(1)
        assert device.l1k2_prune_form_of(1 << 20, 1 << 20) == NARROW
        assert device.l1k2_prune_form_of(262144, 262144) == NARROW
        device.l1k2_set_prune_form("wide")
        assert device.l1k2_prune_form_of(262144, 262144) == WIDE and device.l1k2_prune_form_of(40, 3) == WIDE
        device.l1k2_set_prune("auto")
        device.l1k2_set_prune_form("narrow")
        assert device.l1k2_prune_form_of(1 << 20, 1 << 20) == NARROW
        assert clib.spv_l1k2_set_prune_form(2) == SPV_ERR_INVALID and clib.spv_l1k2_set_prune_form(-2) == SPV_ERR_INVALID
        for bad in (7, "big", None, 1.0, True):
            with pytest.raises(ValueError):
                device.l1k2_set_prune_form(bad)
        assert device.l1k2_get_prune_form() == NARROW
    finally:
        device.l1k2_set_prune(before[0])
        device.l1k2_set_prune_form(before[1])


if __name__ == "__main__":
    from oracle import oracle as _oracle
    try:
        for _c in wc.cases_of(sys.argv[1]):
            check_case(_c, _oracle.nn_bruteforcel1k2)
    except CaseFailed as e:
        print("FAILED %s" % e, flush=True)
        sys.exit(1)
    print("all ok: %s, %d cases" % (sys.argv[1], len(wc.cases_of(sys.argv[1]))))
