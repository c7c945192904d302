"""CPU only: the case table of the bound path (tests/l1k2_prune_cases.py) has teeth.  Nobody can mutate
the kernel on a GPU in review, so the plain numpy model of what the path decides
(tests/l1k2_prune_model.py) stands in for it: unmutated it gives the oracle's bytes on every case under
every schedule, and every named mutant of it is told apart from the oracle by at least one case.  The
plans the table claims are checked against the library itself, one child process per setting (the
library reads SPECTAVI_L1K2_BLOCKS once)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import l1k2_prune_cases as pc
from tests import l1k2_prune_model as pm
from tests.test_l1k2_bound_table import _table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH_CASES = [c for c in pc.CASES if c.path]


@pytest.fixture(scope="module")
def table():
    return _table()


@pytest.fixture(scope="module")
def prepared(oracle, table):
    """case id -> (x, y, expect, oracle idx, oracle dist, model precomputation), computed once."""
    out = {}
    for c in PATH_CASES:
        x, y, expect = pc.make_case(c, table)
        oidx, odist = oracle.nn_bruteforcel1k2(x, y)
        out[c.id] = (x, y, expect, oidx, odist, pm.prepare(x, y, table))
    return out


def _model(c, prepared, table, schedule, mutant=None):
    x, y, _, oidx, odist, pre = prepared[c.id]
    idx, dist, stats = pm.run(x, y, table, pc.blocks_of(c.setting), pc.share_of(c.setting), schedule, mutant, pre)
    n = len(y)
    same = np.array_equal(idx[:n], oidx) and np.array_equal(dist[:n], odist) and bool((idx[n:] == pm.NONE).all())
    return same, stats


def test_the_table_contains_what_it_is_for():
    """By the plans, not by comment."""
    one = [c for c in pc.CASES if c.slices == 1 and c.path]
    assert {c.tiles[0] for c in one} >= set(range(1, 10)) | {12, 13}
    for kind in ("cluster", "zeroq"):
        assert {c.last_rows for c in one if c.kind == kind and c.tiles[0] > 1} >= set(pc.RAGGED), kind
    for tiles in (5, 1):
        assert {c.yrows for c in pc.CASES if set(c.tiles) == {tiles} and c.path} >= set(pc.QUERY_TAILS), tiles
    # two and three slices of 3, 4, 5, 8 tiles: only a last slice can have an odd count (l1k2_prune_cases.SLICE_UNIT)
    assert {c.tiles for c in pc.CASES} >= {(4, 3), (4, 4), (6, 5), (8, 8), (4, 4, 3), (4, 4, 4), (6, 6, 5), (8, 8, 8)}
    last = {(c.tiles[-1], c.last_rows) for c in pc.CASES if c.slices > 1}
    assert (1, 1) in last and (1, 32) in last             # a last slice of one row, and of one full tile
    full = [c for c in pc.CASES if pc.share_of(c.setting) == 1024]
    assert any(c.tiles[0] > 8 and c.stats[0] == c.stats[1] > 0 and c.stats[2] == 0 for c in full)
    assert any(c.kind == "tight" and c.slices == 2 and min(c.tiles) >= 64 for c in pc.CASES)
    assert any((c.arg or {}).get("ties") and c.stats[2] for c in pc.CASES)
    assert any(not c.path and c.stats == (0, 0, 0) for c in pc.CASES)
    assert len(pc.SETTINGS) - 1 <= 4                      # child processes of the GPU test


@pytest.mark.parametrize("setting", sorted(pc.SETTINGS))
def test_plans_are_the_library_s(setting):
    """spv_l1k2_plan, in a process that has the setting's environment, gives every case the slices the
    table claims (host only: no device is touched)."""
    code = ("import ctypes as ct, json, sys; sys.path.insert(0, %r)\n"
            "from spectavi_amd._lib import clib\n"
            "out = []\n"
            "for xr, yr in json.loads(sys.argv[1]):\n"
            "    o = (ct.c_int * 5)(); assert clib.spv_l1k2_plan(xr, yr, 128, o) == 0; out.append(list(o))\n"
            "print(json.dumps(out))\n" % ROOT)
    cases = pc.cases_of(setting)
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPECTAVI_L1K2_")}
    env.update(pc.SETTINGS[setting])
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code, json.dumps([(c.xrows, c.yrows) for c in cases])]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for c, (dim_pad, q, slices, slice_rows, wide) in zip(cases, json.loads(r.stdout.splitlines()[-1])):
        assert (dim_pad, wide) == (128, 0), c.id
        assert (slices, pc.shape_of(c.xrows, slices, slice_rows)) == (c.slices, (c.tiles, c.last_rows)), c.id


def test_model_gives_the_oracle_s_bytes_on_every_case(prepared, table):
    """(a) under every schedule; the statistics the table pins are the model's under every schedule,
    which is what "does not depend on timing" means here; and the neighbours the recipes plant are the
    oracle's."""
    for c in PATH_CASES:
        _, _, expect, oidx, _, _ = prepared[c.id]
        for k, rows in expect.items():
            assert tuple(int(v) for v in oidx[k]) == rows, (c.id, k)
        for schedule in pm.SCHEDULES:
            same, stats = _model(c, prepared, table, schedule)
            assert same, (c.id, schedule)
            assert all(e is None or e == g for e, g in zip(c.stats, stats)), (c.id, schedule, c.stats, stats)


def test_every_mutant_is_caught(prepared, table):
    """(b) each named mutant differs from the oracle on at least one case under at least one schedule;
    the catching cases are printed (pytest -s, and profiles/r12_l1k2_prune_shapes.txt)."""
    missed = []
    for mutant, what in pm.MUTANTS.items():
        caught = ["%s/%s" % (c.id, s) for c in PATH_CASES for s in pm.SCHEDULES if not _model(c, prepared, table, s, mutant)[0]]
        print("mutant %-20s (%s): %d catches%s" % (mutant, what, len(caught), ": " + ", ".join(caught[:4]) if caught else ""))
        if mutant in pm.INERT:
            # not a gap in the table: see l1k2_prune_model.INERT.  Were it ever to change a result, that would be news.
            assert not caught, (mutant, caught)
        elif not caught:
            missed.append(mutant)
    assert not missed, "no case tells these mutants from the oracle: %s" % missed
