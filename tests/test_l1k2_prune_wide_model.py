"""CPU only: the numpy statement of the wide form of the bound kernel (tests/l1k2_prune_wide_model.py) gives the
oracle's bytes on every case of tests/l1k2_prune_wide_cases.py under every schedule, its statistics on the
one-slice cases do not depend on the schedule (the GPU test compares the kernel's with them), and the cases
contain what they are for: by their plans and by the model's survivor counts, not by comment."""
import numpy as np
import pytest

from tests import l1k2_prune_cases as pc
from tests import l1k2_prune_wide_cases as wc
from tests import l1k2_prune_wide_model as wm
from tests.test_l1k2_bound_table import _table


@pytest.fixture(scope="module")
def table():
    return _table()


@pytest.fixture(scope="module")
def prepared(oracle, table):
    """case id -> (x, y, expect, oracle idx, oracle dist, model precomputation), computed once."""
    out = {}
    for c in wc.CASES:
        x, y, expect = wc.make_case(c, table)
        oidx, odist = oracle.nn_bruteforcel1k2(x, y)
        out[c.id] = (x, y, expect, oidx, odist, wm.prepare(x, y, table))
    return out


def _model(c, prepared, table, schedule, per_tile=None):
    x, y, _, oidx, odist, pre = prepared[c.id]
    idx, dist, stats = wm.run(x, y, table, pc.blocks_of(c.setting), pc.share_of(c.setting), schedule, pre, per_tile)
    n = len(y)
    same = np.array_equal(idx[:n], oidx) and np.array_equal(dist[:n], odist) and bool((idx[n:] == wm.NONE).all())
    return same, stats


def test_the_table_contains_what_it_is_for():
    one = [c for c in wc.CASES if wc.plan(c)[0] == 1]
    assert {c.xrows for c in one} >= set(wc.DB_ROWS)
    assert {c.yrows for c in one} >= set(wc.QUERIES)
    several = {wc.plan(c)[2] for c in wc.CASES if c.setting in ("two", "three")}
    assert several >= {(2, 2), (3, 3), (4, 4), (5, 5), (3, 3, 3), (5, 5, 5)}, several
    assert any(c.setting == "default" and wc.plan(c)[0] > 2 and set(wc.plan(c)[2]) == {1} for c in wc.CASES)
    assert {c.kind for c in wc.CASES} >= {"planted", "ties", "second", "tight", "constant", "nearconstant"}
    leaving = [c for c in wc.CASES if c.kind == "constant" and pc.share_of(c.setting) == pc.BREAK_EVEN_SHARE]
    assert {c.yrows for c in leaving} == {300, 513}
    assert len({c.setting for c in wc.CASES} - {"default"}) <= 4      # child processes of the GPU test


def test_model_gives_the_oracle_s_bytes_on_every_case(prepared, table):
    for c in wc.CASES:
        _, _, expect, oidx, _, _ = prepared[c.id]
        for k, rows in expect.items():
            assert tuple(int(v) for v in oidx[k]) == rows, (c.id, k)
        stats = {}
        for schedule in wm.SCHEDULES:
            same, stats[schedule] = _model(c, prepared, table, schedule)
            assert same, (c.id, schedule)
        if wc.plan(c)[0] == 1:
            assert len(set(stats.values())) == 1, (c.id, stats)


def test_planted_survivor_counts(prepared, table):
    """Every wave of the planted case keeps all 4096 pairs of tile 0 and then exactly the planted pairs; over waves
    and tiles these are the counts the survivor pass changes its form at."""
    c, = [c for c in wc.CASES if c.kind == "planted"]
    per_tile = []
    same, stats = _model(c, prepared, table, "up", per_tile)
    assert same and stats[2] == 0
    got = {(w, tl): int(n) for _, _, tl, surv in per_tile for w, n in enumerate(surv)}
    assert all(got[(w, 0)] == 64 * 64 for w in range(wm.WAVES))
    assert {k: v for k, v in got.items() if k[1] > 0} == wc.planted_counts()
    assert set(wc.planted_counts().values()) >= set(wc.WANTED_COUNTS)


def test_leaving_and_full_cases(prepared, table):
    """Constant rows under the shipped share: every workgroup leaves its slice, `fallback` is the slice's rows x 512
    for each; with the share rule off nobody leaves and every pair survives."""
    for c in wc.CASES:
        if c.kind not in ("constant", "nearconstant"):
            continue
        _, stats = _model(c, prepared, table, "up")
        groups = wc.plan(c)[3]
        if pc.share_of(c.setting) == 1024:
            assert stats == (c.xrows * 512 * groups,) * 2 + (0,), (c.id, stats)
        else:
            assert stats[2] == c.xrows * 512 * groups and 0 < stats[0] < stats[2], (c.id, stats)
