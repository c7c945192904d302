"""CPU only: the half-step protocol of l1k2_prune_wide_kernel, stated as the event model of
tests/l1k2_prune_stagger_model.py, keeps its barriers, buffer windows and leaving decisions for 0, 1, 2, 3, 4 and 7
tiles with the flag raised at every tile by a leading wave, a trailing wave and both; its statistics are those of
tests/l1k2_prune_wide_model.py on the one-slice cases in which workgroups leave; and the model is not blind: a load
issued a half-step early, a missing wait and a missing first barrier of the trailing waves are each reported."""
import numpy as np
import pytest

from tests import l1k2_prune_cases as pc
from tests import l1k2_prune_stagger_model as sm
from tests import l1k2_prune_wide_cases as wc
from tests import l1k2_prune_wide_model as wm
from tests.test_l1k2_bound_table import _table

TILES = (0, 1, 2, 3, 4, 7)
RAISERS = {"lead": (1,), "trail": (6,), "both": (2, 5), "all": tuple(range(sm.WAVES))}


@pytest.mark.parametrize("ntiles", TILES)
def test_nobody_leaves(ntiles):
    res = sm.simulate(ntiles)
    assert sm.check(res) == []
    assert res.barriers == [2 * ntiles + 1] * sm.WAVES
    assert res.counted == [list(range(ntiles))] * sm.WAVES
    assert res.gave_up == [False] * sm.WAVES


@pytest.mark.parametrize("who", sorted(RAISERS))
@pytest.mark.parametrize("ntiles", TILES[1:])
def test_a_flag_at_every_tile(ntiles, who):
    for at in range(ntiles):
        res = sm.simulate(ntiles, lambda w, tl: tl == at and w in RAISERS[who])
        assert sm.check(res) == [], (ntiles, at, who)
        # tiles 0 .. at are counted by every wave, nothing of tile at + 1, and 2 at + 3 barriers are passed: at the last
        # tile that is the 2 n + 1 of a slice that ends
        assert res.counted == [list(range(at + 1))] * sm.WAVES, (ntiles, at, who)
        assert res.barriers == [2 * at + 3] * sm.WAVES, (ntiles, at, who)
        assert res.gave_up == [True] * sm.WAVES, (ntiles, at, who)


def test_flags_at_two_tiles_leave_at_the_first():
    res = sm.simulate(7, lambda w, tl: (tl == 2 and w == 5) or (tl == 3 and w == 0) or tl == 4)
    assert sm.check(res) == []
    assert res.counted == [[0, 1, 2]] * sm.WAVES and res.barriers == [7] * sm.WAVES


@pytest.mark.parametrize("ntiles", (3, 4, 7))
def test_a_load_issued_a_half_step_early_is_detected(ntiles):
    raw_early = sm.check(sm.simulate(ntiles, proto=sm.PROTOCOL._replace(lead_raw="M")))
    assert raw_early and all(p.startswith("R tile") or "reads R" in p for p in raw_early), raw_early
    feat_early = sm.check(sm.simulate(ntiles, proto=sm.PROTOCOL._replace(lead_feat="C-1")))
    assert feat_early and all(p.startswith("F tile") or "reads F" in p for p in feat_early), feat_early


@pytest.mark.parametrize("ntiles", TILES)
def test_a_missing_first_barrier_is_detected(ntiles):
    problems = sm.check(sm.simulate(ntiles, proto=sm.PROTOCOL._replace(trail_first_barrier=False)))
    assert any("hang" in p for p in problems), problems


def test_a_missing_wait_is_detected():
    problems = sm.check(sm.simulate(3, proto=sm.PROTOCOL._replace(wait_before_mid=False)))
    assert any("was waited for in None" in p for p in problems), problems


@pytest.fixture(scope="module")
def table():
    return _table()


def test_statistics_are_the_wide_models(table):
    """One-slice cases with the share rule at work: per-tile survivor counts from the wide model drive the event
    model's waves through the kernel's share rule; what they count is what the wide model counted, so a leading wave's
    dropped tile is in neither."""
    cases = [c for c in wc.CASES if wc.plan(c)[0] == 1 and c.kind in ("constant", "planted", "ties")]
    assert {c.kind for c in cases} == {"constant", "planted", "ties"}
    left = 0
    for c in cases:
        x, y, _ = wc.make_case(c, table)
        share = pc.share_of(c.setting)
        per_tile = []
        _, _, stats = wm.run(x, y, table, pc.blocks_of(c.setting), share, "up", None, per_tile)
        groups = wc.plan(c)[3]
        ntiles = wc.plan(c)[2][0]
        bounded = survivors = fallback = 0
        for qb in range(groups):
            surv = {tl: s for q, _, tl, s in per_tile if q == qb}
            res = sm.simulate(ntiles, sm.share_rule(lambda w, tl: int(surv[tl][w]), share))
            assert sm.check(res) == [], c.id
            tiles = res.counted[0]
            assert tiles == sorted(surv), (c.id, tiles, sorted(surv))     # the tiles the wide model ran, no other
            bounded += sum(min(wm.TILE, c.xrows - wm.TILE * tl) for tl in tiles) * wm.QBLOCK
            survivors += sum(int(surv[tl][w]) for w in range(sm.WAVES) for tl in res.counted[w])
            if res.gave_up[0]:
                fallback += c.xrows * wm.QBLOCK
                left += 1
        assert (bounded, survivors, fallback) == stats, (c.id, (bounded, survivors, fallback), stats)
    assert left >= 2
