"""The half-step form of l1k2_prune_wide_kernel (two barriers per tile, waves 4-7 half a tile behind waves 0-3) on the
GPU, forced on through spv_l1k2_set_prune(1) and spv_l1k2_set_prune_form(1), with both bound tables: bit for bit
against the CPU oracle, and on one-slice cases with the statistics of tests/l1k2_prune_wide_model.py, which pin the
tile at which a workgroup leaves and that the tile the leading waves drop is counted nowhere.

Shapes: 1 to 5 tiles, odd and even, the last one ragged in either row half, against 256 queries (waves 4-7 hold only
clamped copies) up to 700.  Planted inputs (the two-cluster recipe of tests/l1k2_prune_wide_cases.py, with the
clusters given to chosen waves): survivors only in waves 0-3 or only in waves 4-7; 0, 8, 9, 65 and 200 survivors in one
wave's tile while the others have none; the share rule fired by a wave of 0-3 only and of 4-7 only.  The rule cannot
fire before tile 3 of a workgroup without inherited thresholds (l1k2_prune.hip: the limit is the whole tile up to
kWideSkipTilesAlone), which is what one slice gives, so "the first tile" is tile 3; it is made to fire there and at
tile 4 (odd and even flag slot), each as a middle and as the last tile.  Every such case first asserts on the model's
per-tile counts that it does what it is for.

One fresh child per setting (the library reads its environment once per process) runs all of its cases and stops at
the first that fails.  A child that ends by a signal, an abort or the time limit fails its test and makes the rest of
this module skip: nothing more is started on the GPU from here."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # run as the child of test_setting_in_a_child_process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import l1k2_prune_cases as pc  # noqa: E402
from tests import l1k2_prune_stagger_model as sm  # noqa: E402
from tests import l1k2_prune_wide_cases as wc  # noqa: E402
from tests import l1k2_prune_wide_model as wm  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120
TILE = 64
DB_ROWS = (64, 65, 128, 129, 191, 192, 64 * 4 + 33)
QUERIES = (256, 257, 300, 512, 513, 700)
COUNTS = (0, 8, 9, 65, 200)
SETTINGS = {
    "one": {"SPECTAVI_L1K2_BLOCKS": "1"},
    # any share up to 3/4 gives the same rule in a lone workgroup's first 128 tiles: 3/4
    "share": {"SPECTAVI_L1K2_BLOCKS": "1", "SPECTAVI_L1K2_PRUNE_SHARE": "512"},
    "three": {"SPECTAVI_L1K2_BLOCKS": "3"},
    "octet0": {"SPECTAVI_L1K2_BLOCKS": "1", "SPECTAVI_L1K2_PRUNE_OCTET": "0"},
}
_gpu_lost = []   # why nothing more may be started on the GPU from this module

# make(table) -> (x, y); intent(per_tile of the model with table 0, stats) asserts what the case is for, or None
Case = collections.namedtuple("Case", "id xrows yrows make intent fallback")


class CaseFailed(AssertionError):
    pass


def planted(xrows, yrows, a_per_wave, plant):
    """Two clusters of queries as in tests/l1k2_prune_wide_cases.py: wave w holds a_per_wave[w] queries of cluster A
    (the rest are B), tile t >= 1 holds plant[t] = (rows near A, rows near B), every other row is far from both.  A
    wave keeps nA a + nB (64 - a) pairs of such a tile and all of tile 0."""
    def make(table):
        rng = np.random.default_rng([xrows, yrows, 23])
        pairs = pc.tight_pairs(table)
        pick = rng.integers(0, len(pairs), 128)
        b_c = np.array([pairs[i][0] for i in pick])
        a_c = np.array([pairs[i][1] for i in pick])

        def noisy(center, rows, npos, sign):
            out = np.repeat(center[None, :], rows, axis=0).astype(np.int16)
            for r in range(rows):
                out[r, rng.choice(128, npos, replace=False)] += sign * rng.integers(1, 4, npos)
            return out
        in_a = np.zeros(yrows, bool)
        for w, a in enumerate(a_per_wave):
            in_a[64 * w:64 * w + a] = True       # past the last query: nothing
        y = np.where(in_a[:, None], noisy(a_c, yrows, 8, -1), noisy(b_c, yrows, 8, +1))
        near_a = np.zeros(xrows, bool)
        near_b = np.zeros(xrows, bool)
        near_a[0:2] = True                        # tile 0: every query has a second best
        near_b[2:4] = True
        for t, (na, nb) in plant.items():
            offs = [o for o in (37 * np.arange(TILE) + 5) % TILE if TILE * t + o < xrows]   # 5, 42, 15, ...: both halves
            assert t >= 1 and na + nb <= len(offs)
            near_a[[TILE * t + o for o in offs[:na]]] = True
            near_b[[TILE * t + o for o in offs[na:na + nb]]] = True
        xa, xb = noisy(a_c, xrows, 12, -1), noisy(b_c, xrows, 12, +1)
        far = np.where(rng.random((xrows, 128)) < 0.5, 0, 255)
        x = np.where(near_a[:, None], xa, np.where(near_b[:, None], xb, far))
        return np.ascontiguousarray(x.astype(np.uint8)), np.ascontiguousarray(y.astype(np.uint8))
    return make


def _counts(per_tile):
    return {(w, tl): int(n) for _, _, tl, surv in per_tile for w, n in enumerate(surv)}


def _only_waves(waves, ntiles):
    def intent(per_tile, stats):
        got = _counts(per_tile)
        assert stats[2] == 0 and max(tl for _, tl in got) == ntiles - 1
        for (w, tl), n in got.items():
            if tl > 0:
                assert (n > 0) == (w in waves), ("survivors of wave %d in tile %d: %d" % (w, tl, n))
    return intent


def _imbalance(wave, counts):
    def intent(per_tile, stats):
        got = _counts(per_tile)
        assert stats[2] == 0
        for tl, want in counts.items():
            for w in range(8):
                assert got[(w, tl)] == (want if w == wave else 0), (w, tl, got[(w, tl)], want)
    return intent


def _fires(wave, at, ntiles):
    def intent(per_tile, stats):
        surv = {tl: s for _, _, tl, s in per_tile}
        assert sorted(surv) == list(range(at + 1)), sorted(surv)           # the model left after tile `at`
        rule = sm.share_rule(lambda w, tl: int(surv[tl][w]), 512)
        raised = {(w, tl) for tl in range(at + 1) for w in range(8) if rule(w, tl)}
        assert raised == {(wave, at)}, raised
        assert stats == ((at + 1) * TILE * 512, int(sum(s.sum() for s in surv.values())), ntiles * TILE * 512), stats
    return intent


def _cluster(setting, xrows, yrows, kind="cluster", tag=""):
    c = wc._case(setting, xrows, yrows, kind)
    return Case("stagger-" + tag + c.id, xrows, yrows, lambda table, c=c: wc.make_case(c, table)[:2], None,
                xrows * 512 * -(-yrows // 512) if kind == "constant" else None)


def _build():
    cases = {s: [] for s in SETTINGS}
    for x in DB_ROWS:
        for n in QUERIES:
            cases["one"].append(_cluster("one", x, n))
    full = 4 * TILE + 33
    for name, waves in (("lead", (0, 1, 2, 3)), ("trail", (4, 5, 6, 7))):
        a = tuple(5 + w if w in waves else 0 for w in range(8))
        cases["one"].append(Case("stagger-one-%dx512-only-%s" % (full, name), full, 512,
                                 planted(full, 512, a, {1: (1, 0), 2: (3, 0), 3: (2, 0), 4: (4, 0)}), _only_waves(waves, 5), None))
    for wave in (2, 6):
        for a, plant, counts in ((1, {1: (8, 0), 2: (9, 0), 3: (0, 0)}, {1: 8, 2: 9, 3: 0}),
                                 (5, {1: (13, 0), 2: (40, 0), 3: (0, 0)}, {1: 65, 2: 200, 3: 0})):
            a_per = tuple(a if w == wave else 0 for w in range(8))
            for setting in ("one", "octet0"):
                cases[setting].append(Case("stagger-%s-%dx512-wave%d-counts-%s" % (setting, full, wave, "-".join(map(str, counts.values()))),
                                           full, 512, planted(full, 512, a_per, plant), _imbalance(wave, counts), None))
    cases["octet0"].append(_cluster("one", 129, 300, tag="octet0-"))
    cases["octet0"].append(_cluster("one", full, 700, tag="octet0-"))
    # the share rule: every pair of the wave's tiles 2 and 3 kept fires at tile 3; 44 of 64 rows of tile 2 and all of
    # tiles 3 and 4 fires at tile 4 (22528 -> 23808 -> 24928 against 24576)
    for wave in (1, 6):
        a_per = tuple(64 if w == wave else 0 for w in range(8))
        for at, ntiles, plant in ((3, 5, {2: (64, 0), 3: (64, 0)}), (3, 4, {2: (64, 0), 3: (64, 0)}),
                                  (4, 7, {2: (44, 0), 3: (64, 0), 4: (64, 0)}), (4, 5, {2: (44, 0), 3: (64, 0), 4: (64, 0)})):
            rows = ntiles * TILE
            cases["share"].append(Case("stagger-share-%dx512-wave%d-fires-at-%d-of-%d" % (rows, wave, at, ntiles), rows, 512,
                                       planted(rows, 512, a_per, plant), _fires(wave, at, ntiles), rows * 512))
    # three slices: thresholds handed on between them, and the hand-over list with every workgroup leaving every slice
    for x, n in ((567, 64), (959, 255), (3 * 5 * TILE, 256)):
        cases["three"].append(_cluster("three", x, n))
    cases["three"].append(_cluster("three", 3 * 5 * TILE, 256, "constant"))
    ids = [c.id for cs in cases.values() for c in cs]
    assert len(set(ids)) == len(ids), ids
    return cases


CASES = _build()


def _run(x, y, bound):
    """(idx, dist, (bounded, survivors, fallback pairs)) of the wide form with the bound forced on."""
    import torch
    from spectavi_amd import device
    before = device.l1k2_get_prune(), device.l1k2_get_prune_form(), device.l1k2_get_bound()
    device.l1k2_set_prune(1)
    device.l1k2_set_prune_form(1)
    device.l1k2_set_bound(bound)
    try:
        idx, dist = device.l1k2(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
        stats = device.l1k2_prune_stats()
        return idx.cpu().numpy().view(np.uint64), dist.cpu().numpy(), stats
    finally:
        device.l1k2_set_prune(before[0])
        device.l1k2_set_prune_form(before[1])
        device.l1k2_set_bound(before[2])


def check_case(c, setting, oracle_fn):
    from spectavi_amd import device
    env = SETTINGS[setting]
    blocks = int(env.get("SPECTAVI_L1K2_BLOCKS", 16384))
    share = int(env.get("SPECTAVI_L1K2_PRUNE_SHARE", pc.BREAK_EVEN_SHARE))
    slices, slice_rows, _ = pc.plan_of(c.xrows, c.yrows, blocks)
    got = device.l1k2_plan(c.xrows, c.yrows, 128)
    if (got["slices"], got["slice_rows"]) != (slices, slice_rows):
        raise CaseFailed("%s: plan %r, the case needs %d slices of %d rows" % (c.id, got, slices, slice_rows))
    if (slices == 3) != (setting == "three"):
        raise CaseFailed("%s: %d slices under setting %s" % (c.id, slices, setting))
    tables = {which: device.l1k2_bound_table(which) for which in (0, 1)}
    x, y = c.make(tables[0])
    oidx, odist = oracle_fn(x, y)
    problems, seen = [], None
    for which in (0, 1):
        per_tile = []
        want = wm.run(x, y, tables[which], blocks, share, "up", None, per_tile)[2]
        if which == 0 and c.intent is not None:
            c.intent(per_tile, want)
        idx, dist, stats = _run(x, y, which)
        seen = seen or stats
        bad = np.flatnonzero((idx != oidx).any(axis=1) | (dist != odist).any(axis=1))
        if len(bad):
            k = int(bad[0])
            problems.append("table %d: %d of %d queries differ from the oracle, first query %d: got idx %s dist %s, want idx %s dist %s" % (
                which, len(bad), len(oidx), k, idx[k].tolist(), dist[k].tolist(), oidx[k].tolist(), odist[k].tolist()))
        if not 0 < stats[1] <= stats[0] or stats[0] % 512 or stats[2] % 512:
            problems.append("table %d: statistics %r are not the wide form's" % (which, stats))
        if slices == 1 and stats != want:
            problems.append("table %d: statistics %r, the model's %r" % (which, stats, want))
        if c.fallback is not None and stats[2] != c.fallback:
            problems.append("table %d: fallback %d, every workgroup leaves every slice: %d" % (which, stats[2], c.fallback))
    if problems:
        raise CaseFailed("%s (slices %d):\n  %s" % (c.id, slices, "\n  ".join(problems)))
    print("ok %s slices %d %s" % (c.id, slices, seen), flush=True)


def _skip_if_gpu_lost():
    if _gpu_lost:
        pytest.skip("nothing more is started on the GPU from this module: %s" % _gpu_lost[0])


@pytest.mark.parametrize("setting", sorted(SETTINGS))
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
    assert r.returncode == 0 and ("all ok: %s, %d cases" % (setting, len(CASES[setting]))) in r.stdout, r.stdout


if __name__ == "__main__":
    from oracle import oracle as _oracle
    try:
        for _c in CASES[sys.argv[1]]:
            check_case(_c, sys.argv[1], _oracle.nn_bruteforcel1k2)
    except CaseFailed as e:
        print("FAILED %s" % e, flush=True)
        sys.exit(1)
    print("all ok: %s, %d cases" % (sys.argv[1], len(CASES[sys.argv[1]])))
