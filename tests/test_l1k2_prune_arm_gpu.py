"""l1k2_prune_wide_kernel arms a tile's accumulators (thresholds from k2s[] and the shared values, 64 moves, every second
tile the publication) at the end of the tile before, behind its drains and ahead of the end-of-tile barrier, and once
ahead of the loop.  On the GPU, with the wide form forced on through spv_l1k2_set_prune(1) and
spv_l1k2_set_prune_form(1) and with both bound tables: every case bit for bit against the CPU oracle, one-slice cases
also with the statistics of tests/l1k2_prune_wide_model.py.  A threshold that reaches a tile stale (made before the
drains of the tile before it were done, or not made again at all) shows as a survivor total above the model's.

  * tile:    one tile alone, 64 and 33 rows: only the arm ahead of the loop is used, the one behind the last tile is inert;
  * ragged:  two and three tiles, the last ragged in either row half (65, 97, 129, 161 rows), against 256, 257, 512 and
             700 queries: lanes past the last query carry the last query's thresholds;
  * moving:  a threshold that must move between adjacent tiles (see `moving`), for t even and odd and a wave of either
             half; and one slice of exactly 2, 3, 4 and 5 tiles, so that the last arm falls on a tile that would publish
             and on one that would not;
  * three, four: slices of 4-5 tiles that hand thresholds on (the publication at the end of every second tile);
  * share:   the share rule fires at tile 3 and at tile 4, as a middle and as the last tile, by a wave of either half:
             the leading waves drop a tile whose accumulators were armed, the statistics are the model's;
  * octet0:  the one-pair-per-lane drain ahead of the arm.

One fresh child per setting, as in tests/test_l1k2_prune_stagger_gpu.py, whose `planted` recipe, case type and intents
are used here: a child runs all of its cases and stops at the first that fails; one that ends by a signal, an abort or
the time limit fails its test and makes the rest of this module skip."""
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
from tests import test_l1k2_prune_stagger_gpu as sg  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120
TILE = 64
ONE = {"SPECTAVI_L1K2_BLOCKS": "1"}
SETTINGS = {
    "tile": ONE,
    "ragged": ONE,
    "moving": ONE,
    # any share up to 3/4 gives the same rule in a lone workgroup's first 128 tiles: 3/4
    "share": {"SPECTAVI_L1K2_BLOCKS": "1", "SPECTAVI_L1K2_PRUNE_SHARE": "512"},
    "three": {"SPECTAVI_L1K2_BLOCKS": "3"},
    "four": {"SPECTAVI_L1K2_BLOCKS": "4"},
    "octet0": {"SPECTAVI_L1K2_BLOCKS": "1", "SPECTAVI_L1K2_PRUNE_OCTET": "0"},
}
SLICES = {"three": 3, "four": 4}
QUERIES = (256, 257, 512, 700)
_gpu_lost = []   # why nothing more may be started on the GPU from this module

Case = sg.Case   # id xrows yrows make intent fallback; intent(per_tile of the model with table 0, its statistics)
CaseFailed = sg.CaseFailed


def _cluster(xrows, yrows, tag):
    c = wc._case("one", xrows, yrows, "cluster")
    return Case("arm-%s-%s" % (tag, c.id), xrows, yrows, lambda table, c=c: wc.make_case(c, table)[:2], None, None)


def _centres(xrows, yrows, table):
    """The two cluster centres that sg.planted(xrows, yrows, ...) draws first from its generator."""
    rng = np.random.default_rng([xrows, yrows, 23])
    pairs = pc.tight_pairs(table)
    pick = rng.integers(0, len(pairs), 128)
    return (np.array([pairs[i][1] for i in pick], np.uint8), np.array([pairs[i][0] for i in pick], np.uint8))


MOVING_A, MOVING_ROWS = 20, (3, 17, 33, 34, 62)


def moving(t, wave, lower=True):
    """`planted` with 20 queries of cluster A in `wave` and none elsewhere, and three kinds of rows made from A's
    centre with k bytes of B's (a byte pair of the two centres is tight: the bound of such a row is exact in those
    bytes): tile 0 holds two rows with k = 4, the second best of an A query after tile 0 (about 900); tile t holds
    two copies of the centre itself, which lower it to the queries' own noise (below 25); tile t + 1 holds five rows
    with k = 2 in both row halves, whose bound (about 210) lies between the two.  With lower = False tile t has no such
    rows.  Rows: t + 3 tiles, the last ragged."""
    xrows = (t + 3) * TILE - 7
    base = sg.planted(xrows, 512, tuple(MOVING_A if w == wave else 0 for w in range(8)), {})

    def make(table):
        x, y = base(table)
        a_c, b_c = _centres(xrows, 512, table)

        def part(k, first):
            r = a_c.copy()
            r[first:first + k] = b_c[first:first + k]
            return r
        x[0], x[1] = part(4, 0), part(4, 4)
        if lower:
            x[TILE * t + 9] = x[TILE * t + 40] = a_c
        for i, o in enumerate(MOVING_ROWS):
            x[TILE * (t + 1) + o] = part(2, 8 + 2 * i)
        return x, y
    return xrows, make


def _moves(t, wave):
    """The case does what it is for: tile t's two rows are kept by the wave's A queries and lower their second best,
    and tile t + 1's five rows, kept by all of them without tile t's rows, are then kept by none."""
    def intent(per_tile, stats):
        from tests.test_l1k2_bound_table import _table
        table = _table()                      # the recipe, table 0
        x, y = moving(t, wave, lower=False)[1](table)
        without = []
        wm.run(x, y, table, 1, pc.BREAK_EVEN_SHARE, "up", None, without)
        got, old = sg._counts(per_tile), sg._counts(without)
        assert stats[2] == 0
        for w in range(8):
            for tl in range(1, t + 3):
                want = 2 * MOVING_A if (w, tl) == (wave, t) else 0
                assert got[(w, tl)] == want, (w, tl, got[(w, tl)], want)
                want_old = len(MOVING_ROWS) * MOVING_A if (w, tl) == (wave, t + 1) else 0
                assert old[(w, tl)] == want_old, (w, tl, old[(w, tl)], want_old)
    return intent


def _sliced(setting, xrows, yrows):
    """`planted` over several slices: queries of both clusters in every wave, two rows near either cluster at the head
    of every slice and some in every later tile."""
    slices, slice_rows, _ = pc.plan_of(xrows, yrows, int(SETTINGS[setting]["SPECTAVI_L1K2_BLOCKS"]))
    plant = {}
    for tl in range(1, -(-xrows // TILE)):
        plant[tl] = (2, 2) if tl * TILE % slice_rows == 0 else (1 + tl % 3, tl % 2) if xrows - tl * TILE >= 4 else (1, 0)
    return Case("arm-%s-%dx%d-planted" % (setting, xrows, yrows), xrows, yrows,
                sg.planted(xrows, yrows, (1, 7, 8, 9, 16, 17, 63, 32), plant), None, None)


def _build():
    cases = {s: [] for s in SETTINGS}
    for x in (64, 33):
        for n in QUERIES:
            cases["tile"].append(_cluster(x, n, "tile"))
    for x in (65, 97, 129, 161):
        for n in QUERIES:
            cases["ragged"].append(_cluster(x, n, "ragged"))
    for t in (1, 2):
        for wave in (2, 6):
            xrows, make = moving(t, wave)
            # without the octet pass once for either parity of t and either half
            for setting in ("moving", "octet0") if (t, wave) in ((1, 6), (2, 2)) else ("moving",):
                cases[setting].append(Case("arm-%s-%dx512-tile%d-lowers-wave%d" % (setting, xrows, t, wave), xrows, 512, make,
                                           _moves(t, wave), None))
    for x, n in ((2 * TILE, 512), (3 * TILE, 64), (4 * TILE, 300), (5 * TILE - 9, 513)):
        cases["moving"].append(_cluster(x, n, "cadence"))
    cases["octet0"].append(_cluster(161, 700, "octet0"))
    # the share rule: every pair of the wave's tiles 2 and 3 kept fires at tile 3; 44 of 64 rows of tile 2 and all of
    # tiles 3 and 4 fires at tile 4 (22528 -> 23808 -> 24928 against 24576)
    for wave in (2, 5):
        a_per = tuple(64 if w == wave else 0 for w in range(8))
        for at, ntiles, plant in ((3, 5, {2: (64, 0), 3: (64, 0)}), (3, 4, {2: (64, 0), 3: (64, 0)}),
                                  (4, 7, {2: (44, 0), 3: (64, 0), 4: (64, 0)}), (4, 5, {2: (44, 0), 3: (64, 0), 4: (64, 0)})):
            rows = ntiles * TILE
            cases["share"].append(Case("arm-share-%dx512-wave%d-fires-at-%d-of-%d" % (rows, wave, at, ntiles), rows, 512,
                                       sg.planted(rows, 512, a_per, plant), sg._fires(wave, at, ntiles), rows * 512))
    # slices of 4-5 tiles, the last one ragged in either row half
    for x, n in ((750, 64), (940, 256)):
        cases["three"].append(_sliced("three", x, n))
    for x, n in ((1000, 255), (1217, 256)):
        cases["four"].append(_sliced("four", x, n))
    ids = [c.id for cs in cases.values() for c in cs]
    assert len(set(ids)) == len(ids), ids
    return cases


CASES = _build()


def check_case(c, setting, oracle_fn):
    from spectavi_amd import device
    env = SETTINGS[setting]
    blocks = int(env["SPECTAVI_L1K2_BLOCKS"])
    share = int(env.get("SPECTAVI_L1K2_PRUNE_SHARE", pc.BREAK_EVEN_SHARE))
    slices, slice_rows, _ = pc.plan_of(c.xrows, c.yrows, blocks)
    got = device.l1k2_plan(c.xrows, c.yrows, 128)
    if (got["slices"], got["slice_rows"]) != (slices, slice_rows):
        raise CaseFailed("%s: plan %r, the case needs %d slices of %d rows" % (c.id, got, slices, slice_rows))
    if slices != SLICES.get(setting, 1):
        raise CaseFailed("%s: %d slices under setting %s" % (c.id, slices, setting))
    if slices > 1 and not all(4 <= -(-(min(c.xrows, (s + 1) * slice_rows) - s * slice_rows) // TILE) <= 5 for s in range(slices)):
        raise CaseFailed("%s: slices of %d rows are not 4-5 tiles each" % (c.id, slice_rows))
    tables = {which: device.l1k2_bound_table(which) for which in (0, 1)}
    x, y = c.make(tables[0])
    oidx, odist = oracle_fn(x, y)
    problems, seen = [], None
    for which in (0, 1):
        per_tile = []
        want = wm.run(x, y, tables[which], blocks, share, "up", None, per_tile)[2]
        if which == 0 and c.intent is not None:
            c.intent(per_tile, want)
        idx, dist, stats = sg._run(x, y, which)
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
