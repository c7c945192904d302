"""The per-tile chain of the dim-128 bound path of the L1 2-NN (l1k2_prune.hip) where a tile leaves a handful of
survivors: the one octet round that serves up to eight pairs and the first count past it, survivors that share a
lane (two compaction rounds), the bail flag that is read at one tile's end and looked at at the next tile's top,
and the stage loads that take their addresses from a scalar base.  Results are the oracle's bit for bit, the
statistics those of the numpy model (tests/l1k2_prune_model.py); that the tiles hold the survivor counts they were
built to hold is itself asserted, through the model, as tests/test_l1k2_prune_drain_gpu.py does.

How the counts are planted.  64 distinct random queries, so the first wave holds them all and the other three work
on copies of the last one, which is never planted after the warm tiles.  Random rows are far from everything: once
a query has a second best they are ruled out.  Tiles 0..3 are two near copies of every query.  From tile 4 on a
tile holds copies of chosen queries at chosen rows, each nearer than every copy of that query before it, so each
survives for its own query only.  A survivor's lane is the query column c of queries c and 32 + c crossed with
the row half g = (row >> 2) & 1.  The kinds of tile:
  * n = 0, 1, 7, 8, 9 survivors in distinct lanes: one compaction round, one octet round up to eight, the first count past it;
  * 2 and 8 survivors of which two share a lane (once two rows of one half for one query, once queries c and
    32 + c on rows of one half): a second compaction round;
  * two equally distant copies of one query in different lanes: one octet round evaluates both, the row decides.
Every kind stands once at an even and once at an odd tile (both LDS buffers), and the ragged last tile, of 1 or of
31 live rows, has a survivor in its last live row.

One slice of many tiles needs SPECTAVI_L1K2_BLOCKS=1, and the hand-over off needs SPECTAVI_L1K2_PRUNE_SHARE=1024;
the library reads both once, so each setting runs in a child process: "full" (hand-over off), "full" with
SPECTAVI_L1K2_PRUNE_OCTET=0 (one pair per lane always: nothing else may change), and
"one" (hand-over on: the planted data, and bytes in [0, 128), on which the model says that the workgroup leaves
at its tile 4 -- the flag of tile 4 is then seen at the top of tile 5 and the slice comes back from the exact
kernel).  The addressing test runs in the test process: with the default knobs slices are 64 rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # run as a child of the tests below
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import l1k2_prune_cases as pc  # noqa: E402
from tests import l1k2_prune_model as pm  # noqa: E402

CHILD_TIMEOUT = 180
TILE, NQ = pc.TILE, 64
WARM_TILES = 4
TIE_QUERIES = (61, 62)                 # planted as ties once each and never again; 63 is never planted after the warm tiles
POOL = 61                              # queries 0..60 take turns for everything else
DISTINCT_ROWS = (2, 7, 12, 17, 22, 27, 0, 5, 10)
SHARED_ROWS = (8, 9)                   # one half: g = 0
TIE_ROWS = (8, 12)                     # different halves
KINDS = [("distinct", 0), ("distinct", 1), ("distinct", 7), ("distinct", 8), ("distinct", 9),
         ("same_query", 2), ("cross", 2), ("same_query", 8), ("cross", 8), ("tie", 2)]
SEQUENCE = KINDS + [("distinct", 0)] + KINDS     # 21 tiles: every kind at an even and at an odd tile
LAST_ROWS = (1, 31)


def lane_of(q, row):
    return (q & 31) + 32 * ((row >> 2) & 1)


def plants_of(last_rows):
    """[(tile after the warm ones, [(query, row, tie)])] with the lane property of every tile asserted."""
    nxt = [0]

    def take(n, avoid_c31=False):
        out = []
        while len(out) < n:
            q = nxt[0] % POOL
            nxt[0] += 1
            if not (avoid_c31 and q & 31 == 31):
                out.append(q)
        return out

    tiles, ties = [], list(TIE_QUERIES)
    for kind, n in SEQUENCE:
        if kind == "distinct":
            plants = [(q, DISTINCT_ROWS[i], False) for i, q in enumerate(take(n))]
        elif kind == "tie":
            q = ties.pop(0)
            plants = [(q, TIE_ROWS[0], False), (q, TIE_ROWS[1], True)]
        else:
            plants = [(q, DISTINCT_ROWS[i], False) for i, q in enumerate(take(n - 2))]
            if kind == "same_query":
                q = take(1)[0]
                plants += [(q, SHARED_ROWS[0], False), (q, SHARED_ROWS[1], False)]
            else:
                c = take(1, avoid_c31=True)[0] & 31
                plants += [(c, SHARED_ROWS[0], False), (32 + c, SHARED_ROWS[1], False)]
        lanes = [lane_of(q, r) for q, r, _ in plants]
        shared = len(lanes) - len(set(lanes))
        assert shared == (1 if kind in ("same_query", "cross") else 0), (kind, n, plants)
        assert len(plants) == n and all(q != NQ - 1 for q, _, _ in plants)
        tiles.append(plants)
    # the ragged last tile: a survivor in the last live row, and one more where there is room, in distinct lanes
    qs = take(2)
    tiles.append([(qs[0], last_rows - 1, False)] + ([(qs[1], 3, False)] if last_rows > 4 else []))
    return tiles


def make_data(last_rows):
    rng = np.random.default_rng(1700 + last_rows)
    tiles = plants_of(last_rows)
    xrows = (WARM_TILES + len(tiles) - 1) * TILE + last_rows
    x = rng.integers(1, 255, (xrows, 128)).astype(np.int16)
    y = rng.integers(1, 255, (NQ, 128)).astype(np.int16)
    dist_next = np.full(NQ, 120)                      # the distance of a query's next copy: falls from copy to copy

    def copy_of(q, tie=False):
        if not tie:
            dist_next[q] -= 1
        row = y[q].copy()
        row[rng.choice(128, dist_next[q], replace=False)] += 1     # bytes 1..254: no saturation, the distance is exact
        return row

    slots = rng.permutation(WARM_TILES * TILE)
    for q in range(NQ):
        x[slots[2 * q]], x[slots[2 * q + 1]] = copy_of(q), copy_of(q)
    for t, plants in enumerate(tiles):
        for q, r, tie in plants:
            x[(WARM_TILES + t) * TILE + r] = copy_of(q, tie)
    return x.astype(np.uint8), y.astype(np.uint8), [len(p) for p in tiles]


def tile_survivors(x, y, table, ntiles, setting):
    """Survivors of every tile after the warm ones, by the model: the differences between runs on truncated databases."""
    blocks, share = pc.blocks_of(setting), pc.share_of(setting)
    dist, gsum, ysum = pm.prepare(x, y, table)
    ends = [min(len(x), (WARM_TILES + t) * TILE) for t in range(ntiles + 1)]
    totals = [pm.run(x[:e], y, table, blocks, share, pre=(dist[:e], gsum[:e], ysum))[2][1] for e in ends]
    return [int(b - a) for a, b in zip(totals, totals[1:])]


def check(x, y, which, setting, oracle_fn, what):
    """Two runs with the path forced on and one with it off against the oracle and the model; the model's statistics."""
    from spectavi_amd import device
    from tests.test_l1k2_bound_tuned import table_of
    from tests.test_l1k2_prune_gpu import _run
    plan = device.l1k2_plan(len(x), len(y), 128)
    assert plan["slices"] == 1, plan
    table = table_of(which)
    oidx, odist = oracle_fn(x, y)
    midx, mdist, want = pm.run(x, y, table, pc.blocks_of(setting), pc.share_of(setting))
    assert np.array_equal(midx[:len(y)], oidx) and np.array_equal(mdist[:len(y)], odist)
    before = device.l1k2_get_bound()
    device.l1k2_set_bound(which)
    try:
        runs = [_run(x, y, 1), _run(x, y, 1), _run(x, y, 0)]
    finally:
        device.l1k2_set_bound(before)
    for name, (idx, dist, stats) in zip(("prune on", "prune on, second run", "prune off"), runs):
        print("%s, table %d, %s: statistics %r, model %r" % (what, which, name, stats, want), flush=True)
        assert idx.tobytes() == oidx.tobytes() and dist.tobytes() == odist.tobytes(), (what, which, name)
    assert runs[0][2] == want and runs[1][2] == want and runs[2][2] == (0, 0, 0), (what, which)
    return oidx, odist, want


def run_planted(setting, oracle_fn, last_rows_of=LAST_ROWS):
    from tests.test_l1k2_bound_tuned import table_of
    for last_rows in last_rows_of:
        x, y, want_tiles = make_data(last_rows)
        assert (len(x) - 1) % TILE + 1 == last_rows
        for which in (0, 1):
            if setting == "full":    # with the hand-over on the workgroup may leave, by the model's own rule
                got = tile_survivors(x, y, table_of(which), len(want_tiles), setting)
                assert got == want_tiles, (which, last_rows, got, want_tiles)     # the tiles hold what they were built to hold
            oidx, odist, _ = check(x, y, which, setting, oracle_fn, "planted, last tile of %d rows" % last_rows)
            for q in TIE_QUERIES:                     # equally far, the lower row first
                assert odist[q][0] == odist[q][1] and oidx[q][0] + TIE_ROWS[1] - TIE_ROWS[0] == oidx[q][1], (q, oidx[q], odist[q])


def run_leaving(oracle_fn):
    """Bytes in [0, 128): nearly everything survives, the workgroup leaves, the exact kernel computes the slice."""
    rng = np.random.default_rng(1717)
    x = rng.integers(0, 128, (8 * TILE + 5, 128), dtype=np.uint8)
    y = rng.integers(0, 128, (NQ, 128), dtype=np.uint8)
    for which in (0, 1):
        _, _, want = check(x, y, which, "one", oracle_fn, "bytes in [0, 128)")
        # it left, at its tile 4: five tiles were bounded and the whole slice went to the exact kernel
        assert want[2] == len(x) * pc.QBLOCK and want[0] == 5 * TILE * pc.QBLOCK, want


def _child(mode, env_extra, marker):
    setting = "one" if mode == "one" else "full"
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPECTAVI_L1K2_")}
    env.update(pc.SETTINGS[setting])
    env.update(env_extra)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), mode]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    print(r.stdout)
    assert r.returncode == 0 and marker in r.stdout, r.stdout


def test_planted_tiles_have_the_lanes_they_claim():
    """CPU only: the planting itself (lanes distinct or shared as each kind says, every kind at both tile parities)."""
    for last_rows in LAST_ROWS:
        tiles = plants_of(last_rows)
        assert len(tiles) == len(SEQUENCE) + 1
        for k, kind in enumerate(KINDS):
            assert (WARM_TILES + k) % 2 != (WARM_TILES + len(KINDS) + 1 + k) % 2, kind
        assert tiles[-1][0][1] == last_rows - 1


@pytest.mark.gpu
def test_sparse_tiles_in_a_child_process():
    _child("full", {}, "chain ok: full")


@pytest.mark.gpu
def test_sparse_tiles_with_one_pair_per_lane_in_a_child_process():
    _child("octet0", {"SPECTAVI_L1K2_PRUNE_OCTET": "0"}, "chain ok: octet0")


@pytest.mark.gpu
def test_hand_over_on_in_a_child_process():
    _child("one", {}, "chain ok: one")


@pytest.mark.gpu
def test_scalar_base_addressing_over_slices(oracle):
    """Four slices with the default knobs: tiles that start at a slice's first row for slice > 0 (the scalar base of
    that slice), and a ragged last tile of one row.  l1k2_plan cuts slices in multiples of 64 rows, so only the last
    slice of a plan can end in a ragged tile (asserted below, not forced): the shape gives the last slice a full
    tile and a tile of one live row.  The "cluster" recipe of tests/l1k2_prune_cases.py puts two near rows at the
    head of every slice and copies of three queries at row 5, in the middle and in the last row.  Results are
    the oracle's bit for bit, and the bounded pairs and the fallback are the model's exactly.  How many pairs
    survive over several slices depends on which slice had published a threshold when another read it, that is on
    scheduling, so that count is only bounded: by the model's run in which no slice ever sees another's thresholds."""
    from spectavi_amd import device
    from tests.test_l1k2_bound_table import _table
    from tests.test_l1k2_prune_gpu import _run
    xrows, yrows = 3 * 64 + 33, 300
    case = pc._case("default", xrows, yrows, "cluster")
    plan = device.l1k2_plan(xrows, yrows, 128)
    assert (plan["slices"], plan["slice_rows"]) == (4, 64) and plan["slice_rows"] % TILE == 0, plan
    assert case.slices == 4 and case.tiles == (2, 2, 2, 2) and case.last_rows == 1, case
    table = _table()
    x, y, _ = pc.make_case(case, table)
    oidx, odist = oracle.nn_bruteforcel1k2(x, y)
    survivors = {}
    for schedule in pm.SCHEDULES:
        midx, mdist, mstats = pm.run(x, y, table, pc.blocks_of("default"), pc.share_of("default"), schedule)
        assert np.array_equal(midx[:yrows], oidx) and np.array_equal(mdist[:yrows], odist), schedule
        assert (mstats[0], mstats[2]) == (case.stats[0], 0), (schedule, mstats)
        survivors[schedule] = mstats[1]
    for attempt in range(2):
        idx, dist, stats = _run(x, y, 1)
        print("addressing %d x %d run %d: statistics %r, the model's survivors %r" % (xrows, yrows, attempt, stats, survivors))
        assert idx.tobytes() == np.ascontiguousarray(oidx).view(np.uint64).tobytes() and dist.tobytes() == odist.tobytes()
        assert (stats[0], stats[2]) == (case.stats[0], 0), stats
        assert stats[1] <= survivors["blind"], (stats, survivors)      # sharing thresholds only ever rules more out
    for k, r in zip((yrows - 1, yrows // 2, 0), (xrows - 1, xrows // 2, 5)):
        assert int(oidx[k][0]) == r and int(odist[k][0]) == 0, (k, oidx[k], odist[k])


if __name__ == "__main__":
    from oracle import oracle as _oracle
    _mode = sys.argv[1]
    if _mode == "full":
        run_planted("full", _oracle.nn_bruteforcel1k2)
    elif _mode == "octet0":
        run_planted("full", _oracle.nn_bruteforcel1k2, last_rows_of=(31,))
    else:
        run_planted("one", _oracle.nn_bruteforcel1k2, last_rows_of=(31,))
        run_leaving(_oracle.nn_bruteforcel1k2)
    print("chain ok: %s" % _mode)
