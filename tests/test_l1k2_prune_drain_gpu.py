"""The survivor pass of the dim-128 bound path of the L1 2-NN (the queue and `drain` of l1k2_prune.hip) at its round
and queue boundaries: one slice whose tiles hold, for the first wave, exactly 0, 1, 7, 8, 9, 63, 64, 65 and 160 surviving
pairs (eight pairs make a round of the octet form, 64 fill the queue, more than 128 wrap it), planted at odd and even
tile positions, with equal distances at different rows so that the row index decides, and a ragged last tile.  Both
bound tables are run.  Results are the oracle's bit for bit and the statistics are those of the numpy model
(tests/l1k2_prune_model.py); that the tiles hold the counts above is itself asserted, through the model.

How the counts are planted.  64 queries, so the first wave holds them all and the other three work on copies of the
last one.  Queries 0..31 are one and the same row G ("the group"), queries 32..63 are distinct random rows ("singles").
Random rows are far from everything: once a query has a second best they are ruled out.  Tiles 0..3 give every query
two near copies (tile 0, met without thresholds, survives whole: 2048 pairs per wave).  From tile 4 on a tile holds `a`
copies of distinct singles and `b` copies of G, each copy nearer than every copy before it (or as near as its
neighbour: the ties), so each survives for its own queries only: a + 32 b pairs.  The last single is never planted
again, so the copies of it in the other waves add nothing to the later tiles.

One slice of many tiles with the hand-over off needs SPECTAVI_L1K2_BLOCKS=1 and SPECTAVI_L1K2_PRUNE_SHARE=1024, which
the library reads once: the cases run in one child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # run as the child of test_drain_boundaries_in_a_child_process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import l1k2_prune_cases as pc  # noqa: E402
from tests import l1k2_prune_model as pm  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120
SETTING = "full"                       # one slice, no hand-over
TILE, NQ, GROUP = pc.TILE, 64, 32
# (copies of distinct singles, copies of G) of tiles 4, 5, ...: 0, 1, 7, 8, 9, 63, 64, 65, 160 pairs, then 1 and, in the
# ragged last tile of 9 live rows, 3 + 64
PLANTS = [(0, 0), (1, 0), (7, 0), (8, 0), (9, 0), (31, 1), (0, 2), (1, 2), (0, 5), (1, 0), (3, 2)]
WANT = [a + GROUP * b for a, b in PLANTS]
LAST_ROWS = 9
WARM_TILES = 4


def make_data():
    rng = np.random.default_rng(1608)
    xrows = (WARM_TILES + len(PLANTS) - 1) * TILE + LAST_ROWS
    x = rng.integers(1, 255, (xrows, 128)).astype(np.int16)
    y = rng.integers(1, 255, (NQ, 128)).astype(np.int16)
    y[:GROUP] = y[0]
    dist_next = np.full(NQ, 120)                      # the distance of a query's next copy: falls from copy to copy

    def copy_of(q, tie=False):
        if not tie:
            dist_next[q] -= 1
        row = y[q].copy()
        row[rng.choice(128, dist_next[q], replace=False)] += 1     # bytes 1..254: no saturation, the distance is exact
        return row

    # two copies of G and of every single in tiles 0..3, at scattered rows
    slots = rng.permutation(WARM_TILES * TILE)[:2 * (1 + NQ - GROUP)]
    for k, q in enumerate([0] + list(range(GROUP, NQ))):
        x[slots[2 * k]], x[slots[2 * k + 1]] = copy_of(q), copy_of(q)
    singles = list(range(GROUP, NQ - 1))              # the last single is never planted again
    for t, (a, b) in enumerate(PLANTS):
        row0 = (WARM_TILES + t) * TILE
        live = min(TILE, xrows - row0)
        assert a + 2 * b <= live + 1 and a <= len(singles)
        # odd and even positions alike: the copies of G at the odd rows from the top down, the singles from row 0 up
        pos_g = [live - 1 - 2 * i for i in range(b)]
        for i, r in enumerate(pos_g):
            x[row0 + r] = copy_of(0, tie=(i % 2 == 1))           # every second copy of G ties with the one before it
        for i, r in enumerate(sorted(set(range(live)) - set(pos_g))[:a]):
            x[row0 + r] = copy_of(singles[(i + 5 * t) % len(singles)])
    return x.astype(np.uint8), y.astype(np.uint8)


def tile_survivors(x, y, table):
    """Survivors of every tile after the warm ones, by the model: the differences between runs on truncated databases."""
    blocks, share = pc.blocks_of(SETTING), pc.share_of(SETTING)
    ends = [min(len(x), (WARM_TILES + t) * TILE) for t in range(len(PLANTS) + 1)]
    totals = [pm.run(x[:e], y, table, blocks, share)[2][1] for e in ends]
    return [int(b - a) for a, b in zip(totals, totals[1:])]


def run_case(which, oracle_fn):
    from spectavi_amd import device
    from tests.test_l1k2_bound_tuned import table_of
    from tests.test_l1k2_prune_gpu import _run
    table = table_of(which)
    x, y = make_data()
    plan = device.l1k2_plan(len(x), len(y), 128)
    assert plan["slices"] == 1 and (len(x) - 1) % TILE + 1 == LAST_ROWS, plan
    got = tile_survivors(x, y, table)
    assert got == WANT, (which, got, WANT)             # the tiles hold what they were built to hold
    oidx, odist = oracle_fn(x, y)
    midx, mdist, want = pm.run(x, y, table, pc.blocks_of(SETTING), pc.share_of(SETTING))
    assert np.array_equal(midx[:NQ], oidx) and np.array_equal(mdist[:NQ], odist)
    before = device.l1k2_get_bound()
    device.l1k2_set_bound(which)
    try:
        runs = [_run(x, y, 1), _run(x, y, 1), _run(x, y, 0)]
    finally:
        device.l1k2_set_bound(before)
    for what, (idx, dist, stats) in zip(("prune on", "prune on, second run", "prune off"), runs):
        print("table %d, %s: statistics %r, model %r" % (which, what, stats, want), flush=True)
        assert idx.tobytes() == oidx.tobytes() and dist.tobytes() == odist.tobytes(), (which, what)
    assert runs[0][2] == want and runs[1][2] == want and runs[2][2] == (0, 0, 0)
    # the ties: the two nearest copies of G are equally far, the lower row first
    assert odist[0][0] == odist[0][1] and oidx[0][0] < oidx[0][1]


def test_drain_boundaries_in_a_child_process():
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPECTAVI_L1K2_")}
    env.update(pc.SETTINGS[SETTING])
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    print(r.stdout)
    assert r.returncode == 0 and "drain boundaries ok: tables 0 and 1" in r.stdout, r.stdout


if __name__ == "__main__":
    from oracle import oracle as _oracle
    for _which in (0, 1):
        run_case(_which, _oracle.nn_bruteforcel1k2)
    print("drain boundaries ok: tables 0 and 1")
