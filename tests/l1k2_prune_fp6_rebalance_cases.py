"""Data for tests/test_l1k2_prune_fp6_rebalance_gpu.py: the small shapes at which moving the arming of a tile's accumulators
from the end of the compare of the tile before into the tile's own top (l1k2_prune_wide6_kernel) could go wrong.  Built
from the FP6 table's own tight pairs, read from the library and never hard-coded; every recipe checks on the CPU, against
the table and the model of tests/l1k2_prune_fp6_model.py, that its data does what its name says, before anything runs.

  * SHAPES: one 64-row tile alone (armed once, at tile 0), and two and three tiles ragged in either row half, with the
    "cluster" recipe of tests/l1k2_prune_cases.py;
  * lowering(table, t): every query is the query byte q of one tight pair (far, q); a row of "level" j has j bytes far - 1
    and the rest far.  Tile 0 holds two rows of level HIGH, tile t two of level LOW, tile t + 1 three PROBE rows, in either
    row half; all other rows are far away.  Under the second best that tile 0 left (the threshold a stale arming of tile
    t + 1 would use) the probes survive, under the one that tile t's drain leaves they are ruled out: the model counts no
    survivor in tile t + 1, a stale k2s[] shows as 3 per query above it;
  * leaving(table, wave, tile): the 64 queries of one wave are all equally far from the rows they keep, so nothing ever rules
    those rows out for them, and their counts per tile are chosen so that the wave's running share passes 3/4 exactly at
    `tile` (3 or 4); the other waves rule every such row out and never raise the flag."""
import numpy as np

from tests import l1k2_prune_cases as pc
from tests import l1k2_prune_fp6_model as fm
from tests import l1k2_prune_wide_cases as wc

TILE = wc.TILE
SHAPES = ((64, 256), (65, 300), (97, 511), (129, 513), (161, 700))
LOWERING = (1, 2)                    # the tile whose drain lowers the second best: odd and even
LEAVING = ((1, 3), (6, 3), (2, 4), (5, 4))   # (the wave that raises the flag, at which tile): either half of the workgroup
HIGH, LOW, PROBE = 128, 10, 100
PROBE_ROWS = (3, 35, 60)
KEEP_PART = 47                       # rows of tiles 2 and 3 that the leaving wave keeps where it is to leave at tile 4


def shape_cases():
    return [wc._case("one", x, n, "cluster") for x, n in SHAPES]


def _pair(table):
    """(far, q): a tight pair with room below far for the levels and rows that are far from q under the bound too."""
    k, p, m = table
    G = k @ k.T
    for far, q in pc.tight_pairs(table):
        lb = (m - G[:, q]) / p          # the bound's share of one byte, in units of distance
        if far >= 8 and q - far > 128 and 0 < lb[far - 1] - lb[far] <= 1 and lb[:4].min() > lb[far] + 8:
            return far, q
    raise AssertionError("no tight pair of the table fits the recipe")


def _tq(table, second):
    return 128 * table[2] - table[1] * min(second, pc.MAX_DIST)


def lowering(table, t, yrows=700):
    """(x, y, the tile that must hold no survivor)."""
    far, q = _pair(table)
    rng = np.random.default_rng([t, yrows, 61])
    xrows = (t + 2) * TILE + 9        # one more, ragged tile behind the probes
    y = np.full((yrows, 128), q, np.uint8)
    x = rng.integers(0, 4, (xrows, 128)).astype(np.uint8)

    def level(j):
        row = np.full(128, far, np.uint8)
        row[:j] = far - 1
        return row
    x[0], x[1] = level(HIGH), level(HIGH)
    x[t * TILE + 7], x[t * TILE + 40] = level(LOW), level(LOW)
    probes = [(t + 1) * TILE + o for o in PROBE_ROWS]
    x[probes] = level(PROBE)
    # what the recipe claims, from the table: the probes are kept under tile 0's second best and ruled out under tile t's
    d0 = 128 * (q - far)
    _, gsum, _ = fm.prepare(x, y, table)
    assert (gsum[probes][:, 0] >= _tq(table, d0 + HIGH)).all() and (gsum[probes][:, 0] < _tq(table, d0 + LOW)).all()
    per_tile = []
    fm.run(x, y, table, 1, pc.BREAK_EVEN_SHARE, per_tile=per_tile)
    surv = {(qb, tl): n for qb, s, tl, n in per_tile}
    assert all(surv[(qb, t + 1)].sum() == 0 for qb in range(-(-yrows // wc.QBLOCK))), surv
    assert surv[(0, t)].sum() == 2 * min(yrows, wc.QBLOCK)
    return x, y, t + 1


def leaving(table, wave, tile, yrows=512):
    """(x, y, the tile at which the model leaves): wave `wave` of the one workgroup passes the 3/4 share at `tile`."""
    assert tile in (3, 4)
    far, q = _pair(table)
    rng = np.random.default_rng([wave, tile, 67])
    xrows = 7 * TILE + 5
    z = 2                             # the leaving wave's queries and the rows they keep: byte z, all ties
    y = np.full((yrows, 128), q, np.uint8)
    y[64 * wave:64 * wave + 64] = z
    x = np.full((xrows, 128), far + 4, np.uint8)     # far from z, and behind `far` for q: ruled out by both once they have a second best
    x[0], x[1] = far, far
    x[2], x[3] = z, z
    keep = {2: TILE if tile == 3 else KEEP_PART, 3: TILE if tile == 3 else KEEP_PART, 4: TILE}
    for tl, n in keep.items():
        rows = tl * TILE + rng.permutation(TILE)[:n]
        x[rows] = z
    per_tile = []
    stats = fm.run(x, y, table, 1, pc.BREAK_EVEN_SHARE, per_tile=per_tile)[2]
    assert len(per_tile) == tile + 1 and stats[2] == xrows * wc.QBLOCK, (len(per_tile), stats)
    last = per_tile[-1][3]
    assert last[wave] == keep[tile] * 64 and np.delete(last, wave).max() == 0, last
    return x, y, tile
