"""The collections tests/test_l1k2_batch_plan.py (host only) and tests/test_l1k2_batch_gpu.py share, and which
kernel instantiation (row width, queries per lane) the planner gives each: the plan test asserts these, so a
retuned planner that leaves an instantiation of l1k2_batch_kernel without a case fails without a GPU."""
import numpy as np

NINE = [0, 1, 2, 63, 64, 65, 257, 513, 1000]          # rows of the nine-set collection
ALL81 = [(a, b) for a in range(9) for b in range(9)]   # every ordered pair, self pairs included
# fewer pairs over the same sets: every set as query and as database, the empty and one-row databases, a self pair
FEW = [(8, 0), (8, 1), (7, 8), (6, 7), (5, 6), (4, 5), (3, 4), (2, 3), (1, 2), (0, 8), (8, 8), (7, 2), (6, 8)]

DIMS = tuple(range(16, 257, 16))


def library_instantiations():
    """The (row width, queries per lane) pairs l1k2_batch_kernel ships in, asked of the library itself (host only):
    the widths are the dim_pad of every dim the call takes, and a width's Q values are the powers of two up to the q a
    collection that fills the chip at any q gets (l1k2_tile.h: TileWidths, max_q_for)."""
    from spectavi_amd import device
    inst = set()
    for dim in DIMS:
        plan = device.l1k2_batch_plan(seg_of([70000, 70000]), [(1, 0)], dim)
        inst |= {(plan["dim_pad"], q) for q in (1, 2, 4) if q <= plan["q"]}
    return inst


def width_of(dim):
    from spectavi_amd import device
    return device.l1k2_batch_plan(seg_of([1, 1]), [(1, 0)], dim)["dim_pad"]


def seg_of(rows):
    return np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)


# (name, set rows, pairs, dim, queries per lane the planner must pick, database rows of the plan's longest item)
#   q = 1: too few (query block, 64-row slice) groups to fill the chip even at one query per lane
#   q = 2 at widths <= 64: 40000 / 64 = 625 possible slices; one query block at q = 4, two at q = 2 (>= 1024 groups)
#   q = max: 70000 / 64 = 1093 possible slices fill the chip with one query block
# A collection of fewer than 1024 whole-set items is cut down to 64-row slices, one LDS tile per item: the cases
# above reach every instantiation, but none of them swaps the double buffer or has a tile-local base above 0.
#   tiles-*: 1024 times the same pair fill the chip, so the 4096-row floor holds: items of 4096 and 904 database
#            rows, 64 and 15 tiles, the last one ragged (8 rows); 300 queries are two ragged query blocks at q = 1.
#            The planner gives such a collection the largest q; tests/l1k2_batch_child.py runs the same cases
#            under SPECTAVI_L1K2_Q = 1 and 2 (read once per process), which is the only way to the smaller q there.
#   maxslice: 16384 times the same pair: no cut at all, so the 70000-row set is one item of 65536 rows, the limit of
#            the 16-bit local index, and one of 4464.
NARROW = (16, 32, 48, 64)
Q_CASES = ([("nine-%d" % d, NINE, FEW, d, 1, 64) for d in DIMS if d != 128]
           + [("nine-128", NINE, ALL81, 128, 1, 64)]
           + [("mid-%d" % d, [40000, 600], [(1, 0)], d, 2, 64) for d in NARROW]
           + [("long-%d" % d, [70000, 257], [(1, 0)], d, 4 if d in NARROW else 2, 64) for d in DIMS]
           + [("tiles-%d" % d, [5000, 300], [(1, 0)] * 1024, d, 4 if d in NARROW else 2, 4096) for d in DIMS]
           + [("maxslice-16", [70000, 3], [(1, 0)] * 16384, 16, 4, 65536)])
TILE_CASES = [c for c in Q_CASES if c[0].startswith("tiles-")]
