"""The small-shape case table of the dim-128 bound path of the L1 2-NN (l1k2_prune.hip): every case names
its shape, the process setting it needs (SPECTAVI_L1K2_BLOCKS / SPECTAVI_L1K2_PRUNE_SHARE are read once
per process), the plan that setting must give it (slices, tiles of every slice, live rows of the last
tile) and, where they do not depend on timing, the statistics the path must report.

Used by tests/test_l1k2_prune_shapes_gpu.py (the cases on the GPU against the oracle, the plan asserted
through device.l1k2_plan() first) and by tests/test_l1k2_prune_model.py (the cases and the mutants of
tests/l1k2_prune_model.py on the CPU).

Why the statistics of most cases are known in advance.  The data recipes below are built on the bound's
tight byte pairs (p |a - b| + G(a, b) = m, read from spv_l1k2_bound_table, never hard-coded):
  * "cluster": the queries are a tight cluster around a pattern P of the two tight query bytes, "far"
    rows use the bytes that pair tightly with P, so their bound is (nearly) their true distance and
    rules them out as soon as a query has any second best among the near rows; "near" rows are P with
    a little noise, whose bound is negative: they always survive.  Two near rows stand at the head of
    every slice.  A workgroup without inherited thresholds keeps all of its tile 0 and, from tile 1
    on, exactly the near rows.
  * a slice whose tiles are all near rows exceeds the 3/4 share at its tile 4 (tile 1 if it starts
    with inherited thresholds) and is handed to the exact kernel; a slice with at most three near
    rows per tile never is, under either rule.  WHICH slices leave is therefore fixed; the tile at
    which one leaves, and the survivors of a tile 0, depend on whether another slice had published
    a threshold by then, so cases of several slices pin only `bounded` and `fallback`.
"""
import collections

import numpy as np

TILE = 32          # database rows per tile of the bound kernel
SLICE_UNIT = 64    # slices are whole tiles of the exact kernel (l1k2.hip), that is pairs of bound tiles: only
                   # the last slice of a plan can have an odd number of tiles
QBLOCK = 256
MAX_DIST = 128 * 255

# name -> the environment of the process that runs the cases of that setting.  "default" runs
# in the test process itself (16384 wanted blocks: every slice is 64 rows, the shortest there is).
SETTINGS = {
    "default": {},
    "one": {"SPECTAVI_L1K2_BLOCKS": "1"},
    "two": {"SPECTAVI_L1K2_BLOCKS": "2"},
    "three": {"SPECTAVI_L1K2_BLOCKS": "3"},
    "full": {"SPECTAVI_L1K2_BLOCKS": "1", "SPECTAVI_L1K2_PRUNE_SHARE": "1024"},
}
BREAK_EVEN_SHARE = 164     # kBreakEvenShare of l1k2_prune.hip, in 1/1024


def blocks_of(setting):
    return int(SETTINGS[setting].get("SPECTAVI_L1K2_BLOCKS", 16384))


def share_of(setting):
    return int(SETTINGS[setting].get("SPECTAVI_L1K2_PRUNE_SHARE", BREAK_EVEN_SHARE))


def plan_of(xrows, yrows, blocks):
    """(slices, slice_rows, query blocks of the bound kernel) as l1k2_plan() of l1k2.hip computes them
    at dim 128 with SPECTAVI_L1K2_BLOCKS = blocks.  The GPU test asserts the first two against the library."""
    q = 2
    while q > 1:
        if -(-yrows // (256 * q)) * max(1, xrows // TILE) >= 1024:
            break
        q //= 2
    qblocks = max(1, -(-yrows // (256 * q)))
    s_target = max(1, -(-blocks // qblocks))
    rows = -(-xrows // s_target)
    rows = min(max(-(-rows // SLICE_UNIT) * SLICE_UNIT, SLICE_UNIT), 65536)
    return max(1, -(-xrows // rows)), rows, -(-yrows // QBLOCK)


def shape_of(xrows, slices, slice_rows):
    """(tiles of every slice, live rows of the last tile of the last slice)."""
    tiles = tuple(-(-(min(xrows, (s + 1) * slice_rows) - s * slice_rows) // TILE) for s in range(slices))
    return tiles, (xrows - 1) % TILE + 1


# stats: (bounded, survivors, fallback pairs) as device.l1k2_prune_stats() must report them with the
# path forced on; None = that figure depends on timing (or on the data in no simple way) and is not pinned.
# path: False = the shape is below the path (fewer than 32 rows): statistics (0, 0, 0).
Case = collections.namedtuple("Case", "id setting xrows yrows kind arg slices tiles last_rows stats path")


def _case(setting, xrows, yrows, kind, arg=None, stats="auto", leave=(), tag=""):
    slices, slice_rows, qb = plan_of(xrows, yrows, blocks_of(setting))
    tiles, last = shape_of(xrows, slices, slice_rows)
    path = xrows >= TILE
    bounded = xrows * QBLOCK * qb
    if not path:
        stats = (0, 0, 0)
    elif leave:                                   # the slices that hand over, each with all of its rows
        rows = sum(min(xrows, (s + 1) * slice_rows) - s * slice_rows for s in leave)
        stats = (None, None, rows * QBLOCK * qb)
    elif stats == "free":                         # uniform bytes in several slices: a slice that starts with
        stats = (None, None, None)                # inherited thresholds may leave at its tile 1, another not
    elif stats == "auto":
        stats = (bounded, None, 0)
    elif stats == "all":                          # nothing can be ruled out and nobody leaves
        stats = (bounded, bounded, 0)
    elif stats == "near":                         # one slice: all of tile 0, then exactly the near rows
        near = near_rows(xrows, slices, slice_rows, arg)
        stats = (bounded, (min(TILE, xrows) + int(near[TILE:].sum())) * QBLOCK * qb, 0)
    cid = "%s-%dx%d-%s%s" % (setting, xrows, yrows, kind, tag)
    return Case(cid, setting, xrows, yrows, kind, arg, slices, tiles, last, stats, path)


def near_rows(xrows, slices, slice_rows, arg):
    """The near rows of the "cluster" / "zeroq" recipes: two at the head of every slice, one more in
    every later tile, the three rows that copy a query (see make_case), and every row of the slices
    listed in arg["leave"]."""
    near = np.zeros(xrows, bool)
    for s in range(slices):
        near[s * slice_rows:s * slice_rows + 2] = True
    t = np.arange(1, -(-xrows // TILE))
    r = TILE * t + (7 * t + 3) % TILE
    near[r[r < xrows]] = True
    for s in (arg or {}).get("leave", ()):
        near[s * slice_rows:(s + 1) * slice_rows] = True
    for r in _copy_rows(xrows):
        near[r] = True
    return near


def _copy_rows(xrows):
    """Rows that copy the queries N - 1, N // 2, 0: the last row (in the ragged tile), one in the middle, row 5."""
    return (xrows - 1, xrows // 2, 5) if xrows >= 64 else ()


QUERY_TAILS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300)
RAGGED = (1, 3, 4, 5, 8, 31)
TIGHT_PROBES = 8


def _build():
    cases = []
    # ---- loop phases: one slice of t tiles, t = 1..9, 12, 13; the ragged counts ride on t = 2..7,
    # once with ordinary (cluster) queries and once with queries next to the all-zero row
    for t, live in [(1, 32), (2, 1), (3, 3), (4, 4), (5, 5), (6, 8), (7, 31), (8, 32), (9, 17), (12, 32), (13, 9)]:
        x = TILE * (t - 1) + live
        cases.append(_case("one", x, 77, "cluster", stats="near"))
        if live in RAGGED:
            cases.append(_case("one", x, 70, "zeroq", stats="near"))
    # ---- query tails against a 5-tile slice (ragged: 5 live rows) ...
    for n in QUERY_TAILS:
        cases.append(_case("one", 4 * TILE + 5, n, "cluster", stats="near"))
    # ... and against a slice of one tile, where nothing has a threshold yet, in the test process itself
    for n in QUERY_TAILS:
        cases.append(_case("default", TILE, n, "uniform", stats="all"))
    for n in (65, 300):
        cases.append(_case("default", 70, n, "uniform", stats="free"))   # slices of 2 tiles and of one tile of 6 rows
    cases.append(_case("default", 65, 65, "uniform", stats="free"))      # a last slice of exactly one row
    cases.append(_case("default", 31, 65, "uniform"))            # below the path
    # ---- the second best, not the best, is the threshold: within a slice ...
    cases.append(_case("one", 3 * TILE, 40, "second"))
    # ---- two and three slices of 3, 4, 5, 8 tiles, full and ragged ends.  A slice that is not the last has an
    # even number of tiles (SLICE_UNIT): the odd counts are 4 + 3, 6 + 5 and 4 + 4 + 3, 6 + 6 + 5
    for x, n in ((195, 200), (237, 200), (351, 256), (488, 200)):
        cases.append(_case("two", x, n, "cluster"))
    for x, n in ((324, 200), (384, 200), (520, 256), (744, 200)):
        cases.append(_case("three", x, n, "cluster"))
    cases.append(_case("two", 65, 100, "cluster"))               # slices of 2 tiles and of one row
    cases.append(_case("two", 96, 100, "cluster"))               # ... and of one full tile
    cases.append(_case("three", 129, 100, "cluster"))            # 2, 2 tiles and one row
    cases.append(_case("three", 160, 100, "cluster"))            # 2, 2 tiles and one full tile
    # ... and across slices: what a slice publishes is its second best
    cases.append(_case("two", 6 * TILE, 40, "second"))
    # ---- hand-over placement (see the module docstring)
    cases.append(_case("two", 6 * TILE + 4 * TILE + 5, 65, "cluster", {"leave": (1,)}, leave=(1,), tag="-leave1"))   # at the last, ragged tile of a 5-tile slice
    cases.append(_case("two", 16 * TILE, 256, "cluster", {"leave": (0,)}, leave=(0,), tag="-leave0"))         # in mid-slice (tile 4 of 8)
    cases.append(_case("three", 15 * TILE - 29, 200, "cluster", {"leave": (1,)}, leave=(1,), tag="-leave1"))    # in mid-slice (tile 4 of 6)
    cases.append(_case("three", 24 * TILE - 7, 130, "cluster", {"leave": (1,), "ties": True}, leave=(1,), tag="-leave1-ties"))
    # ---- the keep rule at equality
    cases.append(_case("two", 2 * 64 * TILE, 40, "tight"))
    # ---- nothing pruned and no hand-over: every lane queues 32 survivors in every tile
    for x, n in ((8 * TILE + 17, 300), (13 * TILE, 64)):
        cases.append(_case("full", x, n, "constant", stats="all"))
        cases.append(_case("full", x, n, "nearconstant", stats="all"))
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), ids
    return cases


def tight_pairs(table):
    """[(database byte, query byte)] with p |a - b| + G(a, b) == m, the query byte the larger one."""
    phi, p, m = table
    a = np.arange(256, dtype=np.int64)
    slack = p * np.abs(a[:, None] - a[None, :]) + phi @ phi.T - m
    assert slack.min() == 0
    return [(int(i), int(j)) for i, j in np.argwhere(slack == 0) if i < j]


def make_case(case, table):
    """(x, y, expect): the case's data and {query: (two row indices)} that the recipe plants (checked on
    top of the comparison with the oracle).  table = (phi int64 [256, 4], p, m) from spv_l1k2_bound_table."""
    xrows, yrows, kind, arg = case.xrows, case.yrows, case.kind, case.arg or {}
    rng = np.random.default_rng([xrows, yrows, len(kind), ord(kind[0]), len(case.setting)])
    slice_rows = plan_of(xrows, yrows, blocks_of(case.setting))[1]
    expect = {}
    if kind == "uniform":
        x = rng.integers(0, 256, (xrows, 128), dtype=np.uint8)
        y = rng.integers(0, 256, (yrows, 128), dtype=np.uint8)
    elif kind in ("cluster", "zeroq"):
        def noisy(center, rows, npos, lo, hi):
            out = np.repeat(center[None, :], rows, axis=0).astype(np.int16)
            for r in range(rows):
                out[r, rng.choice(128, npos, replace=False)] += rng.integers(lo, hi + 1, npos)
            return out
        if kind == "cluster":
            pairs = tight_pairs(table)
            pick = rng.integers(0, len(pairs), 128)
            far_c = np.array([pairs[i][0] for i in pick])
            near_c = np.array([pairs[i][1] for i in pick])
            y = noisy(near_c, yrows, 8, -3, -1)
            xn, xf = noisy(near_c, xrows, 12, -3, -1), noisy(far_c, xrows, 6, 0, 2)
        else:   # queries a few units from the all-zero row, their true neighbours more than 128 m / p away
            p, m = table[1], table[2]
            near_b = 128 * m // (128 * p) + 12
            assert 128 * near_b > 128 * m // p + 128 and near_b < 200
            y = noisy(np.zeros(128, np.int64), yrows, 5, 1, 2)
            xn = noisy(np.full(128, near_b), xrows, 10, 0, 2)
            xf = noisy(np.full(128, 250), xrows, 10, 0, 3)
        near = near_rows(xrows, case.slices, slice_rows, arg)
        x = np.where(near[:, None], xn, xf)
        for r, k in zip(_copy_rows(xrows), (yrows - 1, yrows // 2, 0)):
            if kind == "cluster":
                x[r] = y[k]
        if arg.get("ties"):
            # identical rows in the slice that leaves (1) and in those that stay (0, 2): the partial pairs of
            # these queries come from both kernels and tie at distance 0
            a, b, c = slice_rows // 2, slice_rows + 6 * TILE + 9, 2 * slice_rows + 70
            x[a], x[b] = y[3], y[3]
            x[b + 40], x[c], x[c + 33] = y[yrows - 2], y[yrows - 2], y[yrows - 2]
            expect = {3: (a, b), yrows - 2: (b + 40, c)}
        x, y = x.astype(np.uint8), y.astype(np.uint8)
    elif kind in ("tight", "second"):
        far_b, q_b = min(ab for ab in tight_pairs(table) if ab[0] >= 4)
        assert q_b - far_b > 128                      # bytes below far_b are strictly farther than the tight distance
        y = np.full((yrows, 128), q_b, np.uint8)
        x = rng.integers(0, 2, (xrows, 128)).astype(np.uint8)         # bytes 0 / 1: farther than every row below
        if kind == "tight":
            # slice 0: two rows one unit per byte farther than tight at its head (its own threshold), tight rows
            # in its last two tiles; slice 1 begins with tight rows and publishes the tight distance early
            x[0:2] = far_b - 1
            rows = [slice_rows - 2 * TILE + 7, slice_rows - 2 * TILE + 30, slice_rows - TILE + 4,
                    slice_rows - TILE + 5, slice_rows - 1]
            x[rows] = far_b
            x[slice_rows:slice_rows + 4] = far_b
            # witnesses of the timing, without influence on the result: rows half a unit per byte farther than
            # tight in tiles 40..47 of slice 0.  Its own threshold keeps them, the tight distance inherited from
            # slice 1 rules them out: TIGHT_PROBES * 256 more survivors mean that it had not arrived by then
            for i in range(TIGHT_PROBES):
                x[(40 + i) * TILE + 3 + i, :64] = far_b
                x[(40 + i) * TILE + 3 + i, 64:] = far_b - 1
            expect = {k: (rows[0], rows[1]) for k in (0, yrows // 2, yrows - 1)}
        else:
            # the best row first, a poor second best next to it; the true second best and a third come later (in
            # the next slice if there is one): their bounds lie between the best and the second best so far
            x[0], x[1] = far_b, far_b - 3
            later = slice_rows if case.slices > 1 else 2 * TILE + 8
            x[later], x[later + 1] = far_b - 1, far_b - 2
            expect = {k: (0, later) for k in (0, yrows - 1)}
    elif kind == "constant":
        x = np.full((xrows, 128), 93, np.uint8)
        y = np.full((yrows, 128), 93, np.uint8)
        y[::7] = 94
        expect = {k: (0, 1) for k in (0, 7, yrows - 1)}
    elif kind == "nearconstant":
        # every row is equally far from every query (byte 0 is 93 in the queries, 92 or 94 in the rows), but for
        # rows 0 and 1 of tile 0, which are farther: nothing is ever ruled out, and rows 2, 3 win the ties
        x = np.full((xrows, 128), 93, np.uint8)
        x[:, 0] = 92 + 2 * (np.arange(xrows) % 2)
        x[0:2] = 90
        y = rng.integers(92, 95, (yrows, 128)).astype(np.uint8)
        y[:, 0] = 93
        expect = {k: (2, 3) for k in (0, yrows // 2, yrows - 1)}
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x), np.ascontiguousarray(y), expect


CASES = _build()


def cases_of(setting):
    return [c for c in CASES if c.setting == setting]
