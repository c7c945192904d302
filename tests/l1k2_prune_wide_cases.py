"""The small-shape case table of the wide form of the bound kernel (l1k2_prune_wide_kernel: 64-row tiles, 512-query
workgroups), for tests/test_l1k2_prune_wide_model.py (CPU, the model of tests/l1k2_prune_wide_model.py) and
tests/test_l1k2_prune_wide_gpu.py.  Settings, plans and the data recipes "cluster", "uniform", "second", "tight",
"constant" and "nearconstant" are those of tests/l1k2_prune_cases.py, imported and not edited; what is added here:

  * "planted": two clusters of queries, A around the query bytes of tight pairs and B around their partners, so that
    a row near one cluster is (nearly) tightly far from the other.  Wave w of the one workgroup holds A_PER_WAVE[w]
    queries of A, and tile t >= 1 holds PLANT[t - 1] = (rows near A, rows near B): the wave keeps exactly
    nA a + nB (64 - a) pairs of it.  Over waves and tiles that gives every count of WANTED_COUNTS.  One tile has
    its two A rows 32 apart: two survivors in one lane, for the queries c and 32 + c of a lane alike.
  * "ties": the cluster recipe with rows that copy a query twice: both in one half of a tile, in its two halves,
    and in two tiles."""
import collections

import numpy as np

from tests import l1k2_prune_cases as pc

TILE = 64
QBLOCK = 512
A_PER_WAVE = (1, 7, 8, 9, 16, 17, 63, 32)
PLANT = ((0, 0), (1, 0), (0, 1), (1, 1), (2, 1), (4, 3))
WANTED_COUNTS = (0, 1, 7, 8, 9, 16, 17, 63, 64, 65, 200)
DB_ROWS = (32, 33, 63, 64, 65, 127, 128, 129) + tuple(64 * t + d for t in (2, 3) for d in (1, 31, 33, 63))
QUERIES = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 700)

WideCase = collections.namedtuple("WideCase", "id setting xrows yrows kind base")


def _case(setting, xrows, yrows, kind, arg=None, tag=""):
    base_kind = {"ties": "cluster", "planted": "cluster"}.get(kind, kind)
    base = pc._case(setting, xrows, yrows, base_kind, arg)
    return WideCase("wide-%s-%dx%d-%s%s" % (setting, xrows, yrows, kind, tag), setting, xrows, yrows, kind, base)


def plan(case):
    """(slices, slice_rows, wide tiles of every slice, workgroups of 512 queries)."""
    slices, slice_rows, _ = pc.plan_of(case.xrows, case.yrows, pc.blocks_of(case.setting))
    tiles = tuple(-(-(min(case.xrows, (s + 1) * slice_rows) - s * slice_rows) // TILE) for s in range(slices))
    return slices, slice_rows, tiles, -(-case.yrows // QBLOCK)


def _build():
    cases = []
    # ragged tiles in either half, at even and odd tiles, one slice; the query counts ride along
    for i, x in enumerate(DB_ROWS):
        cases.append(_case("one", x, QUERIES[i % len(QUERIES)], "cluster"))
    for n in QUERIES[len(DB_ROWS) % len(QUERIES):]:
        cases.append(_case("one", 3 * TILE + 5, n, "cluster"))
    cases.append(_case("one", TILE * (1 + len(PLANT)), QBLOCK, "planted"))
    cases.append(_case("one", 5 * TILE + 9, 200, "ties"))
    cases.append(_case("one", 3 * TILE, 40, "second"))
    # workgroups that leave under the shipped share: the second block of 256 partly filled; a workgroup of one query
    cases.append(_case("one", 10 * TILE, 300, "constant"))
    cases.append(_case("one", 6 * TILE + 3, 513, "constant"))
    # several slices of one tile each, in the test process itself
    cases.append(_case("default", 200, 700, "uniform"))
    cases.append(_case("default", 321, 513, "cluster"))
    # two and three slices of 2..5 wide tiles.  The plan cuts SPECTAVI_L1K2_BLOCKS / (query blocks of 256) slices: "two"
    # gives two up to 256 queries, "three" three up to 256 and two up to 512
    for x, n in ((256, 200), (379, 255), (479, 256), (623, 65)):
        cases.append(_case("two", x, n, "cluster"))
    cases.append(_case("two", 6 * 32, 40, "second"))
    cases.append(_case("two", 2 * 64 * 32, 40, "tight"))
    for x, n in ((567, 64), (959, 255), (379, 300), (623, 512)):
        cases.append(_case("three", x, n, "cluster"))
    # nothing pruned and nobody leaves: every wave queues all 4096 pairs of every tile
    cases.append(_case("full", 8 * TILE + 17, 300, "constant"))
    cases.append(_case("full", 4 * TILE + 40, 513, "nearconstant"))
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), ids
    return cases


def make_case(case, table):
    """(x, y, expect) as tests/l1k2_prune_cases.make_case."""
    if case.kind not in ("planted", "ties"):
        return pc.make_case(case.base, table)
    if case.kind == "ties":
        x, y, expect = pc.make_case(case.base, table)
        expect = dict(expect)
        for k, (a, b) in {3: (70, 75), 5: (2 * TILE + 2, 2 * TILE + 42), 7: (3 * TILE + 8, 4 * TILE + 4)}.items():
            x[a], x[b] = y[k], y[k]
            expect[k] = (a, b)
        return x, y, expect
    rng = np.random.default_rng([case.xrows, case.yrows, 17])
    pairs = pc.tight_pairs(table)
    pick = rng.integers(0, len(pairs), 128)
    b_c = np.array([pairs[i][0] for i in pick])     # cluster B: the smaller bytes
    a_c = np.array([pairs[i][1] for i in pick])     # cluster A: their tight partners

    def noisy(center, rows, npos, sign):
        out = np.repeat(center[None, :], rows, axis=0).astype(np.int16)
        for r in range(rows):
            out[r, rng.choice(128, npos, replace=False)] += sign * rng.integers(1, 4, npos)
        return out
    in_a = np.zeros(case.yrows, bool)
    for w, a in enumerate(A_PER_WAVE):
        in_a[64 * w:64 * w + a] = True
    y = np.where(in_a[:, None], noisy(a_c, case.yrows, 8, -1), noisy(b_c, case.yrows, 8, +1))
    near_a = np.zeros(case.xrows, bool)
    near_b = np.zeros(case.xrows, bool)
    near_a[0:2] = True                               # tile 0: two rows of either cluster, every query has a second best
    near_b[2:4] = True
    for t, (na, nb) in enumerate(PLANT, start=1):
        offs_a = (5, 37, 50, 63)[:na]                # 5 and 37: one lane's rows in the two halves
        offs_b = (0, 31, 32)[:nb]
        near_a[[TILE * t + o for o in offs_a]] = True
        near_b[[TILE * t + o for o in offs_b]] = True
    xa, xb = noisy(a_c, case.xrows, 12, -1), noisy(b_c, case.xrows, 12, +1)
    # every other row is far from both clusters and tightly so from neither: bytes 0 / 255 on the far side of each pair
    far = np.where(rng.random((case.xrows, 128)) < 0.5, 0, 255)
    x = np.where(near_a[:, None], xa, np.where(near_b[:, None], xb, far))
    return np.ascontiguousarray(x.astype(np.uint8)), np.ascontiguousarray(y.astype(np.uint8)), {}


def planted_counts():
    """{(wave, tile): survivors} the "planted" case is built for, tiles 1..len(PLANT)."""
    return {(w, t): na * a + nb * (64 - a) for w, a in enumerate(A_PER_WAVE) for t, (na, nb) in enumerate(PLANT, start=1)}


CASES = _build()


def cases_of(setting):
    return [c for c in CASES if c.setting == setting]
