"""A plain numpy statement of what the dim-128 bound path of the L1 2-NN (l1k2_prune.hip) decides, and
named mutants of it.  No timing is modelled: a run takes a schedule instead ("up": the slices one after
the other in ascending order, each seeing all that the earlier ones published; "down": descending;
"blind": no slice ever sees another's thresholds), and a correct path gives the oracle's bytes under
every one of them.

What is stated: the features from the table; the exact integer sum; keep iff sum >= 128 m - p min(thr,
32640); per (query lane, slice) a top-2 of dist << 32 | row keys over the kept rows of the live rows of
every tile; thr = min(the lane's running second best, the shared threshold read last: before the loop
and again at tiles 3, 7, ...); publication of the second best at tiles 0, 4, ... and when the workgroup
ends or leaves; the survivor-share rule by which a workgroup leaves, after which its slice is recomputed
exactly; the lexicographic merge of the slice partials; lanes past the last query working on a copy of
the last query without ever storing.  The statistics are those of l1k2_prune_stats().

tests/test_l1k2_prune_model.py runs the case table through it; the GPU runs the same table."""
import numpy as np

from tests.l1k2_prune_cases import MAX_DIST, QBLOCK, TILE, plan_of

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_THR = 0xFFFFFFFF
SHARE_UNIT = 1024

# name -> what the mutant does wrong
MUTANTS = {
    "skip_on_equality": "a pair is kept only if sum > 128 m - p thr",
    "padding_unmasked": "the zero rows past the end of a ragged last tile are not masked out",
    "thr_from_best": "the lane's own threshold is its best distance, not its second best",
    "published_from_best": "the threshold a workgroup publishes is its best distance",
    "filter_le": "the survivor filter passes key <= k2 instead of key < k2",
    "filter_dist_strict": "the survivor filter compares distances only: passes dist < second-best dist",
    "phantom_store": "lanes past the last query store their partial pairs",
}
# filter_le changes nothing: the keys of a slice are distinct (the row is in them), and k2 is one of them
# or "none", so key == k2 never happens.  The test asserts that it is inert instead of pretending that a
# case catches it; filter_dist_strict is the neighbouring mistake that does change results.
INERT = ("filter_le",)

SCHEDULES = ("up", "down", "blind")


def features(table, rows):
    """[rows, 512] int64: phi of every byte."""
    return table[0][rows].reshape(len(rows), -1)


def _tile_order():
    """The order in which one query's rows of a tile reach the exact evaluation: a lane holds the rows
    8 (v / 4) + 4 g + v % 4, v = 0..15, of half g, and queues them in ascending v, both halves a round."""
    v = np.arange(16)
    rows = 8 * (v // 4) + v % 4
    return np.stack([rows, rows + 4], axis=1).reshape(-1)


ORDER = _tile_order()


def _top2_insert(k1, k2, key, take):
    """old = min(k1, key); k2 = min(k2, max(old, key)) on the lanes in `take`."""
    lo = np.minimum(k1, key)
    hi = np.minimum(k2, np.maximum(k1, key))
    return np.where(take, lo, k1), np.where(take, hi, k2)


def prepare(x, y, table):
    """What every run on the same data shares: the exact distances [M, N], the feature sums [M, N] and the
    distance of every query to a zero padding row."""
    dist = np.abs(x.astype(np.int16)[:, None, :] - y.astype(np.int16)[None, :, :]).sum(axis=2, dtype=np.int64)
    return dist, features(table, x) @ features(table, y).T, y.astype(np.int64).sum(axis=1)


def run(x, y, table, blocks, share, schedule="up", mutant=None, pre=None):
    """(idx uint64 [Q, 2], dist int32 [Q, 2], (bounded, survivors, fallback)) with Q = the query count
    rounded up to whole workgroups: the rows past the last query must stay "none" (idx = 2^64 - 1)."""
    assert schedule in SCHEDULES and (mutant is None or mutant in MUTANTS)
    phi, p, m = table
    M, N = len(x), len(y)
    dist, gsum, ysum = pre or prepare(x, y, table)
    S, slice_rows, qblocks = plan_of(M, N, blocks)
    m128 = 128 * m
    thr = np.full(N, NO_THR, np.int64)
    part = np.full((qblocks * QBLOCK, S, 2), NONE, np.uint64)
    stats = [0, 0, 0]

    def publish(q, live, value, seen_now):
        ok = live & (value < seen_now)
        np.minimum.at(thr, q[ok], value[ok])

    for qb in range(qblocks):
        lane_q = qb * QBLOCK + np.arange(QBLOCK)
        live = lane_q < N
        q = np.minimum(lane_q, N - 1)
        for s in (range(S) if schedule != "down" else range(S - 1, -1, -1)):
            row_begin, row_end = s * slice_rows, min(M, (s + 1) * slice_rows)
            ntiles = -(-(row_end - row_begin) // TILE)
            k1 = np.full(QBLOCK, NONE, np.uint64)
            k2 = np.full(QBLOCK, NONE, np.uint64)
            blind = schedule == "blind"
            seen = np.full(QBLOCK, NO_THR, np.int64) if blind else thr[q].copy()
            inherited = (seen.reshape(4, 64) != NO_THR).any(axis=1)           # per wave
            warm = np.where(inherited, 8, 256)
            skip_tiles = np.where(inherited, 0, 3)
            recent = np.zeros(4, np.int64)
            n_bound = n_surv = 0
            gave_up = False
            for tl in range(ntiles):
                row0 = row_begin + tl * TILE
                nrows = min(TILE, row_end - row0)
                best = (k1 >> np.uint64(32)).astype(np.int64)
                second = (k2 >> np.uint64(32)).astype(np.int64)
                loc = best if mutant == "thr_from_best" else second
                tq = m128 - p * np.minimum(np.minimum(loc, seen), MAX_DIST)
                if tl % 4 == 0:
                    publish(q, live, best if mutant == "published_from_best" else second, seen)
                if tl % 4 == 3 and not blind:
                    seen = thr[q].copy()
                # the tile: 32 rows, those past the end of the slice are zero rows with zero features
                sums = np.zeros((TILE, QBLOCK), np.int64)
                dists = np.repeat(ysum[q][None, :], TILE, axis=0)
                sums[:nrows] = gsum[row0:row0 + nrows][:, q]
                dists[:nrows] = dist[row0:row0 + nrows][:, q]
                keep = (sums > tq) if mutant == "skip_on_equality" else (sums >= tq)
                if mutant != "padding_unmasked":
                    keep[nrows:] = False
                keys = (dists.astype(np.uint64) << np.uint64(32)) | (row0 + np.arange(TILE, dtype=np.uint64))[:, None]
                if mutant in ("filter_le", "filter_dist_strict"):
                    for i in ORDER:
                        if mutant == "filter_le":
                            take = keep[i] & (keys[i] <= k2)
                        else:
                            take = keep[i] & ((keys[i] >> np.uint64(32)) < (k2 >> np.uint64(32)))
                        k1, k2 = _top2_insert(k1, k2, keys[i], take)
                else:
                    allk = np.concatenate([k1[None], k2[None], np.where(keep, keys, NONE)])
                    allk.sort(axis=0)
                    k1, k2 = allk[0], allk[1]
                tile_surv = keep.reshape(TILE, 4, 64).sum(axis=(0, 2))        # per wave
                n_bound += nrows * QBLOCK
                n_surv += int(tile_surv.sum())
                recent = np.where(tl <= skip_tiles, 8 * tile_surv, recent + tile_surv - (recent >> 3))
                limit = np.where(tl >= warm, share, np.where(tl > skip_tiles, max(share, SHARE_UNIT * 3 // 4), SHARE_UNIT))
                if (recent * (SHARE_UNIT // 8) > limit * (TILE * 64)).any():
                    gave_up = True
                    break
            best = (k1 >> np.uint64(32)).astype(np.int64)
            second = (k2 >> np.uint64(32)).astype(np.int64)
            publish(q, live, best if mutant == "published_from_best" else second, thr[q])
            stats[0] += n_bound
            stats[1] += n_surv
            if gave_up:   # the exact kernel computes the slice from scratch
                stats[2] += (row_end - row_begin) * QBLOCK
                keys = (dist[row_begin:row_end][:, q].astype(np.uint64) << np.uint64(32)) | \
                    np.arange(row_begin, row_end, dtype=np.uint64)[:, None]
                keys = np.concatenate([keys, np.full((2, QBLOCK), NONE, np.uint64)])
                keys.sort(axis=0)
                k1, k2 = keys[0], keys[1]
            stores = np.ones(QBLOCK, bool) if mutant == "phantom_store" else live
            part[lane_q[stores], s, 0] = k1[stores]
            part[lane_q[stores], s, 1] = k2[stores]

    merged = np.sort(part.reshape(len(part), -1), axis=1)[:, :2]
    idx = np.where(merged == NONE, NONE, merged & np.uint64(0xFFFFFFFF))
    d = np.where(merged == NONE, np.uint64(0x7FFFFFFF), merged >> np.uint64(32)).astype(np.int32)
    return idx, d, tuple(stats)
