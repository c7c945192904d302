"""A plain numpy statement of what the wide form of the bound kernel (l1k2_prune_wide_kernel of l1k2_prune.hip)
decides, beside tests/l1k2_prune_model.py, which states the narrow form: tiles of 64 rows, workgroups of 8 waves
of 64 queries, and what the narrow form counts in tiles kept in rows.

  * thr = min(the lane's running second best, the shared threshold read last: before the loop and again at
    tiles 1, 3, ...); the second best is published at tiles 0, 2, ... and when the workgroup ends or leaves;
  * the share rule per wave with the tile's 64 x 64 pairs as denominator, judged at the break-even share from
    tile 4 on with inherited thresholds and from tile 128 on without (3/4 before, nothing in tiles 0..2 then);
  * a workgroup that leaves has its slice recomputed exactly for its two query blocks of 256: `fallback` counts
    the slice's rows x 512.

Schedules as in the narrow model ("up", "down", "blind"); a correct path gives the oracle's bytes under each."""
import numpy as np

from tests.l1k2_prune_cases import MAX_DIST, plan_of
from tests.l1k2_prune_model import NO_THR, NONE, SCHEDULES, SHARE_UNIT, prepare  # noqa: F401  (prepare: for callers)

TILE = 64
WAVES = 8
QBLOCK = 64 * WAVES
THR_EVERY = 2
WARM_SHARED, WARM_ALONE, SKIP_ALONE = 4, 128, 2


def run(x, y, table, blocks, share, schedule="up", pre=None, per_tile=None):
    """(idx uint64 [Q, 2], dist int32 [Q, 2], (bounded, survivors, fallback)) with Q = the query count rounded up
    to whole workgroups of 512.  per_tile, if a list, receives (query block, slice, tile, survivors of each wave)."""
    assert schedule in SCHEDULES
    phi, p, m = table
    M, N = len(x), len(y)
    dist, gsum, _ = pre or prepare(x, y, table)
    S, slice_rows, _ = plan_of(M, N, blocks)
    qblocks = -(-N // QBLOCK)
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
            k1 = np.full(QBLOCK, NONE, np.uint64)
            k2 = np.full(QBLOCK, NONE, np.uint64)
            blind = schedule == "blind"
            seen = np.full(QBLOCK, NO_THR, np.int64) if blind else thr[q].copy()
            inherited = (seen.reshape(WAVES, 64) != NO_THR).any(axis=1)
            warm = np.where(inherited, WARM_SHARED, WARM_ALONE)
            skip_tiles = np.where(inherited, 0, SKIP_ALONE)
            recent = np.zeros(WAVES, np.int64)
            gave_up = False
            for tl in range(-(-(row_end - row_begin) // TILE)):
                row0 = row_begin + tl * TILE
                nrows = min(TILE, row_end - row0)
                second = (k2 >> np.uint64(32)).astype(np.int64)
                tq = 128 * m - p * np.minimum(np.minimum(second, seen), MAX_DIST)
                if tl % THR_EVERY == 0:
                    publish(q, live, second, seen)
                if tl % THR_EVERY == THR_EVERY - 1 and not blind:
                    seen = thr[q].copy()
                keep = gsum[row0:row0 + nrows][:, q] >= tq      # rows past the end of a ragged tile are never kept
                keys = (dist[row0:row0 + nrows][:, q].astype(np.uint64) << np.uint64(32)) | \
                    (row0 + np.arange(nrows, dtype=np.uint64))[:, None]
                allk = np.concatenate([k1[None], k2[None], np.where(keep, keys, NONE)])
                allk.sort(axis=0)
                k1, k2 = allk[0], allk[1]
                tile_surv = keep.reshape(nrows, WAVES, 64).sum(axis=(0, 2))
                if per_tile is not None:
                    per_tile.append((qb, s, tl, tile_surv.copy()))
                stats[0] += nrows * QBLOCK
                stats[1] += int(tile_surv.sum())
                recent = np.where(tl <= skip_tiles, 8 * tile_surv, recent + tile_surv - (recent >> 3))
                limit = np.where(tl >= warm, share, np.where(tl > skip_tiles, max(share, SHARE_UNIT * 3 // 4), SHARE_UNIT))
                if (recent * (SHARE_UNIT // 8) > limit * (TILE * 64)).any():
                    gave_up = True
                    break
            publish(q, live, (k2 >> np.uint64(32)).astype(np.int64), thr[q])
            if gave_up:   # the exact kernel computes the slice from scratch
                stats[2] += (row_end - row_begin) * QBLOCK
                keys = (dist[row_begin:row_end][:, q].astype(np.uint64) << np.uint64(32)) | \
                    np.arange(row_begin, row_end, dtype=np.uint64)[:, None]
                keys = np.concatenate([keys, np.full((2, QBLOCK), NONE, np.uint64)])
                keys.sort(axis=0)
                k1, k2 = keys[0], keys[1]
            part[lane_q[live], s, 0] = k1[live]
            part[lane_q[live], s, 1] = k2[live]

    merged = np.sort(part.reshape(len(part), -1), axis=1)[:, :2]
    idx = np.where(merged == NONE, NONE, merged & np.uint64(0xFFFFFFFF))
    d = np.where(merged == NONE, np.uint64(0x7FFFFFFF), merged >> np.uint64(32)).astype(np.int32)
    return idx, d, tuple(stats)
