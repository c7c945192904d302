"""Inputs of tests/test_tracks_batch_gpu.py: small collections with their matches in the form ratio_test writes
them, (out row, row within the database set), built on the host with numpy alone."""
import numpy as np

from tests import tracks_model as tm

RAGGED_SIZES = [0, 1, 2, 255, 256, 257, 0, 1500, 3]
RAGGED_SEED = 11


def seg_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def ragged(seed=RAGGED_SEED, sizes=RAGGED_SIZES, prob=0.05):
    """Every pair i < j as (j, i), the self pair (7, 7) and the duplicate (5, 3); each query row matches with
    probability `prob` a uniformly random row of the database set.  The tiny sets act as hubs.
    Returns (seg_off, pairs int32 [npairs, 2], matches int32 [k, 2])."""
    rng = np.random.default_rng(seed)
    seg = seg_of(sizes)
    n = len(sizes)
    pairs = [(j, i) for i in range(n) for j in range(i + 1, n)] + [(7, 7), (5, 3)]
    out_off = tm.out_offsets(seg, pairs)
    m = []
    for p, (q, d) in enumerate(pairs):
        hit = np.flatnonzero(rng.random(sizes[q]) < prob)
        if sizes[d] == 0 or hit.size == 0:
            continue
        m.append(np.stack([out_off[p] + hit, rng.integers(0, sizes[d], hit.size)], 1))
    return seg, np.array(pairs, np.int32), np.concatenate(m).astype(np.int32)


def depth():
    """A path through 20 000 nodes: 40 sets of 500 rows, row r of set v + 1 matched to row r of set v, and inside
    set 0 row r + 1 matched to row r, which joins the 500 paths into one."""
    sizes = [500] * 40
    pairs = [(v + 1, v) for v in range(39)] + [(0, 0)]
    seg = seg_of(sizes)
    out_off = tm.out_offsets(seg, pairs)
    r = np.arange(500)
    m = [np.stack([out_off[p] + r, r], 1) for p in range(39)]
    m.append(np.stack([out_off[39] + r[1:], r[:-1]], 1))
    return seg, np.array(pairs, np.int32), np.concatenate(m).astype(np.int32)


def star(centre_last):
    """4 096 edges from distinct nodes to one node, which is the smallest row of all or the largest."""
    if centre_last:
        sizes, pairs = [4096, 1], [(0, 1)]
    else:
        sizes, pairs = [1, 4096], [(1, 0)]
    m = np.stack([np.arange(4096), np.zeros(4096, np.int64)], 1)
    return seg_of(sizes), np.array(pairs, np.int32), m.astype(np.int32)


def chains(lengths, sizes=None):
    """One track per entry of `lengths`, their rows interleaved (track j holds rows j, j + T, j + 2 T, ... while it
    lasts, compacted), each a chain whose edges are supplied in descending row order.  One set unless `sizes` cuts
    the same rows into several; the pair list is every (query set, database set)."""
    T, longest = len(lengths), max(lengths)
    grid = [(k, j) for k in range(longest) for j in range(T) if k < lengths[j]]     # ascending row order
    rows_of = [[] for _ in range(T)]
    for g, (k, j) in enumerate(grid):
        rows_of[j].append(g)
    total = len(grid)
    sizes = [total] if sizes is None else sizes
    assert sum(sizes) == total
    seg = seg_of(sizes)
    ns = len(sizes)
    pairs = [(q, d) for q in range(ns) for d in range(ns)]
    out_off = tm.out_offsets(seg, pairs)
    set_of = np.searchsorted(seg, np.arange(total), side="right") - 1
    m = []
    for rows in rows_of:
        for a, b in zip(rows[:0:-1], rows[-2::-1]):       # (later row, the row before it), from the far end
            q, d = set_of[a], set_of[b]
            m.append((out_off[q * ns + d] + a - seg[q], b - seg[d]))
    return seg, np.array(pairs, np.int32), np.array(m, np.int32).reshape(-1, 2)
