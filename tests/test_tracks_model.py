"""CPU-only: tests/tracks_model.py, the judge of the tracks_batch GPU tests, against a breadth-first search on small
graphs (exhaustively over small edge sets) and against scipy's connected_components where scipy imports."""
import itertools

import numpy as np
import pytest

from tests import tracks_model as tm


def bfs_tracks(seg, edges, min_len):
    """The contract from the definition: components by breadth-first search, everything else by sorting."""
    seg = [int(s) for s in seg]
    n = seg[-1]
    adj = [[] for _ in range(n)]
    for a, b in edges:
        adj[a].append(b)
        adj[b].append(a)
    label = [-1] * n
    comps = []
    for s in range(n):
        if label[s] >= 0:
            continue
        seen, todo = {s}, [s]
        while todo:
            nxt = []
            for u in todo:
                for v in adj[u]:
                    if v not in seen:
                        seen.add(v)
                        nxt.append(v)
            todo = nxt
        for u in seen:
            label[u] = s        # s is the smallest row of its component: every smaller row has its label already
        comps.append(sorted(seen))
    kept = [c for c in comps if len(c) >= min_len]      # comps is in ascending order of the smallest row
    track = [-1] * n
    members, off, flags = [], [0], []
    set_of = lambda g: max(s for s in range(len(seg) - 1) if seg[s] <= g and seg[s + 1] > g)
    for t, c in enumerate(kept):
        sets = [set_of(g) for g in c]
        for g, s in zip(c, sets):
            track[g] = t
            members.append((s, g - seg[s]))
        off.append(len(members))
        flags.append(int(len(set(sets)) < len(sets)))
    return (np.array(label, np.int32), np.array(track, np.int32), np.array(off, np.int64),
            np.array(members, np.int32).reshape(-1, 2), np.array(flags, np.uint8))


def assert_same(got, want, what):
    for name, g, w in zip(("label", "track", "track_off", "members", "flags"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name, g, w)


def test_exhaustive_small_edge_sets():
    """Every set of at most 3 edges (self loops included) on 5 nodes in sets of sizes [2, 0, 1, 2], both min_len."""
    seg = [0, 2, 2, 3, 5]
    pool = [(a, b) for a in range(5) for b in range(a + 1)]
    for k in range(4):
        for edges in itertools.combinations(pool, k):
            for min_len in (2, 3):
                assert_same(tm.tracks(seg, np.array(edges, np.int64).reshape(-1, 2), min_len),
                            bfs_tracks(seg, edges, min_len), (edges, min_len))


@pytest.mark.parametrize("seed", range(20))
def test_random_graphs_of_12_nodes(seed):
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.integers(0, 13, rng.integers(0, 5)))
    seg = np.concatenate([[0], cuts, [12]])
    edges = rng.integers(0, 12, (int(rng.integers(0, 14)), 2))
    for min_len in (2, 3, 5):
        want = bfs_tracks(seg, edges.tolist(), min_len)
        assert_same(tm.tracks(seg, edges, min_len), want, (seed, min_len))
        # continuing: any split of the edges, the first half's label passed on
        h = len(edges) // 2
        first = tm.tracks(seg, edges[:h], min_len)
        assert_same(tm.tracks(seg, edges[h:], min_len, label=first[0]), want, (seed, min_len, "continued"))
    # an incoming label outside [0, its own row] stands for its own row
    bad = np.arange(12, dtype=np.int64)
    bad[[1, 5, 7]] = [-5, 2 ** 31 - 1, 8]
    assert_same(tm.tracks(seg, edges, 2, label=bad), bfs_tracks(seg, edges.tolist(), 2), (seed, "garbage label"))


def test_against_scipy():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    rng = np.random.default_rng(5)
    sizes = [0, 1, 2, 255, 256, 257, 0, 1500, 3]
    seg = np.concatenate([[0], np.cumsum(sizes)])
    n = int(seg[-1])
    edges = rng.integers(0, n, (600, 2))
    label, track, track_off, members, flags = tm.tracks(seg, edges, 2)
    ncomp, comp = connected_components(sp.coo_matrix((np.ones(len(edges)), (edges[:, 0], edges[:, 1])), shape=(n, n)),
                                       directed=False)
    first = np.full(ncomp, n)
    np.minimum.at(first, comp, np.arange(n))
    assert np.array_equal(label, first[comp])
    sizes_c = np.bincount(comp)
    assert np.array_equal(track >= 0, sizes_c[comp] >= 2)
    assert len(track_off) - 1 == int((sizes_c >= 2).sum()) and track_off[-1] == int((track >= 0).sum()) == len(members)
    g = seg[members[:, 0]] + members[:, 1]
    assert np.array_equal(track[g], np.repeat(np.arange(len(track_off) - 1), np.diff(track_off)))
    assert all(np.all(np.diff(g[a:b]) > 0) for a, b in zip(track_off[:-1], track_off[1:]))


def test_edges_of_skips_what_the_contract_skips():
    seg = [0, 3, 3, 7]                       # sets of 3, 0 and 4 rows
    pairs = [[2, 0], [1, 0], [0, 2], [2, 2]]  # out rows 0..3, none, 4..6, 7..10
    m = [[0, 2], [3, 0], [4, 3], [7, 0], [10, 3], [-1, 0], [11, 0], [0, 3], [0, -1], [5, 4], [6, 1]]
    e = tm.edges_of(seg, pairs, m)
    assert e.tolist() == [[3, 2], [6, 0], [0, 6], [3, 3], [6, 6], [2, 4]]
    assert tm.edges_of(seg, pairs, m, count=2).tolist() == [[3, 2], [6, 0]]
    assert tm.edges_of(seg, pairs, m, count=99, mask=[0, 1] + [0] * 9).tolist() == [[6, 0]]
    assert tm.edges_of(seg, [], m).shape == (0, 2)
