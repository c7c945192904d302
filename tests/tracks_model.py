"""The contract of tracks_batch (include/spectavi_amd.h) restated in plain numpy / Python: a union-find over the rows
of the concatenated tables.  It is the judge of every GPU test of the feature; tests/test_tracks_model.py checks the
model itself against a breadth-first search and against scipy.

    edges_of(seg_off, pairs, matches, count=None, mask=None)  -> int64 [k, 2] global rows of the valid edges
    tracks(seg_off, edges, min_len=2, label=None)             -> (label, track, track_off, members, flags)
"""
import numpy as np


def out_offsets(seg_off, pairs):
    seg = np.asarray(seg_off, np.int64).reshape(-1)
    prs = np.asarray(pairs, np.int64).reshape(-1, 2)
    return np.concatenate([[0], np.cumsum(np.diff(seg)[prs[:, 0]])]).astype(np.int64)


def edges_of(seg_off, pairs, matches, count=None, mask=None):
    """The edges the call reads: rows [0, min(count, capacity)) of matches = (out row, row within the database set),
    those the mask keeps, without the rows whose out row or database row is out of range."""
    seg = np.asarray(seg_off, np.int64).reshape(-1)
    prs = np.asarray(pairs, np.int64).reshape(-1, 2)
    m = np.asarray(matches, np.int64).reshape(-1, 2)
    n = len(m) if count is None else max(0, min(int(count), len(m)))
    out_off = out_offsets(seg, prs)
    edges = []
    for i in range(n):
        if mask is not None and not mask[i]:
            continue
        o, k = int(m[i, 0]), int(m[i, 1])
        if o < 0 or o >= out_off[-1]:
            continue
        p = int(np.searchsorted(out_off, o, side="right")) - 1   # the last pair that begins at or before o
        q, db = int(prs[p, 0]), int(prs[p, 1])
        if k < 0 or k >= seg[db + 1] - seg[db]:
            continue
        edges.append((seg[q] + o - out_off[p], seg[db] + k))
    return np.array(edges, np.int64).reshape(-1, 2)


def tracks(seg_off, edges, min_len=2, label=None):
    """label int32 [n] (smallest row of the component), track int32 [n] (-1: none), track_off int64 [ntracks + 1],
    members int32 [nmembers, 2] = (set, row within the set), flags uint8 [ntracks].  label: an earlier result to
    continue from; an entry outside [0, its own row] stands for its own row."""
    seg = np.asarray(seg_off, np.int64).reshape(-1)
    n = int(seg[-1])
    parent = list(range(n))
    if label is not None:
        for i, v in enumerate(np.asarray(label).tolist()):
            if 0 <= v < i:
                parent[i] = v

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for a, b in np.asarray(edges, np.int64).reshape(-1, 2).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    lab = np.array([find(i) for i in range(n)], np.int32).reshape(n)
    size = np.bincount(lab, minlength=n) if n else np.zeros(0, np.int64)
    roots = np.flatnonzero((lab == np.arange(n)) & (size >= min_len))
    number = np.full(n, -1, np.int32)
    number[roots] = np.arange(len(roots), dtype=np.int32)
    track = number[lab] if n else number
    track_off = np.concatenate([[0], np.cumsum(size[roots])]).astype(np.int64)
    rows = np.flatnonzero(track >= 0)
    rows = rows[np.argsort(track[rows], kind="stable")]          # by track, inside a track by global row
    sets = np.searchsorted(seg, rows, side="right") - 1          # the last set that begins at or before the row
    members = np.stack([sets, rows - seg[sets]], 1).astype(np.int32).reshape(-1, 2)
    flags = np.zeros(len(roots), np.uint8)
    of = track[rows]                                             # inside a track the sets ascend with the rows:
    twice = (sets[1:] == sets[:-1]) & (of[1:] == of[:-1])        # two members of one set are neighbours
    flags[of[1:][twice]] = 1
    return lab, track.astype(np.int32), track_off, members, flags
