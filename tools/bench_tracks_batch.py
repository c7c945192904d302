"""Measures device.tracks_batch against what a user had before it, on one GPU, and prints one JSON line per collection.

Forms, all from the same (matches, count, mask) resident in HBM to the track arrays:
  tracks_batch  device.tracks_batch
  torch         what could be done on the device with torch ops only: the matches decoded with searchsorted, min-label
                propagation (scatter_reduce_ 'amin' over both ends, then label = label[label] until nothing changes,
                until no edge changes a label), then bincount / sort / unique_consecutive for the track arrays
  host          matches and mask copied back, scipy's connected_components where scipy imports (else the union-find
                of tests/tracks_model.py), numpy for the track arrays
Every figure is a device-event time around a window of repetitions of at least --window seconds, after a warm-up of
every form; the forms alternate, window by window, in one process, and the spread is over the windows of a form.
The record says whether the three forms' outputs are equal, and holds the library's per-phase event brackets.

  python tools/bench_tracks_batch.py [--views 64] [--rows 8192] [--correct 0.25] [--random 0.02]

Collection: --views views of --rows rows of one --rows-point scene, each view's rows permuted; every pair i < j as
(query j, database i); each pair matches a --correct share of the points correctly plus a --random share of its
query rows to random database rows; a mask keeps 9 matches in 10."""
import argparse
import json
import math
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--rows", type=int, default=8192)
ap.add_argument("--correct", type=float, default=0.25)
ap.add_argument("--random", type=float, default=0.02)
ap.add_argument("--window", type=float, default=1.0, help="seconds of device time per timed window, at least")
ap.add_argument("--rounds", type=int, default=5, help="windows per form")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectavi_amd import device as spv  # noqa: E402

PHASES = ("tracks_init", "tracks_hook", "tracks_flatten", "tracks_sizes", "tracks_scan", "tracks_place", "tracks_order",
          "tracks_flags")


def window(fn, reps):
    """ms per call over `reps` back-to-back calls, by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def collection(views, rows, correct, random, seed=7):
    rng = np.random.default_rng(seed)
    inv = [np.argsort(rng.permutation(rows)) for _ in range(views)]     # the row of every scene point in each view
    pairs = np.array([(j, i) for i in range(views) for j in range(i + 1, views)], np.int32)
    nc, nr = int(round(correct * rows)), int(round(random * rows))
    m = np.empty((len(pairs), nc + nr, 2), np.int32)
    for p, (q, d) in enumerate(pairs.tolist()):
        pts = rng.choice(rows, nc, replace=False)
        m[p, :nc, 0], m[p, :nc, 1] = inv[q][pts], inv[d][pts]
        m[p, nc:, 0], m[p, nc:, 1] = rng.integers(0, rows, nr), rng.integers(0, rows, nr)
        m[p, :, 0] += p * rows
    m = m.reshape(-1, 2)
    m = m[np.argsort(m[:, 0], kind="stable")]                           # ascending out rows, as ratio_test writes them
    mask = (rng.random(len(m)) < 0.9).astype(np.uint8)
    return np.arange(views + 1, dtype=np.int64) * rows, pairs, m, mask


def torch_form(seg_t, out_off_t, qbase_t, dbase_t, matches, count, mask, n):
    k = int(count)
    m = matches[:k].long()
    keep = mask[:k] != 0
    p = torch.searchsorted(out_off_t, m[:, 0].contiguous(), right=True) - 1
    a = (qbase_t[p] + m[:, 0] - out_off_t[p])[keep]
    b = (dbase_t[p] + m[:, 1])[keep]
    label = torch.arange(n, device=matches.device)
    while True:
        low = torch.minimum(label[a], label[b])
        new = label.clone()
        new.scatter_reduce_(0, a, low, "amin")
        new.scatter_reduce_(0, b, low, "amin")
        new.scatter_reduce_(0, label[a], low, "amin")
        new.scatter_reduce_(0, label[b], low, "amin")
        while True:
            nxt = new[new]
            if torch.equal(nxt, new):
                break
            new = nxt
        if torch.equal(new, label):
            break
        label = new
    size = torch.bincount(label, minlength=n)
    rows = torch.nonzero(size[label] >= 2).reshape(-1)
    key, order = torch.sort(label[rows], stable=True)
    rows = rows[order]
    uniq, length = torch.unique_consecutive(key, return_counts=True)
    track_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=rows.device), torch.cumsum(length, 0)])
    track = torch.full((n,), -1, dtype=torch.int64, device=rows.device)
    track[uniq] = torch.arange(len(uniq), device=rows.device)
    track = track[label]
    sets = torch.searchsorted(seg_t, rows, right=True) - 1
    members = torch.stack([sets, rows - seg_t[sets]], 1)
    of = track[rows]
    twice = (sets[1:] == sets[:-1]) & (of[1:] == of[:-1])
    flags = torch.zeros(len(uniq), dtype=torch.uint8, device=rows.device)
    flags[of[1:][twice]] = 1
    return track_off.cpu().numpy(), members.int(), flags, label.int(), track.int()


def host_form(seg, pairs, matches, count, mask):
    k = int(count)
    m = matches[:k].cpu().numpy().astype(np.int64)
    keep = mask[:k].cpu().numpy() != 0
    n = int(seg[-1])
    out_off = np.concatenate([[0], np.cumsum(np.diff(seg)[pairs[:, 0]])])
    p = np.searchsorted(out_off, m[:, 0], side="right") - 1
    a = (seg[pairs[p, 0]] + m[:, 0] - out_off[p])[keep]
    b = (seg[pairs[p, 1]] + m[:, 1])[keep]
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        from tests import tracks_model as tm
        label, track, track_off, members, flags = tm.tracks(seg, np.stack([a, b], 1))
        return track_off, members, flags, label, track
    ncomp, comp = connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n)), directed=False)
    first = np.full(ncomp, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    label = first[comp]
    size = np.bincount(label, minlength=n)
    roots = np.flatnonzero((label == np.arange(n)) & (size >= 2))
    number = np.full(n, -1, np.int64)
    number[roots] = np.arange(len(roots))
    track = number[label]
    rows = np.flatnonzero(track >= 0)
    rows = rows[np.argsort(track[rows], kind="stable")]
    sets = np.searchsorted(seg, rows, side="right") - 1
    of = track[rows]
    flags = np.zeros(len(roots), np.uint8)
    flags[of[1:][(sets[1:] == sets[:-1]) & (of[1:] == of[:-1])]] = 1
    return (np.concatenate([[0], np.cumsum(size[roots])]), np.stack([sets, rows - seg[sets]], 1).astype(np.int32), flags,
            label.astype(np.int32), track.astype(np.int32))


def as_numpy(out):
    return [np.asarray(o.cpu().numpy() if isinstance(o, torch.Tensor) else o).astype(np.int64) for o in out]


def main():
    seg, pairs, m, mask = collection(args.views, args.rows, args.correct, args.random)
    n = int(seg[-1])
    matches, tmask = torch.from_numpy(m).cuda(), torch.from_numpy(mask).cuda()
    count = torch.tensor([len(m)], dtype=torch.int32).cuda()
    seg_t = torch.from_numpy(seg).cuda()
    out_off_t = torch.from_numpy(spv.l1k2_batch_plan(seg, pairs, 128)["out_off"]).cuda()   # the matcher's out rows per pair
    qbase_t, dbase_t = torch.from_numpy(seg[pairs[:, 0]]).cuda(), torch.from_numpy(seg[pairs[:, 1]]).cuda()
    calls = {"tracks_batch": lambda: spv.tracks_batch(seg, pairs, matches, count, mask=tmask),
             "torch": lambda: torch_form(seg_t, out_off_t, qbase_t, dbase_t, matches, count, tmask, n),
             "host": lambda: host_form(seg, pairs, matches, count, tmask)}
    outs = {name: as_numpy(fn()) for name, fn in calls.items()}        # also the warm-up
    torch.cuda.synchronize()
    ours = outs["tracks_batch"]
    length = np.diff(ours[0])
    rec = {"metric": "multi-view tracks from the matches of all pairs of a collection, ms per collection",
           "config": {"workload": "%d views x %d rows, all %d pairs i < j, %d matches, mask keeps %d" % (
               args.views, args.rows, len(pairs), len(m), int(mask.sum()))},
           "unit": "ms", "data": "synthetic", "window_s": args.window, "rounds": args.rounds,
           "tracks": int(len(length)), "members": int(ours[0][-1]), "longest_track": int(length.max()) if len(length) else 0,
           "inconsistent_tracks": int(ours[2].sum()),
           "workspace_bytes": int(spv.clib.spv_tracks_batch_workspace_bytes(n, len(m))),
           "outputs_equal": {name: bool(all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(ours, o)))
                             for name, o in outs.items() if name != "tracks_batch"}}
    del outs
    reps = {name: max(1, math.ceil(args.window * 1e3 / window(fn, 1))) for name, fn in calls.items()}
    times = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            times[name].append(window(fn, reps[name]))
    for name, ms in times.items():
        med = float(np.median(ms))
        rec[name] = {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "spread": (max(ms) - min(ms)) / med,
                     "reps_per_window": reps[name]}
    # the phases, from the library's event brackets, in a pass of their own
    spv.profile_reset()
    spv.profile_enable(True)
    for _ in range(5):
        calls["tracks_batch"]()
    torch.cuda.synchronize()
    spv.profile_enable(False)
    rec["tracks_batch"]["phase_ms"] = {k: spv.profile_read(k)[1] / max(spv.profile_read(k)[0], 1) for k in PHASES}
    rec["torch_over_tracks_batch"] = rec["torch"]["ms"] / rec["tracks_batch"]["ms"]
    rec["host_over_tracks_batch"] = rec["host"]["ms"] / rec["tracks_batch"]["ms"]
    rec["tracks_batch_faster_than_torch_in_every_window"] = bool(max(times["tracks_batch"]) < min(times["torch"]))
    rec["tracks_batch_faster_than_host_in_every_window"] = bool(max(times["tracks_batch"]) < min(times["host"]))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_tracks_batch.py needs a GPU: it measures and has nothing to fall back to")
    main()
