"""Measures the many-pairs cascade (device.cascade_batch) on a multi-view collection against (b) a loop of
device.cascade over the same pairs -- all a build without cascade_batch can do -- and (c) the exact many-pairs brute
force device.l1k2_batch on the uint8 image of the same rows, on one GPU, and prints one JSON line.

The collection is examples/multiview_from_sift_tables.synthetic_sift_views: --views views (12) of --points scene
points plus half as many unrelated keypoints (10000 + 5000 = 15000 rows per view), every pair i < j as (query j,
database i) (66 pairs), descriptors normalised per view as the reference's front-end does, m from
feature.auto_hash_bit_rate of the largest view, n 2, g 2.  Everything is resident in HBM before the clock starts.

Every figure is a device-event time around a window of back-to-back calls that lasts at least --window seconds,
after a warm-up of all forms; the forms alternate, window by window, in one process; a form's spread is
(max - min) / median over its --rounds windows.  Before anything is timed the batch form's result is compared, pair by
pair, with the loop's (they must be equal) and with the exact brute force's (how often the nearest neighbour agrees:
the cascade is approximate).

  python tools/cascade_batch_bench.py > profiles/cascade_batch_bench_1.json
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=12)
ap.add_argument("--points", type=int, default=10000, help="scene points per view (half as many unrelated rows are added)")
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
ap.add_argument("--rounds", type=int, default=7, help="windows per form")
ap.add_argument("--forms", default="batch,loop,l1k2_batch")
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from examples.multiview_from_sift_tables import synthetic_sift_views  # noqa: E402
from spectavi_amd import device as spv, feature  # noqa: E402


def window(fn, reps):
    """ms per call over `reps` back-to-back calls, by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    tables, _ = synthetic_sift_views(args.seed, args.views, args.points)
    seg = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64)
    nv = len(tables)
    pairs = [(q, d) for d in range(nv) for q in range(d + 1, nv)]
    _, desc = spv.split_sift_table(torch.from_numpy(np.concatenate(tables)).cuda())
    norm = [spv.normalize(desc[a:b].to(torch.float32), want_ubyte=True) for a, b in zip(seg[:-1], seg[1:])]
    rows, u8 = torch.cat([f for f, _ in norm]), torch.cat([u for _, u in norm])
    sets = [rows[a:b] for a, b in zip(seg[:-1], seg[1:])]
    dim = rows.shape[1]
    m, n, g = feature.auto_hash_bit_rate(*[int(np.diff(seg).max())] * 2), 2, 2
    hd = torch.from_numpy(feature.generate_hash_dict(0x5eed, dim, m, n)).cuda()

    calls = {"batch": lambda: spv.cascade_batch(rows, seg, pairs, hd, g=g),
             "loop": lambda: [spv.cascade(sets[b], sets[a], hd, g=g) for a, b in pairs],
             "l1k2_batch": lambda: spv.l1k2_batch(u8, seg, pairs)}
    calls = {k: calls[k] for k in args.forms.split(",") if k}
    plan = spv.cascade_batch_plan(seg, pairs, dim, m, n, g)
    rec = {"metric": "cascade-hash 2-NN of a multi-view collection, ms per collection",
           "config": {"workload": "%d views x ~%d rows, D=%d, all %d pairs i < j, m=%d n=%d g=%d"
                                  % (nv, int(np.diff(seg).mean()), dim, len(pairs), m, n, g)},
           "unit": "ms", "data": "synthetic_sift_views", "window_s": args.window, "rounds": args.rounds,
           "plan": {k: plan[k] for k in ("items", "out_rows", "hb", "workspace_bytes")}}

    outs = {name: fn() for name, fn in calls.items()}      # warm-up: code objects, workspaces
    torch.cuda.synchronize()
    if "batch" in outs:
        bi, bd, off = outs["batch"]
        if "loop" in outs:   # the two forms must agree before their times are compared
            rec["batch_equals_loop"] = bool(all(torch.equal(bi[off[p]:off[p + 1]], li) and torch.equal(bd[off[p]:off[p + 1]], ld)
                                                for p, (li, ld) in enumerate(outs["loop"])))
        if "l1k2_batch" in outs:
            rec["nearest_agrees_with_exact"] = float((bi[:, 0] == outs["l1k2_batch"][0][:, 0]).double().mean())
        _, _, _, ncand = spv.cascade_batch(rows, seg, pairs, hd, g=g, want_ncand=True)
        rec["mean_candidates_per_query"] = float(ncand.double().mean())
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
    if "batch" in calls:   # the three brackets of the batch form, from the library's events, in a pass of its own
        spv.profile_reset()
        spv.profile_enable(True)
        for _ in range(5):
            calls["batch"]()
        torch.cuda.synchronize()
        spv.profile_enable(False)
        for k in ("cascade_batch_project", "cascade_batch_buckets", "cascade_batch_probe"):
            cnt, ms = spv.profile_read(k)
            rec["batch"][k + "_ms"] = ms / max(cnt, 1)
        spv.profile_reset()
    if "batch" in calls and "loop" in calls:
        rec["loop_over_batch"] = rec["loop"]["ms"] / rec["batch"]["ms"]
        # the acceptance: faster than the loop by more than the run-to-run spread of the loop's own windows
        rec["loop_minus_batch_ms"] = rec["loop"]["ms"] - rec["batch"]["ms"]
        rec["loop_window_range_ms"] = rec["loop"]["ms_max"] - rec["loop"]["ms_min"]
        rec["batch_faster_by_more_than_the_loops_spread"] = bool(rec["loop_minus_batch_ms"] > rec["loop_window_range_ms"])
        rec["batch_faster_in_every_window"] = bool(max(times["batch"]) < min(times["loop"]))
    if "batch" in calls and "l1k2_batch" in calls:
        rec["l1k2_batch_over_batch"] = rec["l1k2_batch"]["ms"] / rec["batch"]["ms"]
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("cascade_batch_bench.py needs a GPU: it measures and has nothing to fall back to")
    main()
