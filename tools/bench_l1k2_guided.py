"""Measures the guided many-pairs L1 2-NN (device.l1k2_guided_batch) against device.l1k2_batch on the same
collection on one GPU and prints one JSON line per band half-width.  l1k2_batch does every SAD; it is also a floor
for what a masked all-pairs kernel would cost, so the guided call has to beat it in every window to have bought
anything.  Inputs are resident in HBM.  Every figure is a device-event time around a window of repetitions of at
least --window seconds, after a warm-up of both forms; the two forms alternate, window by window, in one process,
and the spread is over the windows of a form.

  python tools/bench_l1k2_guided.py [--sets 32] [--rows 8192] [--max-dist 2,8,32]

Collection: --sets sets of --rows rows, every pair i < j as (query j, database i), dim 128, uniform bytes, keypoints
uniform in 1280 x 960; every query gets a random unit-normal line through a random point of the frame, so that
max_dist = 2 gives a band share near 0.5 %.  The true share is read from ncand."""
import argparse
import json
import math
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--sets", type=int, default=32)
ap.add_argument("--rows", type=int, default=8192)
ap.add_argument("--max-dist", default="2,8,32", help="comma list of band half-widths in pixels")
ap.add_argument("--window", type=float, default=1.0, help="seconds of device time per timed window, at least")
ap.add_argument("--rounds", type=int, default=5, help="windows per form")
args = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectavi_amd import device as spv  # noqa: E402


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
    nsets, rows, dim = args.sets, args.rows, 128
    g = torch.Generator(device="cuda").manual_seed(0x9d1de + nsets)
    total = nsets * rows
    desc = torch.randint(0, 256, (total, dim), dtype=torch.uint8, device="cuda", generator=g)
    geom = torch.rand((total, 4), dtype=torch.float32, device="cuda", generator=g) * torch.tensor(
        [1280.0, 960.0, 7.0, 6.28], device="cuda")
    seg = np.arange(nsets + 1, dtype=np.int64) * rows
    pairs = [(j, i) for i in range(nsets) for j in range(i + 1, nsets)]
    out_rows = len(pairs) * rows
    th = torch.rand(out_rows, dtype=torch.float64, device="cuda", generator=g) * (2 * math.pi)
    px = torch.rand(out_rows, dtype=torch.float64, device="cuda", generator=g) * 1280.0
    py = torch.rand(out_rows, dtype=torch.float64, device="cuda", generator=g) * 960.0
    l0, l1 = torch.cos(th), torch.sin(th)
    lines = torch.stack([l0, l1, -(l0 * px + l1 * py)], dim=1).contiguous()
    del th, px, py, l0, l1
    plan = spv.l1k2_guided_batch_plan(seg, pairs, dim)
    batch = lambda: spv.l1k2_batch(desc, seg, pairs)  # noqa: E731
    batch()
    for md in (float(v) for v in args.max_dist.split(",")):
        guided = lambda: spv.l1k2_guided_batch(desc, geom, seg, pairs, lines, md)  # noqa: E731
        calls = {"guided": guided, "l1k2_batch": batch}
        ncand = spv.l1k2_guided_batch(desc, geom, seg, pairs, lines, md, want_ncand=True)[2]   # also the warm-up
        torch.cuda.synchronize()
        rec = {"metric": "guided L1 2-NN of a collection of descriptor-set pairs, ms per collection",
               "config": {"workload": "%d sets x %d rows, D=%d, all %d pairs i < j" % (nsets, rows, dim, len(pairs)),
                          "max_dist": md},
               "unit": "ms", "dtype": "u8", "data": "synthetic", "window_s": args.window, "rounds": args.rounds,
               "band_share": float(ncand.double().mean()) / rows,
               "plan": {k: plan[k] for k in ("items", "max_slices", "workspace_bytes")}}
        del ncand
        reps = {name: max(1, math.ceil(args.window * 1e3 / window(fn, 1))) for name, fn in calls.items()}
        times = {name: [] for name in calls}
        for _ in range(args.rounds):
            for name, fn in calls.items():
                times[name].append(window(fn, reps[name]))
        for name, ms in times.items():
            med = float(np.median(ms))
            rec[name] = {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "spread": (max(ms) - min(ms)) / med,
                         "reps_per_window": reps[name]}
        # the main kernel alone, from the library's event brackets, in a pass of its own
        spv.profile_reset()
        spv.profile_enable(True)
        for _ in range(3):
            guided()
        torch.cuda.synchronize()
        spv.profile_enable(False)
        n, ms = spv.profile_read("l1k2_guided")
        nm, msm = spv.profile_read("l1k2_guided_merge")
        rec["guided"]["kernel_ms"] = ms / max(n, 1)
        rec["guided"]["merge_ms"] = msm / max(nm, 1)
        rec["guided"]["kernel_share_of_call"] = rec["guided"]["kernel_ms"] / rec["guided"]["ms"]
        rec["l1k2_batch_over_guided"] = rec["l1k2_batch"]["ms"] / rec["guided"]["ms"]
        rec["guided_faster_in_every_window"] = bool(max(times["guided"]) < min(times["l1k2_batch"]))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_l1k2_guided.py needs a GPU: it measures and has nothing to fall back to")
    main()
