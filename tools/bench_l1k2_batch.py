"""Measures the many-pairs L1 2-NN (device.l1k2_batch) against a loop of device.l1k2 per pair on one GPU and
prints one JSON line per shape.  Inputs are resident in HBM.  Every figure is a device-event time around a window
of repetitions of at least --window seconds, after a warm-up of both forms; the two forms alternate, window by
window, in one process, and the spread is over the windows of a form.

  python tools/bench_l1k2_batch.py                      # both forms of this build
  python tools/bench_l1k2_batch.py --forms loop --root DIR
        # the loop alone with spectavi_amd imported from DIR: a build of the commit before l1k2_batch existed

Shapes, all at dim 128: 32 sets x 8192 rows, 64 x 2048 and 8 x 50000, every pair i < j as (query j, database i).
The share of the v_sad issue peak is lane-ops over time over 39.32e12 lane-ops/s at dim / 4 lane-ops per pair, as
l1k2.hip computes it: for the whole call from the windows, for the main kernel alone from the library's brackets."""
import argparse
import json
import math
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="directory to import spectavi_amd from")
ap.add_argument("--forms", default="batch,loop", help="comma list of: batch, loop")
ap.add_argument("--shapes", default="32x8192,64x2048,8x50000", help="comma list of SETSxROWS")
ap.add_argument("--window", type=float, default=1.0, help="seconds of device time per timed window, at least")
ap.add_argument("--rounds", type=int, default=5, help="windows per form")
ap.add_argument("--dim", type=int, default=128)
args = ap.parse_args()
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectavi_amd import device as spv  # noqa: E402

SAD_PEAK = 39.3216e12  # v_sad_hi_u8 lane-ops/s: 256 CUs x 4 SIMDs x 64 lanes / 4 cycles x 2.4 GHz


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
    forms = [f for f in args.forms.split(",") if f]
    for shape in args.shapes.split(","):
        nsets, rows = (int(v) for v in shape.split("x"))
        g = torch.Generator(device="cuda").manual_seed(0x5e75 + nsets)
        desc = torch.randint(0, 256, (nsets * rows, args.dim), dtype=torch.uint8, device="cuda", generator=g)
        seg = np.arange(nsets + 1, dtype=np.int64) * rows
        pairs = [(j, i) for i in range(nsets) for j in range(i + 1, nsets)]
        sets = [desc[s * rows:(s + 1) * rows] for s in range(nsets)]
        calls = {}
        if "batch" in forms:
            calls["batch"] = lambda: spv.l1k2_batch(desc, seg, pairs)
        if "loop" in forms:
            calls["loop"] = lambda: [spv.l1k2(sets[b], sets[a]) for a, b in pairs]
        rec = {"metric": "L1 2-NN of a collection of descriptor-set pairs, ms per collection",
               "config": {"workload": "%d sets x %d rows, D=%d, all %d pairs i < j" % (nsets, rows, args.dim, len(pairs))},
               "unit": "ms", "dtype": "u8", "data": "synthetic", "window_s": args.window, "rounds": args.rounds}
        if "batch" in calls:
            plan = spv.l1k2_batch_plan(seg, pairs, args.dim)
            rec["plan"] = {k: plan[k] for k in ("dim_pad", "q", "items", "max_slices", "workspace_bytes")}
        outs = {name: fn() for name, fn in calls.items()}      # warm-up: code objects, workspaces
        torch.cuda.synchronize()
        if len(outs) == 2:  # the two forms must agree before their times are compared
            bi, bd, off = outs["batch"]
            same = all(torch.equal(bi[off[p]:off[p + 1]], li) and torch.equal(bd[off[p]:off[p + 1]], ld)
                       for p, (li, ld) in enumerate(outs["loop"]))
            rec["forms_agree"] = bool(same)
        del outs
        reps = {name: max(1, math.ceil(args.window * 1e3 / window(fn, 1))) for name, fn in calls.items()}
        times = {name: [] for name in calls}
        for _ in range(args.rounds):
            for name, fn in calls.items():
                times[name].append(window(fn, reps[name]))
        npairs_rows = float(len(pairs)) * rows * rows
        for name, ms in times.items():
            med = float(np.median(ms))
            rec[name] = {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "spread": (max(ms) - min(ms)) / med,
                         "reps_per_window": reps[name], "pairs_per_s": npairs_rows / (med * 1e-3),
                         "call_share_of_v_sad_issue_peak": npairs_rows * (args.dim // 4) / (med * 1e-3) / SAD_PEAK}
        if "batch" in calls:  # the main kernel alone, from the library's event brackets, in a pass of its own
            spv.profile_reset()
            spv.profile_enable(True)
            for _ in range(3):
                calls["batch"]()
            torch.cuda.synchronize()
            spv.profile_enable(False)
            n, ms = spv.profile_read("l1k2_batch")
            nm, msm = spv.profile_read("l1k2_batch_merge")
            rec["batch"]["kernel_ms"] = ms / max(n, 1)
            rec["batch"]["merge_ms"] = msm / max(nm, 1)
            rec["batch"]["kernel_share_of_v_sad_issue_peak"] = npairs_rows * (args.dim // 4) / (ms / max(n, 1) * 1e-3) / SAD_PEAK
        if len(calls) == 2:
            rec["loop_over_batch"] = rec["loop"]["ms"] / rec["batch"]["ms"]
            rec["batch_faster_in_every_window"] = bool(max(times["batch"]) < min(times["loop"]))
        rec["root"] = "this build" if os.path.samefile(args.root, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))) else "other build"
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_l1k2_batch.py needs a GPU: it measures and has nothing to fall back to")
    main()
