"""Measures the many-tables normalisation (device.normalize_batch) of a view set's uint8 descriptors against the loop
a build without it runs -- torch.cat of device.normalize(desc[a:b].to(float32)) over the views -- on one GPU, and
prints one JSON line.

Two collections of random uint8 descriptors, D = 128, resident in HBM before the clock starts: 64 views x 8192 rows
and 8 views x 60000 rows.  Both forms start from the same uint8 `desc` and produce the float32 table.

Every figure is a device-event time around a window of back-to-back calls that lasts at least --window seconds,
after a warm-up of all forms; the forms alternate, window by window, in one process; a form's spread is
(max - min) / median over its --rounds windows.  Before anything is timed the two results are compared (they must be
the same bits).  --forms loop runs on a build that has no normalize_batch: that is how the baseline is taken on the
parent commit, whose windows also give the run-to-run spread the comparison is held against.

The batch form's three brackets come from the library's events in a pass of their own; the element-wise pass's
share of the HBM rate counts rows x D bytes in and rows x D16 x 4 bytes out.

  python tools/normalize_batch_bench.py > profiles/normalize_batch_bench_branch_1.json
  python tools/normalize_batch_bench.py --forms loop > profiles/normalize_batch_bench_parent_1.json   (parent build)
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="64x8192,8x60000", help="views x rows per view, comma separated")
ap.add_argument("--dim", type=int, default=128)
ap.add_argument("--window", type=float, default=0.5, help="seconds of device time per timed window, at least")
ap.add_argument("--rounds", type=int, default=7, help="windows per form")
ap.add_argument("--forms", default="batch,loop")
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectavi_amd import device as spv  # noqa: E402

HBM_TBS = 6.29  # measured float4 copy rate of the MI355X, TB/s


def window(fn, reps):
    """ms per call over `reps` back-to-back calls, by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(views, rows_per_view):
    gen = torch.Generator(device="cuda").manual_seed(args.seed)
    desc = torch.randint(0, 256, (views * rows_per_view, args.dim), dtype=torch.uint8, device="cuda", generator=gen)
    seg = np.arange(views + 1, dtype=np.int64) * rows_per_view
    calls = {"batch": lambda: spv.normalize_batch(desc, seg),
             "loop": lambda: torch.cat([spv.normalize(desc[a:b].to(torch.float32)) for a, b in zip(seg[:-1], seg[1:])])}
    calls = {k: calls[k] for k in args.forms.split(",") if k}
    rec = {"workload": "%d views x %d rows, D=%d, uint8 in, float32 out" % (views, rows_per_view, args.dim)}

    outs = {name: fn() for name, fn in calls.items()}      # warm-up: code objects, workspaces
    torch.cuda.synchronize()
    if "batch" in outs and "loop" in outs:   # the two forms must agree before their times are compared
        rec["batch_equals_loop"] = bool(torch.equal(outs["batch"].view(torch.int32), outs["loop"].view(torch.int32)))
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
    if "batch" in calls:   # the brackets of the batch form, from the library's events, in a pass of its own
        spv.profile_reset()
        spv.profile_enable(True)
        for _ in range(20):
            calls["batch"]()
        torch.cuda.synchronize()
        spv.profile_enable(False)
        for k in ("normalize_batch_stats", "normalize_batch_finish", "normalize_batch"):
            cnt, ms = spv.profile_read(k)
            rec["batch"][k + "_ms"] = ms / max(cnt, 1)
        spv.profile_reset()
        dim16 = (args.dim + 15) // 16 * 16
        nbytes = views * rows_per_view * (args.dim + 4 * dim16)
        rec["batch"]["apply_bytes"] = nbytes
        rec["batch"]["apply_tb_per_s"] = nbytes / (rec["batch"]["normalize_batch_ms"] * 1e-3) / 1e12
        rec["batch"]["apply_share_of_hbm_copy_rate"] = rec["batch"]["apply_tb_per_s"] / HBM_TBS
    if "batch" in calls and "loop" in calls:
        rec["loop_over_batch"] = rec["loop"]["ms"] / rec["batch"]["ms"]
    return rec


def main():
    rec = {"metric": "per-view normalisation of a view set's descriptors, ms per collection", "unit": "ms",
           "data": "random uint8", "window_s": args.window, "rounds": args.rounds, "forms": args.forms, "shapes": []}
    for shape in args.shapes.split(","):
        views, rows = (int(v) for v in shape.split("x"))
        rec["shapes"].append(measure(views, rows))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("normalize_batch_bench.py needs a GPU: it measures and has nothing to fall back to")
    main()
