"""Measures device.resect_fit_batch on one GPU and prints one JSON line per workload.

Workloads (views x rows x tries), each a collection of tests/resect_model.py's scenes (pixel units, 30 % of the rows
redrawn, 0.5 px noise) with a share no try reaches and find_best_even_in_failure, so that every set runs every try:
  64 x 2000 x 512    a few large views: 512 row blocks, the tries of a round are cut into ranges
  512 x 500 x 512    many small views: 1024 row blocks a round of 128 sets
The scenes are built by tests/resect_model.py's `collection` (tests/tracks_triangulate_model.py's cameras, points and
observations with the outliers planted), the same code the GPU tests draw theirs from, so the tool needs the tests
package next to it, as tools/bench_tracks_triangulate.py does.
Per workload: the call's milliseconds (device events around a window of back-to-back calls of at least --window
seconds, after a warm-up; median and range over --rounds windows), and the kernels by the library's event brackets
(spv_profile_read: "resect_solve", "resect_score", "resect_reduce"; five calls in a pass of their own after every
window): milliseconds per call, resect_score's share of the three, and its rate in (try, row) verdicts per second.

The reference for the scorer, since the op has no predecessor: a verdict is 12 fma / mul for P X, 5 for the reciprocal
(one v_rcp_f64 at a quarter of the rate and four fma), 5 for the squared residual and 2 for the depth term.  A SIMD
issues an fp64 fma / mul for 64 lanes every 4 cycles (dlt_device.h, profiles/r03_f64_rate.txt) and v_rcp_f64 every 16:
(22 x 4 + 16) = 104 cycles a wave and try, so 1024 SIMDs at --clock-ghz (2.4) take at most 64 x 1024 x 2.4e9 / 104
verdicts a second.  `share_of_fp64_issue` is the measured rate over that bound.

  python tools/bench_resect_batch.py [--window 1.0] [--rounds 5] [--clock-ghz 2.4]
"""
import argparse
import json
import math
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--window", type=float, default=1.0, help="seconds of device time per timed window, at least")
ap.add_argument("--rounds", type=int, default=5, help="windows per workload")
ap.add_argument("--clock-ghz", type=float, default=2.4)
ap.add_argument("--workloads", default="64x2000x512,512x500x512")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectavi_amd import device as spv  # noqa: E402
from tests import resect_model as rm  # noqa: E402

NAMES = ("resect_solve", "resect_score", "resect_reduce")
CYCLES_PER_WAVE_VERDICT = 22 * 4 + 16


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
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for spec in args.workloads.split(","):
        views, rows, tries = (int(v) for v in spec.split("x"))
        col = rm.collection(np.random.default_rng(views), [rows] * views, noise=0.5, outliers=0.3)
        x, Xw = torch.from_numpy(col["x"]).cuda(), torch.from_numpy(col["Xw"]).cuda()
        seeds = np.arange(1, views + 1, dtype=np.uint64)

        def call():
            return spv.resect_fit_batch(x, Xw, col["off"], required_percent_inliers=2.0, max_error=3.0, maximum_tries=tries,
                                        find_best_even_in_failure=True, seeds=seeds)
        fits = call()                                                   # warm-up, and what the call finds
        assert all(f["tries_run"] == tries for f in fits)
        verdicts = views * rows * tries
        rec = {"metric": "RANSAC resection of many views, ms per call", "workload": spec, "unit": "ms", "data": "synthetic",
               "config": {"views": views, "rows": rows, "tries": tries, "verdicts": verdicts, "compute_units": cus,
                          "first_round": spv.resect_fit_batch_plan(col["off"], tries, cus)},
               "window_s": args.window, "rounds": args.rounds,
               "median_inlier_percent_of_the_kept_tries": float(np.median([f["inlier_percent"] for f in fits]))}
        reps = max(1, math.ceil(args.window * 1e3 / window(call, 1)))
        ms, kernels = [], {k: [] for k in NAMES}
        for _ in range(args.rounds):
            ms.append(window(call, reps))
            spv.profile_reset()
            spv.profile_enable(True)
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            spv.profile_enable(False)
            for k in NAMES:
                kernels[k].append(spv.profile_read(k)[1] / 5)
        spv.profile_reset()
        med = float(np.median(ms))
        rec["call_ms"] = {"median": med, "min": min(ms), "max": max(ms), "spread": (max(ms) - min(ms)) / med,
                          "reps_per_window": reps}
        rec["kernels_ms"] = {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in kernels.items()}
        total = sum(rec["kernels_ms"][k]["median"] for k in NAMES)
        score = rec["kernels_ms"]["resect_score"]["median"]
        rec["kernels_sum_ms"] = total
        rec["resect_score_share_of_kernels"] = score / total
        rec["resect_score_verdicts_per_s"] = verdicts / (score * 1e-3)
        bound = 64 * 4 * cus * args.clock_ghz * 1e9 / CYCLES_PER_WAVE_VERDICT
        rec["fp64_issue_bound_verdicts_per_s"] = bound
        rec["share_of_fp64_issue"] = rec["resect_score_verdicts_per_s"] / bound
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_resect_batch.py needs a GPU: it measures and has nothing to fall back to")
    main()
