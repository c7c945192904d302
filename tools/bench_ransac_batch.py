"""Measures the many-sets RANSAC (device.ransac_fit_batch) against a loop of device.ransac_fit over the same sets
with the same subsets on one GPU and prints one JSON line per collection.  The correspondences are resident in
HBM.  Both calls return host results, so every figure is wall time around a window of repetitions of at least
--window seconds with the device synchronised at both ends, after a warm-up of both forms; the two forms
alternate, window by window, in one process, and the spread is over the windows of a form.

  python tools/bench_ransac_batch.py
  python tools/bench_ransac_batch.py --collections 64x2000 --rounds 9

Collections (SETSxROWS[:p], p = every p-th set is pure outliers), maximum_tries 500, noise-free two-view scenes
with 40 % outliers, required share 0.5, threshold 1e-3, find_best_even_in_failure:
  64x2000      many medium sets, all of which succeed early
  256x500:2    a view set's usual lot: small sets, half of which never succeed and run every try
  8x50000      few large sets: nothing to gain from batching but the host waits"""
import argparse
import json
import math
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="directory to import spectavi_amd from")
ap.add_argument("--collections", default="64x2000,256x500:2,8x50000", help="comma list of SETSxROWS[:p]")
ap.add_argument("--tries", type=int, default=500)
ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window, at least")
ap.add_argument("--rounds", type=int, default=5, help="windows per form")
args = ap.parse_args()
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectavi_amd import device as spv  # noqa: E402
from spectavi_amd import mvg  # noqa: E402


def scene(rng, npt, outliers):
    """A calibrated pair [I | 0], [R | t] with a small rotation and a unit baseline, points 4-8 units in front of
    both; a share of the second view replaced by gross outliers.  Homogeneous float64 [npt,3] each."""
    a = rng.standard_normal(3)
    a /= np.linalg.norm(a)
    th = rng.uniform(-0.3, 0.3)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    t = rng.standard_normal(3)
    t /= np.linalg.norm(t)
    Xw = np.hstack([rng.uniform(-2, 2, (npt, 2)), rng.uniform(4, 8, (npt, 1)), np.ones((npt, 1))])
    x0 = Xw[:, :3].copy()
    x1 = Xw @ np.hstack([R, t[:, None]]).T
    nout = int(round(outliers * npt))
    if nout:
        rows = rng.choice(npt, nout, replace=False)
        x1[rows] = np.c_[rng.uniform(-0.6, 0.6, (nout, 2)), np.ones(nout)] * rng.uniform(4, 8, (nout, 1))
    return x0, x1


def window(fn, reps):
    """ms per call over `reps` back-to-back calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def main():
    kw = dict(required_percent_inliers=0.5, reprojection_error_allowed=1e-3, find_best_even_in_failure=True)
    for spec in args.collections.split(","):
        shape, _, every = spec.partition(":")
        nsets, rows = (int(v) for v in shape.split("x"))
        every = int(every) if every else 0
        rng = np.random.default_rng(0xba7c + nsets)
        sets = [scene(rng, rows, 1.0 if every and p % every == every - 1 else 0.4) for p in range(nsets)]
        samples = np.stack([mvg.ransac_sample(100 + p, rows, args.tries) for p in range(nsets)])
        off = np.arange(nsets + 1, dtype=np.int64) * rows
        x0 = torch.from_numpy(np.concatenate([a for a, _ in sets])).cuda()
        x1 = torch.from_numpy(np.concatenate([b for _, b in sets])).cuda()
        per0 = [x0[off[p]:off[p + 1]] for p in range(nsets)]
        per1 = [x1[off[p]:off[p + 1]] for p in range(nsets)]
        calls = {"batch": lambda: spv.ransac_fit_batch(x0, x1, off, samples=samples, **kw),
                 "loop": lambda: [spv.ransac_fit(per0[p], per1[p], samples=samples[p], **kw) for p in range(nsets)]}
        outs = {name: fn() for name, fn in calls.items()}  # warm-up: code objects, scratch
        same = all(b["success"] == l["success"] and b["best_try"] == l["best_try"] and
                   np.array_equal(b["inlier_idx"], l["inlier_idx"]) and
                   (b["essential"] is None) == (l["essential"] is None) and
                   (b["essential"] is None or b["essential"].tobytes() == l["essential"].tobytes())
                   for b, l in zip(outs["batch"], outs["loop"]))
        plan = spv.ransac_fit_batch_plan(off, args.tries, torch.cuda.get_device_properties(0).multi_processor_count)
        rec = {"metric": "two-view RANSAC of a collection of correspondence sets, ms per collection",
               "config": {"workload": "%d sets x %d correspondences, %d tries%s" %
                          (nsets, rows, args.tries, ", every %d. set pure outliers" % every if every else "")},
               "unit": "ms", "dtype": "f64", "data": "synthetic", "window_s": args.window, "rounds": args.rounds,
               "forms_agree": bool(same), "sets_that_succeed": int(sum(b["success"] for b in outs["batch"])),
               "tries_run": {"batch": int(sum(b["tries_run"] for b in outs["batch"])),
                             "loop": int(sum(l["tries_run"] for l in outs["loop"]))},
               "first_round": plan}
        reps = {name: max(1, math.ceil(args.window * 1e3 / window(fn, 1))) for name, fn in calls.items()}
        times = {name: [] for name in calls}
        for _ in range(args.rounds):
            for name, fn in calls.items():
                times[name].append(window(fn, reps[name]))
        for name, ms in times.items():
            med = float(np.median(ms))
            rec[name] = {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "spread": (max(ms) - min(ms)) / med,
                         "reps_per_window": reps[name], "ms_per_set": med / nsets}
        spv.profile_reset()  # the new kernels alone, from the library's event brackets, in a pass of their own
        spv.profile_enable(True)
        calls["batch"]()
        torch.cuda.synchronize()
        spv.profile_enable(False)
        rec["batch"]["kernels_ms"] = {k: spv.profile_read(k)[1] for k in
                                      ("seven_point", "ransac_cameras", "ransac_batch_score", "ransac_batch_reduce")}
        rec["batch"]["rounds"] = spv.profile_read("ransac_batch_reduce")[0]
        rec["loop_over_batch"] = rec["loop"]["ms"] / rec["batch"]["ms"]
        rec["batch_faster_in_every_window"] = bool(max(times["batch"]) < min(times["loop"]))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_ransac_batch.py needs a GPU: it measures and has nothing to fall back to")
    main()
