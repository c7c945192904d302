"""Measures the many-sets triangulation (device.dlt_triangulate_batch) on one GPU and prints one JSON line per
case.  Everything is resident in HBM.  A figure is wall time per call over a window of back-to-back calls of at
least --window seconds with the device synchronised at both ends, after a warm-up of both forms; the two forms
alternate, window by window, in one process, and the median and the spread are over the windows of a form.  The
kernels alone come from the library's event brackets (spv_profile_read), in passes of their own.

  python tools/bench_dlt_batch.py
  python tools/bench_dlt_batch.py --cases small --rounds 9

Cases:
  small   2 000 sets of 200 rows, a mask of density 0.5, one camera pair per set: one batch call against the loop
          the library offered before -- per set a gather of the selected rows and device.dlt_triangulate
  large   1 set of 10M rows, no mask: the batch call against device.dlt_triangulate on the same rows (very large
          single sets remain the single call's job; the ratio is what the item walk costs)"""
import argparse
import json
import math
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="directory to import spectavi_amd from")
ap.add_argument("--cases", default="small,large")
ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window, at least")
ap.add_argument("--rounds", type=int, default=7, help="windows per form")
ap.add_argument("--out", default=None, help="also write the records, a JSON list, to this file")
args = ap.parse_args()
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectavi_amd import device as spv  # noqa: E402


def window(fn, reps):
    """ms per call over `reps` back-to-back calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def kernels_ms(fn, names, reps=5):
    """{name: ms per call} from the library's event brackets over `reps` calls."""
    spv.profile_reset()
    spv.profile_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    spv.profile_enable(False)
    return {k: spv.profile_read(k)[1] / reps for k in names}


def collection(nsets, rows, seed):
    """x0, x1 CUDA float64 [nsets * rows, 3], cameras: per set P0 = [I|0] and a random [R|t]-like P1, noisy points."""
    rng = np.random.default_rng(seed)
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    P1s = rng.standard_normal((nsets, 3, 4)) * 0.1 + P0 + np.array([0, 0, 0, 1.0]) * rng.standard_normal((nsets, 3, 1))
    g = torch.Generator(device="cuda").manual_seed(seed)
    Xw = torch.randn((nsets * rows, 4), dtype=torch.float64, device="cuda", generator=g)
    Xw[:, 2] += 5
    Xw[:, 3] = 1
    x0 = Xw[:, :3].contiguous()
    x1 = torch.empty_like(x0)
    for p in range(nsets):
        x1[p * rows:(p + 1) * rows] = Xw[p * rows:(p + 1) * rows] @ torch.from_numpy(P1s[p].T.copy()).cuda()
    x1[:, :2] += 1e-3 * torch.randn((nsets * rows, 2), dtype=torch.float64, device="cuda", generator=g)
    return x0, x1.contiguous(), P0, P1s


def measure(calls, rec, base, new):
    reps = {name: max(1, math.ceil(args.window * 1e3 / window(fn, 1))) for name, fn in calls.items()}
    times = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            times[name].append(window(fn, reps[name]))
    for name, ms in times.items():
        med = float(np.median(ms))
        rec[name] = {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "spread": (max(ms) - min(ms)) / med,
                     "reps_per_window": reps[name]}
    rec["%s_over_%s" % (base, new)] = rec[base]["ms"] / rec[new]["ms"]
    rec["%s_faster_in_every_window" % new] = bool(max(times[new]) < min(times[base]))


def case_small():
    nsets, rows = 2000, 200
    x0, x1, P0, P1s = collection(nsets, rows, 0xd17)
    off = np.arange(nsets + 1, dtype=np.int64) * rows
    mask = (torch.rand(nsets * rows, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) < 0.5).to(torch.uint8)
    # what the loop needs per set and the batch call does not: the selected rows as index tensors (prepared once,
    # outside the timing, as a caller that has the fits' inlier lists would hold them)
    sel = [torch.nonzero(mask[off[p]:off[p + 1]]).reshape(-1) + int(off[p]) for p in range(nsets)]

    def batch():
        return spv.dlt_triangulate_batch(x0, x1, off, P1s, mask=mask)

    def loop():
        return [spv.dlt_triangulate(P0, P1s[p], x0[sel[p]], x1[sel[p]]) for p in range(nsets)]

    (X, out_off), per = batch(), loop()  # warm-up: code objects, scratch
    n = int(out_off[-1])
    same = n == sum(len(a) for a in per) and bool((X[:n].view(torch.int64) == torch.cat(per).view(torch.int64)).all())
    rec = {"metric": "DLT triangulation of a collection of correspondence sets, ms per collection",
           "config": {"workload": "%d sets x %d rows, mask density 0.5, one camera pair per set" % (nsets, rows)},
           "unit": "ms", "dtype": "f64", "data": "synthetic", "window_s": args.window, "rounds": args.rounds,
           "forms_agree": same, "selected_rows": n,
           "plan": spv.dlt_triangulate_batch_plan(off, compute_units=torch.cuda.get_device_properties(0).multi_processor_count)}
    measure({"batch": batch, "loop": loop}, rec, "loop", "batch")
    rec["batch"]["kernels_ms"] = kernels_ms(batch, ("dlt_batch", "dlt_batch_scan"))
    rec["loop"]["kernels_ms"] = kernels_ms(loop, ("dlt",), reps=2)
    return rec


def case_large():
    rows = 10_000_000
    x0, x1, P0, P1s = collection(1, rows, 0xb16)
    off = np.array([0, rows], np.int64)

    def batch():
        return spv.dlt_triangulate_batch(x0, x1, off, P1s)

    def single():
        return spv.dlt_triangulate(P0, P1s[0], x0, x1)

    (X, _), one = batch(), single()
    same = bool((X.view(torch.int64) == one.view(torch.int64)).all())
    del X, one
    rec = {"metric": "DLT triangulation of one large set, ms per call",
           "config": {"workload": "1 set x %d rows, no mask" % rows},
           "unit": "ms", "dtype": "f64", "data": "synthetic", "window_s": args.window, "rounds": args.rounds,
           "forms_agree": same, "plan": spv.dlt_triangulate_batch_plan(off)}
    measure({"batch": batch, "single": single}, rec, "batch", "single")
    rec["batch"]["kernels_ms"] = kernels_ms(batch, ("dlt_batch", "dlt_batch_scan"))
    rec["single"]["kernels_ms"] = kernels_ms(single, ("dlt",))
    rec["kernel_batch_over_single"] = rec["batch"]["kernels_ms"]["dlt_batch"] / rec["single"]["kernels_ms"]["dlt"]
    return rec


def main():
    recs = []
    for name in args.cases.split(","):
        rec = {"small": case_small, "large": case_large}[name]()
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_dlt_batch.py needs a GPU: it measures and has nothing to fall back to")
    main()
