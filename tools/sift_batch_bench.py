"""Measures SIFT of many images on one GPU: nimg calls of spv_sift_device in a loop (the only many-image form the
library had before sift_batch) against one spv_sift_batch_device call, and prints one JSON line per case.

Both forms run on the same device-resident images, on the same stream, into the same table regions with the same
capacities (the true row counts), each with its own warm workspace.  A figure is wall time per collection over a
window of back-to-back runs of at least --window seconds with the device synchronised at both ends, after a warm-up
of both forms; the forms alternate, window by window, in one process, and the median and the spread (max - min) are
over the windows of a form.  The kernels alone come from the library's event brackets (spv_profile_read), in passes
of their own.  The tables of the two forms are compared bit for bit before anything is timed.

  python tools/sift_batch_bench.py --out profiles/sift_batch_vs_loop.json
  python tools/sift_batch_bench.py --cases 32x480x640 --rounds 9

Cases: 32x480x640, 32x960x1280, 8x233x310 (N x hgt x wid), ragged (the three sizes mixed), and 32x480x640/4: the
first case with the workspace capped so that the call runs as 4 groups, which shows what grouping costs."""
import argparse
import json
import math
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="directory to import spectavi_amd from")
ap.add_argument("--cases", default="32x480x640,32x480x640/4,32x960x1280,8x233x310,ragged")
ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window, at least")
ap.add_argument("--rounds", type=int, default=7, help="windows per form")
ap.add_argument("--out", default=None, help="also write the records, a JSON list, to this file")
args = ap.parse_args()
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectavi_amd import device as spv  # noqa: E402
from spectavi_amd._lib import check, clib  # noqa: E402

LOOP_NAMES = ("sift_pyramid", "sift_detect", "sift_describe")
BATCH_NAMES = ("sift_batch_pyramid", "sift_batch_detect", "sift_batch_describe")


def texture(seed, h, w, passes=3):
    """tests/sift_cases.smooth_random on the device: uniform noise in [0, 255), smoothed by circular [1 1 1]/3 passes."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = torch.rand((h, w), dtype=torch.float64, device="cuda", generator=g) * 255
    for _ in range(passes):
        r = (r + torch.roll(r, 1, 0) + torch.roll(r, -1, 0)) / 3
        r = (r + torch.roll(r, 1, 1) + torch.roll(r, -1, 1)) / 3
    return r.to(torch.float32).contiguous()


def shapes_of(case):
    if case == "ragged":
        return [(480, 640), (960, 1280), (233, 310), (480, 640)] * 6 + [(233, 310)] * 2
    n, h, w = (int(v) for v in case.split("/")[0].split("x"))
    return [(h, w)] * n


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def kernels_ms(fn, names, reps=3):
    spv.profile_reset()
    spv.profile_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    spv.profile_enable(False)
    return {k: spv.profile_read(k)[1] / reps for k in names}


def run_case(case):
    shapes = shapes_of(case)
    n = len(shapes)
    ngroups = int(case.split("/")[1]) if "/" in case else 1
    ims = [texture(1000 + i, h, w) for i, (h, w) in enumerate(shapes)]
    flat = torch.cat([im.reshape(-1) for im in ims])
    pix_off = np.concatenate([[0], np.cumsum([h * w for h, w in shapes])]).astype(np.int64)
    sizes = np.array([(w, h) for h, w in shapes], np.int32)
    plan = spv.sift_batch_plan(sizes)
    ws_bytes = plan["workspace_bytes"]
    if ngroups > 1:  # the least workspace that gives at most ngroups groups
        lo, hi = plan["min_workspace_bytes"], plan["workspace_bytes"]
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if spv.sift_batch_plan(sizes, mid)["groups"] <= ngroups else (mid + 1, hi)
        ws_bytes = lo
    groups = spv.sift_batch_plan(sizes, ws_bytes)["groups"]
    assert groups == ngroups, (groups, ngroups)
    ws_batch = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    ws_loop = torch.empty(max(clib.spv_sift_workspace_bytes(w, h) for h, w in shapes), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def batch_into(table, cap_off, counts):
        check(clib.spv_sift_batch_device(flat.data_ptr(), sizes.ctypes.data, n, ws_batch.data_ptr(), ws_batch.numel(),
                                         table.data_ptr(), cap_off.ctypes.data, counts.data_ptr(), stream))

    def loop_into(table, cap_off, counts):
        for i, (h, w) in enumerate(shapes):
            check(clib.spv_sift_device(flat.data_ptr() + 4 * int(pix_off[i]), w, h, ws_loop.data_ptr(), ws_loop.numel(),
                                       table.data_ptr() + 528 * int(cap_off[i]), int(cap_off[i + 1] - cap_off[i]),
                                       counts.data_ptr() + 4 * i, stream))

    # the true counts first, then both forms with exact capacities
    none = torch.empty((1, 132), dtype=torch.float32, device="cuda")
    counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    batch_into(none, np.zeros(n + 1, np.int64), counts)
    rows = counts.cpu().numpy().astype(np.int64)
    cap_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    tb = torch.zeros((int(cap_off[-1]), 132), dtype=torch.float32, device="cuda")
    tl = torch.zeros_like(tb)
    cb, cl = torch.zeros_like(counts), torch.zeros_like(counts)

    def batch():
        batch_into(tb, cap_off, cb)

    def loop():
        loop_into(tl, cap_off, cl)

    batch(), loop()  # warm-up: code objects, workspaces
    torch.cuda.synchronize()
    same = bool(torch.equal(cb, cl) and torch.equal(cb, counts) and torch.equal(tb.view(torch.int32), tl.view(torch.int32)))
    rec = {"metric": "SIFT of a collection of images, ms per collection", "case": case,
           "config": {"images": n, "shapes_hgt_wid": sorted(set(shapes)), "groups": groups, "workspace_bytes": int(ws_bytes),
                      "pixels": plan["pixels"], "rows": int(cap_off[-1])},
           "unit": "ms", "dtype": "f32", "data": "synthetic (smoothed noise)", "window_s": args.window,
           "rounds": args.rounds, "forms_agree": same}
    calls = {"batch": batch, "loop": loop}
    reps = {name: max(1, math.ceil(args.window * 1e3 / window(fn, 1))) for name, fn in calls.items()}
    times = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            times[name].append(window(fn, reps[name]))
    for name, ms in times.items():
        rec[name] = {"ms": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms), "spread_ms": max(ms) - min(ms),
                     "reps_per_window": reps[name]}
    rec["loop_over_batch"] = rec["loop"]["ms"] / rec["batch"]["ms"]
    # the requirement: the batch median below the loop median by more than the larger of the two spreads
    rec["batch_below_loop_by_more_than_the_spreads"] = bool(
        rec["loop"]["ms"] - rec["batch"]["ms"] > max(rec["loop"]["spread_ms"], rec["batch"]["spread_ms"]))
    rec["batch"]["kernels_ms"] = kernels_ms(batch, BATCH_NAMES)
    rec["loop"]["kernels_ms"] = kernels_ms(loop, LOOP_NAMES)
    return rec


def main():
    recs = []
    for case in args.cases.split(","):
        rec = run_case(case)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("sift_batch_bench.py needs a GPU: it measures and has nothing to fall back to")
    main()
