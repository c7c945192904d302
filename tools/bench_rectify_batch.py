"""Measures the many-pairs rectification (device.rectify_batch) on one GPU against the loop a user ran before it, and
prints one JSON line per case.  Everything is resident in HBM.  A figure is wall time per collection over a window of
back-to-back calls of at least --window seconds with the device synchronised at both ends, after a warm-up of every
form; the forms alternate, window by window, in one process, and the median and the spread are over the windows of a
form.  The kernels alone come from the library's event brackets (spv_profile_read), in passes of their own.

  python tools/bench_rectify_batch.py
  python tools/bench_rectify_batch.py --cases vga --dtypes uint8 --rounds 9

Cases: 12 gray views and all their 66 pairs, `vga` 480 x 640 and `big` 960 x 1280, sampling factor 1.2.
Forms:
  batch       device.rectify_batch(crop_invalid=True): bounds, one read-back of the boxes, one resampling launch
  loop        device.image_pair_rectification per pair (whole frames, no crop, nothing read back)
  loop_crop   the same plus the front-end's crop per pair: both index images read back, the box found on the host,
              the four tensors sliced
float32 is timed on the batch side only: the loop has no float32 form (the single call takes float64 and uint8)."""
import argparse
import itertools
import json
import math
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="directory to import spectavi_amd from")
ap.add_argument("--cases", default="vga,big")
ap.add_argument("--dtypes", default="uint8,float64,float32")
ap.add_argument("--views", type=int, default=12)
ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window, at least")
ap.add_argument("--rounds", type=int, default=5, help="windows per form")
ap.add_argument("--out", default=None, help="also write the records, a JSON list, to this file")
args = ap.parse_args()
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectavi_amd import device as spv  # noqa: E402
from spectavi_amd import mvg  # noqa: E402
from tests.test_rectify_gpu import pair  # noqa: E402

SF = 1.2
HBM_PEAK_GBS = 8000.  # MI355X: 8 TB/s


def window(fn, reps):
    """ms per call over `reps` back-to-back calls."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def kernels_ms(fn, names, reps=3):
    """{name: ms per call} from the library's event brackets over `reps` calls."""
    spv.profile_reset()
    spv.profile_enable(True)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    spv.profile_enable(False)
    return {k: spv.profile_read(k)[1] / reps for k in names}


def measure(calls, rec):
    reps = {name: max(1, math.ceil(args.window * 1e3 / window(fn, 1))) for name, fn in calls.items()}
    times = {name: [] for name in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            times[name].append(window(fn, reps[name]))
    for name, ms in times.items():
        med = float(np.median(ms))
        rec[name] = {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "spread": (max(ms) - min(ms)) / med,
                     "reps_per_window": reps[name]}
    return times


def case(name, hgt, wid, dtype):
    rng = np.random.default_rng(hgt)
    tdt = {"uint8": torch.uint8, "float64": torch.float64, "float32": torch.float32}[dtype]
    esize = {"uint8": 1, "float64": 8, "float32": 4}[dtype]
    ims = [torch.from_numpy(rng.integers(0, 256, (hgt, wid), dtype=np.uint8)).cuda().to(tdt) for _ in range(args.views)]
    pairs = list(itertools.combinations(range(args.views), 2))
    cams = [pair(rng, hgt, wid, baseline=(-0.25 - 0.01 * p, 0.01 * ((p % 5) - 2), 0.02)) for p in range(len(pairs))]
    P0s, P1s = [c[0] for c in cams], [c[1] for c in cams]
    packed = torch.cat([im.reshape(-1) for im in ims])
    sizes = [(wid, hgt)] * args.views

    def batch():
        return spv.rectify_batch(packed, sizes, pairs, P1s, P0s, sampling_factor=SF)

    def loop():
        for (a, b), P0, P1 in zip(pairs, P0s, P1s):
            spv.image_pair_rectification(P0, P1, ims[a], ims[b], sampling_factor=SF)

    def loop_crop():
        for (a, b), P0, P1 in zip(pairs, P0s, P1s):
            r0, r1, ri0, ri1 = spv.image_pair_rectification(P0, P1, ims[a], ims[b], sampling_factor=SF)
            y, x = np.where((ri0.cpu().numpy() != -1) | (ri1.cpu().numpy() != -1))
            ys, xs = slice(y.min(), y.max() + 1), slice(x.min(), x.max() + 1)
            r0, r1, ri0, ri1 = r0[ys, xs], r1[ys, xs], ri0[ys, xs], ri1[ys, xs]

    r0, r1, ri0, ri1, box, off = batch()  # warm-up: code objects, the cached tables
    rows, cols, _ = mvg.rectification_shape(wid, hgt, 1, SF)
    window_share = float(off[-1]) / (len(pairs) * rows * cols)
    batch_bytes = int(off[-1]) * 2 * (esize + 4)
    loop_bytes = len(pairs) * rows * cols * 2 * (esize + 4)
    rec = {"metric": "rectification of all pairs of a view set, ms per collection",
           "config": {"workload": "%d views, %d pairs, %d x %d gray, sf %.1f" % (args.views, len(pairs), hgt, wid, SF)},
           "case": name, "unit": "ms", "dtype": dtype, "data": "synthetic", "window_s": args.window,
           "rounds": args.rounds, "window_share_of_frame": window_share, "batch_bytes_written": batch_bytes,
           "loop_bytes_written": loop_bytes}
    calls = {"batch": batch}
    if dtype != "float32":
        # the forms agree: pair 0's window is the slice of the single call
        s = spv.image_pair_rectification(P0s[0], P1s[0], ims[0], ims[1], sampling_factor=SF)
        b = box[0]
        rec["forms_agree"] = bool(
            (spv.rectify_batch_view(ri0, 0, box, off) == s[2][b[0]:b[1], b[2]:b[3]]).all() and
            (spv.rectify_batch_view(r0, 0, box, off) == s[0][b[0]:b[1], b[2]:b[3]]).all())
        del s
        loop()
        loop_crop()
        calls.update(loop=loop, loop_crop=loop_crop)
    else:
        rec["note"] = "the loop has no float32 form: batch only"
    del r0, r1, ri0, ri1
    times = measure(calls, rec)
    k = kernels_ms(batch, ("rectify_batch_bounds", "rectify_batch_box", "rectify_batch"))
    rec["batch"]["kernels_ms"] = k
    rec["batch"]["store_GBps"] = batch_bytes / (k["rectify_batch"] * 1e-3) / 1e9
    rec["batch"]["store_share_of_hbm_peak"] = rec["batch"]["store_GBps"] / HBM_PEAK_GBS
    if dtype != "float32":
        kl = kernels_ms(loop, ("rectify",), reps=2)
        rec["loop"]["kernels_ms"] = kl
        rec["loop"]["store_GBps"] = loop_bytes / (kl["rectify"] * 1e-3) / 1e9
        for form in ("loop", "loop_crop"):
            rec["%s_over_batch" % form] = rec[form]["ms"] / rec["batch"]["ms"]
            rec["batch_faster_than_%s_in_every_window" % form] = bool(max(times["batch"]) < min(times[form]))
    return rec


def main():
    shapes = {"vga": (480, 640), "big": (960, 1280)}
    recs = []
    for name in args.cases.split(","):
        for dtype in args.dtypes.split(","):
            rec = case(name, *shapes[name], dtype)
            print(json.dumps(rec), flush=True)
            recs.append(rec)
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_rectify_batch.py needs a GPU: it measures and has nothing to fall back to")
    main()
