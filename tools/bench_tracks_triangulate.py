"""Measures device.triangulate_tracks on one GPU and prints one JSON line per input.

Inputs, both of --tracks tracks over --views views of one synthetic scene (tests/tracks_triangulate_model.py's: K with
f = 1000, rotations of 0.05-0.25 rad, centres at distance 1, 0.5 px noise):
  short   track lengths drawn from the shape of examples/multiview_from_sift_tables.py's histogram: mostly 2-6 members,
          a tail to 40
  tail    the same with 1 % of the tracks at 200-2000 members
For each input the call is timed with the lane/wave threshold L (tracks_triangulate_set_long) at 8, 16, 32, 64 and
"never" (no track takes the wave form).  Every figure is a device-event time around a window of back-to-back calls of
at least --window seconds, after a warm-up of every setting; the settings alternate window by window in one process,
and the spread is over the windows of a setting.  The call includes the host's share -- the plan over track_off and the
upload of the tables (track_off is 8 bytes a track) -- behind which the kernels of back-to-back calls hide, so
`kernels_ms`, the two kernels by the library's event brackets, is taken beside it: five calls per setting after every
round of windows, median and range over the rounds.

Two references, since the op has no predecessor:
  bytes   what the call must move -- members (8 B each), one gathered geom row per member (16 B; the 32 B sector the
          hardware fetches is given too), the outputs (32 + 1 + 4 B a track, 8 B a member) -- over 6.29 TB/s, the
          measured HBM copy rate of the MI355X
  host    the numpy model of tests/tracks_triangulate_model.py on a sample of --model-tracks tracks of the same input,
          scaled to the whole input by the member count (not run on the whole input: it is a Python loop)

  python tools/bench_tracks_triangulate.py [--tracks 1000000] [--views 64] [--window 1.0] [--rounds 5]
"""
import argparse
import json
import math
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tracks", type=int, default=1000000)
ap.add_argument("--views", type=int, default=64)
ap.add_argument("--points", type=int, default=65536, help="scene points; tracks share them")
ap.add_argument("--window", type=float, default=1.0, help="seconds of device time per timed window, at least")
ap.add_argument("--rounds", type=int, default=5, help="windows per setting")
ap.add_argument("--model-tracks", type=int, default=5000)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectavi_amd import device as spv  # noqa: E402
from tests import tracks_triangulate_model as ttm  # noqa: E402

HBM_BYTES_PER_S = 6.29e12
SETTINGS = (("8", 8), ("16", 16), ("32", 32), ("64", 64), ("never", 2 ** 31 - 1))
NAMES = ("tracks_triangulate", "tracks_triangulate_long")


def window(fn, reps):
    """ms per call over `reps` back-to-back calls, by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def lengths_of(rng, n, tail):
    """Mostly 2-6 (geometric from 2), a thin tail to 40; with `tail`, 1 % of the tracks at 200-2000."""
    length = 2 + rng.geometric(0.45, n) - 1
    far = rng.random(n) < 0.02
    length[far] = rng.integers(7, 41, int(far.sum()))
    length = np.minimum(length, 40)
    if tail:
        big = rng.random(n) < 0.01
        length[big] = rng.integers(200, 2001, int(big.sum()))
    return length.astype(np.int64)


def collection(ntracks, views, npoints, tail, seed=9):
    rng = np.random.default_rng(seed)
    cams = ttm.wide_cameras(rng, views)
    geom, seg = ttm.observe(rng, cams, ttm.points(rng, npoints), 0.5)
    length = lengths_of(rng, ntracks, tail)
    off = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    nm = int(off[-1])
    point = np.repeat(rng.integers(0, npoints, ntracks), length)
    sets = rng.integers(0, views, nm)
    first = off[:-1]
    sets[first + 1] = (sets[first] + 1 + rng.integers(0, views - 1, ntracks)) % views   # two different views at least
    return cams, geom, seg, off, np.stack([sets, point], 1).astype(np.int32), length


def main():
    before = spv.tracks_triangulate_get_long()
    for name, tail in (("short", False), ("tail", True)):
        cams, geom, seg, off, mem, length = collection(args.tracks, args.views, args.points, tail)
        nt, nm = len(length), len(mem)
        tg, tm_ = torch.from_numpy(geom).cuda(), torch.from_numpy(mem).cuda()

        def call():
            return spv.triangulate_tracks(tg, seg, cams, off, tm_, max_error=3.0)
        rec = {"metric": "N-view DLT of every track, ms per call", "input": name, "unit": "ms", "data": "synthetic",
               "config": {"tracks": nt, "members": nm, "views": args.views, "longest": int(length.max()),
                          "mean_length": float(length.mean())},
               "window_s": args.window, "rounds": args.rounds}
        outs, plans = {}, {}
        for label, L in SETTINGS:                                   # warm-up of every setting, and the outputs
            spv.tracks_triangulate_set_long(L)
            plans[label] = spv.triangulate_tracks_plan(off)
            outs[label] = [t.cpu().numpy() for t in call()]
        base = outs["never"]
        rec["ok_tracks"] = int(base[2].sum())
        rec["max_abs_X_difference_from_never"] = {k: float(np.abs(o[0] - base[0]).max()) for k, o in outs.items()}
        rec["ok_equal_to_never"] = {k: bool(np.array_equal(o[2], base[2])) for k, o in outs.items()}
        del outs
        reps, times = {}, {label: [] for label, _ in SETTINGS}
        kernels = {label: {k: [] for k in NAMES} for label, _ in SETTINGS}
        for label, L in SETTINGS:
            spv.tracks_triangulate_set_long(L)
            reps[label] = max(1, math.ceil(args.window * 1e3 / window(call, 1)))
        for _ in range(args.rounds):
            for label, L in SETTINGS:
                spv.tracks_triangulate_set_long(L)
                times[label].append(window(call, reps[label]))
            for label, L in SETTINGS:                               # the kernels alone, in passes of their own
                spv.tracks_triangulate_set_long(L)
                spv.profile_reset()
                spv.profile_enable(True)
                for _ in range(5):
                    call()
                torch.cuda.synchronize()
                spv.profile_enable(False)
                for k in NAMES:
                    kernels[label][k].append(spv.profile_read(k)[1] / 5)
        for label, L in SETTINGS:
            ms = times[label]
            med = float(np.median(ms))
            both = [sum(v) for v in zip(*(kernels[label][k] for k in NAMES))]
            rec["L=" + label] = {"ms": med, "ms_min": min(ms), "ms_max": max(ms), "spread": (max(ms) - min(ms)) / med,
                                 "reps_per_window": reps[label], "plan": plans[label],
                                 "kernels_ms": {k: float(np.median(kernels[label][k])) for k in NAMES},
                                 "kernels_sum_ms": {"median": float(np.median(both)), "min": min(both), "max": max(both)}}
        spv.profile_reset()
        spv.tracks_triangulate_set_long(before)
        must = nm * 8 + nm * 16 + nt * (32 + 1 + 4) + nm * 8
        rec["bytes_moved_at_least"] = must
        rec["bytes_with_32B_sectors"] = must + nm * 16
        rec["hbm_floor_ms"] = must / HBM_BYTES_PER_S * 1e3
        for label, _ in SETTINGS:
            k = rec["L=" + label]["kernels_sum_ms"]["median"]
            rec["L=" + label]["kernels_over_hbm_floor"] = k / rec["hbm_floor_ms"]
        # the numpy model on a sample, scaled by members
        ns = min(args.model_tracks, nt)
        s = time.perf_counter()
        ttm.model(geom, seg, cams, off[:ns + 1], mem[:int(off[ns])], max_error=3.0)
        model_s = (time.perf_counter() - s) * nm / max(int(off[ns]), 1)
        rec["numpy_model_ms_scaled_from_%d_tracks" % ns] = model_s * 1e3
        rec["numpy_model_over_call"] = {label: model_s * 1e3 / rec["L=" + label]["ms"] for label, _ in SETTINGS}
        rec["fastest_call"] = min((rec["L=" + label]["ms"], label) for label, _ in SETTINGS)[1]
        rec["fastest_kernels"] = min((rec["L=" + label]["kernels_sum_ms"]["median"], label) for label, _ in SETTINGS)[1]
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_tracks_triangulate.py needs a GPU: it measures and has nothing to fall back to")
    main()
