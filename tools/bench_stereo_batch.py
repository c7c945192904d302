"""Measures device.stereo_batch on one GPU against a plain PyTorch statement of the same op, and writes one JSON
line per case to profiles/stereo_batch.jsonl (--out), replacing the file.  A case whose outputs differ from the PyTorch
statement's is not recorded: the run ends with a non-zero status.  Everything is resident in HBM.

Workload of record: the textured plane of spectavi_amd/scenes.py rendered at 1280 x 960, rectified by
device.rectify_batch (sf 1.2, cropped), radius 3, 128 disparities (-112..15), both directions, 1 pair and 15 pairs
(the same two images 15 times: every pair has its own window).  Warm; three runs of each form, alternating, median
and range.  Per run: the kernel time from the library's event brackets (spv_profile_read "stereo_batch": one bracket
per direction) in a pass of its own, and the wall time of the call ending in a synchronise.

  naive-equivalent rate   samples x disparities x (2r + 1)^2 / 4 SAD lane-operations over the kernel time of one
                          direction, as a share of the v_sad_u8 issue peak BASELINE.md uses (256 x 64 x 2.4e9 / s).
                          It counts the work of the definition, not the instructions issued: a form that reuses row
                          sums may exceed 1 by this account.
  torch                   per d: abs of the shifted difference, a box sum by avg_pool2d(divisor_override=1), a running
                          minimum under the admissibility mask -- float32 holds these integers exactly, so disp and
                          cost are checked equal to the library's.

  python tools/bench_stereo_batch.py [--pairs 1,15] [--runs 3] [--wid 1280 --hgt 960]
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="directory to import spectavi_amd from")
ap.add_argument("--pairs", default="1,15")
ap.add_argument("--wid", type=int, default=1280)
ap.add_argument("--hgt", type=int, default=960)
ap.add_argument("--radius", type=int, default=3)
ap.add_argument("--dmin", type=int, default=-112)
ap.add_argument("--dmax", type=int, default=15)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None, help="the JSONL file to write (default profiles/stereo_batch.jsonl); replaced")
args = ap.parse_args()
sys.path.insert(0, args.root)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from spectavi_amd import device as spv  # noqa: E402
from spectavi_amd.scenes import plane_scene  # noqa: E402

SAD_PEAK = 256 * 64 * 2.4e9  # v_sad_u8 lane-operations per second
NONE = spv.STEREO_NONE


def torch_stereo(ref, oth, ok_ref, ok_oth, r, d_lo, d_hi):
    """One direction of one window, [R, C] tensors: (disp int32, cost float32 with inf where none)."""
    R, C = ref.shape
    a, b = ref.float(), oth.float()
    inner = torch.zeros((R, C), dtype=torch.bool, device=ref.device)
    if R > 2 * r and C > 2 * r:
        inner[r:R - r, r:C - r] = True
    adm_ref, adm_oth = ok_ref & inner, ok_oth & inner
    best = torch.full((R, C), float("inf"), device=ref.device)
    disp = torch.full((R, C), NONE, dtype=torch.int32, device=ref.device)
    for d in range(max(d_lo, -(C - 1)), min(d_hi, C - 1) + 1):
        x0, x1 = max(0, -d), min(C, C - d)
        diff = torch.zeros((R, C), device=ref.device)
        diff[:, x0:x1] = (a[:, x0:x1] - b[:, x0 + d:x1 + d]).abs()
        s = F.avg_pool2d(diff[None, None], 2 * r + 1, stride=1, padding=r, divisor_override=1)[0, 0]
        adm = torch.zeros((R, C), dtype=torch.bool, device=ref.device)
        adm[:, x0:x1] = adm_ref[:, x0:x1] & adm_oth[:, x0 + d:x1 + d]
        c = torch.where(adm, s, best.new_tensor(float("inf")))
        upd = c < best
        best = torch.where(upd, c, best)
        disp = torch.where(upd, disp.new_tensor(d), disp)
    return disp, best


def case(npairs):
    im0, im1, P0, P1 = plane_scene(args.wid, args.hgt, 1)
    ims = [torch.from_numpy(im0).cuda(), torch.from_numpy(im1).cuda()]
    pairs = [(0, 1)] * npairs
    r0, r1, ri0, ri1, box, off = spv.rectify_batch(ims, None, pairs, [P1] * npairs, [P0] * npairs)
    drange, r = (args.dmin, args.dmax), args.radius
    nd = args.dmax - args.dmin + 1
    samples = int(off[-1])

    def lib():
        return spv.stereo_batch(r0, r1, ri0, ri1, box, drange, radius=r, both=True)

    def tor():
        out = []
        for p in range(npairs):
            w = [spv.rectify_batch_view(t, p, box, off) for t in (r0, r1, ri0, ri1)]
            out.append((torch_stereo(w[0], w[1], w[2] != -1, w[3] != -1, r, *drange),
                        torch_stereo(w[1], w[0], w[3] != -1, w[2] != -1, r, -drange[1], -drange[0])))
        return out

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    (d0, c0, _), (d1, c1, _) = lib()  # warm-up, and the outputs to compare
    t_out = tor()
    equal = True
    for p in range(npairs):
        for (td, tc), ld, lc in ((t_out[p][0], d0, c0), (t_out[p][1], d1, c1)):
            wd, wc = spv.rectify_batch_view(ld, p, box, off), spv.rectify_batch_view(lc, p, box, off)
            has = td != NONE
            equal = equal and bool((wd == td).all()) and bool((wc.to(torch.int32)[has] == tc[has].to(torch.int32)).all())
            equal = equal and bool((wc.to(torch.int32)[~has] == 0xFFFF).all())
    del t_out
    if not equal:
        sys.exit("bench_stereo_batch.py: disp or cost of %d pair(s) differ from the PyTorch statement's; nothing recorded" % npairs)
    walls = {"library": [], "torch": []}
    for _ in range(args.runs):  # alternating
        walls["library"].append(wall(lib))
        walls["torch"].append(wall(tor))
    kern = []
    for _ in range(args.runs):
        spv.profile_reset()
        spv.profile_enable(True)
        lib()
        torch.cuda.synchronize()
        spv.profile_enable(False)
        n, ms = spv.profile_read("stereo_batch")
        assert n == 2
        kern.append(ms / 2)  # per direction

    def stat(v):
        return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    k = stat(kern)
    naive = samples * nd * (2 * r + 1) ** 2 / 4.
    rec = {"metric": "stereo_batch, both directions of every pair", "unit": "ms", "data": "rendered plane, random texture",
           "config": {"image": "%d x %d" % (args.wid, args.hgt), "pairs": npairs, "radius": r, "disparities": nd,
                      "drange": list(drange), "window": [int(v) for v in box[0]], "samples": samples, "runs": args.runs},
           "kernel_ms_per_direction": k,
           "kernel_ms_per_direction_and_pair": {q: v / npairs for q, v in k.items()},
           "wall_ms_both_directions": {"library": stat(walls["library"]), "torch": stat(walls["torch"])},
           "naive_equivalent_sad_lane_ops_per_s": naive / (k["median"] * 1e-3),
           "naive_equivalent_share_of_v_sad_u8_peak": naive / (k["median"] * 1e-3) / SAD_PEAK,
           "torch_over_library_wall": float(np.median(walls["torch"]) / np.median(walls["library"])),
           "library_faster_in_every_run": bool(max(walls["library"]) < min(walls["torch"])),
           "disp_and_cost_equal_torch": equal}
    return rec


def main():
    out = args.out or os.path.join(args.root, "profiles", "stereo_batch.jsonl")
    lines = []
    for n in [int(v) for v in args.pairs.split(",")]:
        lines.append(json.dumps(case(n)))  # (exits where the outputs differ)
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_stereo_batch.py needs a GPU: it measures and has nothing to fall back to")
    main()
