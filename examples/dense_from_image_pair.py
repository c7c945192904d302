"""From two calibrated images to a dense point cloud, everything resident in HBM.

The step after rectification: `device.rectify_batch` -> `device.stereo_batch(both=True)` (block-matching
disparity along the rectified rows, both directions) -> `device.stereo_keep_batch` (left-right and uniqueness
tests) -> `device.stereo_matches_batch` (the kept samples as pixel correspondences) ->
`device.dlt_triangulate_batch`.  The scene is a textured plane z = 4 + 0.25 x seen by two cameras whose
poses are known, so the cloud can be held against the plane: the script prints the counts, the warm time of every
step and the distances of the points from the plane.

    python examples/dense_from_image_pair.py [--wid 96 --hgt 64] [--radius 7] [--dmin -24 --dmax 8] [--seed 1]

(the disparity range scales with the image: -24..8 is right for 96 x 64)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectavi_amd.scenes import plane_distance, plane_scene  # noqa: E402


def dense_cloud(ims, sizes, pairs, P0s, P1s, radius, drange, lr_tol=1, uniqueness=10, sampling_factor=1.2, timer=None):
    """The chain on the device for a collection of pairs: (X float64 CUDA [n, 4], pair_off, stats)."""
    from spectavi_amd import device
    tick = timer or (lambda name: None)
    r0, r1, ri0, ri1, box, out_off = device.rectify_batch(ims, sizes, pairs, P1s, P0s, sampling_factor=sampling_factor)
    tick("rectify_batch")
    (disp0, cost0, cost20), (disp1, _, _) = device.stereo_batch(r0, r1, ri0, ri1, box, drange, radius=radius, both=True)
    tick("stereo_batch")
    keep = device.stereo_keep_batch(box, disp0, cost0, cost20, disp1, lr_tol=lr_tol, uniqueness=uniqueness)
    tick("stereo_keep_batch")
    if sizes is None:
        sizes = [(im.shape[1], im.shape[0]) for im in ims]
    x0, x1, _, pair_off = device.stereo_matches_batch(box, sizes, pairs, disp0, keep, ri0, ri1)
    tick("stereo_matches_batch")
    X, _ = device.dlt_triangulate_batch(x0, x1, pair_off, P1s, P0s)
    tick("dlt_triangulate_batch")
    stats = dict(samples=int(out_off[-1]), with_disparity=int((disp0 != device.STEREO_NONE).sum()), kept=int(pair_off[-1]))
    return X, pair_off, stats


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--wid", type=int, default=96)
    ap.add_argument("--hgt", type=int, default=64)
    ap.add_argument("--radius", type=int, default=7)
    ap.add_argument("--dmin", type=int, default=-24)
    ap.add_argument("--dmax", type=int, default=8)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    import torch
    im0, im1, P0, P1 = plane_scene(a.wid, a.hgt, a.seed)
    ims = [torch.from_numpy(im0).cuda(), torch.from_numpy(im1).cuda()]
    times = {}

    def timer(name):
        torch.cuda.synchronize()
        now = time.perf_counter()
        times[name] = now - timer.last
        timer.last = now
    for warm in (False, True):  # the second pass is timed
        torch.cuda.synchronize()
        timer.last = time.perf_counter()
        X, pair_off, stats = dense_cloud(ims, None, [(0, 1)], [P0], [P1], a.radius, (a.dmin, a.dmax), timer=timer)
    X = X.cpu().numpy()
    pts = X[:, :3] / X[:, 3:4]
    dist = plane_distance(pts)
    print("window samples %d, with a disparity %d, kept %d (%.3f of those with a disparity)"
          % (stats["samples"], stats["with_disparity"], stats["kept"], stats["kept"] / max(stats["with_disparity"], 1)))
    for name, s in times.items():
        print("  %-22s %8.3f ms (warm, wall, ending in a synchronise)" % (name, s * 1e3))
    if len(dist):
        print("distance from the plane: median %.3f, max %.3f (depth about 4)" % (np.median(dist), dist.max()))


if __name__ == "__main__":
    main()
