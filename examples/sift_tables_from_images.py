"""Step 1 of a multi-view pipeline: the SIFT tables of N images in one chain of launches, handed straight to matching.

examples/multiview_from_sift_tables.py starts from SIFT tables; this file makes them.  Overlapping crops of one
smooth random texture stand in for the views (the true displacement between two crops is the difference of their
offsets), and every intermediate stays in HBM:

    sift_batch(want_split=True)  vlfeat-exact SIFT of all crops: geometry, descriptors and seg_off
    l1k2_batch                   exact L1 2-NN of every (query crop, database crop) pair
    ratio_test                   over the concatenated result
    match_coordinates_batch      matches -> per-pair pixel coordinates and pair_off

Per pair it prints the number of matches and the median displacement of the matched keypoints next to the crops'
offset.

    python examples/sift_tables_from_images.py [--crops 5] [--size 240 320]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def smooth_random(seed, h, w, passes=3):
    """Uniform noise in [0, 255) smoothed by `passes` circular [1 1 1]/3 passes along each axis."""
    r = np.random.default_rng(seed).random((h, w)) * 255
    for _ in range(passes):
        r = (r + np.roll(r, 1, 0) + np.roll(r, -1, 0)) / 3
        r = (r + np.roll(r, 1, 1) + np.roll(r, -1, 1)) / 3
    return r.astype(np.float32)


def crops_of_texture(seed, n, h, w, step=(7, 11)):
    """n crops of h x w pixels of one texture, crop i at offset (i * step[0], i * step[1]) = (dy, dx)."""
    tex = smooth_random(seed, h + (n - 1) * step[0], w + (n - 1) * step[1])
    offsets = [(i * step[0], i * step[1]) for i in range(n)]
    return [np.ascontiguousarray(tex[dy:dy + h, dx:dx + w]) for dy, dx in offsets], offsets


def match_crops(crops, min_ratio=1.75):
    """crops (float32 [h, w] arrays, any sizes) -> dict: seg_off (keypoints per crop), pairs int32 [npairs, 2] (query
    crop, database crop), pair_off (matches per pair), x0 / x1 (CUDA float64 [matches, 3]: the matched keypoints'
    pixel coordinates in the database and the query crop)."""
    import torch
    from spectavi_amd import device as spv
    geom, desc, seg_off = spv.sift_batch([torch.from_numpy(c).cuda() for c in crops], want_split=True)
    n = len(crops)
    pairs = np.array([(q, d) for d in range(n) for q in range(d + 1, n)], np.int32).reshape(-1, 2)
    idx, dist, _ = spv.l1k2_batch(desc, seg_off, pairs)
    matches, count = spv.ratio_test(idx, dist, min_ratio)
    x0, x1, pair_off = spv.match_coordinates_batch(geom, seg_off, pairs, matches, count)
    return {'seg_off': seg_off, 'pairs': pairs, 'pair_off': pair_off, 'x0': x0[:pair_off[-1]], 'x1': x1[:pair_off[-1]]}


def report(out, offsets):
    print("keypoints per crop: %s" % np.diff(out['seg_off']).tolist())
    for p, (q, d) in enumerate(out['pairs'].tolist()):
        lo, hi = int(out['pair_off'][p]), int(out['pair_off'][p + 1])
        want = (offsets[q][1] - offsets[d][1], offsets[q][0] - offsets[d][0])   # (dx, dy) of x0 - x1: query crop's offset minus database crop's
        if hi > lo:
            med = (out['x0'][lo:hi, :2] - out['x1'][lo:hi, :2]).median(dim=0).values.tolist()
            print("pair %d-%d: matches %4d  median displacement (%+.2f, %+.2f)  crop offset (%+d, %+d)" % (
                d, q, hi - lo, med[0], med[1], want[0], want[1]))
        else:
            print("pair %d-%d: matches    0  crop offset (%+d, %+d)" % (d, q, want[0], want[1]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--crops", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=(240, 320), metavar=("HGT", "WID"))
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    crops, offsets = crops_of_texture(a.seed, a.crops, a.size[0], a.size[1])
    for rep in range(2):  # the second round is the warm one
        torch.cuda.synchronize()
        s = time.perf_counter()
        out = match_crops(crops)
        torch.cuda.synchronize()
        dt = time.perf_counter() - s
    report(out, offsets)
    print("%d crops of %d x %d, %d keypoints, %d matches, %.1f ms (warm, uploads included)" % (
        a.crops, a.size[0], a.size[1], int(out['seg_off'][-1]), int(out['pair_off'][-1]), dt * 1e3))


if __name__ == "__main__":
    main()
