"""Steps 2-4 (with --rectify also step 5) of the reference's example pipeline for every image pair of a view set, one
call per step.

examples/essential_from_sift_tables.py runs matching, RANSAC and triangulation for ONE image pair, as the reference's
example/ex01_essential_estimation.py does.  A multi-view front-end has N views and up to N (N - 1) / 2 pairs; this file
runs all of them through the many-pairs forms of the same steps, with every intermediate resident in HBM:

    l1k2_batch               exact L1 2-NN of every (query view, database view) pair; or, with --matcher cascade,
    normalize_batch          every view's uint8 descriptors normalised per view, as the reference's front-end does, and
    cascade_batch            the cascade hash + L1 refine of every pair, each view coded and bucket-sorted once
    ratio_test               over the concatenated result
    match_coordinates_batch  matches -> per-pair homogeneous coordinates and pair_off
    ransac_fit_batch         one essential matrix and camera per pair, and the inlier mask over all rows
    dlt_triangulate_batch    every pair's inliers triangulated with that pair's camera; pairs without a model skipped
    rectify_batch            (--rectify) every fitted pair's two images rectified, cropped on the device to the valid
                             samples; the images are noise here, only the geometry is the pipeline's
    epipolar_lines_batch     (--guided PIXELS) every fitted pair's model as one line per query keypoint, and
    l1k2_guided_batch        the L1 2-NN again, only among the database keypoints within PIXELS of that line; the
                             same ratio test then holds more matches than the blind one
    tracks_batch             (--tracks) every pair's inlier matches linked into multi-view tracks: the connected
                             components of the keypoint graph; with --guided the second pass's matches are then
                             accumulated onto the same labels
    triangulate_tracks       (--triangulate PIXELS, with --tracks) one 3-D point per track from all its observations,
                             a residual per observation and a verdict per track.  The op takes one camera per view
                             as given; here they are the synthetic scene's own pixel cameras K [R | t]
    resect_gather            (--resect PIXELS, with --tracks) the cameras estimated instead, incrementally: the fitted
    resect_fit_batch         pair with the most inliers is registered as K [I | 0] and K camera, the tracks it sees are
                             triangulated, every other view is resected from the points its keypoints belong to -- all
                             of them in one call -- and the tracks are triangulated again over all registered views.
                             Chaining the other pairwise fits and their scales is not part of the library
    bundle_adjust            (--bundle, with --resect) every registered camera as a pose K [R | t] (pose_from_camera),
                             the two seed views fixed, and all other cameras and all ok track points refined together
                             over all their observations under a Huber loss of the --resect width

Only the small per-pair results (the fits, the offsets) come back on the way; the points stay on the device until
they are asked for.  The SIFT tables (rows of 132 float32: x, y, sigma, angle, 128 descriptor values) are synthetic
here, so that the scene and the cameras are known; extracting them from images is the library's sift_batch, the step
before l1k2_batch, which examples/sift_tables_from_images.py shows.

    python examples/multiview_from_sift_tables.py [--images 6] [--points 2000] [--matcher {l1k2,cascade}] [--rectify]
                                                  [--guided PIXELS] [--tracks] [--triangulate PIXELS] [--resect PIXELS]
                                                  [--bundle]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_sift_views(seed=0, n_views=6, n_points=2000, n_extra=None, wrong_fraction=0.08, desc_noise=6.0,
                         return_cameras=False):
    """SIFT tables of one scene seen by n_views calibrated cameras (the first at [I|0]).  Every scene point appears
    in every table, its descriptor perturbed by N(0, desc_noise) per component and view; in every view but the first
    a `wrong_fraction` of them sits at an unrelated position (a descriptor match that is a geometric outlier), and
    n_extra unrelated keypoints are added to each table.  Rows are shuffled per view.  Returns (tables, K); with
    return_cameras (tables, K, cameras), cameras float64 [n_views,3,4] the scene's pixel cameras K [R | t]."""
    rng = np.random.default_rng(seed)
    n_extra = n_points // 2 if n_extra is None else n_extra
    K = np.array([[1000.0, 0.0, 640.0], [0.0, 1000.0, 480.0], [0.0, 0.0, 1.0]])
    X = np.c_[rng.uniform(-2.5, 2.5, n_points), rng.uniform(-1.8, 1.8, n_points), rng.uniform(4, 8, n_points)]

    def descriptors(n):  # SIFT-like: non-negative, unit norm, stored as uint8(512 d) (src/Sift.h:118-121)
        d = np.abs(rng.standard_normal((n, 128))) ** 2
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return np.minimum(np.floor(512.0 * d), 255.0)

    d_scene = descriptors(n_points)
    tables, cameras = [], []
    for v in range(n_views):
        R, t = np.eye(3), np.zeros(3)
        if v:
            a = rng.standard_normal(3)
            a /= np.linalg.norm(a)
            th = rng.uniform(0.05, 0.25) * rng.choice([-1, 1])
            S = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            R = np.eye(3) + np.sin(th) * S + (1 - np.cos(th)) * (S @ S)
            t = rng.standard_normal(3)
            t /= np.linalg.norm(t)
        cameras.append(K @ np.c_[R, t])
        Xc = X @ R.T + t
        pix = ((Xc / Xc[:, 2:]) @ K.T)[:, :2]
        if v:
            wrong = rng.choice(n_points, int(round(wrong_fraction * n_points)), replace=False)
            pix[wrong] = np.c_[rng.uniform(0, 1280, len(wrong)), rng.uniform(0, 960, len(wrong))]
        desc = np.clip(np.round(d_scene + desc_noise * rng.standard_normal(d_scene.shape)), 0, 255)
        pix = np.vstack([pix, np.c_[rng.uniform(0, 1280, n_extra), rng.uniform(0, 960, n_extra)]])
        desc = np.vstack([desc, descriptors(n_extra)])
        n = len(pix)
        table = np.hstack([pix, rng.uniform(1, 8, (n, 1)), rng.uniform(-np.pi, np.pi, (n, 1)), desc]).astype(np.float32)
        tables.append(table[rng.permutation(n)])
    if return_cameras:
        return tables, K, np.array(cameras)
    return tables, K


def multiview_pipeline(tables, K, min_ratio=1.75, required_percent_inliers=0.6, maximum_tries=2000, seed=1,
                       matcher='l1k2', hash_seed=0x5eed, guided=None, tracks=False, triangulate=None):
    """SIFT tables (a list of float32 [n_v,132] arrays) -> one upload -> split -> exact L1 2-NN of all pairs (or,
    matcher='cascade', the cascade hash of all pairs: descriptors normalised per view as the reference's front-end
    does, m by its rule from the largest view, n = 2, g = 2, hyperplanes from hash_seed) -> ratio
    test -> per-pair coordinates -> calibration -> one RANSAC fit per pair -> triangulation of every pair's inliers
    with that pair's camera.  Returns a dict: pairs int32 [npairs,2] (query view, database view), pair_off (matches
    per pair), fits (the `ransac_fit` dicts), out_off (points per pair), X (CUDA float64 [total,4], rows
    out_off[p]:out_off[p + 1] are pair p's unit-norm homogeneous points) and rows (CUDA int32: the match each point
    belongs to, numbered inside its pair).  With guided (pixels) also guided_pair_off: the matches per pair of the
    second pass, the same ratio test over the L1 2-NN inside a band of that half-width around each query's epipolar
    line in the database view; a pair without a model has none.  With tracks also tracks: `tracks_batch`'s (track_off,
    members, flags, label, track) over every pair's inlier matches and, with guided, the second pass's matches
    accumulated onto them; and track_inputs: the seg_off, matches, count and mask (and guided_matches, guided_count)
    those calls read.  With triangulate (one pixel camera [3,4] per view, e.g. synthetic_sift_views' own, or what
    resect_views below estimates) and tracks also track_points: `triangulate_tracks`' (X, err, ok, nused) of those tracks, ok
    without a residual bound (cheirality alone; call `triangulate_tracks` with max_error for one)."""
    import torch
    from spectavi_amd import device as spv
    seg = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64)
    table = torch.from_numpy(np.concatenate(tables)).cuda()
    geom, desc = spv.split_sift_table(table)
    nv = len(tables)
    pairs = np.array([(q, d) for d in range(nv) for q in range(d + 1, nv)], np.int32).reshape(-1, 2)
    if matcher == 'cascade':
        from spectavi_amd import feature
        m = feature.auto_hash_bit_rate(*[max(len(t) for t in tables)] * 2)
        if m < 4:
            raise ValueError("tables too small for the cascade hash (the front-end falls back to brute force)")
        rows = spv.normalize_batch(desc, seg)
        hd = torch.from_numpy(feature.generate_hash_dict(hash_seed, rows.shape[1], m, 2)).to(table.device)
        idx, dist, _ = spv.cascade_batch(rows, seg, pairs, hd, g=2)
    else:
        idx, dist, _ = spv.l1k2_batch(desc, seg, pairs)
    matches, count = spv.ratio_test(idx, dist, min_ratio)
    p0, p1, pair_off = spv.match_coordinates_batch(geom, seg, pairs, matches, count)
    n = int(pair_off[-1])
    iKt = torch.from_numpy(np.linalg.inv(K).T.copy()).to(table.device)
    x0 = (p0[:n] @ iKt).contiguous()
    x1 = (p1[:n] @ iKt).contiguous()
    fits, mask = spv.ransac_fit_batch(x0, x1, pair_off, required_percent_inliers=required_percent_inliers,
                                      reprojection_error_allowed=3.35e-4, maximum_tries=maximum_tries,
                                      find_best_even_in_failure=False, singular_value_ratio_allowed=1e-3,
                                      seeds=np.arange(seed, seed + len(pairs), dtype=np.uint64), want_mask=True)
    use = [f['best_try'] >= 0 for f in fits]            # a pair without a model owns no points
    cameras = [f['camera'] for f in fits]               # None where there is none
    X, rows, out_off = spv.dlt_triangulate_batch(x0, x1, pair_off, cameras, use=use, mask=mask, want_rows=True)
    out = {'pairs': pairs, 'pair_off': pair_off, 'fits': fits, 'out_off': out_off, 'X': X, 'rows': rows}
    if tracks:
        # the mask has one entry per match: rows [0, n) of matches are the call's capacity
        out['tracks'] = spv.tracks_batch(seg, pairs, matches[:n], count, mask=mask)
        out['track_inputs'] = {'seg_off': seg, 'matches': matches[:n], 'count': count, 'mask': mask, 'geom': geom}
    if guided is not None:
        # x1^T E x0 = 0 with x0 the database view: a query pixel's line in the database view is (K^-T E K^-1)^T x
        iK = np.linalg.inv(K)
        G = np.stack([(iK.T @ np.asarray(f['essential']).reshape(3, 3) @ iK).T if u else np.zeros((3, 3))
                      for f, u in zip(fits, use)])
        lines = spv.epipolar_lines_batch(geom, seg, pairs, G, use=use)
        gidx, gdist, goff = spv.l1k2_guided_batch(desc, geom, seg, pairs, lines, guided)
        gm, gcount = spv.ratio_test(gidx, gdist, min_ratio)
        qrows = gm[:int(gcount)].cpu().numpy()[:, 0]
        out['guided_pair_off'] = np.searchsorted(qrows, goff).astype(np.int64)
        if tracks:
            out['tracks'] = spv.tracks_batch(seg, pairs, gm, gcount, label=out['tracks'][3])
            out['track_inputs'].update(guided_matches=gm, guided_count=gcount)
    if triangulate is not None and tracks:
        track_off, members = out['tracks'][:2]
        out['track_points'] = spv.triangulate_tracks(geom, seg, triangulate, track_off, members)
        out['track_inputs']['geom'] = geom
    return out


def resect_views(out, K, max_error, required_percent_inliers=0.6, maximum_tries=500, seed=1):
    """Incremental registration from the pipeline's tracks (multiview_pipeline(..., tracks=True)), every step on the
    device: the fitted pair with the most inliers is the seed -- its database view K [I | 0], its query view K camera
    --, the tracks are triangulated from those two views with a residual bound of max_error pixels, all other views
    are resected in one call from the ok points their keypoints belong to, and the tracks are triangulated again over
    every registered view.  Returns a dict: seed (database view, query view), cameras (one pixel camera [3,4] per
    view, None where a view was not registered), views (the resected views), fits (their `resect_fit_batch` dicts),
    view_off, x and Xw (their correspondences), track_off and points (`triangulate_tracks`' (X, err, ok, nused) of
    the last step)."""
    from spectavi_amd import device as spv
    fits, pairs, ti = out['fits'], out['pairs'], out['track_inputs']
    track_off, members, track = out['tracks'][0], out['tracks'][1], out['tracks'][4]
    nv = len(ti['seg_off']) - 1
    best = max(range(len(fits)), key=lambda p: len(fits[p]['inlier_idx']) if fits[p]['best_try'] >= 0 else -1)
    if fits[best]['best_try'] < 0:
        raise ValueError("no pair has a model to seed from")
    q, d = (int(v) for v in pairs[best])
    cameras = [None] * nv
    cameras[d] = K @ np.hstack([np.eye(3), np.zeros((3, 1))])
    cameras[q] = K @ fits[best]['camera']
    X, _, ok, _ = spv.triangulate_tracks(ti['geom'], ti['seg_off'], cameras, track_off, members, max_error=max_error,
                                         want_err=False)
    views = [v for v in range(nv) if v not in (q, d)]
    x, Xw, _, view_off = spv.resect_gather(ti['geom'], track, ti['seg_off'], views, X, ok)
    n = int(view_off[-1])
    res = spv.resect_fit_batch(x[:n], Xw[:n], view_off, required_percent_inliers=required_percent_inliers,
                               max_error=max_error, maximum_tries=maximum_tries,
                               seeds=np.arange(seed, seed + len(views), dtype=np.uint64))
    for v, f in zip(views, res):
        if f['success']:
            cameras[v] = f['camera']
    points = spv.triangulate_tracks(ti['geom'], ti['seg_off'], cameras, track_off, members, max_error=max_error)
    return {'seed': (d, q), 'cameras': cameras, 'views': views, 'fits': res, 'view_off': view_off, 'x': x[:n], 'Xw': Xw[:n],
            'points': points, 'track_off': track_off}


def camera_parts(P, K):
    """A pixel camera lambda K [R | t] -> (R, the camera centre)."""
    M = np.linalg.inv(K) @ P
    lam = np.cbrt(np.linalg.det(M[:, :3]))
    return M[:, :3] / lam, -np.linalg.solve(M[:, :3], M[:, 3])


def report_resection(reg, K, scene_cameras):
    """Registered views, every resected camera's median reprojection residual over its inliers, and its agreement
    with the scene's camera in the gauge of the seed pair (the seed's database view at [I | 0], lengths in units of
    the seed's baseline): the angle between the rotations and the distance between the centres."""
    d, q = reg['seed']
    Rd, Cd = camera_parts(scene_cameras[d], K)
    Cq_scene = Rd @ (camera_parts(scene_cameras[q], K)[1] - Cd)
    scale = np.linalg.norm(camera_parts(reg['cameras'][q], K)[1]) / np.linalg.norm(Cq_scene)
    print("registered %d of %d views; seed pair %d-%d" % (sum(c is not None for c in reg['cameras']), len(reg['cameras']), d, q))
    x, Xw = reg['x'].cpu().numpy(), reg['Xw'].cpu().numpy()
    for i, (v, f) in enumerate(zip(reg['views'], reg['fits'])):
        lo, hi = reg['view_off'][i], reg['view_off'][i + 1]
        if f['camera'] is None:
            print("view %d: %d correspondences, no camera" % (v, hi - lo))
            continue
        idx = f['inlier_idx']
        h = Xw[lo:hi][idx] @ f['camera'].T
        res = np.hypot(h[:, 0] / h[:, 2] - x[lo:hi][idx, 0], h[:, 1] / h[:, 2] - x[lo:hi][idx, 1])
        R, C = camera_parts(f['camera'], K)
        Rs, Cs = camera_parts(scene_cameras[v], K)
        Rs, Cs = Rs @ Rd.T, scale * (Rd @ (Cs - Cd))
        angle = np.degrees(np.arccos(np.clip((np.trace(R @ Rs.T) - 1) / 2, -1, 1)))
        print("view %d: %d correspondences, %d inliers (%s, try %d of %d run), median residual %.2e px, rotation off by "
              "%.3f deg, centre off by %.2e baselines" % (v, hi - lo, len(idx), "success" if f['success'] else "best effort",
                                                         f['best_try'], f['tries_run'], float(np.median(res)) if len(res) else
                                                         float('nan'), angle, np.linalg.norm(C - Cs)))
    X, err, ok, nused = reg['points']
    ok, err = ok.cpu().numpy() != 0, err.cpu().numpy()
    of_ok = np.repeat(ok, np.diff(reg['track_off']))
    print("track points over the registered views: ok %d of %d, median residual of the ok tracks %.2e px" % (
        int(ok.sum()), len(ok), float(np.nanmedian(err[of_ok])) if of_ok.any() else float('nan')))


def bundle_views(out, reg, K, huber):
    """Bundle adjustment of what resect_views registered: every camera goes through pose_from_camera, the two seed
    views are held fixed, the ok track points of the last triangulation and all other cameras are refined together
    (Huber width `huber` pixels).  Returns (cameras: one pixel camera K [R | t] per view or None, X, info) with
    `bundle_adjust`'s X and info (want_err)."""
    from spectavi_amd import device as spv
    from spectavi_amd import mvg
    ti, (track_off, members) = out['track_inputs'], out['tracks'][:2]
    poses = []
    for P in reg['cameras']:
        if P is None:
            poses.append(None)
            continue
        R, t = mvg.pose_from_camera(P, K)
        poses.append(np.hstack([R, t[:, None]]))
    fixed = [v in reg['seed'] for v in range(len(poses))]
    X, _, ok, _ = reg['points']
    P, Xo, info = spv.bundle_adjust(ti['geom'], ti['seg_off'], K, poses, track_off, members, X, use=ok, fixed=fixed, huber=huber,
                                    want_err=True)
    return [None if p is None else K @ P[v] for v, p in enumerate(poses)], Xo, info


def report_cameras(label, cameras, reg, K, scene_cameras, err, of_track):
    """report_resection's figures for a set of cameras: the median residual over the observations `of_track` selects,
    and every non-seed view's rotation and centre offsets against the scene in the gauge of the seed pair."""
    d, q = reg['seed']
    Rd, Cd = camera_parts(scene_cameras[d], K)
    Cq_scene = Rd @ (camera_parts(scene_cameras[q], K)[1] - Cd)
    scale = np.linalg.norm(camera_parts(reg['cameras'][q], K)[1]) / np.linalg.norm(Cq_scene)
    print("%s: median residual %.3e px over %d observations" % (label, float(np.nanmedian(err[of_track])), int(of_track.sum())))
    for v in reg['views']:
        if cameras[v] is None:
            continue
        R, C = camera_parts(cameras[v], K)
        Rs, Cs = camera_parts(scene_cameras[v], K)
        Rs, Cs = Rs @ Rd.T, scale * (Rd @ (Cs - Cd))
        angle = np.degrees(np.arccos(np.clip((np.trace(R @ Rs.T) - 1) / 2, -1, 1)))
        print("%s: view %d rotation off by %.4f deg, centre off by %.3e baselines" % (label, v, angle, np.linalg.norm(C - Cs)))


def rectify_pairs(out, K, images):
    """Step 5 for every pair with a model: images is a list of CUDA tensors [960, 1280], one per view.  The fits'
    cameras are calibrated and map the database view's coordinates, so the pixel cameras are K [I|0] for the
    database view and K P for the query view, and a matcher's pair (query, database) is passed as (database, query).
    Returns device.rectify_batch's (r0, r1, ri0, ri1, box, out_off)."""
    from spectavi_amd import device as spv
    P0 = K @ np.hstack([np.eye(3), np.zeros((3, 1))])
    P1s = [None if f['best_try'] < 0 else K @ f['camera'] for f in out['fits']]
    return spv.rectify_batch(images, None, out['pairs'][:, ::-1], P1s, [P0] * len(P1s))


def report(out):
    fitted = 0
    for p, (q, d) in enumerate(out['pairs'].tolist()):
        f = out['fits'][p]
        fitted += f['best_try'] >= 0
        print("pair %d-%d: matches %d model %s inliers %d points %d" % (
            d, q, out['pair_off'][p + 1] - out['pair_off'][p], "yes" if f['best_try'] >= 0 else "no",
            len(f['inlier_idx']), out['out_off'][p + 1] - out['out_off'][p]))
        if 'guided_pair_off' in out:
            g = out['guided_pair_off']
            print("pair %d-%d: guided pass holds %d matches against %d" % (d, q, g[p + 1] - g[p],
                                                                          out['pair_off'][p + 1] - out['pair_off'][p]))
    print("pairs %d fitted %d inliers %d points %d" % (len(out['pairs']), fitted, sum(len(f['inlier_idx']) for f in out['fits']),
                                                       out['out_off'][-1]))
    if 'tracks' in out:
        track_off, members, flags = out['tracks'][:3]
        nt, length = len(track_off) - 1, np.diff(track_off)
        bad = int(flags.sum())
        print("tracks %d members %d inconsistent %d (%.1f %%)" % (nt, track_off[-1], bad, 100.0 * bad / max(1, nt)))
        hist = np.bincount(length) if nt else np.zeros(0, np.int64)
        print("track length: " + ", ".join("%d x %d" % (c, l) for l, c in enumerate(hist.tolist()) if c))


def report_track_points(out, cameras, max_error):
    """The tracks triangulated again with a residual bound of max_error pixels: solved and ok counts and the median
    residual of the ok tracks' observations."""
    from spectavi_amd import device as spv
    track_off, members = out['tracks'][:2]
    X, err, ok, nused = spv.triangulate_tracks(out['track_inputs']['geom'], out['track_inputs']['seg_off'], cameras,
                                               track_off, members, max_error=max_error)
    ok, nused, err = ok.cpu().numpy() != 0, nused.cpu().numpy(), err.cpu().numpy()
    of_ok = np.repeat(ok, np.diff(track_off))
    med = float(np.nanmedian(err[of_ok])) if of_ok.any() else float('nan')
    print("track points: solved %d of %d, ok %d within %.2f px, median residual of the ok tracks %.2e px" % (
        int((nused >= 2).sum()), len(ok), int(ok.sum()), max_error, med))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--images", type=int, default=6, help="views of the scene")
    ap.add_argument("--points", type=int, default=2000, help="scene points seen in every view")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--matcher", default="l1k2", choices=["l1k2", "cascade"], help="exact brute force, or the cascade hash")
    ap.add_argument("--rectify", action="store_true", help="also rectify every fitted pair (step 5), on noise images")
    ap.add_argument("--guided", type=float, default=None, metavar="PIXELS",
                    help="match again inside a band of this half-width around the fitted epipolar lines")
    ap.add_argument("--tracks", action="store_true", help="link every pair's inlier matches into multi-view tracks")
    ap.add_argument("--triangulate", type=float, default=None, metavar="PIXELS",
                    help="with --tracks: one point per track from the scene's own cameras, ok within this residual")
    ap.add_argument("--resect", type=float, default=None, metavar="PIXELS",
                    help="with --tracks: register every view from the best fitted pair on, inliers within this residual")
    ap.add_argument("--bundle", action="store_true", help="with --resect: bundle adjustment of the registered views")
    a = ap.parse_args()
    import torch
    tables, K, cameras = synthetic_sift_views(a.seed, a.images, a.points, return_cameras=True)
    triangulate = cameras if (a.triangulate is not None and a.tracks) else None
    for rep in range(2):  # the second round is the warm one
        torch.cuda.synchronize()
        s = time.perf_counter()
        out = multiview_pipeline(tables, K, matcher=a.matcher, guided=a.guided, tracks=a.tracks, triangulate=triangulate)
        torch.cuda.synchronize()
        dt = time.perf_counter() - s
    report(out)
    if triangulate is not None:
        report_track_points(out, cameras, a.triangulate)
    if a.resect is not None and a.tracks:
        for rep in range(2):
            torch.cuda.synchronize()
            s = time.perf_counter()
            reg = resect_views(out, K, a.resect)
            torch.cuda.synchronize()
            dt_reg = time.perf_counter() - s
        report_resection(reg, K, cameras)
        print("seed, triangulation, resection of %d views, triangulation: %.1f ms (warm)" % (len(reg['views']), dt_reg * 1e3))
        if a.bundle:
            for rep in range(2):
                torch.cuda.synchronize()
                s = time.perf_counter()
                cams, Xb, info = bundle_views(out, reg, K, a.resect)
                torch.cuda.synchronize()
                dt_ba = time.perf_counter() - s
            active = info['active'].cpu().numpy() != 0
            of_track = np.repeat(active, np.diff(reg['track_off']))
            report_cameras("before the bundle", reg['cameras'], reg, K, cameras, reg['points'][1].cpu().numpy(), of_track)
            report_cameras("after the bundle", cams, reg, K, cameras, info['err'].cpu().numpy(), of_track)
            print("bundle adjustment: %d tracks, %d observations, %d steps (%d accepted, stop: %s), cost %.6e -> %.6e, "
                  "%.1f ms (warm)" % (info['tracks'], info['observations'], info['steps'], info['accepted'], info['stop'],
                                      info['first_cost'], info['last_cost'], dt_ba * 1e3))
    n = int(out['out_off'][-1])
    E = out['X'][:n, :3] / out['X'][:n, 3:]
    print("%d views, %.1f ms (warm); depth of the points: median %.2f" % (a.images, dt * 1e3, float(E[:, 2].median()) if n else 0.0))
    if a.rectify:
        images = [torch.randint(0, 256, (960, 1280), dtype=torch.uint8, device="cuda") for _ in range(a.images)]
        for rep in range(2):
            torch.cuda.synchronize()
            s = time.perf_counter()
            r0, r1, ri0, ri1, box, off = rectify_pairs(out, K, images)
            torch.cuda.synchronize()
            dt = time.perf_counter() - s
        print("rectified %d pairs, %.1f ms (warm); windows hold %d samples, %.2f of the whole frames" % (
            int((off[1:] > off[:-1]).sum()), dt * 1e3, off[-1], off[-1] / max(1, sum(f['best_try'] >= 0 for f in out['fits'])) / (2240 * 1536)))


if __name__ == "__main__":
    main()
