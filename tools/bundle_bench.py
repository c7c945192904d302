#!/usr/bin/env python
"""Times bundle_adjust (spv_bundle_adjust_device) on synthetic collections generated directly, with no matching.

A scene of --views cameras on an arc (tests/bundle_cases.py's) and --tracks points, every point seen by 2 to
--max-len views chosen at random, pixels with 0.5 px of noise rounded to float32; the start is the scene with every
free camera turned by 1 degree and moved by 1 % and every point moved by 1 %, the first two cameras fixed.

Per input, --runs runs of --steps LM steps with cg_max = --cg iterations a step and cg_tol = 0, so that every CG launch
does its work and the kernel timers (spv_profile_read) hold real iterations only.  One JSON line per input:
  linearise_ms    bundle_linearise + bundle_cam_sum + bundle_gradient_max, per linearisation
  cg_iter_ms      bundle_cg_track + bundle_cg_cam + bundle_cg_step, per CG iteration, and hbm_share = the time the bytes
                  of DESIGN.md's account (84 useful bytes per observation, 105 per track) take at 6.3 TB/s, over that figure
  step_ms, call_ms   wall time of the whole call and per LM step (the loop's host waits included)
  kernels_ms      every spv_profile_read name of the op: milliseconds per bracketed launch, the median run's
each as the median and the range of the runs.  --scipy N adds, for scale only, scipy.optimize.least_squares (trf,
sparse Jacobian, the same residuals) on the first N tracks of the same scene on the host, capped at --scipy-nfev
evaluations.

  python tools/bundle_bench.py [--views 8 64] [--tracks 1000000] [--max-len 8] [--steps 5] [--cg 10] [--runs 3] [--scipy 20000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import bundle_cases as bc  # noqa: E402
from tests import bundle_model as bm  # noqa: E402

HBM = 6.3e12                  # achievable bytes per second of one MI355X (a float4 copy)
BYTES_OBS, BYTES_TRACK = 84, 105
CG_NAMES = ("bundle_cg_track", "bundle_cg_cam", "bundle_cg_step")
LIN_NAMES = ("bundle_linearise", "bundle_cam_sum", "bundle_gradient_max")
ALL_NAMES = ("bundle_mark", "bundle_sort", "bundle_linearise", "bundle_cam_sum", "bundle_gradient_max", "bundle_cost_sum",
             "bundle_point_blocks", "bundle_precondition", "bundle_cg_start", "bundle_cg_track", "bundle_cg_cam", "bundle_cg_step",
             "bundle_move", "bundle_cost", "bundle_commit", "bundle_finish")


def collection(nviews, ntracks, max_len, seed):
    """tests/bundle_cases.scene's collection without its per-track loop."""
    rng = np.random.default_rng(seed)
    poses = bc.cameras(nviews, rng)
    X = np.array([0.3 * bc.span(nviews), 0., 6.]) + rng.uniform(-1, 1, (ntracks, 3)) * np.array([1.5, 1., 1.5])
    lengths = rng.integers(2, min(max_len, nviews) + 1, ntracks)
    order = np.argsort(rng.random((ntracks, nviews)), axis=1)
    visible = np.zeros((ntracks, nviews), bool)
    np.put_along_axis(visible, order, np.arange(nviews)[None, :] < lengths[:, None], axis=1)
    row = np.cumsum(visible, axis=0) - 1              # a member's row inside its view: the view's tracks in order
    t, v = np.nonzero(visible)                        # track-major, views ascending inside a track
    members = np.stack([v, row[t, v]], 1).astype(np.int32)
    seg = np.concatenate([[0], np.cumsum(visible.sum(axis=0))]).astype(np.int64)
    geom = np.zeros((seg[-1], 4), np.float32)
    for s in range(nviews):
        seen = np.flatnonzero(visible[:, s])
        geom[seg[s]:seg[s + 1], :2] = bc.project(poses[s], bc.K0, X[seen]) + 0.5 * rng.standard_normal((len(seen), 2))
    return dict(geom=geom, seg=seg, K=bc.K0, poses=poses, X=np.hstack([X, np.ones((ntracks, 1))]), nviews=nviews,
                track_off=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), members=members)


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def bench(a, nviews):
    import torch
    from spectavi_amd import device as spv
    sc = collection(nviews, a.tracks, a.max_len, a.seed)
    poses, X, mode = bc.perturbed(sc, a.seed + 1)
    geom, mem, Xd = torch.from_numpy(sc["geom"]).cuda(), torch.from_numpy(sc["members"]).cuda(), torch.from_numpy(X).cuda()
    kw = dict(fixed=mode == 2, max_steps=a.steps, cg_max=a.cg, cg_tol=0., ftol=0., gtol=0.)
    nobs, runs = len(sc["members"]), []
    spv.bundle_adjust(geom, sc["seg"], sc["K"], list(poses), sc["track_off"], mem, Xd, **kw)   # warm: allocations, code objects
    for _ in range(a.runs):
        spv.profile_enable(True)
        spv.profile_reset()
        torch.cuda.synchronize()
        s = time.perf_counter()
        _, _, info = spv.bundle_adjust(geom, sc["seg"], sc["K"], list(poses), sc["track_off"], mem, Xd, **kw)
        torch.cuda.synchronize()
        call = (time.perf_counter() - s) * 1e3
        prof = {n: spv.profile_read(n) for n in ALL_NAMES}
        spv.profile_enable(False)
        iters = int(info["trace"][:, 3].sum())
        # bundle_cg_track and bundle_cg_cam also run once a step outside the iterations (E q0, the back-substitution)
        cg = sum(prof[n][1] * (iters / max(prof[n][0], 1)) for n in CG_NAMES) / max(iters, 1)
        lin = sum(prof[n][1] / max(prof[n][0], 1) for n in LIN_NAMES)
        runs.append(dict(call_ms=call, step_ms=call / max(info["steps"], 1), cg_iter_ms=cg, linearise_ms=lin, steps=info["steps"],
                         accepted=info["accepted"], cg_iters=iters, first_cost=info["first_cost"], last_cost=info["last_cost"],
                         kernels_ms={n: prof[n][1] / max(prof[n][0], 1) for n in ALL_NAMES}))
    ideal = (BYTES_OBS * nobs + BYTES_TRACK * a.tracks) / HBM * 1e3
    out = dict(what="bundle_adjust", views=nviews, tracks=a.tracks, observations=nobs, steps=a.steps, cg_max=a.cg, runs=a.runs,
               first_cost=runs[0]["first_cost"], last_cost=runs[0]["last_cost"], accepted=runs[0]["accepted"],
               cg_iters=runs[0]["cg_iters"], hbm_ms_per_cg_iter=ideal)
    for k in ("linearise_ms", "cg_iter_ms", "step_ms", "call_ms"):
        out[k] = spread([r[k] for r in runs])
    out["hbm_share"] = ideal / out["cg_iter_ms"]["median"]
    out["kernels_ms"] = sorted(runs, key=lambda r: r["call_ms"])[len(runs) // 2]["kernels_ms"]
    if a.scipy:
        out["scipy"] = scipy_scale(sc, poses, X, mode, a.scipy, a.scipy_nfev)
    return out


def scipy_scale(sc, poses, X, mode, ntracks, nfev):
    import scipy.optimize
    off = sc["track_off"]
    pb = bm.Problem(sc["geom"], sc["seg"], sc["K"], poses, mode, off[:ntracks + 1], sc["members"][:off[ntracks]], X[:ntracks])

    def fun(x):
        return pb.residuals(*pb.moved(pb.poses0, pb.Xe0, x))[0].reshape(-1)
    _, J, F0 = pb.linearise(pb.poses0, pb.Xe0, sparse=True)
    s = time.perf_counter()
    ref = scipy.optimize.least_squares(fun, np.zeros(pb.nunknowns), jac_sparsity=(J != 0), method="trf", x_scale="jac", max_nfev=nfev)
    return dict(tracks=ntracks, observations=len(pb.obs_member), seconds=time.perf_counter() - s, nfev=int(ref.nfev),
                first_cost=F0, last_cost=float(ref.cost), status=int(ref.status))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--views", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--tracks", type=int, default=1000000)
    ap.add_argument("--max-len", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--cg", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--scipy", type=int, default=0, metavar="TRACKS")
    ap.add_argument("--scipy-nfev", type=int, default=10)
    a = ap.parse_args()
    import spectavi_amd
    if spectavi_amd.device_count() < 1:
        sys.exit("bundle_bench.py needs a GPU: it measures and has nothing to fall back to")
    for nviews in a.views:
        print(json.dumps(bench(a, nviews)), flush=True)


if __name__ == "__main__":
    main()
