"""Generates the tuned rank-4 int8 table of the dim-128 L1 2-NN bound path (spectavi_amd/csrc/l1k2_bound_tuned.h).

The bound.  For an int8 table phi[256][4], G = phi phi^T, an integer slope p and m = min over all byte pairs of
p |a - b| + G(a, b), every pair satisfies |a - b| >= (m - G(a, b)) / p, and the mean of the right-hand side over
all byte pairs, (m - mean G) / p, is what decides how many pairs the kernel has to evaluate exactly (the true
mean of |a - b| is 85.33).  The shipped recipe (harmonics 1 and 3 of the cosine series) reaches 74.40.

The objective.  With F = phi / sqrt(p) real, the mean bound is   min(D + F F^T) - mean(F F^T),   D(a, b) = |a - b|.
It is maximised over a real 256 x 4 F with Adam, the minimum replaced by a soft minimum -1/beta log sum exp(-beta .)
whose beta is annealed upwards, started from the recipe.  The result is scaled into int8 (the scale is swept),
rounded, p swept as l1k2_prune.hip does at load, and polished by a coordinate descent over single int8 entries
(+-1 steps that raise the exact integer objective).  Correctness never depends on any of this: m is the exact
minimum for whatever table comes out, and the library refuses a table that fails its exhaustive check.

Everything is seeded and runs on the CPU: python tools/l1k2_bound_tune.py [--write HEADER] [--pairs N]."""
import argparse
import sys

import numpy as np
import torch

P_RANGE = (64, 400)                      # the sweep of l1k2_prune.hip's make_bound
A = np.arange(256, dtype=np.int64)
D = np.abs(A[:, None] - A[None, :])


def recipe():
    a = A.astype(np.float64)
    return np.stack([np.rint(127 * np.cos(np.pi * a / 255)), np.rint(127 * np.sin(np.pi * a / 255)),
                     np.rint(127 * np.cos(3 * np.pi * a / 255) / 3), np.rint(127 * np.sin(3 * np.pi * a / 255) / 3)],
                    axis=1).astype(np.int64)


def derive(phi, p_range=P_RANGE):
    """(mean bound per dimension, p, m) of an integer table: the slope whose mean bound is largest."""
    G = phi @ phi.T
    best = (-1e300, 0, 0)
    for p in range(*p_range):
        m = int((p * D + G).min())
        mean = (m - G.mean()) / p
        if mean > best[0]:
            best = (mean, p, m)
    return best


def optimise(steps=30000, seed=0):
    torch.manual_seed(seed)
    torch.set_num_threads(4)
    phi0 = recipe()
    _, p0, _ = derive(phi0)
    F = torch.tensor(phi0 / np.sqrt(p0), dtype=torch.float64, requires_grad=True)
    Dt = torch.tensor(D, dtype=torch.float64)
    opt = torch.optim.Adam([F], lr=0.02)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, steps, eta_min=1e-4)
    for it in range(steps):
        beta = 0.05 * (200.0 ** (it / (steps - 1)))            # 0.05 -> 10
        Gr = F @ F.T
        soft_min = -torch.logsumexp(-beta * (Dt + Gr).reshape(-1), 0) / beta
        loss = -(soft_min - Gr.mean())
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
    Fr = F.detach().numpy()
    Gr = Fr @ Fr.T
    return Fr, float((D + Gr).min() - Gr.mean())


def quantise(Fr):
    """The best int8 rounding over a sweep of scales (p comes out near scale^2)."""
    best = None
    top = np.abs(Fr).max()
    for peak in np.arange(90.0, 127.45, 0.25):
        phi = np.rint(Fr * (peak / top)).astype(np.int64)
        got = derive(phi)
        if best is None or got[0] > best[1][0]:
            best = (phi, got)
    return best


def polish(phi, passes=3):
    """Coordinate descent on single entries, the slope free within +-4 of the current one."""
    mean, p, m = derive(phi)
    for _ in range(passes):
        moved = 0
        for a in range(256):
            for f in range(4):
                for step in (1, -1):
                    v = phi[a, f] + step
                    if abs(v) > 127:
                        continue
                    trial = phi.copy()
                    trial[a, f] = v
                    got = derive(trial, (max(P_RANGE[0], p - 4), min(P_RANGE[1], p + 5)))
                    if got[0] > mean + 1e-12:
                        phi, (mean, p, m) = trial, got
                        moved += 1
                        break
        if not moved:
            break
    return phi, derive(phi)


def check(phi, p, m):
    G = phi @ phi.T
    assert np.abs(phi).max() <= 127
    assert (p * D - (m - G)).min() == 0
    assert 128 * int(np.abs(G).max()) < 2 ** 31 and p * 32640 + 128 * abs(m) < 2 ** 31


def shares(phi, p, m, thresholds, pairs, seed=1):
    """Share of uniform random 128-byte pairs that the bound lets through at each threshold, and the mean and
    sigma of the bound sum (128 m - sum G) / p."""
    rng = np.random.default_rng(seed)
    G = (phi @ phi.T).astype(np.int32)
    out = []
    for _ in range(0, pairs, 1 << 18):
        x = rng.integers(0, 256, (1 << 18, 128))
        y = rng.integers(0, 256, (1 << 18, 128))
        out.append(128 * m - G[x, y].sum(axis=1, dtype=np.int64))
    s = np.concatenate(out)
    return [float((s <= p * t).mean()) for t in thresholds], float(s.mean() / p), float(s.std() / p)


def header(phi, mean, p, m):
    lines = ["// l1k2_bound_tuned.h -- the tuned rank-4 int8 table of the L1 2-NN bound path (l1k2_prune.hip).",
             "// Generated by tools/l1k2_bound_tune.py; do not edit.  Only phi is committed: the slope p and the offset m are",
             "// derived at load, with the exhaustive check that every table has to pass (make_bound).  As generated:",
             "// mean bound %.2f per dimension, p = %d, m = %d." % (mean, p, m),
             "#pragma once", "#include <cstdint>", "", "namespace spv {", "",
             "constexpr int8_t kL1K2BoundTunedPhi[256][4] = {"]
    for a in range(0, 256, 4):
        lines.append("    " + " ".join("{%4d,%4d,%4d,%4d}," % tuple(phi[b]) for b in range(a, a + 4)))
    lines += ["};", "", "}  // namespace spv", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", help="header file to write the table to")
    ap.add_argument("--pairs", type=int, default=1 << 21, help="random pairs of the share simulation")
    ap.add_argument("--steps", type=int, default=30000)
    ap.add_argument("--passes", type=int, default=3, help="coordinate-descent passes over the int8 table")
    args = ap.parse_args()

    rec = recipe()
    r_mean, r_p, r_m = derive(rec, (100, 260))
    Fr, real_obj = optimise(args.steps)
    print("real optimum: %.3f per dimension" % real_obj, flush=True)
    phi, (q_mean, q_p, q_m) = quantise(Fr)
    print("quantised:    %.3f (p = %d, m = %d, |phi| <= %d)" % (q_mean, q_p, q_m, np.abs(phi).max()), flush=True)
    phi, (t_mean, t_p, t_m) = polish(phi, args.passes)
    check(rec, r_p, r_m)
    check(phi, t_p, t_m)
    print("mean bound per dimension (true mean %.2f):" % D.mean())
    print("  recipe %.3f (p = %d, m = %d)" % (r_mean, r_p, r_m))
    print("  tuned  %.3f (p = %d, m = %d, |phi| <= %d)" % (t_mean, t_p, t_m, np.abs(phi).max()))
    thresholds = (8600, 8190, 7900)
    for name, tab in (("recipe", (rec, r_p, r_m)), ("tuned", (phi, t_p, t_m))):
        sh, mu, sigma = shares(*tab, thresholds, args.pairs)
        print("  %-6s bound sum mean %.0f sigma %.0f; share let through at %s: %s" %
              (name, mu, sigma, "/".join(map(str, thresholds)), " / ".join("%.3f %%" % (100 * v) for v in sh)))
    if args.write:
        with open(args.write, "w") as f:
            f.write(header(phi, t_mean, t_p, t_m))
        print("wrote", args.write)
    return 0


if __name__ == "__main__":
    sys.exit(main())
