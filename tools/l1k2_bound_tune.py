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

Everything is seeded and runs on the CPU: python tools/l1k2_bound_tune.py [--write HEADER] [--pairs N].

--rank 5 --grid e2m3 makes the table of the FP6 form instead (spectavi_amd/csrc/l1k2_bound_fp6.h): five components per
byte value, each an e2m3 number k/8 stored as its integer k, so that G, p and m are integers in units of 1/64 and
everything above holds as it stands.  Adam runs on a real 256 x 5 table started from the recipe plus a fifth harmonic;
the result is rounded to the grid over random rotations (G is invariant under them, the rounding is not) and scales,
and a coordinate descent over grid steps runs on the exact integer objective until no entry moves."""
import argparse
import re
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


# ---- the FP6 (e2m3) form: |k| in {0..15, 16..30 step 2, 32..60 step 4}, the value is k/8
E2M3 = np.array(list(range(16)) + list(range(16, 32, 2)) + list(range(32, 64, 4)), dtype=np.int64)
GRID = np.concatenate([-E2M3[:0:-1], E2M3])          # 63 signed codes, ascending
P6_RANGE = (8, 200)                                  # the sweep of l1k2_prune.hip's make_bound6
_IU, _JU = np.triu_indices(256)
_ORD = np.argsort(_JU - _IU, kind="stable")
_IU, _JU = _IU[_ORD], _JU[_ORD]
_STARTS = np.concatenate([[0], np.cumsum(256 - np.arange(255))])


def derive6(phi, p_range=P6_RANGE):
    """derive() for any integer table, through the minimum of G on each diagonal |a - b| = d."""
    G = phi @ phi.T
    gmin = np.minimum.reduceat(G[_IU, _JU], _STARTS)
    ps = np.arange(*p_range)
    ms = (ps[:, None] * np.arange(256)[None, :] + gmin[None, :]).min(axis=1)
    means = (ms - G.mean()) / ps
    i = int(np.argmax(means))
    return float(means[i]), int(ps[i]), int(ms[i])


def recipe5():
    a = A.astype(np.float64)
    return np.concatenate([recipe().astype(np.float64), (127 * np.cos(5 * np.pi * a / 255) / 5)[:, None]], axis=1)


def optimise5(steps=8000, seed=0):
    torch.manual_seed(seed)
    torch.set_num_threads(4)
    _, p0, _ = derive(recipe())
    F = torch.tensor(recipe5() / np.sqrt(p0), dtype=torch.float64, requires_grad=True)
    Dt = torch.tensor(D, dtype=torch.float64)
    opt = torch.optim.Adam([F], lr=0.02)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, steps, eta_min=1e-4)
    for it in range(steps):
        beta = 0.05 * (200.0 ** (it / (steps - 1)))
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


def to_grid(v):
    """Nearest signed e2m3 code k of each entry."""
    i = np.clip(np.searchsorted(GRID, v), 1, len(GRID) - 1)
    return np.where(v - GRID[i - 1] <= GRID[i] - v, GRID[i - 1], GRID[i])


def quantise6(Fr, rotations=60, seed=2):
    rng = np.random.default_rng(seed)
    best = None
    for r in range(rotations):
        Q = np.eye(Fr.shape[1]) if r == 0 else np.linalg.qr(rng.standard_normal((Fr.shape[1],) * 2))[0]
        R = Fr @ Q
        top = np.abs(R).max()
        for peak in (44.0, 48.0, 52.0, 56.0, 60.0):
            phi = to_grid(R * (peak / top))
            got = derive6(phi)
            if best is None or got[0] > best[1][0]:
                best = (phi, got)
    return best


def polish6(phi):
    """Coordinate descent over one or two grid steps of single entries until no entry moves."""
    mean, p, m = derive6(phi)
    pos = np.searchsorted(GRID, phi)
    while True:
        moved = 0
        for a in range(256):
            for f in range(phi.shape[1]):
                for step in (1, -1, 2, -2):
                    j = pos[a, f] + step
                    if j < 0 or j >= len(GRID):
                        continue
                    old = phi[a, f]
                    phi[a, f] = GRID[j]
                    got = derive6(phi, (max(P6_RANGE[0], p - 3), min(P6_RANGE[1], p + 4)))
                    if got[0] > mean + 1e-12:
                        (mean, p, m), pos[a, f] = got, j
                        moved += 1
                        break
                    phi[a, f] = old
        print("  polish pass: %d moved, %.4f" % (moved, mean), flush=True)
        if not moved:
            return phi, derive6(phi)


def check6(phi, p, m):
    G = phi @ phi.T
    assert np.isin(np.abs(phi), E2M3).all()
    assert (p * D - (m - G)).min() == 0
    assert 128 * abs(m) < 2 ** 24 and p * 128 * 255 < 2 ** 24 and 128 * int(np.abs(G).max()) < 2 ** 24


def header6(phi, mean, p, m, share_lines):
    lines = ["// l1k2_bound_fp6.h -- the rank-5 FP6 (e2m3) table of the L1 2-NN bound path (l1k2_prune.hip).",
             "// Generated by tools/l1k2_bound_tune.py --rank 5 --grid e2m3; do not edit.  An entry is the integer k of the e2m3",
             "// value k/8.  Only the codes are committed: the slope p and the offset m, in units of 1/64, are derived at load,",
             "// with the exhaustive check that every table has to pass (make_bound6).  As generated:",
             "// mean bound %.2f per dimension, p = %d, m = %d." % (mean, p, m)]
    lines += ["// " + l for l in share_lines]
    lines += ["#pragma once", "#include <cstdint>", "", "namespace spv {", "",
              "constexpr int8_t kL1K2BoundFp6K[256][5] = {"]
    for a in range(0, 256, 4):
        lines.append("    " + " ".join("{%3d,%3d,%3d,%3d,%3d}," % tuple(phi[b]) for b in range(a, a + 4)))
    lines += ["};", "", "}  // namespace spv", ""]
    return "\n".join(lines)


def main6(args):
    Fr, real_obj = optimise5(args.steps if args.steps != 30000 else 8000)
    print("real optimum: %.3f per dimension" % real_obj, flush=True)
    phi, (q_mean, q_p, q_m) = quantise6(Fr)
    print("quantised:    %.3f (p = %d, m = %d)" % (q_mean, q_p, q_m), flush=True)
    phi, (t_mean, t_p, t_m) = polish6(phi)
    check6(phi, t_p, t_m)
    print("fp6 rank 5: mean bound %.3f per dimension (p = %d, m = %d, in 1/64)" % (t_mean, t_p, t_m))
    thresholds = (8600, 8190, 7900)
    tuned = None
    try:
        src = open(args.int8_header).read()
        vals = [int(v) for v in re.findall(r"-?\d+", src.split("= {", 1)[1])]
        tuned = np.array(vals, dtype=np.int64).reshape(256, 4)
    except OSError:
        pass
    share_lines = []
    tabs = [("fp6 rank 5", (phi, t_p, t_m))]
    if tuned is not None:
        i_mean, i_p, i_m = derive(tuned)
        tabs.append(("int8 rank 4", (tuned, i_p, i_m)))
    for name, tab in tabs:
        sh, mu, sigma = shares(*tab, thresholds, args.pairs)
        share_lines.append("%-11s bound sum mean %.0f sigma %.0f; simulated share let through at %s: %s" %
                           (name, mu, sigma, " / ".join(map(str, thresholds)), " / ".join("%.3f %%" % (100 * v) for v in sh)))
        print("  " + share_lines[-1])
    if args.write:
        with open(args.write, "w") as f:
            f.write(header6(phi, t_mean, t_p, t_m, share_lines))
        print("wrote", args.write)
    return 0


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
    ap.add_argument("--rank", type=int, default=4, choices=(4, 5))
    ap.add_argument("--grid", default="int8", choices=("int8", "e2m3"))
    ap.add_argument("--int8-header", default="spectavi_amd/csrc/l1k2_bound_tuned.h",
                    help="the int8 table whose simulated shares are printed beside the FP6 table's")
    args = ap.parse_args()
    if (args.rank == 5) != (args.grid == "e2m3"):
        ap.error("the two forms are --rank 4 --grid int8 (the default) and --rank 5 --grid e2m3")
    if args.rank == 5:
        return main6(args)

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
