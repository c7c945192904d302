"""Measures the non-headline rows of the hot path on one GPU (BASELINE configs[2], [3]) and
prints one JSON line each: cascade 1M x 1M (m=17, n=2, g=2) and 10M-point DLT.
Inputs are resident in HBM; kernel times come from the library's hipEvent brackets."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from spectavi_amd import device as spv  # noqa: E402
from spectavi_amd import feature  # noqa: E402

HBM_PEAK = 8000.0


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    spv.profile_reset()
    spv.profile_enable(True)
    t0 = time.perf_counter()
    for _ in range(steps):
        out = fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    spv.profile_enable(False)
    return out, dt


def cascade(rows, steps, warmup, planted):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0xdeadbeef)
    x = torch.randint(0, 256, (rows, 128), dtype=torch.uint8, device=dev, generator=g).float() - 128
    if planted:
        perm = torch.randperm(rows, device=dev, generator=g)
        noise = torch.randint(-3, 4, (rows, 128), device=dev, generator=g).float()
        y = torch.clamp(x[perm] + noise, -128, 127)
    else:
        y = torch.randint(0, 256, (rows, 128), dtype=torch.uint8, device=dev, generator=g).float() - 128
    m = feature.auto_hash_bit_rate(rows, rows)
    n, gg = 2, 2
    d = torch.from_numpy(feature.generate_hash_dict(0x5eed, 128, m, n)).to(dev)
    (idx, dist, ncand), dt = timed(lambda: spv.cascade(x, y, d, g=gg, want_ncand=True), steps, warmup)
    k = {name: spv.profile_read(name) for name in ("cascade_project", "cascade_buckets", "cascade_probe_refine")}
    cbar = float(ncand.float().mean())
    probe_s = k["cascade_probe_refine"][1] / max(k["cascade_probe_refine"][0], 1) / 1e3
    proj_s = k["cascade_project"][1] / max(k["cascade_project"][0], 1) / 1e3
    probe_bytes = rows * (128 + 128 * cbar + 24 + n * (1 << gg) * 8 + cbar * 4)
    setup_bytes = 2 * rows * (512 + 128 + 4 * n)
    rec = {
        "metric": "cascade-hash L1 2-NN, queries/s (1M x 1M, m=%d n=%d g=%d)" % (m, n, gg),
        "value": rows / dt, "unit": "queries/s", "n_gpus": 1, "steps": steps, "warmup": warmup,
        "ms_per_step": dt * 1e3, "higher_is_better": True, "dtype": "f32 hash + u8 refine", "data": "synthetic",
        "config": {"workload": "cascade %d x %d D=128, %s queries" % (rows, rows, "planted" if planted else "uniform"),
                   "m": m, "n": n, "g": gg},
        "mean_candidates": cbar, "equiv_bruteforce_pairs_per_s": float(rows) * rows / dt,
        "evaluated_pairs_per_s": rows * cbar / dt,
        "found_fraction": float((idx[:, 0] >= 0).float().mean()),
        "kernels_ms": {kk: v[1] / max(v[0], 1) for kk, v in k.items()},
        "roofline": {"bound": "hbm", "kernel": "probe_refine_kernel", "achieved": probe_bytes / probe_s / 1e9,
                     "peak": HBM_PEAK, "unit": "GB/s", "frac": probe_bytes / probe_s / 1e9 / HBM_PEAK,
                     "algorithmic": "%.0f B per query (128 + 128*C + 24 + bucket look-ups + 4*C index reads), C=%.1f" % (
                         probe_bytes / rows, cbar), "traffic": None},
        "roofline_project": {"bound": "hbm", "kernel": "project_kernel", "achieved": setup_bytes / proj_s / 1e9,
                             "peak": HBM_PEAK, "unit": "GB/s", "frac": setup_bytes / proj_s / 1e9 / HBM_PEAK},
    }
    if planted:
        rec["recall_planted_top1"] = float((idx[:, 0] == perm).float().mean())
    # recall against the exact L1 2-NN on a 10k-query subsample; uniform random data
    # has no cluster structure, so a low value there is a property of the input
    sub = torch.arange(0, rows, max(1, rows // 10000), device=dev)[:10000]
    ux = (x + 128).to(torch.uint8).contiguous()
    uy = (y[sub] + 128).to(torch.uint8).contiguous()
    eidx, _ = spv.l1k2(ux, uy)
    rec["recall_vs_exact_top1_10k"] = float((idx[sub, 0] == eidx[:, 0]).float().mean())
    rec["recall_vs_exact_top2_10k"] = float((idx[sub] == eidx).float().mean())
    print(json.dumps(rec), flush=True)


def dlt(npt, steps, warmup):
    dev = torch.device("cuda")
    rng = np.random.default_rng(1)
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    P1 = np.hstack([R, rng.standard_normal((3, 1))])
    g = torch.Generator(device=dev).manual_seed(7)
    Xw = torch.randn((npt, 4), dtype=torch.float64, device=dev, generator=g)
    Xw[:, 2] += 5.0
    Xw[:, 3] = 1.0
    x = Xw @ torch.from_numpy(P0).to(dev).T
    xp = Xw @ torch.from_numpy(P1).to(dev).T
    x[:, :2] += 1e-3 * torch.randn((npt, 2), dtype=torch.float64, device=dev, generator=g) * x[:, 2:3]
    xp[:, :2] += 1e-3 * torch.randn((npt, 2), dtype=torch.float64, device=dev, generator=g) * xp[:, 2:3]
    for name, fn, nbytes in (("dlt_triangulate", spv.dlt_triangulate, 80), ("dlt_reprojection_error", spv.dlt_reprojection_error, 56)):
        # 0.15 ms launches: the first launches after an idle period (the set-up above) run at a lower
        # clock state; tools/exp/dlt_exp.hip measured the same ISA at 0.160 ms after a 20-launch
        # (3 ms) warm-up and at 0.145 ms after 0.3 s of launches, so warm up for 2000 launches
        steps, warmup = max(steps, 200), max(warmup, 2000)
        _, dt = timed(lambda: fn(P0, P1, x, xp), steps, warmup)
        n, ms = spv.profile_read("dlt")
        ks = ms / max(n, 1) / 1e3
        print(json.dumps({
            "metric": "%s, points/s (10M point pairs)" % name, "value": npt / dt, "unit": "points/s", "n_gpus": 1,
            "steps": steps, "warmup": warmup, "ms_per_step": dt * 1e3, "higher_is_better": True, "dtype": "f64",
            "data": "synthetic", "config": {"workload": "%s %d points, noisy observations" % (name, npt)},
            "roofline": {"bound": "hbm", "kernel": "dlt_kernel", "achieved": nbytes * npt / ks / 1e9, "peak": HBM_PEAK,
                         "unit": "GB/s", "frac": nbytes * npt / ks / 1e9 / HBM_PEAK, "avg_launch_ms": ks * 1e3,
                         "algorithmic": "%d B per point" % nbytes, "traffic": None},
        }), flush=True)


def end_to_end():
    """Host-pointer C-ABI path (pageable numpy in / numpy out): includes hipMalloc, H2D, D2H."""
    n = 262144
    rng = np.random.default_rng(0xdeadbeef)
    x = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    y = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    feature.nn_bruteforcel1k2(x[:1024], y[:1024])
    t0 = time.perf_counter()
    feature.nn_bruteforcel1k2(x, y)
    dt = time.perf_counter() - t0
    print(json.dumps({"metric": "nn_bruteforcel1k2 through the host-pointer C-ABI (PCIe-inclusive), pairs/s",
                      "value": float(n) * n / dt, "unit": "pairs/s", "ms_per_step": dt * 1e3,
                      "config": {"workload": "256k x 256k D=128, numpy in / numpy out"}, "dtype": "u8",
                      "data": "synthetic"}), flush=True)

    # BASELINE configs[2] and [3] through the same boundary: 1 GB of float32 in for the cascade,
    # 480 MB in / 320 MB out for the triangulation
    from spectavi_amd import mvg
    rows = 1_000_000
    xf = rng.integers(0, 256, (rows, 128), dtype=np.uint8).astype(np.float32) - 128
    yf = rng.integers(0, 256, (rows, 128), dtype=np.uint8).astype(np.float32) - 128
    m = feature.auto_hash_bit_rate(rows, rows)
    d = feature.generate_hash_dict(0x5eed, 128, m, 2)
    feature.nn_cascading_hash_with_dict(xf[:4096], yf[:4096], d[:, :, :6].copy(), g=2)
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        feature.nn_cascading_hash_with_dict(xf, yf, d, g=2)
        best = min(best, time.perf_counter() - t0)
    print(json.dumps({"metric": "nn_cascading_hash through the host-pointer C-ABI (PCIe-inclusive), queries/s",
                      "value": rows / best, "unit": "queries/s", "ms_per_step": best * 1e3,
                      "config": {"workload": "cascade 1M x 1M D=128 m=%d n=2 g=2, numpy float32 in / numpy out" % m,
                                 "host_bytes_in": int(xf.nbytes + yf.nbytes), "host_bytes_out": rows * 24},
                      "dtype": "f32 hash + u8 refine", "data": "synthetic"}), flush=True)
    del xf, yf
    npt = 10_000_000
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    P1 = np.hstack([R, rng.standard_normal((3, 1))])
    Xw = rng.standard_normal((npt, 4))
    Xw[:, 2] += 5.0
    Xw[:, 3] = 1.0
    px = np.ascontiguousarray(Xw @ P0.T)
    pxp = np.ascontiguousarray(Xw @ P1.T)
    mvg.dlt_triangulate(P0, P1, px[:1000], pxp[:1000])
    for name, fn, out_b in (("dlt_triangulate", mvg.dlt_triangulate, 32), ("dlt_reprojection_error", mvg.dlt_reprojection_error, 8)):
        # results are kept alive while timing: handing a 320 MB array back to the OS costs the caller
        # 11-15 ms on this box (reported separately); it is not part of the call
        best, keep = 1e9, []
        for _ in range(6):
            t0 = time.perf_counter()
            keep.append(fn(P0, P1, px, pxp))
            best = min(best, time.perf_counter() - t0)
        t0 = time.perf_counter()
        del keep
        free_ms = (time.perf_counter() - t0) * 1e3 / 6
        print(json.dumps({"metric": "%s through the host-pointer C-ABI (PCIe-inclusive), points/s" % name,
                          "value": npt / best, "unit": "points/s", "ms_per_step": best * 1e3,
                          "caller_free_ms_per_result": free_ms,
                          "config": {"workload": "%s 10M points, numpy float64 in / numpy out" % name,
                                     "host_bytes_in": int(px.nbytes + pxp.nbytes), "host_bytes_out": npt * out_b},
                          "dtype": "f64", "data": "synthetic"}), flush=True)


def l1k2_shapes(steps, warmup):
    """Other descriptor widths and small problems (device-resident, kernel + merge)."""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(11)
    extra = tuple((65536, int(d)) for d in os.environ.get("SPECTAVI_BENCH_DIMS", "").split(",") if d)
    for rows, dim in ((262144, 64), (262144, 144), (262144, 192), (262144, 256), (65536, 272), (65536, 400), (65536, 512),
                      (1000, 128), (10000, 128)) + extra:
        x = torch.randint(0, 256, (rows, dim), dtype=torch.uint8, device=dev, generator=g)
        y = torch.randint(0, 256, (rows, dim), dtype=torch.uint8, device=dev, generator=g)
        _, dt = timed(lambda: spv.l1k2(x, y), steps, warmup)
        n, ms = spv.profile_read("l1k2_tile")
        ks = ms / max(n, 1) / 1e3
        ops = float(rows) * rows * (dim // 4)
        print(json.dumps({"metric": "L1 2-NN, pairs/s", "value": float(rows) * rows / dt, "unit": "pairs/s",
                          "ms_per_step": dt * 1e3, "kernel_ms": ks * 1e3,
                          "sad_lane_ops_per_s": ops / ks, "frac_of_sad_peak": ops / ks / 39.3216e12,
                          "config": {"workload": "%d x %d, D=%d" % (rows, rows, dim)}, "dtype": "u8",
                          "data": "synthetic"}), flush=True)
    # host-pointer latency of small calls (numpy in/out through nn_bruteforcel1k2)
    rng = np.random.default_rng(2)
    for rows in (1000, 10000):
        xh = rng.integers(0, 256, (rows, 128), dtype=np.uint8)
        yh = rng.integers(0, 256, (rows, 128), dtype=np.uint8)
        feature.nn_bruteforcel1k2(xh, yh)
        t0 = time.perf_counter()
        for _ in range(20):
            feature.nn_bruteforcel1k2(xh, yh)
        dt = (time.perf_counter() - t0) / 20
        print(json.dumps({"metric": "nn_bruteforcel1k2 host-pointer call latency", "value": dt * 1e3, "unit": "ms",
                          "ms_per_step": dt * 1e3, "config": {"workload": "%d x %d, D=128, numpy in/out" % (rows, rows)},
                          "dtype": "u8", "data": "synthetic"}), flush=True)


def next_rows(steps, warmup):
    """The SURVEY 8(f) rows: RANSAC scoring, ratio test, normalisation, SIFT adapter."""
    dev = torch.device("cuda")
    rng = np.random.default_rng(5)
    # --- RANSAC scoring: 4096 hypotheses x 2000 correspondences
    nh, npt = 4096, 2000
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    P1s = torch.from_numpy(rng.standard_normal((nh, 3, 4))).to(dev)
    Xw = np.hstack([rng.standard_normal((npt, 2)), rng.uniform(4, 8, (npt, 1)), np.ones((npt, 1))])
    x = torch.from_numpy(Xw @ P0.T).to(dev)
    xp = torch.from_numpy(Xw @ P1s[0].cpu().numpy().T).to(dev)
    _, dt = timed(lambda: spv.dlt_score_hypotheses(P0, P1s, x, xp, 1e-2), steps, warmup)
    n, ms = spv.profile_read("dlt_score")
    print(json.dumps({"metric": "RANSAC hypothesis scoring, point-hypothesis solves/s", "value": nh * npt / dt,
                      "unit": "solves/s", "ms_per_step": dt * 1e3, "kernel_ms": ms / max(n, 1),
                      "config": {"workload": "%d hypotheses x %d correspondences" % (nh, npt)},
                      "dtype": "f64", "data": "synthetic"}), flush=True)
    # --- RANSAC candidate processing on what RANSAC actually produces: essential matrices fitted to
    # noisy minimal samples (the true E perturbed by 1e-3 .. 0.3 relative), 1024 candidates = 4096
    # cameras x 2000 correspondences with 20 % outliers
    th = 0.2
    K = np.array([[0, -0.3, 0.5], [0.3, 0, -0.8], [-0.5, 0.8, 0]]) / np.sqrt(0.98)
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    t = np.array([0.8, 0.5, 0.33]); t /= np.linalg.norm(t)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ R
    x1 = Xw @ np.hstack([R, t[:, None]]).T
    x1[:, :2] += rng.normal(0, 2e-3, (npt, 2)) * x1[:, 2:3]
    x1[::5] = rng.standard_normal((len(x1[::5]), 3))
    nF = 1024
    Fs = np.stack([E * rng.uniform(0.5, 2) + 10 ** rng.uniform(-3, -0.5) * rng.standard_normal((3, 3)) for _ in range(nF)])
    dFs, dx0, dx1 = torch.from_numpy(Fs).to(dev), torch.from_numpy(Xw @ P0.T).to(dev), torch.from_numpy(x1).to(dev)
    out, dt = timed(lambda: spv.ransac_process_candidates(dFs, dx0, dx1, 3e-2, .5, 1e-2, False), steps, warmup)
    n, ms = spv.profile_read("dlt_score")
    ungated = int((out["counts4"][:, 0] >= 0).sum().item())
    print(json.dumps({"metric": "RANSAC candidate processing (gate, E, 4 cameras, scoring, best camera), candidates/s",
                      "value": nF / dt, "unit": "candidates/s", "ms_per_step": dt * 1e3, "score_kernel_ms": ms / max(n, 1),
                      "solves_per_s": 4.0 * ungated * npt / (ms / max(n, 1) * 1e-3),
                      "config": {"workload": "%d candidates (%d pass the gate) x %d correspondences" % (nF, ungated, npt)},
                      "successes": int(out["success"].sum().item()), "dtype": "f64", "data": "synthetic"}), flush=True)
    # --- ratio test + compaction: 4M queries
    nq = 4_000_000
    g = torch.Generator(device=dev).manual_seed(3)
    idx = torch.randint(0, 1 << 20, (nq, 2), dtype=torch.int64, device=dev, generator=g)
    dist = torch.sort(torch.randint(0, 30000, (nq, 2), dtype=torch.int32, device=dev, generator=g), dim=1).values
    (m, c), dt = timed(lambda: spv.ratio_test(idx, dist, 1.75), steps, warmup)
    n, ms = spv.profile_read("ratio_test")
    nbytes = nq * (16 + 8) * 2 + int(c.item()) * 8  # two passes over idx+dist, matches out
    print(json.dumps({"metric": "ratio test + ordered compaction, queries/s", "value": nq / dt, "unit": "queries/s",
                      "ms_per_step": dt * 1e3, "kernel_ms": ms / max(n, 1), "matches": int(c.item()),
                      "roofline": {"bound": "hbm", "achieved": nbytes / (ms / max(n, 1) * 1e-3) / 1e9, "peak": HBM_PEAK,
                                   "unit": "GB/s", "frac": nbytes / (ms / max(n, 1) * 1e-3) / 1e9 / HBM_PEAK,
                                   "algorithmic": "2 x 24 B per query (count pass + scatter pass) + 8 B per match"},
                      "config": {"workload": "%d queries" % nq}, "dtype": "i32/f64", "data": "synthetic"}), flush=True)
    # --- normalisation + SIFT split: 1M x 132
    from spectavi_amd._lib import clib
    import ctypes as ct
    rows = 1_000_000
    table = torch.rand((rows, 132), dtype=torch.float32, device=dev, generator=g) * 200
    table = table.floor().contiguous()
    _, dt = timed(lambda: spv.split_sift_table(table), steps, warmup)
    n, ms = spv.profile_read("sift_split")
    nbytes = rows * (132 * 4 + 16 + 128)
    print(json.dumps({"metric": "SIFT table split, rows/s", "value": rows / dt, "unit": "rows/s", "ms_per_step": dt * 1e3,
                      "kernel_ms": ms / max(n, 1),
                      "roofline": {"bound": "hbm", "achieved": nbytes / (ms / max(n, 1) * 1e-3) / 1e9, "peak": HBM_PEAK,
                                   "unit": "GB/s", "frac": nbytes / (ms / max(n, 1) * 1e-3) / 1e9 / HBM_PEAK,
                                   "algorithmic": "672 B per row"},
                      "config": {"workload": "%d x 132 float32" % rows}, "dtype": "f32->u8", "data": "synthetic"}), flush=True)
    out = torch.empty((rows, 144), dtype=torch.float32, device=dev)
    ws_walk = torch.empty(clib.spv_normalize_workspace_bytes(132), dtype=torch.uint8, device=dev)
    ws_fold = torch.empty(clib.spv_normalize_workspace_bytes_rows(rows, 132), dtype=torch.uint8, device=dev)
    # the same rows as a real SIFT table has them: sub-pixel x, y, scale, angle in (-pi, pi], 128 descriptor values
    sift = table.clone()
    g2 = torch.Generator(device=dev).manual_seed(11)
    sift[:, 0] = torch.rand(rows, device=dev, generator=g2) * 1280
    sift[:, 1] = torch.rand(rows, device=dev, generator=g2) * 960
    sift[:, 2] = torch.rand(rows, device=dev, generator=g2) * 7 + 1
    sift[:, 3] = (torch.rand(rows, device=dev, generator=g2) * 2 - 1) * 3.14159
    for name, tab, ws, note in (
            ("walked (row-ordered float32 chain per column, the small workspace)", table, ws_walk, "5 waves per 16-column block, dependent v_add_f32 at 9.25 cycles"),
            ("folded, integer-valued table", table, ws_fold, "parity -> (increment, parity) function per 1024-row chunk; same bits"),
            ("folded, SIFT-like table (sub-pixel x, y, scale, angle + descriptors)", sift, ws_fold, "the angle column is a random walk around zero: about 40 % of its chunks are walked")):
        def norm():
            clib.spv_normalize_device(tab.data_ptr(), rows, 132, out.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                      ct.c_void_p(torch.cuda.current_stream().cuda_stream))
        _, dt = timed(norm, steps, warmup)
        n, ms = spv.profile_read("normalize")
        print(json.dumps({"metric": "normalize_to_ubyte_and_multiple_16_dim on device, rows/s; " + name, "value": rows / dt,
                          "unit": "rows/s", "ms_per_step": dt * 1e3, "kernel_ms": ms / max(n, 1), "note": note,
                          "config": {"workload": "%d x 132 float32" % rows}, "dtype": "f32", "data": "synthetic"}), flush=True)


# VALU instructions per pair-element of the tile kernel's 32-column body (bf_tile_kernel, gfx950
# disassembly: v_pk_* count one instruction for two rows) and the microbench op (tools/microbench.py)
# whose measured rate prices them; s_nop hazards and the per-row-group work are not counted.
BF_ISSUE = {("f32", 2.0): (1.5, "v_pk_add_f32/v_pk_mul_f32", 8), ("f32", 1.0): (2.0, "v_pk_add_f32 + 2 v_and_b32", 8),
            ("f32", 0.5): (None, "sqrtf sequence", 10), ("i32", 1.0): (None, "scalar", 7)}


def bruteforce_rows(steps, warmup):
    """Exact p-norm k-NN (device.bruteforce), inputs resident: the 131072^2 x 128 rows and the
    reference test's 1000 x 1000 x 132 call."""
    from spectavi_amd._lib import clib
    import ctypes as ct
    rates = {}
    for op in (7, 8, 10):
        r, c = ct.c_double(0), ct.c_double(0)
        clib.spv_microbench_valu(op, 4096, 20000, ct.byref(r), ct.byref(c))
        rates[op] = r.value
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0xbf)
    rows, dim = 131072, 128
    xf = torch.randn((rows, dim), device=dev, generator=g)
    yf = torch.randn((rows, dim), device=dev, generator=g)
    xi = torch.randint(-100, 100, (rows, dim), dtype=torch.int32, device=dev, generator=g)
    yi = torch.randint(-100, 100, (rows, dim), dtype=torch.int32, device=dev, generator=g)
    for dt_name, p, k in (("f32", 2.0, 2), ("f32", 1.0, 2), ("f32", 0.5, 2), ("i32", 1.0, 2), ("f32", 2.0, 16)):
        x, y = (xf, yf) if dt_name == "f32" else (xi, yi)
        _, dt = timed(lambda: spv.bruteforce(x, y, k=k, p=p), steps, warmup)
        n, ms = spv.profile_read("bruteforce")
        nm, msm = spv.profile_read("bruteforce_merge")
        ks = ms / max(n, 1) / 1e3
        pairs = float(rows) * rows
        rec = {"metric": "exact p-norm k-NN, pairs/s (%s p=%g k=%d)" % (dt_name, p, k), "value": pairs / dt,
               "unit": "pairs/s", "ms_per_step": dt * 1e3, "kernel_ms": ks * 1e3, "merge_ms": msm / max(nm, 1),
               "kernel_pairs_per_s": pairs / ks, "config": {"workload": "%d x %d, D=%d" % (rows, rows, dim)},
               "dtype": dt_name, "data": "synthetic"}
        per, what, op = BF_ISSUE.get((dt_name, p), (None, None, None))
        if per is not None and k <= 2:
            bound = rates[op] / (per * dim)  # pairs/s if the body's VALU instructions issued at the measured rate
            rec["issue_bound"] = {"instr_per_pair_element": per, "instructions": what, "rate_op": op,
                                  "measured_lane_instr_per_s": rates[op], "bound_pairs_per_s": bound,
                                  "frac": pairs / ks / bound}
        print(json.dumps(rec), flush=True)
    print(json.dumps({"metric": "microbench rates (lane-instructions/s)", "v_sub_f32": rates[7],
                      "v_pk_add_f32": rates[8], "sqrtf_sequence": rates[10]}), flush=True)
    # the reference test's shape through the host-pointer entry point (numpy in / out), latency
    rng = np.random.default_rng(67)
    xh = rng.standard_normal((1000, 132)).astype(np.float32)
    yh = rng.standard_normal((1000, 132)).astype(np.float32)
    feature.nn_bruteforce(xh, yh, p=2, k=2)
    t0 = time.perf_counter()
    for _ in range(20):
        feature.nn_bruteforce(xh, yh, p=2, k=2)
    dt = (time.perf_counter() - t0) / 20
    print(json.dumps({"metric": "nn_bruteforce host-pointer call latency", "value": dt * 1e3, "unit": "ms",
                      "ms_per_step": dt * 1e3, "config": {"workload": "1000 x 1000, D=132, p=2, k=2, numpy in/out"},
                      "dtype": "f32", "data": "synthetic"}), flush=True)


BF16_MFMA_PEAK = 2.5e15  # dense bf16 MFMA, FLOP/s (MI355X spec)


def ann_rows(steps, warmup):
    """Approximate L2 k-NN (device.ann_l2) against the exact p = 2 route (device.bruteforce) at the
    bruteforce row's shape, 131072^2 x 128, k = 2, inputs resident: the two calls alternate in one
    process, every step timed by device events; kernel times from the library's own brackets."""
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0xbf)
    rows, dim, k = 131072, 128, 2
    x = torch.randn((rows, dim), device=dev, generator=g)
    y = torch.randn((rows, dim), device=dev, generator=g)
    plan = spv.ann_l2_plan(rows, rows, dim, k)
    calls = {"ann_l2": lambda: spv.ann_l2(x, y, k=k), "nn_bruteforce": lambda: spv.bruteforce(x, y, k=k, p=2.0)}
    for _ in range(max(warmup, 1)):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    names = ("ann_prep", "ann_coarse", "ann_merge", "ann_rerank")
    spv.profile_reset()
    times = {n: [] for n in calls}
    for _ in range(max(steps, 3)):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            spv.profile_enable(name == "ann_l2")
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    spv.profile_enable(False)
    kern = {n: spv.profile_read(n)[1] / max(spv.profile_read(n)[0], 1) for n in names}
    ai, _ = calls["ann_l2"]()
    bi, _ = calls["nn_bruteforce"]()
    differ = int((ai != bi).sum().item())
    pairs = float(rows) * rows
    share = 2.0 * plan["kpad"] * pairs / (kern["ann_coarse"] * 1e-3) / BF16_MFMA_PEAK
    ann, bf = times["ann_l2"], times["nn_bruteforce"]
    print(json.dumps({
        "metric": "approximate L2 k-NN vs exact p=2 k-NN, pairs/s (f32 k=%d)" % k, "value": pairs / (np.mean(ann) * 1e-3),
        "unit": "pairs/s", "ann_ms": ann, "bruteforce_ms": bf, "ratio": float(np.mean(bf) / np.mean(ann)),
        "every_ann_step_faster": bool(max(ann) < min(bf)), "kernel_ms": kern, "plan": plan,
        "coarse_share_of_bf16_mfma_peak": share, "coarse_mfma_bound": bool(share > 0.5),
        "positions_differing_from_exact": differ, "positions": int(ai.numel()),
        "config": {"workload": "%d x %d, D=%d" % (rows, rows, dim)}, "dtype": "f32", "data": "synthetic"}), flush=True)


def rectify_rows(steps, warmup):
    """image_pair_rectification with resident images (device.image_pair_rectification): 1920 x 1080,
    sf = 1.2, gray and 3-channel, float64 and uint8.  Bytes moved = the four outputs written once plus
    the valid samples' pixels read; the fraction is of spv_microbench_memory's streaming-copy rate."""
    import ctypes as ct
    from spectavi_amd._lib import clib, check
    from tests.test_rectify_gpu import image, pair
    stream = ct.c_double(0)
    check(clib.spv_microbench_memory(0, 1 << 30, ct.byref(stream)))
    rng = np.random.default_rng(1080)
    hgt, wid, sf = 1080, 1920, 1.2
    P0, P1 = pair(rng, hgt, wid)
    for nchan in (1, 3):
        for dt in (np.float64, np.uint8):
            im0, im1 = (torch.from_numpy(image(rng, hgt, wid, nchan, dt, specials=False)).cuda() for _ in range(2))
            out, dt_call = timed(lambda: spv.image_pair_rectification(P0, P1, im0, im1, sf), steps, warmup)
            n, ms = spv.profile_read("rectify")
            ks = ms / max(n, 1) / 1e3
            rows, cols = out[2].shape
            item = np.dtype(dt).itemsize
            nvalid = int((out[2] >= 0).sum() + (out[3] >= 0).sum())
            moved = 2 * rows * cols * (nchan * item + 4) + nvalid * nchan * item
            print(json.dumps({"metric": "image_pair_rectification kernel, bytes moved / s (%s, nchan=%d)" % (
                np.dtype(dt).name, nchan), "value": moved / ks, "unit": "B/s", "kernel_ms": ks * 1e3,
                "ms_per_call": dt_call * 1e3, "bytes_moved": moved, "output_shape": [rows, cols, nchan],
                "valid_fraction": nvalid / (2.0 * rows * cols), "stream_copy_B_per_s": stream.value,
                "frac_of_stream": moved / ks / stream.value,
                "config": {"workload": "%d x %d, sf=%g, stereo pair, images resident" % (wid, hgt, sf)},
                "dtype": np.dtype(dt).name, "data": "synthetic"}), flush=True)


def sift_rows(steps, warmup):
    """SIFT with the image resident (device.sift_into, table preallocated): 640 x 480, 1920 x 1080 and
    3840 x 2160 smoothed-noise images.  Device time per image split by the library's hipEvent brackets:
    sift_pyramid (upsample / downsample + 12 smoothing passes per octave), sift_detect (extrema,
    scans, refinement, compaction) and sift_describe (gradients, orientation, descriptors).  The
    pyramid's bound is its minimum traffic (each pass reads and writes every pixel of its octave once,
    4 bytes each way) at spv_microbench_memory's streaming-copy rate; the oracle's CPU time is for the
    numpy restatement at 640 x 480."""
    import ctypes as ct
    from spectavi_amd._lib import clib, check
    from tests import sift_oracle as so
    from tests.sift_cases import smooth_random
    stream = ct.c_double(0)
    check(clib.spv_microbench_memory(0, 1 << 30, ct.byref(stream)))
    t0 = time.perf_counter()
    so.sift(smooth_random(11, 480, 640))
    oracle_s = time.perf_counter() - t0
    for wid, hgt in ((640, 480), (1920, 1080), (3840, 2160)):
        im = torch.from_numpy(smooth_random(11, hgt, wid)).cuda()
        table = torch.empty((1 << 20, 132), dtype=torch.float32, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        _, dt_call = timed(lambda: spv.sift_into(im, table, count), steps, warmup)
        parts = {}
        for k in ("sift_pyramid", "sift_detect", "sift_describe"):
            n, ms = spv.profile_read(k)
            parts[k] = ms / steps
        nrow = int(count.item())
        O = so.noctaves(wid, hgt)
        area = sum((2 * wid * 2 * hgt) if o < 0 else (wid >> o) * (hgt >> o) for o in range(-1, -1 + O))
        passes_bytes = 8.0 * (10 * area + 2 * 4 * wid * hgt) + 4 * wid * hgt + 16 * wid * hgt
        bound_ms = passes_bytes / stream.value * 1e3
        print(json.dumps({"metric": "sift_filter device time per image (%d x %d)" % (wid, hgt),
                          "value": sum(parts.values()), "unit": "ms", "pyramid_ms": parts["sift_pyramid"],
                          "detect_ms": parts["sift_detect"], "describe_ms": parts["sift_describe"],
                          "ms_per_call": dt_call * 1e3, "rows": nrow, "octaves": O,
                          "pyramid_min_bytes": passes_bytes, "pyramid_bound_ms": bound_ms,
                          "pyramid_frac_of_bound": bound_ms / parts["sift_pyramid"],
                          "stream_copy_B_per_s": stream.value, "oracle_cpu_s_640x480": oracle_s,
                          "config": {"workload": "%d x %d smoothed noise, image resident" % (wid, hgt)},
                          "dtype": "f32", "data": "synthetic"}), flush=True)


def ransac_fit():
    """The RANSAC loop itself (seven-point solve + candidate processing + best-model rule) through the
    host-pointer entry: all tries evaluated (requirement out of reach) for the rate, then the time to
    the first success on the same scene.  (The CPU side of this line is tests/cpu_baseline.py ransac.)"""
    from spectavi_amd import mvg
    from tests import mvg_checks as mc
    rng = np.random.default_rng(21)
    for npt, tries in ((500, 40000), (2000, 20000), (20000, 4000)):
        x0, x1, E, out_idx = mc.two_view_scene(rng, npt=npt, outlier_fraction=0.4, noise=1e-4)
        kw = dict(reprojection_error_allowed=1e-3, singular_value_ratio_allowed=3e-2)
        mvg.ransac_fit(x0, x1, required_percent_inliers=0.999, maximum_tries=tries, seed=1, **kw)  # warm-up (same workspace size)
        spv.profile_reset()
        spv.profile_enable(True)
        t0 = time.perf_counter()
        r = mvg.ransac_fit(x0, x1, required_percent_inliers=0.999, maximum_tries=tries, seed=2, **kw)
        dt = time.perf_counter() - t0
        spv.profile_enable(False)
        assert r["tries_run"] == tries and not r["success"]
        parts = {k: spv.profile_read(k)[1] for k in ("seven_point", "ransac_cameras", "dlt_score", "ransac_reduce")}
        # time to the first model with more than half of the correspondences as inliers
        t_succ, n_succ = [], []
        for seed in range(3, 11):
            t0 = time.perf_counter()
            rs = mvg.ransac_fit(x0, x1, required_percent_inliers=0.5, maximum_tries=tries, seed=seed, **kw)
            t_succ.append(time.perf_counter() - t0)
            n_succ.append(rs["tries_run"] if rs["success"] else -1)
        print(json.dumps({"metric": "RANSAC fit (7-subset -> seven-point -> 3 candidates x 4 cameras x all correspondences -> best model), tries/s",
                          "value": tries / dt, "unit": "tries/s", "ms_total": dt * 1e3, "kernel_ms": parts,
                          "config": {"workload": "%d correspondences, 40 %% outliers, %d tries, none succeeds" % (npt, tries)},
                          "first_success": {"required_percent_inliers": 0.5, "ms": [round(t * 1e3, 2) for t in t_succ],
                                            "tries_run": n_succ},
                          "cpu_baseline": "tests/cpu_baseline.py ransac (the oracle's serial loop on the same scenes)",
                          "dtype": "f64", "data": "synthetic"}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--npt", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="", help="comma list of: cascade,dlt,next,shapes,e2e,fit,bf,ann,rectify,sift (default all)")
    a = ap.parse_args()
    want = set(filter(None, a.only.split(",")))
    if not want or "cascade" in want:
        cascade(a.rows, a.steps, a.warmup, planted=False)
        cascade(a.rows, a.steps, a.warmup, planted=True)
    if not want or "dlt" in want:
        dlt(a.npt, a.steps, a.warmup)
    if not want or "next" in want:
        next_rows(a.steps, a.warmup)
    if not want or "shapes" in want:
        l1k2_shapes(a.steps, a.warmup)
    if not want or "e2e" in want:
        end_to_end()
    if not want or "fit" in want:
        ransac_fit()
    if not want or "bf" in want:
        bruteforce_rows(a.steps, a.warmup)
    if not want or "ann" in want:
        ann_rows(a.steps, a.warmup)
    if not want or "rectify" in want:
        rectify_rows(a.steps, a.warmup)
    if not want or "sift" in want:
        sift_rows(a.steps, a.warmup)
