"""The judge of triangulate_tracks (spv_tracks_triangulate*): a plain numpy restatement of the contract in
include/spectavi_amd.h that shares no code and no algorithm with the kernel, the criteria a result must meet, and
the synthetic scenes of the tests.

Per track the model forms the 2m x 4 DLT matrix A_t in np.longdouble from the float64-widened float32 observations
and rounds once (as tests/dlt_checks.dlt_matrices does, with the same `formation` bound), takes sigma and v4 from
numpy.linalg.svd, and computes the residuals, the depth-sign rule, ok, nused and the unsolved / NaN conventions.

check_definition holds a kernel result against it with the project's criteria (tests/dlt_checks.py):
  unit norm    | ||X|| - 1 | <= 1e-12
  residual     ||A X|| <= sigma4 (1 + 1e-9) + 1e-13 sigma1 + 2 formation; for tracks of more than 64 members the
               1e-13 sigma1 becomes max(1e-13, 8 c m eps) sigma1 with c the worst excess, in units of m eps sigma1, of
               the model's own float64 route (numpy.linalg.qr, then the SVD of R) on the same tracks
  direction    |<X, v4>| >= 1 - 1e-9 - 2 (slack / gap)^2 where gap = sigma3 - sigma4 > 1e-6 sigma1
  err          within 1e-6 relative + (1e-13 + 4 slack / sigma1) kappa scale / |depth| of the model's
  ok           equal to the model's, but for tracks where a model residual lies within that tolerance of max_error
               or a depth term within it of 0, which must stay under 1 % of the case
"""
import numpy as np

EPS = np.finfo(np.float64).eps
GAP = 1e-6


# ---- scenes ---------------------------------------------------------------------------------------------------------
def intrinsics(f=1000.0, cx=640.0, cy=480.0):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def wide_cameras(rng, n=40, K=None):
    """n pixel cameras K R [I | -C]: rotations of 0.05-0.25 rad about random axes, centres at distance 1."""
    K = intrinsics() if K is None else K
    cams = []
    for _ in range(n):
        R = rodrigues(rng.standard_normal(3), rng.uniform(0.05, 0.25))
        C = rng.standard_normal(3)
        C /= np.linalg.norm(C)
        cams.append(K @ R @ np.hstack([np.eye(3), -C[:, None]]))
    return np.array(cams)


def narrow_cameras(rng, n=12, K=None):
    """n pixel cameras K [I | t] with |t| = 2e-3: the narrow-baseline set a Gram-matrix solver fails."""
    K = intrinsics() if K is None else K
    cams = []
    for _ in range(n):
        t = rng.standard_normal(3)
        t *= 2e-3 / np.linalg.norm(t)
        cams.append(K @ np.hstack([np.eye(3), t[:, None]]))
    return np.array(cams)


def points(rng, n):
    return np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-1.8, 1.8, n), rng.uniform(4, 8, n), np.ones(n)], 1)


def observe(rng, cams, Xw, noise):
    """geom float32 [nseg * npts, 4] (every camera sees every point; row s * npts + j is point j in camera s, x and y
    rounded to float32, sigma and angle filled with values the op must not read as coordinates) and seg_off."""
    nseg, npts = len(cams), len(Xw)
    geom = np.empty((nseg * npts, 4), np.float32)
    for s, P in enumerate(cams):
        h = Xw @ P.T
        uv = h[:, :2] / h[:, 2:3]
        if noise:
            uv = uv + rng.normal(0, noise, uv.shape)
        geom[s * npts:(s + 1) * npts, :2] = uv
    geom[:, 2] = 1e30
    geom[:, 3] = -7.0
    return geom, (np.arange(nseg + 1) * npts).astype(np.int64)


def make_tracks(rng, lengths, nseg, distinct=True):
    """Track t observes point t in lengths[t] sets: distinct ones (lengths up to nseg), or drawn with repetition
    but never fewer than two different sets.  Returns track_off int64, members int32 [nm, 2]."""
    mem = []
    for t, m in enumerate(lengths):
        if distinct:
            sets = rng.choice(nseg, m, replace=False)
        else:
            sets = rng.integers(0, nseg, m)
            if m >= 2 and len(set(sets.tolist())) < 2:
                sets[0] = (sets[1] + 1) % nseg
        mem.extend((int(s), t) for s in sets)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return off, np.array(mem, np.int32).reshape(-1, 2)


def calibrate(K, cams, geom):
    """The calibrated variant: cameras and coordinates premultiplied by K^-1 (coordinates rounded to float32 again)."""
    Ki = np.linalg.inv(K)
    g = geom.copy()
    h = np.concatenate([geom[:, :2].astype(np.float64), np.ones((len(geom), 1))], 1) @ Ki.T
    g[:, :2] = h[:, :2] / h[:, 2:3]
    return np.array([Ki @ P for P in cams]), g


# ---- the model ------------------------------------------------------------------------------------------------------
def canonical_sign(v):
    for i in (3, 0, 1, 2):
        if v[i] != 0:
            return -v if v[i] < 0 else v
    return v


def usable_members(seg_off, nseg, members, use):
    seg = np.asarray(seg_off, np.int64)
    mem = np.asarray(members, np.int64).reshape(-1, 2)
    s, r = mem[:, 0], mem[:, 1]
    ok = (s >= 0) & (s < nseg)
    sc = np.clip(s, 0, max(nseg - 1, 0))
    if nseg == 0:
        return np.zeros(len(mem), bool)
    ok &= (r >= 0) & (r < seg[sc + 1] - seg[sc])
    if use is not None:
        ok &= np.asarray(use)[sc] != 0
    return ok


def track_matrix(P, uv):
    """A [2m, 4] in extended precision rounded once, and the formation bound (dlt_checks.dlt_matrices)."""
    L = np.longdouble
    u, v = uv[:, 0], uv[:, 1]
    P = np.asarray(P, np.float64)
    r0 = (u.astype(L)[:, None] * P[:, 2].astype(L) - P[:, 0].astype(L)).astype(np.float64)
    r1 = (v.astype(L)[:, None] * P[:, 2].astype(L) - P[:, 1].astype(L)).astype(np.float64)
    A = np.empty((2 * len(uv), 4))
    A[0::2], A[1::2] = r0, r1
    mags = np.concatenate([np.abs(u)[:, None] * np.abs(P[:, 2]), np.abs(v)[:, None] * np.abs(P[:, 2])])
    return A, EPS * np.linalg.norm(mags)


def residuals(P, uv, X):
    """Per observation: |proj(P X) - (u, v)|, the depth (P X)[2] and the depth-sign term."""
    with np.errstate(all="ignore"):
        h = np.einsum("mij,j->mi", P, X)
        e = np.hypot(h[:, 0] / h[:, 2] - uv[:, 0], h[:, 1] / h[:, 2] - uv[:, 1])
        sgn = np.where(np.linalg.det(P[:, :, :3]) < 0, -1.0, 1.0)
        dc = sgn / np.sum(P[:, 2, :3] ** 2, axis=1) * h[:, 2] / X[3]
    return e, h[:, 2], dc


def model(geom, seg_off, cams, track_off, members, max_error=np.inf, use=None, qr_route=False):
    """The contract, track by track.  cams [nseg, 3, 4] (rows of sets without a camera are not read; pass `use`)."""
    geom = np.asarray(geom)
    assert geom.dtype == np.float32
    cams = np.asarray(cams, np.float64).reshape(-1, 3, 4)
    off = np.asarray(track_off, np.int64)
    mem = np.asarray(members, np.int64).reshape(-1, 2)
    nseg, nt, nm = len(seg_off) - 1, len(off) - 1, len(mem)
    usable = usable_members(seg_off, nseg, mem, use)
    out = dict(X=np.zeros((nt, 4)), err=np.full(nm, np.nan), ok=np.zeros(nt, np.uint8), nused=np.zeros(nt, np.int32),
               S=np.full((nt, 4), np.nan), formation=np.full(nt, np.nan), depth=np.full(nm, np.nan),
               dc=np.full(nm, np.nan), usable=usable, solved=np.zeros(nt, bool), A=[None] * nt, qr_excess=np.zeros(nt))
    for t in range(nt):
        idx = np.arange(off[t], off[t + 1])[usable[off[t]:off[t + 1]]]
        out["nused"][t] = len(idx)
        if len(idx) < 2:
            continue
        P = cams[mem[idx, 0]]
        uv = geom[np.asarray(seg_off)[mem[idx, 0]] + mem[idx, 1], :2].astype(np.float64)
        A, formation = track_matrix(P, uv)
        _, s, vt = np.linalg.svd(A)
        X = canonical_sign(vt[3])
        e, z, dc = residuals(P, uv, X)
        out["solved"][t] = True
        out["X"][t], out["S"][t], out["formation"][t], out["A"][t] = X, s, formation, A
        out["err"][idx], out["depth"][idx], out["dc"][idx] = e, z, dc
        out["ok"][t] = np.isfinite(X).all() and bool(np.all(dc > 0)) and bool(np.all(e <= max_error))
        if qr_route:
            R = np.linalg.qr(A, mode="r")
            v = np.linalg.svd(R)[2][3]
            excess = np.linalg.norm(A @ v) - s[3] * (1 + 1e-9) - 2 * formation
            out["qr_excess"][t] = max(excess, 0.0) / (len(idx) * EPS * s[0])
    return out


# ---- the criteria ---------------------------------------------------------------------------------------------------
def check_definition(X, err, mo, geom, seg_off, track_off, members, long_c=0.0, what="X"):
    """Asserts the criteria of the module docstring for a result (X [nt, 4], err [nm] or None) against model output
    `mo`.  long_c: the measured constant of the float64 QR route for tracks of more than 64 members.  Returns the
    worst margins."""
    X = np.asarray(X, np.float64)
    off = np.asarray(track_off, np.int64)
    mem = np.asarray(members, np.int64).reshape(-1, 2)
    seg = np.asarray(seg_off, np.int64)
    stats = dict(tracks=0, well_separated=0, worst_residual_excess=-np.inf, worst_direction=0.0, worst_err_rel=0.0,
                 min_gap=np.inf)
    if err is not None:
        err = np.asarray(err, np.float64)
        assert np.array_equal(np.isnan(err), np.isnan(mo["err"])), "%s: err is NaN in other places than the model's" % what
    for t in range(len(off) - 1):
        if not mo["solved"][t]:
            assert np.all(X[t] == 0), "%s: unsolved track %d has X %r" % (what, t, X[t])
            continue
        stats["tracks"] += 1
        A, s, slack = mo["A"][t], mo["S"][t], 2.0 * mo["formation"][t]
        m = int(mo["nused"][t])
        assert np.isfinite(X[t]).all(), "%s: track %d is not finite" % (what, t)
        assert abs(np.linalg.norm(X[t]) - 1) <= 1e-12, "%s: track %d is not of unit norm" % (what, t)
        rel = 1e-13 if m <= 64 else max(1e-13, 8 * long_c * m * EPS)
        resid = np.linalg.norm(A @ X[t])
        excess = (resid - (s[3] * (1 + 1e-9) + rel * s[0] + slack)) / s[0]
        stats["worst_residual_excess"] = max(stats["worst_residual_excess"], excess)
        assert excess <= 0, "%s: track %d (%d members): ||A X|| = %.6e exceeds sigma4 = %.6e by %.3e sigma1" % (
            what, t, m, resid, s[3], excess + rel)
        gap = s[2] - s[3]
        stats["min_gap"] = min(stats["min_gap"], gap / s[0])
        if not gap > GAP * s[0]:
            continue
        stats["well_separated"] += 1
        dot = abs(float(X[t] @ mo["X"][t]))
        stats["worst_direction"] = max(stats["worst_direction"], 1 - dot)
        assert dot >= 1 - 1e-9 - 2 * (slack / gap) ** 2, "%s: track %d: |<X, v4>| = %.12f" % (what, t, dot)
        if err is None:
            continue
        sl = np.arange(off[t], off[t + 1])[mo["usable"][off[t]:off[t + 1]]]
        uv = np.abs(np.asarray(geom)[seg[mem[sl, 0]] + mem[sl, 1], :2].astype(np.float64))
        scale = np.maximum(1.0, uv.max(axis=1))
        z = np.abs(mo["depth"][sl])
        cmp = z > 1e-3
        kappa = s[0] / gap
        tol = 1e-6 * mo["err"][sl] + (1e-13 + 4 * slack / s[0]) * kappa * scale / np.maximum(z, 1e-300)
        diff = np.abs(err[sl] - mo["err"][sl])
        if cmp.any():
            stats["worst_err_rel"] = max(stats["worst_err_rel"], float(np.max(diff[cmp] / tol[cmp])))
            assert np.all(diff[cmp] <= tol[cmp]), "%s: track %d: err differs from the model's by %.3e (tol %.3e)" % (
                what, t, diff[cmp].max(), tol[cmp][np.argmax(diff[cmp])])
    return stats


def verdict_undecided(mo, geom, seg_off, track_off, members, max_error):
    """bool [nt]: tracks whose verdict the tolerances leave open -- a model residual within the err tolerance of
    max_error, or a depth term within it of 0 -- or whose singular values are not well separated."""
    off = np.asarray(track_off, np.int64)
    mem = np.asarray(members, np.int64).reshape(-1, 2)
    seg = np.asarray(seg_off, np.int64)
    und = np.zeros(len(off) - 1, bool)
    for t in np.flatnonzero(mo["solved"]):
        s, slack = mo["S"][t], 2.0 * mo["formation"][t]
        gap = s[2] - s[3]
        if not gap > GAP * s[0]:
            und[t] = True
            continue
        sl = np.arange(off[t], off[t + 1])[mo["usable"][off[t]:off[t + 1]]]
        uv = np.abs(np.asarray(geom)[seg[mem[sl, 0]] + mem[sl, 1], :2].astype(np.float64))
        scale = np.maximum(1.0, uv.max(axis=1))
        z = np.abs(mo["depth"][sl])
        tol = 1e-6 * mo["err"][sl] + (1e-13 + 4 * slack / s[0]) * (s[0] / gap) * scale / np.maximum(z, 1e-300)
        und[t] = bool(np.any(np.abs(mo["err"][sl] - max_error) <= tol) or np.any(np.abs(mo["dc"][sl]) <= tol)
                      or not np.all(np.isfinite(tol)))
    return und


def check_verdict(ok, nused, mo, geom, seg_off, track_off, members, max_error, what="ok"):
    """nused equals the model's everywhere; ok equals it outside the undecided tracks, which are under 1 %."""
    assert np.array_equal(np.asarray(nused), mo["nused"]), "%s: nused differs from the model's" % what
    und = verdict_undecided(mo, geom, seg_off, track_off, members, max_error)
    assert und.sum() <= 0.01 * max(len(und), 1), "%s: %d of %d tracks are undecided" % (what, und.sum(), len(und))
    bad = np.flatnonzero((np.asarray(ok) != mo["ok"]) & ~und)
    assert bad.size == 0, "%s: ok differs from the model's at %d tracks, first %d" % (what, bad.size, bad[0])
    return int(und.sum())
