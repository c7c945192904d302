"""A numpy restatement of spv_bundle_adjust_device's contract (include/spectavi_amd.h): the residual model, who takes
part, the first-order Huber weighting and the Levenberg-Marquardt loop, with dense normal equations and
numpy.linalg.solve -- no Schur complement, no conjugate gradients.  It is what the GPU tests compare against;
tests/test_bundle_model.py checks it against scipy.optimize.least_squares and its Jacobian against differences."""
import numpy as np

DIAG_MIN, DIAG_MAX = 1e-6, 1e32
STOPS = ("max_steps", "gradient", "cost", "damping")


def skew(a):
    return np.array([[0., -a[2], a[1]], [a[2], 0., -a[0]], [-a[1], a[0], 0.]])


def rodrigues(w):
    """Exp(w), the rotation about w by |w|."""
    th = np.linalg.norm(w)
    W = skew(w)
    if th < 1e-8:
        return np.eye(3) + (1 - th * th / 6) * W + (0.5 - th * th / 24) * W @ W
    return np.eye(3) + np.sin(th) / th * W + 2 * (np.sin(th / 2) / th) ** 2 * W @ W


class Problem:
    """One call's inputs and who takes part in it.  geom float32 [rows, >=2], seg int [nseg + 1], K [nseg,3,3] or [3,3],
    poses [nseg,3,4] (rows of sets without a camera are not read), mode int [nseg], track_off, members [nm, 2],
    X [nt, 4], use [nt] or None."""

    def __init__(self, geom, seg, K, poses, mode, track_off, members, X, use=None, huber=np.inf):
        self.geom = np.asarray(geom, np.float32)
        self.seg = np.asarray(seg, np.int64)
        self.nseg = len(self.seg) - 1
        K = np.asarray(K, np.float64)
        self.K = np.broadcast_to(K, (self.nseg, 3, 3)) if K.shape == (3, 3) else K
        self.mode = np.asarray(mode, np.int64)
        self.poses0 = np.array(poses, np.float64).reshape(self.nseg, 3, 4)
        self.off = np.asarray(track_off, np.int64)
        self.members = np.asarray(members, np.int64).reshape(-1, 2)
        self.X0 = np.array(X, np.float64).reshape(-1, 4)
        self.huber = float(huber)
        nt = len(self.off) - 1
        s, r = self.members[:, 0], self.members[:, 1]
        ok = (s >= 0) & (s < self.nseg)
        sc = np.where(ok, s, 0)
        ok &= self.mode[sc] != 0
        ok &= (r >= 0) & (r < (self.seg[sc + 1] - self.seg[sc]))
        self.usable = ok
        track_of = np.repeat(np.arange(nt), np.diff(self.off))
        with np.errstate(all="ignore"):
            Xe = self.X0[:, :3] / self.X0[:, 3:4]
        good = np.all(np.isfinite(self.X0), axis=1) & (self.X0[:, 3] != 0) & np.all(np.isfinite(Xe), axis=1)
        if use is not None:
            good &= np.asarray(use).reshape(-1) != 0
        good &= np.bincount(track_of[ok], minlength=nt) >= 2
        # the observations of the candidate tracks, then the test at the starting parameters
        self.obs_member = np.flatnonzero(ok & good[track_of])
        self._index(track_of)
        with np.errstate(all="ignore"):
            r, y2 = self.residuals(self.poses0, np.where(good[:, None], Xe, 0.))
        bad = ~(np.all(np.isfinite(r), axis=1) & (y2 > 0))
        good[np.unique(self.obs_track[bad])] = False
        self.active = good
        self.obs_member = np.flatnonzero(ok & good[track_of])
        self._index(track_of)
        self.Xe0 = np.where(good[:, None], Xe, 0.)
        # unknowns: the free cameras that have an observation, then the participating points
        seen = np.bincount(self.obs_set, minlength=self.nseg) > 0
        self.free = np.flatnonzero((self.mode == 1) & seen)
        self.cam_col = np.full(self.nseg, -1)
        self.cam_col[self.free] = 6 * np.arange(len(self.free))
        self.pts = np.flatnonzero(good)
        self.pt_col = np.full(nt, -1)
        self.pt_col[self.pts] = 6 * len(self.free) + 3 * np.arange(len(self.pts))
        self.nunknowns = 6 * len(self.free) + 3 * len(self.pts)

    def _index(self, track_of):
        m = self.obs_member
        self.obs_track = track_of[m]
        self.obs_set = self.members[m, 0]
        rows = self.seg[self.obs_set] + self.members[m, 1]
        self.uv = self.geom[rows, :2].astype(np.float64)

    def residuals(self, poses, Xe):
        """(r [nobs, 2], y2 [nobs]) of the participating observations."""
        P, K = poses[self.obs_set], self.K[self.obs_set]
        y = np.einsum("nij,nj->ni", P[:, :, :3], Xe[self.obs_track]) + P[:, :, 3]
        a, b = y[:, 0] / y[:, 2], y[:, 1] / y[:, 2]
        u = K[:, 0, 0] * a + K[:, 0, 1] * b + K[:, 0, 2]
        v = K[:, 1, 1] * b + K[:, 1, 2]
        return np.stack([u, v], 1) - self.uv, y[:, 2]

    def rho(self, n):
        h = self.huber
        with np.errstate(invalid="ignore"):
            return np.where(n <= h, 0.5 * n * n, h * (n - 0.5 * h) if np.isfinite(h) else 0.5 * n * n)

    def cost(self, poses, Xe):
        """F = sum rho; +inf when an observation has y2 <= 0 or a residual that is not finite."""
        with np.errstate(all="ignore"):
            r, y2 = self.residuals(poses, Xe)
            if not (np.all(np.isfinite(r)) and np.all(y2 > 0)):
                return np.inf
            return float(np.sum(self.rho(np.hypot(r[:, 0], r[:, 1]))))

    def linearise(self, poses, Xe, sparse=False):
        """(r~ [2 nobs], J~ [2 nobs, nunknowns], F) at the parameters; J~ is dense, or a scipy.sparse matrix of the
        same entries for the shapes whose dense form does not fit."""
        r, _ = self.residuals(poses, Xe)
        n = np.hypot(r[:, 0], r[:, 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            w = np.where(n <= self.huber, 1., self.huber / n)
        sw = np.sqrt(w)
        P, K = poses[self.obs_set], self.K[self.obs_set]
        R = P[:, :, :3]
        RX = np.einsum("nij,nj->ni", R, Xe[self.obs_track])
        y = RX + P[:, :, 3]
        a, b, iz = y[:, 0] / y[:, 2], y[:, 1] / y[:, 2], 1 / y[:, 2]
        Jy = np.zeros((len(r), 2, 3))   # d(u, v) / dy, times sqrt(w)
        Jy[:, 0, 0], Jy[:, 0, 1], Jy[:, 0, 2] = K[:, 0, 0] * iz, K[:, 0, 1] * iz, -(K[:, 0, 0] * a + K[:, 0, 1] * b) * iz
        Jy[:, 1, 1], Jy[:, 1, 2] = K[:, 1, 1] * iz, -K[:, 1, 1] * b * iz
        Jy *= sw[:, None, None]
        # -Jy [R X]x: row j is (R X) x Jy[j]
        Jc = np.concatenate([np.cross(RX[:, None, :], Jy), Jy], axis=2)
        Jp = np.einsum("nij,njk->nik", Jy, R)
        rows = 2 * np.arange(len(r))[:, None, None] + np.arange(2)[None, :, None]
        has = self.cam_col[self.obs_set] >= 0
        cc = self.cam_col[self.obs_set][has][:, None, None] + np.arange(6)[None, None, :]
        pc = self.pt_col[self.obs_track][:, None, None] + np.arange(3)[None, None, :]
        ri = np.concatenate([np.broadcast_to(rows[has], cc.shape[:1] + (2, 6)).reshape(-1), np.broadcast_to(rows, (len(r), 2, 3)).reshape(-1)])
        ci = np.concatenate([np.broadcast_to(cc, cc.shape[:1] + (2, 6)).reshape(-1), np.broadcast_to(pc, (len(r), 2, 3)).reshape(-1)])
        vals = np.concatenate([Jc[has].reshape(-1), Jp.reshape(-1)])
        if sparse:
            import scipy.sparse
            J = scipy.sparse.csr_matrix((vals, (ri, ci)), shape=(2 * len(r), self.nunknowns))
        else:
            J = np.zeros((2 * len(r), self.nunknowns))
            J[ri, ci] = vals
        return (r * sw[:, None]).reshape(-1), J, float(np.sum(self.rho(n)))

    def moved(self, poses, Xe, delta):
        """p (+) delta."""
        poses, Xe = poses.copy(), Xe.copy()
        for k, s in enumerate(self.free):
            d = delta[6 * k:6 * k + 6]
            poses[s][:, :3] = rodrigues(d[:3]) @ poses[s][:, :3]
            poses[s][:, 3] += d[3:]
        Xe[self.pts] += delta[6 * len(self.free):].reshape(-1, 3)
        return poses, Xe

    def step(self, poses, Xe, lam):
        """One solve at lambda: (delta, F', max |g|, F) -- no acceptance test."""
        if self.nunknowns > 2500:   # the same normal equations, held and factored as a sparse matrix
            import scipy.sparse
            import scipy.sparse.linalg
            r, J, F = self.linearise(poses, Xe, sparse=True)
            g, H = J.T @ r, (J.T @ J).tocsc()
            D = np.clip(H.diagonal(), DIAG_MIN, DIAG_MAX)
            delta = scipy.sparse.linalg.spsolve(H + lam * scipy.sparse.diags(D, format="csc"), -g)
        else:
            r, J, F = self.linearise(poses, Xe)
            g, H = J.T @ r, J.T @ J
            D = np.clip(np.diag(H), DIAG_MIN, DIAG_MAX)
            delta = np.linalg.solve(H + lam * np.diag(D), -g)
        return delta, self.cost(*self.moved(poses, Xe, delta)), float(np.max(np.abs(g))) if len(g) else 0., F

    def run(self, max_steps=50, lambda0=1e-4, ftol=1e-10, gtol=1e-10):
        """The whole loop: (poses, X [nt, 4] with the participating rows (X, Y, Z, 1), info)."""
        poses, Xe, lam = self.poses0.copy(), self.Xe0.copy(), lambda0
        trace, stop, accepted = [], 0, 0
        F = first = self.cost(poses, Xe) if len(self.pts) else 0.
        for _ in range(max_steps if len(self.pts) else 0):
            delta, Fn, gmax, F = self.step(poses, Xe, lam)
            if gmax <= gtol:
                stop = 1
                break
            ok = Fn < F
            trace.append((F, Fn, lam, np.nan, float(ok), gmax))
            if ok:
                poses, Xe = self.moved(poses, Xe, delta)
                accepted += 1
                lam = max(lam / 10, 1e-15)
                done = (F - Fn) / F <= ftol
                F = Fn
                if done:
                    stop = 2
                    break
            else:
                lam *= 10
                if lam > 1e15:
                    stop = 3
                    break
        X = self.X0.copy()
        X[self.pts, :3], X[self.pts, 3] = Xe[self.pts], 1.
        info = dict(steps=len(trace), accepted=accepted, stop=STOPS[stop], tracks=len(self.pts), observations=len(self.obs_member),
                    first_cost=first, last_cost=F, trace=np.array(trace).reshape(-1, 6))
        return poses, X, info

    def err(self, poses, X):
        """d_err: |r| of every participating observation at (poses, X), NaN elsewhere."""
        out = np.full(len(self.members), np.nan)
        r, _ = self.residuals(poses, X[:, :3])
        out[self.obs_member] = np.hypot(r[:, 0], r[:, 1])
        return out
