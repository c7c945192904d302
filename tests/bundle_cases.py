"""Synthetic scenes for the bundle adjustment tests: known cameras on an arc, points in front of all of them,
observations as float32 pixels, tracks built directly (no matcher).  Needs numpy alone."""
import numpy as np

from tests.bundle_model import rodrigues

K0 = np.array([[1000., 0., 640.], [0., 1000., 480.], [0., 0., 1.]])


def cameras(nviews, rng):
    """[nviews, 3, 4] poses [R | t]: view 0 is [I | 0], the others turn about y and slide along x, a little jitter."""
    poses = np.zeros((nviews, 3, 4))
    for v in range(nviews):
        at = v * span(nviews) / max(nviews - 1, 1)   # = v up to five views; more views share the same arc
        R = rodrigues(np.array([0.01 * rng.standard_normal(), -0.08 * at, 0.01 * rng.standard_normal()]) if v else np.zeros(3))
        C = np.array([0.6 * at, 0.05 * rng.standard_normal(), 0.05 * rng.standard_normal()]) if v else np.zeros(3)
        poses[v, :, :3], poses[v, :, 3] = R, -R @ C
    return poses


def span(nviews):
    return min(nviews - 1, 4)


def project(pose, K, X):
    y = X @ pose[:, :3].T + pose[:, 3]
    return (y[:, :2] / y[:, 2:3]) @ K[:2, :2].T + K[:2, 2]


def scene(nviews, npts, seed, min_len=2, max_len=None, noise=0., outliers=0., lengths=None, visible=None):
    """A collection: every point is seen by a random subset of the views, of min_len..max_len of them (`lengths`: the
    subset size of every point instead; `visible` bool [npts, nviews]: the subsets themselves).  Returns a dict: geom
    float32 [rows, 4], seg, K, poses (the scene's), X (the scene's, [npts, 4] with w = 1), track_off, members int32
    [nm, 2] in track order, views ascending inside a track."""
    rng = np.random.default_rng(seed)
    max_len = nviews if max_len is None else max_len
    poses = cameras(nviews, rng)
    centre = np.array([0.3 * span(nviews), 0., 6.])
    X = centre + rng.uniform(-1, 1, (npts, 3)) * np.array([1.5, 1., 1.5])
    if visible is not None:
        lengths = np.asarray(visible).sum(axis=1)
    lengths = rng.integers(min_len, max_len + 1, npts) if lengths is None else np.asarray(lengths)
    per_view = [[] for _ in range(nviews)]
    members = []
    for t in range(npts):
        seen = np.flatnonzero(visible[t]) if visible is not None else sorted(rng.choice(nviews, int(lengths[t]), replace=False))
        for v in seen:
            members.append((v, len(per_view[v])))
            per_view[v].append(t)
    seg = np.concatenate([[0], np.cumsum([len(p) for p in per_view])]).astype(np.int64)
    geom = np.zeros((seg[-1], 4), np.float32)
    for v in range(nviews):
        px = project(poses[v], K0, X[per_view[v]]) if per_view[v] else np.zeros((0, 2))
        px = px + noise * rng.standard_normal(px.shape)
        bad = rng.random(len(px)) < outliers
        ang = rng.uniform(0, 2 * np.pi, len(px))
        px = px + np.where(bad[:, None], 50. * np.stack([np.cos(ang), np.sin(ang)], 1), 0.)
        geom[seg[v]:seg[v + 1], :2] = px
    return dict(geom=geom, seg=seg, K=K0, poses=poses, X=np.hstack([X, np.ones((npts, 1))]),
                track_off=np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64),
                members=np.array(members, np.int32).reshape(-1, 2), nviews=nviews)


def perturbed(sc, seed, fixed=(0, 1), deg=1., rel=0.01):
    """The start of the tests: every camera outside `fixed` turned by `deg` degrees about a random axis and moved by
    `rel` of |t|, every point moved by `rel` of its distance from the origin.  Returns (poses, X, mode)."""
    rng = np.random.default_rng(seed)
    poses, X = sc["poses"].copy(), sc["X"].copy()
    mode = np.ones(len(poses), np.int32)
    for v in range(len(poses)):
        if v in fixed:
            mode[v] = 2
            continue
        ax = rng.standard_normal(3)
        poses[v, :, :3] = rodrigues(np.deg2rad(deg) * ax / np.linalg.norm(ax)) @ poses[v, :, :3]
        d = rng.standard_normal(3)
        poses[v, :, 3] += rel * np.linalg.norm(poses[v, :, 3]) * d / np.linalg.norm(d)
    d = rng.standard_normal((len(X), 3))
    X[:, :3] += rel * np.linalg.norm(X[:, :3], axis=1, keepdims=True) * d / np.linalg.norm(d, axis=1, keepdims=True)
    return poses, X, mode


def run_gpu(sc, poses, X, mode, use=None, **kw):
    """device.bundle_adjust on a scene's collection from the start (poses, X, mode; a mode 0 set has no camera):
    (poses [nseg,3,4], X ndarray, info with active and err as ndarrays)."""
    import torch
    from spectavi_amd import device
    geom = torch.from_numpy(sc["geom"]).cuda()
    mem = torch.from_numpy(np.ascontiguousarray(sc["members"], dtype=np.int32)).cuda()
    start = [None if m == 0 else p for p, m in zip(poses, mode)]
    P, Xo, info = device.bundle_adjust(geom, sc["seg"], sc["K"], start, sc["track_off"], mem,
                                       torch.from_numpy(np.ascontiguousarray(X)).cuda(),
                                       use=None if use is None else torch.from_numpy(np.ascontiguousarray(use, dtype=np.uint8)).cuda(),
                                       fixed=np.asarray(mode) == 2, **kw)
    info = dict(info, active=info["active"].cpu().numpy(), err=info["err"].cpu().numpy() if "err" in info else None)
    return P, Xo.cpu().numpy(), info


def log_rotation(R):
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    s = np.linalg.norm(w)
    return w if s < 1e-12 else w * np.arcsin(s) / s


def recovered_delta(pb, poses0, X0, poses1, X1):
    """The step between two parameter sets in the unknowns of the model `pb`: (omega, tau) of every free camera from
    R1 R0^T and t1 - t0, then the points' moves (X0's rows divided by their w)."""
    d = [np.concatenate([log_rotation(poses1[s][:, :3] @ poses0[s][:, :3].T), poses1[s][:, 3] - poses0[s][:, 3]]) for s in pb.free]
    return np.concatenate(d + [(X1[pb.pts, :3] - X0[pb.pts, :3] / X0[pb.pts, 3:4]).reshape(-1)])


def rotation_angle(Ra, Rb):
    """The angle between two rotations, from the sine and the cosine (arccos alone loses angles below 1e-8)."""
    R = Ra.T @ Rb
    s = np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    return float(np.arctan2(s, (np.trace(R) - 1) / 2))


def centre(pose):
    return -pose[:, :3].T @ pose[:, 3]
