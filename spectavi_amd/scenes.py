"""Synthetic scenes with known geometry, shared by the examples, the bench tools and the tests.  numpy only: nothing
here touches a device.

The plane scene: a textured plane z = 4 + 0.25 x seen by two calibrated cameras, rendered to two uint8 images.  Its
cameras and the plane are known, so a dense reconstruction can be held against the plane."""
import numpy as np

PLANE = np.array([-0.25, 0., 1., -4.])  # z = 4 + 0.25 x as PLANE . (X, Y, Z, 1) = 0


def plane_cameras(wid=96, hgt=64):
    """(P0, P1): K [I | 0] and K [R | t] with K = [[f, 0, wid / 2], [0, f, hgt / 2], [0, 0, 1]], f = 100 wid / 96,
    R a rotation of 0.03 rad about y and t = (-0.3, 0.01, 0)."""
    f = 100. * wid / 96.
    K = np.array([[f, 0., wid / 2.], [0., f, hgt / 2.], [0., 0., 1.]])
    c, s = np.cos(0.03), np.sin(0.03)
    R = np.array([[c, 0., s], [0., 1., 0.], [-s, 0., c]])
    t = np.array([-0.3, 0.01, 0.])
    return K @ np.hstack([np.eye(3), np.zeros((3, 1))]), K @ np.hstack([R, t[:, None]])


def render_plane(P, wid, hgt, grid):
    """The plane's texture as camera P sees it, uint8 [hgt, wid]: the pixel (column, row) is the ray through its
    integer coordinates; the texture is the bilinear interpolation of `grid`, 25 texels per unit, shifted by 8
    units."""
    M, p4 = P[:, :3], P[:, 3]
    C = -np.linalg.solve(M, p4)
    px, py = np.meshgrid(np.arange(wid, dtype=np.float64), np.arange(hgt, dtype=np.float64))
    dirs = np.linalg.solve(M, np.stack([px.ravel(), py.ravel(), np.ones(wid * hgt)]))  # [3, n]
    n = PLANE[:3]
    lam = (-PLANE[3] - n @ C) / (n @ dirs)
    X = C[:, None] + lam[None, :] * dirs
    u = np.clip((X[0] + 8.) * 25., 0., grid.shape[1] - 1.001)
    v = np.clip((X[1] + 8.) * 25., 0., grid.shape[0] - 1.001)
    u0, v0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    fu, fv = u - u0, v - v0
    g = grid.astype(np.float64)
    val = ((1 - fv) * ((1 - fu) * g[v0, u0] + fu * g[v0, u0 + 1]) + fv * ((1 - fu) * g[v0 + 1, u0] + fu * g[v0 + 1, u0 + 1]))
    return np.clip(np.rint(val), 0, 255).astype(np.uint8).reshape(hgt, wid)


def plane_scene(wid=96, hgt=64, seed=1):
    """(im0, im1, P0, P1): the two uint8 images of the textured plane and their cameras."""
    grid = np.random.default_rng(seed).integers(0, 256, (400, 400), dtype=np.uint8)
    P0, P1 = plane_cameras(wid, hgt)
    return render_plane(P0, wid, hgt, grid), render_plane(P1, wid, hgt, grid), P0, P1


def plane_distance(X):
    """Distance of inhomogeneous points [n, 3] from the plane."""
    return np.abs(X @ PLANE[:3] + PLANE[3]) / np.linalg.norm(PLANE[:3])
