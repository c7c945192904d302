"""What tests/test_l1k2_guided_plan.py (host only) and tests/test_l1k2_guided_gpu.py share: the numpy oracle of the
guided L1 2-NN, the generator of inputs on which the candidate decision is exact under any evaluation order, the
collections of the cases, and a copy of the multiview example's scene that also returns the cameras and every
keypoint's scene point."""
import numpy as np

from tests import l1k2_batch_cases as bc

NONE_IDX, NONE_DIST = np.uint64(2 ** 64 - 1), np.int32(2 ** 31 - 1)
NINE, FEW, seg_of = bc.NINE, bc.FEW, bc.seg_of

LONE = ([5000, 300], [(1, 0)])            # fewer query blocks than fill the chip: the database set is cut
TILES = ([5000, 300], [(1, 0)] * 1024)    # 2048 query blocks: whole-set items of 79 tiles
LONG = ([70000, 64], [(1, 0)])            # row numbers past 16 bits


# ---- the oracle ---------------------------------------------------------------------------------------------
def candidate_mask(geom_d, lines, max_dist):
    """bool [queries, database rows]: |l0 u + l1 v + l2| <= max_dist in float64, the plain expression."""
    u, v = geom_d[:, 0].astype(np.float64), geom_d[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = lines[:, 0:1] * u[None, :] + lines[:, 1:2] * v[None, :] + lines[:, 2:3]
        return np.abs(s) <= max_dist


def oracle(tables, geoms, pairs, lines, max_dist):
    """(idx uint64 [out_rows, 2], dist int32 [out_rows, 2], ncand int32 [out_rows]) of the collection: per out row
    the candidate mask, SAD in int32 over the candidates only, a stable sort by (dist, row)."""
    rows = sum(len(tables[q]) for q, _ in pairs)
    idx = np.full((rows, 2), NONE_IDX, np.uint64)
    dist = np.full((rows, 2), NONE_DIST, np.int32)
    ncand = np.zeros(rows, np.int32)
    o = 0
    for q, d in pairs:
        yq, xd = tables[q].astype(np.int32), tables[d].astype(np.int32)
        mask = candidate_mask(geoms[d], lines[o:o + len(yq)], max_dist)
        for r in range(len(yq)):
            cand = np.flatnonzero(mask[r])
            ncand[o + r] = len(cand)
            if len(cand):
                sad = np.abs(xd[cand] - yq[r]).sum(axis=1, dtype=np.int32)
                best = np.argsort(sad, kind="stable")[:2]  # cand ascends, so stable by dist is by (dist, row)
                idx[o + r, :len(best)] = cand[best]
                dist[o + r, :len(best)] = sad[best]
        o += len(yq)
    return idx, dist, ncand


def ratio_passes(idx, dist, min_ratio):
    """The rows spv_ratio_test keeps: a nearest neighbour exists and d1 / d0 >= min_ratio in float64."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (idx[:, 0] != NONE_IDX) & (dist[:, 1].astype(np.float64) / dist[:, 0].astype(np.float64) >= min_ratio)


# ---- exact-decision inputs ------------------------------------------------------------------------------------
# u, v multiples of 1/16 in [0, 4096); l0, l1 multiples of 2^-12 in [-1, 1]; l2 a multiple of 2^-16 below 8192 in
# magnitude; max_dist a multiple of 2^-16.  Every product and sum then has at most 31 significant bits and is exact
# in float64 whatever the evaluation order: the oracle's plain expression and an FMA chain agree bit for bit.
def dyadic_geom(rng, n):
    g = np.zeros((n, 4), np.float32)
    g[:, :2] = rng.integers(0, 4096 * 16, (n, 2)) / 16.0
    g[:, 2:] = rng.uniform(1, 8, (n, 2))
    return g


def dyadic_lines(rng, n):
    """n lines, each through a point of the frame that is itself on the 1/16 grid."""
    l01 = rng.integers(-4096, 4097, (n, 2)) / 4096.0
    p = rng.integers(0, 4096 * 16, (n, 2)) / 16.0
    l2 = -(l01[:, 0] * p[:, 0] + l01[:, 1] * p[:, 1])   # multiples of 2^-16, |l2| < 8192: exact
    return np.ascontiguousarray(np.c_[l01, l2])


def is_dyadic(geoms, lines, max_dist):
    fin = lines[np.isfinite(lines).all(axis=1)]
    return (all(np.array_equal(g[:, :2] * 16, np.round(g[:, :2] * 16)) and (g[:, :2] >= 0).all() and (g[:, :2] < 4096).all()
                for g in geoms)
            and np.array_equal(fin[:, :2] * 4096, np.round(fin[:, :2] * 4096)) and (np.abs(fin[:, :2]) <= 1).all()
            and np.array_equal(fin[:, 2] * 65536, np.round(fin[:, 2] * 65536)) and (np.abs(fin[:, 2]) < 8192).all()
            and max_dist * 65536 == round(max_dist * 65536))


def collection(rows, pairs, seed):
    """(tables uint8, geoms float32, lines float64 [out_rows, 3]) of a collection with exact-decision inputs."""
    rng = np.random.default_rng(seed)
    tables = [rng.integers(0, 256, (n, 128), dtype=np.uint8) for n in rows]
    geoms = [dyadic_geom(rng, n) for n in rows]
    lines = dyadic_lines(rng, sum(rows[q] for q, _ in pairs))
    return tables, geoms, lines


RAGGED_SEED, RAGGED_DIST = 7, 32.0   # a band of about 2 % of the frame


def ragged():
    return collection(NINE, FEW, RAGGED_SEED)


def ragged_counts_ok(ncand):
    """The two conditions of the ragged case over the out rows whose database set has 257 rows or more."""
    big, o = [], 0
    for q, d in FEW:
        big += [NINE[d] >= 257] * NINE[q]
        o += NINE[q]
    c = ncand[np.array(big, bool)]
    return all((c == k).any() for k in (0, 1, 2)) and (c >= 3).mean() >= 0.1


# ---- the scene of examples/multiview_from_sift_tables.py, with what a test of the guided pass must know ---------
def synthetic_sift_views(seed=0, n_views=6, n_points=2000, n_extra=None, wrong_fraction=0.08, desc_noise=6.0):
    """examples/multiview_from_sift_tables.py's synthetic_sift_views, draw for draw; returns (tables, K, cameras,
    ids): cameras[v] = (R, t) with x = K (R X + t), ids[v][row] = the scene point of the row, or -1 for an
    unrelated keypoint and for a scene point that sits at an unrelated position in this view."""
    rng = np.random.default_rng(seed)
    n_extra = n_points // 2 if n_extra is None else n_extra
    K = np.array([[1000.0, 0.0, 640.0], [0.0, 1000.0, 480.0], [0.0, 0.0, 1.0]])
    X = np.c_[rng.uniform(-2.5, 2.5, n_points), rng.uniform(-1.8, 1.8, n_points), rng.uniform(4, 8, n_points)]

    def descriptors(n):
        d = np.abs(rng.standard_normal((n, 128))) ** 2
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return np.minimum(np.floor(512.0 * d), 255.0)

    d_scene = descriptors(n_points)
    tables, cameras, ids = [], [], []
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
        Xc = X @ R.T + t
        pix = ((Xc / Xc[:, 2:]) @ K.T)[:, :2]
        pid = np.arange(n_points)
        if v:
            wrong = rng.choice(n_points, int(round(wrong_fraction * n_points)), replace=False)
            pix[wrong] = np.c_[rng.uniform(0, 1280, len(wrong)), rng.uniform(0, 960, len(wrong))]
            pid[wrong] = -1
        desc = np.clip(np.round(d_scene + desc_noise * rng.standard_normal(d_scene.shape)), 0, 255)
        pix = np.vstack([pix, np.c_[rng.uniform(0, 1280, n_extra), rng.uniform(0, 960, n_extra)]])
        desc = np.vstack([desc, descriptors(n_extra)])
        pid = np.r_[pid, np.full(n_extra, -1)]
        n = len(pix)
        table = np.hstack([pix, rng.uniform(1, 8, (n, 1)), rng.uniform(-np.pi, np.pi, (n, 1)), desc]).astype(np.float32)
        perm = rng.permutation(n)
        tables.append(table[perm])
        cameras.append((R, t))
        ids.append(pid[perm])
    return tables, K, cameras, ids


def true_line_matrix(K, cam_q, cam_d):
    """G with l = G x_q: the line in the database view's pixels of a pixel x_q of the query view."""
    (Rq, tq), (Rd, td) = cam_q, cam_d
    R = Rq @ Rd.T                      # database camera frame -> query camera frame
    t = tq - R @ td
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R   # x_q^T E x_d = 0 (calibrated)
    iK = np.linalg.inv(K)
    return (iK.T @ E @ iK).T
