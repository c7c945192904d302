"""numpy statement of the stereo_batch contracts (include/spectavi_amd.h): cost and winner, keep mask,
correspondences.  Integer arithmetic throughout, so its values are the contract's values.

`stereo`, `keep` and `matches` work on one window ([R, C] arrays); the `*_batch` forms on the flat arrays of a
collection, as the device ops do.  `literal_stereo` and `literal_keep` are per-sample Python transcriptions of the
contract's sentences, against which the vectorised forms are checked (tests/test_stereo_model.py)."""
import numpy as np

NONE = -2**31
NOCOST = 0xFFFF
_BIG = np.int64(1) << 40


def _box_sums(a, r):
    """Sum of a over the (2r + 1)^2 block around every sample whose block is inside a, int64 [R - 2r, C - 2r]."""
    ii = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
    ii[1:, 1:] = a.astype(np.int64).cumsum(0).cumsum(1)
    b = 2 * r + 1
    return ii[b:, b:] - ii[:-b, b:] - ii[b:, :-b] + ii[:-b, :-b]


def cost_volume(ref, oth, ri_ref, ri_oth, radius, d_lo, d_hi):
    """(ds int64 [n], cost int64 [n, R, C]): the cost of every d of the range that some sample can admit, _BIG
    where d is not admissible for the sample."""
    R, C = ref.shape
    r = int(radius)
    ds = np.arange(max(int(d_lo), -(C - 1)), min(int(d_hi), C - 1) + 1, dtype=np.int64)
    vol = np.full((len(ds), R, C), _BIG, np.int64)
    if R < 2 * r + 1 or C < 2 * r + 1:
        return ds, vol
    a, b = ref.astype(np.int64), oth.astype(np.int64)
    ys = slice(r, R - r)
    for k, d in enumerate(ds.tolist()):
        # reference columns x with r <= x < C - r and r <= x + d < C - r
        x0, x1 = max(r, r - d), min(C - r, C - r - d)
        if x0 >= x1:
            continue
        # |ref[y, x] - oth[y, x + d]| wherever both are inside the window, over the columns the blocks need
        diff = np.abs(a[:, x0 - r:x1 + r] - b[:, x0 - r + d:x1 + r + d])
        s = _box_sums(diff, r)  # [R - 2r, x1 - x0]
        ok = (ri_ref[ys, x0:x1] != -1) & (ri_oth[ys, x0 + d:x1 + d] != -1)
        vol[k, ys, x0:x1] = np.where(ok, s, _BIG)
    return ds, vol


def stereo(ref, oth, ri_ref, ri_oth, radius, d_lo, d_hi):
    """(disp int32, cost uint16, cost2 uint16), each [R, C]."""
    R, C = ref.shape
    ds, vol = cost_volume(ref, oth, ri_ref, ri_oth, radius, d_lo, d_hi)
    disp = np.full((R, C), NONE, np.int32)
    cost = np.full((R, C), NOCOST, np.uint16)
    cost2 = np.full((R, C), NOCOST, np.uint16)
    if len(ds) == 0 or R * C == 0:
        return disp, cost, cost2
    k = vol.argmin(0)  # the first smallest: ds ascend, so the smallest d among equal costs
    best = np.take_along_axis(vol, k[None], 0)[0]
    any_ = best < _BIG
    disp[any_] = ds[k][any_]
    cost[any_] = best[any_]
    far = np.abs(ds[:, None, None] - ds[k][None]) >= 2
    second = np.where(far, vol, _BIG).min(0)
    has2 = any_ & (second < _BIG)
    cost2[has2] = second[has2]
    return disp, cost, cost2


def literal_stereo(ref, oth, ri_ref, ri_oth, radius, d_lo, d_hi):
    """The contract, one sample and one disparity at a time."""
    R, C = ref.shape
    r = int(radius)
    disp = np.full((R, C), NONE, np.int32)
    cost = np.full((R, C), NOCOST, np.uint16)
    cost2 = np.full((R, C), NOCOST, np.uint16)
    a, b = ref.astype(int).tolist(), oth.astype(int).tolist()
    for y in range(R):
        for x in range(C):
            costs = {}
            for d in range(max(d_lo, -C), min(d_hi, C) + 1):
                inside = r <= y < R - r and r <= x < C - r and r <= x + d < C - r
                if not inside or ri_ref[y, x] == -1 or ri_oth[y, x + d] == -1:
                    continue
                costs[d] = sum(abs(a[y + dy][x + dx] - b[y + dy][x + d + dx])
                               for dy in range(-r, r + 1) for dx in range(-r, r + 1))
            if not costs:
                continue
            c, d = min((c, d) for d, c in costs.items())
            disp[y, x], cost[y, x] = d, c
            others = [c2 for d2, c2 in costs.items() if abs(d2 - d) >= 2]
            if others:
                cost2[y, x] = min(others)
    return disp, cost, cost2


def keep(disp0, cost0, cost20, disp1=None, lr_tol=1, uniqueness=10):
    """uint8 [R, C]."""
    R, C = disp0.shape
    k = disp0 != NONE
    k &= cost0.astype(np.uint32) * np.uint32(100) <= cost20.astype(np.uint32) * np.uint32(100 - uniqueness)
    if disp1 is not None:
        d = np.where(k, disp0, 0).astype(np.int64)
        xo = np.arange(C, dtype=np.int64)[None, :] + d
        inside = (xo >= 0) & (xo < C)
        back = np.take_along_axis(disp1.astype(np.int64), np.clip(xo, 0, max(C - 1, 0)), 1) if C else d
        k &= inside & (back != NONE) & (np.abs(d + back) <= lr_tol)
    return k.astype(np.uint8)


def literal_keep(disp0, cost0, cost20, disp1=None, lr_tol=1, uniqueness=10):
    R, C = disp0.shape
    out = np.zeros((R, C), np.uint8)
    for y in range(R):
        for x in range(C):
            d = int(disp0[y, x])
            if d == NONE:
                continue
            if disp1 is not None:
                xo = x + d
                if not 0 <= xo < C or int(disp1[y, xo]) == NONE or abs(d + int(disp1[y, xo])) > lr_tol:
                    continue
            if (int(cost0[y, x]) * 100) % 2**32 <= (int(cost20[y, x]) * (100 - uniqueness)) % 2**32:
                out[y, x] = 1
    return out


def matches(disp0, kept, ri0, ri1, wid0, wid1):
    """(x0 float64 [n, 3], x1 float64 [n, 3], rows int32 [n]) of one window, row-major."""
    R, C = disp0.shape
    y, x = np.nonzero(kept)
    d = disp0[y, x].astype(np.int64)
    s0 = ri0[y, x].astype(np.int64)
    s1 = ri1[y, x + d].astype(np.int64)
    one = np.ones(len(y))
    x0 = np.stack([(s0 % wid0).astype(np.float64), (s0 // wid0).astype(np.float64), one], 1)
    x1 = np.stack([(s1 % wid1).astype(np.float64), (s1 // wid1).astype(np.float64), one], 1)
    return x0.reshape(-1, 3), x1.reshape(-1, 3), (y * C + x).astype(np.int32)


# ---- the flat forms of a collection -----------------------------------------------------------------
def out_offsets(box):
    box = np.asarray(box, np.int64).reshape(-1, 4)
    return np.concatenate([[0], np.cumsum((box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2]))]).astype(np.int64)


def window(flat, p, box, off):
    return flat[off[p]:off[p + 1]].reshape(int(box[p][1] - box[p][0]), int(box[p][3] - box[p][2]))


def stereo_batch(r0, r1, ri0, ri1, box, use, radius, drange, swap=0):
    """Flat (disp, cost, cost2) of every window; a pair that is not used has NONE / 0xFFFF / 0xFFFF."""
    box = np.asarray(box).reshape(-1, 4)
    off = out_offsets(box)
    disp = np.full(off[-1], NONE, np.int32)
    cost = np.full(off[-1], NOCOST, np.uint16)
    cost2 = np.full(off[-1], NOCOST, np.uint16)
    if swap:
        r0, r1, ri0, ri1 = r1, r0, ri1, ri0
    for p in range(len(box)):
        if off[p] == off[p + 1] or (use is not None and not use[p]):
            continue
        w = [window(a, p, box, off) for a in (r0, r1, ri0, ri1)]
        d, c, c2 = stereo(*w, radius, int(drange[p][0]), int(drange[p][1]))
        disp[off[p]:off[p + 1]], cost[off[p]:off[p + 1]], cost2[off[p]:off[p + 1]] = d.ravel(), c.ravel(), c2.ravel()
    return disp, cost, cost2


def keep_batch(box, disp0, cost0, cost20, disp1=None, lr_tol=1, uniqueness=10):
    box = np.asarray(box).reshape(-1, 4)
    off = out_offsets(box)
    out = np.zeros(off[-1], np.uint8)
    for p in range(len(box)):
        if off[p] == off[p + 1]:
            continue
        w = [window(a, p, box, off) for a in (disp0, cost0, cost20)]
        out[off[p]:off[p + 1]] = keep(*w, None if disp1 is None else window(disp1, p, box, off), lr_tol, uniqueness).ravel()
    return out


def matches_batch(box, sizes, pairs, disp0, kept, ri0, ri1):
    """(x0, x1, rows, pair_off int64 [npairs + 1]) of the collection."""
    box = np.asarray(box).reshape(-1, 4)
    off = out_offsets(box)
    x0s, x1s, rows, pair_off = [np.zeros((0, 3))], [np.zeros((0, 3))], [np.zeros(0, np.int32)], [0]
    for p in range(len(box)):
        if off[p] < off[p + 1]:
            w = [window(a, p, box, off) for a in (disp0, kept, ri0, ri1)]
            a, b, r = matches(*w, int(sizes[pairs[p][0]][0]), int(sizes[pairs[p][1]][0]))
            x0s.append(a)
            x1s.append(b)
            rows.append(r)
        pair_off.append(pair_off[-1] + (len(rows[-1]) if off[p] < off[p + 1] else 0))
    return np.concatenate(x0s), np.concatenate(x1s), np.concatenate(rows), np.array(pair_off, np.int64)


# ---- the plane scene's geometry check ------------------------------------------------------------------
def triangulate(P0, P1, x0, x1):
    """Linear two-view triangulation of pixel correspondences [n, 3] -> inhomogeneous points [n, 3] (float64 SVD;
    used for the conditions on the scene, never compared with the library bit for bit)."""
    A = np.stack([x0[:, 0:1] * P0[2] - P0[0], x0[:, 1:2] * P0[2] - P0[1],
                  x1[:, 0:1] * P1[2] - P1[0], x1[:, 1:2] * P1[2] - P1[1]], 1)
    X = np.linalg.svd(A)[2][:, 3]
    return X[:, :3] / X[:, 3:4]


def plane_window(seed=1, wid=96, hgt=64, sf=1.2):
    """The plane scene of spectavi_amd/scenes.py through tests/rectify_oracle.rectify (the library's own
    F), cropped to the box of the valid samples: (r0, r1, ri0, ri1, P0, P1)."""
    from spectavi_amd.scenes import plane_scene
    from spectavi_amd import mvg
    from tests import rectify_oracle as ro
    im0, im1, P0, P1 = plane_scene(wid, hgt, seed)
    full = ro.rectify(mvg.rectification_fundamental(P0, P1), im0, im1, sf)
    return tuple(np.ascontiguousarray(a) for a in ro.crop(*full)) + (P0, P1)


def plane_conditions(disp0, kept, x0, x1, P0, P1):
    """(share of the samples with a disparity that are kept, largest distance of a triangulated kept sample from
    the plane)."""
    from spectavi_amd.scenes import plane_distance
    share = float(kept.sum()) / max(int((disp0 != NONE).sum()), 1)
    dist = plane_distance(triangulate(P0, P1, x0, x1)) if len(x0) else np.zeros(0)
    return share, float(dist.max()) if len(dist) else 0.
