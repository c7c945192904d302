"""The argument rules of a collection -- many sets back to back in one table, and pairs of them -- stated once for
the Python wrappers of spectavi_amd.device, .feature and .mvg, as csrc/collection.h states them for the C entries.
Needs numpy alone; touches neither the library nor a device.  Every refusal is a ValueError unless the caller names
another class."""
import numpy as np

MAX_SETS = 2 ** 20      # of spv_ransac_fit_batch and spv_dlt_triangulate_batch, which keep state per set


def offsets_unchecked(off, name):
    """off -> int64[n + 1] with at least the one entry that lets n be read; the rules of check_offsets (collection.h)
    are left to the library, as the *_plan entries that take bare offsets do."""
    off = np.ascontiguousarray(off, dtype=np.int64).reshape(-1)
    if off.size < 1:
        raise ValueError("%s must start at 0 and never decrease" % name)
    return off


def offsets(off, name, rows=None, rows_of=None, count=None):
    """off -> int64[n + 1] under check_offsets (collection.h): starts at 0, never decreases, ends below 2^31 -- and at
    `rows`, the rows of the table `rows_of` (None: any); with `count`, n must be count."""
    off = offsets_unchecked(off, name)
    if count is not None and off.size != count + 1:
        raise ValueError("%s must hold %d offsets" % (name, count + 1))
    if off[0] != 0 or np.any(np.diff(off) < 0):
        raise ValueError("%s must start at 0 and never decrease" % name)
    if rows is not None and int(off[-1]) != int(rows):
        raise ValueError("%s ends at %d, %s has %d rows" % (name, int(off[-1]), rows_of, int(rows)))
    if int(off[-1]) >= 2 ** 31:
        raise ValueError("%s must end below 2^31: fewer than 2^31 rows in all" % name)
    return off


def offsets_of(sizes):
    """int64[n + 1]: the offsets of sets of `sizes` rows back to back (no rule applied: see offsets)."""
    return np.concatenate([[0], np.cumsum(sizes, dtype=np.int64)]).astype(np.int64)


def offsets_of_sizes(sizes, per):
    """A list of row counts, one per `per` -> (n, int64[n + 1]) under the 2^31 rule of check_offsets (collection.h)."""
    sizes = np.asarray(sizes)
    if sizes.ndim != 1 or (sizes.size and (sizes.dtype.kind not in "iu" or sizes.min() < 0)):
        raise ValueError("sizes must be non-negative integers, one per %s" % per)
    return len(sizes), offsets(offsets_of(sizes), "the %ss' offsets" % per)


def check_set_count(n):
    """The 2^20 sets cap that spv_ransac_fit_batch and spv_dlt_triangulate_batch state."""
    if n > MAX_SETS:
        raise ValueError("more than 2^20 sets per call")


def all_pairs(n):
    """The default pair list: every i < j as (query j, database i)."""
    return [(j, i) for i in range(n) for j in range(i + 1, n)]


def pair_table(pairs, nseg, noun="sets"):
    """pairs -> int32[npairs, 2] under the pair rule of check_collection (collection.h): integers, every entry in
    [0, nseg); an empty list is [0, 2]."""
    prs = np.asarray(pairs)
    if prs.size == 0:
        prs = np.zeros((0, 2), np.int32)
    if prs.ndim != 2 or prs.shape[1] != 2 or prs.dtype.kind not in "iu":
        raise ValueError("pairs must be integers of shape [npairs, 2]")
    if prs.size and (int(prs.min()) < 0 or int(prs.max()) >= nseg):
        raise ValueError("pairs name %s outside [0, %d)" % (noun, nseg))
    return np.ascontiguousarray(prs, dtype=np.int32)


def out_offsets(seg, prs, below_2_31=False):
    """int64[npairs + 1]: pair p owns the out rows [out_off[p], out_off[p + 1]), one per row of its query set
    (pair_out_off of collection.h); below_2_31 is the rule check_collection_out32 adds."""
    out_off = offsets_of(np.diff(seg)[prs[:, 0]])
    if below_2_31 and int(out_off[-1]) >= 2 ** 31:
        raise ValueError("the pairs must own fewer than 2^31 out rows in all")
    return out_off


def per_pair(out_off, *arrays):
    """One tuple of views per pair: rows out_off[p]:out_off[p + 1] of every array."""
    return [tuple(a[lo:hi] for a in arrays) for lo, hi in zip(out_off[:-1], out_off[1:])]


def check_matcher_dim(dim):
    """The row width rule of spv_l1k2_batch_device and spv_cascade_batch_device."""
    if dim <= 0 or dim % 16 != 0:
        raise ValueError("Input matrix inner dimensions must be 16-byte aligned.")
    if dim > 256:
        raise ValueError("the many-pairs form takes dim <= 256 (dim=%d)" % dim)


def use_flags(use, n, per="set"):
    """use -> int32[n] of 0 / 1 (anything non-zero is 1), or None: the `use` array of the C entries."""
    if use is None:
        return None
    use = np.ascontiguousarray(np.asarray(use) != 0, dtype=np.int32).reshape(-1)
    if use.size != n:
        raise ValueError("use must hold one value per %s" % per)
    return use


def packed_cameras(Ps, n, name, per="set"):
    """Ps ([n, 3, 4], [n, 12] or a list of [3, 4]) -> float64[n, 12], as the C entries read cameras."""
    cams = np.ascontiguousarray(Ps, dtype=np.float64).reshape(-1, 12) if n else np.zeros((0, 12))
    if cams.shape[0] != n:
        raise ValueError("%s must hold one [3,4] camera per %s" % (name, per))
    return cams


def none_cameras_skip(Ps, n, name, use, per="set"):
    """A None entry of a camera list skips its set: (Ps with zeros there, `use` -- use_flags' -- with 0 there) for
    packed_cameras and the C entry; both as they came where no entry is None."""
    if not isinstance(Ps, np.ndarray) and any(P is None for P in Ps):
        skip = np.array([P is None for P in Ps])
        if len(skip) != n:
            raise ValueError("%s must hold one [3,4] camera per %s" % (name, per))
        use = (~skip).astype(np.int32) if use is None else (use * ~skip).astype(np.int32)
        Ps = [np.zeros((3, 4)) if P is None else P for P in Ps]
    return Ps, use


def listed_cameras(Ps, n, name, exc, needed=None):
    """A list of n [3, 4] cameras or None -> (float64[n, 12] with zeros at the None entries, int32[n]: 1 where there
    is a camera).  `exc` is raised for an entry that is not [3, 4], and for a None entry where `needed` is not 0."""
    have = np.array([P is not None for P in Ps], dtype=np.int32)
    if needed is not None and any(u and not h for u, h in zip(needed, have)):
        raise exc("%s must be [3,4] camera matrices." % name)
    cams = np.zeros((n, 12))
    for p, P in enumerate(Ps):
        if P is None:
            continue
        P = np.asarray(P, dtype=np.float64)
        if P.shape != (3, 4):
            raise exc("%s must be [3,4] camera matrices." % name)
        cams[p] = P.reshape(12)
    return cams, have


BUNDLE_STOPS = ("max_steps", "gradient", "cost", "damping")   # spv_bundle_adjust_device's stop reasons, by number


def bundle_cameras(K, poses, fixed, nseg, per="set"):
    """The camera tables of spv_bundle_adjust_device: K one [3,3] or one per set -> float64[nseg, 9]; poses a list or
    array of [3,4] = [R | t] whose None entries are sets without a camera -> float64[nseg, 12]; fixed (None, or one
    switch per set) -> mode int32[nseg] of 0 no camera / 1 free / 2 fixed.  ValueError for what the library would
    refuse in K or in a rotation, with its bound of 1e-6."""
    if len(poses) != nseg:
        raise ValueError("poses must hold one [3,4] pose or None per %s" % per)
    P, have = listed_cameras(poses, nseg, "poses", ValueError)
    fixed = np.zeros(nseg, bool) if fixed is None else np.asarray(fixed).reshape(-1) != 0
    if fixed.size != nseg:
        raise ValueError("fixed must hold one value per %s" % per)
    mode = np.where(have == 0, 0, np.where(fixed, 2, 1)).astype(np.int32)
    try:
        K = np.asarray(K, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("K must be one [3,3] matrix, or one per %s" % per)
    if K.shape == (3, 3):
        K = np.broadcast_to(K, (nseg, 3, 3))
    if K.shape != (nseg, 3, 3):
        raise ValueError("K must be one [3,3] matrix, or one per %s" % per)
    K = np.ascontiguousarray(K).reshape(nseg, 9)
    for s in np.flatnonzero(mode):
        k, R = K[s], P[s].reshape(3, 4)[:, :3]
        if not (np.all(np.isfinite(k)) and k[8] == 1 and k[3] == 0 and k[6] == 0 and k[7] == 0 and k[0] != 0 and k[4] != 0):
            raise ValueError("K must be finite and upper triangular with K[2,2] = 1 and non-zero focal lengths")
        if not (np.all(np.isfinite(P[s])) and np.abs(R.T @ R - np.eye(3)).max() <= 1e-6
                and abs(np.linalg.det(R) - 1) <= 1e-6):
            raise ValueError("poses must be [R | t] with R a rotation (to 1e-6)")
    return K, P, mode


def bundle_options(huber, max_steps, lambda0, ftol, gtol, cg_tol, cg_max, mode):
    """The scalar arguments of spv_bundle_adjust_device under its rules; cg_max None -> 6 * free cameras + 10."""
    huber, lambda0, ftol, gtol, cg_tol = (float(v) for v in (huber, lambda0, ftol, gtol, cg_tol))
    if not huber > 0:
        raise ValueError("huber must be positive")
    if not (lambda0 >= 0 and ftol >= 0 and gtol >= 0 and cg_tol >= 0):
        raise ValueError("lambda0, ftol, gtol and cg_tol must be non-negative numbers")
    cg_max = 6 * int(np.sum(mode == 1)) + 10 if cg_max is None else int(cg_max)
    max_steps = int(max_steps)
    if max_steps < 0 or cg_max < 0 or max_steps >= 2 ** 31 or cg_max >= 2 ** 31:
        raise ValueError("max_steps and cg_max must be non-negative")
    return huber, max_steps, lambda0, ftol, gtol, cg_tol, cg_max


def bundle_info(info, trace):
    """spv_bundle_adjust_device's info and trace as the wrappers return them."""
    steps = int(info[0])
    return {'steps': steps, 'accepted': int(info[1]), 'stop': BUNDLE_STOPS[int(info[2])], 'tracks': int(info[3]),
            'observations': int(info[4]), 'first_cost': float(info[5]), 'last_cost': float(info[6]),
            'trace': trace[:steps].copy()}


def seeds_and_tries(seeds, samples, maximum_tries, n):
    """The subsets' arguments of spv_ransac_fit_batch: (seeds uint64[n] -- zeros by default, not looked at when
    samples int32[n, ntries, 7] are given --, maximum_tries in [0, 7e8], which samples set to their ntries)."""
    if samples is not None:
        maximum_tries = samples.shape[1]
    else:
        seeds = np.zeros(n, np.uint64) if seeds is None else np.ascontiguousarray(seeds, dtype=np.uint64).reshape(-1)
        if seeds.size != n:
            raise ValueError("seeds must hold one value per set")
    maximum_tries = int(maximum_tries)
    if maximum_tries < 0 or maximum_tries > 700000000:
        raise ValueError("maximum_tries must be in [0, 7e8]")
    return seeds, maximum_tries


def sample_table(samples, npt, width, min_rows):
    """samples -> int32[n, ntries, width] or None: the subsets of a many-sets fit whose sets have `npt` rows, row
    numbers inside the set; the subsets of a set under min_rows rows -- a skipped set -- are not looked at."""
    if samples is None:
        return None
    n = len(npt)
    samples = np.asarray(samples)
    if samples.dtype.kind not in "iu" and samples.size:
        raise ValueError("samples must be integers")
    if samples.ndim != 3 or samples.shape[0] != n or samples.shape[2] != width:
        raise ValueError("samples must be [npairs, ntries, %d]" % width)
    samples = np.ascontiguousarray(samples, dtype=np.int32)
    runs = npt >= min_rows
    if samples[runs].size and (int(samples[runs].min()) < 0 or
                               np.any(samples[runs].reshape(int(runs.sum()), -1).max(axis=1) >= npt[runs])):
        raise ValueError("a sample row lies outside its set")
    return samples


def resect_dicts(off, ok, P, pct, bt, ran, mask):
    """The per-set outputs of spv_resect_fit_batch as one dict per set; inlier_idx from the mask uint8[total]."""
    out = []
    for p in range(off.size - 1):
        found = bt[p] >= 0
        idx = np.flatnonzero(mask[off[p]:off[p + 1]]).astype(np.int32) if found else np.zeros(0, np.int32)
        out.append({'success': bool(ok[p]), 'camera': P[p].reshape(3, 4).copy() if found else None,
                    'inlier_percent': float(pct[p]), 'inlier_idx': idx, 'best_try': int(bt[p]), 'tries_run': int(ran[p])})
    return out


def fit_dicts(off, ok, F, P, pct, idx, n, bt, br, ran):
    """The per-set outputs of spv_ransac_fit_batch as one `ransac_fit` dict per set."""
    out = []
    for p in range(off.size - 1):
        found = bt[p] >= 0
        out.append({'success': bool(ok[p]), 'essential': F[p].reshape(3, 3).copy() if found else None,
                    'camera': P[p].reshape(3, 4).copy() if found else None, 'inlier_percent': float(pct[p]),
                    'inlier_idx': idx[off[p]:off[p] + n[p]].copy(), 'best_try': int(bt[p]), 'best_root': int(br[p]),
                    'tries_run': int(ran[p])})
    return out
