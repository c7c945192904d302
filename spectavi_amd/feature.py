"""
``spectavi_amd.feature``
========================
Descriptor matching front-end, the counterpart of the hot-path functions of the
reference's ``spectavi.feature`` (reference spectavi/feature.py:234-243,
292-304, 346-407): same names, arguments, return types and error behaviour,
bound with ctypes to the gfx950 build of ``libspectavi.so``.
"""
import ctypes as ct

import numpy as np

from spectavi_amd import _collection as col
from spectavi_amd._lib import clib, check
from spectavi_amd.ndarray import NdArray

# ==================================================================================
# brute-force L1, k = 2       (reference spectavi/feature.py:234-243)
# ==================================================================================
_nn_bruteforcel1k2 = clib.nn_bruteforcel1k2


def nn_bruteforcel1k2(x, y, nthreads=1):
    """
    Exact L1 nearest neighbours with k=2 of every row of `y` (queries) among the
    rows of `x` (database); inputs are unsigned bytes with a row length that is
    a multiple of 16 (reference spectavi/feature.py:292-304).

    Returns
    -------
    nn_idx : uint64 ndarray [yrows, 2]   index into `x`, nearest first
    nn_dist : int32 ndarray [yrows, 2]   L1 distances, ascending

    `nthreads` is accepted for signature compatibility; the GPU path ignores it.
    """
    xrows, xdim = x.shape
    yrows, ydim = y.shape
    assert ydim == xdim
    dim = xdim
    if dim % 16 != 0:
        # the reference throws std::runtime_error through extern "C" here
        # (src/BruteForceNnL1K2.h:77-81), which aborts the interpreter
        raise ValueError("Input matrix inner dimensions must be 16-byte aligned.")
    nn_idx = NdArray(dtype='uint64')
    nn_dist = NdArray(dtype='int32')
    _nn_bruteforcel1k2(x, y, xrows, yrows, dim, nthreads, ct.byref(nn_idx), ct.byref(nn_dist))
    check()
    return nn_idx.asarray(), nn_dist.asarray()


def _table_width(tables, dtype, what):
    """dim of a non-empty list of `dtype` arrays [rows_i, dim]; ValueError where they are not that."""
    if not tables:
        raise ValueError("no tables")
    dim = tables[0].shape[1] if tables[0].ndim == 2 else -1
    if any(t.ndim != 2 or t.dtype != dtype or t.shape[1] != dim for t in tables):
        raise ValueError("tables must be %s arrays [rows, dim] of one width" % what)
    return dim


def _tables_and_pairs(tables, pairs):
    """(n, seg_off int64[n + 1], pairs int32[npairs, 2] -- None: col.all_pairs --, out_off int64[npairs + 1]) of a
    list of tables that a many-pairs matcher stores back to back."""
    n = len(tables)
    prs = col.pair_table(col.all_pairs(n) if pairs is None else pairs, n, "tables")
    seg = col.offsets_of([len(t) for t in tables])
    return n, seg, prs, col.out_offsets(seg, prs)


def nn_bruteforcel1k2_batch(tables, pairs=None):
    """
    nn_bruteforcel1k2 for many pairs of descriptor tables in one call (an addition: the reference has no
    such function).  `tables` is a list of uint8 arrays [rows_i, dim], one width for all; `pairs` a list
    of (query table, database table) numbers, by default every i < j as (query j, database i).

    Returns a list with one (nn_idx uint64 [rows, 2], nn_dist int32 [rows, 2]) per pair, each what
    nn_bruteforcel1k2(tables[database], tables[query]) returns.  The arrays of the list are views of one
    concatenated result, to which spv_ratio_test applies as it stands: its matches are (row of the
    concatenated output, row within the database table).
    """
    tables = [np.ascontiguousarray(t) for t in tables]
    dim = _table_width(tables, np.uint8, "uint8")
    col.check_matcher_dim(dim)
    n, seg, prs, out_off = _tables_and_pairs(tables, pairs)
    desc = np.concatenate(tables) if seg[-1] else np.zeros((0, dim), np.uint8)
    idx = np.empty((int(out_off[-1]), 2), np.uint64)
    dist = np.empty((int(out_off[-1]), 2), np.int32)
    check(clib.spv_nn_bruteforcel1k2_batch(desc.ctypes.data, seg.ctypes.data, n, dim, prs.ctypes.data, len(prs),
                                           idx.ctypes.data, dist.ctypes.data))
    return col.per_pair(out_off, idx, dist)


def nn_bruteforcel1k2_guided_batch(tables, geoms, lines, max_dist, pairs=None):
    """
    nn_bruteforcel1k2_batch searched only inside a band around each query's line (an addition: the reference has
    no such function; its BruteForceNnL1K2::find_neighbours<Filter> is the hook this fills).  `tables` is a list of
    uint8 arrays [rows_i, 128]; `geoms` the matching list of float32 arrays [rows_i, 4] whose columns 0 and 1 are
    the keypoints (u, v); `pairs` as for nn_bruteforcel1k2_batch; `lines` float64 [out_rows, 3], one line
    (l0, l1, l2) in the database view's pixels per query row of every pair, pairs back to back, or a list with one
    such array per pair.  Database row j is a candidate of a query iff |l0 u_j + l1 v_j + l2| <= max_dist.

    Returns a list with one (nn_idx uint64 [rows, 2], nn_dist int32 [rows, 2], ncand int32 [rows]) per pair: the
    two nearest candidates, ((size_t)-1, INT_MAX) where fewer than two exist, and the number of candidates.
    """
    tables = [np.ascontiguousarray(t) for t in tables]
    geoms = [np.ascontiguousarray(g) for g in geoms]
    dim = _table_width(tables, np.uint8, "uint8")
    if dim != 128:
        raise ValueError("the guided L1 2-NN takes dim 128 only (dim=%d)" % dim)
    if len(geoms) != len(tables) or any(g.ndim != 2 or g.dtype != np.float32 or g.shape != (len(t), 4)
                                        for g, t in zip(geoms, tables)):
        raise ValueError("geoms must be float32 arrays [rows, 4], one per table")
    n, seg, prs, out_off = _tables_and_pairs(tables, pairs)
    desc = np.concatenate(tables) if seg[-1] else np.zeros((0, dim), np.uint8)
    geom = np.concatenate(geoms) if seg[-1] else np.zeros((0, 4), np.float32)
    rows = int(out_off[-1])
    if isinstance(lines, (list, tuple)):
        lines = np.concatenate([np.asarray(l, np.float64).reshape(-1, 3) for l in lines]) if lines else np.zeros((0, 3))
    lines = np.ascontiguousarray(lines)
    if lines.dtype != np.float64 or lines.shape != (rows, 3):
        raise ValueError("lines must be float64 [out_rows, 3] = [%d, 3]" % rows)
    idx = np.empty((rows, 2), np.uint64)
    dist = np.empty((rows, 2), np.int32)
    ncand = np.empty((rows,), np.int32)
    check(clib.spv_nn_bruteforcel1k2_guided_batch(desc.ctypes.data, geom.ctypes.data, seg.ctypes.data, n, dim,
                                                  prs.ctypes.data, len(prs), lines.ctypes.data, float(max_dist),
                                                  idx.ctypes.data, dist.ctypes.data, ncand.ctypes.data))
    return col.per_pair(out_off, idx, dist, ncand)


def match_tracks_batch(sizes, pairs, matches, masks=None, min_len=2):
    """
    Multi-view tracks from the matches of many table pairs (an addition: the reference has no such function; its
    pipeline stops at two views).  `sizes` holds the rows of every table, `pairs` is a list of (query table,
    database table) numbers, `matches` a list with one integer array [k_p, 2] of (query row, database row) per pair,
    `masks` None or a list with one array [k_p] per pair: a match counts only where its mask entry is not zero.
    Matches whose rows lie outside their tables are skipped.

    The keypoints are the nodes of a graph, the matches its edges; a track is a connected component of at least
    `min_len` keypoints.  Returns (track_off int64 [ntracks + 1], members int32 [nmembers, 2] = (table, row), flags
    uint8 [ntracks]): track t owns members[track_off[t]:track_off[t + 1]], ascending by table and row; tracks are
    in ascending order of their first member; bit 0 of flags[t] is set iff the track holds two keypoints of one table.
    """
    n, seg = col.offsets_of_sizes(sizes, "table")
    prs = col.pair_table(pairs, n, "tables")
    out_off = col.out_offsets(seg, prs, below_2_31=True)
    if int(min_len) != min_len or int(min_len) < 2:
        raise ValueError("min_len must be an integer >= 2: a track has at least two members")
    if len(matches) != len(prs) or (masks is not None and len(masks) != len(prs)):
        raise ValueError("matches (and masks) must hold one array per pair")
    rows, keep = [], []
    for p in range(len(prs)):
        m = np.asarray(matches[p]).reshape(-1, 2).astype(np.int64)
        k = np.ones(len(m), bool) if masks is None else np.asarray(masks[p]).reshape(-1) != 0
        if len(k) != len(m):
            raise ValueError("mask %d has %d entries for %d matches" % (p, len(k), len(m)))
        k = k & (m[:, 0] >= 0) & (m[:, 0] < out_off[p + 1] - out_off[p])   # a query row outside its table is no out row
        m = m[k]
        rows.append(np.stack([m[:, 0] + out_off[p], np.clip(m[:, 1], -1, 2 ** 31 - 1)], 1))
    cat = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 2)), dtype=np.int32)
    if len(cat) >= 2 ** 31:
        raise ValueError("fewer than 2^31 matches in all")
    total, bound = int(seg[-1]), min(int(seg[-1]), 2 * len(cat))
    label, track = np.empty(total, np.int32), np.empty(total, np.int32)
    track_off, members = np.empty(bound // 2 + 1, np.int64), np.empty((bound, 2), np.int32)
    flags, counts = np.empty(bound // 2, np.uint8), np.zeros(2, np.int32)
    check(clib.spv_tracks_batch(seg.ctypes.data, n, prs.ctypes.data, len(prs), cat.ctypes.data, len(cat), None,
                                int(min_len), 0, label.ctypes.data, track.ctypes.data, track_off.ctypes.data,
                                members.ctypes.data, flags.ctypes.data, counts.ctypes.data))
    nt, nm = int(counts[0]), int(counts[1])
    return track_off[:nt + 1].copy(), members[:nm].copy(), flags[:nt].copy()


# ==================================================================================
# brute-force p-norm k-NN     (reference spectavi/feature.py:204-289)
# ==================================================================================
_nn_bruteforce = clib.nn_bruteforce
_nn_bruteforcei = clib.nn_bruteforcei

BRUTEFORCE_MAX_K = 64
BRUTEFORCE_MAX_DIM = 2048


def check_bruteforce_args(xshape, yshape, k, p):
    """The limits of nn_bruteforce (include/spectavi_amd.h) as ValueError, before any device work."""
    if len(xshape) != 2 or len(yshape) != 2:
        raise ValueError("x and y must be 2-D")
    if xshape[1] != yshape[1]:
        raise ValueError("x and y must have the same number of columns (%d != %d)" % (xshape[1], yshape[1]))
    if not 1 <= xshape[1] <= BRUTEFORCE_MAX_DIM:
        raise ValueError("dim=%d outside [1, %d]" % (xshape[1], BRUTEFORCE_MAX_DIM))
    if int(k) != k or not 1 <= k <= BRUTEFORCE_MAX_K:
        raise ValueError("k=%r outside [1, %d]" % (k, BRUTEFORCE_MAX_K))
    pf = np.float32(p)  # what the library receives (a C float)
    if not (np.isfinite(pf) and pf > 0):
        raise ValueError("p=%r: a finite p > 0 is required" % (p,))


def nn_bruteforce(x, y, p=.5, mu=0., k=2, use_int=False):
    """
    Exact k nearest neighbours of every row of `y` (queries) among the rows of `x`
    (database) under the p-norm distance sum_c |x_c - y_c|^p (no p-th root), on the GPU.

    The distance of each pair is the sequential, unfused float32 sum over the columns of
    |d|, d*d, sqrtf(|d|) (p = 1, 2, 0.5; bit-exact) or float(pow(|d|, p)) (other p); with
    `use_int` the rows are ``np.round(100 * x).astype('int32')`` and every term is truncated
    to int and summed in int32 (reference spectavi/feature.py:204-289).  Ties are broken by
    the lower database index.  `mu` is accepted and ignored: the result is always exact.

    Returns
    -------
    nn_idx : uint64 ndarray [yrows, k]   index into `x`, nearest first
    nn_dist : float32 (int32 with `use_int`) ndarray [yrows, k], ascending
    With fewer than k database rows the missing columns hold idx 2**64-1 and dist
    +inf (INT_MAX with `use_int`).

    Raises ValueError for k outside [1, 64], dim outside [1, 2048], mismatched
    column counts and p that is not finite and > 0.
    """
    x = np.asarray(x)
    y = np.asarray(y)
    check_bruteforce_args(x.shape, y.shape, k, p)
    k = int(k)
    xrows, dim = x.shape
    yrows = y.shape[0]
    nn_idx = NdArray(dtype='uint64')
    if not use_int:
        nn_dist = NdArray(dtype='float32')
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y, dtype=np.float32)
        _nn_bruteforce(x, y, xrows, yrows, dim, k, p, mu, ct.byref(nn_idx), ct.byref(nn_dist))
    else:
        nn_dist = NdArray(dtype='int32')
        xi = np.ascontiguousarray(np.round(100 * x).astype('int32'))
        yi = np.ascontiguousarray(np.round(100 * y).astype('int32'))
        _nn_bruteforcei(xi, yi, xrows, yrows, dim, k, p, mu, ct.byref(nn_idx), ct.byref(nn_dist))
    check()
    return nn_idx.asarray(), nn_dist.asarray()


# ==================================================================================
# approximate L2 k-NN         (reference spectavi/feature.py:161-199)
# ==================================================================================
_ann_hnswlib = clib.ann_hnswlib
_spv_ann_l2 = clib.spv_ann_l2

ANN_MAX_NCAND = 256


def check_ann_args(xshape, yshape, k, ncand=0):
    """The limits of ann_hnswlib / spv_ann_l2 (include/spectavi_amd.h) as ValueError, before any device work."""
    if len(xshape) != 2 or len(yshape) != 2:
        raise ValueError("x and y must be 2-D")
    if xshape[1] != yshape[1]:
        raise ValueError("x and y must have the same number of columns (%d != %d)" % (xshape[1], yshape[1]))
    if not 1 <= xshape[1] <= BRUTEFORCE_MAX_DIM:
        raise ValueError("dim=%d outside [1, %d]" % (xshape[1], BRUTEFORCE_MAX_DIM))
    if int(k) != k or not 1 <= k <= BRUTEFORCE_MAX_K:
        raise ValueError("k=%r outside [1, %d]" % (k, BRUTEFORCE_MAX_K))
    if int(ncand) != ncand or (ncand != 0 and not k <= ncand <= ANN_MAX_NCAND):
        raise ValueError("ncand=%r outside [k=%d, %d] (0: the default max(16, 4k))" % (ncand, k, ANN_MAX_NCAND))


def ann_hnswlib(x, y, k=2):
    """
    Approximate L2 k nearest neighbours of every row of `y` (queries) among the rows of `x`
    (database), indices only: the reference's call (spectavi/feature.py:172-199), answered by a
    coarse score of every pair on the bf16 matrix cores and an exact re-rank of the best
    max(16, 4k) rows of each query (include/spectavi_amd.h, ann_hnswlib).  `ann_l2` also takes
    the candidate count and returns the distances.

    Returns
    -------
    nn_idx : uint64 ndarray [yrows, k]   index into `x`, nearest first; 2**64-1 where `x` has
    fewer than k rows.
    """
    x = np.asarray(x)
    y = np.asarray(y)
    check_ann_args(x.shape, y.shape, k)
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    xrows, dim = x.shape
    yrows = y.shape[0]
    ann_ret = NdArray(dtype='uint64')
    _ann_hnswlib(x, y, xrows, yrows, dim, int(k), ct.byref(ann_ret))
    check()
    return ann_ret.asarray()


def ann_l2(x, y, k=2, ncand=0, return_dist=False):
    """
    `ann_hnswlib` with `ncand` candidates per query (0: max(16, 4k); otherwise k <= ncand <= 256)
    and, with `return_dist`, the distances: float32 [yrows, k], the exact sequential unfused
    sum of (x - y)**2 of every returned pair, ascending; +inf where a neighbour is missing.
    The result is a function of (x, y, k, ncand) alone; a larger `ncand` never gives a larger
    j-th distance; on integer rows inside one window of 256 values and dim <= 128 it equals
    ``nn_bruteforce(x, y, p=2, k=k)`` bit for bit.
    """
    x = np.asarray(x)
    y = np.asarray(y)
    check_ann_args(x.shape, y.shape, k, ncand)
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    xrows, dim = x.shape
    yrows = y.shape[0]
    idx = np.empty((yrows, int(k)), np.uint64)
    dist = np.empty((yrows, int(k)), np.float32) if return_dist else None
    check(_spv_ann_l2(x.ctypes.data, y.ctypes.data, xrows, yrows, dim, int(k), int(ncand), idx.ctypes.data,
                      dist.ctypes.data if return_dist else None))
    return (idx, dist) if return_dist else idx


# ==================================================================================
# k-medians exports           (reference spectavi/feature.py:313-337)
# ==================================================================================
_nn_kmedians = clib.nn_kmedians


def nn_kmedians(x, y, k, c=5):
    """
    The reference's k-medians matcher (spectavi/feature.py:328-337), answered exactly: the L1
    k nearest neighbours, ``nn_bruteforce(x, y, p=1., k=k)``, which is what the reference's randomly
    seeded cluster filter approximates.  `c` only sets the cluster counts the library ignores.

    Returns (uint64 [yrows, k], float32 [yrows, k]).
    """
    x = np.asarray(x)
    y = np.asarray(y)
    check_bruteforce_args(x.shape, y.shape, k, 1.)
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    xrows, dim = x.shape
    yrows, ydim = y.shape
    nmx = int(np.round(np.sqrt(xrows / c) * c))
    nmy = int(np.round(np.sqrt(yrows / c) * c))
    assert ydim == dim
    nn_idx = NdArray(dtype='uint64')
    nn_dist = NdArray(dtype='float32')
    _nn_kmedians(x, y, xrows, yrows, dim, nmx, nmy, c, int(k), ct.byref(nn_idx), ct.byref(nn_dist))
    check()
    return nn_idx.asarray(), nn_dist.asarray()


# ==================================================================================
# cascading hash              (reference spectavi/feature.py:346-376)
# ==================================================================================
_nn_cascading_hash = clib.nn_cascading_hash
_spv_nn_cascading_hash = clib.spv_nn_cascading_hash
_spv_generate_hash_dict = clib.spv_generate_hash_dict


def auto_hash_bit_rate(xrows, yrows):
    """`m` auto-tune of the reference: ~6 points per hash code
    (reference spectavi/feature.py:364-367)."""
    mrows = max([xrows, yrows])
    return int(np.floor(np.log2(mrows / 6.)))


def nn_cascading_hash(x, y, k=2, m=None, n=2, g=2):
    """
    Approximate L1 2-NN through a cascade of `n` random-hyperplane hash tables of
    `m` bits probed at the `g` least-confident bits, then exact L1 over the
    candidates (reference spectavi/feature.py:360-376).  `x`, `y` are float32,
    integer-valued in [-128,127] (see `normalize_to_ubyte_and_multiple_16_dim`).

    Returns (uint64 [yrows,k], float32 [yrows,k]); with `m=None` and fewer than
    ~96 rows the reference falls back to exact brute force on the +128 shifted
    bytes and returns int32 distances -- reproduced here.
    """
    xrows, xdim = x.shape
    yrows, ydim = y.shape
    assert ydim == xdim
    if m is None:  # auto-tune `m` if specified with None
        m = auto_hash_bit_rate(xrows, yrows)
        if m < 4:
            # using hashes is not appropriate:
            return nn_bruteforcel1k2((x + 128).astype('uint8'),
                                     (y + 128).astype('uint8'), nthreads=8)
    dim = xdim
    if k != 2:
        raise ValueError("nn_cascading_hash: only k=2 is defined (the reference writes two columns)")
    if dim % 16 != 0:
        raise ValueError("Input matrix inner dimensions must be 16-byte aligned.")
    if not (1 <= m <= 31):
        raise ValueError("hash bit rate m must be in [1, 31]")
    if n < 1 or not (0 <= g <= min(m, 16)):
        raise ValueError("need n >= 1 and 0 <= g <= min(m, 16)")
    cashash_idx = NdArray(dtype='uint64')
    cashash_dist = NdArray(dtype='float32')
    _nn_cascading_hash(x, y, xrows, yrows, dim, k, m, n, g, ct.byref(cashash_idx), ct.byref(cashash_dist))
    check()
    return cashash_idx.asarray(), cashash_dist.asarray()


def generate_hash_dict(seed, dim, m, n):
    """float32 [n, dim, m] hyperplanes exactly as `nn_cascading_hash` draws them
    for a given std::mt19937 seed (reference src/CascadingHashNn.h:86-100)."""
    d = np.empty((n, dim, m), np.float32)
    check(_spv_generate_hash_dict(int(seed) & 0xFFFFFFFF, dim, m, n, d))
    return d


def nn_cascading_hash_with_dict(x, y, hash_dict, g=2, return_ncand=False):
    """`nn_cascading_hash` with explicit hyperplanes `hash_dict` float32 [n, dim, m]
    (reproducible: the reference seeds from std::random_device)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    hash_dict = np.ascontiguousarray(hash_dict, dtype=np.float32)
    xrows, dim = x.shape
    yrows, ydim = y.shape
    assert ydim == dim
    n, ddim, m = hash_dict.shape
    assert ddim == dim
    idx = np.empty((yrows, 2), np.uint64)
    dist = np.empty((yrows, 2), np.float32)
    ncand = np.zeros(yrows, np.int32)
    check(_spv_nn_cascading_hash(x, y, xrows, yrows, dim, m, n, g, hash_dict, idx, dist,
                                 ncand.ctypes.data if return_ncand else None))
    if return_ncand:
        return idx, dist, ncand
    return idx, dist


def nn_cascading_hash_batch(tables, hash_dict, pairs=None, g=2, return_ncand=False):
    """
    nn_cascading_hash_with_dict for many pairs of tables in one call (an addition: the reference has no such
    function).  `tables` is a list of float32 arrays [rows_i, dim], one width for all; `hash_dict` float32
    [n, dim, m], one for the collection; `pairs` a list of (query table, database table) numbers, by default
    every i < j as (query j, database i).  Every table is projected and bucket-sorted once, whatever number of
    pairs it takes part in.

    Returns a list with one (nn_idx uint64 [rows, 2], nn_dist float32 [rows, 2][, ncand int32 [rows]]) per pair,
    each what nn_cascading_hash_with_dict(tables[database], tables[query], hash_dict, g) returns.  The arrays of
    the list are views of one concatenated result, to which spv_ratio_test applies as it stands.
    """
    tables = [np.ascontiguousarray(t, dtype=np.float32) for t in tables]
    hash_dict = np.ascontiguousarray(hash_dict, dtype=np.float32)
    dim = _table_width(tables, np.float32, "float32")
    if hash_dict.ndim != 3 or hash_dict.shape[1] != dim:
        raise ValueError("hash_dict must be float32 [n, dim, m] of the tables' width")
    col.check_matcher_dim(dim)
    ntab, _, m = hash_dict.shape
    if not 1 <= m <= 31:
        raise ValueError("hash bit rate m must be in [1, 31]")
    if ntab < 1 or not 0 <= g <= min(m, 16):
        raise ValueError("need n >= 1 and 0 <= g <= min(m, 16)")
    n, seg, prs, out_off = _tables_and_pairs(tables, pairs)
    rows = np.concatenate(tables) if seg[-1] else np.zeros((0, dim), np.float32)
    idx = np.empty((int(out_off[-1]), 2), np.uint64)
    dist = np.empty((int(out_off[-1]), 2), np.float32)
    ncand = np.zeros(int(out_off[-1]), np.int32)
    check(clib.spv_nn_cascading_hash_batch(rows.ctypes.data, seg.ctypes.data, n, dim, m, ntab, g, prs.ctypes.data,
                                           len(prs), hash_dict.ctypes.data, idx.ctypes.data, dist.ctypes.data,
                                           ncand.ctypes.data if return_ncand else None))
    return col.per_pair(out_off, idx, dist, ncand) if return_ncand else col.per_pair(out_off, idx, dist)


# ==================================================================================
# normalization               (reference spectavi/feature.py:384-407)
# ==================================================================================
def normalize_to_ubyte_and_multiple_16_dim(x, dtype='float32'):
    """
    Normalize a data matrix to:
    - have zero mean for each column
    - be in the range [-128,127]
    - have a column count that is a multiple of 16 (zero padded)
    - the required `dtype`
    for use with `nn_cascading_hash` (expects [-128,127]) and, after `+128`,
    `nn_bruteforcel1k2` (expects [0,255]).
    """
    x0 = x - np.mean(x, axis=0, keepdims=True)  # de-mean
    max_per_col = np.max(x0, axis=0, keepdims=True)
    min_per_col = np.min(x0, axis=0, keepdims=True)
    norm = np.max(np.stack([max_per_col, -min_per_col]), axis=0)
    x0 = np.round(x0 / norm * 128)
    x0[x0 > 127] = 127
    x0[x0 < -128] = -128
    xrows, dim = x0.shape
    new_dim = int(np.ceil(dim / 16.) * 16)
    xx = np.zeros([xrows, new_dim])
    xx[:, :dim] = x0
    return xx.astype(dtype)


# ==================================================================================
# ratio test + match compaction (reference example/ex01_essential_estimation.py:102-106)
# ==================================================================================
_spv_ratio_test = clib.spv_ratio_test


def ratio_test_matches(nn_idx, nn_dist, min_ratio):
    """
    The match filter of the reference's pipeline, on the GPU:
    ``pass = nn_dist[:,1] / nn_dist[:,0].astype('float64') >= min_ratio`` and the
    compaction ``(where(pass), nn_idx[pass, 0])``.  Returns int32 [nmatch, 2] rows
    (query row, database row) in ascending query order.  Queries without any
    neighbour never pass.
    """
    nn_idx = np.ascontiguousarray(nn_idx, dtype=np.uint64)
    if nn_dist.dtype == np.float32:
        is_float, nn_dist = 1, np.ascontiguousarray(nn_dist)
    else:
        is_float, nn_dist = 0, np.ascontiguousarray(nn_dist, dtype=np.int32)
    yrows = nn_idx.shape[0]
    assert nn_idx.shape == (yrows, 2) and nn_dist.shape == (yrows, 2)
    matches = np.empty((yrows, 2), np.int32)
    count = ct.c_int32(0)
    check(_spv_ratio_test(nn_idx, nn_dist.ctypes.data, is_float, yrows, float(min_ratio), matches,
                          ct.byref(count)))
    return matches[:count.value].copy()


# ==================================================================================
# SIFT table adapter (reference src/Sift.h:13,115-123: rows of 132 floats)
# ==================================================================================
_spv_sift_split = clib.spv_sift_split


def split_sift_table(table):
    """Split the reference's SIFT table (float32 [n,132] = x, y, sigma, angle + 128 descriptor
    values that are uint8(512*d) stored as float) into (geometry float32 [n,4], descriptors
    uint8 [n,128]) so that `nn_bruteforcel1k2` runs on the true 128-D bytes."""
    table = np.ascontiguousarray(table, dtype=np.float32)
    if table.ndim != 2 or table.shape[1] != 132:
        raise TypeError("SIFT table must be [n, 132]")
    n = table.shape[0]
    geom = np.empty((n, 4), np.float32)
    desc = np.empty((n, 128), np.uint8)
    check(_spv_sift_split(table, n, geom, desc))
    return geom, desc


# ==================================================================================
# normalisation on device (same result as normalize_to_ubyte_and_multiple_16_dim above)
# ==================================================================================
_spv_normalize = clib.spv_normalize


def normalize_to_ubyte_and_multiple_16_dim_gpu(x, want_ubyte=False):
    """`normalize_to_ubyte_and_multiple_16_dim(x)` for a float32 `x`, computed on the GPU and
    bit-identical to the numpy version; with `want_ubyte` also returns the
    `(out + 128).astype('uint8')` image that `nn_bruteforcel1k2` takes.  A single-column
    table (which numpy sums pairwise instead of row by row) is refused with SpectaviError."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    rows, dim = x.shape
    dim16 = int(np.ceil(dim / 16.) * 16)
    out = np.empty((rows, dim16), np.float32)
    u8 = np.empty((rows, dim16), np.uint8) if want_ubyte else None
    check(_spv_normalize(x, rows, dim, out.ctypes.data, u8.ctypes.data if want_ubyte else None))
    return (out, u8) if want_ubyte else out


def normalize_to_ubyte_and_multiple_16_dim_batch(tables, want_ubyte=False):
    """`normalize_to_ubyte_and_multiple_16_dim_gpu` for many tables in one call (an addition: the reference
    normalises table by table).  `tables` is a list of arrays [rows_i, dim], all float32 or all uint8 (whose values
    stand for their float32 conversions), one width for all; empty tables are allowed.

    Returns a list with one result per table, each what normalize_to_ubyte_and_multiple_16_dim_gpu(table,
    want_ubyte) returns; the arrays of the list are views of one concatenated result."""
    tables = [np.ascontiguousarray(t) for t in tables]
    if not tables:
        return []
    dim = tables[0].shape[1] if tables[0].ndim == 2 else -1
    dtype = tables[0].dtype
    if dtype not in (np.float32, np.uint8) or any(t.ndim != 2 or t.dtype != dtype or t.shape[1] != dim for t in tables):
        raise ValueError("tables must be arrays [rows, dim] of one width, all float32 or all uint8")
    if not 1 <= dim <= 2048:
        raise ValueError("the many-tables form takes 1 <= dim <= 2048 (dim=%d)" % dim)
    seg = col.offsets_of([len(t) for t in tables])
    x = np.concatenate(tables)
    dim16 = (dim + 15) // 16 * 16
    out = np.empty((int(seg[-1]), dim16), np.float32)
    u8 = np.empty((int(seg[-1]), dim16), np.uint8) if want_ubyte else None
    check(clib.spv_normalize_batch(x.ctypes.data, int(dtype == np.uint8), seg.ctypes.data, len(tables), dim,
                                   out.ctypes.data, u8.ctypes.data if want_ubyte else None))
    return col.per_pair(seg, out, u8) if want_ubyte else [o for o, in col.per_pair(seg, out)]


# ==================================================================================
# SIFT                        (reference spectavi/feature.py:17-148)
# ==================================================================================
_sift_filter = clib.sift_filter
_sift_filter_batch_create = clib.sift_filter_batch_create
_sift_filter_batch_destroy = clib.sift_filter_batch_destroy
_sift_filter_batch_register_image = clib.sift_filter_batch_register_image
_sift_filter_batch_process = clib.sift_filter_batch_process
_spv_sift_table = clib.spv_sift_table


def _gray(im):
    if len(np.shape(im)) != 2:
        raise TypeError("Only 2d images are supported.")
    return np.ascontiguousarray(im, dtype=np.float32)


def sift_filter(im):
    """
    SIFT keypoints and descriptors of a grayscale image `im` (2-d): vlfeat with default settings
    (include/spectavi_amd.h, sift_filter).

    Returns
    -------
    kps : float32 ndarray [nkp, 132]
        x, y, sigma, angle, then 128 descriptor values (uint8 stored as float).
    """
    im = _gray(im)
    hgt, wid = im.shape
    ret = NdArray(dtype='float32')
    _sift_filter(im, wid, hgt, ret)
    check()
    return ret.asarray()


def sift_table(im, capacity):
    """sift_filter into a table of `capacity` rows: (table float32 [capacity, 132], true row count).
    A result longer than `capacity` raises SpectaviError (SPV_ERR_OVERFLOW) naming the true count."""
    im = _gray(im)
    hgt, wid = im.shape
    table = np.zeros((max(int(capacity), 0), 132), np.float32)
    count = ct.c_int32(0)
    check(_spv_sift_table(im, wid, hgt, table, int(capacity), ct.byref(count)))
    return table, int(count.value)


def sift_filter_batch(ims, nthread=8):
    """
    sift_filter of every image of the list `ims`, processed on the GPU one after another.
    `nthread` is accepted for the reference's signature and ignored.

    Returns
    -------
    kps : list of float32 ndarrays [nkp, 132], one per image.
    """
    ims = [_gray(im) for im in ims]
    nims = len(ims)
    nthread = int(np.min([nims, nthread])) if nims else 0
    sfb = _sift_filter_batch_create()
    if not sfb:
        raise MemoryError("sift_filter_batch_create failed")
    rets = [NdArray(dtype='float32') for _ in range(nims)]
    try:
        for im, ret in zip(ims, rets):
            hgt, wid = im.shape
            _sift_filter_batch_register_image(sfb, im, wid, hgt, ret)
            check()
        _sift_filter_batch_process(sfb, nthread)
        check()
    finally:
        _sift_filter_batch_destroy(sfb)
    return [ret.asarray() for ret in rets]


def sift_filter_striped(im, nthread=8, buffer_size=20):
    """
    SIFT of one image cut into `nthread` horizontal stripes with `buffer_size` rows of overlap, the
    reference's stitching (reference spectavi/feature.py:96-148): each stripe's keypoints are shifted
    back by the stripe's first buffered row and kept when iy_start < y < iy_end.  Boundary effects
    make the result close to, but usually not equal to, sift_filter's.
    """
    if len(np.shape(im)) != 2:
        raise TypeError("Only 2d images are supported.")
    hgt, _ = im.shape
    split_hgt = int(np.ceil(hgt / float(nthread)))
    bboxes = list()
    ims = list()
    for iy in range(0, hgt, split_hgt):
        iy_start = iy
        iy_end = min([iy + split_hgt, hgt])
        bf_start = max([iy_start - buffer_size, 0])
        bf_end = min([iy_end + buffer_size + 1, hgt])
        bboxes.append([iy_start, iy_end, bf_start])
        ims.append(im[bf_start:bf_end])
    sifts = sift_filter_batch(ims, nthread=nthread)
    ret_sift = list()
    for bb, sift in zip(bboxes, sifts):
        iy_start, iy_end, bf_start = bb
        sy = sift[:, 1]
        sy += bf_start
        idx = (sy > iy_start) & (sy < iy_end)
        ret_sift.append(sift[idx])
    return np.vstack(ret_sift)
