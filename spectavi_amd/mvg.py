"""
``spectavi_amd.mvg``
====================
Multi-view-geometry front-end: the batched DLT triangulator of the reference's
``spectavi.mvg`` (reference spectavi/mvg.py:259-306) and its callers, the seven-point
algorithm and the RANSAC fitter (reference spectavi/mvg.py:112-248), and the image-pair
rectification (reference spectavi/mvg.py:47-106), bound to the gfx950 build of ``libspectavi.so``.
"""
import ctypes as ct

import numpy as np

from spectavi_amd import _collection as col
from spectavi_amd._lib import clib, check
from spectavi_amd.ndarray import NdArray


def hnormalize(x):
    """Homogeneous -> euclidean (reference spectavi/mvg.py:14-18)."""
    return x[..., :-1] / np.expand_dims(x[..., -1], axis=-1)


_dlt_triangulate = clib.dlt_triangulate
_dlt_reprojection_error = clib.dlt_reprojection_error


def dlt_triangulate(P0, P1, x, xp, ret_error=False):
    """
    Triangulate `npt` two-view correspondences (reference spectavi/mvg.py:282-302).

    P0, P1 : float64 [3,4] camera matrices; x, xp : float64 [npt,3] (or [3])
    homogeneous image points.  Returns float64 [npt,4] unit-norm homogeneous
    points (sign canonicalised to X[3] >= 0), or [npt,1] reprojection errors
    with `ret_error=True`.
    """
    if not (P0.shape == (3, 4) and P1.shape == (3, 4)):
        raise TypeError('P0,P1 must be camera matrices.')
    if len(x.shape) == 1:
        x = np.expand_dims(x, axis=0)
    if len(xp.shape) == 1:
        xp = np.expand_dims(xp, axis=0)
    if not (x.shape[0] == xp.shape[0]):
        raise TypeError('Must be same # points or shape.')
    if not (len(x.shape) == 2 and len(xp.shape) == 2):
        raise TypeError('Wrong dimensionality of input.')
    if not (x.shape[1] == 3 and xp.shape[1] == 3):
        raise TypeError('Coords must be homogenous.')
    npt = x.shape[0]
    if ret_error:
        dst = np.empty((npt, 1))
        _dlt_reprojection_error(P0, P1, npt, x, xp, dst)
    else:
        dst = np.empty((npt, 4))
        _dlt_triangulate(P0, P1, npt, x, xp, dst)
    check()
    return dst


def dlt_reprojection_error(P0, P1, x, xp):
    return dlt_triangulate(P0, P1, x, xp, ret_error=True)


# ==================================================================================
# RANSAC hypothesis scoring (the inner loops of reference src/RansacFitter.h:59-95)
# ==================================================================================
_spv_dlt_score_hypotheses = clib.spv_dlt_score_hypotheses


def dlt_score_hypotheses(P0, P1s, x, xp, max_error, return_mask=False):
    """
    Score candidate second cameras the way the reference's RANSAC does
    (reference src/RansacFitter.h:59-73): for every camera P1s[h] triangulate all
    correspondences against P0 and count the points whose reprojection error is
    <= `max_error` and which lie in front of both cameras.

    P0 float64 [3,4]; P1s float64 [H,3,4]; x, xp float64 [npt,3].
    Returns counts int32 [H] (and the inlier mask bool [H,npt] with `return_mask`).
    """
    P0 = np.ascontiguousarray(P0, dtype=np.float64)
    P1s = np.ascontiguousarray(P1s, dtype=np.float64)
    if P1s.ndim == 2:
        P1s = P1s[None]
    if not (P0.shape == (3, 4) and P1s.shape[1:] == (3, 4)):
        raise TypeError('P0,P1s must be camera matrices.')
    x = np.ascontiguousarray(x, dtype=np.float64)
    xp = np.ascontiguousarray(xp, dtype=np.float64)
    if not (x.ndim == 2 and xp.ndim == 2 and x.shape == xp.shape and x.shape[1] == 3):
        raise TypeError('Coords must be homogenous [npt,3] pairs.')
    nhyp, npt = P1s.shape[0], x.shape[0]
    counts = np.zeros(nhyp, np.int32)
    mask = np.zeros((nhyp, npt), np.uint8) if return_mask else None
    check(_spv_dlt_score_hypotheses(P0, P1s.reshape(-1), nhyp, npt, x, xp, float(max_error), counts,
                                    mask.ctypes.data if return_mask else None))
    return (counts, mask.astype(bool)) if return_mask else counts


# ==================================================================================
# RANSAC candidate processing (reference src/RansacFitter.h:42-95 + src/Camera.h:31-46)
# ==================================================================================
_spv_ransac_process = clib.spv_ransac_process_candidates


def process_fundamental_matrices(Fs, x0, x1, options={'required_percent_inliers': .9,
                                                     'reprojection_error_allowed': .5,
                                                     'find_best_even_in_failure': True,
                                                     'singular_value_ratio_allowed': 3e-2}, return_mask=False):
    """
    What the reference's `ransac_fitter` does with every candidate fundamental matrix of a trial
    (`RansacFitter::process_fundamental_matrix`, reference src/RansacFitter.h:42-95), for a batch of
    candidates at once: singular-value-ratio gate, E = U diag(1,1,0) V^T, the four candidate
    second cameras of E (`Essential2Cameras`, src/Camera.h:31-46), every camera scored over all
    correspondences against [I | 0], the best camera kept.  The option names and defaults are the
    reference front-end's (spectavi/mvg.py:138-143).

    Fs float64 [nF,3,3] (or [3,3]); x0, x1 float64 [npt,3] homogeneous.
    Returns a dict of arrays over the candidates: success bool [nF], inlier_count int32 [nF],
    inlier_percent float64 [nF], camera float64 [nF,3,4] (zeros where no camera qualified),
    best_camera int32 [nF] (0..3, -1 = none), essential float64 [nF,3,3] (NaN where gated),
    singular_value_ratio float64 [nF], counts4 int32 [nF,4] (-1 where gated) and, with
    `return_mask`, inlier_mask bool [nF,npt] (np.flatnonzero of a row = the reference's inlier_idx).
    """
    Fs = np.ascontiguousarray(Fs, dtype=np.float64)
    if Fs.ndim == 2:
        Fs = Fs[None]
    if Fs.ndim != 3 or Fs.shape[1:] != (3, 3):
        raise TypeError('Fs must be [nF,3,3] fundamental matrices.')
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    x1 = np.ascontiguousarray(x1, dtype=np.float64)
    if not (x0.ndim == 2 and x0.shape == x1.shape and x0.shape[1] == 3):
        raise TypeError('Coords must be homogenous [npt,3] pairs.')
    nF, npt = Fs.shape[0], x0.shape[0]
    if npt < 1:
        raise ValueError('Supplied no point matches.')
    success = np.zeros(nF, np.int32)
    count = np.zeros(nF, np.int32)
    best = np.full(nF, -1, np.int32)
    best_P = np.zeros((nF, 3, 4))
    ratio = np.zeros(nF)
    E = np.zeros((nF, 3, 3))
    counts4 = np.zeros((nF, 4), np.int32)
    mask = np.zeros((nF, npt), np.uint8) if return_mask else None
    check(_spv_ransac_process(Fs.reshape(-1), nF, x0, x1, npt, float(options['singular_value_ratio_allowed']),
                              float(options['required_percent_inliers']), float(options['reprojection_error_allowed']),
                              int(bool(options['find_best_even_in_failure'])), success, count, best,
                              best_P.reshape(-1), ratio, E.reshape(-1), counts4.reshape(-1),
                              mask.ctypes.data if return_mask else None))
    ret = {'success': success.astype(bool), 'inlier_count': count, 'inlier_percent': count / float(npt),
           'camera': best_P, 'best_camera': best, 'essential': E, 'singular_value_ratio': ratio, 'counts4': counts4}
    if return_mask:
        ret['inlier_mask'] = mask.astype(bool)
    return ret


# ==================================================================================
# seven_point_algorithm / ransac_fitter (reference spectavi/mvg.py:112-248)
# ==================================================================================
_seven_point_algorithm = clib.seven_point_algorithm


def seven_point_algorithm(x, xp):
    """
    The fundamental matrices through seven correspondences (reference spectavi/mvg.py:237-248).

    x, xp : float64 [7,2] euclidean or [7,3] homogeneous image points.
    Returns float64 [3*nroot, 3]: the nroot (0..3) solutions stacked, each with xp^T F x = 0.
    """
    if not (x.shape[0] == 7 and xp.shape[0] == 7):
        raise TypeError('Must be 7 points.')
    if not (x.shape[1] == 2 and xp.shape[1] == 2):
        x, xp = hnormalize(x), hnormalize(xp)
    x = np.ascontiguousarray(x, dtype=np.float64)
    xp = np.ascontiguousarray(xp, dtype=np.float64)
    dst = np.empty((3, 3, 3))
    nroot = ct.c_int()
    _seven_point_algorithm(x, xp, ct.byref(nroot), dst)
    check()
    nroot = nroot.value
    return np.vstack(dst[:nroot]) if nroot else np.empty((0, 3))


_spv_seven_point = clib.spv_seven_point


def seven_point_batch(x, xp, return_basis=False):
    """
    Seven-point algorithm for n independent 7-subsets at once.

    x, xp : float64 [n,7,2] euclidean.  Returns (nroot int32 [n], Fs float64 [n,3,3,3]) -- slots
    of missing roots are NaN -- and, with `return_basis`, the null-space pair [n,2,3,3].
    """
    x = np.ascontiguousarray(x, dtype=np.float64)
    xp = np.ascontiguousarray(xp, dtype=np.float64)
    if not (x.ndim == 3 and x.shape[1:] == (7, 2) and xp.shape == x.shape):
        raise TypeError('x, xp must be [n,7,2].')
    n = x.shape[0]
    nroot = np.zeros(n, np.int32)
    Fs = np.zeros((n, 3, 3, 3))
    basis = np.zeros((n, 2, 3, 3)) if return_basis else None
    check(_spv_seven_point(x.reshape(-1), xp.reshape(-1), n, nroot, Fs.reshape(-1),
                           basis.ctypes.data if return_basis else None))
    return (nroot, Fs, basis) if return_basis else (nroot, Fs)


_ransac_fitter = clib.ransac_fitter


def ransac_fitter(x0, x1, options={'required_percent_inliers': .9,
                                   'reprojection_error_allowed': .5,
                                   'maximum_tries': 500,
                                   'find_best_even_in_failure': True,
                                   'singular_value_ratio_allowed': 3e-2,
                                   'progressbar': False}):
    """
    Fit a two-view geometry to tentatively corresponding points by RANSAC
    (reference spectavi/mvg.py:131-221; same option names and defaults).

    x0, x1 : float64 [npt,3] homogeneous normalised coordinates, npt >= 10.
    Returns the reference's dict: success, essential [3,3] (the winning seven-point solution),
    camera [3,4] (second camera; the first is [I | 0]), inlier_percent, inlier_idx int32 [n,1].
    If no model was kept essential and inlier_idx are empty and camera is [I | 0].
    Set SPECTAVI_RANSAC_SEED for reproducible subsets; `progressbar` is ignored.
    """
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    x1 = np.ascontiguousarray(x1, dtype=np.float64)
    if not (x0.ndim == 2 and x0.shape == x1.shape and x0.shape[1] == 3):
        raise TypeError('Coords must be homogenous [npt,3] pairs.')
    npt = x0.shape[0]
    if npt < 10:
        raise ValueError('Supplied less than 10 point matches, unsupported.')
    success = ct.c_bool()
    essential = NdArray()
    camera = NdArray()
    inlier_idx = NdArray(dtype='int32')
    inlier_percent = ct.c_double()
    _ransac_fitter(x0, x1, npt, options['required_percent_inliers'],
                   options['reprojection_error_allowed'],
                   options['maximum_tries'],
                   options['find_best_even_in_failure'],
                   options['singular_value_ratio_allowed'],
                   options.get('progressbar', False),
                   ct.byref(success),
                   ct.byref(essential),
                   ct.byref(camera),
                   ct.byref(inlier_percent),
                   ct.byref(inlier_idx))
    check()
    return {'success': success.value,
            'essential': essential.asarray(),
            'camera': camera.asarray(),
            'inlier_percent': inlier_percent.value,
            'inlier_idx': inlier_idx.asarray(), }


_spv_ransac_sample = clib.spv_ransac_sample


def ransac_sample(seed, npt, ntries):
    """The 7-subsets int32 [ntries,7] that `ransac_fit(seed=seed)` evaluates (drawn as the reference's
    floyd_sample draws them, reference src/RansacFitter.h:120-132, from one mt19937)."""
    samples = np.zeros((ntries, 7), np.int32)
    check(_spv_ransac_sample(int(seed), int(npt), int(ntries), samples.reshape(-1)))
    return samples


_spv_ransac_fit = clib.spv_ransac_fit
_spv_ransac_fit_samples = clib.spv_ransac_fit_samples


def ransac_fit(x0, x1, required_percent_inliers=.9, reprojection_error_allowed=.5, maximum_tries=500,
               find_best_even_in_failure=True, singular_value_ratio_allowed=3e-2, seed=0, samples=None):
    """
    `ransac_fitter` with plain outputs and explicit control of the subsets: `samples` int32 [ntries,7]
    (then `maximum_tries` and `seed` are ignored) or `seed` (0 = SPECTAVI_RANSAC_SEED / random).

    Returns the `ransac_fitter` dict (essential / camera None and inlier_idx empty when no model was
    kept) plus best_try, best_root (which try and which of its roots won; -1 if none) and tries_run.
    """
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    x1 = np.ascontiguousarray(x1, dtype=np.float64)
    if not (x0.ndim == 2 and x0.shape == x1.shape and x0.shape[1] == 3):
        raise TypeError('Coords must be homogenous [npt,3] pairs.')
    npt = x0.shape[0]
    if npt < 10:
        raise ValueError('Supplied less than 10 point matches, unsupported.')
    ok, n, bt, br, ran = ct.c_int32(0), ct.c_int32(0), ct.c_int32(-1), ct.c_int32(-1), ct.c_int32(0)
    pct = ct.c_double(0.0)
    F, P, idx = np.zeros(9), np.zeros(12), np.zeros(npt, np.int32)
    outs = (ct.byref(ok), F, P, ct.byref(pct), idx, ct.byref(n), ct.byref(bt), ct.byref(br), ct.byref(ran))
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        if not (samples.ndim == 2 and samples.shape[1] == 7):
            raise TypeError('samples must be [ntries,7].')
        check(_spv_ransac_fit_samples(x0, x1, npt, float(required_percent_inliers), float(reprojection_error_allowed),
                                      samples.reshape(-1), samples.shape[0], int(bool(find_best_even_in_failure)),
                                      float(singular_value_ratio_allowed), *outs))
    else:
        check(_spv_ransac_fit(x0, x1, npt, float(required_percent_inliers), float(reprojection_error_allowed),
                              int(maximum_tries), int(bool(find_best_even_in_failure)),
                              float(singular_value_ratio_allowed), int(seed), *outs))
    found = bt.value >= 0
    return {'success': bool(ok.value), 'essential': F.reshape(3, 3) if found else None,
            'camera': P.reshape(3, 4) if found else None, 'inlier_percent': float(pct.value),
            'inlier_idx': idx[:n.value].copy(), 'best_try': bt.value, 'best_root': br.value,
            'tries_run': ran.value}


_spv_ransac_fit_batch = clib.spv_ransac_fit_batch


def _coordinate_sets(x0s, x1s):
    """Two lists of float64 [npt_p, 3] arrays, set for set of one shape (TypeError otherwise) -> (the sets of x0s, x0
    and x1 [total, 3] with the sets back to back, npairs, off int64[npairs + 1], total) under the rules of
    spv_ransac_fit_batch and spv_dlt_triangulate_batch."""
    a0 = [np.ascontiguousarray(x, dtype=np.float64) for x in x0s]
    a1 = [np.ascontiguousarray(x, dtype=np.float64) for x in x1s]
    for u, v in zip(a0, a1):
        if not (u.ndim == 2 and u.shape == v.shape and u.shape[1] == 3):
            raise TypeError('Coords must be homogenous [npt,3] pairs.')
    off = col.offsets(col.offsets_of([len(u) for u in a0]), "the sets' offsets")
    col.check_set_count(len(a0))
    total = int(off[-1])
    return (a0, np.concatenate(a0) if total else np.zeros((0, 3)), np.concatenate(a1) if total else np.zeros((0, 3)),
            len(a0), off, total)


def ransac_fit_batch(x0s, x1s, required_percent_inliers=.9, reprojection_error_allowed=.5, maximum_tries=500,
                     find_best_even_in_failure=True, singular_value_ratio_allowed=3e-2, seeds=None, samples=None):
    """
    `ransac_fit` for many correspondence sets in one call: x0s, x1s are lists of float64 [npt_p,3] arrays
    (npt_p may be anything; a set of fewer than 10 rows is skipped: success False, no model, tries_run 0).
    `samples`: a list of int32 [ntries,7] arrays, one per set, all of one ntries (`maximum_tries` and `seeds`
    are then ignored), or `seeds`: one value per set (0 = SPECTAVI_RANSAC_SEED / random).

    Returns a list of `ransac_fit` dicts, each bit for bit what `ransac_fit` returns for that set alone with
    the same subsets, but for tries_run (the rounds of the call cut the tries differently).
    """
    if len(x0s) != len(x1s):
        raise ValueError('x0s and x1s must hold one array per set each.')
    a0, x0, x1, npairs, off, total = _coordinate_sets(x0s, x1s)
    if samples is not None:
        if len(samples) != npairs:
            raise ValueError('samples must hold one [ntries,7] array per set.')
        rows = [np.asarray(s) for s in samples]
        ntries = rows[0].shape[0] if npairs else 0
        for p, s in enumerate(rows):
            if not (s.ndim == 2 and s.shape == (ntries, 7)):
                raise ValueError('samples must be [ntries,7] arrays of one ntries.')
            if len(a0[p]) >= 10 and s.size and (s.min() < 0 or s.max() >= len(a0[p])):
                raise ValueError('a sample row lies outside its set')
        samples = np.ascontiguousarray(np.stack(rows) if npairs else np.zeros((0, 0, 7)), dtype=np.int32)
    seeds, maximum_tries = col.seeds_and_tries(seeds, samples, maximum_tries, npairs)
    ok, n, bt, br, ran = (np.zeros(npairs, np.int32) for _ in range(5))
    pct, F, P, idx = np.zeros(npairs), np.zeros((npairs, 9)), np.zeros((npairs, 12)), np.zeros(total, np.int32)
    check(_spv_ransac_fit_batch(x0.ctypes.data, x1.ctypes.data, off.ctypes.data, npairs, float(required_percent_inliers),
                                float(reprojection_error_allowed), maximum_tries, int(bool(find_best_even_in_failure)),
                                float(singular_value_ratio_allowed),
                                samples.ctypes.data if samples is not None else None,
                                seeds.ctypes.data if samples is None else None, ok.ctypes.data, F.ctypes.data,
                                P.ctypes.data, pct.ctypes.data, idx.ctypes.data, n.ctypes.data, bt.ctypes.data,
                                br.ctypes.data, ran.ctypes.data))
    return col.fit_dicts(off, ok, F, P, pct, idx, n, bt, br, ran)


_spv_dlt_triangulate_batch = clib.spv_dlt_triangulate_batch


def dlt_triangulate_batch(P1s, x0s, x1s, P0s=None, masks=None, ret_error=False):
    """
    `dlt_triangulate` for many correspondence sets in one call, each with its own cameras: x0s, x1s are lists of
    float64 [npt_p,3] arrays, P1s a list of [3,4] second cameras -- a None entry skips its set, which is what a
    `ransac_fit_batch` row without a model becomes --, P0s a list of first cameras or None for [I|0] everywhere (the
    frame `ransac_fit_batch`'s cameras are expressed in).  `masks`: a list of per-set row selections (anything
    non-zero selects; a None entry selects the whole set), e.g. built from the fits' inlier_idx.

    Returns a list with one float64 [n_p,4] array per set, the selected rows in input order ([0,4] for a skipped
    set), each bit for bit what `dlt_triangulate` returns for those rows alone; with `ret_error` also the list of
    [n_p,1] reprojection errors.
    """
    if not (len(x0s) == len(x1s) == len(P1s)):
        raise ValueError('P1s, x0s and x1s must hold one entry per set each.')
    a0, x0, x1, npairs, off, total = _coordinate_sets(x0s, x1s)
    c1, use = col.listed_cameras(P1s, npairs, 'P1s', TypeError)
    if P0s is not None and len(P0s) != npairs:
        raise ValueError('P0s must hold one camera per set.')
    c0 = None if P0s is None else col.listed_cameras(P0s, npairs, 'P0s', TypeError, needed=use)[0]
    mask = None
    if masks is not None:
        if len(masks) != npairs:
            raise ValueError('masks must hold one entry per set.')
        mask = np.ones(total, np.uint8)
        for p, m in enumerate(masks):
            if m is None:
                continue
            m = np.asarray(m).reshape(-1)
            if m.size != len(a0[p]):
                raise ValueError('a mask must hold one value per row of its set')
            mask[off[p]:off[p + 1]] = m != 0
    X = np.empty((total, 4))
    err = np.empty(total) if ret_error else None
    out_off = np.zeros(npairs + 1, np.int64)
    count = ct.c_longlong(0)
    check(_spv_dlt_triangulate_batch(x0.ctypes.data, x1.ctypes.data, off.ctypes.data, npairs,
                                     c0.ctypes.data if c0 is not None else None, c1.ctypes.data, use.ctypes.data,
                                     mask.ctypes.data if mask is not None else None, X.ctypes.data,
                                     err.ctypes.data if ret_error else None, None, total, out_off.ctypes.data,
                                     ct.addressof(count)))
    Xs = [X[out_off[p]:out_off[p + 1]].copy() for p in range(npairs)]
    if ret_error:
        return Xs, [err[out_off[p]:out_off[p + 1]].reshape(-1, 1).copy() for p in range(npairs)]
    return Xs


def triangulate_tracks(coords, sizes, cameras, track_off, members, max_error=float('inf'), use=None):
    """
    One 3-D point per multi-view track from all its observations (an addition: the reference stops at two views).
    `coords` is a list with one [n_v, >=2] array per view whose first two columns are the keypoints' x and y (they
    are rounded to float32, the precision of a SIFT table), `sizes` the rows of every view as `match_tracks_batch`
    takes them (None: the rows of coords), `cameras` one [3,4] camera per view -- a None entry is a view without a
    camera --, `use` an optional per-view switch, (`track_off`, `members`) what `match_tracks_batch` returned.  The
    cameras are taken as given; `resect_batch` estimates those of views that see points already triangulated.

    Returns numpy arrays (X float64 [ntracks,4], err float64 [nmembers], ok uint8 [ntracks], nused int32 [ntracks]).
    A member is usable when its view and row exist and the view has a camera.  X is the unit null vector of the
    track's 2m x 4 DLT matrix, sign as `dlt_triangulate` gives it, all zeros for a track with fewer than 2 usable
    members; err is the image-plane residual of every usable member of a solved track, NaN elsewhere; ok is 1 where
    the track is solved, X is finite, the point lies in front of every usable member's camera and every err <=
    max_error; nused counts the usable members.
    """
    arrs = [np.asarray(c) for c in coords]
    for a in arrs:
        if a.ndim != 2 or a.shape[1] < 2:
            raise ValueError('coords must hold one [n, >=2] array per view.')
    if sizes is None:
        sizes = [len(a) for a in arrs]
    nseg, seg = col.offsets_of_sizes(sizes, 'view')
    if len(arrs) != nseg or any(len(a) != n for a, n in zip(arrs, np.diff(seg))):
        raise ValueError('coords must hold sizes[v] rows for every view.')
    if len(cameras) != nseg:
        raise ValueError('cameras must hold one entry per view.')
    cams, usable = col.listed_cameras(cameras, nseg, 'cameras', ValueError)
    if use is not None:
        usable = usable * col.use_flags(use, nseg, 'view')
    mem = np.asarray(members)
    if mem.size == 0:
        mem = np.zeros((0, 2), np.int32)
    if mem.ndim != 2 or mem.shape[1] != 2 or mem.dtype.kind not in 'iu':
        raise ValueError('members must be integers of shape [nmembers, 2].')
    off = col.offsets(track_off, 'track_off', len(mem), 'members')
    mem = np.ascontiguousarray(np.clip(mem, -1, 2 ** 31 - 1), dtype=np.int32)
    max_error = float(max_error)
    if max_error != max_error:
        raise ValueError('max_error must not be NaN.')
    geom = np.zeros((int(seg[-1]), 4), np.float32)
    for v, a in enumerate(arrs):
        geom[seg[v]:seg[v + 1], :2] = a[:, :2]
    nt, nm = off.size - 1, len(mem)
    X, err = np.zeros((nt, 4)), np.full(nm, np.nan)
    ok, nused = np.zeros(nt, np.uint8), np.zeros(nt, np.int32)
    check(clib.spv_tracks_triangulate(geom.ctypes.data, seg.ctypes.data, nseg, cams.ctypes.data, usable.ctypes.data,
                                      off.ctypes.data, nt, mem.ctypes.data, nm, max_error, X.ctypes.data,
                                      err.ctypes.data, ok.ctypes.data, nused.ctypes.data))
    return X, err, ok, nused


def camera_from_pose(R, t, K):
    """The 3x4 pixel camera K [R | t]."""
    R, t, K = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(3), np.asarray(K, dtype=np.float64)
    if R.shape != (3, 3) or K.shape != (3, 3):
        raise ValueError('R and K must be [3,3].')
    return K @ np.hstack([R, t[:, None]])


def pose_from_camera(P, K):
    """
    A general 3x4 camera, e.g. one `resect_batch` returned, as the pose `bundle_adjust` takes: (R, t) with K [R | t]
    nearest to P up to scale.  M = K^-1 P has its sign fixed by det M[:, :3] > 0 and its scale by |det M[:, :3]|^(1/3);
    R is the rotation nearest to the scaled M[:, :3] (numpy SVD), t its scaled last column.
    """
    P, K = np.asarray(P, dtype=np.float64), np.asarray(K, dtype=np.float64)
    if P.shape != (3, 4) or K.shape != (3, 3):
        raise ValueError('P must be [3,4] and K [3,3].')
    M = np.linalg.solve(K, P)
    det = np.linalg.det(M[:, :3])
    if not np.isfinite(det) or det == 0:
        raise ValueError('P has no pose: K^-1 P[:, :3] is singular.')
    M = M / (np.sign(det) * abs(det) ** (1. / 3))
    U, _, Vt = np.linalg.svd(M[:, :3])
    R = U @ np.diag([1., 1., np.linalg.det(U @ Vt)]) @ Vt
    return R, M[:, 3].copy()


def bundle_adjust(coords, sizes, K, poses, track_off, members, X, use=None, fixed=None, huber=float('inf'), max_steps=50,
                  lambda0=1e-4, ftol=1e-10, gtol=1e-10, cg_tol=1e-8, cg_max=None):
    """
    Levenberg-Marquardt refinement of all free cameras and all participating track points over all observations (an
    addition: the reference stops at two views).  `coords`, `sizes`, (`track_off`, `members`) as `triangulate_tracks`
    takes them, `X` [ntracks,4] its points, `use` an optional per-track switch (e.g. its ok), `K` one [3,3]
    calibration or one per view (held fixed), `poses` one [3,4] = [R | t] per view -- None for a view without a
    camera; `pose_from_camera` makes one of a resected camera --, `fixed` an optional per-view switch.  `huber` is the
    width of the robust loss in pixels; `cg_max` None means 6 * free cameras + 10.

    Returns (poses [nviews,3,4], X [ntracks,4], info): a track takes part when it is switched on, its X row is finite
    with X[3] != 0, it has two usable members or more and lies in front of all their cameras; its row comes back as
    (X, Y, Z, 1), every other row as it came.  info has steps, accepted, stop, tracks, observations, first_cost,
    last_cost, trace [steps, 6] = (F before, F', lambda, CG iterations, accepted, max |g|), active uint8 [ntracks]
    and err [nmembers] (the residual norm of every participating member, NaN elsewhere).
    """
    arrs = [np.asarray(c) for c in coords]
    for a in arrs:
        if a.ndim != 2 or a.shape[1] < 2:
            raise ValueError('coords must hold one [n, >=2] array per view.')
    if sizes is None:
        sizes = [len(a) for a in arrs]
    nseg, seg = col.offsets_of_sizes(sizes, 'view')
    if len(arrs) != nseg or any(len(a) != n for a, n in zip(arrs, np.diff(seg))):
        raise ValueError('coords must hold sizes[v] rows for every view.')
    Ks, P, mode = col.bundle_cameras(K, poses, fixed, nseg, 'view')
    mem = np.asarray(members)
    if mem.size == 0:
        mem = np.zeros((0, 2), np.int32)
    if mem.ndim != 2 or mem.shape[1] != 2 or mem.dtype.kind not in 'iu':
        raise ValueError('members must be integers of shape [nmembers, 2].')
    off = col.offsets(track_off, 'track_off', len(mem), 'members')
    mem = np.ascontiguousarray(np.clip(mem, -1, 2 ** 31 - 1), dtype=np.int32)
    nt, nm = off.size - 1, len(mem)
    X = np.array(X, dtype=np.float64, order='C')
    if X.shape != (nt, 4):
        raise ValueError('X must be [ntracks, 4].')
    if use is not None:
        use = np.ascontiguousarray(np.asarray(use) != 0, dtype=np.uint8).reshape(-1)
        if use.size != nt:
            raise ValueError('use must hold one value per track.')
    huber, max_steps, lambda0, ftol, gtol, cg_tol, cg_max = col.bundle_options(huber, max_steps, lambda0, ftol, gtol,
                                                                               cg_tol, cg_max, mode)
    geom = np.zeros((int(seg[-1]), 4), np.float32)
    for v, a in enumerate(arrs):
        geom[seg[v]:seg[v + 1], :2] = a[:, :2]
    err, active = np.full(nm, np.nan), np.zeros(nt, np.uint8)
    trace, info = np.full((max_steps, 6), np.nan), np.zeros(7)
    check(clib.spv_bundle_adjust(geom.ctypes.data, seg.ctypes.data, nseg, Ks.ctypes.data, P.ctypes.data, mode.ctypes.data,
                                 off.ctypes.data, nt, mem.ctypes.data, nm, X.ctypes.data,
                                 use.ctypes.data if use is not None else None, huber, max_steps, lambda0, ftol, gtol, cg_tol,
                                 cg_max, err.ctypes.data, active.ctypes.data, trace.ctypes.data, info.ctypes.data))
    out = col.bundle_info(info, trace)
    out['active'], out['err'] = active, err
    return P.reshape(nseg, 3, 4), X, out


def resect_batch(xs, Xws, required_percent_inliers=.9, max_error=2., maximum_tries=500, find_best_even_in_failure=False,
                 seeds=None, samples=None, want_tries=False):
    """
    RANSAC camera resection of many views in one call (an addition: the reference stops at two views).  `xs` is a
    list with one [n_v, >=2] array per view -- image points (u, v), a third column, if any, is the homogeneous
    scale --, `Xws` the list of [n_v, 4] homogeneous 3-D points they observe, in whatever units the caller has;
    `max_error` is in the units of xs.  `samples`: a list of int32 [ntries,6] arrays, one per view, all of one ntries
    (`maximum_tries` and `seeds` are then ignored), or `seeds`: one value per view (0 = SPECTAVI_RANSAC_SEED /
    random), the first six columns of `ransac_sample`.  A view of fewer than 6 rows is skipped.

    Returns a list of dicts (success, camera [3,4] or None, inlier_percent, inlier_idx, best_try, tries_run): a try's
    camera is the unit null vector of the 11 x 12 matrix of its six rows (the sixth with its u row only); a row is an
    inlier when it reprojects within max_error in front of the camera; the winner is the first try whose inlier share
    reaches required_percent_inliers, else -- with find_best_even_in_failure -- the try with the most inliers.  With
    `want_tries` also (try_cameras [nviews, ntries, 12], try_inliers [nviews, ntries]), every try evaluated.
    """
    if len(xs) != len(Xws):
        raise ValueError('xs and Xws must hold one array per view each.')
    ax, aX = [], []
    for u, X in zip(xs, Xws):
        u, X = np.asarray(u, dtype=np.float64), np.ascontiguousarray(X, dtype=np.float64)
        if not (u.ndim == 2 and u.shape[1] in (2, 3) and X.ndim == 2 and X.shape == (len(u), 4)):
            raise TypeError('Coords must be [npt,2] or [npt,3] with [npt,4] points.')
        ax.append(np.concatenate([u, np.ones((len(u), 1))], 1) if u.shape[1] == 2 else u)
        aX.append(X)
    nviews = len(ax)
    off = col.offsets(col.offsets_of([len(u) for u in ax]), "the views' offsets")
    col.check_set_count(nviews)
    total = int(off[-1])
    x = np.ascontiguousarray(np.concatenate(ax)) if total else np.zeros((0, 3))
    Xw = np.ascontiguousarray(np.concatenate(aX)) if total else np.zeros((0, 4))
    if samples is not None:
        if len(samples) != nviews:
            raise ValueError('samples must hold one [ntries,6] array per view.')
        rows = [np.asarray(s) for s in samples]
        if any(s.ndim != 2 or s.shape != rows[0].shape for s in rows):
            raise ValueError('samples must be [ntries,6] arrays of one ntries.')
        samples = col.sample_table(np.stack(rows) if nviews else np.zeros((0, 0, 6), np.int32), np.diff(off), 6, 6)
    seeds, maximum_tries = col.seeds_and_tries(seeds, samples, maximum_tries, nviews)
    max_error, share = float(max_error), float(required_percent_inliers)
    if max_error != max_error or share != share:
        raise ValueError('max_error and required_percent_inliers must not be NaN.')
    ok, n, bt, ran = (np.zeros(nviews, np.int32) for _ in range(4))
    pct, P, mask = np.zeros(nviews), np.zeros((nviews, 12)), np.zeros(total, np.uint8)
    cams = np.empty((nviews, maximum_tries, 12)) if want_tries else None
    inl = np.empty((nviews, maximum_tries), np.int32) if want_tries else None
    check(clib.spv_resect_fit_batch(x.ctypes.data, Xw.ctypes.data, off.ctypes.data, nviews, share, max_error, maximum_tries,
                                    int(bool(find_best_even_in_failure)),
                                    samples.ctypes.data if samples is not None else None,
                                    seeds.ctypes.data if samples is None else None, ok.ctypes.data, P.ctypes.data,
                                    pct.ctypes.data, n.ctypes.data, bt.ctypes.data, ran.ctypes.data, mask.ctypes.data,
                                    cams.ctypes.data if want_tries else None, inl.ctypes.data if want_tries else None))
    fits = col.resect_dicts(off, ok, P, pct, bt, ran, mask)
    return (fits, cams, inl) if want_tries else fits


# ==================================================================================
# image_pair_rectification (reference spectavi/mvg.py:47-106)
# ==================================================================================
_image_pair_rectification = clib.image_pair_rectification
_spv_rectify_fundamental = clib.spv_rectify_fundamental
_spv_rectify_shape = clib.spv_rectify_shape


def _cameras(P0, P1):
    P0 = np.ascontiguousarray(P0, dtype=np.float64)
    P1 = np.ascontiguousarray(P1, dtype=np.float64)
    if not (P0.shape == (3, 4) and P1.shape == (3, 4)):
        raise TypeError('P0,P1 must be camera matrices.')
    return P0, P1


def rectification_fundamental(P0, P1):
    """The fundamental matrix float64 [3,3] that `image_pair_rectification` resamples along:
    [P1 C]x P1 P0^T (P0 P0^T)^-1 with C the unit null vector of P0.  All NaN when P0 P0^T is
    singular, zero when the two camera centres coincide (every sample is then invalid)."""
    P0, P1 = _cameras(P0, P1)
    F = np.zeros(9)
    check(_spv_rectify_fundamental(P0, P1, F))
    return F.reshape(3, 3)


def rectification_shape(wid, hgt, nchan, sampling_factor):
    """(output_rows, output_cols, rnx) of a rectification, as include/spectavi_amd.h states them."""
    out = np.zeros(3, np.int32)
    check(_spv_rectify_shape(int(wid), int(hgt), int(nchan), float(sampling_factor), out))
    return tuple(int(v) for v in out)


def image_dims(shape):
    """(hgt, wid, nchan) of an image shape [hgt, wid] or [hgt, wid, nchan]."""
    if len(shape) == 2:
        return shape[0], shape[1], 1
    if len(shape) == 3:
        return shape
    raise TypeError('Images must be [hgt, wid] or [hgt, wid, nchan].')


def image_pair_rectification(P0, P1, im0, im1, sampling_factor=1.2, crop_invalid=True):
    """
    Rectify an image pair given their two camera matrices (reference spectavi/mvg.py:47-106; the
    contract is stated with image_pair_rectification in include/spectavi_amd.h).

    P0, P1 : float64 [3,4] camera matrices.  im0, im1 : images of the same shape, [hgt, wid] or
    [hgt, wid, nchan] (taken as float64).  Every output row resamples im0 along an epipolar line
    and im1 along its corresponding line, `sampling_factor` samples per input column.
    Returns (r0, r1, ri0, ri1): the rectified images float64 [rows, cols] (or [rows, cols, nchan])
    and the flat source pixel index (y * wid + x) of every sample, int32 [rows, cols], -1 (value 0)
    where a sample falls outside its image.  With `crop_invalid` all four are cropped to the
    bounding box of the samples valid in either image; ValueError if there are none.
    """
    if np.any(np.shape(im0) != np.shape(im1)):
        raise TypeError("Input images must have same size.")
    P0, P1 = _cameras(P0, P1)
    im0 = np.ascontiguousarray(im0, dtype=np.float64)
    im1 = np.ascontiguousarray(im1, dtype=np.float64)
    hgt, wid, nchan = image_dims(im0.shape)
    r0, r1 = NdArray(), NdArray()
    ri0, ri1 = NdArray(dtype='int32'), NdArray(dtype='int32')
    _image_pair_rectification(P0, P1, im0, im1, wid, hgt, nchan, float(sampling_factor),
                              ct.byref(r0), ct.byref(r1), ct.byref(ri0), ct.byref(ri1))
    check()
    r0, r1, ri0, ri1 = r0.asarray(), r1.asarray(), ri0.asarray(), ri1.asarray()
    if crop_invalid:
        y, x = np.where((ri0 != -1) | (ri1 != -1))
        if y.size == 0:
            raise ValueError("No valid rectified sample: nothing to crop to.")
        ys, xs = slice(y.min(), y.max() + 1), slice(x.min(), x.max() + 1)
        r0, r1, ri0, ri1 = r0[ys, xs, ...], r1[ys, xs, ...], ri0[ys, xs], ri1[ys, xs]
    return r0, r1, ri0, ri1


_spv_rectify_batch = clib.spv_rectify_batch
_RECTIFY_BATCH_DTYPE = {np.dtype(np.float64): 0, np.dtype(np.uint8): 1, np.dtype(np.float32): 2}  # SPV_RECTIFY_*


def image_pair_rectification_batch(ims, pairs, P1s, P0s=None, sampling_factor=1.2, crop_invalid=True):
    """
    `image_pair_rectification` for many image pairs in one call (spv_rectify_batch), cropped on the device.

    ims : list of numpy images [hgt, wid] or [hgt, wid, nchan] of one dtype and one nchan; float32 and uint8
    images keep their dtype, anything else is taken as float64.  pairs : [npairs, 2] = (image 0, image 1), numbers
    into ims; the two images of a pair have the same size.  A matcher's pair (query set, database set) is passed as
    (database, query).  P1s : list of [3,4] second cameras, a None entry skips its pair (what a `ransac_fit_batch`
    row without a model becomes); P0s : list of first cameras or None for [I|0] everywhere.

    Returns a list with one (r0, r1, ri0, ri1) per pair, each what `image_pair_rectification` returns for that pair
    alone -- cropped to the bounding box of the valid samples with `crop_invalid`, on the device, so only the boxes
    are written and brought back --, or None where a pair is skipped or, with `crop_invalid`, has no valid sample
    (the single call raises ValueError there; the batch never does).
    """
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    npairs = len(pairs)
    if len(P1s) != npairs or (P0s is not None and len(P0s) != npairs):
        raise ValueError('P1s (and P0s) must hold one entry per pair.')
    ims = [np.asarray(im) for im in ims]
    dtype = ims[0].dtype if ims and ims[0].dtype in _RECTIFY_BATCH_DTYPE else np.dtype(np.float64)
    ims = [np.ascontiguousarray(im, dtype=dtype) for im in ims]
    dims = [image_dims(im.shape) for im in ims]
    if len({d[2] for d in dims}) > 1:
        raise TypeError('Input images must have the same number of channels.')
    nchan = dims[0][2] if dims else 1
    for a, b in pairs:
        if 0 <= a < len(ims) and 0 <= b < len(ims) and ims[a].shape != ims[b].shape:
            raise TypeError("Input images must have same size.")
    sizes = np.array([(d[1], d[0]) for d in dims], dtype=np.int32).reshape(-1, 2)
    c1, use = col.listed_cameras(P1s, npairs, 'P1s', TypeError)
    c0 = None if P0s is None else col.listed_cameras(P0s, npairs, 'P0s', TypeError, needed=use)[0]
    packed = np.concatenate([im.reshape(-1) for im in ims]) if ims else np.zeros(0, dtype)
    r0, r1 = NdArray(dtype=dtype), NdArray(dtype=dtype)
    ri0, ri1 = NdArray(dtype='int32'), NdArray(dtype='int32')
    box = np.zeros((npairs, 4), np.int32)
    out_off = np.zeros(npairs + 1, np.int64)
    check(_spv_rectify_batch(packed.ctypes.data, _RECTIFY_BATCH_DTYPE[dtype], sizes.ctypes.data, len(sizes), nchan,
                             float(sampling_factor), pairs.ctypes.data, npairs,
                             c0.ctypes.data if c0 is not None else None, c1.ctypes.data, use.ctypes.data,
                             1 if crop_invalid else 0, ct.byref(r0), ct.byref(r1), ct.byref(ri0), ct.byref(ri1),
                             box.ctypes.data, out_off.ctypes.data))
    r0, r1, ri0, ri1 = (a.asarray().reshape(-1) for a in (r0, r1, ri0, ri1))
    out = []
    for p in range(npairs):
        rows, cols = int(box[p, 1] - box[p, 0]), int(box[p, 3] - box[p, 2])
        if not use[p] or rows * cols == 0:
            out.append(None)
            continue
        lo, hi = int(out_off[p]), int(out_off[p + 1])
        vshape = (rows, cols) if nchan == 1 else (rows, cols, nchan)
        out.append((r0[lo * nchan:hi * nchan].reshape(vshape), r1[lo * nchan:hi * nchan].reshape(vshape),
                    ri0[lo:hi].reshape(rows, cols), ri1[lo:hi].reshape(rows, cols)))
    return out
