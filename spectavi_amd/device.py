"""Device-resident entry points: torch tensors in HBM in, torch tensors out.

Thin binding of section 3 of include/spectavi_amd.h (spv_*_device).  torch is
used only for device memory and the current HIP stream; every kernel launched
here is hand-written HIP inside libspectavi.so and is enqueued on torch's
current stream, so `torch.cuda.Event` timing and stream ordering apply.
"""
import ctypes as ct

import numpy as np
import torch

from spectavi_amd import _collection as col
from spectavi_amd._lib import clib, check


def _stream(dev=None):
    return ct.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


class _on_device_of:
    """All tensors of one call must live on ONE GPU; the call then runs with that GPU as the current
    device and on torch's current stream OF THAT GPU, whatever the process-wide current device is
    (the library launches on the calling thread's current HIP device), and the previous device is
    restored afterwards."""

    def __init__(self, *tensors):
        devs = {t.device for t in tensors if t is not None}
        if len(devs) != 1:
            raise ValueError("all tensors of one call must live on the same GPU, got %s" % sorted(map(str, devs)))
        self.device = devs.pop()
        self._ctx = torch.cuda.device(self.device)

    def __enter__(self):
        self._ctx.__enter__()
        return _stream(self.device)

    def __exit__(self, *exc):
        return self._ctx.__exit__(*exc)


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _need(t, dtype, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise TypeError("%s must be a contiguous %s tensor on the GPU" % (name, dtype))


class Workspace:
    """Grow-only scratch buffer reused across calls (one per device)."""

    def __init__(self):
        self._buf = None

    def get(self, nbytes, device):
        nbytes = max(int(nbytes), 256)
        if self._buf is None or self._buf.numel() < nbytes or self._buf.device != device:
            self._buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self._buf


_default_ws = Workspace()


def l1k2(x, y, workspace=None):
    """Exact L1 2-NN on device: x uint8 [M,D], y uint8 [N,D] (CUDA tensors).
    Returns (idx int64 [N,2] -- the ABI's size_t bits, -1 = no neighbour --,
    dist int32 [N,2]).  Asynchronous on the current stream."""
    _need(x, torch.uint8, "x")
    _need(y, torch.uint8, "y")
    xrows, dim = x.shape
    yrows, ydim = y.shape
    assert dim == ydim
    if dim % 16 != 0:
        raise ValueError("Input matrix inner dimensions must be 16-byte aligned.")
    idx = torch.empty((yrows, 2), dtype=torch.int64, device=y.device)
    dist = torch.empty((yrows, 2), dtype=torch.int32, device=y.device)
    nbytes = clib.spv_l1k2_workspace_bytes(xrows, yrows, dim)
    with _on_device_of(x, y) as stream:
        ws = (workspace or _default_ws).get(nbytes, y.device)
        check(clib.spv_l1k2_device(x.data_ptr(), y.data_ptr(), xrows, yrows, dim, idx.data_ptr(),
                                   dist.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    return idx, dist


def bruteforce(x, y, k=2, p=2.0, workspace=None, slices=0):
    """Exact p-norm k-NN on device (the contract of feature.nn_bruteforce): x [M,D], y [N,D] both
    float32 or both int32 CUDA tensors.  Returns (idx int64 [N,k] -- the ABI's size_t bits, -1 = no
    neighbour --, dist float32 / int32 [N,k]).  `slices` > 0 forces that many database slices (the
    result does not depend on it).  Asynchronous on the current stream."""
    from spectavi_amd.feature import check_bruteforce_args
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.int32):
        raise TypeError("x must be a float32 or int32 tensor")
    _need(x, x.dtype, "x")
    _need(y, x.dtype, "y")
    check_bruteforce_args(tuple(x.shape), tuple(y.shape), k, p)
    if int(slices) < 0:
        raise ValueError("slices must be >= 0")
    k, slices = int(k), int(slices)
    xrows, dim = x.shape
    yrows = y.shape[0]
    idx = torch.empty((yrows, k), dtype=torch.int64, device=y.device)
    dist = torch.empty((yrows, k), dtype=x.dtype, device=y.device)
    nbytes = clib.spv_bruteforce_workspace_bytes(xrows, yrows, dim, k)
    if slices > 0:
        nbytes = max(nbytes, yrows * slices * k * 8)
    with _on_device_of(x, y) as stream:
        ws = (workspace or _default_ws).get(nbytes, y.device)
        check(clib.spv_bruteforce_device(x.data_ptr(), y.data_ptr(), int(x.dtype == torch.int32), xrows, yrows, dim,
                                         k, float(p), slices, idx.data_ptr(), dist.data_ptr(), ws.data_ptr(),
                                         ws.numel(), stream))
    return idx, dist


def ann_l2_plan(xrows, yrows, dim, k=2, ncand=0, slices=0):
    """The launch plan ann_l2() follows for this shape (spv_ann_l2_plan; host only, no device touched):
    dict of kpad (padded row width), qtile, rtile (queries per workgroup, database rows per tile), slices,
    slice_rows, ncand (in force), buflen (keys in the survivor buffer of a query and slice), mfma (32 or 16)."""
    out = (ct.c_int * 8)()
    check(clib.spv_ann_l2_plan(xrows, yrows, dim, k, ncand, slices, out))
    return dict(zip(("kpad", "qtile", "rtile", "slices", "slice_rows", "ncand", "buflen", "mfma"), out))


def ann_l2(x, y, k=2, ncand=0, workspace=None, slices=0):
    """Approximate L2 k-NN on device (the contract of feature.ann_l2): x [M,D], y [N,D] float32 CUDA
    tensors.  Returns (idx int64 [N,k] -- the ABI's size_t bits, -1 = no neighbour --, dist float32 [N,k],
    exact).  `slices` > 0 forces that many database slices (the result does not depend on it).
    Asynchronous on the current stream."""
    from spectavi_amd.feature import check_ann_args
    _need(x, torch.float32, "x")
    _need(y, torch.float32, "y")
    check_ann_args(tuple(x.shape), tuple(y.shape), k, ncand)
    if int(slices) < 0:
        raise ValueError("slices must be >= 0")
    k, ncand, slices = int(k), int(ncand), int(slices)
    xrows, dim = x.shape
    yrows = y.shape[0]
    idx = torch.empty((yrows, k), dtype=torch.int64, device=y.device)
    dist = torch.empty((yrows, k), dtype=torch.float32, device=y.device)
    nbytes = clib.spv_ann_l2_workspace_bytes(xrows, yrows, dim, k, ncand)
    if slices > 0:
        nbytes += yrows * slices * (8 * ann_l2_plan(xrows, yrows, dim, k, ncand)["buflen"] + 4) + 512
    with _on_device_of(x, y) as stream:
        ws = (workspace or _default_ws).get(nbytes, y.device)
        check(clib.spv_ann_l2_device(x.data_ptr(), y.data_ptr(), xrows, yrows, dim, k, ncand, slices, idx.data_ptr(),
                                     dist.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    return idx, dist


def l1k2_set_prune(mode):
    """Whether l1k2() at dim 128 rules pairs out with the matrix-core lower bound first
    (spv_l1k2_set_prune): "auto" (shapes whose database slices are at least 32768 rows long, the default), 1 / True (wherever the path exists),
    0 / False (never).  The results do not depend on it."""
    if isinstance(mode, str):
        mode = {"auto": -1}.get(mode)
    if isinstance(mode, bool):
        mode = int(mode)
    if not isinstance(mode, int) or mode not in (-1, 0, 1):
        raise ValueError("prune mode must be 'auto', 0 or 1")
    check(clib.spv_l1k2_set_prune(mode))


def l1k2_get_prune():
    """The prune mode in force: -1 (auto), 0 or 1."""
    return int(clib.spv_l1k2_get_prune())


def l1k2_set_bound(which):
    """Which table the matrix-core lower bound of l1k2() runs with (spv_l1k2_set_bound): "default" (the tuned
    table where prune mode "auto" takes the path, the recipe under prune mode 1), 0 / "recipe", 1 / "tuned".
    The results do not depend on it."""
    if isinstance(which, str):
        which = {"default": -1, "recipe": 0, "tuned": 1}.get(which)
    if isinstance(which, bool) or not isinstance(which, int) or which not in (-1, 0, 1):
        raise ValueError("bound table must be 'default', 'recipe' (0) or 'tuned' (1)")
    check(clib.spv_l1k2_set_bound(which))


def l1k2_get_bound():
    """The bound table setting in force: -1 (default), 0 (recipe) or 1 (tuned)."""
    return int(clib.spv_l1k2_get_bound())


def l1k2_set_prune_form(form):
    """Which form of the bound kernel l1k2() runs where it takes the bound path (spv_l1k2_set_prune_form): "default"
    (the wide one where prune mode "auto" takes the path and its grid fills the chip, else the narrow one),
    0 / "narrow" (256 queries over 32-row tiles), 1 / "wide" (512 queries over 64-row tiles).
    The results do not depend on it."""
    if isinstance(form, str):
        form = {"default": -1, "narrow": 0, "wide": 1}.get(form)
    if isinstance(form, bool) or not isinstance(form, int) or form not in (-1, 0, 1):
        raise ValueError("bound kernel form must be 'default', 'narrow' (0) or 'wide' (1)")
    check(clib.spv_l1k2_set_prune_form(form))


def l1k2_get_prune_form():
    """The bound kernel form setting in force: -1 (default), 0 (narrow) or 1 (wide)."""
    return int(clib.spv_l1k2_get_prune_form())


def l1k2_prune_form_of(xrows, yrows, dim=128):
    """The form l1k2() would run for this shape under the settings in force (spv_l1k2_prune_form_of; host only):
    0 (narrow), 1 (wide), or -1 where it would not take the bound path."""
    return int(clib.spv_l1k2_prune_form_of(xrows, yrows, dim))


def l1k2_bound_table(which=0):
    """(phi int64 [256, 4], p, m) of the recipe (0) or the tuned (1) table (spv_l1k2_bound_table_of; host only):
    p |a - b| >= m - phi[a] . phi[b] for all bytes a, b."""
    import numpy as np
    phi = np.zeros((256, 4), np.int8)
    p, m = ct.c_int(0), ct.c_int(0)
    check(clib.spv_l1k2_bound_table_of(int(which), phi.ctypes.data, ct.byref(p), ct.byref(m)))
    return phi.astype(np.int64), int(p.value), int(m.value)


def l1k2_set_prune_matrix(matrix):
    """The matrix format of the wide bound kernel (spv_l1k2_set_prune_matrix): "default" (FP6 where prune mode "auto"
    takes the path, the form is wide and no bound table is named, else int8), 0 / "i8", 1 / "fp6" (every shape whose
    form is wide).  The results do not depend on it."""
    if isinstance(matrix, str):
        matrix = {"default": -1, "i8": 0, "fp6": 1}.get(matrix)
    if isinstance(matrix, bool) or not isinstance(matrix, int) or matrix not in (-1, 0, 1):
        raise ValueError("bound matrix format must be 'default', 'i8' (0) or 'fp6' (1)")
    check(clib.spv_l1k2_set_prune_matrix(matrix))


def l1k2_get_prune_matrix():
    """The matrix format setting in force: -1 (default), 0 (int8) or 1 (FP6)."""
    return int(clib.spv_l1k2_get_prune_matrix())


def l1k2_prune_matrix_of(xrows, yrows, dim=128):
    """The matrix format l1k2() would run for this shape under the settings in force (spv_l1k2_prune_matrix_of; host
    only): 0 (int8), 1 (FP6), or -1 where it would not take the bound path."""
    return int(clib.spv_l1k2_prune_matrix_of(xrows, yrows, dim))


def l1k2_bound6_table():
    """(k int64 [256, 5], p, m) of the FP6 table (spv_l1k2_bound6_table; host only): the features are k / 8, and
    p |a - b| >= m - k[a] . k[b] for all bytes a, b, in units of 1/64."""
    import numpy as np
    k = np.zeros((256, 5), np.int8)
    p, m = ct.c_int(0), ct.c_int(0)
    check(clib.spv_l1k2_bound6_table(k.ctypes.data, ct.byref(p), ct.byref(m)))
    return k.astype(np.int64), int(p.value), int(m.value)


def l1k2_prune_stats():
    """(pairs put to the bound, survivors, pairs of the exact fallback) of this thread's last l1k2()
    call; all zero if it ran the tile kernels.  Synchronises with that call."""
    out = (ct.c_ulonglong * 3)()
    check(clib.spv_l1k2_prune_stats(out))
    return int(out[0]), int(out[1]), int(out[2])


def l1k2_plan(xrows, yrows, dim):
    """The launch plan l1k2() follows for this shape (spv_l1k2_plan; host only, no device touched):
    dict of dim_pad (kernel row width), q (queries per lane), slices, slice_rows, wide (bool)."""
    out = (ct.c_int * 5)()
    check(clib.spv_l1k2_plan(xrows, yrows, dim, out))
    return dict(dim_pad=out[0], q=out[1], slices=out[2], slice_rows=out[3], wide=bool(out[4]))


def _plan_items(fn, args, n_out, cols, want_items, at=0, tail=()):
    """The two calls of a plan entry fn(*args, out[n_out], *tail, items, items_cap): out as ints and, with
    want_items, the out[at] items as int32[items, cols] (else None)."""
    out = (ct.c_longlong * n_out)()
    check(fn(*args, out, *tail, None, 0))
    items = None
    if want_items:
        items = np.empty((int(out[at]), cols), np.int32)
        check(fn(*args, out, *tail, items.ctypes.data, len(items)))
    return [int(v) for v in out], items


def _collection_args(seg_off, pairs, total_rows, table, out32=False):
    """seg_off -> int64[nseg + 1], pairs -> int32[npairs, 2], out_off int64[npairs + 1]; ValueError for anything
    check_collection (collection.h; with out32, check_collection_out32) would reject or that does not describe a
    `table` of total_rows rows (None: any)."""
    seg = col.offsets(seg_off, "seg_off", total_rows, table)
    prs = col.pair_table(pairs, seg.size - 1)
    return seg, prs, col.out_offsets(seg, prs, out32)


def _batch_args(seg_off, pairs, total_rows, dim):
    """_collection_args of a matcher's descriptor table, whose rows are dim wide: the arguments of
    spv_l1k2_batch_device."""
    col.check_matcher_dim(dim)
    return _collection_args(seg_off, pairs, total_rows, "desc")


def l1k2_batch_plan(seg_off, pairs, dim, want_items=False):
    """The launch plan l1k2_batch() follows for a collection (spv_l1k2_batch_plan; host only, no device
    touched): dict of dim_pad (kernel row width), q (queries per lane), items (work items = workgroups),
    out_rows, max_slices (largest number of database slices of any pair), workspace_bytes and out_off
    (int64[npairs + 1]: pair p owns out rows [out_off[p], out_off[p + 1])).  With want_items also the work
    items themselves, int32[items, 5] = (pair, first query row within the query set, query rows, first
    database row within the database set, database rows), in launch order."""
    seg, prs, out_off = _batch_args(seg_off, pairs, None, dim)
    out, items = _plan_items(clib.spv_l1k2_batch_plan, (seg.ctypes.data, seg.size - 1, dim, prs.ctypes.data, len(prs)),
                             6, 5, want_items, at=2)
    plan = dict(dim_pad=out[0], q=out[1], items=out[2], out_rows=out[3], max_slices=out[4], workspace_bytes=out[5],
                out_off=out_off)
    return (plan, items) if want_items else plan


def l1k2_batch(desc, seg_off, pairs, workspace=None):
    """Exact L1 2-NN of many descriptor-set pairs on device, one main launch for all of them: desc uint8
    [total_rows, D] (CUDA tensor) holds the sets back to back, set s = rows seg_off[s]:seg_off[s + 1];
    pairs [npairs, 2] = (query set, database set).  Returns (idx int64 [out_rows, 2] -- the ABI's size_t
    bits, -1 = no neighbour; the row number inside the database set --, dist int32 [out_rows, 2], out_off
    int64 ndarray [npairs + 1]): pair p owns rows out_off[p]:out_off[p + 1], each bit for bit
    l1k2(database set, query set).  ratio_test() applies to the concatenated output as it stands: its
    matches are (out row, row within the database set).  Asynchronous on the current stream but for the
    upload of the work table."""
    _need(desc, torch.uint8, "desc")
    if desc.dim() != 2:
        raise ValueError("desc must be [total_rows, dim]")
    total, dim = desc.shape
    seg, prs, out_off = _batch_args(seg_off, pairs, total, dim)
    out_rows = int(out_off[-1])
    idx = torch.empty((out_rows, 2), dtype=torch.int64, device=desc.device)
    dist = torch.empty((out_rows, 2), dtype=torch.int32, device=desc.device)
    nbytes = clib.spv_l1k2_batch_workspace_bytes(seg.ctypes.data, seg.size - 1, dim, prs.ctypes.data, len(prs))
    with _on_device_of(desc) as stream:
        ws = (workspace or _default_ws).get(nbytes, desc.device)
        check(clib.spv_l1k2_batch_device(desc.data_ptr(), seg.ctypes.data, seg.size - 1, dim, prs.ctypes.data, len(prs),
                                         idx.data_ptr(), dist.data_ptr(), ws.data_ptr(), ws.numel(), stream))
    return idx, dist, out_off


def l1k2_guided_batch_plan(seg_off, pairs, dim=128, want_items=False):
    """The launch plan l1k2_guided_batch() follows for a collection (spv_l1k2_guided_batch_plan; host only, no
    device touched): dict of items (work items = workgroups), out_rows, max_slices (largest number of database
    slices of any pair), workspace_bytes and out_off (int64[npairs + 1]).  With want_items also the work items,
    int32[items, 5] = (pair, first query row within the query set, query rows, first database row within the
    database set, database rows), in launch order."""
    seg, prs, out_off = _batch_args(seg_off, pairs, None, dim)
    if dim != 128:
        raise ValueError("the guided L1 2-NN takes dim 128 only (dim=%d)" % dim)
    out, items = _plan_items(clib.spv_l1k2_guided_batch_plan,
                             (seg.ctypes.data, seg.size - 1, dim, prs.ctypes.data, len(prs)), 4, 5, want_items)
    plan = dict(items=out[0], out_rows=out[1], max_slices=out[2], workspace_bytes=out[3], out_off=out_off)
    return (plan, items) if want_items else plan


def _need_geom(geom, total):
    if not isinstance(geom, torch.Tensor) or geom.dim() != 2 or geom.shape[1] != 4 or geom.dtype != torch.float32:
        raise ValueError("geom must be a float32 tensor [total_rows, 4]")
    if total is not None and geom.shape[0] != total:
        raise ValueError("geom has %d rows, desc has %d" % (geom.shape[0], total))
    _need(geom, torch.float32, "geom")


def l1k2_guided_batch(desc, geom, seg_off, pairs, lines, max_dist, workspace=None, want_ncand=False):
    """`l1k2_batch` searched only inside a band around each query's line (spv_l1k2_guided_batch_device): desc uint8
    [total_rows, 128], seg_off and pairs as for `l1k2_batch`; geom float32 [total_rows, 4], row for row the geometry
    of desc (`split_sift_table`), of which columns 0 and 1 (u, v) are read; lines float64 [out_rows, 3], row r the
    line (l0, l1, l2) of out row r in the database view's pixels (`epipolar_lines_batch`, or (0, 1, -v) for a
    rectified pair).  Database row j is a candidate of out row r iff |fma(l0, u_j, fma(l1, v_j, l2))| <= max_dist in
    float64 (pixels, for unit-normal lines); a NaN line or keypoint has no candidates.  Returns (idx int64 [out_rows,
    2], dist int32 [out_rows, 2][, ncand int32 [out_rows]], out_off): the two nearest candidates by (dist, row),
    -1 / INT_MAX where fewer than two exist, and with want_ncand the number of candidates.  Asynchronous on the
    current stream but for the upload of the work table."""
    _need(desc, torch.uint8, "desc")
    if desc.dim() != 2:
        raise ValueError("desc must be [total_rows, dim]")
    total, dim = desc.shape
    seg, prs, out_off = _batch_args(seg_off, pairs, total, dim)
    if dim != 128:
        raise ValueError("the guided L1 2-NN takes dim 128 only (dim=%d)" % dim)
    _need_geom(geom, total)
    out_rows = int(out_off[-1])
    if not isinstance(lines, torch.Tensor) or lines.dtype != torch.float64 or tuple(lines.shape) != (out_rows, 3):
        raise ValueError("lines must be a float64 tensor [out_rows, 3] = [%d, 3]" % out_rows)
    _need(lines, torch.float64, "lines")
    idx = torch.empty((out_rows, 2), dtype=torch.int64, device=desc.device)
    dist = torch.empty((out_rows, 2), dtype=torch.int32, device=desc.device)
    ncand = torch.empty((out_rows,), dtype=torch.int32, device=desc.device) if want_ncand else None
    nbytes = clib.spv_l1k2_guided_batch_workspace_bytes(seg.ctypes.data, seg.size - 1, dim, prs.ctypes.data, len(prs))
    with _on_device_of(desc, geom, lines) as stream:
        ws = (workspace or _default_ws).get(nbytes, desc.device)
        check(clib.spv_l1k2_guided_batch_device(
            desc.data_ptr(), geom.data_ptr(), seg.ctypes.data, seg.size - 1, dim, prs.ctypes.data, len(prs),
            lines.data_ptr(), float(max_dist), idx.data_ptr(), dist.data_ptr(),
            ncand.data_ptr() if want_ncand else None, ws.data_ptr(), ws.numel(), stream))
    return (idx, dist, ncand, out_off) if want_ncand else (idx, dist, out_off)


def epipolar_lines_batch(geom, seg_off, pairs, G, use=None):
    """The lines `l1k2_guided_batch` takes, from one 3x3 matrix per pair (spv_epipolar_lines_batch_device): geom
    float32 [total_rows, 4], seg_off and pairs as for `l1k2_batch`; G [npairs, 3, 3] (or [npairs, 9]) host float64,
    G[p] mapping a pixel of the query view to its line in the database view; use [npairs] or None.  Out row r of
    pair p, query keypoint (u, v), gets G[p] (u, v, 1)^T / hypot(l0, l1); three NaNs where use[p] is 0 or the norm
    is zero or not finite.  Returns lines, CUDA float64 [out_rows, 3].  Asynchronous on the current stream.

    The convention of `ransac_fit_batch`: its 'essential' E is the seven-point solution with x1^T E x0 = 0
    (`mvg.seven_point_algorithm`: xp^T F x = 0), x0 from the database set and x1 from the query set as
    `match_coordinates_batch` returns them.  A query point's line in the database view is therefore E^T x1, and for
    pixel coordinates with calibration K, G = (K^-T E K^-1)^T."""
    _need_geom(geom, None)
    seg, prs, out_off = _collection_args(seg_off, pairs, geom.shape[0], "geom")
    G = np.ascontiguousarray(G, dtype=np.float64).reshape(-1, 9) if np.size(G) else np.zeros((0, 9))
    if len(G) != len(prs):
        raise ValueError("G must hold one 3x3 matrix per pair (%d), got %d" % (len(prs), len(G)))
    use = col.use_flags(use, len(prs), "pair")
    lines = torch.empty((int(out_off[-1]), 3), dtype=torch.float64, device=geom.device)
    with _on_device_of(geom) as stream:
        check(clib.spv_epipolar_lines_batch_device(geom.data_ptr(), seg.ctypes.data, seg.size - 1, prs.ctypes.data,
                                                   len(prs), G.ctypes.data, _ptr(use), lines.data_ptr(), stream))
    return lines


def cascade_plan(xrows, yrows, dim, m, n, g):
    """The launch plan cascade() follows for this shape under the SPECTAVI_CASCADE_* environment of the
    moment (spv_cascade_plan; host only, no device touched): dict of family, pa, pb, gmax_q, probe_kind,
    cpl, ru, wpe, shift, full, sorted, qhist_fused as the header lists them, and the instantiations
    project_db, project_query and probe spelled as tools/kernel_coverage.py --list prints them."""
    out = (ct.c_int * 12)()
    check(clib.spv_cascade_plan(xrows, yrows, dim, m, n, g, out))
    p = dict(zip(("family", "pa", "pb", "gmax_q", "probe_kind", "cpl", "ru", "wpe"), out[:8]))
    p.update(zip(("shift", "full", "sorted", "qhist_fused"), map(bool, out[8:])))
    tf = ("false", "true")
    name = ("project_kernel", "project_mfma_kernel", "project_mfma4_kernel")[p["family"]]
    for key, query, gmax in (("project_db", 0, 1), ("project_query", 1, p["gmax_q"])):
        # project_mfma_kernel<CT, IS_QUERY, GMAX, FULL>; the other two <.., .., IS_QUERY, GMAX>
        args = (p["pa"], tf[query], gmax, tf[p["pb"]]) if p["family"] == 1 else (p["pa"], p["pb"], tf[query], gmax)
        p[key] = "%s<%s>" % (name, ", ".join(map(str, args)))
    p["probe"] = ("probe_table_kernel<%d, %d, %d, %s, %s>" % (p["cpl"], p["ru"], p["wpe"], tf[p["shift"]], tf[p["full"]])
                  if p["probe_kind"] else "probe_refine_kernel<%d, %d>" % (p["cpl"], p["ru"]))
    return p


def shard_bounds(total, shards):
    """[lo_0, lo_1, ..., total]: the contiguous balanced shards the library itself uses."""
    return [int(clib.spv_shard_lo(int(total), int(shards), r)) for r in range(int(shards) + 1)]


def l1k2_gathered(xs, ys, transport="rccl"):
    """The sharded query loop inside ONE process (reference loop
    src/BruteForceNnL1K2.h:92-93): xs[r] = replica of the database on GPU r, ys[r] = query shard r
    (contiguous balanced shards, `shard_bounds`), one tensor per listed GPU.  Every GPU matches its
    shard; the 16-byte (idx0, idx1, d0, d1) records are gathered on ys[0]'s GPU by ncclGather on the
    library's ncclCommInitAll clique ("rccl") or by peer copies ("copy") and widened there.
    Returns (idx int64 [N,2], dist int32 [N,2]) on that GPU.  Synchronous."""
    if len(xs) != len(ys) or not xs:
        raise ValueError("one database replica and one query shard per GPU")
    G = len(xs)
    for x, y in zip(xs, ys):
        _need(x, torch.uint8, "x")
        _need(y, torch.uint8, "y")
        if x.device != y.device:
            raise ValueError("replica and shard of one rank must share a GPU")
    xrows, dim = xs[0].shape
    if any(tuple(x.shape) != (xrows, dim) for x in xs) or any(y.shape[1] != dim for y in ys):
        raise ValueError("database replicas must be identical in shape; all rows %d wide" % dim)
    total = sum(int(y.shape[0]) for y in ys)
    if [int(y.shape[0]) for y in ys] != [b - a for a, b in zip(shard_bounds(total, G)[:-1], shard_bounds(total, G)[1:])]:
        raise ValueError("query shards must be the contiguous balanced split of the %d queries" % total)
    root = ys[0].device
    idx = torch.empty((total, 2), dtype=torch.int64, device=root)
    dist = torch.empty((total, 2), dtype=torch.int32, device=root)
    devs = (ct.c_int * G)(*[y.device.index for y in ys])
    px = (ct.c_void_p * G)(*[x.data_ptr() for x in xs])
    py = (ct.c_void_p * G)(*[y.data_ptr() for y in ys])
    for y in ys:
        torch.cuda.synchronize(y.device)  # the library runs on streams of its own
    mode = {"rccl": 1, "copy": 2}[transport]
    check(clib.spv_l1k2_gathered_device(G, devs, px, py, xrows, total, dim, idx.data_ptr(), dist.data_ptr(), mode))
    return idx, dist


def _gather_lists(G, per_rank, total):
    if [int(t.shape[0]) for t in per_rank] != [b - a for a, b in zip(shard_bounds(total, G)[:-1], shard_bounds(total, G)[1:])]:
        raise ValueError("the per-GPU shards must be the contiguous balanced split of the %d rows" % total)
    for t in per_rank:
        torch.cuda.synchronize(t.device)  # the library runs on streams of its own


def cascade_gathered(xs, ys, dicts, g=2, transport="rccl", want_ncand=False):
    """nn_cascading_hash sharded inside ONE process with everything resident: per GPU a
    replica of the database xs[r] and of the hyperplanes dicts[r] (float32 [n,D,m]) and the query shard
    ys[r]; results gathered (16-byte records, ncand as int32) and widened on ys[0]'s GPU."""
    G = len(xs)
    if not (G == len(ys) == len(dicts)) or not xs:
        raise ValueError("one database replica, one dictionary replica and one query shard per GPU")
    for x, y, d in zip(xs, ys, dicts):
        _need(x, torch.float32, "x")
        _need(y, torch.float32, "y")
        _need(d, torch.float32, "hash_dict")
        if not (x.device == y.device == d.device):
            raise ValueError("the tensors of one rank must share a GPU")
    xrows, dim = xs[0].shape
    n, ddim, m = dicts[0].shape
    total = sum(int(y.shape[0]) for y in ys)
    _gather_lists(G, ys, total)
    root = ys[0].device
    idx = torch.empty((total, 2), dtype=torch.int64, device=root)
    dist = torch.empty((total, 2), dtype=torch.float32, device=root)
    ncand = torch.empty((total,), dtype=torch.int32, device=root) if want_ncand else None
    devs = (ct.c_int * G)(*[y.device.index for y in ys])
    vp = ct.c_void_p * G
    check(clib.spv_cascade_gathered_device(G, devs, vp(*[x.data_ptr() for x in xs]), vp(*[y.data_ptr() for y in ys]), xrows,
                                           total, dim, m, n, g, vp(*[d.data_ptr() for d in dicts]), idx.data_ptr(),
                                           dist.data_ptr(), ncand.data_ptr() if want_ncand else None,
                                           {"rccl": 1, "copy": 2}[transport]))
    return (idx, dist, ncand) if want_ncand else (idx, dist)


def dlt_gathered(P0, P1, xs, xps, want_error=False, transport="rccl"):
    """dlt_triangulate / dlt_reprojection_error sharded inside ONE process with the point shards
    resident (xs[r], xps[r] float64 [cnt_r,3] on GPU r); rows gathered on xs[0]'s GPU."""
    G = len(xs)
    if G != len(xps) or not xs:
        raise ValueError("one shard of each view per GPU")
    for x, xp in zip(xs, xps):
        _need(x, torch.float64, "x")
        _need(xp, torch.float64, "xp")
        if x.device != xp.device or x.shape != xp.shape:
            raise ValueError("the two views of one rank must share a GPU and a shape")
    total = sum(int(x.shape[0]) for x in xs)
    _gather_lists(G, xs, total)
    out = torch.empty((total, 1 if want_error else 4), dtype=torch.float64, device=xs[0].device)
    devs = (ct.c_int * G)(*[x.device.index for x in xs])
    vp = ct.c_void_p * G
    check(clib.spv_dlt_gathered_device(G, devs, np.ascontiguousarray(P0, np.float64), np.ascontiguousarray(P1, np.float64), total,
                                       vp(*[x.data_ptr() for x in xs]), vp(*[xp.data_ptr() for xp in xps]), out.data_ptr(),
                                       int(bool(want_error)), {"rccl": 1, "copy": 2}[transport]))
    return out


def cascade(x, y, hash_dict, g=2, workspace=None, want_ncand=False):
    """Cascade-hash 2-NN on device: x,y float32 [rows,D]; hash_dict float32 [n,D,m]."""
    _need(x, torch.float32, "x")
    _need(y, torch.float32, "y")
    _need(hash_dict, torch.float32, "hash_dict")
    xrows, dim = x.shape
    yrows, ydim = y.shape
    n, ddim, m = hash_dict.shape
    assert dim == ydim == ddim
    idx = torch.empty((yrows, 2), dtype=torch.int64, device=y.device)
    dist = torch.empty((yrows, 2), dtype=torch.float32, device=y.device)
    ncand = torch.empty((yrows,), dtype=torch.int32, device=y.device) if want_ncand else None
    nbytes = clib.spv_cascade_workspace_bytes(xrows, yrows, dim, m, n, g)
    with _on_device_of(x, y, hash_dict) as stream:
        ws = (workspace or _default_ws).get(nbytes, y.device)
        check(clib.spv_cascade_device(x.data_ptr(), y.data_ptr(), xrows, yrows, dim, m, n, g,
                                      hash_dict.data_ptr(), idx.data_ptr(), dist.data_ptr(),
                                      ncand.data_ptr() if want_ncand else None, ws.data_ptr(),
                                      ws.numel(), stream))
    return (idx, dist, ncand) if want_ncand else (idx, dist)


def _cascade_batch_args(seg_off, pairs, total_rows, dim, m, n, g):
    """_batch_args plus the cascade's own limits, as ValueError before any device work."""
    seg, prs, out_off = _batch_args(seg_off, pairs, total_rows, dim)
    if not 1 <= m <= 31:
        raise ValueError("hash bit rate m must be in [1, 31]")
    if n < 1 or not 0 <= g <= min(m, 16):
        raise ValueError("need n >= 1 and 0 <= g <= min(m, 16)")
    if (seg.size - 1) * n > 65535:
        raise ValueError("the many-pairs cascade takes nseg * n <= 65535 (%d sets, %d tables)" % (seg.size - 1, n))
    return seg, prs, out_off


def cascade_batch_plan(seg_off, pairs, dim, m, n, g, want_items=False):
    """The launch plan cascade_batch() follows for a collection (spv_cascade_batch_plan; host only, no device
    touched): dict of items (work items = workgroups of the probe), out_rows, hb (bucket bits of every (set,
    table)), workspace_bytes and out_off (int64[npairs + 1]: pair p owns out rows [out_off[p], out_off[p + 1])).
    With want_items also the work items themselves, int32[items, 3] = (pair, first query row within the query
    set, query rows), in launch order."""
    seg, prs, out_off = _cascade_batch_args(seg_off, pairs, None, dim, m, n, g)
    out, items = _plan_items(clib.spv_cascade_batch_plan,
                             (seg.ctypes.data, seg.size - 1, dim, m, n, g, prs.ctypes.data, len(prs)), 4, 3, want_items)
    plan = dict(items=out[0], out_rows=out[1], hb=out[2], workspace_bytes=out[3], out_off=out_off)
    return (plan, items) if want_items else plan


def cascade_batch(rows, seg_off, pairs, hash_dict, g=2, workspace=None, want_ncand=False):
    """Cascade-hash 2-NN of many set pairs on device, in a chain of launches whose length depends neither on the
    number of pairs nor on the number of sets: rows float32 [total_rows, D] (CUDA tensor) holds the sets back to
    back, set s = rows seg_off[s]:seg_off[s + 1]; pairs [npairs, 2] = (query set, database set); hash_dict
    float32 [n, D, m], one for the collection.  Every row is projected, coded and bucket-sorted once.  Returns
    (idx int64 [out_rows, 2] -- the ABI's size_t bits, -1 = no neighbour; the row number inside the database
    set --, dist float32 [out_rows, 2], out_off int64 ndarray [npairs + 1][, ncand int32 [out_rows]]): pair p owns
    rows out_off[p]:out_off[p + 1], each bit for bit cascade(database set, query set, hash_dict, g).
    ratio_test() applies to the concatenated output as it stands.  Asynchronous on the current stream but for
    the upload of the small tables."""
    _need(rows, torch.float32, "rows")
    _need(hash_dict, torch.float32, "hash_dict")
    if rows.dim() != 2 or hash_dict.dim() != 3:
        raise ValueError("rows must be [total_rows, dim], hash_dict [n, dim, m]")
    total, dim = rows.shape
    n, ddim, m = hash_dict.shape
    if ddim != dim:
        raise ValueError("hash_dict is %d wide, rows %d" % (ddim, dim))
    seg, prs, out_off = _cascade_batch_args(seg_off, pairs, total, dim, m, n, g)
    out_rows = int(out_off[-1])
    idx = torch.empty((out_rows, 2), dtype=torch.int64, device=rows.device)
    dist = torch.empty((out_rows, 2), dtype=torch.float32, device=rows.device)
    ncand = torch.empty((out_rows,), dtype=torch.int32, device=rows.device) if want_ncand else None
    nbytes = clib.spv_cascade_batch_workspace_bytes(seg.ctypes.data, seg.size - 1, dim, m, n, g, prs.ctypes.data,
                                                    len(prs))
    with _on_device_of(rows, hash_dict) as stream:
        ws = (workspace or _default_ws).get(nbytes, rows.device)
        check(clib.spv_cascade_batch_device(rows.data_ptr(), seg.ctypes.data, seg.size - 1, dim, m, n, g,
                                            prs.ctypes.data, len(prs), hash_dict.data_ptr(), idx.data_ptr(),
                                            dist.data_ptr(), ncand.data_ptr() if want_ncand else None, ws.data_ptr(),
                                            ws.numel(), stream))
    return (idx, dist, out_off, ncand) if want_ncand else (idx, dist, out_off)


def _dlt(fn, P0, P1, x, xp, cols):
    _need(x, torch.float64, "x")
    _need(xp, torch.float64, "xp")
    assert x.shape == xp.shape and x.shape[1] == 3
    P0 = np.ascontiguousarray(P0, dtype=np.float64)
    P1 = np.ascontiguousarray(P1, dtype=np.float64)
    assert P0.shape == (3, 4) and P1.shape == (3, 4)
    npt = x.shape[0]
    dst = torch.empty((npt, cols), dtype=torch.float64, device=x.device)
    with _on_device_of(x, xp) as stream:
        check(fn(P0, P1, npt, x.data_ptr(), xp.data_ptr(), dst.data_ptr(), stream))
    return dst


def dlt_triangulate(P0, P1, x, xp):
    """P0,P1 host float64 [3,4]; x,xp CUDA float64 [npt,3] -> CUDA float64 [npt,4]."""
    return _dlt(clib.spv_dlt_triangulate_device, P0, P1, x, xp, 4)


def dlt_reprojection_error(P0, P1, x, xp):
    return _dlt(clib.spv_dlt_reprojection_error_device, P0, P1, x, xp, 1)


def ratio_test(idx, dist, min_ratio, workspace=None):
    """Ratio test + ordered compaction on device.  idx int64 [N,2], dist int32/float32 [N,2]
    (outputs of l1k2 / cascade).  Returns (matches int32 [N,2] capacity, count int32 [1]);
    rows [0, count) are (query row, database row).  Asynchronous."""
    _need(idx, torch.int64, "idx")
    if dist.dtype == torch.float32:
        is_float = 1
    else:
        _need(dist, torch.int32, "dist")
        is_float = 0
    n = idx.shape[0]
    matches = torch.empty((n, 2), dtype=torch.int32, device=idx.device)
    count = torch.zeros((1,), dtype=torch.int32, device=idx.device)
    with _on_device_of(idx, dist) as stream:
        ws = (workspace or _default_ws).get(clib.spv_ratio_test_workspace_bytes(n), idx.device)
        check(clib.spv_ratio_test_device(idx.data_ptr(), dist.data_ptr(), is_float, n, float(min_ratio),
                                         matches.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                         stream))
    return matches, count


def dlt_score_hypotheses(P0, P1s, x, xp, max_error, want_mask=False, workspace=None):
    """RANSAC scoring on device: P0 host [3,4]; P1s CUDA float64 [H,3,4]; x,xp CUDA [npt,3].
    Returns counts int32 [H] (and mask uint8 [H,npt])."""
    _need(P1s, torch.float64, "P1s")
    _need(x, torch.float64, "x")
    _need(xp, torch.float64, "xp")
    P0 = np.ascontiguousarray(P0, dtype=np.float64)
    nh, npt = P1s.shape[0], x.shape[0]
    counts = torch.empty((nh,), dtype=torch.int32, device=x.device)
    mask = torch.empty((nh, npt), dtype=torch.uint8, device=x.device) if want_mask else None
    with _on_device_of(P1s, x, xp) as stream:
        ws = (workspace or _default_ws).get(clib.spv_dlt_score_workspace_bytes(nh, npt), x.device)
        check(clib.spv_dlt_score_hypotheses_device_ws(P0, P1s.data_ptr(), nh, npt, x.data_ptr(), xp.data_ptr(),
                                                      float(max_error), counts.data_ptr(),
                                                      mask.data_ptr() if want_mask else None, ws.data_ptr(),
                                                      ws.numel(), stream))
    return (counts, mask) if want_mask else counts


def split_sift_table(table):
    """CUDA float32 [n,132] -> (geom float32 [n,4], desc uint8 [n,128])."""
    _need(table, torch.float32, "table")
    assert table.shape[1] == 132
    n = table.shape[0]
    geom = torch.empty((n, 4), dtype=torch.float32, device=table.device)
    desc = torch.empty((n, 128), dtype=torch.uint8, device=table.device)
    with _on_device_of(table) as stream:
        check(clib.spv_sift_split_device(table.data_ptr(), n, geom.data_ptr(), desc.data_ptr(), stream))
    return geom, desc


def match_coordinates(geom_x, geom_y, matches, count):
    """Homogeneous float64 coordinates of matched keypoints: (x0 [cap,3] from geom_x[database row],
    x1 [cap,3] from geom_y[query row]); rows [0, count) are valid."""
    _need(geom_x, torch.float32, "geom_x")
    _need(geom_y, torch.float32, "geom_y")
    _need(matches, torch.int32, "matches")
    cap = matches.shape[0]
    x0 = torch.zeros((cap, 3), dtype=torch.float64, device=matches.device)
    x1 = torch.zeros((cap, 3), dtype=torch.float64, device=matches.device)
    with _on_device_of(geom_x, geom_y, matches, count) as stream:
        check(clib.spv_gather_match_coords_device(geom_x.data_ptr(), geom_y.data_ptr(), matches.data_ptr(),
                                                  count.data_ptr(), cap, x0.data_ptr(), x1.data_ptr(), stream))
    return x0, x1


def profile_enable(on=True):
    """Bracket the hot kernels with HIP events on their launch stream."""
    clib.spv_profile_enable(1 if on else 0)


def profile_reset():
    clib.spv_profile_reset()


def profile_read(name):
    """(launch count, total milliseconds) of the named kernel since the last reset.
    Synchronises with the recorded events."""
    n = ct.c_longlong(0)
    ms = ct.c_double(0.0)
    check(clib.spv_profile_read(name.encode(), ct.byref(n), ct.byref(ms)))
    return int(n.value), float(ms.value)


def ransac_process_candidates(Fs, x0, x1, singular_value_ratio_allowed=3e-2, required_percent_inliers=.9,
                              reprojection_error_allowed=.5, find_best_even_in_failure=True, want_mask=False,
                              workspace=None):
    """RANSAC candidate processing on device (reference src/RansacFitter.h:42-95 for a batch of
    candidates): Fs CUDA float64 [nF,3,3] (nF <= 16383), x0, x1 CUDA float64 [npt,3].  Returns a dict of
    CUDA tensors: success int32 [nF], inlier_count int32 [nF], best_camera int32 [nF], camera float64
    [nF,3,4], singular_value_ratio float64 [nF], essential float64 [nF,3,3], counts4 int32 [nF,4] and,
    with want_mask, inlier_mask uint8 [nF,npt].  Asynchronous on the current stream."""
    _need(Fs, torch.float64, "Fs")
    _need(x0, torch.float64, "x0")
    _need(x1, torch.float64, "x1")
    nF, npt = Fs.shape[0], x0.shape[0]
    assert Fs.shape[1:] == (3, 3) and x0.shape == x1.shape and x0.shape[1] == 3
    dev = x0.device
    out = {"success": torch.empty(nF, dtype=torch.int32, device=dev),
           "inlier_count": torch.empty(nF, dtype=torch.int32, device=dev),
           "best_camera": torch.empty(nF, dtype=torch.int32, device=dev),
           "camera": torch.empty((nF, 3, 4), dtype=torch.float64, device=dev),
           "singular_value_ratio": torch.empty(nF, dtype=torch.float64, device=dev),
           "essential": torch.empty((nF, 3, 3), dtype=torch.float64, device=dev),
           "counts4": torch.empty((nF, 4), dtype=torch.int32, device=dev)}
    mask = torch.empty((nF, npt), dtype=torch.uint8, device=dev) if want_mask else None
    with _on_device_of(Fs, x0, x1) as stream:
        ws = (workspace or _default_ws).get(clib.spv_ransac_workspace_bytes(nF, npt, 1 if want_mask else 0), dev)
        check(clib.spv_ransac_process_candidates_device(
            Fs.data_ptr(), nF, npt, x0.data_ptr(), x1.data_ptr(), float(singular_value_ratio_allowed),
            float(required_percent_inliers), float(reprojection_error_allowed), int(bool(find_best_even_in_failure)),
            out["success"].data_ptr(), out["inlier_count"].data_ptr(), out["best_camera"].data_ptr(),
            out["camera"].data_ptr(), out["singular_value_ratio"].data_ptr(), out["essential"].data_ptr(),
            out["counts4"].data_ptr(), mask.data_ptr() if want_mask else None, ws.data_ptr(), ws.numel(), stream))
    if want_mask:
        out["inlier_mask"] = mask
    return out


def ransac_fit(x0, x1, required_percent_inliers=.9, reprojection_error_allowed=.5, maximum_tries=500,
               find_best_even_in_failure=True, singular_value_ratio_allowed=3e-2, seed=0, samples=None):
    """`mvg.ransac_fit` with the correspondences resident in HBM (reference RansacFitter::fit_essential,
    src/RansacFitter.h:152-272): x0, x1 CUDA float64 [npt,3] (e.g. the output of `match_coordinates` after
    calibration).  The small results come back as numpy: the `mvg.ransac_fit` dict.  Synchronises the
    current stream once per batch of tries."""
    _need(x0, torch.float64, "x0")
    _need(x1, torch.float64, "x1")
    assert x0.shape == x1.shape and x0.dim() == 2 and x0.shape[1] == 3
    npt = x0.shape[0]
    if npt < 10:
        raise ValueError('Supplied less than 10 point matches, unsupported.')
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        if not (samples.ndim == 2 and samples.shape[1] == 7):
            raise TypeError('samples must be [ntries,7].')
        maximum_tries = samples.shape[0]
    ok, n, bt, br, ran = ct.c_int32(0), ct.c_int32(0), ct.c_int32(-1), ct.c_int32(-1), ct.c_int32(0)
    pct = ct.c_double(0.0)
    F, P, idx = np.zeros(9), np.zeros(12), np.zeros(npt, np.int32)
    with _on_device_of(x0, x1) as stream:
        check(clib.spv_ransac_fit_device(
            x0.data_ptr(), x1.data_ptr(), npt, float(required_percent_inliers), float(reprojection_error_allowed),
            int(maximum_tries), int(bool(find_best_even_in_failure)), float(singular_value_ratio_allowed), int(seed),
            samples.ctypes.data if samples is not None else None, ct.byref(ok), F, P, ct.byref(pct), idx, ct.byref(n),
            ct.byref(bt), ct.byref(br), ct.byref(ran), stream))
    found = bt.value >= 0
    return {'success': bool(ok.value), 'essential': F.reshape(3, 3) if found else None,
            'camera': P.reshape(3, 4) if found else None, 'inlier_percent': float(pct.value),
            'inlier_idx': idx[:n.value].copy(), 'best_try': bt.value, 'best_root': br.value, 'tries_run': ran.value}


def _fit_batch_args(pair_off, total, maximum_tries, seeds, samples):
    """pair_off -> int64[npairs + 1], samples -> int32[npairs, T, 7] or None, seeds -> uint64[npairs] or None,
    maximum_tries; ValueError for anything spv_ransac_fit_batch_device would reject or that does not describe
    arrays of `total` rows.  Touches no device."""
    off = col.offsets(pair_off, "pair_off", total, "x0")
    npairs = off.size - 1
    col.check_set_count(npairs)
    samples = col.sample_table(samples, np.diff(off), 7, 10)
    seeds, maximum_tries = col.seeds_and_tries(seeds, samples, maximum_tries, npairs)
    return off, samples, seeds, maximum_tries


_fit_batch_dicts = col.fit_dicts   # the name tests/test_ransac_batch_rounds_gpu.py builds its rows with


def ransac_fit_batch_plan(pair_off, maximum_tries=500, compute_units=256, want_items=False):
    """The first round of ransac_fit_batch() for a collection (spv_ransac_fit_batch_plan; host only, no device
    touched): dict of sets and tries in the round, items (work items = workgroups of the scorer) and row_blocks
    (blocks of 256 rows).  With want_items also the items, int32[items, 5] = (set, first row, rows, first
    candidate of the round, candidates)."""
    off = col.offsets_unchecked(pair_off, "pair_off")
    out, items = _plan_items(clib.spv_ransac_fit_batch_plan,
                             (off.ctypes.data, off.size - 1, int(maximum_tries), int(compute_units)), 4, 5, want_items, at=2)
    plan = dict(sets=out[0], tries=out[1], items=out[2], row_blocks=out[3])
    return (plan, items) if want_items else plan


def ransac_fit_batch(x0, x1, pair_off, required_percent_inliers=.9, reprojection_error_allowed=.5, maximum_tries=500,
                     find_best_even_in_failure=True, singular_value_ratio_allowed=3e-2, seeds=None, samples=None,
                     want_mask=False):
    """`ransac_fit` for every set of a collection in one call (spv_ransac_fit_batch_device): x0, x1 CUDA float64
    [total,3] hold the sets back to back, set p = rows pair_off[p]:pair_off[p + 1] (e.g. the output of
    `match_coordinates_batch`).  samples int32 [npairs, ntries, 7] (row numbers inside the set; `maximum_tries` and
    `seeds` are then ignored) or seeds [npairs] (0 = SPECTAVI_RANSAC_SEED / random) choose the subsets.  Returns a
    list of `ransac_fit` dicts, each bit for bit the single call's but for tries_run; a set of fewer than 10 rows
    is skipped (success False, no model, tries_run 0).  With want_mask also a CUDA uint8 [total] tensor: 1 = inlier
    of its set's kept model.  Synchronises the current stream once per round of tries, however many sets."""
    if not (x0.shape == x1.shape and x0.dim() == 2 and x0.shape[1] == 3):
        raise ValueError("x0, x1 must be [total,3]")
    total = x0.shape[0]
    off, samples, seeds, maximum_tries = _fit_batch_args(pair_off, total, maximum_tries, seeds, samples)
    _need(x0, torch.float64, "x0")
    _need(x1, torch.float64, "x1")
    npairs = off.size - 1
    ok, n, bt, br, ran = (np.zeros(npairs, np.int32) for _ in range(5))
    pct, F, P, idx = np.zeros(npairs), np.zeros((npairs, 9)), np.zeros((npairs, 12)), np.zeros(total, np.int32)
    mask = torch.empty(total, dtype=torch.uint8, device=x0.device) if want_mask else None
    with _on_device_of(x0, x1) as stream:
        check(clib.spv_ransac_fit_batch_device(
            x0.data_ptr(), x1.data_ptr(), off.ctypes.data, npairs, float(required_percent_inliers),
            float(reprojection_error_allowed), maximum_tries, int(bool(find_best_even_in_failure)),
            float(singular_value_ratio_allowed), _ptr(samples), seeds.ctypes.data if samples is None else None,
            ok.ctypes.data, F.ctypes.data, P.ctypes.data, pct.ctypes.data, idx.ctypes.data, n.ctypes.data,
            bt.ctypes.data, br.ctypes.data, ran.ctypes.data, mask.data_ptr() if want_mask else None, stream))
    fits = col.fit_dicts(off, ok, F, P, pct, idx, n, bt, br, ran)
    return (fits, mask) if want_mask else fits


def _dlt_batch_args(pair_off, total, P1s, P0s, use):
    """pair_off -> int64[npairs + 1], P1s / P0s -> float64[npairs, 12] (P0s or None), use -> int32[npairs] or None;
    ValueError for anything spv_dlt_triangulate_batch_device would reject or that does not describe arrays of `total`
    rows.  A None entry of a P1s list is a skipped set.  Touches no device."""
    off = col.offsets(pair_off, "pair_off", total, "x0")
    npairs = off.size - 1
    col.check_set_count(npairs)
    P1s, use = col.none_cameras_skip(P1s, npairs, "P1s", col.use_flags(use, npairs))
    return off, col.packed_cameras(P1s, npairs, "P1s"), None if P0s is None else col.packed_cameras(P0s, npairs, "P0s"), use


def dlt_triangulate_batch_plan(pair_off, use=None, compute_units=256, want_items=False):
    """The work items dlt_triangulate_batch() launches for a collection (spv_dlt_triangulate_batch_plan; host only,
    no device touched): dict of sets (used sets), items (workgroup steps) and bound (rows of the used sets).  With
    want_items also the items, int32[items, 4] = (set, first row, rows, out row of the first row without a mask)."""
    off = col.offsets_unchecked(pair_off, "pair_off")
    use = col.use_flags(use, off.size - 1)
    out, items = _plan_items(clib.spv_dlt_triangulate_batch_plan, (off.ctypes.data, off.size - 1, _ptr(use), int(compute_units)),
                             3, 4, want_items, at=1)
    plan = dict(sets=out[0], items=out[1], bound=out[2])
    return (plan, items) if want_items else plan


def dlt_triangulate_batch(x0, x1, pair_off, P1s, P0s=None, use=None, mask=None, want_error=False, want_rows=False):
    """`dlt_triangulate` (and `dlt_reprojection_error`) for every set of a collection in one call
    (spv_dlt_triangulate_batch_device): x0, x1 CUDA float64 [total,3] hold the sets back to back, set p = rows
    pair_off[p]:pair_off[p + 1], solved with the cameras P0s[p] (None: [I|0] for every set) and P1s[p] (host [3,4]
    arrays); a set with use[p] == 0 (or a None entry of a P1s list) is skipped.  mask: CUDA uint8 [total], e.g. what
    `ransac_fit_batch(want_mask=True)` returns; only rows with a non-zero byte are solved.  Returns X CUDA float64
    [total,4] -- plus err float64 [total] with want_error, rows int32 [total] (row numbers inside the set) with
    want_rows -- and out_off, an int64 ndarray [npairs + 1]: set p's results are out rows out_off[p]:out_off[p + 1],
    in input order, each bit for bit the single call's; rows from out_off[-1] on are not written.  Asynchronous but
    for the upload of the cameras; reading out_off back synchronises the current stream only when a mask is given
    (without one the host computes it)."""
    if not (x0.shape == x1.shape and x0.dim() == 2 and x0.shape[1] == 3):
        raise ValueError("x0, x1 must be [total,3]")
    total = x0.shape[0]
    off, P1s, P0s, use = _dlt_batch_args(pair_off, total, P1s, P0s, use)
    _need(x0, torch.float64, "x0")
    _need(x1, torch.float64, "x1")
    if mask is not None:
        _need(mask, torch.uint8, "mask")
        if mask.shape != (total,):
            raise ValueError("mask must be [total]")
    npairs = off.size - 1
    X = torch.empty((total, 4), dtype=torch.float64, device=x0.device)
    err = torch.empty(total, dtype=torch.float64, device=x0.device) if want_error else None
    rows = torch.empty(total, dtype=torch.int32, device=x0.device) if want_rows else None
    d_off = torch.empty(npairs + 1, dtype=torch.int64, device=x0.device) if mask is not None else None
    with _on_device_of(x0, x1, mask) as stream:
        check(clib.spv_dlt_triangulate_batch_device(
            x0.data_ptr(), x1.data_ptr(), off.ctypes.data, npairs, _ptr(P0s), P1s.ctypes.data, _ptr(use),
            mask.data_ptr() if mask is not None else None,
            X.data_ptr(), err.data_ptr() if want_error else None, rows.data_ptr() if want_rows else None, total,
            d_off.data_ptr() if mask is not None else None, None, stream))
    if mask is not None:
        out_off = d_off.cpu().numpy()
    else:
        out_off = col.offsets_of(np.diff(off) if use is None else np.diff(off) * (use != 0))
    out = (X,) + ((err,) if want_error else ()) + ((rows,) if want_rows else ())
    return out + (out_off,)


def match_coordinates_batch(geom, seg_off, pairs, matches, count):
    """`match_coordinates` for the matches of an `l1k2_batch` + `ratio_test` run: geom CUDA float32 [total_rows,4]
    holds the geometry of all sets back to back (row for row the desc of the matching call), seg_off and pairs are
    that call's.  Returns (x0 [cap,3], x1 [cap,3], pair_off int64 ndarray [npairs + 1]): rows
    pair_off[p]:pair_off[p + 1] are pair p's matches, x0 from the database set, x1 from the query set -- the
    arguments of `ransac_fit_batch`.  Reading pair_off back synchronises the current stream."""
    if geom.dim() != 2 or geom.shape[1] != 4 or matches.dim() != 2 or matches.shape[1] != 2:
        raise ValueError("geom must be [total_rows,4], matches [capacity,2]")
    seg, prs, _ = _collection_args(seg_off, pairs, geom.shape[0], "geom", out32=True)
    _need(geom, torch.float32, "geom")
    _need(matches, torch.int32, "matches")
    _need(count, torch.int32, "count")
    cap = matches.shape[0]
    x0 = torch.zeros((cap, 3), dtype=torch.float64, device=matches.device)
    x1 = torch.zeros((cap, 3), dtype=torch.float64, device=matches.device)
    pair_off = torch.zeros(len(prs) + 1, dtype=torch.int64, device=matches.device)
    with _on_device_of(geom, matches, count) as stream:
        check(clib.spv_gather_match_coords_batch_device(geom.data_ptr(), seg.ctypes.data, seg.size - 1, prs.ctypes.data,
                                                        len(prs), matches.data_ptr(), count.data_ptr(), cap,
                                                        x0.data_ptr(), x1.data_ptr(), pair_off.data_ptr(), stream))
    return x0, x1, pair_off.cpu().numpy()


def _tracks_batch_args(seg_off, pairs, capacity, min_len):
    """seg_off -> int64[nseg + 1], pairs -> int32[npairs, 2]; ValueError for anything spv_tracks_batch_device would
    reject, before any device is touched."""
    seg, prs, _ = _collection_args(seg_off, pairs, None, None, out32=True)
    if int(capacity) < 0:
        raise ValueError("capacity must not be negative")
    if int(min_len) != min_len or int(min_len) < 2:
        raise ValueError("min_len must be an integer >= 2: a track has at least two members")
    return seg, prs


def tracks_batch(seg_off, pairs, matches, count, mask=None, min_len=2, label=None, workspace=None):
    """Multi-view tracks on device: the connected components of the graph whose nodes are the rows of the
    concatenated tables (global row seg_off[s] + r) and whose edges are the matches of all pairs.  seg_off and pairs
    are the arguments of the `l1k2_batch` / `cascade_batch` / `l1k2_guided_batch` call, (matches, count) what
    `ratio_test` returned over its output, in any order; mask (uint8 [capacity], e.g. `ransac_fit_batch(want_mask=
    True)`'s) keeps row i only where it is not zero.  Rows out of range are skipped.

    Returns (track_off int64 ndarray [ntracks + 1], members int32 [nmembers, 2] = (set, row within the set), flags
    uint8 [ntracks], label int32 [total_rows], track int32 [total_rows]), the last four CUDA tensors: a track is a
    component of at least min_len members, tracks are numbered in ascending order of their label (the smallest
    global row), a track's members ascend by global row, bit 0 of flags marks a track with two members in one set,
    track is -1 outside every track.  Every output is a function of the edge set alone, bit for bit.

    Passing `label` (an earlier call's, over the same seg_off) continues from it -- the guided pass's matches on top
    of the blind pass's: the tensor is updated in place and returned, and the result is that of one call over both
    edge sets.  Reading the two counts back (and then the ntracks + 1 offsets they size) is where the call
    synchronises with the current stream; the library call itself does not."""
    if matches.dim() != 2 or matches.shape[1] != 2:
        raise ValueError("matches must be [capacity, 2]")
    cap = int(matches.shape[0])
    seg, prs = _tracks_batch_args(seg_off, pairs, cap, min_len)
    total = int(seg[-1])
    _need(matches, torch.int32, "matches")
    _need(count, torch.int32, "count")
    if mask is not None:
        _need(mask, torch.uint8, "mask")
        if mask.numel() < cap:
            raise ValueError("mask must have one entry per row of matches")
    dev = matches.device
    accumulate = label is not None
    if accumulate:
        _need(label, torch.int32, "label")
        if label.dim() != 1 or label.numel() != total:
            raise ValueError("label must be int32 [%d]" % total)
    else:
        label = torch.empty(total, dtype=torch.int32, device=dev)
    bound = total if accumulate else min(total, 2 * cap)
    track = torch.empty(total, dtype=torch.int32, device=dev)
    track_off = torch.empty(bound // 2 + 1, dtype=torch.int64, device=dev)
    members = torch.empty((bound, 2), dtype=torch.int32, device=dev)
    flags = torch.empty(bound // 2, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    nbytes = clib.spv_tracks_batch_workspace_bytes(total, cap)
    with _on_device_of(matches, count, mask, label) as stream:
        ws = (workspace or _default_ws).get(nbytes, dev)
        check(clib.spv_tracks_batch_device(seg.ctypes.data, seg.size - 1, prs.ctypes.data, len(prs), matches.data_ptr(),
                                           count.data_ptr(), cap, mask.data_ptr() if mask is not None else None,
                                           int(min_len), int(accumulate), label.data_ptr(), track.data_ptr(),
                                           track_off.data_ptr(), members.data_ptr(), flags.data_ptr(), counts.data_ptr(),
                                           ws.data_ptr(), ws.numel(), stream))
    nt, nm = counts.cpu().tolist()
    return track_off[:nt + 1].cpu().numpy(), members[:nm], flags[:nt], label, track


def tracks_triangulate_set_long(L):
    """The longest track `triangulate_tracks` solves with one lane (spv_tracks_triangulate_set_long; default 16, the
    fastest of 8, 16, 32 and 64 measured): longer tracks take one wave each.  0 sends every track of 3 or more members to
    the wave form, a value no track reaches sends none.  The results of a track with more than two usable observations
    differ between the forms by rounding only."""
    if int(L) != L or int(L) < 0:
        raise ValueError("L must be an integer >= 0")
    check(clib.spv_tracks_triangulate_set_long(int(min(int(L), 2 ** 31 - 1))))


def tracks_triangulate_get_long():
    """The setting of `tracks_triangulate_set_long`."""
    return int(clib.spv_tracks_triangulate_get_long())


def triangulate_tracks_plan(track_off):
    """Which form solves how many tracks under the current setting (spv_tracks_triangulate_plan; host only, no device
    touched): dict of lane_tracks, wave_tracks, lane_groups (workgroups of the lane launch) and longest."""
    off = col.offsets(track_off, "track_off")
    out = (ct.c_longlong * 4)()
    check(clib.spv_tracks_triangulate_plan(off.ctypes.data, off.size - 1, out))
    return dict(lane_tracks=int(out[0]), wave_tracks=int(out[1]), lane_groups=int(out[2]), longest=int(out[3]))


def _tracks_triangulate_args(geom_shape, seg_off, cameras, track_off, members_shape, max_error, use):
    """seg_off -> int64[nseg + 1], cameras -> float64[nseg, 12], use -> int32[nseg] or None, track_off ->
    int64[ntracks + 1], max_error -> float; ValueError for anything spv_tracks_triangulate_device would reject or that
    does not describe geom [total_rows, 4] and members [nmembers, 2].  A None entry of a cameras list is a set
    without a camera.  Touches no device."""
    if len(geom_shape) != 2 or geom_shape[1] != 4:
        raise ValueError("geom must be [total_rows, 4]")
    if len(members_shape) != 2 or members_shape[1] != 2:
        raise ValueError("members must be [nmembers, 2]")
    seg = col.offsets(seg_off, "seg_off", geom_shape[0], "geom")
    nseg = seg.size - 1
    off = col.offsets(track_off, "track_off", members_shape[0], "members")
    cameras, use = col.none_cameras_skip(cameras, nseg, "cameras", col.use_flags(use, nseg))
    try:
        cams = col.packed_cameras(cameras, nseg, "cameras")
    except (TypeError, ValueError):
        raise ValueError("cameras must hold one [3,4] camera per set")
    max_error = float(max_error)
    if max_error != max_error:
        raise ValueError("max_error must not be NaN")
    return seg, cams, use, off, max_error


def triangulate_tracks(geom, seg_off, cameras, track_off, members, max_error=float("inf"), use=None, want_err=True):
    """One 3-D point per track from all its observations (spv_tracks_triangulate_device): geom CUDA float32
    [total_rows, 4] (x, y, sigma, angle of every set's rows back to back, as `sift_split` writes them), seg_off the
    sets' offsets, cameras one host [3,4] camera per set ([nseg,3,4], or a list whose None entries are sets without
    a camera), use an optional per-set switch, (track_off, members) what `tracks_batch` returned.  The cameras are
    taken as given -- pixel cameras for pixel geom; `resect_fit_batch` estimates those of views that see points
    already triangulated.

    Returns (X float64 [ntracks,4], err float64 [nmembers] or None without want_err, ok uint8 [ntracks], nused int32
    [ntracks]) as CUDA tensors, aligned with the inputs.  An observation is usable when its set and row exist and the
    set has a camera; X is the unit null vector of the track's 2m x 4 DLT matrix (sign as `dlt_triangulate`'s), all
    zeros for a track with fewer than 2 usable observations; err the image-plane residual norm of every usable
    observation of a solved track, NaN elsewhere; ok is 1 where the track is solved, X is finite, the point lies in
    front of every usable observation's camera and every err <= max_error.  A track with exactly two usable
    observations is bit for bit `dlt_triangulate_batch`'s answer for them.  Asynchronous but for the upload of the
    cameras and offsets."""
    if not isinstance(geom, torch.Tensor) or geom.dtype != torch.float32:
        raise ValueError("geom must be a float32 tensor [total_rows, 4]")
    if not isinstance(members, torch.Tensor) or members.dtype != torch.int32:
        raise ValueError("members must be an int32 tensor [nmembers, 2]")
    seg, cams, use, off, max_error = _tracks_triangulate_args(tuple(geom.shape), seg_off, cameras, track_off,
                                                              tuple(members.shape), max_error, use)
    _need(geom, torch.float32, "geom")
    _need(members, torch.int32, "members")
    nt, nm, dev = off.size - 1, int(members.shape[0]), geom.device
    X = torch.empty((nt, 4), dtype=torch.float64, device=dev)
    err = torch.empty(nm, dtype=torch.float64, device=dev) if want_err else None
    ok = torch.empty(nt, dtype=torch.uint8, device=dev)
    nused = torch.empty(nt, dtype=torch.int32, device=dev)
    with _on_device_of(geom, members) as stream:
        check(clib.spv_tracks_triangulate_device(
            geom.data_ptr(), seg.ctypes.data, seg.size - 1, cams.ctypes.data, _ptr(use), off.ctypes.data, nt,
            members.data_ptr(), nm, max_error, X.data_ptr(), err.data_ptr() if want_err else None, ok.data_ptr(),
            nused.data_ptr(), stream))
    return X, err, ok, nused


def bundle_adjust_plan(track_off, members=None, seg_off=None, mode=None):
    """How bundle_adjust() lays a collection out (spv_bundle_adjust_plan; host only, no device touched): dict of
    lane_tracks, wave_tracks, chunk (observations of a view-major chunk), chunks and longest.  chunks needs the host
    members int32 [nmembers, 2] and seg_off, and counts the chunks of the free sets (mode 1; every set without mode)
    when every usable member of a track with two or more takes part; it is 0 without members."""
    off = col.offsets(track_off, "track_off")
    mem = seg = md = None
    if members is not None:
        mem = np.ascontiguousarray(members, dtype=np.int32).reshape(-1, 2)
        if len(mem) != off[-1]:
            raise ValueError("track_off ends at %d, members has %d rows" % (off[-1], len(mem)))
        seg = col.offsets(seg_off, "seg_off")
        if mode is not None:
            md = np.ascontiguousarray(mode, dtype=np.int32).reshape(-1)
            if md.size != seg.size - 1:
                raise ValueError("mode must hold one value per set")
    out = (ct.c_longlong * 5)()
    check(clib.spv_bundle_adjust_plan(off.ctypes.data, off.size - 1, _ptr(mem), _ptr(seg), 0 if seg is None else seg.size - 1,
                                      _ptr(md), out))
    return dict(lane_tracks=int(out[0]), wave_tracks=int(out[1]), chunk=int(out[2]), chunks=int(out[3]), longest=int(out[4]))


def bundle_adjust(geom, seg_off, K, poses, track_off, members, X, use=None, fixed=None, huber=float("inf"), max_steps=50,
                  lambda0=1e-4, ftol=1e-10, gtol=1e-10, cg_tol=1e-8, cg_max=None, want_err=False, workspace=None):
    """Levenberg-Marquardt refinement of cameras and track points over all observations (spv_bundle_adjust_device):
    geom, seg_off, (track_off, members) as `triangulate_tracks` takes them, X CUDA float64 [ntracks, 4] its points
    (not modified: the refined points are returned), use an optional per-track switch (CUDA uint8, e.g. its ok), K
    one [3,3] calibration or one per set (held fixed), poses one [3,4] = [R | t] per set, None for a set without a
    camera, fixed an optional per-set switch: a fixed camera's observations count but it is never moved.  huber is
    the width of the robust loss in pixels (inf: least squares); cg_max None means 6 * free cameras + 10.

    Returns (poses ndarray [nseg,3,4] -- zeros for sets without a camera --, X CUDA float64 [ntracks,4] with (X, Y, Z,
    1) in the rows of the tracks that took part and the input's bits elsewhere, info): info has steps, accepted,
    stop ('max_steps', 'gradient', 'cost' or 'damping'), tracks, observations, first_cost, last_cost, trace
    [steps, 6] = (F before, F', lambda, CG iterations, accepted, max |g|), active (CUDA uint8 [ntracks]) and, with
    want_err, err (CUDA float64 [nmembers]: the residual norm of every participating observation, NaN elsewhere).
    The same inputs give the same bits.  Waits for the stream once per step."""
    if not isinstance(geom, torch.Tensor) or geom.dtype != torch.float32 or geom.dim() != 2 or geom.shape[1] != 4:
        raise ValueError("geom must be a float32 tensor [total_rows, 4]")
    if not isinstance(members, torch.Tensor) or members.dtype != torch.int32 or members.dim() != 2 or members.shape[1] != 2:
        raise ValueError("members must be an int32 tensor [nmembers, 2]")
    seg = col.offsets(seg_off, "seg_off", geom.shape[0], "geom")
    nseg = seg.size - 1
    off = col.offsets(track_off, "track_off", members.shape[0], "members")
    nt, nm = off.size - 1, int(members.shape[0])
    if not isinstance(X, torch.Tensor) or X.dtype != torch.float64 or tuple(X.shape) != (nt, 4):
        raise ValueError("X must be a float64 tensor [ntracks, 4]")
    if use is not None and (not isinstance(use, torch.Tensor) or use.dtype != torch.uint8 or tuple(use.shape) != (nt,)):
        raise ValueError("use must be a uint8 tensor [ntracks]")
    Ks, P, mode = col.bundle_cameras(K, poses, fixed, nseg)
    huber, max_steps, lambda0, ftol, gtol, cg_tol, cg_max = col.bundle_options(huber, max_steps, lambda0, ftol, gtol,
                                                                               cg_tol, cg_max, mode)
    _need(geom, torch.float32, "geom")
    _need(members, torch.int32, "members")
    _need(X, torch.float64, "X")
    if use is not None:
        _need(use, torch.uint8, "use")
    dev = geom.device
    Xo = X.clone()
    err = torch.empty(nm, dtype=torch.float64, device=dev) if want_err else None
    active = torch.empty(nt, dtype=torch.uint8, device=dev)
    trace, info = np.full((max_steps, 6), np.nan), np.zeros(7)
    nbytes = clib.spv_bundle_adjust_workspace_bytes(nseg, nt, nm)
    with _on_device_of(geom, members, X) as stream:
        ws = (workspace or _default_ws).get(nbytes, dev)
        check(clib.spv_bundle_adjust_device(
            geom.data_ptr(), seg.ctypes.data, nseg, Ks.ctypes.data, P.ctypes.data, mode.ctypes.data, off.ctypes.data, nt,
            members.data_ptr(), nm, Xo.data_ptr(), use.data_ptr() if use is not None else None, huber, max_steps, lambda0,
            ftol, gtol, cg_tol, cg_max, err.data_ptr() if want_err else None, active.data_ptr(), trace.ctypes.data,
            info.ctypes.data, ws.data_ptr(), ws.numel(), stream))
    out = col.bundle_info(info, trace)
    out['active'] = active
    if want_err:
        out['err'] = err
    return P.reshape(nseg, 3, 4), Xo, out


def _resect_gather_args(geom_shape, seg_off, views, track_shape, X_shape, ok_shape, capacity):
    """seg_off -> int64[nseg + 1], views -> int32[nviews] (each in [0, nseg)), capacity (None: the rows of the listed
    views); ValueError for anything spv_resect_gather_device would reject or that does not describe geom [total_rows,
    4], track [total_rows], X [ntracks, 4] and ok [ntracks].  Touches no device."""
    if len(geom_shape) != 2 or geom_shape[1] != 4:
        raise ValueError("geom must be [total_rows, 4]")
    seg = col.offsets(seg_off, "seg_off", geom_shape[0], "geom")
    nseg = seg.size - 1
    if tuple(track_shape) != (geom_shape[0],):
        raise ValueError("track must hold one entry per row of geom")
    if len(X_shape) != 2 or X_shape[1] != 4:
        raise ValueError("X must be [ntracks, 4]")
    if ok_shape is not None and tuple(ok_shape) != (X_shape[0],):
        raise ValueError("ok must hold one entry per track")
    v = np.asarray(views)
    if v.size == 0:
        v = np.zeros(0, np.int32)
    if v.ndim != 1 or v.dtype.kind not in "iu":
        raise ValueError("views must be a list of set numbers")
    if v.size and (int(v.min()) < 0 or int(v.max()) >= nseg):
        raise ValueError("views name sets outside [0, %d)" % nseg)
    col.check_set_count(v.size)
    v = np.ascontiguousarray(v, dtype=np.int32)
    rows = int(np.diff(seg)[v].sum())
    if rows >= 2 ** 31:
        raise ValueError("the listed views must have fewer than 2^31 rows in all")
    capacity = rows if capacity is None else int(capacity)
    if capacity < 0:
        raise ValueError("capacity must not be negative")
    return seg, v, capacity


def resect_gather(geom, track, seg_off, views, X, ok=None, capacity=None):
    """The 2-D / 3-D correspondences of the listed views (spv_resect_gather_device): geom CUDA float32 [total_rows, 4]
    and seg_off as for `triangulate_tracks`, track CUDA int32 [total_rows] what `tracks_batch` returned, (X, ok) what
    `triangulate_tracks` returned, views the sets to resect (repeats are legal).  A row is taken when its track number
    is in range, ok (if given) is not zero there and the track's X is finite.  Returns (x float64 [capacity, 3] =
    (u, v, 1), Xw float64 [capacity, 4], rows int32 [capacity] = the row within its view, view_off int64 ndarray
    [nviews + 1]): listed view i owns rows view_off[i]:view_off[i + 1], the arguments of `resect_fit_batch`.  capacity
    defaults to the rows of the listed views; view_off counts every taken row even beyond it, and nothing beyond it
    is written.  Reading view_off back synchronises the current stream."""
    if not isinstance(geom, torch.Tensor) or geom.dtype != torch.float32:
        raise ValueError("geom must be a float32 tensor [total_rows, 4]")
    seg, v, capacity = _resect_gather_args(tuple(geom.shape), seg_off, views, tuple(track.shape), tuple(X.shape),
                                           None if ok is None else tuple(ok.shape), capacity)
    _need(geom, torch.float32, "geom")
    _need(track, torch.int32, "track")
    _need(X, torch.float64, "X")
    if ok is not None:
        _need(ok, torch.uint8, "ok")
    dev = geom.device
    x = torch.zeros((capacity, 3), dtype=torch.float64, device=dev)
    Xw = torch.zeros((capacity, 4), dtype=torch.float64, device=dev)
    rows = torch.zeros(capacity, dtype=torch.int32, device=dev)
    view_off = np.zeros(v.size + 1, np.int64)
    with _on_device_of(geom, track, X, ok) as stream:
        check(clib.spv_resect_gather_device(
            geom.data_ptr(), track.data_ptr(), seg.ctypes.data, seg.size - 1, v.ctypes.data, v.size, X.data_ptr(),
            ok.data_ptr() if ok is not None else None, int(X.shape[0]), capacity, x.data_ptr(), Xw.data_ptr(),
            rows.data_ptr(), None, view_off.ctypes.data, stream))
    return x, Xw, rows, view_off


def _resect_fit_args(view_off, total, max_error, required_percent_inliers, maximum_tries, seeds, samples):
    """view_off -> int64[nviews + 1], samples -> int32[nviews, T, 6] or None, seeds -> uint64[nviews] or None,
    maximum_tries, max_error and the share as floats; ValueError for anything spv_resect_fit_batch_device would reject
    or that does not describe arrays of `total` rows.  Touches no device."""
    off = col.offsets(view_off, "view_off", total, "x")
    nviews = off.size - 1
    col.check_set_count(nviews)
    samples = col.sample_table(samples, np.diff(off), 6, 6)
    seeds, maximum_tries = col.seeds_and_tries(seeds, samples, maximum_tries, nviews)
    max_error, share = float(max_error), float(required_percent_inliers)
    if max_error != max_error or share != share:
        raise ValueError("max_error and required_percent_inliers must not be NaN")
    return off, samples, seeds, maximum_tries, max_error, share


def resect_fit_batch_plan(view_off, maximum_tries=500, compute_units=256, want_items=False):
    """The first round of resect_fit_batch() for a collection (spv_resect_fit_batch_plan; host only, no device
    touched): dict of sets and tries in the round, items (work items = workgroups of the scorer) and row_blocks
    (blocks of 256 rows).  With want_items also the items, int32[items, 5] = (set, first row, rows, first try of the
    round, tries)."""
    off = col.offsets(view_off, "view_off")
    out, items = _plan_items(clib.spv_resect_fit_batch_plan,
                             (off.ctypes.data, off.size - 1, int(maximum_tries), int(compute_units)), 4, 5, want_items, at=2)
    plan = dict(sets=out[0], tries=out[1], items=out[2], row_blocks=out[3])
    return (plan, items) if want_items else plan


def resect_fit_batch(x, Xw, view_off, required_percent_inliers=.9, max_error=2., maximum_tries=500,
                     find_best_even_in_failure=False, samples=None, seeds=None, want_mask=False, want_tries=False):
    """RANSAC camera resection of every set of a collection in one call (spv_resect_fit_batch_device): x CUDA float64
    [total, 3] = (u, v, 1) and Xw CUDA float64 [total, 4] hold the sets back to back, set p = rows
    view_off[p]:view_off[p + 1] (e.g. the output of `resect_gather`), in the caller's units -- max_error is in those of
    x.  samples int32 [nviews, ntries, 6] (row numbers inside the set; `maximum_tries` and `seeds` are then ignored) or
    seeds [nviews] (0 = SPECTAVI_RANSAC_SEED / random; the first six columns of `mvg.ransac_sample`) choose the subsets.
    A try's camera is the unit null vector of the 11 x 12 matrix of its six rows; a row is an inlier when it reprojects
    within max_error in front of the camera; the winner is the first try whose inlier share reaches
    required_percent_inliers, else -- with find_best_even_in_failure -- the try with the most inliers.  Returns a list
    of dicts (success, camera [3,4] or None, inlier_percent, inlier_idx, best_try, tries_run); a set of fewer than 6
    rows is skipped.  With want_mask also a CUDA uint8 [total] tensor (1 = inlier of its set's kept camera), with
    want_tries also the CUDA tensors try_cameras float64 [nviews, ntries, 12] and try_inliers int32 [nviews, ntries]
    (every try is then evaluated).  Synchronises the current stream once per round of tries, however many sets; the
    mask is computed and copied to the host (one byte a row) whether it is wanted or not: inlier_idx is read from it."""
    if not (x.dim() == 2 and x.shape[1] == 3 and Xw.dim() == 2 and Xw.shape[1] == 4 and x.shape[0] == Xw.shape[0]):
        raise ValueError("x must be [total,3] and Xw [total,4]")
    total = x.shape[0]
    off, samples, seeds, maximum_tries, max_error, share = _resect_fit_args(view_off, total, max_error, required_percent_inliers,
                                                                           maximum_tries, seeds, samples)
    _need(x, torch.float64, "x")
    _need(Xw, torch.float64, "Xw")
    nviews = off.size - 1
    ok, n, bt, ran = (np.zeros(nviews, np.int32) for _ in range(4))
    pct, P = np.zeros(nviews), np.zeros((nviews, 12))
    mask = torch.empty(total, dtype=torch.uint8, device=x.device)
    cams = torch.empty((nviews, maximum_tries, 12), dtype=torch.float64, device=x.device) if want_tries else None
    inl = torch.empty((nviews, maximum_tries), dtype=torch.int32, device=x.device) if want_tries else None
    with _on_device_of(x, Xw) as stream:
        check(clib.spv_resect_fit_batch_device(
            x.data_ptr(), Xw.data_ptr(), off.ctypes.data, nviews, share, max_error, maximum_tries,
            int(bool(find_best_even_in_failure)), _ptr(samples), seeds.ctypes.data if samples is None else None,
            ok.ctypes.data, P.ctypes.data, pct.ctypes.data, n.ctypes.data, bt.ctypes.data, ran.ctypes.data,
            mask.data_ptr(), cams.data_ptr() if want_tries else None, inl.data_ptr() if want_tries else None, stream))
    fits = col.resect_dicts(off, ok, P, pct, bt, ran, mask.cpu().numpy())
    out = (fits,) + ((mask,) if want_mask else ()) + ((cams, inl) if want_tries else ())
    return out if len(out) > 1 else fits


def normalize(x, want_float=True, want_ubyte=False, workspace=None):
    """`normalize_to_ubyte_and_multiple_16_dim` (reference spectavi/feature.py:384-407) on a CUDA float32
    [rows, dim] table, bit-identical to the numpy function: returns the float32 [rows, dim16] table
    and / or its `(out + 128).astype('uint8')` image (what `l1k2` takes).  Asynchronous."""
    _need(x, torch.float32, "x")
    rows, dim = x.shape
    dim16 = (dim + 15) // 16 * 16
    out = torch.empty((rows, dim16), dtype=torch.float32, device=x.device) if want_float else None
    u8 = torch.empty((rows, dim16), dtype=torch.uint8, device=x.device) if want_ubyte else None
    with _on_device_of(x) as stream:
        ws = (workspace or _default_ws).get(clib.spv_normalize_workspace_bytes_rows(rows, dim), x.device)
        check(clib.spv_normalize_device(x.data_ptr(), rows, dim, out.data_ptr() if want_float else None,
                                        u8.data_ptr() if want_ubyte else None, ws.data_ptr(), ws.numel(), stream))
    if want_float and want_ubyte:
        return out, u8
    return out if want_float else u8


NORMALIZE_F32, NORMALIZE_U8 = 0, 1  # SPV_NORMALIZE_* of include/spectavi_amd.h


def _normalize_batch_args(seg_off, total_rows, dim, dtype):
    """seg_off -> int64[nseg + 1], dtype -> SPV_NORMALIZE_*; ValueError for anything spv_normalize_batch_device would
    reject or that does not describe a table of total_rows rows.  Touches no device."""
    seg = col.offsets(seg_off, "seg_off", total_rows, "x")
    if not 1 <= int(dim) <= 2048:
        raise ValueError("the many-tables form takes 1 <= dim <= 2048 (dim=%d)" % dim)
    if dim == 1 and np.any(np.diff(seg) > 1):
        raise ValueError("normalisation of a single-column table is not supported (dim=1)")
    name = str(dtype)[6:] if isinstance(dtype, torch.dtype) else np.dtype(dtype).name
    if name not in ("float32", "uint8"):
        raise TypeError("dtype must be float32 or uint8")
    return seg, NORMALIZE_U8 if name == "uint8" else NORMALIZE_F32


def normalize_batch_plan(seg_off, dim, dtype, compute_units=256, want_items=False):
    """The work items normalize_batch() walks for a collection (spv_normalize_batch_plan; host only, no device
    touched): dict of sets (non-empty sets), items (workgroup steps), workspace_bytes and rows (in all).  dtype:
    torch / numpy float32 or uint8.  With want_items also the items, int32[items, 3] = (set, first row within the
    set, rows), in the order the device call walks them."""
    seg, kind = _normalize_batch_args(seg_off, None, dim, dtype)
    out, items = _plan_items(clib.spv_normalize_batch_plan, (seg.ctypes.data, seg.size - 1, int(dim), kind, int(compute_units)),
                             4, 3, want_items, at=1)
    plan = dict(sets=out[0], items=out[1], workspace_bytes=out[2], rows=out[3])
    return (plan, items) if want_items else plan


def normalize_batch(x, seg_off, want_float=True, want_ubyte=False, workspace=None):
    """`normalize` of every table of a collection in one fixed chain of launches (spv_normalize_batch_device): x CUDA
    float32 or uint8 [total, dim] holds the tables back to back, set s = rows seg_off[s]:seg_off[s + 1] (empty sets
    allowed); uint8 values stand for their float32 conversions, no float copy is made.  Returns what `normalize`
    returns, for all rows: the float32 [total, dim16] table and / or its uint8 image, every set's rows bit for bit
    `normalize` of that set alone.  Asynchronous on the current stream but for the upload of the work table."""
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.uint8):
        raise TypeError("x must be a float32 or uint8 tensor")
    _need(x, x.dtype, "x")
    if x.dim() != 2:
        raise ValueError("x must be [total_rows, dim]")
    if not (want_float or want_ubyte):
        raise ValueError("neither the float32 nor the uint8 table is wanted")
    total, dim = x.shape
    seg, kind = _normalize_batch_args(seg_off, total, dim, x.dtype)
    dim16 = (dim + 15) // 16 * 16
    out = torch.empty((total, dim16), dtype=torch.float32, device=x.device) if want_float else None
    u8 = torch.empty((total, dim16), dtype=torch.uint8, device=x.device) if want_ubyte else None
    nbytes = clib.spv_normalize_batch_workspace_bytes(seg.ctypes.data, seg.size - 1, dim, kind)
    with _on_device_of(x) as stream:
        ws = (workspace or _default_ws).get(nbytes, x.device)
        check(clib.spv_normalize_batch_device(x.data_ptr(), kind, seg.ctypes.data, seg.size - 1, dim,
                                              out.data_ptr() if want_float else None,
                                              u8.data_ptr() if want_ubyte else None, ws.data_ptr(), ws.numel(), stream))
    if want_float and want_ubyte:
        return out, u8
    return out if want_float else u8


def seven_point(x, xp, want_basis=False):
    """Seven-point algorithm for n 7-subsets resident in HBM (reference src/FundamentalMatrixFitter.h:108-246):
    x, xp CUDA float64 [n,7,2] euclidean.  Returns (nroot int32 [n], Fs float64 [n,3,3,3], NaN in the slots of
    missing roots) and, with want_basis, the null-space pair [n,2,3,3].  Asynchronous on the current stream."""
    _need(x, torch.float64, "x")
    _need(xp, torch.float64, "xp")
    assert x.dim() == 3 and x.shape[1:] == (7, 2) and xp.shape == x.shape
    n = x.shape[0]
    nroot = torch.empty(n, dtype=torch.int32, device=x.device)
    Fs = torch.empty((n, 3, 3, 3), dtype=torch.float64, device=x.device)
    basis = torch.empty((n, 2, 3, 3), dtype=torch.float64, device=x.device) if want_basis else None
    with _on_device_of(x, xp) as stream:
        check(clib.spv_seven_point_device(x.data_ptr(), xp.data_ptr(), n, Fs.data_ptr(), nroot.data_ptr(),
                                          basis.data_ptr() if want_basis else None, stream))
    return (nroot, Fs, basis) if want_basis else (nroot, Fs)


_RECTIFY_DTYPE = {torch.float64: 0, torch.uint8: 1}  # SPV_RECTIFY_F64, SPV_RECTIFY_U8


def image_pair_rectification(P0, P1, im0, im1, sampling_factor=1.2):
    """mvg.image_pair_rectification with the images resident in HBM: im0, im1 CUDA tensors of one
    shape, [hgt, wid] or [hgt, wid, nchan], both float64 or both uint8 (values are copied, never
    computed, so 8-bit images stay 8-bit).  P0, P1 float64 [3,4] on the host.  Returns the uncropped
    (r0, r1 [rows, cols] or [rows, cols, nchan] of the images' dtype, ri0, ri1 int32 [rows, cols]).
    Asynchronous on the current stream."""
    from spectavi_amd import mvg
    if not isinstance(im0, torch.Tensor) or im0.dtype not in _RECTIFY_DTYPE:
        raise TypeError("im0 must be a float64 or uint8 tensor")
    _need(im0, im0.dtype, "im0")
    _need(im1, im0.dtype, "im1")
    if im0.shape != im1.shape:
        raise TypeError("Input images must have same size.")
    hgt, wid, nchan = mvg.image_dims(tuple(im0.shape))
    F = mvg.rectification_fundamental(P0, P1).reshape(-1)
    rows, cols, _ = mvg.rectification_shape(wid, hgt, nchan, sampling_factor)
    vshape = (rows, cols) if nchan == 1 else (rows, cols, nchan)
    r0 = torch.empty(vshape, dtype=im0.dtype, device=im0.device)
    r1 = torch.empty(vshape, dtype=im0.dtype, device=im0.device)
    ri0 = torch.empty((rows, cols), dtype=torch.int32, device=im0.device)
    ri1 = torch.empty((rows, cols), dtype=torch.int32, device=im0.device)
    with _on_device_of(im0, im1) as stream:
        check(clib.spv_rectify_device(F, im0.data_ptr(), im1.data_ptr(), _RECTIFY_DTYPE[im0.dtype], wid, hgt, nchan,
                                      float(sampling_factor), r0.data_ptr(), r1.data_ptr(), ri0.data_ptr(),
                                      ri1.data_ptr(), stream))
    return r0, r1, ri0, ri1


_RECTIFY_BATCH_DTYPE = dict(_RECTIFY_DTYPE)
_RECTIFY_BATCH_DTYPE[torch.float32] = 2  # SPV_RECTIFY_F32: the batch form alone


def _rectify_batch_args(sizes, pairs, P1s, P0s, use, box=None):
    """sizes -> int32[nimg, 2], pairs -> int32[npairs, 2], P1s / P0s -> float64[npairs, 12] (P0s or None), use ->
    int32[npairs] or None, box -> int32[npairs, 4] or None.  A None entry of a P1s list is a pair that is not used.
    ValueError where the counts disagree; the library checks the rest.  Touches no device."""
    sizes = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 2)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    npairs = len(pairs)
    use = col.use_flags(use, npairs, "pair")
    if P1s is not None:
        P1s, use = col.none_cameras_skip(P1s, npairs, "P1s", use, "pair")
        P1s = col.packed_cameras(P1s, npairs, "P1s", "pair")
    if box is not None:
        box = np.ascontiguousarray(box, dtype=np.int32).reshape(-1, 4)
        if len(box) != npairs:
            raise ValueError("box must hold one (row_lo, row_hi, col_lo, col_hi) per pair")
    return sizes, pairs, P1s, None if P0s is None else col.packed_cameras(P0s, npairs, "P0s", "pair"), use, box


def rectify_batch_plan(sizes, pairs, nchan=1, sampling_factor=1.2, use=None, box=None, want_items=False):
    """What rectify_batch() writes and launches for a collection (spv_rectify_batch_plan; host only, no device
    touched): dict of pairs (used pairs), items (workgroup steps), samples (window samples in all) and out_off, an
    int64 ndarray [npairs + 1] -- pair p owns samples out_off[p]:out_off[p + 1] of the flat outputs, its window
    box[p] = (row_lo, row_hi, col_lo, col_hi) in row-major order (box None: whole frames).  With want_items also the
    items, int32[items, 4] = (pair, image 0 or 1, first frame row, rows <= 8)."""
    sizes, pairs, _, _, use, box = _rectify_batch_args(sizes, pairs, None, None, use, box)
    out_off = np.zeros(len(pairs) + 1, np.int64)
    args = (sizes.ctypes.data, len(sizes), int(nchan), float(sampling_factor), pairs.ctypes.data, len(pairs), _ptr(use),
            _ptr(box))
    out, items = _plan_items(clib.spv_rectify_batch_plan, args, 3, 4, want_items, at=1, tail=(out_off.ctypes.data,))
    plan = dict(pairs=out[0], items=out[1], samples=out[2], out_off=out_off)
    return (plan, items) if want_items else plan


def rectify_batch_bounds(sizes, pairs, P1s, P0s=None, use=None, nchan=1, sampling_factor=1.2, device=None):
    """The window every pair of a collection rectifies into (spv_rectify_batch_bounds_device): a CUDA int32
    [npairs, 4] tensor of (row_lo, row_hi, col_lo, col_hi), half-open, in each pair's uncropped frame -- the bounding
    box of the samples valid in either image, what `mvg.image_pair_rectification(crop_invalid=True)` keeps --,
    (0, 0, 0, 0) where a pair has none or is not used.  No image is read.  Asynchronous on the current stream of
    `device` (default: the current device) but for the upload of the cameras."""
    sizes, pairs, P1s, P0s, use, _ = _rectify_batch_args(sizes, pairs, P1s, P0s, use)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    d_box = torch.empty((len(pairs), 4), dtype=torch.int32, device=dev)
    with _on_device_of(d_box) as stream:
        check(clib.spv_rectify_batch_bounds_device(sizes.ctypes.data, len(sizes), int(nchan), float(sampling_factor),
                                                   pairs.ctypes.data, len(pairs), _ptr(P0s), _ptr(P1s), _ptr(use),
                                                   d_box.data_ptr(), stream))
    return d_box


def rectify_batch(images, sizes, pairs, P1s, P0s=None, use=None, sampling_factor=1.2, crop_invalid=True, box=None):
    """`image_pair_rectification` for every pair of a collection in one call, cropped on the device
    (spv_rectify_batch_bounds_device, spv_rectify_batch_device).  images: a list of CUDA tensors [hgt, wid] or
    [hgt, wid, nchan] of one dtype (float64, float32 or uint8) and one nchan -- sizes may then be None --, or one
    packed tensor holding the images back to back together with sizes = (wid, hgt) per image (gray images:
    `sift_batch`'s layout; more channels: the packed tensor's last dimension is nchan).  pairs [npairs, 2] =
    (image 0, image 1): a matcher's pair (query set, database set) is passed as (database, query).  P1s, P0s
    (None: [I|0]) host [3,4] cameras per pair; a pair with use[p] == 0 (or a None entry of a P1s list) is skipped.

    With crop_invalid every pair is written only inside the bounding box of its valid samples, which costs the
    call's one synchronisation (the boxes come back to size the outputs); box, int32 [npairs, 4] on the host, gives
    the windows instead, and with neither whole frames are written, both without a synchronisation.  Returns
    (r0, r1, ri0, ri1, box, out_off): flat CUDA tensors (values of the images' dtype, [samples * nchan]; indices
    int32 [samples]), box and out_off as ndarrays; pair p owns samples out_off[p]:out_off[p + 1], see
    rectify_batch_view().  Every window is bit for bit the slice of what `image_pair_rectification` returns for the
    pair alone; a pair without a valid sample has an empty box and no output."""
    if isinstance(images, torch.Tensor):
        if sizes is None:
            raise ValueError("a packed tensor needs sizes")
        packed = images
        nchan = packed.shape[-1] if packed.dim() > 1 else 1
    else:
        from spectavi_amd import mvg
        dims = [mvg.image_dims(tuple(im.shape)) for im in images]
        if len({d[2] for d in dims}) > 1 or len({im.dtype for im in images}) > 1:
            raise TypeError("the images must share one dtype and one number of channels")
        nchan = dims[0][2] if dims else 1
        if sizes is None:
            sizes = [(d[1], d[0]) for d in dims]
        packed = torch.cat([im.reshape(-1) for im in images]) if len(images) else torch.empty(0, device="cuda")
    if packed.dtype not in _RECTIFY_BATCH_DTYPE:
        raise TypeError("the images must be float64, float32 or uint8 tensors")
    sizes, pairs, P1s, P0s, use, box = _rectify_batch_args(sizes, pairs, P1s, P0s, use, box)
    sf = float(sampling_factor)
    if box is None and crop_invalid:
        d_box = rectify_batch_bounds(sizes, pairs, P1s, P0s, use, nchan, sf, device=packed.device)
        box = d_box.cpu().numpy()  # the call's one synchronisation
    plan = rectify_batch_plan(sizes, pairs, nchan, sf, use, box)
    if box is None:  # whole frames (the plan has checked the pairs)
        from spectavi_amd import mvg
        box = np.zeros((len(pairs), 4), np.int32)
        for p, (a, _) in enumerate(pairs):
            if use is None or use[p]:
                rows, cols, _ = mvg.rectification_shape(sizes[a, 0], sizes[a, 1], nchan, sf)
                box[p] = (0, rows, 0, cols)
    elif use is not None:
        box = box * (use != 0)[:, None].astype(np.int32)
    out_off, total = plan["out_off"], plan["samples"]
    r0 = torch.empty(total * nchan, dtype=packed.dtype, device=packed.device)
    r1 = torch.empty(total * nchan, dtype=packed.dtype, device=packed.device)
    ri0 = torch.empty(total, dtype=torch.int32, device=packed.device)
    ri1 = torch.empty(total, dtype=torch.int32, device=packed.device)
    rectify_batch_into(packed, sizes, pairs, P1s, P0s, use, sf, box, nchan, r0, r1, ri0, ri1)
    return r0, r1, ri0, ri1, box, out_off


def rectify_batch_into(packed, sizes, pairs, P1s, P0s, use, sampling_factor, box, nchan, r0, r1, ri0, ri1):
    """The resampling step of rectify_batch() into caller-allocated flat tensors (spv_rectify_batch_device): r0, r1
    of the images' dtype with at least samples * nchan elements, ri0, ri1 int32 with at least samples, `samples` from
    rectify_batch_plan().  Only the windows are written.  Asynchronous on the current stream."""
    if not isinstance(packed, torch.Tensor) or packed.dtype not in _RECTIFY_BATCH_DTYPE:
        raise TypeError("the images must be float64, float32 or uint8 tensors")
    sizes, pairs, P1s, P0s, use, box = _rectify_batch_args(sizes, pairs, P1s, P0s, use, box)
    _need(packed, packed.dtype, "images")
    _need(r0, packed.dtype, "r0")
    _need(r1, packed.dtype, "r1")
    _need(ri0, torch.int32, "ri0")
    _need(ri1, torch.int32, "ri1")
    if int((sizes[:, 0].astype(np.int64) * sizes[:, 1]).sum()) * nchan != packed.numel():
        raise ValueError("sizes do not describe the packed images")
    if box is None:
        samples = rectify_batch_plan(sizes, pairs, nchan, sampling_factor, use)["samples"]
    else:  # (the library checks the boxes against the frames)
        area = (box[:, 1] - box[:, 0]).astype(np.int64) * (box[:, 3] - box[:, 2])
        samples = int(area.sum() if use is None else area[use != 0].sum())
    if min(r0.numel(), r1.numel()) < samples * nchan or min(ri0.numel(), ri1.numel()) < samples:
        raise ValueError("the outputs are too short for the %d samples of the windows" % samples)
    with _on_device_of(packed, r0, r1, ri0, ri1) as stream:
        check(clib.spv_rectify_batch_device(packed.data_ptr(), _RECTIFY_BATCH_DTYPE[packed.dtype],
                                            sizes.ctypes.data, len(sizes), int(nchan), float(sampling_factor),
                                            pairs.ctypes.data, len(pairs), _ptr(P0s), _ptr(P1s), _ptr(use), _ptr(box),
                                            r0.data_ptr(), r1.data_ptr(), ri0.data_ptr(), ri1.data_ptr(), stream))


def rectify_batch_view(flat, p, box, out_off, nchan=1):
    """Pair p's window of a flat output of rectify_batch() as a view, nothing copied: [rows, cols] for ri0 / ri1
    and for gray values, [rows, cols, nchan] for r0 / r1 when nchan (the images' channels) is given above 1."""
    rows, cols = int(box[p][1] - box[p][0]), int(box[p][3] - box[p][2])
    w = flat[int(out_off[p]) * nchan:int(out_off[p + 1]) * nchan]
    return w.reshape(rows, cols) if nchan == 1 else w.reshape(rows, cols, nchan)


STEREO_NONE = -2**31  # SPV_STEREO_NONE: the disparity of a sample that admits none


def _stereo_batch_args(box, use=None, drange=None, radius=None):
    """box -> int32[npairs, 4], use -> int32[npairs] or None, drange -> int32[npairs, 2] (one (d_lo, d_hi) for
    every pair is broadcast) or None.  ValueError where the counts disagree or radius is outside 0..7; the library
    checks the rest.  Touches no device."""
    box = np.ascontiguousarray(box, dtype=np.int32).reshape(-1, 4)
    npairs = len(box)
    use = col.use_flags(use, npairs, "pair")
    if drange is not None:
        drange = np.asarray(drange, dtype=np.int32)
        if drange.shape == (2,):
            drange = np.tile(drange, (npairs, 1))
        drange = np.ascontiguousarray(drange).reshape(-1, 2)
        if len(drange) != npairs:
            raise ValueError("drange must hold one (d_lo, d_hi), or one per pair")
    if radius is not None and not 0 <= int(radius) <= 7:
        raise ValueError("radius must be in 0..7")
    return box, use, drange


def _stereo_samples(box):
    return int(((box[:, 1] - box[:, 0]).astype(np.int64) * (box[:, 3] - box[:, 2])).sum())


def _need_samples(t, dtype, name, samples, exact=False):
    """t: a contiguous CUDA tensor of `dtype` with at least `samples` elements (a caller-allocated output or a
    per-sample result) or, with exact, with `samples` elements and no more: what rectify_batch() returns for gray
    images.  The rectified values of images with more channels hold samples * nchan elements and are refused here,
    since the library is given no channel count."""
    _need(t, dtype, name)
    if exact and t.numel() != samples:
        raise ValueError("%s must hold exactly the %d samples of the windows, one element per sample (gray images, "
                         "nchan == 1, only); it has %d elements" % (name, samples, t.numel()))
    if t.numel() < samples:
        raise ValueError("%s is too short for the %d samples of the windows" % (name, samples))


def stereo_batch_plan(box, use=None, radius=0, drange=None, want_items=False):
    """What stereo_batch() writes and launches for a collection of windows (spv_stereo_batch_plan; host only, no
    device touched): dict of pairs (used pairs), items (workgroup steps), samples and out_off, an int64 ndarray
    [npairs + 1] -- the running areas of all boxes.  With want_items also the items, int32[items, 4] = (pair, first
    window row, rows <= 4, first window column of a tile of at most 64)."""
    box, use, drange = _stereo_batch_args(box, use, drange)
    out_off = np.zeros(len(box) + 1, np.int64)
    args = (box.ctypes.data, len(box), _ptr(use), int(radius), _ptr(drange))
    out, items = _plan_items(clib.spv_stereo_batch_plan, args, 3, 4, want_items, at=1, tail=(out_off.ctypes.data,))
    plan = dict(pairs=out[0], items=out[1], samples=out[2], out_off=out_off)
    return (plan, items) if want_items else plan


def stereo_batch_into(r0, r1, ri0, ri1, box, use, radius, drange, swap, disp, cost, cost2):
    """One direction of stereo_batch() into caller-allocated flat tensors (spv_stereo_batch_device): disp int32,
    cost and cost2 uint16, at least `samples` elements each; r0, r1, ri0, ri1 exactly `samples`, which refuses the
    rectified values of images with more than one channel.  Asynchronous on the current stream."""
    box, use, drange = _stereo_batch_args(box, use, drange, radius)
    if drange is None:
        raise ValueError("drange is needed")
    samples = _stereo_samples(box)
    for t, dt, name in ((r0, torch.uint8, "r0"), (r1, torch.uint8, "r1"), (ri0, torch.int32, "ri0"), (ri1, torch.int32, "ri1")):
        _need_samples(t, dt, name, samples, exact=True)
    for t, dt, name in ((disp, torch.int32, "disp"), (cost, torch.uint16, "cost"), (cost2, torch.uint16, "cost2")):
        _need_samples(t, dt, name, samples)
    with _on_device_of(r0, r1, ri0, ri1, disp, cost, cost2) as stream:
        check(clib.spv_stereo_batch_device(r0.data_ptr(), r1.data_ptr(), ri0.data_ptr(), ri1.data_ptr(), box.ctypes.data,
                                           len(box), _ptr(use), int(radius), drange.ctypes.data, int(swap),
                                           disp.data_ptr(), cost.data_ptr(), cost2.data_ptr(), stream))


def stereo_batch(r0, r1, ri0, ri1, box, drange, radius=3, use=None, swap=0, both=False):
    """Dense block-matching disparity of every rectified pair of a collection (spv_stereo_batch_device): r0, r1
    (uint8) and ri0, ri1 (int32) the flat outputs of rectify_batch() for gray 8-bit images, box its boxes.  For the
    reference sample (y, x) and every d of drange = (d_lo, d_hi) (one for all pairs, or [npairs, 2]) the cost is the
    sum of absolute differences of the (2 radius + 1)^2 blocks around (y, x) and (y, x + d) of the other image; d is
    admissible where both blocks are inside the window and both centres are valid samples.  Returns flat CUDA tensors
    (disp int32, cost uint16, cost2 uint16): the admissible d of smallest (cost, d), STEREO_NONE where there is none;
    its cost; the smallest cost at |d' - disp| >= 2 (0xFFFF where none).  rectify_batch_view() shows a pair's window
    of any of them.  swap=1 exchanges the roles of the two images (drange as given).  both=True returns
    (result of swap 0, result of swap 1 with the range (-d_hi, -d_lo)).  Asynchronous on the current stream; exactly
    the integers of the numpy statement of the contract."""
    box, use, drange = _stereo_batch_args(box, use, drange, radius)
    if drange is None:
        raise ValueError("drange is needed")
    samples = _stereo_samples(box)
    for t, dt, name in ((r0, torch.uint8, "r0"), (r1, torch.uint8, "r1"), (ri0, torch.int32, "ri0"), (ri1, torch.int32, "ri1")):
        _need_samples(t, dt, name, samples, exact=True)  # (before anything is allocated from them)

    def run(sw, rng):
        out = (torch.empty(samples, dtype=torch.int32, device=r0.device),
               torch.empty(samples, dtype=torch.uint16, device=r0.device),
               torch.empty(samples, dtype=torch.uint16, device=r0.device))
        stereo_batch_into(r0, r1, ri0, ri1, box, use, radius, rng, sw, *out)
        return out
    if not both:
        return run(int(swap), drange)
    return run(0, drange), run(1, np.ascontiguousarray(-drange[:, ::-1]))


def stereo_keep_batch(box, disp0, cost0, cost20, disp1=None, lr_tol=1, uniqueness=10):
    """Which samples of a stereo_batch() result to keep (spv_stereo_keep_batch_device): a flat uint8 CUDA tensor, 1
    where disp0 is a disparity, the left-right check holds -- with disp1, the disp of the swap=1 run: the sample
    x + disp0 of the same row has a disparity there and |disp0 + disp1| <= lr_tol -- and the best cost is unique:
    cost0 * 100 <= cost20 * (100 - uniqueness).  Asynchronous on the current stream."""
    box, _, _ = _stereo_batch_args(box)
    if lr_tol < 0 or not 0 <= uniqueness <= 100:
        raise ValueError("lr_tol must be >= 0 and uniqueness in 0..100")
    samples = _stereo_samples(box)
    _need_samples(disp0, torch.int32, "disp0", samples)
    _need_samples(cost0, torch.uint16, "cost0", samples)
    _need_samples(cost20, torch.uint16, "cost20", samples)
    if disp1 is not None:
        _need_samples(disp1, torch.int32, "disp1", samples)
    kept = torch.empty(samples, dtype=torch.uint8, device=disp0.device)
    with _on_device_of(disp0, cost0, cost20, disp1, kept) as stream:
        check(clib.spv_stereo_keep_batch_device(box.ctypes.data, len(box), disp0.data_ptr(), cost0.data_ptr(),
                                                cost20.data_ptr(), None if disp1 is None else disp1.data_ptr(),
                                                int(lr_tol), int(uniqueness), kept.data_ptr(), stream))
    return kept


def stereo_matches_batch(box, sizes, pairs, disp0, keep, ri0, ri1, capacity=None):
    """The kept samples of every pair as pixel correspondences (spv_stereo_matches_batch_device), pair by pair and
    row-major inside a window: (x0, x1, rows, pair_off) with x0, x1 float64 CUDA [n, 3] = (column, row, 1) of the
    source pixels in image 0 and image 1 of the pair (sizes, pairs as rectify_batch() takes them), rows int32 [n] the
    sample's number inside its window, pair_off an int64 ndarray [npairs + 1] -- what dlt_triangulate_batch() takes,
    with pixel cameras.  The call counts first and reads pair_off back to size the outputs: its one synchronisation.
    With capacity the outputs hold that many rows, only the first capacity matches are written and pair_off still
    reports the true counts."""
    box, _, _ = _stereo_batch_args(box)
    sizes = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, 2)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    if len(pairs) != len(box):
        raise ValueError("box and pairs must hold one entry per pair")
    samples = _stereo_samples(box)
    _need_samples(disp0, torch.int32, "disp0", samples)
    _need_samples(keep, torch.uint8, "keep", samples)
    _need_samples(ri0, torch.int32, "ri0", samples, exact=True)
    _need_samples(ri1, torch.int32, "ri1", samples, exact=True)
    d_off = torch.empty(len(box) + 1, dtype=torch.int64, device=disp0.device)

    def call(cap, x0, x1, rows):
        with _on_device_of(disp0, keep, ri0, ri1, d_off, x0, x1, rows) as stream:
            check(clib.spv_stereo_matches_batch_device(box.ctypes.data, len(box), sizes.ctypes.data, len(sizes),
                                                       pairs.ctypes.data, disp0.data_ptr(), keep.data_ptr(),
                                                       ri0.data_ptr(), ri1.data_ptr(), int(cap),
                                                       None if x0 is None else x0.data_ptr(),
                                                       None if x1 is None else x1.data_ptr(),
                                                       None if rows is None else rows.data_ptr(), d_off.data_ptr(), stream))
    call(0, None, None, None)
    pair_off = d_off.cpu().numpy()  # the call's one synchronisation
    n = int(pair_off[-1]) if capacity is None else int(capacity)
    if n < 0:
        raise ValueError("negative capacity")
    x0 = torch.empty((n, 3), dtype=torch.float64, device=disp0.device)
    x1 = torch.empty((n, 3), dtype=torch.float64, device=disp0.device)
    rows = torch.empty(n, dtype=torch.int32, device=disp0.device)
    if n > 0:
        call(n, x0, x1, rows)
    return x0, x1, rows, pair_off


def sift_into(im, table, count, workspace=None):
    """vlfeat-exact SIFT of im (float32 [H, W] CUDA tensor) into table (float32 [capacity, 132]): rows
    [0, min(n, capacity)) are written and count (int32 [1]) receives the true row count n.
    Asynchronous on the current stream; nothing is synchronised."""
    _need(im, torch.float32, "im")
    _need(table, torch.float32, "table")
    _need(count, torch.int32, "count")
    if im.dim() != 2:
        raise TypeError("Only 2d images are supported.")
    if table.dim() != 2 or table.shape[1] != 132 or count.numel() < 1:
        raise ValueError("table must be [capacity, 132] and count hold one int32")
    hgt, wid = im.shape
    nbytes = clib.spv_sift_workspace_bytes(wid, hgt)
    with _on_device_of(im, table, count) as stream:
        ws = (workspace or _default_ws).get(nbytes, im.device)
        check(clib.spv_sift_device(im.data_ptr(), wid, hgt, ws.data_ptr(), ws.numel(), table.data_ptr(),
                                   table.shape[0], count.data_ptr(), stream))


def sift(im_tensor, workspace=None):
    """vlfeat-exact SIFT on device: im_tensor float32 [H, W] (CUDA).  Returns the float32 [nkp, 132]
    table (x, y, sigma, angle, 128 descriptor values), which split_sift_table and normalize accept.
    Reads the row count back once (a second pass when the first table guess is short)."""
    if not isinstance(im_tensor, torch.Tensor) or im_tensor.dim() != 2:
        raise TypeError("Only 2d images are supported.")
    im = im_tensor.to(torch.float32).contiguous()
    hgt, wid = im.shape
    count = torch.zeros(1, dtype=torch.int32, device=im.device)
    cap = max(1024, min(wid * hgt // 16, 1 << 20))
    for _ in range(2):
        table = torch.empty((cap, 132), dtype=torch.float32, device=im.device)
        sift_into(im, table, count, workspace)
        n = int(count.item())
        if n <= cap:
            return table[:n]
        cap = n
    raise AssertionError("unreachable: the second pass is sized to the true count")


def _sift_sizes(sizes):
    """sizes -> int32[nimg, 2] = (wid, hgt); ValueError for what spv_sift_batch_plan would reject."""
    sz = np.asarray(sizes)
    if sz.size == 0:
        sz = np.zeros((0, 2), np.int32)
    if sz.ndim != 2 or sz.shape[1] != 2 or sz.dtype.kind not in "iu":
        raise ValueError("sizes must be integers of shape [nimg, 2] = (wid, hgt)")
    if sz.size and (int(sz.min()) < 1 or int(sz.max()) > 8192):
        raise ValueError("every image side must be in [1, 8192]")
    return np.ascontiguousarray(sz, dtype=np.int32)


def sift_batch_plan(sizes, ws_bytes=0, want_groups=False):
    """How sift_batch_into() cuts a call into groups for a workspace of ws_bytes (0: as much as needed;
    spv_sift_batch_plan, host only, no device touched): dict of groups, workspace_bytes (with which only the
    65535-image cap closes a group), min_workspace_bytes (the largest image's slice, the least that works) and
    pixels.  With want_groups also int32[groups, 2] = (first image, images)."""
    sz = _sift_sizes(sizes)
    out, groups = _plan_items(clib.spv_sift_batch_plan, (sz.ctypes.data, len(sz), int(ws_bytes)), 4, 2, want_groups)
    plan = dict(groups=out[0], workspace_bytes=out[1], min_workspace_bytes=out[2], pixels=out[3])
    return (plan, groups) if want_groups else plan


def sift_batch_into(images, sizes, table, cap_off, counts, workspace=None):
    """vlfeat-exact SIFT of many images in one chain of launches (spv_sift_batch_device): images float32 CUDA
    tensor holding the images back to back, image i row-major [hgt_i, wid_i] with sizes[i] = (wid_i, hgt_i);
    image i owns rows cap_off[i]:cap_off[i + 1] of table (float32 [cap_off[-1], 132]), of which the first
    min(n_i, capacity_i) are written, and counts (int32 [nimg]) receives the true row counts n_i.  workspace:
    a Workspace, or a uint8 CUDA tensor whose size decides the groups (at least sift_batch_plan's
    min_workspace_bytes).  Asynchronous on the current stream but for the upload of the per-image table."""
    sz = _sift_sizes(sizes)
    cap = col.offsets(cap_off, "cap_off", count=len(sz))
    _need(images, torch.float32, "images")
    _need(table, torch.float32, "table")
    _need(counts, torch.int32, "counts")
    if images.numel() != int((sz[:, 0].astype(np.int64) * sz[:, 1]).sum()):
        raise ValueError("images must hold exactly the pixels of sizes")
    if table.dim() != 2 or table.shape[1] != 132 or table.shape[0] < int(cap[-1]) or counts.numel() < len(sz):
        raise ValueError("table must be [cap_off[-1], 132] and counts hold one int32 per image")
    with _on_device_of(images, table, counts) as stream:
        if isinstance(workspace, torch.Tensor):
            _need(workspace, torch.uint8, "workspace")
            ws = workspace
        else:
            ws = (workspace or _default_ws).get(clib.spv_sift_batch_workspace_bytes(sz.ctypes.data, len(sz)), images.device)
        check(clib.spv_sift_batch_device(images.data_ptr(), sz.ctypes.data, len(sz), ws.data_ptr(), ws.numel(),
                                         table.data_ptr(), cap.ctypes.data, counts.data_ptr(), stream))


def sift_batch_pack(table, cap_off, seg_off, want_packed=True, want_split=False):
    """The regions of a sift_batch_into() table packed back to back (spv_sift_batch_pack_device): rows
    cap_off[i]:cap_off[i] + (seg_off[i + 1] - seg_off[i]) go to rows seg_off[i]:seg_off[i + 1].  Returns the
    wanted ones of (packed float32 [total, 132], geom float32 [total, 4], desc uint8 [total, 128]), geom and desc
    as split_sift_table gives them."""
    _need(table, torch.float32, "table")
    seg = np.ascontiguousarray(seg_off, dtype=np.int64).reshape(-1)
    cap = col.offsets(cap_off, "cap_off", count=seg.size - 1)
    seg = col.offsets(seg, "seg_off")
    total = int(seg[-1])
    packed = torch.empty((total, 132), dtype=torch.float32, device=table.device) if want_packed else None
    geom = torch.empty((total, 4), dtype=torch.float32, device=table.device) if want_split else None
    desc = torch.empty((total, 128), dtype=torch.uint8, device=table.device) if want_split else None
    if not (want_packed or want_split):
        raise ValueError("neither the packed table nor its split is wanted")
    with _on_device_of(table) as stream:
        if total == 0:   # nothing to copy (and an empty tensor has no address to give)
            return ((packed,) if want_packed else ()) + ((geom, desc) if want_split else ())
        check(clib.spv_sift_batch_pack_device(table.data_ptr(), cap.ctypes.data, seg.ctypes.data, seg.size - 1,
                                              packed.data_ptr() if want_packed else None,
                                              geom.data_ptr() if want_split else None,
                                              desc.data_ptr() if want_split else None, stream))
    return ((packed,) if want_packed else ()) + ((geom, desc) if want_split else ())


def sift_batch(images, capacity=None, workspace=None, max_workspace_bytes=None, want_split=False):
    """vlfeat-exact SIFT of a list of 2-D float32 CUDA tensors of any sizes, in one chain of launches.  Returns
    (table float32 [total, 132], seg_off int64 ndarray [n + 1]): image i's table is rows seg_off[i]:seg_off[i + 1],
    bit for bit sift(images[i]); with want_split (geom float32 [total, 4], desc uint8 [total, 128], seg_off)
    instead, what l1k2_batch and match_coordinates_batch take.  capacity: rows reserved per image (an int, or
    one per image; default sift()'s guess).  The counts are read back once; the images whose count exceeded
    their capacity are run again, together, with exact capacities -- the same bits either way.
    max_workspace_bytes caps the scratch (at least the largest image's need), at the price of several groups."""
    n = len(images)
    for im in images:
        if not isinstance(im, torch.Tensor) or im.dim() != 2:
            raise TypeError("Only 2d images are supported.")
    if n == 0:
        raise ValueError("sift_batch needs at least one image")
    sizes = _sift_sizes([(im.shape[1], im.shape[0]) for im in images])
    if capacity is None:
        caps = [max(1024, min(int(w) * int(h) // 16, 1 << 20)) for w, h in sizes]
    else:
        caps = [int(c) for c in np.broadcast_to(np.asarray(capacity, dtype=np.int64), (n,))]
    dev = images[0].device

    def run(which, caps):
        """(table, cap_off, counts on the host) of images[which] with the capacities caps."""
        flat = torch.cat([images[i].to(torch.float32).reshape(-1) for i in which])
        cap_off = col.offsets_of(caps)
        table = torch.empty((int(cap_off[-1]), 132), dtype=torch.float32, device=dev)
        counts = torch.zeros(len(which), dtype=torch.int32, device=dev)
        ws = workspace
        if max_workspace_bytes is not None:
            plan = sift_batch_plan(sizes[which])
            nbytes = max(min(int(max_workspace_bytes), plan["workspace_bytes"]), plan["min_workspace_bytes"])
            buf = workspace if isinstance(workspace, torch.Tensor) else (workspace or _default_ws).get(nbytes, dev)
            ws = buf[:nbytes]
        sift_batch_into(flat, sizes[which], table, cap_off, counts, ws)
        return table, cap_off, counts.cpu().numpy().astype(np.int64)

    every = list(range(n))
    table, cap_off, counts = run(every, caps)
    seg_off = col.offsets_of(counts)
    short = [i for i in every if counts[i] > caps[i]]
    if not short:
        out = sift_batch_pack(table, cap_off, seg_off, want_packed=not want_split, want_split=want_split)
        return out + (seg_off,)
    # the complete regions packed, the short images again with exact capacities, each into its place
    fit = counts.copy()
    fit[short] = 0
    part_off = col.offsets_of(fit)
    table2, cap_off2, counts2 = run(short, [int(counts[i]) for i in short])
    assert np.array_equal(counts2, counts[short])
    parts = sift_batch_pack(table, cap_off, part_off, want_packed=not want_split, want_split=want_split)
    parts2 = sift_batch_pack(table2, cap_off2, cap_off2, want_packed=not want_split, want_split=want_split)
    outs = []
    for a, b in zip(parts, parts2):
        o = torch.empty((int(seg_off[-1]),) + tuple(a.shape[1:]), dtype=a.dtype, device=dev)
        for i in every:
            if i in short:
                k = short.index(i)
                o[seg_off[i]:seg_off[i + 1]] = b[cap_off2[k]:cap_off2[k + 1]]
            else:
                o[seg_off[i]:seg_off[i + 1]] = a[part_off[i]:part_off[i + 1]]
        outs.append(o)
    return tuple(outs) + (seg_off,)
