"""The ctypes prototype of every function include/spectavi_amd.h and include/NdArray.h declare:
PROTOTYPES[name] = (restype, [argtypes]).  This is the one Python statement of the C-ABI; _lib.py
applies it to the library once, and tests/test_abi.py checks every slot against the headers.

What the headers cannot say is chosen here: a numpy array that is checked (dtype, C-contiguity) on
every call, or a plain address (a device pointer, or a host pointer that may be NULL)."""
import ctypes as ct

import numpy as np
from numpy.ctypeslib import ndpointer

from spectavi_amd.ndarray import NdArray

i, f, d, b = ct.c_int, ct.c_float, ct.c_double, ct.c_bool
u32, ll, ull, sz, s = ct.c_uint32, ct.c_longlong, ct.c_ulonglong, ct.c_size_t, ct.c_char_p
vp = ct.c_void_p                       # device pointers, streams, handles, nullable host pointers
vpp = ct.POINTER(ct.c_void_p)          # one device pointer per rank
nd = ct.POINTER(NdArray)               # callee-allocated outputs
pi, pi32, pu64 = ct.POINTER(ct.c_int), ct.POINTER(ct.c_int32), ct.POINTER(ct.c_uint64)
pll, pull, pd, pb = ct.POINTER(ll), ct.POINTER(ull), ct.POINTER(d), ct.POINTER(b)
u8a, i32a, u64a, f32a, f64a = (ndpointer(t, flags="C_CONTIGUOUS")     # host numpy arrays
                               for t in (np.uint8, np.int32, np.uint64, np.float32, np.float64))

_knn = [i, i, i, i, f, f, nd, nd]
_dlt = [f64a, f64a, i, f64a, f64a, f64a]
_dlt_device = [f64a, f64a, ll, vp, vp, vp, vp]
_score_device = [f64a, vp, i, ll, vp, vp, d, vp, vp]
_fit_out = [pi32, f64a, f64a, pd, i32a, pi32, pi32, pi32, pi32]
_ranks = [i, pi, vpp, vpp, i, ll, i]   # ndev, devices, d_x[r], d_y[r], xrows, yrows_total, dim

PROTOTYPES = {
    # ---- NdArray.h
    "ndarray_set_size": (None, [nd, sz, sz]),
    "ndarray_set_size3": (None, [nd, sz, sz, sz]),
    "ndarray_alloc": (i, [nd]),
    "ndarray_free": (None, [nd]),
    # ---- status, configuration, diagnostics
    "spv_last_status": (i, []),
    "spv_last_error": (s, []),
    "spv_device_count": (i, []),
    "spv_set_device": (i, [i]),
    "spv_set_devices": (i, [pi, i]),
    "spv_set_gather_mode": (i, [i]),
    "spv_l1k2_set_prune": (i, [i]),
    "spv_l1k2_get_prune": (i, []),
    "spv_l1k2_prune_stats": (i, [pull]),
    "spv_l1k2_bound_table": (i, [vp, pi, pi]),
    "spv_l1k2_set_bound": (i, [i]),
    "spv_l1k2_get_bound": (i, []),
    "spv_l1k2_set_prune_form": (i, [i]),
    "spv_l1k2_get_prune_form": (i, []),
    "spv_l1k2_prune_form_of": (i, [i, i, i]),
    "spv_l1k2_bound_table_of": (i, [i, vp, pi, pi]),
    "spv_l1k2_set_prune_matrix": (i, [i]),
    "spv_l1k2_get_prune_matrix": (i, []),
    "spv_l1k2_prune_matrix_of": (i, [i, i, i]),
    "spv_l1k2_bound6_table": (i, [vp, pi, pi]),
    "spv_records_pack": (i, [pu64, vp, ll, pi32]),
    "spv_records_unpack": (i, [pi32, ll, i, ll, pu64, vp]),
    "spv_release_cached_memory": (None, []),
    "spv_version": (s, []),
    "spv_profile_enable": (None, [i]),
    "spv_profile_reset": (None, []),
    "spv_profile_read": (i, [s, pll, pd]),
    "spv_microbench_valu": (i, [i, i, i, pd, pd]),
    "spv_microbench_memory": (i, [i, sz, pd]),
    # ---- 1. reference-compatible symbols
    "nn_bruteforcel1k2": (None, [u8a, u8a, i, i, i, i, nd, nd]),
    "nn_bruteforce": (None, [f32a, f32a] + _knn),
    "nn_bruteforcei": (None, [i32a, i32a] + _knn),
    "ann_hnswlib": (None, [f32a, f32a, i, i, i, i, nd]),
    "nn_kmedians": (None, [f32a, f32a] + [i] * 7 + [nd, nd]),
    "kmedians": (None, [f32a, i, i, i]),
    "nn_cascading_hash": (None, [f32a, f32a] + [i] * 7 + [nd, nd]),
    "dlt_triangulate": (None, _dlt),
    "dlt_reprojection_error": (None, _dlt),
    "seven_point_algorithm": (None, [f64a, f64a, pi, f64a]),
    "ransac_fitter": (None, [f64a, f64a, i, d, d, i, b, d, b, pb, nd, nd, pd, nd]),
    "image_pair_rectification": (None, [f64a] * 4 + [i, i, i, d] + [nd] * 4),
    "sift_filter": (None, [f32a, i, i, nd]),
    "sift_filter_batch_create": (vp, []),
    "sift_filter_batch_register_image": (None, [vp, f32a, i, i, nd]),
    "sift_filter_batch_process": (None, [vp, i]),
    "sift_filter_batch_destroy": (None, [vp]),
    # ---- 2. host-pointer variants
    "spv_nn_bruteforcel1k2": (i, [vp, vp, i, i, i, vp, vp]),
    "spv_nn_bruteforcel1k2_batch": (i, [vp, vp, i, i, vp, i, vp, vp]),
    "spv_nn_bruteforcel1k2_guided_batch": (i, [vp, vp, vp, i, i, vp, i, vp, d, vp, vp, vp]),
    "spv_nn_bruteforce": (i, [vp, vp, i, i, i, i, i, f, vp, vp]),
    "spv_ann_l2": (i, [vp, vp, i, i, i, i, i, vp, vp]),
    "spv_nn_cascading_hash": (i, [f32a, f32a] + [i] * 6 + [f32a, u64a, f32a, vp]),
    "spv_nn_cascading_hash_batch": (i, [vp, vp] + [i] * 5 + [vp, i] + [vp] * 4),
    "spv_generate_hash_dict": (i, [u32, i, i, i, f32a]),
    "spv_set_hash_seed": (None, [u32, i]),
    "spv_dlt_score_hypotheses": (i, [f64a, f64a, i, i, f64a, f64a, d, i32a, vp]),
    "spv_ransac_process_candidates": (i, [f64a, i, f64a, f64a, i, d, d, d, i, i32a, i32a, i32a, f64a, f64a, f64a,
                                          i32a, vp]),
    "spv_ransac_workspace_bytes": (sz, [i, ll, i]),
    "spv_ransac_process_candidates_device": (i, [vp, i, ll, vp, vp, d, d, d, i] + [vp] * 9 + [sz, vp]),
    "spv_seven_point": (i, [f64a, f64a, i, i32a, f64a, vp]),
    "spv_seven_point_device": (i, [vp, vp, i, vp, vp, vp, vp]),
    "spv_ransac_sample": (i, [ull, i, i, i32a]),
    "spv_ransac_fit": (i, [f64a, f64a, i, d, d, i, i, d, ull] + _fit_out),
    "spv_ransac_fit_samples": (i, [f64a, f64a, i, d, d, i32a, i, i, d] + _fit_out),
    "spv_ransac_fit_device": (i, [vp, vp, i, d, d, i, i, d, ull, vp] + _fit_out + [vp]),
    "spv_ransac_fit_batch": (i, [vp, vp, vp, i, d, d, i, i, d] + [vp] * 11),
    "spv_ransac_fit_batch_device": (i, [vp, vp, vp, i, d, d, i, i, d] + [vp] * 13),
    "spv_ransac_fit_batch_plan": (i, [vp, i, i, i, pll, vp, ll]),
    "spv_dlt_triangulate_batch": (i, [vp, vp, vp, i] + [vp] * 7 + [ll, vp, vp]),
    "spv_dlt_triangulate_batch_plan": (i, [vp, i, vp, i, pll, vp, ll]),
    "spv_rectify_batch": (i, [vp, i, vp, i, i, d, vp, i, vp, vp, vp, i] + [nd] * 4 + [vp, vp]),
    "spv_rectify_batch_plan": (i, [vp, i, i, d, vp, i, vp, vp, pll, vp, vp, ll]),
    "spv_rectify_shape": (i, [i, i, i, d, i32a]),
    "spv_rectify_fundamental": (i, [f64a, f64a, f64a]),
    "spv_dlt_triangulate": (i, _dlt),
    "spv_dlt_reprojection_error": (i, _dlt),
    # ---- 3. device-pointer variants
    "spv_l1k2_workspace_bytes": (sz, [i, i, i]),
    "spv_l1k2_plan": (i, [i, i, i, pi]),
    "spv_l1k2_device": (i, [vp, vp, i, i, i, vp, vp, vp, sz, vp]),
    "spv_l1k2_batch_plan": (i, [vp, i, i, vp, i, pll, vp, ll]),
    "spv_l1k2_batch_workspace_bytes": (sz, [vp, i, i, vp, i]),
    "spv_l1k2_batch_device": (i, [vp, vp, i, i, vp, i, vp, vp, vp, sz, vp]),
    "spv_l1k2_guided_batch_plan": (i, [vp, i, i, vp, i, pll, vp, ll]),
    "spv_l1k2_guided_batch_workspace_bytes": (sz, [vp, i, i, vp, i]),
    "spv_l1k2_guided_batch_device": (i, [vp, vp, vp, i, i, vp, i, vp, d, vp, vp, vp, vp, sz, vp]),
    "spv_epipolar_lines_batch_device": (i, [vp, vp, i, vp, i, vp, vp, vp, vp]),
    "spv_l1k2_gathered_device":(i, _ranks + [vp, vp, i]),
    "spv_cascade_gathered_device": (i, _ranks + [i, i, i, vpp, vp, vp, vp, i]),
    "spv_dlt_gathered_device": (i, [i, pi, f64a, f64a, ll, vpp, vpp, vp, i, i]),
    "spv_shard_lo": (ll, [ll, i, i]),
    "spv_bruteforce_workspace_bytes": (sz, [i] * 4),
    "spv_bruteforce_device": (i, [vp, vp, i, i, i, i, i, f, i, vp, vp, vp, sz, vp]),
    "spv_ann_l2_workspace_bytes": (sz, [i] * 5),
    "spv_ann_l2_plan": (i, [i] * 6 + [pi]),
    "spv_ann_l2_device": (i, [vp, vp] + [i] * 6 + [vp] * 3 + [sz, vp]),
    "spv_rectify_device": (i, [f64a, vp, vp, i, i, i, i, d, vp, vp, vp, vp, vp]),
    "spv_rectify_batch_bounds_device": (i, [vp, i, i, d, vp, i, vp, vp, vp, vp, vp]),
    "spv_rectify_batch_device": (i, [vp, i, vp, i, i, d, vp, i] + [vp] * 9),
    "spv_sift_filter": (i, [vp, i, i, nd]),
    "spv_sift_table": (i, [f32a, i, i, f32a, i, pi32]),
    "spv_sift_set_first_capacity": (i, [i]),
    "spv_sift_workspace_bytes": (sz, [i, i]),
    "spv_sift_device": (i, [vp, i, i, vp, sz, vp, i, vp, vp]),
    "spv_sift_tables": (i, [vp, vp, i, vp, vp, vp]),
    "spv_sift_batch_plan": (i, [vp, i, sz, pll, vp, ll]),
    "spv_sift_batch_workspace_bytes": (sz, [vp, i]),
    "spv_sift_batch_device": (i, [vp, vp, i, vp, sz, vp, vp, vp, vp]),
    "spv_sift_batch_pack_device": (i, [vp, vp, vp, i, vp, vp, vp, vp]),
    "spv_cascade_workspace_bytes": (sz, [i] * 6),
    "spv_cascade_plan": (i, [i] * 6 + [pi]),
    "spv_cascade_device": (i, [vp, vp] + [i] * 6 + [vp] * 5 + [sz, vp]),
    "spv_cascade_batch_plan": (i, [vp] + [i] * 5 + [vp, i, pll, vp, ll]),
    "spv_cascade_batch_workspace_bytes": (sz, [vp] + [i] * 5 + [vp, i]),
    "spv_cascade_batch_device": (i, [vp, vp] + [i] * 5 + [vp, i] + [vp] * 5 + [sz, vp]),
    "spv_dlt_triangulate_device": (i, _dlt_device),
    "spv_dlt_reprojection_error_device": (i, _dlt_device),
    "spv_dlt_triangulate_batch_device": (i, [vp, vp, vp, i] + [vp] * 7 + [ll, vp, vp, vp]),
    "spv_ratio_test": (i, [u64a, vp, i, i, d, i32a, pi32]),
    "spv_ratio_test_workspace_bytes": (sz, [i]),
    "spv_ratio_test_device": (i, [vp, vp, i, i, d, vp, vp, vp, sz, vp]),
    "spv_sift_split": (i, [f32a, i, f32a, u8a]),
    "spv_sift_split_device": (i, [vp, i, vp, vp, vp]),
    "spv_gather_match_coords_device": (i, [vp] * 4 + [i] + [vp] * 3),
    "spv_gather_match_coords_batch_device": (i, [vp, vp, i, vp, i, vp, vp, i, vp, vp, vp, vp]),
    "spv_tracks_batch_workspace_bytes": (sz, [ll, i]),
    "spv_tracks_batch_device": (i, [vp, i, vp, i, vp, vp, i, vp, i, i] + [vp] * 7 + [sz, vp]),
    "spv_tracks_batch": (i, [vp, i, vp, i, vp, i, vp, i, i] + [vp] * 6),
    "spv_tracks_triangulate_set_long": (i, [i]),
    "spv_tracks_triangulate_get_long": (i, []),
    "spv_tracks_triangulate_plan": (i, [vp, i, pll]),
    "spv_tracks_triangulate_device": (i, [vp, vp, i, vp, vp, vp, i, vp, ll, d] + [vp] * 5),
    "spv_tracks_triangulate": (i, [vp, vp, i, vp, vp, vp, i, vp, ll, d] + [vp] * 4),
    "spv_resect_gather_device": (i, [vp, vp, vp, i, vp, i, vp, vp, i, ll] + [vp] * 6),
    "spv_resect_fit_batch_device": (i, [vp, vp, vp, i, d, d, i, i] + [vp] * 12),
    "spv_resect_fit_batch": (i, [vp, vp, vp, i, d, d, i, i] + [vp] * 11),
    "spv_resect_fit_batch_plan": (i, [vp, i, i, i, pll, vp, ll]),
    "spv_normalize": (i, [f32a, i, i, vp, vp]),
    "spv_normalize_workspace_bytes": (sz, [i]),
    "spv_normalize_workspace_bytes_rows": (sz, [i, i]),
    "spv_normalize_device": (i, [vp, i, i, vp, vp, vp, sz, vp]),
    "spv_normalize_batch_plan": (i, [vp, i, i, i, i, pll, vp, ll]),
    "spv_normalize_batch_workspace_bytes": (sz, [vp, i, i, i]),
    "spv_normalize_batch_device": (i, [vp, i, vp, i, i, vp, vp, vp, sz, vp]),
    "spv_normalize_batch": (i, [vp, i, vp, i, i, vp, vp]),
    "spv_dlt_score_hypotheses_device": (i, _score_device + [vp]),
    "spv_dlt_score_workspace_bytes": (sz, [i, ll]),
    "spv_dlt_score_hypotheses_device_ws": (i, _score_device + [vp, sz, vp]),
}
