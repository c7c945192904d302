/*
 * spectavi_amd.h -- C-ABI of libspectavi.so (MI355X / gfx950 build).
 *
 * Drop-in boundary for the descriptor-matching + DLT hot path of
 * vvhitedog/spectavi.  Section 1 re-exports, symbol for symbol, what the
 * reference's ctypes front-end binds (reference src/Spectavi.cpp, declared to
 * ctypes in spectavi/feature.py and spectavi/mvg.py).  Sections 2 and 3 add
 * status-returning variants with caller-allocated outputs (host pointers) and
 * device-pointer variants (inputs/outputs resident in HBM, asynchronous on a
 * caller stream) used by the benchmark, the tests and multi-GPU sharding.
 *
 * Conventions: row-major C-contiguous arrays, plain pointers and ints, no C++
 * or torch types.  Nothing throws across this boundary (the reference lets
 * std::runtime_error escape extern "C": src/BruteForceNnL1K2.h:75,79).
 * All compute happens in hand-written HIP kernels; there is NO CPU fallback:
 * without a usable gfx950 device every entry point fails with SPV_ERR_HIP.
 */
#ifndef SPECTAVI_AMD_H
#define SPECTAVI_AMD_H

#include <stddef.h>
#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

/* NdArray: the in-repo definition, or -- when libspectavi.so is built with
 * `make NDARRAY_INC=/path/to/ctypes_ndarray/src` -- the reference's own <NdArray.h>
 * (reference src/EigenDefinitions.h:22, CMakeLists.txt:26-27). */
#ifdef SPECTAVI_EXTERNAL_NDARRAY
#include <NdArray.h>
#else
#include "NdArray.h"
#endif

/* libspectavi.so is built with -fvisibility=hidden: only what is declared between this push and
 * the matching pop is exported. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* status                                                                    */
/* ------------------------------------------------------------------------ */
#define SPV_OK 0
#define SPV_ERR_INVALID 1 /* argument rejected (dim % 16, m > 31, k != 2, NULL ...) */
#define SPV_ERR_HIP 2     /* HIP runtime / no device / launch failure */
#define SPV_ERR_NOMEM 3   /* host or device allocation failed */
#define SPV_ERR_INTERNAL 4 /* a C++ exception was caught at the boundary (never propagated) */
#define SPV_ERR_OVERFLOW 5 /* a caller-sized output was too small (the true count is still reported) */

/* Status of the last call made by this thread through any entry point below
 * (the void reference-compatible symbols report errors only this way). */
int spv_last_status(void);
/* Human-readable message for spv_last_status(); valid until the thread's next call. */
const char *spv_last_error(void);
/* Number of visible HIP devices (0 if none / no driver). */
int spv_device_count(void);
/* Device used by the host-pointer entry points of this process (default:
 * environment SPECTAVI_DEVICE, else 0). */
int spv_set_device(int device);
/* Shard the host-pointer entry points over several devices of this node (default:
 * environment SPECTAVI_DEVICES = "0,1,..." or "all", else the single device above).
 * Queries / points are split into contiguous balanced shards, the database is
 * replicated, and each shard is written straight into its slice of the caller's
 * output by a host thread per device; a device may be listed more than once. */
int spv_set_devices(const int *devices, int count);
/* How the shards of a multi-device host-pointer call reach the caller's arrays.
 *   SPV_GATHER_RCCL   every device leaves its (idx0, idx1, d0, d1) records (16 bytes per query;
 *                     DLT: its output rows) in HBM, one ncclCommInitAll clique (cached per device
 *                     list) gathers them on the first listed device with ncclGather, one kernel
 *                     widens them to the ABI layout, one copy brings them to the host -- the
 *                     exchange step of SURVEY 8(e) for the loop the reference shards over OpenMP
 *                     threads (src/BruteForceNnL1K2.h:92-93).  Works with a single device too
 *                     (a clique of one).  Kernel names for spv_profile_read: "gather",
 *                     "gather_widen".  librccl is opened on first use (SPECTAVI_RCCL_LIB overrides
 *                     the name).
 *   SPV_GATHER_PEERCOPY the same records, the same root layout and widening kernel, moved with one
 *                     hipMemcpyPeerAsync per device instead of RCCL (no librccl in the process;
 *                     accepts a device listed more than once).
 *   SPV_GATHER_DIRECT every shard is copied straight into its slice of the caller's arrays; no
 *                     collective.
 *   SPV_GATHER_AUTO   (default) environment SPECTAVI_GATHER = "rccl" | "copy" | "direct" if set,
 *                     else RCCL exactly when more than one distinct device is configured. */
#define SPV_GATHER_AUTO (-1)
#define SPV_GATHER_DIRECT 0
#define SPV_GATHER_RCCL 1
#define SPV_GATHER_PEERCOPY 2
int spv_set_gather_mode(int mode);
/* L1 2-NN at dim 128: whether spv_l1k2_device and everything built on it rule most pairs out with an
 * exact integer lower bound on the matrix cores (l1k2_prune.hip) before the exact distances.  AUTO (the
 * default, also SPECTAVI_L1K2_PRUNE=auto): where the plan's database slices are at least 32768 rows long
 * (from about 512k x 512k rows on; 1M x 1M and 4M x 500k qualify, 256k x 256k does not); ON (=1): wherever the path
 * exists, i.e. dim 128 and at least 32 database rows; OFF (=0): never.  Results are bit-identical
 * either way, and neither spv_l1k2_plan nor spv_l1k2_workspace_bytes depends on it. */
#define SPV_L1K2_PRUNE_AUTO (-1)
#define SPV_L1K2_PRUNE_OFF 0
#define SPV_L1K2_PRUNE_ON 1
int spv_l1k2_set_prune(int mode);
/* The mode in force (the setter's last value, else SPECTAVI_L1K2_PRUNE, else AUTO). */
int spv_l1k2_get_prune(void);
/* Which path the calling thread's last spv_l1k2_device call took: out = {pairs put to the bound,
 * pairs that survived it, pairs evaluated by waves that gave the bound up}; all zero if the tile
 * kernels ran.  Waits for that launch; the workspace it was given must still be allocated. */
int spv_l1k2_prune_stats(unsigned long long out[3]);
/* The bound's table (host only, no GPU involved): phi = the four int8 features of every byte value,
 * and integers p, m with p |a-b| >= m - phi(a).phi(b) for all bytes a, b, m being the largest such. */
int spv_l1k2_bound_table(int8_t phi[256][4], int *p, int *m);
/* Which table the bound runs with.  RECIPE: harmonics 1 and 3 of the cosine series of |a - b|, what
 * spv_l1k2_bound_table returns.  TUNED: the table tools/l1k2_bound_tune.py optimised for the mean bound, which lets
 * about a tenth as many pairs through on uniform bytes; p and m are derived from it at load under the same exhaustive
 * check, and if it ever failed that check the recipe would run in its place.  DEFAULT (also SPECTAVI_L1K2_BOUND unset):
 * TUNED where prune mode AUTO takes the path, RECIPE under prune mode ON.  Results are bit-identical either way. */
#define SPV_L1K2_BOUND_DEFAULT (-1)
#define SPV_L1K2_BOUND_RECIPE 0
#define SPV_L1K2_BOUND_TUNED 1
int spv_l1k2_set_bound(int which);
/* The setting in force (the setter's last value, else SPECTAVI_L1K2_BOUND = 0 | 1, else DEFAULT). */
int spv_l1k2_get_bound(void);
/* Which form of the bound kernel runs where the bound path is taken.  NARROW: 256 queries per workgroup over 32-row
 * database tiles, two workgroups per CU.  WIDE: 512 queries over 64-row tiles, one workgroup per CU, which pays what a
 * tile costs whatever survives half as often.  DEFAULT (also SPECTAVI_L1K2_PRUNE_FORM unset): WIDE where prune mode
 * AUTO takes the path and there are at least 1024 such workgroups (1M x 1M and 4M x 500k qualify), else NARROW; always
 * NARROW under prune mode ON.  Results are bit-identical either way, and neither spv_l1k2_plan nor
 * spv_l1k2_workspace_bytes depends on it. */
#define SPV_L1K2_PRUNE_FORM_DEFAULT (-1)
#define SPV_L1K2_PRUNE_FORM_NARROW 0
#define SPV_L1K2_PRUNE_FORM_WIDE 1
int spv_l1k2_set_prune_form(int form);
/* The setting in force (the setter's last value, else SPECTAVI_L1K2_PRUNE_FORM = 0 | 1, else DEFAULT). */
int spv_l1k2_get_prune_form(void);
/* The form that spv_l1k2_device would run for this shape under the settings in force (host only, no GPU involved):
 * NARROW or WIDE, or -1 where it would not take the bound path at all. */
int spv_l1k2_prune_form_of(int xrows, int yrows, int dim);
/* spv_l1k2_bound_table for either table (which = RECIPE or TUNED). */
int spv_l1k2_bound_table_of(int which, int8_t phi[256][4], int *p, int *m);
/* The matrix format of the WIDE form's bound.  I8: the rank-4 int8 table, 64 v_mfma_i32_32x32x32_i8 per 64-row tile and
 * wave.  FP6: the rank-5 e2m3 table of spv_l1k2_bound6_table, 40 v_mfma_scale_f32_32x32x64_f8f6f4 with unit scales, exact in
 * f32 because every sum is a multiple of 1/64 below 2^24/64.  DEFAULT (also SPECTAVI_L1K2_PRUNE_MATRIX unset or "default";
 * "i8" and "fp6" name the others): FP6 exactly where prune mode AUTO takes the path, the form is WIDE and the bound table
 * setting is DEFAULT; I8 under prune mode ON and with a table named.  FP6 forces it onto every shape whose form is WIDE;
 * the NARROW form is always I8.  Results are bit-identical either way, and neither spv_l1k2_plan nor
 * spv_l1k2_workspace_bytes depends on it. */
#define SPV_L1K2_PRUNE_MATRIX_DEFAULT (-1)
#define SPV_L1K2_PRUNE_MATRIX_I8 0
#define SPV_L1K2_PRUNE_MATRIX_FP6 1
int spv_l1k2_set_prune_matrix(int matrix);
/* The setting in force (the setter's last value, else SPECTAVI_L1K2_PRUNE_MATRIX, else DEFAULT). */
int spv_l1k2_get_prune_matrix(void);
/* The matrix format that spv_l1k2_device would run for this shape under the settings in force (host only, no GPU
 * involved): I8 or FP6, or -1 where it would not take the bound path at all. */
int spv_l1k2_prune_matrix_of(int xrows, int yrows, int dim);
/* The FP6 bound's table (host only, no GPU involved): k = the five e2m3 features of every byte value as the integers k
 * of the values k/8, and integers p, m in units of 1/64 with p |a-b| >= m - k(a).k(b) for all bytes a, b, m being the
 * largest such. */
int spv_l1k2_bound6_table(int8_t k[256][5], int *p, int *m);
/* Host statement of the 16-byte record format (no GPU involved), for callers that run their own
 * collective on raw records.  pack: idx uint64[n,2] ((size_t)-1 = no neighbour), dist32 = int32 or
 * float32 [n,2] -> rec int32[n,4] = (idx0, idx1, d0 bits, d1 bits), -1 = no neighbour.
 * unpack: rec [G][max_cnt][4] in rank order, ragged shards (contiguous balanced split of `total`
 * rows, the first total % G shards one row longer) padded to max_cnt -> idx uint64[total,2],
 * dist32 [total,2]. */
int spv_records_pack(const uint64_t *idx, const void *dist32, long long n, int32_t *rec);
int spv_records_unpack(const int32_t *rec, long long total, int G, long long max_cnt, uint64_t *idx,
                       void *dist32);
/* The host-pointer entry points keep freed device buffers in a per-device cache (up to
 * 4 GiB) for reuse by later calls; this releases them. */
void spv_release_cached_memory(void);
/* Library version string. */
const char *spv_version(void);

/* Optional in-library kernel timing: when enabled, the hot kernels (names:
 * "l1k2_tile", "l1k2_merge", "l1k2_batch", "l1k2_batch_merge", "l1k2_guided", "l1k2_guided_merge", "epipolar_lines", "bruteforce", "bruteforce_merge", "ann_prep", "ann_coarse",
 * "ann_merge", "ann_rerank", "cascade_project",
 * "cascade_buckets", "cascade_probe_refine", "cascade_batch_project", "cascade_batch_buckets", "cascade_batch_probe", "dlt", "dlt_batch", "dlt_batch_scan", "rectify", "rectify_batch_bounds", "rectify_batch_box",
 * "rectify_batch", "stereo_batch", "stereo_keep_batch", "stereo_matches_count", "stereo_matches_fill", "ransac_batch_score",
 * "ransac_batch_reduce",
 * "gather_match_coords_batch", "normalize_batch_stats", "normalize_batch_finish", "normalize_batch", "tracks_init", "tracks_hook",
 * "tracks_flatten", "tracks_sizes", "tracks_scan", "tracks_place", "tracks_order", "tracks_flags",
 * "tracks_triangulate", "tracks_triangulate_long") are bracketed by hipEvents recorded on the
 * stream they are launched on.  spv_profile_read synchronises with the
 * recorded events and returns launch count and summed milliseconds since the
 * last reset. */
void spv_profile_enable(int on);
void spv_profile_reset(void);
int spv_profile_read(const char *kernel, long long *launches, double *total_ms);
/* Diagnostic: sustained issue rate of one VALU instruction with register
 * operands only (op: 0 v_sad_hi_u8, 1 v_sad_u8, 2 v_sad_u16, 3 v_xor+v_add,
 * 4 v_fma_f32, 5 v_dot4_u32_u8, 6 v_med3_u32, 7 v_sub_f32, 8 v_pk_add_f32, 9 v_pk_mul_f32,
 * 10 the correctly rounded sqrtf sequence) and the shader clock held.  A packed instruction
 * counts as one op (two results); op 10 counts one sequence per op. */
int spv_microbench_valu(int op, int blocks, int iters, double *lane_ops_per_s, double *clock_ghz);
/* Diagnostic: memory ceilings.  mode 0 = 16-byte-per-lane streaming copy of table_bytes
 * (bytes read + written per second); mode 1 = random 128-byte row gathers, 8 lanes per row,
 * from a table of table_bytes (bytes gathered per second). */
int spv_microbench_memory(int mode, size_t table_bytes, double *bytes_per_s);

/* ------------------------------------------------------------------------ */
/* 1. Reference-compatible symbols (same names, argument order and meaning)  */
/* ------------------------------------------------------------------------ */

/* Exact L1 (sum |x-y|) 2-nearest-neighbour of every query row y against every
 * database row x.  Replaces reference src/Spectavi.cpp:284-298
 * (BruteForceNnL1K2::find_neighbours<IdentityFilter>, src/BruteForceNnL1K2.h:84-145).
 *   x: uint8[xrows, dim] database, y: uint8[yrows, dim] queries, dim % 16 == 0
 *   (dim <= 2048 on gfx950; wider rows are rejected with SPV_ERR_INVALID).
 *   outidx : callee-allocated size_t[yrows,2]  (col 0 = nearest)
 *   outdist: callee-allocated int  [yrows,2]
 * Result per query = the two smallest (dist, idx) pairs in lexicographic order;
 * missing neighbours (xrows < 2) are (INT_MAX, (size_t)-1) as in the reference
 * (src/BruteForceNnL1K2.h:100-103).  `nthreads` is accepted and ignored (the
 * reference uses it as the OpenMP team size, src/BruteForceNnL1K2.h:92). */
void nn_bruteforcel1k2(const uint8_t *x, const uint8_t *y, int xrows, int yrows, int dim,
                       int nthreads, NdArray *outidx, NdArray *outdist);

/* Exact p-norm k-nearest-neighbour of every query row y against every database row x.
 * Replaces reference src/Spectavi.cpp:258-282 (BruteForceNn::find_neighbours, src/BruteForceNn.h).
 *   x: float32 (nn_bruteforce) or int32 (nn_bruteforcei) [xrows, dim], y: same type [yrows, dim];
 *   outidx: callee-allocated size_t[yrows,k] (col 0 = nearest), outdist: float / int [yrows,k].
 * Distance of (y_i, x_j): s = 0; for c = 0..dim-1 in order: s = s + t_c, every operation rounded on
 * its own (no FMA, no reassociation), with d = float(x - y) (int rows: float(int32(x - y))) and
 *   p == 1: t = |d|   p == 2: t = d*d   p == 0.5: t = sqrtf(|d|) (correctly rounded)
 *   other p: t = float(pow((double)|d|, (double)p))
 * where p is the float argument widened to double; int rows truncate every t to int and sum in
 * int32.  For p in {1, 2, 0.5} the distances are bit-identical to that arithmetic; for other p the
 * device pow may differ from glibc's by an ulp of the double (int rows: a term whose pow lands an
 * ulp below an integer truncates one lower, so a distance may be up to dim units off).  The int domain is: no int32 overflow
 * in x - y, t or s; outside it, and for NaN / inf inputs, the result is unspecified (no fault).
 * Finite inputs are always specified: float32 subnormals are kept (in x - y, t and s), and a distance
 * that overflows to +inf belongs to a real neighbour, which sorts by idx ahead of the missing ones.
 * Result per query: the k smallest (dist, idx) pairs in lexicographic order, ascending -- what the
 * reference's strict-< scan in ascending idx yields where it is defined (it is not on a tie at the
 * k-th place, src/BruteForceNn.h:93-116).  Missing neighbours (xrows < k) fill the end of the row
 * with idx (size_t)-1 and dist +inf (float) / INT_MAX (int); the reference leaves them unwritten.
 * `mu` is accepted and ignored: the result is always exact (with mu <= 0 the reference's prune is
 * exact too; with mu > 0 it is approximate and scan-order dependent).
 * Limits: 1 <= k <= 64, 1 <= dim <= 2048 (any dim), p finite and > 0, xrows, yrows >= 0; outside
 * them SPV_ERR_INVALID and the outputs are not allocated.  One device: the first one selected by
 * spv_set_device / spv_set_devices (sharding over the device list is not implemented). */
void nn_bruteforce(const float *x, const float *y, int xrows, int yrows, int dim, int k, float p, float mu,
                   NdArray *outidx, NdArray *outdist);
void nn_bruteforcei(const int *x, const int *y, int xrows, int yrows, int dim, int k, float p, float mu,
                    NdArray *outidx, NdArray *outdist);

/* Approximate L2 k-nearest-neighbour of every query row y against every database row x, indices only.
 * Takes the place of reference src/Spectavi.cpp:230-241 (src/Hnswlib.h); there is no HNSW graph here: every
 * pair is scored coarsely on the bf16 matrix cores, the ncand best rows of each query are kept, and
 * those are re-ranked exactly.  ann_hnswlib uses the default ncand; spv_ann_l2 (section 2) takes
 * ncand and also returns the distances.
 *   x: float32[xrows, dim] database, y: float32[yrows, dim] queries;
 *   out: callee-allocated size_t[yrows,k] (col 0 = nearest).
 * Limits: 1 <= dim <= 2048, 1 <= k <= 64, xrows, yrows >= 0; ncand = 0 means max(16, 4k), otherwise
 * k <= ncand <= 256; outside them SPV_ERR_INVALID and the outputs are not allocated.  One device: the
 * first one selected by spv_set_device / spv_set_devices, as for nn_bruteforce.
 * 1. Centring: m_c = rintf(mean of column c of x), the mean from a fixed-order reduction (double sums of
 *    1024-row chunks, added in chunk order; no float atomics; a mean that is not finite counts as 0);
 *    x' = bf16(x - m), y' = bf16(y - m), each rounded to nearest even.  L2 is translation invariant;
 *    centring removes the cancellation bf16 cannot carry, and an integer m keeps integer data integer.
 * 2. Coarse score: s(i,j) = n_j - 2 (y'_i . x'_j), n_j = sum_c x'_jc^2 (fp32, column order).  The products
 *    run on the bf16 MFMA with fp32 accumulation in one fixed K order: the bits of s(i,j) depend on the
 *    pair alone, not on tile position, slice count or launch shape; the zero padding of dim (to a
 *    multiple of 32) and of edge tiles is exact.
 * 3. Candidates: per query the ncand smallest keys (s, idx) in lexicographic order, s as the
 *    order-preserving integer image of the float.  If xrows <= ncand every row is a candidate.
 * 4. Re-rank: the exact distance of every candidate from the original float32 rows in nn_bruteforce's
 *    p = 2 arithmetic (d = x - y, t = d*d, s = s + t in column order, each operation rounded on its
 *    own); the result is the k smallest (dist, idx) pairs, ascending.  Missing neighbours are
 *    ((size_t)-1, +inf).
 * Consequences: every returned distance is exact; the result is a function of (x, y, k, ncand) only;
 * candidate sets are nested in ncand, so a larger ncand never gives a larger j-th distance.  Exact
 * domain: when all values of both sides are integers inside one window [a, a+255], and dim <= 128 (or,
 * more generally, every partial sum of products stays below 2^24), steps 1-2 introduce no rounding, s
 * orders the pairs exactly as the true distance does, and the result equals nn_bruteforce(p = 2) bit
 * for bit, even at ncand = k.  With NaN or inf inputs, or scores that overflow, a pair may be missed;
 * the distances that are returned are still exact, and nothing ever faults. */
void ann_hnswlib(const float *x, const float *y, int xrows, int yrows, int dim, int k, NdArray *out);

/* The reference's k-medians exports (src/Spectavi.cpp:300-319), so that its front-end binds against this
 * library alone.  nn_kmedians returns the EXACT L1 k-NN -- nn_bruteforce with p = 1, same outputs and
 * limits -- which is the quantity the reference's randomly seeded cluster filter approximates
 * (src/KMedians.h:260-295); nmx, nmy and c (its cluster counts) are accepted and ignored.  kmedians
 * validates its arguments (x non-NULL, xrows >= 0, dim >= 1, k >= 1: SPV_ERR_INVALID otherwise) and
 * returns: the reference computes a clustering there and discards it.  There is no k-medians
 * clustering in this library. */
void nn_kmedians(const float *x, const float *y, int xrows, int yrows, int dim, int nmx, int nmy, int c, int k,
                 NdArray *outidx, NdArray *outdist);
void kmedians(const float *x, int xrows, int dim, int k);

/* Cascade-hash candidate prefilter + L1 refine.  Replaces reference
 * src/Spectavi.cpp:321-336 (CascadingHashNn, src/CascadingHashNn.h:86-245).
 *   x,y: float32[rows, dim], integer-valued in [-128,127]; dim % 16 == 0, dim <= 2048.
 *   k must be 2 (the reference sizes the buffers by k but writes two columns,
 *   src/Spectavi.cpp:329-335); hash_bit_rate m in [1,31]; num_hash_tables n >= 1;
 *   num_candidate_neighbours g in [0, m].
 *   outidx size_t[yrows,k], outdist float[yrows,k]; queries with fewer than two
 *   candidates carry ((size_t)-1, 2147483648.0f) (src/CascadingHashNn.h:244).
 * Hyperplanes: n matrices float32[dim, m] of N(0,1) drawn from std::mt19937
 * filled dim-major (src/CascadingHashNn.h:86-100); seeded from
 * std::random_device like the reference unless spv_set_hash_seed() /
 * SPECTAVI_HASH_SEED fixed a seed. */
void nn_cascading_hash(const float *x, const float *y, int xrows, int yrows, int dim, int k,
                       int hash_bit_rate, int num_hash_tables, int num_candidate_neighbours,
                       NdArray *outidx, NdArray *outdist);

/* Two-view DLT triangulation of npt points.  Replaces reference
 * src/Spectavi.cpp:38-52 (DltTriangulator::solve, src/DltTriangulator.h:36-65).
 *   P0,P1: double[3,4]; x,xp: double[npt,3] homogeneous; dst: caller double[npt,4].
 * dst row = unit-norm right singular vector of the smallest singular value of
 * the 4x4 DLT matrix; its sign (arbitrary in the reference: Eigen JacobiSVD)
 * is canonicalised to dst[3] >= 0 (first nonzero component > 0 if dst[3]==0). */
void dlt_triangulate(const double *P0, const double *P1, int npt, const double *x,
                     const double *xp, double *dst);

/* Reprojection error of the triangulated point, ||hn(P0 X)-hn(x)|| + ||hn(P1 X)-hn(xp)||.
 * Replaces reference src/Spectavi.cpp:54-68 (src/DltTriangulator.h:67-74).
 * dst: caller double[npt].  +inf and NaN come out exactly where the reference's IEEE arithmetic
 * gives them for the same X (+inf where a squared residual overflows; NaN for w = 0 with x = 0,
 * nan observations, ...), so `err > thr` rejects them.  Both results (here and dlt_triangulate)
 * are the same bits after a row of x or xp is multiplied by +-2^k (whenever the scaled row is
 * exact: |w| up to 2^1023 and subnormal entries included) and after both cameras are multiplied
 * by the same 2^k (|k| <= 200), and do not depend on the point's position in the batch. */
void dlt_reprojection_error(const double *P0, const double *P1, int npt, const double *x,
                            const double *xp, double *dst);

/* The seven-point algorithm: the up to three fundamental matrices through seven correspondences.
 * Replaces reference src/Spectavi.cpp:14-36 (FundamentalMatrixFitter::solve,
 * src/FundamentalMatrixFitter.h:108-246).
 *   x, xp: double[7,2] euclidean image points; *nroot: number of solutions (0..3);
 *   dst: caller double[3,3,3], the first *nroot matrices written (row-major), F = z F0 + (1-z) F1
 *   unnormalised as in the reference, with xp^T F x = 0 for the seven pairs. */
void seven_point_algorithm(const double *x, const double *xp, int *nroot, double *dst);

/* RANSAC fit of the two-view geometry.  Replaces reference src/Spectavi.cpp:70-87
 * (RansacFitter::fit_essential, src/RansacFitter.h:152-272): per try a 7-subset of the
 * correspondences, the seven-point solutions, every solution through
 * process_fundamental_matrix, the best model kept; stops at the first model whose inlier share
 * exceeds required_percent_inliers.
 *   x0, x1: double[npt,3] homogeneous (npt >= 10, as the reference's constructor demands).
 *   *success; essential: callee-allocated double[3,3] = the winning seven-point solution (what the
 *   reference stores, :205); camera: double[3,4]; *inlier_percent; inlier_idx: int32[n,1].
 *   No model kept: essential and inlier_idx are 0 x 0, camera is [I | 0], as in the reference.
 * Tries run in batches on the device and are ranked in try order, i.e. the result is the
 * reference's for nthread = 1 given the same subsets (with OpenMP the reference's own result
 * depends on thread timing).  The subsets come from one std::mt19937 per call, seeded from
 * std::random_device like the reference unless SPECTAVI_RANSAC_SEED is set.  `progressbar` is
 * accepted and ignored. */
void ransac_fitter(const double *x0, const double *x1, int npt, double required_percent_inliers,
                   double reprojection_error_allowed, int maximum_tries, bool find_best_even_in_failure,
                   double singular_value_ratio_allowed, bool progressbar, bool *success, NdArray *essential,
                   NdArray *camera, double *inlier_percent, NdArray *inlier_idx);

/* Epipolar-line rectification of an image pair.  Replaces reference src/Spectavi.cpp:89-119
 * (Rectifier::resample, src/Camera.h:61-445).
 *   P0, P1: double[3,4]; im0, im1: double[hgt, wid, nchan] (nchan = 1: [hgt, wid]).
 *   rectified0/1: callee-allocated double[output_rows, output_cols] (nchan = 1) or
 *   [output_rows, output_cols, nchan]; rectified_idx0/1: int32[output_rows, output_cols].
 * Contract (IEEE double, every operation rounded on its own, sums left to right as written):
 *   F = [P1 C]x P1 P0^T (P0 P0^T)^-1, C the unit null vector of P0, computed once on the host
 *   (spv_rectify_fundamental; its bits are not part of the contract).
 *   Shape (spv_rectify_shape): C = wid*nchan, output_cols = int(sf*C/nchan),
 *   extra_rows = int(max(hgt, C)/2.), output_rows = hgt + 2*extra_rows, rnx = int(sf*wid).
 *   Row r, v = r - extra_rows, x_i = 0. + i*delta with delta = (wid-1)/(rnx-1), i < min(rnx, output_cols):
 *     image 0: l_j = (F[0][j]*0. + F[1][j]*v) + F[2][j], y_i = ((-l_2) - (l_0*x_i)) / l_1;
 *     image 1: the same with m_j = (F[j][0]*x_0 + F[j][1]*y_0) + F[j][2], (x_0, y_0) image 0's
 *     first sample of the row.
 *   A sample is valid iff x > -1 && x < wid && y > -1 && y < hgt (NaN: invalid); then
 *   value = im[(int)y, (int)x, :] copied bit for bit and idx = (int)y*wid + (int)x; otherwise
 *   value 0.0 and idx -1.  Columns [rnx, output_cols) are 0 / -1; samples i >= output_cols are
 *   dropped (the reference writes them past the row).  The reference's column alignment is a no-op
 *   (every shift is 0) and is not reproduced.
 * Defined where the reference is not: a singular P0 P0^T or a non-finite F (F all NaN) and cameras
 * sharing a centre (F = 0) leave every sample invalid.  Rejected with SPV_ERR_INVALID (outputs not
 * allocated): non-finite or non-positive sf, wid, hgt or nchan < 1, hgt*wid or wid*nchan >= 2^31,
 * rnx < 1 or output_cols < 1, output_rows >= 2^31.  One device: the first one selected. */
void image_pair_rectification(const double *P0, const double *P1, const double *im0, const double *im1, int wid,
                              int hgt, int nchan, double sampling_factor, NdArray *rectified0, NdArray *rectified1,
                              NdArray *rectified_idx0, NdArray *rectified_idx1);

/* SIFT keypoints and descriptors of a grayscale image.  Replaces reference src/Spectavi.cpp:130-215
 * (SiftFilter::filter, src/Sift.h:49-129): vlfeat vl_sift_* with every setting at its default,
 * O = max(floor(log2(min(w, h))) - omin - 3, 1), S = 3, omin = -1, peak_thresh = 0,
 * edge_thresh = 10, magnif = 3, norm_thresh = 0.
 *   im: float32[hgt, wid]; out: callee-allocated float32[nkp, 132].  Row: x, y, sigma, angle in
 *   input pixels, then 128 values (uint8) min(512 d, 255).  The clamp is vlfeat's command-line
 *   tool's; the reference's unclamped (vl_uint8) cast is undefined above 255.
 *   Row order is vlfeat's: octave by octave; within an octave the DoG scan order (s, then y, then
 *   x) of the candidates that survive refinement; per keypoint up to four orientations in
 *   histogram-bin order.
 * Contract (IEEE float / double as vlfeat computes them, no contraction; k = 2^(1/3),
 * sigma0 = 1.6 k, dsigma0 = sigma0 sqrt(1 - 1/k^2); f() rounds to float):
 *   Scale space.  Octave -1: upsample along x then y (out[2i] = a[i], out[2i+1] = (a[i]+a[i+1])*0.5f,
 *   the last two samples a[n-1]), then smooth by sqrt(sa^2 - sb^2), sa = sigma0 k^-1, sb = 1.
 *   Level s = 0..4 is level s-1 smoothed by dsigma0 k^s.  Octave o >= 0: level -1 is [::2, ::2]
 *   of level 2 of octave o-1, cropped to (hgt >> o, wid >> o).  Smoothing by sigma: W =
 *   max(ceil(4 sigma), 1), tap j = f(exp(-0.5 (double) f(d d))), d = f(f(j - W) / f(sigma)),
 *   divided by their float sum; vertical pass then horizontal pass, each acc += in[clamp(p)] * tap
 *   in float over p ascending.  Taps are computed on the host with the C library's exp.
 *   Detection.  D[s] = L[s+1] - L[s]; a candidate at s in {0,1,2}, 1 <= x <= w-2, 1 <= y <= h-2
 *   is v >= 0 and strictly above its 26 neighbours, or v <= 0 and strictly below.  Refinement:
 *   vlfeat's five Newton steps in double (Gauss elimination with partial pivoting, pivot below
 *   (double) 1e-10f gives b = 0), moves of one pixel where |b| > 0.6; kept if |val| > 0,
 *   0 <= score < 12.1, every |b| < 1.5, the refined x, y inside the octave and -1 <= s + b2 <= 4.
 *   Stored x = f(xn 2^o), y = f(yn 2^o), sigma = f(sigma0 2^(sn/3) 2^o); these floats feed the
 *   orientation and the descriptor.
 *   Gradients, orientation histogram (36 bins, bilinear, in double, six [1 1 1]/3 passes, peaks
 *   above 0.8 max, at most four) and descriptor (4x4x8 bins, index (by+2)*32 + (bx+2)*8 + bt,
 *   window offsets max(-W, 1-xi) .. min(W, w-xi-2)) follow vlfeat's fast_sqrt, fast_atan2,
 *   mod_2pi and 257-entry fast_expn table (the C library's exp) bit for bit; every bin is a float
 *   (orientation: double) sum over the window in raster order; the norm is a float sum of squares
 *   in index order, divided by fast_sqrt(norm) + FLT_EPSILON, clamped at 0.2f, normalised again.
 *   sin and cos of the angle and pow in sigma are the device's; a last-bit difference from the
 *   C library's can move a value by one float ulp.
 * Every row's descriptor follows the window rule above, for keypoints on the octave's border too
 * (where the reference may leave its descriptor buffer unwritten).
 * Rejected with SPV_ERR_INVALID: wid or hgt < 1 or > 8192.  A constant image gives 0 rows.  One
 * device: the first one selected. */
void sift_filter(const float *im, int wid, int hgt, NdArray *out);

/* Batch form (reference src/Spectavi.cpp:160-215): images and callee-allocated outputs are
 * registered, then processed one after another on the device.  nthread is accepted and ignored.
 * The registered image buffers must stay alive until sift_filter_batch_process returns. */
void *sift_filter_batch_create(void);
void sift_filter_batch_register_image(void *sfb, const float *im, int wid, int hgt, NdArray *out);
void sift_filter_batch_process(void *sfb, int nthread);
void sift_filter_batch_destroy(void *sfb);

/* ------------------------------------------------------------------------ */
/* 2. Host-pointer variants: caller-allocated outputs, int status            */
/* ------------------------------------------------------------------------ */

/* idx: uint64[yrows,2], dist: int32[yrows,2]. */
int spv_nn_bruteforcel1k2(const uint8_t *x, const uint8_t *y, int xrows, int yrows, int dim,
                          uint64_t *idx, int32_t *dist);

/* The L1 2-NN of many (query set, database set) pairs in one call: spv_l1k2_batch_device (section 3, which
 * states the contract) through host pointers.  desc uint8[seg_off[nseg], dim], idx uint64[out_rows,2], dist
 * int32[out_rows,2], out_rows = the query-set rows summed over pairs.  One device: the first one selected by
 * spv_set_device / spv_set_devices (sharding over the device list is not implemented for this form).  An
 * addition: the reference has no such symbol. */
int spv_nn_bruteforcel1k2_batch(const uint8_t *desc, const long long *seg_off, int nseg, int dim,
                                const int32_t *pairs, int npairs, uint64_t *idx, int32_t *dist);

/* spv_l1k2_guided_batch_device (section 3, which states the contract) through host pointers: desc
 * uint8[seg_off[nseg], dim], geom float32[seg_off[nseg], 4], lines double[out_rows, 3], idx uint64[out_rows,2],
 * dist int32[out_rows,2], ncand int32[out_rows] or NULL.  One device: the first one selected by spv_set_device /
 * spv_set_devices.  An addition: the reference has no such symbol. */
int spv_nn_bruteforcel1k2_guided_batch(const uint8_t *desc, const float *geom, const long long *seg_off, int nseg,
                                       int dim, const int32_t *pairs, int npairs, const double *lines,
                                       double max_dist, uint64_t *idx, int32_t *dist, int32_t *ncand);

/* nn_bruteforce (is_int = 0: float32 rows, float32 dist) / nn_bruteforcei (is_int = 1: int32 rows,
 * int32 dist) with caller-allocated idx uint64[yrows,k], dist [yrows,k]. */
int spv_nn_bruteforce(const void *x, const void *y, int is_int, int xrows, int yrows, int dim, int k, float p,
                      uint64_t *idx, void *dist);

/* ann_hnswlib with the candidate count as an argument (0: the default) and the distances: idx
 * uint64[yrows,k], dist float32[yrows,k] or NULL. */
int spv_ann_l2(const float *x, const float *y, int xrows, int yrows, int dim, int k, int ncand, uint64_t *idx,
               float *dist);

/* As nn_cascading_hash but with explicit hyperplanes: dict is
 * float32[n, dim, m] (table-major, then dim, then bit: the fill order of
 * src/CascadingHashNn.h:92-98).  idx: uint64[yrows,2], dist: float32[yrows,2].
 * ncand (may be NULL): int32[yrows] number of candidate rows examined (bucket
 * entries visited; a row reached through several tables counts once per table). */
int spv_nn_cascading_hash(const float *x, const float *y, int xrows, int yrows, int dim, int m,
                          int n, int g, const float *dict, uint64_t *idx, float *dist,
                          int32_t *ncand);

/* The cascade-hash 2-NN of many (query set, database set) pairs in one call: spv_cascade_batch_device (section 3,
 * which states the contract) through host pointers.  rows float32[seg_off[nseg], dim], dict float32[n, dim, m],
 * idx uint64[out_rows,2], dist float32[out_rows,2], ncand (may be NULL) int32[out_rows]; out_rows = the query-set
 * rows summed over pairs.  One device: the first one selected by spv_set_device / spv_set_devices.  An addition:
 * the reference has no such symbol. */
int spv_nn_cascading_hash_batch(const float *rows, const long long *seg_off, int nseg, int dim, int m, int n, int g,
                                const int32_t *pairs, int npairs, const float *dict, uint64_t *idx, float *dist,
                                int32_t *ncand);

/* Fill dict[n*dim*m] exactly as the reference's generate_hash_dict would from
 * std::mt19937(seed) + std::normal_distribution<float>(0,1). */
int spv_generate_hash_dict(uint32_t seed, int dim, int m, int n, float *dict);
/* Fix (use_fixed != 0) or release the seed used by nn_cascading_hash. */
void spv_set_hash_seed(uint32_t seed, int use_fixed);

/* RANSAC hypothesis scoring (the inner loops of reference src/RansacFitter.h:59-95):
 * for each of nhyp candidate second cameras P1s[h] (double[nhyp,3,4]) triangulate all npt
 * correspondences against P0 and count the inliers, i.e. points with
 * reprojection_error() <= max_error that are in front of both cameras
 * (src/DltTriangulator.h:67-86).  counts: int32[nhyp]; mask (may be NULL):
 * uint8[nhyp, npt], 1 = inlier. */
int spv_dlt_score_hypotheses(const double *P0, const double *P1s, int nhyp, int npt,
                             const double *x, const double *xp, double max_error,
                             int32_t *counts, uint8_t *mask);

/* What the reference's RANSAC does with each candidate fundamental matrix,
 * RansacFitter::process_fundamental_matrix (reference src/RansacFitter.h:42-95), batched over nF
 * candidates Fs double[nF,3,3] and all npt correspondences x0, x1 double[npt,3]:
 *   - JacobiSVD of F; gate_ratio = |s0 - s1| / (|s0 + s1| / 2); candidates with
 *     gate_ratio > singular_value_ratio_allowed are rejected (:49-53);
 *   - E = U diag(1,1,0) V^T (:54-56) and its four candidate second cameras, Essential2Cameras
 *     (src/Camera.h:31-46), against the first camera [I | 0];
 *   - every camera scored over all correspondences (spv_dlt_score_hypotheses' rule, :59-73);
 *   - in camera order, a camera becomes the best when its inlier fraction reaches
 *     required_percent_inliers (or find_best_even_in_failure) and exceeds the best so far (:74-84).
 * Outputs per candidate: success int32[nF] (0/1), inlier_count int32[nF], best_camera int32[nF]
 * (0..3 in the order (Ra,t) (Ra,-t) (Rb,t) (Rb,-t), -1 if none); optional (NULL to skip): best_P
 * double[nF,3,4] (zeros if none), gate_ratio double[nF], E double[nF,3,3] (NaN if gated), counts4
 * int32[nF,4] (-1 if gated), inlier_mask uint8[nF,npt] = inliers of the best camera (the
 * reference's inlier_idx, :86-94, as a mask).  The two SVDs run the same two-sided Jacobi iteration
 * as Eigen's JacobiSVD (which of the four cameras comes first depends on its column signs).
 * A candidate with a NaN entry is rejected like a gated one (gate_ratio NaN, counts4 -1). */
int spv_ransac_process_candidates(const double *Fs, int nF, const double *x0, const double *x1, int npt,
                                  double singular_value_ratio_allowed, double required_percent_inliers,
                                  double reprojection_error_allowed, int find_best_even_in_failure,
                                  int32_t *success, int32_t *inlier_count, int32_t *best_camera,
                                  double *best_P, double *gate_ratio, double *E, int32_t *counts4,
                                  uint8_t *inlier_mask);
/* Device form: everything resident in HBM, nF <= 16383 per call, d_ws >=
 * spv_ransac_workspace_bytes(nF, npt, d_inlier_mask != NULL). */
size_t spv_ransac_workspace_bytes(int nF, long long npt, int want_mask);
int spv_ransac_process_candidates_device(const double *d_Fs, int nF, long long npt, const double *d_x0,
                                         const double *d_x1, double singular_value_ratio_allowed,
                                         double required_percent_inliers, double reprojection_error_allowed,
                                         int find_best_even_in_failure, int32_t *d_success,
                                         int32_t *d_inlier_count, int32_t *d_best_camera, double *d_best_P,
                                         double *d_gate_ratio, double *d_E, int32_t *d_counts4,
                                         uint8_t *d_inlier_mask, void *d_ws, size_t ws_bytes, void *stream);

/* Batched seven-point algorithm: x, xp double[n,7,2]; nroot int32[n]; Fs double[n,3,3,3] (slots of
 * missing roots are NaN); basis (may be NULL) double[n,2,3,3], the null-space pair (F0, F1). */
int spv_seven_point(const double *x, const double *xp, int n, int32_t *nroot, double *Fs, double *basis);
int spv_seven_point_device(const double *d_x, const double *d_xp, int n, double *d_Fs, int32_t *d_nroot,
                           double *d_basis, void *stream);

/* ransac_fitter with plain outputs.  seed != 0 fixes the subsets (0: SPECTAVI_RANSAC_SEED if set,
 * else std::random_device); spv_ransac_sample(seed, npt, ntries, samples) writes the very subsets
 * (int32[ntries,7], drawn as the reference's floyd_sample draws them, src/RansacFitter.h:120-132)
 * that spv_ransac_fit(seed) uses, and spv_ransac_fit_samples takes them from the caller.
 *   essential double[9], camera double[12] (untouched if no model was kept), inlier_idx int32[npt]
 *   (first *n_inliers entries); optional (NULL to skip): *best_try / *best_root (-1 if none),
 *   *tries_run (tries actually evaluated: batches end early at the first success). */
int spv_ransac_sample(unsigned long long seed, int npt, int ntries, int32_t *samples);
int spv_ransac_fit(const double *x0, const double *x1, int npt, double required_percent_inliers,
                   double reprojection_error_allowed, int maximum_tries, int find_best_even_in_failure,
                   double singular_value_ratio_allowed, unsigned long long seed, int32_t *success,
                   double *essential, double *camera, double *inlier_percent, int32_t *inlier_idx,
                   int32_t *n_inliers, int32_t *best_try, int32_t *best_root, int32_t *tries_run);
int spv_ransac_fit_samples(const double *x0, const double *x1, int npt, double required_percent_inliers,
                           double reprojection_error_allowed, const int32_t *samples, int ntries,
                           int find_best_even_in_failure, double singular_value_ratio_allowed, int32_t *success,
                           double *essential, double *camera, double *inlier_percent, int32_t *inlier_idx,
                           int32_t *n_inliers, int32_t *best_try, int32_t *best_root, int32_t *tries_run);
/* The correspondences already in HBM (d_x0, d_x1 double[npt,3] on the caller's current device, e.g.
 * what spv_gather_match_coords_device left there): samples (host int32[maximum_tries,7]) or, if
 * NULL, the seed choose the subsets; the small results come back to host memory.  Synchronises
 * `stream` after every batch of tries (the loop stops at the first success). */
int spv_ransac_fit_device(const double *d_x0, const double *d_x1, int npt, double required_percent_inliers,
                          double reprojection_error_allowed, int maximum_tries, int find_best_even_in_failure,
                          double singular_value_ratio_allowed, unsigned long long seed, const int32_t *samples,
                          int32_t *success, double *essential, double *camera, double *inlier_percent,
                          int32_t *inlier_idx, int32_t *n_inliers, int32_t *best_try, int32_t *best_root,
                          int32_t *tries_run, void *stream);

/* spv_ransac_fit_samples for every set of a collection of correspondence sets, in one call (ransac_batch.hip):
 * what a multi-view front-end runs after the matches of its image pairs have become coordinates.
 *   x0, x1   double[total, 3]: the homogeneous correspondences of npairs sets back to back (the device form:
 *            on the caller's current device).
 *   pair_off host long long[npairs + 1], pair_off[0] = 0, non-decreasing, pair_off[npairs] = total < 2^31; set p
 *            is rows [pair_off[p], pair_off[p + 1]).  npairs <= 2^20.
 *   required_percent_inliers ... singular_value_ratio_allowed: as in spv_ransac_fit, one value for all sets.
 *   samples  host int32[npairs, maximum_tries, 7], row numbers inside the set; or, if NULL,
 *   seeds    host unsigned long long[npairs]: set p evaluates the subsets spv_ransac_sample(seeds[p], rows of p,
 *            maximum_tries) returns (an entry 0: the environment seed, else std::random_device).
 * Host outputs, one row per set: success int32[npairs], essential double[npairs, 9], camera double[npairs, 12]
 * (both rows untouched where no model was kept), inlier_percent double[npairs], n_inliers int32[npairs], and --
 * NULL to skip -- best_try, best_root, tries_run int32[npairs].  inlier_idx host int32[total]: set p's list is
 * inlier_idx[pair_off[p] .. pair_off[p] + n_inliers[p]), row numbers inside the set, ascending.  d_inlier_mask
 * (device form, may be NULL) uint8[total]: 1 = inlier of its set's kept model, 0 elsewhere, every byte written.
 *
 * A set with fewer than 10 rows is skipped, not an error: success 0, inlier_percent 0, n_inliers 0, best_try =
 * best_root = -1, tries_run 0; its samples are not read.  npairs = 0 and maximum_tries = 0 are valid.
 * SPV_ERR_INVALID, nothing launched and no output touched: a NULL required pointer, a pair_off that does not
 * follow the rules above, maximum_tries < 0 or > 7e8, a sample row outside its set.
 *
 * For every set, success, essential, camera, inlier_percent, n_inliers, the inlier list, best_try and best_root
 * are bit for bit what spv_ransac_fit_samples returns for that set alone with the same subsets, whatever else the
 * collection holds and however the call cuts the work.  tries_run -- the number of leading tries of the set that
 * were evaluated -- depends on the cuts: best_try < tries_run <= maximum_tries for a set that succeeds,
 * maximum_tries for one that runs and does not.
 *
 * The call works in rounds: every set that is still running contributes its next block of tries, and `stream`
 * is synchronised once per round, however many sets there are.  Scratch comes from the library's cache
 * (spv_release_cached_memory).  One device: the host form runs on the first selected device and touches none if
 * no set has 10 rows or maximum_tries is 0.  Kernel names for spv_profile_read: "ransac_batch_score" (the
 * segmented scorer and its second pass), "ransac_batch_reduce"; "seven_point" and "ransac_cameras" as elsewhere.
 *
 * spv_ransac_fit_batch_plan: host only, touches no device.  The first round of such a call on a device of
 * compute_units compute units: out = {sets in the round, tries in the round, work items, row blocks of 256};
 * items may be NULL, otherwise int32[items_cap, 5] receives the first min(work items, items_cap) work items, one
 * workgroup each, as (set, first row in x0 / x1, rows <= 256, first candidate of the round, candidates; a try
 * has 3 candidates).  An item never straddles two sets; a set's candidates are cut over several items while the
 * round has fewer than 4 row blocks per compute unit. */
int spv_ransac_fit_batch(const double *x0, const double *x1, const long long *pair_off, int npairs,
                         double required_percent_inliers, double reprojection_error_allowed, int maximum_tries,
                         int find_best_even_in_failure, double singular_value_ratio_allowed, const int32_t *samples,
                         const unsigned long long *seeds, int32_t *success, double *essential, double *camera,
                         double *inlier_percent, int32_t *inlier_idx, int32_t *n_inliers, int32_t *best_try,
                         int32_t *best_root, int32_t *tries_run);
int spv_ransac_fit_batch_device(const double *d_x0, const double *d_x1, const long long *pair_off, int npairs,
                                double required_percent_inliers, double reprojection_error_allowed, int maximum_tries,
                                int find_best_even_in_failure, double singular_value_ratio_allowed,
                                const int32_t *samples, const unsigned long long *seeds, int32_t *success,
                                double *essential, double *camera, double *inlier_percent, int32_t *inlier_idx,
                                int32_t *n_inliers, int32_t *best_try, int32_t *best_root, int32_t *tries_run,
                                uint8_t *d_inlier_mask, void *stream);
int spv_ransac_fit_batch_plan(const long long *pair_off, int npairs, int maximum_tries, int compute_units,
                              long long out[4], int32_t *items, long long items_cap);

/* dlt_triangulate and dlt_reprojection_error for every set of a collection of correspondence sets, in one call
 * (dlt_batch.hip), each set with its own camera pair: the step after spv_ransac_fit_batch -- the reference's
 * RX = dlt_triangulate(P0, ransac['camera'], x0[idx], x1[idx]) for every image pair at once, with the fits' cameras
 * as P1s and the fit's d_inlier_mask as the selection.  spv_dlt_triangulate_batch_device is in section 3.
 *   x0, x1   double[total, 3]: the homogeneous correspondences of npairs sets back to back (the device form:
 *            on the caller's current device).
 *   pair_off host long long[npairs + 1]: the rules of spv_ransac_fit_batch.
 *   P1s      host double[npairs, 12]: the second camera of every set.
 *   P0s      host double[npairs, 12]: the first camera of every set; NULL: [I | 0] for every set, the frame the
 *            cameras of spv_ransac_fit_batch are expressed in.
 *   use      host int32[npairs], or NULL for all sets: a set with use[p] = 0 is skipped -- its cameras are not read
 *            and it owns no out rows --, which is what a fit that kept no model becomes.
 *   mask     uint8[total] (the device form: device memory), or NULL for all rows: a row is selected iff its byte
 *            is non-zero and its set is used.
 * The selected rows are written back to back, in ascending input-row order: out rows [0, min(count, capacity)) of
 * X double[capacity, 4] (dlt_triangulate's unit-norm points), err double[capacity] (dlt_reprojection_error's values)
 * and rows int32[capacity] (the row number inside its set, the numbering of spv_ransac_fit_batch's inlier_idx).
 * Each of the three may be NULL, but not both X and err; nothing at or beyond min(count, capacity) is touched.
 * out_off long long[npairs + 1] (may be NULL): the selected rows before every set, out_off[npairs] = *count (may be
 * NULL) = the number of selected rows, also where it exceeds capacity -- the host form then returns
 * SPV_ERR_OVERFLOW with the rows that fit written; the device form cannot know and returns SPV_OK.
 *
 * For every selected row, X is bit for bit what spv_dlt_triangulate_device writes for that row with its set's
 * cameras and err what spv_dlt_reprojection_error_device writes, whatever else the collection holds and however the
 * call cuts the work; rows with inf, NaN or w = 0 included.
 *
 * SPV_ERR_INVALID, nothing launched and no output touched: a NULL required pointer, a pair_off outside the rules,
 * negative capacity.  npairs = 0, empty sets and a collection without a used set are valid: the host form then
 * touches no device (the device form only sets d_out_off and d_count to zero).
 *
 * The device form is asynchronous on `stream` but for the upload of its small tables (the cameras and the work
 * items); with a mask the out rows' places are counted on the device, without one the host computes them and
 * nothing but the one kernel runs.  Scratch comes from the library's cache (spv_release_cached_memory) and goes
 * back to it once the call's last kernel has ended.  One device: the host form runs on the first selected device.
 * Kernel names for spv_profile_read: "dlt_batch" (the solve), "dlt_batch_scan" (count and scan, with a mask).
 * Very large single sets remain the job of spv_dlt_triangulate_device, whose lanes stream their rows ahead of the
 * solve.
 *
 * spv_dlt_triangulate_batch_plan: host only, touches no device.  out = {used sets, work items, rows of the used
 * sets (the most a mask can select)}; items may be NULL, otherwise int32[items_cap, 4] receives the first
 * min(work items, items_cap) work items, one workgroup's step each, in launch order, as (set, first row in x0 / x1,
 * rows <= 256, out row of the first row where the call has no mask -- with a mask the device counts, and the call's
 * own table holds -1).  An item never straddles two sets and a set that is not used owns none.  compute_units >= 1
 * caps the grid (32 workgroups per unit, each walking items b, b + grid, ...) and does not change the items. */
int spv_dlt_triangulate_batch(const double *x0, const double *x1, const long long *pair_off, int npairs,
                              const double *P0s, const double *P1s, const int32_t *use, const uint8_t *mask, double *X,
                              double *err, int32_t *rows, long long capacity, long long *out_off, long long *count);
int spv_dlt_triangulate_batch_plan(const long long *pair_off, int npairs, const int32_t *use, int compute_units,
                                   long long out[3], int32_t *items, long long items_cap);

/* The output shape of image_pair_rectification: out = {output_rows, output_cols, rnx}.  Host only;
 * SPV_ERR_INVALID (out untouched) for the arguments image_pair_rectification rejects. */
int spv_rectify_shape(int wid, int hgt, int nchan, double sf, int out[3]);
/* The fundamental matrix image_pair_rectification resamples with, F double[3,3] row-major (all NaN
 * for a singular P0 P0^T, zero for cameras sharing a centre).  Host only. */
int spv_rectify_fundamental(const double *P0, const double *P1, double *F);

/* image_pair_rectification for every pair of a collection of image pairs, cropped on the device (rectify_batch.hip):
 * the last step of a view set's pipeline in the form of the other many-pairs calls.  Two device steps -- the
 * bounding box of every pair's valid samples, then the resampling of only that window of the four outputs, all pairs
 * packed back to back -- with one host synchronisation between them however many pairs there are.  The device forms
 * spv_rectify_batch_bounds_device and spv_rectify_batch_device are in section 3.
 *   sizes    host int32[nimg, 2] = (wid, hgt) of every image.
 *   images   the images back to back in that order, each [hgt, wid, nchan] (the device form: d_images, on the
 *            caller's current device) -- for nchan = 1 exactly what spv_sift_batch_device takes.
 *   dtype    SPV_RECTIFY_F64, SPV_RECTIFY_U8 or SPV_RECTIFY_F32 (float32 images, this call only): values are
 *            copied as integers of their width, so NaN payloads and -0.0 pass through.  Images and outputs are
 *            aligned to their element size.
 *   nchan >= 1 and sampling_factor: one value each for the call.
 *   pairs    host int32[npairs, 2] = (image 0, image 1) of every pair, numbers in [0, nimg).  Repeats are allowed
 *            and an image may appear in many pairs; the two images of a pair have the same size.  The matcher's
 *            pair (query set, database set) is passed here as (database, query): x0 -- the coordinates the cameras
 *            of spv_ransac_fit_batch map with [I | 0] -- comes from the database view.
 *   P0s      host double[npairs, 12], or NULL for [I | 0] for every pair; P1s host double[npairs, 12].
 *   use      host int32[npairs], or NULL for all pairs: a pair with use[p] = 0 has its cameras unread, the box
 *            (0, 0, 0, 0) and owns no output.
 * F of every pair is spv_rectify_fundamental(P0, P1), computed on the host.  The uncropped frame of pair p is
 * spv_rectify_shape(wid, hgt, nchan, sf) of its images; box[p] = (row_lo, row_hi, col_lo, col_hi), half-open, in
 * that frame, is the pair's window.
 *
 * Bounds (spv_rectify_batch_bounds_device): d_box int32[npairs, 4] receives, for every pair, the bounding box of the
 * samples with ri0 != -1 || ri1 != -1 under the sample rule of image_pair_rectification (section 1) -- what the
 * front-end's crop_invalid keeps --, or (0, 0, 0, 0) where there is none: F all NaN or zero, rnx = 1, or a pair
 * that is not used.  No image is read.  Every sample of every other pair is evaluated, in items of 16 frame rows of
 * one pair (one workgroup's step each, over the capped grid of the resampling step); the partial results are
 * combined with integer minima and maxima, so the result does not depend on their order.
 *
 * Plan (spv_rectify_batch_plan): host only, touches no device.  box: host int32[npairs, 4], or NULL for every used
 * pair's whole frame (the entries of pairs that are not used are not read).  out = {used pairs, work items, total
 * window samples}.  out_off long long[npairs + 1]: pair p owns samples [out_off[p], out_off[p + 1]) of the outputs,
 * its window in row-major order, (row_hi - row_lo) * (col_hi - col_lo) samples.  items may be NULL, otherwise
 * int32[items_cap, 4] receives the first min(work items, items_cap) work items, exactly the list the device call
 * walks, in its order: (pair, image 0 or 1 of the pair, first row in the pair's frame, rows <= 8), one workgroup's
 * step each -- pair by pair, the row blocks of image 0 then those of image 1.  Together they cover every window row
 * of both images exactly once; an item never straddles two pairs and a window without a sample owns none.
 * SPV_ERR_INVALID, outputs untouched: what spv_rectify_shape rejects for any image, image numbers outside
 * [0, nimg), a pair of unequal sizes, a box outside its frame or with lo > hi, negative counts, more than 2^20
 * pairs, a NULL required pointer.  npairs = 0 and a collection without a used pair are valid.
 *
 * Resample (spv_rectify_batch_device): box as for the plan, a HOST array.  d_r0, d_r1 hold
 * dtype[out_off[npairs] * nchan], d_ri0, d_ri1 int32[out_off[npairs]].  Every element of every window is written
 * exactly once, the padding columns [rnx, cols) included, and nothing else is touched.  For every pair the window
 * is bit for bit the slice [row_lo:row_hi, col_lo:col_hi] of what spv_rectify_device writes for that pair alone
 * with the same F (float32: of what it writes for the images widened to double, narrowed again), whatever else the
 * collection contains and however the call cuts the work; the index is the flat index inside the pair's own image.
 * Asynchronous on `stream` but for the upload of its small per-pair and item tables, which live in the library's
 * cache (spv_release_cached_memory) and go back to it once the call's last kernel has ended.  One launch for the
 * whole collection, its grid capped at 32 workgroups per compute unit, each walking items b, b + grid, ...
 * Kernel names for spv_profile_read: "rectify_batch_bounds" (one launch per bounds call, followed by
 * "rectify_batch_box", which turns the minima and maxima into boxes), "rectify_batch" (one launch per resample).
 *
 * spv_rectify_batch: the host-pointer form, on the first selected device.  crop != 0 runs the bounds step and reads
 * the boxes back (the one synchronisation); crop = 0 takes whole frames.  rectified0/1: callee-allocated
 * [out_off[npairs] * nchan, 1] of the dtype (the NdArray's item size must be the dtype's), rectified_idx0/1:
 * int32[out_off[npairs], 1].  box int32[npairs, 4] and out_off long long[npairs + 1] are caller arrays the call
 * fills.  A pair without a valid sample has an empty box and owns no output; that is no error.  No device is
 * touched when no pair is used. */
#define SPV_RECTIFY_F64 0
#define SPV_RECTIFY_U8 1
#define SPV_RECTIFY_F32 2
int spv_rectify_batch(const void *images, int dtype, const int32_t *sizes, int nimg, int nchan, double sampling_factor,
                      const int32_t *pairs, int npairs, const double *P0s, const double *P1s, const int32_t *use,
                      int crop, NdArray *rectified0, NdArray *rectified1, NdArray *rectified_idx0,
                      NdArray *rectified_idx1, int32_t *box, long long *out_off);
int spv_rectify_batch_plan(const int32_t *sizes, int nimg, int nchan, double sampling_factor, const int32_t *pairs,
                           int npairs, const int32_t *use, const int32_t *box, long long out[3], long long *out_off,
                           int32_t *items, long long items_cap);

int spv_dlt_triangulate(const double *P0, const double *P1, int npt, const double *x,
                        const double *xp, double *dst);
int spv_dlt_reprojection_error(const double *P0, const double *P1, int npt, const double *x,
                               const double *xp, double *dst);

/* ------------------------------------------------------------------------ */
/* 3. Device-pointer variants: everything resident in HBM, async on `stream` */
/*    (`stream` is a hipStream_t passed as void*; NULL = the null stream).    */
/*    Buffers must belong to the calling thread's current HIP device.         */
/* ------------------------------------------------------------------------ */

/* Scratch bytes needed by spv_l1k2_device for this shape.  At dim 128 with at least 32 database rows this
 * includes 512 bytes per database row and per query row for the int8 features of the bound path
 * (spv_l1k2_set_prune), whether or not the path is switched on: the size depends on the shape alone.
 * That is about five times the input (1.0 GB more at 1M x 1M). */
size_t spv_l1k2_workspace_bytes(int xrows, int yrows, int dim);
/* The launch plan spv_l1k2_device follows for this shape (on one device; the host-pointer entry
 * points shard the queries over the devices first): out = {kernel row width in bytes, queries per
 * lane, database slices, rows per slice, 1 if the wide-row kernel runs else 0}.  The
 * SPECTAVI_L1K2_Q / SPECTAVI_L1K2_BLOCKS overrides are applied.  Host only, touches no device.
 * SPV_ERR_INVALID (out untouched) for a shape the kernels do not take. */
int spv_l1k2_plan(int xrows, int yrows, int dim, int out[5]);
/* d_x uint8[xrows,dim], d_y uint8[yrows,dim] (16-byte aligned bases),
 * d_idx uint64[yrows,2], d_dist int32[yrows,2], d_ws >= workspace bytes. */
int spv_l1k2_device(const uint8_t *d_x, const uint8_t *d_y, int xrows, int yrows, int dim,
                    uint64_t *d_idx, int32_t *d_dist, void *d_ws, size_t ws_bytes,
                    void *stream);

/* The exact L1 2-NN of a collection of descriptor-set pairs, one main launch for all of them (l1k2_batch.hip):
 * what a multi-view front-end runs between "SIFT for N images" and "geometry per image pair".
 *   desc     uint8[total_rows, dim]: the tables of nseg descriptor sets back to back.
 *   seg_off  host long long[nseg + 1], non-decreasing, seg_off[0] = 0, seg_off[nseg] = total_rows < 2^31; set s is
 *            rows [seg_off[s], seg_off[s + 1]) and may be empty.
 *   pairs    host int32[npairs, 2] = (query set, database set), in any order, repeats allowed, a set may be
 *            paired with itself (no self-exclusion: a row then finds itself at distance 0, as
 *            nn_bruteforcel1k2(x, x) does).
 *   idx      uint64[out_rows, 2], dist int32[out_rows, 2]; out_rows = the query-set row counts summed over pairs.
 *            Pair p owns the rows from the sum over the pairs before it, in query-row order; idx is the row
 *            number inside the database set; missing neighbours are ((size_t)-1, INT_MAX).
 * Per pair the rows are bit for bit what spv_l1k2_device(database set, query set) writes: the two smallest
 * (dist, idx) in lexicographic order, whatever way the call cuts the work.  Limits: dim a positive multiple of
 * 16 and <= 256, the widths of the tile kernels (widths without a kernel of their own are zero-padded once, for
 * the whole of desc, into the workspace; dim > 256 is SPV_ERR_INVALID in this form), nseg >= 0, npairs >= 0, set
 * numbers in [0, nseg), d_desc and d_ws 16-byte aligned, d_idx 8-byte, d_dist 4-byte.  Outside them
 * SPV_ERR_INVALID, nothing launched, no output touched.  One device.  Very large single pairs remain the job of
 * spv_l1k2_device (its bound path from 512k rows on is not taken here).
 *
 * spv_l1k2_batch_plan: host only, touches no device.  out = {kernel row width in bytes, queries per lane, work
 * items, out_rows, largest slice count of any pair, workspace bytes}; items may be NULL, otherwise int32[items_cap, 5]
 * receives the first min(work items, items_cap) work items, one workgroup each, as (pair, first query row within
 * the query set, query rows, first database row within the database set, database rows): exactly the list the
 * device call launches, in its order.  The SPECTAVI_L1K2_Q / SPECTAVI_L1K2_BLOCKS overrides are applied.
 * SPV_ERR_INVALID leaves out and items untouched.  spv_l1k2_batch_workspace_bytes: out[5] (0 for arguments the
 * plan rejects): 16 bytes per out row, 32 per work item, the padded desc if any; it does not grow with the slice count.
 *
 * spv_l1k2_batch_device: seg_off and pairs are read before the call returns.  The call may wait for the upload
 * of its small work table, which is queued on `stream`; it never waits for its kernels, and everything else is
 * asynchronous on `stream`.  Kernel names for spv_profile_read: "l1k2_batch" (the main kernel, one launch per
 * call), "l1k2_batch_merge" (keys to idx / dist).  spv_ratio_test and spv_ratio_test_device apply to the
 * concatenated output as it stands: their matches are (out row, row within the database set). */
int spv_l1k2_batch_plan(const long long *seg_off, int nseg, int dim, const int32_t *pairs, int npairs,
                        long long out[6], int32_t *items, long long items_cap);
size_t spv_l1k2_batch_workspace_bytes(const long long *seg_off, int nseg, int dim, const int32_t *pairs,
                                      int npairs);
int spv_l1k2_batch_device(const uint8_t *d_desc, const long long *seg_off, int nseg, int dim,
                          const int32_t *pairs, int npairs, uint64_t *d_idx, int32_t *d_dist, void *d_ws,
                          size_t ws_bytes, void *stream);

/* The guided pass of a multi-view front-end (l1k2_guided.hip): the exact L1 2-NN of spv_l1k2_batch_device, searched
 * for every query only among the database keypoints within max_dist of that query's line -- its epipolar line
 * once a model is fitted, or the scan line (0, 1, -v) of a rectified pair.  The two nearest rows inside the band
 * are in general not the two nearest overall, so this is not a filter over spv_l1k2_batch_device's result.
 *   desc, seg_off, pairs, idx, dist, out_rows
 *            as for spv_l1k2_batch_device, rule for rule.
 *   geom     float32[total_rows, 4]: row for row the geometry of desc, as spv_sift_split_device writes it; only
 *            columns 0 and 1 (u, v) are read.
 *   lines    double[out_rows, 3]: row r is the line (l0, l1, l2) of out row r in the database view's pixel
 *            coordinates.
 *   Candidates: row j of the pair's database set, keypoint (u_j, v_j), is a candidate of out row r iff
 *            fabs(fma(l0, (double)u_j, fma(l1, (double)v_j, l2))) <= max_dist, in fp64 and in that operation
 *            order.  A NaN anywhere makes the comparison false: a NaN line or a NaN keypoint yields no candidate.
 *            Nothing is normalised inside: max_dist is in pixels when the lines have l0^2 + l1^2 = 1.
 *   Result:  the two smallest (L1 distance, row within the database set) among the candidates, in lexicographic
 *            order, ((size_t)-1, INT_MAX) where fewer than two candidates exist; bit for bit the same however the
 *            call cuts the work.  ncand (may be NULL): int32[out_rows], the number of candidates of each out row.
 * Limits: dim == 128 only in this form (any other width is SPV_ERR_INVALID); d_desc, d_geom and d_ws 16-byte
 * aligned, d_idx and d_lines 8-byte, d_dist and d_ncand 4-byte; d_lines and d_geom may be NULL only when there are
 * no out rows.  Outside them SPV_ERR_INVALID, nothing launched, no output touched.  One device.
 *
 * spv_l1k2_guided_batch_plan: host only, touches no device.  out = {work items, out_rows, largest slice count of
 * any pair, workspace bytes}; items may be NULL, otherwise int32[items_cap, 5] receives the first min(work items,
 * items_cap) work items, one workgroup each, as (pair, first query row within the query set, query rows, first
 * database row within the database set, database rows), in launch order.  An item is up to 256 queries against one
 * slice of the database set: a collection of at least 512 query blocks runs whole sets, a smaller one is cut into
 * slices of at least 256 rows until it has 512 items.  SPV_ERR_INVALID leaves out and items untouched.
 * spv_l1k2_guided_batch_workspace_bytes: out[3] (0 for arguments the plan rejects): 16 bytes per out row, 32 per
 * work item.
 *
 * spv_l1k2_guided_batch_device: seg_off and pairs are read before the call returns.  The call may wait for the
 * upload of its small work table, which is queued on `stream`; everything else is asynchronous on `stream`.
 * Kernel names for spv_profile_read: "l1k2_guided" (the main kernel), "l1k2_guided_merge" (keys to idx / dist). */
int spv_l1k2_guided_batch_plan(const long long *seg_off, int nseg, int dim, const int32_t *pairs, int npairs,
                               long long out[4], int32_t *items, long long items_cap);
size_t spv_l1k2_guided_batch_workspace_bytes(const long long *seg_off, int nseg, int dim, const int32_t *pairs,
                                             int npairs);
int spv_l1k2_guided_batch_device(const uint8_t *d_desc, const float *d_geom, const long long *seg_off, int nseg,
                                 int dim, const int32_t *pairs, int npairs, const double *d_lines, double max_dist,
                                 uint64_t *d_idx, int32_t *d_dist, int32_t *d_ncand, void *d_ws, size_t ws_bytes,
                                 void *stream);

/* The lines of spv_l1k2_guided_batch_device from one 3x3 matrix per pair.  G is host double[npairs, 9], row major;
 * G_p maps a pixel of the query view to its line in the database view: out row r of pair p, whose query keypoint
 * is (u, v) (geom of the query set), gets l = G_p (u, v, 1)^T divided by hypot(l0, l1).  use is host int32[npairs]
 * or NULL; three NaNs are written where use[p] == 0 or the norm is zero or not finite, so a pair without a model
 * owns no candidates.  d_geom, seg_off, pairs and the out rows are those of spv_l1k2_guided_batch_device; d_lines is
 * double[out_rows, 3].  G and use are read before the call returns; asynchronous on `stream`, no workspace.
 * Kernel name for spv_profile_read: "epipolar_lines". */
int spv_epipolar_lines_batch_device(const float *d_geom, const long long *seg_off, int nseg, const int32_t *pairs,
                                    int npairs, const double *G, const int32_t *use, double *d_lines, void *stream);

/* The query loop sharded over the GPUs of one node with everything resident (the loop
 * the reference shards over OpenMP threads, src/BruteForceNnL1K2.h:92-93): one process, rank r =
 * devices[r].  d_x[r] is that device's replica of the database uint8[xrows,dim]; d_y[r] its query
 * shard uint8[spv_shard_lo(total, ndev, r + 1) - spv_shard_lo(total, ndev, r), dim] (contiguous
 * balanced shards of the yrows_total queries, the first total % ndev one row longer).  Every device
 * runs the L1 kernels on its shard and packs (idx0, idx1, d0, d1) into 16-byte records; the records
 * are gathered on devices[0] -- transport SPV_GATHER_RCCL: ncclGather on a cached ncclCommInitAll
 * clique (distinct devices), SPV_GATHER_PEERCOPY: one hipMemcpyPeerAsync per rank -- and widened
 * there into d_idx uint64[yrows_total,2], d_dist int32[yrows_total,2] (memory of devices[0]).
 * Synchronous: returns after all ranks' streams have drained; the caller's buffers must be ready
 * (its own streams synchronised) on entry.  Scratch comes from the library's per-device cache.
 * spv_profile_read("gather") / ("gather_widen") time the exchange. */
int spv_l1k2_gathered_device(int ndev, const int *devices, const uint8_t *const *d_x,
                             const uint8_t *const *d_y, int xrows, long long yrows_total, int dim,
                             uint64_t *d_idx, int32_t *d_dist, int transport);
/* The same for the cascade hash (every device also holds a replica of the hyperplanes d_dict[r],
 * float32[n,dim,m], and rebuilds identical codes and bucket tables; d_ncand int32[yrows_total] on
 * devices[0], may be NULL) and for the DLT (point shards d_x[r], d_xp[r] double[cnt_r,3]; d_dst on
 * devices[0]: double[npt_total,4], or double[npt_total] with want_error != 0; 32 or 8 bytes per point
 * travel, already in the ABI layout).  Loops sharded: src/CascadingHashNn.h:229-245 (the query loop of
 * its BruteForceNnL1K2 with SetFilter), src/Spectavi.cpp:48-51 / :64-67. */
int spv_cascade_gathered_device(int ndev, const int *devices, const float *const *d_x,
                                const float *const *d_y, int xrows, long long yrows_total, int dim, int m,
                                int n, int g, const float *const *d_dict, uint64_t *d_idx, float *d_dist,
                                int32_t *d_ncand, int transport);
int spv_dlt_gathered_device(int ndev, const int *devices, const double *P0, const double *P1,
                            long long npt_total, const double *const *d_x, const double *const *d_xp,
                            double *d_dst, int want_error, int transport);
/* First row of shard r of `total` rows over `shards` contiguous balanced shards (r = shards: total). */
long long spv_shard_lo(long long total, int shards, int r);

/* Exact p-norm k-NN with everything resident: d_x, d_y float32 or int32 [rows, dim] (4-byte
 * aligned), d_idx uint64[yrows,k], d_dist float32 / int32 [yrows,k], contract as nn_bruteforce.
 * slices = 0: the automatic plan, which needs spv_bruteforce_workspace_bytes(xrows, yrows, dim, k)
 * bytes of d_ws (8-byte aligned).  slices > 0 forces that many database slices (fewer if some would
 * be empty; at most 65535) and needs max(that, yrows * slices * k * 8) bytes.  The result does not
 * depend on the slice count.  Kernel names for spv_profile_read: "bruteforce", "bruteforce_merge". */
size_t spv_bruteforce_workspace_bytes(int xrows, int yrows, int dim, int k);
int spv_bruteforce_device(const void *d_x, const void *d_y, int is_int, int xrows, int yrows, int dim, int k,
                          float p, int slices, uint64_t *d_idx, void *d_dist, void *d_ws, size_t ws_bytes,
                          void *stream);

/* Approximate L2 k-NN on device pointers: d_x float32[xrows,dim], d_y float32[yrows,dim] (4-byte aligned;
 * 16-byte aligned rows let the re-rank load 16 bytes at a time), d_idx uint64[yrows,k], d_dist
 * float32[yrows,k], contract as ann_hnswlib.  slices = 0: the automatic plan, which needs
 * spv_ann_l2_workspace_bytes(xrows, yrows, dim, k, ncand) bytes of 256-byte aligned workspace (0 for an
 * invalid shape); slices > 0 forces that many database slices (fewer if some would be empty) and needs
 * at most yrows * slices * (8 * buffer length + 4) + 512 bytes more.  The result does not depend on the
 * slice count.  spv_ann_l2_plan is host-only and touches no device: out = {padded K, query tile, row
 * tile, slices, rows per slice, ncand in force, keys in the survivor buffer of a (query, slice), MFMA
 * shape (32: 32x32x16, 16: 16x16x32)}; outside the limits SPV_ERR_INVALID and out is untouched.
 * The plan always takes the 32x32x16 shape; SPECTAVI_ANN_MFMA=16 in the environment selects the other for
 * measurements (off the exact domain its K order, hence a score's last bit, may differ).
 * Kernel names for spv_profile_read: "ann_prep", "ann_coarse", "ann_merge", "ann_rerank". */
size_t spv_ann_l2_workspace_bytes(int xrows, int yrows, int dim, int k, int ncand);
int spv_ann_l2_plan(int xrows, int yrows, int dim, int k, int ncand, int slices, int out[8]);
int spv_ann_l2_device(const float *d_x, const float *d_y, int xrows, int yrows, int dim, int k, int ncand, int slices,
                      uint64_t *d_idx, float *d_dist, void *d_ws, size_t ws_bytes, void *stream);

/* image_pair_rectification with everything resident and F given (a HOST pointer, 9 doubles, from
 * spv_rectify_fundamental): dtype SPV_RECTIFY_F64 (d_im0, d_im1, d_r0, d_r1 double, 8-byte aligned)
 * or SPV_RECTIFY_U8 (uint8_t: 8-bit images, values copied as bytes); d_ri0, d_ri1 int32.  Output
 * shapes from spv_rectify_shape; every element of the four outputs is written.  Asynchronous, no
 * host synchronisation.  Kernel name for spv_profile_read: "rectify".  (SPV_RECTIFY_F32 is spv_rectify_batch's
 * alone.) */
int spv_rectify_device(const double *F, const void *d_im0, const void *d_im1, int dtype, int wid, int hgt, int nchan,
                       double sf, void *d_r0, void *d_r1, int32_t *d_ri0, int32_t *d_ri1, void *stream);

/* Device forms of spv_rectify_batch (section 2, where the contract is): d_images, d_box and the four outputs on the
 * caller's current device; sizes, pairs, the cameras, use and box host arrays. */
int spv_rectify_batch_bounds_device(const int32_t *sizes, int nimg, int nchan, double sampling_factor,
                                    const int32_t *pairs, int npairs, const double *P0s, const double *P1s,
                                    const int32_t *use, int32_t *d_box, void *stream);
int spv_rectify_batch_device(const void *d_images, int dtype, const int32_t *sizes, int nimg, int nchan,
                             double sampling_factor, const int32_t *pairs, int npairs, const double *P0s,
                             const double *P1s, const int32_t *use, const int32_t *box, void *d_r0, void *d_r1,
                             int32_t *d_ri0, int32_t *d_ri1, void *stream);

/* Dense disparity of every rectified pair of a collection (stereo_batch.hip): block matching along the rows of the
 * windows spv_rectify_batch_device wrote, by an integer sum of absolute differences on 8-bit gray values (nchan 1,
 * SPV_RECTIFY_U8; nothing else has this step).  box: HOST int32[npairs, 4] = (row_lo, row_hi, col_lo, col_hi) per pair,
 * rectify_batch's boxes; pair p's window has R = row_hi - row_lo rows and C = col_hi - col_lo columns and owns samples
 * [out_off[p], out_off[p + 1]) of every flat array below, row-major, out_off the running sum of the areas R * C of ALL
 * pairs (a pair that is not used keeps its window).  use: HOST int32[npairs] or NULL (every pair).
 *
 * 1. Cost and winner (spv_stereo_batch_device).  d_r0, d_r1 uint8 and d_ri0, d_ri1 int32, [samples]: rectify_batch's
 * outputs.  radius r in 0..7; drange HOST int32[npairs, 2] = (d_lo, d_hi) per pair.  swap 0: image 0 (d_r0, d_ri0) is
 * the reference, image 1 the other; swap 1: the roles are exchanged, drange is taken as given.  For the reference
 * sample (y, x) and a disparity d the candidate is (y, x + d) of the other image and
 *     cost(y, x, d) = sum over dy, dx in [-r, r] of |ref[y + dy, x + dx] - oth[y + dy, x + d + dx]|.
 * d is admissible for (y, x) iff r <= y < R - r, r <= x < C - r and r <= x + d < C - r (both blocks inside the
 * window), ri_ref[y, x] != -1, ri_oth[y, x + d] != -1 and d_lo <= d <= d_hi.  Only the two centres are tested for
 * validity: an invalid sample inside a block counts with the value 0 rectification gave it.  Outputs, one per sample
 * of every window, each element written exactly once:
 *   d_disp   int32: the admissible d of smallest (cost, d), lexicographic -- among equal costs the smallest d --,
 *            SPV_STEREO_NONE where no d is admissible
 *   d_cost   uint16_t: that cost (at most 225 * 255 = 57375), 0xFFFF where none
 *   d_cost2  uint16_t: the smallest cost over the admissible d' with |d' - disp| >= 2, 0xFFFF where there is none
 * A pair with use[p] == 0 gets SPV_STEREO_NONE / 0xFFFF / 0xFFFF over its whole window; an empty box owns nothing.
 * SPV_ERR_INVALID, nothing launched, outputs untouched: radius outside 0..7; d_lo > d_hi, |d_lo| or |d_hi| > 32767
 * (of a used pair); a box with a negative entry or row_lo > row_hi or col_lo > col_hi (of any pair); npairs < 0 or
 * above 2^20; 2^31 samples or more; a null pointer where there are samples.  Asynchronous on `stream`: the pair
 * table is uploaded into a buffer the calling thread keeps between calls (one per value of swap), so a call waits
 * only for the same thread's previous call of the same swap to have left the device.
 * Kernel name for spv_profile_read: "stereo_batch" (one bracket per call: the kernel of the call's radius over the
 * items, and the kernel that fills the windows of the pairs that are not used, where there are any).
 *
 * Plan (spv_stereo_batch_plan): host only.  out[3] = {used pairs, items, samples}; out_off long long[npairs + 1];
 * items NULL or int32[items_cap, 4] = (pair, first window row, rows <= 4, first window column): an item is one
 * workgroup step over a band of rows and a tile of at most 64 columns; the items of the used pairs with a non-empty
 * window cover every (row, column) of those windows exactly once.  drange may be NULL (not checked then).
 *
 * 2. Keep mask (spv_stereo_keep_batch_device).  d_disp0, d_cost0, d_cost20: a swap = 0 result; d_disp1: the disp of
 * a swap = 1 run or NULL; lr_tol >= 0; uniqueness in 0..100.  d_keep uint8[samples], every element written:
 * keep[y, x] = 1 iff disp0[y, x] != SPV_STEREO_NONE; and, where d_disp1 is given, with x' = x + disp0[y, x]:
 * 0 <= x' < C, disp1[y, x'] != SPV_STEREO_NONE and |disp0[y, x] + disp1[y, x']| <= lr_tol; and
 * cost0 * 100 <= cost20 * (100 - uniqueness) in 32-bit unsigned arithmetic, 0xFFFF taking part as 65535.  Else 0.
 * Kernel name: "stereo_keep_batch".
 *
 * 3. Correspondences (spv_stereo_matches_batch_device).  The kept samples of all pairs in order -- pair by pair,
 * row-major inside a window -- compacted by scans (no atomic decides a position).  sizes HOST int32[nimg, 2] =
 * (wid, hgt) and pairs HOST int32[npairs, 2] as spv_rectify_batch takes them (the two images of a pair may differ in
 * width here).  Kept sample (y, x) with d = disp0[y, x] has the source pixels s0 = ri0[y, x], s1 = ri1[y, x + d]:
 *   d_x0, d_x1  double[capacity, 3]: (s0 % wid0, s0 / wid0, 1.) and (s1 % wid1, s1 / wid1, 1.)
 *   d_rows      int32[capacity]: the sample's number inside its window, y * C + x
 *   d_pair_off  long long[npairs + 1]: pair p's matches are [pair_off[p], pair_off[p + 1])
 * These are the x0, x1, pair_off of spv_dlt_triangulate_batch_device with pixel cameras.  Only the first `capacity`
 * matches are written, nothing past them; d_pair_off always holds the true counts, so a call with capacity 0 (d_x0,
 * d_x1, d_rows may be NULL then) counts.  d_keep must be 0 wherever disp0 is not an admissible disparity (what step 2
 * writes); a kept sample whose candidate is outside its window is written with s1 = -1.  Asynchronous on `stream`,
 * the scratch of the scan taken from the library's device cache.  Kernel names: "stereo_matches_count" (the counts of
 * blocks of 1024 samples, their scan and pair_off), "stereo_matches_fill". */
#define SPV_STEREO_NONE (-2147483647 - 1)
int spv_stereo_batch_plan(const int32_t *box, int npairs, const int32_t *use, int radius, const int32_t *drange,
                          long long out[3], long long *out_off, int32_t *items, long long items_cap);
int spv_stereo_batch_device(const uint8_t *d_r0, const uint8_t *d_r1, const int32_t *d_ri0, const int32_t *d_ri1,
                            const int32_t *box, int npairs, const int32_t *use, int radius, const int32_t *drange,
                            int swap, int32_t *d_disp, void *d_cost, void *d_cost2, void *stream);
int spv_stereo_keep_batch_device(const int32_t *box, int npairs, const int32_t *d_disp0, const void *d_cost0,
                                 const void *d_cost20, const int32_t *d_disp1, int lr_tol, int uniqueness,
                                 uint8_t *d_keep, void *stream);
int spv_stereo_matches_batch_device(const int32_t *box, int npairs, const int32_t *sizes, int nimg,
                                    const int32_t *pairs, const int32_t *d_disp0, const uint8_t *d_keep,
                                    const int32_t *d_ri0, const int32_t *d_ri1, long long capacity, double *d_x0,
                                    double *d_x1, int32_t *d_rows, long long *d_pair_off, void *stream);

/* sift_filter with a status.  out: float32 NdArray, allocated by the callee. */
int spv_sift_filter(const float *im, int wid, int hgt, NdArray *out);
/* sift_filter into a caller-allocated float32[capacity, 132] table.  *count receives the true
 * number of rows; when it exceeds capacity the first capacity rows are written and the call
 * returns SPV_ERR_OVERFLOW. */
int spv_sift_table(const float *im, int wid, int hgt, float *table, int capacity, int32_t *count);
/* spv_sift_batch_device (below, where the contract is) through host pointers, on the first selected device: images,
 * table float32[cap_off[nimg], 132] and counts int32[nimg] are host memory.  The workspace comes from the library's
 * cache, never more than the cache keeps (or than the largest image needs), hence possibly several groups.  Returns
 * SPV_ERR_OVERFLOW, with the rows that fit written and all counts set, if any count exceeds its capacity. */
int spv_sift_tables(const float *images, const int32_t *sizes, int nimg, float *table, const long long *cap_off,
                    int32_t *counts);

/* Rows of the first table that sift_filter, spv_sift_filter and the batch form allocate before they
 * know the count (0: the default, max(1024, min(wid*hgt/16, 2^20))).  A longer result runs the
 * pipeline a second time into an exact table; the results are the same either way. */
int spv_sift_set_first_capacity(int rows);

/* Scratch bytes needed by spv_sift_device (0 for a size sift_filter rejects). */
size_t spv_sift_workspace_bytes(int wid, int hgt);
/* sift_filter with everything resident: d_im float32[hgt, wid], d_table float32[capacity, 132],
 * d_count int32[1].  Rows [0, min(*d_count, capacity)) are written and *d_count receives the true
 * row count (a count above capacity means overflow).  Asynchronous on `stream`: keypoint counts
 * stay on the device, the host never waits.  Kernel names for spv_profile_read: "sift_pyramid",
 * "sift_detect", "sift_describe". */
int spv_sift_device(const float *d_im, int wid, int hgt, void *d_ws, size_t ws_bytes, float *d_table, int capacity,
                    int32_t *d_count, void *stream);

/* sift_filter of many images in one chain of launches (sift.hip): the step before spv_l1k2_batch_device, "N images
 * -> N tables, back to back".  The octaves are walked once for a group of images; every launch has the image as one
 * more grid dimension, sized by the group's largest image at that octave, and the serial scans run one workgroup
 * per image side by side.  The launch count of a group is that of its largest image alone.
 *   sizes    host int32[nimg, 2] = (wid, hgt), each a size sift_filter takes (sides in [1, 8192]).
 *   d_images float32: the images back to back in that order, each row-major [hgt, wid].
 *   cap_off  host long long[nimg + 1], cap_off[0] = 0, non-decreasing, cap_off[nimg] < 2^31: image i owns rows
 *            [cap_off[i], cap_off[i + 1]) of d_table float32[cap_off[nimg], 132]; that many rows are its capacity.
 *   d_counts int32[nimg]: the true row count of every image, also where it exceeds the capacity.
 * The rows [cap_off[i], cap_off[i] + min(count_i, capacity_i)) are written; nothing else in d_table is touched.  For
 * every image the written rows and the count are bit for bit what spv_sift_device writes for that image alone,
 * whatever else the call holds, wherever the image stands in it and however the call is cut into groups.
 *
 * spv_sift_batch_plan: host only, touches no device.  Every image has a slice of the workspace, laid out as
 * spv_sift_device's workspace for its size.  The images are cut, in order, into groups that use the workspace one
 * after another: a group is closed when the next image's slice would no longer fit into ws_bytes (0: as much as
 * needed), or at 65535 images.  out = {groups, bytes with which only the 65535 cap closes a group, bytes of the
 * largest slice (the least that works), total pixels}; groups may be NULL, otherwise int32[groups_cap, 2] receives
 * (first image, images) of the first min(groups, groups_cap) groups.  SPV_ERR_INVALID, out and groups untouched: a
 * size sift_filter rejects, nimg < 0, NULL sizes with nimg > 0, ws_bytes non-zero and below out[2].
 * spv_sift_batch_workspace_bytes: out[1] (0 for arguments the plan rejects).
 *
 * spv_sift_batch_device follows the plan for the ws_bytes it is given, group after group on `stream` (stream order
 * lets the groups share d_ws, 256-byte aligned).  sizes and cap_off are read before the call returns.  The call may
 * wait for the upload of its small per-image table, which is queued on `stream`; it never waits for its kernels.
 * nimg = 0 is valid and launches nothing.  SPV_ERR_INVALID, nothing launched and no output touched: what the plan
 * rejects, a cap_off outside the rules, a NULL required pointer (d_table only where cap_off[nimg] > 0).  Kernel
 * names for spv_profile_read: "sift_batch_pyramid", "sift_batch_detect", "sift_batch_describe".
 *
 * spv_sift_batch_pack_device: the regions as what the next steps take.  seg_off: host long long[nimg + 1], the rules
 * of spv_l1k2_batch_device, each seg_off[i + 1] - seg_off[i] at most image i's capacity (the caller computes it from
 * the counts it read back).  One kernel copies row cap_off[i] + r of d_table to row seg_off[i] + r of d_packed
 * float32[total, 132], d_geom float32[total, 4] and d_desc uint8[total, 128] (4-byte aligned), the last two with the
 * values spv_sift_split_device gives for the same rows; each may be NULL, not all three.  SPV_ERR_INVALID, outputs
 * untouched, outside these rules.  Asynchronous but for the upload of the offsets.  Kernel name: "sift_batch_pack". */
int spv_sift_batch_plan(const int32_t *sizes, int nimg, size_t ws_bytes, long long out[4], int32_t *groups,
                        long long groups_cap);
size_t spv_sift_batch_workspace_bytes(const int32_t *sizes, int nimg);
int spv_sift_batch_device(const float *d_images, const int32_t *sizes, int nimg, void *d_ws, size_t ws_bytes,
                          float *d_table, const long long *cap_off, int32_t *d_counts, void *stream);
int spv_sift_batch_pack_device(const float *d_table, const long long *cap_off, const long long *seg_off, int nimg,
                               float *d_packed, float *d_geom, uint8_t *d_desc, void *stream);

/* Scratch bytes needed by spv_cascade_device. */
size_t spv_cascade_workspace_bytes(int xrows, int yrows, int dim, int m, int n, int g);
/* The launch plan spv_cascade_device follows for this shape under the SPECTAVI_CASCADE_* environment
 * of the moment (MFMA, MFMA4, GROUP, QHIST = 0 switch a form off, SORT = 0 / 1 forces the sorted probe
 * off / on, RU = 2 selects probe_refine_kernel<1, 2>; all are read on every call).  Host only, touches no device.  out =
 *   [0]      projection family: 0 project_kernel, 1 project_mfma_kernel, 2 project_mfma4_kernel
 *   [1], [2] the family's two template parameters: (MC, NT), (CT, FULL) or (CT, NG)
 *   [3]      GMAX of the query-side projection (the database side always has 1)
 *   [4]      probe: 0 probe_refine_kernel, 1 probe_table_kernel
 *   [5], [6] its CPL and RU
 *   [7]      its WPE                 (0 for probe_refine_kernel)
 *   [8], [9] its SHIFT and FULL      (0 for probe_refine_kernel)
 *   [10]     1 if the probe walks the queries sorted by each table's sign code
 *   [11]     1 if the query histogram is fused into the projection
 * SPV_ERR_INVALID (out untouched) outside the limits of spv_cascade_device: dim a positive multiple of
 * 16 up to 2048, m in [1,31], n >= 1, g in [0, min(m,16)], row counts >= 0. */
int spv_cascade_plan(int xrows, int yrows, int dim, int m, int n, int g, int out[12]);
/* d_x,d_y float32[rows,dim]; d_dict float32[n,dim,m]; outputs as in section 2
 * (d_ncand may be NULL). */
int spv_cascade_device(const float *d_x, const float *d_y, int xrows, int yrows, int dim,
                       int m, int n, int g, const float *d_dict, uint64_t *d_idx,
                       float *d_dist, int32_t *d_ncand, void *d_ws, size_t ws_bytes,
                       void *stream);

/* The cascade-hash 2-NN of a collection of (query set, database set) pairs in one chain of launches whose length
 * depends neither on the number of pairs nor on the number of sets (cascade_batch.hip).  Every row of the
 * collection is projected, sign-coded, imaged and bucket-sorted once, whatever number of pairs its set takes part in.
 *   rows     float32[total_rows, dim]: the tables of nseg sets back to back.
 *   seg_off  host long long[nseg + 1], non-decreasing, seg_off[0] = 0, seg_off[nseg] = total_rows < 2^31; set s is
 *            rows [seg_off[s], seg_off[s + 1]) and may be empty (the seg_off of spv_l1k2_batch_device).
 *   dict     float32[n, dim, m], one dictionary for the whole collection; g as for spv_cascade_device.
 *   pairs    host int32[npairs, 2] = (query set, database set), in any order, repeats and self pairs allowed.
 *   idx      uint64[out_rows, 2], dist float32[out_rows, 2], ncand (may be NULL) int32[out_rows]; out_rows = the
 *            query-set row counts summed over pairs.  Pair p owns the rows from the sum over the pairs before it, in
 *            query-row order; idx is the row number inside the database set; a missing neighbour is
 *            ((size_t)-1, 2147483648.0f); an empty database set gives two of them and ncand 0.
 * Per pair the rows are bit for bit what spv_cascade_device(database set, query set) writes: the same candidate
 * set, its two smallest distinct (dist, idx) in lexicographic order, the same visited count.  Limits: dim a
 * positive multiple of 16 and <= 256, m in [1,31], n >= 1, g in [0, min(m,16)], nseg >= 0, npairs >= 0, set numbers
 * in [0, nseg), nseg * n <= 65535 (the scan kernels take the (set, table) as a grid row), at most 2^31 - 1 work
 * items (64 query rows of one pair each), d_rows, d_dict and d_ws 16-byte aligned, d_idx 8-byte, d_dist and d_ncand
 * 4-byte, ws_bytes at least the workspace bytes.  Outside them SPV_ERR_INVALID, nothing launched, no output
 * touched.  One device.
 *
 * spv_cascade_batch_plan: host only, touches no device.  out = {work items, out_rows, bucket bits hb, workspace
 * bytes}; items may be NULL, otherwise int32[items_cap, 3] receives the first min(work items, items_cap) work items,
 * one workgroup of the probe each, as (pair, first query row within the query set, query rows): exactly the list
 * the device call launches, in its order; together they cover every out row once.  hb = min(m, 22, max(12,
 * ceil(log2(rows of the largest set)))), lowered until the nseg * n tables of 2^hb + 1 words fit 1 GiB; with hb < m
 * the probe compares the full code of every bucket entry, so the results do not depend on hb.  SPV_ERR_INVALID
 * leaves out and items untouched.  spv_cascade_batch_workspace_bytes: out[3] (0 for arguments the plan rejects).
 *
 * spv_cascade_batch_device: seg_off and pairs are read before the call returns.  The call may wait for the upload
 * of its small tables (work items, seg_off), which is queued on `stream`; it never waits for its kernels, and
 * everything else is asynchronous on `stream`.  Kernel names for spv_profile_read, one bracket per call each:
 * "cascade_batch_project" (dictionary repack and the projection of all rows), "cascade_batch_buckets" (histogram,
 * scan, fill), "cascade_batch_probe" (probe and refine of every out row).  spv_ratio_test and
 * spv_ratio_test_device (dist_is_float = 1) apply to the concatenated output as it stands: their matches are (out
 * row, row within the database set). */
int spv_cascade_batch_plan(const long long *seg_off, int nseg, int dim, int m, int n, int g, const int32_t *pairs,
                           int npairs, long long out[4], int32_t *items, long long items_cap);
size_t spv_cascade_batch_workspace_bytes(const long long *seg_off, int nseg, int dim, int m, int n, int g,
                                         const int32_t *pairs, int npairs);
int spv_cascade_batch_device(const float *d_rows, const long long *seg_off, int nseg, int dim, int m, int n, int g,
                             const int32_t *pairs, int npairs, const float *d_dict, uint64_t *d_idx, float *d_dist,
                             int32_t *d_ncand, void *d_ws, size_t ws_bytes, void *stream);

/* P0,P1 are HOST pointers (24 doubles, passed by value to the kernel);
 * d_x,d_xp double[npt,3]; d_dst double[npt,4] (triangulate) / double[npt] (error). */
int spv_dlt_triangulate_device(const double *P0, const double *P1, long long npt,
                               const double *d_x, const double *d_xp, double *d_dst,
                               void *stream);
int spv_dlt_reprojection_error_device(const double *P0, const double *P1, long long npt,
                                      const double *d_x, const double *d_xp, double *d_dst,
                                      void *stream);
/* Device form of spv_dlt_triangulate_batch (section 2, where the contract is): d_x0, d_x1, d_mask, d_X, d_err,
 * d_rows, d_out_off long long[npairs + 1] and d_count long long[1] are device memory; pair_off, P0s, P1s and use
 * are HOST pointers.  d_count holds the true count also above capacity. */
int spv_dlt_triangulate_batch_device(const double *d_x0, const double *d_x1, const long long *pair_off, int npairs,
                                     const double *P0s, const double *P1s, const int32_t *use, const uint8_t *d_mask,
                                     double *d_X, double *d_err, int32_t *d_rows, long long capacity,
                                     long long *d_out_off, long long *d_count, void *stream);

/* Ratio test + ordered match compaction, the step right after the NN path in the
 * reference's pipeline (example/ex01_essential_estimation.py:102-106): query q passes iff
 * it has a nearest neighbour and (double)dist[q,1] / (double)dist[q,0] >= min_ratio under
 * IEEE division (x/0 = inf passes, 0/0 = NaN fails).  Passing (query, database index)
 * pairs are written in ascending query order.  dist_is_float: 0 = int32 distances
 * (nn_bruteforcel1k2), 1 = float32 (nn_cascading_hash).
 * Host form: matches int32[yrows,2] capacity, returns status; *count receives the number
 * of matches. */
int spv_ratio_test(const uint64_t *idx, const void *dist, int dist_is_float, int yrows,
                   double min_ratio, int32_t *matches, int32_t *count);
size_t spv_ratio_test_workspace_bytes(int yrows);
/* Device form: d_matches int32[yrows,2] capacity, d_count int32[1]. */
int spv_ratio_test_device(const uint64_t *d_idx, const void *d_dist, int dist_is_float, int yrows,
                          double min_ratio, int32_t *d_matches, int32_t *d_count, void *d_ws,
                          size_t ws_bytes, void *stream);

/* SIFT table adapter: rows of 132 float32 = x, y, sigma, angle + 128 descriptor values that
 * are uint8(512*d) stored as float (reference src/Sift.h:13,115-123) are split into
 * geom float32[rows,4] and desc uint8[rows,128] (truncating cast).  Host form. */
int spv_sift_split(const float *table, int rows, float *geom, uint8_t *desc);
int spv_sift_split_device(const float *d_table, int rows, float *d_geom, uint8_t *d_desc,
                          void *stream);
/* (x, y, 1) float64 coordinates of both keypoints of every match (query row, database row)
 * written by spv_ratio_test_device: d_x0[i] from d_geom_x[database row], d_x1[i] from
 * d_geom_y[query row]; rows [0, *d_count) of the [capacity,3] outputs are written
 * (reference example/ex01_essential_estimation.py:104-106). */
int spv_gather_match_coords_device(const float *d_geom_x, const float *d_geom_y,
                                   const int32_t *d_matches, const int32_t *d_count, int capacity,
                                   double *d_x0, double *d_x1, void *stream);

/* The same for the matches of a spv_l1k2_batch_device + spv_ratio_test_device run, as per-pair coordinates.
 *   d_geom   float32[total_rows, 4]: the geometry of all sets back to back, row for row the desc of the matching call
 *   seg_off, nseg, pairs, npairs: host arrays, the very arguments of the matching call (same rules, SPV_ERR_INVALID
 *            with nothing launched outside them)
 *   d_matches int32[capacity, 2], d_count: as spv_ratio_test_device wrote them over the concatenated output: a
 *            match is (out row, row within the database set), in ascending out-row order
 *   d_x0, d_x1 double[capacity, 3]: rows [0, *d_count) are written, x0 = (x, y, 1) of row seg_off[db] + k of d_geom,
 *            x1 = (x, y, 1) of row seg_off[q] + (out row - first out row of the pair), for the pair (q, db) that owns
 *            the out row
 *   d_pair_off device long long[npairs + 1]: where pair p's matches begin; d_pair_off[npairs] = *d_count.  Read
 *            back, it is the pair_off of spv_ransac_fit_batch_device.
 * Asynchronous on `stream` but for the upload of its small per-pair table, which stays with the calling thread
 * until its next call.  Kernel name for spv_profile_read: "gather_match_coords_batch". */
int spv_gather_match_coords_batch_device(const float *d_geom, const long long *seg_off, int nseg, const int32_t *pairs,
                                         int npairs, const int32_t *d_matches, const int32_t *d_count, int capacity,
                                         double *d_x0, double *d_x1, long long *d_pair_off, void *stream);

/* Multi-view tracks (tracks_batch.hip): the connected components of the keypoint graph whose nodes are the rows of
 * the concatenated tables (global row g = seg_off[s] + r) and whose edges are the matches of all pairs, as
 * spv_ratio_test_device writes them over a spv_l1k2_batch_device / spv_cascade_batch_device /
 * spv_l1k2_guided_batch_device output.  The reference has no such step.
 *   seg_off, nseg, pairs, npairs: host arrays, the very arguments of the matching call.
 *   d_matches int32[capacity, 2], d_count: row i = (out row, row within the database set).  Its pair p is the one with
 *            out_off[p] <= out row < out_off[p + 1] (out_off: the running sum of the query sets' rows; empty pairs own
 *            nothing), pairs[p] = (q, db), and the edge joins seg_off[q] + (out row - out_off[p]) and seg_off[db] + the
 *            database row.  Only rows [0, min(*d_count, capacity)) are read, in any order.  A row whose out row lies
 *            outside [0, out_rows) or whose database row lies outside its set is skipped.  Duplicate edges, duplicate
 *            pairs and self pairs are legal.
 *   d_mask   uint8[capacity] or NULL: row i is an edge only where d_mask[i] != 0.
 *   min_len  >= 2: a track is a component of at least min_len members.
 * Outputs, all a function of the edge set alone (the same bits for any edge order and from run to run):
 *   d_label  int32[total_rows]: the smallest global row of the node's component.
 *   d_track  int32[total_rows]: the node's track number or -1; tracks are numbered in ascending order of their label.
 *   d_track_off long long[B / 2 + 1]: track t owns members [d_track_off[t], d_track_off[t + 1]).
 *   d_members int32[B, 2] = (set, row within the set), inside a track ascending by global row.
 *   d_flags  uint8[B / 2]: bit 0 is set iff two members of the track lie in the same set; the other bits are 0.
 *   d_counts int32[2] = (ntracks, nmembers).
 * B = min(total_rows, 2 * capacity); with accumulate != 0, whose members this call's capacity does not bound,
 * B = total_rows.  Entries [0, ntracks] of d_track_off, [0, nmembers) of d_members and [0, ntracks) of d_flags are
 * written; nothing outside d_label, d_track, d_counts and these is.
 * accumulate != 0: d_label is read first as an earlier call's result over the same seg_off and the new edges are added
 * to its components; two calls that split an edge set give the bits of one call over the whole set.  An incoming
 * entry outside [0, its own row] stands for "its own row": garbage may give meaningless tracks, never an access out
 * of bounds or a loop without an end.
 * SPV_ERR_INVALID, nothing launched: seg_off[0] != 0 or decreasing, total_rows >= 2^31, 2^31 out rows or more, a pair
 * outside [0, nseg), nseg < 0, npairs < 0, capacity < 0, min_len < 2, a NULL required pointer, a workspace shorter
 * than spv_tracks_batch_workspace_bytes(total_rows, capacity) (21 bytes a row and small change, every piece rounded
 * up to 256; it does not depend on capacity) or not 16-byte aligned.  Asynchronous on `stream` but for the upload of
 * its small per-pair table, which stays with the calling thread until its next call; no host synchronisation.
 * d_label doubles as the parent array of the forest while the call runs.  Kernel names for spv_profile_read, one per
 * phase that launches: "tracks_init", "tracks_hook" (agent-scope compare-and-swap from a root's self value, larger
 * root under smaller; not launched without a possible edge), "tracks_flatten" (ceil(log2(total_rows) / 2) + 1
 * launches of pointer jumping, which return at once after a round that changed nothing), "tracks_sizes",
 * "tracks_scan", "tracks_place", "tracks_order" (a stable radix sort of (track, row) by track, 8 bits a pass, as many
 * passes as the track count has bytes), "tracks_flags".
 * spv_tracks_batch: host pointers, on the first selected device; matches int32[count, 2], every output sized as above
 * with capacity = count; label is read only with accumulate != 0.  Touches no device when total_rows is 0. */
size_t spv_tracks_batch_workspace_bytes(long long total_rows, int capacity);
int spv_tracks_batch_device(const long long *seg_off, int nseg, const int32_t *pairs, int npairs,
                            const int32_t *d_matches, const int32_t *d_count, int capacity, const uint8_t *d_mask,
                            int min_len, int accumulate, int32_t *d_label, int32_t *d_track, long long *d_track_off,
                            int32_t *d_members, uint8_t *d_flags, int32_t *d_counts, void *d_ws, size_t ws_bytes,
                            void *stream);
int spv_tracks_batch(const long long *seg_off, int nseg, const int32_t *pairs, int npairs, const int32_t *matches,
                     int count, const uint8_t *mask, int min_len, int accumulate, int32_t *label, int32_t *track,
                     long long *track_off, int32_t *members, uint8_t *flags, int32_t *counts);

/* N-view DLT of every track (tracks_triangulate.hip): one 3-D point per track from all its observations, a residual
 * per observation and a verdict per track, for a caller who has one camera per set (a calibrated rig, an earlier
 * reconstruction, a pose graph of their own, or spv_resect_fit_batch_device below for views that see points already
 * triangulated).  The cameras are taken as given: chaining pairwise fits into global cameras is not part of the
 * library; spv_bundle_adjust_device below refines cameras and points together.  The reference has no such step.
 *   d_geom   float32[total_rows, 4]: x, y, sigma, angle of every row, as spv_sift_split_device writes them; only x
 *            and y are read, widened to double.
 *   seg_off, nseg: host, the seg_off of spv_l1k2_batch_device.
 *   cams     host double[nseg, 12]: the row-major 3x4 camera P_s of every set, pixel or calibrated to match d_geom.
 *   use_set  host int32[nseg] or NULL: a set with use_set[s] == 0 has no camera (its row of cams is not read).
 *   track_off host long long[ntracks + 1], d_members int32[nmembers, 2] = (set, row within the set): as
 *            spv_tracks_batch_device returns them; track t owns members [track_off[t], track_off[t + 1]).
 * A member is usable when its set is in [0, nseg), its row inside that set and the set has a camera.  Nothing else
 * is dereferenced: garbage members give unsolved tracks, never an access out of bounds.  Per track t:
 *   matrix   usable observation i in set s with (u, v) = (double)d_geom[row][0..1] contributes the reference's two
 *            DLT rows u P_s[2] - P_s[0], v P_s[2] - P_s[1] (src/DltTriangulator.h:38-54), in member order: A_t, 2m x 4.
 *   d_X      double[ntracks, 4]: the unit right singular vector of A_t's smallest singular value, sign as
 *            spv_dlt_triangulate_device gives it.  A_t is reduced to a 4x4 triangle by Givens rotations (never through
 *            A^T A) and solved by the two-view solver.  A track with exactly two usable observations goes through the
 *            two-view arithmetic itself: d_X is bit for bit spv_dlt_triangulate_batch_device's for the same two
 *            observations (w = 1) with P0 = the first member's camera, P1 = the second's, and the two d_err add up to
 *            its err exactly.  A track with fewer than 2 usable observations is not solved: its d_X row is all zeros.
 *   d_err    double[nmembers] or NULL: |proj(P_s X) - (u, v)| of every usable observation of a solved track, NaN
 *            everywhere else.
 *   d_ok     uint8[ntracks] or NULL: 1 iff the track is solved, X is finite, every usable observation has
 *            sign(det P[:, :3]) / |P[2, :3]|^2 * (P X)[2] / X[3] > 0 and err <= max_error (+inf: cheirality alone).
 *   d_nused  int32[ntracks] or NULL: the usable observations.
 * Nothing is screened beyond "usable".  A usable observation whose (u, v) or whose camera holds a NaN or an infinity
 * stays usable and counts in d_nused; its track has d_ok 0 and a d_X that is NaN or finite garbage, and no other track
 * of the call notices.  A track whose A_t has rank 3 gets its null vector -- members of one set alone: that camera's
 * centre, where every depth term is a rounding of 0 and d_ok and d_err are not determined --, one of rank 2 (the same
 * observation over and over) some unit vector with ||A X|| <= 1e-13 sigma1.  All cameras times one power of two, or
 * times -1, leave d_X, d_err, d_ok and d_nused the same bits while no intermediate leaves the double range (tested
 * at 2^+-40); at 2^+-445 d_X, d_err and d_nused still meet the definition, d_ok does not (det P[:, :3] overflows).
 * Outputs are aligned with the inputs; nothing is compacted.  A track's results depend on its own members, d_geom and
 * the cameras alone: not on its neighbours, its place in the call or the form that solves it beyond the rounding
 * of the reduction order (tracks of at most two usable observations: not at all).
 * Two forms, chosen by a track's member count alone: the lane form (one lane per track, at most L members) and the
 * wave form (one wave per track, the lanes' triangles combined in 6 butterfly steps); kernel names for
 * spv_profile_read "tracks_triangulate" and "tracks_triangulate_long".  spv_tracks_triangulate_set_long(L): L >= 0,
 * default 16, the fastest of 8, 16, 32, 64 measured on two inputs of a million tracks; 0 sends every track of 3 or more
 * members to the wave form, a value no track reaches sends none.  spv_tracks_triangulate_get_long: the setting.
 * spv_tracks_triangulate_plan: host only, touches no device.  out = {lane-form tracks, wave-form tracks, workgroups
 * of the lane launch, longest track} under the current setting.
 * SPV_ERR_INVALID, nothing launched: the rules of seg_off (spv_l1k2_batch_device); track_off[0] != 0, decreasing, or
 * not ending at nmembers; nmembers >= 2^31; a negative count; a NULL required pointer (seg_off, track_off; cams where
 * nseg > 0; d_members where nmembers > 0; d_geom where both total_rows and nmembers > 0; d_X where ntracks > 0); a
 * NaN max_error; an output not aligned to its element size.  Asynchronous on `stream` but for the one upload of the
 * call's tables (cameras, use_set, seg_off, track_off, the wave-form list).
 * spv_tracks_triangulate: host pointers, on the first selected device; touches no device when ntracks is 0. */
int spv_tracks_triangulate_set_long(int L);
int spv_tracks_triangulate_get_long(void);
int spv_tracks_triangulate_plan(const long long *track_off, int ntracks, long long out[4]);
int spv_tracks_triangulate_device(const float *d_geom, const long long *seg_off, int nseg, const double *cams,
                                  const int32_t *use_set, const long long *track_off, int ntracks,
                                  const int32_t *d_members, long long nmembers, double max_error, double *d_X,
                                  double *d_err, uint8_t *d_ok, int32_t *d_nused, void *stream);
int spv_tracks_triangulate(const float *geom, const long long *seg_off, int nseg, const double *cams,
                           const int32_t *use_set, const long long *track_off, int ntracks, const int32_t *members,
                           long long nmembers, double max_error, double *X, double *err, uint8_t *ok, int32_t *nused);

/* RANSAC camera resection of many views (resect_batch.hip): the camera of every view that has none yet, from the 3-D
 * points of the tracks the view observes.  With it the chain runs incremental structure from motion on the device:
 * seed with one pair (spv_ransac_fit_batch: [I | 0] and `camera`), spv_tracks_triangulate_device with use_set = the
 * registered views, resect all other views in one call, triangulate again.  Two ops, split the way
 * spv_gather_match_coords_batch_device and spv_ransac_fit_batch_device are.  The reference has no such step.
 *
 * spv_resect_gather_device: the 2-D / 3-D correspondences of the listed views.
 *   d_geom, seg_off, nseg: as in spv_tracks_triangulate_device.
 *   d_track  int32[total_rows]: the track of every row, as spv_tracks_batch_device writes it.
 *   views    host int32[nviews], each in [0, nseg): the sets to gather; repeats are legal, every listed view owns a
 *            block of its own.  At most 2^20 views, and fewer than 2^31 rows in the listed views together.
 *   d_X      double[ntracks, 4], d_ok uint8[ntracks] or NULL: spv_tracks_triangulate_device's outputs.
 * Row r of view views[i] = set s is taken iff 0 <= d_track[seg_off[s] + r] < ntracks, d_ok is NULL or d_ok[track] != 0,
 * and all four entries of d_X[track] are finite.  Nothing else is dereferenced: garbage track numbers give skipped
 * rows, never an access out of bounds.  Taken rows are written back to back, view after view in the order of `views`,
 * inside a view in ascending row order: d_x double[capacity, 3] = (u, v, 1) widened from float32, d_Xw
 * double[capacity, 4] = the track's d_X row bit for bit, d_rows int32[capacity] (may be NULL) = the row within the view.
 * d_view_off device long long[nviews + 1] and view_off, the same on the host (either may be NULL; a host view_off makes
 * the call wait for its kernels): listed view i owns rows [view_off[i], view_off[i + 1]); both count all taken rows
 * even beyond `capacity`, as spv_dlt_triangulate_batch_device does, and nothing at or beyond `capacity` is written.
 * A flag / segmented scan / place chain over the listed views' rows in blocks of 256; the same bits from run to run;
 * spv_profile_read name "resect_gather".  SPV_ERR_INVALID, nothing launched: the rules of seg_off; a negative count or
 * capacity; a view outside [0, nseg); the limits above; a NULL required pointer (seg_off; views where nviews > 0;
 * d_geom, d_track where the listed views have rows; d_X where they have rows and ntracks > 0; d_x, d_Xw where
 * moreover capacity > 0); a pointer not aligned to its element size.
 *
 * spv_resect_fit_batch_device: one camera per set.  d_x double[total, 3] and d_Xw double[total, 4] hold the sets back
 * to back, set p = rows [view_off[p], view_off[p + 1]) (host, the rules of spv_ransac_fit_batch's pair_off), in whatever
 * units and scale the caller has, pixel or calibrated: nothing is normalised.  The pixel of a row is (u, v) =
 * (x[0] / x[2], x[1] / x[2]) by IEEE division: a third column of 1 leaves the first two as they are.
 *   subsets  samples host int32[nviews, maximum_tries, 6]: row numbers inside the set, each in [0, rows); duplicates
 *            are legal and give a degenerate hypothesis.  NULL: seeds host unsigned long long[nviews], and set p uses
 *            the first six columns of what spv_ransac_sample(seeds[p], rows, maximum_tries) returns (a set of 6 to 9
 *            rows, which that sampler does not take, the first six of a shuffle of its rows by the same generator).
 *            Sets of fewer than 6 rows are skipped: success 0, best_try -1, tries_run 0, camera row untouched.
 *   hypothesis  of a try, whatever solves it: the six sampled rows give the 11 x 12 matrix A, row i contributing
 *            [X_i^T, 0, -u_i X_i^T] and [0, X_i^T, -v_i X_i^T] in sample order, the sixth its u row only.  P is the
 *            unit-norm null vector of A read as a row-major 3x4 matrix, its last non-zero entry positive.  (11 rows,
 *            not the 12-row least-squares DLT: the null vector is then defined exactly, whatever a solver normalises
 *            by.)  The kernel eliminates P's first two rows through one Givens QR of the X_i, takes P[2] as the
 *            vector orthogonal to the three rows that remain (Householder, unpivoted) and solves the two triangles:
 *            ||A p|| stays below 1e-15 sigma1(A) on subsets in general position.
 *   verdict  a row is an inlier of P iff |proj(P Xw) - (u, v)| <= max_error and the depth term of
 *            spv_tracks_triangulate_device's d_ok is positive: sign(det P[:, :3]) / |P[2, :3]|^2 (P Xw)[2] / Xw[3] > 0.
 *            The kernel compares squares and multiplies by 1 / Xw[3]; NaNs compare false, a non-finite P counts 0.
 *            Rows are taken as they come.  A row with x[2] = 0, with a NaN, or with an all-zero Xw is an inlier of no
 *            camera and spoils only the tries that sample it (their P is not finite, or finite garbage that is scored
 *            like any other); Xw[3] = 0 makes the depth term +-inf, which passes where it is +inf.  A row of x times
 *            +-2^k, all of Xw times one power of two (tested at 2^+-30): the same bits in every output; a negated Xw
 *            row is the same point.  A degenerate subset (duplicates, coplanar or collinear points) gives a P that is
 *            finite garbage or not finite, scored by the same verdict; a set of coplanar points may keep such a P.
 *   rule     on try order: the first try with count / (double) rows >= required_percent_inliers (success 1); failing
 *            that, with find_best_even_in_failure, the try with the most inliers -- at least one --, the earliest
 *            among equals (success 0); otherwise no model.  The result does not depend on how tries are cut into
 *            rounds and work items: counts are integer sums.
 * Host outputs as spv_ransac_fit_batch_device's: success int32[nviews], camera double[nviews, 12] (written where a
 * model was kept), inlier_percent double[nviews] = n_inliers / rows, n_inliers int32[nviews], best_try and tries_run
 * int32[nviews] or NULL.  d_inlier_mask uint8[total] or NULL: the kept camera's verdict of every row, 0 where a set
 * kept none.  d_try_cameras double[nviews, maximum_tries, 12] and d_try_inliers int32[nviews, maximum_tries] (device,
 * either may be NULL) make the op checkable try by try; rows of skipped sets are NaN / 0.  With either of them no set
 * leaves early: every try is evaluated and tries_run = maximum_tries.  Otherwise sets advance in rounds (256 tries of
 * a set, then fourfold up to 4096; 32768 tries a round) and leave at their first success: tries_run lies in
 * [best_try + 1, maximum_tries].  The call waits for `stream` once a round.
 * Kernels, spv_profile_read names: "resect_solve" (one try per lane), "resect_score" (one workgroup per work item =
 * at most 256 rows of one set and a range of its tries; a lane keeps its row in registers, a try's camera is
 * workgroup-uniform; one ballot and popcount per wave and try), "resect_reduce" (per set over its tries in order).
 * Work items are spv_ransac_fit_batch's: rows in blocks of 256, a set's tries cut into ranges of at least 48 while the
 * round has fewer than 4 row blocks per compute unit.  spv_resect_fit_batch_plan: host only; the first round of such a
 * call on a device of compute_units, out = {sets, tries, items, row blocks}, items int32[items_cap, 5] = (set, first
 * row of the concatenated arrays, rows, first try of the round, tries) or NULL.
 * SPV_ERR_INVALID, nothing launched: the rules of view_off; NaN max_error or required_percent_inliers; a negative
 * count; more than 2^20 sets or 7e8 tries; a NULL required pointer; neither samples nor seeds while a set has >= 6
 * rows and maximum_tries > 0; a sample out of range; a pointer not aligned to its element size.
 * spv_resect_fit_batch: host pointers (inlier_mask, try_cameras, try_inliers on the host, each may be NULL), on the
 * first selected device; touches no device when no set has 6 rows or maximum_tries is 0.
 * Not part of the op: a refit of the winner on all its inliers, a calibrated P3P solver.  The joint refinement of
 * cameras and points is spv_bundle_adjust_device. */
int spv_resect_gather_device(const float *d_geom, const int32_t *d_track, const long long *seg_off, int nseg,
                             const int32_t *views, int nviews, const double *d_X, const uint8_t *d_ok, int ntracks,
                             long long capacity, double *d_x, double *d_Xw, int32_t *d_rows, long long *d_view_off,
                             long long *view_off, void *stream);
int spv_resect_fit_batch_device(const double *d_x, const double *d_Xw, const long long *view_off, int nviews,
                                double required_percent_inliers, double max_error, int maximum_tries,
                                int find_best_even_in_failure, const int32_t *samples, const unsigned long long *seeds,
                                int32_t *success, double *camera, double *inlier_percent, int32_t *n_inliers,
                                int32_t *best_try, int32_t *tries_run, uint8_t *d_inlier_mask, double *d_try_cameras,
                                int32_t *d_try_inliers, void *stream);
int spv_resect_fit_batch(const double *x, const double *Xw, const long long *view_off, int nviews,
                         double required_percent_inliers, double max_error, int maximum_tries,
                         int find_best_even_in_failure, const int32_t *samples, const unsigned long long *seeds,
                         int32_t *success, double *camera, double *inlier_percent, int32_t *n_inliers, int32_t *best_try,
                         int32_t *tries_run, uint8_t *inlier_mask, double *try_cameras, int32_t *try_inliers);
int spv_resect_fit_batch_plan(const long long *view_off, int nviews, int maximum_tries, int compute_units,
                              long long out[4], int32_t *items, long long items_cap);

/* Bundle adjustment (bundle_adjust.hip): Levenberg-Marquardt refinement of all free cameras and all participating track
 * points over all observations, by a matrix-free Schur complement and preconditioned conjugate gradients (Wu et al.,
 * "Multicore Bundle Adjustment"; Agarwal et al., "Bundle Adjustment in the Large").  The reference has no such step;
 * tests/bundle_model.py restates this text in numpy with dense normal equations.
 *   d_geom, seg_off, nseg, track_off, ntracks, d_members, nmembers: as in spv_tracks_triangulate_device.
 *   d_X      double[ntracks, 4], in and out: spv_tracks_triangulate_device's points.
 *   d_use    uint8[ntracks] or NULL: e.g. spv_tracks_triangulate_device's d_ok.
 *   K        host double[nseg, 9]: row-major, upper triangular, K[8] == 1, K[3] == K[6] == K[7] == 0, K[0] and K[4]
 *            non-zero, all finite.  Held fixed.
 *   poses    host double[nseg, 12], in and out: row-major [R | t].
 *   mode     host int32[nseg]: 0 the set has no camera (its rows of K and poses are not read), 1 free, 2 fixed (read,
 *            its observations count, never moved).
 * Residual of an observation of the point X (Euclidean: d_X[:3] / d_X[3]) in set s: y = R X + t, (u, v) = (K0 y0/y2 +
 * K1 y1/y2 + K2, K4 y1/y2 + K5), r = (u, v) - (double)d_geom[row][0..1].  Loss: rho(|r|) = r^2 / 2 for |r| <= huber,
 * huber (|r| - huber / 2) beyond; huber = +inf is plain least squares.  Robustification is first order: the weight is
 * w = min(1, huber / |r|), Jacobian rows and residual are scaled by sqrt(w) (J~, r~), there is no second-order
 * correction, and the cost reported and compared is F = sum rho.
 * Parameters: a free camera has six, R <- Exp(omega) R (Rodrigues) and t <- t + tau, linearised at omega = 0:
 * dy/d omega = -[R X]x, dy/d tau = I, dy/dX = R; a point has its three Euclidean coordinates.  p (+) delta applies both.
 * Who takes part: a member is usable under spv_tracks_triangulate_device's rule with "has a camera" = mode != 0;
 * nothing else is dereferenced, garbage members give ignored observations and never an access out of bounds.  A track
 * takes part iff d_use is NULL or non-zero there, its d_X row is finite with d_X[3] != 0 (and a finite quotient), it has
 * at least 2 usable observations, and at the starting parameters every one of them has a finite residual and y2 > 0.
 * A track that does not take part is left untouched bit for bit and contributes nothing; one that does has its d_X
 * row written as (X, Y, Z, 1).  d_active uint8[ntracks] or NULL: which tracks took part.  A free camera with no
 * observation among the participating tracks does not move: its row of poses comes back bit for bit, as do the rows
 * of mode 2 and mode 0.
 * Loop, with g = J~^T r~, H = J~^T J~ and D = diag(H), every entry clamped to [1e-6, 1e32]:
 *   lambda = lambda0; linearise; F = cost
 *   for step in 0 .. max_steps - 1:
 *     if max |g| <= gtol: stop (gradient, reason 1)
 *     solve (H + lambda D) delta = -g
 *     F' = cost at p (+) delta; +inf if any participating observation has y2 <= 0 or a non-finite residual there
 *     if F' < F: accept, lambda = max(lambda / 10, 1e-15), linearise again; if (F - F') / F <= ftol: stop (cost, 2)
 *     else:      reject, lambda *= 10; if lambda > 1e15: stop (damping, 3)
 *   (reason 0: max_steps ran out)
 * Solve: the point blocks V_t + lambda D_t (3x3) are inverted in closed form per track; the reduced camera system
 * S dc = b, S = (U + lambda Dc) - E (V + lambda Dp)^-1 E^T, b = -gc + E (V + lambda Dp)^-1 gp, is never formed:
 * conjugate gradients from x0 = 0 apply S as (U + lambda Dc) dc - E (Vl^-1 (E^T dc)), preconditioned by the inverses of
 * the 6x6 blocks U_s + lambda D_s (Cholesky, once per step), and stop at |r| <= cg_tol |b| (r the true recurrence
 * residual), after cg_max iterations, or when p^T S p or r^T z is not positive; then dp = -Vl^-1 (gp + E^T dc).
 * Outputs: poses on the host, d_X on the device, d_err double[nmembers] or NULL with spv_tracks_triangulate_device's
 * meaning at the final parameters (|r| of every observation of a participating track, NaN elsewhere), trace host
 * double[max_steps, 6] or NULL, row = (F before, F', lambda used, CG iterations, accepted 0/1, max |g| before), unused
 * rows NaN, and info host double[7] = (steps run, steps accepted, stop reason, participating tracks, participating
 * observations, first F, last F).
 * Kernels: track-major ones take one lane per track of at most 16 members and one wave per longer track (the lanes'
 * sums meet in an xor butterfly); view-major ones walk a stable counting sort of the participating observations by
 * set, built once per call from scans, each camera's list cut into chunks of 1024 observations, one workgroup per
 * chunk, the chunk partials added in chunk order.  The Jacobians are made again wherever they are needed, not stored
 * (measured faster than streaming 144 bytes per observation twice per CG iteration, with the same bits).  There are no
 * floating-point atomics and no order that depends on timing: the op returns the same bits from run to run.  CG scalars
 * and a `done` flag stay on the device, a step's cg_max iterations are enqueued back to back and become no-ops once
 * `done` is set; the call waits for `stream` twice before the loop (the view-major order, the first cost), once per
 * step and once after the loop, to bring the poses back.  F and max |g| are summed over the tracks in two stages
 * (partials of 2048 tracks, then the partials), in a fixed order.  spv_profile_read names: "bundle_mark", "bundle_sort", "bundle_linearise", "bundle_cam_sum",
 * "bundle_gradient_max", "bundle_cost_sum", "bundle_point_blocks", "bundle_precondition", "bundle_cg_start",
 * "bundle_cg_track", "bundle_cg_cam", "bundle_cg_step", "bundle_move", "bundle_cost", "bundle_commit", "bundle_finish".
 * d_ws: spv_bundle_adjust_workspace_bytes(nseg, ntracks, nmembers) bytes, aligned to 256.
 * spv_bundle_adjust_plan: host only, touches no device.  out = {lane-form tracks, wave-form tracks, view-major chunk
 * size, chunks, longest track}; chunks counts those of the mode 1 sets (every set where mode is NULL) when every usable
 * member of a track with two or more takes part, and is 0 where members (host int32[nmembers, 2]) is NULL, in which
 * case seg_off, nseg and mode are not read.
 * SPV_ERR_INVALID, nothing launched: the seg_off and track_off rules of spv_tracks_triangulate_device; nseg *
 * ceil(nmembers / 256) >= 2^31; a mode outside {0, 1, 2}; a K row that breaks the shape above; an R with |R^T R - I|
 * or |det R - 1| above 1e-6, or non-finite, in a set with mode != 0; a NaN or non-positive huber; a NaN or negative
 * lambda0, ftol, gtol or cg_tol; a negative max_steps or cg_max; a NULL required pointer (as there, and K, poses, mode
 * where nseg > 0, info); an output not aligned to its element size; a workspace that is missing, short or misaligned.
 * spv_bundle_adjust: host pointers (X, use, err, active on the host), on the first selected device; touches no device
 * when ntracks is 0 or no set has mode != 0. */
int spv_bundle_adjust_plan(const long long *track_off, int ntracks, const int32_t *members, const long long *seg_off,
                           int nseg, const int32_t *mode, long long out[5]);
size_t spv_bundle_adjust_workspace_bytes(int nseg, int ntracks, long long nmembers);
int spv_bundle_adjust_device(const float *d_geom, const long long *seg_off, int nseg, const double *K, double *poses,
                             const int32_t *mode, const long long *track_off, int ntracks, const int32_t *d_members,
                             long long nmembers, double *d_X, const uint8_t *d_use, double huber, int max_steps,
                             double lambda0, double ftol, double gtol, double cg_tol, int cg_max, double *d_err,
                             uint8_t *d_active, double *trace, double *info, void *d_ws, size_t ws_bytes, void *stream);
int spv_bundle_adjust(const float *geom, const long long *seg_off, int nseg, const double *K, double *poses,
                      const int32_t *mode, const long long *track_off, int ntracks, const int32_t *members,
                      long long nmembers, double *X, const uint8_t *use, double huber, int max_steps, double lambda0,
                      double ftol, double gtol, double cg_tol, int cg_max, double *err, uint8_t *active, double *trace,
                      double *info);

/* normalize_to_ubyte_and_multiple_16_dim (reference spectavi/feature.py:384-407) for a float32
 * input, bit for bit what numpy computes: per-column de-mean (numpy's row-ordered float32 sum),
 * divide by the per-column max-abs, x128, round half-to-even, clip to [-128,127], zero-pad the
 * columns to dim16 = roundup(dim,16).  out_f32 float32[rows,dim16] and/or out_u8 =
 * uint8(out + 128)[rows,dim16] (either may be NULL, not both). */
int spv_normalize(const float *x, int rows, int dim, float *out_f32, uint8_t *out_u8);
size_t spv_normalize_workspace_bytes(int dim);
/* A larger workspace (it grows with rows) with which spv_normalize_device computes the column sums
 * of a table of 65536 rows or more by folding 1024-row chunks instead of walking every row: the same
 * bits, 1.5x (full SIFT tables) to 3.7x (integer-valued tables) faster at a million rows.  With only spv_normalize_workspace_bytes(dim) it walks. */
size_t spv_normalize_workspace_bytes_rows(int rows, int dim);
int spv_normalize_device(const float *d_x, int rows, int dim, float *d_out_f32, uint8_t *d_out_u8,
                         void *d_ws, size_t ws_bytes, void *stream);

/* spv_normalize_device for every table of a collection in one fixed chain of launches (normalize_batch.hip): the
 * step between spv_sift_batch (or spv_sift_split) and spv_cascade_batch_device, whose rows are the normalised tables.
 *   x        dtype[seg_off[nseg], dim]: the tables of nseg sets back to back; SPV_NORMALIZE_F32 float32, or
 *            SPV_NORMALIZE_U8 uint8, whose values stand for their float32 conversions (no float copy is made).
 *   seg_off  the seg_off of spv_l1k2_batch_device: host long long[nseg + 1], non-decreasing, seg_off[0] = 0,
 *            seg_off[nseg] = total < 2^31; set s is rows [seg_off[s], seg_off[s + 1]) and may be empty.
 *   out_f32  float32[total, dim16], out_u8 uint8[total, dim16], dim16 = roundup(dim, 16); either may be NULL, not both.
 * For every set the rows [seg_off[s], seg_off[s + 1]) of both outputs are bit for bit what spv_normalize_device
 * writes for that set alone (for SPV_NORMALIZE_U8: for that set's rows converted to float32), whatever else the
 * collection holds, wherever the set stands in it and however the call cuts the work: the padding columns, and the
 * NaN rows (and their uint8 image) of a constant column or a one-row set, which divide 0 by 0, included.  Every
 * element of every non-empty set's rows is written exactly once; nothing else is touched.
 * SPV_ERR_INVALID, nothing launched, no output touched: a seg_off outside the rules, nseg < 0, dim < 1 or
 * dim > 2048, dim == 1 with any set of more than one row (the single call's refusal), an unknown dtype, a NULL
 * required pointer (x, the workspace: only where total > 0), a workspace shorter than the size query's or not
 * 16-byte aligned, a d_x or d_out_f32 not aligned to its element size.  nseg = 0 and all-empty collections are valid
 * and launch nothing.  One device; asynchronous on `stream` but for the upload of its small item and segment
 * tables, which the call waits for.  Very large single tables remain the job of spv_normalize_device (its folded
 * column sums are not taken here).
 *
 * The launches (kernel names for spv_profile_read): "normalize_batch_stats", SPV_NORMALIZE_U8 only -- per work
 * item (256 rows of one set) and column the integer sum, minimum and maximum; "normalize_batch_finish" -- per (set,
 * 16-column block): where every integer column sum of the block is at most 2^24 it IS numpy's row-ordered float32
 * sum (every prefix is an integer that float32 holds: any uint8 set of up to 65793 rows), so mean = float(S) /
 * float(rows); every other block, and every float32 set, is walked in row order as spv_normalize_device does, its
 * minimum and maximum taken on the way; "normalize_batch" -- the element-wise pass over the same work items.
 * "normalize" does not tick.
 *
 * spv_normalize_batch_plan: host only, touches no device.  out = {non-empty sets, work items, workspace bytes, total
 * rows}; items may be NULL, otherwise int32[items_cap, 3] receives the first min(work items, items_cap) work items as
 * (set, first row within the set, rows): exactly the list the device call walks, in its order -- set by set, rows
 * in order, every row once, no item in two sets.  compute_units >= 1 caps the grid (32 workgroups per compute
 * unit, each walking items b, b + grid, ...) and does not change the items.  SPV_ERR_INVALID leaves out and items
 * untouched.  spv_normalize_batch_workspace_bytes: out[2] (0 for arguments the plan rejects): 12 bytes per work
 * item, 8 per set, the statistics float32[nseg, 2, dim], and for SPV_NORMALIZE_U8 4 bytes per work item and column,
 * each piece rounded up to 256.
 * spv_normalize_batch: host pointers, on the first selected device; touches none when total is 0. */
#define SPV_NORMALIZE_F32 0
#define SPV_NORMALIZE_U8 1
int spv_normalize_batch_plan(const long long *seg_off, int nseg, int dim, int dtype, int compute_units,
                             long long out[4], int32_t *items, long long items_cap);
size_t spv_normalize_batch_workspace_bytes(const long long *seg_off, int nseg, int dim, int dtype);
int spv_normalize_batch_device(const void *d_x, int dtype, const long long *seg_off, int nseg, int dim,
                               float *d_out_f32, uint8_t *d_out_u8, void *d_ws, size_t ws_bytes, void *stream);
int spv_normalize_batch(const void *x, int dtype, const long long *seg_off, int nseg, int dim,
                        float *out_f32, uint8_t *out_u8);

/* Device form of spv_dlt_score_hypotheses: P0 is a HOST pointer (12 doubles), d_P1s
 * double[nhyp,12], d_counts int32[nhyp] (zeroed by the call), d_mask uint8[nhyp,npt] or NULL. */
int spv_dlt_score_hypotheses_device(const double *P0, const double *d_P1s, int nhyp,
                                    long long npt, const double *d_x, const double *d_xp,
                                    double max_error, int32_t *d_counts, uint8_t *d_mask,
                                    void *stream);
/* The same with a workspace (spv_dlt_score_workspace_bytes): the solves that do not converge on the
 * fast path are collected in a work list and finished by a second kernel in full waves instead of
 * in place -- same results, about three times the throughput on RANSAC-like hypotheses.  A NULL or
 * short workspace falls back to the one-pass form. */
size_t spv_dlt_score_workspace_bytes(int nhyp, long long npt);
int spv_dlt_score_hypotheses_device_ws(const double *P0, const double *d_P1s, int nhyp, long long npt,
                                       const double *d_x, const double *d_xp, double max_error,
                                       int32_t *d_counts, uint8_t *d_mask, void *d_ws, size_t ws_bytes,
                                       void *stream);

#ifdef __cplusplus
}
#endif

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#endif /* SPECTAVI_AMD_H */
