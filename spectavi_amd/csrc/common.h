// common.h -- shared host-side helpers for libspectavi.so (gfx950 build).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <algorithm>
#include <exception>
#include <functional>
#include <mutex>
#include <new>
#include <random>
#include <type_traits>
#include <vector>

#include "../../include/spectavi_amd.h"
#include "collection.h"

namespace spv {

// Records status + message for the calling thread; returns `status`.
int set_error(int status, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void clear_error();

#define SPV_HIP_CHECK(expr)                                                              \
  do {                                                                                   \
    hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) {                                                              \
      return ::spv::set_error(_e == hipErrorOutOfMemory ? SPV_ERR_NOMEM : SPV_ERR_HIP,   \
                              "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),     \
                              __FILE__, __LINE__);                                       \
    }                                                                                    \
  } while (0)

#define SPV_TRY(expr)            \
  do {                           \
    int _s = (expr);             \
    if (_s != SPV_OK) return _s; \
  } while (0)

// No C++ exception may cross the extern "C" boundary (the reference's own symbols let them
// escape into libffi and abort the process, src/BruteForceNnL1K2.h:75,79): every entry point,
// and every host thread a call runs a shard on, runs its body through this.
template <typename Fn>
int guard(Fn fn) {
  try {
    return fn();
  } catch (const std::bad_alloc &) {
    return set_error(SPV_ERR_NOMEM, "host allocation failed");
  } catch (const std::exception &e) {
    return set_error(SPV_ERR_INTERNAL, "unexpected C++ exception: %s", e.what());
  } catch (...) {
    return set_error(SPV_ERR_INTERNAL, "unexpected C++ exception");
  }
}

// Selects the process-wide device for host-pointer entry points on this thread.
int ensure_device();

// Compute units of the calling thread's current device (cached per device; 256 on MI355X).
int device_cu_count();

// Brackets a kernel launch with hipEvents on `stream` while profiling is enabled.
struct ProfScope {
  ProfScope(const char *name, hipStream_t stream);
  ~ProfScope();
  const char *name_;
  hipStream_t stream_;
  hipEvent_t start_ = nullptr;
};

inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A workspace layout is stated once, as a function of the shape that takes its pieces from a WsWalk one after
// another.  The size query walks it from a null base and reports end(); the run walks it from the caller's buffer,
// gets its pointers and holds the same end() against the bytes it was given.  A piece starts on a multiple of 256
// bytes from the base and takes at least min_piece bytes.
struct WsWalk {
  explicit WsWalk(void *base = nullptr, size_t min_piece = 0) : base_(static_cast<unsigned char *>(base)), min_(min_piece) {}
  size_t reserve(size_t bytes) {  // the offset of the next piece
    const size_t at = end_;
    end_ += round_up(std::max(bytes, min_), 256);
    return at;
  }
  template <typename T = unsigned char>
  T *take(size_t bytes) {  // the next piece itself; null on a walk without a base
    const size_t at = reserve(bytes);
    return base_ ? reinterpret_cast<T *>(base_ + at) : nullptr;
  }
  size_t end() const { return end_; }

 private:
  unsigned char *base_;
  size_t min_, end_ = 0;
};

// Small compile-time tables of template arguments.  pick: f(std::integral_constant<int, V>{}), a launch that
// returns true, for the first V among Vs that equals v; false if there is none.  first_at_least: the first V >= v
// (Vs ascending), else 0.  hipcc emits kernel instantiations in the order the host code first names them: pick is
// a left fold, and the lists name their values in the order the code objects have always had.
template <int... Vs> struct Ints {};
template <int... Vs, typename F>
bool pick(Ints<Vs...>, int v, F f) {
  return (... || (v == Vs && f(std::integral_constant<int, Vs>{})));
}
template <int... Vs>
int first_at_least(Ints<Vs...>, int v) {
  int r = 0;
  ((r == 0 && v <= Vs ? r = Vs : 0), ...);
  return r;
}

// ---- L1 2-NN (l1k2.hip, l1k2_prune.hip) ---------------------------------------------
// The SPECTAVI_L1K2_* variables, read once per process.
struct L1K2Knobs {
  int q;             // SPECTAVI_L1K2_Q: queries per lane (1, 2 or 4; anything else: the plan's own choice)
  int blocks;        // SPECTAVI_L1K2_BLOCKS: workgroups the slicing aims for
  int prune;         // SPECTAVI_L1K2_PRUNE: the prune mode a process starts with (-1 auto, 0 never, 1 wherever possible)
  int prune_share;   // SPECTAVI_L1K2_PRUNE_SHARE: hand-over share in 1/1024 (-1: the measured break-even)
  int prune_octet;   // SPECTAVI_L1K2_PRUNE_OCTET: most pairs a survivor pass takes eight lanes per pair for (-1: the measured crossover; 0: never)
  bool prune_stats;  // SPECTAVI_L1K2_PRUNE_STATS=1: the bound path prints its counters (synchronises)
  int bound;         // SPECTAVI_L1K2_BOUND: the bound table a process starts with (-1 default, 0 recipe, 1 tuned)
  int prune_form;    // SPECTAVI_L1K2_PRUNE_FORM: the form of the bound kernel a process starts with (-1 default, 0 narrow, 1 wide)
  int prune_matrix;  // SPECTAVI_L1K2_PRUNE_MATRIX=default|i8|fp6: the matrix format of the wide form's bound a process starts with (-1, 0, 1)
};
const L1K2Knobs &l1k2_knobs();

enum L1K2Path {
  kL1K2Tile,   // l1k2_tile_kernel<dim_pad / 4, q>
  kL1K2Wide,   // l1k2_wide_kernel<q>: widths above 256
  kL1K2Bound,  // l1k2_prune.hip, then l1k2_tile_kernel<32, 2, 128> over its work list: dim 128, where the prune mode says so
};
// Everything l1k2_run launches for a shape under the knobs and the prune mode of the moment.  The workspace
// layout and all that spv_l1k2_plan reports are a function of the shape and the knobs alone: the prune mode
// only turns kL1K2Tile into kL1K2Bound.
struct L1K2Plan {
  int dim_pad;     // kernel row width in bytes (>= dim, zero padded); < 0: no kernel takes this width
  int q;           // queries per lane
  int slice_rows;  // database rows per slice (<= 65536)
  int slices;      // number of database slices
  int qblocks;     // query blocks
  bool padded;     // pad_rows_kernel copies both sides to dim_pad first
  L1K2Path path;
  int merge_lanes;       // l1k2_merge_kernel<1 | 8 | 64>: lanes per query
  dim3 grid;             // tile kernel: (query blocks, slices); wide kernel: one XCD-padded row of both
  size_t wide_lds;       // wide kernel: dynamic LDS bytes
  dim3 bound_grid;       // l1k2_prune_kernel: (blocks of 256 queries, slices)
  int bound;             // ... and the table it runs with (kL1K2BoundRecipe / kL1K2BoundTuned)
  int form;              // ... and the form that runs (kL1K2FormNarrow / kL1K2FormWide)
  int matrix;            // ... and its matrix format (kL1K2MatrixI8 / kL1K2MatrixFp6; FP6 runs its own table, l1k2_bound6, whatever `bound` says)
  dim3 bound_wide_grid;  // l1k2_prune_wide_kernel: (blocks of 512 queries, slices)
  unsigned work_grid;    // tile kernel over the bound path's work list: kWorkSub blocks for every workgroup there
  unsigned merge_grid;
  size_t thr_words;      // bound path: shared thresholds (an even number: the counters behind them are 64-bit)
  size_t init_words;     // ... and the dwords l1k2_thr_init_kernel sets: thresholds, counters, the work list's header
  // workspace: byte offsets, in this order.  Padded copies (empty unless `padded`), partial top-2 keys, then the
  // bound path's scratch (empty unless dim 128 with >= 32 database rows): int8 features, shared thresholds, counters,
  // work list {count, -, (query block of 256, slice) ...} of the workgroups that gave the bound up.
  size_t off_pad_x, off_pad_y, off_part, off_feat_x, off_feat_y, off_thr, off_stats, off_work, total_bytes;
};
L1K2Plan l1k2_plan(int xrows, int yrows, int dim);  // host only
int l1k2_run(const uint8_t *d_x, const uint8_t *d_y, int xrows, int yrows, int dim,
             uint64_t *d_idx, int32_t *d_dist, void *d_ws, size_t ws_bytes, hipStream_t stream);

// l1k2.hip's pad_rows_kernel on `stream`: rows of dim bytes -> rows of dim_pad bytes, zero filled (both multiples of 16)
void l1k2_pad_rows(const uint8_t *d_src, uint8_t *d_dst, size_t rows, int dim, int dim_pad, hipStream_t stream);

// ---- L1 2-NN of many descriptor-set pairs in one launch (l1k2_batch.hip, l1k2_guided.hip) ---------------
// One workgroup's share of a collection: query rows of one pair's query set against one slice of its database set.
struct L1K2BatchItem {
  int32_t pair, y0, yrows, x0, xrows;  // pair; first query row within the query set, query rows; first database row within the database set, database rows
};
// How l1k2_slice_plan cuts a collection into items, in plain numbers.  `whole` being the items with whole database
// sets, every set is cut ceil(aim / whole) ways into slices of whole 64-row tiles, none (but a set's last) shorter
// than floor_few rows while whole < fill, than floor_full from there on, and none longer than cap.
struct L1K2SliceRule {
  int qrows;  // query rows per item
  long long aim, fill, floor_few, floor_full, cap;
};
// The part of a plan the two L1 forms share, and all of the guided form's.
struct L1K2SlicePlan {
  int max_slices;   // largest number of database slices of any pair
  long long total_rows, out_rows;
  std::vector<long long> out_off;    // [npairs + 1]: pair p owns out rows [out_off[p], out_off[p + 1])
  std::vector<L1K2BatchItem> items;  // the grid, longest item first
  // workspace: byte offsets, in this order.  The out rows' pairs of 64-bit keys, the device form of `items`.
  size_t off_keys, off_items, total_bytes;
};
// Of a checked collection: all of *p but the workspace offsets.  SPV_ERR_INVALID for more items than a grid takes.
int l1k2_slice_plan(const long long *seg_off, int nseg, const int32_t *pairs, int npairs, const L1K2SliceRule &rule,
                    L1K2SlicePlan *p);
// The plan's items as the kernels read them into d_items (the one wait of a run: the upload has ended on return)
// and "none" into the out rows' keys d_keys; then, after the main kernel, keys -> idx, dist and their sentinels
// under the ProfScope name `prof`.
int l1k2_work_upload(const L1K2SlicePlan &p, const long long *seg_off, const int32_t *pairs, void *d_items,
                     unsigned long long *d_keys, hipStream_t stream);
int l1k2_keys_finish(const char *prof, const unsigned long long *d_keys, long long out_rows, uint64_t *d_idx,
                     int32_t *d_dist, hipStream_t stream);
// Everything l1k2_batch_run launches for a collection under the SPECTAVI_L1K2_Q / SPECTAVI_L1K2_BLOCKS knobs: an
// item is 256 q queries.  The workspace ends with the padded copy of desc (empty unless `padded`).
struct L1K2BatchPlan : L1K2SlicePlan {
  int dim_pad;      // kernel row width in bytes (>= dim, zero padded)
  int q;            // queries per lane, one value for the whole call
  bool padded;      // pad_rows_kernel copies the whole of desc to dim_pad first
  size_t off_pad;
};
// SPV_ERR_INVALID (message set, *p untouched) outside the limits of include/spectavi_amd.h; host only
int l1k2_batch_plan(const long long *seg_off, int nseg, int dim, const int32_t *pairs, int npairs, L1K2BatchPlan *p);
int l1k2_batch_run(const uint8_t *d_desc, const long long *seg_off, int nseg, int dim, const int32_t *pairs, int npairs,
                   uint64_t *d_idx, int32_t *d_dist, void *d_ws, size_t ws_bytes, hipStream_t stream);

// ---- L1 2-NN inside a band around each query's line, many pairs (l1k2_guided.hip) -----
// Everything l1k2_guided_run launches for a collection.  An item is 256 queries of one pair against one slice of
// its database set.
using L1K2GuidedPlan = L1K2SlicePlan;
// SPV_ERR_INVALID (message set, *p untouched) outside the limits of include/spectavi_amd.h; host only
int l1k2_guided_plan(const long long *seg_off, int nseg, int dim, const int32_t *pairs, int npairs, L1K2GuidedPlan *p);
int l1k2_guided_run(const uint8_t *d_desc, const float *d_geom, const long long *seg_off, int nseg, int dim,
                    const int32_t *pairs, int npairs, const double *d_lines, double max_dist, uint64_t *d_idx,
                    int32_t *d_dist, int32_t *d_ncand, void *d_ws, size_t ws_bytes, hipStream_t stream);
// G host double[npairs, 9], use host int32[npairs] or null; asynchronous on `stream`
int epipolar_lines_run(const float *d_geom, const long long *seg_off, int nseg, const int32_t *pairs, int npairs,
                       const double *G, const int32_t *use, double *d_lines, hipStream_t stream);

// ---- matrix-core lower bound for the L1 2-NN at dim 128 (l1k2_prune.hip) -------------
struct L1K2Bound {
  int8_t phi[256][4];  // features of a byte value
  int p, m;            // p |a-b| >= m - phi(a).phi(b) for all bytes a, b
  bool ok;             // the table passed its exhaustive check
};
enum { kL1K2BoundRecipe = 0, kL1K2BoundTuned = 1 };           // the cosine recipe; the optimised table of l1k2_bound_tuned.h
const L1K2Bound &l1k2_bound();                               // the recipe; host only, built once
const L1K2Bound &l1k2_bound_of(int which);                   // either table, each built once; a tuned table that fails its check is the recipe
int l1k2_set_bound(int which);                               // -1 default (tuned under prune mode auto, the recipe under mode 1), 0, 1; returns the setting before
int l1k2_get_bound();
enum { kL1K2FormNarrow = 0, kL1K2FormWide = 1 };             // l1k2_prune_kernel (32-row tiles, 256 queries); l1k2_prune_wide_kernel (64, 512)
int l1k2_set_prune_form(int form);                           // -1 default (wide where `auto` takes the path and the grid fills the chip), 0, 1; returns the setting before
int l1k2_get_prune_form();
// The rank-5 FP6 table of l1k2_bound_fp6.h: an entry is the integer k of the e2m3 value k/8, p and m are in units of 1/64.
struct L1K2Bound6 {
  int8_t k[256][5];
  int p, m;            // p |a-b| >= m - k(a).k(b) for all bytes a, b
  bool ok;             // on the e2m3 grid, the inequality on every byte pair, and every sum exact in f32
};
const L1K2Bound6 &l1k2_bound6();                             // host only, built once
enum { kL1K2MatrixI8 = 0, kL1K2MatrixFp6 = 1 };              // l1k2_prune_wide_kernel; l1k2_prune_wide6_kernel
int l1k2_set_prune_matrix(int matrix);                       // -1 default (FP6 where `auto` takes the path, the form is wide and the table the default one), 0, 1; returns the setting before
int l1k2_get_prune_matrix();
int l1k2_set_prune(int mode);                                // -1 auto, 0 never, 1 wherever possible; returns the mode before
int l1k2_get_prune();
// The bound path's part of a plan whose slicing is done: its scratch, the next pieces of the plan's walk, and
// path / bound_grid where the prune mode takes the path for this shape.
void l1k2_prune_plan(int xrows, int yrows, int dim, WsWalk *w, L1K2Plan *p);
// features, thresholds and the bound-and-survivor kernel; writes the partial keys l1k2_merge_kernel reads, but
// for the workgroups on the work list, whose keys l1k2_run has yet to compute with the tile kernel
int l1k2_prune_run(const uint8_t *d_x, const uint8_t *d_y, int xrows, int yrows, const L1K2Plan &p, uint8_t *ws,
                   hipStream_t stream);
// l1k2_run notes where the counters of the calling thread's run lie, or null: it took the tile kernels
void l1k2_prune_note_run(const void *d_stats, hipStream_t stream);
// {pairs bounded, survivors, pairs of the exact fallback} of the calling thread's last l1k2_run (zeros: tile kernels);
// waits for that launch; its workspace must still be allocated
int l1k2_prune_last_stats(unsigned long long out[3]);

// ---- exact p-norm k-NN (bruteforce.hip) ---------------------------------------------
struct BruteForcePlan {
  int qblocks;       // query blocks of 256
  int slice_rows;    // database rows per slice
  int slices;        // database slices
  size_t part_bytes; // per-slice top-k keys (the whole workspace)
};
int bruteforce_p_kind(double p);  // 0: p = 1, 1: p = 2, 2: p = 0.5, 3: any other p
// SPV_ERR_INVALID (message set) outside the limits of include/spectavi_amd.h; touches no device
int bruteforce_check(int xrows, int yrows, int dim, int k, float p);
// slices > 0 forces that many database slices (fewer if some would be empty)
BruteForcePlan bruteforce_plan(int xrows, int yrows, int k, int slices);
int bruteforce_run(const void *d_x, const void *d_y, int is_int, int xrows, int yrows, int dim, int k, float p,
                   int slices, uint64_t *d_idx, void *d_dist, void *d_ws, size_t ws_bytes, hipStream_t stream);

// ---- approximate L2 k-NN: bf16 matrix-core score, exact re-rank (ann.hip) -------------
// Everything ann_run launches for a shape.
struct AnnPlan {
  int kpad;        // row width of the bf16 images (dim rounded up to 32)
  int qtile;       // queries per workgroup of the coarse kernel
  int rtile;       // database rows per tile
  int slices;      // database slices
  int slice_rows;  // database rows per slice
  int ncand;       // candidates per query in force
  int buflen;      // keys in the survivor buffer of one (query, slice)
  int mfma;        // 32: mfma_f32_32x32x16_bf16, 16: mfma_f32_16x16x32_bf16 (SPECTAVI_ANN_MFMA, for measurements)
  bool all_rows;   // xrows <= ncand: every row is a candidate, only the re-rank runs
  int qblocks;     // query blocks
  int chunks;      // partial column sums
  // workspace: byte offsets, in this order
  size_t off_part, off_mean, off_xb, off_yb, off_norm, off_cand, off_cnt, off_buf, total_bytes;
};
// SPV_ERR_INVALID (message set) outside the limits of include/spectavi_amd.h; touches no device
int ann_check(int xrows, int yrows, int dim, int k, int ncand);
// slices > 0 forces that many database slices (fewer if some would be empty); host only
AnnPlan ann_plan(int xrows, int yrows, int dim, int k, int ncand, int slices);
int ann_run(const float *d_x, const float *d_y, int xrows, int yrows, int dim, int k, int ncand, int slices,
            uint64_t *d_idx, float *d_dist, void *d_ws, size_t ws_bytes, hipStream_t stream);

// ---- cascade hash (cascade.hip) -----------------------------------------------------
constexpr int kCascadeMaxDim = 2048;  // the widest row the refine kernels take
// Everything cascade_run decides for a shape under the SPECTAVI_CASCADE_* knobs of the moment.
struct CascadePlan {
  // workspace layout
  int mc, hb;  // accumulators per table of the VALU projection (m rounded up to 4); bucket bits
  size_t off_dictp, off_dictm, off_ux, off_uy, off_xcodes, off_ysign, off_ymask, off_bstart,
      off_order, off_ranks, off_segsum, off_qbstart, off_qorder, off_qranks, off_partial, off_pvisited, total;
  // projection: 0 project_kernel<MC, NT>, 1 project_mfma_kernel<CT, FULL>, 2 project_mfma4_kernel<CT, NG>
  int family, pa, pb;
  int gmax_q;          // GMAX of the query side (the database side is always 1)
  int proj_rows;       // rows per workgroup of that kernel
  bool use_group;      // probe_table_kernel (one 8-lane group per query), else probe_refine_kernel
  bool sorted;         // the group probe walks the queries in the order of each table's sign code
  bool qhist_fused;    // sorted: query histogram + ranks in the projection's epilogue, else query_rank_kernel
  int cpl, ru, wpe;    // the probe's template parameters (wpe, shift, full: probe_table_kernel only)
  bool shift, full;
  int dshift;          // ceil(log2(dim))
  int nblk, per_xcd;   // group probe: query blocks, blocks per XCD range (0: unsorted)
  unsigned probe_grid;
};
CascadePlan cascade_plan(int xrows, int yrows, int dim, int m, int n, int g);  // host only
size_t cascade_workspace_bytes(int xrows, int yrows, int dim, int m, int n, int g);
int cascade_run(const float *d_x, const float *d_y, int xrows, int yrows, int dim, int m, int n,
                int g, const float *d_dict, uint64_t *d_idx, float *d_dist, int32_t *d_ncand,
                void *d_ws, size_t ws_bytes, hipStream_t stream);

// ---- cascade hash of many set pairs in one chain of launches (cascade_batch.hip) --------
constexpr int kCascadeBatchMaxDim = 256;        // the limit of the other many-pairs forms
constexpr int kCascadeBatchMaxTables = 65535;   // nseg * n: the scan kernels take the (set, table) as blockIdx.y
constexpr int kCascadeBatchItemRows = 64;       // query rows per work item
// One workgroup's share of a collection: rows [y0, y0 + yrows) of one pair's query set.
struct CascadeBatchItem {
  int32_t pair, y0, yrows;
};
// Everything cascade_batch_run launches for a collection.
struct CascadeBatchPlan {
  CascadePlan proj;  // the projection of all rows in the query form: family, pa, pb, gmax_q, proj_rows, mc
  int hb;            // bucket bits of every (set, table); hb < m: the probe compares full codes
  long long total_rows, out_rows;
  std::vector<long long> out_off;       // [npairs + 1]: pair p owns out rows [out_off[p], out_off[p + 1])
  std::vector<CascadeBatchItem> items;  // the probe's grid, in pair order
  // workspace: byte offsets, in this order.  The device form of `items` followed by seg_off as uint32, the repacked
  // dictionary, the uint8 image, sign codes / masks / ranks / order [n][total_rows], the bucket offsets
  // [nseg * n][2^hb + 1], the scan's segment sums.
  size_t off_tables, off_dict, off_img, off_codes, off_masks, off_ranks, off_order, off_bstart, off_segsum, total_bytes;
};
// SPV_ERR_INVALID (message set, *p untouched) outside the limits of include/spectavi_amd.h; host only
int cascade_batch_plan(const long long *seg_off, int nseg, int dim, int m, int n, int g, const int32_t *pairs,
                       int npairs, CascadeBatchPlan *p);
int cascade_batch_run(const float *d_rows, const long long *seg_off, int nseg, int dim, int m, int n, int g,
                      const int32_t *pairs, int npairs, const float *d_dict, uint64_t *d_idx, float *d_dist,
                      int32_t *d_ncand, void *d_ws, size_t ws_bytes, hipStream_t stream);

// ---- DLT (dlt.hip) ------------------------------------------------------------------
int dlt_run(const double *P0, const double *P1, long long npt, const double *d_x,
            const double *d_xp, double *d_dst, bool want_error, hipStream_t stream);

// ---- epipolar rectification (rectify.hip) --------------------------------------------
// out = {output_rows, output_cols, rnx}; SPV_ERR_INVALID (message set) outside the header's limits
int rectify_shape(int wid, int hgt, int nchan, double sf, int out[3]);
void rectify_fundamental(const double *P0, const double *P1, double *F);  // host only
int rectify_run(const double *F, const void *d_im0, const void *d_im1, int dtype, int wid, int hgt, int nchan,
                double sf, void *d_r0, void *d_r1, int32_t *d_ri0, int32_t *d_ri1, hipStream_t stream);

// ---- epipolar rectification of many image pairs in one call (rectify_batch.hip) ---------
constexpr int kRectifyBatchRows = 8;             // window rows per work item
constexpr int kRectifyBatchGroupsPerCu = 32;     // the grid cap: workgroups per compute unit, each walking its items
constexpr int kRectifyBatchMaxPairs = 1 << 20;   // the limit of the other many-pairs forms
// One workgroup's share of a collection: rows [row0, row0 + rows) of pair `pair`'s uncropped frame, all inside its
// window, in image `img` (0 or 1) of the pair.
struct RectifyBatchItem {
  int32_t pair, img, row0, rows;
};
// Everything rectify_batch_run launches for a collection, a function of the shapes, `use` and the boxes alone.
struct RectifyBatchPlan {
  long long used = 0;
  std::vector<long long> img_off;       // [nimg + 1]: pixels before every image of the packed array
  std::vector<int32_t> frame;           // [npairs, 3]: rectify_shape of every used pair (zero where not used)
  std::vector<int32_t> box;             // [npairs, 4]: the window in force (zero where not used)
  std::vector<long long> out_off;       // [npairs + 1]: pair p owns samples [out_off[p], out_off[p + 1])
  std::vector<RectifyBatchItem> items;  // pair by pair, image 0's row blocks then image 1's
};
// box: host int32[npairs, 4] or null for whole frames.  SPV_ERR_INVALID (message set, *p untouched) for what
// include/spectavi_amd.h rejects; host only
int rectify_batch_plan(const int32_t *sizes, int nimg, int nchan, double sf, const int32_t *pairs, int npairs,
                       const int32_t *use, const int32_t *box, RectifyBatchPlan *p);
// Device outputs as in include/spectavi_amd.h; asynchronous on `stream` but for the upload of the call's tables.
int rectify_batch_bounds_run(const int32_t *sizes, int nimg, int nchan, double sf, const int32_t *pairs, int npairs,
                             const double *P0s, const double *P1s, const int32_t *use, int32_t *d_box,
                             hipStream_t stream);
int rectify_batch_run(const void *d_images, int dtype, const int32_t *sizes, int nimg, int nchan, double sf,
                      const int32_t *pairs, int npairs, const double *P0s, const double *P1s, const int32_t *use,
                      const int32_t *box, void *d_r0, void *d_r1, int32_t *d_ri0, int32_t *d_ri1, hipStream_t stream);

// ---- dense SAD disparity of many rectified pairs (stereo_batch.hip) ---------------------
constexpr int kStereoRows = 4;          // window rows per work item: one wave each
constexpr int kStereoCols = 64;         // window columns per work item: one lane each
constexpr int kStereoGroupsPerCu = 32;  // the grid cap: workgroups per compute unit, each walking its items
// One workgroup's share of a collection: rows [row0, row0 + rows) and columns [col0, min(col0 + 64, C)) of pair
// `pair`'s window.
struct StereoBatchItem {
  int32_t pair, row0, rows, col0;
};
// Everything stereo_batch_run launches for a collection, a function of the boxes and `use` alone.
struct StereoBatchPlan {
  long long used = 0;
  std::vector<long long> out_off;      // [npairs + 1]: the running areas of all boxes
  std::vector<StereoBatchItem> items;  // pair by pair, band by band, tile by tile: used pairs only
};
// SPV_ERR_INVALID (message set, *p untouched) for what include/spectavi_amd.h rejects; drange may be null; host only
int stereo_batch_plan(const int32_t *box, int npairs, const int32_t *use, int radius, const int32_t *drange,
                      StereoBatchPlan *p);
// Device outputs as in include/spectavi_amd.h; asynchronous on `stream`.
int stereo_batch_run(const uint8_t *d_r0, const uint8_t *d_r1, const int32_t *d_ri0, const int32_t *d_ri1,
                     const int32_t *box, int npairs, const int32_t *use, int radius, const int32_t *drange, int swap,
                     int32_t *d_disp, uint16_t *d_cost, uint16_t *d_cost2, hipStream_t stream);
int stereo_keep_batch_run(const int32_t *box, int npairs, const int32_t *d_disp0, const uint16_t *d_cost0,
                          const uint16_t *d_cost20, const int32_t *d_disp1, int lr_tol, int uniqueness, uint8_t *d_keep,
                          hipStream_t stream);
int stereo_matches_batch_run(const int32_t *box, int npairs, const int32_t *sizes, int nimg, const int32_t *pairs,
                             const int32_t *d_disp0, const uint8_t *d_keep, const int32_t *d_ri0, const int32_t *d_ri1,
                             long long capacity, double *d_x0, double *d_x1, int32_t *d_rows, long long *d_pair_off,
                             hipStream_t stream);

// ---- vlfeat-exact SIFT (sift.hip) ----------------------------------------------------
constexpr int kSiftMaxSide = 8192;  // candidates pack x, y of octave -1 in 15 bits each; counts stay below 2^31
int sift_check(int wid, int hgt);   // SPV_ERR_INVALID (message set) outside the header's limits
int sift_noctaves(int wid, int hgt);
size_t sift_workspace_bytes(int wid, int hgt);
// Writes rows [0, min(count, capacity)) of d_table float32[capacity,132] and the true row count to
// *d_count; asynchronous on `stream`.
int sift_run(const float *d_im, int wid, int hgt, void *d_ws, size_t ws_bytes, float *d_table, int capacity,
             int *d_count, hipStream_t stream);

// ---- SIFT of many images in one chain of launches (sift.hip) ---------------------------
constexpr int kSiftBatchMaxImages = 65535;  // the image is grid dimension y or z
// How a call cuts its images, in order, into groups that share the workspace one after another.
struct SiftBatchPlan {
  std::vector<std::pair<int, int>> groups;  // (first image, images)
  size_t all_bytes = 0;                     // workspace with which only kSiftBatchMaxImages closes a group
  size_t min_bytes = 0;                     // the most demanding single image's slice
  long long pixels = 0;
};
// sizes int32[nimg, 2] = (wid, hgt); ws_bytes = 0: as much as needed.  SPV_ERR_INVALID (message set, *p untouched)
// for what include/spectavi_amd.h rejects; host only
int sift_batch_plan(const int32_t *sizes, int nimg, size_t ws_bytes, SiftBatchPlan *p);
// Device outputs as in include/spectavi_amd.h; asynchronous on `stream` but for the upload of the images' records.
int sift_batch_run(const float *d_images, const int32_t *sizes, int nimg, void *d_ws, size_t ws_bytes, float *d_table,
                   const long long *cap_off, int32_t *d_counts, hipStream_t stream);
int sift_batch_pack_run(const float *d_table, const long long *cap_off, const long long *seg_off, int nimg,
                        float *d_packed, float *d_geom, uint8_t *d_desc, hipStream_t stream);

// ---- ratio test + compaction (match.hip) ---------------------------------------------
size_t ratio_workspace_bytes(int yrows);
int ratio_run(const uint64_t *d_idx, const void *d_dist, int dist_is_float, int yrows,
              double min_ratio, int *d_matches, int *d_count, void *d_ws, size_t ws_bytes,
              hipStream_t stream);

// ---- format adapters (adapter.hip) ---------------------------------------------------
int sift_split_run(const float *d_table, int rows, float *d_geom, uint8_t *d_desc, hipStream_t stream);
int gather_match_coords_run(const float *d_geom_x, const float *d_geom_y, const int *d_matches,
                            const int *d_count, int capacity, double *d_x0, double *d_x1,
                            hipStream_t stream);

size_t normalize_workspace_bytes(int dim);
// the larger workspace with which normalize_run folds the column sums of a big table instead of
// walking them (same results; with the smaller one it walks)
size_t normalize_workspace_bytes_rows(int rows, int dim);
int normalize_run(const float *d_x, int rows, int dim, float *d_out_f32, unsigned char *d_out_u8,
                  void *d_ws, size_t ws_bytes, hipStream_t stream);

// ---- normalisation of many tables in one chain of launches (normalize_batch.hip) -------
constexpr int kNormalizeBatchMaxDim = 2048;
constexpr int kNormalizeBatchItemRows = 256;   // rows per work item
constexpr int kNormalizeBatchGroupsPerCu = 32; // the grid cap: workgroups per compute unit, each walking its items
// One workgroup's step: rows [row0, row0 + rows) of set `set`, row0 counted within the set.
struct NormalizeBatchItem {
  int32_t set, row0, rows;
};
// Everything normalize_batch_run launches for a collection, a function of seg_off, dim and dtype alone.
struct NormalizeBatchPlan {
  long long sets = 0, total_rows = 0;     // non-empty sets; rows in all
  std::vector<NormalizeBatchItem> items;  // set by set, every set's rows in blocks of kNormalizeBatchItemRows, in order
  // workspace: byte offsets, in this order.  The device form of `items`, seg_off as uint32[nseg + 1], the first
  // item at or after every set int32[nseg + 1], (mean, norm) float[nseg][2][dim], and for uint8 input the items'
  // partial statistics uint32[items][dim].
  size_t off_items = 0, off_seg = 0, off_item0 = 0, off_stats = 0, off_part = 0, total_bytes = 0;
};
// SPV_ERR_INVALID (message set, *p untouched) for what include/spectavi_amd.h rejects; host only
int normalize_batch_plan(const long long *seg_off, int nseg, int dim, int dtype, NormalizeBatchPlan *p);
// Device outputs as in include/spectavi_amd.h; asynchronous on `stream` but for the upload of the call's tables.
int normalize_batch_run(const void *d_x, int dtype, const long long *seg_off, int nseg, int dim, float *d_out_f32,
                        uint8_t *d_out_u8, void *d_ws, size_t ws_bytes, hipStream_t stream);

// ---- multi-device result gather over RCCL (gather.hip) -------------------------------
struct GatherCtx;                    // communicator clique + one stream per rank, cached per device list
std::mutex &gather_mutex();          // held by the caller around every use of a clique
int gather_ctx_get(const std::vector<int> &devs, bool use_rccl, GatherCtx **out);
hipStream_t gather_stream(GatherCtx *ctx, int rank);
// (idx uint64[cnt,2], 32-bit dist[cnt,2]) -> cnt 16-byte records (records.h)
int gather_pack_run(const uint64_t *d_idx, const void *d_d32, long long cnt, void *d_rec, hipStream_t stream);
// bytes_per_rank bytes from every rank's d_send[r] into slot r of d_recv_root on rank 0: ncclGather, or
// (peer-copy transport) one hipMemcpyPeerAsync per rank
int gather_bytes_run(GatherCtx *ctx, const std::vector<const void *> &d_send, void *d_recv_root,
                     size_t bytes_per_rank);
// [G][max_cnt] records -> the ABI layout over all `total` rows
int gather_widen_run(const void *d_recv, long long total, int G, long long max_cnt, uint64_t *d_idx, void *d_d32,
                     hipStream_t stream);

size_t dlt_score_workspace_bytes(int nhyp, long long npt);
// d_ws (may be NULL / short: the scorer then runs in one pass, same results) holds the work list of
// the solves that are deferred to the second pass
// d_live / d_nlive (may be NULL): score only the hypotheses 4 f .. 4 f + 3 of the *d_nlive candidates f
// listed in d_live (device memory); the counts of the others stay 0, their mask rows unwritten
int dlt_score_run(const double *P0, const double *d_p1s, int nhyp, long long npt, const double *d_x,
                  const double *d_xp, double max_error, int *d_counts, unsigned char *d_mask, void *d_ws,
                  size_t ws_bytes, hipStream_t stream, const int *d_live = nullptr, const int *d_nlive = nullptr,
                  int rows_cap = 65535);


// ---- RANSAC candidate processing (dlt.hip): gate, E, four cameras, scoring, best camera ----
size_t ransac_workspace_bytes(int nF, long long npt, bool want_mask);
int ransac_process_run(const double *d_Fs, int nF, long long npt, const double *d_x0, const double *d_x1,
                       double ratio_allowed, double required_percent, double max_error, int find_best,
                       int *d_success, int *d_inlier_count, int *d_best_cam, double *d_best_P, double *d_ratio,
                       double *d_E, int *d_counts4, unsigned char *d_mask, void *d_ws, size_t ws_bytes,
                       hipStream_t stream, int score_rows_cap = 65535);  // grid rows of the scorer: a RANSAC batch, whose
                                                                          // candidates are nearly all gated, passes 2048

// ... its first stage alone (gate, E, four cameras), any nF: d_cams double[nF,4,12], NaN for a gated candidate
int ransac_cameras_run(const double *d_Fs, int nF, double ratio_allowed, double *d_cams, int *d_gated, int *d_live,
                       int *d_nlive, hipStream_t stream);

// ---- seven-point solver and the RANSAC loop around the candidate processing (ransac.hip) ----
// d_x, d_xp double[n,7,2] euclidean; d_Fs double[n,3,9] (NaN in the slots of missing roots);
// d_nroot int[n] and d_basis double[n,2,9] may be NULL
int seven_point_run(const double *d_x, const double *d_xp, int n, double *d_Fs, int *d_nroot, double *d_basis,
                    hipStream_t stream);
int ransac_fit_batch_limit(long long npt);  // tries per batch for this many correspondences
int ransac_first_step(long long npt, int batch);  // tries of a fit's first batch, of any set of a many-sets fit too
size_t ransac_fit_workspace_bytes(int batch, long long npt);
int ransac_fit_run(const double *d_x0, const double *d_x1, long long npt, double required_percent,
                   double max_error, int max_tries, int find_best, double ratio_allowed,
                   const std::function<void(int, int, int *)> &next_samples, int *success, double *essential,
                   double *camera, int *n_inliers, unsigned char *inlier_mask, int *best_try, int *best_root,
                   int *tries_run, void *d_ws, size_t ws_bytes, int batch, hipStream_t stream);

int seven_point_sampled_run(const double *d_x0, const double *d_x1, const int *d_samples, int n, double *d_Fs,
                            hipStream_t stream);  // subsets as rows of d_x0 / d_x1 double[.,3]; d_Fs double[n,3,9]
// The best model of a fit so far, device resident; the four ints are what the host reads after a batch.
struct FitState {
  int found;    // a model has been kept
  int success;  // ... and it is above required_percent_inliers: stop
  int count;    // its inliers
  int cand;     // 3 * try + root
  double F[9];
  double P[12];
};
void floyd_sample(std::mt19937 &gen, int N, int *out);  // one 7-subset of [1, N), as the reference draws it
uint32_t ransac_seed(uint64_t seed);                    // the generator's seed for a caller's seed (0: environment, else random)
int check_fit_args(const double *x0, const double *x1, int npt, int max_tries);

// ---- two-view RANSAC of many correspondence sets in one call (ransac_batch.hip) ----------
// One workgroup's share of a round: rows [row0, row0 + rows) of the concatenated correspondences, all of one set,
// against the candidates [cand0, cand0 + ncand) of the round, all of that set.
struct RansacBatchItem {
  int32_t set, row0, rows, cand0, ncand;
};
// One set's part of a round.
struct RansacBatchSlot {
  int32_t set, npt, cand0, ncand, cand_base;  // cand_base: 3 x the tries of the set that earlier rounds evaluated
};
// Row blocks of a set of npt rows: the scorers' workgroups take 256 rows each.
inline size_t batch_row_blocks(long long npt) { return (size_t)((npt + 255) / 256); }
// (The rule that fills a round, the round driver and the argument check of a many-sets fit: fit_rounds.h.)
// The work items of a round, a function of the slots and the compute units alone; host only.
void ransac_batch_items(const std::vector<RansacBatchSlot> &slots, const long long *pair_off, int cus,
                        std::vector<RansacBatchItem> *items);
// The slots of the first round of a call (host only): every set of >= 10 rows, in order, while the round has room.
void ransac_batch_first_round(const long long *pair_off, int npairs, int max_tries, std::vector<RansacBatchSlot> *slots);
// SPV_ERR_INVALID (message set) for what include/spectavi_amd.h rejects; touches no device, no output
int ransac_batch_check(const long long *pair_off, int npairs, int max_tries, const int32_t *samples);
// Host results as in include/spectavi_amd.h; d_x0 / d_x1 on the current device.  Synchronises `stream` once a round.
int ransac_fit_batch_run(const double *d_x0, const double *d_x1, const long long *pair_off, int npairs,
                         double required_percent, double max_error, int max_tries, int find_best, double ratio_allowed,
                         const int32_t *samples, const unsigned long long *seeds, int32_t *success, double *essential,
                         double *camera, double *inlier_percent, int32_t *inlier_idx, int32_t *n_inliers,
                         int32_t *best_try, int32_t *best_root, int32_t *tries_run, unsigned char *d_inlier_mask,
                         hipStream_t stream);

// ---- DLT triangulation of many correspondence sets in one call (dlt_batch.hip) -----------
// One workgroup's share of a collection: rows [row0, row0 + rows) of the concatenated correspondences, all of one
// set; out: the out row of its first row where every row is selected (no mask), else -1 (the device counts).
struct DltBatchItem {
  int32_t set, row0, rows, out;
};
// The work items of a call, a function of pair_off and use alone (host only): every used set's rows in blocks of
// 256, in order.  *bound (may be null): the rows of the used sets.
void dlt_batch_items(const long long *pair_off, int npairs, const int32_t *use, bool masked,
                     std::vector<DltBatchItem> *items, long long *used_sets, long long *bound);
// SPV_ERR_INVALID (message set) for what include/spectavi_amd.h rejects; touches no device, no output
int dlt_batch_check(const double *d_x0, const double *d_x1, const long long *pair_off, int npairs, const double *P1s,
                    const void *X, const void *err, long long capacity);
// Device outputs as in include/spectavi_amd.h; asynchronous on `stream` but for the upload of the call's tables.
int dlt_batch_run(const double *d_x0, const double *d_x1, const long long *pair_off, int npairs, const double *P0s,
                  const double *P1s, const int32_t *use, const uint8_t *d_mask, double *d_X, double *d_err,
                  int32_t *d_rows, long long capacity, long long *d_out_off, long long *d_count, hipStream_t stream);

// ---- the matches of an l1k2_batch + ratio-test run as per-pair coordinates (adapter.hip) ----
int gather_match_coords_batch_run(const float *d_geom, const long long *seg_off, int nseg, const int32_t *pairs,
                                  int npairs, const int *d_matches, const int *d_count, int capacity, double *d_x0,
                                  double *d_x1, long long *d_pair_off, hipStream_t stream);

// ---- multi-view tracks from the matches of all pairs (tracks_batch.hip) --------------------
// SPV_ERR_INVALID (message set) for what include/spectavi_amd.h rejects; touches no device, no output
int tracks_batch_check(const long long *seg_off, int nseg, const int32_t *pairs, int npairs, int capacity, int min_len);
size_t tracks_batch_workspace_bytes(long long total_rows, int capacity);
// B of include/spectavi_amd.h: the rows of members; track_off has B / 2 + 1 entries, flags B / 2
long long tracks_batch_member_bound(long long total_rows, int capacity, int accumulate);
// Device outputs as in include/spectavi_amd.h; asynchronous on `stream` but for the upload of the call's table.
int tracks_batch_run(const long long *seg_off, int nseg, const int32_t *pairs, int npairs, const int32_t *d_matches,
                     const int32_t *d_count, int capacity, const uint8_t *d_mask, int min_len, int accumulate,
                     int32_t *d_label, int32_t *d_track, long long *d_track_off, int32_t *d_members, uint8_t *d_flags,
                     int32_t *d_counts, void *d_ws, size_t ws_bytes, hipStream_t stream);

// ---- N-view DLT of every track (tracks_triangulate.hip) ------------------------------------
// The longest track the lane form takes; 0: every track of 3 or more members takes the wave form.  The setter
// returns the setting before.
int tracks_triangulate_set_long(int L);
int tracks_triangulate_get_long();
// Which tracks take which form, a function of track_off and the setting alone (host only).
struct TracksTriangulatePlan {
  long long lane_tracks = 0, wave_tracks = 0, lane_groups = 0, longest = 0;
  std::vector<int32_t> wave_list;  // the wave-form tracks, ascending
};
void tracks_triangulate_plan(const long long *track_off, int ntracks, TracksTriangulatePlan *plan);
// SPV_ERR_INVALID (message set) for what include/spectavi_amd.h rejects; touches no device, no output
int tracks_triangulate_check(const void *geom, const long long *seg_off, int nseg, const double *cams,
                             const long long *track_off, int ntracks, const void *members, long long nmembers,
                             double max_error, const void *X, const void *err, const void *ok, const void *nused);
// Device outputs as in include/spectavi_amd.h; asynchronous on `stream` but for the upload of the call's tables.
int tracks_triangulate_run(const float *d_geom, const long long *seg_off, int nseg, const double *cams,
                           const int32_t *use_set, const long long *track_off, int ntracks, const int32_t *d_members,
                           long long nmembers, double max_error, double *d_X, double *d_err, uint8_t *d_ok,
                           int32_t *d_nused, hipStream_t stream);

// ---- RANSAC camera resection of many views (resect_batch.hip) -------------------------------
constexpr int kResectMinRows = 6;  // a hypothesis takes six rows: smaller sets are skipped
// One workgroup's step of the gather: rows [row0, row0 + rows) of geom, all of the listed view `view` (an index into
// views), the first of them row view_row0 of that view.
struct ResectGatherItem {
  int32_t view, row0, rows, view_row0;
};
// The work items of a gather, a function of seg_off and views alone (host only): every listed view's rows in blocks
// of 256, in order.
void resect_gather_items(const long long *seg_off, const int32_t *views, int nviews, std::vector<ResectGatherItem> *items);
// SPV_ERR_INVALID (message set) for what include/spectavi_amd.h rejects; touches no device, no output
int resect_gather_check(const void *geom, const void *track, const long long *seg_off, int nseg, const int32_t *views,
                        int nviews, const void *X, int ntracks, long long capacity, const void *x, const void *Xw);
// Device outputs as in include/spectavi_amd.h; asynchronous on `stream` but for the upload of the call's tables, and
// for the wait that a host view_off asks for.
int resect_gather_run(const float *d_geom, const int32_t *d_track, const long long *seg_off, int nseg, const int32_t *views,
                      int nviews, const double *d_X, const uint8_t *d_ok, int ntracks, long long capacity, double *d_x,
                      double *d_Xw, int32_t *d_rows, long long *d_view_off, long long *view_off, hipStream_t stream);
// The slots of the first round of a fit (host only): every set of >= 6 rows, in order, while the round has room; a
// slot's cand0 / ncand / cand_base count tries.  Its work items are ransac_batch_items'; the rule that fills a round,
// the round driver, the heads and the argument check are the two-view fit's too (fit_rounds.h).
void resect_first_round(const long long *view_off, int nviews, int max_tries, std::vector<RansacBatchSlot> *slots);
// SPV_ERR_INVALID (message set) for what include/spectavi_amd.h rejects; touches no device, no output
int resect_check(const long long *view_off, int nviews, double required_percent, double max_error, int max_tries,
                 const int32_t *samples);
// Host results as in include/spectavi_amd.h; d_x / d_Xw on the current device.  Synchronises `stream` once a round.
int resect_fit_batch_run(const double *d_x, const double *d_Xw, const long long *view_off, int nviews,
                         double required_percent, double max_error, int max_tries, int find_best, const int32_t *samples,
                         const unsigned long long *seeds, int32_t *success, double *camera, double *inlier_percent,
                         int32_t *n_inliers, int32_t *best_try, int32_t *tries_run, unsigned char *d_inlier_mask,
                         double *d_try_cameras, int32_t *d_try_inliers, hipStream_t stream);

// ---- Bundle adjustment of cameras and track points (bundle_adjust.hip) -----------------------
struct BundleAdjustOptions {
  double huber, lambda0, ftol, gtol, cg_tol;
  int max_steps, cg_max;
};
// Which tracks take which form, the view-major chunk size and, where the host has the members, the chunks of the free
// cameras when every usable member of a track of two or more takes part (host only).
struct BundleAdjustPlan {
  long long lane_tracks = 0, wave_tracks = 0, chunk = 0, chunks = 0, longest = 0;
  std::vector<int32_t> wave_list;  // the wave-form tracks, ascending
};
void bundle_adjust_plan(const long long *track_off, int ntracks, const int32_t *members, const long long *seg_off, int nseg,
                        const int32_t *mode, BundleAdjustPlan *plan);
size_t bundle_adjust_workspace_bytes(int nseg, int ntracks, long long nmembers);
// SPV_ERR_INVALID (message set) for what include/spectavi_amd.h rejects; touches no device, no output
int bundle_adjust_check(const void *geom, const long long *seg_off, int nseg, const double *K, const double *poses,
                        const int32_t *mode, const long long *track_off, int ntracks, const void *members, long long nmembers,
                        const void *X, const BundleAdjustOptions &o, const void *err, const void *trace, const void *info);
// Whether a checked call has a track and a camera; the trace and info of one that has not.
bool bundle_adjust_has_work(const int32_t *mode, int nseg, int ntracks);
void bundle_adjust_idle(const BundleAdjustOptions &o, double *trace, double *info);
// Host and device outputs as in include/spectavi_amd.h.  Waits for `stream` twice before the loop and once per step.
int bundle_adjust_run(const float *d_geom, const long long *seg_off, int nseg, const double *K, double *poses, const int32_t *mode,
                      const long long *track_off, int ntracks, const int32_t *d_members, long long nmembers, double *d_X,
                      const uint8_t *d_use, const BundleAdjustOptions &o, double *d_err, uint8_t *d_active, double *trace,
                      double *info, void *d_ws, size_t ws_bytes, hipStream_t stream);

}  // namespace spv
