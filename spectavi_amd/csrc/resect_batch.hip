// resect_batch.hip -- RANSAC camera resection of many views in one call (gfx950).
//
// tracks_triangulate.hip turns tracks into 3-D points from the cameras it is given; this file gives a camera to a
// view that has none yet, from the points of the tracks the view observes.  Two ops, split the way
// match_coordinates_batch and ransac_fit_batch are.  The contract is the library's own and is stated in
// include/spectavi_amd.h; tests/resect_model.py is its plain restatement.  The reference has no such step.
//
// resect_gather: the (u, v) of the requested views' rows whose track has a usable point, next to that point, back to
// back.  A flag / segmented scan / place chain over the requested views' rows in blocks of 256:
//   resect_gather_count_kernel   taken rows per block
//   resect_gather_scan_kernel    one workgroup: the blocks' out bases, view_off
//   resect_gather_place_kernel   the flags again, a wave scan, the rows that fit the capacity
//
// resect_fit_batch: one camera per set of 2-D / 3-D correspondences.  The sets of a collection advance together in
// the rounds of fit_rounds.hip, which ransac_batch.hip shares: the running sets, the rule that fills a round, the
// upload of its subsets, slots and work items, the read-back of the heads, the one stream synchronisation and which
// sets leave.  This file supplies (kResect): 6-subsets (spv_ransac_sample's first six columns, or the first six of a
// shuffle for a set under 10 rows), one candidate a try, sets of 6 rows and more, a round of at most kRoundTries
// tries and kRoundVerdicts verdicts at one a row, 256 tries a set and round, then fourfold up to 4096, no leaving on
// success where per-try outputs are wanted, and the kernels of a round:
//   resect_solve_kernel    one try per lane: the unit null vector of the try's 11 x 12 matrix (resect_device.h), and
//                          the camera's factor of the depth term, 16 doubles a try
//   resect_score_kernel    the hot path.  One workgroup per work item = (<= 256 rows of one set, a range of that
//                          set's tries): a lane keeps its row (u, v, X) in registers, the 13 doubles of a try are
//                          scalar loads, a verdict is 12 fma / mul for P X, one reciprocal with two Newton steps, five
//                          more for the squared residual and two for the depth term; one ballot and one popcount per
//                          wave and try, kept in the lane try % 64 and added to the try's counter 64 tries at a time
//   resect_reduce_kernel   one workgroup per set of the round over that set's tries in order (best_model_device.h, a
//                          share AT the required one succeeds), into the set's state and its four-int head; with
//                          the per-try outputs it also copies the round's cameras and counts to them.
// A last pass writes the kept camera's verdict of every row (resect_mask_kernel) with the scorer's very statements.
//
// The result does not depend on the cuts: a hypothesis is per try, a verdict per (try, row), counts are integer
// sums, and the best-model rule is defined on try order.  Only tries_run depends on the rounds.  Work items come from
// ransac_batch_items, the slice rule of the many-sets RANSAC.
#include "best_model_device.h"
#include "common.h"
#include "device_util.h"
#include "dlt_device.h"
#include "fit_rounds.h"
#include "host_io.h"
#include "resect_device.h"

#include <limits.h>
#include <string.h>

namespace spv {
namespace {

constexpr int kScanThreads = 1024;                  // block_scan_inplace's workgroup
constexpr int kSolveThreads = 64;
constexpr int kReduceThreads = 256;
constexpr int kCamStride = 16;                      // doubles a try: P, the depth factor, padding
constexpr int kRoundTries = 32768;                  // tries of all sets in one round
constexpr long long kRoundVerdicts = 4000000000ll;  // (try, row) verdicts of a round
constexpr int kFirstStep = 256, kLastStep = 4096;   // a set's tries per round: 256, then fourfold

typedef double __attribute__((address_space(4))) ConstDouble;  // memory no kernel writes while this one runs

static_assert(sizeof(ResectGatherItem) == 16, "items travel as int32[4]");

// ---- gather ------------------------------------------------------------------------------------------------------
struct GatherTables {
  const ResectGatherItem *items;
  const int32_t *item0;  // [nviews + 1]: the first item at or after every listed view; [nviews] = nitems
  int nitems, nviews, ntracks;
};

// Whether lane t's row of the item is taken, and then its track.  Nothing but track, ok and X is read.
__device__ __forceinline__ bool gather_flag(const ResectGatherItem &it, int t, const int32_t *__restrict__ track,
                                            const double *__restrict__ X, const uint8_t *__restrict__ ok, int ntracks,
                                            int &tr) {
  if (t >= it.rows) return false;
  tr = track[(size_t)it.row0 + t];
  if (tr < 0 || tr >= ntracks) return false;
  if (ok && ok[tr] == 0) return false;
  const double *p = X + 4 * (size_t)tr;
  return __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) && __builtin_isfinite(p[2]) && __builtin_isfinite(p[3]);
}

__global__ __launch_bounds__(kDltThreads) void resect_gather_count_kernel(GatherTables tb, const int32_t *__restrict__ track,
                                                                          const double *__restrict__ X,
                                                                          const uint8_t *__restrict__ ok,
                                                                          int32_t *__restrict__ counts) {
  __shared__ int s_w[kDltThreads / 64];
  for (int b = blockIdx.x; b < tb.nitems; b += gridDim.x) {
    const ResectGatherItem it = tb.items[b];
    int tr;
    const bool sel = gather_flag(it, threadIdx.x, track, X, ok, tb.ntracks, tr);
    const unsigned long long bal = __ballot(sel);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) counts[b] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();  // the sums have been read before the next item writes them
  }
}

// counts -> the items' out bases, in place; view_off[i] = taken rows before listed view i, view_off[nviews] = all.
__global__ __launch_bounds__(kScanThreads) void resect_gather_scan_kernel(GatherTables tb, int32_t *__restrict__ counts,
                                                                          long long *__restrict__ view_off) {
  const int32_t total = block_scan_inplace<int32_t>(counts, tb.nitems);  // (ends in a barrier: the bases are visible)
  for (int i = threadIdx.x; i <= tb.nviews; i += kScanThreads) {
    const int k = tb.item0[i];
    view_off[i] = k < tb.nitems ? counts[k] : total;
  }
}

__global__ __launch_bounds__(kDltThreads) void resect_gather_place_kernel(GatherTables tb, const float *__restrict__ geom,
                                                                          const int32_t *__restrict__ track,
                                                                          const double *__restrict__ X,
                                                                          const uint8_t *__restrict__ ok,
                                                                          const int32_t *__restrict__ bases, long long capacity,
                                                                          double *__restrict__ dx, double *__restrict__ dXw,
                                                                          int32_t *__restrict__ drows) {
  __shared__ int s_w[kDltThreads / 64];
  const int t = threadIdx.x;
  for (int b = blockIdx.x; b < tb.nitems; b += gridDim.x) {
    const ResectGatherItem it = tb.items[b];
    int tr = 0;
    const bool sel = gather_flag(it, t, track, X, ok, tb.ntracks, tr);
    const int incl = wave_scan_incl<int>(sel ? 1 : 0, t & 63);
    if ((t & 63) == 63) s_w[t >> 6] = incl;
    __syncthreads();
    int woff = 0;
    for (int k = 0; k < (t >> 6); ++k) woff += s_w[k];
    __syncthreads();  // the sums have been read before the next item writes them
    const long long out = (long long)bases[b] + woff + incl - 1;
    if (!sel || out >= capacity) continue;
    const float *g = geom + 4 * ((size_t)it.row0 + t);
    dx[3 * out] = (double)g[0];
    dx[3 * out + 1] = (double)g[1];
    dx[3 * out + 2] = 1.0;
    // (as 64-bit words: the copy is bit for bit)
    const unsigned long long *src = reinterpret_cast<const unsigned long long *>(X) + 4 * (size_t)tr;
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(dXw) + 4 * (size_t)out;
#pragma unroll
    for (int c = 0; c < 4; ++c) dst[c] = src[c];
    if (drows) drows[out] = it.view_row0 + t;
  }
}

// ---- fit ---------------------------------------------------------------------------------------------------------
struct ResectState {
  int found, success, count, try_;
  double P[kCamStride];  // the kept try's 16 doubles
};

// A row as the scorer keeps it: (u, v) = (x0, x1) / x2 by IEEE division (a third column of 1 leaves them as they
// are), the point and 1 / X3.
struct ResectRow {
  double u, v, X[4], rX3;
};
__device__ __forceinline__ void load_row(const double *__restrict__ x, const double *__restrict__ Xw, size_t row, ResectRow &r) {
  const double x2 = x[3 * row + 2];
  r.u = x[3 * row] / x2;
  r.v = x[3 * row + 1] / x2;
#pragma unroll
  for (int c = 0; c < 4; ++c) r.X[c] = Xw[4 * row + c];
  r.rX3 = 1.0 / r.X[3];
}

// The verdict of a row under the camera p[0..12) with depth factor p[12]: the squared residual against the squared
// bound (me2 < 0: nothing passes), and the depth term's sign.  NaNs compare false.
template <typename Cam>
__device__ __forceinline__ bool resect_inlier(const Cam &p, const ResectRow &r, double me2) {
  double h[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double a = p[4 * k] * r.X[0];
#pragma unroll
    for (int c = 1; c < 4; ++c) a = __builtin_fma(p[4 * k + c], r.X[c], a);
    h[k] = a;
  }
  const double iz = rcp_nr2(h[2]);
  const double ex = __builtin_fma(h[0], iz, -r.u), ey = __builtin_fma(h[1], iz, -r.v);
  const double e2 = __builtin_fma(ex, ex, ey * ey);
  const double dc = (p[12] * h[2]) * r.rX3;
  return (e2 <= me2) && (dc > 0);
}

__global__ __launch_bounds__(kSolveThreads) void resect_solve_kernel(const int32_t *__restrict__ samples, int ntries,
                                                                     const double *__restrict__ x,
                                                                     const double *__restrict__ Xw,
                                                                     double *__restrict__ cams) {
  const int t = blockIdx.x * kSolveThreads + threadIdx.x;
  if (t >= ntries) return;
  double u[6], v[6], X[6][4], P[12];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const size_t row = (size_t)samples[6 * (size_t)t + i];
    const double x2 = x[3 * row + 2];
    u[i] = x[3 * row] / x2;
    v[i] = x[3 * row + 1] / x2;
#pragma unroll
    for (int c = 0; c < 4; ++c) X[i][c] = Xw[4 * row + c];
  }
  resect_solve6(u, v, X, P);
  double *o = cams + (size_t)t * kCamStride;
#pragma unroll
  for (int c = 0; c < 12; ++c) o[c] = P[c];
  o[12] = resect_depth_factor(P);
  o[13] = o[14] = o[15] = 0.0;
}

__global__ __launch_bounds__(kDltThreads) void resect_score_kernel(const RansacBatchItem *__restrict__ items,
                                                                   const double *__restrict__ cams,
                                                                   const double *__restrict__ x,
                                                                   const double *__restrict__ Xw, double me2,
                                                                   int *__restrict__ counts) {
  const RansacBatchItem it = items[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63;
  const bool live = t < it.rows;
  ResectRow r;
  load_row(x, Xw, (size_t)it.row0 + (live ? t : 0), r);  // an item has at least one row
  const int c0 = __builtin_amdgcn_readfirstlane(it.cand0), n = __builtin_amdgcn_readfirstlane(it.ncand);
  int mine = 0;
  // the 13 doubles of a try are scalar loads (uniform index, constant address space).  A wave waits for them once a
  // step; the other waves of the SIMD -- the planner aims at four row blocks per compute unit and more -- issue their
  // verdicts meanwhile.  (A prefetch of the next step's cameras was tried: the compiler's wait for the loads before
  // the loop lands in the loop header and takes the prefetch's place.)
  // Two tries a step: one wait for both cameras, and two independent chains of dependent fp64 operations to issue from.
  const ConstDouble *cp = (const ConstDouble *)(cams + (size_t)c0 * kCamStride);
  for (int i = 0; i < n; i += 2) {  // workgroup-uniform
    const int j = i + 1 < n ? i + 1 : i;  // an odd range's last step scores its last try twice and counts it once
    double p[13], q[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) {
      p[k] = cp[(size_t)i * kCamStride + k];
      q[k] = cp[(size_t)j * kCamStride + k];
    }
    const bool inl0 = resect_inlier(p, r, me2) && live, inl1 = resect_inlier(q, r, me2) && live;
    const unsigned long long bal0 = __ballot(inl0), bal1 = __ballot(inl1);
    if (lane == (i & 63)) mine = __popcll(bal0);
    if (j != i && lane == (j & 63)) mine = __popcll(bal1);
    if ((j & 63) == 63 || j == n - 1) {  // lane l holds the wave's count of try (j & ~63) + l
      if (mine) atomicAdd(&counts[c0 + (j & ~63) + lane], mine);
      mine = 0;
    }
  }
}

// The best-model rule over the slot's tries in order, into the set's state.  try_cams / try_inl (may be null): the
// call's per-try outputs, [nsets, max_tries, 12] and [nsets, max_tries].
__global__ __launch_bounds__(kReduceThreads) void resect_reduce_kernel(const RansacBatchSlot *__restrict__ slots,
                                                                       const int *__restrict__ counts,
                                                                       const double *__restrict__ cams, double share,
                                                                       int find_best, int max_tries,
                                                                       ResectState *__restrict__ states,
                                                                       FitHead *__restrict__ heads,
                                                                       double *__restrict__ try_cams,
                                                                       int32_t *__restrict__ try_inl) {
  const RansacBatchSlot sl = slots[blockIdx.x];
  ResectState *state = states + sl.set;
  if (try_inl || try_cams)  // every try of the slot, whether or not the set has already succeeded
    for (int i = threadIdx.x; i < sl.ncand; i += kReduceThreads) {
      const size_t at = (size_t)sl.set * max_tries + sl.cand_base + i;
      if (try_inl) try_inl[at] = counts[sl.cand0 + i];
      if (try_cams)
        for (int k = 0; k < 12; ++k) try_cams[at * 12 + k] = cams[(size_t)(sl.cand0 + i) * kCamStride + k];
    }
  int success;
  // (state->success is uniform: nothing after the first success is looked at; every try is eligible)
  const int win = best_model<kReduceThreads>(
      sl.ncand, state->success != 0, (double)sl.npt, state->found ? state->count : 0, find_best,
      [=](int i) { return counts[sl.cand0 + i]; }, [=](double s) { return s >= share; }, &success);
  if (threadIdx.x != 0) return;
  if (win >= 0) {
    const size_t w = (size_t)sl.cand0 + win;
    state->found = 1;
    state->success = success;
    state->count = counts[w];
    state->try_ = sl.cand_base + win;
    for (int k = 0; k < kCamStride; ++k) state->P[k] = cams[w * kCamStride + k];
  }
  heads[blockIdx.x] = FitHead{state->found, state->success, state->count, state->try_};
}

// mask[row] = the verdict of the row under the camera its set kept; 0 where the set kept none.  One workgroup per
// row block of the last pass's items, which cover every row of the collection.
__global__ __launch_bounds__(kDltThreads) void resect_mask_kernel(const RansacBatchItem *__restrict__ items,
                                                                  const ResectState *__restrict__ states,
                                                                  const double *__restrict__ x,
                                                                  const double *__restrict__ Xw, double me2,
                                                                  unsigned char *__restrict__ mask) {
  const RansacBatchItem it = items[blockIdx.x];
  if ((int)threadIdx.x >= it.rows) return;
  const size_t row = (size_t)it.row0 + threadIdx.x;
  const ResectState *st = states + it.set;
  bool inl = false;
  if (st->found) {
    ResectRow r;
    load_row(x, Xw, row, r);
    double p[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) p[k] = st->P[k];
    inl = resect_inlier(p, r, me2);
  }
  mask[row] = inl ? 1 : 0;
}

// One 6-subset of [0, N) for a set the many-sets sampler does not take (N < 10): the first six of a shuffle.
void small_sample(std::mt19937 &gen, int N, int *out) {
  int idx[16];
  for (int i = 0; i < N; ++i) idx[i] = i;
  for (int k = 0; k < 6; ++k) {
    const int j = k + (int)(gen() % (uint32_t)(N - k));
    std::swap(idx[k], idx[j]);
    out[k] = idx[k];
  }
}

// What this fit gives the round driver (fit_rounds.h).  A set's steps: 256 tries, then fourfold up to 4096.  A
// sample: spv_ransac_sample's rows, the first six columns, where that sampler takes the set.  A try is one candidate,
// a verdict a row.
void resect_steps(long long, int max_tries, int *first, int *top) {
  *first = std::min(kFirstStep, max_tries);
  *top = kLastStep;
}
void resect_sample(std::mt19937 &gen, int npt, int *out) {
  int seven[7];
  if (npt >= 10) floyd_sample(gen, npt, seven);
  else small_sample(gen, npt, seven);
  memcpy(out, seven, 6 * sizeof(int));
}
const FitRoundsOp kResect{6, 1, kResectMinRows, kRoundTries, kRoundVerdicts, 1, resect_steps, resect_sample, false};

struct FitBufs {
  ResectState *states;
  FitHead *heads;
  unsigned char *tables;  // a round's upload (fit_rounds.h); the last pass: items
  size_t tables_bytes;
  double *cams;
  int *counts;
  size_t end;
};
FitBufs carve(void *base, int nviews, int tries, size_t tables_bytes) {
  WsWalk w(base);
  FitBufs b{};
  b.states = w.take<ResectState>((size_t)nviews * sizeof(ResectState));
  b.heads = w.take<FitHead>((size_t)nviews * sizeof(FitHead));
  b.tables_bytes = tables_bytes;
  b.tables = w.take(b.tables_bytes);
  b.cams = w.take<double>((size_t)tries * kCamStride * sizeof(double));
  b.counts = w.take<int>(((size_t)tries + 64) * sizeof(int));
  b.end = w.end();
  return b;
}

}  // namespace

// ---- gather: host side -------------------------------------------------------------------------------------------
void resect_gather_items(const long long *seg_off, const int32_t *views, int nviews, std::vector<ResectGatherItem> *items) {
  items->clear();
  for (int i = 0; i < nviews; ++i) {
    const long long lo = seg_off[views[i]], hi = seg_off[views[i] + 1];
    for (long long r = lo; r < hi; r += kDltThreads)
      items->push_back(ResectGatherItem{i, (int32_t)r, (int32_t)std::min<long long>(kDltThreads, hi - r), (int32_t)(r - lo)});
  }
}

int resect_gather_check(const void *geom, const void *track, const long long *seg_off, int nseg, const int32_t *views,
                        int nviews, const void *X, int ntracks, long long capacity, const void *x, const void *Xw) {
  if (nseg < 0 || nviews < 0 || ntracks < 0)
    return set_error(SPV_ERR_INVALID, "negative count (nseg=%d, nviews=%d, ntracks=%d)", nseg, nviews, ntracks);
  if (nviews > (1 << 20)) return set_error(SPV_ERR_INVALID, "more than 2^20 views per call");
  if (capacity < 0) return set_error(SPV_ERR_INVALID, "negative capacity");
  SPV_TRY(check_offsets(seg_off, nseg, "seg_off"));
  if (nviews > 0 && !views) return set_error(SPV_ERR_INVALID, "null views");
  long long rows = 0;
  for (int i = 0; i < nviews; ++i) {
    if (views[i] < 0 || views[i] >= nseg) return set_error(SPV_ERR_INVALID, "views[%d] = %d outside [0, %d)", i, views[i], nseg);
    rows += seg_off[views[i] + 1] - seg_off[views[i]];
  }
  if (rows >= (1ll << 31)) return set_error(SPV_ERR_INVALID, "the listed views have %lld rows, must be below 2^31", rows);
  if (rows > 0 && (!geom || !track || (ntracks > 0 && !X))) return set_error(SPV_ERR_INVALID, "null pointer");
  if (rows > 0 && ntracks > 0 && capacity > 0 && (!x || !Xw)) return set_error(SPV_ERR_INVALID, "null output pointer");
  if (((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(Xw)) & 7) ||
      ((reinterpret_cast<uintptr_t>(geom) | reinterpret_cast<uintptr_t>(track)) & 3))
    return set_error(SPV_ERR_INVALID, "pointers must be aligned to their element size");
  return SPV_OK;
}

int resect_gather_run(const float *d_geom, const int32_t *d_track, const long long *seg_off, int nseg, const int32_t *views,
                      int nviews, const double *d_X, const uint8_t *d_ok, int ntracks, long long capacity, double *d_x,
                      double *d_Xw, int32_t *d_rows, long long *d_view_off, long long *view_off, hipStream_t stream) {
  SPV_TRY(resect_gather_check(d_geom, d_track, seg_off, nseg, views, nviews, d_X, ntracks, capacity, d_x, d_Xw));
  if ((reinterpret_cast<uintptr_t>(d_rows) & 3) || (reinterpret_cast<uintptr_t>(d_view_off) & 7))
    return set_error(SPV_ERR_INVALID, "pointers must be aligned to their element size");
  std::vector<ResectGatherItem> items;
  resect_gather_items(seg_off, views, nviews, &items);
  const size_t nitems = items.size(), nv1 = (size_t)nviews + 1;
  if (nitems == 0 || ntracks == 0) {  // nothing can be taken
    if (d_view_off) SPV_HIP_CHECK(hipMemsetAsync(d_view_off, 0, nv1 * sizeof(long long), stream));
    if (view_off) memset(view_off, 0, nv1 * sizeof(long long));
    return SPV_OK;
  }
  // the call's tables, one upload: items | item0; behind them the items' counts / bases and view_off
  const size_t off_item0 = nitems * sizeof(ResectGatherItem), table_bytes = off_item0 + nv1 * sizeof(int32_t);
  const size_t off_counts = round_up(table_bytes, 256), off_voff = round_up(off_counts + nitems * sizeof(int32_t), 256);
  std::vector<unsigned char> host(table_bytes, 0);
  memcpy(host.data(), items.data(), off_item0);
  int32_t *h_item0 = reinterpret_cast<int32_t *>(host.data() + off_item0);
  {
    size_t k = 0;
    for (int i = 0; i <= nviews; ++i) {
      while (k < nitems && items[k].view < i) ++k;
      h_item0[i] = (int32_t)k;
    }
  }
  DevBuf ws;
  SPV_TRY(ws.alloc(off_voff + nv1 * sizeof(long long)));
  // the scratch goes back to the cache behind the last kernel of this call, on every way out
  struct Release {
    DevBuf &b;
    hipStream_t st;
    ~Release() { b.release_after(st); }
  } release{ws, stream};
  unsigned char *base = ws.as<unsigned char>();
  // (pageable source: the copy has left `host` when the call returns)
  SPV_HIP_CHECK(hipMemcpyAsync(base, host.data(), table_bytes, hipMemcpyHostToDevice, stream));
  const GatherTables tb{reinterpret_cast<const ResectGatherItem *>(base), reinterpret_cast<const int32_t *>(base + off_item0),
                        (int)nitems, nviews, ntracks};
  int32_t *bases = reinterpret_cast<int32_t *>(base + off_counts);
  long long *voff = d_view_off ? d_view_off : reinterpret_cast<long long *>(base + off_voff);
  // at most 32 workgroups per compute unit, each walking its items
  const dim3 grid((unsigned)std::min<size_t>(nitems, (size_t)std::max(device_cu_count(), 1) * 32));
  {
    ProfScope prof("resect_gather", stream);
    hipLaunchKernelGGL(resect_gather_count_kernel, grid, dim3(kDltThreads), 0, stream, tb, d_track, d_X, d_ok, bases);
    SPV_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(resect_gather_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, tb, bases, voff);
    SPV_HIP_CHECK(hipGetLastError());
    if (capacity > 0) {
      hipLaunchKernelGGL(resect_gather_place_kernel, grid, dim3(kDltThreads), 0, stream, tb, d_geom, d_track, d_X, d_ok,
                         (const int32_t *)bases, capacity, d_x, d_Xw, d_rows);
      SPV_HIP_CHECK(hipGetLastError());
    }
  }
  if (view_off) {
    SPV_HIP_CHECK(hipMemcpyAsync(view_off, voff, nv1 * sizeof(long long), hipMemcpyDeviceToHost, stream));
    SPV_HIP_CHECK(hipStreamSynchronize(stream));
  }
  return SPV_OK;
}

// ---- fit: host side ----------------------------------------------------------------------------------------------
void resect_first_round(const long long *view_off, int nviews, int max_tries, std::vector<RansacBatchSlot> *slots) {
  FitRounds(kResect, view_off, nviews, max_tries).fill_round(slots, nullptr);
}

int resect_check(const long long *view_off, int nviews, double required_percent, double max_error, int max_tries,
                 const int32_t *samples) {
  if (max_error != max_error) return set_error(SPV_ERR_INVALID, "max_error is NaN");
  if (required_percent != required_percent) return set_error(SPV_ERR_INVALID, "required_percent_inliers is NaN");
  return fit_sets_check(view_off, nviews, max_tries, samples, kResect.width, kResect.min_rows, "view_off",
                        "maximum_tries above 7e8");
}

int resect_fit_batch_run(const double *d_x, const double *d_Xw, const long long *view_off, int nviews,
                         double required_percent, double max_error, int max_tries, int find_best, const int32_t *samples,
                         const unsigned long long *seeds, int32_t *success, double *camera, double *inlier_percent,
                         int32_t *n_inliers, int32_t *best_try, int32_t *tries_run, unsigned char *d_inlier_mask,
                         double *d_try_cameras, int32_t *d_try_inliers, hipStream_t stream) {
  SPV_TRY(resect_check(view_off, nviews, required_percent, max_error, max_tries, samples));
  const long long total = view_off[nviews];
  if (nviews > 0 && (!success || !camera || !inlier_percent || !n_inliers)) return set_error(SPV_ERR_INVALID, "null pointer");
  if (total > 0 && (!d_x || !d_Xw)) return set_error(SPV_ERR_INVALID, "null pointer");
  if (((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_Xw) | reinterpret_cast<uintptr_t>(d_try_cameras)) & 7) ||
      (reinterpret_cast<uintptr_t>(d_try_inliers) & 3))
    return set_error(SPV_ERR_INVALID, "pointers must be aligned to their element size");
  FitRounds rounds(kResect, view_off, nviews, max_tries);
  if (!rounds.empty() && !samples && !seeds) return set_error(SPV_ERR_INVALID, "neither samples nor seeds");
  const FitOutputs out{success, inlier_percent, n_inliers, best_try, tries_run};
  fit_outputs_clear(out, nviews);
  if (rounds.empty()) {
    if (d_inlier_mask && total > 0) SPV_HIP_CHECK(hipMemsetAsync(d_inlier_mask, 0, (size_t)total, stream));
    return SPV_OK;
  }
  const bool every_try = d_try_cameras || d_try_inliers;
  rounds.size_scratch(device_cu_count());
  DevBuf ws;
  SPV_TRY(ws.alloc(carve(nullptr, nviews, rounds.round_cap(), rounds.tables_bytes()).end));
  const FitBufs b = carve(ws.p, nviews, rounds.round_cap(), rounds.tables_bytes());
  StreamDrain drain{stream};
  SPV_HIP_CHECK(hipMemsetAsync(b.states, 0, (size_t)nviews * sizeof(ResectState), stream));
  if (every_try) {  // the rows of skipped sets: NaN cameras, zero counts
    if (d_try_inliers) SPV_HIP_CHECK(hipMemsetAsync(d_try_inliers, 0, (size_t)nviews * max_tries * sizeof(int32_t), stream));
    if (d_try_cameras) SPV_HIP_CHECK(hipMemsetAsync(d_try_cameras, 0xFF, (size_t)nviews * max_tries * 12 * sizeof(double), stream));
  }
  const double me2 = max_error < 0 ? -1.0 : max_error * max_error;
  // with per-try outputs no set leaves early
  SPV_TRY(rounds.run(samples, seeds, every_try, b.tables, b.heads, stream, [&](const FitRoundTables &t) -> int {
    SPV_HIP_CHECK(hipMemsetAsync(b.counts, 0, (size_t)t.ntries * sizeof(int), stream));
    {
      ProfScope prof("resect_solve", stream);
      hipLaunchKernelGGL(resect_solve_kernel, dim3((unsigned)((t.ntries + kSolveThreads - 1) / kSolveThreads)),
                         dim3(kSolveThreads), 0, stream, t.samples, t.ntries, d_x, d_Xw, b.cams);
      SPV_HIP_CHECK(hipGetLastError());
    }
    {
      ProfScope prof("resect_score", stream);
      hipLaunchKernelGGL(resect_score_kernel, dim3((unsigned)t.nitems), dim3(kDltThreads), 0, stream, t.items,
                         (const double *)b.cams, d_x, d_Xw, me2, b.counts);
      SPV_HIP_CHECK(hipGetLastError());
    }
    ProfScope prof("resect_reduce", stream);
    hipLaunchKernelGGL(resect_reduce_kernel, dim3((unsigned)t.nslots), dim3(kReduceThreads), 0, stream, t.slots,
                       (const int *)b.counts, (const double *)b.cams, required_percent, find_best, max_tries, b.states,
                       b.heads, d_try_cameras, d_try_inliers);
    SPV_HIP_CHECK(hipGetLastError());
    return SPV_OK;
  }, tries_run));
  const std::vector<FitHead> &last = rounds.last();
  fit_outputs_set(out, kResect, view_off, last);
  if (d_inlier_mask) {
    // the kept camera of every set over all its rows: the scorer's statements, hence the scorer's count
    std::vector<RansacBatchItem> items;  // one item per row block of every set, all under "try" 0
    for (int p = 0; p < nviews; ++p)
      for (long long r = view_off[p]; r < view_off[p + 1]; r += kDltThreads)
        items.push_back(RansacBatchItem{p, (int32_t)r, (int32_t)std::min<long long>(kDltThreads, view_off[p + 1] - r), 0, 1});
    const size_t bytes = items.size() * sizeof(RansacBatchItem);
    if (bytes > b.tables_bytes) return set_error(SPV_ERR_INTERNAL, "last pass of %zu items outgrew its scratch", items.size());
    SPV_HIP_CHECK(hipMemcpyAsync(b.tables, items.data(), bytes, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(resect_mask_kernel, dim3((unsigned)items.size()), dim3(kDltThreads), 0, stream,
                       reinterpret_cast<const RansacBatchItem *>(b.tables), (const ResectState *)b.states, d_x, d_Xw, me2,
                       d_inlier_mask);
    SPV_HIP_CHECK(hipGetLastError());
  }
  std::vector<ResectState> full((size_t)nviews);
  SPV_HIP_CHECK(hipMemcpyAsync(full.data(), b.states, (size_t)nviews * sizeof(ResectState), hipMemcpyDeviceToHost, stream));
  SPV_HIP_CHECK(hipStreamSynchronize(stream));
  for (int p = 0; p < nviews; ++p)
    if (last[p].found)
      for (int i = 0; i < 12; ++i) camera[(size_t)p * 12 + i] = full[p].P[i];
  return SPV_OK;
}

}  // namespace spv
