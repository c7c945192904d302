// ransac_batch.hip -- two-view RANSAC of many correspondence sets in one call (gfx950).
//
// ransac.hip fits one set: a few small launches per batch of tries and one host wait per batch.  A view set has
// hundreds of image pairs with a few hundred to a few thousand correspondences each, many of which never succeed
// and run every try; one after another they are a chain of small launches and host waits on a chip that each of
// them fills to a few percent.  Here the sets of a collection (rows [pair_off[p], pair_off[p + 1]) of one pair of
// arrays) advance together, in rounds.  The rounds are fit_rounds.hip's, which resect_batch.hip shares: the running
// sets, the rule that fills a round, the upload of its tables, the read-back of the heads, the one stream
// synchronisation and which sets leave.  This file supplies (kTwoView): 7-subsets drawn by floyd_sample, three
// candidates a try, sets of 10 rows and more, a round of at most kRoundTries tries and kRoundSolves solves at 12 a
// row, ransac_fit_run's small-first growth per set (256 tries or fewer, then fourfold to the set's batch), each
// try's set size as an extra table, and the kernels of a round:
//
//   seven_point_kernel<true> (ransac.hip) and essential_cameras_kernel (dlt.hip) run unchanged over all tries
//   and all 3 x tries candidates of the round;
//   ransac_batch_score_kernel   one workgroup per work item = (<= 256 rows of one set, a range of that set's
//                               candidates): rows staged in LDS once, the range's ungated candidates compacted
//                               into LDS 256 at a time, four cameras each scored with dlt_score_kernel's very
//                               statements (dlt_device.h), slow solves to the sharded work list
//   ransac_batch_fallback_kernel the work list, one lane per entry, as dlt_score_fallback_kernel
//   ransac_batch_select_kernel  select_camera_kernel with the candidate's own set size
//   ransac_batch_reduce_kernel  ransac_reduce_kernel, one workgroup per set of the round over that set's
//                               candidates in order (best_model_device.h), into that set's FitState; the
//                               four-int heads of the round's sets go to one compact array.
//
// A last pass scores the kept candidate of every set once more, with masks, through the same kernels.
//
// Why the results are the single fit's bits: the seven-point solve is per try and reads the same seven rows; the
// gate, E and the cameras are per candidate; an inlier decision is per (camera, correspondence) and does not
// depend on the path that took it; counts are integer sums; and the best-model rule is defined on try order --
// the first candidate above the share, else most inliers with the earliest among equals -- which holds however
// the tries are cut into rounds.  Only tries_run depends on the cuts.
//
// The work items (ransac_batch_items, host): a set's rows are cut into blocks of 256; with B row blocks in the
// round and fewer than 4 workgroups per compute unit, every set's candidates are cut into ceil(4 CUs / B)
// ranges (never below kMinPieceCands candidates a range, so that staging the rows stays a small part of an
// item).  64 sets of 500 rows are 128 row blocks: uncut they would leave half of the chip idle.
#include "best_model_device.h"
#include "common.h"
#include "dlt_device.h"
#include "fit_rounds.h"
#include "host_io.h"

#include <limits.h>
#include <string.h>

namespace spv {
namespace {

constexpr int kRoundTries = 32768;                  // tries of all sets in one round: 98 304 candidates, ~60 MB of scratch
constexpr long long kRoundSolves = 2000000000ll;    // (camera, correspondence) solves if nothing were gated, as ransac_fit_batch_limit
constexpr int kMinPieceCands = 48;                  // candidates per work item when a set's candidates are cut
constexpr int kMinSetRows = 10;                     // RansacFitter's constructor limit, here per set: smaller sets are skipped
constexpr int kBatchReduceThreads = 256;

// The scorer.  mask4 (the last pass only, where a row meets one candidate): uint8[4, total], camera k of the
// row's candidate at mask4[k total + row]; rows of gated candidates stay unwritten.
template <bool TWO_PASS>
__global__ __launch_bounds__(kDltThreads) void ransac_batch_score_kernel(
    Cameras cam0, const RansacBatchItem *__restrict__ items, const double *__restrict__ cams,
    const int *__restrict__ gated, const double *__restrict__ x, const double *__restrict__ xp, double max_error,
    int *__restrict__ counts, unsigned char *__restrict__ mask4, long long total, WorkList wl) {
  __shared__ double sx[kDltThreads * 3];
  __shared__ double sxp[kDltThreads * 3];
  __shared__ int s_live[kDltThreads];
  __shared__ int s_nlive;
  const RansacBatchItem it = items[blockIdx.x];
  const long long base = it.row0;
  const int nblk = it.rows;
  for (int e = threadIdx.x; e < nblk * 3; e += kDltThreads) {
    sx[e] = x[base * 3 + e];
    sxp[e] = xp[base * 3 + e];
  }
  const int t = threadIdx.x;
  const bool live = t < nblk;
  const int cend = it.cand0 + it.ncand;
  for (int c0 = it.cand0; c0 < cend; c0 += kDltThreads) {  // workgroup-uniform
    __syncthreads();  // the rows are staged; the list of the round before has been walked
    if (t == 0) s_nlive = 0;
    __syncthreads();
    // almost every candidate of a RANSAC round is gated: the ungated ones of this stretch, in any order
    // (every (camera, correspondence) result stands alone)
    if (c0 + t < cend && !gated[c0 + t]) s_live[atomicAdd(&s_nlive, 1)] = c0 + t;
    __syncthreads();
    const int nl = s_nlive;
    for (int y = 0; y < 4 * nl; ++y) {
      const int h = 4 * s_live[y >> 2] + (y & 3);
      Cameras cam;
#pragma unroll
      for (int i = 0; i < 12; ++i) {
        cam.p0[i] = cam0.p0[i];
        cam.p1[i] = cams[(size_t)h * 12 + i];  // wave-uniform
      }
      if (cam.p1[0] != cam.p1[0]) continue;  // a NaN camera of an ungated candidate: nothing is an inlier
      double A[4][4], xv[4], u = 0, v = 0, up = 0, vp = 0;
      bool solved = true;  // dead lanes have nothing to solve
      if (live) {
        dlt_matrix(cam, sx[3 * t], sx[3 * t + 1], sx[3 * t + 2], sxp[3 * t], sxp[3 * t + 1], sxp[3 * t + 2], A, u, v,
                   up, vp);
        solved = null_gs_inverse_iteration(A, xv);
      }
      bool deferred = false;
      if (TWO_PASS) {
        // slow lanes of the wave -> work list
        const unsigned long long slow = __ballot(!solved);
        if (slow) {
          const int lane = threadIdx.x & 63;
          const unsigned int shard = ((unsigned)h * gridDim.x + blockIdx.x) * (kDltThreads / 64) + (threadIdx.x >> 6);
          const unsigned int sh = shard % kListShards;
          unsigned int first = 0;
          if (lane == 0) first = atomicAdd(wl.count + sh * kCountStride, (unsigned int)__popcll(slow));
          first = __shfl(first, 0, 64);
          if (!solved) {
            const unsigned int slot = first + (unsigned int)__popcll(slow & ((1ull << lane) - 1ull));
            if (slot < wl.segment) {
              wl.entries[(size_t)sh * wl.segment + slot] = ((unsigned long long)h << 40) | (unsigned long long)(base + t);
              deferred = true;
            }
          }
        }
      }
      if (!solved && !deferred) null_jacobi(A, xv);  // in place: no work list, or it is full
      bool inlier = false;
      if (live && !deferred) {
        double X[4];
        dlt_finish(xv, X);
        inlier = score_inlier(cam, X, u, v, up, vp, max_error);
        if (mask4) mask4[(size_t)(h & 3) * total + base + t] = inlier ? 1 : 0;
      }
      const unsigned long long bal = __ballot(inlier);
      if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&counts[h], __popcll(bal));
    }
  }
}

// Second pass: one lane per work-list entry, method 1 (dlt_score_fallback_kernel with this file's mask layout).
__global__ __launch_bounds__(kDltThreads) void ransac_batch_fallback_kernel(
    Cameras cam0, const double *__restrict__ cams, const double *__restrict__ x, const double *__restrict__ xp,
    double max_error, int *__restrict__ counts, unsigned char *__restrict__ mask4, long long total, WorkList wl) {
  const unsigned int n = kListShards * wl.segment;
  for (unsigned int i = blockIdx.x * kDltThreads + threadIdx.x; i < n; i += gridDim.x * kDltThreads) {
    const unsigned int sh = i % kListShards, slot = i / kListShards;  // slot-major: full waves over the filled part
    if (slot >= min(wl.count[sh * kCountStride], wl.segment)) continue;
    const unsigned long long e = wl.entries[(size_t)sh * wl.segment + slot];
    const int h = (int)(e >> 40);
    const long long p = (long long)(e & ((1ull << 40) - 1ull));
    Cameras cam;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      cam.p0[k] = cam0.p0[k];
      cam.p1[k] = cams[(size_t)h * 12 + k];
    }
    double A[4][4], xv[4], X[4], u, v, up, vp;
    dlt_matrix(cam, x[3 * p], x[3 * p + 1], x[3 * p + 2], xp[3 * p], xp[3 * p + 1], xp[3 * p + 2], A, u, v, up, vp);
    null_jacobi(A, xv);
    dlt_finish(xv, X);
    const bool inlier = score_inlier(cam, X, u, v, up, vp, max_error);
    if (mask4) mask4[(size_t)(h & 3) * total + p] = inlier ? 1 : 0;
    if (inlier) atomicAdd(&counts[h], 1);
  }
}

// select_camera_kernel (dlt.hip, src/RansacFitter.h:74-84) with the set size of the candidate's own set:
// npt_of[f / per].
__global__ __launch_bounds__(kDltThreads) void ransac_batch_select_kernel(
    const int *__restrict__ counts, const int *__restrict__ gated, const double *__restrict__ cams, int nF,
    const int *__restrict__ npt_of, int per, double required_percent, int find_best, int *__restrict__ success,
    int *__restrict__ inlier_count, int *__restrict__ best_cam, double *__restrict__ best_P) {
  const int f = blockIdx.x * kDltThreads + threadIdx.x;
  if (f >= nF) return;
  const int npt = npt_of[f / per];
  int ok = 0, best = -1, nbest = 0;
  if (!gated[f]) {
    double best_percent = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ninlier = counts[4 * f + k];
      const double percent = ninlier / (double)npt;
      if ((percent >= required_percent || find_best) && percent > best_percent) {
        best_percent = percent;
        nbest = ninlier;
        best = k;
        ok = 1;
      }
    }
  }
  success[f] = ok;
  inlier_count[f] = nbest;
  best_cam[f] = best;
  if (best_P)
#pragma unroll
    for (int i = 0; i < 12; ++i) best_P[(size_t)f * 12 + i] = ok ? cams[(size_t)f * 48 + 12 * best + i] : 0.0;
}

// ransac_reduce_kernel (ransac.hip, src/RansacFitter.h:196-214), one workgroup per slot of the round.
__global__ __launch_bounds__(kBatchReduceThreads) void ransac_batch_reduce_kernel(
    const RansacBatchSlot *__restrict__ slots, const int *__restrict__ ok, const int *__restrict__ count,
    const double *__restrict__ Fs, const double *__restrict__ best_P, double required_percent, int find_best,
    FitState *__restrict__ states, FitHead *__restrict__ heads) {
  const RansacBatchSlot sl = slots[blockIdx.x];
  FitState *state = states + sl.set;
  int success;
  // (state->success is uniform: nothing after the first success is looked at)
  const int win = best_model<kBatchReduceThreads>(
      sl.ncand, state->success != 0, (double)(long long)sl.npt, state->found ? state->count : 0, find_best,
      [=](int i) { return ok[sl.cand0 + i] ? count[sl.cand0 + i] : -1; },
      [=](double share) { return share > required_percent; }, &success);
  if (threadIdx.x != 0) return;
  if (win >= 0) {
    const size_t w = (size_t)sl.cand0 + win;
    state->found = 1;
    state->success = success;
    state->count = count[w];
    state->cand = sl.cand_base + win;
    for (int i = 0; i < 9; ++i) state->F[i] = Fs[w * 9 + i];
    for (int i = 0; i < 12; ++i) state->P[i] = best_P[w * 12 + i];
  }
  heads[blockIdx.x] = FitHead{state->found, state->success, state->count, state->cand};
}

// The last pass's candidates: the kept F of every set, NaN (= gated) where a set kept none.
__global__ __launch_bounds__(kDltThreads) void ransac_batch_kept_kernel(const FitState *__restrict__ states, int nsets,
                                                                        double *__restrict__ Fs) {
  const int p = blockIdx.x * kDltThreads + threadIdx.x;
  if (p >= nsets) return;
  const double nan = __builtin_nan("");
  for (int i = 0; i < 9; ++i) Fs[(size_t)p * 9 + i] = states[p].found ? states[p].F[i] : nan;
}

// mask[row] = the inlier flag of the best camera of the row's set; 0 where the set kept no model.  One workgroup
// per row block of the last pass's items, which cover every row of the collection.
__global__ __launch_bounds__(kDltThreads) void ransac_batch_mask_kernel(const RansacBatchItem *__restrict__ items,
                                                                        const unsigned char *__restrict__ mask4,
                                                                        const int *__restrict__ best_cam, long long total,
                                                                        unsigned char *__restrict__ mask) {
  const RansacBatchItem it = items[blockIdx.x];
  if ((int)threadIdx.x >= it.rows) return;
  const int b = best_cam[it.set];
  const size_t row = (size_t)it.row0 + threadIdx.x;
  mask[row] = b >= 0 ? mask4[(size_t)b * total + row] : 0;
}

unsigned int batch_segment(unsigned long long pairs) {  // entries per shard of the work list, as dlt.hip sizes it
  const unsigned long long cap = std::min<unsigned long long>(pairs, 1ull << 22);
  return (unsigned int)std::max<unsigned long long>((cap + kListShards - 1) / kListShards, 64);
}
constexpr size_t kCountBytes = (size_t)kListShards * kCountStride * sizeof(unsigned int);

// Scratch of one call, carved once: the round buffers hold `tries` tries and `items` work items, the last pass
// npairs candidates over `total` rows.
struct BatchBufs {
  FitState *states;
  FitHead *heads;
  unsigned char *tables;  // a round's upload: samples, try_npt, slots, items (the last pass: set_npt, items)
  size_t tables_bytes;
  double *Fs, *cams, *best_P;
  int *gated, *nlive, *counts, *ok, *count, *best_cam;
  unsigned int *wl_count;
  unsigned long long *wl_entries;
  unsigned int segment;
  unsigned char *mask4, *mask;
  size_t end;
};
BatchBufs carve(void *base, int npairs, long long total, int tries, size_t tables_bytes, bool own_mask) {
  const size_t nc = (size_t)std::max(3 * tries, npairs);
  WsWalk w(base);
  BatchBufs b{};
  b.states = w.take<FitState>((size_t)npairs * sizeof(FitState));
  b.heads = w.take<FitHead>((size_t)npairs * sizeof(FitHead));
  b.tables_bytes = tables_bytes;
  b.tables = w.take(b.tables_bytes);
  b.Fs = w.take<double>(nc * 9 * sizeof(double));
  b.cams = w.take<double>(nc * 48 * sizeof(double));
  b.best_P = w.take<double>(nc * 12 * sizeof(double));
  b.gated = w.take<int>(nc * sizeof(int));
  b.nlive = w.take<int>((nc + 1) * sizeof(int));
  b.counts = w.take<int>(nc * 4 * sizeof(int));
  b.ok = w.take<int>(nc * sizeof(int));
  b.count = w.take<int>(nc * sizeof(int));
  b.best_cam = w.take<int>(nc * sizeof(int));
  b.wl_count = w.take<unsigned int>(kCountBytes);
  b.segment = batch_segment(std::max<unsigned long long>(4ull * (unsigned long long)total, 1ull << 22));
  b.wl_entries = w.take<unsigned long long>((size_t)kListShards * b.segment * sizeof(unsigned long long));
  b.mask4 = w.take(4 * (size_t)total);
  if (own_mask) b.mask = w.take((size_t)total);
  b.end = w.end();
  return b;
}

// The scorer and its second pass over `nitems` items of d_items.
int score_items(const BatchBufs &b, const RansacBatchItem *d_items, int nitems, const double *d_x0, const double *d_x1,
                double max_error, int ncand, unsigned char *mask4, long long total, hipStream_t stream) {
  const double P0[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // Camera(): Identity(3,4), src/Camera.h:27
  Cameras cam0;
  for (int i = 0; i < 12; ++i) cam0.p0[i] = cam0.p1[i] = P0[i];
  SPV_HIP_CHECK(hipMemsetAsync(b.counts, 0, (size_t)ncand * 4 * sizeof(int), stream));
  SPV_HIP_CHECK(hipMemsetAsync(b.wl_count, 0, kCountBytes, stream));
  if (nitems == 0) return SPV_OK;
  const WorkList wl{b.wl_count, b.wl_entries, b.segment};
  ProfScope prof("ransac_batch_score", stream);
  hipLaunchKernelGGL(ransac_batch_score_kernel<true>, dim3((unsigned)nitems), dim3(kDltThreads), 0, stream, cam0, d_items,
                     (const double *)b.cams, (const int *)b.gated, d_x0, d_x1, max_error, b.counts, mask4, total, wl);
  SPV_HIP_CHECK(hipGetLastError());
  const unsigned fb = (unsigned)std::min<unsigned long long>(((unsigned long long)kListShards * wl.segment + kDltThreads - 1) / kDltThreads,
                                                             (unsigned long long)device_cu_count() * 16);
  hipLaunchKernelGGL(ransac_batch_fallback_kernel, dim3(std::max(fb, 1u)), dim3(kDltThreads), 0, stream, cam0,
                     (const double *)b.cams, d_x0, d_x1, max_error, b.counts, mask4, total, wl);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

}  // namespace

void ransac_batch_items(const std::vector<RansacBatchSlot> &slots, const long long *pair_off, int cus,
                        std::vector<RansacBatchItem> *items) {
  items->clear();
  size_t blocks = 0;
  for (const RansacBatchSlot &s : slots) blocks += batch_row_blocks(s.npt);
  if (blocks == 0) return;
  const size_t target = 4 * (size_t)std::max(cus, 1);
  const int pieces = (int)std::min<size_t>((target + blocks - 1) / blocks, 1u << 16);
  for (const RansacBatchSlot &s : slots) {
    const int cut = std::max(1, std::min(pieces, s.ncand / kMinPieceCands));
    const int chunk = (s.ncand + cut - 1) / cut;
    for (long long r = 0; r < s.npt; r += kDltThreads)
      for (int c = 0; c < s.ncand; c += chunk)
        items->push_back(RansacBatchItem{s.set, (int32_t)(pair_off[s.set] + r), (int32_t)std::min<long long>(kDltThreads, s.npt - r),
                                         s.cand0 + c, std::min(chunk, s.ncand - c)});
  }
}

namespace {
// What this fit gives the round driver (fit_rounds.h).  A set's steps are ransac_fit_run's: its first batch, then
// fourfold up to its full batch.  A try is three candidates of four cameras each: 12 solves a row.
void two_view_steps(long long npt, int max_tries, int *first, int *top) {
  *top = std::min(ransac_fit_batch_limit(npt), max_tries);
  *first = ransac_first_step(npt, *top);
}
const FitRoundsOp kTwoView{7, 3, kMinSetRows, kRoundTries, kRoundSolves, 12, two_view_steps, floyd_sample, true};
}  // namespace

void ransac_batch_first_round(const long long *pair_off, int npairs, int max_tries, std::vector<RansacBatchSlot> *slots) {
  FitRounds(kTwoView, pair_off, npairs, max_tries).fill_round(slots, nullptr);
}

int ransac_batch_check(const long long *pair_off, int npairs, int max_tries, const int32_t *samples) {
  return fit_sets_check(pair_off, npairs, max_tries, samples, kTwoView.width, kTwoView.min_rows, "pair_off",
                        "maximum_tries above 7e8 (candidate ids are 32-bit: 3 per try)");
}

int ransac_fit_batch_run(const double *d_x0, const double *d_x1, const long long *pair_off, int npairs,
                         double required_percent, double max_error, int max_tries, int find_best, double ratio_allowed,
                         const int32_t *samples, const unsigned long long *seeds, int32_t *success, double *essential,
                         double *camera, double *inlier_percent, int32_t *inlier_idx, int32_t *n_inliers,
                         int32_t *best_try, int32_t *best_root, int32_t *tries_run, unsigned char *d_inlier_mask,
                         hipStream_t stream) {
  SPV_TRY(ransac_batch_check(pair_off, npairs, max_tries, samples));
  const long long total = pair_off[npairs];
  if (npairs > 0 && (!success || !essential || !camera || !inlier_percent || !n_inliers))
    return set_error(SPV_ERR_INVALID, "null pointer");
  if (total > 0 && (!d_x0 || !d_x1 || !inlier_idx)) return set_error(SPV_ERR_INVALID, "null pointer");
  FitRounds rounds(kTwoView, pair_off, npairs, max_tries);
  if (!rounds.empty() && !samples && !seeds) return set_error(SPV_ERR_INVALID, "neither samples nor seeds");
  const FitOutputs out{success, inlier_percent, n_inliers, best_try, tries_run};
  fit_outputs_clear(out, npairs);
  for (int p = 0; p < npairs && best_root; ++p) best_root[p] = -1;
  if (rounds.empty()) {
    if (d_inlier_mask && total > 0) SPV_HIP_CHECK(hipMemsetAsync(d_inlier_mask, 0, (size_t)total, stream));
    return SPV_OK;
  }
  const int cus = device_cu_count();
  rounds.size_scratch(cus);
  // (the last pass's tables: every set's size, and items that the rounds' cap covers)
  const size_t tables_bytes = rounds.tables_bytes() + (size_t)npairs * sizeof(int);
  DevBuf ws;
  const size_t ws_bytes = carve(nullptr, npairs, total, rounds.round_cap(), tables_bytes, d_inlier_mask == nullptr).end;
  SPV_TRY(ws.alloc(ws_bytes));
  BatchBufs b = carve(ws.p, npairs, total, rounds.round_cap(), tables_bytes, d_inlier_mask == nullptr);
  if (d_inlier_mask) b.mask = d_inlier_mask;
  StreamDrain drain{stream};
  SPV_HIP_CHECK(hipMemsetAsync(b.states, 0, (size_t)npairs * sizeof(FitState), stream));

  SPV_TRY(rounds.run(samples, seeds, false, b.tables, b.heads, stream, [&](const FitRoundTables &t) -> int {
    const int ncand = 3 * t.ntries;
    SPV_TRY(seven_point_sampled_run(d_x0, d_x1, t.samples, t.ntries, b.Fs, stream));
    SPV_TRY(ransac_cameras_run(b.Fs, ncand, ratio_allowed, b.cams, b.gated, b.nlive + 1, b.nlive, stream));
    SPV_TRY(score_items(b, t.items, t.nitems, d_x0, d_x1, max_error, ncand, nullptr, total, stream));
    hipLaunchKernelGGL(ransac_batch_select_kernel, dim3((ncand + kDltThreads - 1) / kDltThreads), dim3(kDltThreads), 0,
                       stream, (const int *)b.counts, (const int *)b.gated, (const double *)b.cams, ncand, t.try_npt, 3,
                       required_percent, find_best, b.ok, b.count, b.best_cam, b.best_P);
    SPV_HIP_CHECK(hipGetLastError());
    ProfScope prof("ransac_batch_reduce", stream);
    hipLaunchKernelGGL(ransac_batch_reduce_kernel, dim3((unsigned)t.nslots), dim3(kBatchReduceThreads), 0, stream, t.slots,
                       (const int *)b.ok, (const int *)b.count, (const double *)b.Fs, (const double *)b.best_P,
                       required_percent, find_best, b.states, b.heads);
    SPV_HIP_CHECK(hipGetLastError());
    return SPV_OK;
  }, tries_run));
  const std::vector<FitHead> &last = rounds.last();
  fit_outputs_set(out, kTwoView, pair_off, last);
  int nfound = 0;
  for (int p = 0; p < npairs; ++p) {
    if (best_root) best_root[p] = last[p].found ? last[p].cand % 3 : -1;
    nfound += last[p].found ? 1 : 0;
  }
  if (nfound == 0) {
    if (d_inlier_mask && total > 0) SPV_HIP_CHECK(hipMemsetAsync(d_inlier_mask, 0, (size_t)total, stream));
    return SPV_OK;
  }
  // the kept candidate of every set once more, this time with masks (same statements per (camera, correspondence),
  // hence the same best camera and the same count); the items cover every row, so every mask byte is written
  std::vector<RansacBatchSlot> slots;
  std::vector<RansacBatchItem> items;
  for (int p = 0; p < npairs; ++p) {
    const long long npt = pair_off[p + 1] - pair_off[p];
    if (npt > 0) slots.push_back(RansacBatchSlot{p, (int)npt, p, 1, 0});
  }
  ransac_batch_items(slots, pair_off, cus, &items);
  const size_t off_items = round_up((size_t)npairs * sizeof(int), 16);
  const size_t bytes = off_items + items.size() * sizeof(RansacBatchItem);
  if (bytes > b.tables_bytes) return set_error(SPV_ERR_INTERNAL, "last pass of %zu items outgrew its scratch", items.size());
  std::vector<unsigned char> host(bytes, 0);
  int *h_npt = reinterpret_cast<int *>(host.data());
  for (int p = 0; p < npairs; ++p) h_npt[p] = (int)std::max<long long>(pair_off[p + 1] - pair_off[p], 1);
  memcpy(host.data() + off_items, items.data(), items.size() * sizeof(RansacBatchItem));
  SPV_HIP_CHECK(hipMemcpyAsync(b.tables, host.data(), bytes, hipMemcpyHostToDevice, stream));
  const int *d_npt = reinterpret_cast<const int *>(b.tables);
  const RansacBatchItem *d_items = reinterpret_cast<const RansacBatchItem *>(b.tables + off_items);
  hipLaunchKernelGGL(ransac_batch_kept_kernel, dim3((npairs + kDltThreads - 1) / kDltThreads), dim3(kDltThreads), 0, stream,
                     (const FitState *)b.states, npairs, b.Fs);
  SPV_HIP_CHECK(hipGetLastError());
  SPV_TRY(ransac_cameras_run(b.Fs, npairs, ratio_allowed, b.cams, b.gated, b.nlive + 1, b.nlive, stream));
  SPV_TRY(score_items(b, d_items, (int)items.size(), d_x0, d_x1, max_error, npairs, b.mask4, total, stream));
  hipLaunchKernelGGL(ransac_batch_select_kernel, dim3((npairs + kDltThreads - 1) / kDltThreads), dim3(kDltThreads), 0,
                     stream, (const int *)b.counts, (const int *)b.gated, (const double *)b.cams, npairs, d_npt, 1,
                     required_percent, find_best, b.ok, b.count, b.best_cam, (double *)nullptr);
  SPV_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(ransac_batch_mask_kernel, dim3((unsigned)items.size()), dim3(kDltThreads), 0, stream, d_items,
                     (const unsigned char *)b.mask4, (const int *)b.best_cam, total, b.mask);
  SPV_HIP_CHECK(hipGetLastError());
  std::vector<FitState> full((size_t)npairs);
  std::vector<unsigned char> mask((size_t)total);
  SPV_HIP_CHECK(hipMemcpyAsync(full.data(), b.states, (size_t)npairs * sizeof(FitState), hipMemcpyDeviceToHost, stream));
  SPV_HIP_CHECK(hipMemcpyAsync(mask.data(), b.mask, (size_t)total, hipMemcpyDeviceToHost, stream));
  SPV_HIP_CHECK(hipStreamSynchronize(stream));
  for (int p = 0; p < npairs; ++p) {
    if (!last[p].found) continue;
    for (int i = 0; i < 9; ++i) essential[(size_t)p * 9 + i] = full[p].F[i];
    for (int i = 0; i < 12; ++i) camera[(size_t)p * 12 + i] = full[p].P[i];
    const long long r0 = pair_off[p], npt = pair_off[p + 1] - r0;
    int n = 0;
    for (long long i = 0; i < npt; ++i)
      if (mask[(size_t)(r0 + i)]) inlier_idx[r0 + n++] = (int32_t)i;
    if (n != n_inliers[p]) return set_error(SPV_ERR_HIP, "set %d: inlier list has %d entries, the count was %d", p, n, n_inliers[p]);
  }
  return SPV_OK;
}

}  // namespace spv
