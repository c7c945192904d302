// dlt_batch.hip -- two-view DLT triangulation of many correspondence sets in one call (gfx950).
//
// dlt.hip triangulates one set per launch, its camera pair passed by value: the step after a many-sets RANSAC
// (ransac_batch.hip) -- every set's inliers against that set's camera -- would be one row gather and one launch per
// set of a kernel shaped for millions of points.  Here the sets of a collection (rows [pair_off[p], pair_off[p + 1])
// of one pair of arrays) are solved by one kernel, each with the camera pair of its set from a table in HBM, and
// the selection (ransac_batch.hip's inlier mask over the concatenated rows) is applied on the way: selected rows
// come out back to back, in input order.
//
//   work items (dlt_batch_items, host)   every used set's rows in blocks of 256, in order; an item never straddles
//                                        two sets.  One upload brings the cameras, the items and two per-set tables.
//   dlt_batch_count_kernel   (mask only) selected rows per item
//   dlt_batch_scan_kernel    (mask only) one workgroup: the items' out bases (exclusive scan of the counts), the
//                                        selected rows before every set, the total
//   dlt_batch_kernel                     one workgroup per item, walking b, b + gridDim.x, ...: with a mask the
//                                        item's selected rows are compacted, in order, into an LDS list (one wave
//                                        scan and four wave sums) and lanes [0, selected) solve one listed row each
//                                        -- the solving waves are full whatever the mask's density, waves beyond the
//                                        list leave --; without a mask lane = row.  The item's set is uniform over
//                                        the workgroup: its 24 camera doubles are scalar loads.
//
// Why the results are the single calls' bits: a lane runs dlt_solve<true, false> (dlt_device.h), the very vector
// dlt.hip's error kernel passes to reprojection_error; and dlt_finish of that vector is dlt_finish of the solver's
// own iterate, which is what dlt.hip's triangulation kernel computes: the vector is the iterate times the power of
// two that brings its max-norm into [0.5, 1), dlt_finish looks for that power first, finds 2^0, and goes on with
// the same four numbers.  Nothing of a row's arithmetic depends on the item, the lane or the neighbours.
#include "common.h"
#include "device_util.h"
#include "dlt_device.h"
#include "host_io.h"

#include <string.h>

namespace spv {
namespace {

constexpr int kScanThreads = 1024;  // block_scan_inplace's workgroup

static_assert(sizeof(DltBatchItem) == 16, "items travel as int32[4]");

typedef double __attribute__((address_space(4))) ConstDouble;  // memory no kernel writes while this one runs

// The device form of a call's tables, one upload.
struct DltBatchTables {
  const double *cams;        // [npairs, 24]: P0, P1 of every set (zero where a set is not used)
  const DltBatchItem *items;
  const int32_t *set_row0;   // [npairs]: the first row of every set
  const int32_t *set_item0;  // [npairs + 1]: the first item at or after every set; [npairs] = nitems
  int nitems, npairs;
};

// rows [row0, row0 + rows) of the item that are selected, as a count per wave in s_wsum; returns this lane's flag
// and its inclusive rank within the wave.  One barrier.
__device__ __forceinline__ bool select_rows(const DltBatchItem &it, const uint8_t *__restrict__ mask, int *s_wsum,
                                            int &incl) {
  const int t = threadIdx.x;
  const bool sel = t < it.rows && mask[(size_t)it.row0 + t] != 0;
  incl = wave_scan_incl<int>(sel ? 1 : 0, t & 63);
  if ((t & 63) == 63) s_wsum[t >> 6] = incl;
  __syncthreads();
  return sel;
}

__global__ __launch_bounds__(kDltThreads) void dlt_batch_count_kernel(DltBatchTables tb, const uint8_t *__restrict__ mask,
                                                                      int32_t *__restrict__ counts) {
  __shared__ int s_wsum[kDltThreads / 64];
  for (int b = blockIdx.x; b < tb.nitems; b += gridDim.x) {
    const DltBatchItem it = tb.items[b];
    int incl;
    select_rows(it, mask, s_wsum, incl);
    if (threadIdx.x == 0) counts[b] = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
    __syncthreads();  // the sums have been read before the next item writes them
  }
}

// counts -> the items' out bases, in place; out_off[p] = selected rows before set p, out_off[npairs] = *count = all.
__global__ __launch_bounds__(kScanThreads) void dlt_batch_scan_kernel(DltBatchTables tb, int32_t *__restrict__ counts,
                                                                      long long *__restrict__ out_off,
                                                                      long long *__restrict__ count) {
  const int32_t total = block_scan_inplace<int32_t>(counts, tb.nitems);  // (ends in a barrier: the bases are visible)
  if (out_off)
    for (int p = threadIdx.x; p <= tb.npairs; p += kScanThreads) {
      const int i = tb.set_item0[p];
      out_off[p] = i < tb.nitems ? counts[i] : total;
    }
  if (count && threadIdx.x == 0) *count = total;
}

template <bool MASKED, bool WANT_X, bool WANT_ERR>
__global__ __launch_bounds__(kDltThreads) void dlt_batch_kernel(DltBatchTables tb, const double *__restrict__ x,
                                                                const double *__restrict__ xp,
                                                                const uint8_t *__restrict__ mask,
                                                                const int32_t *__restrict__ bases, long long capacity,
                                                                double *__restrict__ dX, double *__restrict__ derr,
                                                                int32_t *__restrict__ drows) {
  __shared__ int s_wsum[kDltThreads / 64];
  __shared__ int s_list[kDltThreads];
  const int t = threadIdx.x;
  for (int b = blockIdx.x; b < tb.nitems; b += gridDim.x) {  // workgroup-uniform
    const DltBatchItem it = tb.items[b];
    int r = t, n = it.rows;  // this lane's row within the item; rows the item solves
    long long out = it.out;
    if (MASKED) {
      int incl;
      const bool sel = select_rows(it, mask, s_wsum, incl);
      int woff = 0;
      for (int k = 0; k < (t >> 6); ++k) woff += s_wsum[k];
      n = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
      if (sel) s_list[woff + incl - 1] = t;
      __syncthreads();  // the list is whole; the next item's flags are a barrier away from these reads
      if (t < n) r = s_list[t];
      out = bases[b];
    }
    if (t >= n) continue;  // whole waves beyond the item's rows leave; the last wave's idle lanes wait in it
    out += t;
    if (out >= capacity) continue;
    // the set is the same in every lane: through an index the compiler can see is uniform, and the constant address
    // space (the table is written before the launch; behind a barrier the compiler would otherwise not take a
    // scalar load for granted), the 24 doubles are scalar loads into scalar registers
    const int set = __builtin_amdgcn_readfirstlane(it.set);
    const ConstDouble *cp = (const ConstDouble *)(tb.cams + (size_t)set * 24);
    Cameras cam;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      cam.p0[i] = cp[i];
      cam.p1[i] = cp[12 + i];
    }
    const size_t row = (size_t)it.row0 + r;
    double Xs[4], u, v, up, vp;
    dlt_solve<true, false>(cam, x[3 * row], x[3 * row + 1], x[3 * row + 2], xp[3 * row], xp[3 * row + 1], xp[3 * row + 2],
                           Xs, u, v, up, vp);
    if (WANT_ERR) {
      double z0, z1;
      derr[out] = reprojection_error(cam, Xs, u, v, up, vp, z0, z1);
    }
    if (WANT_X) {
      double X[4];
      dlt_finish(Xs, X);
      reinterpret_cast<double4 *>(dX)[out] = make_double4(X[0], X[1], X[2], X[3]);
    }
    if (drows) drows[out] = (int32_t)(row - (size_t)tb.set_row0[set]);
  }
}

template <bool MASKED>
void launch_main(bool want_x, bool want_err, dim3 grid, hipStream_t stream, const DltBatchTables &tb, const double *x,
                 const double *xp, const uint8_t *mask, const int32_t *bases, long long capacity, double *dX, double *derr,
                 int32_t *drows) {
  if (want_x && want_err)
    hipLaunchKernelGGL((dlt_batch_kernel<MASKED, true, true>), grid, dim3(kDltThreads), 0, stream, tb, x, xp, mask, bases,
                       capacity, dX, derr, drows);
  else if (want_x)
    hipLaunchKernelGGL((dlt_batch_kernel<MASKED, true, false>), grid, dim3(kDltThreads), 0, stream, tb, x, xp, mask, bases,
                       capacity, dX, derr, drows);
  else
    hipLaunchKernelGGL((dlt_batch_kernel<MASKED, false, true>), grid, dim3(kDltThreads), 0, stream, tb, x, xp, mask, bases,
                       capacity, dX, derr, drows);
}

}  // namespace

void dlt_batch_items(const long long *pair_off, int npairs, const int32_t *use, bool masked,
                     std::vector<DltBatchItem> *items, long long *used_sets, long long *bound) {
  items->clear();
  long long out = 0, used = 0;
  for (int p = 0; p < npairs; ++p) {
    if (use && !use[p]) continue;
    ++used;
    for (long long r = pair_off[p]; r < pair_off[p + 1]; r += kDltThreads) {
      const int rows = (int)std::min<long long>(kDltThreads, pair_off[p + 1] - r);
      items->push_back(DltBatchItem{p, (int32_t)r, rows, masked ? -1 : (int32_t)out});
      out += rows;
    }
  }
  if (used_sets) *used_sets = used;
  if (bound) *bound = out;
}

int dlt_batch_check(const double *d_x0, const double *d_x1, const long long *pair_off, int npairs, const double *P1s,
                    const void *X, const void *err, long long capacity) {
  SPV_TRY(ransac_batch_check(pair_off, npairs, 0, nullptr));  // the rules of pair_off are that call's
  if (capacity < 0) return set_error(SPV_ERR_INVALID, "negative capacity");
  if (npairs > 0 && !P1s) return set_error(SPV_ERR_INVALID, "null camera pointer");
  if (pair_off[npairs] > 0 && (!d_x0 || !d_x1)) return set_error(SPV_ERR_INVALID, "null pointer");
  if (!X && !err) return set_error(SPV_ERR_INVALID, "neither X nor err is wanted");
  return SPV_OK;
}

int dlt_batch_run(const double *d_x0, const double *d_x1, const long long *pair_off, int npairs, const double *P0s,
                  const double *P1s, const int32_t *use, const uint8_t *d_mask, double *d_X, double *d_err,
                  int32_t *d_rows, long long capacity, long long *d_out_off, long long *d_count, hipStream_t stream) {
  SPV_TRY(dlt_batch_check(d_x0, d_x1, pair_off, npairs, P1s, d_X, d_err, capacity));
  if (((reinterpret_cast<uintptr_t>(d_X) | reinterpret_cast<uintptr_t>(d_err)) & 7) || (reinterpret_cast<uintptr_t>(d_rows) & 3))
    return set_error(SPV_ERR_INVALID, "output pointers must be aligned to their element size");
  const bool masked = d_mask != nullptr;
  std::vector<DltBatchItem> items;
  dlt_batch_items(pair_off, npairs, use, masked, &items, nullptr, nullptr);
  const size_t nitems = items.size();
  // what the host knows of the offsets: everything without a mask, and that nothing is selected without an item
  std::vector<long long> off((size_t)npairs + 2, 0);
  if (!masked)
    for (int p = 0; p < npairs; ++p)
      off[(size_t)p + 1] = off[p] + ((use && !use[p]) ? 0 : pair_off[p + 1] - pair_off[p]);
  off[(size_t)npairs + 1] = off[npairs];  // the count
  if (!masked || nitems == 0) {
    // (pageable source: the copies have left `off` when the calls return)
    if (d_out_off) SPV_HIP_CHECK(hipMemcpyAsync(d_out_off, off.data(), ((size_t)npairs + 1) * sizeof(long long), hipMemcpyHostToDevice, stream));
    if (d_count) SPV_HIP_CHECK(hipMemcpyAsync(d_count, off.data() + npairs + 1, sizeof(long long), hipMemcpyHostToDevice, stream));
  }
  if (nitems == 0) return SPV_OK;

  // the call's tables, one upload: cameras | items | set_row0 | set_item0; behind them the items' counts / bases
  const size_t off_items = (size_t)npairs * 24 * sizeof(double), off_row0 = off_items + nitems * sizeof(DltBatchItem);
  const size_t off_item0 = off_row0 + (size_t)npairs * sizeof(int32_t);
  const size_t table_bytes = off_item0 + ((size_t)npairs + 1) * sizeof(int32_t);
  const size_t off_counts = round_up(table_bytes, 256);
  std::vector<unsigned char> host(table_bytes, 0);
  double *h_cams = reinterpret_cast<double *>(host.data());
  int32_t *h_row0 = reinterpret_cast<int32_t *>(host.data() + off_row0);
  int32_t *h_item0 = reinterpret_cast<int32_t *>(host.data() + off_item0);
  const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // Camera(): Identity(3,4), src/Camera.h:27
  for (int p = 0; p < npairs; ++p) {
    h_row0[p] = (int32_t)pair_off[p];
    if (use && !use[p]) continue;  // a skipped set's cameras are not read
    memcpy(h_cams + (size_t)p * 24, P0s ? P0s + (size_t)p * 12 : eye, 12 * sizeof(double));
    memcpy(h_cams + (size_t)p * 24 + 12, P1s + (size_t)p * 12, 12 * sizeof(double));
  }
  memcpy(host.data() + off_items, items.data(), nitems * sizeof(DltBatchItem));
  {
    size_t i = 0;
    for (int p = 0; p <= npairs; ++p) {
      while (i < nitems && items[i].set < p) ++i;
      h_item0[p] = (int32_t)i;
    }
  }
  DevBuf ws;
  SPV_TRY(ws.alloc(off_counts + (masked ? nitems * sizeof(int32_t) : 0)));
  // the scratch goes back to the cache behind the last kernel of this call, on every way out
  struct Release {
    DevBuf &b;
    hipStream_t st;
    ~Release() { b.release_after(st); }
  } release{ws, stream};
  unsigned char *base = ws.as<unsigned char>();
  // (pageable source: the copy has left `host` when the call returns)
  SPV_HIP_CHECK(hipMemcpyAsync(base, host.data(), table_bytes, hipMemcpyHostToDevice, stream));
  const DltBatchTables tb{reinterpret_cast<const double *>(base), reinterpret_cast<const DltBatchItem *>(base + off_items),
                          reinterpret_cast<const int32_t *>(base + off_row0),
                          reinterpret_cast<const int32_t *>(base + off_item0), (int)nitems, npairs};
  int32_t *bases = masked ? reinterpret_cast<int32_t *>(base + off_counts) : nullptr;
  // at most 32 workgroups per compute unit, each walking its items
  const dim3 grid((unsigned)std::min<size_t>(nitems, (size_t)std::max(device_cu_count(), 1) * 32));
  if (masked) {
    ProfScope prof("dlt_batch_scan", stream);
    hipLaunchKernelGGL(dlt_batch_count_kernel, grid, dim3(kDltThreads), 0, stream, tb, d_mask, bases);
    SPV_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(dlt_batch_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, tb, bases, d_out_off, d_count);
    SPV_HIP_CHECK(hipGetLastError());
  }
  ProfScope prof("dlt_batch", stream);
  if (masked)
    launch_main<true>(d_X != nullptr, d_err != nullptr, grid, stream, tb, d_x0, d_x1, d_mask, bases, capacity, d_X, d_err, d_rows);
  else
    launch_main<false>(d_X != nullptr, d_err != nullptr, grid, stream, tb, d_x0, d_x1, d_mask, bases, capacity, d_X, d_err, d_rows);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

}  // namespace spv
