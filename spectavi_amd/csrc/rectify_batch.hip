// rectify_batch.hip -- epipolar-line rectification of many image pairs in one call (gfx950).
//
// rectify.hip rectifies one pair per launch, its F passed by value, and always writes the whole frame of
// hgt + 2 * int(max(hgt, wid * nchan) / 2) rows, of which the bounding box of the valid samples -- what the
// front-end's crop keeps, after reading both index images back -- is well under half for a real stereo pair.  Here
// the pairs of a view set (two images each out of one packed array of images, spv_sift_batch_device's layout) are
// rectified in two device steps with every table in HBM:
//
//   rectify_batch_bounds_kernel   one workgroup per item of 16 frame rows of one pair: every sample of those rows in
//                                 both images is evaluated (no pixel is read), the rows and columns of the valid ones
//                                 are reduced over the workgroup (wave shuffles, then LDS) and one lane folds the
//                                 item's four numbers into the pair's with integer atomicMin / atomicMax -- exact and
//                                 order-free.  A pair whose F is all NaN or all zero, or with rnx = 1, has no valid
//                                 sample by the contract (y, respectively x, is NaN) and owns no item.
//   rectify_batch_box_kernel      one lane per pair: the accumulated (min, max) as the half-open box, (0,0,0,0) where
//                                 nothing was valid
//   rectify_batch_kernel<T>       one workgroup per item of 8 window rows of one image of one pair, walking
//                                 b, b + gridDim.x, ...: lanes stride the window's columns, so a wave stores 64
//                                 consecutive samples; the gathered pixels come from L2.  Every element of the window
//                                 is written exactly once, the padding columns [rnx, cols) included; a pair's window
//                                 is a contiguous range of the outputs, all pairs back to back.
//
// Why the windows are the single call's bits: a sample is rectify_line + rectify_sample (rectify_device.h), the very
// functions rectify_kernel calls, with the same F (rectify_fundamental), delta and shape; nothing of a sample's
// arithmetic depends on the item, the lane or the rest of the collection.
#include "common.h"
#include "host_io.h"
#include "rectify_device.h"

#include <climits>
#include <cmath>
#include <string.h>

namespace spv {
namespace {

constexpr int kThreads = 256;
constexpr int kBoundsRows = 16;  // frame rows per item of the bounds kernel

static_assert(sizeof(RectifyBatchItem) == 16, "items travel as int32[4]");

// One pair as the kernels read it (a table in HBM, uniform over a workgroup).
struct RectifyBatchPair {
  double F[9];                  // row-major
  double delta;                 // (wid - 1) / (rnx - 1): inf or NaN when rnx = 1
  long long im0, im1;           // the pair's images: pixels before them in the packed array
  long long out;                // the pair's window: samples before it in the outputs
  int32_t wid, hgt, rnx, cols;  // cols: columns of the uncropped frame
  int32_t extra, row_lo, col_lo, col_hi;
};
static_assert(sizeof(RectifyBatchPair) % 8 == 0, "the items behind the table stay aligned");

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
  return v;
}

// acc int32[npairs, 4] = (min row, max row, min col, max col) of the valid samples, set to (INT_MAX, -1, INT_MAX, -1)
// before the launch.
__global__ __launch_bounds__(kThreads) void rectify_batch_bounds_kernel(const RectifyBatchPair *__restrict__ pairs,
                                                                        const RectifyBatchItem *__restrict__ items,
                                                                        long long nitems, int32_t *__restrict__ acc) {
  __shared__ int s_part[kThreads / 64][4];
  const int t = threadIdx.x;
  for (long long b = blockIdx.x; b < nitems; b += gridDim.x) {  // workgroup-uniform
    const RectifyBatchItem it = items[b];
    const RectifyBatchPair pr = pairs[it.pair];
    const int n = min(pr.rnx, pr.cols);  // samples beyond the frame's columns are dropped
    int rlo = INT_MAX, rhi = -1, clo = INT_MAX, chi = -1;
    for (int r = it.row0; r < it.row0 + it.rows; ++r) {
      const double v = (double)(r - pr.extra);
      double a0, a1, a2, b0, b1, b2;
      rectify_line(pr.F, pr.delta, v, 0, a0, a1, a2);
      rectify_line(pr.F, pr.delta, v, 1, b0, b1, b2);
      for (int i = t; i < n; i += kThreads) {
        if (rectify_sample(a0, a1, a2, pr.delta, i, pr.wid, pr.hgt) >= 0 ||
            rectify_sample(b0, b1, b2, pr.delta, i, pr.wid, pr.hgt) >= 0) {
          rlo = min(rlo, r);
          rhi = max(rhi, r);
          clo = min(clo, i);
          chi = max(chi, i);
        }
      }
    }
    rlo = wave_min(rlo);
    rhi = wave_max(rhi);
    clo = wave_min(clo);
    chi = wave_max(chi);
    if ((t & 63) == 0) {
      s_part[t >> 6][0] = rlo;
      s_part[t >> 6][1] = rhi;
      s_part[t >> 6][2] = clo;
      s_part[t >> 6][3] = chi;
    }
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < kThreads / 64; ++w) {
        rlo = min(rlo, s_part[w][0]);
        rhi = max(rhi, s_part[w][1]);
        clo = min(clo, s_part[w][2]);
        chi = max(chi, s_part[w][3]);
      }
      if (rhi >= 0) {
        int32_t *a = acc + (size_t)it.pair * 4;
        atomicMin(a + 0, rlo);
        atomicMax(a + 1, rhi);
        atomicMin(a + 2, clo);
        atomicMax(a + 3, chi);
      }
    }
    __syncthreads();  // the parts have been read before the next item writes them
  }
}

__global__ __launch_bounds__(kThreads) void rectify_batch_box_kernel(const int32_t *__restrict__ acc, int npairs,
                                                                     int32_t *__restrict__ box) {
  const int p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= npairs) return;
  const int32_t *a = acc + (size_t)p * 4;
  const bool any = a[1] >= 0;
  box[(size_t)p * 4 + 0] = any ? a[0] : 0;
  box[(size_t)p * 4 + 1] = any ? a[1] + 1 : 0;
  box[(size_t)p * 4 + 2] = any ? a[2] : 0;
  box[(size_t)p * 4 + 3] = any ? a[3] + 1 : 0;
}

// T: uint64_t for float64 images (bit copies), uint32_t for float32 ones, uint8_t for 8-bit ones.
template <typename T>
__global__ __launch_bounds__(kThreads) void rectify_batch_kernel(const RectifyBatchPair *__restrict__ pairs,
                                                                const RectifyBatchItem *__restrict__ items,
                                                                long long nitems, int nchan, const T *__restrict__ images,
                                                                T *__restrict__ r0, T *__restrict__ r1,
                                                                int *__restrict__ ri0, int *__restrict__ ri1) {
  for (long long b = blockIdx.x; b < nitems; b += gridDim.x) {  // workgroup-uniform
    const RectifyBatchItem it = items[b];
    const RectifyBatchPair pr = pairs[it.pair];
    const T *im = images + (size_t)(it.img ? pr.im1 : pr.im0) * nchan;
    T *out = it.img ? r1 : r0;
    int *outi = it.img ? ri1 : ri0;
    const int wcols = pr.col_hi - pr.col_lo;
    for (int r = it.row0; r < it.row0 + it.rows; ++r) {
      double L0, L1, L2;
      rectify_line(pr.F, pr.delta, (double)(r - pr.extra), it.img, L0, L1, L2);
      const size_t row_base = (size_t)pr.out + (size_t)(r - pr.row_lo) * wcols;
      for (int c = pr.col_lo + (int)threadIdx.x; c < pr.col_hi; c += kThreads) {
        const int idx = c < pr.rnx ? rectify_sample(L0, L1, L2, pr.delta, c, pr.wid, pr.hgt) : -1;
        const size_t o = row_base + (size_t)(c - pr.col_lo);
        outi[o] = idx;
        if (idx >= 0) {
          const T *src = im + (size_t)idx * nchan;
          for (int ch = 0; ch < nchan; ++ch) out[o * nchan + ch] = src[ch];
        } else {
          for (int ch = 0; ch < nchan; ++ch) out[o * nchan + ch] = T(0);
        }
      }
    }
  }
}

bool all_nan_or_zero(const double *F) {
  bool nan = true, zero = true;
  for (int j = 0; j < 9; ++j) {
    nan = nan && std::isnan(F[j]);
    zero = zero && F[j] == 0.;
  }
  return nan || zero;
}

// The device table of a call's pairs (zero where a pair is not used, whose cameras are not read).
void fill_pairs(const RectifyBatchPlan &pl, const int32_t *sizes, const int32_t *pairs, int npairs, const double *P0s,
                const double *P1s, const int32_t *use, RectifyBatchPair *tab) {
  const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // Camera(): Identity(3,4), src/Camera.h:27
  for (int p = 0; p < npairs; ++p) {
    RectifyBatchPair &pr = tab[p];
    memset(&pr, 0, sizeof(pr));
    if (use && !use[p]) continue;
    const int i0 = pairs[2 * p], i1 = pairs[2 * p + 1];
    rectify_fundamental(P0s ? P0s + (size_t)p * 12 : eye, P1s + (size_t)p * 12, pr.F);
    pr.wid = sizes[2 * i0];
    pr.hgt = sizes[2 * i0 + 1];
    const int32_t *fr = &pl.frame[(size_t)p * 3], *bx = &pl.box[(size_t)p * 4];
    pr.cols = fr[1];
    pr.rnx = fr[2];
    pr.extra = (fr[0] - pr.hgt) / 2;
    pr.delta = ((double)(pr.wid - 1) - 0.) / (double)(pr.rnx - 1);
    pr.im0 = pl.img_off[i0];
    pr.im1 = pl.img_off[i1];
    pr.out = pl.out_off[p];
    pr.row_lo = bx[0];
    pr.col_lo = bx[2];
    pr.col_hi = bx[3];
  }
}

// table | items into one cached buffer, one upload; the buffer goes back to the cache behind the call's last kernel
struct Tables {
  DevBuf ws;
  hipStream_t st;
  const RectifyBatchPair *pairs = nullptr;
  const RectifyBatchItem *items = nullptr;
  int32_t *acc = nullptr;  // bounds only: [npairs, 4] behind the items
  explicit Tables(hipStream_t s) : st(s) {}
  ~Tables() { ws.release_after(st); }
  int upload(const std::vector<RectifyBatchPair> &tab, const std::vector<RectifyBatchItem> &its, bool with_acc) {
    const size_t tb = tab.size() * sizeof(RectifyBatchPair), ib = its.size() * sizeof(RectifyBatchItem);
    const size_t ab = with_acc ? tab.size() * 4 * sizeof(int32_t) : 0;
    std::vector<unsigned char> host(tb + ib + ab);
    memcpy(host.data(), tab.data(), tb);
    memcpy(host.data() + tb, its.data(), ib);
    int32_t *a = reinterpret_cast<int32_t *>(host.data() + tb + ib);
    for (size_t p = 0; p < (with_acc ? tab.size() : 0); ++p) {
      a[4 * p + 0] = a[4 * p + 2] = INT_MAX;
      a[4 * p + 1] = a[4 * p + 3] = -1;
    }
    SPV_TRY(ws.alloc(host.size()));
    // (pageable source: the copy has left `host` when the call returns)
    SPV_HIP_CHECK(hipMemcpyAsync(ws.p, host.data(), host.size(), hipMemcpyHostToDevice, st));
    unsigned char *base = ws.as<unsigned char>();
    pairs = reinterpret_cast<const RectifyBatchPair *>(base);
    items = reinterpret_cast<const RectifyBatchItem *>(base + tb);
    acc = reinterpret_cast<int32_t *>(base + tb + ib);
    return SPV_OK;
  }
};

// at most 32 workgroups per compute unit, each walking its items
unsigned capped_grid(size_t nitems) {
  return (unsigned)std::min<size_t>(nitems, (size_t)std::max(device_cu_count(), 1) * kRectifyBatchGroupsPerCu);
}

}  // namespace

int rectify_batch_plan(const int32_t *sizes, int nimg, int nchan, double sf, const int32_t *pairs, int npairs,
                       const int32_t *use, const int32_t *box, RectifyBatchPlan *out) {
  if (nimg < 0 || npairs < 0) return set_error(SPV_ERR_INVALID, "negative count (nimg=%d, npairs=%d)", nimg, npairs);
  if ((nimg > 0 && !sizes) || (npairs > 0 && !pairs)) return set_error(SPV_ERR_INVALID, "null sizes or pairs");
  if (npairs > kRectifyBatchMaxPairs) return set_error(SPV_ERR_INVALID, "more than 2^20 pairs per call");
  if (!(std::isfinite(sf) && sf > 0.) || nchan < 1)  // (also where there is no image for rectify_shape to refuse)
    return set_error(SPV_ERR_INVALID, "bad sampling_factor %g or nchan %d", sf, nchan);
  RectifyBatchPlan pl;
  pl.img_off.assign((size_t)nimg + 1, 0);
  std::vector<int32_t> shapes((size_t)nimg * 3);
  for (int k = 0; k < nimg; ++k) {
    SPV_TRY(rectify_shape(sizes[2 * k], sizes[2 * k + 1], nchan, sf, &shapes[(size_t)k * 3]));
    pl.img_off[(size_t)k + 1] = pl.img_off[k] + (long long)sizes[2 * k] * sizes[2 * k + 1];
  }
  pl.frame.assign((size_t)npairs * 3, 0);
  pl.box.assign((size_t)npairs * 4, 0);
  pl.out_off.assign((size_t)npairs + 1, 0);
  for (int p = 0; p < npairs; ++p) {
    const int i0 = pairs[2 * p], i1 = pairs[2 * p + 1];
    if (i0 < 0 || i0 >= nimg || i1 < 0 || i1 >= nimg)
      return set_error(SPV_ERR_INVALID, "pair %d names images %d and %d of %d", p, i0, i1, nimg);
    if (sizes[2 * i0] != sizes[2 * i1] || sizes[2 * i0 + 1] != sizes[2 * i1 + 1])
      return set_error(SPV_ERR_INVALID, "pair %d: images %d and %d differ in size", p, i0, i1);
    pl.out_off[(size_t)p + 1] = pl.out_off[p];
    if (use && !use[p]) continue;
    ++pl.used;
    int32_t *fr = &pl.frame[(size_t)p * 3], *bx = &pl.box[(size_t)p * 4];
    memcpy(fr, &shapes[(size_t)i0 * 3], 3 * sizeof(int32_t));
    if (box) {
      memcpy(bx, box + (size_t)p * 4, 4 * sizeof(int32_t));
      if (bx[0] < 0 || bx[0] > bx[1] || bx[1] > fr[0] || bx[2] < 0 || bx[2] > bx[3] || bx[3] > fr[1])
        return set_error(SPV_ERR_INVALID, "pair %d: box (%d, %d, %d, %d) outside its frame of %d x %d", p, bx[0], bx[1],
                         bx[2], bx[3], fr[0], fr[1]);
    } else {
      bx[1] = fr[0];
      bx[3] = fr[1];
    }
    const long long wrows = bx[1] - bx[0], wcols = bx[3] - bx[2];
    pl.out_off[(size_t)p + 1] += wrows * wcols;
    if (wcols == 0) continue;
    for (int img = 0; img < 2; ++img)
      for (long long r = bx[0]; r < bx[1]; r += kRectifyBatchRows)
        pl.items.push_back(RectifyBatchItem{p, img, (int32_t)r, (int32_t)std::min<long long>(kRectifyBatchRows, bx[1] - r)});
  }
  *out = std::move(pl);
  return SPV_OK;
}

int rectify_batch_bounds_run(const int32_t *sizes, int nimg, int nchan, double sf, const int32_t *pairs, int npairs,
                             const double *P0s, const double *P1s, const int32_t *use, int32_t *d_box,
                             hipStream_t stream) {
  RectifyBatchPlan pl;
  SPV_TRY(rectify_batch_plan(sizes, nimg, nchan, sf, pairs, npairs, use, nullptr, &pl));
  if (npairs == 0) return SPV_OK;
  if (!d_box || (reinterpret_cast<uintptr_t>(d_box) & 3)) return set_error(SPV_ERR_INVALID, "null or misaligned d_box");
  if (pl.used > 0 && !P1s) return set_error(SPV_ERR_INVALID, "null camera pointer");
  std::vector<RectifyBatchPair> tab((size_t)npairs);
  fill_pairs(pl, sizes, pairs, npairs, P0s, P1s, use, tab.data());
  std::vector<RectifyBatchItem> its;  // (pair, -, first frame row, rows): both images of those rows
  for (int p = 0; p < npairs; ++p) {
    if ((use && !use[p]) || tab[p].rnx == 1 || all_nan_or_zero(tab[p].F)) continue;
    const int rows = pl.frame[(size_t)p * 3];
    for (int r = 0; r < rows; r += kBoundsRows) its.push_back(RectifyBatchItem{p, 0, r, std::min(kBoundsRows, rows - r)});
  }
  if (its.empty()) {
    SPV_HIP_CHECK(hipMemsetAsync(d_box, 0, (size_t)npairs * 4 * sizeof(int32_t), stream));
    return SPV_OK;
  }
  Tables tb(stream);
  SPV_TRY(tb.upload(tab, its, true));
  {
    ProfScope prof("rectify_batch_bounds", stream);
    hipLaunchKernelGGL(rectify_batch_bounds_kernel, dim3(capped_grid(its.size())), dim3(kThreads), 0, stream, tb.pairs,
                       tb.items, (long long)its.size(), tb.acc);
    SPV_HIP_CHECK(hipGetLastError());
  }
  ProfScope prof("rectify_batch_box", stream);
  hipLaunchKernelGGL(rectify_batch_box_kernel, dim3((npairs + kThreads - 1) / kThreads), dim3(kThreads), 0, stream,
                     tb.acc, npairs, d_box);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

int rectify_batch_run(const void *d_images, int dtype, const int32_t *sizes, int nimg, int nchan, double sf,
                      const int32_t *pairs, int npairs, const double *P0s, const double *P1s, const int32_t *use,
                      const int32_t *box, void *d_r0, void *d_r1, int32_t *d_ri0, int32_t *d_ri1, hipStream_t stream) {
  if (dtype != SPV_RECTIFY_F64 && dtype != SPV_RECTIFY_U8 && dtype != SPV_RECTIFY_F32)
    return set_error(SPV_ERR_INVALID, "dtype %d", dtype);
  RectifyBatchPlan pl;
  SPV_TRY(rectify_batch_plan(sizes, nimg, nchan, sf, pairs, npairs, use, box, &pl));
  if (pl.used > 0 && !P1s) return set_error(SPV_ERR_INVALID, "null camera pointer");
  if (pl.items.empty()) return SPV_OK;  // no window holds a sample: nothing to write
  if (!d_images || !d_r0 || !d_r1 || !d_ri0 || !d_ri1) return set_error(SPV_ERR_INVALID, "null device pointer");
  const uintptr_t align = dtype == SPV_RECTIFY_F64 ? 7 : dtype == SPV_RECTIFY_F32 ? 3 : 0;
  if (((reinterpret_cast<uintptr_t>(d_images) | reinterpret_cast<uintptr_t>(d_r0) | reinterpret_cast<uintptr_t>(d_r1)) & align) ||
      ((reinterpret_cast<uintptr_t>(d_ri0) | reinterpret_cast<uintptr_t>(d_ri1)) & 3))
    return set_error(SPV_ERR_INVALID, "misaligned image or output pointer");
  std::vector<RectifyBatchPair> tab((size_t)npairs);
  fill_pairs(pl, sizes, pairs, npairs, P0s, P1s, use, tab.data());
  Tables tb(stream);
  SPV_TRY(tb.upload(tab, pl.items, false));
  const dim3 grid(capped_grid(pl.items.size()));
  const long long nitems = (long long)pl.items.size();
  ProfScope prof("rectify_batch", stream);
  if (dtype == SPV_RECTIFY_F64)
    hipLaunchKernelGGL((rectify_batch_kernel<uint64_t>), grid, dim3(kThreads), 0, stream, tb.pairs, tb.items, nitems,
                       nchan, static_cast<const uint64_t *>(d_images), static_cast<uint64_t *>(d_r0),
                       static_cast<uint64_t *>(d_r1), d_ri0, d_ri1);
  else if (dtype == SPV_RECTIFY_F32)
    hipLaunchKernelGGL((rectify_batch_kernel<uint32_t>), grid, dim3(kThreads), 0, stream, tb.pairs, tb.items, nitems,
                       nchan, static_cast<const uint32_t *>(d_images), static_cast<uint32_t *>(d_r0),
                       static_cast<uint32_t *>(d_r1), d_ri0, d_ri1);
  else
    hipLaunchKernelGGL((rectify_batch_kernel<uint8_t>), grid, dim3(kThreads), 0, stream, tb.pairs, tb.items, nitems,
                       nchan, static_cast<const uint8_t *>(d_images), static_cast<uint8_t *>(d_r0),
                       static_cast<uint8_t *>(d_r1), d_ri0, d_ri1);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

}  // namespace spv
