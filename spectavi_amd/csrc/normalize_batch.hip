// normalize_batch.hip -- normalize_to_ubyte_and_multiple_16_dim of many tables in one chain of launches (gfx950).
//
// adapter.hip normalises one table per call with kernels shaped for a million rows: one workgroup per 16 columns
// walks the column sums in row order, because float addition is not associative and numpy's bits are the contract.
// A view set -- tens of tables of a few thousand rows -- leaves the device almost empty that way, once per table.
// Here the tables of a collection (rows [seg_off[s], seg_off[s + 1]) of one array) take a fixed number of launches:
//
//   work items (normalize_batch_plan, host)  every set's rows in blocks of 256, in order; an item never straddles
//                                            two sets.  One upload brings the items and two per-set tables.
//   normalize_batch_stats_kernel  (uint8)    one workgroup per item, walking b, b + gridDim.x, ...: per column the
//                                            integer sum, minimum and maximum of the item's rows, one packed word
//                                            (sum << 16 | max << 8 | min; 255 * 256 rows fit 16 bits).
//   normalize_batch_finish_kernel            one workgroup per (set, 16-column block).  uint8: the items' words of
//                                            the set are combined in integers; where every column sum of the block
//                                            is at most 2^24, mean = float(S) / float(rows) and the workgroup is
//                                            done.  Otherwise, and for every float32 set, it is
//                                            column_stats_block (normalize_device.h), the walk of adapter.hip.
//   normalize_batch_kernel                   one workgroup per item: normalize_value with the (mean, norm) of the
//                                            item's set, a lane keeping its columns over the item's rows.
//
// Why the integer sum is numpy's float32 sum: the addends are integers >= 0, so every prefix of the row-ordered
// chain is an integer at most S; while S <= 2^24 each is representable, each add is exact and the chain ends at S.
// 255 * 65793 = 2^24 - 1: no uint8 table of up to 65793 rows is ever walked.  Minimum and maximum are exact in any
// order.  A float32 table gets its minimum and maximum from the walk's loaders, which see every element anyway, so
// it has no statistics launch.
#include "common.h"
#include "normalize_device.h"

#include <type_traits>

namespace spv {
namespace {

constexpr int kThreads = 256;
constexpr int kItemRows = kNormalizeBatchItemRows;
static_assert(255 * kItemRows < (1 << 16), "an item's column sum travels in 16 bits");
static_assert(sizeof(NormalizeBatchItem) == 12, "items travel as int32[3]");

// The device form of a call's tables, one upload.
struct NormalizeBatchTables {
  const NormalizeBatchItem *items;
  const uint32_t *seg;     // [nseg + 1]: the first row of every set
  const int32_t *item0;    // [nseg + 1]: the first item at or after every set; [nseg] = nitems
  int nitems;
};

// How a 256-lane workgroup lays itself over rows of `groups` column groups: w groups side by side, nrl row lanes;
// lane t is (group t % w of a pass, row lane t / w) and idle where t / w >= nrl.
struct LaneGrid {
  int w, nrl, gl, rl;
  __device__ LaneGrid(int groups) : w(min(groups, kThreads)), nrl(kThreads / w), gl(threadIdx.x % w), rl(threadIdx.x / w) {}
};

// VEC = 16: dim % 16 == 0 and x 16-byte aligned, one 16-byte load per lane and row; VEC = 1: any dim.
template <int VEC>
__global__ __launch_bounds__(kThreads) void normalize_batch_stats_kernel(NormalizeBatchTables tb,
                                                                         const uint8_t *__restrict__ x, int dim,
                                                                         uint32_t *__restrict__ part) {
  __shared__ uint32_t s_part[kThreads * VEC];  // [row lane][column of the pass]
  const int t = threadIdx.x;
  const int groups = dim / VEC;
  const LaneGrid lg(groups);
  const int pass_cols = lg.w * VEC;
  for (int b = blockIdx.x; b < tb.nitems; b += gridDim.x) {  // workgroup-uniform
    const NormalizeBatchItem it = tb.items[b];
    const uint8_t *src = x + ((size_t)tb.seg[it.set] + it.row0) * dim;
    for (int g0 = 0; g0 < groups; g0 += lg.w) {  // (one pass unless VEC == 1 and dim > 256)
      const int g = g0 + lg.gl;
      const bool live = lg.rl < lg.nrl && g < groups;
      uint32_t sum[VEC], mx[VEC], mn[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) sum[k] = 0, mx[k] = 0, mn[k] = 255;
      if (live) {
#pragma unroll 4
        for (int r = lg.rl; r < it.rows; r += lg.nrl) {
          const uint8_t *p = src + (size_t)r * dim + g * VEC;
          uint32_t q[(VEC + 3) / 4];
          if constexpr (VEC == 16) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p);
            q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
          } else {
            q[0] = *p;
          }
#pragma unroll
          for (int k = 0; k < VEC; ++k) {
            const uint32_t v = (q[k >> 2] >> (8 * (k & 3))) & 255u;
            sum[k] += v;
            mx[k] = max(mx[k], v);
            mn[k] = min(mn[k], v);
          }
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k)
          s_part[lg.rl * pass_cols + lg.gl * VEC + k] = sum[k] << 16 | mx[k] << 8 | mn[k];
      }
      __syncthreads();
      // the row lanes' words of a column, combined; a row lane without a row holds (0, 0, 255)
      const int ncols = min(lg.w, groups - g0) * VEC;
      for (int j = t; j < ncols; j += kThreads) {
        uint32_t s = 0, hi = 0, lo = 255;
        for (int rr = 0; rr < lg.nrl; ++rr) {
          const uint32_t wd = s_part[rr * pass_cols + j];
          s += wd >> 16;
          hi = max(hi, (wd >> 8) & 255u);
          lo = min(lo, wd & 255u);
        }
        part[(size_t)b * dim + g0 * VEC + j] = s << 16 | hi << 8 | lo;
      }
      __syncthreads();  // the words have been read before the next pass or item writes them
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kStatThreads) void normalize_batch_finish_kernel(NormalizeBatchTables tb,
                                                                              const T *__restrict__ x, int dim, int nblk,
                                                                              const uint32_t *__restrict__ part,
                                                                              float *__restrict__ stats) {
  const int set = blockIdx.x / nblk, cb = blockIdx.x % nblk;
  const uint32_t r0 = tb.seg[set];
  const int rows = (int)(tb.seg[set + 1] - r0);
  if (rows == 0) return;
  float *mean = stats + (size_t)set * 2 * dim, *norm = mean + dim;
  if constexpr (std::is_same<T, uint8_t>::value) {
    // lanes 0..255 as (column, one of 16 item lanes) over the set's items, then lanes 0..15 over the item lanes
    const int t = threadIdx.x;
    const int c0 = cb * kStatCols, ncol = min(kStatCols, dim - c0);
    __shared__ unsigned long long s_sum[256];
    __shared__ uint32_t s_mm[256];
    if (t < 256) {
      const int col = t & 15;
      unsigned long long S = 0;
      uint32_t hi = 0, lo = 255;
      if (col < ncol)
        for (int i = tb.item0[set] + (t >> 4); i < tb.item0[set + 1]; i += 16) {
          const uint32_t wd = part[(size_t)i * dim + c0 + col];
          S += wd >> 16;
          hi = max(hi, (wd >> 8) & 255u);
          lo = min(lo, wd & 255u);
        }
      s_sum[t] = S;
      s_mm[t] = hi << 8 | lo;
    }
    __syncthreads();
    unsigned long long S = 0;
    uint32_t hi = 0, lo = 255;
    if (t < ncol)
      for (int k = 0; k < 16; ++k) {
        S += s_sum[16 * k + t];
        hi = max(hi, s_mm[16 * k + t] >> 8);
        lo = min(lo, s_mm[16 * k + t] & 255u);
      }
    if (!__syncthreads_or(t < ncol && S > (1ull << 24))) {
      if (t < ncol) {
        const float m = (float)(uint32_t)S / (float)rows;
        mean[c0 + t] = m;
        norm[c0 + t] = fmaxf((float)hi - m, -((float)lo - m));
      }
      return;
    }
  }
  column_stats_block<T>(x + (size_t)r0 * dim, rows, dim, cb, mean);
}

// VEC = 4: dim % 4 == 0, x aligned to four elements, out_f32 to 16 bytes and out_u8 to 4: one load and one store
// per output, four columns wide, which are four columns of the table or four of the padding; VEC = 1: anything.
template <typename T, int VEC>
__global__ __launch_bounds__(kThreads) void normalize_batch_kernel(NormalizeBatchTables tb, const T *__restrict__ x,
                                                                   int dim, int dim16, const float *__restrict__ stats,
                                                                   float *__restrict__ out_f32,
                                                                   uint8_t *__restrict__ out_u8) {
  const int groups = dim16 / VEC;
  const LaneGrid lg(groups);
  if (lg.rl >= lg.nrl) return;  // (no barrier in this kernel)
  for (int b = blockIdx.x; b < tb.nitems; b += gridDim.x) {
    const NormalizeBatchItem it = tb.items[b];
    const size_t row0 = (size_t)tb.seg[it.set] + it.row0;
    const float *mean = stats + (size_t)it.set * 2 * dim, *norm = mean + dim;
    for (int g = lg.gl; g < groups; g += lg.w) {  // (one pass unless dim16 / VEC > 256)
      const int c = g * VEC;
      const bool live = c < dim;
      float m[VEC], n[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        m[k] = live ? mean[c + k] : 0.f;
        n[k] = live ? norm[c + k] : 1.f;
      }
#pragma unroll 4
      for (int r = lg.rl; r < it.rows; r += lg.nrl) {
        const size_t row = row0 + r;
        float v[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = 0.f;
        if (live) {
          const T *p = x + row * dim + c;
          float xv[VEC];
          if constexpr (VEC == 1) {
            xv[0] = (float)*p;
          } else if constexpr (std::is_same<T, float>::value) {
            const float4 q = *reinterpret_cast<const float4 *>(p);
            xv[0] = q.x, xv[1] = q.y, xv[2] = q.z, xv[3] = q.w;
          } else {
            const uint32_t q = *reinterpret_cast<const uint32_t *>(p);
#pragma unroll
            for (int k = 0; k < 4; ++k) xv[k] = (float)((q >> (8 * k)) & 255u);
          }
#pragma unroll
          for (int k = 0; k < VEC; ++k) v[k] = normalize_value(xv[k], m[k], n[k]);
        }
        const size_t e = row * dim16 + c;
        if constexpr (VEC == 1) {
          if (out_f32) out_f32[e] = v[0];
          if (out_u8) out_u8[e] = normalize_ubyte(v[0]);
        } else {
          if (out_f32) *reinterpret_cast<float4 *>(out_f32 + e) = make_float4(v[0], v[1], v[2], v[3]);
          if (out_u8)
            *reinterpret_cast<uint32_t *>(out_u8 + e) = (uint32_t)normalize_ubyte(v[0]) | (uint32_t)normalize_ubyte(v[1]) << 8 |
                                                        (uint32_t)normalize_ubyte(v[2]) << 16 | (uint32_t)normalize_ubyte(v[3]) << 24;
        }
      }
    }
  }
}

// The workspace, stated once: the size query walks it from a null base.
size_t batch_layout(int nseg, size_t nitems, int dim, int dtype, NormalizeBatchPlan *p) {
  WsWalk w;
  p->off_items = w.reserve(nitems * sizeof(NormalizeBatchItem));
  p->off_seg = w.reserve(((size_t)nseg + 1) * sizeof(uint32_t));
  p->off_item0 = w.reserve(((size_t)nseg + 1) * sizeof(int32_t));
  p->off_stats = w.reserve((size_t)nseg * 2 * dim * sizeof(float));
  p->off_part = w.reserve(dtype == SPV_NORMALIZE_U8 ? nitems * dim * sizeof(uint32_t) : 0);
  return w.end();
}

template <typename T>
void launch_apply(bool vec, dim3 grid, hipStream_t stream, const NormalizeBatchTables &tb, const void *d_x, int dim,
                  int dim16, const float *stats, float *d_out_f32, uint8_t *d_out_u8) {
  if (vec)
    hipLaunchKernelGGL((normalize_batch_kernel<T, 4>), grid, dim3(kThreads), 0, stream, tb, static_cast<const T *>(d_x), dim,
                       dim16, stats, d_out_f32, d_out_u8);
  else
    hipLaunchKernelGGL((normalize_batch_kernel<T, 1>), grid, dim3(kThreads), 0, stream, tb, static_cast<const T *>(d_x), dim,
                       dim16, stats, d_out_f32, d_out_u8);
}

}  // namespace

int normalize_batch_plan(const long long *seg_off, int nseg, int dim, int dtype, NormalizeBatchPlan *out) {
  if (nseg < 0) return set_error(SPV_ERR_INVALID, "negative set count (nseg=%d)", nseg);
  if (dim < 1 || dim > kNormalizeBatchMaxDim)
    return set_error(SPV_ERR_INVALID, "dim=%d, must be in [1, %d]", dim, kNormalizeBatchMaxDim);
  if (dtype != SPV_NORMALIZE_F32 && dtype != SPV_NORMALIZE_U8) return set_error(SPV_ERR_INVALID, "unknown dtype %d", dtype);
  // the finish kernel's grid is (sets, 16-column blocks) in one dimension; empty sets count, their workgroups leave at once
  if ((size_t)nseg * ((dim + kStatCols - 1) / kStatCols) > 0x7FFFFFFFull)
    return set_error(SPV_ERR_INVALID, "%d sets of %d columns, more than a grid takes", nseg, dim);
  SPV_TRY(check_offsets(seg_off, nseg, "seg_off"));
  NormalizeBatchPlan p;
  p.total_rows = seg_off[nseg];
  for (int s = 0; s < nseg; ++s) {
    const long long rows = seg_off[s + 1] - seg_off[s];
    // numpy sums a single contiguous column pairwise: normalize_run's refusal
    if (dim == 1 && rows > 1)
      return set_error(SPV_ERR_INVALID, "normalisation of a single-column table is not supported (dim=1, set %d)", s);
    p.sets += rows > 0;    for (long long r = 0; r < rows; r += kItemRows)
      p.items.push_back({s, (int32_t)r, (int32_t)std::min<long long>(kItemRows, rows - r)});
  }
  p.total_bytes = batch_layout(nseg, p.items.size(), dim, dtype, &p);
  *out = std::move(p);
  return SPV_OK;
}

int normalize_batch_run(const void *d_x, int dtype, const long long *seg_off, int nseg, int dim, float *d_out_f32,
                        uint8_t *d_out_u8, void *d_ws, size_t ws_bytes, hipStream_t stream) {
  NormalizeBatchPlan p;
  SPV_TRY(normalize_batch_plan(seg_off, nseg, dim, dtype, &p));
  if (!d_out_f32 && !d_out_u8) return set_error(SPV_ERR_INVALID, "neither the float32 nor the uint8 table is wanted");
  const size_t esize = dtype == SPV_NORMALIZE_U8 ? 1 : sizeof(float);
  if ((reinterpret_cast<uintptr_t>(d_x) & (esize - 1)) || (reinterpret_cast<uintptr_t>(d_out_f32) & 3))
    return set_error(SPV_ERR_INVALID, "device pointers must be aligned to their element size");
  if (p.total_rows == 0) return SPV_OK;
  if (!d_x || !d_ws) return set_error(SPV_ERR_INVALID, "null device pointer");
  if (reinterpret_cast<uintptr_t>(d_ws) & 15) return set_error(SPV_ERR_INVALID, "the workspace must be 16-byte aligned");
  if (ws_bytes < p.total_bytes) return set_error(SPV_ERR_INVALID, "workspace too small: %zu < %zu", ws_bytes, p.total_bytes);

  // the call's tables, one upload: items | seg | item0 (adjacent pieces of the layout)
  const size_t nitems = p.items.size(), table_bytes = p.off_item0 + ((size_t)nseg + 1) * sizeof(int32_t);
  std::vector<unsigned char> host(table_bytes, 0);
  std::copy(p.items.begin(), p.items.end(), reinterpret_cast<NormalizeBatchItem *>(host.data() + p.off_items));
  uint32_t *h_seg = reinterpret_cast<uint32_t *>(host.data() + p.off_seg);
  int32_t *h_item0 = reinterpret_cast<int32_t *>(host.data() + p.off_item0);
  for (int s = 0; s <= nseg; ++s) h_seg[s] = (uint32_t)seg_off[s];
  for (size_t i = 0, s = 0; s <= (size_t)nseg; ++s) {
    while (i < nitems && (size_t)p.items[i].set < s) ++i;
    h_item0[s] = (int32_t)i;
  }
  unsigned char *ws = static_cast<unsigned char *>(d_ws);
  // the one wait of the call: `host` is gone when it returns, so its upload must have ended
  SPV_HIP_CHECK(hipMemcpyWithStream(ws, host.data(), table_bytes, hipMemcpyHostToDevice, stream));
  const NormalizeBatchTables tb{reinterpret_cast<const NormalizeBatchItem *>(ws + p.off_items),
                                reinterpret_cast<const uint32_t *>(ws + p.off_seg),
                                reinterpret_cast<const int32_t *>(ws + p.off_item0), (int)nitems};
  float *stats = reinterpret_cast<float *>(ws + p.off_stats);
  uint32_t *part = reinterpret_cast<uint32_t *>(ws + p.off_part);
  const int dim16 = (dim + 15) / 16 * 16, nblk = (dim + kStatCols - 1) / kStatCols;
  const uintptr_t xa = reinterpret_cast<uintptr_t>(d_x);
  // at most 32 workgroups per compute unit, each walking its items
  const dim3 grid((unsigned)std::min<size_t>(nitems, (size_t)std::max(device_cu_count(), 1) * kNormalizeBatchGroupsPerCu));
  const dim3 fgrid((unsigned)nseg * (unsigned)nblk);
  if (dtype == SPV_NORMALIZE_U8) {
    const uint8_t *x = static_cast<const uint8_t *>(d_x);
    {
      ProfScope prof("normalize_batch_stats", stream);
      if (dim % 16 == 0 && (xa & 15) == 0)
        hipLaunchKernelGGL(normalize_batch_stats_kernel<16>, grid, dim3(kThreads), 0, stream, tb, x, dim, part);
      else
        hipLaunchKernelGGL(normalize_batch_stats_kernel<1>, grid, dim3(kThreads), 0, stream, tb, x, dim, part);
      SPV_HIP_CHECK(hipGetLastError());
    }
    ProfScope prof("normalize_batch_finish", stream);
    hipLaunchKernelGGL(normalize_batch_finish_kernel<uint8_t>, fgrid, dim3(kStatThreads), 0, stream, tb, x, dim, nblk, part, stats);
    SPV_HIP_CHECK(hipGetLastError());
  } else {
    ProfScope prof("normalize_batch_finish", stream);
    hipLaunchKernelGGL(normalize_batch_finish_kernel<float>, fgrid, dim3(kStatThreads), 0, stream, tb,
                       static_cast<const float *>(d_x), dim, nblk, part, stats);
    SPV_HIP_CHECK(hipGetLastError());
  }
  const bool vec = dim % 4 == 0 && (xa & (4 * esize - 1)) == 0 && (reinterpret_cast<uintptr_t>(d_out_f32) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(d_out_u8) & 3) == 0;
  ProfScope prof("normalize_batch", stream);
  if (dtype == SPV_NORMALIZE_U8)
    launch_apply<uint8_t>(vec, grid, stream, tb, d_x, dim, dim16, stats, d_out_f32, d_out_u8);
  else
    launch_apply<float>(vec, grid, stream, tb, d_x, dim, dim16, stats, d_out_f32, d_out_u8);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

}  // namespace spv
