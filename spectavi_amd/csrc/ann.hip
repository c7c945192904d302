// ann.hip -- approximate L2 k-nearest-neighbour on float32 rows for gfx950 (MI355X): a coarse score
// of every pair on the bf16 matrix cores, the ncand best rows of every query kept, and an exact
// re-rank of those rows in nn_bruteforce's own p = 2 arithmetic.
//
// The contract is stated in include/spectavi_amd.h (ann_hnswlib / spv_ann_l2); in short
//
//   1. m_c = rintf(mean of column c of x); x' = bf16(x - m), y' = bf16(y - m)  (round to nearest even);
//   2. s(i,j) = n_j - 2 (y'_i . x'_j), n_j = sum x'_j^2: products on the bf16 MFMA, fp32 accumulation,
//      one fixed K order, so the bits of s(i,j) depend on the pair alone;
//   3. per query the ncand smallest keys (s, idx) -- s as its order-preserving integer image;
//   4. the exact sequential unfused fp32 distance of every candidate, then the k smallest (dist, idx).
//
// Kernels, in launch order ("ann_prep", "ann_coarse", "ann_merge", "ann_rerank" for spv_profile_read):
//
//   * prep: column sums of x in double over fixed chunks of kMeanChunk rows, one thread per column and
//     chunk, then one thread per column adds the chunks in order (no atomics: the mean is a function of
//     x alone); the bf16 images of both sides with the row width padded to a multiple of 32; n_j from
//     the rounded values, one thread per row in column order.
//   * coarse: grid = (blocks of 128 queries, database slices), 4 waves; a wave owns 32 queries and
//     every 128-row tile of the slice.  The x' tile goes through LDS (row stride 272 bytes: the 16-byte
//     fragment reads of consecutive lanes fall 4 banks apart), the y' fragments of a wave stay in
//     VGPRs for the whole slice when the padded width is <= 128 (one instantiation per width of 32, 64, 96
//     and 128; wider rows run 128 columns at a time and multiply the zero padding of the last chunk through).  The queries are the B operand, so
//     they lie on the C/D column side: a lane owns one query per sub-tile and keeps that query's
//     threshold and buffer fill in registers (replicated over the 2 or 4 lanes of a column).  The
//     epilogue is one fused multiply-add and one compare per score; a survivor is appended to the
//     query's buffer of this slice at a position taken from the ballot of the compare.  A buffer
//     that could overflow in the next sub-tile is first compacted by the whole wave to its ncand
//     smallest keys (rank by counting in LDS), which also tightens the threshold.  Rows arrive in
//     ascending index, so "s < threshold" alone is the lexicographic (s, idx) rule.
//   * merge: one wave per query folds the slices' buffers, in slice order, into the ncand smallest
//     keys.  Keys are unique and a slice's buffer always holds that slice's ncand smallest, so the
//     candidate set does not depend on the slice count.
//   * re-rank: one wave per query, candidates over the lanes, 16-byte row loads where the rows allow
//     them, d = x - y, t = d * d, s = s + t in column order (-ffp-contract=off), then the wave selects
//     the k smallest (dist bits, idx).
//
// Both bf16 MFMA shapes are built at the same per-wave tile (128 rows x 32 queries, 64 accumulator
// registers); AnnPlan::mfma names the one a launch uses (DESIGN.md has the measurement).

#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace spv {
namespace {

constexpr int kThreads = 256;
constexpr int kQT = 128;         // queries per workgroup (32 per wave)
constexpr int kRT = 128;         // database rows per tile
constexpr int kKC = 128;         // bf16 columns staged at a time
constexpr int kLdsStride = kKC + 8;  // in bf16: 272 bytes
constexpr int kMeanChunk = 1024; // rows per partial column sum
constexpr int kMaxDim = 2048;
constexpr int kMaxK = 64;
constexpr int kMaxCand = 256;
constexpr int kMaxBuf = 384;     // longest survivor buffer (ncand = 256)
constexpr int kRoom = 32;        // a sub-tile adds at most this many keys to one query
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kKeyNone = ~0ull;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- number formats -------------------------------------------------------------------------
__device__ __forceinline__ uint16_t to_bf16(float f) {  // round to nearest even; NaN stays NaN
  uint32_t u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
__device__ __forceinline__ float from_bf16(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
// the order-preserving integer image of a float and its inverse
__device__ __forceinline__ uint32_t ordered(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t o) {
  return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// ---- prep -----------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ann_colsum_kernel(const float *__restrict__ x, int M, int dim,
                                                              double *__restrict__ part) {
  const int c = blockIdx.y * kThreads + threadIdx.x;
  if (c >= dim) return;
  const long long r0 = (long long)blockIdx.x * kMeanChunk;
  const int r1 = (int)std::min<long long>(M, r0 + kMeanChunk);
  double s = 0.0;
  for (int r = (int)r0; r < r1; ++r) s = s + (double)x[(size_t)r * dim + c];
  part[(size_t)blockIdx.x * dim + c] = s;
}

__global__ __launch_bounds__(kThreads) void ann_mean_kernel(const double *__restrict__ part, int M, int dim,
                                                            int kpad, int chunks, float *__restrict__ mean) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= kpad) return;
  float m = 0.f;
  if (c < dim) {
    double s = 0.0;
    for (int p = 0; p < chunks; ++p) s = s + part[(size_t)p * dim + c];
    m = rintf((float)(s / (double)M));
    if (!(fabsf(m) <= 3.0e38f)) m = 0.f;  // NaN or inf: leave the column where it is
  }
  mean[c] = m;
}

// one thread per row and group of 8 columns: 16 bytes of the bf16 image
__global__ __launch_bounds__(kThreads) void ann_convert_kernel(const float *__restrict__ src, int rows, int dim,
                                                               int kpad, const float *__restrict__ mean,
                                                               uint16_t *__restrict__ dst) {
  const long long gt = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int groups = kpad >> 3;
  const long long row = gt / groups;
  const int g = (int)(gt - row * groups);
  if (row >= rows) return;
  uint32_t w[4];
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    uint32_t h[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int c = 8 * g + j + e;
      h[e] = c < dim ? to_bf16(src[(size_t)row * dim + c] - mean[c]) : 0u;
    }
    w[j >> 1] = h[0] | (h[1] << 16);
  }
  *reinterpret_cast<uint4 *>(dst + (size_t)row * kpad + 8 * g) = make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(kThreads) void ann_norm_kernel(const uint16_t *__restrict__ xb, int rows, int kpad,
                                                            float *__restrict__ norm) {
  const long long row = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (row >= rows) return;
  const uint4 *p = reinterpret_cast<const uint4 *>(xb + (size_t)row * kpad);
  float s = 0.f;
  for (int g = 0; g < (kpad >> 3); ++g) {
    const uint4 v = p[g];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = from_bf16((uint16_t)(w[j] & 0xFFFFu)), b = from_bf16((uint16_t)(w[j] >> 16));
      const float ta = a * a;
      s = s + ta;
      const float tb = b * b;
      s = s + tb;
    }
  }
  norm[row] = s;
}

// ---- wave-wide selection in LDS ---------------------------------------------------------------
// scr[0, n): keys, unique but for kKeyNone.  Afterwards scr[0, min(n, keep)) holds the smallest keys in
// ascending order (slots past the real keys are unspecified).  Rank by counting: every lane ranks the
// keys lane, lane + 64, ... against all n, which it reads as broadcasts.  n <= 64 PER.
template <int PER>
__device__ __forceinline__ void wave_select(uint64_t *scr, int n, int keep, int lane) {
  uint64_t my[PER];
  int rk[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int e = lane + 64 * i;
    my[i] = e < n ? scr[e] : kKeyNone;
    rk[i] = 0;
  }
#pragma unroll 8
  for (int j = 0; j < n; ++j) {  // unrolled: the broadcast reads of a batch are in flight together
    const uint64_t kj = scr[j];
#pragma unroll
    for (int i = 0; i < PER; ++i) rk[i] += kj < my[i] ? 1 : 0;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int i = 0; i < PER; ++i)
    if (lane + 64 * i < n && rk[i] < keep) scr[rk[i]] = my[i];
  __builtin_amdgcn_wave_barrier();
}

// ---- coarse score + survivors ------------------------------------------------------------------
// The two bf16 MFMA shapes at one per-wave tile of kRT rows x 32 queries.  W query columns per
// sub-tile, G lanes per column, NQ column blocks per wave, RS rows per sub-tile; accumulator
// register e of lane group grp is row 8 (e >> 2) + 4 grp + (e & 3) of its sub-tile in both shapes.
template <int SHAPE>
struct Mfma;
template <>
struct Mfma<32> {
  static constexpr int W = 32, G = 2, NQ = 1, RS = 32, REGS = 16, KSTEP = 16;
  using Acc = f32x16;
  static __device__ __forceinline__ Acc run(bf16x8 a, bf16x8 b, Acc c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <>
struct Mfma<16> {
  static constexpr int W = 16, G = 4, NQ = 2, RS = 16, REGS = 4, KSTEP = 32;
  using Acc = f32x4;
  static __device__ __forceinline__ Acc run(bf16x8 a, bf16x8 b, Acc c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};

// buf[(query * S + slice) * B + e], e < cnt[query * S + slice]: the slice's surviving keys
// (ordered(s) << 32 | row), among them its ncand smallest.
// KG > 0: the padded width is 32 KG <= kKC and the y' fragments are loaded once; KG = 0: any width, kKC
// columns at a time (the zero padding of the last chunk is multiplied through: exact).
template <int SHAPE, int KG>
__global__ __launch_bounds__(kThreads) void ann_coarse_kernel(const uint16_t *__restrict__ xb,
                                                              const uint16_t *__restrict__ yb,
                                                              const float *__restrict__ norm, int M, int N,
                                                              int kpad, int slice_rows, int S, int ncand, int B,
                                                              uint64_t *buf, int *__restrict__ cntg) {
  using MF = Mfma<SHAPE>;
  constexpr int W = MF::W, G = MF::G, NQ = MF::NQ, RS = MF::RS, REGS = MF::REGS, KSTEP = MF::KSTEP;
  constexpr bool HOIST = KG > 0;
  constexpr int NR = kRT / RS;                           // row sub-tiles
  constexpr int NKS = (HOIST ? 32 * KG : kKC) / KSTEP;   // k steps of a staged chunk
  constexpr int NG8 = (HOIST ? 32 * KG : kKC) / 8;       // 16-byte groups of a staged row
  __shared__ __attribute__((aligned(16))) uint16_t tile[kRT * kLdsStride];
  __shared__ __attribute__((aligned(16))) float ntile[kRT];
  __shared__ uint64_t scratch[kThreads / 64][kMaxBuf];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int col = lane & (W - 1), grp = lane / W;
  const int s = blockIdx.y;
  const long long row_begin = (long long)s * slice_rows;
  const int row_end = (int)std::min<long long>(M, row_begin + slice_rows);
  const int qbase = blockIdx.x * kQT + wave * 32;
  uint64_t *scr = scratch[wave];

  // per query column block: the query's threshold and buffer fill, the same in all G lanes of a column
  float thr[NQ];
  int cnt[NQ];
  const uint16_t *yrow[NQ];
  uint64_t *qbuf[NQ];  // the query's buffer of this slice
#pragma unroll
  for (int nq = 0; nq < NQ; ++nq) {
    const int q = qbase + nq * W + col;
    qbuf[nq] = buf + ((size_t)std::min(q, N - 1) * S + s) * B;
    thr[nq] = q < N ? INFINITY : -INFINITY;  // a lane past the last query keeps nothing
    cnt[nq] = 0;
    yrow[nq] = yb + (size_t)std::min(q, N - 1) * kpad;
  }

  bf16x8 bq[NQ][NKS];
  auto load_queries = [&](int k0) {
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq)
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks) {
        const int kk = k0 + ks * KSTEP + 8 * grp;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (kk < kpad) v = *reinterpret_cast<const uint4 *>(yrow[nq] + kk);
        bq[nq][ks] = __builtin_bit_cast(bf16x8, v);
      }
  };
  if constexpr (HOIST) load_queries(0);

  for (int row0 = (int)row_begin; row0 < row_end; row0 += kRT) {
    typename MF::Acc acc[NR][NQ];
#pragma unroll
    for (int m = 0; m < NR; ++m)
#pragma unroll
      for (int nq = 0; nq < NQ; ++nq)
#pragma unroll
        for (int e = 0; e < REGS; ++e) acc[m][nq][e] = 0.f;

    for (int k0 = 0; k0 < kpad; k0 += kKC) {
      __syncthreads();  // the tile before this one has been consumed
      for (int e = t; e < kRT * NG8; e += kThreads) {
        const int rr = e / NG8, g = e % NG8;
        const int row = row0 + rr, kk = k0 + 8 * g;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row < row_end && kk < kpad) v = *reinterpret_cast<const uint4 *>(xb + (size_t)row * kpad + kk);
        *reinterpret_cast<uint4 *>(&tile[rr * kLdsStride + 8 * g]) = v;
      }
      // rows past the slice: +inf is never below a threshold
      if (k0 == 0 && t < kRT) ntile[t] = row0 + t < row_end ? norm[row0 + t] : INFINITY;
      __syncthreads();
      if constexpr (!HOIST) load_queries(k0);
      // k steps outside, sub-tiles inside: consecutive MFMAs write different accumulators
#pragma unroll
      for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
        for (int m = 0; m < NR; ++m) {
          const uint4 v =
              *reinterpret_cast<const uint4 *>(&tile[(m * RS + col) * kLdsStride + ks * KSTEP + 8 * grp]);
          const bf16x8 a = __builtin_bit_cast(bf16x8, v);
#pragma unroll
          for (int nq = 0; nq < NQ; ++nq) acc[m][nq] = MF::run(a, bq[nq][ks], acc[m][nq]);
        }
    }

    // epilogue: one fused multiply-add per score (2 acc is exact, so it rounds once, as n - 2 acc
    // does), the minimum of four scores, one compare
#pragma unroll
    for (int m = 0; m < NR; ++m) {
      // a buffer that the next sub-tile could overflow is compacted first
#pragma unroll
      for (int nq = 0; nq < NQ; ++nq) {
        uint32_t full = (uint32_t)(__builtin_amdgcn_ballot_w64(cnt[nq] > B - kRoom) & ((1ull << W) - 1ull));
        while (full) {
          const int qq = __builtin_ctz(full);  // uniform
          full &= full - 1;
          const int n = __shfl(cnt[nq], qq, 64);
          uint64_t *qb = buf + ((size_t)(qbase + nq * W + qq) * S + s) * B;
          // this wave's own appends: a wider scope would write the whole L2 back on every compaction
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
          for (int e = lane; e < n; e += 64) scr[e] = qb[e];
          if (B <= 128) wave_select<2>(scr, n, ncand, lane);  // uniform
          else wave_select<kMaxBuf / 64>(scr, n, ncand, lane);
          for (int e = lane; e < ncand; e += 64) qb[e] = scr[e];
          const float nthr = unordered((uint32_t)(scr[ncand - 1] >> 32));
          if (col == qq) {
            cnt[nq] = ncand;
            thr[nq] = nthr;
          }
          __builtin_amdgcn_wave_barrier();
        }
      }
#pragma unroll
      for (int v = 0; v < REGS / 4; ++v) {
        const f32x4 nv = *reinterpret_cast<const f32x4 *>(&ntile[m * RS + 8 * v + 4 * grp]);
#pragma unroll
        for (int nq = 0; nq < NQ; ++nq) {
          float sc[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) sc[i] = __builtin_fmaf(-2.f, acc[m][nq][4 * v + i], nv[i]);
          // fminf passes a NaN over, and a NaN is never below a threshold
          const float best = fminf(fminf(sc[0], sc[1]), fminf(sc[2], sc[3]));
          if (__builtin_amdgcn_ballot_w64(best < thr[nq]) == 0ull) continue;  // nearly always, after the first tiles
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const bool pass = sc[i] < thr[nq];
            const uint64_t mask = __builtin_amdgcn_ballot_w64(pass);
            if (mask) {
              int before = 0, all = 0;
#pragma unroll
              for (int g = 0; g < G; ++g) {
                const int b = (int)((mask >> (col + W * g)) & 1ull);
                all += b;
                before += g < grp ? b : 0;
              }
              if (pass)
                qbuf[nq][cnt[nq] + before] =
                    ((uint64_t)ordered(sc[i]) << 32) | (uint32_t)(row0 + m * RS + 8 * v + 4 * grp + i);
              cnt[nq] += all;
            }
          }
        }
      }
    }
  }

  if (grp == 0) {
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq) {
      const int q = qbase + nq * W + col;
      if (q < N) cntg[(size_t)q * S + s] = cnt[nq];
    }
  }
}

// ---- merge: the ncand smallest keys of a query over all slices ----------------------------------
// cand[query * ncand + e]: database rows, kNone past the last.
__global__ __launch_bounds__(kThreads) void ann_merge_kernel(const uint64_t *__restrict__ buf,
                                                             const int *__restrict__ cntg, int N, int S, int B,
                                                             int ncand, uint32_t *__restrict__ cand) {
  __shared__ uint64_t scratch[kThreads / 64][kMaxCand + kMaxBuf];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long query = (long long)blockIdx.x * (kThreads / 64) + wave;  // wave-uniform
  if (query >= N) return;
  uint64_t *scr = scratch[wave];
  int have = 0;
  for (int s = 0; s < S; ++s) {
    const int n = std::min(cntg[(size_t)query * S + s], B);
    const uint64_t *qb = buf + ((size_t)query * S + s) * B;
    for (int e = lane; e < n; e += 64) scr[have + e] = qb[e];
    have += n;
    if (have > ncand) {
      wave_select<(kMaxCand + kMaxBuf) / 64>(scr, have, ncand, lane);
      have = ncand;
    } else {
      __builtin_amdgcn_wave_barrier();
    }
  }
  for (int e = lane; e < ncand; e += 64) cand[(size_t)query * ncand + e] = e < have ? (uint32_t)scr[e] : kNone;
}

// ---- re-rank: exact distances of the candidates, then the k smallest (dist, idx) ----------------
// cand == nullptr: every database row is a candidate (M <= ncand).
template <int PER>
__global__ __launch_bounds__(kThreads) void ann_rerank_kernel(const float *__restrict__ x,
                                                              const float *__restrict__ y, int M, int N, int dim,
                                                              int k, int ncand, const uint32_t *__restrict__ cand,
                                                              int vec, uint64_t *__restrict__ out_idx,
                                                              float *__restrict__ out_dist) {
  __shared__ uint64_t scratch[kThreads / 64][64 * PER];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long query = (long long)blockIdx.x * (kThreads / 64) + wave;  // wave-uniform
  if (query >= N) return;
  uint64_t *scr = scratch[wave];
  const float *yr = y + (size_t)query * dim;
  int real = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int c = lane + 64 * i;
    uint32_t row = kNone;
    if (c < ncand) row = cand ? cand[(size_t)query * ncand + c] : (c < M ? (uint32_t)c : kNone);
    uint64_t key = kKeyNone;
    if (row != kNone) {
      const float *xr = x + (size_t)row * dim;
      float sum = 0.f;
      if (vec) {
        for (int c4 = 0; c4 < dim; c4 += 4) {
          const float4 xv = *reinterpret_cast<const float4 *>(xr + c4);
          const float4 yv = *reinterpret_cast<const float4 *>(yr + c4);
          float d = xv.x - yv.x, tt = d * d;
          sum = sum + tt;
          d = xv.y - yv.y, tt = d * d;
          sum = sum + tt;
          d = xv.z - yv.z, tt = d * d;
          sum = sum + tt;
          d = xv.w - yv.w, tt = d * d;
          sum = sum + tt;
        }
      } else {
        for (int cc = 0; cc < dim; ++cc) {
          const float d = xr[cc] - yr[cc], tt = d * d;
          sum = sum + tt;
        }
      }
      key = ((uint64_t)__float_as_uint(sum) << 32) | row;
    }
    scr[c] = key;
    real += __popcll(__builtin_amdgcn_ballot_w64(row != kNone));
  }
  wave_select<PER>(scr, 64 * PER, k, lane);
  for (int j = lane; j < k; j += 64) {
    const uint64_t key = j < real ? scr[j] : kKeyNone;
    const bool none = key == kKeyNone;
    out_idx[(size_t)query * k + j] = none ? ~0ull : (key & 0xFFFFFFFFull);
    out_dist[(size_t)query * k + j] = none ? INFINITY : __uint_as_float((uint32_t)(key >> 32));
  }
}

int env_mfma() {
  static const int v = [] {
    const char *e = getenv("SPECTAVI_ANN_MFMA");
    const int s = e && *e ? atoi(e) : 0;
    return s == 16 || s == 32 ? s : 0;
  }();
  return v;
}

}  // namespace

int ann_check(int xrows, int yrows, int dim, int k, int ncand) {
  if (xrows < 0 || yrows < 0) return set_error(SPV_ERR_INVALID, "negative row count");
  if (dim < 1 || dim > kMaxDim) return set_error(SPV_ERR_INVALID, "dim=%d outside [1, %d]", dim, kMaxDim);
  if (k < 1 || k > kMaxK) return set_error(SPV_ERR_INVALID, "k=%d outside [1, %d]", k, kMaxK);
  if (ncand != 0 && (ncand < k || ncand > kMaxCand))
    return set_error(SPV_ERR_INVALID, "ncand=%d outside [k=%d, %d] (0: the default)", ncand, k, kMaxCand);
  return SPV_OK;
}

AnnPlan ann_plan(int xrows, int yrows, int dim, int k, int ncand, int slices) {
  AnnPlan p{};
  p.kpad = (dim + 31) / 32 * 32;
  p.qtile = kQT;
  p.rtile = kRT;
  p.ncand = ncand ? ncand : std::max(16, 4 * k);
  p.buflen = (p.ncand + 96 + 63) / 64 * 64;  // >= ncand + kRoom + 64 appends between two compactions
  p.mfma = env_mfma() ? env_mfma() : 32;
  p.all_rows = xrows <= p.ncand;
  p.qblocks = std::max(1, (yrows + kQT - 1) / kQT);
  long long rows;
  if (slices > 0) {
    rows = std::max<long long>(1, ((long long)xrows + slices - 1) / slices);
  } else {
    // One round of resident workgroups (three on each of the 256 CUs) and no more: every slice pays for
    // its own first survivors, about 1.9 ms of the coarse kernel's 11 ms at 131072 x 131072 x 128
    // (profiles/r14_ann_paths.jsonl).  Slices of whole tiles and at least 2048 rows.
    const long long s = std::max<long long>(1, (768 + p.qblocks - 1) / p.qblocks);
    rows = ((long long)xrows + s - 1) / s;
    rows = std::max<long long>(2048, (rows + kRT - 1) / kRT * kRT);
  }
  p.slice_rows = (int)std::min<long long>(rows, std::max(xrows, 1));
  p.slices = std::max(1, (int)(((long long)xrows + p.slice_rows - 1) / p.slice_rows));
  p.chunks = std::max(1, (xrows + kMeanChunk - 1) / kMeanChunk);
  const size_t xr = (size_t)std::max(xrows, 1), yr = (size_t)std::max(yrows, 1);
  WsWalk w;
  p.off_part = w.reserve((size_t)p.chunks * dim * sizeof(double));
  p.off_mean = w.reserve((size_t)p.kpad * sizeof(float));
  p.off_xb = w.reserve(xr * p.kpad * 2);
  p.off_yb = w.reserve(yr * p.kpad * 2);
  p.off_norm = w.reserve(xr * sizeof(float));
  p.off_cand = w.reserve(yr * p.ncand * sizeof(uint32_t));
  p.off_cnt = w.reserve(yr * p.slices * sizeof(int));
  p.off_buf = w.reserve(yr * p.slices * p.buflen * sizeof(uint64_t));
  p.total_bytes = p.all_rows ? 0 : w.end();
  return p;
}

int ann_run(const float *d_x, const float *d_y, int xrows, int yrows, int dim, int k, int ncand, int slices,
            uint64_t *d_idx, float *d_dist, void *d_ws, size_t ws_bytes, hipStream_t stream) {
  SPV_TRY(ann_check(xrows, yrows, dim, k, ncand));
  if (slices < 0) return set_error(SPV_ERR_INVALID, "slices=%d", slices);
  if (yrows == 0) return SPV_OK;
  if (!d_y || !d_idx || !d_dist || (xrows > 0 && !d_x)) return set_error(SPV_ERR_INVALID, "null device pointer");
  if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_y) | reinterpret_cast<uintptr_t>(d_dist)) & 3)
    return set_error(SPV_ERR_INVALID, "x, y and dist must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_idx) & 7) return set_error(SPV_ERR_INVALID, "idx must be 8-byte aligned");
  const AnnPlan p = ann_plan(xrows, yrows, dim, k, ncand, slices);
  if (p.slices > 65535) return set_error(SPV_ERR_INVALID, "slices=%d > 65535", p.slices);
  uint8_t *ws = static_cast<uint8_t *>(d_ws);
  if (!p.all_rows) {
    if (!d_ws || (reinterpret_cast<uintptr_t>(d_ws) & 255))
      return set_error(SPV_ERR_INVALID, "the workspace must be 256-byte aligned");
    if (ws_bytes < p.total_bytes)
      return set_error(SPV_ERR_INVALID, "workspace too small: %zu < %zu", ws_bytes, p.total_bytes);
  }
  const uint32_t *cand = nullptr;
  if (!p.all_rows) {
    double *part = reinterpret_cast<double *>(ws + p.off_part);
    float *mean = reinterpret_cast<float *>(ws + p.off_mean);
    uint16_t *xb = reinterpret_cast<uint16_t *>(ws + p.off_xb);
    uint16_t *yb = reinterpret_cast<uint16_t *>(ws + p.off_yb);
    float *norm = reinterpret_cast<float *>(ws + p.off_norm);
    uint64_t *buf = reinterpret_cast<uint64_t *>(ws + p.off_buf);
    int *cnt = reinterpret_cast<int *>(ws + p.off_cnt);
    uint32_t *cnd = reinterpret_cast<uint32_t *>(ws + p.off_cand);
    {
      ProfScope prof("ann_prep", stream);
      const unsigned cb = (unsigned)((dim + kThreads - 1) / kThreads), kb = (unsigned)((p.kpad + kThreads - 1) / kThreads);
      hipLaunchKernelGGL(ann_colsum_kernel, dim3(p.chunks, cb), dim3(kThreads), 0, stream, d_x, xrows, dim, part);
      hipLaunchKernelGGL(ann_mean_kernel, dim3(kb), dim3(kThreads), 0, stream, part, xrows, dim, p.kpad, p.chunks, mean);
      auto blocks = [](long long n) { return (unsigned)((n + kThreads - 1) / kThreads); };
      hipLaunchKernelGGL(ann_convert_kernel, dim3(blocks((long long)xrows * (p.kpad / 8))), dim3(kThreads), 0, stream,
                         d_x, xrows, dim, p.kpad, mean, xb);
      hipLaunchKernelGGL(ann_convert_kernel, dim3(blocks((long long)yrows * (p.kpad / 8))), dim3(kThreads), 0, stream,
                         d_y, yrows, dim, p.kpad, mean, yb);
      hipLaunchKernelGGL(ann_norm_kernel, dim3(blocks(xrows)), dim3(kThreads), 0, stream, xb, xrows, p.kpad, norm);
    }
    SPV_HIP_CHECK(hipGetLastError());
    {
      ProfScope prof("ann_coarse", stream);
      const dim3 grid(p.qblocks, p.slices);
      const int kg = p.kpad <= kKC ? p.kpad / 32 : 0;
      pick(Ints<32, 16>{}, p.mfma, [&](auto SHAPE) {
        return pick(Ints<1, 2, 3, 4, 0>{}, kg, [&](auto KG) {
          hipLaunchKernelGGL((ann_coarse_kernel<decltype(SHAPE)::value, decltype(KG)::value>), grid, dim3(kThreads), 0,
                             stream, xb, yb, norm, xrows, yrows, p.kpad, p.slice_rows, p.slices, p.ncand, p.buflen, buf, cnt);
          return true;
        });
      });
    }
    SPV_HIP_CHECK(hipGetLastError());
    {
      ProfScope prof("ann_merge", stream);
      const unsigned blocks = (unsigned)(((long long)yrows + kThreads / 64 - 1) / (kThreads / 64));
      hipLaunchKernelGGL(ann_merge_kernel, dim3(blocks), dim3(kThreads), 0, stream, buf, cnt, yrows, p.slices,
                         p.buflen, p.ncand, cnd);
    }
    SPV_HIP_CHECK(hipGetLastError());
    cand = cnd;
  }
  {
    ProfScope prof("ann_rerank", stream);
    const unsigned blocks = (unsigned)(((long long)yrows + kThreads / 64 - 1) / (kThreads / 64));
    const int vec = dim % 4 == 0 &&
                    ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_y)) & 15) == 0;
    if (p.ncand <= 64)
      hipLaunchKernelGGL((ann_rerank_kernel<1>), dim3(blocks), dim3(kThreads), 0, stream, d_x, d_y, xrows, yrows, dim,
                         k, p.ncand, cand, vec, d_idx, d_dist);
    else
      hipLaunchKernelGGL((ann_rerank_kernel<4>), dim3(blocks), dim3(kThreads), 0, stream, d_x, d_y, xrows, yrows, dim,
                         k, p.ncand, cand, vec, d_idx, d_dist);
  }
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

}  // namespace spv
