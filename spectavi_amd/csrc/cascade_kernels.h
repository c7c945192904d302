// cascade_kernels.h -- the device code cascade.hip and cascade_batch.hip share: the dictionary repack, the three
// projection families with the launch helper that turns a CascadePlan's choice into an instantiation, the bucket
// scan kernels, and the v_sad_u8 / top-2 / probe-code helpers of the refine.  The design they serve is described at
// the top of cascade.hip.  Each file that includes this compiles its own copies of the instantiations it names.
#pragma once

#include "common.h"
#include "device_util.h"

namespace spv {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxBucketBits = 22;
constexpr int kListCap = 512;  // candidate indices staged in LDS per wave
constexpr uint64_t kNone64 = ~0ull;

inline int bucket_bits(int m) { return std::min(m, kMaxBucketBits); }

// ---------------------------------------------------------------------------------
// 1. dictionary repack
// ---------------------------------------------------------------------------------
__global__ void repack_dict_kernel(const float *__restrict__ dict, float *__restrict__ dictp, int n,
                                   int dim, int m, int mc) {
  const int total = n * dim * mc;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int b = e % mc;
    const int ji = e / mc;  // j*dim + i
    dictp[e] = b < m ? dict[(size_t)ji * m + b] : 0.f;
  }
}

// ---------------------------------------------------------------------------------
// 2/3. projections, codes, uint8 image.  A workgroup owns 256 rows, one per lane
// (kProjRows).  Per 16-dim step the row tile is staged in LDS by coalesced 16-byte loads
// (the uint8 image is written from the same registers), the hyperplanes of that step
// are staged next to it and read by broadcast ds_read_b128 -- one LDS dword feeds
// 64 lanes.  Accumulators of up to two tables stay in registers, so float32 rows are
// read from HBM once.  The projection of (row, bit) is ONE
// dim-ordered fp32 FMA chain (mirrored by the oracle).
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t f2u8(float v) {
  return (uint32_t)((int)v + 128) & 0xFFu;  // trunc toward zero, wrap mod 256
}

constexpr int kProjRows = 1;                 // rows per lane (2 halves the broadcast reads per FMA but its
                                             // 77 KB of LDS allow only two workgroups per CU: measured slower)
constexpr int kProjTile = kThreads * kProjRows;  // rows per workgroup
constexpr int kProjChunk = 16;               // dims staged per step (dim % 16 == 0 always)
constexpr int kProjXStride = kProjChunk * 4 + 16;  // bytes per row in LDS: 80 -> conflict-free b128 reads

// NT tables are accumulated per pass over the rows (NT*R*MC accumulators per lane); NT = 2 (the
// choice whenever MC <= 24, see cascade_plan) reads the float32 rows from HBM exactly once.
template <int MC, int NT, bool IS_QUERY, int GMAX>
__global__ __launch_bounds__(kThreads) void project_kernel(
    const float *__restrict__ rows, int nrows, int dim, int m, int n, int g,
    const float *__restrict__ dictp,     // [n][dim][MC]
    uint32_t *__restrict__ codes,        // [n][nrows] sign codes
    uint32_t *__restrict__ masks,        // [n][nrows] (queries only)
    uint8_t *__restrict__ u8img,         // [nrows][dim]
    uint32_t *__restrict__ counts,       // [n][nb+1] bucket histogram (may be NULL: none wanted)
    uint32_t *__restrict__ ranks,        // [n][nrows] rank of the row inside its bucket (with counts)
    uint32_t hbmask, int nb) {
  constexpr int R = kProjRows;
  __shared__ __attribute__((aligned(16))) uint8_t xs[kProjTile * kProjXStride];  // row tile, 16 dims
  __shared__ __attribute__((aligned(16))) uint8_t u8s[kProjTile * 64];  // uint8 image, four steps
  __shared__ float4 sd[NT][kProjChunk * MC / 4];  // hyperplanes [table][dim of the chunk][MC]
  // accumulator start values: +0 for real hyperplanes, +inf for the zero-padded ones so
  // that they are never picked as "least confident" (their code bits are masked off)
  __shared__ float sinit[MC];
  const int t = threadIdx.x;
  const int base = blockIdx.x * kProjTile;
  if (t < MC) sinit[t] = t < m ? 0.f : __builtin_inff();
  __syncthreads();

  for (int jt = 0; jt < n; jt += NT) {
    float acc[NT][R][MC];
#pragma unroll
    for (int b = 0; b < MC; ++b) {
      const float a0 = sinit[b];
#pragma unroll
      for (int tj = 0; tj < NT; ++tj)
#pragma unroll
        for (int k = 0; k < R; ++k) acc[tj][k][b] = a0;
    }
    // register-prefetched staging: the global loads of step c0+16 are in flight while
    // step c0 is being computed out of LDS
    constexpr int NX = kProjTile * (kProjChunk / 4) / kThreads;           // row-tile vectors per lane
    constexpr int ND = (NT * kProjChunk * MC / 4 + kThreads - 1) / kThreads;  // hyperplane vectors per lane
    float4 px[NX], pd[ND];
    auto prefetch = [&](int c0) {
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int e = t + i * kThreads;
        const int grow = base + (e >> 2);
        px[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (grow < nrows)
          px[i] = *reinterpret_cast<const float4 *>(rows + (size_t)grow * dim + c0 + 4 * (e & 3));
      }
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        const int e = t + i * kThreads;                 // [table of the pass][dim][MC/4]
        const int tj = e / (kProjChunk * MC / 4), w = e % (kProjChunk * MC / 4);
        pd[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tj < NT && jt + tj < n)
          pd[i] = reinterpret_cast<const float4 *>(dictp + ((size_t)(jt + tj) * dim + c0) * MC)[w];
      }
    };
    prefetch(0);
    for (int c0 = 0; c0 < dim; c0 += kProjChunk) {
      __syncthreads();  // everyone is done reading the previous step out of LDS
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        const int e = t + i * kThreads;
        const int row = e >> 2, c = e & 3;
        *reinterpret_cast<float4 *>(xs + row * kProjXStride + 16 * c) = px[i];
        if (jt == 0) {
          // uint8 image: four 16-dim steps are collected per row in LDS (64 bytes per row,
          // unpadded: 16*e addressing) and flushed below as 64-byte runs = full sectors
          const float4 v = px[i];
          const uint32_t pk = f2u8(v.x) | (f2u8(v.y) << 8) | (f2u8(v.z) << 16) | (f2u8(v.w) << 24);
          *reinterpret_cast<uint32_t *>(u8s + row * 64 + ((c0 >> 4) & 3) * 16 + 4 * c) = pk;
        }
      }
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        const int e = t + i * kThreads;
        if (e < NT * kProjChunk * MC / 4) (&sd[0][0])[e] = pd[i];
      }
      __syncthreads();
      if (jt == 0 && ((((c0 >> 4) & 3) == 3) || c0 + kProjChunk >= dim)) {
        const int ngrp = ((c0 >> 4) & 3) + 1;
        const int col0 = c0 - (ngrp - 1) * kProjChunk;
#pragma unroll
        for (int i = 0; i < NX; ++i) {
          const int e = t + i * kThreads;
          const int row = e >> 2, q = e & 3;
          if (q < ngrp && base + row < nrows)
            *reinterpret_cast<uint4 *>(u8img + (size_t)(base + row) * dim + col0 + 16 * q) =
                *reinterpret_cast<const uint4 *>(u8s + 16 * e);
        }
      }
      if (c0 + kProjChunk < dim) prefetch(c0 + kProjChunk);
#pragma unroll
      for (int i0 = 0; i0 < kProjChunk; i0 += 4) {
        float4 xv[R];
#pragma unroll
        for (int k = 0; k < R; ++k)
          xv[k] = *reinterpret_cast<const float4 *>(xs + (t + k * kThreads) * kProjXStride + 4 * i0);
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
#pragma unroll
          for (int tj = 0; tj < NT; ++tj) {
            // all lanes read the same hyperplane row: LDS broadcast, MC/4 x ds_read_b128
            float dv[MC];
#pragma unroll
            for (int b4 = 0; b4 < MC / 4; ++b4) {
              const float4 d4 = sd[tj][(i0 + ii) * (MC / 4) + b4];
              dv[4 * b4 + 0] = d4.x;
              dv[4 * b4 + 1] = d4.y;
              dv[4 * b4 + 2] = d4.z;
              dv[4 * b4 + 3] = d4.w;
            }
#pragma unroll
            for (int k = 0; k < R; ++k) {
              const float xsv =
                  ii == 0 ? xv[k].x : (ii == 1 ? xv[k].y : (ii == 2 ? xv[k].z : xv[k].w));
#pragma unroll
              for (int b = 0; b < MC; ++b) acc[tj][k][b] = __builtin_fmaf(xsv, dv[b], acc[tj][k][b]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) {
      const int j = jt + tj;
      if (j >= n) break;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        const int r = base + t + k * kThreads;
        uint32_t code = 0;
#pragma unroll
        for (int b = 0; b < MC; ++b) code |= (acc[tj][k][b] >= 0.f ? 1u : 0u) << b;
        code &= 0xFFFFFFFFu >> (32 - m);  // padded hyperplanes: drop their bits
        if (r < nrows) {
          codes[(size_t)j * nrows + r] = code;
          // database rows: bucket histogram for the counting sort, fused here
          // (the value the atomic returns is the row's rank inside its bucket: the fill pass
          // needs no second round of atomics; the matrix-core kernels' epilogue does the same for
          // query rows too, this kernel leaves those to query_rank_kernel: the atomic in this
          // epilogue's query form cost its widest instantiation its full unrolling)
          if (!IS_QUERY && counts)
            ranks[(size_t)j * nrows + r] = atomicAdd(&counts[(size_t)j * (nb + 1) + (code & hbmask)], 1u);
        }
        if (IS_QUERY) {
          // g smallest (|proj|, bit) pairs, lexicographic like the reference's max-heap of
          // pairs (src/CascadingHashNn.h:153-159): sorted insertion with the bit as tie-break,
          // which matters for an entry displaced down the list past an equal magnitude
          float best[GMAX];
          int bbit[GMAX];
#pragma unroll
          for (int q = 0; q < GMAX; ++q) {
            best[q] = __builtin_inff();
            bbit[q] = -1;
          }
#pragma unroll
          for (int b = 0; b < MC; ++b) {
            float v = fabsf(acc[tj][k][b]);  // +inf for padded hyperplanes: never inserted
            int vb = b;
#pragma unroll
            for (int q = 0; q < GMAX; ++q) {
              const bool lt = q < g && (v < best[q] || (v == best[q] && vb < bbit[q]));
              const float tv = best[q];
              const int tb = bbit[q];
              best[q] = lt ? v : tv;
              bbit[q] = lt ? vb : tb;
              v = lt ? tv : v;
              vb = lt ? tb : vb;
            }
          }
          uint32_t mask = 0;
#pragma unroll
          for (int q = 0; q < GMAX; ++q)
            if (q < g && bbit[q] >= 0) mask |= 1u << bbit[q];
          if (r < nrows) masks[(size_t)j * nrows + r] = mask;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// 2b/3b. the same projections on the matrix cores (used when all n*m hyperplanes fit 64
// columns, i.e. every default configuration).  The projection is the one GEMM-shaped step of
// the path: P[rows][n*m] = X[rows][dim] * H[dim][n*m].  v_mfma_f32_16x16x4_f32 accumulates each
// output element as a sequential fp32 FMA chain in k order -- checked against std::fmaf on
// 64 000 outputs, tools/exp/mfma_order.hip: 100 % identical -- so the result is bit for bit the
// chain the oracle and the VALU kernel above compute, at four times the FMA rate and without
// the LDS broadcast traffic that bounds the VALU kernel.
//
// One wave owns 64 rows (waves are independent: no workgroup barriers).  Per 32-dim step
// the wave's float4 loads (eight lanes cover one full 128-byte line of a row; prefetched one
// step ahead; the uint8 image is packed from the same registers) are staged in a
// wave-private LDS tile, from which lane
// (r = lane % 16, q = lane / 16) reads A[row r of row-tile rt][k + q]; the hyperplane operand
// B[k + q][column] comes straight from the repacked dictionary dictm[dim][16*CT] (L1/L2
// resident).  4 x CT accumulator tiles of 16 x 16.  Afterwards the tiles are transposed
// through LDS so that one lane holds one row's n*m projections and runs the same epilogue as
// the VALU kernel: sign codes, the g least-confident bits, bucket histogram.
// ---------------------------------------------------------------------------------
constexpr int kMfmaChunkC = 32;  // = kMfmaChunk (declared below): dims per step of the MFMA kernels
__global__ void repack_dict_mfma_kernel(const float *__restrict__ dict, float *__restrict__ dictm, int n,
                                        int dim, int m, int nc) {
  const int dimpad = (dim + kMfmaChunkC - 1) / kMfmaChunkC * kMfmaChunkC;  // whole chunks: zero rows past dim
  const int total = dimpad * nc;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int c = e % nc, i = e / nc;  // column c = table * m + bit
    const int tj = c / m, b = c % m;
    dictm[e] = (tj < n && i < dim) ? dict[((size_t)tj * dim + i) * m + b] : 0.f;
  }
}

typedef float mfma_f4 __attribute__((ext_vector_type(4)));

constexpr int kMfmaChunk = kMfmaChunkC;  // dims per step: 8 lanes x 16 B = one full 128-byte line per row

// Row part of the matrix-core projection kernels' epilogue: lane l holds the n*m projections of row
// row0 + l at `mine` (LDS, column c = table*m + bit; column `pad` is a harmless filler for the slots
// past m): sign codes, the g least-confident bits and the bucket histogram as in the VALU kernel.
// Rows at and past row_limit are not written.
template <bool IS_QUERY, int GMAX>
__device__ __forceinline__ void project_rows_epilogue(
    const float *mine, int pad, int lane, long long row0, long long row_limit, long long nrows_total,
    int m, int n, int g, uint32_t *__restrict__ codes, uint32_t *__restrict__ masks,
    uint32_t *__restrict__ counts, uint32_t *__restrict__ ranks, uint32_t hbmask, int nb) {
  const long long r = row0 + lane;
  const long long nrows = row_limit;  // rows at and past it belong to nobody here
  for (int j = 0; j < n; ++j) {
    uint32_t code = 0;
    float best[GMAX];
    int bbit[GMAX];
#pragma unroll
    for (int q = 0; q < GMAX; ++q) {
      best[q] = __builtin_inff();
      bbit[q] = -1;
    }
    // eight projections per round: the LDS reads of a round are independent, so their latency
    // is paid once per round instead of once per bit
    for (int b0 = 0; b0 < m; b0 += 8) {
      float p8[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) p8[i] = mine[min(j * m + b0 + i, pad)];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int b = b0 + i;
        const bool live = b < m;
        const float p = p8[i];
        code |= (live && p >= 0.f ? 1u : 0u) << (b & 31);
        if (IS_QUERY) {
          // g smallest (|proj|, bit) pairs, lexicographic (see the VALU kernel's epilogue);
          // slots past m enter as +inf and are never inserted
          float v = live ? fabsf(p) : __builtin_inff();
          int vb = b;
#pragma unroll
          for (int q = 0; q < GMAX; ++q) {
            const bool lt = q < g && (v < best[q] || (v == best[q] && vb < bbit[q]));
            const float tv = best[q];
            const int tb = bbit[q];
            best[q] = lt ? v : tv;
            bbit[q] = lt ? vb : tb;
            v = lt ? tv : v;
            vb = lt ? tb : vb;
          }
        }
      }
    }
    if (r < nrows) {
      codes[(size_t)j * nrows_total + r] = code;
      // bucket histogram, fused (database rows: the buckets; query rows: the order the probe walks
      // them in); the value the atomic returns is the row's rank inside its bucket, so the fill pass
      // needs no second round of atomics.  (Issuing the atomics of all tables together after this
      // loop, one round trip per wave instead of one per table, measured 0.385 -> 0.405 ms for the
      // 1M + 1M rows of the sorted form, no change for the database pass alone: kept per table.)
      if (counts)
        ranks[(size_t)j * nrows_total + r] = atomicAdd(&counts[(size_t)j * (nb + 1) + (code & hbmask)], 1u);
    }
    if (IS_QUERY) {
      uint32_t mask = 0;
#pragma unroll
      for (int q = 0; q < GMAX; ++q)
        if (q < g && bbit[q] >= 0) mask |= 1u << bbit[q];
      if (r < nrows) masks[(size_t)j * nrows_total + r] = mask;
    }
  }
}

// Epilogue of project_mfma_kernel: the wave's 4 x CT accumulator tiles are transposed through its LDS
// tile so that lane l holds the projections of row row0 + l, then the row part above.
template <int CT, bool IS_QUERY, int GMAX>
__device__ __forceinline__ void project_mfma_epilogue(
    const mfma_f4 (&acc)[4][CT], float *ws, int lane, long long row0, long long row_limit, long long nrows_total,
    int m, int n, int g, uint32_t *__restrict__ codes, uint32_t *__restrict__ masks,
    uint32_t *__restrict__ counts, uint32_t *__restrict__ ranks, uint32_t hbmask, int nb) {
  constexpr int NC = 16 * CT;
  constexpr int ES = NC + 1;
  const int r16 = lane & 15, q4 = lane >> 4;
  // transpose: D tile element v of lane (r16, q4) is row 16*rt + 4*q4 + v, column 16*ct + r16
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int v = 0; v < 4; ++v) ws[(16 * rt + 4 * q4 + v) * ES + 16 * ct + r16] = acc[rt][ct][v];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  project_rows_epilogue<IS_QUERY, GMAX>(ws + lane * ES, NC, lane, row0, row_limit, nrows_total, m, n, g, codes, masks,
                                        counts, ranks, hbmask, nb);
}

template <int CT, bool IS_QUERY, int GMAX, bool FULL>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(CT <= 3 ? 3 : 2))) void project_mfma_kernel(
    const float *__restrict__ rows, int nrows, int dim, int m, int n, int g,
    const float *__restrict__ dictm,     // [roundup(dim, 32)][16*CT], column = table*m + bit, zero padded
    uint32_t *__restrict__ codes, uint32_t *__restrict__ masks, uint8_t *__restrict__ u8img,
    uint32_t *__restrict__ counts, uint32_t *__restrict__ ranks, uint32_t hbmask, int nb) {
  constexpr int NC = 16 * CT;
  constexpr int KS = kMfmaChunk / 4;   // MFMA k-steps per chunk
  constexpr int NX = kMfmaChunk / 4;   // float4 loads per lane per chunk (64 rows x 32 dims / 64 lanes / 4)
  constexpr int XS = kMfmaChunk + 1;   // floats per staged row (+1: spreads the rows over the banks)
  constexpr int ES = NC + 1;           // floats per row of the transposed projections
  constexpr int kWaveFloats = 64 * (ES > XS ? ES : XS);
  __shared__ float lds[(kThreads / 64) * kWaveFloats];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float *ws = lds + wv * kWaveFloats;
  const long long row0 = ((long long)blockIdx.x * (kThreads / 64) + wv) * 64;
  if (row0 >= nrows) return;  // whole wave past the end (nothing below synchronises across waves)
  const int r16 = lane & 15, q4 = lane >> 4;
  const int quad = lane & 3;

  mfma_f4 acc[4][CT];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = mfma_f4{0.f, 0.f, 0.f, 0.f};

  float4 px[NX];
  // FULL: dim is a whole number of 32-dim chunks, every load is unconditional.  Otherwise
  // (dim % 32 == 16) the dims past the end of a row are staged as zeros and multiply the zero
  // rows the repacked dictionary is padded with: fmaf(0, 0, acc) leaves every accumulator as it is
  auto prefetch = [&](int c0) {
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int e = lane + 64 * j;  // (row of the tile, 4-dim part of the step): 8 lanes per row
      const long long grow = min(row0 + (e >> 3), (long long)nrows - 1);
      const int d0 = c0 + 4 * (e & 7);
      if (FULL || d0 < dim) {  // read once: keep the rows out of the way of the hyperplanes in L1
        const mfma_f4 t4 = __builtin_nontemporal_load(reinterpret_cast<const mfma_f4 *>(rows + (size_t)grow * dim + d0));
        px[j] = make_float4(t4[0], t4[1], t4[2], t4[3]);
      } else {
        px[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  // Hyperplane operands of a whole chunk (KS k-steps x CT column tiles, L1 / L2 resident), requested
  // right after the previous chunk's MFMAs -- i.e. AFTER that chunk's row prefetch and BEFORE this
  // chunk's stores and the next row prefetch.  Vector-memory operations of a wave complete in issue
  // order (s_waitcnt vmcnt counts the youngest N): fetched inside the MFMA loop, behind the
  // prefetch, every operand wait would also wait for the HBM stream.
  float bq[KS][CT];
  auto fetch_b_chunk = [&](int c0) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) bq[ks][ct] = dictm[(size_t)(c0 + 4 * ks + q4) * NC + 16 * ct + r16];
  };
  prefetch(0);
  fetch_b_chunk(0);
  for (int c0 = 0; c0 < dim; c0 += kMfmaChunk) {
    // stage the chunk in LDS (A operand order) and assemble the uint8 image: the four lanes of a
    // quad hold 16 consecutive bytes of a row; quad broadcasts give every lane all four dwords,
    // lane t of the quad keeps those of load j = t (mod 4), so that two 16-byte-per-lane stores
    // per chunk replace eight 4-byte ones
    uint4 keep = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int e = lane + 64 * j;
      const int row = e >> 3, part = e & 7;
      const float4 v = px[j];
      float *dstp = ws + row * XS + 4 * part;
      dstp[0] = v.x;
      dstp[1] = v.y;
      dstp[2] = v.z;
      dstp[3] = v.w;
      const uint32_t pk = f2u8(v.x) | (f2u8(v.y) << 8) | (f2u8(v.z) << 16) | (f2u8(v.w) << 24);
      const uint32_t g0 = __builtin_amdgcn_mov_dpp(pk, 0x00, 0xF, 0xF, true);  // quad_perm [0,0,0,0]
      const uint32_t g1 = __builtin_amdgcn_mov_dpp(pk, 0x55, 0xF, 0xF, true);  // [1,1,1,1]
      const uint32_t g2 = __builtin_amdgcn_mov_dpp(pk, 0xAA, 0xF, 0xF, true);  // [2,2,2,2]
      const uint32_t g3 = __builtin_amdgcn_mov_dpp(pk, 0xFF, 0xF, 0xF, true);  // [3,3,3,3]
      if (quad == (j & 3)) keep = make_uint4(g0, g1, g2, g3);
      if ((j & 3) == 3) {
        const int krow = 8 * ((j & ~3) + quad) + (lane >> 3);  // row of the load this lane kept
        const int kbyte = c0 + 16 * ((lane & 7) >> 2);         // first byte of the quad's 16
        if (row0 + krow < nrows && (FULL || kbyte < dim))
          *reinterpret_cast<uint4 *>(u8img + (size_t)(row0 + krow) * dim + kbyte) = keep;
      }
    }
    if (c0 + kMfmaChunk < dim) prefetch(c0 + kMfmaChunk);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      float a[4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) a[rt] = ws[(16 * rt + r16) * XS + 4 * ks + q4];
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt], bq[ks][ct], acc[rt][ct], 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (c0 + kMfmaChunk < dim) fetch_b_chunk(c0 + kMfmaChunk);
  }

  project_mfma_epilogue<CT, IS_QUERY, GMAX>(acc, ws, lane, row0, nrows, nrows, m, n, g, codes, masks, counts, ranks,
                                            hbmask, nb);
}

// The same projection when n*m is not a whole number of 16-column tiles and 1..8 columns are left
// over (the default configuration: n*m = 2 x 17 = 34 = two tiles + 2): the left-over columns go
// through v_mfma_f32_4x4x1_16B_f32 -- 16 blocks of D[4x4] += A[4x1] B[1x4], i.e. 64 rows x 4 columns
// x ONE k per instruction at ~11 cycles per SIMD -- instead of a third, 7/8-empty 16-column tile at
// 32 cycles per 4 k and 16 rows (measured, tools/exp/mfma_4x4_exp.hip: lane l feeds A[row l] and
// B[column l % 4], D[i] of lane l is row 4 (l / 4) + i, column l % 4; 51 200 of 51 200 outputs equal the
// std::fmaf chain in k order).  -21 % matrix-pipe time per row at n*m = 34.  Differences from
// project_mfma_kernel besides that: whole-chunk dims only (dim % 32 == 0, dim <= 512; anything else
// takes project_mfma_kernel, as does SPECTAVI_CASCADE_MFMA4=0 for A/B runs); staged rows
// are 16-byte aligned (36 floats: one ds_write_b128 per load, one ds_read_b128 per k-step for the
// 4x4x1 A operand); the left-over hyperplanes sit in a workgroup-shared LDS table [dim/4][4][4].
// workgroups per CU by LDS (4 wave tiles + the left-over table): three for the default shape
constexpr int mfma4_waves_per_simd(int ct, int ng) {
  // wave tiles + uint8 staging (static) + the left-over table at its largest (dim 512, dynamic)
  return 4 * 64 * 4 * (16 * ct + 4 * ng + 1 > 36 ? 16 * ct + 4 * ng + 1 : 36) + 4 * 2048 + ng * 8192 <= 160 * 1024 / 3 ? 3 : 2;
}

template <int CT, int NG, bool IS_QUERY, int GMAX>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(mfma4_waves_per_simd(CT, NG)))) void project_mfma4_kernel(
    const float *__restrict__ rows, int nrows, int dim, int m, int n, int g,
    const float *__restrict__ dictm,     // [dim][NCD], column = table*m + bit, zero padded; NCD = 16*(CT+1)
    uint32_t *__restrict__ codes, uint32_t *__restrict__ masks, uint8_t *__restrict__ u8img,
    uint32_t *__restrict__ counts, uint32_t *__restrict__ ranks, uint32_t hbmask, int nb) {
  constexpr int NCD = 16 * (CT + 1);     // row length of dictm (the layout the 16-column kernel uses)
  constexpr int NCOL = 16 * CT + 4 * NG; // columns computed here
  constexpr int KS = kMfmaChunk / 4;
  constexpr int NX = kMfmaChunk / 4;
  constexpr int XS = kMfmaChunk + 4;     // floats per staged row: 16-byte aligned rows
  constexpr int ES = NCOL + 1;           // floats per row of the transposed projections
  constexpr int kWaveFloats = 64 * (ES > XS ? ES : XS);
  __shared__ __attribute__((aligned(16))) float lds[(kThreads / 64) * kWaveFloats];
  // uint8 image of the chunk being staged, per wave: 64 rows x 32 bytes, written one packed dword per
  // lane and load (byte offset 256 j + 4 lane = row-major) and read back 16 bytes per lane for the
  // stores.  Round 2 assembled those 16 bytes with four quad broadcasts and a predicated copy per
  // load: 80 VALU instructions per chunk, a fifth of the database pass's.
  __shared__ __attribute__((aligned(16))) uint32_t u8s[kThreads / 64][64 * kMfmaChunk / 4];
  // left-over hyperplanes [group][k / 4][column][k % 4], sized by the launch: NG * dim * 16 bytes
  // (8 KB per group at dim 512, 2 KB at 128: statically sized for 512 they cost dim 128 its third
  // workgroup per CU once the uint8 staging above was added)
  extern __shared__ __attribute__((aligned(16))) float hl_dyn[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float *ws = lds + wv * kWaveFloats;
  uint32_t *u8w = u8s[wv];
  const int hl_group = dim * 4;  // floats per group
  const long long row0 = ((long long)blockIdx.x * (kThreads / 64) + wv) * 64;
  const int r16 = lane & 15, q4 = lane >> 4;
  const int quad = lane & 3;

  mfma_f4 acc[4][CT > 0 ? CT : 1];
  mfma_f4 accl[NG];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = mfma_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int gq = 0; gq < NG; ++gq) accl[gq] = mfma_f4{0.f, 0.f, 0.f, 0.f};

  float4 px[NX];
  auto prefetch = [&](int c0) {
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int e = lane + 64 * j;  // (row of the tile, 4-dim part of the step): 8 lanes per row
      const long long grow = min(row0 + (e >> 3), (long long)nrows - 1);
      const mfma_f4 t4 = __builtin_nontemporal_load(reinterpret_cast<const mfma_f4 *>(rows + (size_t)grow * dim + c0 + 4 * (e & 7)));
      px[j] = make_float4(t4[0], t4[1], t4[2], t4[3]);
    }
  };
  // operands of the 16-column tiles for a whole chunk, requested ahead of the next row prefetch
  // (see project_mfma_kernel)
  float bq[KS][CT > 0 ? CT : 1];
  // one per-lane base pointer, the (k-step, tile) offsets as immediates: the sixteen separately
  // indexed loads of round 2 kept sixteen 64-bit addresses (32 VGPRs) alive across the chunk loop
  const float *bp = dictm + (size_t)q4 * NCD + r16;
  auto fetch_b_chunk = [&](int c0) {
    const float *bc = bp + (size_t)c0 * NCD;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) bq[ks][ct] = bc[4 * ks * NCD + 16 * ct];
  };
  // left-over hyperplanes -> LDS (whole workgroup; the only workgroup-level step).  (Requesting the
  // wave's first row chunk BEFORE this staging was tried: __syncthreads() waits for vmcnt(0), so the
  // HBM round trip moved in front of the barrier instead of under it: 0.385 -> 0.41 ms.)
  for (int e = threadIdx.x; e < NG * dim * 4; e += kThreads) {
    const int gq = e / (dim * 4), rem = e - gq * dim * 4;
    const int k = rem >> 2, j = rem & 3;
    hl_dyn[gq * hl_group + ((k >> 2) * 4 + j) * 4 + (k & 3)] = dictm[(size_t)k * NCD + 16 * CT + 4 * gq + j];
  }
  __syncthreads();
  if (row0 >= nrows) return;  // whole wave past the end (nothing below synchronises across waves)
  prefetch(0);
  fetch_b_chunk(0);
  for (int c0 = 0; c0 < dim; c0 += kMfmaChunk) {
#pragma unroll
    for (int j = 0; j < NX; ++j) {
      const int e = lane + 64 * j;
      const int row = e >> 3, part = e & 7;
      const float4 v = px[j];
      *reinterpret_cast<float4 *>(ws + row * XS + 4 * part) = v;
      // row (lane >> 3) + 8 j, bytes 4 (lane & 7) .. +3 of its 32: dword 64 j + lane of the image
      u8w[64 * j + lane] = f2u8(v.x) | (f2u8(v.y) << 8) | (f2u8(v.z) << 16) | (f2u8(v.w) << 24);
    }
    if (c0 + kMfmaChunk < dim) prefetch(c0 + kMfmaChunk);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // the chunk's uint8 image out: 16-byte piece p = lane + 64 k is half (p & 1) of row p >> 1
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int piece = lane + 64 * k;
      const uint4 img = *reinterpret_cast<const uint4 *>(u8w + 4 * piece);
      if (row0 + (piece >> 1) < nrows)
        *reinterpret_cast<uint4 *>(u8img + (size_t)(row0 + (piece >> 1)) * dim + c0 + 16 * (piece & 1)) = img;
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      // left-over columns first in program order (any order is fine: separate accumulators)
      const float4 al = *reinterpret_cast<const float4 *>(ws + lane * XS + 4 * ks);  // row = lane, 4 consecutive k
#pragma unroll
      for (int gq = 0; gq < NG; ++gq) {
        const float4 bl = *reinterpret_cast<const float4 *>(hl_dyn + gq * hl_group + (((c0 >> 2) + ks) * 4 + quad) * 4);
        accl[gq] = __builtin_amdgcn_mfma_f32_4x4x1f32(al.x, bl.x, accl[gq], 0, 0, 0);
        accl[gq] = __builtin_amdgcn_mfma_f32_4x4x1f32(al.y, bl.y, accl[gq], 0, 0, 0);
        accl[gq] = __builtin_amdgcn_mfma_f32_4x4x1f32(al.z, bl.z, accl[gq], 0, 0, 0);
        accl[gq] = __builtin_amdgcn_mfma_f32_4x4x1f32(al.w, bl.w, accl[gq], 0, 0, 0);
      }
      if constexpr (CT > 0) {
        float a[4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt) a[rt] = ws[(16 * rt + r16) * XS + 4 * ks + q4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
            acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[rt], bq[ks][ct], acc[rt][ct], 0, 0, 0);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (c0 + kMfmaChunk < dim) fetch_b_chunk(c0 + kMfmaChunk);
  }
  // transpose to one row per lane: 16-column tiles (D element v of lane (r16, q4) is row
  // 16 rt + 4 q4 + v, column 16 ct + r16), then the 4-column groups (D[i] of lane l is row
  // 4 (l / 4) + i, column l % 4)
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int v = 0; v < 4; ++v) ws[(16 * rt + 4 * q4 + v) * ES + 16 * ct + r16] = acc[rt][ct][v];
#pragma unroll
  for (int gq = 0; gq < NG; ++gq)
#pragma unroll
    for (int i = 0; i < 4; ++i) ws[(4 * (lane >> 2) + i) * ES + 16 * CT + 4 * gq + quad] = accl[gq][i];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  project_rows_epilogue<IS_QUERY, GMAX>(ws + lane * ES, NCOL, lane, row0, nrows, nrows, m, n, g, codes, masks, counts,
                                        ranks, hbmask, nb);
}

// ---------------------------------------------------------------------------------
// 4-6. counting sort of database indices by bucket, per table
// ---------------------------------------------------------------------------------
// Exclusive scan of counts[j][0..nb] in place, three small kernels: per-segment sums
// (1024 entries each), a scan of the segment sums (one workgroup per table), and the
// segment-local scans with the carried offset.
constexpr int kScanSeg = 1024;

__global__ __launch_bounds__(256) void bucket_segsum_kernel(const uint32_t *__restrict__ counts,
                                                            int nb, int nseg,
                                                            uint32_t *__restrict__ segsum) {
  __shared__ uint32_t wsum[4];
  const int j = blockIdx.y, seg = blockIdx.x;
  const uint32_t *c = counts + (size_t)j * (nb + 1);
  uint32_t v = 0;
  for (int e = seg * kScanSeg + threadIdx.x; e < min((seg + 1) * kScanSeg, nb + 1); e += 256) v += c[e];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) segsum[(size_t)j * nseg + seg] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// in-place exclusive scan of segsum[j][0..nseg) (nseg <= 4097 for 2^22 buckets)
__global__ __launch_bounds__(1024) void bucket_segscan_kernel(uint32_t *__restrict__ segsum, int nseg) {
  block_scan_inplace(segsum + (size_t)blockIdx.x * nseg, nseg);
}

__global__ __launch_bounds__(1024) void bucket_scan_kernel(uint32_t *__restrict__ counts, int nb,
                                                           int nseg,
                                                           const uint32_t *__restrict__ segoff) {
  __shared__ uint32_t wsum[16];
  const int j = blockIdx.y, seg = blockIdx.x;
  uint32_t *c = counts + (size_t)j * (nb + 1);
  const int e = seg * kScanSeg + threadIdx.x;
  const uint32_t v = e <= nb ? c[e] : 0u;
  const uint32_t excl = block_scan_excl(v, wsum) + segoff[(size_t)j * nseg + seg];
  if (e <= nb) c[e] = excl;
}

// ---------------------------------------------------------------------------------
// refine helpers: v_sad_u8, the 8-lane sum, the lexicographic distinct top-2, the probe codes
// ---------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sad_u8(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_sad_u8(a, b, c);
}

// sum over the 8 lanes of an aligned lane group (DPP: half-mirror, xor 1, xor 2)
__device__ __forceinline__ uint32_t group8_sum(uint32_t v) {
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141 /*row_half_mirror*/, 0xF, 0xF, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1 /*quad_perm [1,0,3,2]*/, 0xF, 0xF, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E /*quad_perm [2,3,0,1]*/, 0xF, 0xF, true);
  return v;
}

__device__ __forceinline__ void top2_insert_distinct(uint64_t &k1, uint64_t &k2, uint64_t k) {
  if (k == k1 || k == k2) return;  // same database row reached through another table
  if (k < k1) {
    k2 = k1;
    k1 = k;
  } else if (k < k2) {
    k2 = k;
  }
}

// two smallest DISTINCT keys of {a1,a2,b1,b2}
__device__ __forceinline__ void merge_distinct(uint64_t &a1, uint64_t &a2, uint64_t b1, uint64_t b2) {
  const uint64_t lo = a1 < b1 ? a1 : b1;
  uint64_t second = kNone64;
  if (a1 > lo && a1 < second) second = a1;
  if (a2 > lo && a2 < second) second = a2;
  if (b1 > lo && b1 < second) second = b1;
  if (b2 > lo && b2 < second) second = b2;
  a1 = lo;
  a2 = second;
}

// Spread the low bits of v over the set bits of mask (software pdep).
__device__ __forceinline__ uint32_t deposit_bits(uint32_t v, uint32_t mask) {
  uint32_t out = 0;
  while (mask) {
    const uint32_t low = mask & (0u - mask);
    if (v & 1u) out |= low;
    v >>= 1;
    mask ^= low;
  }
  return out;
}

// ---------------------------------------------------------------------------------
// Host side: the launch of the projection a plan names
// ---------------------------------------------------------------------------------
// A projection family's GMAX values: QGs on the query side; the database side has GMAX 1 alone.
template <bool IS_QUERY, int... QGs>
using GMaxes = std::conditional_t<IS_QUERY, Ints<QGs...>, Ints<1>>;

// The plan's projection over the database rows or the query rows.  False if the plan names no
// instantiation.  (The lists descend: the order these kernels have always had in the code object.)
template <bool IS_QUERY>
bool launch_project(const CascadePlan &P, const float *rows, int nrows, int dim, int m, int n, int g,
                    const float *dict, uint32_t *codes, uint32_t *masks, uint8_t *img, uint32_t *counts,
                    uint32_t *ranks, uint32_t hbmask, int nb, hipStream_t stream) {
  if (nrows <= 0) return true;
  const dim3 grid((nrows + P.proj_rows - 1) / P.proj_rows), block(kThreads);
  const int gmax = IS_QUERY ? P.gmax_q : 1;
  auto go = [&](auto kernel, size_t lds) {
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, rows, nrows, dim, m, n, g, dict, codes, masks, img,
                       counts, ranks, hbmask, nb);
    return true;
  };
  if (P.family == 0)
    return pick(Ints<32, 28, 24, 20, 16, 12, 8, 4>{}, P.pa, [&](auto MC) {
      constexpr int mc = decltype(MC)::value;
      return pick(GMaxes<IS_QUERY, 16, 4>{}, gmax, [&](auto G) {
        return go(project_kernel<mc, (mc <= 24 ? 2 : 1), IS_QUERY, decltype(G)::value>, 0);
      });
    });
  if (P.family == 1)
    return pick(Ints<4, 3, 2, 1>{}, P.pa, [&](auto CT) {
      return pick(GMaxes<IS_QUERY, 16, 4, 2>{}, gmax, [&](auto G) {
        constexpr int ct = decltype(CT)::value, gm = decltype(G)::value;
        return P.pb ? go(project_mfma_kernel<ct, IS_QUERY, gm, true>, 0) : go(project_mfma_kernel<ct, IS_QUERY, gm, false>, 0);
      });
    });
  return pick(Ints<3, 2, 1, 0>{}, P.pa, [&](auto CT) {
    return pick(Ints<2, 1>{}, P.pb, [&](auto NG) {
      return pick(GMaxes<IS_QUERY, 16, 2>{}, gmax, [&](auto G) {
        constexpr int ng = decltype(NG)::value;  // the left-over hyperplanes' LDS table [dim/4][4][4] per group
        return go(project_mfma4_kernel<decltype(CT)::value, ng, IS_QUERY, decltype(G)::value>, (size_t)ng * dim * 16);
      });
    });
  });
}

}  // namespace
}  // namespace spv
