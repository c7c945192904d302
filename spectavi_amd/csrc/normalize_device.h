// normalize_device.h -- the device arithmetic of normalize_to_ubyte_and_multiple_16_dim that the single-table form
// (adapter.hip) and the many-tables form (normalize_batch.hip) share: the per-element expression and the row-ordered
// walk of a 16-column block.  Stated once, so both forms give the same bits by construction.
#pragma once

#include <hip/hip_runtime.h>

namespace spv {

// out = clip(rint((x - mean) / norm * 128), -128, 127): numpy's float32 arithmetic, round half to even.  A NaN
// (0 / 0: a constant column, a one-row table) passes both comparisons and stays NaN.
__device__ __forceinline__ float normalize_value(float x, float mean, float norm) {
  float v = (x - mean) / norm * 128.f;
  v = rintf(v);  // numpy round: half to even
  if (v > 127.f) v = 127.f;
  if (v < -128.f) v = -128.f;
  return v;
}
// ... and its uint8 image, (out + 128).astype('uint8')
__device__ __forceinline__ unsigned char normalize_ubyte(float v) { return (unsigned char)((int)(v + 128.f)); }

constexpr int kStatCols = 16;   // columns per workgroup: one 64-byte sector of every float32 row
constexpr int kStatRows = 512;  // rows per LDS tile (double buffered: 2 x 32 KB)
constexpr int kStatThreads = 320;

// One workgroup of five waves on one block of 16 columns of x = T[rows, dim] (T = float, or uint8_t whose values
// stand for their float32 conversions).  Waves 1..4 (256 lanes) stream the block's row tiles into LDS,
// register-prefetched one tile ahead, and fold max / min of what they load (order-independent).  Wave 0 does
// nothing but the serial per-column chains, lanes 0..15, over the tile the loaders finished in the previous
// round: s += v in row order (float32, exactly numpy's order), its LDS reads issued one 16-row batch ahead of the
// adds so the chain runs at the dependent-add rate.  One barrier per tile; the loaders' round (LDS writes +
// issuing the next prefetch) hides behind the chain's.
// stats[0][c] = mean = sum / rows, stats[1][c] = norm = max(max - mean, -(min - mean)) for the block's columns c
// (stats is float[2][dim]).
// rows >= 1; called by all kStatThreads threads of the workgroup.  The 64 KB of LDS tiles are this function's own: an
// array handed in through a pointer reaches the loop optimisations as generic memory, and the chain loses its unrolling.
template <typename T>
__device__ __forceinline__ void column_stats_block(const T *__restrict__ x, int rows, int dim, int block,
                                                   float *__restrict__ stats) {
  __shared__ float tile[2][kStatRows * kStatCols];  // [row][column]
  constexpr int NL = kStatRows * kStatCols / 256;   // 32 floats per loader lane per tile
  const int t = threadIdx.x;
  const bool loader = t >= 64;
  const int lt = t - 64;
  const int c0 = block * kStatCols;
  const int ncol = min(kStatCols, dim - c0);
  const int col = lt & 15, rsub = lt >> 4;  // loader lane -> (column, row within a group of 16 rows)
  const int ntiles = (rows + kStatRows - 1) / kStatRows;
  float pre[NL];
  float s = 0.f, mx = -__builtin_inff(), mn = __builtin_inff();
  const int colc = min(col, ncol - 1);
  auto prefetch = [&](int row0) {  // clamped addresses, raw values: nothing here waits for the loads
#pragma unroll
    for (int i = 0; i < NL; ++i)
      pre[i] = (float)x[(size_t)min(row0 + rsub + 16 * i, rows - 1) * dim + c0 + colc];
  };
  auto publish = [&](int tl) {  // registers -> LDS tile tl, folding max / min on the way
    float *buf = tile[tl & 1];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      // rows past the end and columns past the block become +0 (bitwise, so the load above
      // stays unconditional and the 32 of them stay in flight together)
      const bool live = tl * kStatRows + rsub + 16 * i < rows && col < ncol;
      const float v = __uint_as_float(__float_as_uint(pre[i]) & (live ? 0xFFFFFFFFu : 0u));
      buf[(rsub + 16 * i) * kStatCols + col] = v;
      mx = live ? fmaxf(mx, v) : mx;
      mn = live ? fminf(mn, v) : mn;
    }
  };
  if (loader && ntiles > 0) {
    prefetch(0);
    publish(0);
    if (ntiles > 1) prefetch(kStatRows);
  }
  __syncthreads();
  for (int tl = 0; tl < ntiles; ++tl) {
    if (loader) {
      // tile tl + 1 goes into the buffer the chain finished with before the last barrier
      if (tl + 1 < ntiles) {
        publish(tl + 1);
        if (tl + 2 < ntiles) prefetch((tl + 2) * kStatRows);
      }
    } else if (t < kStatCols) {
      // rows past the end of the input were published as +0, which leaves a float32 sum
      // unchanged, so every tile is walked in full: 16 batches of 32 rows, no conditionals.
      // The scheduling barriers pin "reads of the next half-batch, then adds of this one".
      const float *buf = tile[tl & 1] + t;
      float va[16], vb[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) va[k] = buf[k * kStatCols];
      for (int r = 0; r < kStatRows; r += 32) {
#pragma unroll
        for (int k = 0; k < 16; ++k) vb[k] = buf[(r + 16 + k) * kStatCols];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 16; ++k) s += va[k];  // strictly in row order
        __builtin_amdgcn_sched_barrier(0);
        const int rn = (r + 32) & (kStatRows - 1);  // the last round re-reads rows 0..15, unused
#pragma unroll
        for (int k = 0; k < 16; ++k) va[k] = buf[(rn + k) * kStatCols];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 16; ++k) s += vb[k];
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
  }
  // combine the 16 row-groups' max / min per column
  float *red = tile[0];
  if (loader) {
    red[lt] = mx;
    red[256 + lt] = mn;
  }
  __syncthreads();
  if (t < ncol) {
    float cmx = red[t], cmn = red[256 + t];
    for (int k = 1; k < 16; ++k) {
      cmx = fmaxf(cmx, red[16 * k + t]);
      cmn = fminf(cmn, red[256 + 16 * k + t]);
    }
    const float mean = s / (float)rows;
    stats[c0 + t] = mean;
    stats[dim + c0 + t] = fmaxf(cmx - mean, -(cmn - mean));
  }
}

}  // namespace spv
