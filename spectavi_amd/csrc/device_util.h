// device_util.h -- device helpers the kernel files share (gfx950: 64-lane waves).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spv {

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int mask) {
  const uint32_t lo = __shfl_xor((uint32_t)v, mask, 64);
  const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), mask, 64);
  return ((uint64_t)hi << 32) | lo;
}

// Inclusive scan of v over the 64 lanes of a wave.
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// Exclusive scan of v over the 1024 lanes of a workgroup, lane t = threadIdx.x; wsum: 16 shared words that no lane
// still reads from an earlier use.  One barrier.
template <typename T>
__device__ __forceinline__ T block_scan_excl(T v, T *wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const T incl = wave_scan_incl(v, lane);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  T woff = 0;
  for (int k = 0; k < w; ++k) woff += wsum[k];
  return woff + incl - v;
}

// In-place exclusive scan of c[0..n) by one workgroup of 1024 lanes, 1024 entries at a time with a carry.
// Returns the sum of all entries to every lane.
template <typename T>
__device__ __forceinline__ T block_scan_inplace(T *c, int n) {
  __shared__ T wsum[16];
  __shared__ T carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int e = base + t;
    const T v = e < n ? c[e] : 0;
    const T excl = block_scan_excl(v, wsum) + carry;  // (carry is only written between the two barriers below)
    if (e < n) c[e] = excl;
    __syncthreads();
    if (t == 1023) carry = excl + v;
    __syncthreads();
  }
  return carry;
}

}  // namespace spv
