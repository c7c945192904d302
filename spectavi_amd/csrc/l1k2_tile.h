// l1k2_tile.h -- the inline pieces of the L1 2-NN tile kernels that l1k2.hip and l1k2_batch.hip share: the packed
// 32-bit key, its SAD chain, the lazy top-2, the 64-bit key of the partial results and the two-minimum protocol
// on a pair of them in memory; and the work record of l1k2_batch.hip and l1k2_guided.hip.  The design they serve is
// described at the top of l1k2.hip.
#pragma once

#include "common.h"

namespace spv {
namespace {

constexpr int kThreads = 256;
constexpr int kTileRows = 64;               // database rows per LDS tile
constexpr uint32_t kKeyNone = 0xFFFFFFFFu;  // > any real key (dist <= 65280)
constexpr uint64_t kKey64None = ~0ull;

// A work item of the many-pairs forms as their kernels read it (l1k2_work_upload packs it): rows of desc (and geom),
// the out row of its first query, and the number of its first database row inside the database set.
struct alignas(32) L1K2Work {
  uint32_t x_row0, x_rows, y_row0, y_rows, out_lo, out_hi, x_local0, unused;
};

__device__ __forceinline__ uint32_t sad_hi(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_sad_hi_u8(a, b, c);  // (SAD_U8(a,b) << 16) + c
}

// Insert key k into the sorted pair (k1 <= k2).  min + med3.
__device__ __forceinline__ void top2_insert(uint32_t &k1, uint32_t &k2, uint32_t k) {
  k2 = max(min(k1, k), min(max(k1, k), k2));  // median of (k1, k, k2) -> v_med3_u32
  k1 = min(k1, k);
}

template <int V4>
__device__ __forceinline__ void lds_row(uint4 (&dst)[V4], const uint4 *row) {
#pragma unroll
  for (int c = 0; c < V4; ++c) dst[c] = row[c];
}

// One chunk of a row, C of NCH (CH4 = D4 / NCH dwords), into the Q accumulators: Q independent chains,
// interleaved so consecutive v_sad_hi_u8 never depend on each other.  Narrow rows are one chunk; wide
// descriptors are consumed in chunks (two for dim 192, four for dim 256) so that only one chunk-sized buffer
// pair is live next to the 2 x D4 query registers (two queries per lane keep the LDS broadcast amortised)
// and the kernel keeps three waves per SIMD.
template <int D4, int Q, int NCH, int C>
__device__ __forceinline__ void chunk_accumulate(const uint32_t (&qreg)[Q][D4],
                                                 const uint4 (&xc)[D4 / NCH / 4], uint32_t (&acc)[Q]) {
  constexpr int CH4 = D4 / NCH;
#pragma unroll
  for (int c = 0; c < CH4 / 4; ++c) {
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = sad_hi(qreg[q][C * CH4 + 4 * c + 0], xc[c].x, acc[q]);
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = sad_hi(qreg[q][C * CH4 + 4 * c + 1], xc[c].y, acc[q]);
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = sad_hi(qreg[q][C * CH4 + 4 * c + 2], xc[c].z, acc[q]);
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = sad_hi(qreg[q][C * CH4 + 4 * c + 3], xc[c].w, acc[q]);
  }
}

// Lazy top-2: a new key enters only if it beats the current second best of its query.  After the first few
// hundred rows of a slice that is rare, so the common case is Q compares and one wave-uniform branch instead
// of Q x (v_min + v_med3).  Result-identical to the eager update.
template <int Q>
__device__ __forceinline__ void lazy_top2(const uint32_t (&acc)[Q], uint32_t (&k1)[Q], uint32_t (&k2)[Q]) {
  bool any = false;
#pragma unroll
  for (int q = 0; q < Q; ++q) any |= acc[q] < k2[q];
  if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
#pragma unroll
    for (int q = 0; q < Q; ++q) top2_insert(k1[q], k2[q], acc[q]);
  }
}

// One whole row xr with tile-local index j against the lane's Q queries.
template <int D4, int Q>
__device__ __forceinline__ void row_update(const uint32_t (&qreg)[Q][D4], const uint4 (&xr)[D4 / 4],
                                           uint32_t j, uint32_t (&k1)[Q], uint32_t (&k2)[Q]) {
  uint32_t acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = j;
  chunk_accumulate<D4, Q, 1, 0>(qreg, xr, acc);
  lazy_top2<Q>(acc, k1, k2);
}

// Partial-key layout: part[(query * S + slice) * 2 + {0,1}], key = dist<<32 | global idx.
__device__ __forceinline__ uint64_t widen_key(uint32_t k, uint32_t slice_base) {
  if (k == kKeyNone) return kKey64None;
  return ((uint64_t)(k >> 16) << 32) | (uint64_t)(slice_base + (k & 0xFFFFu));
}

// The two-minimum protocol of l1k2_prune.hip on a partial pair in memory: old = min(k1, key);
// min(k2, max(old, key)).  "None" never enters.
__device__ __forceinline__ void top2_atomic_insert(unsigned long long *k1, unsigned long long *k2, uint64_t key) {
  if (key == kKey64None) return;
  const unsigned long long old = atomicMin(k1, (unsigned long long)key);
  atomicMin(k2, old > key ? old : (unsigned long long)key);
}

// Row widths in bytes with a tile-kernel instantiation; other dims up to 256 are zero-padded to the next one.
// (They are better off so than in the wide kernel unpadded: measured 0.55-0.80 of the SAD peak on the true
// width against 0.51-0.64, dims 48..240, when only {64, 128, 144, 192, 256} existed.)
using TileWidths = Ints<32, 48, 64, 80, 96, 112, 128, 144, 160, 192, 256>;

// Queries per lane.  Measured on MI355X at 256k x 256k, D=128 (tools/l1k2_sweep.py): Q=2
// (154 VGPRs, 3 waves/SIMD) beats Q=4 (224 VGPRs, 2 waves/SIMD) by ~3 % and Q=1 by ~15 %.
// Wide rows (192 / 256) also take Q=2: with one query per lane the broadcast LDS reads, not
// the SADs, bound the kernel (0.66 of the SAD peak measured at Q=1).
constexpr int max_q_for(int dim_pad) { return dim_pad <= 64 ? 4 : 2; }

}  // namespace
}  // namespace spv
