// l1k2_guided.hip -- the exact L1 2-NN of a collection of (query set, database set) pairs, searched for each query
// only among the database keypoints that lie within max_dist of the query's line (its epipolar line, or the scan
// line of a rectified pair), and the small kernel that turns per-pair matrices into those lines.
//
// The band holds a fraction of a percent of the pairs, so the kernel does not mask an all-pairs SAD: it decides
// every (query, database row) pair with two v_fma_f64 and one compare and pays the 32 v_sad_u8 only for the hits.
//
//   * blockIdx.x indexes a table of work items in the workspace, as in l1k2_batch.hip: 256 queries of one pair, one
//     per lane, against one slice of its database set.  An item's fields are workgroup-uniform and live in SGPRs;
//   * the lane keeps the line (l0, l1, l2) of its query in six VGPRs; the workgroup's query rows stay in LDS;
//   * database tiles of 64 rows stream through LDS with l1k2_batch.hip's register-prefetched double buffer.  A
//     tile is the 128-byte rows and, beside them, the rows' (u, v) widened to fp64 when they are staged, so a pair
//     costs one broadcast ds_read_b128 (amortised over the wave), two v_fma_f64 and one v_cmp_le_f64 with the abs
//     modifier; rows past the slice's end are staged as NaN and are nobody's candidate.  Four rows are decided per
//     wave-uniform branch;
//   * hits are lane-divergent and rare: they are balloted and appended as (query of the wave << 6 | row of the tile)
//     to the wave's queue in LDS, which is drained whenever it holds 64 entries (one pair per lane) and at the end
//     of the tile, before the buffer is reused (eight lanes per pair for up to kOctetMax entries).  A drained key
//     dist << 32 | row of the database set enters the query's top-2 in LDS by the two-minimum protocol;
//   * at the end of the item the two keys merge into the out row's pair of 64-bit keys in the workspace
//     (top2_atomic_insert, l1k2_tile.h), exact and order-independent because a key is unique per database row, and
//     the lane's hit count goes to ncand with one atomic add; a finish kernel writes idx, dist and the sentinels.
//
// drain_lanes and drain_octets are l1k2_prune.hip's, restated here with this file's LDS arrays: that file's
// instruction stream is pinned by its ISA test and must not move with this one's.  A change to the protocol is
// made in both.
//
// Budget (tests/test_l1k2_guided_isa.py): 56320 bytes of LDS, two workgroups = two waves per SIMD on a CU, which
// allows 256 VGPRs; no scratch.  Measurements and the planner's constants: DESIGN.md 4.1c.

#include "common.h"
#include "l1k2_tile.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace spv {
namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kRowV4 = 8;      // 16-byte vectors of a 128-byte row
constexpr int kRowBits = 6;    // a queue entry: query of the wave << kRowBits | row of the tile
constexpr int kQueue = 128;    // < 64 queued, then <= 64 appended in one round
constexpr int kOctetMax = 16;  // most entries the end-of-tile drain takes eight lanes per pair for
static_assert(kTileRows == 1 << kRowBits && kTileRows % 8 == 0, "a queue entry holds a tile row in kRowBits bits");

// LDS accesses of one wave are executed in order; this keeps the compiler from moving them
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// The newest n <= 64 entries of the wave's queue, one pair per lane: both rows from LDS in 16-byte pieces, each
// lane starting at a piece of its own so that the 64 rows, which all begin on bank 0, are not read through the
// same four banks.  qslot: the wave's first query among the workgroup's; row0: the tile's first row in the set.
__device__ __forceinline__ void drain_lanes(int n, int &cnt, int lane, const uint16_t *queue, int qslot, const uint4 *qraw,
                                            const uint4 *xr, unsigned long long *k1s, unsigned long long *k2s, uint32_t row0) {
  wave_lds_fence();
  const int base = cnt - n;
  if (lane < n) {
    const uint32_t e = queue[base + lane];
    const int q6 = e >> kRowBits, i = e & ((1 << kRowBits) - 1);
    const uint4 *qa = qraw + (qslot + q6) * kRowV4, *xa = xr + i * kRowV4;
    const unsigned long long k2now = k2s[qslot + q6];
    uint32_t d = 0;
    uint4 a[kRowV4], b[kRowV4];
#pragma unroll
    for (int k = 0; k < kRowV4; ++k) {
      const int j = (k + lane) & 7;
      a[k] = qa[j];
      b[k] = xa[j];
    }
#pragma unroll
    for (int k = 0; k < kRowV4; ++k) {
      d = __builtin_amdgcn_sad_u8(a[k].x, b[k].x, d);
      d = __builtin_amdgcn_sad_u8(a[k].y, b[k].y, d);
      d = __builtin_amdgcn_sad_u8(a[k].z, b[k].z, d);
      d = __builtin_amdgcn_sad_u8(a[k].w, b[k].w, d);
    }
    // a key that does not beat the query's second best of this moment never will (k2 only falls)
    const unsigned long long key = ((unsigned long long)d << 32) | (row0 + i);
    if (key < k2now) {
      const unsigned long long old = atomicMin(&k1s[qslot + q6], key);
      atomicMin(&k2s[qslot + q6], old > key ? old : key);
    }
  }
  cnt = base;
  wave_lds_fence();
}

// The same for few entries, eight lanes per pair and eight pairs per round: lane 8 o + j holds piece j of octet
// o's two rows, four v_sad_u8 and three DPP adds give every lane of the octet the distance, and the octet's first
// lane does the key compare and the two minima.  All lanes stay active (octets past the last pair repeat it and
// store nothing): the DPP adds read their neighbours.
__device__ __forceinline__ void drain_octets(int n, int &cnt, int lane, const uint16_t *queue, int qslot, const uint4 *qraw,
                                             const uint4 *xr, unsigned long long *k1s, unsigned long long *k2s, uint32_t row0) {
  wave_lds_fence();
  const int base = cnt - n;
  const int oct = lane >> 3, piece = lane & 7;
  for (int r = 0; r < n; r += 8) {
    const int j = r + oct;
    const uint32_t e = queue[base + min(j, n - 1)];
    const int q6 = e >> kRowBits, i = e & ((1 << kRowBits) - 1);
    const uint4 a = qraw[(qslot + q6) * kRowV4 + piece], b = xr[i * kRowV4 + piece];
    const unsigned long long k2now = k2s[qslot + q6];
    uint32_t d = __builtin_amdgcn_sad_u8(a.x, b.x, 0u);
    d = __builtin_amdgcn_sad_u8(a.y, b.y, d);
    d = __builtin_amdgcn_sad_u8(a.z, b.z, d);
    d = __builtin_amdgcn_sad_u8(a.w, b.w, d);
    d += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)d, 0xB1, 0xF, 0xF, false);   // quad_perm [1,0,3,2]
    d += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)d, 0x4E, 0xF, 0xF, false);   // quad_perm [2,3,0,1]
    d += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)d, 0x141, 0xF, 0xF, false);  // row_half_mirror: the other quad
    const unsigned long long key = ((unsigned long long)d << 32) | (row0 + i);
    if (piece == 0 && j < n && key < k2now) {
      const unsigned long long old = atomicMin(&k1s[qslot + q6], key);
      atomicMin(&k2s[qslot + q6], old > key ? old : key);
    }
  }
  cnt = base;
  wave_lds_fence();
}

// grid = work items; block = 256 threads = 4 waves.  Thread t owns query t of the item; wave w owns the top-2
// slots and the queue of queries 64 w .. 64 w + 63, so nothing but the tiles is shared between waves.
__global__ __launch_bounds__(kThreads, 2) void l1k2_guided_kernel(const uint4 *__restrict__ desc,
                                                                 const float4 *__restrict__ geom,
                                                                 const L1K2Work *__restrict__ work,
                                                                 const double *__restrict__ lines, double max_dist,
                                                                 unsigned long long *keys, int *ncand) {
  constexpr int TILE_V4 = kTileRows * kRowV4;
  constexpr int NL = TILE_V4 / kThreads;  // staging loads per thread
  static_assert(TILE_V4 % kThreads == 0 && kTileRows <= kThreads, "the staging below");
  __shared__ uint4 s_q[kThreads * kRowV4];   // the workgroup's query rows
  __shared__ uint4 s_x[2][TILE_V4];          // the tile's database rows, double buffered
  __shared__ double2 s_uv[2][kTileRows];     // ... and their keypoints in fp64
  __shared__ unsigned long long s_k1[kThreads], s_k2[kThreads];
  __shared__ uint16_t s_queue[kWaves][kQueue];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const L1K2Work w = work[blockIdx.x];
  const uint4 *x = desc + (size_t)w.x_row0 * kRowV4;
  const float4 *xg = geom + w.x_row0;
  const int row_end = (int)w.x_rows, N = (int)w.y_rows;
  const size_t out0 = ((size_t)w.out_hi << 32) | w.out_lo;

  // ---- the queries: rows to LDS, the lane's line to registers (NaN past the last query: no candidates)
#pragma unroll
  for (int i = 0; i < kRowV4; ++i) {
    const int e = t + i * kThreads;
    s_q[e] = e / kRowV4 < N ? desc[(size_t)w.y_row0 * kRowV4 + e] : make_uint4(0, 0, 0, 0);
  }
  const double nan = __builtin_nan("");
  double l0 = nan, l1 = nan, l2 = nan;
  if (t < N) {
    const double *l = lines + 3 * (out0 + t);
    l0 = l[0];
    l1 = l[1];
    l2 = l[2];
  }
  // the line has arrived before the tile loop: a wait for it inside the loop would also wait for the next tile's
  // staging loads, which are then in flight
  asm volatile("" : "+v"(l0), "+v"(l1), "+v"(l2));
  s_k1[t] = s_k2[t] = kKey64None;
  int mine = 0;  // candidates of this lane's query
  int cnt = 0;   // entries in the wave's queue

  // ---- database slice through LDS, register-prefetched double buffer
  uint4 stage[NL];
  float2 stage_uv = make_float2(0.f, 0.f);
  auto stage_load = [&](int row0) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int e = t + i * kThreads;
      stage[i] = row0 + e / kRowV4 < row_end ? x[(size_t)row0 * kRowV4 + e] : make_uint4(0, 0, 0, 0);
    }
    if (t < kTileRows && row0 + t < row_end) {
      const float4 g = xg[row0 + t];
      stage_uv = make_float2(g.x, g.y);
    }
  };
  auto stage_store = [&](int b, int row0) {
#pragma unroll
    for (int i = 0; i < NL; ++i) s_x[b][t + i * kThreads] = stage[i];
    if (t < kTileRows) {
      const bool in = row0 + t < row_end;
      s_uv[b][t] = make_double2(in ? (double)stage_uv.x : nan, in ? (double)stage_uv.y : nan);
    }
  };

  const int ntiles = (row_end + kTileRows - 1) / kTileRows;
  if (ntiles > 0) {
    stage_load(0);
    stage_store(0, 0);
  }
  __syncthreads();

  uint16_t *queue = s_queue[wv];
  const int qslot = wv * 64;
  for (int tl = 0; tl < ntiles; ++tl) {
    const int row0 = tl * kTileRows;
    const bool has_next = tl + 1 < ntiles;
    if (has_next) stage_load(row0 + kTileRows);

    const int b = tl & 1;
    const int nrows = min(kTileRows, row_end - row0);
    const uint32_t jbase = w.x_local0 + (uint32_t)row0;
    const double2 *uv = s_uv[b];
    // four rows per step, the next step's broadcast reads issued before this step's arithmetic; two steps per
    // iteration so that the two register sets swap roles without a copy (rows past nrows are NaN: no hits)
    auto step = [&](int r, const double2 (&p)[4], double2 (&ahead)[4]) {
      const double2 *next = uv + min(r + 4, kTileRows - 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) ahead[k] = next[k];
      // a v_cmp's result is the ballot: the masks stay in SGPRs and the common case is three s_or and one branch
      bool hit[4];
      unsigned long long m[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        hit[k] = fabs(fma(l0, p[k].x, fma(l1, p[k].y, l2))) <= max_dist;
        m[k] = __builtin_amdgcn_ballot_w64(hit[k]);
      }
      if ((m[0] | m[1] | m[2] | m[3]) == 0ull) return;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (m[k] == 0ull) continue;
        if (hit[k]) {
          const int at = cnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m[k] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m[k], 0u));
          queue[at] = (uint16_t)((lane << kRowBits) | (r + k));
          ++mine;
        }
        cnt += __popcll(m[k]);
        if (cnt >= 64) drain_lanes(64, cnt, lane, queue, qslot, s_q, s_x[b], s_k1, s_k2, jbase);
      }
    };
    double2 pa[4], pb[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) pa[k] = uv[k];
    for (int r = 0; r < nrows; r += 8) {
      step(r, pa, pb);
      step(r + 4, pb, pa);
    }
    if (cnt > kOctetMax) drain_lanes(cnt, cnt, lane, queue, qslot, s_q, s_x[b], s_k1, s_k2, jbase);
    else if (cnt > 0) drain_octets(cnt, cnt, lane, queue, qslot, s_q, s_x[b], s_k1, s_k2, jbase);

    if (has_next) stage_store(b ^ 1, row0 + kTileRows);
    __syncthreads();
  }

  // ---- into the out rows' key pairs, which other slices of the same pair merge into as well
  wave_lds_fence();
  if (t < N) {
    unsigned long long *d = keys + 2 * (out0 + t);
    top2_atomic_insert(&d[0], &d[1], s_k1[t]);
    top2_atomic_insert(&d[0], &d[1], s_k2[t]);
    if (ncand && mine) atomicAdd(&ncand[out0 + t], mine);
  }
}

// ---- lines: out row r of a pair, query keypoint (u, v), gets G (u, v, 1)^T over hypot(l0, l1), or three NaNs.
// A launch takes the pairs of one chunk by value; blockIdx.y is the pair of the chunk.
struct LinesPair {
  double g[9];
  long long geom_row0, out_row0, rows;
};
constexpr int kLinesChunk = 32;
struct LinesChunk {
  LinesPair p[kLinesChunk];
};
static_assert(sizeof(LinesChunk) <= 3584, "kernel arguments are limited to 4 KB");

__global__ __launch_bounds__(kThreads) void epipolar_lines_kernel(const float4 *__restrict__ geom, const LinesChunk c,
                                                                  double *__restrict__ lines) {
  const LinesPair &p = c.p[blockIdx.y];
  const double nan = __builtin_nan("");
  for (long long r = blockIdx.x * (long long)kThreads + threadIdx.x; r < p.rows; r += (long long)gridDim.x * kThreads) {
    const float4 k = geom[p.geom_row0 + r];
    const double u = k.x, v = k.y;
    const double l0 = p.g[0] * u + p.g[1] * v + p.g[2];
    const double l1 = p.g[3] * u + p.g[4] * v + p.g[5];
    const double l2 = p.g[6] * u + p.g[7] * v + p.g[8];
    const double n = hypot(l0, l1);
    const bool ok = n > 0.0 && n < std::numeric_limits<double>::infinity();
    double *o = lines + 3 * (p.out_row0 + r);
    o[0] = ok ? l0 / n : nan;
    o[1] = ok ? l1 / n : nan;
    o[2] = ok ? l2 / n : nan;
  }
}

// Planner constants.  kGuidedFill: work items that fill the chip, two workgroups on each of 256 CUs.  A collection
// with that many query blocks runs whole database sets (the row number in a key is 32 bits wide, so no set is too
// long for an item); below it every database set is cut until the items fill the chip, but never below
// kGuidedMinSlice rows: the 32 KB of query rows a workgroup loads then stay at or under the database bytes it meets.
constexpr long long kGuidedFill = 512;
constexpr int kGuidedMinSlice = 256;

}  // namespace

int l1k2_guided_plan(const long long *seg_off, int nseg, int dim, const int32_t *pairs, int npairs, L1K2GuidedPlan *out) {
  if (dim != 128) return set_error(SPV_ERR_INVALID, "the guided L1 2-NN takes dim 128 only (dim=%d)", dim);
  if (!seg_off && nseg == 0 && npairs == 0) seg_off = kNoSets;  // nothing at all: seg_off may be null
  SPV_TRY(check_collection(seg_off, nseg, pairs, npairs));
  L1K2GuidedPlan p{};
  // 256 queries per item; one floor whatever the item count; no cap, the row number in a key being 32 bits wide
  SPV_TRY(l1k2_slice_plan(seg_off, nseg, pairs, npairs,
                          {kThreads, kGuidedFill, 0, kGuidedMinSlice, kGuidedMinSlice, std::numeric_limits<long long>::max()},
                          &p));

  WsWalk w;
  p.off_keys = w.reserve((size_t)p.out_rows * 2 * sizeof(uint64_t));
  p.off_items = w.reserve(p.items.size() * sizeof(L1K2Work));
  p.total_bytes = w.end();
  *out = std::move(p);
  return SPV_OK;
}

int l1k2_guided_run(const uint8_t *d_desc, const float *d_geom, const long long *seg_off, int nseg, int dim,
                    const int32_t *pairs, int npairs, const double *d_lines, double max_dist, uint64_t *d_idx,
                    int32_t *d_dist, int32_t *d_ncand, void *d_ws, size_t ws_bytes, hipStream_t stream) {
  L1K2GuidedPlan p;
  SPV_TRY(l1k2_guided_plan(seg_off, nseg, dim, pairs, npairs, &p));
  if (p.out_rows == 0) return SPV_OK;
  if (!d_desc || !d_geom || !d_lines || !d_idx || !d_dist || !d_ws) return set_error(SPV_ERR_INVALID, "null device pointer");
  if ((reinterpret_cast<uintptr_t>(d_desc) | reinterpret_cast<uintptr_t>(d_geom) | reinterpret_cast<uintptr_t>(d_ws)) & 15)
    return set_error(SPV_ERR_INVALID, "device pointers must be 16-byte aligned (desc %p, geom %p, ws %p)", (const void *)d_desc,
                     (const void *)d_geom, d_ws);
  if ((reinterpret_cast<uintptr_t>(d_idx) & 7) || (reinterpret_cast<uintptr_t>(d_lines) & 7) ||
      (reinterpret_cast<uintptr_t>(d_dist) & 3) || (reinterpret_cast<uintptr_t>(d_ncand) & 3))
    return set_error(SPV_ERR_INVALID, "lines and output pointers must be aligned to their element size");
  if (ws_bytes < p.total_bytes) return set_error(SPV_ERR_INVALID, "workspace too small: %zu < %zu", ws_bytes, p.total_bytes);

  uint8_t *ws = static_cast<uint8_t *>(d_ws);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws + p.off_keys);
  SPV_TRY(l1k2_work_upload(p, seg_off, pairs, ws + p.off_items, keys, stream));
  if (d_ncand) SPV_HIP_CHECK(hipMemsetAsync(d_ncand, 0, (size_t)p.out_rows * sizeof(int32_t), stream));
  {
    ProfScope prof("l1k2_guided", stream);
    hipLaunchKernelGGL(l1k2_guided_kernel, dim3((unsigned)p.items.size()), dim3(kThreads), 0, stream,
                       reinterpret_cast<const uint4 *>(d_desc), reinterpret_cast<const float4 *>(d_geom),
                       reinterpret_cast<const L1K2Work *>(ws + p.off_items), d_lines, max_dist, keys, d_ncand);
  }
  SPV_HIP_CHECK(hipGetLastError());
  return l1k2_keys_finish("l1k2_guided_merge", keys, p.out_rows, d_idx, d_dist, stream);
}

int epipolar_lines_run(const float *d_geom, const long long *seg_off, int nseg, const int32_t *pairs, int npairs,
                       const double *G, const int32_t *use, double *d_lines, hipStream_t stream) {
  if (nseg == 0 && npairs == 0) return SPV_OK;
  SPV_TRY(check_collection(seg_off, nseg, pairs, npairs));
  long long out_rows = 0;
  for (int i = 0; i < npairs; ++i) out_rows += seg_off[pairs[2 * i] + 1] - seg_off[pairs[2 * i]];
  if (out_rows == 0) return SPV_OK;
  if (!G || !d_geom || !d_lines) return set_error(SPV_ERR_INVALID, "null pointer");
  if ((reinterpret_cast<uintptr_t>(d_geom) & 15) || (reinterpret_cast<uintptr_t>(d_lines) & 7))
    return set_error(SPV_ERR_INVALID, "geom must be 16-byte aligned and lines 8-byte");

  ProfScope prof("epipolar_lines", stream);
  long long out_row = 0;
  for (int i0 = 0; i0 < npairs; i0 += kLinesChunk) {
    LinesChunk c{};
    long long most = 0;
    const int n = std::min(kLinesChunk, npairs - i0);
    for (int k = 0; k < n; ++k) {
      const int i = i0 + k, q = pairs[2 * i];
      LinesPair &lp = c.p[k];
      for (int e = 0; e < 9; ++e) lp.g[e] = (use && !use[i]) ? std::numeric_limits<double>::quiet_NaN() : G[9 * (size_t)i + e];
      lp.geom_row0 = seg_off[q];
      lp.out_row0 = out_row;
      lp.rows = seg_off[q + 1] - seg_off[q];
      out_row += lp.rows;
      most = std::max(most, lp.rows);
    }
    if (most == 0) continue;
    hipLaunchKernelGGL(epipolar_lines_kernel, dim3((unsigned)std::min<long long>((most + kThreads - 1) / kThreads, 4096), (unsigned)n),
                       dim3(kThreads), 0, stream, reinterpret_cast<const float4 *>(d_geom), c, d_lines);
    SPV_HIP_CHECK(hipGetLastError());
  }
  return SPV_OK;
}

}  // namespace spv
