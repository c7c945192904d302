// l1k2_batch.hip -- the exact L1 2-NN of l1k2.hip for a collection of (query set, database set) pairs over
// descriptor tables stored back to back, in one main launch.
//
// The single-pair path cuts one pair finely enough to fill the chip by itself: at 10000 x 10000 every workgroup
// loads 64 KB of queries to meet 8 KB of database rows, and the partial keys it writes and re-reads outweigh the
// input.  A collection fills the chip with its pairs, so here
//
//   * blockIdx.x indexes a table of work items in the workspace: 256 Q queries of one pair against one slice of
//     its database set.  An item's fields are workgroup-uniform and live in SGPRs;
//   * the body is l1k2_tile_kernel's: Q query rows per lane in VGPRs, 64-row database tiles through LDS with the
//     register-prefetched double buffer, broadcast ds_read_b128, v_sad_hi_u8 building the dist<<16 | idx16 key,
//     the lazy top-2 (l1k2_tile.h);
//   * an item covers at most 65536 database rows (16-bit local index) and merges its two keys into the out row's
//     pair of 64-bit keys by the two-minimum protocol (top2_atomic_insert): exact and order-independent, keys being
//     unique per database row.  The workspace holds 16 bytes per out row whatever the slice count;
//   * a finish kernel turns the keys into the ABI layout and its sentinels.
//
// Roofline: the issue rate of v_sad_hi_u8, as for l1k2.hip.  See DESIGN.md 4.1b.

#include "common.h"
#include "l1k2_tile.h"

#include <algorithm>

namespace spv {
namespace {

// grid = work items (L1K2Work, l1k2_tile.h); block = 256 threads = 4 waves.  Thread t owns queries q * 256 + t of the item, q = 0..Q-1.
// From the query load to the end of the tile loop this is a copy of l1k2_tile_kernel's body (l1k2.hip), whose code
// must not move with this file's: a change to either is made in both.
template <int D4, int Q>
__global__ __launch_bounds__(kThreads, 3) void l1k2_batch_kernel(const uint4 *__restrict__ desc,
                                                                const L1K2Work *__restrict__ work,
                                                                unsigned long long *keys) {
  constexpr int V4 = D4 / 4;                                   // 16-byte vectors per row
  constexpr int TILE_V4 = kTileRows * V4;                      // vectors per tile
  constexpr int NL = (TILE_V4 + kThreads - 1) / kThreads;      // staging loads per thread
  __shared__ uint4 tile[2][TILE_V4];

  const int t = threadIdx.x;
  const L1K2Work w = work[blockIdx.x];
  const uint4 *x = desc + (size_t)w.x_row0 * V4;
  const uint4 *y = desc + (size_t)w.y_row0 * V4;
  const int row_end = (int)w.x_rows, N = (int)w.y_rows;

  // ---- this lane's queries -> registers
  uint32_t qreg[Q][D4];
  int qi[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    qi[q] = q * kThreads + t;
    const int src = min(qi[q], N - 1);
    const uint4 *yr = y + (size_t)src * V4;
#pragma unroll
    for (int c = 0; c < V4; ++c) {
      const uint4 v = yr[c];
      qreg[q][4 * c + 0] = v.x;
      qreg[q][4 * c + 1] = v.y;
      qreg[q][4 * c + 2] = v.z;
      qreg[q][4 * c + 3] = v.w;
    }
  }
  uint32_t k1[Q], k2[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) k1[q] = k2[q] = kKeyNone;

  // ---- database slice through LDS, register-prefetched double buffer
  uint4 stage[NL];
  auto stage_load = [&](int row0) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int e = t + i * kThreads;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (e < TILE_V4 && row0 + e / V4 < row_end) v = x[(size_t)row0 * V4 + e];
      stage[i] = v;
    }
  };
  auto stage_store = [&](uint4 *dst) {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int e = t + i * kThreads;
      if (e < TILE_V4) dst[e] = stage[i];
    }
  };

  const int ntiles = (row_end + kTileRows - 1) / kTileRows;
  if (ntiles > 0) {
    stage_load(0);
    stage_store(tile[0]);
  }
  __syncthreads();

  for (int tl = 0; tl < ntiles; ++tl) {
    const int row0 = tl * kTileRows;
    const bool has_next = tl + 1 < ntiles;
    if (has_next) stage_load(row0 + kTileRows);

    const int nrows = min(kTileRows, row_end - row0);
    const uint4 *buf = tile[tl & 1];
    const uint32_t jbase = (uint32_t)row0;

    if constexpr (D4 >= 40) {
      // wide rows: NCH chunks per row, the next chunk's LDS reads issued before the current
      // chunk's SAD chain (xa / xb alternate; the last chunk prefetches the next row's first)
      constexpr int NCH = D4 >= 64 ? 4 : 2;
      constexpr int CV = V4 / NCH;
      static_assert(V4 % NCH == 0, "the row must split into NCH chunks of whole 16-byte vectors");
      uint4 xa[CV], xb[CV];
      lds_row<CV>(xa, buf);
      for (int r = 0; r < nrows; ++r) {
        uint32_t acc[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[q] = jbase + r;
        const uint4 *row = buf + r * V4;
        const uint4 *nxt = buf + min(r + 1, kTileRows - 1) * V4;
        lds_row<CV>(xb, row + CV);
        chunk_accumulate<D4, Q, NCH, 0>(qreg, xa, acc);
        if constexpr (NCH == 2) {
          lds_row<CV>(xa, nxt);
          chunk_accumulate<D4, Q, NCH, 1>(qreg, xb, acc);
        } else {
          lds_row<CV>(xa, row + 2 * CV);
          chunk_accumulate<D4, Q, NCH, 1>(qreg, xb, acc);
          lds_row<CV>(xb, row + 3 * CV);
          chunk_accumulate<D4, Q, NCH, 2>(qreg, xa, acc);
          lds_row<CV>(xa, nxt);
          chunk_accumulate<D4, Q, NCH, 3>(qreg, xb, acc);
        }
        lazy_top2<Q>(acc, k1, k2);
      }
    } else {
      // two rows per iteration, next row's LDS reads issued before the current
      // row's SAD chain so the broadcast reads hide behind VALU work
      uint4 xa[V4], xb[V4];
      lds_row<V4>(xa, buf);
      for (int r = 0; r < nrows; r += 2) {
        lds_row<V4>(xb, buf + min(r + 1, kTileRows - 1) * V4);
        row_update<D4, Q>(qreg, xa, jbase + r, k1, k2);
        lds_row<V4>(xa, buf + min(r + 2, kTileRows - 1) * V4);
        if (r + 1 < nrows) row_update<D4, Q>(qreg, xb, jbase + r + 1, k1, k2);
      }
    }

    if (has_next) stage_store(tile[(tl + 1) & 1]);
    __syncthreads();
  }

  // ---- into the out rows' key pairs, which other slices of the same pair merge into as well
  unsigned long long *out = keys + 2 * (((size_t)w.out_hi << 32) | w.out_lo);
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    if (qi[q] < N) {
      unsigned long long *d = out + 2 * (size_t)qi[q];
      top2_atomic_insert(&d[0], &d[1], widen_key(k1[q], w.x_local0));
      top2_atomic_insert(&d[0], &d[1], widen_key(k2[q], w.x_local0));
    }
  }
}

// keys (dist<<32 | idx, or "none") -> the ABI layout, one thread per key: of this file's run and l1k2_guided.hip's.
__global__ __launch_bounds__(kThreads) void l1k2_finish_kernel(const uint64_t *__restrict__ keys, size_t nkeys,
                                                               uint64_t *__restrict__ out_idx,
                                                               int32_t *__restrict__ out_dist) {
  for (size_t e = blockIdx.x * (size_t)kThreads + threadIdx.x; e < nkeys; e += (size_t)gridDim.x * kThreads) {
    const uint64_t k = keys[e];
    const bool none = k == kKey64None;
    out_idx[e] = none ? ~0ull : (k & 0xFFFFFFFFull);
    out_dist[e] = none ? 0x7FFFFFFF : (int32_t)(k >> 32);
  }
}

struct BatchOperands {
  const uint4 *desc;
  const L1K2Work *work;
  unsigned long long *keys;
  unsigned grid;
  hipStream_t stream;
};

// The instantiation of the plan's q: per tile width, the values max_q_for allows.
template <int D4>
bool launch_batch_q(const BatchOperands &o, int q) {
  auto go = [&](auto Q) {
    hipLaunchKernelGGL((l1k2_batch_kernel<D4, decltype(Q)::value>), dim3(o.grid), dim3(kThreads), 0, o.stream, o.desc,
                       o.work, o.keys);
    return true;
  };
  if constexpr (max_q_for(4 * D4) >= 4) return pick(Ints<4, 2, 1>{}, q, go);
  else return pick(Ints<2, 1>{}, q, go);
}

// Planner constants.  kBatchFill: work items that fill the chip, the threshold of l1k2_plan.  Below it every
// database set is cut down to 64-row slices if need be, as a single pair is; from it on a slice is never shorter
// than kBatchTailRows, so that the 256 Q query rows a workgroup loads (64 KB at dim 128) stay under 1/8 of the
// database bytes it meets, and sets are cut only to keep the last round of workgroups short against the run.
constexpr long long kBatchFill = 1024;
constexpr int kBatchTailRows = 4096;
constexpr int kBatchMaxSlice = 65536;  // 16-bit local index

}  // namespace

int l1k2_slice_plan(const long long *seg_off, int nseg, const int32_t *pairs, int npairs, const L1K2SliceRule &rule,
                    L1K2SlicePlan *p) {
  auto rows = [&](int s) { return seg_off[s + 1] - seg_off[s]; };
  auto qblocks = [&](long long n) { return (n + rule.qrows - 1) / rule.qrows; };
  p->total_rows = seg_off[nseg];
  p->out_off = pair_out_off(seg_off, pairs, npairs);
  p->out_rows = p->out_off[npairs];

  // items with whole database sets; every set is then cut `cut` ways, no finer than the rule's floor
  long long whole = 0;
  for (int i = 0; i < npairs; ++i) whole += qblocks(rows(pairs[2 * i]));
  const long long cut = whole > 0 ? std::max<long long>(1, (rule.aim + whole - 1) / whole) : 1;
  const long long floor_rows = whole < rule.fill ? rule.floor_few : rule.floor_full;
  auto slice_rows = [&](long long m) {
    const long long r = ((m + cut - 1) / cut + kTileRows - 1) / kTileRows * kTileRows;
    return std::min(std::max(r, floor_rows), rule.cap);
  };
  long long count = 0;
  p->max_slices = 0;
  for (int i = 0; i < npairs; ++i) {
    const long long m = rows(pairs[2 * i + 1]), r = slice_rows(m);
    const long long slices = std::max<long long>(1, (m + r - 1) / r);
    count += qblocks(rows(pairs[2 * i])) * slices;
    if (rows(pairs[2 * i]) > 0) p->max_slices = (int)std::max<long long>(p->max_slices, slices);
  }
  if (count > 0x7FFFFFFFll) return set_error(SPV_ERR_INVALID, "%lld work items, more than a grid takes", count);
  p->items.clear();
  p->items.reserve((size_t)count);
  for (int i = 0; i < npairs; ++i) {
    const long long n = rows(pairs[2 * i]), m = rows(pairs[2 * i + 1]), r = slice_rows(m);
    for (long long y0 = 0; y0 < n; y0 += rule.qrows)
      for (long long x0 = 0; x0 == 0 || x0 < m; x0 += r)  // an empty database set keeps one item
        p->items.push_back({i, (int32_t)y0, (int32_t)std::min<long long>(rule.qrows, n - y0), (int32_t)x0,
                            (int32_t)std::min(r, m - x0)});
  }
  // longest first: the last round of workgroups is the short items
  std::stable_sort(p->items.begin(), p->items.end(), [](const L1K2BatchItem &a, const L1K2BatchItem &b) {
    return (long long)a.yrows * a.xrows > (long long)b.yrows * b.xrows;
  });
  return SPV_OK;
}

int l1k2_work_upload(const L1K2SlicePlan &p, const long long *seg_off, const int32_t *pairs, void *d_items,
                     unsigned long long *d_keys, hipStream_t stream) {
  std::vector<L1K2Work> work(p.items.size());
  for (size_t e = 0; e < work.size(); ++e) {
    const L1K2BatchItem &it = p.items[e];
    const long long xs = seg_off[pairs[2 * it.pair + 1]], ys = seg_off[pairs[2 * it.pair]];
    const unsigned long long o = (unsigned long long)(p.out_off[it.pair] + it.y0);
    work[e] = {(uint32_t)(xs + it.x0), (uint32_t)it.xrows, (uint32_t)(ys + it.y0), (uint32_t)it.yrows,
               (uint32_t)o,            (uint32_t)(o >> 32), (uint32_t)it.x0,        0u};
  }
  // the one wait of the call: `work` is gone when it returns, so its upload must have ended
  SPV_HIP_CHECK(hipMemcpyWithStream(d_items, work.data(), work.size() * sizeof(L1K2Work), hipMemcpyHostToDevice, stream));
  SPV_HIP_CHECK(hipMemsetAsync(d_keys, 0xFF, (size_t)p.out_rows * 2 * sizeof(uint64_t), stream));  // kKey64None
  return SPV_OK;
}

int l1k2_keys_finish(const char *prof, const unsigned long long *d_keys, long long out_rows, uint64_t *d_idx,
                     int32_t *d_dist, hipStream_t stream) {
  ProfScope prof_merge(prof, stream);
  const size_t nkeys = (size_t)out_rows * 2;
  hipLaunchKernelGGL(l1k2_finish_kernel, dim3((unsigned)std::min<size_t>((nkeys + kThreads - 1) / kThreads, 1u << 20)),
                     dim3(kThreads), 0, stream, reinterpret_cast<const uint64_t *>(d_keys), nkeys, d_idx, d_dist);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

int l1k2_batch_plan(const long long *seg_off, int nseg, int dim, const int32_t *pairs, int npairs, L1K2BatchPlan *out) {
  if (dim <= 0 || dim % 16 != 0)
    return set_error(SPV_ERR_INVALID, "Input matrix inner dimensions must be 16-byte aligned (dim=%d).", dim);
  L1K2BatchPlan p{};
  p.dim_pad = first_at_least(TileWidths{}, dim);
  if (p.dim_pad == 0)
    return set_error(SPV_ERR_INVALID, "dim=%d > 256 is not supported by the many-pairs form of the L1 2-NN", dim);
  if (!seg_off && nseg == 0) seg_off = kNoSets;  // no sets: seg_off may be null
  SPV_TRY(check_collection(seg_off, nseg, pairs, npairs));
  p.padded = p.dim_pad != dim;
  auto rows = [&](int s) { return seg_off[s + 1] - seg_off[s]; };
  auto qblocks = [&](long long n, int q) { return (n + kThreads * q - 1) / (kThreads * q); };

  // as many queries per lane as registers allow, unless that leaves too few workgroups (query blocks x possible
  // database slices, over all pairs) to fill the chip: the rule of l1k2_plan
  int q = max_q_for(p.dim_pad);
  for (; q > 1; q /= 2) {
    long long groups = 0;
    for (int i = 0; i < npairs && groups < kBatchFill; ++i)
      groups += qblocks(rows(pairs[2 * i]), q) * std::max<long long>(1, rows(pairs[2 * i + 1]) / kTileRows);
    if (groups >= kBatchFill) break;
  }
  const L1K2Knobs &knobs = l1k2_knobs();
  if (knobs.q == 1 || knobs.q == 2 || knobs.q == 4) q = std::min(knobs.q, max_q_for(p.dim_pad));
  p.q = q;

  // 256 q queries per item; sets cut SPECTAVI_L1K2_BLOCKS / whole ways, no finer than the floor described above
  SPV_TRY(l1k2_slice_plan(seg_off, nseg, pairs, npairs,
                          {kThreads * q, knobs.blocks, kBatchFill, kTileRows, kBatchTailRows, kBatchMaxSlice}, &p));

  WsWalk w;
  p.off_keys = w.reserve((size_t)p.out_rows * 2 * sizeof(uint64_t));
  p.off_items = w.reserve(p.items.size() * sizeof(L1K2Work));
  p.off_pad = w.reserve(p.padded ? (size_t)p.total_rows * p.dim_pad : 0);
  p.total_bytes = w.end();
  *out = std::move(p);
  return SPV_OK;
}

int l1k2_batch_run(const uint8_t *d_desc, const long long *seg_off, int nseg, int dim, const int32_t *pairs, int npairs,
                   uint64_t *d_idx, int32_t *d_dist, void *d_ws, size_t ws_bytes, hipStream_t stream) {
  L1K2BatchPlan p;
  SPV_TRY(l1k2_batch_plan(seg_off, nseg, dim, pairs, npairs, &p));
  if (p.out_rows == 0) return SPV_OK;
  if (!d_desc || !d_idx || !d_dist || !d_ws) return set_error(SPV_ERR_INVALID, "null device pointer");
  if ((reinterpret_cast<uintptr_t>(d_desc) | reinterpret_cast<uintptr_t>(d_ws)) & 15)
    return set_error(SPV_ERR_INVALID, "device pointers must be 16-byte aligned (desc %p, ws %p)", (const void *)d_desc, d_ws);
  if ((reinterpret_cast<uintptr_t>(d_idx) & 7) || (reinterpret_cast<uintptr_t>(d_dist) & 3))
    return set_error(SPV_ERR_INVALID, "output pointers must be aligned to their element size");
  if (ws_bytes < p.total_bytes) return set_error(SPV_ERR_INVALID, "workspace too small: %zu < %zu", ws_bytes, p.total_bytes);

  uint8_t *ws = static_cast<uint8_t *>(d_ws);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws + p.off_keys);
  SPV_TRY(l1k2_work_upload(p, seg_off, pairs, ws + p.off_items, keys, stream));
  const uint8_t *kdesc = d_desc;
  if (p.padded) {
    l1k2_pad_rows(d_desc, ws + p.off_pad, (size_t)p.total_rows, dim, p.dim_pad, stream);
    kdesc = ws + p.off_pad;
  }
  const BatchOperands o{reinterpret_cast<const uint4 *>(kdesc), reinterpret_cast<const L1K2Work *>(ws + p.off_items), keys,
                        (unsigned)p.items.size(), stream};
  {
    ProfScope prof("l1k2_batch", stream);
    if (!pick(TileWidths{}, p.dim_pad, [&](auto W) { return launch_batch_q<decltype(W)::value / 4>(o, p.q); }))
      return set_error(SPV_ERR_INVALID, "internal: no kernel for dim_pad %d, q %d", p.dim_pad, p.q);
  }
  SPV_HIP_CHECK(hipGetLastError());
  return l1k2_keys_finish("l1k2_batch_merge", keys, p.out_rows, d_idx, d_dist, stream);
}

}  // namespace spv
