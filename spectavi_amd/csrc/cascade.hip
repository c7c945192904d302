// cascade.hip -- cascade-hash candidate prefilter + exact L1 refine for gfx950 (MI355X).
//
// Replaces reference CascadingHashNn (src/CascadingHashNn.h:86-245) behind
// nn_cascading_hash (src/Spectavi.cpp:321-336).  The reference builds
// unordered_map<code, list<idx>> buckets on the host, and per query unions the
// buckets of 2^g multi-probe codes per table into an unordered_set that feeds
// the L1 brute force as a candidate filter.  Here everything is flat arrays in
// HBM and these kernels:
//
//   1 repack_dict     dict[n][dim][m] -> dictp[n][dim][MC], MC = roundup(m,4), zero padded
//   2 project<false>  database rows: n*m random-hyperplane projections (on the matrix cores
//                     when n*m <= 64, project_mfma_kernel; else the VALU project_kernel) as a
//                     dim-ordered fp32 FMA chain (the oracle runs the identical
//                     chain, so sign bits match bit for bit), sign-packed codes
//                     (bit b set iff proj >= 0, src/CascadingHashNn.h:102-111), the
//                     uint8 refine image  u8 = (int(trunc v) + 128) & 255
//                     (src/CascadingHashNn.h:236-239) and the bucket histogram
//   3 project<true>   query rows: sign code + mask of the g least-confident bits
//                     (smallest (|proj|, bit) pairs, src/CascadingHashNn.h:150-160)
//                     + uint8 image
//   4 bucket_segsum / segscan / scan, 5 bucket_fill   counting sort of database
//                     indices by bucket = code & (2^HB - 1), per table
//   6 probe_table     one launch per table, one 8-lane group per query (8 queries per wave), the
//                     queries walked in the order of that table's sign code (a second counting
//                     sort, large inputs only) so that a bucket's rows stay in the XCD's L2: 2^g
//                     probe codes (src/CascadingHashNn.h:170-179) -> bucket ranges -> the group's
//                     candidate list in LDS -> per round each group gathers one 128-byte
//                     candidate row (8 different queries' lines per wave instruction), v_sad_u8 +
//                     DPP reduce, branch-free two smallest (dist, idx) keys carried from table
//                     to table
//   7 probe_refine    one wave per query (the first design, issue-bound): used when
//                     kernel 6 does not apply -- full-code check (m > 22) or rows wider
//                     than 256 bytes (up to 2048)
//
// Which instantiation of 2, 3, 6 and 7 runs for a shape is decided in one host function,
// cascade_plan (after the kernels), from the shape and the SPECTAVI_CASCADE_MFMA / MFMA4 / GROUP /
// QHIST / SORT / RU environment; cascade_run launches what the plan names and spv_cascade_plan exports it.
//
// Candidate semantics (closed form of filter_potential_neighbours, :208-227):
// database row k is a candidate of query i iff for some table j
//   ((code_j(x_k) ^ sign_j(y_i)) & ~mask_j(y_i)) == 0.
// The reference visits the candidate set in unordered_set order, so its
// tie-break on equal distance is unspecified; here the result is the two
// smallest (dist, idx) pairs of the candidate set, lexicographic.
//
// Kernels 1-4 and the refine helpers are in cascade_kernels.h, which cascade_batch.hip (the many-pairs form)
// includes as well.

#include "cascade_kernels.h"

#include <algorithm>
#include <cstdlib>

namespace spv {
namespace {

// ---------------------------------------------------------------------------------
// 4-6. counting sort of database indices by bucket, per table (the scan kernels: cascade_kernels.h)
// ---------------------------------------------------------------------------------
// Histogram + ranks of the QUERY sign codes, per table, for the VALU projection path (the
// matrix-core epilogue has it fused): what the probe's query order is built from.
__global__ __launch_bounds__(256) void query_rank_kernel(const uint32_t *__restrict__ codes, int N, int n,
                                                         uint32_t hbmask, int nb, uint32_t *__restrict__ counts,
                                                         uint32_t *__restrict__ ranks) {
  const size_t total = (size_t)n * N;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
    const size_t j = e / N;
    ranks[e] = atomicAdd(&counts[j * (nb + 1) + (codes[e] & hbmask)], 1u);
  }
}

__global__ void bucket_fill_kernel(const uint32_t *__restrict__ codes,
                                   const uint32_t *__restrict__ ranks, int M, int n, uint32_t hbmask,
                                   int nb, const uint32_t *__restrict__ bstart,
                                   uint32_t *__restrict__ order) {
  const size_t total = (size_t)n * M;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total;
       e += (size_t)gridDim.x * blockDim.x) {
    const int j = (int)(e / M);
    const uint32_t idx = (uint32_t)(e - (size_t)j * M);
    const uint32_t pos = bstart[(size_t)j * (nb + 1) + (codes[e] & hbmask)] + ranks[e];
    order[(size_t)j * M + pos] = idx;
  }
}

// ---------------------------------------------------------------------------------
// 7. probe + gather + refine, one wave per query
// ---------------------------------------------------------------------------------
// CPL: 16-byte chunks of the row per lane of an 8-lane group (dim <= 128*CPL);
// RU: rounds of 8 candidate rows in flight per wave
template <int CPL, int RU>
__global__ __launch_bounds__(kThreads) void probe_refine_kernel(
    const uint8_t *__restrict__ ux, const uint8_t *__restrict__ uy, int M, int N, int dim, int m,
    int n, int g, int hb, const uint32_t *__restrict__ xcodes, const uint32_t *__restrict__ ysign,
    const uint32_t *__restrict__ ymask, const uint32_t *__restrict__ bstart,
    const uint32_t *__restrict__ order,
    uint64_t *__restrict__ out_idx, float *__restrict__ out_dist, int32_t *__restrict__ out_ncand) {
  __shared__ uint32_t lists[kThreads / 64][kListCap];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  // one query per wave
  auto process_query = [&](const int query) {
  uint32_t *list = lists[wave];
  const int sub = lane & 7;    // chunk owner inside the 8-lane group
  const int grp = lane >> 3;   // candidate slot 0..7
  const int nchunk = dim / 16;
  const uint32_t nb = 1u << hb;
  const uint32_t hbmask = nb - 1;
  const bool check_code = m > hb;

  // this lane's share of the query row
  uint4 qv[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const int ch = sub + 8 * c;
    qv[c] = ch < nchunk ? *reinterpret_cast<const uint4 *>(uy + (size_t)query * dim + 16 * ch)
                        : make_uint4(0, 0, 0, 0);
  }

  uint64_t k1 = kNone64, k2 = kNone64;
  int visited = 0;

  auto refine = [&](int count) {
    // `count` candidate indices in list[0..count).  Each 8-lane group takes one candidate
    // per round (8 rows = 8 full 128-byte lines per wave instruction); four rounds of row
    // gathers are issued before the first is consumed so the random-row latency overlaps.
    for (int c0 = 0; c0 < count; c0 += 8 * RU) {
      uint4 xv[RU][CPL];
      uint32_t cand[RU];
      bool live[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const int ci = c0 + 8 * u + grp;
        live[u] = ci < count;
        cand[u] = list[live[u] ? ci : 0];
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
          const int ch = sub + 8 * c;
          xv[u][c] = make_uint4(0, 0, 0, 0);
          if (live[u] && ch < nchunk)
            xv[u][c] = *reinterpret_cast<const uint4 *>(ux + (size_t)cand[u] * dim + 16 * ch);
        }
      }
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        uint32_t d = 0;
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
          d = sad_u8(qv[c].x, xv[u][c].x, d);
          d = sad_u8(qv[c].y, xv[u][c].y, d);
          d = sad_u8(qv[c].z, xv[u][c].z, d);
          d = sad_u8(qv[c].w, xv[u][c].w, d);
        }
        d = group8_sum(d);
        if (live[u]) top2_insert_distinct(k1, k2, ((uint64_t)d << 32) | cand[u]);
      }
    }
  };

  const int nvar = 1 << g;
  const int nprobe = n * nvar;
  // lanes per probe: with few probes (n * 2^g = 8 by default) several lanes share one
  // bucket and copy it cooperatively
  int lpp = 1;
  while (lpp * 2 * nprobe <= 64) lpp *= 2;
  const int ppc = 64 / lpp;  // probes per pass of the wave
  for (int p0 = 0; p0 < nprobe; p0 += ppc) {
    const int p = p0 + lane / lpp;
    const int psub = lane % lpp;
    uint32_t s = 0, len = 0, pcode = 0;
    int tj = 0;
    if (p < nprobe) {
      tj = p >> g;
      const uint32_t var = (uint32_t)(p & (nvar - 1));
      const uint32_t sg = ysign[(size_t)tj * N + query];
      const uint32_t mk = ymask[(size_t)tj * N + query];
      pcode = (sg & ~mk) | deposit_bits(var, mk);
      const uint32_t *bs = bstart + (size_t)tj * (nb + 1) + (pcode & hbmask);
      s = bs[0];
      len = bs[1] - s;
    }
    // exclusive offsets of the buckets in the list: scan over the first lane of each probe
    const uint32_t mylen = psub == 0 ? len : 0u;
    const uint32_t incl = wave_scan_incl(mylen, lane);
    const uint32_t total = __shfl(incl, 63, 64);
    if (!check_code && total <= (uint32_t)kListCap) {
      // fast path: the lanes of a probe copy its bucket into the shared list
      const uint32_t dst = __shfl(incl - mylen, lane - psub, 64);
      const uint32_t *src = order + (size_t)tj * M + s;
      for (uint32_t i = psub; i < len; i += lpp) list[dst + i] = src[i];
      __builtin_amdgcn_wave_barrier();
      refine((int)total);
      visited += (int)total;
      __builtin_amdgcn_wave_barrier();
    } else {
      // general path: buckets one at a time, 64 entries per step, optional full-code check
      const int np = min(ppc, nprobe - p0);
      for (int pp = 0; pp < np; ++pp) {
        const uint32_t ps = __shfl(s, pp * lpp, 64);
        const uint32_t pl = __shfl(len, pp * lpp, 64);
        const uint32_t pc = __shfl(pcode, pp * lpp, 64);
        const int pj = __shfl(tj, pp * lpp, 64);
        for (uint32_t off = 0; off < pl; off += 64) {
          const uint32_t e = off + lane;
          bool keep = e < pl;
          uint32_t cand = 0;
          if (keep) {
            cand = order[(size_t)pj * M + ps + e];
            if (check_code) keep = xcodes[(size_t)pj * M + cand] == pc;
          }
          const unsigned long long bal = __ballot(keep);
          const int pos = __popcll(bal & ((1ull << lane) - 1ull));
          if (keep) list[pos] = cand;
          const int cnt = __popcll(bal);
          __builtin_amdgcn_wave_barrier();
          refine(cnt);
          visited += cnt;
          __builtin_amdgcn_wave_barrier();
        }
      }
    }
  }

  // argmin-2 butterfly over the 8 lane groups (keys are uniform inside a group)
#pragma unroll
  for (int msk = 8; msk < 64; msk <<= 1) {
    const uint64_t b1 = shfl_xor_u64(k1, msk);
    const uint64_t b2 = shfl_xor_u64(k2, msk);
    merge_distinct(k1, k2, b1, b2);
  }
  if (lane == 0) {
    const bool n1 = k1 == kNone64, n2 = k2 == kNone64;
    out_idx[2 * (size_t)query + 0] = n1 ? ~0ull : (k1 & 0xFFFFFFFFull);
    out_idx[2 * (size_t)query + 1] = n2 ? ~0ull : (k2 & 0xFFFFFFFFull);
    // int -> float as reference src/CascadingHashNn.h:244; sentinel INT_MAX -> 2147483648.0f
    out_dist[2 * (size_t)query + 0] = n1 ? 2147483648.0f : (float)(uint32_t)(k1 >> 32);
    out_dist[2 * (size_t)query + 1] = n2 ? 2147483648.0f : (float)(uint32_t)(k2 >> 32);
    if (out_ncand) out_ncand[query] = visited;
  }
  };  // process_query

  const int nwaves = gridDim.x * (kThreads / 64);
  const int wave_id = blockIdx.x * (kThreads / 64) + wave;
  for (int query = wave_id; query < N; query += nwaves) process_query(query);
}


// ---------------------------------------------------------------------------------
// 7b. group-per-query probe + refine, one table per launch: one 8-lane group per query, 8 queries
// per wave, 32 per workgroup.  The one-wave-per-query kernel above spends ~1100 wave instructions
// per query and is issue-bound; here every wave instruction serves 8 queries: lane s of a group owns
// probe s of each round of 8 probes (the default 2^g is 4), the group lays the probed buckets'
// entries out in a private LDS list, and in every round each group gathers ONE candidate row
// (8 lanes x 16 bytes = one 128-byte line, 8 different queries' lines per wave instruction),
// v_sad_u8 + DPP sum, branch-free top-2.  All 8 lanes of a group hold the same keys, so no
// cross-lane merge is needed at the end.  A round whose candidate stream is longer than 128
// entries is processed in several windows of the list.
//
// Round 3: the kernel runs once per TABLE, over the queries in the order of that table's sign code
// (counting sort fused into the query projection like the database's), with the query blocks dealt
// so that the blocks sharing an XCD (b % 8 under the dispatcher's round-robin; speed only) walk one
// contiguous eighth of the sorted order: the ~7.6 queries of a bucket, and the queries of the
// buckets one low bit away, are then in flight together on one XCD and find that bucket's rows in
// its L2 instead of gathering them again over the fabric (1M x 1M: FETCH_SIZE 13.3 -> 3.7 GB per
// step, L2 hit rate 5 -> 60 %, profiles/r03_cascade_pmc.md).  Between the passes a query's two best
// keys and its candidate count wait in `partial` / `pvisited`; the last pass writes the ABI outputs.
// Small inputs skip the sort (qorder = NULL, input order) but still go table by table.  Results do
// not depend on the order of the queries or of the tables: the two smallest distinct keys.
//
// That made the kernel issue-bound (SQ_INSTS_VALU 2 800 per wave and pass = 0.57 of the pass's
// 0.64 ms), so the instruction count per candidate went from ~54 to ~30:
//   * keys ordered by v_min_f64 / v_max_f64: a key (distance << 32 | index) is a positive double
//     whose order is the integer order of its bits (distances < 2^20: denormals, which the f64 units
//     keep), "none" = the largest finite double; the top-2 network is 3 instructions instead of
//     3 x (v_cmp_u64 + 2 v_cndmask) + hazard nops;
//   * "same row again" (a row reached through an earlier table, or twice when nan projections
//     leave a query with fewer than g probe bits) is a 32-bit index comparison with the two kept rows
//     at insertion instead of two 64-bit key comparisons;
//   * the candidate list of a round of probes is filled flat: list position p finds its bucket by a
//     packed byte comparison against the 8 bucket offsets (4 instructions) and loads its entry, four
//     independent loads per lane in flight -- rounds 1-2 walked the buckets one by one, one dependent
//     global load per 8 entries, every one of those round trips serial;
//   * four list entries per ds_read_b128; row addresses as a uniform base + 32-bit shifted offset
//     (dim a power of two, the image below 4 GiB) instead of two v_mad_u64_u32 per row; unconditional
//     loads (row 0 / entry 0 for the slots past the end) instead of an exec-mask branch per load;
//   * RU = 8 (rows of up to 128 bytes): eight rows in flight per group, and instead of all eight lanes
//     reducing every candidate's eight partial sums (3 DPP adds each) a transposing butterfly leaves
//     lane s with the whole sum of candidate s (7 DPP adds + 14 selects per 8 candidates); each lane
//     keeps the best two of ITS candidates, the eight pairs are merged once at the end of the pass
//     (equal keys = the same row, counted once).  ~12 instructions per candidate.
// ---------------------------------------------------------------------------------
constexpr uint64_t kNoneD = 0x7FEFFFFFFFFFFFFFull;

__device__ __forceinline__ uint64_t key_min(uint64_t a, uint64_t b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(__longlong_as_double((long long)a)), "v"(__longlong_as_double((long long)b)));
  return (uint64_t)__double_as_longlong(r);
}
__device__ __forceinline__ uint64_t key_max(uint64_t a, uint64_t b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(__longlong_as_double((long long)a)), "v"(__longlong_as_double((long long)b)));
  return (uint64_t)__double_as_longlong(r);
}

// (k1 <= k2) of this lane and of the lane CTRL pairs it with -> the two smallest distinct keys of the four
template <int CTRL>
__device__ __forceinline__ void merge_keys_with(uint64_t &k1, uint64_t &k2) {
  const uint64_t o1 = ((uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(k1 >> 32), CTRL, 0xF, 0xF, true) << 32) |
                      (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)k1, CTRL, 0xF, 0xF, true);
  const uint64_t o2 = ((uint64_t)(uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(k2 >> 32), CTRL, 0xF, 0xF, true) << 32) |
                      (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)k2, CTRL, 0xF, 0xF, true);
  const uint64_t lo = key_min(k1, o1);
  uint64_t mid = key_max(k1, o1);
  if (mid == lo) mid = kNoneD;
  k2 = key_min(mid, key_min(k2, o2));
  k1 = lo;
}

template <int CPL, int RU, int WPE, bool SHIFT, bool FULL>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void probe_table_kernel(
    const uint8_t *__restrict__ ux, const uint8_t *__restrict__ uy, int M, int N, int dim, int dshift, int g, int hb,
    const uint32_t *__restrict__ ysign,   // [N] sign codes of THIS table
    const uint32_t *__restrict__ ymask,   // [N]
    const uint32_t *__restrict__ bstart,  // [2^hb + 1] bucket offsets of this table
    const uint32_t *__restrict__ order,   // [M] database rows grouped by bucket
    const uint32_t *__restrict__ qorder,  // [N] queries in this pass's order, or NULL (identity)
    int nblk, int per_xcd,                // query blocks; blocks per XCD range (0: block b takes slot block b)
    uint64_t *__restrict__ partial, int32_t *__restrict__ pvisited, int first_pass, int last_pass,
    uint64_t *__restrict__ out_idx, float *__restrict__ out_dist, int32_t *__restrict__ out_ncand) {
  constexpr int CAP = 128;
  static_assert(RU == 4 || RU == 8, "list entries come four per ds_read_b128");
  __shared__ __attribute__((aligned(16))) uint32_t lists[kThreads / 8][CAP];
  __shared__ __attribute__((aligned(16))) uint32_t gtab[kThreads / 8][16];  // [0..7] bucket offsets, [8..15] start - offset
  const int t = threadIdx.x;
  const int sub = t & 7;
  int slotblk = blockIdx.x;
  if (per_xcd > 0) {
    slotblk = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    if (slotblk >= nblk) return;  // whole workgroup (nothing below synchronises across waves)
  }
  const int slot = slotblk * (kThreads / 8) + (t >> 3);
  const bool valid = slot < N;
  const int sq = valid ? slot : N - 1;  // keep every lane alive for the cross-lane ops
  const int q = qorder ? (int)qorder[sq] : sq;
  uint32_t *list = lists[t >> 3];
  uint32_t *tab = gtab[t >> 3];
  const int nchunk = dim / 16;
  const uint32_t hbmask = (1u << hb) - 1;
  const int nvar = 1 << g;

  uint4 qv[CPL];
#pragma unroll
  for (int c = 0; c < CPL; ++c) {
    const int ch = sub + 8 * c;
    qv[c] = ch < nchunk ? *reinterpret_cast<const uint4 *>(uy + (size_t)q * dim + 16 * ch)
                        : make_uint4(0, 0, 0, 0);
  }
  const uint32_t sg = ysign[q], mk = ymask[q];
  uint64_t k1 = kNoneD, k2 = kNoneD;
  int visited = 0;
  if (!first_pass) {
    k1 = partial[2 * (size_t)q];
    k2 = partial[2 * (size_t)q + 1];
    visited = pvisited[q];
  }

  for (int p0 = 0; p0 < nvar; p0 += 8) {
    // lane `sub` owns probe p0 + sub of this round
    const int p = p0 + sub;
    uint32_t s = 0, len = 0;
    if (p < nvar) {
      const uint32_t pcode = (sg & ~mk) | deposit_bits((uint32_t)p, mk);
      const uint32_t *bs = bstart + (pcode & hbmask);
      s = bs[0];
      len = bs[1] - s;
    }
    // exclusive offsets of the 8 buckets inside the round's candidate stream
    uint32_t incl = len;
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) {
      const uint32_t o = __shfl_up(incl, d, 8);
      if (sub >= d) incl += o;
    }
    const uint32_t total = __shfl(incl, 7, 8);
    const uint32_t excl = incl - len;
    visited += (int)total;
    tab[sub] = excl;
    tab[8 + sub] = s - excl;  // entry of stream position x of this bucket: order[x + (s - excl)]
    __builtin_amdgcn_wave_barrier();
    // the stream [0, total) is processed in windows of CAP entries (one almost always)
    for (uint32_t w0 = 0; __any(w0 < total); w0 += CAP) {
      const uint32_t T = w0 < total ? min((uint32_t)CAP, total - w0) : 0u;
      // bucket offsets relative to the window, clamped to [0, 128], one byte each
      uint32_t thrA, thrB;
      {
        const uint4 ea = *reinterpret_cast<const uint4 *>(tab), eb = *reinterpret_cast<const uint4 *>(tab + 4);
        auto rel = [&](uint32_t e) { return (uint32_t)min(max((int)(e - w0), 0), 128); };
        thrA = rel(ea.x) | (rel(ea.y) << 8) | (rel(ea.z) << 16) | (rel(ea.w) << 24);
        thrB = rel(eb.x) | (rel(eb.y) << 8) | (rel(eb.z) << 16) | (rel(eb.w) << 24);
      }
      // (not unrolled: unrolled, the sixteen lane-constant positions and their byte-replicated forms
      // were hoisted out of every loop and held 31 VGPRs through the gather loop -- 88 in all, five
      // waves per SIMD)
#pragma unroll 1
      for (int it = 0; it < 4; ++it) {  // 32 list positions per step, four independent loads per lane
        if (!__any(T > 32u * it)) break;
        uint32_t ent[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const uint32_t pos = (uint32_t)sub + 8u * (4 * it + i);  // < 128
          // bucket of position pos: the last one whose offset is <= pos.  Per byte, bit 7 of
          // 0x80 + pos - offset is set iff offset <= pos (pos <= 127, offset <= 128: no borrow)
          const uint32_t rep = (pos * 0x01010101u) | 0x80808080u;
          const uint32_t cnt = __builtin_popcount((rep - thrA) & 0x80808080u) + __builtin_popcount((rep - thrB) & 0x80808080u);
          const uint32_t delta = tab[8 + ((cnt - 1) & 7)];
          // unconditional load (entry 0 for the positions past the end): no exec-mask branch per entry
          ent[i] = order[pos < T ? delta + w0 + pos : 0u];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) list[sub + 8 * (4 * it + i)] = ent[i];
      }
      __builtin_amdgcn_wave_barrier();
      if constexpr (RU == 8) {
        // Eight candidate rows per round; afterwards lane s of the group OWNS candidate s: the eight
        // partial sums of the eight lanes are reduced by a transposing butterfly (7 DPP adds + 14
        // selects per 8 candidates instead of 3 DPP adds per candidate), and the top-2 update runs once
        // per lane and round on that lane's candidate.  The lanes' pairs are merged after the last round.
        const bool up4 = (sub & 4) != 0, up2 = (sub & 2) != 0, up1 = (sub & 1) != 0;
        for (uint32_t f0 = 0; __any(f0 < T); f0 += 8) {
          const uint32_t fb = f0 < T ? f0 : 0u;
          const uint4 ca = *reinterpret_cast<const uint4 *>(list + fb);
          const uint4 cb = *reinterpret_cast<const uint4 *>(list + fb + 4);
          const uint32_t cand[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
          const uint32_t mine = list[fb + sub];
          uint4 xv[8][CPL];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const uint32_t row = f0 + u < T ? cand[u] : 0u;  // slots past the end gather row 0, dropped below
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
              const int ch = sub + 8 * c;
              const int chc = FULL ? ch : min(ch, nchunk - 1);
              if (SHIFT) {
                const uint32_t off = (row << dshift) + 16u * (uint32_t)chc;
                xv[u][c] = *reinterpret_cast<const uint4 *>(ux + off);
              } else {
                xv[u][c] = *reinterpret_cast<const uint4 *>(ux + (size_t)row * dim + 16 * chc);
              }
              if (!FULL && ch >= nchunk) xv[u][c] = make_uint4(0, 0, 0, 0);
            }
          }
          uint32_t d[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            d[u] = 0;
#pragma unroll
            for (int c = 0; c < CPL; ++c) {
              d[u] = sad_u8(qv[c].x, xv[u][c].x, d[u]);
              d[u] = sad_u8(qv[c].y, xv[u][c].y, d[u]);
              d[u] = sad_u8(qv[c].z, xv[u][c].z, d[u]);
              d[u] = sad_u8(qv[c].w, xv[u][c].w, d[u]);
            }
          }
          // lanes i and 7 - i exchange halves (upper lanes keep candidates 4..7), then i and i ^ 2, then
          // i and i ^ 1: lane i ends with the whole sum of candidate i
          uint32_t e[4], f[2];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t keep = up4 ? d[j + 4] : d[j], send = up4 ? d[j] : d[j + 4];
            e[j] = keep + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send, 0x141 /*row_half_mirror*/, 0xF, 0xF, true);
          }
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const uint32_t keep = up2 ? e[j + 2] : e[j], send = up2 ? e[j] : e[j + 2];
            f[j] = keep + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send, 0x4E /*quad_perm [2,3,0,1]*/, 0xF, 0xF, true);
          }
          const uint32_t keep = up1 ? f[1] : f[0], send = up1 ? f[0] : f[1];
          const uint32_t dsum = keep + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)send, 0xB1 /*quad_perm [1,0,3,2]*/, 0xF, 0xF, true);
          const bool dead = !(f0 + (uint32_t)sub < T) || mine == (uint32_t)k1 || mine == (uint32_t)k2;
          const uint64_t k = dead ? kNoneD : (((uint64_t)dsum << 32) | mine);
          const uint64_t hi = key_max(k, k1);
          k1 = key_min(k, k1);
          k2 = key_min(hi, k2);
        }
      } else
      // rounds: one candidate row per group per round, RU rounds in flight
      for (uint32_t f0 = 0; __any(f0 < T); f0 += RU) {
        const uint4 c4 = *reinterpret_cast<const uint4 *>(list + (f0 < T ? f0 : 0u));
        const uint32_t cand[RU] = {c4.x, c4.y, c4.z, c4.w};
        uint4 xv[RU][CPL];
        bool live[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          live[u] = f0 + u < T;
          // the slots past the end of the list gather row 0 (unconditional loads: no exec-mask branch
          // per row; at most RU - 1 such rows per window, L2 hits) and are dropped at insertion
          const uint32_t row = live[u] ? cand[u] : 0u;
#pragma unroll
          for (int c = 0; c < CPL; ++c) {
            // FULL: the row fills all 8 * CPL chunks (dim 128, 256); otherwise the lanes past the row's
            // end re-read its last chunk and are zeroed (their query chunk is zero too)
            const int ch = sub + 8 * c;
            const int chc = FULL ? ch : min(ch, nchunk - 1);
            if (SHIFT) {
              const uint32_t off = (row << dshift) + 16u * (uint32_t)chc;
              xv[u][c] = *reinterpret_cast<const uint4 *>(ux + off);
            } else {
              xv[u][c] = *reinterpret_cast<const uint4 *>(ux + (size_t)row * dim + 16 * chc);
            }
            if (!FULL && ch >= nchunk) xv[u][c] = make_uint4(0, 0, 0, 0);
          }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          uint32_t d = 0;
#pragma unroll
          for (int c = 0; c < CPL; ++c) {
            d = sad_u8(qv[c].x, xv[u][c].x, d);
            d = sad_u8(qv[c].y, xv[u][c].y, d);
            d = sad_u8(qv[c].z, xv[u][c].z, d);
            d = sad_u8(qv[c].w, xv[u][c].w, d);
          }
          d = group8_sum(d);
          // a row that already holds a place (an earlier table's pass, or a bucket probed twice)
          // would only repeat its own key
          const bool dead = !live[u] || cand[u] == (uint32_t)k1 || cand[u] == (uint32_t)k2;
          const uint64_t k = dead ? kNoneD : (((uint64_t)d << 32) | cand[u]);
          const uint64_t hi = key_max(k, k1);
          k1 = key_min(k, k1);
          k2 = key_min(hi, k2);
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    __builtin_amdgcn_wave_barrier();
  }

  if constexpr (RU == 8) {
    // the eight lanes' pairs -> the group's pair (every lane ends with it).  Equal keys are the same
    // row (the carried pair every lane started from, a row met again): counted once.
    merge_keys_with<0x141>(k1, k2);  // i <-> 7 - i
    merge_keys_with<0x4E>(k1, k2);   // i <-> i ^ 2
    merge_keys_with<0xB1>(k1, k2);   // i <-> i ^ 1
  }
  if (valid && sub == 0) {
    if (!last_pass) {
      partial[2 * (size_t)q] = k1;
      partial[2 * (size_t)q + 1] = k2;
      pvisited[q] = visited;
    } else {
      const bool n1 = k1 == kNoneD, n2 = k2 == kNoneD;
      out_idx[2 * (size_t)q + 0] = n1 ? ~0ull : (k1 & 0xFFFFFFFFull);
      out_idx[2 * (size_t)q + 1] = n2 ? ~0ull : (k2 & 0xFFFFFFFFull);
      out_dist[2 * (size_t)q + 0] = n1 ? 2147483648.0f : (float)(uint32_t)(k1 >> 32);
      out_dist[2 * (size_t)q + 1] = n2 ? 2147483648.0f : (float)(uint32_t)(k2 >> 32);
      if (out_ncand) out_ncand[q] = visited;
    }
  }
}

// ---------------------------------------------------------------------------------
// Host side: the plan -- every choice between kernels, made once from the shape and the knobs -- and
// the launches it names
// ---------------------------------------------------------------------------------

// The SPECTAVI_CASCADE_* environment, read on every call (tests switch SORT inside one process).
// MFMA=0, MFMA4=0, GROUP=0 and QHIST=0 turn a form off where the shape would take it (A/B runs; each
// forces a form that other shapes select anyway); SORT=0 / 1 forces the sorted probe off / on; RU=2
// halves the rows in flight of the wave-per-query probe at rows of up to 128 bytes.
struct CascadeKnobs {
  bool mfma, mfma4, group, qhist, ru2;
  int sort;  // -1: by size
};

CascadeKnobs cascade_knobs() {
  auto first = [](const char *name) {
    const char *e = getenv(name);
    return e ? e[0] : '\0';
  };
  const char sort = first("SPECTAVI_CASCADE_SORT");
  return {first("SPECTAVI_CASCADE_MFMA") != '0', first("SPECTAVI_CASCADE_MFMA4") != '0',
          first("SPECTAVI_CASCADE_GROUP") != '0', first("SPECTAVI_CASCADE_QHIST") != '0',
          first("SPECTAVI_CASCADE_RU") == '2', sort == '0' || sort == '1' ? sort - '0' : -1};
}

}  // namespace

CascadePlan cascade_plan(int xrows, int yrows, int dim, int m, int n, int g) {
  const CascadeKnobs K = cascade_knobs();
  CascadePlan P{};
  P.mc = (m + 3) / 4 * 4;  // accumulators per table: multiples of 4 (one ds_read_b128 each)
  P.hb = bucket_bits(m);
  const size_t nb1 = ((size_t)1 << P.hb) + 1;
  WsWalk w(nullptr, 16);  // no piece shorter than 16 bytes
  P.off_dictp = w.reserve((size_t)n * dim * P.mc * sizeof(float));
  P.off_dictm = w.reserve((size_t)(dim + 16) * 64 * sizeof(float));  // MFMA layout, at most 64 columns, rows padded to a multiple of 32
  P.off_ux = w.reserve((size_t)xrows * dim);
  P.off_uy = w.reserve((size_t)yrows * dim);
  P.off_xcodes = w.reserve((size_t)n * xrows * sizeof(uint32_t));
  P.off_ysign = w.reserve((size_t)n * yrows * sizeof(uint32_t));
  P.off_ymask = w.reserve((size_t)n * yrows * sizeof(uint32_t));
  P.off_bstart = w.reserve((size_t)2 * n * nb1 * sizeof(uint32_t));  // [n] database tables, then [n] query tables (one scan)
  P.off_order = w.reserve((size_t)n * xrows * sizeof(uint32_t));
  P.off_ranks = w.reserve((size_t)n * xrows * sizeof(uint32_t));
  P.off_segsum = w.reserve((size_t)2 * n * ((nb1 + kScanSeg - 1) / kScanSeg) * sizeof(uint32_t));
  // the probe's per-table query order (counting sort of the queries by sign code) and what a
  // query carries from one table's pass to the next
  P.off_qbstart = P.off_bstart + (size_t)n * nb1 * sizeof(uint32_t);
  P.off_qorder = w.reserve((size_t)n * yrows * sizeof(uint32_t));
  P.off_qranks = w.reserve((size_t)n * yrows * sizeof(uint32_t));
  P.off_partial = w.reserve((size_t)yrows * 2 * sizeof(uint64_t));
  P.off_pvisited = w.reserve((size_t)yrows * sizeof(int32_t));
  P.total = w.end();

  // Projection: on the matrix cores when the n*m hyperplanes fit 64 columns, else on the VALU.
  const long long nm = (long long)n * m;
  const bool on_mfma = K.mfma && nm <= 64;
  const bool whole_chunks = dim % kMfmaChunk == 0;
  const int left = (int)(nm % 16);
  if (on_mfma && K.mfma4 && whole_chunks && dim <= 512 && left >= 1 && left <= 8) {
    // 1..8 columns beyond whole 16-column tiles (the default 2 x 17): left-over columns on 4x4x1 MFMAs
    P.family = 2;
    P.pa = (int)(nm / 16);
    P.pb = (left + 3) / 4;
    P.gmax_q = g <= 2 ? 2 : 16;
  } else if (on_mfma) {
    P.family = 1;
    P.pa = (int)((nm + 15) / 16);
    P.pb = whole_chunks;
    P.gmax_q = g <= 2 ? 2 : g <= 4 ? 4 : 16;
  } else {
    // Two tables per pass (rows read from HBM once, an odd last pass included) while 2 x MC
    // accumulators fit the register budget (MC <= 24), with one row per lane: 0.47 ms for 1M + 1M
    // rows; measured alternatives: one table per pass 0.54 ms; two rows per lane 0.58 (one table) /
    // 0.65 (two tables) -- its 77 KB of LDS per workgroup halve the occupancy.
    P.family = 0;
    P.pa = P.mc;
    P.pb = P.mc <= 24 ? 2 : 1;
    P.gmax_q = g <= 4 ? 4 : 16;
  }
  P.proj_rows = P.family == 0 ? kProjTile : kThreads;

  // Probe: the group-per-query kernel unless the full-code check is needed (m > bucket bits) or rows
  // are wider than 256 bytes; otherwise the wave-per-query kernel.  The group kernel walks the
  // queries table by table in the order of that table's sign code when the input is large enough for
  // the order to matter (the per-table counting sorts and passes cost a dozen small launches).
  const int cpl = (dim / 16 + 7) / 8;
  P.use_group = K.group && m <= P.hb && cpl <= 2;
  P.sorted = P.use_group && xrows > 0 && (K.sort >= 0 ? K.sort == 1 : (n <= 8 && (long long)yrows >= 65536));
  // query histogram + ranks: fused into the matrix-core projection's epilogue (+0.05 ms on the query
  // pass at 1M rows: every wave ends on the round trip of its returning atomics) or, with QHIST=0
  // and always on the VALU path, a kernel of their own after it (+0.10 ms)
  P.qhist_fused = P.sorted && K.qhist && P.family != 0;
  if (P.use_group) {
    while ((1 << P.dshift) < dim) ++P.dshift;
    P.nblk = (yrows + kThreads / 8 - 1) / (kThreads / 8);
    P.per_xcd = P.sorted ? (P.nblk + 7) / 8 : 0;
    P.probe_grid = P.sorted ? 8 * P.per_xcd : P.nblk;
    if (cpl == 1) {
      // rows of up to 128 bytes: eight rows in flight per group, lane s owning candidate s after the
      // transposing reduce (69 VGPRs, seven waves per SIMD): 0.90 ms per 1M queries against 0.98 for
      // four rows in flight with every lane reducing every candidate (59 VGPRs, eight waves;
      // profiles/r03_cascade_variants.txt has the earlier builds)
      P.cpl = 1, P.ru = 8, P.wpe = 7;
      // row offsets by shift: dim 16, 32, 64 and SIFT's 128 (FULL: the benchmark's shape), unless
      // the image has 4 GiB or more; by multiplication at dim 48, 80, 96, 112
      P.shift = (1 << P.dshift) == dim && (unsigned long long)xrows * (unsigned)dim < (1ull << 32);
      P.full = P.shift && dim == 128;
    } else {
      P.cpl = 2, P.ru = 4, P.wpe = 6;  // dim 144 .. 256 (80 VGPRs)
    }
  } else {
    P.probe_grid = (yrows + kThreads / 64 - 1) / (kThreads / 64);
    // rows up to 128, 256, 512, 1024 and 2048 bytes, the widest the L1 kernels take as well
    P.cpl = cpl <= 2 ? cpl : cpl <= 4 ? 4 : cpl <= 8 ? 8 : 16;
    // RU=2 at rows of up to 128 bytes: 1.16 ms against 1.32 for 1M x 1M, m = 24 on uniform rows (1.1
    // candidates per query; RU 8 took 1.94 and is gone): profiles/r10_cascade_ru_ab.txt
    P.ru = P.cpl == 1 && K.ru2 ? 2 : P.cpl <= 2 ? 4 : P.cpl == 4 ? 2 : 1;
  }
  return P;
}

size_t cascade_workspace_bytes(int xrows, int yrows, int dim, int m, int n, int g) {
  return cascade_plan(xrows, yrows, dim, m, n, g).total;
}

int cascade_run(const float *d_x, const float *d_y, int xrows, int yrows, int dim, int m, int n,
                int g, const float *d_dict, uint64_t *d_idx, float *d_dist, int32_t *d_ncand,
                void *d_ws, size_t ws_bytes, hipStream_t stream) {
  if (yrows == 0) return SPV_OK;
  if (!d_y || !d_dict || !d_idx || !d_dist || (xrows > 0 && !d_x))
    return set_error(SPV_ERR_INVALID, "null device pointer");
  if (g > 16) return set_error(SPV_ERR_INVALID, "num_candidate_neighbours g=%d > 16", g);
  // before anything is enqueued: rows wider than the refine kernels take, misaligned bases
  if (dim > kCascadeMaxDim)
    return set_error(SPV_ERR_INVALID, "dim=%d > %d is not supported by the cascade refine kernel", dim,
                     kCascadeMaxDim);
  if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_y) |
       reinterpret_cast<uintptr_t>(d_dict) | reinterpret_cast<uintptr_t>(d_ws)) & 15)
    return set_error(SPV_ERR_INVALID, "device pointers must be 16-byte aligned (x %p, y %p, dict %p, ws %p)",
                     (const void *)d_x, (const void *)d_y, (const void *)d_dict, d_ws);
  if ((reinterpret_cast<uintptr_t>(d_idx) & 7) || (reinterpret_cast<uintptr_t>(d_dist) & 3) ||
      (reinterpret_cast<uintptr_t>(d_ncand) & 3))
    return set_error(SPV_ERR_INVALID, "output pointers must be aligned to their element size");
  const CascadePlan P = cascade_plan(xrows, yrows, dim, m, n, g);
  if (!d_ws || ws_bytes < P.total)
    return set_error(SPV_ERR_INVALID, "workspace too small: %zu < %zu", ws_bytes, P.total);
  uint8_t *ws = static_cast<uint8_t *>(d_ws);
  uint8_t *ux = ws + P.off_ux;
  uint8_t *uy = ws + P.off_uy;
  uint32_t *xcodes = reinterpret_cast<uint32_t *>(ws + P.off_xcodes);
  uint32_t *ysign = reinterpret_cast<uint32_t *>(ws + P.off_ysign);
  uint32_t *ymask = reinterpret_cast<uint32_t *>(ws + P.off_ymask);
  uint32_t *bstart = reinterpret_cast<uint32_t *>(ws + P.off_bstart);
  uint32_t *order = reinterpret_cast<uint32_t *>(ws + P.off_order);
  uint32_t *ranks = reinterpret_cast<uint32_t *>(ws + P.off_ranks);
  uint32_t *qbstart = reinterpret_cast<uint32_t *>(ws + P.off_qbstart);
  uint32_t *qorder = reinterpret_cast<uint32_t *>(ws + P.off_qorder);
  uint32_t *qranks = reinterpret_cast<uint32_t *>(ws + P.off_qranks);
  const int nb = 1 << P.hb;
  const uint32_t hbmask = (uint32_t)nb - 1;

  SPV_HIP_CHECK(hipMemsetAsync(bstart, 0, (size_t)(P.sorted ? 2 : 1) * n * (nb + 1) * sizeof(uint32_t), stream));
  {
  ProfScope prof("cascade_project", stream);
  float *dict = reinterpret_cast<float *>(ws + (P.family == 0 ? P.off_dictp : P.off_dictm));
  if (P.family == 0)
    hipLaunchKernelGGL(repack_dict_kernel, dim3(64), dim3(kThreads), 0, stream, d_dict, dict, n, dim, m, P.mc);
  else
    hipLaunchKernelGGL(repack_dict_mfma_kernel, dim3(64), dim3(kThreads), 0, stream, d_dict, dict, n, dim, m,
                       (n * m + 15) / 16 * 16);
  if (!launch_project<false>(P, d_x, xrows, dim, m, n, 0, dict, xcodes, nullptr, ux, bstart, ranks, hbmask, nb,
                             stream) ||
      !launch_project<true>(P, d_y, yrows, dim, m, n, g, dict, ysign, ymask, uy, P.qhist_fused ? qbstart : nullptr,
                            P.qhist_fused ? qranks : nullptr, hbmask, nb, stream))
    return set_error(SPV_ERR_INTERNAL, "cascade plan names no projection kernel (family %d <%d, %d>, GMAX %d)",
                     P.family, P.pa, P.pb, P.gmax_q);
  if (P.sorted && !P.qhist_fused)
    hipLaunchKernelGGL(query_rank_kernel, dim3(1024), dim3(256), 0, stream, ysign, yrows, n, hbmask, nb, qbstart,
                       qranks);
  }
  SPV_HIP_CHECK(hipGetLastError());

  {
  ProfScope prof("cascade_buckets", stream);
  {
    // database and (sorted probe) query histograms sit back to back: one scan over 2n "tables"
    const int nseg = (nb + 1 + kScanSeg - 1) / kScanSeg;
    const int ntab = P.sorted ? 2 * n : n;
    uint32_t *segsum = reinterpret_cast<uint32_t *>(ws + P.off_segsum);
    hipLaunchKernelGGL(bucket_segsum_kernel, dim3(nseg, ntab), dim3(256), 0, stream, bstart, nb, nseg, segsum);
    hipLaunchKernelGGL(bucket_segscan_kernel, dim3(ntab), dim3(1024), 0, stream, segsum, nseg);
    hipLaunchKernelGGL(bucket_scan_kernel, dim3(nseg, ntab), dim3(1024), 0, stream, bstart, nb, nseg, segsum);
  }
  if (xrows > 0)
    hipLaunchKernelGGL(bucket_fill_kernel, dim3(2048), dim3(kThreads), 0, stream, xcodes, ranks, xrows, n,
                       hbmask, nb, bstart, order);
  if (P.sorted)  // the queries' own order, per table, by sign code
    hipLaunchKernelGGL(bucket_fill_kernel, dim3(2048), dim3(kThreads), 0, stream, ysign, qranks, yrows, n,
                       hbmask, nb, qbstart, qorder);
  }
  SPV_HIP_CHECK(hipGetLastError());

  ProfScope prof_probe("cascade_probe_refine", stream);
  const dim3 grid(P.probe_grid), block(kThreads);
  if (P.use_group) {
    uint64_t *partial = reinterpret_cast<uint64_t *>(ws + P.off_partial);
    int32_t *pvisited = reinterpret_cast<int32_t *>(ws + P.off_pvisited);
    auto go = [&](auto kernel) {  // one pass per table, the two smallest keys carried from pass to pass
      for (int ps = 0; ps < n; ++ps)
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, ux, uy, xrows, yrows, dim, P.dshift, g, P.hb,
                           ysign + (size_t)ps * yrows, ymask + (size_t)ps * yrows, bstart + (size_t)ps * (nb + 1),
                           order + (size_t)ps * xrows, P.sorted ? qorder + (size_t)ps * yrows : nullptr, P.nblk,
                           P.per_xcd, partial, pvisited, ps == 0, ps == n - 1, d_idx, d_dist, d_ncand);
    };
    if (P.cpl == 2) go(probe_table_kernel<2, 4, 6, false, false>);
    else if (P.full) go(probe_table_kernel<1, 8, 7, true, true>);
    else if (P.shift) go(probe_table_kernel<1, 8, 7, true, false>);
    else go(probe_table_kernel<1, 8, 7, false, false>);
  } else {
    auto go = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, grid, block, 0, stream, ux, uy, xrows, yrows, dim, m, n, g, P.hb, xcodes, ysign,
                         ymask, bstart, order, d_idx, d_dist, d_ncand);
    };
    switch (P.cpl) {
      case 1:
        if (P.ru == 2) go(probe_refine_kernel<1, 2>);
        else go(probe_refine_kernel<1, 4>);
        break;
      case 2: go(probe_refine_kernel<2, 4>); break;
      case 4: go(probe_refine_kernel<4, 2>); break;
      case 8: go(probe_refine_kernel<8, 1>); break;
      default: go(probe_refine_kernel<16, 1>); break;
    }
  }
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

}  // namespace spv
