// cascade_batch.hip -- the cascade-hash 2-NN of cascade.hip for a collection of (query set, database set) pairs
// over float32 tables stored back to back, in a chain of launches whose length depends neither on the number of
// pairs nor on the number of sets.
//
// A loop of single calls projects, sign-codes, images and bucket-sorts both sides of every pair again, although a
// set's codes do not depend on its partner; and each call is a memset plus about 8 + n launches of microseconds.
// Here every row of the collection goes through that work once:
//
//   1 repack_dict          as cascade.hip (cascade_kernels.h), by the projection family of cascade_plan
//   2 project<query form>  one pass over all total_rows rows: sign codes [n][total_rows], masks of the g
//                          least-confident bits, the uint8 refine image.  A row's database code IS its query sign
//                          code (the same bits of the same FMA chains), so the query form serves both roles
//   3 batch_rank           histogram of bucket = code & (2^hb - 1) per (set, table), the value the atomic returns
//                          being the row's rank inside its bucket; a row finds its set by bisection of seg_off
//   4 bucket_segsum / segscan / scan   exclusive scan of the nseg * n histograms, cascade.hip's kernels
//   5 batch_fill           order[table][seg_off[s] + position] = row number inside set s
//   6 batch_probe          one launch for every out row of every pair: a workgroup takes one item of the table the
//                          host plan builds -- up to 64 query rows of one pair, with the bases of its query set and
//                          database set -- and each wave walks its share of them as probe_refine_kernel does: 2^g
//                          probe codes per table -> the DATABASE SET'S OWN buckets -> candidate list in LDS ->
//                          v_sad_u8 gather over the uint8 image -> the two smallest distinct (dist, idx) keys
//
// hb (cascade_batch_plan): bucket memory is nseg * n * (2^hb + 1) words, zeroed and scanned on every call, so the
// single call's min(m, 22) does not carry over.  With hb < m the probe compares the full code of every bucket
// entry, which keeps the candidate set and the visited count what they are at hb = m.
//
// Results do not depend on the order of a bucket's entries (atomic ranks): the two smallest distinct keys.

#include "cascade_kernels.h"

#include <algorithm>

namespace spv {
namespace {

// A work item as the probe reads it: rows of the packed table, the database set's number (its bucket tables) and
// the out row of the item's first query.
struct alignas(32) ProbeWork {
  uint32_t q_row0, q_rows, x_row0, x_rows, x_set, out_lo, out_hi, unused;
};

// The set of packed row r: the s with seg[s] <= r < seg[s + 1] (empty sets are skipped by construction).
__device__ __forceinline__ int set_of_row(const uint32_t *__restrict__ seg, int nseg, uint32_t r) {
  int lo = 0, hi = nseg;  // seg[lo] <= r < seg[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg[mid] <= r) lo = mid;
    else hi = mid;
  }
  return lo;
}

// 3. histogram + ranks per (set, table): counts[(s * n + j)][bucket]
__global__ __launch_bounds__(kThreads) void batch_rank_kernel(const uint32_t *__restrict__ codes, uint32_t total, int n,
                                                              const uint32_t *__restrict__ seg, int nseg,
                                                              uint32_t hbmask, int nb, uint32_t *__restrict__ counts,
                                                              uint32_t *__restrict__ ranks) {
  for (size_t r = blockIdx.x * (size_t)kThreads + threadIdx.x; r < total; r += (size_t)gridDim.x * kThreads) {
    const size_t tab0 = (size_t)set_of_row(seg, nseg, (uint32_t)r) * n;
    for (int j = 0; j < n; ++j) {
      const size_t e = (size_t)j * total + r;
      ranks[e] = atomicAdd(&counts[(tab0 + j) * (nb + 1) + (codes[e] & hbmask)], 1u);
    }
  }
}

// 5. order[j][seg[s] + bucket start + rank] = row number inside set s
__global__ __launch_bounds__(kThreads) void batch_fill_kernel(const uint32_t *__restrict__ codes,
                                                              const uint32_t *__restrict__ ranks, uint32_t total, int n,
                                                              const uint32_t *__restrict__ seg, int nseg,
                                                              uint32_t hbmask, int nb,
                                                              const uint32_t *__restrict__ bstart,
                                                              uint32_t *__restrict__ order) {
  for (size_t r = blockIdx.x * (size_t)kThreads + threadIdx.x; r < total; r += (size_t)gridDim.x * kThreads) {
    const int s = set_of_row(seg, nseg, (uint32_t)r);
    const uint32_t base = seg[s];
    for (int j = 0; j < n; ++j) {
      const size_t e = (size_t)j * total + r;
      // < rows of set s: the (set, table) histogram counted exactly the set's rows
      const uint32_t pos = bstart[((size_t)s * n + j) * (nb + 1) + (codes[e] & hbmask)] + ranks[e];
      order[(size_t)j * total + base + pos] = (uint32_t)r - base;
    }
  }
}

// 6. probe + gather + refine: grid = work items, wave w of the workgroup takes queries w, w + 4, ... of its item.
// The body of a query is probe_refine_kernel's (cascade.hip) with every table reached through the item's bases:
// codes / masks / image at packed rows, buckets and order of the database set alone, candidates as row numbers
// inside that set.  All row offsets are 64-bit (the image passes 4 GiB at 2^24 rows of 256 bytes).
// CPL: 16-byte chunks of the row per lane of an 8-lane group (dim <= 128 * CPL); RU: rounds of 8 rows in flight
template <int CPL, int RU>
__global__ __launch_bounds__(kThreads) void batch_probe_kernel(
    const uint8_t *__restrict__ img, const ProbeWork *__restrict__ work, uint32_t total, int dim, int m, int n, int g,
    int hb, const uint32_t *__restrict__ codes, const uint32_t *__restrict__ masks,
    const uint32_t *__restrict__ bstart, const uint32_t *__restrict__ order, uint64_t *__restrict__ out_idx,
    float *__restrict__ out_dist, int32_t *__restrict__ out_ncand) {
  __shared__ uint32_t lists[kThreads / 64][kListCap];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const ProbeWork *wp = work + blockIdx.x;  // workgroup-uniform: scalar loads, field by field
  const uint32_t q_row0 = wp->q_row0, q_rows = wp->q_rows, x_row0 = wp->x_row0;
  const uint8_t *ux = img + (size_t)x_row0 * dim;                     // the database set's image
  const uint32_t *xorder = order + x_row0;                            // ... its order, table j at + j * total
  const uint32_t *xcodes = codes + x_row0;                            // ... its codes
  const uint32_t *xbstart = bstart + (size_t)wp->x_set * n * ((1u << hb) + 1);
  const size_t out0 = ((size_t)wp->out_hi << 32) | wp->out_lo;
  uint32_t *list = lists[wave];
  const int sub = lane & 7;    // chunk owner inside the 8-lane group
  const int grp = lane >> 3;   // candidate slot 0..7
  const int nchunk = dim / 16;
  const uint32_t nb = 1u << hb;
  const uint32_t hbmask = nb - 1;
  const bool check_code = m > hb;

  for (uint32_t qi = wave; qi < q_rows; qi += kThreads / 64) {
    const size_t query = (size_t)q_row0 + qi;  // packed row
    uint4 qv[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int ch = sub + 8 * c;
      qv[c] = ch < nchunk ? *reinterpret_cast<const uint4 *>(img + query * dim + 16 * ch) : make_uint4(0, 0, 0, 0);
    }

    uint64_t k1 = kNone64, k2 = kNone64;
    int visited = 0;

    auto refine = [&](int count) {
      // `count` candidates in list[0..count), all row numbers inside the database set; an 8-lane group takes one per round, RU rounds of
      // gathers in flight.  Slots past `count` load nothing.
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
    int lpp = 1;  // lanes per probe: few probes share their buckets' copies
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
        const uint32_t sg = codes[(size_t)tj * total + query];
        const uint32_t mk = masks[(size_t)tj * total + query];
        pcode = (sg & ~mk) | deposit_bits(var, mk);
        const uint32_t *bs = xbstart + (size_t)tj * (nb + 1) + (pcode & hbmask);
        s = bs[0];
        len = bs[1] - s;  // s + len <= the rows of the set: the set's own scan
      }
      const uint32_t mylen = psub == 0 ? len : 0u;
      const uint32_t incl = wave_scan_incl(mylen, lane);
      const uint32_t tot = __shfl(incl, 63, 64);
      if (!check_code && tot <= (uint32_t)kListCap) {
        // fast path: the lanes of a probe copy its bucket into the shared list
        const uint32_t dst = __shfl(incl - mylen, lane - psub, 64);
        const uint32_t *src = xorder + (size_t)tj * total + s;
        for (uint32_t i = psub; i < len; i += lpp) list[dst + i] = src[i];
        __builtin_amdgcn_wave_barrier();
        refine((int)tot);
        visited += (int)tot;
        __builtin_amdgcn_wave_barrier();
      } else {
        // general path (a stream longer than the list, or hb < m): buckets one at a time, 64 entries per step,
        // an entry kept only if its full code is the probe's
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
              cand = xorder[(size_t)pj * total + ps + e];
              if (check_code) keep = xcodes[(size_t)pj * total + cand] == pc;
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
      const size_t o = out0 + qi;
      const bool n1 = k1 == kNone64, n2 = k2 == kNone64;
      out_idx[2 * o + 0] = n1 ? ~0ull : (k1 & 0xFFFFFFFFull);
      out_idx[2 * o + 1] = n2 ? ~0ull : (k2 & 0xFFFFFFFFull);
      out_dist[2 * o + 0] = n1 ? 2147483648.0f : (float)(uint32_t)(k1 >> 32);
      out_dist[2 * o + 1] = n2 ? 2147483648.0f : (float)(uint32_t)(k2 >> 32);
      if (out_ncand) out_ncand[o] = visited;
    }
    __builtin_amdgcn_wave_barrier();  // the next query reuses the list
  }
}

constexpr int kBatchMinBucketBits = 12;
constexpr size_t kBatchBucketBytes = (size_t)1 << 30;

}  // namespace

int cascade_batch_plan(const long long *seg_off, int nseg, int dim, int m, int n, int g, const int32_t *pairs,
                       int npairs, CascadeBatchPlan *out) {
  if (!seg_off && nseg == 0) seg_off = kNoSets;  // no sets: seg_off may be null
  SPV_TRY(check_collection(seg_off, nseg, pairs, npairs));
  if (dim <= 0 || dim % 16 != 0)
    return set_error(SPV_ERR_INVALID, "Input matrix inner dimensions must be 16-byte aligned (dim=%d).", dim);
  if (dim > kCascadeBatchMaxDim)
    return set_error(SPV_ERR_INVALID, "dim=%d > %d is not supported by the many-pairs form of the cascade", dim,
                     kCascadeBatchMaxDim);
  if (m < 1 || m > 31) return set_error(SPV_ERR_INVALID, "hash_bit_rate m=%d must be in [1,31]", m);
  if (n < 1) return set_error(SPV_ERR_INVALID, "num_hash_tables n=%d must be >= 1", n);
  if (g < 0 || g > m || g > 16)
    return set_error(SPV_ERR_INVALID, "num_candidate_neighbours g=%d must be in [0,min(m,16)]", g);
  if ((long long)nseg * n > kCascadeBatchMaxTables)
    return set_error(SPV_ERR_INVALID, "nseg * n = %lld bucket tables, more than the %d a scan launch takes",
                     (long long)nseg * n, kCascadeBatchMaxTables);
  CascadeBatchPlan p{};
  p.total_rows = seg_off[nseg];
  auto rows = [&](int s) { return seg_off[s + 1] - seg_off[s]; };

  p.out_off = pair_out_off(seg_off, pairs, npairs);
  p.out_rows = p.out_off[npairs];
  long long count = 0;
  for (int i = 0; i < npairs; ++i) count += (rows(pairs[2 * i]) + kCascadeBatchItemRows - 1) / kCascadeBatchItemRows;
  if (count > 0x7FFFFFFFll) return set_error(SPV_ERR_INVALID, "%lld work items, more than a grid takes", count);
  p.items.reserve((size_t)count);
  for (int i = 0; i < npairs; ++i) {
    const long long nq = rows(pairs[2 * i]);
    for (long long y0 = 0; y0 < nq; y0 += kCascadeBatchItemRows)
      p.items.push_back({i, (int32_t)y0, (int32_t)std::min<long long>(kCascadeBatchItemRows, nq - y0)});
  }

  // The projection of all rows, in the query form, as cascade_plan picks it for that many query rows.
  p.proj = cascade_plan(0, (int)p.total_rows, dim, m, n, g);
  // Bucket bits: m where the tables stay small -- then a bucket holds one code and is copied as it is -- but no more
  // than the largest set can spread over (floor 12: 16 KB per table), and never more than 1 GiB of tables.
  long long max_rows = 0;
  for (int s = 0; s < nseg; ++s) max_rows = std::max(max_rows, rows(s));
  int spread = 0;
  while ((1ll << spread) < max_rows) ++spread;
  p.hb = std::min(std::min(m, 22), std::max(kBatchMinBucketBits, spread));
  const size_t ntab = (size_t)nseg * n;
  while (p.hb > 0 && ntab * (((size_t)1 << p.hb) + 1) * sizeof(uint32_t) > kBatchBucketBytes) --p.hb;
  const size_t nb1 = ((size_t)1 << p.hb) + 1;

  const size_t total = (size_t)p.total_rows;
  WsWalk w(nullptr, 16);
  p.off_tables = w.reserve(p.items.size() * sizeof(ProbeWork) + ((size_t)nseg + 1) * sizeof(uint32_t));
  p.off_dict = w.reserve(std::max((size_t)n * dim * p.proj.mc, (size_t)(dim + 16) * 64) * sizeof(float));
  p.off_img = w.reserve(total * dim);
  p.off_codes = w.reserve((size_t)n * total * sizeof(uint32_t));
  p.off_masks = w.reserve((size_t)n * total * sizeof(uint32_t));
  p.off_ranks = w.reserve((size_t)n * total * sizeof(uint32_t));
  p.off_order = w.reserve((size_t)n * total * sizeof(uint32_t));
  p.off_bstart = w.reserve(ntab * nb1 * sizeof(uint32_t));
  p.off_segsum = w.reserve(ntab * ((nb1 + kScanSeg - 1) / kScanSeg) * sizeof(uint32_t));
  p.total_bytes = w.end();
  *out = std::move(p);
  return SPV_OK;
}

int cascade_batch_run(const float *d_rows, const long long *seg_off, int nseg, int dim, int m, int n, int g,
                      const int32_t *pairs, int npairs, const float *d_dict, uint64_t *d_idx, float *d_dist,
                      int32_t *d_ncand, void *d_ws, size_t ws_bytes, hipStream_t stream) {
  CascadeBatchPlan p;
  SPV_TRY(cascade_batch_plan(seg_off, nseg, dim, m, n, g, pairs, npairs, &p));
  if (p.out_rows == 0) return SPV_OK;
  if (!d_rows || !d_dict || !d_idx || !d_dist || !d_ws) return set_error(SPV_ERR_INVALID, "null device pointer");
  if ((reinterpret_cast<uintptr_t>(d_rows) | reinterpret_cast<uintptr_t>(d_dict) | reinterpret_cast<uintptr_t>(d_ws)) & 15)
    return set_error(SPV_ERR_INVALID, "device pointers must be 16-byte aligned (rows %p, dict %p, ws %p)",
                     (const void *)d_rows, (const void *)d_dict, d_ws);
  if ((reinterpret_cast<uintptr_t>(d_idx) & 7) || (reinterpret_cast<uintptr_t>(d_dist) & 3) ||
      (reinterpret_cast<uintptr_t>(d_ncand) & 3))
    return set_error(SPV_ERR_INVALID, "output pointers must be aligned to their element size");
  if (ws_bytes < p.total_bytes) return set_error(SPV_ERR_INVALID, "workspace too small: %zu < %zu", ws_bytes, p.total_bytes);

  // the small tables: the work items, then seg_off as 32-bit packed rows
  const size_t items_bytes = p.items.size() * sizeof(ProbeWork);
  std::vector<unsigned char> tables(items_bytes + ((size_t)nseg + 1) * sizeof(uint32_t));
  ProbeWork *work = reinterpret_cast<ProbeWork *>(tables.data());
  for (size_t e = 0; e < p.items.size(); ++e) {
    const CascadeBatchItem &it = p.items[e];
    const int qs = pairs[2 * it.pair], xs = pairs[2 * it.pair + 1];
    const unsigned long long o = (unsigned long long)(p.out_off[it.pair] + it.y0);
    work[e] = {(uint32_t)(seg_off[qs] + it.y0), (uint32_t)it.yrows, (uint32_t)seg_off[xs],
               (uint32_t)(seg_off[xs + 1] - seg_off[xs]), (uint32_t)xs, (uint32_t)o, (uint32_t)(o >> 32), 0u};
  }
  uint32_t *seg32 = reinterpret_cast<uint32_t *>(tables.data() + items_bytes);
  for (int s = 0; s <= nseg; ++s) seg32[s] = (uint32_t)seg_off[s];

  uint8_t *ws = static_cast<uint8_t *>(d_ws);
  const ProbeWork *d_work = reinterpret_cast<const ProbeWork *>(ws + p.off_tables);
  const uint32_t *d_seg = reinterpret_cast<const uint32_t *>(ws + p.off_tables + items_bytes);
  float *dict = reinterpret_cast<float *>(ws + p.off_dict);
  uint8_t *img = ws + p.off_img;
  uint32_t *codes = reinterpret_cast<uint32_t *>(ws + p.off_codes);
  uint32_t *masks = reinterpret_cast<uint32_t *>(ws + p.off_masks);
  uint32_t *ranks = reinterpret_cast<uint32_t *>(ws + p.off_ranks);
  uint32_t *order = reinterpret_cast<uint32_t *>(ws + p.off_order);
  uint32_t *bstart = reinterpret_cast<uint32_t *>(ws + p.off_bstart);
  uint32_t *segsum = reinterpret_cast<uint32_t *>(ws + p.off_segsum);
  const int nb = 1 << p.hb;
  const uint32_t hbmask = (uint32_t)nb - 1;
  const int ntab = nseg * n;
  const uint32_t total = (uint32_t)p.total_rows;

  // the one wait of the call: `tables` is gone when it returns, so its upload must have ended
  SPV_HIP_CHECK(hipMemcpyWithStream(ws + p.off_tables, tables.data(), tables.size(), hipMemcpyHostToDevice, stream));
  SPV_HIP_CHECK(hipMemsetAsync(bstart, 0, (size_t)ntab * (nb + 1) * sizeof(uint32_t), stream));
  {
    ProfScope prof("cascade_batch_project", stream);
    if (p.proj.family == 0)
      hipLaunchKernelGGL(repack_dict_kernel, dim3(64), dim3(kThreads), 0, stream, d_dict, dict, n, dim, m, p.proj.mc);
    else
      hipLaunchKernelGGL(repack_dict_mfma_kernel, dim3(64), dim3(kThreads), 0, stream, d_dict, dict, n, dim, m,
                         (n * m + 15) / 16 * 16);
    if (!launch_project<true>(p.proj, d_rows, (int)total, dim, m, n, g, dict, codes, masks, img, nullptr, nullptr, hbmask,
                              nb, stream))
      return set_error(SPV_ERR_INTERNAL, "cascade plan names no projection kernel (family %d <%d, %d>, GMAX %d)",
                       p.proj.family, p.proj.pa, p.proj.pb, p.proj.gmax_q);
  }
  SPV_HIP_CHECK(hipGetLastError());

  {
    ProfScope prof("cascade_batch_buckets", stream);
    const unsigned rgrid = (unsigned)std::min<size_t>(((size_t)total + kThreads - 1) / kThreads, 2048);
    const int nscan = (nb + 1 + kScanSeg - 1) / kScanSeg;
    hipLaunchKernelGGL(batch_rank_kernel, dim3(rgrid), dim3(kThreads), 0, stream, codes, total, n, d_seg, nseg, hbmask,
                       nb, bstart, ranks);
    hipLaunchKernelGGL(bucket_segsum_kernel, dim3(nscan, ntab), dim3(256), 0, stream, bstart, nb, nscan, segsum);
    hipLaunchKernelGGL(bucket_segscan_kernel, dim3(ntab), dim3(1024), 0, stream, segsum, nscan);
    hipLaunchKernelGGL(bucket_scan_kernel, dim3(nscan, ntab), dim3(1024), 0, stream, bstart, nb, nscan, segsum);
    hipLaunchKernelGGL(batch_fill_kernel, dim3(rgrid), dim3(kThreads), 0, stream, codes, ranks, total, n, d_seg, nseg,
                       hbmask, nb, bstart, order);
  }
  SPV_HIP_CHECK(hipGetLastError());

  ProfScope prof_probe("cascade_batch_probe", stream);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.items.size()), dim3(kThreads), 0, stream, img, d_work, total, dim, m, n,
                       g, p.hb, codes, masks, bstart, order, d_idx, d_dist, d_ncand);
  };
  if (dim <= 128) go(batch_probe_kernel<1, 4>);
  else go(batch_probe_kernel<2, 4>);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

}  // namespace spv
