// tracks_batch.hip -- multi-view tracks from the matches of all pairs of a collection, on the device.
//
// The many-pairs chain ends with one match list per call over all pairs; a consumer with more than two views needs
// the connected components of the keypoint graph whose edges are the accepted matches.  The reference has no such
// step (its pipeline stops at two views, example/ex01_essential_estimation.py), so the contract is this library's
// own and is stated in include/spectavi_amd.h; tests/tracks_model.py is its plain restatement.
//
// Nodes are the rows of the concatenated tables.  `label` is the parent array of a forest throughout:
//   init      parent[i] = i, or (continuing) the caller's label clamped into [0, i]: parent[i] <= i always holds
//   hook      one lane per match: both ends are walked to a root with agent-scope loads, the larger root goes under
//             the smaller by an agent-scope compare-and-swap FROM ITS SELF VALUE.  A word is therefore written at
//             most once in the launch and only away from "I am a root"; a load that another workgroup's past shows
//             can only present a hooked node as still a root, the CAS on it then fails and returns the fresh parent,
//             and the lane goes on from there.  No plain store touches parent in this launch.  The smallest row of a
//             component is never the larger of two roots, so it stays a root: the labels are a function of the edge
//             set alone.  Every walk ends because the chain strictly decreases.
//   flatten   pointer jumping in a fixed number of launches (kernel boundaries are the only ordering relied on);
//             a lane takes up to kHops steps a round, a round in which no lane stopped short of a root leaves a zero
//             in the next round's control word and the remaining launches return at once
//   sizes     members per root by integer atomicAdd, one add per wave and root
//   scan      three exclusive scans over the rows in blocks of 1024: track numbers (roots of >= min_len members,
//             ascending), track_off (their sizes), and the members' places in row order
//   place     track[] of every row; the members as (track, row) keys in ascending row order
//   order     a stable LSD radix sort of those keys by track, 8 bits a pass, as many passes as the track count has
//             bytes (none for a single track): inside a track the rows keep their ascending order
//   flags     (set, row within the set) of every member; bit 0 of a track where two neighbours share a set
// No float atomics, no slot handed out by an atomic: every output is identical from run to run.

#include "common.h"
#include "device_util.h"

namespace spv {
namespace {

constexpr int kThreads = 256;
constexpr int kScanRows = 1024;  // rows per workgroup of the row scans (block_scan_excl's workgroup)
constexpr int kSortKeys = 1024;  // keys per workgroup of an ordering pass
constexpr int kSortWave = 64;    // ... which its scatter walks 64 at a time with one wave
constexpr int kHops = 4;         // parent steps per lane and flattening round

// The call's uploaded table: out_off[npairs + 1] | first row of the query set [npairs] | first row of the database
// set [npairs] | rows of the database set [npairs] | seg_off[nseg + 1].
struct TracksTab {
  const long long *out_off, *qbase, *dbase, *dsize, *seg;
  int npairs, nseg;
  long long out_rows;
};

__device__ __forceinline__ int32_t load_agent(const int32_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above x as this lane's loads show it (a hooked node may still look like one).
__device__ __forceinline__ int32_t find_root(const int32_t *parent, int32_t x) {
  for (;;) {
    const int32_t p = load_agent(parent + x);
    if (p >= x) return x;
    x = p;
  }
}

__global__ __launch_bounds__(kThreads) void tracks_init_kernel(int32_t *__restrict__ label, int32_t *__restrict__ size,
                                                               int n, int accumulate, int32_t *__restrict__ ctl, int nctl) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < nctl) ctl[i] = i == 0;  // the first flattening round always runs
  if (i >= n) return;
  int32_t v = (int32_t)i;
  if (accumulate) {
    const int32_t w = label[i];
    if (w >= 0 && w < v) v = w;  // anything else stands for "its own row"
  }
  label[i] = v;
  size[i] = 0;
}

__global__ __launch_bounds__(kThreads) void tracks_hook_kernel(TracksTab t, const int32_t *__restrict__ matches,
                                                               const int32_t *__restrict__ count, int capacity,
                                                               const uint8_t *__restrict__ mask, int32_t *parent) {
  const int n = min(max(*count, 0), capacity);
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  if (mask && mask[i] == 0) return;
  const long long o = matches[2 * i], k = matches[2 * i + 1];
  if (o < 0 || o >= t.out_rows) return;
  int lo = 0, hi = t.npairs;  // the first pair whose out rows begin beyond o
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (t.out_off[mid] <= o) lo = mid + 1; else hi = mid;
  }
  const int p = lo - 1;  // >= 0: out_off[0] = 0 <= o
  if (k < 0 || k >= t.dsize[p]) return;
  int32_t a = find_root(parent, (int32_t)(t.qbase[p] + (o - t.out_off[p])));
  int32_t b = find_root(parent, (int32_t)(t.dbase[p] + k));
  while (a != b) {
    const int32_t big = max(a, b), small = min(a, b);
    int32_t seen = big;
    if (__hip_atomic_compare_exchange_strong(parent + big, &seen, small, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      break;
    if (seen >= big) break;  // (cannot happen: parent[i] <= i; keeps the loop bounded whatever memory holds)
    // big was hooked meanwhile and `seen` is its parent, fresh from the atomic: max(a, b) strictly decreases
    a = find_root(parent, seen);
    b = find_root(parent, small);
  }
}

__global__ __launch_bounds__(kThreads) void tracks_flatten_kernel(int32_t *parent, int n, int32_t *ctl, int round) {
  if (ctl[round] == 0) return;  // the round before left every row at its root
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int32_t p = parent[i];
  if (p >= i) return;
  // whatever these loads return is an ancestor of i: other lanes only replace a parent by one further up
  int32_t q = p;
  bool at_root = false;
  for (int h = 0; h < kHops; ++h) {
    const int32_t g = parent[q];
    if (g >= q) {
      at_root = true;
      break;
    }
    q = g;
  }
  if (q != p) parent[i] = q;
  if (!at_root) ctl[round + 1] = 1;
}

__global__ __launch_bounds__(kThreads) void tracks_sizes_kernel(const int32_t *__restrict__ label, int n,
                                                                int32_t *__restrict__ size) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int32_t r = -1;
  if (i < n) {
    r = label[i];
    if (r == (int32_t)i) r = -1;  // a root counts itself where the size is read
  }
  // one add per wave and root: a component of half a million rows would otherwise be as many adds to one word
  unsigned long long todo = __ballot(r >= 0);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    const int32_t rr = __shfl(r, src, 64);
    const unsigned long long same = __ballot(r == rr);
    if (lane == src) atomicAdd(size + rr, (int32_t)__popcll(same));
    todo &= ~same;
  }
}

// Row i of the scans: a = it is the root of a track, b = that track's members, c = it is a member of a track.
__device__ __forceinline__ void row_terms(const int32_t *__restrict__ label, const int32_t *__restrict__ size, long long i,
                                          int n, int min_len, int32_t &a, int32_t &b, int32_t &c) {
  a = b = c = 0;
  if (i >= n) return;
  const int32_t r = label[i];
  const int32_t s = size[r] + 1;
  if (s < min_len) return;
  c = 1;
  if (r == (int32_t)i) {
    a = 1;
    b = s;
  }
}

// bsum: three arrays of nblk + 1 words, the sums of a, b and c of every block of kScanRows rows.
__global__ __launch_bounds__(kScanRows) void tracks_block_sums_kernel(const int32_t *__restrict__ label,
                                                                      const int32_t *__restrict__ size, int n, int min_len,
                                                                      int32_t *__restrict__ bsum, int nblk) {
  __shared__ int32_t s[3];
  if (threadIdx.x < 3) s[threadIdx.x] = 0;
  __syncthreads();
  int32_t v[3];
  row_terms(label, size, (long long)blockIdx.x * kScanRows + threadIdx.x, n, min_len, v[0], v[1], v[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int32_t w = v[k];
    for (int d = 32; d > 0; d >>= 1) w += __shfl_xor(w, d, 64);
    if ((threadIdx.x & 63) == 0 && w) atomicAdd(&s[k], w);
  }
  __syncthreads();
  if (threadIdx.x < 3) bsum[(size_t)threadIdx.x * (nblk + 1) + blockIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(1024) void tracks_scan_kernel(int32_t *__restrict__ bsum, int nblk, int32_t *__restrict__ counts,
                                                           long long *__restrict__ track_off) {
  const int32_t ntracks = block_scan_inplace(bsum, nblk);
  const int32_t nmembers = block_scan_inplace(bsum + (size_t)(nblk + 1), nblk);
  block_scan_inplace(bsum + (size_t)2 * (nblk + 1), nblk);
  if (threadIdx.x == 0) {
    counts[0] = ntracks;
    counts[1] = nmembers;
    track_off[ntracks] = nmembers;
  }
}

// Roots get their track number (or -1), tracks their offset and a clear flag, members their place in row order.
__global__ __launch_bounds__(kScanRows) void tracks_number_kernel(const int32_t *__restrict__ label,
                                                                  const int32_t *__restrict__ size, int n, int min_len,
                                                                  const int32_t *__restrict__ bsum, int nblk,
                                                                  int32_t *__restrict__ track, long long *__restrict__ track_off,
                                                                  uint8_t *__restrict__ flags, int2 *__restrict__ keys) {
  __shared__ int32_t wa[16], wb[16], wc[16];
  const long long i = (long long)blockIdx.x * kScanRows + threadIdx.x;
  int32_t a, b, c;
  row_terms(label, size, i, n, min_len, a, b, c);
  const int32_t ta = bsum[blockIdx.x] + block_scan_excl(a, wa);
  const int32_t tb = bsum[(size_t)(nblk + 1) + blockIdx.x] + block_scan_excl(b, wb);
  const int32_t tc = bsum[(size_t)2 * (nblk + 1) + blockIdx.x] + block_scan_excl(c, wc);
  if (i >= n) return;
  if (a) {
    track[i] = ta;
    track_off[ta] = tb;
    flags[ta] = 0;
  } else if (label[i] == (int32_t)i) {
    track[i] = -1;
  }
  if (c) keys[tc].y = (int32_t)i;
}

__global__ __launch_bounds__(kThreads) void tracks_place_kernel(const int32_t *__restrict__ label, int n,
                                                                const int32_t *__restrict__ counts, int32_t *track,
                                                                int2 *__restrict__ keys) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) {
    const int32_t r = label[i];
    if (r != (int32_t)i) track[i] = track[r];  // (a root's entry is not written in this launch)
  }
  if (i < counts[1]) keys[i].x = track[label[keys[i].y]];
}

// The ordering passes a collection of `ntracks` tracks needs: the bytes of its largest track number.
__device__ __forceinline__ int order_passes(int32_t ntracks) {
  int np = 0;
  for (uint32_t top = ntracks > 0 ? (uint32_t)ntracks - 1u : 0u; top; top >>= 8) ++np;
  return np;
}

// hist[d * nblk + b]: keys of block b whose digit is d (nblk: the blocks that hold a key).
__global__ __launch_bounds__(kThreads) void tracks_order_count_kernel(const int2 *__restrict__ bufa, const int2 *__restrict__ bufb,
                                                                      const int32_t *__restrict__ counts, int pass,
                                                                      int32_t *__restrict__ hist) {
  __shared__ int32_t h[256];
  const int32_t nm = counts[1];
  if (pass >= order_passes(counts[0]) || (long long)blockIdx.x * kSortKeys >= nm) return;
  const int2 *src = (pass & 1) ? bufb : bufa;
  const int nblk = (nm + kSortKeys - 1) / kSortKeys;
  h[threadIdx.x] = 0;
  __syncthreads();
  for (int k = 0; k < kSortKeys / kThreads; ++k) {
    const long long e = (long long)blockIdx.x * kSortKeys + k * kThreads + threadIdx.x;
    if (e < nm) atomicAdd(&h[((uint32_t)src[e].x >> (8 * pass)) & 255u], 1);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(1024) void tracks_order_scan_kernel(const int32_t *__restrict__ counts, int pass,
                                                                 int32_t *__restrict__ hist) {
  const int32_t nm = counts[1];
  if (pass >= order_passes(counts[0])) return;
  block_scan_inplace(hist, 256 * ((nm + kSortKeys - 1) / kSortKeys));
}

// One wave per block of kSortKeys keys, 64 at a time in order: a key goes behind every key of its digit in earlier
// blocks (hist), in earlier steps of this block (base) and in lower lanes of this step.
__global__ __launch_bounds__(kSortWave) void tracks_order_scatter_kernel(int2 *__restrict__ bufa, int2 *__restrict__ bufb,
                                                                        const int32_t *__restrict__ counts, int pass,
                                                                        const int32_t *__restrict__ hist) {
  __shared__ int32_t base[256];
  const int32_t nm = counts[1];
  if (pass >= order_passes(counts[0]) || (long long)blockIdx.x * kSortKeys >= nm) return;
  const int2 *src = (pass & 1) ? bufb : bufa;
  int2 *dst = (pass & 1) ? bufa : bufb;
  const int nblk = (nm + kSortKeys - 1) / kSortKeys;
  const int lane = threadIdx.x;
  for (int d = lane; d < 256; d += kSortWave) base[d] = hist[(size_t)d * nblk + blockIdx.x];
  __syncthreads();
  for (int step = 0; step < kSortKeys / kSortWave; ++step) {
    const long long e = (long long)blockIdx.x * kSortKeys + step * kSortWave + lane;
    const bool valid = e < nm;
    int2 kv = make_int2(0, 0);
    if (valid) kv = src[e];
    const uint32_t d = valid ? ((uint32_t)kv.x >> (8 * pass)) & 255u : 0u;
    unsigned long long peers = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool one = (d >> bit) & 1u;
      const unsigned long long bb = __ballot(one);
      peers &= one ? bb : ~bb;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    if (valid) dst[base[d] + rank] = kv;
    __syncthreads();
    if (valid && rank == 0) base[d] += __popcll(peers);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void tracks_finish_kernel(TracksTab t, const int2 *__restrict__ bufa,
                                                                 const int2 *__restrict__ bufb, const int32_t *__restrict__ counts,
                                                                 int32_t *__restrict__ members, uint8_t *__restrict__ flags) {
  const int32_t nm = counts[1];
  const long long m = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (m >= nm) return;
  const int2 *fin = (order_passes(counts[0]) & 1) ? bufb : bufa;
  const int2 kv = fin[m];
  int lo = 0, hi = t.nseg;  // the first set that begins beyond the row
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (t.seg[mid] <= (long long)kv.y) lo = mid + 1; else hi = mid;
  }
  const int s = lo - 1;  // >= 0: seg_off[0] = 0 <= row
  members[2 * m] = s;
  members[2 * m + 1] = (int32_t)(kv.y - t.seg[s]);
  if (m + 1 < nm) {
    const int2 nx = fin[m + 1];  // the next row up: of the same set if it lies below the set's end
    if (nx.x == kv.x && (long long)nx.y < t.seg[s + 1]) flags[kv.x] = 1;
  }
}

int ceil_log2(long long n) {
  int b = 0;
  while ((1ll << b) < n) ++b;
  return b;
}
int flatten_rounds(long long n) { return (ceil_log2(n) + 1) / 2 + 1; }  // depth < n falls to a quarter (kHops) a round

struct TracksLayout {
  int32_t *ctl, *size, *bsum, *hist;
  int2 *bufa, *bufb;
  size_t bytes;
};
// The workspace, a function of total_rows alone: a continuing call's members are bounded by nothing smaller.
TracksLayout tracks_layout(void *base, long long n) {
  WsWalk w(base);
  TracksLayout l;
  const size_t rows = (size_t)std::max<long long>(n, 1), nblk = (rows + kScanRows - 1) / kScanRows;
  l.ctl = w.take<int32_t>((size_t)(flatten_rounds(n) + 1) * sizeof(int32_t));
  l.size = w.take<int32_t>(rows * sizeof(int32_t));
  l.bsum = w.take<int32_t>(3 * (nblk + 1) * sizeof(int32_t));
  l.bufa = w.take<int2>(rows * sizeof(int2));
  l.bufb = w.take<int2>(rows * sizeof(int2));
  l.hist = w.take<int32_t>(256 * ((rows + kSortKeys - 1) / kSortKeys) * sizeof(int32_t));
  l.bytes = w.end();
  return l;
}

// The per-pair table (pair_table, collection.h) lives with the calling thread between calls.
thread_local DeviceTable g_tracks_table;

unsigned grid_of(long long threads, int per) { return (unsigned)std::max<long long>(1, (threads + per - 1) / per); }

}  // namespace

size_t tracks_batch_workspace_bytes(long long total_rows, int capacity) {
  (void)capacity;
  return tracks_layout(nullptr, total_rows).bytes;
}

long long tracks_batch_member_bound(long long total_rows, int capacity, int accumulate) {
  return accumulate ? total_rows : std::min<long long>(total_rows, 2ll * capacity);
}

int tracks_batch_check(const long long *seg_off, int nseg, const int32_t *pairs, int npairs, int capacity, int min_len) {
  if (capacity < 0) return set_error(SPV_ERR_INVALID, "negative capacity");
  if (min_len < 2) return set_error(SPV_ERR_INVALID, "min_len = %d, a track has at least 2 members", min_len);
  return check_collection_out32(seg_off, nseg, pairs, npairs);
}

int tracks_batch_run(const long long *seg_off, int nseg, const int32_t *pairs, int npairs, const int32_t *d_matches,
                     const int32_t *d_count, int capacity, const uint8_t *d_mask, int min_len, int accumulate,
                     int32_t *d_label, int32_t *d_track, long long *d_track_off, int32_t *d_members, uint8_t *d_flags,
                     int32_t *d_counts, void *d_ws, size_t ws_bytes, hipStream_t stream) {
  SPV_TRY(tracks_batch_check(seg_off, nseg, pairs, npairs, capacity, min_len));
  const long long n = seg_off[nseg];
  const long long bound = tracks_batch_member_bound(n, capacity, accumulate);
  if (!d_counts || !d_track_off) return set_error(SPV_ERR_INVALID, "null device pointer");
  if (n > 0 && (!d_label || !d_track)) return set_error(SPV_ERR_INVALID, "null device pointer");
  if (bound > 0 && !d_members) return set_error(SPV_ERR_INVALID, "null device pointer");
  if (bound > 1 && !d_flags) return set_error(SPV_ERR_INVALID, "null device pointer");
  if (capacity > 0 && npairs > 0 && (!d_matches || !d_count)) return set_error(SPV_ERR_INVALID, "null device pointer");
  if (reinterpret_cast<uintptr_t>(d_track_off) & 7) return set_error(SPV_ERR_INVALID, "track_off must be aligned to 8 bytes");
  if (n == 0) {  // no node: no track
    SPV_HIP_CHECK(hipMemsetAsync(d_counts, 0, 2 * sizeof(int32_t), stream));
    SPV_HIP_CHECK(hipMemsetAsync(d_track_off, 0, sizeof(long long), stream));
    return SPV_OK;
  }
  const TracksLayout l = tracks_layout(d_ws, n);
  if (!d_ws || ws_bytes < l.bytes) return set_error(SPV_ERR_INVALID, "workspace too small");
  if (reinterpret_cast<uintptr_t>(d_ws) & 15) return set_error(SPV_ERR_INVALID, "workspace must be aligned to 16 bytes");

  const std::vector<long long> tab = pair_table(seg_off, nseg, pairs, npairs);
  DeviceTable &tt = g_tracks_table;
  SPV_TRY(tt.upload(tab.data(), tab.size() * sizeof(long long), stream));
  const long long *dt = static_cast<const long long *>(tt.p);
  TracksTab t;
  t.out_off = dt;
  t.qbase = dt + npairs + 1;
  t.dbase = dt + 2 * (size_t)npairs + 1;
  t.dsize = dt + 3 * (size_t)npairs + 1;
  t.seg = dt + 4 * (size_t)npairs + 1;
  t.npairs = npairs;
  t.nseg = nseg;
  t.out_rows = tab[npairs];

  const int ni = (int)n, rounds = flatten_rounds(n);
  const int nblk = (int)((n + kScanRows - 1) / kScanRows);
  {
    ProfScope prof("tracks_init", stream);
    hipLaunchKernelGGL(tracks_init_kernel, dim3(grid_of(std::max<long long>(n, rounds + 1), kThreads)), dim3(kThreads), 0, stream,
                       d_label, l.size, ni, accumulate, l.ctl, rounds + 1);
  }
  if (capacity > 0 && npairs > 0 && t.out_rows > 0) {
    ProfScope prof("tracks_hook", stream);
    hipLaunchKernelGGL(tracks_hook_kernel, dim3(grid_of(capacity, kThreads)), dim3(kThreads), 0, stream, t, d_matches, d_count,
                       capacity, d_mask, d_label);
  }
  {
    ProfScope prof("tracks_flatten", stream);
    for (int r = 0; r < rounds; ++r)
      hipLaunchKernelGGL(tracks_flatten_kernel, dim3(grid_of(n, kThreads)), dim3(kThreads), 0, stream, d_label, ni, l.ctl, r);
  }
  {
    ProfScope prof("tracks_sizes", stream);
    hipLaunchKernelGGL(tracks_sizes_kernel, dim3(grid_of(n, kThreads)), dim3(kThreads), 0, stream, d_label, ni, l.size);
  }
  {
    ProfScope prof("tracks_scan", stream);
    hipLaunchKernelGGL(tracks_block_sums_kernel, dim3(nblk), dim3(kScanRows), 0, stream, d_label, l.size, ni, min_len, l.bsum, nblk);
    hipLaunchKernelGGL(tracks_scan_kernel, dim3(1), dim3(1024), 0, stream, l.bsum, nblk, d_counts, d_track_off);
    hipLaunchKernelGGL(tracks_number_kernel, dim3(nblk), dim3(kScanRows), 0, stream, d_label, l.size, ni, min_len, l.bsum, nblk,
                       d_track, d_track_off, d_flags, l.bufa);
  }
  {
    ProfScope prof("tracks_place", stream);
    hipLaunchKernelGGL(tracks_place_kernel, dim3(grid_of(n, kThreads)), dim3(kThreads), 0, stream, d_label, ni, d_counts, d_track,
                       l.bufa);
  }
  if (bound > 0) {
    // the passes the largest possible track count (bound / 2) could need; the device runs those its own count does
    int passes = 0;
    for (unsigned long long top = bound / 2 > 0 ? (unsigned long long)(bound / 2 - 1) : 0; top; top >>= 8) ++passes;
    const unsigned sgrid = grid_of(bound, kSortKeys);
    if (passes > 0) {
      ProfScope prof("tracks_order", stream);
      for (int p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(tracks_order_count_kernel, dim3(sgrid), dim3(kThreads), 0, stream, l.bufa, l.bufb, d_counts, p, l.hist);
        hipLaunchKernelGGL(tracks_order_scan_kernel, dim3(1), dim3(1024), 0, stream, d_counts, p, l.hist);
        hipLaunchKernelGGL(tracks_order_scatter_kernel, dim3(sgrid), dim3(kSortWave), 0, stream, l.bufa, l.bufb, d_counts, p, l.hist);
      }
    }
    ProfScope prof("tracks_flags", stream);
    hipLaunchKernelGGL(tracks_finish_kernel, dim3(grid_of(bound, kThreads)), dim3(kThreads), 0, stream, t, l.bufa, l.bufb, d_counts,
                       d_members, d_flags);
  }
  SPV_HIP_CHECK(hipGetLastError());
  return tt.record(stream);
}

}  // namespace spv
