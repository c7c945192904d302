// stereo_batch.hip -- dense SAD disparity of every rectified pair of a collection (gfx950).
//
// The consumer of rectify_batch.hip's windows: row y of r0 and row y of r1 are a pair of epipolar lines, so a
// reference sample (y, x) is matched against (y, x + d) of the other image by the sum of absolute differences of
// the two (2r + 1)^2 blocks, an integer on 8-bit data.  Three ops (the contract is in include/spectavi_amd.h):
//
//   stereo_batch_kernel<R>        one workgroup per item = (pair, band of 4 window rows, tile of 64 window columns),
//                                 walking b, b + gridDim.x, ...: a wave owns a row of the band, a lane a column.  The
//                                 reference rows of the band (with the r rows above and below, the r columns left and
//                                 right) are staged into LDS once per item, the lane's block goes into registers as
//                                 dwords; the other image's rows are staged per chunk of 128 disparities, with the
//                                 validity of its centres as one byte per column.  Everything outside the window is
//                                 zero in LDS and no address outside a pair's window is formed, so the inner loop has
//                                 no bounds branch: an inadmissible d is masked where its cost is compared.
//   stereo_none_kernel            the windows of the pairs that are not used: NONE / 0xFFFF / 0xFFFF
//   stereo_keep_kernel            one lane per sample: the left-right and uniqueness tests
//   stereo_matches_*_kernel       the kept samples in order: counts of blocks of 1024 samples, one scan of the counts,
//                                 pair_off from the scanned counts, then the fill -- positions from scans alone
//
// The inner loop (direct form).  For four consecutive disparities the other image's bytes of one block row are
// 2r + 4 consecutive bytes of LDS starting at the lane's own byte offset; they are read as aligned dwords and
// realigned with v_alignbyte_b32 -- once by the lane's offset (x & 3), then by the constants 1, 2, 3 -- and each of
// the ceil((2r + 1) / 4) dwords of the row goes through one v_sad_u8 against the lane's register block.  2r + 1 is
// odd, so the last dword of a row holds 1 or 3 bytes of the block: the rest is cleared on both operands.
//
// The winner is kept as a running state over ascending d, which no chunk seam interrupts: (c1, d1) the best so far
// (strict <, so the smallest d wins a tie), m2 the smallest cost at distance >= 2 from d1, pm the smallest cost over
// all d' <= d - 2 and prev the cost at d - 1.  A new winner at d takes m2 = pm: everything before d - 1, the old
// winner included wherever it is far enough.
#include "common.h"
#include "device_util.h"
#include "host_io.h"

#include <climits>
#include <string.h>

namespace spv {
namespace {

constexpr int kThreads = kStereoRows * kStereoCols;  // 256
constexpr int kChunk = 128;                          // disparities per staging of the other image's rows
constexpr uint32_t kInf = 0xFFFFFFFFu;
constexpr int kScanBlock = 1024;  // samples per block of the compaction
constexpr int kMaxPairs = 1 << 20;

static_assert(sizeof(StereoBatchItem) == 16, "items travel as int32[4]");
static_assert(kStereoCols == 64 && kChunk % 4 == 0, "a lane per column of a wave; chunks of whole dwords");

// One pair as the kernels read it (a table in HBM, uniform over a workgroup).
struct StereoPair {
  long long out;        // samples before the pair's window
  int32_t rows, cols;   // of the window
  int32_t d_lo, d_hi;
};
static_assert(sizeof(StereoPair) == 24, "the items behind the table stay aligned to 8 bytes");

__device__ __forceinline__ uint32_t align_bytes(uint32_t hi, uint32_t lo, uint32_t s) {
  return __builtin_amdgcn_alignbyte(hi, lo, s);  // ({hi, lo} >> 8 s) & 0xFFFFFFFF
}

template <int R>
__global__ __launch_bounds__(kThreads) void stereo_batch_kernel(const StereoPair *__restrict__ pairs,
                                                               const StereoBatchItem *__restrict__ items,
                                                               long long nitems, const uint8_t *__restrict__ ref,
                                                               const uint8_t *__restrict__ oth,
                                                               const int32_t *__restrict__ ri_ref,
                                                               const int32_t *__restrict__ ri_oth,
                                                               int32_t *__restrict__ disp, uint16_t *__restrict__ cost,
                                                               uint16_t *__restrict__ cost2) {
  constexpr int B = 2 * R + 1;                 // the block's side
  constexpr int W = (B + 3) / 4;               // dwords of a block row
  constexpr int TV = B - 4 * (W - 1);          // bytes of the block in a row's last dword: 1 or 3
  constexpr uint32_t kTail = (1u << (8 * TV)) - 1u;
  constexpr int NR = kStereoRows + 2 * R;      // staged rows
  constexpr int RW = kStereoCols / 4 + W + 1;  // dwords of a staged reference row: the last lane reads W + 1 from 15
  constexpr int OW = RW + kChunk / 4;          // ... of the other image, the last group of a chunk included
  constexpr int VW = kStereoCols / 4 + kChunk / 4 + 1;
  __shared__ uint32_t s_ref[NR * RW], s_oth[NR * OW], s_val[kStereoRows * VW];
  uint8_t *b_ref = reinterpret_cast<uint8_t *>(s_ref), *b_oth = reinterpret_cast<uint8_t *>(s_oth);
  uint8_t *b_val = reinterpret_cast<uint8_t *>(s_val);

  const int t = threadIdx.x, lx = t & 63, ly = t >> 6;
  const uint32_t sh = lx & 3;
  const int q0 = lx >> 2;
  for (long long b = blockIdx.x; b < nitems; b += gridDim.x) {  // workgroup-uniform
    const StereoBatchItem it = items[b];
    const StereoPair pr = pairs[it.pair];
    const uint8_t *pref = ref + pr.out, *poth = oth + pr.out;
    const int32_t *pri_oth = ri_oth + pr.out;

    // reference rows row0 - R .., columns col0 - R ..: byte j of a staged row is column col0 - R + j
    for (int e = t; e < NR * RW * 4; e += kThreads) {
      const int rr = e / (RW * 4), j = e - rr * (RW * 4);
      // (64-bit: a window may be close to 2^31 rows or columns, where the halo passes INT_MAX)
      const long long y = (long long)it.row0 - R + rr, x = (long long)it.col0 - R + j;
      uint8_t v = 0;
      if (y >= 0 && y < pr.rows && x >= 0 && x < pr.cols) v = pref[(size_t)y * pr.cols + x];
      b_ref[e] = v;
    }
    __syncthreads();

    const int y = it.row0 + ly, x = it.col0 + lx;
    const bool owned = ly < it.rows && x < pr.cols;
    bool lane_ok = owned && y >= R && y < pr.rows - R && x >= R && x < pr.cols - R;
    if (lane_ok) lane_ok = ri_ref[pr.out + (size_t)y * pr.cols + x] != -1;

    uint32_t rb[B][W];  // the lane's block: row ly + dy of the staging, bytes lx .. lx + 2R
#pragma unroll
    for (int dy = 0; dy < B; ++dy) {
      const uint32_t *row = s_ref + (ly + dy) * RW + q0;
#pragma unroll
      for (int m = 0; m < W; ++m) rb[dy][m] = align_bytes(row[m + 1], row[m], sh);
      rb[dy][W - 1] &= kTail;
    }

    // the disparities any lane of the tile can admit
    const int tc = min(kStereoCols, pr.cols - it.col0);
    const int lo = max(pr.d_lo, R - (it.col0 + tc - 1)), hi = min(pr.d_hi, pr.cols - R - 1 - it.col0);
    uint32_t c1 = kInf, m2 = kInf, pm = kInf, prev = kInf;
    int d1 = -(1 << 30);
    for (int dc0 = lo; dc0 <= hi; dc0 += kChunk) {  // workgroup-uniform
      const int n = min(kChunk, hi - dc0 + 1);
      // the other image: byte j of a staged row is column col0 + dc0 - R + j, so the block of lane lx at
      // d = dc0 + k starts at byte lx + k; validity byte j is the centre column col0 + dc0 + j
      for (int e = t; e < NR * OW * 4; e += kThreads) {
        const int rr = e / (OW * 4), j = e - rr * (OW * 4);
        const long long yy = (long long)it.row0 - R + rr, xx = (long long)it.col0 + dc0 - R + j;
        uint8_t v = 0;
        if (yy >= 0 && yy < pr.rows && xx >= 0 && xx < pr.cols) v = poth[(size_t)yy * pr.cols + xx];
        b_oth[e] = v;
      }
      for (int e = t; e < kStereoRows * VW * 4; e += kThreads) {
        const int rr = e / (VW * 4), j = e - rr * (VW * 4);
        const long long yy = (long long)it.row0 + rr, xx = (long long)it.col0 + dc0 + j;
        uint8_t v = 0;
        if (yy < pr.rows && xx >= R && xx < pr.cols - R) v = pri_oth[(size_t)yy * pr.cols + xx] != -1;
        b_val[e] = v;
      }
      __syncthreads();

      for (int g = 0; g * 4 < n; ++g) {  // four disparities dc0 + 4g ..
        uint32_t acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int dy = 0; dy < B; ++dy) {
          const uint32_t *row = s_oth + (ly + dy) * OW + q0 + g;
          uint32_t S[W + 1];
#pragma unroll
          for (int m = 0; m <= W; ++m) S[m] = align_bytes(row[m + 1], row[m], sh);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int m = 0; m < W; ++m) {
              uint32_t v = i ? align_bytes(S[m + 1], S[m], (uint32_t)i) : S[m];
              if (m == W - 1) v &= kTail;
              acc[i] = __builtin_amdgcn_sad_u8(rb[dy][m], v, acc[i]);
            }
          }
        }
        const uint32_t *vrow = s_val + ly * VW + q0 + g;
        const uint32_t V = align_bytes(vrow[1], vrow[0], sh);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = 4 * g + i, d = dc0 + k;
          const bool adm = lane_ok && ((V >> (8 * i)) & 0xFFu) != 0u && k < n;
          const uint32_t c = adm ? acc[i] : kInf;
          if (c < c1) {
            m2 = pm;
            c1 = c;
            d1 = d;
          } else if (d - d1 >= 2) {
            m2 = min(m2, c);
          }
          pm = min(pm, prev);
          prev = c;
        }
      }
      __syncthreads();  // the chunk has been read before the next one, or the next item, is staged
    }
    if (owned) {
      const size_t o = (size_t)pr.out + (size_t)y * pr.cols + x;
      disp[o] = c1 == kInf ? INT_MIN : d1;
      cost[o] = (uint16_t)min(c1, 0xFFFFu);
      cost2[o] = (uint16_t)min(m2, 0xFFFFu);
    }
    __syncthreads();  // every block is in registers before the next item's reference rows are staged
  }
}

// fill[k]: a pair that is not used; its window gets the values of "no admissible d"
__global__ __launch_bounds__(kThreads) void stereo_none_kernel(const StereoPair *__restrict__ pairs,
                                                              const int32_t *__restrict__ fill, int nfill,
                                                              int32_t *__restrict__ disp, uint16_t *__restrict__ cost,
                                                              uint16_t *__restrict__ cost2) {
  for (int k = blockIdx.y; k < nfill; k += gridDim.y) {
    const StereoPair pr = pairs[fill[k]];
    const long long n = (long long)pr.rows * pr.cols;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)gridDim.x * kThreads) {
      disp[pr.out + e] = INT_MIN;
      cost[pr.out + e] = 0xFFFFu;
      cost2[pr.out + e] = 0xFFFFu;
    }
  }
}

// The pair that owns flat sample e: the last p with out_off[p] <= e (empty windows share an offset with their
// successor, which is the one that owns the sample).
__device__ __forceinline__ int pair_of(const long long *__restrict__ out_off, int npairs, long long e) {
  int lo = 0, hi = npairs;  // out_off[lo] <= e < out_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (out_off[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// tab: out_off long long[npairs + 1], then the windows' columns as long long[npairs]
__global__ __launch_bounds__(kThreads) void stereo_keep_kernel(const long long *__restrict__ tab, int npairs,
                                                              long long total, const int32_t *__restrict__ disp0,
                                                              const uint16_t *__restrict__ cost0,
                                                              const uint16_t *__restrict__ cost20,
                                                              const int32_t *__restrict__ disp1, int lr_tol,
                                                              uint32_t uniq, uint8_t *__restrict__ keep) {
  const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= total) return;
  const int d = disp0[e];
  bool k = d != INT_MIN && (uint32_t)cost0[e] * 100u <= (uint32_t)cost20[e] * (100u - uniq);
  if (k && disp1) {
    const int p = pair_of(tab, npairs, e);
    const long long cols = tab[(size_t)npairs + 1 + p];
    const long long x = (e - tab[p]) % cols, xo = x + d;
    k = xo >= 0 && xo < cols;
    if (k) {
      const int dd = disp1[e + d];
      // (both are disparities of at most 32767 in size, or NONE: the sum of two that are not NONE cannot overflow)
      k = dd != INT_MIN && abs(d + dd) <= lr_tol;
    }
  }
  keep[e] = k ? 1 : 0;
}

__global__ __launch_bounds__(kScanBlock) void stereo_matches_count_kernel(const uint8_t *__restrict__ keep,
                                                                         long long total,
                                                                         int32_t *__restrict__ bsum) {
  __shared__ int wsum[kScanBlock / 64];
  const long long e = (long long)blockIdx.x * kScanBlock + threadIdx.x;
  const unsigned long long m = __ballot(e < total && keep[e] != 0);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int w = 0; w < kScanBlock / 64; ++w) s += wsum[w];
    bsum[blockIdx.x] = s;
  }
}

// one workgroup: bsum -> its exclusive scan, the sum of all into bsum[nblk]
__global__ __launch_bounds__(1024) void stereo_matches_scan_kernel(int32_t *__restrict__ bsum, int nblk) {
  const int32_t all = block_scan_inplace(bsum, nblk);
  if (threadIdx.x == 0) bsum[nblk] = all;
}

// one wave per entry of pair_off: the kept samples before out_off[p]
__global__ __launch_bounds__(64) void stereo_matches_offsets_kernel(const long long *__restrict__ tab,
                                                                   const uint8_t *__restrict__ keep,
                                                                   const int32_t *__restrict__ bsum,
                                                                   long long *__restrict__ pair_off) {
  const long long s = tab[blockIdx.x], blk = s / kScanBlock;
  int c = 0;
  for (long long e = blk * kScanBlock + threadIdx.x; e < s; e += 64) c += keep[e] != 0;
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
  if (threadIdx.x == 0) pair_off[blockIdx.x] = (long long)bsum[blk] + c;  // (s = total at a block's start reads bsum[nblk])
}

// tab: out_off [npairs + 1] | columns [npairs] | wid of image 0 [npairs] | wid of image 1 [npairs]
__global__ __launch_bounds__(kScanBlock) void stereo_matches_fill_kernel(
    const long long *__restrict__ tab, int npairs, long long total, const int32_t *__restrict__ disp0,
    const uint8_t *__restrict__ keep, const int32_t *__restrict__ ri0, const int32_t *__restrict__ ri1,
    const int32_t *__restrict__ bsum, long long capacity, double *__restrict__ x0, double *__restrict__ x1,
    int32_t *__restrict__ rows) {
  __shared__ int wsum[16];
  const long long e = (long long)blockIdx.x * kScanBlock + threadIdx.x;
  const bool k = e < total && keep[e] != 0;
  const long long at = (long long)bsum[blockIdx.x] + block_scan_excl<int>(k ? 1 : 0, wsum);
  if (!k || at >= capacity) return;
  const int p = pair_of(tab, npairs, e);
  const long long cols = tab[(size_t)npairs + 1 + p], w0 = tab[(size_t)2 * npairs + 1 + p];
  const long long w1 = tab[(size_t)3 * npairs + 1 + p];
  const long long in = e - tab[p], x = in % cols, d = disp0[e], xo = x + d;
  const int s0 = ri0[e], s1 = (xo >= 0 && xo < cols) ? ri1[e + d] : -1;
  x0[at * 3 + 0] = (double)(s0 % w0);
  x0[at * 3 + 1] = (double)(s0 / w0);
  x0[at * 3 + 2] = 1.;
  x1[at * 3 + 0] = (double)(s1 % w1);
  x1[at * 3 + 1] = (double)(s1 / w1);
  x1[at * 3 + 2] = 1.;
  rows[at] = (int32_t)in;
}

// The rules of the boxes every op shares: out_off [npairs + 1] of all pairs.
int check_boxes(const int32_t *box, int npairs, std::vector<long long> *out_off) {
  if (npairs < 0 || npairs > kMaxPairs) return set_error(SPV_ERR_INVALID, "npairs = %d outside 0..2^20", npairs);
  if (npairs > 0 && !box) return set_error(SPV_ERR_INVALID, "null box");
  std::vector<long long> off((size_t)npairs + 1, 0);
  for (int p = 0; p < npairs; ++p) {
    const int32_t *bx = box + (size_t)p * 4;
    if (bx[0] < 0 || bx[0] > bx[1] || bx[2] < 0 || bx[2] > bx[3])
      return set_error(SPV_ERR_INVALID, "pair %d: box (%d, %d, %d, %d) is negative or inverted", p, bx[0], bx[1], bx[2], bx[3]);
    off[(size_t)p + 1] = off[p] + (long long)(bx[1] - bx[0]) * (bx[3] - bx[2]);
    if (off[(size_t)p + 1] >= (1ll << 31)) return set_error(SPV_ERR_INVALID, "2^31 samples or more");
  }
  *out_off = std::move(off);
  return SPV_OK;
}

unsigned capped_grid(size_t nitems) {
  return (unsigned)std::min<size_t>(nitems, (size_t)std::max(device_cu_count(), 1) * kStereoGroupsPerCu);
}

// The per-call tables live with the calling thread between calls (collection.h): one per direction of the cost
// step, so that the two directions of one frame do not wait for each other, and one each for the other steps.
thread_local DeviceTable g_stereo_table[2], g_keep_table, g_matches_table;

template <int R>
void launch_stereo(unsigned grid, hipStream_t stream, const StereoPair *pairs, const StereoBatchItem *items,
                   long long nitems, const uint8_t *ref, const uint8_t *oth, const int32_t *ri_ref,
                   const int32_t *ri_oth, int32_t *disp, uint16_t *cost, uint16_t *cost2) {
  hipLaunchKernelGGL((stereo_batch_kernel<R>), dim3(grid), dim3(kThreads), 0, stream, pairs, items, nitems, ref, oth,
                     ri_ref, ri_oth, disp, cost, cost2);
}

}  // namespace

int stereo_batch_plan(const int32_t *box, int npairs, const int32_t *use, int radius, const int32_t *drange,
                      StereoBatchPlan *out) {
  if (radius < 0 || radius > 7) return set_error(SPV_ERR_INVALID, "radius %d outside 0..7", radius);
  StereoBatchPlan pl;
  SPV_TRY(check_boxes(box, npairs, &pl.out_off));
  for (int p = 0; p < npairs; ++p) {
    if (use && !use[p]) continue;
    ++pl.used;
    if (drange) {
      const int lo = drange[2 * p], hi = drange[2 * p + 1];
      if (lo > hi || lo < -32767 || lo > 32767 || hi < -32767 || hi > 32767)
        return set_error(SPV_ERR_INVALID, "pair %d: disparity range (%d, %d) is inverted or beyond 32767", p, lo, hi);
    }
    const int32_t *bx = box + (size_t)p * 4;
    const int rows = bx[1] - bx[0], cols = bx[3] - bx[2];
    if (rows == 0 || cols == 0) continue;
    for (long long r = 0; r < rows; r += kStereoRows)  // (64-bit counters: rows or cols may be close to 2^31)
      for (long long c = 0; c < cols; c += kStereoCols)
        pl.items.push_back(StereoBatchItem{p, (int32_t)r, (int32_t)std::min<long long>(kStereoRows, rows - r), (int32_t)c});
  }
  *out = std::move(pl);
  return SPV_OK;
}

int stereo_batch_run(const uint8_t *d_r0, const uint8_t *d_r1, const int32_t *d_ri0, const int32_t *d_ri1,
                     const int32_t *box, int npairs, const int32_t *use, int radius, const int32_t *drange, int swap,
                     int32_t *d_disp, uint16_t *d_cost, uint16_t *d_cost2, hipStream_t stream) {
  if (swap != 0 && swap != 1) return set_error(SPV_ERR_INVALID, "swap = %d", swap);
  if (npairs > 0 && !drange) return set_error(SPV_ERR_INVALID, "null drange");
  StereoBatchPlan pl;
  SPV_TRY(stereo_batch_plan(box, npairs, use, radius, drange, &pl));
  if (pl.out_off[npairs] == 0) return SPV_OK;  // no window holds a sample: nothing to write
  if (!d_r0 || !d_r1 || !d_ri0 || !d_ri1 || !d_disp || !d_cost || !d_cost2)
    return set_error(SPV_ERR_INVALID, "null device pointer");
  if (((reinterpret_cast<uintptr_t>(d_ri0) | reinterpret_cast<uintptr_t>(d_ri1) | reinterpret_cast<uintptr_t>(d_disp)) & 3) ||
      ((reinterpret_cast<uintptr_t>(d_cost) | reinterpret_cast<uintptr_t>(d_cost2)) & 1))
    return set_error(SPV_ERR_INVALID, "misaligned index or output pointer");

  // pairs | items | the pairs to fill, one upload
  std::vector<int32_t> fill;
  const size_t tb = (size_t)npairs * sizeof(StereoPair), ib = pl.items.size() * sizeof(StereoBatchItem);
  std::vector<unsigned char> host(tb + ib);
  StereoPair *tab = reinterpret_cast<StereoPair *>(host.data());
  for (int p = 0; p < npairs; ++p) {
    const int32_t *bx = box + (size_t)p * 4;
    tab[p] = StereoPair{pl.out_off[p], bx[1] - bx[0], bx[3] - bx[2], drange[2 * p], drange[2 * p + 1]};
    if (use && !use[p] && pl.out_off[(size_t)p + 1] > pl.out_off[p]) fill.push_back(p);
  }
  if (ib) memcpy(host.data() + tb, pl.items.data(), ib);
  host.resize(tb + ib + fill.size() * sizeof(int32_t));
  if (!fill.empty()) memcpy(host.data() + tb + ib, fill.data(), fill.size() * sizeof(int32_t));
  DeviceTable &tt = g_stereo_table[swap];
  SPV_TRY(tt.upload(host.data(), host.size(), stream));
  const unsigned char *base = static_cast<const unsigned char *>(tt.p);
  const StereoPair *dpairs = reinterpret_cast<const StereoPair *>(base);
  const StereoBatchItem *ditems = reinterpret_cast<const StereoBatchItem *>(base + tb);
  const int32_t *dfill = reinterpret_cast<const int32_t *>(base + tb + ib);

  const uint8_t *ref = swap ? d_r1 : d_r0, *oth = swap ? d_r0 : d_r1;
  const int32_t *ri_ref = swap ? d_ri1 : d_ri0, *ri_oth = swap ? d_ri0 : d_ri1;
  {
    ProfScope prof("stereo_batch", stream);
    if (!pl.items.empty()) {
      const unsigned grid = capped_grid(pl.items.size());
      const long long nitems = (long long)pl.items.size();
      pick(Ints<0, 1, 2, 3, 4, 5, 6, 7>{}, radius, [&](auto r) {
        launch_stereo<decltype(r)::value>(grid, stream, dpairs, ditems, nitems, ref, oth, ri_ref, ri_oth, d_disp, d_cost,
                                          d_cost2);
        return true;
      });
    }
    if (!fill.empty())
      hipLaunchKernelGGL(stereo_none_kernel, dim3(64, (unsigned)std::min<size_t>(fill.size(), 1024)), dim3(kThreads), 0,
                         stream, dpairs, dfill, (int)fill.size(), d_disp, d_cost, d_cost2);
    SPV_HIP_CHECK(hipGetLastError());
  }
  return tt.record(stream);
}

int stereo_keep_batch_run(const int32_t *box, int npairs, const int32_t *d_disp0, const uint16_t *d_cost0,
                          const uint16_t *d_cost20, const int32_t *d_disp1, int lr_tol, int uniqueness, uint8_t *d_keep,
                          hipStream_t stream) {
  if (lr_tol < 0 || uniqueness < 0 || uniqueness > 100)
    return set_error(SPV_ERR_INVALID, "lr_tol = %d or uniqueness = %d outside their ranges", lr_tol, uniqueness);
  std::vector<long long> tab;
  SPV_TRY(check_boxes(box, npairs, &tab));
  const long long total = tab[npairs];
  if (total == 0) return SPV_OK;
  if (!d_disp0 || !d_cost0 || !d_cost20 || !d_keep) return set_error(SPV_ERR_INVALID, "null device pointer");
  for (int p = 0; p < npairs; ++p) tab.push_back(box[(size_t)p * 4 + 3] - box[(size_t)p * 4 + 2]);
  DeviceTable &tt = g_keep_table;
  SPV_TRY(tt.upload(tab.data(), tab.size() * sizeof(long long), stream));
  {
    ProfScope prof("stereo_keep_batch", stream);
    hipLaunchKernelGGL(stereo_keep_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                       static_cast<const long long *>(tt.p), npairs, total, d_disp0, d_cost0, d_cost20, d_disp1, lr_tol,
                       (uint32_t)uniqueness, d_keep);
    SPV_HIP_CHECK(hipGetLastError());
  }
  return tt.record(stream);
}

int stereo_matches_batch_run(const int32_t *box, int npairs, const int32_t *sizes, int nimg, const int32_t *pairs,
                             const int32_t *d_disp0, const uint8_t *d_keep, const int32_t *d_ri0, const int32_t *d_ri1,
                             long long capacity, double *d_x0, double *d_x1, int32_t *d_rows, long long *d_pair_off,
                             hipStream_t stream) {
  if (capacity < 0 || nimg < 0) return set_error(SPV_ERR_INVALID, "negative capacity or nimg");
  std::vector<long long> tab;
  SPV_TRY(check_boxes(box, npairs, &tab));
  if ((npairs > 0 && (!pairs || !sizes)) || !d_pair_off || (reinterpret_cast<uintptr_t>(d_pair_off) & 7))
    return set_error(SPV_ERR_INVALID, "null sizes or pairs, or a null or misaligned d_pair_off");
  const long long total = tab[npairs];
  tab.resize((size_t)4 * npairs + 1);
  for (int p = 0; p < npairs; ++p) {
    const int i0 = pairs[2 * p], i1 = pairs[2 * p + 1];
    if (i0 < 0 || i0 >= nimg || i1 < 0 || i1 >= nimg)
      return set_error(SPV_ERR_INVALID, "pair %d names images %d and %d of %d", p, i0, i1, nimg);
    if (sizes[2 * i0] < 1 || sizes[2 * i1] < 1) return set_error(SPV_ERR_INVALID, "pair %d: an image without columns", p);
    tab[(size_t)npairs + 1 + p] = box[(size_t)p * 4 + 3] - box[(size_t)p * 4 + 2];
    tab[(size_t)2 * npairs + 1 + p] = sizes[2 * i0];
    tab[(size_t)3 * npairs + 1 + p] = sizes[2 * i1];
  }
  if (total == 0) {
    SPV_HIP_CHECK(hipMemsetAsync(d_pair_off, 0, ((size_t)npairs + 1) * sizeof(long long), stream));
    return SPV_OK;
  }
  if (!d_disp0 || !d_keep || !d_ri0 || !d_ri1 || (capacity > 0 && (!d_x0 || !d_x1 || !d_rows)))
    return set_error(SPV_ERR_INVALID, "null device pointer");
  const int nblk = (int)((total + kScanBlock - 1) / kScanBlock);
  DevBuf ws;  // the counts of the blocks; back to the cache behind the call's last kernel
  SPV_TRY(ws.alloc(((size_t)nblk + 1) * sizeof(int32_t)));
  int32_t *bsum = ws.as<int32_t>();
  DeviceTable &tt = g_matches_table;
  int st = tt.upload(tab.data(), tab.size() * sizeof(long long), stream);
  if (st == SPV_OK) {
    const long long *dtab = static_cast<const long long *>(tt.p);
    {
      ProfScope prof("stereo_matches_count", stream);
      hipLaunchKernelGGL(stereo_matches_count_kernel, dim3(nblk), dim3(kScanBlock), 0, stream, d_keep, total, bsum);
      hipLaunchKernelGGL(stereo_matches_scan_kernel, dim3(1), dim3(1024), 0, stream, bsum, nblk);
      hipLaunchKernelGGL(stereo_matches_offsets_kernel, dim3(npairs + 1), dim3(64), 0, stream, dtab, d_keep, bsum, d_pair_off);
    }
    if (capacity > 0) {
      ProfScope prof("stereo_matches_fill", stream);
      hipLaunchKernelGGL(stereo_matches_fill_kernel, dim3(nblk), dim3(kScanBlock), 0, stream, dtab, npairs, total, d_disp0,
                         d_keep, d_ri0, d_ri1, bsum, capacity, d_x0, d_x1, d_rows);
    }
    if (hipGetLastError() != hipSuccess) st = set_error(SPV_ERR_HIP, "a stereo_matches launch failed");
    if (st == SPV_OK) st = tt.record(stream);
  }
  ws.release_after(stream);
  return st;
}

}  // namespace spv
