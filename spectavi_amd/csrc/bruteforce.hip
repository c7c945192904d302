// bruteforce.hip -- exact p-norm k-nearest-neighbour (float32 or int32 rows) for gfx950 (MI355X).
//
// The GPU form of the reference's generic matcher, nn_bruteforce / nn_bruteforcei
// (reference src/Spectavi.cpp:258-282 over src/BruteForceNn.h), with the contract stated in
// include/spectavi_amd.h: per (query y_i, database row x_j) the distance is the SEQUENTIAL,
// unfused sum over c = 0..dim-1 of t_c, every operation rounded on its own, t_c from
// d = float(x - y) as |d|, d*d, sqrtf(|d|) or float(pow((double)|d|, (double)p)) (int rows: each
// term truncated to int and summed in int32); the result per query is the k smallest
// (dist, idx) pairs in lexicographic order.
//
// Only the summation order fixes the bits, so parallelism comes from pairs, never from the dim:
//
//   * a workgroup of 256 lanes owns 256 queries, one per lane; its database slice streams
//     through LDS in groups of kRows = 32 rows, kStage = 256 columns at a time, stored with the
//     rows of a pair interleaved ((x_2r[c], x_2r+1[c], x_2r[c+1], x_2r+1[c+1]) are 16
//     consecutive bytes), so one broadcast ds_read_b128 -- every lane reads the same address --
//     feeds two database rows x two columns;
//   * a lane keeps kChunk = 32 columns of its query in VGPRs (re-read from L2 once per row group)
//     and 16 float2 accumulators, one per row pair: the float variant does sub / mul / add on both
//     rows of a pair with one v_pk_add_f32 / v_pk_mul_f32 / v_pk_add_f32, which rounds each half
//     exactly like the scalar instruction (-ffp-contract=off: no v_pk_fma); the int variant runs
//     the scalar sequence;
//   * after a row group the 32 distances enter the lane's running top-KB list in ascending row
//     order: one compare against the k-th distance and a wave-uniform branch, the insertion
//     chain only when some lane improves.  Rows arrive in ascending index, so a strict < on the
//     distance alone IS the lexicographic (dist, idx) order;
//   * columns past dim are zero on both sides: their terms are +0 (|0|, 0*0, sqrt(0), pow(0,p>0))
//     and s + 0 = s for every s >= +0, so the padding is exact.
//
// The database is cut into slices (grid.y); each slice leaves its k best keys
// (dist bits << 32 | row) per query, and bf_merge_kernel selects the k smallest of the
// slices x k keys of a query, one wave per query.  Keys are unique, so the result does not
// depend on the slice count.
//
// No MFMA: ||x||^2 + ||y||^2 - 2 x.y does not reproduce the sequential unfused sum.

#include "common.h"
#include "device_util.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

namespace spv {
namespace {

constexpr int kThreads = 256;
constexpr int kRows = 32;    // database rows per group (16 pairs)
constexpr int kStage = 256;  // columns staged in LDS at a time
constexpr int kChunk = 32;   // query columns held in VGPRs at a time
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kKeyNone = ~0ull;
constexpr int kMaxDim = 2048;
constexpr int kMaxK = 64;

typedef float f2 __attribute__((ext_vector_type(2)));

enum PKind { P_ONE = 0, P_TWO = 1, P_HALF = 2, P_GEN = 3 };

// ---- the term t(d) of one column ------------------------------------------------------------
// general p: one out-of-line copy of the double pow (inlined into every unrolled column it made
// the tile kernels take minutes to compile; this path is not the fast one anyway)
__device__ __noinline__ double pow_abs(float d, double p) { return pow((double)fabsf(d), p); }

template <int PK>
__device__ __forceinline__ float term_f(float d, double p) {
  if constexpr (PK == P_ONE) return fabsf(d);
  else if constexpr (PK == P_TWO) return d * d;
  else if constexpr (PK == P_HALF) return sqrtf(fabsf(d));  // correctly rounded (no fast-math)
  else return (float)pow_abs(d, p);
}

template <int PK>
__device__ __forceinline__ f2 term_f2(f2 d, double p) {
  if constexpr (PK == P_TWO) {
    return d * d;  // v_pk_mul_f32
  } else {
    f2 t;
    t.x = term_f<PK>(d.x, p);
    t.y = term_f<PK>(d.y, p);
    return t;
  }
}

template <int PK>
__device__ __forceinline__ int32_t term_i(int32_t xv, int32_t yv, double p) {
  // d = float(int32(x - y)) (wrapping: out of the domain the result is unspecified, not a fault)
  const float d = (float)(int32_t)((uint32_t)xv - (uint32_t)yv);
  if constexpr (PK == P_ONE) return (int32_t)fabsf(d);
  else if constexpr (PK == P_TWO) return (int32_t)(d * d);
  else if constexpr (PK == P_HALF) return (int32_t)sqrtf(fabsf(d));
  else return (int32_t)pow_abs(d, p);
}

// ---- running top-KB of one query: distance bits + row, ascending -----------------------------
// A new row has a larger index than every row already listed (ascending scan), so "key < entry"
// is "dist < entry dist".  Once it has taken a slot, every later entry moves down one slot (the
// displaced entry has a lower index than equal distances behind it, so no compare decides that).
// Only the first k entries are kept exact; thr = the k-th distance.
template <int KB>
__device__ __forceinline__ void list_insert(uint32_t (&dl)[KB], uint32_t (&il)[KB], uint32_t d, uint32_t idx,
                                            int k, uint32_t &thr) {
  bool moving = false;
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    const bool lt = moving || d < dl[i];
    moving = lt;
    const uint32_t od = dl[i], oi = il[i];
    dl[i] = lt ? d : od;
    il[i] = lt ? idx : oi;
    d = lt ? od : d;
    idx = lt ? oi : idx;
  }
  uint32_t t = dl[0];
#pragma unroll
  for (int i = 1; i < KB; ++i) t = (i == k - 1) ? dl[i] : t;
  thr = t;
}

// ---------------------------------------------------------------------------------------------
// Tile kernel.  grid = (query blocks, slices); lane t of query block qb owns query qb*256 + t.
// part[(query * S + slice) * k + j], j < k: the slice's j-th best key, kKeyNone if none.
// ---------------------------------------------------------------------------------------------
template <bool INT, int PK, int KB>
__global__ __launch_bounds__(kThreads) void bf_tile_kernel(const uint32_t *__restrict__ x,
                                                           const uint32_t *__restrict__ y, int M, int N,
                                                           int dim, int slice_rows, int S, int k, double p,
                                                           uint64_t *__restrict__ part) {
  // [row pair][column][2]: one ds_read_b128 = (row 2r, row 2r+1) x (column c, c+1)
  __shared__ uint32_t tile[kRows / 2][kStage][2];
  using Acc = typename std::conditional<INT, int32_t, f2>::type;

  const int t = threadIdx.x;
  const int qi = blockIdx.x * kThreads + t;
  const int s = blockIdx.y;
  const long long row_begin = (long long)s * slice_rows;
  const int row_end = (int)std::min<long long>(M, row_begin + slice_rows);
  const uint32_t *yq = y + (size_t)std::min(qi, N - 1) * dim;

  uint32_t dl[KB], il[KB];
#pragma unroll
  for (int i = 0; i < KB; ++i) dl[i] = il[i] = kNone;
  uint32_t thr = kNone;

  for (int row0 = (int)row_begin; row0 < row_end; row0 += kRows) {
    const int nrows = std::min(kRows, row_end - row0);
    Acc acc[INT ? kRows : kRows / 2];
#pragma unroll
    for (int i = 0; i < (INT ? kRows : kRows / 2); ++i) acc[i] = Acc{};

    for (int c0 = 0; c0 < dim; c0 += kStage) {
      const int width = std::min(kStage, (dim - c0 + 3) & ~3);  // staged columns, a multiple of 4
      __syncthreads();  // the previous stage has been consumed
      for (int e = t; e < kRows * width; e += kThreads) {
        const int r = e / width, c = e - r * width;
        uint32_t v = 0;
        if (r < nrows && c0 + c < dim) v = x[(size_t)(row0 + r) * dim + c0 + c];
        tile[r >> 1][c][r & 1] = v;
      }
      __syncthreads();

      // kChunk columns at a time, then 4 at a time for the rest of the stage
      auto run = [&](auto chunk_tag, int cc) {
        constexpr int CH = decltype(chunk_tag)::value;
        uint32_t q[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) q[j] = (c0 + cc + j < dim) ? yq[c0 + cc + j] : 0u;
#pragma unroll
        for (int j = 0; j < CH; j += 2) {
#pragma unroll
          for (int rp = 0; rp < kRows / 2; ++rp) {
            const uint4 v = *reinterpret_cast<const uint4 *>(&tile[rp][cc + j][0]);
            if constexpr (INT) {
              // dims j, j+1 in order for row 2rp, then for row 2rp+1 (the two sums are independent)
              acc[2 * rp] = acc[2 * rp] + term_i<PK>((int32_t)v.x, (int32_t)q[j], p);
              acc[2 * rp + 1] = acc[2 * rp + 1] + term_i<PK>((int32_t)v.y, (int32_t)q[j], p);
              acc[2 * rp] = acc[2 * rp] + term_i<PK>((int32_t)v.z, (int32_t)q[j + 1], p);
              acc[2 * rp + 1] = acc[2 * rp + 1] + term_i<PK>((int32_t)v.w, (int32_t)q[j + 1], p);
            } else {
              const f2 x0 = {__uint_as_float(v.x), __uint_as_float(v.y)};
              const f2 x1 = {__uint_as_float(v.z), __uint_as_float(v.w)};
              const float q0 = __uint_as_float(q[j]), q1 = __uint_as_float(q[j + 1]);
              acc[rp] = acc[rp] + term_f2<PK>(x0 - f2{q0, q0}, p);
              acc[rp] = acc[rp] + term_f2<PK>(x1 - f2{q1, q1}, p);
            }
          }
        }
      };
      int cc = 0;
      for (; cc + kChunk <= width; cc += kChunk) run(std::integral_constant<int, kChunk>{}, cc);
      for (; cc < width; cc += 4) run(std::integral_constant<int, 4>{}, cc);
    }

    // the group's rows enter the running list in ascending row order.  First the rows that beat
    // the current k-th distance in some lane (thr only falls while inserting, so no other row can
    // enter), then one insertion body for each of them (a select chain picks the row's distance)
    // instead of 32 copies of the chain.
    uint32_t dv[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      if constexpr (INT) dv[r] = (uint32_t)acc[r];
      else dv[r] = __float_as_uint((r & 1) ? acc[r >> 1].y : acc[r >> 1].x);
    }
    uint32_t cand = 0;
#pragma unroll
    for (int r = 0; r < kRows; ++r)
      cand |= (__builtin_amdgcn_ballot_w64(dv[r] < thr) != 0ull ? 1u : 0u) << r;
    cand &= nrows >= 32 ? ~0u : ((1u << nrows) - 1u);
    while (cand) {
      const int r = __builtin_ctz(cand);  // uniform
      cand &= cand - 1;
      uint32_t d = dv[0];
#pragma unroll
      for (int rr = 1; rr < kRows; ++rr) d = rr == r ? dv[rr] : d;
      if (d < thr) list_insert<KB>(dl, il, d, (uint32_t)(row0 + r), k, thr);
    }
  }

  if (qi < N) {
    uint64_t *dst = part + ((size_t)qi * S + s) * k;
#pragma unroll
    for (int i = 0; i < KB; ++i)
      if (i < k) dst[i] = il[i] == kNone ? kKeyNone : (((uint64_t)dl[i] << 32) | il[i]);
  }
}

// ---------------------------------------------------------------------------------------------
// Merge kernel: one wave per query.  Every lane keeps the KB smallest of its strided share of
// the S x k partial keys, then k rounds of a wave-wide minimum: the lane holding it pops.
// Writes idx uint64[N,k] ((size_t)-1 = none) and 32-bit dist[N,k] (+inf / INT_MAX = none).
// ---------------------------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(kThreads) void bf_merge_kernel(const uint64_t *__restrict__ part, int N, int S,
                                                            int k, uint32_t none_dist,
                                                            uint64_t *__restrict__ out_idx,
                                                            uint32_t *__restrict__ out_dist) {
  const long long gt = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int query = (int)(gt >> 6);  // wave-uniform
  const int lane = threadIdx.x & 63;
  if (query >= N) return;
  uint64_t l[KB];
#pragma unroll
  for (int i = 0; i < KB; ++i) l[i] = kKeyNone;
  const uint64_t *pq = part + (size_t)query * S * k;
  const int total = S * k;
  for (int e = lane; e < total; e += 64) {
    uint64_t key = pq[e];
    if (key < l[KB - 1]) {
#pragma unroll
      for (int i = 0; i < KB; ++i) {
        const uint64_t o = l[i];
        const bool lt = key < o;
        l[i] = lt ? key : o;
        key = lt ? o : key;
      }
    }
  }
  for (int j = 0; j < k; ++j) {
    uint64_t m = l[0];
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) {
      const uint64_t o = shfl_xor_u64(m, mask);
      m = o < m ? o : m;
    }
    if (lane == 0) {
      const bool none = m == kKeyNone;
      out_idx[(size_t)query * k + j] = none ? ~0ull : (m & 0xFFFFFFFFull);
      out_dist[(size_t)query * k + j] = none ? none_dist : (uint32_t)(m >> 32);
    }
    if (l[0] == m && m != kKeyNone) {  // keys are unique: exactly one lane pops
#pragma unroll
      for (int i = 0; i < KB - 1; ++i) l[i] = l[i + 1];
      l[KB - 1] = kKeyNone;
    }
  }
}

// ---- launch ---------------------------------------------------------------------------------
int k_bucket(int k) { return k <= 2 ? 2 : k <= 8 ? 8 : 64; }

using KBuckets = Ints<2, 8, 64>;

// the tile kernel of the plan's p kind and k bucket
template <bool INT>
void launch_tile(const void *x, const void *y, int M, int N, int dim, const BruteForcePlan &pl, int k, double p,
                 uint64_t *part, hipStream_t stream) {
  pick(Ints<P_ONE, P_TWO, P_HALF, P_GEN>{}, bruteforce_p_kind(p), [&](auto PK) {
    return pick(KBuckets{}, k_bucket(k), [&](auto KB) {
      hipLaunchKernelGGL((bf_tile_kernel<INT, decltype(PK)::value, decltype(KB)::value>), dim3(pl.qblocks, pl.slices),
                         dim3(kThreads), 0, stream, static_cast<const uint32_t *>(x), static_cast<const uint32_t *>(y), M,
                         N, dim, pl.slice_rows, pl.slices, k, p, part);
      return true;
    });
  });
}

}  // namespace

// p arrives as a C float and is compared as a double, as the reference's branches do
// (src/BruteForceNn.h:68-78).
int bruteforce_p_kind(double p) { return p == 1 ? P_ONE : p == 2 ? P_TWO : p == .5 ? P_HALF : P_GEN; }

int bruteforce_check(int xrows, int yrows, int dim, int k, float p) {
  if (xrows < 0 || yrows < 0) return set_error(SPV_ERR_INVALID, "negative row count");
  if (dim < 1 || dim > kMaxDim) return set_error(SPV_ERR_INVALID, "dim=%d outside [1, %d]", dim, kMaxDim);
  if (k < 1 || k > kMaxK) return set_error(SPV_ERR_INVALID, "k=%d outside [1, %d]", k, kMaxK);
  if (!std::isfinite(p) || !(p > 0)) return set_error(SPV_ERR_INVALID, "p=%g: a finite p > 0 is required", (double)p);
  return SPV_OK;
}

BruteForcePlan bruteforce_plan(int xrows, int yrows, int k, int slices) {
  BruteForcePlan pl{};
  pl.qblocks = std::max(1, (yrows + kThreads - 1) / kThreads);
  long long rows;
  if (slices > 0) {
    rows = std::max<long long>(1, ((long long)xrows + slices - 1) / slices);
  } else {
    // enough workgroups to keep every CU busy several times over (256 CUs, up to four 256-lane
    // workgroups resident on each), slices of whole row groups and at least 64 rows
    const long long want = 2048;
    const long long s = std::max<long long>(1, (want + pl.qblocks - 1) / pl.qblocks);
    rows = ((long long)xrows + s - 1) / s;
    rows = std::max<long long>(64, (rows + kRows - 1) / kRows * kRows);
  }
  pl.slice_rows = (int)std::min<long long>(rows, std::max(xrows, 1));
  pl.slices = std::max(1, (int)(((long long)xrows + pl.slice_rows - 1) / pl.slice_rows));
  pl.part_bytes = round_up((size_t)std::max(yrows, 1) * pl.slices * k * sizeof(uint64_t), 256);
  return pl;
}

int bruteforce_run(const void *d_x, const void *d_y, int is_int, int xrows, int yrows, int dim, int k, float p,
                   int slices, uint64_t *d_idx, void *d_dist, void *d_ws, size_t ws_bytes, hipStream_t stream) {
  SPV_TRY(bruteforce_check(xrows, yrows, dim, k, p));
  if (slices < 0) return set_error(SPV_ERR_INVALID, "slices=%d", slices);
  if (yrows == 0) return SPV_OK;
  if (!d_y || !d_idx || !d_dist || (xrows > 0 && !d_x)) return set_error(SPV_ERR_INVALID, "null device pointer");
  if ((reinterpret_cast<uintptr_t>(d_x) | reinterpret_cast<uintptr_t>(d_y) | reinterpret_cast<uintptr_t>(d_dist)) & 3)
    return set_error(SPV_ERR_INVALID, "x, y and dist must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_idx) | reinterpret_cast<uintptr_t>(d_ws)) & 7)
    return set_error(SPV_ERR_INVALID, "idx and the workspace must be 8-byte aligned");
  const BruteForcePlan pl = bruteforce_plan(xrows, yrows, k, slices);
  if (pl.slices > 65535) return set_error(SPV_ERR_INVALID, "slices=%d > 65535", pl.slices);
  // the plan's part_bytes, which spv_bruteforce_workspace_bytes reports; of a caller who forces the slice count
  // the header asks what the kernels touch (part_bytes is that rounded up to 256)
  const size_t need = slices > 0 ? (size_t)yrows * pl.slices * k * sizeof(uint64_t) : pl.part_bytes;
  if (!d_ws || ws_bytes < need) return set_error(SPV_ERR_INVALID, "workspace too small: %zu < %zu", ws_bytes, need);
  uint64_t *part = static_cast<uint64_t *>(d_ws);
  const double pd = (double)p;
  {
    ProfScope prof("bruteforce", stream);
    if (is_int) launch_tile<true>(d_x, d_y, xrows, yrows, dim, pl, k, pd, part, stream);
    else launch_tile<false>(d_x, d_y, xrows, yrows, dim, pl, k, pd, part, stream);
  }
  SPV_HIP_CHECK(hipGetLastError());
  {
    ProfScope prof("bruteforce_merge", stream);
    const unsigned blocks = (unsigned)(((long long)yrows * 64 + kThreads - 1) / kThreads);
    const uint32_t none = is_int ? 0x7FFFFFFFu : 0x7F800000u;  // INT_MAX / +inf
    uint32_t *dist = static_cast<uint32_t *>(d_dist);
    pick(KBuckets{}, k_bucket(k), [&](auto KB) {
      hipLaunchKernelGGL((bf_merge_kernel<decltype(KB)::value>), dim3(blocks), dim3(kThreads), 0, stream, part, yrows,
                         pl.slices, k, none, d_idx, dist);
      return true;
    });
  }
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

}  // namespace spv
