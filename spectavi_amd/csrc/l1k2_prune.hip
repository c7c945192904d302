// l1k2_prune.hip -- L1 2-NN at dim 128: most pairs are ruled out by an exact integer lower bound
// computed on the matrix cores, and only the survivors pay for the 32 v_sad_u8 of the exact distance.
// Results are bit-identical to l1k2_tile_kernel (l1k2.hip); l1k2_run chooses between the two.
//
// The bound.  |a - b| on bytes has a rank-4 minorant: with the harmonics k = 1, 3 of its cosine series,
//     phi(a) = ( r(127 cos(pi a/255)), r(127 sin(pi a/255)), r(127 cos(3 pi a/255)/3), r(127 sin(3 pi a/255)/3) )
// as int8 (r = round to nearest), G(a,b) = phi(a).phi(b), an integer slope p and
//     m = min over all 65536 byte pairs of ( p |a-b| + G(a,b) ),
// it holds by construction, in integers, that  p |a-b| >= m - G(a,b),  hence for 128-byte rows
//     p L1(x,y) >= 128 m - sum_d G(x_d, y_d).
// The sum is an int8 GEMM of depth 512 accumulated exactly in int32 (v_mfma_i32_32x32x32_i8).  If thr is
// any value >= the query's final second-best distance, a pair with 128 m - sum > p thr (strictly) cannot
// enter the result.  p and m are derived from the finished integer table on the host (l1k2_bound) and
// the inequality is asserted over all byte pairs before the path is ever taken.
//
// The kernel.  grid = (blocks of 256 queries, database slices); 4 waves, each owning 64 queries whose
// 512 feature bytes stay in VGPRs as the B operand (2 column blocks x 16 k-steps x 4 dwords).  Database
// feature tiles (32 rows x 512 B) stream through LDS, double buffered, one barrier per tile, loaded from
// global memory straight into LDS (global_load_lds_dwordx4; see Stage), each load addressed by a scalar
// base that moves on by one tile per iteration plus a tile-invariant lane offset.  Per tile and wave: 32 MFMAs
// whose accumulators start at minus the lane's threshold 128 m - p thr (the C layout puts one query on each
// lane), so that the sign bit of each accumulator register says "ruled out"; the 32 signs are folded into one bit
// mask per lane, and the surviving (query, row) pairs are appended to the wave's queue in LDS, one per lane and
// round.  Whenever 64 are queued, and at the end of the tile, the wave evaluates them exactly, both rows read
// from LDS (the workgroup's 256 query rows and the tile's 32 database rows are kept there as they are, beside
// the features; from global memory the same reads bound the kernel at the vector cache): one pair per lane
// (drain: 16 reads and 32 v_sad_u8 whatever the count), or, up to kOctetPairs pairs, eight lanes per pair and
// eight pairs per round (drain_octets: two reads, four v_sad_u8 and three DPP adds per round).
// A key dist<<32 | row that beats the query's current second best enters its top-2 in LDS
// with two 64-bit atomic minima: old = min(k1, key); min(k2, max(old, key)).  Every key but the final
// minimum is displaced exactly once, so k2 ends as the second smallest under any interleaving.
//
// Thresholds are shared between workgroups through thr[query] in the workspace (initialised to
// 0xFFFFFFFF): a workgroup reads it every fourth tile, one tile before it uses the value, and lowers it with
// atomicMin when its own second best improves.  Every value ever stored is the second best over a subset
// of the database, hence >= the final one: WHICH pairs are skipped depends on timing, the result never does.
//
// Waits.  No tile waits for global memory except at the one explicit vmcnt(0) before its barrier, a whole tile
// after the loads it covers were issued at the tile's top; that wait is also the only thing that makes the
// next tile visible in LDS.  The B operand is waited for once, before the loop (else the compiler guards each
// of the 32 MFMAs of every tile with a vmcnt wait), and the threshold loads ride behind the stage loads of the
// tile before.  The A operand is read from LDS two k-steps ahead of its MFMAs (three 4-register buffers,
// lgkmcnt(1) between the pairs), its first two reads being the tile's first instructions, ahead of the stage
// issue and the thresholds; the survivor pass requests all 16 pieces of its two rows at once: one LDS round trip
// per drain.  The workgroup's bail flag is read right behind the tile's
// barrier and looked at behind the next tile's threshold reads, with which it arrives: no round trip of its own.
//
// Fallback.  Every wave keeps a running survivor share.  When it exceeds the measured break-even (16 %; 3/4
// in a workgroup's first tiles; see l1k2_prune_plan) the wave raises a flag, and at the tile's barrier
// the whole workgroup publishes the thresholds it has, sets its partial keys to "none", puts its (query
// block, slice) on a work list and leaves.  l1k2_run then launches l1k2_tile_kernel<32, 2, 128> over that
// list: the parent's exact kernel, 256 queries per block, eight blocks per listed slice merging their keys
// with the two-minimum protocol.  An in-kernel exact loop (one query per lane, scalar-fed rows) ran at half
// the tile kernel's rate on ordinary data and was dropped.
//
// Register budget: all 256 VGPRs that two waves per SIMD allow (128 of them the B operand, 12 the A
// buffers, 5 the lane offsets of the stage loads and 10 what a ragged tile makes them from again, where 10 held
// the five 64-bit addresses; no register carries the staged tile, which is what lets the 64 of a drain's 16
// pieces fit), no scratch; LDS 78856 of the 81920 bytes that two workgroups per CU allow.  The ISA is checked
// after every change, without a GPU, by six modules that compile this file with the Makefile's flags:
// tests/test_l1k2_prune_isa.py (registers, spills, scratch, LDS, and no vmcnt wait between the first and the last MFMA of
// a tile), tests/test_l1k2_prune_staging_isa.py (the loads to LDS, no vmcnt wait between them and the tile's MFMAs,
// counted lgkmcnt waits among the MFMAs), tests/test_l1k2_prune_chain_isa.py (the scalar-base form of the loads, the
// vector instructions at a tile's top), and for the wide form tests/test_l1k2_prune_wide_isa.py (its budgets),
// tests/test_l1k2_prune_stagger_isa.py (its half-steps) and tests/test_l1k2_prune_arm_isa.py (its arming; that module
// also pins the narrow kernel's instruction stream, register numbers aside).
//
// Two forms.  All of the above is l1k2_prune_kernel, the narrow form, which prune mode 1 runs and whose decisions per
// 32-row tile and 256-query workgroup the case tables of the tests pin.  Where `auto` takes the path and the grid
// fills the chip, l1k2_prune_plan chooses l1k2_prune_wide_kernel instead: 64-row tiles, 512 queries and 8 waves per
// workgroup, one workgroup per CU, so that what a tile costs whatever survives is paid half as often per row.  Its
// LDS and register budget stand at its head.  PruneForm holds every number in which the two differ; what they do alike
// is written once, ahead of them: the LDS arrays, the prologue, the staging (Stage), the thresholds, the sign fold, the
// `valid` mask and the compaction, the share rule, the epilogues and the survivor passes (drain_lanes, drain_octets).  A
// kernel binds those to its own state with one-line lambdas where a piece is called from several places; the tile loops
// differ in structure and are two.  Two short pieces stand in both kernels as they were, the B-operand load and the choice
// between the two drains at the end of a tile: moved into a function, either changes the narrow kernel's schedule ahead of
// its loop, which tests/test_l1k2_prune_arm_isa.py holds fixed.  spv_l1k2_set_prune_form / SPECTAVI_L1K2_PRUNE_FORM force
// either form.
//
// Two matrix formats of the wide form.  The int8 bound above costs a wave 64 MFMAs per 64-row tile, and 1e12 pairs x 512
// MACs is a floor of the matrix pipe's own time whatever the schedule.  l1k2_prune_wide6_kernel does the same job with 40:
// a rank-5 table of FP6 (e2m3) features (l1k2_bound_fp6.h; a feature is k/8, k on the e2m3 grid, so G, p and m are integers
// in units of 1/64), K = 640 per pair in ten v_mfma_scale_f32_32x32x64_f8f6f4 with unit scales per row half and column
// block.  Every value an accumulator ever holds is a multiple of 1/64 below 2^24/64 (make_bound6 refuses a table for which
// it is not), so the f32 accumulation is exact and the bound stays the integer inequality above; the instruction was checked
// bit for bit against an int64 GEMM first (tools/exp/mfma_fp6_exp.hip).  The tile loop is the wide form's, written once
// (wide_body) over a matrix format X: MatI8 or MatFp6 hold the operand types, the A reads, the B load, the MFMA and the
// armed value; geometry, protocol, share rule and hand-over are the same code.  The feature row keeps its 512 bytes (480
// used, see l1k2_feature6_kernel), so Stage and the workspace do not move.  l1k2_prune_plan takes FP6 exactly where `auto`
// takes the path, the form is wide and no table is named (the benchmark's shapes); prune mode 1 and a named table run the
// int8 kernels, whose decisions the case tables of the tests pin.  spv_l1k2_set_prune_matrix / SPECTAVI_L1K2_PRUNE_MATRIX
// force either, tests/test_l1k2_prune_fp6_isa.py holds the FP6 kernel's budgets (256 VGPRs, no spill, 40 MFMAs in one run).
// The two arm a tile's accumulators in different places: the int8 form at the end of the compare of the tile before, under
// its partner's MFMA run, which is the longer half-step there; the FP6 form, whose shorter run made the compare the longer
// half-step, in the tile's own top, ahead of its first MFMA (see "Arming" in wide_body; tests/test_l1k2_prune_fp6_rebalance_isa.py).
#include "common.h"
#include "l1k2_bound_fp6.h"
#include "l1k2_bound_tuned.h"

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace spv {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef int v2i __attribute__((ext_vector_type(2)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kAuxThreads = 256;              // the feature and threshold-init kernels
constexpr int kQPerWave = 64;                 // two MFMA column blocks of 32
constexpr int kFeatV4 = 32;                   // 512 feature bytes per row = 32 x 16 B
constexpr int kLdsRowV4 = kFeatV4;            // no pad: a wave's direct-to-LDS load lands 64 x 16 B in a row
constexpr int kQueue = 128;                   // < 64 queued, then <= 64 appended in one round
constexpr int kDrainBatch = 8;                // 16-byte pieces of each of a survivor's two rows requested at once
constexpr int kShareUnit = 1024;              // the break-even survivor share is passed in 1/1024
constexpr int kBreakEvenShare = 164;          // 16 %, see l1k2_prune_plan and profiles/r07_prune_breakeven.jsonl
constexpr uint32_t kMaxDist = 128 * 255;
constexpr int kStatSlots = 16;                // survivor counters, spread to keep the atomics apart
constexpr int kStatWords = kStatSlots * 4 * 2;
constexpr int kWaitVm0 = 0x0F70;              // s_waitcnt vmcnt(0), the other counters left alone

// A form of the bound kernel: H MFMA row halves of 32 rows per tile, four waves of 64 queries per half.  Narrow (H = 1)
// is l1k2_prune_kernel, Wide (H = 2) l1k2_prune_wide_kernel; the kernels, the plan and the launch take every number
// that depends on the form from here.  What the narrow form counts in tiles keeps its number of rows in the wide form:
// the threshold cadence and the warm-up of the share rule (kSkipTilesAlone is no plain halving: 2 against 3).
template <int H_>
struct PruneForm {
  static_assert(H_ == 1 || H_ == 2, "a 32- or a 64-bit survivor mask per lane");
  static constexpr int H = H_;
  static constexpr int kWaves = 4 * H;
  static constexpr int kThreads = 64 * kWaves;
  static constexpr int kQPerBlock = kWaves * kQPerWave;
  static constexpr int kTileRows = 32 * H;                 // MFMA rows
  static constexpr int kFtileV4 = kTileRows * kLdsRowV4;   // a feature tile in LDS
  static constexpr int kXrawV4 = kTileRows * 8;            // and its raw rows
  static constexpr int kRowBits = 4 + H;                   // a queue entry is query of the wave << kRowBits | row of the tile
  static constexpr int kThrEvery = 4 / H;                  // tiles between two publications of the thresholds: 128 rows
  static constexpr int kSkipTilesAlone = H == 1 ? 3 : 2;   // tiles left out of the running share while a workgroup has no thresholds at all
  static constexpr int kWarmTilesShared = 8 / H;           // ... at the break-even share, with thresholds inherited from other slices
  static constexpr int kWarmTilesAlone = 256 / H;          // ... and without: its own thresholds take thousands of rows to settle
  // up to here the end-of-tile drain takes eight lanes per pair (drain_octets), see l1k2_prune_run; for the wide form 8 / 16 / 24
  // were timed at 1M x 1M, DESIGN.md 4.1, "64-row tiles"
  static constexpr int kOctetPairs = 8;
  static constexpr bool kRaggedFromCopy = H > 1;           // see Stage::ragged_offsets
  static constexpr bool kRefreshFromCopy = false;          // see `refresh` in wide_body
  // Where wide_body arms a tile's accumulators, see "Arming" there: at the end of the compare of the tile before (false) or
  // in the tile's own top, ahead of its first MFMA (true); and, if in the top, whether the refresh of the thresholds goes
  // there with the 64 moves (true) or stays at the end of the compare (false, the split form).
  static constexpr bool kArmAtTop = false;
  static constexpr bool kRefreshAtTop = false;
};
using Narrow = PruneForm<1>;
using Wide = PruneForm<2>;
// the wide form with the FP6 bound (l1k2_prune_wide6_kernel): every number of the form, and LDS arrays of its own
#ifndef SPV_L1K2_FP6_ARM  // 0 end of compare, 1 top, 2 top with the refresh left at the end of compare; measurements only
#define SPV_L1K2_FP6_ARM 1
#endif
struct Wide6 : PruneForm<2> {
  static constexpr bool kRefreshFromCopy = true;
  static constexpr bool kArmAtTop = SPV_L1K2_FP6_ARM != 0;
  static constexpr bool kRefreshAtTop = SPV_L1K2_FP6_ARM == 1;
};

// Phase stamps (-DSPV_L1K2_PHASE_STAMPS, never in the shipped library): every wave sums the shader cycles of each
// phase of its tiles in scalar registers and lane 0 stores the sums once, when the wave ends; l1k2_prune_run
// prints their totals.  Such a build is for attribution only and is never the one that is timed: a stamp waits
// for lgkmcnt(0) and pins the schedule around it.
// The wide form has two barriers per tile: kPhBarrier is the one that ends a tile, kPhMidBarrier the one between its
// MFMA run and its compare, and kPhArm is the arming of the next tile's accumulators at the end of its compare, which
// the narrow form does in its top, kPhStage (the narrow form leaves both zero).  Where the wide form arms in the tile's own top
// (F::kArmAtTop), kPhArm is counted there and lies inside kPhStage.  kPhIssue, the wide form's alone, is the issue of the
// next tile's loads to LDS inside the top, five by a trailing wave and four by a leading one; the stamp ahead of it waits for
// the tile's first two A reads, which the unstamped top leaves in flight across the issue.
enum Phase { kPhStage, kPhMfma, kPhCompact, kPhDrain, kPhVmWait, kPhBarrier, kPhLoop, kPhMidBarrier, kPhArm, kPhIssue, kPhases };
#ifdef SPV_L1K2_PHASE_STAMPS
#define SPV_STAMP_PARAM , unsigned long long *stamps_out
#define SPV_STAMP_ARG , d_stamps
#define SPV_STAMP_PASS , stamps_out
__device__ __forceinline__ unsigned long long stamp() {
  unsigned long long v;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return v;
}
#else
#define SPV_STAMP_PARAM
#define SPV_STAMP_ARG
#define SPV_STAMP_PASS
__device__ __forceinline__ unsigned long long stamp() { return 0; }
#endif

struct FeatTable { uint32_t w[256]; };        // phi(a) packed little-endian, one dword per byte value

__global__ __launch_bounds__(kAuxThreads) void l1k2_feature_kernel(const uint32_t *__restrict__ src,
                                                                uint4 *__restrict__ dst, size_t words,
                                                                FeatTable tab) {
  __shared__ uint32_t t[256];
  t[threadIdx.x] = tab.w[threadIdx.x];
  __syncthreads();
  for (size_t e = blockIdx.x * (size_t)kAuxThreads + threadIdx.x; e < words; e += (size_t)gridDim.x * kAuxThreads) {
    const uint32_t v = src[e];
    dst[e] = make_uint4(t[v & 255], t[(v >> 8) & 255], t[(v >> 16) & 255], t[v >> 24]);
  }
}

// thresholds "none yet"; the counters and the work-list length behind them zero
__global__ __launch_bounds__(kAuxThreads) void l1k2_thr_init_kernel(uint32_t *thr, size_t nthr, size_t n) {
  for (size_t e = blockIdx.x * (size_t)kAuxThreads + threadIdx.x; e < n; e += (size_t)gridDim.x * kAuxThreads)
    thr[e] = e < nthr ? 0xFFFFFFFFu : 0u;
}

// LDS accesses of one wave are executed in order; this keeps the compiler from moving them
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// ---- exact evaluation of the newest n <= 64 queued pairs of the current tile, one per lane; queue[w] is the wave's queue,
// qslot its first query among the workgroup's top-2 slots k1s / k2s and raw rows qraw, xr the tile's raw rows, cnt
// the queue's length.  Both rows
// come from LDS in 16-byte pieces, each lane starting at a piece of its own so that the 64 rows,
// which all begin on bank 0, are not read through the same four banks.
template <int kRowBits>
__device__ __forceinline__ void drain_lanes(int n, int &cnt, int lane, const uint16_t (*queue)[kQueue], int w, int qslot, const uint4 *qraw, const uint4 *xr,
                                            unsigned long long *k1s, unsigned long long *k2s, uint32_t row0) {
  wave_lds_fence();
  const int base = cnt - n;
  if (lane < n) {
    const uint32_t e = queue[w][base + lane];
    const int q6 = e >> kRowBits, i = e & ((1 << kRowBits) - 1);
    const uint4 *qa = qraw + (qslot + q6) * 8, *xa = xr + i * 8;
    const unsigned long long k2now = k2s[qslot + q6];
    uint32_t d = 0;
    // All 16 pieces are in flight before the first is used (the accumulators and the A buffers are dead
    // here, and no register holds a staged tile): one LDS round trip for the rows.
#pragma unroll
    for (int h = 0; h < 8 / kDrainBatch; ++h) {
      uint4 a[kDrainBatch], b[kDrainBatch];
#pragma unroll
      for (int k = 0; k < kDrainBatch; ++k) {
        const int j = (kDrainBatch * h + k + lane) & 7;
        a[k] = qa[j];
        b[k] = xa[j];
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int k = 0; k < kDrainBatch; ++k) {
        d = __builtin_amdgcn_sad_u8(a[k].x, b[k].x, d);
        d = __builtin_amdgcn_sad_u8(a[k].y, b[k].y, d);
        d = __builtin_amdgcn_sad_u8(a[k].z, b[k].z, d);
        d = __builtin_amdgcn_sad_u8(a[k].w, b[k].w, d);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // a key that does not beat the query's second best of this moment never will (k2 only falls):
    // nearly all survivors end here, and the two dependent atomics are left to the few that matter
    const unsigned long long key = ((unsigned long long)d << 32) | (row0 + i);
    if (key < k2now) {
      const unsigned long long old = atomicMin(&k1s[qslot + q6], key);
      atomicMin(&k2s[qslot + q6], old > key ? old : key);
    }
  }
  cnt = base;
  wave_lds_fence();
}

// ---- the same for few pairs, eight lanes per pair and eight pairs per round: a tile of the benchmark leaves a
// handful of survivors, and one pair per lane pays 16 reads and 32 v_sad_u8 for them as for 64.  Lane 8 o + j
// holds piece j of octet o's two rows (one ds_read_b128 each), four v_sad_u8 and three DPP adds give every lane
// of the octet the distance, and the octet's first lane does the key compare and the two minima.  All lanes stay
// active (octets past the last pair repeat it and store nothing): the DPP adds read their neighbours.
// Bank conflicts: a ds_read_b128 lane group ({0-3, 12-15, 20-27} and so on) holds pieces 0-3 of two octets and
// pieces 4-7 of two others; rows are 128 B and the bank row 256 B, so the two octets that share their pieces
// collide exactly when their rows have the same parity.  Two pairs with rows of one parity cover each slot
// twice whatever the map, so 2-way is the floor there; no group ever takes more than two cycles.
template <int kRowBits>
__device__ __forceinline__ void drain_octets(int n, int &cnt, int lane, const uint16_t (*queue)[kQueue], int w, int qslot, const uint4 *qraw, const uint4 *xr,
                                             unsigned long long *k1s, unsigned long long *k2s, uint32_t row0) {
  wave_lds_fence();
  const int base = cnt - n;
  const int oct = lane >> 3, piece = lane & 7;
  for (int r = 0; r < n; r += 8) {
    const int j = r + oct;
    const uint32_t e = queue[w][base + min(j, n - 1)];
    const int q6 = e >> kRowBits, i = e & ((1 << kRowBits) - 1);
    const uint4 a = qraw[(qslot + q6) * 8 + piece], b = xr[i * 8 + piece];
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

// ======== What the two forms share, each piece once.  A kernel below shows the order of its phases, its barriers and
// what is particular to its form; everything else it takes from here, templated on its PruneForm F.

// ---- LDS of a workgroup, one set of arrays per form (a kernel's LDS is what it names of them).
// 78856 bytes in all for the narrow form, two workgroups per CU; 157704 for the wide form, one.
// 512-byte alignment: the A-operand read folds its swizzle into the address with one XOR
template <class F> __shared__ __attribute__((aligned(512))) uint4 lds_ftile[2][F::kFtileV4];  // the feature tiles, double buffered
template <class F> __shared__ unsigned long long lds_k1s[F::kQPerBlock];                      // the top-2 keys of the workgroup's queries
template <class F> __shared__ unsigned long long lds_k2s[F::kQPerBlock];
template <class F> __shared__ uint4 lds_qraw[F::kQPerBlock * 8];                              // the workgroup's query rows as they are
template <class F> __shared__ uint4 lds_xraw[2][F::kXrawV4];                                  // the tile's database rows as they are
template <class F> __shared__ uint16_t lds_queue[F::kWaves][kQueue];                          // survivors: query of the wave << kRowBits | row of the tile
template <class F> __shared__ int lds_bail[2];                                                // set in tile tl & 1: the workgroup gives the bound up

// ---- a thread's place: wave w of the workgroup and its lane; in the MFMA's C layout the lane holds column c (a query) of
// either column block and the rows of group g
template <class F>
struct Place {
  int t, w, lane, c, g;
  int qbase;  // this wave's first query
  int qslot;  // and its first top-2 slot
  __device__ __forceinline__ explicit Place(int t)
      : t(t), w(t >> 6), lane(t & 63), c(lane & 31), g(lane >> 5), qbase(blockIdx.x * F::kQPerBlock + w * kQPerWave), qslot(w * kQPerWave) {}
};

// ---- prologue: no key yet, no flag, and the workgroup's query rows (rows past the last query are copies of it)
template <class F>
__device__ __forceinline__ void prologue(int t, const uint4 *__restrict__ y, int N) {
  lds_k1s<F>[t] = ~0ull;
  lds_k2s<F>[t] = ~0ull;
  if (t < 2) lds_bail<F>[t] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int e = t + i * F::kThreads;
    lds_qraw<F>[e] = y[(size_t)min((int)blockIdx.x * F::kQPerBlock + (e >> 3), N - 1) * 8 + (e & 7)];
  }
}

// ---- staging of the database tiles, from global memory straight into LDS (global_load_lds_dwordx4): no
// registers carry the tile and no ds_write stores it.  A wave's instruction lands its 64 x 16 B one after the
// other from the base in M0, so the LDS image is lane-linear and unpadded, and the swizzle that keeps the
// A-operand reads off each other's banks is made on the source side: the lane that lands on piece j of row r
// fetches piece j ^ (r & 15), and piece q of row r is read back from slot q ^ (r & 15).  EXEC must be full at
// these loads, so rows past the end of a ragged last tile are not predicated off but clamped to the last
// row: the tile then holds copies of it, which the `valid` mask keeps out of the queue.
// The loads are one asm statement, not __builtin_amdgcn_global_load_lds: the compiler, knowing of a load to
// LDS in flight, waits for vmcnt(0) before the first LDS read that may alias it (the A operand of this very
// tile, in the other buffer) and at every workgroup fence (each drain), and turns every counted lgkmcnt wait
// of the MFMA run into lgkmcnt(0).  Unknown to it, they count on vmcnt only, behind its own loads at most,
// which can only make one of its waits longer; nothing but the s_waitcnt vmcnt(0) ahead of the tile's
// barrier makes the data visible.  M0 is the compiler's: it is put back in the same statement.
// Addresses.  The tile's first feature row and first raw row are two wave-uniform 64-bit pointers, which the
// scalar unit advances by one tile per iteration (at 4M rows the feature offset passes 2^31), and each load
// adds the lane's byte offset within the tile (global_load_lds_dwordx4 vOff, s[base:base+1]).  The five
// offsets are the same for every full tile and stay in five registers; only a ragged tile, the last of a
// slice, computes them again with the row clamp, under a wave-uniform branch around that arithmetic alone
// (no full tile follows a ragged one, so they are overwritten in place).
// A tile is F::kThreads x 16 B four times over for the features and once for the raw rows: five loads per thread.
template <class F>
struct Stage {
  uint32_t lds_f, lds_r;  // where this wave's first feature load and its raw load land in buffer 0
  uint32_t voff[5];
  int t;

  __device__ __forceinline__ Stage(const Place<F> &at) : t(at.t) {
    typedef __attribute__((address_space(3))) void *lds_ptr;
    lds_f = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_ptr)(&lds_ftile<F>[0][at.w * 64]));
    lds_r = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_ptr)(&lds_xraw<F>[0][at.w * 64]));
    lane_offsets(F::kTileRows, t);
  }
  __device__ __forceinline__ void lane_offsets(int nrows, int t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = t + i * F::kThreads, r = e >> 5;
      voff[i] = (uint32_t)(min(r, nrows - 1) * kFeatV4 + ((e & 31) ^ (r & 15))) * 16u;
    }
    voff[4] = (uint32_t)(min(t >> 3, nrows - 1) * 8 + (t & 7)) * 16u;
  }
  __device__ __forceinline__ void ragged_offsets(int nrows) {
    if (__builtin_expect(nrows < F::kTileRows, 0)) {
      // F::kRaggedFromCopy: from the thread index alone, behind a move that the compiler cannot see through: else it keeps
      // every row and piece number of the five loads in a register of its own across the loop, for a path that runs once a
      // slice.  The wide form has no such registers to spare; the narrow form has, and is kept as it was.
      int tt = t;
      if constexpr (F::kRaggedFromCopy) asm volatile("" : "+v"(tt));
      lane_offsets(nrows, tt);
    }
  }
  // all five loads of a tile of nrows rows at (ftile0, xtile0) into buffer b
  __device__ __forceinline__ void all(const uint4 *ftile0, const uint4 *xtile0, int nrows, int b) {
    ragged_offsets(nrows);
    const uint32_t f0 = lds_f + b * (F::kFtileV4 * 16), r0 = lds_r + b * (F::kXrawV4 * 16);
    uint32_t m0_kept;
    // s_nop 2: with the two s_mov ahead of it, five states between whatever wrote a base register and its first use
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %6\n\ts_nop 2\n\tglobal_load_lds_dwordx4 %1, %11\n\t"
        "s_mov_b32 m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %11\n\t"
        "s_mov_b32 m0, %8\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %11\n\t"
        "s_mov_b32 m0, %9\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %11\n\t"
        "s_mov_b32 m0, %10\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %5, %12\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(m0_kept)
        : "v"(voff[0]), "v"(voff[1]), "v"(voff[2]), "v"(voff[3]), "v"(voff[4]), "s"(f0), "s"(f0 + F::kThreads * 16u),
          "s"(f0 + F::kThreads * 32u), "s"(f0 + F::kThreads * 48u), "s"(r0), "s"(ftile0), "s"(xtile0)
        : "memory");
  }
  // The five loads in two statements as well, for waves that issue a tile's features and its raw rows at different
  // times (the wide form's leading waves).  The two in a row are not all(): each saves and restores M0.  raw() takes
  // the offset that feat()'s ragged_offsets left: the raw rows of a tile are issued after its features, and nothing
  // follows a ragged tile.
  __device__ __forceinline__ void feat(const uint4 *ftile0, int nrows, int b) {
    ragged_offsets(nrows);
    const uint32_t f0 = lds_f + b * (F::kFtileV4 * 16);
    uint32_t m0_kept;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %5\n\ts_nop 2\n\tglobal_load_lds_dwordx4 %1, %9\n\t"
        "s_mov_b32 m0, %6\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %9\n\t"
        "s_mov_b32 m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %9\n\t"
        "s_mov_b32 m0, %8\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %9\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(m0_kept)
        : "v"(voff[0]), "v"(voff[1]), "v"(voff[2]), "v"(voff[3]), "s"(f0), "s"(f0 + F::kThreads * 16u), "s"(f0 + F::kThreads * 32u),
          "s"(f0 + F::kThreads * 48u), "s"(ftile0)
        : "memory");
  }
  __device__ __forceinline__ void raw(const uint4 *xtile0, int b) {
    const uint32_t r0 = lds_r + b * (F::kXrawV4 * 16);
    uint32_t m0_kept;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\ts_nop 2\n\tglobal_load_lds_dwordx4 %1, %3\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(m0_kept)
        : "v"(voff[4]), "s"(r0), "s"(xtile0)
        : "memory");
  }
};

// ---- the lane's thresholds: a pair of query 32 b + c survives iff its sum >= tq[b] = 128 m - p thr; what is
// kept is ntq[b] = -tq[b], the value that the tile's accumulators start from.  seen[b] is the
// shared threshold read last.  Only atomicMin ever writes thr[], so a later read is never above an earlier
// one and simply replaces it (and any value ever read there is a valid bound).  The two loads are issued
// a tile ahead of the refresh that uses them, behind that tile's stage loads, and have landed by the
// vmcnt(0) before its barrier: no tile waits for them.  Lanes past the last query read the last
// query's threshold, whose features they also carry.
template <class F>
__device__ __forceinline__ void load_thresholds(uint32_t (&seen)[2], const uint32_t *thr, const Place<F> &at, int N) {
#pragma unroll
  for (int b = 0; b < 2; ++b)
    seen[b] = __hip_atomic_load(&thr[min(at.qbase + 32 * b + at.c, N - 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ntq[] from the wave's own second best and seen[]; `shared`: the own second best is published where it is lower
template <class F>
__device__ __forceinline__ void refresh_thresholds(int (&ntq)[2], const uint32_t (&seen)[2], bool shared, uint32_t *thr, const Place<F> &at, int N, int p,
                                                   int m128) {
  uint32_t loc[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    loc[b] = (uint32_t)(lds_k2s<F>[at.qslot + 32 * b + at.c] >> 32);
    // thr = "none yet" keeps every pair: sum >= 128 m - p 32640 always
    ntq[b] = p * (int)min(min(loc[b], seen[b]), kMaxDist) - m128;
  }
  if (shared && at.g == 0) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int qi = at.qbase + 32 * b + at.c;
      if (qi < N && loc[b] < seen[b]) atomicMin(&thr[qi], loc[b]);
    }
  }
}
// whether any lane of the wave has a threshold from another slice
__device__ __forceinline__ bool any_inherited(const uint32_t (&seen)[2]) {
  return __builtin_amdgcn_ballot_w64(min(seen[0], seen[1]) != 0xFFFFFFFFu) != 0ull;
}

// ---- compare and compaction.  A lane's pairs of a tile are numbered n = 32 h + 16 b + v: row half h, column block b,
// accumulator register v, which is row 32 h + 8 (v / 4) + 4 g + v % 4 of the tile; `live` has 32 H bits, pair n at bit
// 32 H - 1 - n (row half 0 on top).
template <int H>
using Live = std::conditional_t<H == 1, uint32_t, unsigned long long>;
__device__ __forceinline__ int first_pair(uint32_t live) { return __clz(live | 1u); }
__device__ __forceinline__ int first_pair(unsigned long long live) { return __clzll(live | 1ull); }

// One bit per accumulator register: the register's sign says that the pair is ruled out (sum < threshold).  The
// accumulators are int32 or, in the FP6 form, f32; an element is passed by value (a bit cast applied to the element
// expression itself reads element 0 of the vector whatever the index).
__device__ __forceinline__ uint32_t sign_word(int v) { return (uint32_t)v; }
__device__ __forceinline__ uint32_t sign_word(float v) { return __builtin_bit_cast(uint32_t, v); }
template <int H, class Acc>
__device__ __forceinline__ Live<H> fold_signs(const Acc (&acc)[H][2]) {
  Live<H> skip = 0;
#pragma unroll
  for (int h = 0; h < H; ++h) {
    uint32_t sk = 0;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
#pragma unroll
      for (int v = 0; v < 16; ++v) sk = __builtin_amdgcn_alignbit(sk, sign_word(acc[h][b][v]), 31);
    }
    if constexpr (H == 1) skip = sk;
    else skip = skip << 32 | sk;
  }
  return ~skip;
}

// Rows past the end of a ragged last tile are copies of the slice's last row and must never be taken for neighbours.
template <int H>
__device__ __forceinline__ Live<H> valid_pairs(int nrows, int g) {
  Live<H> valid = 0;
#pragma unroll
  for (int h = 0; h < H; ++h) {
#pragma unroll
    for (int v = 0; v < 16; ++v)
      if (32 * h + 8 * (v >> 2) + 4 * g + (v & 3) < nrows) valid |= (Live<H>)0x80008000u << (32 * (H - 1 - h)) >> v;
  }
  return valid;
}

// Compaction: every round each lane with survivors left appends its first one to the wave's queue (cnt entries so far),
// and 64 queued pairs are drained at once.  Returns the tile's survivors; drain_cycles is for the stamps.
// drain(n, xr, row0) is the kernel's: drain_lanes over its wave's queue.  xraw[buf] is named at the call, not once ahead
// of the loop: the drains' address arithmetic is hoisted out of the tile loop only in this form.
template <class F, class Drain>
__device__ __forceinline__ int compact(Live<F::H> live, int &cnt, const Place<F> &at, int buf, uint32_t row0, unsigned long long &drain_cycles,
                                       Drain &drain) {
  int tile_surv = 0;
  for (;;) {
    const bool has = live != 0;
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(has);
    if (mask == 0ull) break;
    const int n = first_pair(live);
    const int pos = cnt + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (has) {
      lds_queue<F>[at.w][pos] =
          (uint16_t)(((32 * ((n >> 4) & 1) + at.c) << F::kRowBits) | (32 * (n >> 5) + 8 * ((n >> 2) & 3) + 4 * at.g + (n & 3)));
      live &= ~((Live<F::H>)1 << (32 * F::H - 1) >> n);
    }
    const int add = __popcll(mask);
    cnt += add;
    tile_surv += add;
    if (cnt >= 64) {
      const unsigned long long d0 = stamp();
      drain(64, lds_xraw<F>[buf], row0);
      drain_cycles += stamp() - d0;
    }
  }
  return tile_surv;
}

// ---- the share rule.  Above the break-even share a survivor pass costs more than the exact loop saves.  A wave that
// sees that raises the flag of this tile; after the barrier the whole workgroup reads the same flag
// (the next tile uses the other one, and a flag is never lowered), puts itself on the work list of
// l1k2_tile_kernel, which then computes this (query block, slice) from scratch, and leaves.
// recent: survivors of the last tiles, each tile weighing 7/8 of the one after it: 8 x the running share.  The first
// skip_tiles tiles are left out of it; up to tile `warm` only a share of 3/4 counts (F::kSkipTilesAlone and
// F::kWarmTilesAlone, or 0 and F::kWarmTilesShared where thresholds were inherited from other slices).  The tile counters
// are never negative and are compared unsigned, which is what the compiler made of them when the rule stood in the kernel.
template <class F>
__device__ __forceinline__ int judge_share(int recent, uint32_t warm, uint32_t skip_tiles, uint32_t tl, int tile_surv, int max_share, int lane) {
  recent = tl <= skip_tiles ? 8 * tile_surv : recent + tile_surv - (recent >> 3);
  const int limit = tl >= warm ? max_share : tl > skip_tiles ? max(max_share, kShareUnit * 3 / 4) : kShareUnit;
  if (lane == 0 && recent * (kShareUnit / 8) > limit * (F::kTileRows * kQPerWave)) lds_bail<F>[tl & 1] = 1;
  return recent;
}

// ---- the epilogues, for thread t of the workgroup and its query, in slice s
// Hand-over.  What this workgroup has found still bounds its queries' second best from above: hand it on;
// the exact kernel merges into the partial pair, which starts as "none".  The work list is in query blocks of 256
// (l1k2_tile_kernel<32, 2, 128>): F::kQPerBlock / 256 entries, clipped at the last block that holds a query (the
// workgroup's first block always does).
template <class F>
__device__ __forceinline__ void hand_over(int t, int s, int N, int S, uint32_t *thr, uint32_t *work, uint64_t *__restrict__ part) {
  const int qo = blockIdx.x * F::kQPerBlock + t;
  if (qo < N) {
    const uint32_t loc = (uint32_t)(lds_k2s<F>[t] >> 32);
    if (loc < __hip_atomic_load(&thr[qo], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&thr[qo], loc);
    uint64_t *dst = part + ((size_t)qo * S + s) * 2;
    dst[0] = ~0ull;
    dst[1] = ~0ull;
  }
  if (t == 0) {
    constexpr uint32_t kBlocks = F::kQPerBlock / 256;
    const uint32_t first = kBlocks * blockIdx.x, nblk = 1 + min(kBlocks - 1, (uint32_t)((N + 255) / 256) - first - 1);
    const uint32_t slot = atomicAdd(&work[0], nblk);
#pragma unroll
    for (uint32_t i = 0; i < kBlocks; ++i) {
      if (i < nblk) {
        work[2 + 2 * (slot + i)] = first + i;
        work[3 + 2 * (slot + i)] = blockIdx.y;
      }
    }
  }
}

// Result: the query's two keys of this slice, and its second best for the slices still running.
template <class F>
__device__ __forceinline__ void write_result(int t, int s, int N, int S, uint32_t *thr, uint64_t *__restrict__ part) {
  const int qi = blockIdx.x * F::kQPerBlock + t;
  if (qi < N) {
    const unsigned long long a1 = lds_k1s<F>[t], a2 = lds_k2s<F>[t];
    uint64_t *dst = part + ((size_t)qi * S + s) * 2;
    dst[0] = a1;
    dst[1] = a2;
    const uint32_t loc = (uint32_t)(a2 >> 32);
    if (loc < __hip_atomic_load(&thr[qi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&thr[qi], loc);
  }
}

// Statistics of wave w, by one of its lanes: pairs bounded and survivors.  Returns the wave's counters; the third counts
// the pairs that a workgroup handing over leaves to the exact kernel.
__device__ __forceinline__ unsigned long long *add_stats(unsigned long long *stats, int w, unsigned long long n_bound, unsigned long long n_surv) {
  unsigned long long *st = stats + ((blockIdx.x + w) % kStatSlots) * 4;
  atomicAdd(&st[0], n_bound);
  atomicAdd(&st[1], n_surv);
  return st;
}

#ifdef SPV_L1K2_PHASE_STAMPS
// a wave's cycle sums and, behind them, a word of the form's own (the tiles it ran, at the least)
template <class F>
__device__ __forceinline__ void store_stamps(unsigned long long *stamps_out, int w, const unsigned long long (&ph)[kPhases], unsigned long long last) {
  unsigned long long *out = stamps_out + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * F::kWaves + w) * (kPhases + 1);
#pragma unroll
  for (int k = 0; k < kPhases; ++k) out[k] = ph[k];
  out[kPhases] = last;
}
#endif

// ======== The narrow form: one barrier per tile, every wave in step; a tile's thresholds and accumulators are made at its top.
__global__ __launch_bounds__(Narrow::kThreads, 2) void l1k2_prune_kernel(
    const uint4 *__restrict__ x, const uint4 *__restrict__ y, const uint4 *__restrict__ fx,
    const uint4 *__restrict__ fy, int M, int N, int slice_rows, int S, int m128, int p, int max_share, int octet_max, uint32_t *thr,
    unsigned long long *stats, uint32_t *work, uint64_t *__restrict__ part SPV_STAMP_PARAM) {
  using F = Narrow;
  const Place<F> at(threadIdx.x);
  const int s = blockIdx.y;
  const int row_begin = s * slice_rows;
  const int row_end = min(M, row_begin + slice_rows);

  prologue<F>(at.t, y, N);
  Stage<F> stage(at);
  int cnt = 0;  // the length of the wave's queue, wave-uniform
  unsigned long long ph[kPhases] = {};  // wave-uniform cycle sums, all zero and dead without the stamps
  // the survivor passes over this wave's queue, queries and top-2 slots
  auto drain = [&](int n, const uint4 *xr, uint32_t row0) {
    drain_lanes<F::kRowBits>(n, cnt, at.lane, lds_queue<F>, at.w, at.qslot, lds_qraw<F>, xr, lds_k1s<F>, lds_k2s<F>, row0);
  };
  auto drain_octets = [&](int n, const uint4 *xr, uint32_t row0) {
    spv::drain_octets<F::kRowBits>(n, cnt, at.lane, lds_queue<F>, at.w, at.qslot, lds_qraw<F>, xr, lds_k1s<F>, lds_k2s<F>, row0);
  };
  int ntq[2];
  uint32_t seen[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
  auto thr_load = [&]() { load_thresholds(seen, thr, at, N); };
  auto refresh = [&](bool shared) { refresh_thresholds(ntq, seen, shared, thr, at, N, p, m128); };

  const int ntiles = (row_end - row_begin + F::kTileRows - 1) / F::kTileRows;
  if (ntiles > 0) {
    stage.all(fx + (size_t)row_begin * kFeatV4, x + (size_t)row_begin * 8, min(F::kTileRows, row_end - row_begin), 0);
    __builtin_amdgcn_s_waitcnt(kWaitVm0);
  }
  __syncthreads();
  // the tile that the loop stages next
  const uint4 *fnext = fx + ((size_t)row_begin + F::kTileRows) * kFeatV4, *xnext = x + ((size_t)row_begin + F::kTileRows) * 8;

  unsigned long long n_bound = 0, n_surv = 0;  // wave-uniform statistics
  bool gave_up = false;                        // workgroup-uniform
  int warm = F::kWarmTilesAlone, skip_tiles = F::kSkipTilesAlone, recent = 0;  // see judge_share
  int tl = 0;
  // bail[] of the tile before, read right behind its barrier.  The index carries a zero that the compiler cannot
  // see through: a value it knows to be wave-uniform is moved to a scalar register where it is loaded, which
  // waits for it there; this one stays in its vector register until the tile's top asks for it.
  int bailed = 0, zero_v = 0;
  asm volatile("" : "+v"(zero_v));
  {
    v4i bq[2][16];
    // ---- this wave's queries as the B operand: 2 column blocks x 16 k-steps x 4 dwords
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const uint4 *f = fy + (size_t)min(at.qbase + 32 * b + at.c, N - 1) * kFeatV4;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) bq[b][ks] = __builtin_bit_cast(v4i, f[2 * ks + at.g]);
    }
    thr_load();
    // The B operand is complete before the loop is entered.  Without this wait the compiler, which cannot
    // prove on the back edge that these loads have landed, guards every MFMA of every tile with a vmcnt
    // wait, and the last of them wait for the prefetch of the next tile.
    __builtin_amdgcn_s_waitcnt(kWaitVm0);

    for (; tl < ntiles; ++tl) {
      const unsigned long long t_top = stamp();
      const unsigned long long drained = ph[kPhDrain];
      const int row0 = row_begin + tl * F::kTileRows;
      const bool has_next = tl + 1 < ntiles;
      // this lane's A-operand slot at k-step 0 in this tile's buffer: row c, piece g ^ (c & 15)
      const int a0 = (tl & 1) * F::kFtileV4 + at.c * kLdsRowV4 + (at.g ^ (at.c & 15));
      // the A operand is read two k-steps ahead of its use: a read is in flight behind every MFMA pair.  Each
      // ds_read_b128 lane group ({0-3,12-15,20-27}, {4-11,16-19,28-31} and the same of the upper half) holds 16
      // distinct c mod 16 at one g, hence 16 distinct 16-byte slots of the 256-byte bank row: no conflict.
      // Piece (2 ks + g) ^ (c & 15) = (g ^ (c & 15)) ^ 2 ks; the row and the buffer lie above those bits.
      // The first two reads are the tile's first instructions: the stage issue and the thresholds run in their
      // latency (the memory clobber of the loads keeps them ahead).
      auto lda = [&](int ks) { return __builtin_bit_cast(v4i, lds_ftile<F>[0][a0 ^ (2 * ks)]); };
      v4i a3[3];
      a3[0] = lda(0);
      a3[1] = lda(1);
      // every wave passed the barrier of tile tl - 1 after its last read of these buffers
      if (has_next) {
        stage.all(fnext, xnext, min(F::kTileRows, row_end - row0 - F::kTileRows), (tl + 1) & 1);
        fnext += F::kFtileV4;
        xnext += F::kXrawV4;
      }
      const bool shared = (tl & (F::kThrEvery - 1)) == 0;  // the shared thresholds move slowly: every fourth tile is enough
      const int nrows = min(F::kTileRows, row_end - row0);
      refresh(shared);
      if (tl == 0 && any_inherited(seen)) {
        warm = F::kWarmTilesShared;
        skip_tiles = 0;
      }
      if ((tl & (F::kThrEvery - 1)) == F::kThrEvery - 1) thr_load();  // for the next tile; they land behind this tile's work
      // The workgroup leaves after the tile whose flag was raised, before it bounds a pair of this one.  The loads
      // and the thresholds just issued are harmless: every published value is a valid bound, the exit path
      // publishes anyway, and it waits for the loads.  The flag arrived with the k2s[] that the thresholds were
      // made from; pinning them here keeps that one wait ahead of the branch (sunk below it, the reads would be
      // pending on the way out of the loop and the compiler would wait for them at every tile's top).
      asm volatile("" ::"v"(ntq[0]), "v"(ntq[1]));
      if (__builtin_amdgcn_readfirstlane(bailed)) break;

      // The accumulators start at minus the lane's threshold, so that a register ends as sum - threshold and its
      // sign bit says "ruled out" (the difference cannot overflow: make_bound).  The 32 moves stand where the
      // wave waits for its first A reads anyway, and take a subtraction per register out of the compare.
      v16i acc[1][2];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[0][b][v] = ntq[b];
      }
      const unsigned long long t_mfma = stamp();
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) {
        if (ks + 2 < 16) a3[(ks + 2) % 3] = lda(ks + 2);
        acc[0][0] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a3[ks % 3], bq[0][ks], acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a3[ks % 3], bq[1][ks], acc[0][1], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }

      const unsigned long long t_cmp = stamp();
      Live<F::H> live = fold_signs<F::H>(acc);
      if (nrows < F::kTileRows) live &= valid_pairs<F::H>(nrows, at.g);
      const int tile_surv = compact(live, cnt, at, tl & 1, (uint32_t)row0, ph[kPhDrain], drain);
      // the tile's raw rows are overwritten during the next tile: nothing stays queued
      if (cnt > 0) {
        const unsigned long long d0 = stamp();
        if (cnt <= octet_max)
          drain_octets(cnt, lds_xraw<F>[tl & 1], (uint32_t)row0);
        else
          drain(cnt, lds_xraw<F>[tl & 1], (uint32_t)row0);
        ph[kPhDrain] += stamp() - d0;
      }
      n_bound += (unsigned long long)nrows * kQPerWave;
      n_surv += tile_surv;
      recent = judge_share<F>(recent, warm, skip_tiles, tl, tile_surv, max_share, at.lane);
      const unsigned long long t_wait = stamp();
      // the next tile and the thresholds have landed: a whole tile after their loads were issued
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
      const unsigned long long t_bar = stamp();
      __syncthreads();
      const unsigned long long t_end = stamp();
      ph[kPhStage] += t_mfma - t_top;
      ph[kPhMfma] += t_cmp - t_mfma;
      ph[kPhCompact] += (t_wait - t_cmp) - (ph[kPhDrain] - drained);
      ph[kPhVmWait] += t_bar - t_wait;
      ph[kPhBarrier] += t_end - t_bar;
      ph[kPhLoop] += t_end - t_top;
      // The flag is asked for here and looked at behind the next tile's first LDS wait: no round trip of its own.
      bailed = lds_bail<F>[(tl & 1) + zero_v];
    }
    gave_up = __builtin_amdgcn_readfirstlane(bailed) != 0;  // whether it was seen at a tile's top or the slice ended with it
  }
  // a wave must not end with a load into its workgroup's LDS in flight
  if (gave_up) __builtin_amdgcn_s_waitcnt(kWaitVm0);
#ifdef SPV_L1K2_PHASE_STAMPS
  if (at.lane == 0) store_stamps<F>(stamps_out, at.w, ph, (unsigned long long)tl);
#endif
  if (gave_up) {
    hand_over<F>(at.t, s, N, S, thr, work, part);
    if (at.lane == 0) atomicAdd(&add_stats(stats, at.w, n_bound, n_surv)[2], (unsigned long long)(row_end - row_begin) * kQPerWave);
    return;
  }
  __syncthreads();
  write_result<F>(at.t, s, N, S, thr, part);
  if (at.lane == 0) add_stats(stats, at.w, n_bound, n_surv);
}

// ======== The FP6 form of a feature row (l1k2_prune_wide6_kernel; it stands behind the narrow kernel, whose pinned
// instruction stream names its function's number in every label).  A byte value has five e2m3 codes of 6 bits, and the map from
// (dimension, component) to K is component-major: k-step s of 64 holds component s / 2 of dimensions 64 (s % 2) .. + 63, so
// that lane half g's 32 values of a k-step are the codes of 32 consecutive bytes of the row, packed little-endian into 24
// bytes: chunk u = 2 s + g, component u / 4, dimensions 32 (u % 4) .. + 31.  The row keeps its 512 bytes (Stage and the
// workspace are the int8 form's): the first 16 bytes of chunk u are 16-byte piece u (bytes 0 .. 319), and the last 8 bytes of
// chunk (s, g) lie behind them in 16-byte piece 20 + 2 (s / 2) + g, half s % 2 (bytes 320 .. 479), which a lane reads at a
// constant offset from a 16-byte piece's address, see MatFp6::read_a.  Bytes 480 .. 511 are zero.
struct FeatTable6 { uint32_t w[256]; };       // the five codes of a byte value, component j at bits 6 j .. 6 j + 5
constexpr int kFeat6Chunks = 20;              // 24-byte chunks of a row
constexpr int kFeat6Tail = 320;               // where the 8-byte pieces begin
// byte of a row at which the last 8 bytes of k-step s, lane half g lie
__host__ __device__ constexpr int feat6_tail(int s, int g) { return kFeat6Tail + 32 * (s >> 1) + 16 * g + 8 * (s & 1); }

// One thread per (row, 16-byte piece of the row): pieces 0 .. 19 make a chunk each, 20 .. 29 nothing, 30 and 31 the zeros.
__global__ __launch_bounds__(kAuxThreads) void l1k2_feature6_kernel(const uint4 *__restrict__ src, uint8_t *__restrict__ dst,
                                                                    size_t rows, FeatTable6 tab) {
  __shared__ uint32_t t[256];
  t[threadIdx.x] = tab.w[threadIdx.x];
  __syncthreads();
  for (size_t e = blockIdx.x * (size_t)kAuxThreads + threadIdx.x; e < rows * 32; e += (size_t)gridDim.x * kAuxThreads) {
    const size_t row = e >> 5;
    const int u = (int)(e & 31);
    uint8_t *out = dst + row * 512;
    if (u >= 30) *reinterpret_cast<uint4 *>(out + 16 * u) = make_uint4(0, 0, 0, 0);
    if (u >= kFeat6Chunks) continue;
    const int shift = 6 * (u >> 2);
    const uint4 in[2] = {src[row * 8 + 2 * (u & 3)], src[row * 8 + 2 * (u & 3) + 1]};
    const uint32_t words[8] = {in[0].x, in[0].y, in[0].z, in[0].w, in[1].x, in[1].y, in[1].z, in[1].w};
    uint32_t w[6] = {};
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const uint32_t c = (t[(words[i >> 2] >> (8 * (i & 3))) & 255] >> shift) & 63u;
      const int bit = 6 * i;
      w[bit >> 5] |= c << (bit & 31);
      if ((bit & 31) > 26) w[(bit >> 5) + 1] |= c >> (32 - (bit & 31));
    }
    *reinterpret_cast<uint4 *>(out + 16 * u) = make_uint4(w[0], w[1], w[2], w[3]);
    *reinterpret_cast<uint2 *>(out + feat6_tail(u >> 1, u & 1)) = make_uint2(w[4], w[5]);
  }
}

// ======== The wide form: 64 database rows per loop iteration, so that what a tile costs whatever survives (the LDS round
// trips of its top, queue and drain, the two fences, the vmcnt(0) and the barrier) is paid half as often per row.
// grid = (blocks of 512 queries, slices), 8 waves of 64 queries each, one workgroup per CU; the feature tile is shared
// by 8 waves instead of being staged twice per CU.  Per tile and wave the same five loads to LDS (512 threads stage
// 64 rows), 64 MFMAs into four accumulators (row half h, column block b), a 64-bit survivor mask per lane, queue
// entries query << 6 | row.  Thresholds, share rule and hand-over keep their cadence in rows (PruneForm); a
// leaving workgroup lists its two query blocks of 256.  The shared pieces above are the narrow kernel's too; what
// stands here is the wide form's own: two barriers per tile and the half-tile stagger (below, with Buffers and Leaving),
// the arming of a tile at the end of the one before (Arming), and what its register budget asks of the source.
// LDS 157704 of 163840 bytes: ftile 2 x 64 x 512, qraw 512 x 128, xraw 2 x 64 x 128, k1s / k2s 8192, queue 2048, bail 8.
// Registers: B 128, accumulators 64, A 12, lane offsets 5 and the rest inside the 256 that 8 waves per CU allow, none
// spilled.  The accumulators are declared ahead of the tile loop and armed (set to minus the lane's thresholds) at the end
// of the tile before, see "Arming" below; between a tile's sign fold and that point, the drains among it, they are dead as
// in the narrow form, which is what lets a drain's 64 registers of row pieces fit.  To fit, the ragged tile's offsets and
// the epilogue's addresses are made again from the thread index instead of being carried across the loop.
// A tile's top is the first two A reads, the stage issue, the trailing waves' look at the flag and every second tile the
// two threshold loads; the first MFMA accumulates in place.  tests/test_l1k2_prune_arm_isa.py holds that in the assembly,
// tests/test_l1k2_prune_stagger_isa.py the half-steps.
// The tile loop is written once for both matrix formats, wide_body<F, X>: F = Wide and X = MatI8 is l1k2_prune_wide_kernel,
// F = Wide6 and X = MatFp6 is l1k2_prune_wide6_kernel, the same geometry and protocol with 40 scaled FP6 MFMAs per tile.
// One placement differs (PruneForm::kArmAtTop): with 40 MFMAs the compare is the longer half-step, and the FP6 form arms a
// tile in the tile's own top, behind the flag test and ahead of the threshold loads and the first MFMA; its top is the int8
// form's plus refresh and the 64 moves, and the end of its compare holds neither.  tests/test_l1k2_prune_fp6_rebalance_isa.py
// holds that in the assembly.

// ---- The matrix format of the wide form's bound: what a kernel's operands, accumulators and MFMAs are.
// MatI8: the rank-4 int8 table, K = 512 per pair in 16 k-steps of 32 per row half, exact in int32.
struct MatI8 {
  static constexpr int kSteps = 16;
  using Acc = v16i;
  using Op = v4i;
  struct Lane { int a0; };
  // this lane's A-operand slot at k-step 0 in the tile's buffer, as in the narrow kernel, which has the bank argument
  // (in bytes, so that each read's address is one XOR of it: with a shift behind the XOR the compiler makes the
  // second read's address in the register that the read then fills, and waits ahead of both for the flag read)
  template <class F>
  static __device__ __forceinline__ Lane lane(const Place<F> &at, int buf) {
    return {(buf * F::kFtileV4 + at.c * kLdsRowV4 + (at.g ^ (at.c & 15))) * 16};
  }
  // k-step 16 h + ks is k-step ks of row half h, 32 rows further on
  template <class F>
  static __device__ __forceinline__ Op read_a(const Lane &l, int ks) {
    return __builtin_bit_cast(v4i, *(const uint4 *)((const char *)&lds_ftile<F>[0][0] + ((l.a0 ^ (32 * (ks & 15))) + (ks >> 4) * (32 * kLdsRowV4 * 16))));
  }
  // k-step ks of feature row f (row `row` of the query set) for lane half g
  static __device__ __forceinline__ Op load_b(const uint4 *f, int row, int ks, int g) { return __builtin_bit_cast(v4i, f[2 * ks + g]); }
  static __device__ __forceinline__ Acc mfma(const Op &a, const Op &b, const Acc &c) { return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0); }
  static __device__ __forceinline__ int armed(int ntq) { return ntq; }
  static __device__ __forceinline__ void pin(Acc &, Acc &) {}
};

// MatFp6: the rank-5 e2m3 table (l1k2_bound_fp6.h), K = 640 per pair in 10 k-steps of 64 per row half:
// v_mfma_scale_f32_32x32x64_f8f6f4 with both formats FP6 (cbsz = blgp = 2) and both scales 2^0 (byte 0x7F, the same in every
// byte of the scale register whatever opsel picks).  A code is k/8, a product a multiple of 1/64, and every sum stays below
// 2^24/64 in magnitude (make_bound6), so the f32 accumulation is exact integer arithmetic in units of 1/64
// (profiles/l1k2_fp6_mfma_exp.txt has the instruction checked bit for bit against an int64 GEMM, ties on +0.0 among them): the
// accumulators start at ntq/64 and the sign bit of (ntq + sum G)/64 says "ruled out", strictly, as in the int8 form.
// An operand is the lane's 32 codes of a k-step in 6 registers, read as 16 + 8 bytes (see l1k2_feature6_kernel for the row).
// Banks.  ds_read_b128: as in the int8 form, a lane group holds 16 distinct c mod 16 at one g, and piece u = 2 ks + g lies in
// slot u ^ (c & 15) (the swizzle of Stage; 2 ks + g = 2 ks ^ g, so the address is one XOR of the lane's): for u < 16 these are
// the 16 slots of the 256-byte bank row, for u = 16 .. 19 the XOR stays inside slots 16 .. 31, again 16 distinct slots mod 16:
// no conflict.  ds_read_b64: the last 8 bytes of k-step s lie in 16-byte piece 16 + (2 t + g), t = 2 + s / 2, half s % 2: its
// slot is 16 + ((2 t + g) ^ (c & 15)), the slot of piece 2 t + g plus 256 bytes, so the read takes the address that the
// 16-byte read of k-step t has made, with 256 + 8 (s % 2) in its offset field: no address of its own and no register for
// one, which the budget does not have (with an XOR of their own the ten addresses cost ten registers and two were
// spilled).  A half wave (one g, c = 0 .. 31), 32 x 8 B being the bank row, asks for 16 slots at one half: rows c and
// c + 16 share a slot, a 2-way conflict, two more LDS cycles for each of a wave's 20 such reads per tile.  Swapping the
// halves in rows with bit 4 set would end it, and puts a lane-dependent bit 3 into the address: the ten registers again.
struct MatFp6 {
  static constexpr int kSteps = 10;
  using Acc = v16f;
  struct Op { v4i lo; v2i hi; };
  using Lane = MatI8::Lane;
  template <class F>
  static __device__ __forceinline__ Lane lane(const Place<F> &at, int buf) { return MatI8::lane(at, buf); }
  // k-step 10 h + ks is k-step ks of row half h, 32 rows further on
  template <class F>
  static __device__ __forceinline__ Op read_a(const Lane &l, int ks) {
    const int h = ks / kSteps, s = ks % kSteps;
    const char *base = (const char *)&lds_ftile<F>[0][0] + h * (32 * kLdsRowV4 * 16);
    return {__builtin_bit_cast(v4i, *(const uint4 *)(base + (l.a0 ^ (32 * s)))),
            __builtin_bit_cast(v2i, *(const uint2 *)(base + ((l.a0 ^ (32 * (2 + s / 2))) + (feat6_tail(s, 0) - 32 * (2 + s / 2)))))};
  }
  static __device__ __forceinline__ Op load_b(const uint4 *f, int row, int ks, int g) {
    return {__builtin_bit_cast(v4i, f[2 * ks + g]), __builtin_bit_cast(v2i, *(const uint2 *)((const char *)f + feat6_tail(ks, g)))};
  }
  static __device__ __forceinline__ v8i regs(const Op &o) {  // the builtin takes 8 dwords and reads 6 of them for FP6
    const v8i lo = __builtin_shufflevector(o.lo, o.lo, 0, 1, 2, 3, -1, -1, -1, -1);
    const v8i hi = __builtin_shufflevector(o.hi, o.hi, 0, 1, -1, -1, -1, -1, -1, -1);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 8, 9, -1, -1);
  }
  static __device__ __forceinline__ Acc mfma(const Op &a, const Op &b, const Acc &c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(regs(a), regs(b), c, 2, 2, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
  }
  static __device__ __forceinline__ float armed(int ntq) { return (float)ntq * (1.0f / 64); }  // |ntq| < 2^24: exact
  // A k-step's two accumulators, made where the source makes them.  Nothing but data orders an MFMA against the
  // sched_barrier of its k-step, and left to itself instruction selection puts all 40 behind the 20 A reads, which then
  // hold 120 registers at once and push the B operand out to scratch.
  static __device__ __forceinline__ void pin(Acc &c0, Acc &c1) {
    asm volatile("" : "+v"(c0));
    asm volatile("" : "+v"(c1));
  }
};

template <class F, class X>
__device__ __forceinline__ void wide_body(
    const uint4 *__restrict__ x, const uint4 *__restrict__ y, const uint4 *__restrict__ fx,
    const uint4 *__restrict__ fy, int M, int N, int slice_rows, int S, int m128, int p, int max_share, int octet_max, uint32_t *thr,
    unsigned long long *stats, uint32_t *work, uint64_t *__restrict__ part SPV_STAMP_PARAM) {
  constexpr int H = F::H;
  const Place<F> at(threadIdx.x);
  const int s = blockIdx.y;
  const int row_begin = s * slice_rows;
  const int row_end = min(M, row_begin + slice_rows);

  prologue<F>(at.t, y, N);
  Stage<F> stage(at);
  int cnt = 0;  // the length of the wave's queue, wave-uniform
  unsigned long long ph[kPhases] = {};  // wave-uniform cycle sums, all zero and dead without the stamps
  // the survivor passes over this wave's queue, queries and top-2 slots
  auto drain = [&](int n, const uint4 *xr, uint32_t row0) {
    drain_lanes<F::kRowBits>(n, cnt, at.lane, lds_queue<F>, at.w, at.qslot, lds_qraw<F>, xr, lds_k1s<F>, lds_k2s<F>, row0);
  };
  auto drain_octets = [&](int n, const uint4 *xr, uint32_t row0) {
    spv::drain_octets<F::kRowBits>(n, cnt, at.lane, lds_queue<F>, at.w, at.qslot, lds_qraw<F>, xr, lds_k1s<F>, lds_k2s<F>, row0);
  };
  int ntq[2];
  uint32_t seen[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
  auto thr_load = [&]() { load_thresholds(seen, thr, at, N); };
  // F::kRefreshFromCopy: the place made again from a copy of the thread index that the compiler cannot see through, else it
  // carries the 64-bit address of the publication's atomicMin across the loop, for a path that runs once in a while.  The FP6
  // form has no two registers to spare for it (they were spilled); the int8 form has, and is kept as it was.
  auto refresh = [&](bool shared) {
    if constexpr (F::kRefreshFromCopy) {
      int tt = at.t;
      asm volatile("" : "+v"(tt));
      refresh_thresholds(ntq, seen, shared, thr, Place<F>(tt), N, p, m128);
    } else {
      refresh_thresholds(ntq, seen, shared, thr, at, N, p, m128);
    }
  };

  const int ntiles = (row_end - row_begin + F::kTileRows - 1) / F::kTileRows;
  if (ntiles > 0) {
    stage.all(fx + (size_t)row_begin * kFeatV4, x + (size_t)row_begin * 8, min(F::kTileRows, row_end - row_begin), 0);
    __builtin_amdgcn_s_waitcnt(kWaitVm0);
  }
  __syncthreads();
  // the tile that the loop stages next
  const uint4 *fnext = fx + ((size_t)row_begin + F::kTileRows) * kFeatV4, *xnext = x + ((size_t)row_begin + F::kTileRows) * 8;

  unsigned long long n_bound = 0, n_surv = 0;  // wave-uniform statistics
  bool gave_up = false;                        // workgroup-uniform
  int warm = F::kWarmTilesAlone, skip_tiles = F::kSkipTilesAlone, recent = 0;  // see judge_share
  int tl = 0;
  int bailed = 0, zero_v = 0;  // as in the narrow kernel
  asm volatile("" : "+v"(zero_v));
  {
    typename X::Op bq[2][X::kSteps];
    // ---- this wave's queries as the B operand: 2 column blocks x the format's k-steps (16 x 4 dwords, or 10 x 6)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int row = min(at.qbase + 32 * b + at.c, N - 1);
      const uint4 *f = fy + (size_t)row * kFeatV4;
#pragma unroll
      for (int ks = 0; ks < X::kSteps; ++ks) bq[b][ks] = X::load_b(f, row, ks, at.g);
    }
    thr_load();
    __builtin_amdgcn_s_waitcnt(kWaitVm0);  // the B operand is complete before the loop is entered, as in the narrow kernel

    // ---- Two half-steps per tile, waves 4-7 half a tile behind waves 0-3.  A SIMD holds waves w and w + 4.  M(t) is
    // the top of tile t and its MFMA run (it reads ftile[t & 1]), C(t) its compare, compaction and drains (xraw[t & 1]);
    // a barrier ends each, B_h the one that ends half-step h.  The leading waves run M(t) in half-step 2t and C(t) in
    // 2t + 1, the trailing waves M(t) in 2t + 1 and C(t) in 2t + 2: on every SIMD one wave's chain runs under the
    // other's MFMAs, where in lock-step both had the pipe or neither.  The trailing waves get there by one barrier ahead
    // of their loop (B_0); the leading waves' barrier behind the loop answers the last of the trailing waves' (B_2n).
    // Every wave passes 2n + 1 of them for n tiles.
    // Buffers.  Tile t + 2 replaces tile t.  ftile[b] with tile t is read in half-steps 2t and 2t + 1: loads into it are
    // issued behind B_2t+1 and waited for ahead of B_2t+3.  xraw[b] with tile t is read in 2t + 1 and 2t + 2: issued
    // behind B_2t+2, waited for ahead of B_2t+4.  The trailing waves issue all five loads of tile t + 1 at the top of
    // M(t) (behind B_2t) and wait ahead of their mid-tile barrier B_2t+1; the leading waves issue its features at the
    // top of M(t) (behind B_2t-1), its raw rows at the top of C(t) (behind B_2t), and wait at their mid-tile barriers:
    // B_2t for the features, B_2t+2 for the raw rows.
    // Leaving.  The flag of tile t is complete at B_2t+2 and both halves read it right behind that barrier.  The
    // trailing waves are then at the top of tile t + 1 and leave before they bound a pair of it, as every wave did with
    // one barrier per tile.  The leading waves have run M(t + 1) already: they drop its accumulators (no compare, no
    // queue entry, no statistics) and leave too.  Both have passed 2t + 3 barriers.
    // Arming.  The accumulators live across the loop: a tile's MFMAs accumulate in place into registers that the end of
    // the tile before set to minus the lane's threshold (see the accumulators' comment in the narrow kernel).  arm() is
    // refresh, whose k2s[] only this wave's own drains write and whose seen[] landed at a mid-tile vmcnt(0), and the 64
    // moves; it needs no barrier, so it stands where the wave would wait for the end-of-tile barrier while the other wave
    // of its SIMD runs its MFMAs, and a tile's top is the first A reads, the stage issue and the flag test alone.
    // F::kArmAtTop (the FP6 form): the same refresh and moves stand in the tile's own top instead, behind the first A reads
    // and the stage issue and ahead of the first MFMA, where the wave waits for its LDS reads anyway.  With 40 MFMAs where
    // the int8 form has 64 the compare is the longer half-step on both wave groups, and what the arming costs there
    // bounds the tile; in M the leading waves have slack.  The decisions are the same: between the end of C(t - 1) and
    // the top of M(t) nobody writes this wave's k2s[], and seen[] is written again only by the thr_load that stands
    // behind the arming.  A trailing wave that leaves at the top leaves ahead of it; the exit path publishes anyway.
    // F::kRefreshAtTop false keeps refresh at the end of the compare and moves only the moves (ntq[] then lives across
    // the barrier); it was timed and is the slower of the two.  Estimated before it ran, with a second lever that was not
    // built: 3-7 % of the step.  Measured, best parent over worst branch at 1M x 1M: 1.024x and 1.028x on two GPUs
    // ("FP6: arming back in M").
    typename X::Acc acc[H][2];
    auto set_acc = [&]() {
#pragma unroll
      for (int h = 0; h < H; ++h) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
          for (int v = 0; v < 16; ++v) acc[h][b][v] = X::armed(ntq[b]);
          // made here: left to itself the compiler sinks the moves below the barrier that follows, into the next tile's top
          asm volatile("" : "+v"(acc[h][b]));
        }
      }
    };
    auto arm = [&](bool shared) {
      refresh(shared);
      set_acc();
    };
    // tile 0: armed here, or in its top with the rest (seen[] is complete either way: the vmcnt(0) above)
    if constexpr (!F::kArmAtTop) arm(true);
    else if constexpr (!F::kRefreshAtTop) refresh(true);
    if (any_inherited(seen)) {
      warm = F::kWarmTilesShared;
      skip_tiles = 0;
    }
    const bool trail = __builtin_amdgcn_readfirstlane(at.w) >= F::kWaves / 2;  // wave-uniform
    if (trail) __syncthreads();                                                 // B_0

    unsigned long long t_last = 0;  // stamps: the end of the tile before, so that the loop's back edge is counted too
    for (; tl < ntiles; ++tl) {
      const unsigned long long t_now = stamp(), t_top = tl ? t_last : t_now;
      const unsigned long long drained = ph[kPhDrain];
      const int row0 = row_begin + tl * F::kTileRows;
      const bool has_next = tl + 1 < ntiles;
      // this lane's A-operand addresses at k-step 0 in this tile's buffer (X::lane).
      // The first two reads are the tile's first instructions: the stage issue and the flag test run in their
      // latency (the memory clobber of the loads keeps them ahead).
      const typename X::Lane a_at = X::template lane<F>(at, tl & 1);
      auto lda = [&](int ks) { return X::template read_a<F>(a_at, ks); };
      typename X::Op a3[3];
      a3[0] = lda(0);
      a3[1] = lda(1);
      // every wave has read the last of tile tl - 1's features; only the trailing waves are behind the barrier after
      // which nobody reads its raw rows (the leading waves issue theirs behind the mid-tile barrier)
      const unsigned long long t_iss0 = stamp();
      if (has_next) {
        const int nnext = min(F::kTileRows, row_end - row0 - F::kTileRows);
        if (trail) {
          stage.all(fnext, xnext, nnext, (tl + 1) & 1);
          xnext += F::kXrawV4;
        } else {
          stage.feat(fnext, nnext, (tl + 1) & 1);
        }
        fnext += F::kFtileV4;
      }
      const unsigned long long t_iss1 = stamp();
      const int nrows = min(F::kTileRows, row_end - row0);
      // The trailing waves leave after the tile whose flag was raised, before they bound a pair of this one (a leading
      // wave gets here with `bailed` zero: it looks at the flag behind the mid-tile barrier).  The loads just issued
      // and the thresholds published at the end of the tile before are harmless: every published value is a valid
      // bound, the exit path publishes anyway, and it waits for the loads.  The flag was asked for ahead of the two A
      // reads and is looked at under a counted wait, with them still in flight; the armed accumulators are dropped.
      if (__builtin_amdgcn_readfirstlane(bailed)) break;
      // This tile's accumulators where the form arms in the top: ahead of the thr_load below, which writes seen[] again.
      // The shared thresholds are published at tile 0 and every 128 rows, as at the end of the compare.
      const unsigned long long t_arm0 = F::kArmAtTop ? stamp() : 0;
      if constexpr (F::kArmAtTop) {
        if constexpr (F::kRefreshAtTop) refresh((tl & (F::kThrEvery - 1)) == 0);
        set_acc();
      }
      const unsigned long long t_arm1 = F::kArmAtTop ? stamp() : 0;
      // for the next tile; they land behind this tile's MFMAs.  Behind the branch: on the way out of the loop no load that
      // the compiler knows of is pending, so it asks for none at the loop's end, where a leading wave has the next tile's
      // raw rows in flight.
      if ((tl & (F::kThrEvery - 1)) == F::kThrEvery - 1) thr_load();

      // Row half h of the tile (rows 32 h .. 32 h + 31) has its own pair of accumulators, armed at the end of the tile
      // before; the A reads run on across the boundary between the halves.
      const unsigned long long t_mfma = stamp();
#pragma unroll
      for (int ks = 0; ks < X::kSteps * H; ++ks) {
        if (ks + 2 < X::kSteps * H) a3[(ks + 2) % 3] = lda(ks + 2);
        acc[ks / X::kSteps][0] = X::mfma(a3[ks % 3], bq[0][ks % X::kSteps], acc[ks / X::kSteps][0]);
        acc[ks / X::kSteps][1] = X::mfma(a3[ks % 3], bq[1][ks % X::kSteps], acc[ks / X::kSteps][1]);
        X::pin(acc[ks / X::kSteps][0], acc[ks / X::kSteps][1]);
        __builtin_amdgcn_sched_barrier(0);
      }

      // The mid-tile barrier (B_2tl for the leading waves, B_2tl+1 for the trailing ones), and ahead of it the wave's one
      // wait for global memory: everything it has in flight, see "Buffers" above.
      const unsigned long long t_wait = stamp();
      __builtin_amdgcn_s_waitcnt(kWaitVm0);
      const unsigned long long t_bar = stamp();
      __syncthreads();
      const unsigned long long t_cmp = stamp();
      if (!trail) {
        // the flag of tile tl - 1 (its slot is all zero at tile 0), asked for here and, in the source, looked at behind the
        // sign fold; the compiler waits for it ahead of the fold, and pinned behind it the FP6 step was 1-2 % slower;
        // the raw rows of tile tl + 1 go where the trailing waves have just finished C(tl - 1)
        bailed = lds_bail<F>[((tl + 1) & 1) + zero_v];
        if (has_next) {
          stage.raw(xnext, (tl + 1) & 1);
          xnext += F::kXrawV4;
        }
      }
      Live<H> live = fold_signs<H>(acc);
      // a leading wave drops the tile whose MFMAs it ran while the flag was being raised, and leaves
      if (__builtin_amdgcn_readfirstlane(bailed)) break;
      if (nrows < F::kTileRows) live &= valid_pairs<H>(nrows, at.g);
      const int tile_surv = compact(live, cnt, at, tl & 1, (uint32_t)row0, ph[kPhDrain], drain);
      // the tile's raw rows are overwritten during the next tile: nothing stays queued
      if (cnt > 0) {
        const unsigned long long d0 = stamp();
        if (cnt <= octet_max)
          drain_octets(cnt, lds_xraw<F>[tl & 1], (uint32_t)row0);
        else
          drain(cnt, lds_xraw<F>[tl & 1], (uint32_t)row0);
        ph[kPhDrain] += stamp() - d0;
      }
      n_bound += (unsigned long long)nrows * kQPerWave;
      n_surv += tile_surv;
      recent = judge_share<F>(recent, warm, skip_tiles, tl, tile_surv, max_share, at.lane);
      // The next tile's accumulators, from the second best that this tile's drains left and the shared thresholds that
      // landed at its mid-tile wait.  Armed behind the last tile too, where nobody reads them and nothing is published:
      // under `if (has_next)` the accumulators of the path not taken stay live across the drains, which need their
      // registers for the rows' pieces, and 50 registers spill.
      // Where the form arms in the top, nothing of it stands here, or the refresh alone.
      const unsigned long long t_arm = stamp();
      const bool share_next = has_next && ((tl + 1) & (F::kThrEvery - 1)) == 0;  // the shared thresholds move slowly: every 128 rows is enough
      if constexpr (!F::kArmAtTop) arm(share_next);
      else if constexpr (!F::kRefreshAtTop) refresh(share_next);
      const unsigned long long t_bar2 = stamp();
      __syncthreads();  // B_2tl+1 for the leading waves, B_2tl+2 for the trailing ones
      const unsigned long long t_end = stamp();
      ph[kPhStage] += t_mfma - t_top;
      ph[kPhMfma] += t_wait - t_mfma;
      ph[kPhVmWait] += t_bar - t_wait;
      ph[kPhMidBarrier] += t_cmp - t_bar;
      ph[kPhCompact] += (t_arm - t_cmp) - (ph[kPhDrain] - drained);
      ph[kPhArm] += (t_bar2 - t_arm) + (t_arm1 - t_arm0);  // the second part lies inside the top's count
      ph[kPhBarrier] += t_end - t_bar2;
      ph[kPhIssue] += t_iss1 - t_iss0;
      ph[kPhLoop] += t_end - t_top;
      t_last = t_end;
      // A trailing wave asks for this tile's flag here, complete at the barrier it has just passed, and looks at it
      // behind the next tile's first LDS wait: no round trip of its own.
      if (trail) bailed = lds_bail<F>[(tl & 1) + zero_v];
    }
    // B_2n, which the trailing waves passed as the last of their loop, and behind it the last tile's flag.  A leading
    // wave that left the loop with the flag up has passed as many barriers as the trailing waves that left at the top
    // of the same tile: it takes none here.
    if (!trail && !__builtin_amdgcn_readfirstlane(bailed)) {
      __syncthreads();
      bailed = lds_bail<F>[((tl + 1) & 1) + zero_v];
    }
    gave_up = __builtin_amdgcn_readfirstlane(bailed) != 0;  // whether it was seen inside the loop or the slice ended with it
  }
  // a wave must not end with a load into its workgroup's LDS in flight
  if (gave_up) __builtin_amdgcn_s_waitcnt(kWaitVm0);
  // What follows the loop works from a copy of the thread index that the compiler cannot see through: made from t
  // itself, its LDS addresses and the wave's number are held in registers across the loop, which has none to spare.
  int te = at.t;
  asm volatile("" : "+v"(te));
  const int we = te >> 6;
#ifdef SPV_L1K2_PHASE_STAMPS
  // behind the tiles this wave ran, the SIMD it ran on (HW_ID bits 5:4): the half-steps count on waves w and w + 4 sharing one
  if (at.lane == 0)
    store_stamps<F>(stamps_out, at.w, ph,
                    (unsigned long long)tl | (unsigned long long)(__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4) & 3) << 32);
#endif
  if (gave_up) {
    hand_over<F>(te, s, N, S, thr, work, part);
    if ((te & 63) == 0) atomicAdd(&add_stats(stats, we, n_bound, n_surv)[2], (unsigned long long)(row_end - row_begin) * kQPerWave);
    return;
  }
  // no barrier here: k1s[te] and k2s[te] are this wave's own queries'
  write_result<F>(te, s, N, S, thr, part);
  if ((te & 63) == 0) add_stats(stats, we, n_bound, n_surv);
}

// __launch_bounds__' second argument is waves per SIMD here: 512 threads are two per SIMD already.
__global__ __launch_bounds__(Wide::kThreads, 2) void l1k2_prune_wide_kernel(
    const uint4 *__restrict__ x, const uint4 *__restrict__ y, const uint4 *__restrict__ fx,
    const uint4 *__restrict__ fy, int M, int N, int slice_rows, int S, int m128, int p, int max_share, int octet_max, uint32_t *thr,
    unsigned long long *stats, uint32_t *work, uint64_t *__restrict__ part SPV_STAMP_PARAM) {
  wide_body<Wide, MatI8>(x, y, fx, fy, M, N, slice_rows, S, m128, p, max_share, octet_max, thr, stats, work, part SPV_STAMP_PASS);
}

// The FP6 form.  Registers: B 120 (2 x 10 x 6), accumulators 64, A 18 (3 x 6); LDS as the int8 form's.  m128 and p are the FP6
// table's, in units of 1/64.
__global__ __launch_bounds__(Wide6::kThreads, 2) void l1k2_prune_wide6_kernel(
    const uint4 *__restrict__ x, const uint4 *__restrict__ y, const uint4 *__restrict__ fx,
    const uint4 *__restrict__ fy, int M, int N, int slice_rows, int S, int m128, int p, int max_share, int octet_max, uint32_t *thr,
    unsigned long long *stats, uint32_t *work, uint64_t *__restrict__ part SPV_STAMP_PARAM) {
  wide_body<Wide6, MatFp6>(x, y, fx, fy, M, N, slice_rows, S, m128, p, max_share, octet_max, thr, stats, work, part SPV_STAMP_PASS);
}

// -1 auto, 0 off, 1 forced: SPECTAVI_L1K2_PRUNE until l1k2_set_prune is called
std::atomic<int> &prune_mode() {
  static std::atomic<int> mode{l1k2_knobs().prune};
  return mode;
}

// -1 default, 0 recipe, 1 tuned: SPECTAVI_L1K2_BOUND until l1k2_set_bound is called
std::atomic<int> &bound_choice() {
  static std::atomic<int> which{l1k2_knobs().bound};
  return which;
}

// p, m and the verdict for a finished int8 table, p swept over [p_lo, p_hi).  Nothing about a table is trusted:
// whatever produced it, the path runs only if the inequality holds on every byte pair and nothing can overflow.
L1K2Bound make_bound(const int8_t phi[256][4], int p_lo, int p_hi) {
  L1K2Bound b{};
  for (int a = 0; a < 256; ++a)
    for (int f = 0; f < 4; ++f) b.phi[a][f] = phi[a][f];
  std::vector<int> Gv(256 * 256);
  int(*G)[256] = reinterpret_cast<int(*)[256]>(Gv.data());
  long long sumG = 0;
  for (int a = 0; a < 256; ++a)
    for (int c = 0; c < 256; ++c) {
      int g = 0;
      for (int f = 0; f < 4; ++f) g += (int)b.phi[a][f] * (int)b.phi[c][f];
      G[a][c] = g;
      sumG += g;
    }
  // the slope whose bound is largest on average over all byte pairs: mean of (m_p - G) / p
  double best = -1e300;
  for (int p = p_lo; p < p_hi; ++p) {
    int m = 0x7FFFFFFF;
    for (int a = 0; a < 256; ++a)
      for (int c = 0; c < 256; ++c) m = std::min(m, p * std::abs(a - c) + G[a][c]);
    const double mean = (65536.0 * m - (double)sumG) / p;
    if (mean > best) {
      best = mean;
      b.p = p;
      b.m = m;
    }
  }
  // the path is refused unless the inequality holds on every byte pair and nothing can overflow
  b.ok = true;
  for (int a = 0; a < 256; ++a)
    for (int c = 0; c < 256; ++c)
      if ((long long)b.p * std::abs(a - c) < (long long)b.m - G[a][c] || std::abs(G[a][c]) >= (1 << 24) / 128 * 128)
        b.ok = false;
  if ((long long)b.p * kMaxDist + 128ll * std::abs(b.m) >= 0x7FFFFFFFll) b.ok = false;
  return b;
}

// -1 default, 0 narrow, 1 wide: SPECTAVI_L1K2_PRUNE_FORM until l1k2_set_prune_form is called
std::atomic<int> &form_choice() {
  static std::atomic<int> which{l1k2_knobs().prune_form};
  return which;
}

// -1 default, 0 int8, 1 FP6: SPECTAVI_L1K2_PRUNE_MATRIX until l1k2_set_prune_matrix is called
std::atomic<int> &matrix_choice() {
  static std::atomic<int> which{l1k2_knobs().prune_matrix};
  return which;
}

// make_bound for the FP6 table: the entries are the integers k of e2m3 values k/8, so G, p and m are integers in units of
// 1/64 and the inequality is the same integer one.  Refused unless every entry is on the e2m3 grid (|k| in 0..15, 16..30
// step 2, 32..60 step 4), the inequality holds on every byte pair, and 128 m, p 128 255 and the largest |sum G| of a
// 128-byte pair stay below 2^24: then every value the f32 accumulators ever hold is a multiple of 1/64 below 2^24/64 in
// magnitude, and their arithmetic is exact.
L1K2Bound6 make_bound6(const int8_t k[256][5], int p_lo, int p_hi) {
  L1K2Bound6 b{};
  b.ok = true;
  for (int a = 0; a < 256; ++a)
    for (int f = 0; f < 5; ++f) {
      const int v = b.k[a][f] = k[a][f], mag = std::abs(v);
      if (mag > 60 || (mag >= 16 && mag % 2) || (mag >= 32 && mag % 4)) b.ok = false;
    }
  std::vector<int> Gv(256 * 256);
  int(*G)[256] = reinterpret_cast<int(*)[256]>(Gv.data());
  long long sumG = 0;
  int maxG = 0;
  for (int a = 0; a < 256; ++a)
    for (int c = 0; c < 256; ++c) {
      int g = 0;
      for (int f = 0; f < 5; ++f) g += (int)b.k[a][f] * (int)b.k[c][f];
      G[a][c] = g;
      sumG += g;
      maxG = std::max(maxG, std::abs(g));
    }
  // the slope whose bound is largest on average over all byte pairs, as in make_bound
  double best = -1e300;
  for (int p = p_lo; p < p_hi; ++p) {
    int m = 0x7FFFFFFF;
    for (int a = 0; a < 256; ++a)
      for (int c = 0; c < 256; ++c) m = std::min(m, p * std::abs(a - c) + G[a][c]);
    const double mean = (65536.0 * m - (double)sumG) / p;
    if (mean > best) {
      best = mean;
      b.p = p;
      b.m = m;
    }
  }
  for (int a = 0; a < 256; ++a)
    for (int c = 0; c < 256; ++c)
      if ((long long)b.p * std::abs(a - c) < (long long)b.m - G[a][c]) b.ok = false;
  if (128ll * std::abs(b.m) >= (1 << 24) || (long long)b.p * kMaxDist >= (1 << 24) || 128ll * maxG >= (1 << 24)) b.ok = false;
  return b;
}

// a 6-bit e2m3 code: sign, two exponent bits, three mantissa bits; the value is k/8
uint32_t e2m3_code(int k) {
  const uint32_t mag = (uint32_t)std::abs(k);
  return (k < 0 ? 32u : 0u) | (mag < 16 ? mag : mag < 32 ? mag / 2 + 8 : mag / 4 + 16);
}

FeatTable6 feat_table6(const L1K2Bound6 &b) {
  FeatTable6 t;
  for (int a = 0; a < 256; ++a) {
    t.w[a] = 0;
    for (int f = 0; f < 5; ++f) t.w[a] |= e2m3_code(b.k[a][f]) << (6 * f);
  }
  return t;
}

L1K2Bound make_recipe() {
  int8_t phi[256][4];
  const double pi = 3.14159265358979323846;
  for (int a = 0; a < 256; ++a) {
    phi[a][0] = (int8_t)std::nearbyint(127.0 * std::cos(pi * a / 255.0));
    phi[a][1] = (int8_t)std::nearbyint(127.0 * std::sin(pi * a / 255.0));
    phi[a][2] = (int8_t)std::nearbyint(127.0 * std::cos(3.0 * pi * a / 255.0) / 3.0);
    phi[a][3] = (int8_t)std::nearbyint(127.0 * std::sin(3.0 * pi * a / 255.0) / 3.0);
  }
  return make_bound(phi, 100, 260);
}

FeatTable feat_table(const L1K2Bound &b) {
  FeatTable t;
  for (int a = 0; a < 256; ++a)
    t.w[a] = (uint32_t)(uint8_t)b.phi[a][0] | (uint32_t)(uint8_t)b.phi[a][1] << 8 | (uint32_t)(uint8_t)b.phi[a][2] << 16 |
             (uint32_t)(uint8_t)b.phi[a][3] << 24;
  return t;
}

}  // namespace

const L1K2Bound &l1k2_bound() {
  static const L1K2Bound b = make_recipe();
  return b;
}

// The tuned table (tools/l1k2_bound_tune.py) lets about a tenth of the recipe's pairs through on uniform bytes.
// Its sweep of p is wider than the recipe's, whose range the recipe's tests pin.
const L1K2Bound &l1k2_bound_of(int which) {
  if (which != kL1K2BoundTuned) return l1k2_bound();
  static const L1K2Bound tuned = make_bound(kL1K2BoundTunedPhi, 64, 400);
  return tuned.ok ? tuned : l1k2_bound();
}

// p is swept as tools/l1k2_bound_tune.py sweeps it for this table
const L1K2Bound6 &l1k2_bound6() {
  static const L1K2Bound6 b = make_bound6(kL1K2BoundFp6K, 8, 200);
  return b;
}

int l1k2_set_prune(int mode) { return prune_mode().exchange(mode); }
int l1k2_get_prune() { return prune_mode().load(); }
int l1k2_set_bound(int which) { return bound_choice().exchange(which); }
int l1k2_get_bound() { return bound_choice().load(); }
int l1k2_set_prune_form(int form) { return form_choice().exchange(form); }
int l1k2_get_prune_form() { return form_choice().load(); }
int l1k2_set_prune_matrix(int matrix) { return matrix_choice().exchange(matrix); }
int l1k2_get_prune_matrix() { return matrix_choice().load(); }

namespace {
// where the counters of the calling thread's last l1k2_run lie (null: it took the tile kernels)
thread_local const unsigned long long *t_last_stats = nullptr;
thread_local hipStream_t t_last_stream = nullptr;

int read_stats(const unsigned long long *d_stats, hipStream_t stream, unsigned long long out[3]) {
  out[0] = out[1] = out[2] = 0;
  if (!d_stats) return SPV_OK;
  unsigned long long raw[kStatSlots * 4];
  SPV_HIP_CHECK(hipStreamSynchronize(stream));
  SPV_HIP_CHECK(hipMemcpy(raw, d_stats, sizeof raw, hipMemcpyDeviceToHost));
  for (int i = 0; i < kStatSlots; ++i)
    for (int k = 0; k < 3; ++k) out[k] += raw[4 * i + k];
  return SPV_OK;
}
}  // namespace

void l1k2_prune_note_run(const void *d_stats, hipStream_t stream) {
  t_last_stats = static_cast<const unsigned long long *>(d_stats);
  t_last_stream = stream;
}

int l1k2_prune_last_stats(unsigned long long out[3]) { return read_stats(t_last_stats, t_last_stream, out); }

// When `auto` takes the path (tools/l1k2_prune_sweep.py, tools/l1k2_prune_breakeven.py; profiles/r07_*):
//  * The gain comes with the number of database slices that hand thresholds on: 0.95x at 128k x 128k,
//    1.16x at 256k x 256k, 1.35x at 512k x 512k, 1.44x at 1M x 1M on uniform bytes.
//  * What the path costs when the bound does not pay is the tiles a workgroup spends finding that out, at up
//    to 4.3x the exact cost per pair (all pairs surviving), before it hands its slice to the tile kernel.
//    With the plan's 8192-row slices at 256k x 256k that was +16 %; it is bounded by 8 of a slice's tiles,
//    so `auto` asks for slices of at least 1024 tiles (the plan gives them from about 512k x 512k on).
//  * Break-even: with the fallback off the path ties with the tile kernel at an average survivor share of
//    about 9 % (uniform bytes in [0, 224): 11.8 %, 72.5 ms against 61.7 ms; [0, 256): 5.7 %, 54 ms) and a
//    workgroup of the early slices sees about twice the average.  A workgroup hands over when its running
//    share exceeds 16 % (kBreakEvenShare; judged from its 8th tile on with inherited thresholds, from its 256th
//    without, while its own thresholds settle), or 3/4 right after its first tiles.
//    Since the waits were taken out of the kernel the tie is at about 11 % (47.0 / 63.8 ms at shares 5.7 / 11.7 %
//    against 62.0 ms, profiles/r08_prune_breakeven_knobs.jsonl); the rule was left as it is, its cost on inputs
//    that do not pay has not grown (profiles/r08_prune_breakeven.jsonl).
constexpr int kPruneMinX = 262144, kPruneMinSlice = 32768;
// The wide form holds a CU with one workgroup: it is taken where there is at least this many of them (four per CU).
constexpr unsigned kWideMinGroups = 1024;

void l1k2_prune_plan(int xrows, int yrows, int dim, WsWalk *w, L1K2Plan *p) {
  p->off_feat_x = p->off_feat_y = p->off_thr = p->off_stats = p->off_work = w->end();
  if (dim != 128 || xrows < Narrow::kTileRows || yrows < 1) return;  // no such path, no scratch
  // The scratch is a function of the shape alone, whether or not the path is switched on: the features, then
  // one block of dwords: thresholds (an even number: the counters are 64-bit), the counters, the work list
  // (its length, then one (query block, slice) pair for each workgroup there can be).
  const unsigned qgroups = (unsigned)((yrows + Narrow::kQPerBlock - 1) / Narrow::kQPerBlock);
  p->thr_words = ((size_t)yrows + 1) / 2 * 2;
  p->init_words = p->thr_words + kStatWords + 2;
  p->off_feat_x = w->reserve((size_t)xrows * 512);
  p->off_feat_y = w->reserve((size_t)yrows * 512);
  p->off_thr = w->reserve((p->init_words + 2 * (size_t)qgroups * p->slices) * 4);
  p->off_stats = p->off_thr + p->thr_words * 4;
  p->off_work = p->off_stats + kStatWords * 4;
  const int mode = l1k2_get_prune();
  const bool wanted = mode == 1 || (mode != 0 && xrows >= kPruneMinX && p->slice_rows >= kPruneMinSlice);
  // The table: as set, else the tuned one where `auto` takes the path and the recipe where the path is forced
  // (mode 1 is what the case tables of the tests run, with survivor counts worked out from the recipe).
  const int which = l1k2_get_bound();
  p->bound = which >= 0 ? which : mode == 1 ? kL1K2BoundRecipe : kL1K2BoundTuned;
  if (p->bound == kL1K2BoundTuned && &l1k2_bound_of(kL1K2BoundTuned) == &l1k2_bound()) p->bound = kL1K2BoundRecipe;
  if (wanted && l1k2_bound_of(p->bound).ok) {
    p->path = kL1K2Bound;
    p->bound_grid = dim3(qgroups, (unsigned)p->slices);
    // The form: as set, else the wide one where `auto` took the path and its grid fills the chip.  Mode 1 stays narrow:
    // the case tables of the tests pin what l1k2_prune_kernel decides per 32-row tile and 256-query workgroup.
    const unsigned wgroups = (unsigned)((yrows + Wide::kQPerBlock - 1) / Wide::kQPerBlock);
    const int form = l1k2_get_prune_form();
    p->form = form >= 0 ? form : mode != 1 && (unsigned long long)wgroups * p->slices >= kWideMinGroups ? kL1K2FormWide : kL1K2FormNarrow;
    p->bound_wide_grid = dim3(wgroups, (unsigned)p->slices);
    // The matrix format: as set where the form is wide, else FP6 exactly where `auto` took the path and nobody named a
    // table.  Mode 1 and an explicit table stay int8: the case tables and model statistics of the tests are worked out
    // from the int8 tables.  An FP6 table that fails its check leaves everything to the int8 kernel.
    const int matrix = l1k2_get_prune_matrix();
    const bool fp6 = matrix >= 0 ? matrix == kL1K2MatrixFp6 : mode != 1 && which < 0;
    p->matrix = fp6 && p->form == kL1K2FormWide && l1k2_bound6().ok ? kL1K2MatrixFp6 : kL1K2MatrixI8;
  }
}

int l1k2_prune_run(const uint8_t *d_x, const uint8_t *d_y, int xrows, int yrows, const L1K2Plan &p, uint8_t *ws,
                   hipStream_t stream) {
  const L1K2Bound &b = l1k2_bound_of(p.bound);
  if (!b.ok) return set_error(SPV_ERR_INTERNAL, "the L1 bound table failed its own check");
  const bool fp6 = p.matrix == kL1K2MatrixFp6;
  const L1K2Bound6 &b6 = l1k2_bound6();
  if (fp6 && !(b6.ok && p.form == kL1K2FormWide)) return set_error(SPV_ERR_INTERNAL, "the FP6 bound was planned where it cannot run");
  uint4 *fx = reinterpret_cast<uint4 *>(ws + p.off_feat_x);
  uint4 *fy = reinterpret_cast<uint4 *>(ws + p.off_feat_y);
  uint32_t *thr = reinterpret_cast<uint32_t *>(ws + p.off_thr);
  unsigned long long *stats = reinterpret_cast<unsigned long long *>(ws + p.off_stats);
  uint32_t *work = reinterpret_cast<uint32_t *>(ws + p.off_work);

  static const FeatTable tabs[2] = {feat_table(l1k2_bound_of(kL1K2BoundRecipe)), feat_table(l1k2_bound_of(kL1K2BoundTuned))};
  const FeatTable &tab = tabs[p.bound == kL1K2BoundTuned];
  // Survivor share (in 1/1024 of a tile's pairs) above which a wave finishes its slice exactly.
  // SPECTAVI_L1K2_PRUNE_SHARE overrides it for measurements (tools/l1k2_prune_breakeven.py): 0 = every
  // wave leaves the bound after the warm-up tiles, 1024 = never.  The 3/4 rule of the first tiles yields to a
  // larger value, so that 1024 really means never: before, a workgroup whose pairs all survived still left
  // at its tile 4 and "fallback disabled" measured the exact kernel (profiles/r12_l1k2_prune_shapes.txt).
  const int share = l1k2_knobs().prune_share;
  const int max_share = share < 0 ? kBreakEvenShare : std::min(kShareUnit, share);
  // Most pairs for which the end-of-tile survivor pass takes eight lanes per pair; SPECTAVI_L1K2_PRUNE_OCTET overrides it
  // for measurements (0 = always one pair per lane, 64 = always octets).  One round of eight pairs: with the hand-over off
  // at 256k x 256k, 12 and 22 survivors per wave and tile on average, 0 / 8 / 16 / 24 / 32 / 64 gave 33.7 / 33.5 / 33.9 /
  // 34.2 / 34.3 / 34.5 ms and 34.7 / - / 34.9 / - / 36.5 / 37.3 ms (profiles/r16_prune_octet_crossover.jsonl): the rounds
  // wait for each other.  At 1M x 1M (four pairs per wave and tile on average) 8, 16 and 24 were timed against each other
  // on one build: DESIGN.md 4.1, "The wave's chain per tile", has the three numbers.
  const int octet = l1k2_knobs().prune_octet;
  const bool wide = p.form == kL1K2FormWide;
  const int octet_max = octet < 0 ? (wide ? Wide::kOctetPairs : Narrow::kOctetPairs) : std::min(64, octet);
  const dim3 grid = wide ? p.bound_wide_grid : p.bound_grid;
  const int waves = wide ? Wide::kWaves : Narrow::kWaves;
  const size_t xw = (size_t)xrows * 32, yw = (size_t)yrows * 32;
  auto blocks = [](size_t n) { return dim3((unsigned)std::min<size_t>((n + kAuxThreads - 1) / kAuxThreads, 8192)); };
  if (fp6) {
    static const FeatTable6 tab6 = feat_table6(l1k2_bound6());
    hipLaunchKernelGGL(l1k2_feature6_kernel, blocks(xw), dim3(kAuxThreads), 0, stream, reinterpret_cast<const uint4 *>(d_x),
                       reinterpret_cast<uint8_t *>(fx), (size_t)xrows, tab6);
    hipLaunchKernelGGL(l1k2_feature6_kernel, blocks(yw), dim3(kAuxThreads), 0, stream, reinterpret_cast<const uint4 *>(d_y),
                       reinterpret_cast<uint8_t *>(fy), (size_t)yrows, tab6);
  } else {
    hipLaunchKernelGGL(l1k2_feature_kernel, blocks(xw), dim3(kAuxThreads), 0, stream, reinterpret_cast<const uint32_t *>(d_x), fx,
                       xw, tab);
    hipLaunchKernelGGL(l1k2_feature_kernel, blocks(yw), dim3(kAuxThreads), 0, stream, reinterpret_cast<const uint32_t *>(d_y), fy,
                       yw, tab);
  }
  hipLaunchKernelGGL(l1k2_thr_init_kernel, blocks(p.init_words), dim3(kAuxThreads), 0, stream, thr, p.thr_words,
                     p.init_words);
#ifdef SPV_L1K2_PHASE_STAMPS
  const size_t nstamp = (size_t)grid.x * grid.y * waves * (kPhases + 1);
  unsigned long long *d_stamps = nullptr;
  SPV_HIP_CHECK(hipMalloc(&d_stamps, nstamp * 8));
  SPV_HIP_CHECK(hipMemsetAsync(d_stamps, 0, nstamp * 8, stream));
#endif
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(waves * 64), 0, stream, reinterpret_cast<const uint4 *>(d_x),
                       reinterpret_cast<const uint4 *>(d_y), fx, fy, xrows, yrows, p.slice_rows, p.slices, fp6 ? 128 * b6.m : 128 * b.m,
                       fp6 ? b6.p : b.p,
                       max_share, octet_max, thr, stats, work, reinterpret_cast<uint64_t *>(ws + p.off_part) SPV_STAMP_ARG);
  };
  if (fp6) launch(l1k2_prune_wide6_kernel);
  else if (wide) launch(l1k2_prune_wide_kernel);
  else launch(l1k2_prune_kernel);
  SPV_HIP_CHECK(hipGetLastError());
#ifdef SPV_L1K2_PHASE_STAMPS
  {
    // the narrow form's top holds its refresh and accumulator set-up as well, and its arming line is zero
    // and where the wide form armed: at the end of the compare (its own line of the tile), or inside the top, whose line
    // then holds the arming's cycles as well
    const char *const names[kPhases] = {"top: reads, stage issue", "MFMA run", "compare + compaction", "drains",
                                        "vmcnt(0) wait", "barrier wait", "whole tile", "mid-tile barrier wait",
                                        !(fp6 && Wide6::kArmAtTop) ? "arming (end of compare)"
                                        : Wide6::kRefreshAtTop     ? "arming (inside the top)"
                                                                   : "arming (moves in the top)",
                                        "stage issue (in the top)"};
    std::vector<unsigned long long> h(nstamp);
    SPV_HIP_CHECK(hipStreamSynchronize(stream));
    SPV_HIP_CHECK(hipMemcpy(h.data(), d_stamps, nstamp * 8, hipMemcpyDeviceToHost));
    SPV_HIP_CHECK(hipFree(d_stamps));
    // the wide form per half of its workgroup: waves 0-3 lead, waves 4-7 trail by half a tile; a wave's last word holds
    // its tiles and, above them, the SIMD it ran on
    const int groups = wide ? 2 : 1;
    // (a workgroup's first wave starts on any SIMD; what the half-steps count on is that waves w and w + 4 share one)
    unsigned long long sum[2][kPhases + 1] = {}, apart = 0;
    for (size_t i = 0; i < nstamp; ++i) {
      const size_t k = i % (kPhases + 1), w = i / (kPhases + 1) % waves;
      sum[w * groups / waves][k] += k < kPhases ? h[i] : h[i] & 0xFFFFFFFFull;
      if (k == kPhases && wide && w < 4 && (h[i] >> 32) != (h[i + 4 * (kPhases + 1)] >> 32)) ++apart;
    }
    for (int g = 0; g < groups; ++g) {
      const double tiles = (double)std::max(1ull, sum[g][kPhases]);
      fprintf(stderr, "l1k2_prune phase stamps, %d x %d, waves %d-%d: %llu wave-tiles\n", xrows, yrows, g * waves / groups,
              (g + 1) * waves / groups - 1, sum[g][kPhases]);
      for (int k = 0; k < kPhases; ++k)
        fprintf(stderr, "  %-24s %14llu cycles  %8.1f per wave-tile  %5.1f %%\n", names[k], sum[g][k], sum[g][k] / tiles,
                100.0 * sum[g][k] / (double)std::max(1ull, sum[g][kPhLoop]));
    }
    if (wide) fprintf(stderr, "  waves w < 4 not on the SIMD of wave w + 4: %llu of %zu\n", apart, nstamp / (kPhases + 1) / 2);
  }
#endif
  if (l1k2_knobs().prune_stats) {  // debugging aid: synchronises
    unsigned long long h[3];
    SPV_TRY(read_stats(stats, stream, h));
    fprintf(stderr, "l1k2_prune %d x %d: bounded %llu pairs, %llu survived (%.4f), %llu evaluated by the exact fallback\n",
            xrows, yrows, h[0], h[1], h[0] ? (double)h[1] / (double)h[0] : 0.0, h[2]);
  }
  return SPV_OK;
}

}  // namespace spv
