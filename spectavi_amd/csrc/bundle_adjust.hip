// bundle_adjust.hip -- Levenberg-Marquardt refinement of cameras and track points, on the device (gfx950).
//
// tracks_triangulate.hip gives every track a linear DLT point and resect_batch.hip every view a minimal-sample camera;
// this file refines all free cameras and all participating points jointly over all observations.  The contract (the
// residual model, who takes part, the loop and its stops) is stated in include/spectavi_amd.h, and
// tests/bundle_model.py restates it in numpy with dense normal equations.  The reference has no such step.
//
// The solver is the matrix-free Schur complement of Wu et al., "Multicore Bundle Adjustment", and Agarwal et al.,
// "Bundle Adjustment in the Large".  With J~ = [Jc Jp] the weighted Jacobian, U_s = sum Jc^T Jc (6x6 per camera),
// V_t = sum Jp^T Jp (3x3 per track), E = Jc^T Jp per observation and D = diag(H) clamped, a step solves
//   S dc = -gc + E Vl^-1 gp,   S = Ul - E Vl^-1 E^T,   Ul = U + lambda Dc,  Vl = V + lambda Dp
// by conjugate gradients preconditioned with the 6x6 blocks Ul^-1, S applied as Ul dc - E (Vl^-1 (E^T dc)), and
// back-substitutes dp = -Vl^-1 (gp + E^T dc).  S is never formed: memory and work grow with observations.
//
// Two orders of the observations, built once per call:
//   track-major  the members as they come.  One lane per track of at most L members, one wave per longer track
//                (lane l takes members l, l + 64, ..., the lanes' sums meet in 6 xor-butterfly steps of a + b, which
//                leave the same bits in every lane): bundle_mark, bundle_linearise, bundle_cost, bundle_cg_track.
//   view-major   a stable counting sort of the participating observations by set, so every camera owns a contiguous
//                list in track-major order: a rank inside blocks of 256 members (bundle_sort_count), one scan of the
//                [set][block] counts (bundle_sort_scan, block_scan_inplace), a place pass (bundle_sort_place).  No
//                atomic decides a position.  A camera's list is cut into chunks of kChunk observations; one workgroup
//                reduces one chunk in a fixed order (bundle_cam_sum, bundle_cg_cam), a second stage adds a camera's
//                chunk partials in chunk order (bundle_cam_add).
// No floating-point atomics anywhere, no reduction whose order depends on timing: the op returns the same bits from
// run to run.
//
// The Jacobians are recomputed, not stored: every kernel that needs Jc (2x6) and Jp (2x3) of an observation makes them
// from its pixel (8 bytes), its point (24) and its camera (L2), about 60 fp64 operations, a division and two square
// roots.  Storing them costs 144 bytes per observation and two streams of them per CG iteration; a build of this file
// that stored them took 0.71 and 0.70 ms per CG iteration on 1M tracks and 5.0M observations (8 and 64 views) against
// 0.40 and 0.48 ms recomputed, with the same bits in every output (profiles/bundle_adjust.jsonl).
// Only the weighted residual is kept, 16 bytes per observation, for the camera sums of a linearisation.
//
// CG scalars stay on the device (BundleState): bundle_cg_step, one workgroup, does the dot products in a fixed order,
// updates x, r, z, p and sets `done`; every CG kernel returns at once when it is set, and the cg_max iterations of a
// step are enqueued back to back.  The decision of a step (F' < F), the commit of the new parameters and the next
// linearisation are enqueued behind it, gated on the device's own `accepted`, so the call waits for `stream` once per
// LM step, to read the state.  Kernel boundaries are the only grid barriers.
#include "bundle_device.h"
#include "collection.h"
#include "common.h"
#include "device_util.h"
#include "dlt_device.h"
#include "host_io.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <limits>

namespace spv {
namespace {

constexpr int kLong = 16;            // the longest lane-form track, tracks_triangulate's measured default
constexpr int kChunk = 1024;         // observations of one view-major chunk
constexpr int kSortBlock = 256;      // members of one counting-sort block
constexpr int kWaves = kDltThreads / 64;
constexpr int kScanThreads = 1024;   // block_scan_inplace's workgroup
constexpr int kOneThreads = 256;     // the single-workgroup kernels
constexpr int kRedTracks = 2048;      // tracks of one partial of a sum over the tracks
constexpr int kCamVals = 27;         // a chunk's partial: U (21) and gc (6); a CG iteration uses the first 6

// What the host reads back once per LM step.
struct BundleState {
  double F, Fnew, gmax, rz, bnorm2;
  int32_t done, iters, accepted, pad;
};

// Every device pointer of a call.  Passed by value to the kernels.
struct Ctx {
  // inputs and outputs of the caller
  const float *geom;
  const int32_t *members;
  double *Xio;
  const uint8_t *use;
  // tables
  const long long *seg_off, *track_off;
  const int32_t *wave_list, *mode;   // mode: 0 no camera, 1 free, 2 fixed (or free without observations)
  const double *K5;
  double *pose_cur, *pose_new;
  // per member
  int32_t *obs_set, *obs_track, *rank, *vm;
  double *res;
  // per track
  uint8_t *active;
  double *Xcur, *Xnew, *V, *gp, *Vinv, *q0, *q, *Ft;
  double *red;                       // [nred]: the partials of a sum over the tracks
  // sort and chunks
  int32_t *hist, *cam_off;
  const int32_t *chunks;             // [nchunks, 3] = (set, first view-major position, observations)
  const int32_t *chunk_first;        // [nseg + 1]: a set's chunks
  double *partial;                   // [nchunks, kCamVals]
  // per camera
  double *U, *gc, *Minv, *Eq, *cx, *cr, *cz, *cp;
  BundleState *st;
  int nseg, ntracks, nwave, lane_max, nblocks, nchunks, nred;
  long long nmembers;
  double huber;
};

enum Gate { kAlways = 0, kUnlessDone = 1, kIfAccepted = 2 };
__device__ __forceinline__ bool gate_closed(const Ctx &c, int gate) {
  if (gate == kUnlessDone) return c.st->done != 0;
  if (gate == kIfAccepted) return c.st->accepted == 0;
  return false;
}

// A member's set and geom row, or false: spv_tracks_triangulate_device's rule with "has a camera" = mode != 0.
__device__ __forceinline__ bool usable_member(const Ctx &c, long long i, int &s, long long &row) {
  const int ms = c.members[2 * (size_t)i], mr = c.members[2 * (size_t)i + 1];
  if (ms < 0 || ms >= c.nseg) return false;
  if (c.mode[ms] == 0) return false;
  const long long lo = c.seg_off[ms], hi = c.seg_off[ms + 1];
  if (mr < 0 || (long long)mr >= hi - lo) return false;
  s = ms;
  row = lo + mr;
  return true;
}
// The pixel of a participating member (its set and row were checked when it was marked).
__device__ __forceinline__ void member_pixel(const Ctx &c, long long i, int s, double &u, double &v) {
  const float *g = c.geom + 4 * (size_t)(c.seg_off[s] + c.members[2 * (size_t)i + 1]);
  u = (double)g[0];
  v = (double)g[1];
}

// Jc | Jp (2x6 | 2x3, times sqrt(w)) of participating member i (set s, track t), made again from the pixel, the point
// and the camera of the linearisation: the same operations on the same values as bundle_linearise's, so the same bits.
__device__ __forceinline__ void obs_jacobian(const Ctx &c, size_t i, int s, int t, double (&J)[18]) {
  double X[3], u, v, w;
#pragma unroll
  for (int k = 0; k < 3; ++k) X[k] = c.Xcur[3 * (size_t)t + k];
  member_pixel(c, (long long)i, s, u, v);
  BundleCam cam;
  bundle_load_cam(c.K5, c.pose_cur, s, cam);
  BundleProj pr;
  bundle_project(cam, X, u, v, pr);
  bundle_rho(sqrt(pr.ru * pr.ru + pr.rv * pr.rv), c.huber, w);
  double Jc[2][6], Jp[2][3];
  bundle_jacobians(cam, pr, sqrt(w), Jc, Jp);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int k = 0; k < 6; ++k) J[6 * j + k] = Jc[j][k];
#pragma unroll
    for (int k = 0; k < 3; ++k) J[12 + 3 * j + k] = Jp[j][k];
  }
}

// The sum over the lanes that walk one track: the lane itself, or the wave by xor butterfly (the same bits in all).
template <bool WAVE>
__device__ __forceinline__ double track_sum(double v) {
  if (WAVE) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  }
  return v;
}
template <bool WAVE>
__device__ __forceinline__ int track_sum_int(int v) {
  if (WAVE) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
  }
  return v;
}

__host__ __device__ __forceinline__ bool takes_wave_form(long long len, int lane_max) { return len > lane_max; }

// ---- track-major operations: run<WAVE>(c, t, b, e, lane) walks members b + lane, b + lane + stride, ... ---------

// Who takes part, at the starting parameters.
struct MarkOp {
  template <bool WAVE>
  __device__ __forceinline__ void run(const Ctx &c, int t, long long b, long long e, int lane) const {
    constexpr int stride = WAVE ? 64 : 1;
    double Xh[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) Xh[k] = c.Xio[4 * (size_t)t + k];
    bool part = (!c.use || c.use[t] != 0) && __builtin_isfinite(Xh[0]) && __builtin_isfinite(Xh[1]) &&
                __builtin_isfinite(Xh[2]) && __builtin_isfinite(Xh[3]) && Xh[3] != 0.0;
    double X[3] = {0.0, 0.0, 0.0};
    if (part) {  // (uniform over the lanes of a wave-form track)
#pragma unroll
      for (int k = 0; k < 3; ++k) X[k] = Xh[k] / Xh[3];
      int nu = 0, nbad = 0;
      for (long long i = b + lane; i < e; i += stride) {
        int s;
        long long row;
        if (!usable_member(c, i, s, row)) continue;
        ++nu;
        BundleCam cam;
        bundle_load_cam(c.K5, c.pose_cur, s, cam);
        BundleProj pr;
        if (!bundle_project(cam, X, (double)c.geom[4 * (size_t)row], (double)c.geom[4 * (size_t)row + 1], pr)) ++nbad;
      }
      nu = track_sum_int<WAVE>(nu);
      nbad = track_sum_int<WAVE>(nbad);
      part = nu >= 2 && nbad == 0 && __builtin_isfinite(X[0]) && __builtin_isfinite(X[1]) && __builtin_isfinite(X[2]);
    }
    for (long long i = b + lane; i < e; i += stride) {
      int s = -1;
      long long row;
      if (!part || !usable_member(c, i, s, row)) s = -1;
      c.obs_set[i] = s;
      c.obs_track[i] = t;
    }
    if (lane == 0) {
      c.active[t] = part ? 1 : 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) c.Xcur[3 * (size_t)t + k] = X[k];
      c.Ft[t] = 0.0;
    }
  }
};

// The cost of every track at (pose, X); FULL: also the stored weighted residuals, V and gp.
template <bool FULL>
struct LinOp {
  const double *pose, *X;
  template <bool WAVE>
  __device__ __forceinline__ void run(const Ctx &c, int t, long long b, long long e, int lane) const {
    constexpr int stride = WAVE ? 64 : 1;
    if (!c.active[t]) return;
    double Xt[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) Xt[k] = X[3 * (size_t)t + k];
    double V[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, F = 0.0;
    int nbad = 0;
    for (long long i = b + lane; i < e; i += stride) {
      const int s = c.obs_set[i];
      if (s < 0) continue;
      double u, v;
      member_pixel(c, i, s, u, v);
      BundleCam cam;
      bundle_load_cam(c.K5, pose, s, cam);
      BundleProj pr;
      if (!bundle_project(cam, Xt, u, v, pr)) ++nbad;
      const double n = sqrt(pr.ru * pr.ru + pr.rv * pr.rv);
      double w;
      F += bundle_rho(n, c.huber, w);
      if (FULL) {
        const double sw = sqrt(w);
        double Jc[2][6], Jp[2][3];
        bundle_jacobians(cam, pr, sw, Jc, Jp);
        const double r0 = sw * pr.ru, r1 = sw * pr.rv;
        c.res[2 * (size_t)i] = r0;
        c.res[2 * (size_t)i + 1] = r1;
        V[0] += Jp[0][0] * Jp[0][0] + Jp[1][0] * Jp[1][0];
        V[1] += Jp[0][0] * Jp[0][1] + Jp[1][0] * Jp[1][1];
        V[2] += Jp[0][0] * Jp[0][2] + Jp[1][0] * Jp[1][2];
        V[3] += Jp[0][1] * Jp[0][1] + Jp[1][1] * Jp[1][1];
        V[4] += Jp[0][1] * Jp[0][2] + Jp[1][1] * Jp[1][2];
        V[5] += Jp[0][2] * Jp[0][2] + Jp[1][2] * Jp[1][2];
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] += Jp[0][k] * r0 + Jp[1][k] * r1;
      }
    }
    F = track_sum<WAVE>(F);
    nbad = track_sum_int<WAVE>(nbad);
    if (nbad || F != F) F = __builtin_inf();
    if (FULL) {
#pragma unroll
      for (int k = 0; k < 6; ++k) V[k] = track_sum<WAVE>(V[k]);
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = track_sum<WAVE>(g[k]);
    }
    if (lane != 0) return;
    c.Ft[t] = F;
    if (FULL) {
#pragma unroll
      for (int k = 0; k < 6; ++k) c.V[6 * (size_t)t + k] = V[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) c.gp[3 * (size_t)t + k] = g[k];
    }
  }
};

// q_t = Vl^-1 (E^T vec)_t for the camera vector `vec` (zero outside free cameras).
struct CgTrackOp {
  const double *vec;
  template <bool WAVE>
  __device__ __forceinline__ void run(const Ctx &c, int t, long long b, long long e, int lane) const {
    constexpr int stride = WAVE ? 64 : 1;
    if (!c.active[t]) return;
    double w[3] = {0, 0, 0};
    for (long long i = b + lane; i < e; i += stride) {
      const int s = c.obs_set[i];
      if (s < 0 || c.mode[s] != 1) continue;
      double Ji[18];
      obs_jacobian(c, (size_t)i, s, t, Ji);
      const double *pv = vec + 6 * (size_t)s;
      double a0 = 0.0, a1 = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        a0 += Ji[k] * pv[k];
        a1 += Ji[6 + k] * pv[k];
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] += Ji[12 + k] * a0 + Ji[15 + k] * a1;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = track_sum<WAVE>(w[k]);
    if (lane != 0) return;
    double Vi[6], qt[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) Vi[k] = c.Vinv[6 * (size_t)t + k];
    bundle_sym3_mul(Vi, w, qt);
#pragma unroll
    for (int k = 0; k < 3; ++k) c.q[3 * (size_t)t + k] = qt[k];
  }
};

template <typename Op>
__global__ __launch_bounds__(kDltThreads) void bundle_lane_kernel(Ctx c, Op op, int gate) {
  if (gate_closed(c, gate)) return;
  const long long t = (long long)blockIdx.x * kDltThreads + threadIdx.x;
  if (t >= c.ntracks) return;
  const long long b = c.track_off[t], e = c.track_off[t + 1];
  if (takes_wave_form(e - b, c.lane_max)) return;
  op.template run<false>(c, (int)t, b, e, 0);
}
template <typename Op>
__global__ __launch_bounds__(kDltThreads) void bundle_wave_kernel(Ctx c, Op op, int gate) {
  if (gate_closed(c, gate)) return;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWaves + (threadIdx.x >> 6)));
  if (w >= c.nwave) return;  // the whole wave
  const int t = c.wave_list[w];
  op.template run<true>(c, t, c.track_off[t], c.track_off[t + 1], lane);
}

// ---- per track, one lane each ------------------------------------------------------------------------------

// Vl^-1 and q0 = Vl^-1 gp under this step's lambda.
__global__ __launch_bounds__(kDltThreads) void bundle_point_blocks_kernel(Ctx c, double lambda) {
  const long long t = (long long)blockIdx.x * kDltThreads + threadIdx.x;
  if (t >= c.ntracks || !c.active[t]) return;
  double V[6], Vi[6], g[3], q[3];
#pragma unroll
  for (int k = 0; k < 6; ++k) V[k] = c.V[6 * (size_t)t + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = c.gp[3 * (size_t)t + k];
  bundle_sym3_inverse(V, lambda, Vi);
  bundle_sym3_mul(Vi, g, q);
#pragma unroll
  for (int k = 0; k < 6; ++k) c.Vinv[6 * (size_t)t + k] = Vi[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) c.q0[3 * (size_t)t + k] = q[k];
}

// Xnew = Xcur - q0 - q: the back-substituted points (q = Vl^-1 E^T dc).
__global__ __launch_bounds__(kDltThreads) void bundle_move_points_kernel(Ctx c) {
  const long long t = (long long)blockIdx.x * kDltThreads + threadIdx.x;
  if (t >= c.ntracks || !c.active[t]) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const size_t at = 3 * (size_t)t + k;
    c.Xnew[at] = c.Xcur[at] + (-(c.q0[at] + c.q[at]));
  }
}

// An accepted step's parameters become the current ones.
__global__ __launch_bounds__(kDltThreads) void bundle_commit_kernel(Ctx c) {
  if (c.st->accepted == 0) return;
  const long long t = (long long)blockIdx.x * kDltThreads + threadIdx.x;
  if (t < (long long)c.nseg * 12) c.pose_cur[t] = c.pose_new[t];
  if (t >= c.ntracks || !c.active[t]) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) c.Xcur[3 * (size_t)t + k] = c.Xnew[3 * (size_t)t + k];
}

// The caller's d_X rows of the participating tracks, d_active, and d_err at the final parameters.
__global__ __launch_bounds__(kDltThreads) void bundle_finish_kernel(Ctx c, uint8_t *active_out, double *err) {
  const long long i = (long long)blockIdx.x * kDltThreads + threadIdx.x;
  if (i < c.ntracks) {
    const bool on = c.active[i] != 0;
    if (active_out) active_out[i] = on ? 1 : 0;
    if (on) {
#pragma unroll
      for (int k = 0; k < 3; ++k) c.Xio[4 * (size_t)i + k] = c.Xcur[3 * (size_t)i + k];
      c.Xio[4 * (size_t)i + 3] = 1.0;
    }
  }
  if (!err || i >= c.nmembers) return;
  const int s = c.obs_set[i];
  double ev = __builtin_nan("");
  if (s >= 0) {
    const int t = c.obs_track[i];
    double X[3], u, v;
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = c.Xcur[3 * (size_t)t + k];
    member_pixel(c, i, s, u, v);
    BundleCam cam;
    bundle_load_cam(c.K5, c.pose_cur, s, cam);
    BundleProj pr;
    bundle_project(cam, X, u, v, pr);
    ev = sqrt(pr.ru * pr.ru + pr.rv * pr.rv);
  }
  err[i] = ev;
}

// ---- the view-major order ------------------------------------------------------------------------------------

// Block b of 256 members: a participating member's rank among the block's earlier members of its set, and the
// block's count of every set that occurs (written by the set's last member; the table is zeroed before).
__global__ __launch_bounds__(kSortBlock) void bundle_sort_count_kernel(Ctx c) {
  __shared__ int32_t sets[kSortBlock];
  const long long i = (long long)blockIdx.x * kSortBlock + threadIdx.x;
  const int s = i < c.nmembers ? c.obs_set[i] : -1;
  sets[threadIdx.x] = s;
  __syncthreads();
  if (s < 0) return;
  int before = 0;
  bool later = false;
  for (int k = 0; k < kSortBlock; ++k) {
    const bool same = sets[k] == s;
    before += (same && k < (int)threadIdx.x) ? 1 : 0;
    later = later || (same && k > (int)threadIdx.x);
  }
  c.rank[i] = before;
  if (!later) c.hist[(size_t)s * c.nblocks + blockIdx.x] = before + 1;
}
// The exclusive scan of the [set][block] counts, and with it every camera's first view-major position.
__global__ __launch_bounds__(kScanThreads) void bundle_sort_scan_kernel(Ctx c) {
  const int32_t total = block_scan_inplace<int32_t>(c.hist, c.nseg * c.nblocks);  // (ends in a barrier)
  for (int s = threadIdx.x; s <= c.nseg; s += kScanThreads) c.cam_off[s] = s < c.nseg ? c.hist[(size_t)s * c.nblocks] : total;
}
__global__ __launch_bounds__(kSortBlock) void bundle_sort_place_kernel(Ctx c) {
  const long long i = (long long)blockIdx.x * kSortBlock + threadIdx.x;
  if (i >= c.nmembers) return;
  const int s = c.obs_set[i];
  if (s < 0) return;
  c.vm[c.hist[(size_t)s * c.nblocks + blockIdx.x] + c.rank[i]] = (int32_t)i;
}

// ---- camera sums over the view-major order -------------------------------------------------------------------

// out[k] = the sum of v[k] over the kDltThreads lanes of a workgroup, k < N, in a fixed order: each wave's xor
// butterfly, then the waves in wave order.
template <int N>
__device__ __forceinline__ void group_sum_store(double (&v)[N], double *__restrict__ out) {
  __shared__ double part[kWaves][N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v[k] += __shfl_xor(v[k], d, 64);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) part[w][k] = v[k];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double a = part[0][threadIdx.x];
    for (int k = 1; k < kWaves; ++k) a += part[k][threadIdx.x];
    out[threadIdx.x] = a;
  }
}

// One chunk's U (21) and gc (6).
__global__ __launch_bounds__(kDltThreads) void bundle_cam_sum_kernel(Ctx c, int gate) {
  if (gate_closed(c, gate)) return;
  const int ch = blockIdx.x;
  const int first = c.chunks[3 * ch + 1], n = c.chunks[3 * ch + 2];
  double acc[kCamVals];
#pragma unroll
  for (int k = 0; k < kCamVals; ++k) acc[k] = 0.0;
  for (int k = threadIdx.x; k < n; k += kDltThreads) {
    const size_t i = (size_t)c.vm[first + k];
    double Ji[18];
    obs_jacobian(c, i, c.chunks[3 * ch], c.obs_track[i], Ji);
    double j0[6], j1[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      j0[a] = Ji[a];
      j1[a] = Ji[6 + a];
    }
    const double r0 = c.res[2 * i], r1 = c.res[2 * i + 1];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int b = a; b < 6; ++b) acc[bundle_u21(a, b)] += j0[a] * j0[b] + j1[a] * j1[b];
      acc[21 + a] += j0[a] * r0 + j1[a] * r1;
    }
  }
  group_sum_store<kCamVals>(acc, c.partial + (size_t)ch * kCamVals);
}

// One chunk's E q: sum Jc^T (Jp q_t), for the point vector `qv`.
__global__ __launch_bounds__(kDltThreads) void bundle_cg_cam_kernel(Ctx c, const double *__restrict__ qv, int gate) {
  if (gate_closed(c, gate)) return;
  const int ch = blockIdx.x;
  const int first = c.chunks[3 * ch + 1], n = c.chunks[3 * ch + 2];
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int k = threadIdx.x; k < n; k += kDltThreads) {
    const size_t i = (size_t)c.vm[first + k];
    const int t = c.obs_track[i];
    double Ji[18];
    obs_jacobian(c, i, c.chunks[3 * ch], t, Ji);
    const double *qt = qv + 3 * (size_t)t;
    const double a0 = Ji[12] * qt[0] + Ji[13] * qt[1] + Ji[14] * qt[2];
    const double a1 = Ji[15] * qt[0] + Ji[16] * qt[1] + Ji[17] * qt[2];
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[a] += Ji[a] * a0 + Ji[6 + a] * a1;
  }
  group_sum_store<6>(acc, c.partial + (size_t)ch * kCamVals);
}

// The second stage: entry k of camera s = its chunks' partials added in chunk order.  nvals = 27 writes U and gc,
// nvals = 6 writes Eq.
__global__ __launch_bounds__(kDltThreads) void bundle_cam_add_kernel(Ctx c, int nvals, int gate) {
  if (gate_closed(c, gate)) return;
  const long long e = (long long)blockIdx.x * kDltThreads + threadIdx.x;
  if (e >= (long long)c.nseg * nvals) return;
  const int s = (int)(e / nvals), k = (int)(e % nvals);
  double a = 0.0;
  for (int ch = c.chunk_first[s]; ch < c.chunk_first[s + 1]; ++ch) a += c.partial[(size_t)ch * kCamVals + k];
  if (nvals == 6)
    c.Eq[6 * (size_t)s + k] = a;
  else if (k < 21)
    c.U[21 * (size_t)s + k] = a;
  else
    c.gc[6 * (size_t)s + (k - 21)] = a;
}

// (U_s + lambda D_s)^-1 of every free camera, once per step.
__global__ __launch_bounds__(kDltThreads) void bundle_precondition_kernel(Ctx c, double lambda) {
  const int s = blockIdx.x * kDltThreads + threadIdx.x;
  if (s >= c.nseg || c.mode[s] != 1) return;
  double M[6][6];
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int cc = r; cc < 6; ++cc) {
      const double v = c.U[21 * (size_t)s + bundle_u21(r, cc)];
      M[r][cc] = v;
      M[cc][r] = v;
    }
#pragma unroll
  for (int r = 0; r < 6; ++r) M[r][r] += lambda * bundle_clamp_diag(M[r][r]);
  bundle_spd6_inverse(M);
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int cc = 0; cc < 6; ++cc) c.Minv[36 * (size_t)s + 6 * r + cc] = M[r][cc];
}

// ---- single-workgroup kernels: fixed-order sums, the CG vectors and scalars ----------------------------------

// The sum (MAX: the maximum) of one value per lane over the workgroup: a tree over shared memory in a fixed order.
template <bool MAX>
__device__ __forceinline__ double one_group_reduce(double v, double *sh) {
  __syncthreads();  // sh may still be read from an earlier use
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int d = blockDim.x / 2; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) sh[threadIdx.x] = MAX ? fmax(sh[threadIdx.x], sh[threadIdx.x + d]) : sh[threadIdx.x] + sh[threadIdx.x + d];
    __syncthreads();
  }
  return sh[0];
}

// The sums over the tracks take two stages, like the camera sums: one workgroup per kRedTracks tracks leaves a partial
// (lane k adds tracks k, k + 256, ... of its range, then a tree), and one workgroup adds the partials in the same way.

// Stage 1 of F: the partial sums of the per-track costs.
__global__ __launch_bounds__(kOneThreads) void bundle_cost_part_kernel(Ctx c) {
  __shared__ double sh[kOneThreads];
  const long long t0 = (long long)blockIdx.x * kRedTracks, t1 = t0 + kRedTracks < c.ntracks ? t0 + kRedTracks : c.ntracks;
  double a = 0.0;
  for (long long t = t0 + threadIdx.x; t < t1; t += kOneThreads) a += c.Ft[t];
  a = one_group_reduce<false>(a, sh);
  if (threadIdx.x == 0) c.red[blockIdx.x] = a;
}
// Stage 2.  what = 0: the starting cost (F, and accepted = 1 so that the first linearisation's followers run); 1: a
// step's F', the verdict F' < F, and F = F' where it is accepted.
__global__ __launch_bounds__(kScanThreads) void bundle_cost_sum_kernel(Ctx c, int what) {
  __shared__ double sh[kScanThreads];
  double a = 0.0;
  for (int b = threadIdx.x; b < c.nred; b += kScanThreads) a += c.red[b];
  const double F = one_group_reduce<false>(a, sh);
  if (threadIdx.x != 0) return;
  if (what == 0) {
    c.st->F = F;
    c.st->Fnew = F;
    c.st->accepted = 1;
  } else {
    c.st->Fnew = F;
    const bool ok = F < c.st->F;
    c.st->accepted = ok ? 1 : 0;
    if (ok) c.st->F = F;
  }
}

// max |g|, stage 1: over the participating points of a range of tracks.
__global__ __launch_bounds__(kOneThreads) void bundle_gradient_part_kernel(Ctx c) {
  __shared__ double sh[kOneThreads];
  if (c.st->accepted == 0) return;
  const long long t0 = (long long)blockIdx.x * kRedTracks, t1 = t0 + kRedTracks < c.ntracks ? t0 + kRedTracks : c.ntracks;
  double a = 0.0;
  for (long long t = t0 + threadIdx.x; t < t1; t += kOneThreads) {
    if (!c.active[t]) continue;
#pragma unroll
    for (int k = 0; k < 3; ++k) a = fmax(a, fabs(c.gp[3 * (size_t)t + k]));
  }
  a = one_group_reduce<true>(a, sh);
  if (threadIdx.x == 0) c.red[blockIdx.x] = a;
}
// Stage 2: over the partials and the free cameras.
__global__ __launch_bounds__(kScanThreads) void bundle_gradient_max_kernel(Ctx c) {
  __shared__ double sh[kScanThreads];
  if (c.st->accepted == 0) return;
  double a = 0.0;
  for (int b = threadIdx.x; b < c.nred; b += kScanThreads) a = fmax(a, c.red[b]);
  for (int e = threadIdx.x; e < c.nseg * 6; e += kScanThreads)
    if (c.mode[e / 6] == 1) a = fmax(a, fabs(c.gc[e]));
  const double g = one_group_reduce<true>(a, sh);
  if (threadIdx.x == 0) c.st->gmax = g;
}

// z = Ul^-1 r of camera entry e.
__device__ __forceinline__ double precondition_entry(const Ctx &c, int e) {
  const int s = e / 6, k = e % 6;
  double a = 0.0;
#pragma unroll
  for (int j = 0; j < 6; ++j) a += c.Minv[36 * (size_t)s + 6 * k + j] * c.cr[6 * (size_t)s + j];
  return a;
}

// x = 0, r = b = -gc + E q0, z = Ul^-1 r, p = z; rz, |b|^2, done = (b == 0), iters = 0.
__global__ __launch_bounds__(kOneThreads) void bundle_cg_start_kernel(Ctx c) {
  __shared__ double sh[kOneThreads];
  const int n = c.nseg * 6;
  double bb = 0.0;
  for (int e = threadIdx.x; e < n; e += kOneThreads) {
    const double b = c.mode[e / 6] == 1 ? c.Eq[e] - c.gc[e] : 0.0;
    c.cx[e] = 0.0;
    c.cr[e] = b;
    bb += b * b;
  }
  bb = one_group_reduce<false>(bb, sh);  // (its barriers publish r)
  double rz = 0.0;
  for (int e = threadIdx.x; e < n; e += kOneThreads) {
    const double z = c.mode[e / 6] == 1 ? precondition_entry(c, e) : 0.0;
    c.cz[e] = z;
    c.cp[e] = z;
    rz += c.cr[e] * z;
  }
  rz = one_group_reduce<false>(rz, sh);
  if (threadIdx.x != 0) return;
  c.st->rz = rz;
  c.st->bnorm2 = bb;
  c.st->iters = 0;
  c.st->done = (bb == 0.0 || !(rz > 0.0)) ? 1 : 0;
}

// One CG iteration behind E q = E (Vl^-1 (E^T p)): Sp = Ul p - E q, alpha, x, r, z, beta, p, done.
__global__ __launch_bounds__(kOneThreads) void bundle_cg_step_kernel(Ctx c, double lambda, double tol2) {
  __shared__ double sh[kOneThreads];
  if (c.st->done != 0) return;
  const int n = c.nseg * 6;
  double *Sp = c.cz;  // z is dead between two steps: it holds S p until it is rebuilt below
  double pSp = 0.0;
  for (int e = threadIdx.x; e < n; e += kOneThreads) {
    const int s = e / 6, k = e % 6;
    double a = 0.0;
    if (c.mode[s] == 1) {
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double u = c.U[21 * (size_t)s + (k <= j ? bundle_u21(k, j) : bundle_u21(j, k))];
        a += (j == k ? u + lambda * bundle_clamp_diag(u) : u) * c.cp[6 * (size_t)s + j];
      }
      a -= c.Eq[e];
    }
    Sp[e] = a;
    pSp += c.cp[e] * a;
  }
  pSp = one_group_reduce<false>(pSp, sh);
  const double rz = c.st->rz;
  const double alpha = rz / pSp;
  const bool broke = !(pSp > 0.0) || !__builtin_isfinite(alpha);
  double rr = 0.0;
  if (!broke) {
    for (int e = threadIdx.x; e < n; e += kOneThreads) {
      c.cx[e] += alpha * c.cp[e];
      const double r = c.cr[e] - alpha * Sp[e];
      c.cr[e] = r;
      rr += r * r;
    }
  }
  rr = one_group_reduce<false>(rr, sh);  // (its barriers publish r, and end the reads of S p)
  double rzn = 0.0;
  if (!broke) {
    for (int e = threadIdx.x; e < n; e += kOneThreads) {
      const double z = c.mode[e / 6] == 1 ? precondition_entry(c, e) : 0.0;
      c.cz[e] = z;
      rzn += c.cr[e] * z;
    }
  }
  rzn = one_group_reduce<false>(rzn, sh);
  if (!broke) {
    const double beta = rzn / rz;
    for (int e = threadIdx.x; e < n; e += kOneThreads) c.cp[e] = c.cz[e] + beta * c.cp[e];
  }
  if (threadIdx.x != 0) return;
  if (broke) {
    c.st->done = 1;
    return;
  }
  c.st->rz = rzn;
  c.st->iters += 1;
  if (rr <= tol2 * c.st->bnorm2 || !(rzn > 0.0)) c.st->done = 1;
}

// pose_new = the moved pose of every free camera, the current one of every other.
__global__ __launch_bounds__(kDltThreads) void bundle_move_cameras_kernel(Ctx c) {
  const int s = blockIdx.x * kDltThreads + threadIdx.x;
  if (s >= c.nseg) return;
  if (c.mode[s] == 1) {
    double d[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = c.cx[6 * (size_t)s + k];
    bundle_move_pose(c.pose_cur + 12 * (size_t)s, d, c.pose_new + 12 * (size_t)s);
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k) c.pose_new[12 * (size_t)s + k] = c.pose_cur[12 * (size_t)s + k];
  }
}

// ---- host ----------------------------------------------------------------------------------------------------

unsigned groups(long long n, int threads) { return (unsigned)std::max<long long>(1, (n + threads - 1) / threads); }

// The workspace, stated once.  tables_bytes: the upload of the call's tables, laid out by `Tables`.
struct Tables {
  size_t off_pose, off_k5, off_seg, off_trk, off_mode, off_wave, bytes;
  Tables(int nseg, int ntracks, size_t nwave) {
    off_pose = 0;
    off_k5 = off_pose + (size_t)nseg * 12 * sizeof(double);
    off_seg = off_k5 + (size_t)nseg * 5 * sizeof(double);
    off_trk = off_seg + ((size_t)nseg + 1) * sizeof(long long);
    off_mode = off_trk + ((size_t)ntracks + 1) * sizeof(long long);
    off_wave = off_mode + (size_t)nseg * sizeof(int32_t);
    bytes = off_wave + nwave * sizeof(int32_t);
  }
};
long long max_chunks(int nseg, long long nmembers) { return nmembers / kChunk + nseg; }
long long sort_blocks(long long nmembers) { return (nmembers + kSortBlock - 1) / kSortBlock; }

void layout(WsWalk &w, int nseg, int ntracks, long long nmembers, Ctx *c, unsigned char **tables, int32_t **chunks,
            int32_t **chunk_first) {
  const size_t nt = (size_t)ntracks, nm = (size_t)nmembers, ns = (size_t)nseg, d = sizeof(double);
  const size_t nch = (size_t)max_chunks(nseg, nmembers);
  // (the wave-form list is at most ntracks long)
  *tables = w.take<unsigned char>(Tables(nseg, ntracks, nt).bytes);
  c->pose_new = w.take<double>(ns * 12 * d);
  c->obs_set = w.take<int32_t>(nm * 4);
  c->obs_track = w.take<int32_t>(nm * 4);
  c->rank = w.take<int32_t>(nm * 4);
  c->vm = w.take<int32_t>(nm * 4);
  c->res = w.take<double>(nm * 2 * d);
  c->active = w.take<uint8_t>(nt);
  c->Xcur = w.take<double>(nt * 3 * d);
  c->Xnew = w.take<double>(nt * 3 * d);
  c->V = w.take<double>(nt * 6 * d);
  c->gp = w.take<double>(nt * 3 * d);
  c->Vinv = w.take<double>(nt * 6 * d);
  c->q0 = w.take<double>(nt * 3 * d);
  c->q = w.take<double>(nt * 3 * d);
  c->Ft = w.take<double>(nt * d);
  c->red = w.take<double>((nt / kRedTracks + 1) * d);
  c->hist = w.take<int32_t>(ns * (size_t)sort_blocks(nmembers) * 4);
  c->cam_off = w.take<int32_t>((ns + 1) * 4);
  *chunks = w.take<int32_t>(nch * 3 * 4);
  *chunk_first = w.take<int32_t>((ns + 1) * 4);
  c->partial = w.take<double>(nch * kCamVals * d);
  c->U = w.take<double>(ns * 21 * d);
  c->gc = w.take<double>(ns * 6 * d);
  c->Minv = w.take<double>(ns * 36 * d);
  c->Eq = w.take<double>(ns * 6 * d);
  c->cx = w.take<double>(ns * 6 * d);
  c->cr = w.take<double>(ns * 6 * d);
  c->cz = w.take<double>(ns * 6 * d);
  c->cp = w.take<double>(ns * 6 * d);
  c->st = w.take<BundleState>(sizeof(BundleState));
}

bool finite_all(const double *v, int n) {
  for (int k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

template <typename Op>
int launch_tracks(const char *name, const Ctx &c, const Op &op, int gate, hipStream_t stream) {
  ProfScope prof(name, stream);
  if (c.ntracks > c.nwave) {
    hipLaunchKernelGGL(bundle_lane_kernel<Op>, dim3(groups(c.ntracks, kDltThreads)), dim3(kDltThreads), 0, stream, c, op, gate);
    SPV_HIP_CHECK(hipGetLastError());
  }
  if (c.nwave > 0) {
    hipLaunchKernelGGL(bundle_wave_kernel<Op>, dim3(groups(c.nwave, kWaves)), dim3(kDltThreads), 0, stream, c, op, gate);
    SPV_HIP_CHECK(hipGetLastError());
  }
  return SPV_OK;
}

// U, gc (full) or E qv (CG) of every free camera: the chunk partials, then their sums in chunk order.
int launch_camera_sums(const Ctx &c, const double *qv, int gate, hipStream_t stream) {
  ProfScope prof(qv ? "bundle_cg_cam" : "bundle_cam_sum", stream);
  if (c.nchunks > 0) {
    if (qv)
      hipLaunchKernelGGL(bundle_cg_cam_kernel, dim3((unsigned)c.nchunks), dim3(kDltThreads), 0, stream, c, qv, gate);
    else
      hipLaunchKernelGGL(bundle_cam_sum_kernel, dim3((unsigned)c.nchunks), dim3(kDltThreads), 0, stream, c, gate);
    SPV_HIP_CHECK(hipGetLastError());
  }
  const int nvals = qv ? 6 : kCamVals;
  hipLaunchKernelGGL(bundle_cam_add_kernel, dim3(groups((long long)c.nseg * nvals, kDltThreads)), dim3(kDltThreads), 0, stream, c,
                     nvals, gate);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

int launch_cost_sum(const Ctx &c, int what, hipStream_t stream) {
  ProfScope prof("bundle_cost_sum", stream);
  hipLaunchKernelGGL(bundle_cost_part_kernel, dim3((unsigned)c.nred), dim3(kOneThreads), 0, stream, c);
  SPV_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(bundle_cost_sum_kernel, dim3(1), dim3(kScanThreads), 0, stream, c, what);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}
int launch_gradient_max(const Ctx &c, hipStream_t stream) {
  ProfScope prof("bundle_gradient_max", stream);
  hipLaunchKernelGGL(bundle_gradient_part_kernel, dim3((unsigned)c.nred), dim3(kOneThreads), 0, stream, c);
  SPV_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(bundle_gradient_max_kernel, dim3(1), dim3(kScanThreads), 0, stream, c);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

// Linearise at the current parameters, the camera sums and max |g|; all gated on `accepted` inside the loop.
int launch_linearise(const Ctx &c, int gate, hipStream_t stream) {
  SPV_TRY(launch_tracks("bundle_linearise", c, LinOp<true>{c.pose_cur, c.Xcur}, gate, stream));
  SPV_TRY(launch_camera_sums(c, nullptr, gate, stream));
  return launch_gradient_max(c, stream);
}

int read_state(const Ctx &c, BundleState *h, hipStream_t stream) {
  SPV_HIP_CHECK(hipMemcpyAsync(h, c.st, sizeof(BundleState), hipMemcpyDeviceToHost, stream));
  SPV_HIP_CHECK(hipStreamSynchronize(stream));
  return SPV_OK;
}

}  // namespace

void bundle_adjust_plan(const long long *track_off, int ntracks, const int32_t *members, const long long *seg_off, int nseg,
                        const int32_t *mode, BundleAdjustPlan *plan) {
  *plan = BundleAdjustPlan();
  plan->chunk = kChunk;
  std::vector<long long> per_set(members ? (size_t)nseg : 0, 0);
  std::vector<int> sets;
  for (int t = 0; t < ntracks; ++t) {
    const long long b = track_off[t], e = track_off[t + 1];
    plan->longest = std::max(plan->longest, e - b);
    if (takes_wave_form(e - b, kLong)) plan->wave_list.push_back(t);
    if (!members) continue;
    sets.clear();
    for (long long i = b; i < e; ++i) {
      const int s = members[2 * i], r = members[2 * i + 1];
      if (s < 0 || s >= nseg || (mode && mode[s] == 0) || r < 0 || r >= seg_off[s + 1] - seg_off[s]) continue;
      sets.push_back(s);
    }
    if (sets.size() >= 2)
      for (int s : sets) ++per_set[s];
  }
  plan->wave_tracks = (long long)plan->wave_list.size();
  plan->lane_tracks = ntracks - plan->wave_tracks;
  for (size_t s = 0; s < per_set.size(); ++s)
    if (!mode || mode[s] == 1) plan->chunks += (per_set[s] + kChunk - 1) / kChunk;
}

size_t bundle_adjust_workspace_bytes(int nseg, int ntracks, long long nmembers) {
  WsWalk w;
  Ctx c;
  unsigned char *tables;
  int32_t *chunks, *chunk_first;
  layout(w, nseg, ntracks, nmembers, &c, &tables, &chunks, &chunk_first);
  return w.end();
}

int bundle_adjust_check(const void *geom, const long long *seg_off, int nseg, const double *K, const double *poses,
                        const int32_t *mode, const long long *track_off, int ntracks, const void *members, long long nmembers,
                        const void *X, const BundleAdjustOptions &o, const void *err, const void *trace, const void *info) {
  if (nseg < 0 || ntracks < 0 || nmembers < 0)
    return set_error(SPV_ERR_INVALID, "negative count (nseg=%d, ntracks=%d, nmembers=%lld)", nseg, ntracks, nmembers);
  SPV_TRY(check_offsets(seg_off, nseg, "seg_off"));
  if (nmembers >= (1ll << 31)) return set_error(SPV_ERR_INVALID, "%lld members, must be below 2^31", nmembers);
  SPV_TRY(check_offsets(track_off, ntracks, "track_off"));
  if (track_off[ntracks] != nmembers)
    return set_error(SPV_ERR_INVALID, "track_off ends at %lld, must end at nmembers = %lld", track_off[ntracks], nmembers);
  if ((long long)nseg * sort_blocks(nmembers) >= (1ll << 31))
    return set_error(SPV_ERR_INVALID, "nseg * ceil(nmembers / %d) must be below 2^31", kSortBlock);
  if (!(o.huber > 0.0)) return set_error(SPV_ERR_INVALID, "huber must be positive");
  if (!(o.lambda0 >= 0.0) || !(o.ftol >= 0.0) || !(o.gtol >= 0.0) || !(o.cg_tol >= 0.0))
    return set_error(SPV_ERR_INVALID, "lambda0, ftol, gtol and cg_tol must be non-negative numbers");
  if (o.max_steps < 0 || o.cg_max < 0) return set_error(SPV_ERR_INVALID, "negative max_steps or cg_max");
  if ((nseg > 0 && (!K || !poses || !mode)) || (nmembers > 0 && !members) || (nmembers > 0 && seg_off[nseg] > 0 && !geom) ||
      (ntracks > 0 && !X) || !info)
    return set_error(SPV_ERR_INVALID, "null pointer");
  if (((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(err) | reinterpret_cast<uintptr_t>(trace) |
        reinterpret_cast<uintptr_t>(info) | reinterpret_cast<uintptr_t>(poses)) & 7) ||
      ((reinterpret_cast<uintptr_t>(geom) | reinterpret_cast<uintptr_t>(members)) & 3))
    return set_error(SPV_ERR_INVALID, "pointers must be aligned to their element size");
  for (int s = 0; s < nseg; ++s) {
    if (mode[s] < 0 || mode[s] > 2) return set_error(SPV_ERR_INVALID, "mode[%d] = %d, must be 0, 1 or 2", s, mode[s]);
    if (mode[s] == 0) continue;
    const double *k = K + 9 * (size_t)s, *p = poses + 12 * (size_t)s;
    if (!finite_all(k, 9) || k[8] != 1.0 || k[3] != 0.0 || k[6] != 0.0 || k[7] != 0.0 || k[0] == 0.0 || k[4] == 0.0)
      return set_error(SPV_ERR_INVALID, "K[%d] must be finite and upper triangular with K[8] = 1 and non-zero focal lengths", s);
    if (!finite_all(p, 12)) return set_error(SPV_ERR_INVALID, "poses[%d] is not finite", s);
    double worst = 0.0;
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        const double g = p[a] * p[b] + p[4 + a] * p[4 + b] + p[8 + a] * p[8 + b];
        worst = std::max(worst, fabs(g - (a == b ? 1.0 : 0.0)));
      }
    const double det = p[0] * (p[5] * p[10] - p[6] * p[9]) - p[1] * (p[4] * p[10] - p[6] * p[8]) + p[2] * (p[4] * p[9] - p[5] * p[8]);
    if (!(worst <= 1e-6) || !(fabs(det - 1.0) <= 1e-6))
      return set_error(SPV_ERR_INVALID, "poses[%d] does not start with a rotation (|R^T R - I| = %g, det = %g)", s, worst, det);
  }
  return SPV_OK;
}

bool bundle_adjust_has_work(const int32_t *mode, int nseg, int ntracks) {
  if (ntracks == 0) return false;
  for (int s = 0; s < nseg; ++s)
    if (mode[s] != 0) return true;
  return false;
}

void bundle_adjust_idle(const BundleAdjustOptions &o, double *trace, double *info) {
  if (trace)
    for (long long k = 0; k < (long long)o.max_steps * 6; ++k) trace[k] = std::numeric_limits<double>::quiet_NaN();
  for (int k = 0; k < 7; ++k) info[k] = 0.0;
}

int bundle_adjust_run(const float *d_geom, const long long *seg_off, int nseg, const double *K, double *poses, const int32_t *mode,
                      const long long *track_off, int ntracks, const int32_t *d_members, long long nmembers, double *d_X,
                      const uint8_t *d_use, const BundleAdjustOptions &o, double *d_err, uint8_t *d_active, double *trace,
                      double *info, void *d_ws, size_t ws_bytes, hipStream_t stream) {
  SPV_TRY(bundle_adjust_check(d_geom, seg_off, nseg, K, poses, mode, track_off, ntracks, d_members, nmembers, d_X, o, d_err, trace,
                              info));
  const bool work = bundle_adjust_has_work(mode, nseg, ntracks);
  const size_t need = work ? bundle_adjust_workspace_bytes(nseg, ntracks, nmembers) : 0;
  if (work && (!d_ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(d_ws) & 255)))
    return set_error(SPV_ERR_INVALID, "workspace of %zu bytes, aligned to 256, needed (%zu given)", need, ws_bytes);
  bundle_adjust_idle(o, trace, info);
  if (!work) {
    if (d_active && ntracks > 0) SPV_HIP_CHECK(hipMemsetAsync(d_active, 0, (size_t)ntracks, stream));
    if (d_err && nmembers > 0) SPV_HIP_CHECK(hipMemsetAsync(d_err, 0xff, (size_t)nmembers * sizeof(double), stream));  // NaN
    return SPV_OK;
  }

  BundleAdjustPlan plan;
  bundle_adjust_plan(track_off, ntracks, nullptr, seg_off, nseg, mode, &plan);
  const size_t nwave = plan.wave_list.size();

  Ctx c;
  memset(&c, 0, sizeof(c));
  WsWalk walk(d_ws);
  unsigned char *d_tables;
  int32_t *d_chunks, *d_chunk_first;
  layout(walk, nseg, ntracks, nmembers, &c, &d_tables, &d_chunks, &d_chunk_first);

  // the call's tables, one upload: poses | K | seg_off | track_off | mode | the wave-form list
  const Tables tl(nseg, ntracks, nwave);
  std::vector<unsigned char> host(tl.bytes, 0);
  double *h_pose = reinterpret_cast<double *>(host.data() + tl.off_pose), *h_k5 = reinterpret_cast<double *>(host.data() + tl.off_k5);
  int32_t *h_mode = reinterpret_cast<int32_t *>(host.data() + tl.off_mode);
  for (int s = 0; s < nseg; ++s) {
    h_mode[s] = mode[s];
    if (mode[s] == 0) continue;  // a set without a camera: its rows are not read
    memcpy(h_pose + 12 * (size_t)s, poses + 12 * (size_t)s, 12 * sizeof(double));
    const double *k = K + 9 * (size_t)s;
    const double k5[5] = {k[0], k[1], k[2], k[4], k[5]};
    memcpy(h_k5 + 5 * (size_t)s, k5, sizeof(k5));
  }
  memcpy(host.data() + tl.off_seg, seg_off, ((size_t)nseg + 1) * sizeof(long long));
  memcpy(host.data() + tl.off_trk, track_off, ((size_t)ntracks + 1) * sizeof(long long));
  if (nwave) memcpy(host.data() + tl.off_wave, plan.wave_list.data(), nwave * sizeof(int32_t));
  SPV_HIP_CHECK(hipMemcpyAsync(d_tables, host.data(), host.size(), hipMemcpyHostToDevice, stream));

  c.geom = d_geom;
  c.members = d_members;
  c.Xio = d_X;
  c.use = d_use;
  c.pose_cur = reinterpret_cast<double *>(d_tables + tl.off_pose);
  c.K5 = reinterpret_cast<const double *>(d_tables + tl.off_k5);
  c.seg_off = reinterpret_cast<const long long *>(d_tables + tl.off_seg);
  c.track_off = reinterpret_cast<const long long *>(d_tables + tl.off_trk);
  c.mode = reinterpret_cast<const int32_t *>(d_tables + tl.off_mode);
  c.wave_list = reinterpret_cast<const int32_t *>(d_tables + tl.off_wave);
  c.chunks = d_chunks;
  c.chunk_first = d_chunk_first;
  c.nseg = nseg;
  c.ntracks = ntracks;
  c.nwave = (int)nwave;
  c.lane_max = kLong;
  c.nblocks = (int)sort_blocks(nmembers);
  c.nred = (int)(((long long)ntracks + kRedTracks - 1) / kRedTracks);
  c.nmembers = nmembers;
  c.huber = o.huber;

  // who takes part, and the view-major order
  SPV_TRY(launch_tracks("bundle_mark", c, MarkOp{}, kAlways, stream));
  std::vector<int32_t> cam_off((size_t)nseg + 1, 0);
  if (nmembers > 0) {
    ProfScope prof("bundle_sort", stream);
    SPV_HIP_CHECK(hipMemsetAsync(c.hist, 0, (size_t)nseg * c.nblocks * sizeof(int32_t), stream));
    hipLaunchKernelGGL(bundle_sort_count_kernel, dim3((unsigned)c.nblocks), dim3(kSortBlock), 0, stream, c);
    SPV_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bundle_sort_scan_kernel, dim3(1), dim3(kScanThreads), 0, stream, c);
    SPV_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(bundle_sort_place_kernel, dim3((unsigned)c.nblocks), dim3(kSortBlock), 0, stream, c);
    SPV_HIP_CHECK(hipGetLastError());
    SPV_HIP_CHECK(hipMemcpyAsync(cam_off.data(), c.cam_off, cam_off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  }
  std::vector<uint8_t> h_active((size_t)ntracks);
  SPV_HIP_CHECK(hipMemcpyAsync(h_active.data(), c.active, (size_t)ntracks, hipMemcpyDeviceToHost, stream));
  SPV_HIP_CHECK(hipStreamSynchronize(stream));
  long long npart = 0;
  for (uint8_t a : h_active) npart += a;
  const long long nobs = cam_off[nseg];

  // the chunks of the free cameras that have observations; a free camera without any is held like a fixed one
  std::vector<int32_t> chunks, chunk_first((size_t)nseg + 1, 0);
  int nfree = 0;
  for (int s = 0; s < nseg; ++s) {
    chunk_first[s] = (int32_t)(chunks.size() / 3);
    const int32_t n = cam_off[s + 1] - cam_off[s];
    if (mode[s] == 1 && n == 0) h_mode[s] = 2;
    if (mode[s] != 1 || n == 0) continue;
    ++nfree;
    for (int32_t at = 0; at < n; at += kChunk) {
      chunks.push_back(s);
      chunks.push_back(cam_off[s] + at);
      chunks.push_back(std::min<int32_t>(kChunk, n - at));
    }
  }
  chunk_first[nseg] = (int32_t)(chunks.size() / 3);
  c.nchunks = chunk_first[nseg];
  if ((long long)c.nchunks > max_chunks(nseg, nmembers)) return set_error(SPV_ERR_INTERNAL, "more chunks than the workspace holds");
  SPV_HIP_CHECK(hipMemcpyAsync(d_tables + tl.off_mode, h_mode, (size_t)nseg * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  if (c.nchunks) SPV_HIP_CHECK(hipMemcpyAsync(d_chunks, chunks.data(), chunks.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  SPV_HIP_CHECK(hipMemcpyAsync(d_chunk_first, chunk_first.data(), chunk_first.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));

  info[3] = (double)npart;
  info[4] = (double)nobs;
  int steps = 0, accepted = 0, reason = 0;  // 0: max_steps, 1: gradient, 2: cost, 3: damping
  BundleState h;
  memset(&h, 0, sizeof(h));
  if (npart > 0) {
    SPV_TRY(launch_tracks("bundle_linearise", c, LinOp<true>{c.pose_cur, c.Xcur}, kAlways, stream));
    SPV_TRY(launch_cost_sum(c, 0, stream));
    SPV_TRY(launch_camera_sums(c, nullptr, kAlways, stream));
    SPV_TRY(launch_gradient_max(c, stream));
    SPV_TRY(read_state(c, &h, stream));
    info[5] = h.F;
    double lambda = o.lambda0;
    const double tol2 = o.cg_tol * o.cg_tol;
    for (int step = 0; step < o.max_steps; ++step) {
      if (h.gmax <= o.gtol) {
        reason = 1;
        break;
      }
      const double F = h.F, gmax = h.gmax;
      {
        ProfScope prof("bundle_point_blocks", stream);
        hipLaunchKernelGGL(bundle_point_blocks_kernel, dim3(groups(ntracks, kDltThreads)), dim3(kDltThreads), 0, stream, c, lambda);
        SPV_HIP_CHECK(hipGetLastError());
      }
      {
        ProfScope prof("bundle_precondition", stream);
        hipLaunchKernelGGL(bundle_precondition_kernel, dim3(groups(nseg, kDltThreads)), dim3(kDltThreads), 0, stream, c, lambda);
        SPV_HIP_CHECK(hipGetLastError());
      }
      SPV_TRY(launch_camera_sums(c, c.q0, kAlways, stream));  // E Vl^-1 gp
      {
        ProfScope prof("bundle_cg_start", stream);
        hipLaunchKernelGGL(bundle_cg_start_kernel, dim3(1), dim3(kOneThreads), 0, stream, c);
        SPV_HIP_CHECK(hipGetLastError());
      }
      for (int it = 0; it < o.cg_max && nfree > 0; ++it) {
        SPV_TRY(launch_tracks("bundle_cg_track", c, CgTrackOp{c.cp}, kUnlessDone, stream));
        SPV_TRY(launch_camera_sums(c, c.q, kUnlessDone, stream));
        ProfScope prof("bundle_cg_step", stream);
        hipLaunchKernelGGL(bundle_cg_step_kernel, dim3(1), dim3(kOneThreads), 0, stream, c, lambda, tol2);
        SPV_HIP_CHECK(hipGetLastError());
      }
      // back-substitution, the moved parameters, their cost and the verdict
      SPV_TRY(launch_tracks("bundle_cg_track", c, CgTrackOp{c.cx}, kAlways, stream));
      {
        ProfScope prof("bundle_move", stream);
        hipLaunchKernelGGL(bundle_move_points_kernel, dim3(groups(ntracks, kDltThreads)), dim3(kDltThreads), 0, stream, c);
        SPV_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(bundle_move_cameras_kernel, dim3(groups(nseg, kDltThreads)), dim3(kDltThreads), 0, stream, c);
        SPV_HIP_CHECK(hipGetLastError());
      }
      SPV_TRY(launch_tracks("bundle_cost", c, LinOp<false>{c.pose_new, c.Xnew}, kAlways, stream));
      SPV_TRY(launch_cost_sum(c, 1, stream));
      {
        ProfScope prof("bundle_commit", stream);
        hipLaunchKernelGGL(bundle_commit_kernel, dim3(groups(std::max<long long>(ntracks, (long long)nseg * 12), kDltThreads)),
                           dim3(kDltThreads), 0, stream, c);
        SPV_HIP_CHECK(hipGetLastError());
      }
      SPV_TRY(launch_linearise(c, kIfAccepted, stream));
      SPV_TRY(read_state(c, &h, stream));  // the one wait of this step
      ++steps;
      if (trace) {
        double *row = trace + 6 * (size_t)step;
        row[0] = F;
        row[1] = h.Fnew;
        row[2] = lambda;
        row[3] = (double)h.iters;
        row[4] = (double)h.accepted;
        row[5] = gmax;
      }
      if (h.accepted) {
        ++accepted;
        lambda = std::max(lambda / 10.0, 1e-15);
        if ((F - h.Fnew) / F <= o.ftol) {
          reason = 2;
          break;
        }
      } else {
        lambda *= 10.0;
        if (lambda > 1e15) {
          reason = 3;
          break;
        }
      }
    }
  }
  info[0] = (double)steps;
  info[1] = (double)accepted;
  info[2] = (double)reason;
  info[6] = npart > 0 ? h.F : 0.0;

  {
    ProfScope prof("bundle_finish", stream);
    hipLaunchKernelGGL(bundle_finish_kernel, dim3(groups(std::max<long long>(ntracks, nmembers), kDltThreads)), dim3(kDltThreads), 0,
                       stream, c, d_active, d_err);
    SPV_HIP_CHECK(hipGetLastError());
  }
  // the refined poses of the sets that have a camera
  std::vector<double> h_out((size_t)nseg * 12);
  SPV_HIP_CHECK(hipMemcpyAsync(h_out.data(), c.pose_cur, h_out.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  SPV_HIP_CHECK(hipStreamSynchronize(stream));
  for (int s = 0; s < nseg; ++s)
    if (mode[s] == 1 && h_mode[s] == 1) memcpy(poses + 12 * (size_t)s, h_out.data() + 12 * (size_t)s, 12 * sizeof(double));
  return SPV_OK;
}

}  // namespace spv
