// tracks_triangulate.hip -- N-view DLT of every track of a collection, on the device (gfx950).
//
// tracks_batch.hip ends the many-pairs chain with (track_off, members); dlt_batch.hip triangulates pair by pair, so a
// keypoint seen in five views comes out up to ten times in ten pair frames.  Here a caller who has one camera per
// set gets one point per track from all its observations, a residual per observation and a verdict per track.  The
// contract is the library's own and is stated in include/spectavi_amd.h; tests/tracks_triangulate_model.py is its
// plain restatement.  The reference has no such step.
//
// The matrix of a track is 2m x 4: observation (u, v) in a set with camera P contributes the reference's two DLT rows
// u P[2] - P[0], v P[2] - P[1], formed as dlt_matrix forms them.  It is never squared: A^T A has the squares of the
// singular values, and for narrow baselines (|t| = 2e-3, f = 1000, depths 4-8) the Gram route leaves |A X| 2.6e-13
// sigma1 above sigma4 where a float64 QR stays inside sigma4 + 1e-13 sigma1 (numpy, 2000 tracks).  Instead the rows
// are rotated one observation at a time into a 4x4 upper triangle R by Givens rotations (reciprocal roots through
// rsqrt_nr2, a zero pivot rotates nothing): R has A's singular values and right singular vectors, and goes to the
// two-view solver of dlt_device.h (Gram-Schmidt + inverse iteration, Jacobi where that does not converge) as it is.
//
// Two-member anchor.  The first two usable observations' four rows are kept as a plain A[4][4] and rotated into R
// only when a third arrives, so a track with exactly two usable observations runs dlt_solve<true, false>'s very
// arithmetic on dlt_matrix's very matrix (w = 1: rcp_nr2(1) = 1 and u * 1 = u exactly): its X and residuals are
// dlt_batch.hip's bits.
//
// Two forms, chosen by a track's member count alone (the host owns track_off and builds the list):
//   tracks_triangulate_lane_kernel   one lane per track, tracks of at most L members (and all of fewer than 3); the
//                                    camera of each observation is read per lane from the uploaded table (L2)
//   tracks_triangulate_wave_kernel   one wave per longer track: lane l rotates members l, l + 64, ... into its own
//                                    triangle (zeros for a lane without members), the 64 triangles are combined in 6
//                                    butterfly steps, each re-triangularising [R of the lower lane; R of the higher]
//                                    with the same arithmetic in both partners, so every lane ends with the same R
//                                    and solves it; then the lanes compute their members' residuals and vote.  A
//                                    long track left with fewer than 3 usable observations is solved by the lane
//                                    form's code, every lane the same, so that it keeps the anchor's bits.
// A track's result depends on its members, geom and the cameras alone: not on its neighbours or its place.
// L began as 32, an estimate from instruction counts (a lane costs its wave the longest track in it; a wave costs 64
// lanes for m members).  tools/bench_tracks_triangulate.py measured 8, 16, 32, 64 and "never" on 1M tracks of mostly
// 2-6 members and on the same with 1 % of 200-2000 members (profiles/tracks_triangulate.md): the two kernels together
// take 0.327 ms at 16 against 0.458 at 32 on the first and 0.740 against 0.833 on the second, the ranges of five rounds
// apart on both, so the default is 16.  Values between the five were not measured.
#include "collection.h"
#include "common.h"
#include "device_util.h"
#include "dlt_device.h"
#include "host_io.h"

#include <atomic>
#include <math.h>
#include <string.h>

namespace spv {
namespace {

constexpr int kDefaultLong = 16;
constexpr int kWavesPerGroup = kDltThreads / 64;

// The device form of a call's tables, one upload.
struct TriTables {
  const double *cams;         // [nseg, 12]
  const long long *seg_off;   // [nseg + 1]
  const long long *track_off; // [ntracks + 1]
  const int32_t *use_set;     // [nseg] or null
  const int32_t *wave_list;   // [nwave]
  int nseg, ntracks, nwave, lane_max;
  double max_error;
};

// One observation: whether it is usable, and then its camera and pixel.
struct Obs {
  double p[12];
  double u, v;
};
__device__ __forceinline__ bool load_obs(const TriTables &tb, const float *__restrict__ geom,
                                         const int32_t *__restrict__ members, long long i, Obs &o) {
  const int2 m = make_int2(members[2 * (size_t)i], members[2 * (size_t)i + 1]);
  if (m.x < 0 || m.x >= tb.nseg) return false;
  if (tb.use_set && tb.use_set[m.x] == 0) return false;
  const long long lo = tb.seg_off[m.x], hi = tb.seg_off[m.x + 1];
  if (m.y < 0 || (long long)m.y >= hi - lo) return false;
  const float *g = geom + 4 * (size_t)(lo + m.y);
  o.u = (double)g[0];
  o.v = (double)g[1];
  const double *cp = tb.cams + (size_t)m.x * 12;
#pragma unroll
  for (int k = 0; k < 12; ++k) o.p[k] = cp[k];
  return true;
}
__device__ __forceinline__ void obs_rows(const Obs &o, double (&r0)[4], double (&r1)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    r0[c] = __builtin_fma(o.u, o.p[8 + c], -o.p[c]);
    r1[c] = __builtin_fma(o.v, o.p[8 + c], -o.p[4 + c]);
  }
}

// 1 / sqrt(h) for h > 0: Newton on v_rsq_f64 where its square cannot leave the range, IEEE elsewhere (inf, nan and
// the ends of the range keep IEEE's answers).
__device__ __forceinline__ double rsqrt_guarded(double h) {
  if (__builtin_expect(h >= 0x1p-900 && h <= 0x1p900, 1)) return rsqrt_nr2(h);
  return 1.0 / sqrt(h);
}

// The row (0, .., 0, r[FIRST], .., r[3]) rotated into the upper triangle R (Givens, one rotation per column).  A
// rotation whose pivot and entry are both zero is the identity.  r is used up.
template <int FIRST>
__device__ __forceinline__ void rotate_in(double (&R)[4][4], double (&r)[4]) {
#pragma unroll
  for (int j = FIRST; j < 4; ++j) {
    const double a = R[j][j], b = r[j];
    const double h = __builtin_fma(a, a, b * b);
    if (h == 0.0) continue;
    const double q = rsqrt_guarded(h);
    const double cs = a * q, sn = b * q;
    R[j][j] = h * q;
#pragma unroll
    for (int k = j + 1; k < 4; ++k) {
      const double x = R[j][k], y = r[k];
      R[j][k] = __builtin_fma(cs, x, sn * y);
      r[k] = __builtin_fma(cs, y, -(sn * x));
    }
  }
}
__device__ __forceinline__ void clear(double (&R)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) R[r][c] = 0.0;
}
// The rows of the triangle S rotated into R.
__device__ __forceinline__ void merge_triangle(double (&R)[4][4], const double (&S)[4][4]) {
  double r[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) r[c] = S[0][c];
  rotate_in<0>(R, r);
#pragma unroll
  for (int c = 0; c < 4; ++c) r[c] = S[1][c];
  rotate_in<1>(R, r);
#pragma unroll
  for (int c = 0; c < 4; ++c) r[c] = S[2][c];
  rotate_in<2>(R, r);
#pragma unroll
  for (int c = 0; c < 4; ++c) r[c] = S[3][c];
  rotate_in<3>(R, r);
}

// dlt_solve<true, false> from its matrix on: the iterate brought to max-norm [0.5, 1) by a power of two.
__device__ __forceinline__ void solve_matrix(const double (&M)[4][4], double (&Xs)[4]) {
  double xv[4];
  if (!null_gs_inverse_iteration(M, xv)) null_jacobi(M, xv);
  const double big = fmax(fmax(fabs(xv[0]), fabs(xv[1])), fmax(fabs(xv[2]), fabs(xv[3])));
  const int ex = -__builtin_amdgcn_frexp_exp(big);
#pragma unroll
  for (int i = 0; i < 4; ++i) Xs[i] = __builtin_amdgcn_ldexp(xv[i], ex);
}

// One term of reprojection_error and one of score_inlier's depth-sign tests, for the scaled vector Xs.
__device__ __forceinline__ double obs_residual(const Obs &o, const double (&Xs)[4], bool &infront) {
  double r[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) a = __builtin_fma(o.p[4 * k + c], Xs[c], a);
    r[k] = a;
  }
  const double iz = rcp_nr2_ieee(r[2]);
  const double ex = __builtin_fma(r[0], iz, -o.u), ey = __builtin_fma(r[1], iz, -o.v);
  const double s = det3_left(o.p) < 0 ? -1.0 : 1.0;
  const double n = o.p[8] * o.p[8] + o.p[9] * o.p[9] + o.p[10] * o.p[10];
  infront = s / n * r[2] / Xs[3] > 0;
  return sqrt_fast(__builtin_fma(ex, ex, ey * ey));
}

__device__ __forceinline__ bool all_finite(const double (&X)[4]) {
  return __builtin_isfinite(X[0]) && __builtin_isfinite(X[1]) && __builtin_isfinite(X[2]) && __builtin_isfinite(X[3]);
}

struct TriOut {
  double *X, *err;
  uint8_t *ok;
  int32_t *nused;
};

__device__ __forceinline__ void write_unsolved(const TriOut &out, int t, int nu, bool write) {
  if (!write) return;
#pragma unroll
  for (int c = 0; c < 4; ++c) out.X[4 * (size_t)t + c] = 0.0;
  if (out.ok) out.ok[t] = 0;
  if (out.nused) out.nused[t] = nu;
}

// Track t, members [b, e), by one lane.  `write`: whether this lane stores (the wave form runs it in all 64 lanes
// alike for a long track that has fewer than 3 usable members, and lane 0 stores).
__device__ __forceinline__ void solve_track_serial(const TriTables &tb, const float *__restrict__ geom,
                                                   const int32_t *__restrict__ members, const TriOut &out, int t,
                                                   long long b, long long e, bool write) {
  double M[4][4];  // the anchor's A while nu <= 2, the triangle R afterwards
  clear(M);
  int nu = 0;
  for (long long i = b; i < e; ++i) {
    Obs o;
    if (!load_obs(tb, geom, members, i, o)) continue;
    double r0[4], r1[4];
    obs_rows(o, r0, r1);
    if (nu == 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        M[0][c] = r0[c];
        M[1][c] = r1[c];
      }
    } else if (nu == 1) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        M[2][c] = r0[c];
        M[3][c] = r1[c];
      }
    } else {
      if (nu == 2) {
        double A[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) A[r][c] = M[r][c];
        clear(M);
#pragma unroll
        for (int r = 0; r < 4; ++r) rotate_in<0>(M, A[r]);
      }
      rotate_in<0>(M, r0);
      rotate_in<0>(M, r1);
    }
    ++nu;
  }
  if (nu < 2) {
    if (write && out.err)
      for (long long i = b; i < e; ++i) out.err[i] = __builtin_nan("");
    write_unsolved(out, t, nu, write);
    return;
  }
  double Xs[4], X[4];
  solve_matrix(M, Xs);
  dlt_finish(Xs, X);
  bool good = all_finite(X);
  for (long long i = b; i < e; ++i) {
    Obs o;
    double err = __builtin_nan("");
    if (load_obs(tb, geom, members, i, o)) {
      bool infront;
      err = obs_residual(o, Xs, infront);
      good = good && infront && (err <= tb.max_error);
    }
    if (write && out.err) out.err[i] = err;
  }
  if (!write) return;
#pragma unroll
  for (int c = 0; c < 4; ++c) out.X[4 * (size_t)t + c] = X[c];
  if (out.ok) out.ok[t] = good ? 1 : 0;
  if (out.nused) out.nused[t] = nu;
}

__device__ __forceinline__ bool takes_wave_form(long long len, int lane_max) { return len >= 3 && len > lane_max; }

__global__ __launch_bounds__(kDltThreads) void tracks_triangulate_lane_kernel(TriTables tb, const float *__restrict__ geom,
                                                                              const int32_t *__restrict__ members,
                                                                              TriOut out) {
  const long long t = (long long)blockIdx.x * kDltThreads + threadIdx.x;
  if (t >= tb.ntracks) return;
  const long long b = tb.track_off[t], e = tb.track_off[t + 1];
  if (takes_wave_form(e - b, tb.lane_max)) return;
  solve_track_serial(tb, geom, members, out, (int)t, b, e, true);
}

__global__ __launch_bounds__(kDltThreads) void tracks_triangulate_wave_kernel(TriTables tb, const float *__restrict__ geom,
                                                                              const int32_t *__restrict__ members,
                                                                              TriOut out) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6)));
  if (w >= tb.nwave) return;  // the whole wave
  const int t = tb.wave_list[w];
  const long long b = tb.track_off[t], e = tb.track_off[t + 1];

  double R[4][4];
  clear(R);
  int nu = 0;
  for (long long i = b + lane; i < e; i += 64) {
    Obs o;
    if (!load_obs(tb, geom, members, i, o)) continue;
    double r0[4], r1[4];
    obs_rows(o, r0, r1);
    rotate_in<0>(R, r0);
    rotate_in<0>(R, r1);
    ++nu;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) nu += __shfl_xor(nu, d, 64);
  if (nu < 3) {  // wave-uniform: the anchor's arithmetic, or an unsolved track
    solve_track_serial(tb, geom, members, out, t, b, e, lane == 0);
    return;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    double lo[4][4], hi[4][4];
    clear(lo);
    clear(hi);
    const bool upper = (lane & d) != 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = r; c < 4; ++c) {
        const double mine = R[r][c], theirs = __shfl_xor(mine, d, 64);
        lo[r][c] = upper ? theirs : mine;
        hi[r][c] = upper ? mine : theirs;
      }
    merge_triangle(lo, hi);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = r; c < 4; ++c) R[r][c] = lo[r][c];
  }
  double Xs[4], X[4];
  solve_matrix(R, Xs);
  dlt_finish(Xs, X);
  bool good = all_finite(X);
  for (long long i = b + lane; i < e; i += 64) {
    Obs o;
    double err = __builtin_nan("");
    if (load_obs(tb, geom, members, i, o)) {
      bool infront;
      err = obs_residual(o, Xs, infront);
      good = good && infront && (err <= tb.max_error);
    }
    if (out.err) out.err[i] = err;
  }
  const bool all_good = __ballot(!good) == 0ull;
  if (lane != 0) return;
#pragma unroll
  for (int c = 0; c < 4; ++c) out.X[4 * (size_t)t + c] = X[c];
  if (out.ok) out.ok[t] = all_good ? 1 : 0;
  if (out.nused) out.nused[t] = nu;
}

std::atomic<int> &long_setting() {
  static std::atomic<int> v{kDefaultLong};
  return v;
}

// The plan under the setting L, which a call reads once.
void plan_with(const long long *track_off, int ntracks, int L, TracksTriangulatePlan *plan) {
  *plan = TracksTriangulatePlan();
  for (int t = 0; t < ntracks; ++t) {
    const long long len = track_off[t + 1] - track_off[t];
    plan->longest = std::max(plan->longest, len);
    if (len >= 3 && len > L) plan->wave_list.push_back(t);
  }
  plan->wave_tracks = (long long)plan->wave_list.size();
  plan->lane_tracks = ntracks - plan->wave_tracks;
  // one lane per track of the call, in track order: the lanes of wave-form tracks leave at once
  plan->lane_groups = plan->lane_tracks > 0 ? ((long long)ntracks + kDltThreads - 1) / kDltThreads : 0;
}

}  // namespace

int tracks_triangulate_set_long(int L) { return long_setting().exchange(L); }
int tracks_triangulate_get_long() { return long_setting().load(); }

void tracks_triangulate_plan(const long long *track_off, int ntracks, TracksTriangulatePlan *plan) {
  plan_with(track_off, ntracks, tracks_triangulate_get_long(), plan);
}

int tracks_triangulate_check(const void *geom, const long long *seg_off, int nseg, const double *cams,
                             const long long *track_off, int ntracks, const void *members, long long nmembers,
                             double max_error, const void *X, const void *err, const void *ok, const void *nused) {
  if (nseg < 0 || ntracks < 0 || nmembers < 0)
    return set_error(SPV_ERR_INVALID, "negative count (nseg=%d, ntracks=%d, nmembers=%lld)", nseg, ntracks, nmembers);
  SPV_TRY(check_offsets(seg_off, nseg, "seg_off"));
  if (nmembers >= (1ll << 31)) return set_error(SPV_ERR_INVALID, "%lld members, must be below 2^31", nmembers);
  SPV_TRY(check_offsets(track_off, ntracks, "track_off"));
  if (track_off[ntracks] != nmembers)
    return set_error(SPV_ERR_INVALID, "track_off ends at %lld, must end at nmembers = %lld", track_off[ntracks], nmembers);
  if (max_error != max_error) return set_error(SPV_ERR_INVALID, "max_error is NaN");
  if ((nseg > 0 && !cams) || (nmembers > 0 && !members) || (nmembers > 0 && seg_off[nseg] > 0 && !geom) || (ntracks > 0 && !X))
    return set_error(SPV_ERR_INVALID, "null pointer");
  if (((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(err)) & 7) || (reinterpret_cast<uintptr_t>(nused) & 3) ||
      (reinterpret_cast<uintptr_t>(geom) & 3) || (reinterpret_cast<uintptr_t>(members) & 3))
    return set_error(SPV_ERR_INVALID, "pointers must be aligned to their element size");
  (void)ok;
  return SPV_OK;
}

int tracks_triangulate_run(const float *d_geom, const long long *seg_off, int nseg, const double *cams,
                           const int32_t *use_set, const long long *track_off, int ntracks, const int32_t *d_members,
                           long long nmembers, double max_error, double *d_X, double *d_err, uint8_t *d_ok,
                           int32_t *d_nused, hipStream_t stream) {
  SPV_TRY(tracks_triangulate_check(d_geom, seg_off, nseg, cams, track_off, ntracks, d_members, nmembers, max_error, d_X,
                                   d_err, d_ok, d_nused));
  if (ntracks == 0) return SPV_OK;
  const int L = tracks_triangulate_get_long();
  TracksTriangulatePlan plan;
  plan_with(track_off, ntracks, L, &plan);
  const size_t nwave = plan.wave_list.size();

  // the call's tables, one upload: cameras | seg_off | track_off | use_set | the wave-form list
  const size_t off_seg = (size_t)nseg * 12 * sizeof(double), off_trk = off_seg + ((size_t)nseg + 1) * sizeof(long long);
  const size_t off_use = off_trk + ((size_t)ntracks + 1) * sizeof(long long);
  const size_t off_list = off_use + (use_set ? (size_t)nseg * sizeof(int32_t) : 0);
  const size_t table_bytes = off_list + nwave * sizeof(int32_t);
  std::vector<unsigned char> host(std::max<size_t>(table_bytes, 1), 0);
  double *h_cams = reinterpret_cast<double *>(host.data());
  for (int s = 0; s < nseg; ++s) {
    if (use_set && !use_set[s]) continue;  // a set without a camera: its row is not read
    memcpy(h_cams + (size_t)s * 12, cams + (size_t)s * 12, 12 * sizeof(double));
  }
  memcpy(host.data() + off_seg, seg_off, ((size_t)nseg + 1) * sizeof(long long));
  memcpy(host.data() + off_trk, track_off, ((size_t)ntracks + 1) * sizeof(long long));
  if (use_set && nseg > 0) memcpy(host.data() + off_use, use_set, (size_t)nseg * sizeof(int32_t));
  if (nwave) memcpy(host.data() + off_list, plan.wave_list.data(), nwave * sizeof(int32_t));

  DevBuf ws;
  SPV_TRY(ws.alloc(host.size()));
  // the scratch goes back to the cache behind the last kernel of this call, on every way out
  struct Release {
    DevBuf &b;
    hipStream_t st;
    ~Release() { b.release_after(st); }
  } release{ws, stream};
  unsigned char *base = ws.as<unsigned char>();
  // (pageable source: the copy has left `host` when the call returns)
  SPV_HIP_CHECK(hipMemcpyAsync(base, host.data(), host.size(), hipMemcpyHostToDevice, stream));
  TriTables tb;
  tb.cams = reinterpret_cast<const double *>(base);
  tb.seg_off = reinterpret_cast<const long long *>(base + off_seg);
  tb.track_off = reinterpret_cast<const long long *>(base + off_trk);
  tb.use_set = use_set ? reinterpret_cast<const int32_t *>(base + off_use) : nullptr;
  tb.wave_list = reinterpret_cast<const int32_t *>(base + off_list);
  tb.nseg = nseg;
  tb.ntracks = ntracks;
  tb.nwave = (int)nwave;
  tb.lane_max = L;
  tb.max_error = max_error;
  const TriOut out{d_X, d_err, d_ok, d_nused};
  if (plan.lane_groups > 0) {
    ProfScope prof("tracks_triangulate", stream);
    hipLaunchKernelGGL(tracks_triangulate_lane_kernel, dim3((unsigned)plan.lane_groups), dim3(kDltThreads), 0, stream, tb, d_geom,
                       d_members, out);
    SPV_HIP_CHECK(hipGetLastError());
  }
  if (nwave > 0) {
    ProfScope prof("tracks_triangulate_long", stream);
    hipLaunchKernelGGL(tracks_triangulate_wave_kernel, dim3((unsigned)((nwave + kWavesPerGroup - 1) / kWavesPerGroup)),
                       dim3(kDltThreads), 0, stream, tb, d_geom, d_members, out);
    SPV_HIP_CHECK(hipGetLastError());
  }
  return SPV_OK;
}

}  // namespace spv
