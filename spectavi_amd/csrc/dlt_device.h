// dlt_device.h -- the per-point fp64 arithmetic of the DLT and of RANSAC scoring, as __device__ functions.
//
// dlt.hip (triangulation, reprojection error, the scorer of one correspondence set) and ransac_batch.hip (the
// scorer of many sets) compile the same text: the results of a (camera, correspondence) pair are the same
// bits whichever kernel asks for them.  What the functions do and why is told in dlt.hip's header.
#pragma once

#include "common.h"

namespace spv {
namespace {

constexpr int kDltThreads = 256;
constexpr int kMaxSweeps = 30;

struct Cameras {
  double p0[12];
  double p1[12];
};

// ---- fp64 reciprocals without the IEEE sequences ------------------------------------------
// Measured on gfx950 (tools/exp/f64_rate.hip, profiles/r03_f64_rate.txt): v_fma / v_mul / v_add /
// v_div_scale / v_div_fmas / v_div_fixup / v_ldexp _f64 issue every 4 cycles per SIMD, v_rcp_f64 /
// v_rsq_f64 / v_sqrt_f64 every 16 and are good to 2^-24 (4.6e-8); one Newton step brings them to
// 2e-15, two to 1.1e-16 / 1.4e-16 (worst of 1M values, against 2^-53 = 1.1e-16).  An IEEE x / y
// compiles to 2 v_div_scale + v_rcp + 7 fma / mul + v_div_fmas + v_div_fixup = ~60 issue cycles, an
// IEEE sqrt to ~80; rcp_nr2 is 32, rsqrt_nr2 44.
__device__ __forceinline__ double rcp_nr2(double x) {
  double r = __builtin_amdgcn_rcp(x);
  double e = __builtin_fma(-x, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-x, r, 1.0);
  return __builtin_fma(r, e, r);
}
// the same, keeping IEEE's answers at the ends: 1/0 = inf, 1/inf = 0 (Newton turns both into nan)
__device__ __forceinline__ double rcp_nr2_ieee(double x) {
  const double r0 = __builtin_amdgcn_rcp(x);
  double e = __builtin_fma(-x, r0, 1.0);
  double r = __builtin_fma(r0, e, r0);
  e = __builtin_fma(-x, r, 1.0);
  r = __builtin_fma(r, e, r);
  return (r0 == 0.0 || __builtin_isinf(r0)) ? r0 : r;
}
__device__ __forceinline__ double rsqrt_nr2(double x) {
  double q = __builtin_amdgcn_rsq(x);
  double t = __builtin_fma(-(x * q), q, 1.0);
  q = __builtin_fma(0.5 * q, t, q);
  t = __builtin_fma(-(x * q), q, 1.0);
  return __builtin_fma(0.5 * q, t, q);
}
// sqrt(s) for s >= 0 as s * rsqrt(s); zero, +inf, nan and the ranges whose reciprocal root would
// overflow or lose bits take the IEEE instruction sequence (exact zeros occur: noise-free points
// reproject exactly; a squared residual that overflows must stay +inf, where v_rsq_f64(inf) = 0 and
// the Newton step would make it inf * 0 = nan)
__device__ __forceinline__ double sqrt_fast(double s) {
  if (!(s >= 0x1p-900 && s <= 0x1p900)) return sqrt(s);
  return s * rsqrt_nr2(s);
}

// The perspective division (a / w, b / w) as a * r, b * r with r = rcp_nr2(w) + 2 Newton steps.
// Where |w| is outside [2^-1020, 2^1020] (1 / w subnormal or overflowing, or w itself subnormal --
// what v_rcp_f64 does there is not relied on), a, b and w are first brought to |w| in [0.5, 1) by one
// exact power of two; 0, inf and nan w are left as they are (frexp exponent 0) and keep IEEE's
// answers.  So the quotients are the same bits after the row (a, b, w) is rescaled by any power of
// two that leaves it exact.  a and b are returned scaled.  Both views of a point go through one
// range test: the rescaling is a branch that almost no wave takes, and in range rcp_nr2 needs no
// guard for 0 / inf.
__device__ __forceinline__ bool rcp_in_range(double w) {
  const double aw = fabs(w);
  return aw >= 0x1p-1020 && aw <= 0x1p1020;
}
__device__ __forceinline__ double rcp_hom_slow(double &a, double &b, double w) {
  const int ex = -__builtin_amdgcn_frexp_exp(w);
  a = __builtin_amdgcn_ldexp(a, ex);
  b = __builtin_amdgcn_ldexp(b, ex);
  return rcp_nr2_ieee(__builtin_amdgcn_ldexp(w, ex));
}
__device__ __forceinline__ void rcp_hom2(double &a0, double &b0, double w0, double &a1, double &b1, double w1,
                                         double &r0, double &r1) {
  if (__builtin_expect(rcp_in_range(w0) && rcp_in_range(w1), 1)) {
    r0 = rcp_nr2(w0);
    r1 = rcp_nr2(w1);
  } else {
    r0 = rcp_hom_slow(a0, b0, w0);
    r1 = rcp_hom_slow(a1, b1, w1);
  }
}

// ---- null vector, method 1: one-sided (Hestenes) Jacobi, always converges ----------------
__device__ __forceinline__ void null_jacobi(const double (&A0)[4][4], double (&xv)[4]) {
  double A[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) A[r][c] = A0[r][c];
  double V[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) V[r][c] = (r == c) ? 1.0 : 0.0;

  const double eps2 = 1e-30;  // (1e-15)^2
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          alpha = __builtin_fma(A[i][p], A[i][p], alpha);
          beta = __builtin_fma(A[i][q], A[i][q], beta);
          gamma = __builtin_fma(A[i][p], A[i][q], gamma);
        }
        // skip test |gamma| > eps*sqrt(alpha*beta), squared to avoid the square root
        if (gamma * gamma > eps2 * (alpha * beta)) {
          rotated = true;
          // tan of the rotation angle, t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)) with
          // zeta = (beta - alpha) / (2 gamma), rearranged to one sqrt and one division
          const double dd = beta - alpha;
          const double g2 = 2.0 * gamma;
          const double hh = sqrt(__builtin_fma(dd, dd, g2 * g2));
          const double tn = g2 / (dd + (dd < 0.0 ? -hh : hh));
          const double cs = rsqrt_nr2(__builtin_fma(tn, tn, 1.0));  // argument >= 1
          const double sn = cs * tn;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const double ap = A[i][p], aq = A[i][q];
            A[i][p] = __builtin_fma(cs, ap, -(sn * aq));
            A[i][q] = __builtin_fma(sn, ap, cs * aq);
            const double vp_ = V[i][p], vq_ = V[i][q];
            V[i][p] = __builtin_fma(cs, vp_, -(sn * vq_));
            V[i][q] = __builtin_fma(sn, vp_, cs * vq_);
          }
        }
      }
    }
    if (!rotated) break;
  }
  // smallest column norm -> null direction
  double best = 0.0;
  int kbest = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    double nn = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) nn = __builtin_fma(A[i][c], A[i][c], nn);
    if (c == 0 || nn < best) {
      best = nn;
      kbest = c;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    xv[i] = kbest == 0 ? V[i][0] : (kbest == 1 ? V[i][1] : (kbest == 2 ? V[i][2] : V[i][3]));
}

// ---- null vector, method 2: square-root-free Gram-Schmidt + inverse iteration ------------
// A = Q U with orthogonal (not normalised) columns q_j, d_j = |q_j|^2 and U unit upper
// triangular (modified Gram-Schmidt, no pivoting: only U and d are used, and those are
// backward stable whatever the column order), so A^T A = U^T D U.  The smallest right singular
// vector of A is found by inverse iteration on U^T D U: two unit-triangular solves and one
// diagonal scaling per step, contraction (sigma4/sigma3)^2.  Division-free after the three
// reciprocals 1/d_0..1/d_2 the orthogonalisation needs: the diagonal solve is scaled by d_3
// (y_j = z_j d_3 / d_j, y_3 = z_3), which also keeps the un-normalised iterates from growing by
// 1/sigma4^2 per step (d_3 >= sigma4^2 is the squared distance of the last column from the span of
// the others: the growth per step is d_3 / sigma4^2, O(1) for a consistent point), and the
// convergence test compares DIRECTIONS of consecutive un-normalised iterates,
//   max_i |w_i max|v| - v_i max|w|| <= 1e-13 max|v| max|w|
// (no sign ambiguity: (A^T A)^-1 is positive definite).  Steps 0 (a bare back-substitution from
// e4), 1 and 2 run unconditionally, then a point stops at the first step that moved its direction
// by no more than 1e-13 (step 3 for pixel noise 1e-3; at most 8): what is left of the direction error
// is then 1e-13 rho / (1 - rho), rho = (sigma4/sigma3)^2 the contraction (1e-12 until fuzz seed
// 20261004 case 5249 -- an inconsistent pair, rho = 0.036 -- came out 3.4e-14 from the oracle).
// ~300 fp64 instructions.
// Returns false when the last step still moved it (ill-separated sigma3, sigma4), or the
// iterate left the range (inf / nan from a degenerate A, overflow of a badly conditioned one);
// the caller then falls back to method 1.
__device__ __forceinline__ bool null_gs_inverse_iteration(const double (&A0)[4][4], double (&xv)[4]) {
  double col[4][4];  // col[c][r]
  double U[4][4];    // strictly upper part used
  double g[3];       // d_3 / d_j
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < 4; ++r) col[c][r] = A0[r][c];
  double tiny2 = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double d = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) d = __builtin_fma(col[j][r], col[j][r], d);
    if (j == 0) tiny2 = 4.930380657631324e-32 * d;  // eps^2 |a_0|^2
    if (!(d > tiny2)) d = tiny2;
    if (j == 3) {
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] *= d;
      break;
    }
    const double idj = rcp_nr2(d);
    g[j] = idj;
#pragma unroll
    for (int k = j + 1; k < 4; ++k) {
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) s = __builtin_fma(col[j][r], col[k][r], s);
      const double u = s * idj;
      U[j][k] = u;
#pragma unroll
      for (int r = 0; r < 4; ++r) col[k][r] = __builtin_fma(-u, col[j][r], col[k][r]);
    }
  }
  double v3 = 1.0;
  double v2 = -U[2][3];
  double v1 = __builtin_fma(-U[1][2], v2, -U[1][3]);
  double v0 = __builtin_fma(-U[0][1], v1, __builtin_fma(-U[0][2], v2, -U[0][3]));
  double w0, w1, w2, w3;
  auto step = [&]() {  // w = d_3 (U^T D U)^-1 v
    // U^T z = v
    const double z0 = v0;
    const double z1 = __builtin_fma(-U[0][1], z0, v1);
    const double z2 = __builtin_fma(-U[1][2], z1, __builtin_fma(-U[0][2], z0, v2));
    const double z3 = __builtin_fma(-U[2][3], z2, __builtin_fma(-U[1][3], z1, __builtin_fma(-U[0][3], z0, v3)));
    // D y = d_3 z
    const double y0 = z0 * g[0], y1 = z1 * g[1], y2 = z2 * g[2];
    // U w = y
    w3 = z3;
    w2 = __builtin_fma(-U[2][3], w3, y2);
    w1 = __builtin_fma(-U[1][3], w3, __builtin_fma(-U[1][2], w2, y1));
    w0 = __builtin_fma(-U[0][3], w3, __builtin_fma(-U[0][2], w2, __builtin_fma(-U[0][1], w1, y0)));
  };
#pragma unroll
  for (int it = 1; it <= 2; ++it) {
    step();
    v0 = w0;
    v1 = w1;
    v2 = w2;
    v3 = w3;
  }
  double bv = fmax(fmax(fabs(v0), fabs(v1)), fmax(fabs(v2), fabs(v3)));
  bool ok = false;
  for (int it = 3; it < 8; ++it) {
    step();
    const double bw = fmax(fmax(fabs(w0), fabs(w1)), fmax(fabs(w2), fabs(w3)));
    const double e0 = fabs(__builtin_fma(w0, bv, -(v0 * bw))), e1 = fabs(__builtin_fma(w1, bv, -(v1 * bw)));
    const double e2 = fabs(__builtin_fma(w2, bv, -(v2 * bw))), e3 = fabs(__builtin_fma(w3, bv, -(v3 * bw)));
    const double bound = 1e-13 * (bw * bv);
    // a bound of 0 or inf is an iterate out of range, never agreement
    ok = (fmax(fmax(e0, e1), fmax(e2, e3)) <= bound) && (bound >= 1e-290) && (bound <= 1e290);
    v0 = w0;
    v1 = w1;
    v2 = w2;
    v3 = w3;
    bv = bw;
    if (ok) break;
  }
  if (!ok) return false;
  xv[0] = v0;
  xv[1] = v1;
  xv[2] = v2;
  xv[3] = v3;
  return true;
}

// FAST: method 2 with method 1 as fallback (triangulate / reprojection error: consistent
// correspondences, sigma4 << sigma3); !FAST: method 1 only (RANSAC scoring, where most
// hypotheses are inconsistent and method 2 would rarely converge).
// A = [u P0[2]-P0[0]; v P0[2]-P0[1]; u' P1[2]-P1[0]; v' P1[2]-P1[1]] (reference src/DltTriangulator.h:38-54)
__device__ __forceinline__ void dlt_matrix(const Cameras &cam, double x0, double x1, double x2, double y0,
                                           double y1, double y2, double (&A)[4][4], double &u, double &v,
                                           double &up, double &vp) {
  double ix, iy;  // one reciprocal per view; x / 0 stays +-inf or nan
  rcp_hom2(x0, x1, x2, y0, y1, y2, ix, iy);
  u = x0 * ix;
  v = x1 * ix;
  up = y0 * iy;
  vp = y1 * iy;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    A[0][c] = __builtin_fma(u, cam.p0[8 + c], -cam.p0[0 + c]);
    A[1][c] = __builtin_fma(v, cam.p0[8 + c], -cam.p0[4 + c]);
    A[2][c] = __builtin_fma(up, cam.p1[8 + c], -cam.p1[0 + c]);
    A[3][c] = __builtin_fma(vp, cam.p1[8 + c], -cam.p1[4 + c]);
  }
}

// unit 2-norm and the canonical sign.  xv is an un-normalised iterate of any magnitude (or a
// column of the Jacobi's V): it is first brought to max-norm in [0.5, 1) by an exact power of two,
// so the sum of squares neither overflows nor underflows.
__device__ __forceinline__ void dlt_finish(const double (&xv)[4], double (&X)[4]) {
  const double big = fmax(fmax(fabs(xv[0]), fabs(xv[1])), fmax(fabs(xv[2]), fabs(xv[3])));
  const int ex = -__builtin_amdgcn_frexp_exp(big);  // 0 for big = 0 / inf / nan
  double sv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) sv[i] = __builtin_amdgcn_ldexp(xv[i], ex);
  double nrm2 = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) nrm2 = __builtin_fma(sv[i], sv[i], nrm2);
  bool neg = false;
  if (xv[3] != 0.0)
    neg = xv[3] < 0.0;
  else if (xv[0] != 0.0)
    neg = xv[0] < 0.0;
  else if (xv[1] != 0.0)
    neg = xv[1] < 0.0;
  else
    neg = xv[2] < 0.0;
  const double q = rsqrt_nr2(nrm2);
  const double scale = neg ? -q : q;
#pragma unroll
  for (int i = 0; i < 4; ++i) X[i] = sv[i] * scale;
}

// reprojection_error() of reference src/DltTriangulator.h:61-62, 67-74 for a solved point: the sum
// of the two image-plane residual norms.  One reciprocal per camera; z0 / z1 = the depths P X [2].
__device__ __forceinline__ double reprojection_error(const Cameras &cam, const double (&X)[4], double u, double v,
                                                     double up, double vp, double &z0, double &z1) {
  double r0[3], r1[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      a = __builtin_fma(cam.p0[4 * r + c], X[c], a);
      b = __builtin_fma(cam.p1[4 * r + c], X[c], b);
    }
    r0[r] = a;
    r1[r] = b;
  }
  z0 = r0[2];
  z1 = r1[2];
  // (the depths need no range test: |P X [2]| >= 2^1020 takes cameras near the top of the range, and a
  // subnormal depth's reciprocal overflows or its quotients do; 0 and inf keep IEEE's answers)
  const double i0 = rcp_nr2_ieee(r0[2]), i1 = rcp_nr2_ieee(r1[2]);
  const double e0x = __builtin_fma(r0[0], i0, -u), e0y = __builtin_fma(r0[1], i0, -v);
  const double e1x = __builtin_fma(r1[0], i1, -up), e1y = __builtin_fma(r1[1], i1, -vp);
  return sqrt_fast(__builtin_fma(e0x, e0x, e0y * e0y)) + sqrt_fast(__builtin_fma(e1x, e1x, e1y * e1y));
}

// FAST: method 2 with method 1 as fallback (consistent correspondences converge in 3-4 steps;
// whatever does not within 8 takes the Jacobi); !FAST: method 1 only.
// UNIT = false: X is only brought to max-norm [0.5, 1) by a power of two, neither normalised nor
// sign-canonicalised -- enough for the reprojection error, which is a ratio of components of P X.
template <bool FAST, bool UNIT = true>
__device__ __forceinline__ void dlt_solve(const Cameras &cam, double x0, double x1, double x2,
                                          double y0, double y1, double y2, double (&X)[4],
                                          double &u, double &v, double &up, double &vp) {
  double A[4][4];
  dlt_matrix(cam, x0, x1, x2, y0, y1, y2, A, u, v, up, vp);
  double xv[4];
  bool done = false;
  if (FAST) done = null_gs_inverse_iteration(A, xv);
  if (!done) null_jacobi(A, xv);
  if (UNIT) {
    dlt_finish(xv, X);
  } else {
    const double big = fmax(fmax(fabs(xv[0]), fabs(xv[1])), fmax(fabs(xv[2]), fabs(xv[3])));
    const int ex = -__builtin_amdgcn_frexp_exp(big);
#pragma unroll
    for (int i = 0; i < 4; ++i) X[i] = __builtin_amdgcn_ldexp(xv[i], ex);
  }
}

__device__ __forceinline__ double det3_left(const double *P) {
  return P[0] * (P[5] * P[10] - P[6] * P[9]) - P[1] * (P[4] * P[10] - P[6] * P[8]) +
         P[2] * (P[4] * P[9] - P[5] * P[8]);
}

// reprojection_error() <= max_error && is_infront_both_cameras() (src/DltTriangulator.h:67-86)
__device__ __forceinline__ bool score_inlier(const Cameras &cam, const double (&X)[4], double u, double v,
                                             double up, double vp, double max_error) {
  double z0, z1;
  const double err = reprojection_error(cam, X, u, v, up, vp, z0, z1);
  const double s0 = det3_left(cam.p0) < 0 ? -1.0 : 1.0, s1 = det3_left(cam.p1) < 0 ? -1.0 : 1.0;
  const double n0 = cam.p0[2] * cam.p0[2] + cam.p0[6] * cam.p0[6] + cam.p0[10] * cam.p0[10];
  const double n1 = cam.p1[2] * cam.p1[2] + cam.p1[6] * cam.p1[6] + cam.p1[10] * cam.p1[10];
  const double dc0 = s0 / n0 * z0 / X[3];
  const double dc1 = s1 / n1 * z1 / X[3];
  return (err <= max_error) && (dc0 > 0) && (dc1 > 0);
}

// Every (correspondence, hypothesis) pair is solved by method 2 (8 steps) with method 1 as its
// fallback, exactly as dlt_solve<true> does it for one point.  Most hypotheses of a RANSAC run are
// wrong for most correspondences, and about one solve in five does not converge within the 8 steps
// (sigma4 / sigma3 has a median of 0.02 but a long tail); a wave that ran the ~3100-instruction Jacobi
// for its slow lanes in place would pay for it with all 64.  With a work list (TWO_PASS) the slow
// lanes are appended to it instead -- one atomicAdd per wave, (hypothesis, point) packed in 8 bytes --
// and dlt_score_fallback_kernel solves them afterwards in full waves.  Lanes that find the list full,
// and the form without a work list, run the fallback in place: the results do not depend on the path.
// The list is cut into kListShards segments with a counter each (64 bytes apart): every wave with
// slow lanes does one atomicAdd, and 70 000 of them on ONE address serialise at ~12 ns each (measured:
// the first version of this kernel spent 0.83 of its 0.9 ms there).
constexpr unsigned int kListShards = 1024;
constexpr unsigned int kCountStride = 16;  // uints between two counters
struct WorkList {
  unsigned int *count;          // [kListShards * kCountStride]; may exceed `segment`: the excess ran in place
  unsigned long long *entries;  // [kListShards][segment], (hypothesis << 40) | point
  unsigned int segment;         // entries per shard; 0 = no list
};

}  // namespace
}  // namespace spv
