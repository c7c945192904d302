// bundle_device.h -- device helpers of bundle_adjust.hip: the residual model of one observation, its Jacobians, the
// closed-form inverse of a symmetric 3x3 block, the 6x6 Cholesky inverse of a camera block and Rodrigues' formula.
// Everything is fp64 with IEEE division and square root (the library is built with -ffp-contract=off), so a kernel
// that calls these twice on the same values gets the same bits twice.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace spv {

constexpr double kBundleDiagMin = 1e-6, kBundleDiagMax = 1e32;  // the clamp of D = diag(H)

// A set's camera as the kernels read it: K = [k0 k1 k2; 0 k3 k4; 0 0 1] and the row-major [R | t].
struct BundleCam {
  double k[5];
  double p[12];
};
__device__ __forceinline__ void bundle_load_cam(const double *__restrict__ K5, const double *__restrict__ pose, int s,
                                                BundleCam &c) {
#pragma unroll
  for (int i = 0; i < 5; ++i) c.k[i] = K5[5 * (size_t)s + i];
#pragma unroll
  for (int i = 0; i < 12; ++i) c.p[i] = pose[12 * (size_t)s + i];
}

// y = R X + t, (pu, pv) its pixel, (ru, rv) = pixel - (u, v).  Returns whether y2 > 0 and the residual is finite.
struct BundleProj {
  double y[3], a, b, iz, ru, rv;
};
__device__ __forceinline__ bool bundle_project(const BundleCam &c, const double (&X)[3], double u, double v, BundleProj &o) {
#pragma unroll
  for (int r = 0; r < 3; ++r) o.y[r] = c.p[4 * r] * X[0] + c.p[4 * r + 1] * X[1] + c.p[4 * r + 2] * X[2] + c.p[4 * r + 3];
  o.iz = 1.0 / o.y[2];
  o.a = o.y[0] * o.iz;
  o.b = o.y[1] * o.iz;
  o.ru = (c.k[0] * o.a + c.k[1] * o.b + c.k[2]) - u;
  o.rv = (c.k[3] * o.b + c.k[4]) - v;
  return o.y[2] > 0.0 && __builtin_isfinite(o.ru) && __builtin_isfinite(o.rv);
}

// The loss of a residual of norm n and its first-order weight.
__device__ __forceinline__ double bundle_rho(double n, double huber, double &w) {
  if (n <= huber) {
    w = 1.0;
    return 0.5 * n * n;
  }
  w = huber / n;
  return huber * (n - 0.5 * huber);
}

// Jc (2x6, rotation columns first) and Jp (2x3) of the observation at omega = 0, both times sw.
__device__ __forceinline__ void bundle_jacobians(const BundleCam &c, const BundleProj &o, double sw, double (&Jc)[2][6],
                                                 double (&Jp)[2][3]) {
  // d(u, v) / dy
  double Jy[2][3];
  Jy[0][0] = sw * (c.k[0] * o.iz);
  Jy[0][1] = sw * (c.k[1] * o.iz);
  Jy[0][2] = sw * (-(c.k[0] * o.a + c.k[1] * o.b) * o.iz);
  Jy[1][0] = 0.0;
  Jy[1][1] = sw * (c.k[3] * o.iz);
  Jy[1][2] = sw * (-(c.k[3] * o.b) * o.iz);
  const double a0 = o.y[0] - c.p[3], a1 = o.y[1] - c.p[7], a2 = o.y[2] - c.p[11];  // R X
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    Jc[j][0] = Jy[j][2] * a1 - Jy[j][1] * a2;  // Jy (-[R X]x)
    Jc[j][1] = Jy[j][0] * a2 - Jy[j][2] * a0;
    Jc[j][2] = Jy[j][1] * a0 - Jy[j][0] * a1;
    Jc[j][3] = Jy[j][0];
    Jc[j][4] = Jy[j][1];
    Jc[j][5] = Jy[j][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) Jp[j][k] = Jy[j][0] * c.p[k] + Jy[j][1] * c.p[4 + k] + Jy[j][2] * c.p[8 + k];
  }
}

__device__ __forceinline__ double bundle_clamp_diag(double d) { return fmin(fmax(d, kBundleDiagMin), kBundleDiagMax); }

// The symmetric 3x3 V = (v00 v01 v02 v11 v12 v22) -> (V + lambda clamp(diag V))^-1 in the same packing, by cofactors.
__device__ __forceinline__ void bundle_sym3_inverse(const double (&V)[6], double lambda, double (&I)[6]) {
  const double a = V[0] + lambda * bundle_clamp_diag(V[0]), b = V[1], c = V[2];
  const double d = V[3] + lambda * bundle_clamp_diag(V[3]), e = V[4];
  const double f = V[5] + lambda * bundle_clamp_diag(V[5]);
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double det = a * c00 + b * c01 + c * c02;
  const double id = 1.0 / det;
  I[0] = c00 * id;
  I[1] = c01 * id;
  I[2] = c02 * id;
  I[3] = (a * f - c * c) * id;
  I[4] = (b * c - a * e) * id;
  I[5] = (a * d - b * b) * id;
}
__device__ __forceinline__ void bundle_sym3_mul(const double (&S)[6], const double (&x)[3], double (&y)[3]) {
  y[0] = S[0] * x[0] + S[1] * x[1] + S[2] * x[2];
  y[1] = S[1] * x[0] + S[3] * x[1] + S[4] * x[2];
  y[2] = S[2] * x[0] + S[4] * x[1] + S[5] * x[2];
}

// The place of (r, c), r <= c, in the packed upper triangle of a symmetric 6x6 block (21 values, row by row).
__host__ __device__ constexpr int bundle_u21(int r, int c) { return r * 6 - r * (r - 1) / 2 + (c - r); }

// M (6x6, symmetric positive definite, full storage) -> its inverse in place: Cholesky M = L L^T, L^-1, L^-T L^-1.
// A block that is not positive definite gives NaNs, which the step that uses them then fails to accept.
__device__ __forceinline__ void bundle_spd6_inverse(double (&M)[6][6]) {
  double L[6][6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = M[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    const double l = sqrt(d), il = 1.0 / l;
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = M[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
      L[i][j] = v * il;
    }
  }
  double Li[6][6];  // lower triangle of L^-1
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    Li[j][j] = 1.0 / L[j][j];
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) v -= L[i][k] * Li[k][j];
      Li[i][j] = v / L[i][i];
    }
  }
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) {
      double v = 0.0;
#pragma unroll
      for (int k = c; k < 6; ++k) v += Li[k][r] * Li[k][c];
      M[r][c] = v;
      M[c][r] = v;
    }
}

// pose <- (Exp(omega) R | t + tau), Rodrigues: Exp(w) = I + sin(th)/th [w]x + (1 - cos th)/th^2 [w]x^2.
__device__ __forceinline__ void bundle_move_pose(const double *__restrict__ in, const double (&d)[6], double *__restrict__ out) {
  const double wx = d[0], wy = d[1], wz = d[2];
  const double th2 = wx * wx + wy * wy + wz * wz, th = sqrt(th2);
  double A, B;
  if (th < 1e-8) {
    A = 1.0 - th2 / 6.0;
    B = 0.5 - th2 / 24.0;
  } else {
    A = sin(th) / th;
    const double h = sin(0.5 * th) / th;
    B = 2.0 * h * h;
  }
  double E[3][3];
  E[0][0] = 1.0 - B * (wy * wy + wz * wz);
  E[0][1] = -A * wz + B * wx * wy;
  E[0][2] = A * wy + B * wx * wz;
  E[1][0] = A * wz + B * wx * wy;
  E[1][1] = 1.0 - B * (wx * wx + wz * wz);
  E[1][2] = -A * wx + B * wy * wz;
  E[2][0] = -A * wy + B * wx * wz;
  E[2][1] = A * wx + B * wy * wz;
  E[2][2] = 1.0 - B * (wx * wx + wy * wy);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[4 * r + c] = E[r][0] * in[c] + E[r][1] * in[4 + c] + E[r][2] * in[8 + c];
    out[4 * r + 3] = in[4 * r + 3] + d[3 + r];
  }
}

}  // namespace spv
