// resect_device.h -- the arithmetic of camera resection (resect_batch.hip): the six-point solve of a try and the
// verdict of a (camera, row) pair.  The solve is plain C++ (sqrt, division, fma): it compiles for the host as well,
// where a stand-alone program can put it next to an SVD.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

namespace spv {
namespace {

// The rotation that takes (p, q) to (r, 0), applied to the pair (x, y): x' = cs x + sn y, y' = cs y - sn x.
__host__ __device__ __forceinline__ void resect_rot(double cs, double sn, double &x, double &y) {
  const double nx = __builtin_fma(cs, x, sn * y);
  y = __builtin_fma(cs, y, -(sn * x));
  x = nx;
}

// The row (a | bu | bv) = (X | u X | v X) rotated into the triangle R of the X parts (Givens, one rotation per
// column); the same rotations go over the right-hand blocks Tu and, with V, Tv.  What is left of bu and bv belongs to
// the left null space of the X parts.  A rotation whose pivot and entry are both zero is the identity.
template <bool V>
__host__ __device__ __forceinline__ void resect_rotate_in(double (&R)[4][4], double (&Tu)[4][4], double (&Tv)[4][4],
                                                          double (&a)[4], double (&bu)[4], double (&bv)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double p = R[j][j], q = a[j];
    const double h = __builtin_fma(p, p, q * q);
    if (h == 0.0) continue;
    const double r = sqrt(h);
    const double cs = p / r, sn = q / r;
    R[j][j] = r;
#pragma unroll
    for (int k = j + 1; k < 4; ++k) resect_rot(cs, sn, R[j][k], a[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      resect_rot(cs, sn, Tu[j][k], bu[k]);
      if (V) resect_rot(cs, sn, Tv[j][k], bv[k]);
    }
  }
}

// R y = T z for the upper triangle R.
__host__ __device__ __forceinline__ void resect_back_solve(const double (&R)[4][4], const double (&T)[4][4],
                                                           const double (&z)[4], double (&y)[4]) {
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s = __builtin_fma(T[j][k], z[k], s);
#pragma unroll
    for (int k = j + 1; k < 4; ++k) s = __builtin_fma(-R[j][k], y[k], s);
    y[j] = s / R[j][j];
  }
}

// The unit vector orthogonal to the three rows of C: the rows, each brought to unit length, are the columns of a
// 4 x 3 matrix that three Householder reflections make triangular; the last column of their product is orthogonal to
// all three whatever their condition, so nothing is pivoted.
__host__ __device__ __forceinline__ void resect_null3(const double (&C)[3][4], double (&n)[4]) {
  double B[4][3], beta[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double s = sqrt(C[c][0] * C[c][0] + C[c][1] * C[c][1] + C[c][2] * C[c][2] + C[c][3] * C[c][3]);
#pragma unroll
    for (int r = 0; r < 4; ++r) B[r][c] = C[c][r] / s;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {  // column k below row k becomes the reflection's vector
    double nn = 0.0;
#pragma unroll
    for (int r = k; r < 4; ++r) nn = __builtin_fma(B[r][k], B[r][k], nn);
    const double alpha = B[k][k] > 0 ? -sqrt(nn) : sqrt(nn);
    B[k][k] -= alpha;
    double vv = 0.0;
#pragma unroll
    for (int r = k; r < 4; ++r) vv = __builtin_fma(B[r][k], B[r][k], vv);
    beta[k] = vv > 0 ? 2.0 / vv : 0.0;
#pragma unroll
    for (int c = k + 1; c < 3; ++c) {
      double d = 0.0;
#pragma unroll
      for (int r = k; r < 4; ++r) d = __builtin_fma(B[r][k], B[r][c], d);
      d *= beta[k];
#pragma unroll
      for (int r = k; r < 4; ++r) B[r][c] = __builtin_fma(-d, B[r][k], B[r][c]);
    }
  }
  n[0] = n[1] = n[2] = 0.0;
  n[3] = 1.0;
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    double d = 0.0;
#pragma unroll
    for (int r = k; r < 4; ++r) d = __builtin_fma(B[r][k], n[r], d);
    d *= beta[k];
#pragma unroll
    for (int r = k; r < 4; ++r) n[r] = __builtin_fma(-d, B[r][k], n[r]);
  }
}

// The hypothesis of a try (include/spectavi_amd.h): the unit null vector of the 11 x 12 matrix of six rows (u, v, X),
// the sixth with its u row only, its last non-zero entry positive.  With M6 / M5 the 6 x 4 / 5 x 4 matrices of the
// X and Du, Dv the diagonals of the u and v, A p = 0 says M6 p1 = Du M6 p3 and M5 p2 = Dv M5 p3.  One Givens QR of
// the X, row by row, serves both: after five rows the triangle is M5's, after six M6's.  The parts of Q^T Du M6 and
// Q^T Dv M5 below the triangle -- two rows and one -- must vanish on p3, which is therefore the null vector of a
// 3 x 4 matrix; p1 and p2 follow from the triangles.  Degenerate subsets (a repeated row, coplanar X) end in a
// division by zero or in finite garbage.
__host__ __device__ __forceinline__ void resect_solve6(const double (&u)[6], const double (&v)[6], const double (&X)[6][4],
                                                       double (&P)[12]) {
  double R[4][4], Tu[4][4], Tv[4][4], R5[4][4], C[3][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) R[r][c] = Tu[r][c] = Tv[r][c] = 0.0;
  double a[4], bu[4], bv[4];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      a[c] = X[i][c];
      bu[c] = u[i] * X[i][c];
      bv[c] = v[i] * X[i][c];
    }
    resect_rotate_in<true>(R, Tu, Tv, a, bu, bv);
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {  // the fifth row's remainder
    C[0][c] = bu[c];
    C[1][c] = bv[c];
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) R5[r][c] = R[r][c];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    a[c] = X[5][c];
    bu[c] = u[5] * X[5][c];
    bv[c] = 0.0;
  }
  resect_rotate_in<false>(R, Tu, Tv, a, bu, bv);
#pragma unroll
  for (int c = 0; c < 4; ++c) C[2][c] = bu[c];

  double p3[4], p1[4], p2[4];
  resect_null3(C, p3);
  resect_back_solve(R, Tu, p3, p1);
  resect_back_solve(R5, Tv, p3, p2);
  double nn = 0.0;
#pragma unroll
  for (int c = 0; c < 4; ++c) nn += p1[c] * p1[c] + p2[c] * p2[c] + p3[c] * p3[c];
  double s = 1.0 / sqrt(nn);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    P[c] = p1[c] * s;
    P[4 + c] = p2[c] * s;
    P[8 + c] = p3[c] * s;
  }
  double last = 0.0;  // the last non-zero entry
#pragma unroll
  for (int c = 0; c < 12; ++c) last = P[c] != 0.0 ? P[c] : last;
  if (last < 0.0)
#pragma unroll
    for (int c = 0; c < 12; ++c) P[c] = -P[c];
}

// sign(det P[:, :3]) / |P[2, :3]|^2, the camera's factor of the depth term.
__host__ __device__ __forceinline__ double resect_depth_factor(const double (&P)[12]) {
  const double det = P[0] * (P[5] * P[10] - P[6] * P[9]) - P[1] * (P[4] * P[10] - P[6] * P[8]) +
                     P[2] * (P[4] * P[9] - P[5] * P[8]);
  return (det < 0 ? -1.0 : 1.0) / (P[8] * P[8] + P[9] * P[9] + P[10] * P[10]);
}

}  // namespace
}  // namespace spv
