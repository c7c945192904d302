// rectify.hip -- epipolar-line rectification of an image pair for gfx950 (MI355X).
//
// The GPU form of the reference's image_pair_rectification (reference src/Spectavi.cpp:89-119 over
// the Rectifier of src/Camera.h:61-445), with the contract stated in include/spectavi_amd.h.  Output
// row r (v = r - extra_rows) resamples image 0 along the epipolar line l = F^T (0, v, 1) at the
// rnx abscissae x_i = 0 + i * delta, and image 1 along m = F (x_0, y_0, 1), the line of the first
// image-0 sample of the same row.  Every sample is one truncation to a pixel and one copy of its
// nchan values, so the kernel is a store stream: 12 bytes per gray fp64 sample and image leave, the
// gathered pixels come from L2 (lines are near-horizontal for a real stereo pair, so neighbouring
// lanes read neighbouring pixels).
//
//   * one block of 256 lanes owns 256 consecutive output columns of one row of one image and
//     recomputes that row's line from F (a kernel argument); every output element -- the padding
//     columns [rnx, output_cols) included -- is written exactly once, so no memset precedes it;
//   * the arithmetic is IEEE double with every operation rounded on its own (-ffp-contract=off) and
//     correctly rounded division, in the order the header states; a sample is valid iff
//     x > -1 && x < wid && y > -1 && y < hgt (false for NaN), and only then converted to int, so no
//     out-of-range value reaches v_cvt_i32_f64 (which saturates where the reference's cvttsd2si
//     gives INT_MIN);
//   * values are copied as integers of their width (fp64 as uint64), so NaN payloads and -0.0 pass
//     through unchanged.

#include "common.h"
#include "rectify_device.h"

#include <climits>
#include <cmath>

namespace spv {
namespace {

constexpr int kThreads = 256;

struct RectifyArgs {
  double F[9];  // row-major
  double delta;  // (wid - 1) / (rnx - 1): inf or NaN when rnx = 1
  int wid, hgt, nchan, rnx, cols, rows, extra;
  int col_blocks;  // ceil(cols / kThreads)
};

// T: uint64_t for float64 images (bit copies), uint8_t for 8-bit ones.
template <typename T>
__global__ __launch_bounds__(kThreads) void rectify_kernel(RectifyArgs a, const T *__restrict__ im0,
                                                          const T *__restrict__ im1, T *__restrict__ r0,
                                                          T *__restrict__ r1, int *__restrict__ ri0,
                                                          int *__restrict__ ri1) {
  const long long per_image = (long long)a.rows * a.col_blocks;
  const long long nblocks = 2 * per_image;
  for (long long b = blockIdx.x; b < nblocks; b += gridDim.x) {
    const int img = b >= per_image ? 1 : 0;
    const long long rb = b - img * per_image;
    const int row = (int)(rb / a.col_blocks);
    const int i = (int)(rb - (long long)row * a.col_blocks) * kThreads + (int)threadIdx.x;
    if (i >= a.cols) continue;
    double L0, L1, L2;  // the row's line in this image (rectify_device.h)
    rectify_line(a.F, a.delta, (double)(row - a.extra), img, L0, L1, L2);
    const T *im = img ? im1 : im0;
    T *out = img ? r1 : r0;
    int *outi = img ? ri1 : ri0;
    const size_t o = (size_t)row * a.cols + i;
    const int idx = i < a.rnx ? rectify_sample(L0, L1, L2, a.delta, i, a.wid, a.hgt) : -1;
    outi[o] = idx;
    if (idx >= 0) {
      const T *src = im + (size_t)idx * a.nchan;
      for (int c = 0; c < a.nchan; ++c) out[o * a.nchan + c] = src[c];
    } else {
      for (int c = 0; c < a.nchan; ++c) out[o * a.nchan + c] = T(0);
    }
  }
}

}  // namespace

int rectify_shape(int wid, int hgt, int nchan, double sf, int out[3]) {
  if (!(std::isfinite(sf) && sf > 0.)) return set_error(SPV_ERR_INVALID, "sampling_factor must be finite and > 0");
  if (wid < 1 || hgt < 1 || nchan < 1)
    return set_error(SPV_ERR_INVALID, "bad image shape (wid=%d, hgt=%d, nchan=%d)", wid, hgt, nchan);
  if ((long long)hgt * wid > INT_MAX)
    return set_error(SPV_ERR_INVALID, "hgt*wid=%lld does not fit the int32 index output", (long long)hgt * wid);
  const long long C = (long long)wid * nchan;
  if (C > INT_MAX) return set_error(SPV_ERR_INVALID, "wid*nchan=%lld > INT_MAX", C);
  // the reference's expressions, evaluated in double and truncated where they are assigned to an int
  const double cols_d = sf * (double)C / (double)nchan;
  const double rnx_d = sf * (double)wid;
  if (!(cols_d < 2147483648.0 && rnx_d < 2147483648.0))
    return set_error(SPV_ERR_INVALID, "sampling_factor=%g: output width exceeds INT_MAX", sf);
  const int cols = (int)cols_d, rnx = (int)rnx_d;
  const int extra = (int)((double)std::max<long long>(hgt, C) / 2.);
  const long long rows = (long long)hgt + 2LL * extra;
  if (rows > INT_MAX) return set_error(SPV_ERR_INVALID, "output rows %lld > INT_MAX", rows);
  if (rnx < 1 || cols < 1)
    return set_error(SPV_ERR_INVALID, "sampling_factor=%g leaves %d samples per line and %d output columns (need >= 1)",
                     sf, rnx, cols);
  out[0] = (int)rows;
  out[1] = cols;
  out[2] = rnx;
  return SPV_OK;
}

// F = [P1 C]x P1 P0^T (P0 P0^T)^-1 with C the unit null vector of P0 (its cofactor vector, scaled).
// Singular P0 P0^T (|det| at most 2^-40 of its Hadamard bound) or a non-finite F gives an all-NaN F;
// cameras whose centres coincide (|P1 C| at most 2^-40 |P1|_F; identical cameras included) give F = 0.
// Either way every sample is invalid.
void rectify_fundamental(const double *P0, const double *P1, double *F) {
  auto p0 = [&](int r, int c) { return P0[r * 4 + c]; };
  auto det3 = [](const double m[9]) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) +
           m[2] * (m[3] * m[7] - m[4] * m[6]);
  };
  // null vector: C_k = (-1)^k det(P0 without column k)
  double C[4], norm = 0.;
  for (int k = 0; k < 4; ++k) {
    double m[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0, cc = 0; c < 4; ++c)
        if (c != k) m[r * 3 + cc++] = p0(r, c);
    C[k] = (k & 1 ? -1. : 1.) * det3(m);
    norm += C[k] * C[k];
  }
  norm = std::sqrt(norm);
  // M = P0 P0^T and its inverse through the adjugate
  double M[9], Mi[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      double s = 0.;
      for (int k = 0; k < 4; ++k) s += p0(r, k) * p0(c, k);
      M[r * 3 + c] = s;
    }
  const double det = det3(M);
  double hadamard = 1.;
  for (int r = 0; r < 3; ++r)
    hadamard *= std::sqrt(M[r * 3] * M[r * 3] + M[r * 3 + 1] * M[r * 3 + 1] + M[r * 3 + 2] * M[r * 3 + 2]);
  bool ok = std::fabs(det) > std::ldexp(hadamard, -40) && norm > 0.;
  if (ok) {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
        // cofactor of M[c][r] (adjugate = transposed cofactors)
        Mi[r * 3 + c] = (M[c1 * 3 + r1] * M[c2 * 3 + r2] - M[c1 * 3 + r2] * M[c2 * 3 + r1]) / det;
      }
    // the epipole P1 C; below 2^-40 of |P1| the centres coincide to working precision: F = 0
    double e[3], en = 0., p1n = 0.;
    for (int r = 0; r < 3; ++r) {
      double s = 0.;
      for (int k = 0; k < 4; ++k) {
        s += P1[r * 4 + k] * (C[k] / norm);
        p1n += P1[r * 4 + k] * P1[r * 4 + k];
      }
      e[r] = s;
      en += s * s;
    }
    if (!(std::sqrt(en) > std::ldexp(std::sqrt(p1n), -40))) e[0] = e[1] = e[2] = 0.;
    // A = P1 P0^T Mi (3x3), F = [e]x A
    double B[12], A[9];  // B = P0^T Mi (4x3)
    for (int k = 0; k < 4; ++k)
      for (int c = 0; c < 3; ++c) B[k * 3 + c] = p0(0, k) * Mi[c] + p0(1, k) * Mi[3 + c] + p0(2, k) * Mi[6 + c];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        double s = 0.;
        for (int k = 0; k < 4; ++k) s += P1[r * 4 + k] * B[k * 3 + c];
        A[r * 3 + c] = s;
      }
    const double S[9] = {0., -e[2], e[1], e[2], 0., -e[0], -e[1], e[0], 0.};
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) F[r * 3 + c] = S[r * 3] * A[c] + S[r * 3 + 1] * A[3 + c] + S[r * 3 + 2] * A[6 + c];
    for (int j = 0; j < 9; ++j) ok = ok && std::isfinite(F[j]);
  }
  if (!ok)
    for (int j = 0; j < 9; ++j) F[j] = std::nan("");
}

int rectify_run(const double *F, const void *d_im0, const void *d_im1, int dtype, int wid, int hgt, int nchan,
                double sf, void *d_r0, void *d_r1, int32_t *d_ri0, int32_t *d_ri1, hipStream_t stream) {
  if (!F) return set_error(SPV_ERR_INVALID, "null F");
  if (dtype != SPV_RECTIFY_F64 && dtype != SPV_RECTIFY_U8) return set_error(SPV_ERR_INVALID, "dtype %d", dtype);
  int shape[3];
  SPV_TRY(rectify_shape(wid, hgt, nchan, sf, shape));
  if (!d_im0 || !d_im1 || !d_r0 || !d_r1 || !d_ri0 || !d_ri1) return set_error(SPV_ERR_INVALID, "null device pointer");
  const uintptr_t align = dtype == SPV_RECTIFY_F64 ? 7 : 0;
  if (((reinterpret_cast<uintptr_t>(d_im0) | reinterpret_cast<uintptr_t>(d_im1) | reinterpret_cast<uintptr_t>(d_r0) |
        reinterpret_cast<uintptr_t>(d_r1)) & align) ||
      ((reinterpret_cast<uintptr_t>(d_ri0) | reinterpret_cast<uintptr_t>(d_ri1)) & 3))
    return set_error(SPV_ERR_INVALID, "misaligned image or output pointer");
  RectifyArgs a;
  for (int j = 0; j < 9; ++j) a.F[j] = F[j];
  a.delta = ((double)(wid - 1) - 0.) / (double)(shape[2] - 1);
  a.wid = wid;
  a.hgt = hgt;
  a.nchan = nchan;
  a.rows = shape[0];
  a.cols = shape[1];
  a.rnx = shape[2];
  a.extra = (shape[0] - hgt) / 2;
  a.col_blocks = (a.cols + kThreads - 1) / kThreads;
  const long long nblocks = 2LL * a.rows * a.col_blocks;
  const unsigned grid = (unsigned)std::min<long long>(nblocks, 1LL << 24);
  {
    ProfScope prof("rectify", stream);
    if (dtype == SPV_RECTIFY_F64)
      hipLaunchKernelGGL((rectify_kernel<uint64_t>), dim3(grid), dim3(kThreads), 0, stream,
                         a, static_cast<const uint64_t *>(d_im0), static_cast<const uint64_t *>(d_im1),
                         static_cast<uint64_t *>(d_r0), static_cast<uint64_t *>(d_r1), d_ri0, d_ri1);
    else
      hipLaunchKernelGGL((rectify_kernel<uint8_t>), dim3(grid), dim3(kThreads), 0, stream,
                         a, static_cast<const uint8_t *>(d_im0), static_cast<const uint8_t *>(d_im1),
                         static_cast<uint8_t *>(d_r0), static_cast<uint8_t *>(d_r1), d_ri0, d_ri1);
  }
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

}  // namespace spv
