// rectify_device.h -- the per-sample arithmetic of epipolar rectification, stated once for rectify.hip (one pair per
// launch) and rectify_batch.hip (many pairs per launch), so that both give the same bits.
//
// The contract is include/spectavi_amd.h's (image_pair_rectification): IEEE double, every operation rounded on its
// own (the files are compiled with -ffp-contract=off), sums left to right as written, correctly rounded division.
// A sample is valid iff x > -1 && x < wid && y > -1 && y < hgt (false for NaN), and only then converted to int, so
// no out-of-range value reaches v_cvt_i32_f64 (which saturates where the reference's cvttsd2si gives INT_MIN).
#pragma once

#include <hip/hip_runtime.h>

namespace spv {

// The epipolar line of output row value v = row - extra_rows in image `img`, F row-major:
//   image 0: l_j = (F[0][j]*0. + F[1][j]*v) + F[2][j];
//   image 1: m = F (sx, sy, 1), (sx, sy) being sample 0 of the same row of image 0.
__device__ __forceinline__ void rectify_line(const double *F, double delta, double v, int img, double &L0, double &L1,
                                             double &L2) {
  L0 = (F[0] * 0. + F[3] * v) + F[6];
  L1 = (F[1] * 0. + F[4] * v) + F[7];
  L2 = (F[2] * 0. + F[5] * v) + F[8];
  if (img) {
    const double sx = 0. + 0. * delta;
    const double sy = ((-L2) - (L0 * sx)) / L1;
    const double m0 = (F[0] * sx + F[1] * sy) + F[2];
    const double m1 = (F[3] * sx + F[4] * sy) + F[5];
    const double m2 = (F[6] * sx + F[7] * sy) + F[8];
    L0 = m0;
    L1 = m1;
    L2 = m2;
  }
}

// Sample i of a line: the flat index (int)y * wid + (int)x of its pixel, or -1 where the sample is not valid.
__device__ __forceinline__ int rectify_sample(double L0, double L1, double L2, double delta, int i, int wid, int hgt) {
  const double x = 0. + (double)i * delta;
  const double y = ((-L2) - (L0 * x)) / L1;
  if (x > -1. && x < (double)wid && y > -1. && y < (double)hgt) return (int)y * wid + (int)x;
  return -1;
}

}  // namespace spv
