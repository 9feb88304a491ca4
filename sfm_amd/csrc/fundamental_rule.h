// The error rule of the fundamental- and essential-matrix RANSAC (twoview.hip, essential.hip), written so that it also
// compiles for the host (tests/native/fundamental_solve_check.cpp); epipolar_rule.h brings it to the kernels.
#pragma once
#include "ransac_common.h"

// the error rule without its divisions: max(s^2/den2, s^2/den1) <= thr2  <=>  s^2 <= thr2 * min(den1, den2), with
// min > 0 required so that a zero line (or F = 0, the empty candidate slot) never counts.  NaN fails every test.
SFM_HD bool fund_inlier(const double (&f)[9], double x1, double y1, double x2, double y2, double thr2) {
  const double a = f[0] * x1 + f[1] * y1 + f[2], b = f[3] * x1 + f[4] * y1 + f[5], c = f[6] * x1 + f[7] * y1 + f[8];
  const double s = x2 * a + y2 * b + c;
  const double ta = f[0] * x2 + f[3] * y2 + f[6], tb = f[1] * x2 + f[4] * y2 + f[7];
  const double den = fmin(a * a + b * b, ta * ta + tb * tb);
  return (den > 0.0) && (s * s <= thr2 * den);
}
