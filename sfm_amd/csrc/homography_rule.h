// The error rule of the homography RANSAC (homography.hip), written so that it also compiles for the host
// (tests/native/homography_solve_check.cpp): the forward transfer error of cv2.findHomography without its division.
//   (X, Y, W) = H (x, y, 1);  inlier iff W != 0 and (X - u W)^2 + (Y - v W)^2 <= thr^2 W^2
// The sums are bracketed as written below, so that the device, the host build and the NumPy restatement
// (tests/homography_reference.py) add in the same order.  NaN anywhere fails the comparison; H = 0, the empty slot,
// gives W = 0 and never counts.
#pragma once
#include "ransac_common.h"

SFM_HD bool hom_inlier(const double (&h)[9], double x, double y, double u, double v, double thr2) {
  const double X = (h[0] * x + h[1] * y) + h[2];
  const double Y = (h[3] * x + h[4] * y) + h[5];
  const double W = (h[6] * x + h[7] * y) + h[8];
  const double dx = X - u * W, dy = Y - v * W;
  return (W != 0.0) && (dx * dx + dy * dy <= thr2 * (W * W));
}
