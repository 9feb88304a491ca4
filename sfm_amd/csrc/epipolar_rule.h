// The error rule of the two-view RANSAC stages and the staging of a segment's matches for their scoring loops, shared by
// twoview.hip (fundamental matrix) and essential.hip (essential matrix), so that both count an inlier alike, bit for bit.
// Included by .hip files only.
#pragma once
#include "ransac_kernels.h"

constexpr int FUND_CHUNK = 512;      // points per LDS stage of the scoring loop: 512 x 4 doubles = 16 KiB

// the error rule without its divisions: max(s^2/den2, s^2/den1) <= thr2  <=>  s^2 <= thr2 * min(den1, den2), with
// min > 0 required so that a zero line (or F = 0, the empty candidate slot) never counts.  NaN fails every test.
__device__ __forceinline__ bool fund_inlier(const double (&f)[9], double x1, double y1, double x2, double y2, double thr2) {
  const double a = f[0] * x1 + f[1] * y1 + f[2], b = f[3] * x1 + f[4] * y1 + f[5], c = f[6] * x1 + f[7] * y1 + f[8];
  const double s = x2 * a + y2 * b + c;
  const double ta = f[0] * x2 + f[3] * y2 + f[6], tb = f[1] * x2 + f[4] * y2 + f[7];
  const double den = fmin(a * a + b * b, ta * ta + tb * tb);
  return (den > 0.0) && (s * s <= thr2 * den);
}

// stage points [c0, c0 + cnt) of a segment into LDS as doubles; a non-finite match becomes NaN in all four
__device__ __forceinline__ void stage_points(double2* s_pt, const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                             int64_t base, int cnt, int nthreads) {
  for (int t = threadIdx.x; t < cnt; t += nthreads) {
    const float2 p = pts1[base + t], q = pts2[base + t];
    const bool ok = finite4(p, q);
    const double nan = __builtin_nan("");
    s_pt[2 * t] = ok ? make_double2((double)p.x, (double)p.y) : make_double2(nan, nan);
    s_pt[2 * t + 1] = ok ? make_double2((double)q.x, (double)q.y) : make_double2(nan, nan);
  }
}
