// The per-sample rule of plane-sweep stereo (depth.hip), written so that it also compiles for the host
// (tests/native/depth_check.cpp) and so that NumPy reproduces it operation for operation (tests/depth_reference.py).
// include/sfm_amd.h states the whole stage; this header holds the three pieces that touch floating point, all float64
// without FMA contraction, and the integer cost.
//
// Sample: reference pixel (x, y), plane depth d, warp W = [A | b] (row-major 3 x 4) into a source of ws x hs pixels:
//   a_i = (A_i0 * x + A_i1 * y) + A_i2      q_i = d * a_i + b_i      u = q0 / q2      v = q1 / q2
//   valid = q2 > 0 && u >= -0.5 && u < ws - 0.5 && v >= -0.5 && v < hs - 0.5          (every comparison false on NaN)
//   xi = min((int)floor(u + 0.5), ws - 1), yi likewise.  The min changes nothing the rule means: u + 0.5 < ws holds in
//   exact arithmetic, and the rounded sum reaches ws only for ws = 1 (u one ulp under 0.5); it is there so that no
//   input bit pattern makes a kernel read outside an image.
// Cost: popcount(census_r ^ census_s), 0 .. 48; an invalid sample costs DEPTH_ABSENT_COST = 24.
// Sub-plane step from the integer sums S_{best-1}, S_best, S_{best+1} and the depths of the three planes: refine().
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define DEPTH_HD __host__ __device__ __forceinline__
#else
#define DEPTH_HD inline
#endif

// no FMA: every multiply and add below rounds on its own (host builds add -ffp-contract=off)
#pragma clang fp contract(off)

#define DEPTH_ABSENT_COST 24

namespace depth {

struct Sample { int valid, xi, yi; double q2; };

DEPTH_HD Sample sample(const double* W, double x, double y, double d, int ws, int hs) {
  const double a0 = (W[0] * x + W[1] * y) + W[2];
  const double a1 = (W[4] * x + W[5] * y) + W[6];
  const double a2 = (W[8] * x + W[9] * y) + W[10];
  const double q0 = d * a0 + W[3];
  const double q1 = d * a1 + W[7];
  const double q2 = d * a2 + W[11];
  const double u = q0 / q2, v = q1 / q2;
  Sample s;
  s.q2 = q2;
  s.valid = (q2 > 0.0) && (u >= -0.5) && (u < (double)ws - 0.5) && (v >= -0.5) && (v < (double)hs - 0.5);
  s.xi = 0; s.yi = 0;
  if (s.valid) {
    const int xi = (int)floor(u + 0.5), yi = (int)floor(v + 0.5);
    s.xi = xi < ws - 1 ? xi : ws - 1;
    s.yi = yi < hs - 1 ? yi : hs - 1;
  }
  return s;
}

DEPTH_HD int popcount64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}

DEPTH_HD int cost(uint64_t cen_r, uint64_t cen_s) { return popcount64(cen_r ^ cen_s); }

// depth of the winner `best` of n_planes: sm / s0 / sp are S_{best-1}, S_best, S_{best+1} and dm / d0 / dp the depths of
// those planes (sm, sp, dm, dp are not looked at where the plane does not exist)
DEPTH_HD float refine(int best, int n_planes, int sm, int s0, int sp, double dm, double d0, double dp) {
  if (best > 0 && best < n_planes - 1) {
    const int den = sm - 2 * s0 + sp;
    if (den > 0) {
      const double off = (double)(sm - sp) / (double)(2 * den);
      const double dj = off >= 0.0 ? dp : dm;
      const double f = fabs(off);
      const double w0 = 1.0 / d0;
      const double w = w0 + f * (1.0 / dj - w0);
      return (float)(1.0 / w);
    }
  }
  return (float)d0;
}

// the filter's agreement of a sample with the source's own depth ds (float32 widened): false on NaN / inf
DEPTH_HD int agrees(double ds, double q2, double rel_tol) {
  return (ds - ds == 0.0) && (fabs(ds - q2) <= rel_tol * q2);
}

// one coordinate of the back-projection: d * ((M_i0 * x + M_i1 * y) + M_i2) + c_i with the row (M_i0, M_i1, M_i2, c_i)
DEPTH_HD double backproject(const double* row, double x, double y, double d) {
  return d * ((row[0] * x + row[1] * y) + row[2]) + row[3];
}

}  // namespace depth
