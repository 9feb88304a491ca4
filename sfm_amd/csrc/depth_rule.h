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

// ---- fusion (depth_fuse.hip; include/sfm_amd.h, "fusion of the depth maps"; tests/depth_fuse_reference.py) ----
// whether a number is finite: false on NaN and on +-inf
DEPTH_HD int is_finite(double v) { return v - v == 0.0; }

// the neighbour depth dn belongs to the surface of the centre depth d: finite and within jump * d of it
DEPTH_HD int near_depth(double dn, double d, double jump) { return is_finite(dn) && (fabs(dn - d) <= jump * d); }

// n = (xp - xm) x (yp - ym) of four points, every product and difference rounded on its own
DEPTH_HD void cross_of_differences(const double* xp, const double* xm, const double* yp, const double* ym, double* n) {
  const double a0 = xp[0] - xm[0], a1 = xp[1] - xm[1], a2 = xp[2] - xm[2];
  const double b0 = yp[0] - ym[0], b1 = yp[1] - ym[1], b2 = yp[2] - ym[2];
  n[0] = a1 * b2 - a2 * b1;
  n[1] = a2 * b0 - a0 * b2;
  n[2] = a0 * b1 - a1 * b0;
}

DEPTH_HD double norm2(const double* n) { return (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]; }

// n / sqrt(l2) in place when l2 is finite and > 0 (returns 1); otherwise n = 0 (returns 0)
DEPTH_HD int normalise(double* n, double l2) {
  if (!(is_finite(l2) && l2 > 0.0)) { n[0] = 0.0; n[1] = 0.0; n[2] = 0.0; return 0; }
  const double l = sqrt(l2);
  n[0] = n[0] / l; n[1] = n[1] / l; n[2] = n[2] / l;
  return 1;
}

// turn n towards the camera centre C seen from the point X
DEPTH_HD void orient(double* n, const double* C, const double* X) {
  const double c0 = C[0] - X[0], c1 = C[1] - X[1], c2 = C[2] - X[2];
  if (((n[0] * c0 + n[1] * c1) + n[2] * c2) < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
}

// the normal of a pixel of a view's map: d the centre depth and X its point, dn[4] the depths of the neighbours in the
// order (x+t, x-t, y+t, y-t) and xp / xm / yp / ym their points, C the view's centre.  out = (0, 0, 0) when the normal is
// not valid.
DEPTH_HD int view_normal(double d, const double* X, const double* dn, const double* xp, const double* xm, const double* yp,
                         const double* ym, const double* C, double jump, float* out) {
  double n[3] = {0.0, 0.0, 0.0};
  int valid = is_finite(d);
  for (int k = 0; k < 4; ++k) valid = valid && near_depth(dn[k], d, jump);
  if (valid) {
    cross_of_differences(xp, xm, yp, ym, n);
    valid = normalise(n, norm2(n));
    if (valid) orient(n, C, X);
  }
  out[0] = (float)n[0]; out[1] = (float)n[1]; out[2] = (float)n[2];
  return valid;
}

// one coordinate of the fused point: the sum of the agreeing views' coordinates over their number
DEPTH_HD double fused_mean(double acc, int n_views) { return acc / (double)n_views; }

// the fused normal from the sum of the views' float32 normals: unit length, or zeros when the sum has no length
DEPTH_HD void fused_normal(const double* acc, float* out) {
  double n[3] = {acc[0], acc[1], acc[2]};
  normalise(n, norm2(n));
  out[0] = (float)n[0]; out[1] = (float)n[1]; out[2] = (float)n[2];
}

}  // namespace depth
