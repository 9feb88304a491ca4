// The epipolar gate of guided matching (guided.hip), written so that it also compiles for the host
// (tests/native/guided_check.cpp) and so that NumPy reproduces it operation for operation (tests/guided_reference.py).
//
// For a point (x1, y1) of image i and a point (x2, y2) of image j, float32 pixels widened to double, and the row-major F of
// the pair (x2^T F x1 = 0):
//   a  = (f0*x1 + f1*y1) + f2      b  = (f3*x1 + f4*y1) + f5      c = (f6*x1 + f7*y1) + f8       F x1: the line in image j
//   ta = (f0*x2 + f3*y2) + f6      tb = (f1*x2 + f4*y2) + f7                                     F^T x2: the line in image i
//   s  = (x2*a + y2*b) + c
//   den = fmin(a*a + b*b, ta*ta + tb*tb)
//   gate = den > 0  &&  s*s <= (thr*thr) * den
// i.e. the larger of the two squared point-line distances is at most thr^2 - the rule of epipolar_rule.h with its
// association written out and without FMA contraction (that header compiles with contraction and stays as it is: its bits
// are those of existing outputs).  A NaN anywhere fails the gate, and so does F = 0 (den = 0).  An infinite coordinate on
// ONE side fails it (s*s is infinite or NaN against a finite right side); the rule is not asked about two infinite points.
//
// Image i's point is always in the first slot, whichever side is the query: the reverse pass of the cross-check sees the
// very same truth value for every (q, t).  The halves that depend on one point only - (a, b, c, a*a + b*b) and
// (x2, y2, ta*ta + tb*tb) - may be formed once per point: without contraction the values are the same.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GUIDED_HD __host__ __device__ __forceinline__
#else
#define GUIDED_HD inline
#endif

// no FMA: every multiply and add below rounds on its own (host builds add -ffp-contract=off)
#pragma clang fp contract(off)

namespace guided {

struct Side1 { double a, b, c, den; };      // image i's point under F: the line (a, b, c) in image j and a*a + b*b
struct Side2 { double x, y, den; };         // image j's point and ta*ta + tb*tb of its line in image i

GUIDED_HD Side1 side1(const double* f, float x1f, float y1f) {
  const double x1 = (double)x1f, y1 = (double)y1f;
  Side1 p;
  p.a = (f[0] * x1 + f[1] * y1) + f[2];
  p.b = (f[3] * x1 + f[4] * y1) + f[5];
  p.c = (f[6] * x1 + f[7] * y1) + f[8];
  p.den = p.a * p.a + p.b * p.b;
  return p;
}

GUIDED_HD Side2 side2(const double* f, float x2f, float y2f) {
  const double x2 = (double)x2f, y2 = (double)y2f;
  const double ta = (f[0] * x2 + f[3] * y2) + f[6];
  const double tb = (f[1] * x2 + f[4] * y2) + f[7];
  Side2 p;
  p.x = x2; p.y = y2;
  p.den = ta * ta + tb * tb;
  return p;
}

GUIDED_HD bool gate(double a, double b, double c, double den1, double x2, double y2, double den2, double thr2) {
  const double s = (x2 * a + y2 * b) + c;
  const double den = fmin(den1, den2);
  return (den > 0.0) && (s * s <= thr2 * den);
}

GUIDED_HD bool gate(const double* f, float x1, float y1, float x2, float y2, double thr) {
  const Side1 p = side1(f, x1, y1);
  const Side2 q = side2(f, x2, y2);
  return gate(p.a, p.b, p.c, p.den, q.x, q.y, q.den, thr * thr);
}

}  // namespace guided
