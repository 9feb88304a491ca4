// The minimal solver of the homography RANSAC (homography.hip): four matches -> H, written so that it also compiles
// for the host (tests/native/homography_solve_check.cpp) and restated in NumPy by tests/homography_reference.py.
//
// Sample rule, on the float32 pixels widened to double.  For each of the triples (i, j, k) = (0,1,2), (0,1,3), (0,2,3),
// (1,2,3) and each image:  a = (xj - xi)(yk - yi) - (yj - yi)(xk - xi),  d1 = |pj - pi|^2,  d2 = |pk - pi|^2.  The
// sample gives no model unless a^2 > 1e-6 d1 d2 in both images (a triple on a line, or two matches on one pixel), and
// no model if the triple turns one way in image 1 and the other way in image 2 ((a1 > 0) != (a2 > 0)): no homography
// that keeps the four points in front of the camera reverses an orientation.  The same idea as the subset check of
// OpenCV's findHomography, as recalled.  A non-finite coordinate fails the first comparison.
//
// Solve, on the segment's Hartley-normalised coordinates (t = {sc1, cx1, cy1, sc2, cx2, cy2}, x' = sc (x - c)): the
// 8 x 9 system with the rows [x, y, 1, 0, 0, 0, -u x, -u y, -u] and [0, 0, 0, x, y, 1, -v x, -v y, -v] per match
// (x, y) -> (u, v).  Its null vector without pivoting, as fundamental_solve.h finds its two: Givens rotations of column
// pairs from the right, A G = [L 0] with L lower triangular, one row at a time (row i: apply the rotations so far, then
// zero its entries i+1..8), so only the 36 (c, s) pairs are live and every array index is a compile-time constant
// after unrolling (rot_index, ransac_common.h, numbers them).  The last column of G = G_1 ... G_36 is the null vector
// Hn;  H = T2^-1 Hn T1.  A non-finite H is no model.
#pragma once
#include "ransac_common.h"

namespace homog {

// one triple of the sample rule; px[m] = (x, y, u, v) of match m
SFM_HD bool triple_ok(const float (&px)[4][4], int i, int j, int k) {
  bool ok = true, pos[2];
#pragma unroll
  for (int im = 0; im < 2; ++im) {
    const double xi = (double)px[i][2 * im], yi = (double)px[i][2 * im + 1];
    const double ax = (double)px[j][2 * im] - xi, ay = (double)px[j][2 * im + 1] - yi;
    const double bx = (double)px[k][2 * im] - xi, by = (double)px[k][2 * im + 1] - yi;
    const double a = ax * by - ay * bx, d1 = ax * ax + ay * ay, d2 = bx * bx + by * by;
    ok = ok && (a * a > 1e-6 * d1 * d2);                   // NaN or infinity: false
    pos[im] = a > 0.0;
  }
  return ok && pos[0] == pos[1];
}

SFM_HD bool sample_ok(const float (&px)[4][4]) {
  bool fin = true;
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) fin = fin && std::isfinite(px[m][e]);
  return fin && triple_ok(px, 0, 1, 2) && triple_ok(px, 0, 1, 3) && triple_ok(px, 0, 2, 3) && triple_ok(px, 1, 2, 3);
}

// H = T2^-1 Hn T1 with T = [sc 0 -sc*cx; 0 sc -sc*cy; 0 0 1], T^-1 = [1/sc 0 cx; 0 1/sc cy; 0 0 1]
SFM_HD void denormalise(const double (&hn)[9], const double* t, double (&h)[9]) {
  const double s1 = t[0], tx1 = -t[0] * t[1], ty1 = -t[0] * t[2];
  const double i2 = 1.0 / t[3], cx2 = t[4], cy2 = t[5];
  double g[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    g[3 * r] = s1 * hn[3 * r];
    g[3 * r + 1] = s1 * hn[3 * r + 1];
    g[3 * r + 2] = (hn[3 * r] * tx1 + hn[3 * r + 1] * ty1) + hn[3 * r + 2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    h[c] = i2 * g[c] + cx2 * g[6 + c];
    h[3 + c] = i2 * g[3 + c] + cy2 * g[6 + c];
    h[6 + c] = g[6 + c];
  }
}

// the null vector of the 8 x 9 system of the four normalised matches x[m] = (x, y, u, v); false if a pivot is not a number
SFM_HD bool null_vector(const double (&x)[4][4], double (&hn)[9]) {
  bool ok = true;
  double rc[36], rs[36];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const double xa = x[i / 2][0], xb = x[i / 2][1], w = x[i / 2][2 + (i & 1)];
    double r[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) r[e] = 0.0;
    r[3 * (i & 1)] = xa; r[3 * (i & 1) + 1] = xb; r[3 * (i & 1) + 2] = 1.0;
    r[6] = -w * xa; r[7] = -w * xb; r[8] = -w;
#pragma unroll
    for (int ii = 0; ii < i; ++ii)
#pragma unroll
      for (int j = ii + 1; j < 9; ++j) {
        const double c = rc[rot_index(ii, j)], sn = rs[rot_index(ii, j)];
        const double u = r[ii], v = r[j];
        r[ii] = c * u + sn * v; r[j] = c * v - sn * u;
      }
#pragma unroll
    for (int j = i + 1; j < 9; ++j) {
      const double u = r[i], v = r[j];
      const double hh = sqrt(u * u + v * v);
      const bool nz = hh > 0.0;                            // NaN: (1, 0), and the NaN travels on in r
      const double c = nz ? u / hh : 1.0, sn = nz ? v / hh : 0.0;
      rc[rot_index(i, j)] = c; rs[rot_index(i, j)] = sn;
      r[i] = nz ? hh : u; r[j] = nz ? 0.0 : v;
    }
    ok = ok && (r[i] == r[i]);
  }
  // G e8: the rotations applied in reverse order to the unit vector
#pragma unroll
  for (int e = 0; e < 9; ++e) hn[e] = (e == 8) ? 1.0 : 0.0;
#pragma unroll
  for (int i = 7; i >= 0; --i)
#pragma unroll
    for (int j = 8; j > i; --j) {
      const double c = rc[rot_index(i, j)], sn = rs[rot_index(i, j)];
      const double u = hn[i], v = hn[j];
      hn[i] = c * u - sn * v; hn[j] = sn * u + c * v;
    }
  return ok;
}

// px[m] = (x, y, u, v) of the four matches as float32 pixels, t the segment's transforms.  True and H (not scaled), or
// false: the sample gives no model.
SFM_HD bool solve_sample(const float (&px)[4][4], const double* t, double (&h)[9]) {
  if (!sample_ok(px)) return false;
  double x[4][4];
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    x[m][0] = ((double)px[m][0] - t[1]) * t[0]; x[m][1] = ((double)px[m][1] - t[2]) * t[0];
    x[m][2] = ((double)px[m][2] - t[4]) * t[3]; x[m][3] = ((double)px[m][3] - t[5]) * t[3];
  }
  double hn[9];
  bool ok = null_vector(x, hn);
  denormalise(hn, t, h);
#pragma unroll
  for (int e = 0; e < 9; ++e) ok = ok && std::isfinite(h[e]);
  return ok;
}

}  // namespace homog
