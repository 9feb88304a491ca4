// The minimal solver of the fundamental-matrix RANSAC (twoview.hip): seven matches -> up to three F, written so that it
// also compiles for the host (tests/native/fundamental_solve_check.cpp) and restated in NumPy by
// tests/fundamental_reference.py.
//
// On the segment's Hartley-normalised coordinates (t = {sc1, cx1, cy1, sc2, cx2, cy2}, x' = sc (x - c)): the 7 x 9
// system with the row [u x, u y, u, v x, v y, v, x, y, 1] per match (x, y) -> (u, v).  Null space without pivoting:
// Givens rotations of column pairs from the right, A G = [L 0] with L lower triangular, one row at a time (row i: apply
// the rotations so far, then zero its entries i+1..8), so only the 35 (c, s) pairs are live and every array index is a
// compile-time constant after unrolling (rot_index, ransac_common.h): nothing goes to scratch.  The last two columns of
// G, f1 and f2, span the null space; det(l f1 + (1 - l) f2) is a cubic in l.  No model if one of its coefficients is
// not finite or the leading one is below 1e-14 of the largest.  Its real roots x_k in closed form (three ascending, or
// one), two Newton steps each; candidate k is F = T2^T (x_k f1 + (1 - x_k) f2) T1, not scaled.  A slot without a root
// or with a non-finite F holds F = 0, which the error rule never counts, and so do all three of a sample with a
// non-finite coordinate: a rotation whose length is NaN takes the NaN into c, s and the pivot, which is tested, and an
// infinite one leaves c or s NaN, so that f1, f2 and the cubic are NaN.  Where a sum of two products could be
// contracted either way the fma is written out: which product the compiler fuses depends on where its passes meet the
// expression, and these roundings decide the counts of ill-conditioned samples.
#pragma once
#include "ransac_common.h"

namespace sevenpt {

SFM_HD double det3(double a0, double a1, double a2, double a3, double a4, double a5, double a6, double a7, double a8) {
  return a0 * (a4 * a8 - a5 * a7) - a1 * (a3 * a8 - a5 * a6) + a2 * (a3 * a7 - a4 * a6);
}

// F = T2^T Fn T1 with T = [sc 0 -sc*cx; 0 sc -sc*cy; 0 0 1]
SFM_HD void denormalise(const double (&fn)[9], const double* t, double (&f)[9]) {
  const double s1 = t[0], tx1 = -t[0] * t[1], ty1 = -t[0] * t[2];
  const double s2 = t[3], tx2 = -t[3] * t[4], ty2 = -t[3] * t[5];
  double g[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    g[3 * r] = s1 * fn[3 * r];
    g[3 * r + 1] = s1 * fn[3 * r + 1];
    g[3 * r + 2] = fn[3 * r] * tx1 + fn[3 * r + 1] * ty1 + fn[3 * r + 2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f[c] = s2 * g[c];
    f[3 + c] = s2 * g[3 + c];
    f[6 + c] = tx2 * g[c] + ty2 * g[3 + c] + g[6 + c];
  }
}

// match(i, ok, m) writes match i of the sample as m = (x, y, u, v), float32 pixels, or returns false: no model.  It is
// asked once per row of the elimination, so a kernel fetches the matches as it goes and holds one at a time; ok is
// false once the sample is known to give no model.  t: the segment's transforms.  Fc[k] is candidate k, or zero.
template <typename Match>
SFM_HD void solve_matches(Match match, const double* t, double (&Fc)[3][9]) {
  bool ok = true;
  double rc[35], rs[35];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    float m[4];
    const bool have = match(i, ok, m);
    const double xa = ((double)m[0] - t[1]) * t[0], xb = ((double)m[1] - t[2]) * t[0];
    const double xc = ((double)m[2] - t[4]) * t[3], xd = ((double)m[3] - t[5]) * t[3];
    double r[9] = {xc * xa, xc * xb, xc, xd * xa, xd * xb, xd, xa, xb, 1.0};
#pragma unroll
    for (int ii = 0; ii < i; ++ii)
#pragma unroll
      for (int j = ii + 1; j < 9; ++j) {
        const double c = rc[rot_index(ii, j)], sn = rs[rot_index(ii, j)];
        const double u = r[ii], v = r[j];
        r[ii] = fma(c, u, sn * v); r[j] = fma(c, v, -(sn * u));
      }
#pragma unroll
    for (int j = i + 1; j < 9; ++j) {
      const double u = r[i], v = r[j];
      const double hh = sqrt(fma(u, u, v * v));
      const bool nz = !(hh <= 0.0);                      // NaN counts as non-zero: it goes into c, s and the pivot
      const double c = nz ? u / hh : 1.0, sn = nz ? v / hh : 0.0;
      rc[rot_index(i, j)] = c; rs[rot_index(i, j)] = sn;
      r[i] = nz ? hh : u; r[j] = nz ? 0.0 : v;
    }
    ok = ok && have && (r[i] == r[i]);
  }
  // null vectors G e7, G e8: the rotations applied in reverse order to the unit vectors
  double f1[9], f2[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) { f1[e] = (e == 7) ? 1.0 : 0.0; f2[e] = (e == 8) ? 1.0 : 0.0; }
#pragma unroll
  for (int i = 6; i >= 0; --i)
#pragma unroll
    for (int j = 8; j > i; --j) {
      const double c = rc[rot_index(i, j)], sn = rs[rot_index(i, j)];
      double u = f1[i], v = f1[j];
      f1[i] = fma(c, u, -(sn * v)); f1[j] = fma(c, v, sn * u);
      u = f2[i]; v = f2[j];
      f2[i] = fma(c, u, -(sn * v)); f2[j] = fma(c, v, sn * u);
    }
  // det(l f1 + (1 - l) f2) at l = -1, 0, 1, 2 gives the cubic's coefficients
  double pv[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double l = (double)(k - 1);
    double m[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) m[e] = l * f1[e] + (1.0 - l) * f2[e];
    pv[k] = det3(m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8]);
  }
  const double c0 = pv[1];
  const double c3 = (pv[3] - 3.0 * pv[2] + 3.0 * pv[1] - pv[0]) / 6.0;
  const double c2 = 0.5 * (pv[2] + pv[0]) - pv[1];
  const double c1 = pv[2] - c0 - c2 - c3;
  const double cmax = fmax(fmax(fabs(c0), fabs(c1)), fmax(fabs(c2), fabs(c3)));
  ok = ok && std::isfinite(cmax) && (c0 == c0) && (c1 == c1) && (c2 == c2) && (c3 == c3) && !(fabs(c3) < 1e-14 * cmax);
  const double A = c2 / c3, B = c1 / c3, Cc = c0 / c3;
  double root[3];
  int nr = cubic_roots_monic(A, B, Cc, root);
  if (!ok) nr = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double x = cubic_newton2(root[k], A, B, Cc);
    double fn[9], f[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) fn[e] = fma(x, f1[e], (1.0 - x) * f2[e]);
    denormalise(fn, t, f);
    bool good = k < nr;
#pragma unroll
    for (int e = 0; e < 9; ++e) good = good && std::isfinite(f[e]);
#pragma unroll
    for (int e = 0; e < 9; ++e) Fc[k][e] = good ? f[e] : 0.0;
  }
}

}  // namespace sevenpt
