// Closed-form P3P for pnp.hip, written so that it also compiles for the host (tests/native/pnp_solve_check.cpp).
//
// Three world points P_i seen along unit bearings f_i at depths l_i > 0 obey  l^T M_ij l = a_ij  for the three pairs,
// with a_ij = |P_i - P_j|^2 and M_ij the 3 x 3 form of  l_i^2 + l_j^2 - 2 (f_i . f_j) l_i l_j.  Eliminating the
// constants leaves two homogeneous conics in l,  D1 = a12 M01 - a01 M12  and  D2 = a12 M02 - a02 M12  (the pencil
// Persson & Nordberg's Lambda-Twist works in).  One real root g of the cubic det(D1 + g D2) = 0 makes D0 = D1 + g D2
// a pair of lines; each line meets the other conic in two points, each point fixes l up to scale and one of the
// original equations fixes the scale: up to four depth triples.  Two Newton steps on the three original equations
// polish each triple, and [R|t] maps the world triangle's orthonormal frame onto the frame of the points l_i f_i.
//
// Nothing is indexed at run time: the pivot that splits D0 is brought to variable 0 by a cyclic renaming chosen
// with selects, and every loop is unrolled over constants.
#pragma once
#include "ransac_common.h"

namespace p3p {

struct sym3 { double m00, m11, m22, m01, m02, m12; };          // symmetric 3 x 3

// variable i of the result is variable (i + 1) % 3 of a
SFM_HD sym3 rot(const sym3& a) { return {a.m11, a.m22, a.m00, a.m12, a.m01, a.m02}; }
SFM_HD double sel3(int k, double a, double b, double c) { return k == 0 ? a : (k == 1 ? b : c); }
SFM_HD sym3 rot_by(const sym3& a, int k) {
  const sym3 b = rot(a), c = rot(b);
  return {sel3(k, a.m00, b.m00, c.m00), sel3(k, a.m11, b.m11, c.m11), sel3(k, a.m22, b.m22, c.m22),
          sel3(k, a.m01, b.m01, c.m01), sel3(k, a.m02, b.m02, c.m02), sel3(k, a.m12, b.m12, c.m12)};
}
SFM_HD sym3 axpy(const sym3& a, double g, const sym3& b) {
  return {a.m00 + g * b.m00, a.m11 + g * b.m11, a.m22 + g * b.m22, a.m01 + g * b.m01, a.m02 + g * b.m02, a.m12 + g * b.m12};
}
SFM_HD double det(const sym3& a) {
  return a.m00 * (a.m11 * a.m22 - a.m12 * a.m12) - a.m01 * (a.m01 * a.m22 - a.m12 * a.m02) +
         a.m02 * (a.m01 * a.m12 - a.m11 * a.m02);
}
// sum of the principal 2 x 2 minors over the squared Frobenius norm: the product of the two non-zero eigenvalues of
// a singular matrix, scale-free.  Negative <=> the conic is a pair of real lines; the more negative, the wider apart.
SFM_HD double line_pair_measure(const sym3& a) {
  const double c = (a.m00 * a.m11 - a.m01 * a.m01) + (a.m00 * a.m22 - a.m02 * a.m02) + (a.m11 * a.m22 - a.m12 * a.m12);
  const double fr = a.m00 * a.m00 + a.m11 * a.m11 + a.m22 * a.m22 + 2.0 * (a.m01 * a.m01 + a.m02 * a.m02 + a.m12 * a.m12);
  return c / fr;
}

SFM_HD void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
SFM_HD double dot3(const double (&a)[3], const double (&b)[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// orthonormal frame of the triangle (p0, p1, p2): e1 along p1 - p0, e3 along the normal, e2 = e3 x e1
SFM_HD void frame(const double (&p0)[3], const double (&p1)[3], const double (&p2)[3], double (&e1)[3], double (&e2)[3],
                  double (&e3)[3]) {
  double d1[3], d2[3], n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { d1[k] = p1[k] - p0[k]; d2[k] = p2[k] - p0[k]; }
  cross3(d1, d2, n);
  const double i1 = 1.0 / sqrt(dot3(d1, d1)), i3 = 1.0 / sqrt(dot3(n, n));
#pragma unroll
  for (int k = 0; k < 3; ++k) { e1[k] = d1[k] * i1; e3[k] = n[k] * i3; }
  cross3(e3, e1, e2);
}

// the sample gives no model when its triangle has no area, |d1 x d2|^2 <= 1e-20 |d1|^2 |d2|^2, or holds a
// non-finite coordinate (the comparison then fails)
SFM_HD bool triangle_ok(const double (&P)[3][3]) {
  double d1[3], d2[3], n[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { d1[k] = P[1][k] - P[0][k]; d2[k] = P[2][k] - P[0][k]; }
  cross3(d1, d2, n);
  return dot3(n, n) > 1e-20 * dot3(d1, d1) * dot3(d2, d2);
}

// P [3][3] world points, f [3][3] unit bearings.  Rt [4][12]: row-major [R|t] per candidate slot, all zero for an
// empty slot.  Returns the bit mask of the filled slots.
SFM_HD int solve(const double (&P)[3][3], const double (&f)[3][3], double (&Rt)[4][12]) {
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int e = 0; e < 12; ++e) Rt[c][e] = 0.0;
  bool ok = triangle_ok(P);
  double d01[3], d02[3], d12[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { d01[k] = P[0][k] - P[1][k]; d02[k] = P[0][k] - P[2][k]; d12[k] = P[1][k] - P[2][k]; }
  const double a01 = dot3(d01, d01), a02 = dot3(d02, d02), a12 = dot3(d12, d12);
  const double b01 = dot3(f[0], f[1]), b02 = dot3(f[0], f[2]), b12 = dot3(f[1], f[2]);
  const double amax = fmax(a01, fmax(a02, a12));
  const sym3 D1 = {a12, a12 - a01, -a01, -a12 * b01, 0.0, a01 * b12};
  const sym3 D2 = {a12, -a02, a12 - a02, 0.0, -a12 * b02, a02 * b12};
  // det(D1 + g D2) is a cubic in g: its values at g = -1, 0, 1, 2 give the coefficients
  const double pm = det(axpy(D1, -1.0, D2)), p0 = det(D1), p1 = det(axpy(D1, 1.0, D2)), p2 = det(axpy(D1, 2.0, D2));
  const double c0 = p0;
  const double c3 = (p2 - 3.0 * p1 + 3.0 * p0 - pm) / 6.0;
  const double c2 = 0.5 * (p1 + pm) - p0;
  const double c1 = p1 - c0 - c2 - c3;
  const double cmax = fmax(fmax(fabs(c0), fabs(c1)), fmax(fabs(c2), fabs(c3)));
  ok = ok && std::isfinite(cmax) && (c0 == c0) && (c1 == c1) && (c2 == c2) && (c3 == c3) && !(fabs(c3) < 1e-14 * cmax);
  const double A = c2 / c3, B = c1 / c3, Cc = c0 / c3;
  double root[3];
  const int nr = cubic_roots_monic(A, B, Cc, root);
  // of the real roots, the one whose conic is the widest pair of real lines
  double g = cubic_newton2(root[0], A, B, Cc);
  double best = line_pair_measure(axpy(D1, g, D2));
#pragma unroll
  for (int k = 1; k < 3; ++k) {
    const double gk = cubic_newton2(root[k], A, B, Cc);
    const double mk = line_pair_measure(axpy(D1, gk, D2));
    const bool take = (k < nr) && (mk < best || !(best == best));
    g = take ? gk : g;
    best = take ? mk : best;
  }
  ok = ok && (best < 0.0);
  const sym3 D0 = axpy(D1, g, D2);
  // pivot = the largest diagonal entry of D0, renamed to variable 0; the second conic is the one of D1, D2 that
  // D0 is not close to
  const double g0 = fabs(D0.m00), g1 = fabs(D0.m11), g2 = fabs(D0.m22);
  const int piv = (g0 >= g1 && g0 >= g2) ? 0 : (g1 >= g2 ? 1 : 2);
  const sym3 E = rot_by(D0, piv);
  const bool useD2 = fabs(g) <= 1.0;
  const sym3 Dx = rot_by(useD2 ? D2 : D1, piv);
  const double ajk = sel3(piv, a12, a02, a01), bjk = sel3(piv, b12, b02, b01);
  // E as a quadratic in variable 0: m00 l0^2 + 2 (m01 l1 + m02 l2) l0 + ... = 0 has the discriminant
  // (p l1 + q l2)^2 with p^2 = m01^2 - m00 m11, q^2 = m02^2 - m00 m22, p q = m01 m02 - m00 m12
  const double pp = E.m01 * E.m01 - E.m00 * E.m11, qq = E.m02 * E.m02 - E.m00 * E.m22;
  const double pq = E.m01 * E.m02 - E.m00 * E.m12;
  const bool by_p = pp >= qq;
  const double big = sqrt(by_p ? pp : qq);
  const double lp = by_p ? big : pq / big, lq = by_p ? pq / big : big;
  ok = ok && (big > 0.0);
  // world frame, shared by the candidates
  double e1[3], e2[3], e3[3];
  frame(P[0], P[1], P[2], e1, e2, e3);
  int filled = 0;
#pragma unroll
  for (int ln = 0; ln < 2; ++ln) {
    const double sg = ln == 0 ? 1.0 : -1.0;
    const double w1 = (sg * lp - E.m01) / E.m00, w2 = (sg * lq - E.m02) / E.m00;        // l0 = w1 l1 + w2 l2
    // the second conic on that line, a form in (l1, l2):  al l1^2 + 2 be l1 l2 + de l2^2 = 0, tau = l1 / l2
    const double al = Dx.m00 * w1 * w1 + 2.0 * Dx.m01 * w1 + Dx.m11;
    const double be = Dx.m00 * w1 * w2 + Dx.m01 * w2 + Dx.m02 * w1 + Dx.m12;
    const double de = Dx.m00 * w2 * w2 + 2.0 * Dx.m02 * w2 + Dx.m22;
    const double disc = be * be - al * de;
    const double sq = sqrt(disc);                                                     // NaN when negative: no root
    const double hq = -(be + (be >= 0.0 ? sq : -sq));
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const double tau = rt == 0 ? hq / al : de / hq;
      const double m2 = sqrt(ajk / ((tau - 2.0 * bjk) * tau + 1.0));
      const double m1 = tau * m2, m0 = w1 * m1 + w2 * m2;
      double l0 = sel3(piv, m0, m2, m1), l1 = sel3(piv, m1, m0, m2), l2 = sel3(piv, m2, m1, m0);
      double r0 = 0.0, r1 = 0.0, r2 = 0.0;
#pragma unroll
      for (int it = 0; it < 3; ++it) {                      // the last pass only evaluates the residuals
        // |l_i f_i - l_j f_j|^2 - a_ij from the difference vectors: l_i^2 + l_j^2 - 2 b_ij l_i l_j cancels from the
        // size of the squared depths down to that of the squared side, and the depths inherit that loss
        double q01 = 0.0, q02 = 0.0, q12 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const double u0 = l0 * f[0][k], u1 = l1 * f[1][k], u2 = l2 * f[2][k];
          q01 += (u0 - u1) * (u0 - u1); q02 += (u0 - u2) * (u0 - u2); q12 += (u1 - u2) * (u1 - u2);
        }
        r0 = q01 - a01; r1 = q02 - a02; r2 = q12 - a12;
        if (it == 2) break;
        const double j00 = 2.0 * (l0 - b01 * l1), j01 = 2.0 * (l1 - b01 * l0);
        const double j10 = 2.0 * (l0 - b02 * l2), j12 = 2.0 * (l2 - b02 * l0);
        const double j21 = 2.0 * (l1 - b12 * l2), j22 = 2.0 * (l2 - b12 * l1);
        const double dt = -j00 * j12 * j21 - j01 * j10 * j22;
        const double s0 = (-r0 * j12 * j21 - j01 * r1 * j22 + j01 * j12 * r2) / dt;
        const double s1 = (j00 * r1 * j22 - j00 * j12 * r2 - r0 * j10 * j22) / dt;
        const double s2 = (-j00 * r1 * j21 - j01 * j10 * r2 + r0 * j10 * j21) / dt;
        const bool step = std::isfinite(s0) && std::isfinite(s1) && std::isfinite(s2);
        l0 = step ? l0 - s0 : l0; l1 = step ? l1 - s1 : l1; l2 = step ? l2 - s2 : l2;
      }
      bool good = ok && (tau > 0.0) && (l0 > 0.0) && (l1 > 0.0) && (l2 > 0.0);
      good = good && (fabs(r0) <= 1e-9 * amax) && (fabs(r1) <= 1e-9 * amax) && (fabs(r2) <= 1e-9 * amax);
      double y0[3], y1[3], y2[3], c1[3], c2[3], c3[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) { y0[k] = l0 * f[0][k]; y1[k] = l1 * f[1][k]; y2[k] = l2 * f[2][k]; }
      frame(y0, y1, y2, c1, c2, c3);
      double R[9];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * r + c] = c1[r] * e1[c] + c2[r] * e2[c] + c3[r] * e3[c];
      double t[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) t[r] = y0[r] - (R[3 * r] * P[0][0] + R[3 * r + 1] * P[0][1] + R[3 * r + 2] * P[0][2]);
#pragma unroll
      for (int r = 0; r < 3; ++r) good = good && std::isfinite(t[r]) && std::isfinite(R[3 * r]) &&
                                         std::isfinite(R[3 * r + 1]) && std::isfinite(R[3 * r + 2]);
      const int slot = 2 * ln + rt;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        Rt[slot][4 * r] = good ? R[3 * r] : 0.0; Rt[slot][4 * r + 1] = good ? R[3 * r + 1] : 0.0;
        Rt[slot][4 * r + 2] = good ? R[3 * r + 2] : 0.0; Rt[slot][4 * r + 3] = good ? t[r] : 0.0;
      }
      filled |= good ? (1 << slot) : 0;
    }
  }
  return filled;
}

}  // namespace p3p
