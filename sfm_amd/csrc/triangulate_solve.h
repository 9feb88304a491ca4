// N-view triangulation of one track, for the device (triangulate.hip) and - SFM_HD - for the host, so that the CPU tests
// can set it against the NumPy restatement (tests/triangulate_reference.py, tests/native/triangulate_solve_check.cpp).
//   tri::camera_centre   C = -M^-1 p4 of a row-major 3 x 4 P = [M | p4], by cofactors
//   tri::solve           linear stage (streaming Givens QR of the DLT rows, jacobi::null4 of the factor; a two-view track
//                        goes through jacobi::dlt2 and gives the bits of sfm_triangulate2), a fixed number of Gauss-Newton
//                        steps on the reprojection error, then the gates of include/sfm_amd.h (SFM_TRI_*)
//   tri::gates           the gate tail alone at a given X: cheirality, triangulation angle, reprojection error
//   tri::judge           views, finiteness, then tri::gates: a point that was not triangulated here (sfm_tracks_evaluate)
// The observations come from a source `src` that is walked several times, always in the track's own order:
//   bool src.get(k, tri::Obs&)        false: observation k is not used (its image is not registered)
//   bool src.centre(k, double (&C)[3])   the same answer, the camera centre alone (the pairwise angle test)
// Storage is constant in the track length.  Every sum runs in observation order and there is no FMA contraction (host
// builds pass -ffp-contract=off), so the result of a track is a function of its used observations in their order only.
#pragma once
#include <cmath>
#include <cstdint>
#include "pose_solve.h"
#include "sfm_amd.h"

namespace tri {

struct Obs {
  double P[12];   // row-major 3 x 4 K[R|t]
  double C[3];    // camera centre
  double x, y;    // pixel
};

SFM_HD void camera_centre(const double (&P)[12], double (&C)[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double m00 = P[0], m01 = P[1], m02 = P[2], m10 = P[4], m11 = P[5], m12 = P[6], m20 = P[8], m21 = P[9], m22 = P[10];
  const double p0 = P[3], p1 = P[7], p2 = P[11];
  const double c00 = m11 * m22 - m12 * m21, c01 = m12 * m20 - m10 * m22, c02 = m10 * m21 - m11 * m20;
  const double det = (m00 * c00 + m01 * c01) + m02 * c02;
  const double a01 = m02 * m21 - m01 * m22, a02 = m01 * m12 - m02 * m11;
  const double a11 = m00 * m22 - m02 * m20, a12 = m02 * m10 - m00 * m12;
  const double a21 = m01 * m20 - m00 * m21, a22 = m00 * m11 - m01 * m10;
  C[0] = -((c00 * p0 + a01 * p1) + a02 * p2) / det;
  C[1] = -((c01 * p0 + a11 * p1) + a12 * p2) / det;
  C[2] = -((c02 * p0 + a21 * p1) + a22 * p2) / det;
}

SFM_HD bool finite3(const double (&a)[3]) { return std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]); }

// one DLT row folded into the upper-triangular factor R by Givens rotations; r is destroyed
SFM_HD void fold_row(double (&R)[4][4], double (&r)[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double b = r[j];
    if (b != 0.0) {
      const double a = R[j][j];
      const double h = sqrt(a * a + b * b);
      const double c = a / h, s = b / h;
      R[j][j] = h;
#pragma unroll
      for (int k = j + 1; k < 4; ++k) {
        const double rk = R[j][k], xk = r[k];
        R[j][k] = c * rk + s * xk;
        r[k] = c * xk - s * rk;
      }
    }
  }
}

// reprojection error of one observation at X (e2 its square, hw the depth P[2].(X,1)): the one formula behind every gate
SFM_HD double reproj(const Obs& o, const double (&X)[3], double& hw, double& e2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double hx = o.P[0] * X[0] + o.P[1] * X[1] + o.P[2] * X[2] + o.P[3];
  const double hy = o.P[4] * X[0] + o.P[5] * X[1] + o.P[6] * X[2] + o.P[7];
  hw = o.P[8] * X[0] + o.P[9] * X[1] + o.P[10] * X[2] + o.P[11];
  const double du = hx / hw - o.x, dv = hy / hw - o.y;
  e2 = du * du + dv * dv;
  return sqrt(e2);
}

// cost = sum of squared reprojection errors at X over the used observations, max_err the largest error (NaN once one is
// NaN), behind: some depth P[2].(X,1) <= 0, high: some error > max_error
template <class Src>
SFM_HD void evaluate(const Src& src, int n_raw, const double (&X)[3], double max_error, double& cost, double& max_err,
                     bool& behind, bool& high) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  Obs o;
  cost = 0.0; max_err = 0.0; behind = false; high = false;
  for (int k = 0; k < n_raw; ++k) {
    if (!src.get(k, o)) continue;
    double hw, e2;
    const double e = reproj(o, X, hw, e2);
    cost += e2;
    max_err = (e > max_err || e != e) ? e : max_err;
    behind = behind || (hw <= 0.0);
    high = high || (e > max_error);
  }
}

// The gates of a point X, in their order: evaluate, BEHIND, LOW_ANGLE (when check_angle: no pair of used views has
// d_i.d_j / (|d_i||d_j|) <= cos_min_angle with d = X - C), HIGH_ERROR.  cost and max_err as evaluate gives them.
template <class Src>
SFM_HD int gates(const Src& src, int n_raw, const double (&X)[3], double max_error, bool check_angle, double cos_min_angle,
                 double& cost, double& max_err) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool behind = false, high = false;
  evaluate(src, n_raw, X, max_error, cost, max_err, behind, high);
  if (behind) return SFM_TRI_BEHIND;
  if (check_angle) {
    bool wide = false;
    double Ci[3], Cj[3];
    for (int i = 0; i < n_raw && !wide; ++i) {
      if (!src.centre(i, Ci)) continue;
      const double a0 = X[0] - Ci[0], a1 = X[1] - Ci[1], a2 = X[2] - Ci[2];
      const double na = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
      for (int j = i + 1; j < n_raw; ++j) {
        if (!src.centre(j, Cj)) continue;
        const double b0 = X[0] - Cj[0], b1 = X[1] - Cj[1], b2 = X[2] - Cj[2];
        const double nb = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
        if ((a0 * b0 + a1 * b1 + a2 * b2) / (na * nb) <= cos_min_angle) { wide = true; break; }
      }
    }
    if (!wide) return SFM_TRI_LOW_ANGLE;
  }
  return high ? SFM_TRI_HIGH_ERROR : SFM_TRI_OK;
}

// Returns the status (SFM_TRI_*).  X and max_err are NaN for TOO_FEW_VIEWS and DEGENERATE and written for every other
// status; n_views is the number of used observations.  min_views >= 2.  The angle gate runs when check_angle is set:
// it passes when some pair of used views has d_i.d_j / (|d_i||d_j|) <= cos_min_angle with d = X - C.
template <class Src>
SFM_HD int solve(const Src& src, int n_raw, int min_views, int refine_iters, double max_error, bool check_angle,
                 double cos_min_angle, double (&X)[3], int& n_views, double& max_err) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double nan = NAN;
  X[0] = nan; X[1] = nan; X[2] = nan;
  max_err = nan;
  n_views = 0;
  Obs o;
  bool finite = true;
  for (int k = 0; k < n_raw; ++k) {
    if (!src.get(k, o)) continue;
    ++n_views;
    bool f = std::isfinite(o.x) && std::isfinite(o.y) && finite3(o.C);
#pragma unroll
    for (int e = 0; e < 12; ++e) f = f && std::isfinite(o.P[e]);
    finite = finite && f;
  }
  if (n_views < min_views) return SFM_TRI_TOO_FEW_VIEWS;
  if (!finite) return SFM_TRI_DEGENERATE;

  // ---- linear stage
  double v[4];
  if (n_views == 2) {
    double P0[12], P1[12], x0 = 0.0, y0 = 0.0, x1 = 0.0, y1 = 0.0;
    int seen = 0;
    for (int k = 0; k < n_raw; ++k) {
      if (!src.get(k, o)) continue;
      if (seen == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) P0[e] = o.P[e];
        x0 = o.x; y0 = o.y;
      } else {
#pragma unroll
        for (int e = 0; e < 12; ++e) P1[e] = o.P[e];
        x1 = o.x; y1 = o.y;
      }
      ++seen;
    }
    jacobi::dlt2(P0, P1, x0, y0, x1, y1, v);
  } else {
    double R[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int k = 0; k < 4; ++k) R[r][k] = 0.0;
    for (int k = 0; k < n_raw; ++k) {
      if (!src.get(k, o)) continue;
      double ru[4], rv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ru[e] = o.x * o.P[8 + e] - o.P[e];
        rv[e] = o.y * o.P[8 + e] - o.P[4 + e];
      }
      fold_row(R, ru);
      fold_row(R, rv);
    }
    jacobi::null4(R, v);
  }
  if (v[3] == 0.0) return SFM_TRI_DEGENERATE;
  const double Xl[3] = {v[0] / v[3], v[1] / v[3], v[2] / v[3]};
  if (!finite3(Xl)) return SFM_TRI_DEGENERATE;

  // ---- exactly refine_iters Gauss-Newton steps; a step that cannot be taken ends the loop with the last good X
  double Xc[3] = {Xl[0], Xl[1], Xl[2]};
  double cost_lin = 0.0;
  for (int it = 0; it < refine_iters; ++it) {
    double A00 = 0.0, A10 = 0.0, A11 = 0.0, A20 = 0.0, A21 = 0.0, A22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, cost = 0.0;
    for (int k = 0; k < n_raw; ++k) {
      if (!src.get(k, o)) continue;
      const double hx = o.P[0] * Xc[0] + o.P[1] * Xc[1] + o.P[2] * Xc[2] + o.P[3];
      const double hy = o.P[4] * Xc[0] + o.P[5] * Xc[1] + o.P[6] * Xc[2] + o.P[7];
      const double hw = o.P[8] * Xc[0] + o.P[9] * Xc[1] + o.P[10] * Xc[2] + o.P[11];
      const double pu = hx / hw, pv = hy / hw;
      const double du = pu - o.x, dv = pv - o.y;
      cost += du * du + dv * dv;
      const double ju0 = (o.P[0] - pu * o.P[8]) / hw, ju1 = (o.P[1] - pu * o.P[9]) / hw, ju2 = (o.P[2] - pu * o.P[10]) / hw;
      const double jv0 = (o.P[4] - pv * o.P[8]) / hw, jv1 = (o.P[5] - pv * o.P[9]) / hw, jv2 = (o.P[6] - pv * o.P[10]) / hw;
      A00 += ju0 * ju0 + jv0 * jv0;
      A10 += ju1 * ju0 + jv1 * jv0;
      A11 += ju1 * ju1 + jv1 * jv1;
      A20 += ju2 * ju0 + jv2 * jv0;
      A21 += ju2 * ju1 + jv2 * jv1;
      A22 += ju2 * ju2 + jv2 * jv2;
      g0 += ju0 * du + jv0 * dv;
      g1 += ju1 * du + jv1 * dv;
      g2 += ju2 * du + jv2 * dv;
    }
    if (it == 0) cost_lin = cost;
    if (!(A00 > 0.0)) break;
    const double l00 = sqrt(A00);
    const double l10 = A10 / l00, l20 = A20 / l00;
    const double d1 = A11 - l10 * l10;
    if (!(d1 > 0.0)) break;
    const double l11 = sqrt(d1);
    const double l21 = (A21 - l20 * l10) / l11;
    const double d2 = A22 - l20 * l20 - l21 * l21;
    if (!(d2 > 0.0)) break;
    const double l22 = sqrt(d2);
    const double y0 = g0 / l00;
    const double y1 = (g1 - l10 * y0) / l11;
    const double y2 = (g2 - l20 * y0 - l21 * y1) / l22;
    const double z2 = y2 / l22;
    const double z1 = (y1 - l21 * z2) / l11;
    const double z0 = (y0 - l10 * z1 - l20 * z2) / l00;
    const double Xn[3] = {Xc[0] - z0, Xc[1] - z1, Xc[2] - z2};
    if (!finite3(Xn)) break;
    Xc[0] = Xn[0]; Xc[1] = Xn[1]; Xc[2] = Xn[2];
  }

  // ---- the gates, on the refined point unless it costs more than the linear one
  double cost = 0.0;
  int st = gates(src, n_raw, Xc, max_error, check_angle, cos_min_angle, cost, max_err);
  if (refine_iters > 0 && cost > cost_lin) {
    Xc[0] = Xl[0]; Xc[1] = Xl[1]; Xc[2] = Xl[2];
    st = gates(src, n_raw, Xc, max_error, check_angle, cos_min_angle, cost, max_err);
  }
  X[0] = Xc[0]; X[1] = Xc[1]; X[2] = Xc[2];
  return st;
}

// A point that came from somewhere else (a bundle adjustment moved it) judged by the gates of solve, in solve's order:
// too few views, degenerate (a non-finite input of a used view or a non-finite X), then gates().  max_err is NaN for the
// first two and the largest reprojection error otherwise.  Fed the X solve returned with status OK, BEHIND, LOW_ANGLE or
// HIGH_ERROR it runs the operations of solve's last gates() call on the same numbers: same status, same max_err bits.
template <class Src>
SFM_HD int judge(const Src& src, int n_raw, int min_views, const double (&X)[3], double max_error, bool check_angle,
                 double cos_min_angle, int& n_views, double& max_err) {
  max_err = NAN;
  n_views = 0;
  Obs o;
  bool finite = finite3(X);
  for (int k = 0; k < n_raw; ++k) {
    if (!src.get(k, o)) continue;
    ++n_views;
    bool f = std::isfinite(o.x) && std::isfinite(o.y) && finite3(o.C);
#pragma unroll
    for (int e = 0; e < 12; ++e) f = f && std::isfinite(o.P[e]);
    finite = finite && f;
  }
  if (n_views < min_views) return SFM_TRI_TOO_FEW_VIEWS;
  if (!finite) return SFM_TRI_DEGENERATE;
  double cost = 0.0;
  return gates(src, n_raw, X, max_error, check_angle, cos_min_angle, cost, max_err);
}

}  // namespace tri
