// The two small one-sided Jacobi (Hestenes) decompositions of the two-view rows, for the device and - SFM_HD - for the
// host, so that the CPU tests can set them against LAPACK (tests/native/pose_solve_check.cpp):
//   jacobi::null4       right singular vector of the smallest singular value of a 4 x 4: the DLT of cv2.triangulatePoints
//                       as k_triangulate2 (driver.hip) and the relative-pose kernels (pose.hip) run it
//   jacobi::decompose_essential   the four [R|t] of cv2.decomposeEssentialMat from a 3 x 3 E
// Every array index is a compile-time constant once the loops are unrolled, so the matrices stay in registers.  No FMA
// contraction: the iteration is the reference's arithmetic, operation for operation (host builds pass -ffp-contract=off).
#pragma once
#include <cfloat>
#include <cmath>
#include "ransac_common.h"

namespace jacobi {

// Hestenes sweeps on the columns of U (a 4 x 4, destroyed), eps = 10 * DBL_EPSILON, at most 30 sweeps, as OpenCV's
// JacobiSVDImpl_; v = the column of the accumulated rotations that belongs to the column of U with the smallest norm
// (the first of equal ones).
SFM_HD void null4(double (&U)[4][4], double (&v)[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double V[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) V[r][k] = (r == k) ? 1.0 : 0.0;
  const double eps = 10.0 * DBL_EPSILON;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool changed = false;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int q = p + 1; q < 4; ++q) {
        double a = 0.0, b = 0.0, g = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) { a += U[r][p] * U[r][p]; b += U[r][q] * U[r][q]; g += U[r][p] * U[r][q]; }
        if (fabs(g) > eps * sqrt(a * b)) {
          changed = true;
          const double zeta = (b - a) / (2.0 * g);
          const double tt = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double up = U[r][p], uq = U[r][q];
            U[r][p] = c * up - s * uq; U[r][q] = s * up + c * uq;
            const double vp = V[r][p], vq = V[r][q];
            V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq;
          }
        }
      }
    }
    if (!changed) break;
  }
  double best = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double nk = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) nk += U[r][k] * U[r][k];
    if (k == 0 || nk < best) {
      best = nk;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = V[r][k];
    }
  }
}

// rows x P[2] - P[0], y P[2] - P[1] of both views (P row-major 3 x 4), then null4
SFM_HD void dlt2(const double (&P0)[12], const double (&P1)[12], double x0, double y0, double x1, double y1,
                 double (&v)[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double U[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    U[0][k] = x0 * P0[8 + k] - P0[k];
    U[1][k] = y0 * P0[8 + k] - P0[4 + k];
    U[2][k] = x1 * P1[8 + k] - P1[k];
    U[3][k] = y1 * P1[8 + k] - P1[4 + k];
  }
  null4(U, v);
}

// E = U S V^T by the same iteration on the columns of E (row-major 3 x 3): the rotated columns are S_k u_k, the
// accumulated rotations are V.  Columns sorted by norm, descending; u2 = u0 x u1, because the third column has norm
// ~ 0 for an essential matrix and cannot be normalised - so det U = +1 by construction - and V is negated when its
// determinant is -1.  W = [[0,1,0],[-1,0,0],[0,0,1]], R1 = U W V^T, R2 = U W^T V^T, t = u2 (unit length).
// Rt [4][12] row-major [R|t] in the order [R1|t], [R2|t], [R1|-t], [R2|-t]: this routine's own order (the signs of a
// singular vector pair are not unique, and R1 <-> R2 swap with the sign of u2).  Returns false, with Rt untouched,
// when E is not finite or its second singular value is not > 0.
SFM_HD bool decompose_essential(const double (&E)[9], double (&Rt)[4][12]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double A[3][3], V[3][3];
  bool finite = true;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      A[r][k] = E[3 * r + k];
      V[r][k] = (r == k) ? 1.0 : 0.0;
      finite = finite && std::isfinite(E[3 * r + k]);
    }
  if (!finite) return false;
  const double eps = 10.0 * DBL_EPSILON;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool changed = false;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        double a = 0.0, b = 0.0, g = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) { a += A[r][p] * A[r][p]; b += A[r][q] * A[r][q]; g += A[r][p] * A[r][q]; }
        if (fabs(g) > eps * sqrt(a * b)) {
          changed = true;
          const double zeta = (b - a) / (2.0 * g);
          const double tt = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const double up = A[r][p], uq = A[r][q];
            A[r][p] = c * up - s * uq; A[r][q] = s * up + c * uq;
            const double vp = V[r][p], vq = V[r][q];
            V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq;
          }
        }
      }
    }
    if (!changed) break;
  }
  double nrm[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) nrm[k] = A[0][k] * A[0][k] + A[1][k] * A[1][k] + A[2][k] * A[2][k];
  // three compare-exchanges: (0,1) (1,2) (0,1)
#pragma unroll
  for (int step = 0; step < 3; ++step) {
    const int p = (step == 1) ? 1 : 0, q = p + 1;
    if (nrm[q] > nrm[p]) {
      const double tn = nrm[p]; nrm[p] = nrm[q]; nrm[q] = tn;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double ta = A[r][p]; A[r][p] = A[r][q]; A[r][q] = ta;
        const double tv = V[r][p]; V[r][p] = V[r][q]; V[r][q] = tv;
      }
    }
  }
  const double s0 = sqrt(nrm[0]), s1 = sqrt(nrm[1]);
  if (!(s1 > 0.0) || !std::isfinite(s0)) return false;
  double U[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) { U[r][0] = A[r][0] / s0; U[r][1] = A[r][1] / s1; }
  U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
  U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
  U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  const double detV = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                      V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
  const double sg = detV < 0.0 ? -1.0 : 1.0;
  // U W = [-u1, u0, u2], U W^T = [u1, -u0, u2]; R = (U W) V^T, entry (r, c) = sum_k (U W)[r][k] V[c][k]
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v0 = sg * V[c][0], v1 = sg * V[c][1], v2 = sg * V[c][2];
      const double r1 = -U[r][1] * v0 + U[r][0] * v1 + U[r][2] * v2;
      const double r2 = U[r][1] * v0 - U[r][0] * v1 + U[r][2] * v2;
      Rt[0][4 * r + c] = r1; Rt[2][4 * r + c] = r1;
      Rt[1][4 * r + c] = r2; Rt[3][4 * r + c] = r2;
    }
    Rt[0][4 * r + 3] = U[r][2]; Rt[1][4 * r + 3] = U[r][2];
    Rt[2][4 * r + 3] = -U[r][2]; Rt[3][4 * r + 3] = -U[r][2];
  }
  return true;
}

}  // namespace jacobi
