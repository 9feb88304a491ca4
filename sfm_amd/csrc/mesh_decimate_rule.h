// The rule of decimation by vertex clustering (mesh_decimate.hip): the cell of a vertex and its key, the mean and the
// normal of a cluster, the quadric of its corners with the solve that places the new vertex, and the rule for triangles that
// land on one cluster triple.  include/sfm_amd.h states it.  Plain C++: it compiles for the host too
// (tests/native/mesh_decimate_check.cpp replays it under the sanitizers) and NumPy reproduces it operation for operation
// (tests/mesh_decimate_reference.py).  float64 without FMA contraction: every product and every sum rounds on its own.
#pragma once
#include <cmath>
#include <cstdint>

#include "depth_rule.h"
#include "mesh_clean_rule.h"

#pragma clang fp contract(off)

#define MESH_DEC_AXIS_BITS 21
#define MESH_DEC_AXIS_CELLS 2097152.0                      /* 2^21 cells along an axis */
#define MESH_DEC_DEAD_KEY 0xFFFFFFFFFFFFFFFFull            /* a vertex without a cell, a triangle without a triple */
#define MESH_DEC_DEAD_CORNER 0xFFFFFFFFu                   /* a corner of an unsound triangle */
#define MESH_DEC_LAMBDA 0.015625                           /* 2^-6 of the trace pulls towards the mean */

namespace mesh_decimate {

// the cell index of one coordinate, -1 when it has none: q = floor((v - origin) / cell) with 0 <= q < 2^21.  The comparisons
// are on the double; it becomes an integer only once it is known to fit.
DEPTH_HD int64_t cell_index(double v, double origin, double cell) {
  if (!depth::is_finite(v)) return -1;
  const double q = floor((v - origin) / cell);
  if (!(q >= 0.0 && q < MESH_DEC_AXIS_CELLS)) return -1;
  return (int64_t)q;
}

// (iz << 42) | (iy << 21) | ix, or all ones for an unsound vertex; no live key is all ones (bit 63 is never set)
DEPTH_HD uint64_t vertex_key(const double* v, const double* origin, double cell, int64_t* idx) {
  idx[0] = cell_index(v[0], origin[0], cell);
  idx[1] = cell_index(v[1], origin[1], cell);
  idx[2] = cell_index(v[2], origin[2], cell);
  if (idx[0] < 0 || idx[1] < 0 || idx[2] < 0) return MESH_DEC_DEAD_KEY;
  return ((uint64_t)idx[2] << (2 * MESH_DEC_AXIS_BITS)) | ((uint64_t)idx[1] << MESH_DEC_AXIS_BITS) | (uint64_t)idx[0];
}

// the faces of cell i along one axis
DEPTH_HD double cell_lo(double origin, double cell, int64_t i) { return origin + cell * (double)i; }
DEPTH_HD double cell_hi(double origin, double cell, int64_t i) { return origin + cell * (double)(i + 1); }

// member number i of a cluster, in ascending vertex index: s and ns become the sums so far (the first member starts them)
DEPTH_HD void add_member(int64_t i, const double* v, const float* normal, double* s, double* ns) {
  if (i == 0) {
    s[0] = v[0]; s[1] = v[1]; s[2] = v[2];
    if (normal) { ns[0] = (double)normal[0]; ns[1] = (double)normal[1]; ns[2] = (double)normal[2]; }
  } else {
    s[0] = s[0] + v[0]; s[1] = s[1] + v[1]; s[2] = s[2] + v[2];
    if (normal) { ns[0] = ns[0] + (double)normal[0]; ns[1] = ns[1] + (double)normal[1]; ns[2] = ns[2] + (double)normal[2]; }
  }
}
DEPTH_HD void mean(const double* s, int64_t n, double* m) {
  const double count = (double)n;
  m[0] = s[0] / count; m[1] = s[1] / count; m[2] = s[2] / count;
}
// the sum of the members' normals as a unit float32 vector; zeros when its squared length is 0 or not finite
DEPTH_HD void unit_normal(double* ns, float* out) {
  depth::normalise(ns, depth::norm2(ns));
  out[0] = (float)ns[0]; out[1] = (float)ns[1]; out[2] = (float)ns[2];
}

// The quadric about the mean m: A = (A00, A01, A02, A11, A12, A22) and g, both zeros before the first corner.  One corner of
// the triangle (p0, p1, p2), whichever corner it is: n = (p1 - p0) x (p2 - p0), not normalised, so a triangle weighs with
// the square of its area; s = n . (p0 - m).
DEPTH_HD void add_corner(const double* p0, const double* p1, const double* p2, const double* m, double* A, double* g) {
  const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
  const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
  const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
  const double rx = p0[0] - m[0], ry = p0[1] - m[1], rz = p0[2] - m[2];
  const double s = (nx * rx + ny * ry) + nz * rz;
  A[0] = A[0] + nx * nx; A[1] = A[1] + nx * ny; A[2] = A[2] + nx * nz;
  A[3] = A[3] + ny * ny; A[4] = A[4] + ny * nz; A[5] = A[5] + nz * nz;
  g[0] = g[0] + nx * s; g[1] = g[1] + ny * s; g[2] = g[2] + nz * s;
}

// (A + lambda I) y = g by an L D L^T in the order the header states, x = m + y.  Returns 1 and x when the trace and the three
// pivots are > 0, x is finite and lies in the box [lo, hi] of the cell; otherwise 0 and x = m.
DEPTH_HD int place(const double* A, const double* g, const double* m, const double* lo, const double* hi, double* x) {
  const double tr = (A[0] + A[3]) + A[5];
  const double lambda = tr * MESH_DEC_LAMBDA;
  const double B00 = A[0] + lambda, B01 = A[1], B02 = A[2], B11 = A[3] + lambda, B12 = A[4], B22 = A[5] + lambda;
  const double d0 = B00, l10 = B01 / d0, l20 = B02 / d0;
  const double d1 = B11 - l10 * B01, u = B12 - l20 * B01, l21 = u / d1;
  const double d2 = (B22 - l20 * B02) - l21 * u;
  const double z1 = g[1] - l10 * g[0], z2 = (g[2] - l20 * g[0]) - l21 * z1;
  const double y2 = z2 / d2, y1 = z1 / d1 - l21 * y2, y0 = (g[0] / d0 - l10 * y1) - l20 * y2;
  x[0] = m[0] + y0; x[1] = m[1] + y1; x[2] = m[2] + y2;
  int ok = tr > 0.0 && d0 > 0.0 && d1 > 0.0 && d2 > 0.0;
  for (int a = 0; a < 3; ++a) ok = ok && depth::is_finite(x[a]) && lo[a] <= x[a] && x[a] <= hi[a];
  if (!ok) { x[0] = m[0]; x[1] = m[1]; x[2] = m[2]; }
  return ok;
}

// The clusters (c0, c1, c2) of a triangle sorted into s[0] <= s[1] <= s[2]; *odd = 1 when its own order is an odd
// permutation of that.  Returns 0 when two of them are equal (the triangle is degenerate), 1 otherwise.
DEPTH_HD int sort_triple(int32_t c0, int32_t c1, int32_t c2, int32_t* s, int* odd) {
  int swaps = 0;
  int32_t t;
  if (c0 > c1) { t = c0; c0 = c1; c1 = t; ++swaps; }
  if (c1 > c2) { t = c1; c1 = c2; c2 = t; ++swaps; }
  if (c0 > c1) { t = c0; c0 = c1; c1 = t; ++swaps; }
  s[0] = c0; s[1] = c1; s[2] = c2;
  *odd = swaps & 1;
  return (c0 != c1 && c1 != c2) ? 1 : 0;
}

// The triangle that stays of a group with one sorted triple: n_even / n_odd of them are even / odd permutations, first_even /
// first_odd the first of each in old triangle order.  -1: they cancel.
DEPTH_HD int64_t duplicate_pick(int64_t n_even, int64_t n_odd, int64_t first_even, int64_t first_odd) {
  if (n_even > n_odd) return first_even;
  if (n_odd > n_even) return first_odd;
  return -1;
}

}  // namespace mesh_decimate
