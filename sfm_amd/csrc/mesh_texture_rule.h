// The per-texel rule of the mesh texture (mesh_texture.hip), written so that it also compiles for the host
// (tests/native/mesh_texture_check.cpp) and so that NumPy reproduces it operation for operation
// (tests/mesh_texture_reference.py).  include/sfm_amd.h states the whole stage; this header holds the layout of the atlas
// (integers) and the floating point that turns a texel into a point and a normal (float64 without FMA contraction).  The
// colour of that point is the per-view rule of mesh_color_rule.h, unchanged.
//
// With s = texels and P = s + 3 triangle t lives in cell t >> 1, half t & 1; cell c starts at texel
// ((c % cells_per_row) * P, (c / cells_per_row) * P).  Local coordinates (i, j), i, j >= 0, i + j <= s + 1: half 0 puts
// them at (x0 + i, y0 + j), half 1 at (x0 + P - 1 - i, y0 + P - 1 - j).  The corners sit on texel centres - (0, 0), (s, 0),
// (0, s) - and the diagonal i + j == s + 1 is the gutter; lx + ly == s + 2 belongs to no triangle.
//   texel_of():    the inverse map: the triangle and (i, j) of a texel, or no triangle
//   texel_at():    the map: the texel of (t, i, j)
//   numerators():  barycentric numerators over 2 s; on the gutter the texel centre moved onto the hypotenuse
//   interpolate(): ((n0 * a0 + n1 * a1) + n2 * a2) / (double)(2 s)
//   unit():        g / sqrt(l2) when l2 = (g0 g0 + g1 g1) + g2 g2 is finite and > 0, else zeros; stays double
//   corner_uv():   ((x + 0.5) / W, (y + 0.5) / H) of corner k in double, rounded once to float32; v counts downwards
#pragma once
#include <cmath>
#include <cstdint>

#include "mesh_color_rule.h"

#pragma clang fp contract(off)

namespace mesh_texture {

struct Texel { int64_t tri; int i, j; };                 // tri = -1: the texel belongs to no triangle

DEPTH_HD int patch(int s) { return s + 3; }

DEPTH_HD Texel texel_of(int x, int y, int s, int cells_per_row, int64_t n_triangles) {
  const int P = patch(s);
  const int cx = x / P, cy = y / P, lx = x - cx * P, ly = y - cy * P;
  const int64_t c = (int64_t)cy * cells_per_row + cx;
  Texel t;
  t.tri = -1; t.i = 0; t.j = 0;
  if (lx + ly <= s + 1) { t.tri = 2 * c; t.i = lx; t.j = ly; }
  else if (lx + ly >= s + 3) { t.tri = 2 * c + 1; t.i = P - 1 - lx; t.j = P - 1 - ly; }
  if (t.tri >= n_triangles) { t.tri = -1; t.i = 0; t.j = 0; }
  return t;
}

DEPTH_HD void texel_at(int64_t t, int i, int j, int s, int cells_per_row, int* x, int* y) {
  const int P = patch(s);
  const int64_t c = t >> 1;
  const int x0 = (int)(c % cells_per_row) * P, y0 = (int)(c / cells_per_row) * P;
  if (t & 1) { *x = x0 + P - 1 - i; *y = y0 + P - 1 - j; }
  else { *x = x0 + i; *y = y0 + j; }
}

struct Numerators { int n0, n1, n2; };

DEPTH_HD Numerators numerators(int i, int j, int s) {
  Numerators n;
  if (i + j <= s) { n.n1 = 2 * i; n.n2 = 2 * j; n.n0 = 2 * s - n.n1 - n.n2; }
  else { n.n1 = mesh_color::clamp(2 * i - 1, 2 * s); n.n2 = 2 * s - n.n1; n.n0 = 0; }
  return n;
}

DEPTH_HD double interpolate(const Numerators& n, double a0, double a1, double a2, int s) {
  return (((double)n.n0 * a0 + (double)n.n1 * a1) + (double)n.n2 * a2) / (double)(2 * s);
}

DEPTH_HD void unit(const double* g, double* n) {
  const double l2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
  if (depth::is_finite(l2) && l2 > 0.0) {
    const double l = sqrt(l2);
    n[0] = g[0] / l; n[1] = g[1] / l; n[2] = g[2] / l;
  } else {
    n[0] = 0.0; n[1] = 0.0; n[2] = 0.0;
  }
}

// the point and the normal of a texel from the three corners (V float64 [3][3], m the normals widened [3][3])
DEPTH_HD void point_and_normal(const Numerators& n, const double* V0, const double* V1, const double* V2, const double* m0, const double* m1,
                               const double* m2, int s, double* X, double* normal) {
  double g[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    X[a] = interpolate(n, V0[a], V1[a], V2[a], s);
    g[a] = interpolate(n, m0[a], m1[a], m2[a], s);
  }
  unit(g, normal);
}

DEPTH_HD void corner_uv(int64_t t, int k, int s, int cells_per_row, int W, int H, float* uv) {
  int x, y;
  texel_at(t, k == 1 ? s : 0, k == 2 ? s : 0, s, cells_per_row, &x, &y);
  uv[0] = (float)(((double)x + 0.5) / (double)W);
  uv[1] = (float)(((double)y + 0.5) / (double)H);
}

}  // namespace mesh_texture
