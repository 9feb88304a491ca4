// The per-vertex rule of the mesh colouring (mesh_color.hip), written so that it also compiles for the host
// (tests/native/mesh_color_check.cpp) and so that NumPy reproduces it operation for operation
// (tests/mesh_color_reference.py).  include/sfm_amd.h states the whole stage; this header holds its floating point:
// float64 without FMA contraction.
//
// A vertex X with the normal n (float32 widened) walks the views in position order.  Per view, with proj = [P | p], the
// centre C, w x h pixels, the float32 depth map and the uint8 pixels:
//   project():  q_i, u = q0 / q2, v = q1 / q2, validity and the nearest pixel by the operations of tsdf::project
//   sees():     ds finite, keep != 0 and -tol <= ds - q2 <= tol: the view's own depth map says it sees this surface
//   weight():   g = C - X, l2 = (g0 g0 + g1 g1) + g2 g2 finite and > 0, c = 1 for n = 0 else ((n0 g0 + n1 g1) + n2 g2) / sqrt(l2),
//               c >= min_cos (false on NaN), wgt = c * c
//   taps():     x0 = floor(u), fx = u - x0, columns clamp(x0, 0, w - 1) and clamp(x0 + 1, 0, w - 1); rows likewise from v
//   bilinear(): top = a + fx * (b - a), bot = e + fx * (f - e), s = top + fy * (bot - top)
//   acc_k = acc_k + wgt * s_k, W = W + wgt, m = m + 1, and the view becomes `best` when wgt > bw (ties: the earlier view)
// finish(): (uint8) min(floor(acc_k / W + 0.5), 255) when m > 0 and W > 0, otherwise fill.
#pragma once
#include <cmath>
#include <cstdint>

#include "tsdf_rule.h"

#pragma clang fp contract(off)

namespace mesh_color {

struct Projection { int valid, xi, yi; double q2, u, v; };

// tsdf::project with u and v kept: the same operations in the same order
DEPTH_HD Projection project(const double* P, double X0, double X1, double X2, int w, int h) {
  const double q0 = ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[3];
  const double q1 = ((P[4] * X0 + P[5] * X1) + P[6] * X2) + P[7];
  const double q2 = ((P[8] * X0 + P[9] * X1) + P[10] * X2) + P[11];
  Projection s;
  s.u = q0 / q2;
  s.v = q1 / q2;
  s.q2 = q2;
  s.valid = (q2 > 0.0) && (s.u >= -0.5) && (s.u < (double)w - 0.5) && (s.v >= -0.5) && (s.v < (double)h - 0.5);
  s.xi = 0; s.yi = 0;
  if (s.valid) {
    const int xi = (int)floor(s.u + 0.5), yi = (int)floor(s.v + 0.5);
    s.xi = xi < w - 1 ? xi : w - 1;
    s.yi = yi < h - 1 ? yi : h - 1;
  }
  return s;
}

// the occlusion test: ds the view's depth at the nearest pixel (float32 widened), kept its keep flag, q2 the vertex's depth
DEPTH_HD int sees(double ds, int kept, double q2, double tol) {
  if (!depth::is_finite(ds) || !kept) return 0;
  const double d = ds - q2;
  return (d >= -tol) && (d <= tol);
}

// the weight of a view with the centre C for the vertex X with the normal n; 0 when the view does not count
DEPTH_HD int weight(const double* C, const double* X, const double* n, double min_cos, double* wgt) {
  const double g0 = C[0] - X[0], g1 = C[1] - X[1], g2 = C[2] - X[2];
  const double l2 = (g0 * g0 + g1 * g1) + g2 * g2;
  if (!(depth::is_finite(l2) && l2 > 0.0)) return 0;
  double c = 1.0;
  if (!(n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0)) c = ((n[0] * g0 + n[1] * g1) + n[2] * g2) / sqrt(l2);
  if (!(c >= min_cos)) return 0;
  *wgt = c * c;
  return 1;
}

struct Taps { int x0, x1, y0, y1; double fx, fy; };

DEPTH_HD int clamp(int i, int hi) { return i < 0 ? 0 : (i > hi ? hi : i); }

// the four pixels around (u, v) of a valid projection: -0.5 <= u < w - 0.5, so floor(u) is -1 .. w - 1
DEPTH_HD Taps taps(double u, double v, int w, int h) {
  const double x0 = floor(u), y0 = floor(v);
  Taps t;
  t.fx = u - x0;
  t.fy = v - y0;
  t.x0 = clamp((int)x0, w - 1);
  t.x1 = clamp((int)x0 + 1, w - 1);
  t.y0 = clamp((int)y0, h - 1);
  t.y1 = clamp((int)y0 + 1, h - 1);
  return t;
}

// a, b the upper row and e, f the lower one
DEPTH_HD double bilinear(double a, double b, double e, double f, double fx, double fy) {
  const double top = a + fx * (b - a);
  const double bot = e + fx * (f - e);
  return top + fy * (bot - top);
}

DEPTH_HD double add_sample(double acc, double wgt, double s) { return acc + wgt * s; }

// what a vertex has gathered apart from its colour sums
struct Tally { double W, bw; int m, best; };

DEPTH_HD Tally empty_tally() { return Tally{0.0, 0.0, 0, -1}; }

DEPTH_HD void add_view(Tally* t, double wgt, int v) {
  t->W = t->W + wgt;
  t->m = t->m + 1;
  if (wgt > t->bw) { t->bw = wgt; t->best = v; }
}

DEPTH_HD uint8_t finish(double acc, const Tally& t, int fill) {
  if (!(t.m > 0 && t.W > 0.0)) return (uint8_t)fill;
  const double r = floor(acc / t.W + 0.5);
  return (uint8_t)(int)(r < 255.0 ? r : 255.0);
}

DEPTH_HD uint8_t finish_views(const Tally& t) { return (uint8_t)(t.m < 255 ? t.m : 255); }

}  // namespace mesh_color
