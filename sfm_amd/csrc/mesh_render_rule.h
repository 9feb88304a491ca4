// The rule of the mesh render (mesh_render.hip), written so that it also compiles for the host
// (tests/native/mesh_render_check.cpp) and so that NumPy reproduces it operation for operation
// (tests/mesh_render_reference.py).  include/sfm_amd.h states the whole stage; this header holds its floating point:
// float64 without FMA contraction, and the integers of the key.
//
// A camera P (row-major 3 x 4) and an image of w x h pixels; a, b, c are the projected corners of a triangle.
//   project():    q_i = ((P_i0 X0 + P_i1 X1) + P_i2 X2) + P_i3, u = q0 / q2, v = q1 / q2; usable iff q2 > 0 and u, v, q2
//                 finite; an unusable vertex is stored as (0, 0, 0), so q2 > 0 says usable
//   box():        columns ceil(min u) .. floor(max u), rows likewise, cut to the image in double before they become integers
//   edges():      w0 = (ub - x)(vc - y) - (vb - y)(uc - x), w1 and w2 cyclically, A = (w0 + w1) + w2
//   inside():     A != 0 and (w0, w1, w2 all >= 0 or all <= 0)
//   weights():    r_k = w_k / q2_k, s = (r0 + r1) + r2
//   depth_of():   (float)(A / s); drawn() iff that float32 is finite and > 0
//   key():        the float32's bits in the high word, the triangle in the low word; NO_KEY (all ones) is no triangle
//   bary():       b_k = r_k / s in double
//   round_u8():   min(max(floor(x + 0.5), 0), 255); what is not below 255 - a NaN included - is 255
//   shade():      round_u8((b0 ca + b1 cb) + b2 cc) of three vertex colours
//   atlas_pos():  ((b0 Ua + b1 Ub) + b2 Uc) * W - 0.5 with the float32 uv widened
//   taps():       x0 = floor(px), fx = px - x0, the columns x0 and x0 + 1 clamped to 0 .. W - 1 in double (a NaN becomes 0)
//                 before they become integers; rows likewise.  The sample is mesh_color::bilinear, rounded by round_u8.
#pragma once
#include <cmath>
#include <cstdint>

#include "mesh_color_rule.h"

#pragma clang fp contract(off)

namespace mesh_render {

struct Vertex { double u, v, q2; };                      // q2 == 0: not usable

DEPTH_HD Vertex project(const double* P, double X0, double X1, double X2) {
  const double q0 = ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[3];
  const double q1 = ((P[4] * X0 + P[5] * X1) + P[6] * X2) + P[7];
  const double q2 = ((P[8] * X0 + P[9] * X1) + P[10] * X2) + P[11];
  Vertex p;
  p.u = q0 / q2;
  p.v = q1 / q2;
  p.q2 = q2;
  if (!((q2 > 0.0) && depth::is_finite(p.u) && depth::is_finite(p.v) && depth::is_finite(q2))) { p.u = 0.0; p.v = 0.0; p.q2 = 0.0; }
  return p;
}

DEPTH_HD int usable(const Vertex& a, const Vertex& b, const Vertex& c) { return (a.q2 > 0.0) && (b.q2 > 0.0) && (c.q2 > 0.0); }

struct Box { int x0, x1, y0, y1, empty; };

DEPTH_HD double min3(double a, double b, double c) { const double m = a < b ? a : b; return m < c ? m : c; }
DEPTH_HD double max3(double a, double b, double c) { const double m = a > b ? a : b; return m > c ? m : c; }

// one axis: lo .. hi inclusive, cut to 0 .. n - 1; 0 when nothing is left (n == 0 included)
DEPTH_HD int span(double a, double b, double c, int n, int* first, int* last) {
  double lo = ceil(min3(a, b, c)), hi = floor(max3(a, b, c));
  lo = lo > 0.0 ? lo : 0.0;
  hi = hi < (double)(n - 1) ? hi : (double)(n - 1);
  if (!(lo <= hi)) return 0;
  *first = (int)lo;
  *last = (int)hi;
  return 1;
}

// of three usable corners
DEPTH_HD Box box(const Vertex& a, const Vertex& b, const Vertex& c, int w, int h) {
  Box r;
  r.x0 = 0; r.x1 = -1; r.y0 = 0; r.y1 = -1;
  r.empty = !(span(a.u, b.u, c.u, w, &r.x0, &r.x1) && span(a.v, b.v, c.v, h, &r.y0, &r.y1));
  return r;
}

DEPTH_HD int64_t box_pixels(const Box& r) { return r.empty ? 0 : (int64_t)(r.x1 - r.x0 + 1) * (int64_t)(r.y1 - r.y0 + 1); }

struct Edges { double w0, w1, w2, A; };

DEPTH_HD Edges edges(const Vertex& a, const Vertex& b, const Vertex& c, double x, double y) {
  Edges e;
  e.w0 = (b.u - x) * (c.v - y) - (b.v - y) * (c.u - x);
  e.w1 = (c.u - x) * (a.v - y) - (c.v - y) * (a.u - x);
  e.w2 = (a.u - x) * (b.v - y) - (a.v - y) * (b.u - x);
  e.A = (e.w0 + e.w1) + e.w2;
  return e;
}

DEPTH_HD int inside(const Edges& e) {
  return (e.A != 0.0) && (((e.w0 >= 0.0) && (e.w1 >= 0.0) && (e.w2 >= 0.0)) || ((e.w0 <= 0.0) && (e.w1 <= 0.0) && (e.w2 <= 0.0)));
}

struct Weights { double r0, r1, r2, s; };

DEPTH_HD Weights weights(const Edges& e, const Vertex& a, const Vertex& b, const Vertex& c) {
  Weights t;
  t.r0 = e.w0 / a.q2;
  t.r1 = e.w1 / b.q2;
  t.r2 = e.w2 / c.q2;
  t.s = (t.r0 + t.r1) + t.r2;
  return t;
}

DEPTH_HD float depth_of(const Edges& e, const Weights& t) { return (float)(e.A / t.s); }

DEPTH_HD int drawn(float d) { return (d - d == 0.0f) && (d > 0.0f); }

#define MESH_RENDER_NO_KEY 0xFFFFFFFFFFFFFFFFull
#define MESH_RENDER_NAN_BITS 0x7FC00000u

DEPTH_HD uint32_t float_bits(float d) {
  uint32_t b;
  __builtin_memcpy(&b, &d, 4);
  return b;
}

// a positive float32 orders like its bits: the smallest key is the nearest depth, then the lowest triangle
DEPTH_HD uint64_t key(float d, int64_t tri) { return ((uint64_t)float_bits(d) << 32) | (uint64_t)(uint32_t)tri; }
DEPTH_HD int64_t key_triangle(uint64_t k) { return (int64_t)(k & 0xFFFFFFFFull); }
DEPTH_HD uint32_t key_depth_bits(uint64_t k) { return (uint32_t)(k >> 32); }

// the key of triangle tri at the pixel centre (x, y), NO_KEY when it does not draw there
DEPTH_HD uint64_t claim(const Vertex& a, const Vertex& b, const Vertex& c, int x, int y, int64_t tri) {
  const Edges e = edges(a, b, c, (double)x, (double)y);
  if (!inside(e)) return MESH_RENDER_NO_KEY;
  const float d = depth_of(e, weights(e, a, b, c));
  if (!drawn(d)) return MESH_RENDER_NO_KEY;
  return key(d, tri);
}

// the winner's barycentrics at the pixel centre (x, y)
DEPTH_HD void bary(const Vertex& a, const Vertex& b, const Vertex& c, int x, int y, double* bk) {
  const Edges e = edges(a, b, c, (double)x, (double)y);
  const Weights t = weights(e, a, b, c);
  bk[0] = t.r0 / t.s;
  bk[1] = t.r1 / t.s;
  bk[2] = t.r2 / t.s;
}

DEPTH_HD uint8_t round_u8(double x) {
  const double r = floor(x + 0.5);
  return (uint8_t)(int)(r < 255.0 ? (r > 0.0 ? r : 0.0) : 255.0);
}

DEPTH_HD uint8_t shade(const double* bk, double ca, double cb, double cc) { return round_u8((bk[0] * ca + bk[1] * cb) + bk[2] * cc); }

DEPTH_HD double atlas_pos(const double* bk, float ua, float ub, float uc, int n) {
  return ((bk[0] * (double)ua + bk[1] * (double)ub) + bk[2] * (double)uc) * (double)n - 0.5;
}

// column (or row) t of an atlas n wide, clamped in double: what is not >= 0 - a NaN included - is 0
DEPTH_HD int tap(double t, int n) { return (t >= 0.0) ? ((t <= (double)(n - 1)) ? (int)t : n - 1) : 0; }

DEPTH_HD mesh_color::Taps taps(double px, double py, int W, int H) {
  const double x0 = floor(px), y0 = floor(py);
  mesh_color::Taps t;
  t.fx = px - x0;
  t.fy = py - y0;
  t.x0 = tap(x0, W);
  t.x1 = tap(x0 + 1.0, W);
  t.y0 = tap(y0, H);
  t.y1 = tap(y0 + 1.0, H);
  return t;
}

DEPTH_HD uint8_t sample(double a, double b, double e, double f, const mesh_color::Taps& t) {
  return round_u8(mesh_color::bilinear(a, b, e, f, t.fx, t.fy));
}

}  // namespace mesh_render
