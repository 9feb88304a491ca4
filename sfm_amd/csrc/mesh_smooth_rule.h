// The rule of mesh smoothing (mesh_smooth.hip): the keys of the vertex adjacency, the state of a vertex, one Taubin /
// Laplacian step and the area-weighted vertex normal.  include/sfm_amd.h states it.  Plain C++: it compiles for the host too
// (tests/native/mesh_smooth_check.cpp replays it under the sanitizers) and NumPy reproduces it operation for operation
// (tests/mesh_smooth_reference.py).  float64 without FMA contraction: every product and every sum rounds on its own.
#pragma once
#include <cmath>
#include <cstdint>

#include "depth_rule.h"
#include "mesh_clean_rule.h"

#pragma clang fp contract(off)

#define MESH_ADJ_DEAD_KEY 0xFFFFFFFFFFFFFFFFull            /* a half-edge that is not live */
#define MESH_ADJ_DEAD_CORNER 0xFFFFFFFFu                   /* a corner of an unsound triangle */
#define MESH_ADJ_BOUNDARY 1                                /* vertex_flags */
#define MESH_ADJ_ISOLATED 2
#define MESH_SMOOTH_PIN_BOUNDARY 1                         /* vertex_state */
#define MESH_SMOOTH_PIN_GIVEN 2
#define MESH_SMOOTH_UNSOUND 4
#define MESH_SMOOTH_ISOLATED 8

namespace mesh_smooth {

// Half-edge k of the triangle (v0, v1, v2) runs from a to b; returns 1 when it is live: the triangle is sound and a != b.
DEPTH_HD int halfedge(const int32_t* v, int k, int64_t n_vertices, int32_t* a, int32_t* b) {
  *a = v[k];
  *b = v[k == 2 ? 0 : k + 1];
  return mesh_clean::sound(v[0], v[1], v[2], n_vertices) && *a != *b;
}
// the entry "b is a neighbour of a"; never all ones, a is below 2^31
DEPTH_HD uint64_t edge_key(int32_t a, int32_t b) { return ((uint64_t)(uint32_t)a << 32) | (uint64_t)(uint32_t)b; }
DEPTH_HD int32_t key_vertex(uint64_t key) { return (int32_t)(key >> 32); }
DEPTH_HD int32_t key_neighbour(uint64_t key) { return (int32_t)(key & 0xFFFFFFFFull); }

// the flags of a vertex from the number of its neighbours and whether some edge to one is not used exactly twice
DEPTH_HD uint8_t vertex_flags(int64_t n_neighbours, bool odd_edge) {
  return (uint8_t)((odd_edge ? MESH_ADJ_BOUNDARY : 0) | (n_neighbours == 0 ? MESH_ADJ_ISOLATED : 0));
}

// the state of a vertex, fixed before the first step
DEPTH_HD uint8_t vertex_state(uint8_t flags, bool pinned, bool pin_boundary, const double* x) {
  const bool finite = depth::is_finite(x[0]) && depth::is_finite(x[1]) && depth::is_finite(x[2]);
  return (uint8_t)(((flags & MESH_ADJ_BOUNDARY) && pin_boundary ? MESH_SMOOTH_PIN_BOUNDARY : 0) | (pinned ? MESH_SMOOTH_PIN_GIVEN : 0) |
                   (finite ? 0 : MESH_SMOOTH_UNSOUND) | ((flags & MESH_ADJ_ISOLATED) ? MESH_SMOOTH_ISOLATED : 0));
}

// One step of a free vertex: s starts as (0, 0, 0) and takes the sound neighbours in ascending index, s = s + x_j; then
// m = s / n and x' = x + f (m - x), per axis.
DEPTH_HD void add_neighbour(const double* xj, double* s) { s[0] = s[0] + xj[0]; s[1] = s[1] + xj[1]; s[2] = s[2] + xj[2]; }
DEPTH_HD void move(const double* x, const double* s, int64_t n, double f, double* out) {
  const double count = (double)n;
  for (int a = 0; a < 3; ++a) {
    const double m = s[a] / count;
    out[a] = x[a] + f * (m - x[a]);
  }
}

// (p1 - p0) x (p2 - p0), not normalised: twice the area along the normal
DEPTH_HD void face_normal(const double* p0, const double* p1, const double* p2, double* n) {
  const double e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
  const double e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
  n[0] = e1y * e2z - e1z * e2y;
  n[1] = e1z * e2x - e1x * e2z;
  n[2] = e1x * e2y - e1y * e2x;
}
// the sum over the corners of a vertex, in ascending half-edge, starts as (0, 0, 0): ns = ns + n
DEPTH_HD void add_face(const double* n, double* ns) { ns[0] = ns[0] + n[0]; ns[1] = ns[1] + n[1]; ns[2] = ns[2] + n[2]; }
// the sum as a unit float32 vector, rounded once; zeros when its squared length is 0 or not finite
DEPTH_HD void unit_normal(double* ns, float* out) {
  depth::normalise(ns, depth::norm2(ns));
  out[0] = (float)ns[0]; out[1] = (float)ns[1]; out[2] = (float)ns[2];
}

}  // namespace mesh_smooth
