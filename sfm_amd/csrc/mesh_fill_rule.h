// The rule of the edge table and of hole filling (mesh_fill.hip): the half-edges and their keys, the stack that splits a
// boundary loop where it passes a vertex twice, and the centroid fan.  include/sfm_amd.h states it.  Plain C++: it compiles
// for the host too (tests/native/mesh_fill_check.cpp walks random closed walks through it under the sanitizers) and NumPy
// reproduces it operation for operation (tests/mesh_fill_reference.py).  Integers apart from the new vertex and its normal:
// float64 without FMA contraction.
//
// Half-edge h = 3 t + k of triangle t runs from a_h = tri[t][k] to b_h = tri[t][(k + 1) % 3]; it is live iff the triangle is
// sound (mesh_clean_rule.h) and a_h != b_h.
#pragma once
#include <cmath>
#include <cstdint>

#include "depth_rule.h"
#include "mesh_clean_rule.h"

#pragma clang fp contract(off)

#define MESH_FILL_WAVE 64           /* the longest short loop: one lane of a wavefront per half-edge */
#define MESH_FILL_DEAD_KEY 0xFFFFFFFFFFFFFFFFull

namespace mesh_fill {

DEPTH_HD int next_in_triangle(int h) {
  const int k = h % 3;
  return h - k + (k == 2 ? 0 : k + 1);
}

// the two ends of half-edge k of the triangle (v0, v1, v2)
DEPTH_HD void ends(int32_t v0, int32_t v1, int32_t v2, int k, int32_t* a, int32_t* b) {
  *a = k == 0 ? v0 : (k == 1 ? v1 : v2);
  *b = k == 0 ? v1 : (k == 1 ? v2 : v0);
}

// the sort key of a half-edge: the unordered pair, or all ones for one that is not live (no live key is all ones: an index
// is below 2^31)
DEPTH_HD uint64_t edge_key(int32_t v0, int32_t v1, int32_t v2, int k, int64_t n_vertices) {
  int32_t a, b;
  ends(v0, v1, v2, k, &a, &b);
  if (!mesh_clean::sound(v0, v1, v2, n_vertices) || a == b) return MESH_FILL_DEAD_KEY;
  const uint64_t lo = (uint64_t)(a < b ? a : b), hi = (uint64_t)(a < b ? b : a);
  return (lo << 32) | hi;
}

// The sub-loops of a loop of n <= MESH_FILL_WAVE half-edges in `next` order from its leader: a[i] -> b[i] with the number
// h[i].  Push i; if a stack entry p starts where i ends, the entries p .. top are a sub-loop and are popped.  Per entry:
// name = the smallest half-edge of its sub-loop, len = its edges, succ = the entry after it in the sub-loop's own cyclic
// order.  `stack` is n words of the caller's.  Returns 1 when the stack is empty at the end, as it is for every closed walk
// with b[i] == a[(i + 1) % n]; 0 otherwise, with name = -1 and len = 0 on the entries left over.
DEPTH_HD int split(int n, const int32_t* a, const int32_t* b, const int32_t* h, int32_t* stack, int32_t* name, int32_t* len, int32_t* succ) {
  int top = 0;
  for (int i = 0; i < n; ++i) {
    name[i] = -1; len[i] = 0; succ[i] = i;
    stack[top++] = i;
    const int32_t end = b[i];
    for (int p = 0; p < top; ++p) {
      if (a[stack[p]] != end) continue;
      int32_t low = h[stack[p]];
      for (int j = p + 1; j < top; ++j) low = h[stack[j]] < low ? h[stack[j]] : low;
      for (int j = p; j < top; ++j) {
        const int e = stack[j];
        name[e] = low; len[e] = top - p; succ[e] = stack[j + 1 < top ? j + 1 : p];
      }
      top = p;
      break;
    }
  }
  return top == 0 ? 1 : 0;
}

DEPTH_HD bool filled(int len, int max_edges) { return len >= 3 && len <= max_edges; }

// The new vertex c and its normal for the sub-loop of n entries that starts at entry `start` (its name) and goes on by succ;
// entry e runs from vertex a[e] to vertex a[succ[e]].  c = (((v[a_0] + v[a_1]) + ...)) / n per coordinate; the normal is the
// unit vector of the sum over the same order of cross(v[a] - v[b], c - v[b]), every product and sum rounding on its own,
// each component divided by the square root and rounded once to float32; zeros when the squared length is 0 or not finite.
DEPTH_HD void patch(int n, int start, const int32_t* succ, const int32_t* a, const double* vertices, double* c, float* normal) {
  int e = start;
  double s[3] = {vertices[3 * (int64_t)a[e]], vertices[3 * (int64_t)a[e] + 1], vertices[3 * (int64_t)a[e] + 2]};
  for (int i = 1; i < n; ++i) {
    e = succ[e];
    const double* v = vertices + 3 * (int64_t)a[e];
    s[0] = s[0] + v[0]; s[1] = s[1] + v[1]; s[2] = s[2] + v[2];
  }
  const double count = (double)n;
  c[0] = s[0] / count; c[1] = s[1] / count; c[2] = s[2] / count;
  double m[3] = {0.0, 0.0, 0.0};
  e = start;
  for (int i = 0; i < n; ++i) {
    const double* va = vertices + 3 * (int64_t)a[e];
    const double* vb = vertices + 3 * (int64_t)a[succ[e]];
    const double p0 = va[0] - vb[0], p1 = va[1] - vb[1], p2 = va[2] - vb[2];
    const double q0 = c[0] - vb[0], q1 = c[1] - vb[1], q2 = c[2] - vb[2];
    const double x0 = p1 * q2, x1 = p2 * q1, y0 = p2 * q0, y1 = p0 * q2, z0 = p0 * q1, z1 = p1 * q0;
    m[0] = m[0] + (x0 - x1); m[1] = m[1] + (y0 - y1); m[2] = m[2] + (z0 - z1);
    e = succ[e];
  }
  depth::normalise(m, depth::norm2(m));
  normal[0] = (float)m[0]; normal[1] = (float)m[1]; normal[2] = (float)m[2];
}

}  // namespace mesh_fill
