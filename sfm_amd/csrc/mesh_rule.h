// The rule of marching tetrahedra over the Kuhn split (mesh.hip), written so that it also compiles for the host
// (tests/native/mesh_check.cpp derives the table below from the geometric rule and compares) and so that NumPy reproduces
// it operation for operation (tests/mesh_reference.py).  include/sfm_amd.h states the whole stage.  Everything here is
// integer apart from the cut along an edge and the gradient: float64 without FMA contraction.
//
// A corner of a cell is the number x + 2 y + 4 z of its offset.  A direction d = 0 .. 6 has the offset with the corner
// number MESH_DIR_CORNER(d): (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1).  Tetrahedron T = 0 .. 5 of a
// cell belongs to the permutation (a, b, c) of the axes in lexicographic order and has the local nodes 0, e_a, e_a + e_b,
// (1,1,1): MESH_TET_CORNER[T].  The case of a tetrahedron has bit n set iff its local node n is inside.
// MESH_CASE[T][case] = { number of triangles, then per triangle vertex (corner of the owning node << 3) | direction }.
#pragma once
#include <cmath>
#include <cstdint>

#include "depth_rule.h"

#pragma clang fp contract(off)

#define MESH_DIRS 7
#define MESH_DIR_CORNER(d) ((0x7653421 >> (4 * (d))) & 7)

constexpr uint8_t MESH_TET_CORNER[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};

constexpr uint8_t MESH_CASE[6][16][7] = {
    {{ 0,  0,  0,  0,  0,  0,  0}, { 1,  0,  3,  6,  0,  0,  0}, { 1,  0, 13,  9,  0,  0,  0}, { 2,  3,  6, 13,  3, 13,  9}, { 1,  3,  9, 26,  0,  0,  0}, { 2,  0, 26,  6,  0,  9, 26}, { 2,  0, 13, 26,  0, 26,  3}, { 1,  6, 13, 26,  0,  0,  0}, { 1,  6, 26, 13,  0,  0,  0}, { 2,  0,  3, 26,  0, 26, 13}, { 2,  0, 26,  9,  0,  6, 26}, { 1,  3, 26,  9,  0,  0,  0}, { 2,  3,  9, 13,  3, 13,  6}, { 1,  0,  9, 13,  0,  0,  0}, { 1,  0,  6,  3,  0,  0,  0}, { 0,  0,  0,  0,  0,  0,  0}},
    {{ 0,  0,  0,  0,  0,  0,  0}, { 1,  0,  6,  4,  0,  0,  0}, { 1,  0, 10, 13,  0,  0,  0}, { 2,  4, 13,  6,  4, 10, 13}, { 1,  4, 41, 10,  0,  0,  0}, { 2,  0,  6, 41,  0, 41, 10}, { 2,  0, 41, 13,  0,  4, 41}, { 1,  6, 41, 13,  0,  0,  0}, { 1,  6, 13, 41,  0,  0,  0}, { 2,  0, 41,  4,  0, 13, 41}, { 2,  0, 10, 41,  0, 41,  6}, { 1,  4, 10, 41,  0,  0,  0}, { 2,  4, 13, 10,  4,  6, 13}, { 1,  0, 13, 10,  0,  0,  0}, { 1,  0,  4,  6,  0,  0,  0}, { 0,  0,  0,  0,  0,  0,  0}},
    {{ 0,  0,  0,  0,  0,  0,  0}, { 1,  1,  6,  3,  0,  0,  0}, { 1,  1, 16, 20,  0,  0,  0}, { 2,  3, 20,  6,  3, 16, 20}, { 1,  3, 26, 16,  0,  0,  0}, { 2,  1,  6, 26,  1, 26, 16}, { 2,  1, 26, 20,  1,  3, 26}, { 1,  6, 26, 20,  0,  0,  0}, { 1,  6, 20, 26,  0,  0,  0}, { 2,  1, 26,  3,  1, 20, 26}, { 2,  1, 16, 26,  1, 26,  6}, { 1,  3, 16, 26,  0,  0,  0}, { 2,  3, 20, 16,  3,  6, 20}, { 1,  1, 20, 16,  0,  0,  0}, { 1,  1,  3,  6,  0,  0,  0}, { 0,  0,  0,  0,  0,  0,  0}},
    {{ 0,  0,  0,  0,  0,  0,  0}, { 1,  1,  5,  6,  0,  0,  0}, { 1,  1, 20, 18,  0,  0,  0}, { 2,  5,  6, 20,  5, 20, 18}, { 1,  5, 18, 48,  0,  0,  0}, { 2,  1, 48,  6,  1, 18, 48}, { 2,  1, 20, 48,  1, 48,  5}, { 1,  6, 20, 48,  0,  0,  0}, { 1,  6, 48, 20,  0,  0,  0}, { 2,  1,  5, 48,  1, 48, 20}, { 2,  1, 48, 18,  1,  6, 48}, { 1,  5, 48, 18,  0,  0,  0}, { 2,  5, 18, 20,  5, 20,  6}, { 1,  1, 18, 20,  0,  0,  0}, { 1,  1,  6,  5,  0,  0,  0}, { 0,  0,  0,  0,  0,  0,  0}},
    {{ 0,  0,  0,  0,  0,  0,  0}, { 1,  2,  4,  6,  0,  0,  0}, { 1,  2, 35, 32,  0,  0,  0}, { 2,  4,  6, 35,  4, 35, 32}, { 1,  4, 32, 41,  0,  0,  0}, { 2,  2, 41,  6,  2, 32, 41}, { 2,  2, 35, 41,  2, 41,  4}, { 1,  6, 35, 41,  0,  0,  0}, { 1,  6, 41, 35,  0,  0,  0}, { 2,  2,  4, 41,  2, 41, 35}, { 2,  2, 41, 32,  2,  6, 41}, { 1,  4, 41, 32,  0,  0,  0}, { 2,  4, 32, 35,  4, 35,  6}, { 1,  2, 32, 35,  0,  0,  0}, { 1,  2,  6,  4,  0,  0,  0}, { 0,  0,  0,  0,  0,  0,  0}},
    {{ 0,  0,  0,  0,  0,  0,  0}, { 1,  2,  6,  5,  0,  0,  0}, { 1,  2, 33, 35,  0,  0,  0}, { 2,  5, 35,  6,  5, 33, 35}, { 1,  5, 48, 33,  0,  0,  0}, { 2,  2,  6, 48,  2, 48, 33}, { 2,  2, 48, 35,  2,  5, 48}, { 1,  6, 48, 35,  0,  0,  0}, { 1,  6, 35, 48,  0,  0,  0}, { 2,  2, 48,  5,  2, 35, 48}, { 2,  2, 33, 48,  2, 48,  6}, { 1,  5, 33, 48,  0,  0,  0}, { 2,  5, 35, 33,  5,  6, 35}, { 1,  2, 35, 33,  0,  0,  0}, { 1,  2,  5,  6,  0,  0,  0}, { 0,  0,  0,  0,  0,  0,  0}},
};

namespace mesh {

// flags of a node (one byte): MESH_KNOWN iff weight >= min_weight and tsdf is finite, MESH_INSIDE iff tsdf < 0
enum { KNOWN = 1, INSIDE = 2 };

DEPTH_HD int node_flags(float f, int weight, int min_weight) {
  const double v = (double)f;
  return ((weight >= min_weight && depth::is_finite(v)) ? KNOWN : 0) | (v < 0.0 ? INSIDE : 0);
}

// the case of tetrahedron T from the inside bits of the 8 corners of its cell
DEPTH_HD int tet_case(int T, int inside8) {
  return ((inside8 >> MESH_TET_CORNER[T][0]) & 1) | (((inside8 >> MESH_TET_CORNER[T][1]) & 1) << 1) |
         (((inside8 >> MESH_TET_CORNER[T][2]) & 1) << 2) | (((inside8 >> MESH_TET_CORNER[T][3]) & 1) << 3);
}

// the triangles of an active cell, 0 .. 12
DEPTH_HD int cell_triangles(int inside8) {
  int n = 0;
  for (int T = 0; T < 6; ++T) n += MESH_CASE[T][tet_case(T, inside8)][0];
  return n;
}

// the cells that contain the edge of direction d from a node, as a mask over the corners c the node can be of its cell
// (the cell is then node - offset(c)): those that share no axis with the direction
DEPTH_HD int edge_cells(int d) {
  int m = 0;
  for (int c = 0; c < 8; ++c) m |= (c & MESH_DIR_CORNER(d)) ? 0 : (1 << c);
  return m;
}

// ---- floating point ----
// where the field crosses zero between the values fa (at the owning node) and fb: the share of the way from a to b
DEPTH_HD double cut(double fa, double fb) { return fa / (fa - fb); }

DEPTH_HD double lerp(double a, double b, double t) { return a + t * (b - a); }

// one component of a node's gradient: f0 at the node, fp / fm at the next and the previous node of the axis, kp / km
// whether those are in the grid and known (fp / fm are not looked at otherwise)
DEPTH_HD double gradient(double f0, double fp, double fm, int kp, int km) {
  if (kp && km) return 0.5 * (fp - fm);
  if (kp) return fp - f0;
  if (km) return f0 - fm;
  return 0.0;
}

// the normal of a vertex from the gradients at the two ends of its edge: unit length, or zeros when it has no length
DEPTH_HD void normal(const double* gA, const double* gB, double t, float* out) {
  double n[3] = {lerp(gA[0], gB[0], t), lerp(gA[1], gB[1], t), lerp(gA[2], gB[2], t)};
  depth::normalise(n, depth::norm2(n));
  out[0] = (float)n[0]; out[1] = (float)n[1]; out[2] = (float)n[2];
}

}  // namespace mesh
