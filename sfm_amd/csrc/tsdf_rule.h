// The per-node rule of the TSDF integration (tsdf.hip), written so that it also compiles for the host
// (tests/native/mesh_check.cpp) and so that NumPy reproduces it operation for operation (tests/mesh_reference.py).
// include/sfm_amd.h states the whole stage; this header holds its floating point: float64 without FMA contraction.
//
// Projection of the node X into a view with proj = [P | p] (row-major 3 x 4) and w x h pixels:
//   q_i = ((P_i0 * X0 + P_i1 * X1) + P_i2 * X2) + p_i      u = q0 / q2      v = q1 / q2
//   validity and the nearest pixel are those of depth::sample (depth_rule.h): q2 > 0, the half-open bounds, floor(u + 0.5)
//   with the cut to the last pixel.
// Term of a view: sdf = ds - q2 with ds the float32 depth at the pixel widened; skipped when sdf < -trunc, otherwise
//   acc = acc + (sdf < trunc ? sdf : trunc) / trunc.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "depth_rule.h"

#pragma clang fp contract(off)

#define TSDF_UNKNOWN_BITS 0x7FC00000u        /* the tsdf of a node that no view saw: this quiet NaN, bit for bit */

namespace tsdf {

struct Projection { int valid, xi, yi; double q2; };

DEPTH_HD Projection project(const double* P, double X0, double X1, double X2, int w, int h) {
  const double q0 = ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[3];
  const double q1 = ((P[4] * X0 + P[5] * X1) + P[6] * X2) + P[7];
  const double q2 = ((P[8] * X0 + P[9] * X1) + P[10] * X2) + P[11];
  const double u = q0 / q2, v = q1 / q2;
  Projection s;
  s.q2 = q2;
  s.valid = (q2 > 0.0) && (u >= -0.5) && (u < (double)w - 0.5) && (v >= -0.5) && (v < (double)h - 0.5);
  s.xi = 0; s.yi = 0;
  if (s.valid) {
    const int xi = (int)floor(u + 0.5), yi = (int)floor(v + 0.5);
    s.xi = xi < w - 1 ? xi : w - 1;
    s.yi = yi < h - 1 ? yi : h - 1;
  }
  return s;
}

// coordinate `index` of a grid axis that starts at o with nodes s apart
DEPTH_HD double node_coord(double o, double s, int index) { return o + s * (double)index; }

// one view's share of a node: ds the depth at the pixel (float32 widened), kept its keep flag, q2 the node's depth in the
// view.  Returns 1 and adds to *acc when the view counts.
DEPTH_HD int add_view(double ds, int kept, double q2, double trunc, double* acc) {
  if (!depth::is_finite(ds) || !kept) return 0;
  const double sdf = ds - q2;
  if (sdf < -trunc) return 0;
  *acc = *acc + (sdf < trunc ? sdf : trunc) / trunc;
  return 1;
}

// the bits of the node's tsdf from the sum and the number of the views that counted
DEPTH_HD uint32_t finish_bits(double acc, int w) {
  if (w == 0) return TSDF_UNKNOWN_BITS;
  const float f = (float)(acc / (double)w);
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}

}  // namespace tsdf
