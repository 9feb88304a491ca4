// The arithmetic of the exposure compensation (mesh_exposure.hip), written so that it also compiles for the host
// (tests/native/mesh_exposure_check.cpp) and so that NumPy reproduces it operation for operation
// (tests/mesh_exposure_reference.py).  include/sfm_amd.h states the whole stage.  The sample of a vertex in a view is that of
// mesh_color_rule.h - project(), sees(), weight(), taps(), bilinear(), included and not restated - and this header adds what
// comes after it: float64 without FMA contraction and integers.
//   quantise():  q = (uint8) min(floor(s + 0.5), 255.0), the sample of one view as one byte
//   the operands of the two integer products: f = 1 where seen != 0 else 0, and the signed sample (q - 128 where seen, else 0),
//                four bytes at a time in one 32-bit word; sums = product + 128 * overlap restores the sample
//   gain():      out = (uint8) min(floor((double)I * g + 0.5), 255.0) for a finite g >= 0; the multiply and the add are two
//                roundings, which is why the contraction is off
#pragma once
#include <cmath>
#include <cstdint>

#include "mesh_color_rule.h"

#pragma clang fp contract(off)

namespace mesh_exposure {

// s is a bilinear sample of bytes: 0 <= s <= 255 and never a NaN
DEPTH_HD uint8_t quantise(double s) {
  const double r = floor(s + 0.5);
  return (uint8_t)(int)(r < 255.0 ? r : 255.0);
}

DEPTH_HD int gain_ok(double g) { return (g - g == 0.0) && (g >= 0.0); }

// one pixel value under the gain g (gain_ok): the product is rounded, then the sum
DEPTH_HD uint8_t gain(uint8_t value, double g) {
  const double p = (double)value * g;
  const double r = floor(p + 0.5);
  return (uint8_t)(int)(r < 255.0 ? r : 255.0);
}

// four flags in one word: every byte that is not 0 becomes 1
DEPTH_HD uint32_t flags01(uint32_t seen4) {
  const uint32_t nz = (((seen4 & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | seen4) & 0x80808080u;
  return nz >> 7;
}

// four samples in one word as int8: q - 128 (the top bit flipped) where the flag of flags01() is 1, else 0
DEPTH_HD uint32_t signed4(uint32_t q4, uint32_t f01) { return (q4 ^ 0x80808080u) & (f01 * 255u); }

}  // namespace mesh_exposure
