// The selection rule of mesh cleaning (mesh_clean.hip): which connected components of a mesh stay.  include/sfm_amd.h
// states it; integers only.  Plain C++: it compiles for the host too (tests/native/mesh_clean_check.cpp holds the cut
// against a sort under the sanitizers).
//
// A component is a candidate iff it has at least min_triangles triangles.  With keep_largest = k > 0 and more than k
// candidates the cut of the feature selection applies to the candidates' triangle counts: the size s with
// #(size > s) < k <= #(size >= s); every candidate above s stays, and of those at s the first k - #(size > s) in component
// order.  Nothing is sorted: s comes out of four passes over 8-bit histograms, most significant byte first (a radix
// select), the ties out of one more pass with a running count.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MESH_CLEAN_HD __host__ __device__ __forceinline__
#else
#define MESH_CLEAN_HD inline
#endif

#define MESH_CLEAN_RADIX_PASSES 4
#define MESH_CLEAN_RADIX_BINS 256

namespace mesh_clean {

MESH_CLEAN_HD bool sound(int32_t a, int32_t b, int32_t c, int64_t n_vertices) {
  return a >= 0 && b >= 0 && c >= 0 && a < n_vertices && b < n_vertices && c < n_vertices;
}
MESH_CLEAN_HD bool candidate(int32_t triangles, int64_t min_triangles) { return (int64_t)triangles >= min_triangles; }

// the state of the radix select: the bits of s found so far, how many of the k places are still to fill at or below them
struct Cut { uint32_t prefix; int64_t left; };

MESH_CLEAN_HD int radix_shift(int pass) { return 8 * (MESH_CLEAN_RADIX_PASSES - 1 - pass); }
// whether a size still matches the bytes found in the passes before `pass`
MESH_CLEAN_HD bool radix_match(uint32_t size, uint32_t prefix, int pass) {
  return pass == 0 || (size >> (radix_shift(pass) + 8)) == (prefix >> (radix_shift(pass) + 8));
}
MESH_CLEAN_HD int radix_bin(uint32_t size, int pass) { return (int)((size >> radix_shift(pass)) & 255u); }

// One pass: hist counts the matching candidates by their byte.  The byte of s is the largest bin b with
// #(bins > b) < left <= #(bins >= b); the places the bins above it take are filled.  The caller guarantees
// 1 <= left <= the sum of hist.
MESH_CLEAN_HD void radix_step(const int32_t* hist, int pass, Cut* cut) {
  int64_t above = 0;
  int b = MESH_CLEAN_RADIX_BINS - 1;
  for (; b > 0; --b) {
    if (above + hist[b] >= cut->left) break;
    above += hist[b];
  }
  cut->prefix |= (uint32_t)b << radix_shift(pass);
  cut->left -= above;
}

// after the last pass: prefix is s and left = k - #(size > s), the ties that stay
MESH_CLEAN_HD bool keeps(int32_t triangles, int64_t min_triangles, bool cutting, uint32_t s, int64_t ties_before, int64_t ties_kept) {
  if (!candidate(triangles, min_triangles)) return false;
  if (!cutting) return true;
  const uint32_t size = (uint32_t)triangles;
  return size > s || (size == s && ties_before < ties_kept);
}

// The whole rule in one loop nest, as the one workgroup of k_clean_select walks it; keep has n entries.  Returns the
// number of components kept.
inline int64_t select(const int32_t* triangles, int64_t n, int64_t min_triangles, int64_t keep_largest, uint8_t* keep) {
  int64_t n_cand = 0;
  for (int64_t c = 0; c < n; ++c) n_cand += candidate(triangles[c], min_triangles) ? 1 : 0;
  const bool cutting = keep_largest > 0 && n_cand > keep_largest;
  Cut cut{0u, keep_largest};
  if (cutting)
    for (int pass = 0; pass < MESH_CLEAN_RADIX_PASSES; ++pass) {
      int32_t hist[MESH_CLEAN_RADIX_BINS] = {0};
      for (int64_t c = 0; c < n; ++c)
        if (candidate(triangles[c], min_triangles) && radix_match((uint32_t)triangles[c], cut.prefix, pass)) ++hist[radix_bin((uint32_t)triangles[c], pass)];
      radix_step(hist, pass, &cut);
    }
  int64_t ties = 0, kept = 0;
  for (int64_t c = 0; c < n; ++c) {
    keep[c] = keeps(triangles[c], min_triangles, cutting, cut.prefix, ties, cut.left) ? 1 : 0;
    if (cutting && candidate(triangles[c], min_triangles) && (uint32_t)triangles[c] == cut.prefix) ++ties;
    kept += keep[c];
  }
  return kept;
}

}  // namespace mesh_clean
