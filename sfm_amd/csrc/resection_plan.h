// Host-side planning of the resection lists (resection.hip): the argument checks and the carve-up of the caller's
// workspace.  Plain C++ without a HIP dependency, so that it can be checked on a CPU under the sanitizers
// (tests/native/resection_plan_check.cpp).
#pragma once
#include <cstdint>

constexpr int RESECT_BLOCK = 256;                 // nodes per workgroup = the tile of the scan
constexpr int RESECT_WAVES = RESECT_BLOCK / 64;   // one 64-bit ballot word per wavefront

inline int64_t resect_blocks(int64_t n_nodes) { return (n_nodes + RESECT_BLOCK - 1) / RESECT_BLOCK; }

// 0 when the sizes can be served, else the number of the first offending rule (for the error text)
inline int resect_check_sizes(int64_t n_img, int64_t n_nodes, int64_t n_tracks, int64_t cap_corr) {
  if (n_img < 0 || n_nodes < 0 || n_tracks < 0 || cap_corr < 0) return 1;
  if (n_nodes >= (int64_t)1 << 31) return 2;
  if (n_nodes > 0 && n_img < 1) return 3;
  return 0;
}

struct resect_layout {
  int64_t mask;     // uint64 [blocks * RESECT_WAVES]: the ballot of the listing rule, one word per wavefront
  int64_t blk;      // int32 [blocks + 1]: listed nodes per workgroup, then their exclusive scan in place
  int64_t bytes;
};

inline int64_t resect_align(int64_t v) { return (v + 255) / 256 * 256; }

inline resect_layout resect_plan_layout(int64_t n_nodes) {
  resect_layout L;
  const int64_t blocks = resect_blocks(n_nodes);
  int64_t off = 0;
  L.mask = off; off += resect_align(blocks * RESECT_WAVES * 8);
  L.blk = off;  off += resect_align((blocks + 1) * 4);
  L.bytes = off + 256;
  return L;
}
