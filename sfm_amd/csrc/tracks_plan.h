// Host-side planning of the track builder (tracks.hip): the short / long route of a component, the argument checks and
// the carve-up of the caller's workspace.  Plain C++ without a HIP dependency, so that it can be checked on a CPU under
// the sanitizers (tests/native/tracks_plan_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define TRACKS_HD __host__ __device__ __forceinline__
#else
#define TRACKS_HD inline
#endif

constexpr int TRACKS_SHORT_MAX = 32;       // up to here one lane sorts a component in place (insertion sort)
constexpr int TRACKS_LDS_MAX = 4096;       // up to here a workgroup sorts a long component in LDS, beyond it in global memory
constexpr int TRACKS_LONG_GRID = 1024;     // workgroups that share the list of long components
constexpr int TRACKS_POLICY_DROP = 0, TRACKS_POLICY_KEEP = 1;

// counters of one call (int64 words at the start of the workspace, zeroed by k_tracks_init)
enum { TRACKS_CTR_CAND = 0, TRACKS_CTR_CAND_OBS = 1, TRACKS_CTR_LONG = 2, TRACKS_CTR_KEPT = 3, TRACKS_CTR_KEPT_OBS = 4,
       TRACKS_CTR_COUNT = 8 };

enum { TRACKS_ROUTE_LANE = 0, TRACKS_ROUTE_LDS = 1, TRACKS_ROUTE_GLOBAL = 2 };
inline int tracks_route(int64_t len) {
  return len <= TRACKS_SHORT_MAX ? TRACKS_ROUTE_LANE : (len <= TRACKS_LDS_MAX ? TRACKS_ROUTE_LDS : TRACKS_ROUTE_GLOBAL);
}

// The sorting network of a long component over a[0, len), len arbitrary.  Every comparator (i, j), i < j, puts its minimum
// at i: the first step of the merge of blocks of 2^lk pairs i with the mirror position of its block, the steps after it
// pair i with i + 2^ld for ld = lk - 2 ... 0.  With all comparators in one direction the slots from len up to the next
// power of two can be taken as +infinity that never moves, so a comparator with j >= len is skipped.
// tracks_bitonic_levels: the lp >= 1 with 2^lp >= len; each step has 2^(lp-1) comparators t.
TRACKS_HD unsigned tracks_bitonic_levels(unsigned len) {
  unsigned lp = 1;
  while ((1u << lp) < len) ++lp;
  return lp;
}
TRACKS_HD void tracks_bitonic_mirror(unsigned t, unsigned lk, unsigned& i, unsigned& j) {
  const unsigned blk = t >> (lk - 1), o = t & ((1u << (lk - 1)) - 1);
  i = (blk << lk) + o;
  j = (blk << lk) + ((1u << lk) - 1 - o);
}
TRACKS_HD void tracks_bitonic_step(unsigned t, unsigned ld, unsigned& i, unsigned& j) {
  i = ((t >> ld) << (ld + 1)) + (t & ((1u << ld) - 1));
  j = i + (1u << ld);
}

// bounds of the outputs: a track has at least two nodes, an observation is one node
inline int64_t tracks_cap_tracks(int64_t n_nodes) { return n_nodes / 2; }
inline int64_t tracks_cap_obs(int64_t n_nodes) { return n_nodes; }
// a long component has more than TRACKS_SHORT_MAX nodes
inline int64_t tracks_cap_long(int64_t n_nodes) { return n_nodes / (TRACKS_SHORT_MAX + 1) + 1; }
inline int64_t tracks_scan_blocks(int64_t n_nodes) { return (n_nodes + 255) / 256; }

// 0 when the sizes can be served, else the number of the first offending rule (for the error text)
inline int tracks_check_sizes(int64_t n_img, int64_t n_nodes, int64_t n_seg, int64_t n_edges, int64_t min_len, int64_t policy,
                              int64_t cap_tracks, int64_t cap_obs) {
  if (n_img < 0 || n_seg < 0 || n_edges < 0 || n_nodes < 0) return 1;
  if (n_nodes >= (int64_t)1 << 31) return 2;
  if (min_len < 2) return 3;
  if (policy != TRACKS_POLICY_DROP && policy != TRACKS_POLICY_KEEP) return 4;
  if (cap_tracks < tracks_cap_tracks(n_nodes) || cap_obs < tracks_cap_obs(n_nodes)) return 5;
  if (n_nodes > 0 && n_img < 1) return 6;
  return 0;
}

struct tracks_layout {
  int64_t ctr;                                                       // int64 [TRACKS_CTR_COUNT]
  int64_t parent, label, size, cidx, members;                        // int32 [n_nodes]
  int64_t cand_root, cand_off, cand_len, cand_cur, cand_conf, cand_tid, cand_obs;   // int32 [cap_tracks + 1]
  int64_t long_list;                                                 // int32 [cap_long]
  int64_t blk_a, blk_b;                                              // int32 [scan_blocks]
  int64_t bytes;
};

inline int64_t tracks_align(int64_t v) { return (v + 255) / 256 * 256; }

inline tracks_layout tracks_plan_layout(int64_t n_nodes) {
  tracks_layout L;
  int64_t off = 0;
  auto take = [&](int64_t count, int64_t width) { const int64_t at = off; off += tracks_align(count * width); return at; };
  const int64_t cand = tracks_cap_tracks(n_nodes) + 1;
  L.ctr = take(TRACKS_CTR_COUNT, 8);
  L.parent = take(n_nodes, 4);
  L.label = take(n_nodes, 4);
  L.size = take(n_nodes, 4);
  L.cidx = take(n_nodes, 4);
  L.members = take(n_nodes, 4);
  L.cand_root = take(cand, 4);
  L.cand_off = take(cand, 4);
  L.cand_len = take(cand, 4);
  L.cand_cur = take(cand, 4);
  L.cand_conf = take(cand, 4);
  L.cand_tid = take(cand, 4);
  L.cand_obs = take(cand, 4);
  L.long_list = take(tracks_cap_long(n_nodes), 4);
  L.blk_a = take(tracks_scan_blocks(n_nodes) + 1, 4);
  L.blk_b = take(tracks_scan_blocks(n_nodes) + 1, 4);
  L.bytes = off + 256;
  return L;
}
