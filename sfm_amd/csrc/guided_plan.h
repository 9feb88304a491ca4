// Host-side planning of guided matching (guided.hip): the tile constants, the segment table the kernels read, the size
// checks and the carve-up of the caller's workspace.  Plain C++ without a HIP dependency, so that it can be checked on a
// CPU under the sanitizers (tests/native/guided_check.cpp).
#pragma once
#include <cstdint>
#include <vector>

constexpr int GUIDED_WAVES = 4;                       // wavefronts per workgroup
constexpr int GUIDED_QW = 8;                          // queries a wavefront walks, one at a time
constexpr int GUIDED_QT = GUIDED_WAVES * GUIDED_QW;   // queries per workgroup (one tile)
constexpr int GUIDED_CHUNK = 512;                     // points of the other image staged through LDS at a time
constexpr int GUIDED_DRAIN = 64;                      // queued candidates that trigger a drain (lane = candidate)
constexpr int GUIDED_RING = 2 * GUIDED_DRAIN;         // candidate slots per query: one drain's worth + one ballot's worth

// One image pair.  Forward pass: the rows [q_beg, q_end) of image i are the queries, [t_beg, t_end) of image j the
// candidates; the reverse pass of the cross-check swaps the two.  Record n_seg holds the totals.
struct GuidedSeg {
  int64_t q_beg, q_end, t_beg, t_end;
  int64_t out_first;        // output row of q_beg (forward results, one per query row)
  int64_t rev_first;        // row of t_beg in the reverse results (one per train row)
  int64_t tile_first;       // first workgroup of the forward pass
  int64_t rev_tile_first;   // first workgroup of the reverse pass
};

struct GuidedPlan {
  std::vector<GuidedSeg> segs;      // n_seg + 1 records
  int64_t n_out = 0, n_rev = 0, n_tiles = 0, n_rev_tiles = 0;
};

inline int64_t guided_align(int64_t v) { return (v + 255) / 256 * 256; }
inline int64_t guided_tiles(int64_t n) { return (n + GUIDED_QT - 1) / GUIDED_QT; }

// 0 when the segment table can be served, else the number of the first offending rule (for the error text)
inline int guided_check_segments(int64_t n_seg, const int64_t* q_beg, const int64_t* q_end, const int64_t* t_beg,
                                 const int64_t* t_end, int64_t n_rows) {
  if (n_seg < 0 || n_seg > 0x7FFFFFFFLL) return 1;
  if (n_rows < 0 || n_rows > 0x7FFFFF00LL) return 2;
  if (n_seg > 0 && (!q_beg || !q_end || !t_beg || !t_end)) return 3;
  for (int64_t s = 0; s < n_seg; ++s) {
    if (q_beg[s] < 0 || q_end[s] < q_beg[s] || q_end[s] > n_rows) return 4;
    if (t_beg[s] < 0 || t_end[s] < t_beg[s] || t_end[s] > n_rows) return 5;
  }
  return 0;
}

// the table of a batch that guided_check_segments has accepted
inline GuidedPlan guided_plan(int64_t n_seg, const int64_t* q_beg, const int64_t* q_end, const int64_t* t_beg, const int64_t* t_end) {
  GuidedPlan p;
  p.segs.resize((size_t)n_seg + 1);
  for (int64_t s = 0; s < n_seg; ++s) {
    GuidedSeg& r = p.segs[(size_t)s];
    r.q_beg = q_beg[s]; r.q_end = q_end[s]; r.t_beg = t_beg[s]; r.t_end = t_end[s];
    r.out_first = p.n_out; r.rev_first = p.n_rev; r.tile_first = p.n_tiles; r.rev_tile_first = p.n_rev_tiles;
    p.n_out += r.q_end - r.q_beg;
    p.n_rev += r.t_end - r.t_beg;
    p.n_tiles += guided_tiles(r.q_end - r.q_beg);
    p.n_rev_tiles += guided_tiles(r.t_end - r.t_beg);
  }
  GuidedSeg& e = p.segs[(size_t)n_seg];
  e.q_beg = e.q_end = e.t_beg = e.t_end = 0;
  e.out_first = p.n_out; e.rev_first = p.n_rev; e.tile_first = p.n_tiles; e.rev_tile_first = p.n_rev_tiles;
  return p;
}

// byte offsets into the workspace
struct GuidedLayout {
  int64_t segs;                        // GuidedSeg [n_seg + 1]
  int64_t idx1, d1, d2, ncand;         // int32 / float / float / int32 [n_out]: best, its distance, the second's, |C(q)|
  int64_t rev;                         // int32 [n_rev]: best query of every train row (cross-check)
  int64_t keep;                        // uint8 [n_out]
  int64_t blk_cnt, blk_off;            // int32 [blocks of 256 output rows + 1]: blk_off ends with the total
  int64_t bytes;
};

inline int64_t guided_blocks(int64_t n_out) { return (n_out + 255) / 256; }

inline GuidedLayout guided_layout(int64_t n_seg, int64_t n_out, int64_t n_rev) {
  GuidedLayout L;
  int64_t off = 0;
  auto take = [&](int64_t count, int64_t width) { const int64_t at = off; off += guided_align(count * width); return at; };
  L.segs = take(n_seg + 1, (int64_t)sizeof(GuidedSeg));
  L.idx1 = take(n_out, 4);
  L.d1 = take(n_out, 4);
  L.d2 = take(n_out, 4);
  L.ncand = take(n_out, 4);
  L.rev = take(n_rev, 4);
  L.keep = take(n_out, 1);
  L.blk_cnt = take(guided_blocks(n_out) + 1, 4);
  L.blk_off = take(guided_blocks(n_out) + 1, 4);
  L.bytes = off + 256;
  return L;
}

#if defined(__HIPCC__)
#define GUIDED_PLAN_HD __host__ __device__ __forceinline__
#else
#define GUIDED_PLAN_HD inline
#endif

// The segment that owns item `at` of a running count (output rows, forward tiles, reverse tiles): the last s in [0, n_seg)
// whose first item is <= at.  Segments without items share their first item with the next one and are passed over.
enum { GUIDED_BY_OUT = 0, GUIDED_BY_TILE = 1, GUIDED_BY_REV_TILE = 2 };
GUIDED_PLAN_HD int64_t guided_first(const GuidedSeg& r, int by) {
  return by == GUIDED_BY_OUT ? r.out_first : (by == GUIDED_BY_TILE ? r.tile_first : r.rev_tile_first);
}
GUIDED_PLAN_HD int guided_find(const GuidedSeg* segs, int n_seg, int64_t at, int by) {
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (guided_first(segs[mid], by) <= at) lo = mid; else hi = mid - 1;
  }
  return lo;
}
