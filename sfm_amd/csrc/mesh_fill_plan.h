// Launch plan of the edge table and of hole filling (mesh_fill.hip): the argument checks, the two workspace layouts and the
// grids.  Plain C++: it compiles for the host too (tests/native/mesh_fill_check.cpp replays it under the sanitizers).
//
// The kernels of the table are one thread per half-edge (or per sorted slot), FILL_BLOCK consecutive ones per workgroup; the
// hole work is one wavefront per short loop, FILL_WAVES loops per workgroup.  The leaders are numbered, and the filled
// sub-loops and the fill triangles are ranked, with the block counts and the two-level scan of scan_plan.h: the table scans
// one 32-bit count per block of half-edges, the fill one packed 64-bit count per block - names of filled sub-loops in the
// low half, fill triangles in the high half - as mesh_clean_plan.h does.
#pragma once
#include <cstdint>
#include "scan_plan.h"

#if defined(__HIPCC__)
#define FILL_PLAN_HD __host__ __device__ __forceinline__
#else
#define FILL_PLAN_HD inline
#endif

#define FILL_BLOCK 256
#define FILL_WAVES (FILL_BLOCK / 64)
#define FILL_MAX_VERTICES 0x7FFFFFFFLL
#define FILL_MAX_TRIANGLES (0x7FFFFFFFLL / 3)      /* 3 n_triangles half-edges are numbered by an int32 */
#define FILL_MAX_EDGES 64

static_assert(FILL_BLOCK == SCAN_THREADS, "a workgroup of the scan is a workgroup of the stage");
static_assert((int64_t)SCAN_CHUNK * FILL_BLOCK < 0xFFFFFFFFLL, "sums within a chunk fit 32 bits");

// counts of sfm_mesh_edges (device int64 [8]) and of sfm_mesh_fill_mark (device int64 [4])
enum { EDGES_DISTINCT = 0, EDGES_BOUNDARY = 1, EDGES_INCONSISTENT = 2, EDGES_NONMANIFOLD = 3, EDGES_LOOPS = 4, EDGES_LONG = 5,
       EDGES_UNSOUND = 6, EDGES_STATUS = 7, EDGES_COUNTS = 8 };
enum { FILL_FILLED = 0, FILL_TRIANGLES = 1, FILL_OPEN = 2, FILL_STATUS = 3, FILL_COUNTS = 4 };

FILL_PLAN_HD int64_t fill_blocks(int64_t n) { return (n + FILL_BLOCK - 1) / FILL_BLOCK; }
FILL_PLAN_HD int64_t fill_loop_blocks(int64_t n_loops) { return (n_loops + FILL_WAVES - 1) / FILL_WAVES; }
// the rotation about a vertex visits each triangle of its fan once
FILL_PLAN_HD int64_t edges_budget(int64_t n_triangles) { return n_triangles + 1; }

FILL_PLAN_HD uint64_t fill_count_pack(uint32_t names, uint32_t triangles) { return (uint64_t)names | ((uint64_t)triangles << 32); }
FILL_PLAN_HD int64_t fill_name_base(const int64_t* chunk_base, const uint64_t* blk, int64_t b) {
  return scan_base(chunk_base, 2, 0, b, (int64_t)(blk[b] & 0xFFFFFFFFull));
}
FILL_PLAN_HD int64_t fill_triangle_base(const int64_t* chunk_base, const uint64_t* blk, int64_t b) {
  return scan_base(chunk_base, 2, 1, b, (int64_t)(blk[b] >> 32));
}

// ---- argument checks: 0 = fine, otherwise an index into FILL_WHY ----
static const char* const FILL_WHY[] = {"", "n_vertices must be 0 .. 2^31 - 1 and n_triangles 0 .. (2^31 - 1) / 3", "n_loops must be 0 .. n_triangles",
                                       "max_edges must be 1 .. 64", "null pointer", "a capacity must be 0 .. 2^31 - 1",
                                       "workspace missing or too small"};

inline int fill_check_counts(int64_t n_vertices, int64_t n_triangles) {
  return (n_vertices < 0 || n_vertices > FILL_MAX_VERTICES || n_triangles < 0 || n_triangles > FILL_MAX_TRIANGLES) ? 1 : 0;
}
inline int fill_check_workspace(const void* workspace, int64_t have, int64_t need) { return (!workspace || have < need) ? 6 : 0; }

// sfm_mesh_edges: every array but counts may be null without triangles
inline int edges_check(int64_t n_vertices, int64_t n_triangles, const void* triangles, const void* uses, const void* twin, const void* next,
                       const void* loop, const void* loop_leader, const void* loop_edges, const void* counts) {
  if (fill_check_counts(n_vertices, n_triangles)) return 1;
  if (!counts) return 4;
  if (n_triangles > 0 && (!triangles || !uses || !twin || !next || !loop || !loop_leader || !loop_edges)) return 4;
  return 0;
}

inline int fill_check_mark(int64_t n_vertices, int64_t n_triangles, int64_t n_loops, int64_t max_edges, const void* triangles, const void* next,
                           const void* loop_leader, const void* halfedge_fill, const void* counts) {
  if (fill_check_counts(n_vertices, n_triangles)) return 1;
  if (n_loops < 0 || n_loops > n_triangles) return 2;
  if (max_edges < 1 || max_edges > FILL_MAX_EDGES) return 3;
  if (!counts) return 4;
  if (n_triangles > 0 && (!triangles || !next || !halfedge_fill)) return 4;
  if (n_loops > 0 && !loop_leader) return 4;
  return 0;
}

// the part of sfm_mesh_fill_emit's check in front of the early return
inline int fill_check_emit_counts(int64_t n_vertices, int64_t n_triangles, int64_t n_loops, int64_t cap_fill, int64_t cap_triangles) {
  if (fill_check_counts(n_vertices, n_triangles)) return 1;
  if (n_loops < 0 || n_loops > n_triangles) return 2;
  if (cap_fill < 0 || cap_fill > FILL_MAX_VERTICES || cap_triangles < 0 || cap_triangles > FILL_MAX_VERTICES) return 5;
  return 0;
}
inline int fill_check_emit_pointers(int64_t n_vertices, int64_t n_triangles, int64_t n_loops, int64_t cap_fill, int64_t cap_triangles,
                                    const void* triangles, const void* next, const void* loop_leader, const void* halfedge_fill,
                                    const void* vertices, const void* fill_vertices, const void* fill_normals, const void* fill_name,
                                    const void* fill_triangles, const void* fill_triangle_halfedge) {
  if (n_triangles > 0 && (!triangles || !next || !halfedge_fill)) return 4;
  if (n_loops > 0 && !loop_leader) return 4;
  if (cap_fill > 0 && ((n_vertices > 0 && !vertices) || !fill_vertices || !fill_normals || !fill_name)) return 4;
  if (cap_triangles > 0 && (!fill_triangles || !fill_triangle_halfedge)) return 4;
  return 0;
}

// ---- workspaces ----
inline int64_t fill_align(int64_t v) { return (v + 255) / 256 * 256; }

// the table: the keys and the half-edges in front of and behind the sort, the leader of every half-edge, the leaders per
// block and per chunk, and the temporary storage the sort asks for (sort_bytes; the device call measures it)
struct EdgesLayout { int64_t keys_in, keys_out, vals_in, vals_out, lead, blk, chunk_base, sort, bytes; };
inline EdgesLayout edges_layout(int64_t n_triangles, int64_t sort_bytes) {
  EdgesLayout L;
  const int64_t n = 3 * n_triangles, nb = fill_blocks(n);
  int64_t off = 0;
  L.keys_in = off;    off += fill_align(n * 8);
  L.keys_out = off;   off += fill_align(n * 8);
  L.vals_in = off;    off += fill_align(n * 4);
  L.vals_out = off;   off += fill_align(n * 4);
  L.lead = off;       off += fill_align(n * 4);
  L.blk = off;        off += fill_align(nb * 4);
  L.chunk_base = off; off += fill_align(scan_chunks(nb) * 8);
  L.sort = off;       off += fill_align(sort_bytes);
  L.bytes = off + 256;
  return L;
}

// the fill: per half-edge the name of its filled sub-loop (-1: none) and the rank of the sub-loop it names, the packed
// counts of the blocks and the two sums of every chunk
struct FillLayout { int64_t sub_name, rank, blk, chunk_base, bytes; };
inline FillLayout fill_layout(int64_t n_triangles) {
  FillLayout L;
  const int64_t n = 3 * n_triangles, nb = fill_blocks(n);
  int64_t off = 0;
  L.sub_name = off;   off += fill_align(n * 4);
  L.rank = off;       off += fill_align(n * 4);
  L.blk = off;        off += fill_align(nb * 8);
  L.chunk_base = off; off += fill_align(scan_chunks(nb) * 16);
  L.bytes = off + 256;
  return L;
}
