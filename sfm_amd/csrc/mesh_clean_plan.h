// Launch plan of the component labelling and the cleaning of a mesh (mesh_clean.hip): the argument checks, the two
// workspace layouts and the grids.  Plain C++: it compiles for the host too (tests/native/mesh_clean_check.cpp replays
// it under the sanitizers).
//
// Every kernel but the selection is one thread per vertex or per triangle, CLEAN_BLOCK consecutive ones per workgroup.
// The roots are numbered and the kept vertices and triangles are ranked with the block counts and the two-level scan of
// scan_plan.h: the labelling scans one 32-bit count per block of vertices (the roots), the cleaning one packed 64-bit
// count per block - kept vertices in the low half, kept triangles in the high half, block b of either - as mesh.hip does.
#pragma once
#include <cstdint>
#include "scan_plan.h"

#if defined(__HIPCC__)
#define CLEAN_PLAN_HD __host__ __device__ __forceinline__
#else
#define CLEAN_PLAN_HD inline
#endif

#define CLEAN_BLOCK 256
#define CLEAN_MAX_COUNT 0x7FFFFFFFLL
#define CLEAN_GATHER_MAX_BLOCKS (1 << 20)

static_assert(CLEAN_BLOCK == SCAN_THREADS, "a workgroup of the scan is a workgroup of the stage");
static_assert((int64_t)SCAN_CHUNK * CLEAN_BLOCK < 0xFFFFFFFFLL, "sums within a chunk fit 32 bits");

// counts of sfm_mesh_components (device int64 [3]) and of sfm_mesh_clean_mark (device int64 [3])
enum { CC_COMPONENTS = 0, CC_UNSOUND = 1, CC_STATUS = 2, CC_COUNTS = 3 };
enum { CLEAN_COMPONENTS = 0, CLEAN_VERTICES = 1, CLEAN_TRIANGLES = 2, CLEAN_COUNTS = 3 };

CLEAN_PLAN_HD int64_t clean_blocks(int64_t n) { return (n + CLEAN_BLOCK - 1) / CLEAN_BLOCK; }
CLEAN_PLAN_HD int64_t clean_max(int64_t a, int64_t b) { return a > b ? a : b; }
// a walk towards a root lowers its node at every step, so n_vertices steps end it; the budget is four times that and
// only guards against a defect
CLEAN_PLAN_HD int64_t cc_budget(int64_t n_vertices) { return 4 * n_vertices + 1024; }

CLEAN_PLAN_HD uint64_t clean_count_pack(uint32_t vertices, uint32_t triangles) { return (uint64_t)vertices | ((uint64_t)triangles << 32); }
CLEAN_PLAN_HD int64_t clean_vertex_base(const int64_t* chunk_base, const uint64_t* blk, int64_t b) {
  return scan_base(chunk_base, 2, 0, b, (int64_t)(blk[b] & 0xFFFFFFFFull));
}
CLEAN_PLAN_HD int64_t clean_triangle_base(const int64_t* chunk_base, const uint64_t* blk, int64_t b) {
  return scan_base(chunk_base, 2, 1, b, (int64_t)(blk[b] >> 32));
}

// ---- argument checks: 0 = fine, otherwise an index into CLEAN_WHY ----
static const char* const CLEAN_WHY[] = {"", "n_vertices and n_triangles must be 0 .. 2^31 - 1", "n_components must be 0 .. n_vertices",
                                        "min_triangles and keep_largest must be >= 0", "null pointer", "a capacity must be 0 .. 2^31 - 1",
                                        "row_bytes must be >= 1", "n must be 0 .. 2^31 - 1", "workspace missing or too small"};

inline int clean_check_counts(int64_t n_vertices, int64_t n_triangles) {
  return (n_vertices < 0 || n_vertices > CLEAN_MAX_COUNT || n_triangles < 0 || n_triangles > CLEAN_MAX_COUNT) ? 1 : 0;
}
inline int clean_check_workspace(const void* workspace, int64_t have, int64_t need) { return (!workspace || have < need) ? 8 : 0;  }

// sfm_mesh_components: triangles may be null without triangles, the per-vertex outputs without vertices
inline int cc_check(int64_t n_vertices, int64_t n_triangles, const void* triangles, const void* vertex_component, const void* triangle_component,
                    const void* comp_root, const void* comp_vertices, const void* comp_triangles, const void* counts) {
  if (clean_check_counts(n_vertices, n_triangles)) return 1;
  if (!counts) return 4;
  if (n_triangles > 0 && (!triangles || !triangle_component)) return 4;
  if (n_vertices > 0 && (!vertex_component || !comp_root || !comp_vertices || !comp_triangles)) return 4;
  return 0;
}

inline int clean_check_mark(int64_t n_vertices, int64_t n_triangles, int64_t n_components, int64_t min_triangles, int64_t keep_largest,
                            const void* vertex_component, const void* triangle_component, const void* comp_triangles, const void* comp_keep,
                            const void* counts) {
  if (clean_check_counts(n_vertices, n_triangles)) return 1;
  if (n_components < 0 || n_components > n_vertices) return 2;
  if (min_triangles < 0 || keep_largest < 0) return 3;
  if (!counts) return 4;
  if (n_vertices > 0 && !vertex_component) return 4;
  if (n_triangles > 0 && !triangle_component) return 4;
  if (n_components > 0 && (!comp_triangles || !comp_keep)) return 4;
  return 0;
}

// the part of sfm_mesh_clean_emit's check in front of the early return
inline int clean_check_emit_counts(int64_t n_vertices, int64_t n_triangles, int64_t n_components, int64_t cap_vertices, int64_t cap_triangles) {
  if (clean_check_counts(n_vertices, n_triangles)) return 1;
  if (n_components < 0 || n_components > n_vertices) return 2;
  if (cap_vertices < 0 || cap_vertices > CLEAN_MAX_COUNT || cap_triangles < 0 || cap_triangles > CLEAN_MAX_COUNT) return 5;
  return 0;
}
inline int clean_check_emit_pointers(int64_t n_vertices, int64_t n_triangles, int64_t n_components, int64_t cap_vertices, int64_t cap_triangles,
                                     const void* vertex_component, const void* triangle_component, const void* comp_keep, const void* triangles,
                                     const void* vertices, const void* normals, const void* vertex_map, const void* triangle_map,
                                     const void* triangles_out, const void* vertices_out, const void* normals_out) {
  if (n_vertices > 0 && !vertex_component) return 4;
  if (n_triangles > 0 && (!triangle_component || !triangles)) return 4;
  if (n_components > 0 && !comp_keep) return 4;
  if (cap_vertices > 0 && (!vertices || !normals || !vertex_map || !vertices_out || !normals_out)) return 4;
  if (cap_triangles > 0 && (!triangle_map || !triangles_out)) return 4;
  return 0;
}

inline int clean_check_gather(int64_t row_bytes, int64_t n, const void* src, const void* map, const void* dst) {
  if (row_bytes < 1) return 6;
  if (n < 0 || n > CLEAN_MAX_COUNT) return 7;
  if (n > 0 && (!src || !map || !dst)) return 4;
  return 0;
}

// ---- workspaces ----
inline int64_t clean_align(int64_t v) { return (v + 255) / 256 * 256; }

// labelling: the parent of every vertex, the component number of every root, the roots per block and per chunk
struct CcLayout { int64_t parent, number, blk, chunk_base, bytes; };
inline CcLayout cc_layout(int64_t n_vertices) {
  CcLayout L;
  const int64_t nb = clean_blocks(n_vertices);
  int64_t off = 0;
  L.parent = off;     off += clean_align(n_vertices * 4);
  L.number = off;     off += clean_align(n_vertices * 4);
  L.blk = off;        off += clean_align(nb * 4);
  L.chunk_base = off; off += clean_align(scan_chunks(nb) * 8);
  L.bytes = off + 256;
  return L;
}

// cleaning: the state of the selection (CLEAN_SEL_WORDS int64), the new index of every vertex, the packed counts of the
// blocks and the two sums of every chunk
#define CLEAN_SEL_WORDS 4
struct CleanLayout { int64_t sel, new_index, blk, chunk_base, bytes; };
inline int64_t clean_scan_blocks(int64_t n_vertices, int64_t n_triangles) { return clean_blocks(clean_max(n_vertices, n_triangles)); }
inline CleanLayout clean_layout(int64_t n_vertices, int64_t n_triangles) {
  CleanLayout L;
  const int64_t nb = clean_scan_blocks(n_vertices, n_triangles);
  int64_t off = 0;
  L.sel = off;        off += clean_align(CLEAN_SEL_WORDS * 8);
  L.new_index = off;  off += clean_align(n_vertices * 4);
  L.blk = off;        off += clean_align(nb * 8);
  L.chunk_base = off; off += clean_align(scan_chunks(nb) * 16);
  L.bytes = off + 256;
  return L;
}

// ---- sfm_mesh_gather_rows: the unit a thread copies and the grid ----
// 16, 8 or 4 bytes when the row length and both addresses allow it, else 1
inline int clean_gather_unit(int64_t row_bytes, uintptr_t src, uintptr_t dst) {
  for (int u = 16; u > 1; u >>= 1)
    if (u != 2 && row_bytes % u == 0 && src % u == 0 && dst % u == 0) return u;
  return 1;
}
// the workgroups of a grid-stride loop over `items`
inline int64_t clean_gather_blocks(int64_t items) {
  const int64_t nb = clean_blocks(items);
  return nb > CLEAN_GATHER_MAX_BLOCKS ? CLEAN_GATHER_MAX_BLOCKS : nb;
}
