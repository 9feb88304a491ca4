// Launch plan of decimation by vertex clustering (mesh_decimate.hip): the argument checks, the workspace layout and the
// grids.  Plain C++: it compiles for the host too (tests/native/mesh_decimate_check.cpp replays it under the sanitizers).
//
// Every kernel is one thread per vertex, per corner, per triangle, per sorted slot or per cluster, DEC_BLOCK consecutive ones
// per workgroup.  The clusters are numbered and the kept triangles are ranked with the block counts and the two-level scan
// of scan_plan.h, one 32-bit count per block.  ONE workspace serves the three calls: what a later call reads of an earlier
// one - the vertices sorted by cell, the corners sorted by cluster, the block counts of the kept triangles - stands in
// front, at offsets that depend on the two sizes only; the keys and the values in front of and behind the sorts and the
// temporary storage the sorts ask for stand behind.
#pragma once
#include <cmath>
#include <cstdint>
#include "scan_plan.h"

#if defined(__HIPCC__)
#define DEC_PLAN_HD __host__ __device__ __forceinline__
#else
#define DEC_PLAN_HD inline
#endif

#define DEC_BLOCK 256
#define DEC_WAVES (DEC_BLOCK / 64)
#define DEC_MAX_VERTICES 0x7FFFFFFFLL
#define DEC_MAX_TRIANGLES (0x7FFFFFFFLL / 3)       /* 3 n_triangles corners are numbered by an int32 */

static_assert(DEC_BLOCK == SCAN_THREADS, "a workgroup of the scan is a workgroup of the stage");
static_assert((int64_t)SCAN_CHUNK * DEC_BLOCK < 0xFFFFFFFFLL, "sums within a chunk fit 32 bits");

// counts of sfm_mesh_decimate_cluster (device int64 [2]) and of sfm_mesh_decimate_mark (device int64 [5])
enum { DEC_CLUSTERS = 0, DEC_UNSOUND_VERTICES = 1, DEC_CLUSTER_COUNTS = 2 };
enum { DEC_KEPT = 0, DEC_UNSOUND = 1, DEC_DEGENERATE = 2, DEC_DROPPED = 3, DEC_STATUS = 4, DEC_MARK_COUNTS = 5 };

DEC_PLAN_HD int64_t dec_blocks(int64_t n) { return (n + DEC_BLOCK - 1) / DEC_BLOCK; }

// the bits that hold every cluster number and leave the all-ones pattern above them: 2^bits > n_clusters, 1 .. 31
DEC_PLAN_HD int dec_cluster_bits(int64_t n_clusters) {
  int bits = 1;
  while (bits < 31 && (1ll << bits) <= n_clusters) ++bits;
  return bits;
}
// one sort of the triples when three cluster numbers fit 63 bits; two stable ones, by the largest first, otherwise
DEC_PLAN_HD int dec_triple_passes(int64_t n_clusters) { return 3 * dec_cluster_bits(n_clusters) <= 63 ? 1 : 2; }
DEC_PLAN_HD uint64_t dec_triple_key(int32_t a, int32_t b, int32_t c, int bits) {
  return ((uint64_t)a << (2 * bits)) | ((uint64_t)b << bits) | (uint64_t)c;
}
DEC_PLAN_HD uint64_t dec_pair_key(int32_t a, int32_t b) { return ((uint64_t)a << 32) | (uint64_t)b; }

// ---- argument checks: 0 = fine, otherwise an index into DEC_WHY ----
static const char* const DEC_WHY[] = {"", "n_vertices must be 0 .. 2^31 - 1 and n_triangles 0 .. (2^31 - 1) / 3", "n_clusters must be 0 .. n_vertices",
                                      "origin must be 3 finite numbers and cell a finite number > 0", "placement must be 0 (mean) or 1 (quadric)",
                                      "null pointer", "a capacity must be 0 .. 2^31 - 1", "workspace missing or too small"};

inline int dec_check_counts(int64_t n_vertices, int64_t n_triangles) {
  return (n_vertices < 0 || n_vertices > DEC_MAX_VERTICES || n_triangles < 0 || n_triangles > DEC_MAX_TRIANGLES) ? 1 : 0;
}
inline int dec_check_grid(const double* origin, double cell) {
  if (!origin) return 5;
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(origin[a])) return 3;
  return (std::isfinite(cell) && cell > 0.0) ? 0 : 3;
}
inline int dec_check_workspace(const void* workspace, int64_t have, int64_t need) { return (!workspace || have < need) ? 7 : 0; }

// sfm_mesh_decimate_cluster: the sizes, the pointers, the grid; every array but counts may be null without vertices
inline int dec_check_cluster(int64_t n_vertices, int64_t n_triangles, const void* vertices, const double* origin, double cell, const void* vertex_cluster,
                             const void* cluster_start, const void* cluster_first, const void* cluster_size, const void* counts) {
  if (dec_check_counts(n_vertices, n_triangles)) return 1;
  if (!counts || !cluster_start) return 5;
  if (n_vertices > 0 && (!vertices || !vertex_cluster || !cluster_first || !cluster_size)) return 5;
  return dec_check_grid(origin, cell);
}

// sfm_mesh_decimate_mark
inline int dec_check_mark(int64_t n_vertices, int64_t n_triangles, int64_t n_clusters, const void* triangles, const void* vertex_cluster,
                          const void* triangle_keep, const void* counts) {
  if (dec_check_counts(n_vertices, n_triangles)) return 1;
  if (n_clusters < 0 || n_clusters > n_vertices) return 2;
  if (!counts) return 5;
  if (n_triangles > 0 && (!triangles || !triangle_keep || (n_vertices > 0 && !vertex_cluster))) return 5;
  return 0;
}

// the part of sfm_mesh_decimate_emit's check in front of the early return
inline int dec_check_emit_counts(int64_t n_vertices, int64_t n_triangles, int64_t n_clusters, int64_t cap_clusters, int64_t cap_triangles, int placement,
                                 const double* origin, double cell) {
  if (dec_check_counts(n_vertices, n_triangles)) return 1;
  if (n_clusters < 0 || n_clusters > n_vertices) return 2;
  if (cap_clusters < 0 || cap_clusters > DEC_MAX_VERTICES || cap_triangles < 0 || cap_triangles > DEC_MAX_VERTICES) return 6;
  if (placement < 0 || placement > 1) return 4;
  return dec_check_grid(origin, cell);
}
// normals and new_normals may be null together: then no normal is written
inline int dec_check_emit_pointers(int64_t n_triangles, int64_t cap_clusters, int64_t cap_triangles, const void* vertices, const void* normals,
                                   const void* triangles, const void* vertex_cluster, const void* cluster_start, const void* triangle_keep,
                                   const void* new_vertices, const void* new_normals, const void* cluster_placed, const void* new_triangles,
                                   const void* triangle_map) {
  if (cap_clusters > 0 && (!vertices || !cluster_start || !new_vertices || !cluster_placed || (normals && !new_normals))) return 5;
  if (n_triangles > 0 && (cap_clusters > 0 || cap_triangles > 0) && (!triangles || !vertex_cluster)) return 5;
  if (cap_triangles > 0 && (!triangle_keep || !new_triangles || !triangle_map)) return 5;
  return 0;
}

// ---- the workspace ----
inline int64_t dec_align(int64_t v) { return (v + 255) / 256 * 256; }

// In front, kept from call to call: the vertices in (cell, index) order, the corners in (cluster, corner) order with their
// keys, the kept triangles per block and per chunk.  Behind, scratch of one call: the keys and the values of the vertex sort,
// the heads per block and per chunk, the corner sort's input, the triple sorts' keys (64-bit, and 32-bit for the first of two
// passes) and values, and the temporary storage of the sorts (sort_bytes; the device calls measure it).
struct DecLayout {
  int64_t sorted_vertex, corner_key, corner_val, tri_blk, tri_chunk;
  int64_t vkey_in, vkey_out, vval_in, vblk, vchunk, ckey_in, cval_in, tkey_in, tkey_out, tlow_in, tlow_out, tval_a, tval_b, sort, bytes;
};
inline DecLayout dec_layout(int64_t n_vertices, int64_t n_triangles, int64_t sort_bytes) {
  DecLayout L;
  const int64_t nv = n_vertices, nt = n_triangles, n = 3 * n_triangles, vb = dec_blocks(nv), tb = dec_blocks(nt);
  int64_t off = 0;
  L.sorted_vertex = off; off += dec_align(nv * 4);
  L.corner_key = off;    off += dec_align(n * 4);
  L.corner_val = off;    off += dec_align(n * 4);
  L.tri_blk = off;       off += dec_align(tb * 4);
  L.tri_chunk = off;     off += dec_align(scan_chunks(tb) * 8);
  L.vkey_in = off;       off += dec_align(nv * 8);
  L.vkey_out = off;      off += dec_align(nv * 8);
  L.vval_in = off;       off += dec_align(nv * 4);
  L.vblk = off;          off += dec_align(vb * 4);
  L.vchunk = off;        off += dec_align(scan_chunks(vb) * 8);
  L.ckey_in = off;       off += dec_align(n * 4);
  L.cval_in = off;       off += dec_align(n * 4);
  L.tkey_in = off;       off += dec_align(nt * 8);
  L.tkey_out = off;      off += dec_align(nt * 8);
  L.tlow_in = off;       off += dec_align(nt * 4);
  L.tlow_out = off;      off += dec_align(nt * 4);
  L.tval_a = off;        off += dec_align(nt * 4);
  L.tval_b = off;        off += dec_align(nt * 4);
  L.sort = off;          off += dec_align(sort_bytes);
  L.bytes = off + 256;
  return L;
}
