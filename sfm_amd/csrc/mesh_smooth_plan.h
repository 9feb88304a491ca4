// Launch plan of the vertex adjacency, the smoothing steps and the vertex normals (mesh_smooth.hip): the argument checks, the
// workspace layouts and the grids.  Plain C++: it compiles for the host too (tests/native/mesh_smooth_check.cpp replays it
// under the sanitizers).
//
// Every kernel is one thread per half-edge, per sorted slot, per corner or per vertex, SMO_BLOCK consecutive ones per
// workgroup.  The entries of the adjacency are ranked with the block counts and the two-level scan of scan_plan.h, one 32-bit
// count per block.  Each of the three calls has a workspace of its own; nothing in one is read by another call.
#pragma once
#include <cmath>
#include <cstdint>
#include "scan_plan.h"

#if defined(__HIPCC__)
#define SMO_PLAN_HD __host__ __device__ __forceinline__
#else
#define SMO_PLAN_HD inline
#endif

#define SMO_BLOCK 256
#define SMO_WAVES (SMO_BLOCK / 64)
#define SMO_MAX_VERTICES 0x7FFFFFFFLL
#define SMO_MAX_TRIANGLES (0x7FFFFFFFLL / 6)       /* 6 n_triangles entries are numbered by an int32 */
#define SMO_MAX_ITERATIONS 1000

static_assert(SMO_BLOCK == SCAN_THREADS, "a workgroup of the scan is a workgroup of the stage");
static_assert((int64_t)SCAN_CHUNK * SMO_BLOCK < 0xFFFFFFFFLL, "sums within a chunk fit 32 bits");

// counts of sfm_mesh_adjacency (device int64 [4]) and of sfm_mesh_smooth (device int64 [5])
enum { ADJ_ENTRIES = 0, ADJ_BOUNDARY = 1, ADJ_ISOLATED = 2, ADJ_UNSOUND = 3, ADJ_COUNTS = 4 };
enum { SMO_PINNED_BOUNDARY = 0, SMO_PINNED_GIVEN = 1, SMO_UNSOUND = 2, SMO_ISOLATED = 3, SMO_STATUS = 4, SMO_COUNTS = 5 };

SMO_PLAN_HD int64_t smo_blocks(int64_t n) { return (n + SMO_BLOCK - 1) / SMO_BLOCK; }

// the bits that hold every vertex index and leave the all-ones pattern above them: 2^bits > n_vertices, 1 .. 31
SMO_PLAN_HD int smo_vertex_bits(int64_t n_vertices) {
  int bits = 1;
  while (bits < 31 && (1ll << bits) <= n_vertices) ++bits;
  return bits;
}
// the bits of an entry's key that the sort walks: the neighbour's 32 and the vertex's above them
SMO_PLAN_HD int smo_key_bits(int64_t n_vertices) { return 32 + smo_vertex_bits(n_vertices); }

// The steps of one call and where step i of them writes: 1 the caller's vertices_out, 0 the workspace.  The last step
// writes vertices_out, the ones in front of it alternate, and step i reads what step i - 1 wrote (step 0 the input).
SMO_PLAN_HD int64_t smo_steps(int64_t iterations, int has_mu) { return iterations * (has_mu ? 2 : 1); }
SMO_PLAN_HD int smo_step_writes_out(int64_t n_steps, int64_t i) { return (int)((n_steps - i) & 1); }
// the factor of step i: lam, then mu when there is one
SMO_PLAN_HD double smo_step_factor(int64_t i, double lam, double mu, int has_mu) { return (has_mu && (i & 1)) ? mu : lam; }

// ---- argument checks: 0 = fine, otherwise an index into SMO_WHY ----
static const char* const SMO_WHY[] = {"", "n_vertices must be 0 .. 2^31 - 1 and n_triangles 0 .. (2^31 - 1) / 6", "null pointer", "iterations must be 0 .. 1000",
                                      "lam must be finite with 0 < lam <= 1", "mu must be finite with -2 <= mu < -lam", "n_index must be 0 .. 2^31 - 1",
                                      "vertices_out must not be vertices_in", "workspace missing or too small"};

inline int smo_check_counts(int64_t n_vertices, int64_t n_triangles) {
  return (n_vertices < 0 || n_vertices > SMO_MAX_VERTICES || n_triangles < 0 || n_triangles > SMO_MAX_TRIANGLES) ? 1 : 0;
}
inline int smo_check_workspace(const void* workspace, int64_t have, int64_t need) { return (!workspace || have < need) ? 8 : 0; }

// sfm_mesh_adjacency: ptr, vertex_flags and counts always (ptr has n_vertices + 1 elements); triangles and index with triangles
inline int smo_check_adjacency(int64_t n_vertices, int64_t n_triangles, const void* triangles, const void* ptr, const void* index, const void* vertex_flags,
                               const void* counts) {
  if (smo_check_counts(n_vertices, n_triangles)) return 1;
  if (!counts || !ptr) return 2;
  if (n_vertices > 0 && !vertex_flags) return 2;
  if (n_triangles > 0 && (!triangles || !index)) return 2;
  return 0;
}

// sfm_mesh_smooth: the sizes, the scalars, the pointers; pinned may be null, index may be null without entries
inline int smo_check_smooth(int64_t n_vertices, int64_t n_index, int64_t iterations, double lam, double mu, int has_mu, const void* vertices_in,
                            const void* ptr, const void* index, const void* vertex_flags, const void* vertices_out, const void* vertex_state,
                            const void* counts) {
  if (smo_check_counts(n_vertices, 0)) return 1;
  if (n_index < 0 || n_index > SMO_MAX_VERTICES) return 6;
  if (iterations < 0 || iterations > SMO_MAX_ITERATIONS) return 3;
  if (!(std::isfinite(lam) && lam > 0.0 && lam <= 1.0)) return 4;
  if (has_mu && !(std::isfinite(mu) && mu >= -2.0 && mu < -lam)) return 5;
  if (!counts || !ptr) return 2;
  if (n_vertices > 0 && (!vertices_in || !vertex_flags || !vertices_out || !vertex_state)) return 2;
  if (n_index > 0 && !index) return 2;
  if (n_vertices > 0 && vertices_in == vertices_out) return 7;
  return 0;
}

// sfm_mesh_vertex_normals
inline int smo_check_normals(int64_t n_vertices, int64_t n_triangles, const void* vertices, const void* triangles, const void* normals) {
  if (smo_check_counts(n_vertices, n_triangles)) return 1;
  if (n_vertices > 0 && (!vertices || !normals)) return 2;
  if (n_triangles > 0 && !triangles) return 2;
  return 0;
}

// ---- the workspaces ----
inline int64_t smo_align(int64_t v) { return (v + 255) / 256 * 256; }

// sfm_mesh_adjacency: the 6 n_triangles keys in front of the sort - the compacted keys of the entries afterwards, the sort
// does not touch its input -, the sorted keys, the uses of every entry, the heads per block and per chunk, and the temporary
// storage of the sort (sort_bytes; the device call measures it)
struct AdjLayout { int64_t key_in, key_out, uses, blk, chunk, sort, bytes; };
inline AdjLayout adj_layout(int64_t n_triangles, int64_t sort_bytes) {
  AdjLayout L;
  const int64_t n = 6 * n_triangles, nb = smo_blocks(n);
  int64_t off = 0;
  L.key_in = off;  off += smo_align(n * 8);
  L.key_out = off; off += smo_align(n * 8);
  L.uses = off;    off += smo_align(n * 4);
  L.blk = off;     off += smo_align(nb * 4);
  L.chunk = off;   off += smo_align(scan_chunks(nb) * 8);
  L.sort = off;    off += smo_align(sort_bytes);
  L.bytes = off + 256;
  return L;
}

// sfm_mesh_smooth: the second buffer of the Jacobi steps, float64 [n_vertices, 3]
inline int64_t smo_layout_bytes(int64_t n_vertices) { return smo_align(n_vertices * 24) + 256; }

// sfm_mesh_vertex_normals: the 3 n_triangles (vertex, corner) pairs in front of and behind the sort and its temporary storage
struct NrmLayout { int64_t key_in, key_out, val_in, val_out, sort, bytes; };
inline NrmLayout nrm_layout(int64_t n_triangles, int64_t sort_bytes) {
  NrmLayout L;
  const int64_t n = 3 * n_triangles;
  int64_t off = 0;
  L.key_in = off;  off += smo_align(n * 4);
  L.key_out = off; off += smo_align(n * 4);
  L.val_in = off;  off += smo_align(n * 4);
  L.val_out = off; off += smo_align(n * 4);
  L.sort = off;    off += smo_align(sort_bytes);
  L.bytes = off + 256;
  return L;
}
