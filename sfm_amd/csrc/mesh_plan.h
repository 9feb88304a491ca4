// Launch plan of the meshing stages (tsdf.hip, mesh.hip): the grid, the record a node leaves in the workspace, the block
// counts and their two-level exclusive scan, the workspace layouts and the argument checks.  Plain C++: it compiles for
// the host too (tests/native/mesh_check.cpp replays it under the sanitizers).
//
// Every kernel is one thread per node, x fastest, MESH_BLOCK consecutive nodes per workgroup; a cell is handled by the
// thread of its lowest node.  k_mesh_mark leaves per node one 32-bit record - the 7-bit vertex mask, the vertices of the
// block in front of the node's, the triangles of the block in front of the cell's, whether the cell is active - and per
// block one 64-bit count, vertices in the low half and triangles in the high half.  The two-level scan of scan_plan.h
// runs over the packed counts: level one (k_mesh_scan_chunks) scans both halves with one add and writes the chunk's two
// totals, level two (k_mesh_scan_top) walks each of the two (stride 2) and writes counts.  Nothing waits on another
// workgroup.
#pragma once
#include <cstdint>
#include <vector>
#include "scan_plan.h"

#if defined(__HIPCC__)
#define MESH_PLAN_HD __host__ __device__ __forceinline__
#else
#define MESH_PLAN_HD inline
#endif

#define MESH_BLOCK 256
#define MESH_MIN_DIM 2
#define MESH_MAX_DIM 1024
#define MESH_MAX_CELL_TRIANGLES 12
#define TSDF_MAX_VIEWS 65535

// the record of a node: mask in bits 0 .. 6, vertex rank in 7 .. 17, triangle rank in 18 .. 29, the cell's activity in 30
static_assert((MESH_BLOCK - 1) * 7 < (1 << 11), "the vertices in front of a node within its block fit 11 bits");
static_assert((MESH_BLOCK - 1) * MESH_MAX_CELL_TRIANGLES < (1 << 12), "the triangles in front of a cell within its block fit 12 bits");
static_assert(MESH_BLOCK == SCAN_THREADS, "a workgroup of the scan is a workgroup of the stage");
// a chunk holds at most SCAN_CHUNK * MESH_BLOCK * 12 triangles: both halves of a packed count stay below 2^32
static_assert((int64_t)SCAN_CHUNK * MESH_BLOCK * MESH_MAX_CELL_TRIANGLES < 0xFFFFFFFFLL, "sums within a chunk fit 32 bits");

MESH_PLAN_HD uint32_t mesh_record(int mask, int vrank, int trank, int active) {
  return (uint32_t)mask | ((uint32_t)vrank << 7) | ((uint32_t)trank << 18) | ((uint32_t)active << 30);
}
MESH_PLAN_HD int mesh_record_mask(uint32_t r) { return (int)(r & 127u); }
MESH_PLAN_HD int mesh_record_vrank(uint32_t r) { return (int)((r >> 7) & 2047u); }
MESH_PLAN_HD int mesh_record_trank(uint32_t r) { return (int)((r >> 18) & 4095u); }
MESH_PLAN_HD int mesh_record_active(uint32_t r) { return (int)((r >> 30) & 1u); }

MESH_PLAN_HD int64_t mesh_nodes(int nx, int ny, int nz) { return (int64_t)nx * ny * nz; }
MESH_PLAN_HD int64_t mesh_node(int i, int j, int k, int nx, int ny) { return ((int64_t)k * ny + j) * nx + i; }
MESH_PLAN_HD int64_t mesh_blocks(int64_t n_nodes) { return (n_nodes + MESH_BLOCK - 1) / MESH_BLOCK; }
MESH_PLAN_HD uint64_t mesh_count_pack(uint32_t vertices, uint32_t triangles) { return (uint64_t)vertices | ((uint64_t)triangles << 32); }
// the first vertex / triangle slot of block b; chunk_base holds two sums per chunk
MESH_PLAN_HD int64_t mesh_vertex_base(const int64_t* chunk_base, const uint64_t* blk, int64_t b) {
  return scan_base(chunk_base, 2, 0, b, (int64_t)(blk[b] & 0xFFFFFFFFull));
}
MESH_PLAN_HD int64_t mesh_triangle_base(const int64_t* chunk_base, const uint64_t* blk, int64_t b) {
  return scan_base(chunk_base, 2, 1, b, (int64_t)(blk[b] >> 32));
}

// 0 = fine; otherwise an index into MESH_WHY
inline int mesh_check_grid(int64_t nx, int64_t ny, int64_t nz) {
  if (nx < MESH_MIN_DIM || nx > MESH_MAX_DIM || ny < MESH_MIN_DIM || ny > MESH_MAX_DIM || nz < MESH_MIN_DIM || nz > MESH_MAX_DIM) return 1;
  return 0;
}
inline int mesh_check_frame(const double* origin, double voxel) {
  if (!origin) return 2;
  for (int a = 0; a < 3; ++a) if (!(origin[a] - origin[a] == 0.0)) return 3;
  if (!(voxel - voxel == 0.0) || !(voxel > 0.0)) return 4;
  return 0;
}
static const char* const MESH_WHY[] = {"", "every grid dimension must be 2 .. 1024", "null pointer", "the origin must be finite",
                                       "the voxel size must be finite and > 0", "trunc must be a number > 0", "at most 65,535 views",
                                       "negative image size", "a reference index is out of range",
                                       "a reference image is listed twice, or a negative number of views", "negative or too many images",
                                       "min_weight must be >= 0"};

struct MeshLayout { int64_t flags, record, blk, chunk_base, bytes; };

inline int64_t mesh_align(int64_t v) { return (v + 255) / 256 * 256; }
inline MeshLayout mesh_layout(int64_t n_nodes) {
  MeshLayout L;
  const int64_t nb = mesh_blocks(n_nodes);
  int64_t off = 0;
  L.flags = off;      off += mesh_align(n_nodes);
  L.record = off;     off += mesh_align(n_nodes * 4);
  L.blk = off;        off += mesh_align(nb * 8);
  L.chunk_base = off; off += mesh_align(scan_chunks(nb) * 16);
  L.bytes = off + 256;
  return L;
}

// ---- integration (tsdf.hip): the table of the views ----
struct TsdfView { int64_t out_off; int32_t h, w; };      // first element of the view's maps, their size

// heights / widths per image, ref_image per view; fills views (n_ref records) when it is not null.  0 = fine.
inline int tsdf_check_views(int64_t n_img, const int32_t* heights, const int32_t* widths, int64_t n_ref, const int32_t* ref_image,
                            TsdfView* views) {
  if (n_img < 0 || n_img > 0x7FFFFFFFLL) return 10;
  if (n_ref < 0 || n_ref > n_img) return 9;
  if (n_ref > TSDF_MAX_VIEWS) return 6;
  if (n_img > 0 && (!heights || !widths)) return 2;
  if (n_ref > 0 && !ref_image) return 2;
  for (int64_t i = 0; i < n_img; ++i) if (heights[i] < 0 || widths[i] < 0) return 7;
  int64_t off = 0;
  std::vector<char> seen((size_t)n_img, 0);
  for (int64_t r = 0; r < n_ref; ++r) {
    const int64_t ref = ref_image[r];
    if (ref < 0 || ref >= n_img) return 8;
    if (seen[(size_t)ref]) return 9;
    seen[(size_t)ref] = 1;
    if (views) views[r] = TsdfView{off, heights[ref], widths[ref]};
    off += (int64_t)heights[ref] * widths[ref];
  }
  return 0;
}
// The views of a call as the kernels of tsdf.hip, mesh_color.hip, mesh_texture.hip and mesh_exposure.hip read them: n_ref
// records and one that closes the list (out_off = n_out, no pixel); n_out the pixels of all views together.
struct ViewTable { std::vector<TsdfView> views; int64_t n_out = 0; };

// tsdf_check_views and, where it passes, the table.  0 = fine; otherwise an index into MESH_WHY.  The vector is sized before
// n_ref is checked, so an n_ref out of range gets the closing record alone.
inline int view_table_build(int64_t n_img, const int32_t* heights, const int32_t* widths, int64_t n_ref, const int32_t* ref_image, ViewTable* t) {
  t->views.assign((size_t)(n_ref > 0 && n_ref <= TSDF_MAX_VIEWS ? n_ref : 0) + 1, TsdfView{0, 0, 0});
  t->n_out = 0;
  const int bad = tsdf_check_views(n_img, heights, widths, n_ref, ref_image, t->views.data());
  if (bad) return bad;
  for (int64_t r = 0; r < n_ref; ++r) t->n_out += (int64_t)t->views[(size_t)r].h * t->views[(size_t)r].w;
  t->views[(size_t)n_ref] = TsdfView{t->n_out, 0, 0};
  return 0;
}

// the view pointers of a call whose sizes passed: keep may always be null, proj / centres without a view, depth / pixels when
// the views have no pixel
inline bool view_pointers_ok(int64_t n_ref, int64_t n_out, const void* proj, const void* centres, const void* depth, const void* pixels) {
  return !(n_ref > 0 && (!proj || !centres)) && !(n_out > 0 && (!depth || !pixels));
}

inline int tsdf_check_trunc(double trunc) { return (trunc > 0.0) ? 0 : 5; }
inline int64_t tsdf_workspace_bytes(int64_t n_ref) { return mesh_align((n_ref + 1) * (int64_t)sizeof(TsdfView)) + 256; }
