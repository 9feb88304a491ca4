// Launch plan of the mesh render (mesh_render.hip): the argument checks, the workspace and the grids.  Plain C++: it
// compiles for the host too (tests/native/mesh_render_check.cpp replays it under the sanitizers).
//
// The cameras are a table of TsdfView records (mesh_plan.h): n_cam records and one that closes the list; the outputs of
// camera c start at pixel out_off[c].  The workspace, every array 256-byte aligned:
//   count      one uint64 at byte 0: the length of the large-box list after the call
//   cameras    TsdfView [n_cam + 1]
//   keys       uint64 [n_pix]: per pixel the smallest (depth bits, triangle) so far
//   projected  double [n_cam][n_vertices][3]: u, v, q2 (q2 == 0: not usable)
//   list       uint64 [n_cam * n_triangles]: (camera << 32) | triangle of every box of more than MESH_RENDER_SMALL_BOX pixels
// Grids: k_render_clear walks the keys with a fixed stride; k_render_project and k_render_raster take one thread per
// (camera, vertex) or (camera, triangle) with the camera in blockIdx.y; k_render_raster_large takes a fixed number of
// workgroups that each walk the list with the stride of the grid, one entry to a workgroup at a time; k_render_resolve takes
// one thread per pixel of the largest image with the camera in blockIdx.y.
#pragma once
#include <cstdint>
#include "mesh_plan.h"

#define MESH_RENDER_MAX_CAMERAS 65535
#define MESH_RENDER_MAX_SIDE 32768
#define MESH_RENDER_MAX_ITEMS 0x7FFFFFFFLL           /* vertices, triangles */
#define MESH_RENDER_SMALL_BOX 64                      /* a box of more pixels goes to the list */
#define MESH_RENDER_LARGE_GROUPS 2048
#define MESH_RENDER_CLEAR_GROUPS 65536
#define MESH_RENDER_NONE 0
#define MESH_RENDER_VERTEX 1
#define MESH_RENDER_ATLAS 2

static_assert(MESH_RENDER_MAX_CAMERAS <= 65535, "the camera is blockIdx.y");
static_assert(MESH_RENDER_SMALL_BOX >= 1, "a thread walks at least one pixel");

static const char* const MESH_RENDER_WHY[] = {"", "n_cam must be 0 .. 65535", "every image side must be 0 .. 32768", "n_vertices must be 0 .. 2^31 - 1",
                                              "n_triangles must be 0 .. 2^31 - 1", "color_mode must be 0 (none), 1 (vertex colours) or 2 (atlas)",
                                              "channels must be 1 or 3", "fill must be 0 .. 255", "the atlas must be 1 .. 32768 wide and high",
                                              "workspace missing or too small", "null pointer"};

// heights / widths per camera; fills cams (n_cam + 1 records) when it is not null, the pixels of all cameras and of the
// largest.  0 = fine; otherwise an index into MESH_RENDER_WHY
inline int mesh_render_check_cameras(int64_t n_cam, const int32_t* heights, const int32_t* widths, TsdfView* cams, int64_t* n_pix, int64_t* max_pix) {
  if (n_cam < 0 || n_cam > MESH_RENDER_MAX_CAMERAS) return 1;
  if (n_cam > 0 && (!heights || !widths)) return 10;
  int64_t off = 0, most = 0;
  for (int64_t c = 0; c < n_cam; ++c) {
    if (heights[c] < 0 || heights[c] > MESH_RENDER_MAX_SIDE || widths[c] < 0 || widths[c] > MESH_RENDER_MAX_SIDE) return 2;
    if (cams) cams[c] = TsdfView{off, heights[c], widths[c]};
    const int64_t n = (int64_t)heights[c] * widths[c];
    off += n;
    most = n > most ? n : most;
  }
  if (cams) cams[n_cam] = TsdfView{off, 0, 0};
  if (n_pix) *n_pix = off;
  if (max_pix) *max_pix = most;
  return 0;
}

inline int mesh_render_check_mesh(int64_t n_vertices, int64_t n_triangles) {
  if (n_vertices < 0 || n_vertices > MESH_RENDER_MAX_ITEMS) return 3;
  if (n_triangles < 0 || n_triangles > MESH_RENDER_MAX_ITEMS) return 4;
  return 0;
}

// the atlas may have no texel only where no triangle can win a pixel
inline int mesh_render_check_color(int64_t color_mode, int64_t channels, int64_t fill, int64_t n_triangles, int64_t atlas_w, int64_t atlas_h) {
  if (color_mode != MESH_RENDER_NONE && color_mode != MESH_RENDER_VERTEX && color_mode != MESH_RENDER_ATLAS) return 5;
  if (color_mode != MESH_RENDER_NONE && channels != 1 && channels != 3) return 6;
  if (fill < 0 || fill > 255) return 7;
  if (color_mode == MESH_RENDER_ATLAS && n_triangles > 0 &&
      (atlas_w < 1 || atlas_w > MESH_RENDER_MAX_SIDE || atlas_h < 1 || atlas_h > MESH_RENDER_MAX_SIDE)) return 8;
  return 0;
}

struct MeshRenderLayout { int64_t count, cameras, keys, projected, list, list_capacity, bytes; };

inline MeshRenderLayout mesh_render_layout(int64_t n_cam, int64_t n_pix, int64_t n_vertices, int64_t n_triangles) {
  MeshRenderLayout L;
  int64_t off = 0;
  L.count = off;     off += 256;
  L.cameras = off;   off += mesh_align((n_cam + 1) * (int64_t)sizeof(TsdfView));
  L.keys = off;      off += mesh_align(n_pix * 8);
  L.projected = off; off += mesh_align(n_cam * n_vertices * 24);
  L.list_capacity = n_cam * n_triangles;
  L.list = off;      off += mesh_align(L.list_capacity * 8);
  L.bytes = off + 256;
  return L;
}

// the buffers of a call whose sizes passed: proj may be null without a camera, vertices without a vertex, triangles without
// a triangle, the outputs without a pixel; the colour source and `color` only matter when color_mode asks for them
inline int mesh_render_check_buffers(int64_t n_cam, int64_t n_pix, int64_t n_vertices, int64_t n_triangles, int64_t color_mode, int64_t needed_bytes,
                                     const void* proj, const void* vertices, const void* triangles, const void* vertex_colors, const void* uv,
                                     const void* atlas, const void* depth, const void* triangle, const void* bary, const void* color,
                                     const void* workspace, int64_t workspace_bytes) {
  if (!workspace || workspace_bytes < needed_bytes) return 9;
  if (n_cam > 0 && !proj) return 10;
  if (n_vertices > 0 && !vertices) return 10;
  if (n_triangles > 0 && !triangles) return 10;
  if (color_mode == MESH_RENDER_VERTEX && n_vertices > 0 && !vertex_colors) return 10;
  if (color_mode == MESH_RENDER_ATLAS && n_triangles > 0 && (!uv || !atlas)) return 10;
  if (n_pix > 0 && (!depth || !triangle || !bary)) return 10;
  if (n_pix > 0 && color_mode != MESH_RENDER_NONE && !color) return 10;
  return 0;
}

inline int64_t mesh_render_blocks(int64_t n) { return (n + MESH_BLOCK - 1) / MESH_BLOCK; }
inline int64_t mesh_render_clear_groups(int64_t n_pix) {
  const int64_t b = mesh_render_blocks(n_pix);
  return b < 1 ? 1 : (b > MESH_RENDER_CLEAR_GROUPS ? MESH_RENDER_CLEAR_GROUPS : b);
}
