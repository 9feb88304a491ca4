// Launch plan of the mesh texture (mesh_texture.hip): the size of the atlas, the argument checks, the workspace and the
// grid.  Plain C++: it compiles for the host too (tests/native/mesh_texture_check.cpp replays it under the sanitizers).
//
// One thread per texel of the H x W atlas over tiles of MESH_TEXTURE_TILE_X x MESH_TEXTURE_TILE_Y texels; a tile is one
// wavefront wide, so a wavefront stores one contiguous piece of one row.  The uv of the corners take one thread per
// triangle, MESH_BLOCK per workgroup.  The views and the workspace are those of the colouring (mesh_color_plan.h).
#pragma once
#include <cstdint>
#include "mesh_color_plan.h"

// the views a thread takes before it consumes the first of them (1 is the plain loop, kept here: with a thread per texel
// the launch fills the machine and the registers of four views at a time cost more waves than their round trips save;
// tools/experiments/README.md has both figures)
#define MESH_TEXTURE_BATCH 1
#define MESH_TEXTURE_TILE_X 64
#define MESH_TEXTURE_TILE_Y 4
#define MESH_TEXTURE_MAX_TEXELS 64
#define MESH_TEXTURE_MAX_SIDE 32768
#define MESH_TEXTURE_MAX_TRIANGLES 0x7FFFFFFFLL

static_assert(MESH_TEXTURE_TILE_X % 64 == 0, "a tile is a whole number of wavefronts wide");
static_assert(MESH_TEXTURE_TILE_X * MESH_TEXTURE_TILE_Y == MESH_BLOCK, "a tile is a workgroup");

static const char* const MESH_TEXTURE_WHY[] = {"", "texels must be 1 .. 64", "cells_per_row must be >= 1", "the atlas must be at most 32768 wide and high",
                                               "n_triangles must be 0 .. 2^31 - 1", "workspace missing or too small", "null pointer"};

// the atlas of n_triangles patches: 0 = fine and *width / *height are set; otherwise an index into MESH_TEXTURE_WHY
inline int mesh_texture_size(int64_t n_triangles, int64_t texels, int64_t cells_per_row, int32_t* width, int32_t* height) {
  if (texels < 1 || texels > MESH_TEXTURE_MAX_TEXELS) return 1;
  if (n_triangles < 0 || n_triangles > MESH_TEXTURE_MAX_TRIANGLES) return 4;
  if (cells_per_row < 1) return 2;
  if (cells_per_row > MESH_TEXTURE_MAX_SIDE) return 3;
  const int64_t P = texels + 3, cells = (n_triangles + 1) / 2, rows = (cells + cells_per_row - 1) / cells_per_row;
  const int64_t W = cells_per_row * P, H = rows * P;
  if (W > MESH_TEXTURE_MAX_SIDE || H > MESH_TEXTURE_MAX_SIDE) return 3;
  if (width) *width = (int32_t)W;
  if (height) *height = (int32_t)H;
  return 0;
}

inline int64_t mesh_texture_workspace_bytes(int64_t n_ref) { return mesh_color_workspace_bytes(n_ref); }

// the buffers of a call whose sizes passed: keep may always be null, depth / pixels when the views have no pixel, vertices /
// normals when there is no vertex (every triangle then has a bad index), triangles and the outputs when there is no triangle
inline int mesh_texture_check_buffers(int64_t n_ref, int64_t n_out, int64_t n_vertices, int64_t n_triangles, const void* proj, const void* centres,
                                      const void* depth, const void* pixels, const void* vertices, const void* normals, const void* triangles,
                                      const void* texture, const void* views, const void* uv, const void* workspace, int64_t workspace_bytes) {
  if (!workspace || workspace_bytes < mesh_texture_workspace_bytes(n_ref)) return 5;
  if (!view_pointers_ok(n_ref, n_out, proj, centres, depth, pixels)) return 6;
  if (n_vertices > 0 && (!vertices || !normals)) return 6;
  if (n_triangles > 0 && (!triangles || !texture || !views || !uv)) return 6;
  return 0;
}

inline int64_t mesh_texture_tiles_x(int64_t W) { return (W + MESH_TEXTURE_TILE_X - 1) / MESH_TEXTURE_TILE_X; }
inline int64_t mesh_texture_tiles_y(int64_t H) { return (H + MESH_TEXTURE_TILE_Y - 1) / MESH_TEXTURE_TILE_Y; }
inline int64_t mesh_texture_uv_blocks(int64_t n_triangles) { return (n_triangles + MESH_BLOCK - 1) / MESH_BLOCK; }
