// Launch plan of the mesh colouring (mesh_color.hip): the argument checks, the workspace and the launch size.  Plain C++: it
// compiles for the host too (tests/native/mesh_color_check.cpp replays it under the sanitizers).
//
// One thread per vertex, MESH_BLOCK consecutive vertices per workgroup.  The views are those of the integration: the table
// of TsdfView records (mesh_plan.h, tsdf_check_views) at the start of the workspace, n_ref records and one that closes the
// list.  The pixels of view r start at channels * out_off[r].
#pragma once
#include <cstdint>
#include "mesh_plan.h"

// the views a thread projects, and whose depths and pixels it asks for, before it consumes the first of them (1 is the
// plain loop; tools/experiments/README.md has both figures)
#define MESH_COLOR_BATCH 4
#define MESH_COLOR_MAX_VERTICES 0x7FFFFFFFLL

static const char* const MESH_COLOR_WHY[] = {"", "channels must be 1 or 3", "n_vertices must be 0 .. 2^31 - 1", "tol must be finite and >= 0",
                                             "min_cos must be finite, > 0 and <= 1", "fill must be 0 .. 255", "workspace missing or too small",
                                             "null pointer"};

// 0 = fine; otherwise an index into MESH_COLOR_WHY
inline int mesh_color_check(int64_t channels, int64_t n_vertices, double tol, double min_cos, int64_t fill) {
  if (channels != 1 && channels != 3) return 1;
  if (n_vertices < 0 || n_vertices > MESH_COLOR_MAX_VERTICES) return 2;
  if (!(tol - tol == 0.0) || !(tol >= 0.0)) return 3;
  if (!(min_cos - min_cos == 0.0) || !(min_cos > 0.0) || !(min_cos <= 1.0)) return 4;
  if (fill < 0 || fill > 255) return 5;
  return 0;
}

inline int64_t mesh_color_workspace_bytes(int64_t n_ref) { return tsdf_workspace_bytes(n_ref); }

// the buffers of a call whose sizes passed: keep may always be null, depth / pixels when the views have no pixel (n_out = 0),
// the vertex arrays and the outputs when there is no vertex
inline int mesh_color_check_buffers(int64_t n_ref, int64_t n_out, int64_t n_vertices, const void* proj, const void* centres, const void* depth,
                                    const void* pixels, const void* vertices, const void* normals, const void* colors, const void* n_views,
                                    const void* best_view, const void* workspace, int64_t workspace_bytes) {
  if (!workspace || workspace_bytes < mesh_color_workspace_bytes(n_ref)) return 6;
  if (!view_pointers_ok(n_ref, n_out, proj, centres, depth, pixels)) return 7;
  if (n_vertices > 0 && (!vertices || !normals || !colors || !n_views || !best_view)) return 7;
  return 0;
}
inline int64_t mesh_color_blocks(int64_t n_vertices) { return (n_vertices + MESH_BLOCK - 1) / MESH_BLOCK; }
