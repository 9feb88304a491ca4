// Launch plan of the exposure compensation (mesh_exposure.hip): the argument checks, the workspace, the grids and the split of
// the vertex range.  Plain C++: it compiles for the host too (tests/native/mesh_exposure_check.cpp replays it under the
// sanitizers).
//
// k_exposure_sample  one thread per vertex, MESH_BLOCK consecutive vertices per workgroup, as k_mesh_colors; the workspace
//                    holds the table of TsdfView records (mesh_plan.h), n_ref records and one that closes the list.
// k_exposure_gram    the view pairs are cut into tiles of MESH_EXPOSURE_TILE x MESH_EXPOSURE_TILE (view i of `sums` down,
//                    view j across), the vertices into chunks of MESH_EXPOSURE_CHUNK.  One workgroup of four wavefronts
//                    takes one tile and one chunk: blockIdx.x = the chunk, blockIdx.y = tile_i * tiles + tile_j.  A
//                    wavefront takes the steps of MESH_EXPOSURE_STEP vertices of the chunk whose number is its own
//                    modulo 4, MESH_EXPOSURE_AHEAD of them per round trip to memory, one MFMA per table and step, and the
//                    workgroup adds its tile in int32 before it goes to the int64 tables.  k_exposure_clear zeroes both
//                    tables in one launch in front of it.  The workspace is not used by this call.
// k_images_gain      the bytes of an image are cut into the 16-byte windows of the source ADDRESS; one thread takes one
//                    window, MESH_EXPOSURE_GAIN_BLOCK windows per workgroup, blockIdx.y = the image within a batch of
//                    MESH_EXPOSURE_GAIN_BATCH whose offsets and gains travel as kernel arguments.
#pragma once
#include <cstdint>
#include "mesh_color_plan.h"

#define MESH_EXPOSURE_MAX_VIEWS 1024
#define MESH_EXPOSURE_TILE 32
#define MESH_EXPOSURE_STEP 32                          /* the vertices of one MFMA: its k */
#define MESH_EXPOSURE_CHUNK 2048
#define MESH_EXPOSURE_AHEAD 4                          /* the steps whose operands a wavefront asks for before it multiplies */
#define MESH_EXPOSURE_GRAM_BLOCK 256
#define MESH_EXPOSURE_GAIN_BLOCK 256
#define MESH_EXPOSURE_GAIN_BATCH 32
#define MESH_EXPOSURE_MAX_SIDE 32768
#define MESH_EXPOSURE_MAX_IMAGES 0x7FFFFFFFLL

static_assert(MESH_EXPOSURE_CHUNK % (MESH_EXPOSURE_STEP * (MESH_EXPOSURE_GRAM_BLOCK / 64) * MESH_EXPOSURE_AHEAD) == 0, "every wavefront takes whole rounds of steps");
// a workgroup's entry of a table is a sum over its chunk of products of an int8 and a flag: |entry| <= 128 * chunk
static_assert(128LL * MESH_EXPOSURE_CHUNK < 0x7FFFFFFFLL, "a chunk's sums fit int32");
static_assert(MESH_EXPOSURE_MAX_VIEWS % MESH_EXPOSURE_TILE == 0 &&
              (MESH_EXPOSURE_MAX_VIEWS / MESH_EXPOSURE_TILE) * (MESH_EXPOSURE_MAX_VIEWS / MESH_EXPOSURE_TILE) <= 65535, "the tiles fit a grid dimension");
static_assert((MESH_COLOR_MAX_VERTICES + MESH_EXPOSURE_CHUNK - 1) / MESH_EXPOSURE_CHUNK < 0x7FFFFFFFLL, "the chunks fit blockIdx.x's range");
// the windows of the largest image fit blockIdx.x
static_assert(((int64_t)MESH_EXPOSURE_MAX_SIDE * MESH_EXPOSURE_MAX_SIDE * 3 / 16 + 2) / MESH_EXPOSURE_GAIN_BLOCK + 1 < 0x7FFFFFFFLL, "the windows fit");

static const char* const MESH_EXPOSURE_WHY[] = {"", "n_ref must be 0 .. 1024", "channels must be 1 or 3", "n_vertices must be 0 .. 2^31 - 1",
                                                "workspace missing or too small", "null pointer", "every image side must be 0 .. 32768",
                                                "negative or too many images", "every gain must be finite and >= 0"};

// 0 = fine; otherwise an index into MESH_EXPOSURE_WHY
inline int mesh_exposure_check(int64_t n_ref, int64_t channels, int64_t n_vertices) {
  if (n_ref < 0 || n_ref > MESH_EXPOSURE_MAX_VIEWS) return 1;
  if (channels != 1 && channels != 3) return 2;
  if (n_vertices < 0 || n_vertices > MESH_COLOR_MAX_VERTICES) return 3;
  return 0;
}

inline int64_t mesh_exposure_workspace_bytes(int64_t n_ref) { return tsdf_workspace_bytes(n_ref); }

inline int64_t mesh_exposure_tiles(int64_t n_ref) { return (n_ref + MESH_EXPOSURE_TILE - 1) / MESH_EXPOSURE_TILE; }
inline int64_t mesh_exposure_chunks(int64_t n_vertices) { return (n_vertices + MESH_EXPOSURE_CHUNK - 1) / MESH_EXPOSURE_CHUNK; }

// the buffers of the sample call whose sizes passed (what mesh_color_check_buffers asks of the views and the vertices)
inline int mesh_exposure_check_sample_buffers(int64_t n_ref, int64_t n_out, int64_t n_vertices, const void* proj, const void* centres, const void* depth,
                                              const void* pixels, const void* vertices, const void* normals, const void* seen, const void* samples,
                                              const void* workspace, int64_t workspace_bytes) {
  if (!workspace || workspace_bytes < mesh_exposure_workspace_bytes(n_ref)) return 4;
  if (!view_pointers_ok(n_ref, n_out, proj, centres, depth, pixels)) return 5;
  if (n_vertices > 0 && (!vertices || !normals)) return 5;
  if (n_vertices > 0 && n_ref > 0 && (!seen || !samples)) return 5;
  return 0;
}

// the buffers of the gram call: the tables may be null without a view, the inputs without a view or a vertex
inline int mesh_exposure_check_gram_buffers(int64_t n_ref, int64_t n_vertices, const void* seen, const void* samples, const void* overlap,
                                            const void* sums, const void* workspace, int64_t workspace_bytes) {
  if (!workspace || workspace_bytes < mesh_exposure_workspace_bytes(n_ref)) return 4;
  if (n_ref > 0 && (!overlap || !sums)) return 5;
  if (n_ref > 0 && n_vertices > 0 && (!seen || !samples)) return 5;
  return 0;
}

// ---- the gain pass ----
// heights / widths per image; fills off (n_img + 1 pixel offsets) when it is not null.  0 = fine.
inline int mesh_exposure_check_images(int64_t n_img, const int32_t* heights, const int32_t* widths, int64_t channels, const double* gains,
                                      int64_t* off) {
  if (n_img < 0 || n_img > MESH_EXPOSURE_MAX_IMAGES) return 7;
  if (channels != 1 && channels != 3) return 2;
  if (n_img > 0 && (!heights || !widths || !gains)) return 5;
  int64_t at = 0;
  for (int64_t i = 0; i < n_img; ++i) {
    if (heights[i] < 0 || heights[i] > MESH_EXPOSURE_MAX_SIDE || widths[i] < 0 || widths[i] > MESH_EXPOSURE_MAX_SIDE) return 6;
    if (off) off[i] = at;
    at += (int64_t)heights[i] * widths[i];
  }
  if (off) off[n_img] = at;
  for (int64_t i = 0; i < n_img * channels; ++i)
    if (!(gains[i] - gains[i] == 0.0) || !(gains[i] >= 0.0)) return 8;
  return 0;
}

// the bytes [b0, b1) of an array that starts `mis` bytes (0 .. 15) behind a 16-byte boundary, cut into the windows of that
// boundary: their number, and the bytes of window t
MESH_PLAN_HD int64_t mesh_exposure_windows(int64_t b0, int64_t b1, int mis) {
  return b1 > b0 ? (b1 - 1 + mis) / 16 - (b0 + mis) / 16 + 1 : 0;
}
struct MeshExposureWindow { int64_t lo, hi; };
MESH_PLAN_HD MeshExposureWindow mesh_exposure_window(int64_t b0, int64_t b1, int mis, int64_t t) {
  const int64_t start = ((b0 + mis) / 16 + t) * 16 - mis;
  MeshExposureWindow w;
  w.lo = start > b0 ? start : b0;
  w.hi = start + 16 < b1 ? start + 16 : b1;
  return w;
}
inline int64_t mesh_exposure_gain_blocks(int64_t windows) { return (windows + MESH_EXPOSURE_GAIN_BLOCK - 1) / MESH_EXPOSURE_GAIN_BLOCK; }

// what sfm_mesh_exposure_plan reports: the tile sides, the chunk and the workgroups of the gram launch
inline void mesh_exposure_plan(int64_t n_ref, int64_t n_vertices, int32_t out[4]) {
  const int64_t t = mesh_exposure_tiles(n_ref);
  out[0] = MESH_EXPOSURE_TILE;
  out[1] = MESH_EXPOSURE_TILE;
  out[2] = MESH_EXPOSURE_CHUNK;
  const int64_t groups = t * t * mesh_exposure_chunks(n_vertices);
  out[3] = (int32_t)(groups < 0x7FFFFFFFLL ? groups : 0x7FFFFFFFLL);
}
