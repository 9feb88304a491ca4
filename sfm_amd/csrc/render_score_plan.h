// Launch plan of the render score (render_score.hip): the argument checks, the tiles, the workspace and the grid.  Plain
// C++: it compiles for the host too (tests/native/render_score_check.cpp replays it under the sanitizers).
//
// The views are a table of TsdfView records (mesh_plan.h): n_view records and one that closes the list; the arrays of view v
// start at pixel out_off[v] (times the channel count for the colour arrays).  The workspace holds that table alone.
// An image is cut into tiles of RENDER_SCORE_TILE_W x RENDER_SCORE_TILE_H pixels, rows of tiles from the top; one workgroup
// of RENDER_SCORE_BLOCK threads takes one tile of one view - the tile in blockIdx.x, counted over the view with the most
// tiles, the view in blockIdx.y - and one thread one pixel of it.  The workgroup stages the tile with a halo of window / 2
// pixels on every side: RENDER_SCORE_STAGE_W x RENDER_SCORE_STAGE_H words per image at the largest window, rows sw words apart;
// a staged pixel outside the image is 0, which is not compared.  The window of the tile's pixel (lx, ly) starts at the
// staged word ly * sw + lx.
#pragma once
#include <cstdint>
#include "mesh_plan.h"

#define RENDER_SCORE_MAX_VIEWS 65535
#define RENDER_SCORE_MAX_SIDE 32768
#define RENDER_SCORE_MIN_WINDOW 3
#define RENDER_SCORE_MAX_WINDOW 11
#define RENDER_SCORE_TILE_W 32
#define RENDER_SCORE_TILE_H 8
#define RENDER_SCORE_BLOCK (RENDER_SCORE_TILE_W * RENDER_SCORE_TILE_H)
#define RENDER_SCORE_STAGE_W (RENDER_SCORE_TILE_W + RENDER_SCORE_MAX_WINDOW - 1)
#define RENDER_SCORE_STAGE_H (RENDER_SCORE_TILE_H + RENDER_SCORE_MAX_WINDOW - 1)
#define RENDER_SCORE_STAGE_WORDS (RENDER_SCORE_STAGE_W * RENDER_SCORE_STAGE_H)
#define RENDER_SCORE_STATS 14                         /* the columns a workgroup adds to: 1 .. 14 */

static_assert(RENDER_SCORE_MAX_VIEWS <= 65535, "the view is blockIdx.y");
static_assert(RENDER_SCORE_BLOCK == 256 && RENDER_SCORE_BLOCK % 64 == 0, "four wavefronts to a workgroup");
static_assert(RENDER_SCORE_TILE_W == 32, "a thread's column is its index modulo 32");
static_assert((int64_t)(RENDER_SCORE_MAX_SIDE / RENDER_SCORE_TILE_W) * (RENDER_SCORE_MAX_SIDE / RENDER_SCORE_TILE_H) < 0x7FFFFFFFLL, "the tiles of a view fit blockIdx.x");
// the sums of one wavefront fit 32 bits: 64 lanes of at most 255^2, or of a quantised value of at most 2^24 and a rounding
static_assert(64LL * 16777217LL < 0x7FFFFFFFLL, "a wavefront's sum of quantised values fits int32");

static const char* const RENDER_SCORE_WHY[] = {"", "n_view must be 0 .. 65535", "every image side must be 0 .. 32768", "channels must be 1 or 3",
                                               "window must be odd and 3 .. 11", "rel_tol must be finite and >= 0",
                                               "view_keep is given iff view_depth is given", "workspace missing or too small", "null pointer"};

MESH_PLAN_HD int64_t render_score_tiles_x(int64_t w) { return (w + RENDER_SCORE_TILE_W - 1) / RENDER_SCORE_TILE_W; }
MESH_PLAN_HD int64_t render_score_tiles_y(int64_t h) { return (h + RENDER_SCORE_TILE_H - 1) / RENDER_SCORE_TILE_H; }
MESH_PLAN_HD int64_t render_score_tiles(int64_t h, int64_t w) { return render_score_tiles_x(w) * render_score_tiles_y(h); }

// heights / widths per view; fills views (n_view + 1 records) when it is not null, the pixels of all views and the tiles of
// the view with the most.  0 = fine; otherwise an index into RENDER_SCORE_WHY
inline int render_score_check_views(int64_t n_view, const int32_t* heights, const int32_t* widths, TsdfView* views, int64_t* n_pix, int64_t* max_tiles) {
  if (n_view < 0 || n_view > RENDER_SCORE_MAX_VIEWS) return 1;
  if (n_view > 0 && (!heights || !widths)) return 8;
  int64_t off = 0, most = 0;
  for (int64_t v = 0; v < n_view; ++v) {
    if (heights[v] < 0 || heights[v] > RENDER_SCORE_MAX_SIDE || widths[v] < 0 || widths[v] > RENDER_SCORE_MAX_SIDE) return 2;
    if (views) views[v] = TsdfView{off, heights[v], widths[v]};
    off += (int64_t)heights[v] * widths[v];
    const int64_t t = render_score_tiles(heights[v], widths[v]);
    most = t > most ? t : most;
  }
  if (views) views[n_view] = TsdfView{off, 0, 0};
  if (n_pix) *n_pix = off;
  if (max_tiles) *max_tiles = most;
  return 0;
}

inline int render_score_check_options(int64_t channels, int64_t window, double rel_tol, const void* view_depth, const void* view_keep) {
  if (channels != 1 && channels != 3) return 3;
  if (window < RENDER_SCORE_MIN_WINDOW || window > RENDER_SCORE_MAX_WINDOW || window % 2 != 1) return 4;
  if (!(rel_tol - rel_tol == 0.0) || !(rel_tol >= 0.0)) return 5;
  if ((view_depth != nullptr) != (view_keep != nullptr)) return 6;
  return 0;
}

struct RenderScoreLayout { int64_t views, bytes; };

inline RenderScoreLayout render_score_layout(int64_t n_view) {
  RenderScoreLayout L;
  L.views = 0;
  L.bytes = mesh_align((n_view + 1) * (int64_t)sizeof(TsdfView)) + 256;
  return L;
}

// the buffers of a call whose sizes passed: the images may be null without a pixel, stats without a view; the mask, the
// views' depth and the two maps may always be null
inline int render_score_check_buffers(int64_t n_view, int64_t n_pix, int64_t needed_bytes, const void* render_color, const void* render_triangle,
                                      const void* render_depth, const void* photos, const void* stats, const void* workspace, int64_t workspace_bytes) {
  if (!workspace || workspace_bytes < needed_bytes) return 7;
  if (n_view > 0 && !stats) return 8;
  if (n_pix > 0 && (!render_color || !render_triangle || !render_depth || !photos)) return 8;
  return 0;
}

// tile t of an image w wide: its first pixel, the first staged pixel (negative at the image's edge) and the staged size
struct RenderScoreTile { int x0, y0, sx0, sy0, sw, sh; };

MESH_PLAN_HD RenderScoreTile render_score_tile(int64_t t, int w, int window) {
  const int64_t tx = (w + RENDER_SCORE_TILE_W - 1) / RENDER_SCORE_TILE_W;
  const int r = window / 2;
  RenderScoreTile T;
  T.x0 = (int)(t % tx) * RENDER_SCORE_TILE_W;
  T.y0 = (int)(t / tx) * RENDER_SCORE_TILE_H;
  T.sx0 = T.x0 - r;
  T.sy0 = T.y0 - r;
  T.sw = RENDER_SCORE_TILE_W + 2 * r;
  T.sh = RENDER_SCORE_TILE_H + 2 * r;
  return T;
}
