// Launch plan of the dense-depth stage (depth.hip): the tables a call uploads, the workspace layout, the tile and halo
// sizes of the sweep, the map from a thread to the pixels it fills and owns, and the argument checks.  Plain C++: it
// compiles for the host too (tests/native/depth_check.cpp runs it under the sanitizers).
//
// The sweep gives one workgroup of DEPTH_THREADS threads a tile of DEPTH_TW x DEPTH_TH reference pixels.  For a window of
// radius r the tile needs the per-plane cost c_k on (DEPTH_TW + 2r) x (DEPTH_TH + 2r) pixels, tile plus halo, coordinates
// clamped to the image.  Slot i of that rectangle (row-major) is filled by thread i % DEPTH_THREADS in its round
// i / DEPTH_THREADS; a thread owns the two output pixels (tx, 2 ty) and (tx, 2 ty + 1) of the tile, tx = tid % DEPTH_TW,
// ty = tid / DEPTH_TW, whose windows share 2r of their 2r + 1 rows.
#pragma once
#include <cstdint>
#include <vector>
#include "scan_plan.h"

#if defined(__HIPCC__)
#define DEPTH_PLAN_HD __host__ __device__ __forceinline__
#else
#define DEPTH_PLAN_HD inline
#endif

#define DEPTH_TW 32
#define DEPTH_TH 16
#define DEPTH_THREADS 256
#define DEPTH_MAX_SOURCES 8
#define DEPTH_MAX_RADIUS 4
#define DEPTH_MAX_PLANES 1024
#define DEPTH_PIXEL_BLOCK 256           /* pixels per workgroup of the census and of the filter */

static_assert(DEPTH_TW * DEPTH_TH == 2 * DEPTH_THREADS, "a thread owns two pixels of the tile");
static_assert(DEPTH_TH % 2 == 0 && DEPTH_THREADS % DEPTH_TW == 0, "the two pixels of a thread are vertical neighbours");
// S <= 48 * sources * window fits the uint16 of the cost map
static_assert(48 * DEPTH_MAX_SOURCES * (2 * DEPTH_MAX_RADIUS + 1) * (2 * DEPTH_MAX_RADIUS + 1) <= 65535, "cost fits 16 bits");

struct DepthImage { int64_t off; int32_t h, w; };
struct DepthView {
  int64_t out_off;          // first element of the view's maps in the outputs (views back to back, row-major)
  int64_t tile_first;       // workgroups of the sweep in front of this view
  int64_t pix_block_first;  // workgroups of the filter in front of this view
  int64_t plane_first;      // first of its plane depths
  int32_t image, n_planes, src_first, n_src, tiles_x, tiles_y;
};

DEPTH_PLAN_HD int depth_halo_w(int r) { return DEPTH_TW + 2 * r; }
DEPTH_PLAN_HD int depth_halo_h(int r) { return DEPTH_TH + 2 * r; }
DEPTH_PLAN_HD int depth_halo_count(int r) { return depth_halo_w(r) * depth_halo_h(r); }
DEPTH_PLAN_HD int depth_halo_rounds(int r) { return (depth_halo_count(r) + DEPTH_THREADS - 1) / DEPTH_THREADS; }
DEPTH_PLAN_HD int depth_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }      // to [0, hi]

// image pixel behind slot `slot` of tile plus halo of the tile whose first pixel is (x0, y0), in a w x h image
DEPTH_PLAN_HD void depth_halo_pixel(int slot, int r, int x0, int y0, int w, int h, int* px, int* py) {
  const int hw = depth_halo_w(r);
  *px = depth_clamp(x0 - r + slot % hw, w - 1);
  *py = depth_clamp(y0 - r + slot / hw, h - 1);
}
// slot of tile plus halo under the window offset (dx, dy), |dx|, |dy| <= r, of the tile pixel (tx, ty)
DEPTH_PLAN_HD int depth_halo_slot(int tx, int ty, int dx, int dy, int r) { return (ty + r + dy) * depth_halo_w(r) + (tx + r + dx); }

DEPTH_PLAN_HD int64_t depth_tiles_x(int w) { return (w + DEPTH_TW - 1) / DEPTH_TW; }
DEPTH_PLAN_HD int64_t depth_tiles_y(int h) { return (h + DEPTH_TH - 1) / DEPTH_TH; }
DEPTH_PLAN_HD int64_t depth_pixel_blocks(int64_t n) { return (n + DEPTH_PIXEL_BLOCK - 1) / DEPTH_PIXEL_BLOCK; }

enum { DEPTH_BY_TILE = 0, DEPTH_BY_PIXEL_BLOCK = 1 };
// the image element `e` of the image buffer belongs to: the last one whose slot starts at or before e
DEPTH_PLAN_HD int depth_find_image(const DepthImage* images, int n_img, int64_t e) {
  int lo = 0, hi = n_img;
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (images[mid].off <= e) lo = mid; else hi = mid;
  }
  return lo;
}
// the view workgroup `b` belongs to: the last one whose first workgroup is <= b (record n_ref holds the totals; views
// without a pixel own no workgroup and are stepped over)
DEPTH_PLAN_HD int depth_find_view(const DepthView* views, int n_ref, int64_t b, int by) {
  int lo = 0, hi = n_ref;
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    const int64_t first = by == DEPTH_BY_TILE ? views[mid].tile_first : views[mid].pix_block_first;
    if (first <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// 0 = fine; otherwise the reason (depth.hip has the words)
inline int depth_check_images(int64_t n_img, const int64_t* img_off, const int32_t* heights, const int32_t* widths) {
  if (n_img < 0 || n_img > 0x7FFFFFFFLL) return 1;
  if (!img_off || (n_img > 0 && (!heights || !widths))) return 2;
  if (img_off[0] < 0) return 3;
  for (int64_t i = 0; i < n_img; ++i) {
    if (img_off[i + 1] < img_off[i]) return 3;
    if (heights[i] < 0 || widths[i] < 0) return 4;
    if ((int64_t)heights[i] * (int64_t)widths[i] > img_off[i + 1] - img_off[i]) return 5;
  }
  return 0;
}

inline int depth_check_views(int64_t n_img, int64_t n_ref, const int32_t* ref_image, const int64_t* src_ptr, const int32_t* src_image,
                             const int64_t* plane_ptr, int radius) {
  if (n_ref < 0 || n_ref > n_img) return 6;                  // more views than images: one is listed twice
  if (radius < 0 || radius > DEPTH_MAX_RADIUS) return 7;
  if (!src_ptr || !plane_ptr || (n_ref > 0 && !ref_image)) return 2;
  if (src_ptr[0] != 0 || plane_ptr[0] != 0) return 8;
  std::vector<char> seen((size_t)n_img, 0);
  for (int64_t r = 0; r < n_ref; ++r) {
    const int64_t ref = ref_image[r];
    if (ref < 0 || ref >= n_img) return 9;
    if (seen[(size_t)ref]) return 6;
    seen[(size_t)ref] = 1;
    const int64_t ns = src_ptr[r + 1] - src_ptr[r], np = plane_ptr[r + 1] - plane_ptr[r];
    if (ns < 0 || ns > DEPTH_MAX_SOURCES) return 10;
    if (np < 1 || np > DEPTH_MAX_PLANES) return 11;
    if (ns > 0 && !src_image) return 2;
    for (int64_t e = src_ptr[r]; e < src_ptr[r + 1]; ++e) {
      if (src_image[e] < 0 || src_image[e] >= n_img) return 12;
      if (src_image[e] == ref) return 13;
    }
  }
  return 0;
}

static const char* const DEPTH_WHY[] = {
    "", "negative or too many images", "null pointer", "img_off does not ascend", "negative image size", "an image is larger than its slot",
    "a reference image is listed twice, or a negative number of views", "radius must be 0 .. 4", "src_ptr / plane_ptr must start at 0",
    "a reference index is out of range", "a view has more than 8 sources, or src_ptr descends", "a view needs 1 .. 1024 planes",
    "a source index is out of range", "a source is its own reference"};

struct DepthPlan {
  std::vector<DepthImage> images;          // n_img + 1: the last record holds the end of the last slot
  std::vector<DepthView> views;            // n_ref + 1: the last record holds the totals
  std::vector<int32_t> ref_of_image;       // view of an image, -1 without a depth map
  int64_t n_out = 0, n_tiles = 0, n_pix_blocks = 0;
};

// after depth_check_images (views may be absent: the census needs the image table only)
inline DepthPlan depth_plan(int64_t n_img, const int64_t* img_off, const int32_t* heights, const int32_t* widths, int64_t n_ref,
                            const int32_t* ref_image, const int64_t* src_ptr, const int64_t* plane_ptr) {
  DepthPlan p;
  p.images.resize((size_t)n_img + 1);
  for (int64_t i = 0; i < n_img; ++i) p.images[(size_t)i] = DepthImage{img_off[i], heights[i], widths[i]};
  p.images[(size_t)n_img] = DepthImage{img_off[n_img], 0, 0};
  p.ref_of_image.assign((size_t)n_img, -1);
  p.views.resize((size_t)n_ref + 1);
  for (int64_t r = 0; r <= n_ref; ++r) {
    DepthView& v = p.views[(size_t)r];
    v = DepthView{p.n_out, p.n_tiles, p.n_pix_blocks, 0, -1, 0, 0, 0, 0, 0};
    if (r == n_ref) break;
    const int32_t img = ref_image[r];
    const int h = heights[img], w = widths[img];
    v.image = img;
    v.plane_first = plane_ptr[r]; v.n_planes = (int32_t)(plane_ptr[r + 1] - plane_ptr[r]);
    v.src_first = (int32_t)src_ptr[r]; v.n_src = (int32_t)(src_ptr[r + 1] - src_ptr[r]);
    v.tiles_x = (int32_t)depth_tiles_x(w); v.tiles_y = (int32_t)depth_tiles_y(h);
    p.ref_of_image[(size_t)img] = (int32_t)r;
    const int64_t n = (int64_t)h * w;
    p.n_out += n;
    p.n_tiles += n > 0 ? (int64_t)v.tiles_x * v.tiles_y : 0;
    p.n_pix_blocks += depth_pixel_blocks(n);
  }
  p.views[(size_t)n_ref].plane_first = n_ref > 0 ? plane_ptr[n_ref] : 0;
  p.views[(size_t)n_ref].src_first = n_ref > 0 ? (int32_t)src_ptr[n_ref] : 0;
  return p;
}

struct DepthLayout { int64_t images, views, src_image, ref_of_image, max_cost, bytes; };

inline int64_t depth_align(int64_t v) { return (v + 255) / 256 * 256; }
inline DepthLayout depth_layout(int64_t n_img, int64_t n_ref, int64_t n_entries) {
  DepthLayout L;
  int64_t off = 0;
  L.images = off;       off += depth_align((n_img + 1) * (int64_t)sizeof(DepthImage));
  L.views = off;        off += depth_align((n_ref + 1) * (int64_t)sizeof(DepthView));
  L.src_image = off;    off += depth_align(n_entries * 4);
  L.ref_of_image = off; off += depth_align(n_img * 4);
  L.max_cost = off;     off += depth_align(n_ref * 4);
  L.bytes = off + 256;
  return L;
}

// ---- fusion (depth_fuse.hip): the owner counts of the pixel blocks and their two-level exclusive scan ----
// k_depth_fuse_mark leaves one owner count per pixel block (the blocks of the filter: DEPTH_PIXEL_BLOCK pixels of one view,
// views back to back, block b of the call at blk[b]).  The two-level scan of scan_plan.h runs over them: level one
// (k_depth_fuse_scan_chunks) writes one total per chunk, level two (k_depth_fuse_scan_top) walks the totals and writes
// pt_ptr[v] = depth_scan_base(...) of the first block of view v (the grand total where no block follows).  The first
// output slot of block b is depth_scan_base(chunk_base, blk, b).  Nothing waits on another workgroup: three launches.
#define DEPTH_MAX_NORMAL_STEP 4

static_assert(DEPTH_PIXEL_BLOCK == DEPTH_THREADS && DEPTH_THREADS == SCAN_THREADS, "a pixel block is a workgroup of the scan");
// a chunk holds at most SCAN_CHUNK * DEPTH_PIXEL_BLOCK owners: the counts and the bases within a chunk fit 32 bits
static_assert((int64_t)SCAN_CHUNK * DEPTH_PIXEL_BLOCK < 0x7FFFFFFFLL, "bases within a chunk fit 32 bits");

DEPTH_PLAN_HD int64_t depth_scan_base(const int64_t* chunk_base, const uint32_t* blk, int64_t b) {
  return scan_base(chunk_base, 1, 0, b, (int64_t)blk[b]);
}
// the most pixel blocks a call with n_out output elements in n_ref views can have: every view ends in one partial block
DEPTH_PLAN_HD int64_t depth_max_pixel_blocks(int64_t n_out, int64_t n_ref) { return n_out / DEPTH_PIXEL_BLOCK + n_ref; }

struct DepthFuseLayout { DepthLayout tables; int64_t blk, chunk_base, bytes; };

inline DepthFuseLayout depth_fuse_layout(int64_t n_img, int64_t n_ref, int64_t n_entries, int64_t n_blocks) {
  DepthFuseLayout L;
  L.tables = depth_layout(n_img, n_ref, n_entries);
  int64_t off = depth_align(L.tables.bytes);
  L.blk = off;        off += depth_align(n_blocks * 4);
  L.chunk_base = off; off += depth_align(scan_chunks(n_blocks) * 8);
  L.bytes = off + 256;
  return L;
}

// what the fusion calls refuse beyond depth_check_images / depth_check_views: 0 = fine, else an index into DEPTH_FUSE_WHY
inline int depth_check_fuse(double rel_tol, int normal_step, double normal_jump) {
  if (!(rel_tol >= 0.0)) return 1;
  if (normal_step < 1 || normal_step > DEPTH_MAX_NORMAL_STEP) return 2;
  if (!(normal_jump >= 0.0)) return 3;
  return 0;
}
static const char* const DEPTH_FUSE_WHY[] = {"", "rel_tol must be a number >= 0", "normal_step must be 1 .. 4", "normal_jump must be a number >= 0"};
