// Host-side planning of the multi-scale feature stage (features_pyramid.hip): the option checks, the chained level sizes
// and the offsets of the level batch, the tile tables of the resampling launches, the carve-up of the two workspaces, the
// tap of one destination coordinate and the map of a level coordinate to level 0.  Plain C++ without a HIP dependency
// (tests/native/features_pyramid_check.cpp drives it under the sanitizers); the tap and the map also compile for the device,
// so the kernels and the host restatement share one text.  features_plan.h stays the plan of a single scale.
#pragma once
#include <cstdint>
#include <vector>
#include "features_plan.h"

#if defined(__HIPCC__)
#define PYR_HD __host__ __device__ __forceinline__
#else
#define PYR_HD inline
#endif

constexpr int PYR_MAX_LEVELS = 16;
constexpr int PYR_TILE_W = 256;         // destination pixels of a resampling tile along x: 64 threads of 4 adjacent pixels
constexpr int PYR_TILE_H = 16;          // rows of a resampling tile: 4 thread rows of 4
constexpr int PYR_PX = 4;               // adjacent destination pixels per thread, stored as one dword
constexpr int PYR_COPY_CHUNK = 4096;    // bytes of level 0 one workgroup copies: 256 threads of 16

// 0 when the options can be served, else the number of the offending rule
inline int pyr_check_options(int64_t n_levels, int64_t num, int64_t den) {
  if (n_levels < 2 || n_levels > PYR_MAX_LEVELS) return 1;
  if (den < 1 || num <= den || num > 2 * den) return 2;
  if (num > 16) return 3;
  if (8 * num < 9 * den) return 4;
  return 0;
}

inline const char* pyr_rule_text(int why) {
  static const char* const rule[] = {"", "n_levels must be in [2, 16]", "the scale num/den must satisfy den < num <= 2 den",
                                     "the scale's num must be at most 16", "the scale must be at least 9/8",
                                     "n_img out of range", "null pointer", "negative height or width",
                                     "more than 2^32 pixels in the level batch"};
  return why >= 0 && why <= 8 ? rule[why] : "invalid argument";
}

// a side of the next level: half-up rounding of n den / num, never below 1; an empty side stays empty
inline int32_t pyr_next_size(int32_t n, int num, int den) {
  if (n <= 0) return 0;
  const int64_t v = (2 * (int64_t)n * den + num) / (2 * num);
  return (int32_t)(v < 1 ? 1 : v);
}

// The tables of the level batch: slot i * n_levels + l holds level l of image i in exactly h * w bytes, slots back to back
// from 0.  lvl_off has n_img * n_levels + 1 entries.  0, or the number of the offending rule (outputs then unspecified).
inline int pyr_plan_sizes(int64_t n_img, const int32_t* heights, const int32_t* widths, int64_t n_levels, int64_t num,
                          int64_t den, int64_t* lvl_off, int32_t* lvl_h, int32_t* lvl_w) {
  const int why = pyr_check_options(n_levels, num, den);
  if (why) return why;
  if (n_img < 0 || n_img * n_levels >= (1 << 24)) return 5;
  if (!lvl_off || (n_img > 0 && (!heights || !widths || !lvl_h || !lvl_w))) return 6;
  int64_t off = 0;
  for (int64_t i = 0; i < n_img; ++i) {
    if (heights[i] < 0 || widths[i] < 0) return 7;
    int32_t h = heights[i], w = widths[i];
    for (int64_t l = 0; l < n_levels; ++l) {
      const int64_t s = i * n_levels + l;
      lvl_off[s] = off;
      lvl_h[s] = h;
      lvl_w[s] = w;
      off += (int64_t)h * w;
      if (off > FEAT_MAX_PIXELS) return 8;
      h = pyr_next_size(h, (int)num, (int)den);
      w = pyr_next_size(w, (int)num, (int)den);
    }
  }
  lvl_off[n_img * n_levels] = off;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------- the tap
// Destination pixel x of an axis of nd pixels over a source axis of ns >= nd >= 1 pixels: *i0 and *i1 are the two source
// pixels, *f the weight of i1 in 1/256.  u = (2x + 1) ns - nd >= 0; in 32 bits where u fits, else in 64.
PYR_HD void pyr_tap(int32_t x, int32_t nd, int32_t ns, int32_t* i0, int32_t* i1, int32_t* f) {
  const int64_t u = (2 * (int64_t)x + 1) * ns - nd;
  int64_t q, r;
  if (u < ((int64_t)1 << 32) && nd < (1 << 23)) {      // the remainder is below 2 nd < 2^24, so times 256 below 2^32
    const uint32_t u32 = (uint32_t)u, d32 = 2u * (uint32_t)nd;
    q = u32 / d32;
    r = ((u32 % d32) * 256u) / d32;
  } else {
    const int64_t d = 2 * (int64_t)nd;
    q = u / d;
    r = ((u % d) * 256) / d;
  }
  *i0 = (int32_t)q;
  *i1 = (int32_t)(q + 1 < ns ? q + 1 : ns - 1);
  *f = (int32_t)r;
}

PYR_HD int32_t pyr_blend(int32_t fx, int32_t fy, int32_t a00, int32_t a01, int32_t a10, int32_t a11) {
  return ((256 - fx) * (256 - fy) * a00 + fx * (256 - fy) * a01 + (256 - fx) * fy * a10 + fx * fy * a11 + 32768) >> 16;
}

// level-0 coordinate of pixel x of a level axis of nl pixels over n0: the product is exact, one division, one subtraction
// (nothing for an FMA to contract), one rounding to float32.  Exactly x at level 0.
PYR_HD float pyr_map(int32_t x, int32_t n0, int32_t nl) {
  const double p = (double)(2 * (int64_t)x + 1) * (double)n0;
  const double q = p / (double)(2 * (int64_t)nl);
  return (float)(q - 0.5);
}

// the rule in plain loops: what the kernels compute, for the host check
inline void pyr_resample_host(const uint8_t* src, int32_t hs, int32_t ws, uint8_t* dst, int32_t hd, int32_t wd, bool mask) {
  for (int32_t y = 0; y < hd; ++y) {
    int32_t y0, y1, fy;
    pyr_tap(y, hd, hs, &y0, &y1, &fy);
    for (int32_t x = 0; x < wd; ++x) {
      int32_t x0, x1, fx;
      pyr_tap(x, wd, ws, &x0, &x1, &fx);
      const int a00 = src[(int64_t)y0 * ws + x0], a01 = src[(int64_t)y0 * ws + x1];
      const int a10 = src[(int64_t)y1 * ws + x0], a11 = src[(int64_t)y1 * ws + x1];
      dst[(int64_t)y * wd + x] = mask ? (uint8_t)(a00 > 0 && a01 > 0 && a10 > 0 && a11 > 0)
                                      : (uint8_t)pyr_blend(fx, fy, a00, a01, a10, a11);
    }
  }
}

// ------------------------------------------------------------------------------------------------------- tile tables
// One (level, image) pair as the kernels see it; entry l * n_img + i.  Level 0 is a byte copy in chunks of PYR_COPY_CHUNK,
// level l >= 1 a resampling of level l - 1 in tiles of PYR_TILE_W x PYR_TILE_H destination pixels.
struct pyr_entry {
  int64_t src;            // level 0: the image's offset in `images`; else the offset of level l - 1 in the level batch
  int64_t dst;            // the offset of this level in the level batch
  int32_t hs, ws, hd, wd; // level 0: hs = hd, ws = wd
  int32_t tile0;          // its first tile (level 0: chunk) in the launch of its level
  int32_t tiles_x;        // tiles along x (level 0: its number of chunks)
};

struct pyr_plan {
  std::vector<pyr_entry> entry;         // [n_levels][n_img]
  std::vector<int64_t> tiles;           // [n_levels]: workgroups of the launch of each level
  int64_t pixels = 0;                   // extent of the level batch
};

// the plan of a checked batch (pyr_plan_sizes == 0 filled lvl_*; feat_check_images == 0 for the images)
inline pyr_plan pyr_plan_tiles(int64_t n_img, const int64_t* img_off, int64_t n_levels, const int64_t* lvl_off,
                               const int32_t* lvl_h, const int32_t* lvl_w) {
  pyr_plan P;
  P.entry.resize((size_t)(n_img * n_levels));
  P.tiles.assign((size_t)n_levels, 0);
  for (int64_t l = 0; l < n_levels; ++l)
    for (int64_t i = 0; i < n_img; ++i) {
      const int64_t s = i * n_levels + l;
      pyr_entry& e = P.entry[(size_t)(l * n_img + i)];
      e.dst = lvl_off[s];
      e.hd = lvl_h[s];
      e.wd = lvl_w[s];
      e.tile0 = (int32_t)P.tiles[(size_t)l];
      int64_t n_tiles;
      if (l == 0) {
        e.src = img_off[i];
        e.hs = e.hd;
        e.ws = e.wd;
        n_tiles = ((int64_t)e.hd * e.wd + PYR_COPY_CHUNK - 1) / PYR_COPY_CHUNK;
        e.tiles_x = (int32_t)n_tiles;
      } else {
        e.src = lvl_off[s - 1];
        e.hs = lvl_h[s - 1];
        e.ws = lvl_w[s - 1];
        const bool any = e.hd > 0 && e.wd > 0;
        e.tiles_x = any ? (e.wd + PYR_TILE_W - 1) / PYR_TILE_W : 0;
        n_tiles = any ? (int64_t)e.tiles_x * ((e.hd + PYR_TILE_H - 1) / PYR_TILE_H) : 0;
      }
      P.tiles[(size_t)l] += n_tiles;
    }
  P.pixels = lvl_off[n_img * n_levels];
  return P;
}

// ------------------------------------------------------------------------------------------------------- workspaces
struct pyr_layout {
  int64_t table;          // pyr_entry [n_levels][n_img]
  int64_t bytes;
};

inline pyr_layout pyr_plan_layout(int64_t n_img, int64_t n_levels) {
  pyr_layout L;
  L.table = 0;
  L.bytes = feat_align(n_img * n_levels * (int64_t)sizeof(pyr_entry)) + 256;
  return L;
}

struct merge_layout {
  int64_t dims;           // int32 [n_img * n_levels][2]: (h, w) of every slot of the level batch
  int64_t cut;            // int32 [n_img][2]: cut score (0 = keep all) and the number of ties that stay
  int64_t cnt;            // int32 [n_img + 1]: keypoints of the image after the cut
  int64_t bytes;
};

inline merge_layout merge_plan_layout(int64_t n_img, int64_t n_levels) {
  merge_layout L;
  int64_t off = 0;
  auto take = [&](int64_t count, int64_t width) { const int64_t at = off; off += feat_align(count * width); return at; };
  L.dims = take(n_img * n_levels * 2, 4);
  L.cut = take(n_img * 2, 4);
  L.cnt = take(n_img + 1, 4);
  L.bytes = off + 256;
  return L;
}
