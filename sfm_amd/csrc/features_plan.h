// Host-side planning of the feature stage (features.hip): the argument checks, the per-image table the kernels index, the
// carve-up of the caller's workspace, and the sampling pattern of the descriptor (generator and rotation).  Plain C++
// without a HIP dependency, so that it can be checked on a CPU under the sanitizers (tests/native/features_plan_check.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

constexpr int FEAT_TILE_W = 128;          // pixels of a score / blur tile along x
constexpr int FEAT_SCORE_TILE_H = 32;     // rows of a score tile (3-pixel halo on top)
constexpr int FEAT_BLUR_TILE_H = 16;      // rows of a blur tile (3-pixel halo on top)
constexpr int FEAT_EDGE_MIN = 16;         // 13 (pattern radius, rounding included: 14) + 3 (blur support) stays inside 16
constexpr int FEAT_PATTERN_R2 = 169;      // every endpoint of a base table lies within x^2 + y^2 <= 169
constexpr int FEAT_BINS = 30;             // orientation bins of 12 degrees
constexpr int FEAT_PAIRS = 256;
constexpr int64_t FEAT_MAX_PIXELS = (int64_t)1 << 32;   // a 3x3 strict maximum leaves at most one keypoint per 4 pixels: int32 offsets
constexpr int FEAT_BLUR_W[7] = {18, 33, 49, 56, 49, 33, 18};   // sums to 256

// One image as the kernels see it.  Only an image that can hold a keypoint at the smallest gate (h, w >= 33) has rows in
// the row list and score tiles - whatever the edge of the call, so that detect and describe plan alike; every image with
// pixels has blur tiles.
struct feat_image {
  int64_t off;          // first pixel in the image / mask / map buffers
  int32_t h, w;
  int32_t row0;         // its first row in the row list (rows of all eligible images back to back)
  int32_t rows;         // h if eligible, else 0
  int32_t score_tile0, score_tiles_x;
  int32_t blur_tile0, blur_tiles_x;
};

struct feat_plan {
  std::vector<feat_image> img;
  int64_t pixels = 0;       // img_off[n_img]: the extent of the pixel buffers
  int64_t rows = 0;         // entries of the row list
  int64_t score_tiles = 0, blur_tiles = 0;
};

inline bool feat_eligible(int64_t h, int64_t w, int64_t edge) { return h >= 2 * edge + 1 && w >= 2 * edge + 1; }

// 0 when the options can be served, else the number of the first offending rule (for the error text)
inline int feat_check_options(int64_t threshold, int64_t edge, int64_t max_features) {
  if (threshold < 1 || threshold > 254) return 1;
  if (edge < FEAT_EDGE_MIN || edge > (1 << 20)) return 2;
  if (max_features < 0 || max_features >= ((int64_t)1 << 31)) return 3;
  return 0;
}

// 0 when img_off alone describes a buffer that can be served (what sfm_features_workspace_bytes sees)
inline int feat_check_offsets(int64_t n_img, const int64_t* img_off) {
  if (n_img < 0 || n_img >= (1 << 24)) return 4;
  if (!img_off) return 5;
  if (img_off[0] < 0) return 6;
  for (int64_t i = 0; i < n_img; ++i)
    if (img_off[i + 1] < img_off[i]) return 6;
  if (img_off[n_img] > FEAT_MAX_PIXELS) return 7;
  return 0;
}

// 0 when the images fit their slots: image i occupies h * w bytes from img_off[i] and ends at or before img_off[i + 1]
inline int feat_check_images(int64_t n_img, const int64_t* img_off, const int32_t* heights, const int32_t* widths) {
  const int why = feat_check_offsets(n_img, img_off);
  if (why) return why;
  if (n_img > 0 && (!heights || !widths)) return 5;
  for (int64_t i = 0; i < n_img; ++i) {
    if (heights[i] < 0 || widths[i] < 0) return 8;
    if ((int64_t)heights[i] * widths[i] > img_off[i + 1] - img_off[i]) return 9;
  }
  return 0;
}

inline const char* feat_rule_text(int why) {
  static const char* const rule[] = {"", "threshold must be in [1, 254]", "edge must be at least 16", "max_features must be >= 0",
                                     "n_img out of range", "null pointer", "img_off must ascend from a value >= 0",
                                     "more than 2^32 pixels", "negative height or width",
                                     "an image is larger than its slot of img_off"};
  return why >= 0 && why <= 9 ? rule[why] : "invalid argument";
}

// the table of a checked batch (feat_check_images == 0)
inline feat_plan feat_plan_images(int64_t n_img, const int64_t* img_off, const int32_t* heights, const int32_t* widths) {
  feat_plan P;
  P.img.resize((size_t)n_img);
  for (int64_t i = 0; i < n_img; ++i) {
    feat_image& m = P.img[(size_t)i];
    m.off = img_off[i];
    m.h = heights[i];
    m.w = widths[i];
    const bool ok = feat_eligible(m.h, m.w, FEAT_EDGE_MIN);
    const bool any = m.h > 0 && m.w > 0;
    m.row0 = (int32_t)P.rows;
    m.rows = ok ? m.h : 0;
    m.score_tile0 = (int32_t)P.score_tiles;
    m.score_tiles_x = ok ? (m.w + FEAT_TILE_W - 1) / FEAT_TILE_W : 0;
    m.blur_tile0 = (int32_t)P.blur_tiles;
    m.blur_tiles_x = any ? (m.w + FEAT_TILE_W - 1) / FEAT_TILE_W : 0;
    P.rows += m.rows;
    P.score_tiles += (int64_t)m.score_tiles_x * (ok ? (m.h + FEAT_SCORE_TILE_H - 1) / FEAT_SCORE_TILE_H : 0);
    P.blur_tiles += (int64_t)m.blur_tiles_x * (any ? (m.h + FEAT_BLUR_TILE_H - 1) / FEAT_BLUR_TILE_H : 0);
  }
  P.pixels = n_img > 0 ? img_off[n_img] : 0;
  return P;
}

// An eligible image is at least 2 * FEAT_EDGE_MIN + 1 = 33 pixels wide, so the row list of a buffer of `pixels` bytes has
// at most pixels / 33 entries whatever the images are: the workspace can be sized from img_off alone.
inline int64_t feat_cap_rows(int64_t pixels) { return pixels / (2 * FEAT_EDGE_MIN + 1); }

struct feat_layout {
  int64_t table;                      // feat_image [n_img]
  int64_t raw;                        // uint8 [pixels]: the FAST score map during detect, the blurred images during describe
  int64_t nms;                        // uint8 [pixels]: the score after suppression, border gate and mask (0 = no keypoint)
  int64_t row_cnt, row_off, row_tie;  // int32 [cap_rows + 1]: keypoints per row, their exclusive scan, ties before the row
  int64_t hist;                       // uint32 [n_img][256]
  int64_t cut;                        // int32 [n_img][2]: cut score (0 = keep all) and the number of ties that stay
  int64_t hdr;                        // int32 [1]: the edge of the detect call
  int64_t bytes;
};

inline int64_t feat_align(int64_t v) { return (v + 255) / 256 * 256; }

inline feat_layout feat_plan_layout(int64_t n_img, int64_t pixels) {
  feat_layout L;
  int64_t off = 0;
  auto take = [&](int64_t count, int64_t width) { const int64_t at = off; off += feat_align(count * width); return at; };
  const int64_t rows = feat_cap_rows(pixels) + 1;
  L.table = take(n_img, (int64_t)sizeof(feat_image));
  L.raw = take(pixels, 1);
  L.nms = take(pixels, 1);
  L.row_cnt = take(rows, 4);
  L.row_off = take(rows, 4);
  L.row_tie = take(rows, 4);
  L.hist = take(n_img * 256, 4);
  L.cut = take(n_img * 2, 4);
  L.hdr = take(1, 4);
  L.bytes = off + 256;
  return L;
}

// ------------------------------------------------------------------------------------------------ the sampling pattern
// The base table: 256 pairs (ax, ay, bx, by) drawn by a splitmix64 stream with a fixed seed.  A coordinate is the
// truncated mean of two uniform draws from [-13, 13] (a triangular, centre-weighted law); a pair is drawn again while an
// endpoint lies outside radius 13, both endpoints are equal, or the pair (in either direction) is in the table already.
// Integers only: the table is the same on every platform.
inline uint64_t feat_splitmix(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

inline int feat_draw_coord(uint64_t& s) {
  const int a = (int)(feat_splitmix(s) % 27) - 13, b = (int)(feat_splitmix(s) % 27) - 13;
  return (a + b) / 2;
}

inline void feat_default_pattern(int8_t base[FEAT_PAIRS][4]) {
  uint64_t s = 0x5F3759DF0B5EED01ull;
  for (int k = 0; k < FEAT_PAIRS;) {
    int p[4];
    for (int c = 0; c < 4; ++c) p[c] = feat_draw_coord(s);
    if (p[0] * p[0] + p[1] * p[1] > FEAT_PATTERN_R2 || p[2] * p[2] + p[3] * p[3] > FEAT_PATTERN_R2) continue;
    if (p[0] == p[2] && p[1] == p[3]) continue;
    bool seen = false;
    for (int j = 0; j < k && !seen; ++j)
      seen = (base[j][0] == p[0] && base[j][1] == p[1] && base[j][2] == p[2] && base[j][3] == p[3]) ||
             (base[j][0] == p[2] && base[j][1] == p[3] && base[j][2] == p[0] && base[j][3] == p[1]);
    if (seen) continue;
    for (int c = 0; c < 4; ++c) base[k][c] = (int8_t)p[c];
    ++k;
  }
}

inline bool feat_pattern_ok(const int8_t base[FEAT_PAIRS][4]) {
  for (int k = 0; k < FEAT_PAIRS; ++k)
    for (int e = 0; e < 2; ++e) {
      const int x = base[k][2 * e], y = base[k][2 * e + 1];
      if (x * x + y * y > FEAT_PATTERN_R2) return false;
    }
  return true;
}

// rot[bin] = the base table turned by 12 degrees * bin, each coordinate rounded half away from zero; bins 0 and 15 are the
// exact identity and its negative.  false (and rot untouched) for a table with an endpoint outside radius 13.
inline bool feat_rotate_pattern(const int8_t base[FEAT_PAIRS][4], int8_t rot[FEAT_BINS][FEAT_PAIRS][4]) {
  if (!feat_pattern_ok(base)) return false;
  // bins 0 .. 14 by the rotation; a half turn is the negative, and rounding half away from zero is odd, so bins 15 .. 29
  // are taken as the exact negatives of bins 0 .. 14 rather than from cos / sin of an angle beyond pi
  for (int b = 0; b < FEAT_BINS / 2; ++b) {
    const double th = b * (3.14159265358979323846 / 15.0);
    const double c = std::cos(th), s = std::sin(th);
    for (int k = 0; k < FEAT_PAIRS; ++k)
      for (int e = 0; e < 2; ++e) {
        const int x = base[k][2 * e], y = base[k][2 * e + 1];
        int rx = x, ry = y;
        if (b != 0) {
          const double xc = x * c, ys = y * s, xs = x * s, yc = y * c;
          rx = (int)std::round(xc - ys);
          ry = (int)std::round(xs + yc);
        }
        rot[b][k][2 * e] = (int8_t)rx;
        rot[b][k][2 * e + 1] = (int8_t)ry;
        rot[b + FEAT_BINS / 2][k][2 * e] = (int8_t)-rx;
        rot[b + FEAT_BINS / 2][k][2 * e + 1] = (int8_t)-ry;
      }
  }
  return true;
}

// the orientation bin of the moments (m10, m01): shared by the kernel's host restatement in the checks
inline int feat_angle_bin(int64_t m10, int64_t m01) {
  const double a = (m10 == 0 && m01 == 0) ? 0.0 : std::atan2((double)m01, (double)m10);
  const int q = (int)std::floor(a * 15.0 / 3.14159265358979323846 + 0.5);
  return ((q % FEAT_BINS) + FEAT_BINS) % FEAT_BINS;
}
