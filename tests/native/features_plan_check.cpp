// Host-only check of sfm_amd/csrc/features_plan.h, built with -fsanitize=address,undefined by tests/test_features_reference.py.
//   pattern  the default table: endpoints within radius 13, no degenerate pair, no pair twice, the same on every run;
//            the rotation: bin 0 the identity, bins 15 .. 29 the negatives, every rotated endpoint within 14 per axis
//            (so pattern + blur support stay inside FEAT_EDGE_MIN), a table with an endpoint at radius 14 refused
//   checks   options out of range, zero images, an image of 0 x 0, h = 2 edge, an img_off that does not ascend, an image
//            larger than its slot, negative sizes, null arrays
//   plan     rows / tiles of the table against a direct count; rows never exceed feat_cap_rows(pixels)
//   layout   the arrays of the workspace are 256-byte aligned, lie inside `bytes`, do not overlap and hold what the kernels
//            index
//   bins     feat_angle_bin on the axes and diagonals
// Prints "ok <cases>" or a diagnostic and exits 1.
#include "features_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static int fail(const char* what, long a, long b) { std::printf("FAIL %s %ld %ld\n", what, a, b); return 1; }

static int check_layout(int64_t n_img, int64_t pixels) {
  const feat_layout L = feat_plan_layout(n_img, pixels);
  const int64_t rows = feat_cap_rows(pixels) + 1;
  struct { int64_t at, bytes; } part[] = {
      {L.table, n_img * (int64_t)sizeof(feat_image)}, {L.raw, pixels}, {L.nms, pixels}, {L.row_cnt, rows * 4},
      {L.row_off, rows * 4}, {L.row_tie, rows * 4}, {L.hist, n_img * 256 * 4}, {L.cut, n_img * 8}, {L.hdr, 4}};
  int64_t end = 0;
  for (auto& p : part) {
    if (p.at % 256 != 0) return fail("alignment", (long)pixels, (long)p.at);
    if (p.at < end) return fail("overlap", (long)pixels, (long)p.at);
    end = p.at + p.bytes;
  }
  if (end > L.bytes) return fail("bytes", (long)end, (long)L.bytes);
  return 0;
}

int main(int argc, char** argv) {
  std::mt19937_64 rng(argc > 1 ? std::atoll(argv[1]) : 1);
  long cases = 0;
  // ---- pattern
  static int8_t base[FEAT_PAIRS][4], again[FEAT_PAIRS][4], rot[FEAT_BINS][FEAT_PAIRS][4];
  feat_default_pattern(base);
  feat_default_pattern(again);
  if (std::memcmp(base, again, sizeof(base)) != 0) return fail("generator not deterministic", 0, 0);
  for (int k = 0; k < FEAT_PAIRS; ++k) {
    const int8_t* p = base[k];
    if (p[0] * p[0] + p[1] * p[1] > FEAT_PATTERN_R2 || p[2] * p[2] + p[3] * p[3] > FEAT_PATTERN_R2) return fail("radius", k, 0);
    if (p[0] == p[2] && p[1] == p[3]) return fail("degenerate pair", k, 0);
    for (int j = 0; j < k; ++j) {
      const int8_t* q = base[j];
      if ((p[0] == q[0] && p[1] == q[1] && p[2] == q[2] && p[3] == q[3]) ||
          (p[0] == q[2] && p[1] == q[3] && p[2] == q[0] && p[3] == q[1])) return fail("pair twice", k, j);
    }
  }
  if (!feat_rotate_pattern(base, rot)) return fail("default table refused", 0, 0);
  if (std::memcmp(rot[0], base, sizeof(base)) != 0) return fail("bin 0 is not the identity", 0, 0);
  for (int b = 0; b < FEAT_BINS; ++b)
    for (int k = 0; k < FEAT_PAIRS; ++k)
      for (int c = 0; c < 4; ++c) {
        if (rot[b][k][c] != -rot[(b + 15) % FEAT_BINS][k][c]) return fail("half turn", b, k);
        if (std::abs((int)rot[b][k][c]) > 14) return fail("rotated endpoint beyond 14", b, k);
        if (std::abs((int)rot[b][k][c]) + 3 > FEAT_EDGE_MIN + 1) return fail("support beyond the gate", b, k);
        ++cases;
      }
  // rotation keeps lengths to within the rounding: |r'|^2 <= (13 + sqrt(1/2))^2 < 188
  for (int b = 0; b < FEAT_BINS; ++b)
    for (int k = 0; k < FEAT_PAIRS; ++k)
      for (int e = 0; e < 2; ++e) {
        const int x = rot[b][k][2 * e], y = rot[b][k][2 * e + 1];
        if (x * x + y * y >= 188) return fail("rotated length", b, k);
      }
  std::memcpy(again, base, sizeof(base));
  again[17][2] = 14; again[17][3] = 0;
  static int8_t untouched[FEAT_BINS][FEAT_PAIRS][4];
  std::memset(untouched, 77, sizeof(untouched));
  if (feat_rotate_pattern(again, untouched)) return fail("radius 14 accepted", 0, 0);
  for (size_t i = 0; i < sizeof(untouched); ++i)
    if (((int8_t*)untouched)[i] != 77) return fail("refused table written", (long)i, 0);
  again[17][2] = 10; again[17][3] = 9;      // 181 > 169
  if (feat_rotate_pattern(again, untouched)) return fail("radius^2 181 accepted", 0, 0);
  // ---- option checks
  if (feat_check_options(20, 31, 0) != 0 || feat_check_options(1, 16, 1) != 0 || feat_check_options(254, 16, 10000) != 0)
    return fail("options refused", 0, 0);
  if (feat_check_options(0, 31, 0) == 0 || feat_check_options(255, 31, 0) == 0) return fail("threshold", 0, 0);
  if (feat_check_options(20, 15, 0) == 0 || feat_check_options(20, -1, 0) == 0) return fail("edge", 0, 0);
  if (feat_check_options(20, 31, -1) == 0) return fail("max_features", 0, 0);
  // ---- degenerate batches
  {
    const int64_t off0[1] = {0};
    if (feat_check_images(0, off0, nullptr, nullptr) != 0) return fail("zero images refused", 0, 0);
    const feat_plan P = feat_plan_images(0, off0, nullptr, nullptr);
    if (P.rows || P.pixels || P.score_tiles || P.blur_tiles || !P.img.empty()) return fail("zero images plan", 0, 0);
    if (check_layout(0, 0)) return 1;
    if (feat_check_images(-1, off0, nullptr, nullptr) == 0) return fail("negative n_img", 0, 0);
    if (feat_check_offsets(1, nullptr) == 0) return fail("null img_off", 0, 0);
  }
  {
    const int64_t off[3] = {0, 0, 62 * 70};           // a 0 x 0 image, then h = 2 * edge at edge 31
    const int32_t hh[2] = {0, 62}, ww[2] = {0, 70};
    if (feat_check_images(2, off, hh, ww) != 0) return fail("0x0 refused", 0, 0);
    const feat_plan P = feat_plan_images(2, off, hh, ww);
    if (P.img[0].rows || P.img[0].score_tiles_x || P.img[0].blur_tiles_x) return fail("0x0 has work", 0, 0);
    if (feat_eligible(62, 70, 31) || !feat_eligible(63, 63, 31) || feat_eligible(63, 62, 31)) return fail("h = 2 edge", 0, 0);
    if (!feat_eligible(33, 33, 16) || feat_eligible(32, 40, 16)) return fail("edge 16", 0, 0);
    if (P.img[1].rows != 62 || P.rows != 62) return fail("rows at the smallest gate", (long)P.rows, 0);
    if (feat_check_images(2, off, nullptr, ww) == 0) return fail("null heights", 0, 0);
  }
  {
    const int64_t off[3] = {0, 100, 50};
    const int32_t hh[2] = {10, 5}, ww[2] = {10, 10};
    if (feat_check_images(2, off, hh, ww) == 0 || feat_check_offsets(2, off) == 0) return fail("descending img_off", 0, 0);
    const int64_t neg[2] = {-4, 10};
    if (feat_check_offsets(1, neg) == 0) return fail("negative img_off", 0, 0);
    const int64_t tight[2] = {0, 99};
    const int32_t h1[1] = {10}, w1[1] = {10}, hn[1] = {-1};
    if (feat_check_images(1, tight, h1, w1) == 0) return fail("image beyond its slot", 0, 0);
    if (feat_check_images(1, tight, hn, w1) == 0) return fail("negative height", 0, 0);
    const int64_t huge[2] = {0, FEAT_MAX_PIXELS + 1};
    if (feat_check_offsets(1, huge) == 0) return fail("2^32 pixels", 0, 0);
  }
  // ---- random batches: plan against a direct count, layout
  for (int it = 0; it < 300; ++it) {
    const int n = (int)(rng() % 9);
    std::vector<int64_t> off(n + 1, 0);
    std::vector<int32_t> hh(n), ww(n);
    int64_t rows = 0, st = 0, bt = 0;
    for (int i = 0; i < n; ++i) {
      hh[i] = (int32_t)(rng() % 5 == 0 ? rng() % 40 : rng() % 700);
      ww[i] = (int32_t)(rng() % 5 == 0 ? rng() % 40 : rng() % 900);
      off[i + 1] = off[i] + (int64_t)hh[i] * ww[i] + (int64_t)(rng() % 3);
      const bool ok = hh[i] >= 33 && ww[i] >= 33;
      if (ok) { rows += hh[i]; st += (int64_t)((ww[i] + 127) / 128) * ((hh[i] + 31) / 32); }
      if (hh[i] > 0 && ww[i] > 0) bt += (int64_t)((ww[i] + 127) / 128) * ((hh[i] + 15) / 16);
    }
    if (feat_check_images(n, off.data(), hh.data(), ww.data()) != 0) return fail("batch refused", it, 0);
    const feat_plan P = feat_plan_images(n, off.data(), hh.data(), ww.data());
    if (P.rows != rows || P.score_tiles != st || P.blur_tiles != bt || P.pixels != off[n]) return fail("plan", it, 0);
    if (P.rows > feat_cap_rows(P.pixels)) return fail("row list beyond its bound", (long)P.rows, (long)P.pixels);
    int64_t r = 0;
    for (int i = 0; i < n; ++i) {
      if (P.img[i].row0 != r || P.img[i].off != off[i]) return fail("table", it, i);
      r += P.img[i].rows;
    }
    if (check_layout(n, P.pixels)) return 1;
    ++cases;
  }
  for (int64_t px : {(int64_t)0, (int64_t)1, (int64_t)32, (int64_t)33, (int64_t)1089, (int64_t)36 * 1600 * 1200, FEAT_MAX_PIXELS})
    if (check_layout(36, px)) return 1;
  // ---- bins
  if (feat_angle_bin(0, 0) != 0 || feat_angle_bin(5, 0) != 0 || feat_angle_bin(5, 1) != 1 || feat_angle_bin(1, 5) != 7 ||
      feat_angle_bin(-5, 1) != 14 || feat_angle_bin(-5, -1) != 16 || feat_angle_bin(1, -5) != 23 || feat_angle_bin(5, 5) != 4 ||
      feat_angle_bin(-5, -5) != 19 || feat_angle_bin(5, -1) != 29)
    return fail("angle bin", feat_angle_bin(1, 5), feat_angle_bin(1, -5));
  int blur = 0;
  for (int k = 0; k < 7; ++k) blur += FEAT_BLUR_W[k];
  if (blur != 256) return fail("blur weights", blur, 0);
  std::printf("ok %ld\n", cases);
  return 0;
}
