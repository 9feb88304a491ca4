// Host-only check of sfm_amd/csrc/features_pyramid_plan.h, built with -fsanitize=address,undefined by
// tests/test_features_pyramid_reference.py.
//   options  every (n_levels, num, den) in a box around the allowed set against the rule's text
//   sizes    the level tables over degenerate and random batches - zero images, 0 x 0, 1 x 1, 1 x w and h x 1 images, sides
//            around 33 and around every tile constant, every allowed num/den: levels never grow, a side of at least 33
//            strictly shrinks, slots back to back that fill lvl_off exactly
//   tiles    every tile of every level inside its level, the tiles of a level tile it, tile0 ascending; the copy chunks of
//            level 0 cover the image
//   taps     x0, x1, y0, y1 of every destination pixel inside the source, the weight in [0, 255], the 32-bit and the 64-bit
//            branch of pyr_tap equal where both apply (sides up to 2^31 - 1 at the extremes)
//   map      pyr_map is exactly x at level 0, monotone, and within [-0.5, n0 - 0.5]
//   layout   the arrays of both workspaces are 256-byte aligned, lie inside `bytes` and do not overlap
//   values   argv[2], written by the Python test: cases of (hs, ws, hd, wd, mask, source, expected); pyr_resample_host must
//            give `expected` byte for byte
// Prints "ok <cases>" or a diagnostic and exits 1.
#include "features_pyramid_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static int fail(const char* what, long a, long b) { std::printf("FAIL %s %ld %ld\n", what, a, b); return 1; }

static bool allowed(int64_t n_levels, int64_t num, int64_t den) {
  return n_levels >= 2 && n_levels <= 16 && den >= 1 && den < num && num <= 2 * den && num <= 16 && 8 * num >= 9 * den;
}

static int check_taps(int32_t nd, int32_t ns, bool every) {
  const int64_t step = every ? 1 : (nd / 997 + 1);
  for (int64_t x = 0; x < nd; x += step) {
    int32_t i0, i1, f;
    pyr_tap((int32_t)x, nd, ns, &i0, &i1, &f);
    if (i0 < 0 || i0 >= ns || i1 < i0 || i1 >= ns || i1 > i0 + 1) return fail("tap outside the source", (long)x, (long)i0);
    if (f < 0 || f > 255) return fail("weight", (long)x, (long)f);
    const int64_t u = (2 * x + 1) * ns - nd, d = 2 * (int64_t)nd;
    if (i0 != u / d || f != ((u % d) * 256) / d) return fail("tap differs from the int64 rule", (long)x, (long)nd);
    if (x + step >= nd && x != nd - 1) x = nd - 1 - step;      // always the last pixel too
  }
  return 0;
}

static int check_batch(const std::vector<int32_t>& hs, const std::vector<int32_t>& ws, int n_levels, int num, int den,
                       bool taps, long* cases) {
  const int64_t n_img = (int64_t)hs.size();
  const size_t slots = (size_t)(n_img * n_levels);
  std::vector<int64_t> off(slots + 1, -1), img_off((size_t)n_img + 1, 0);
  std::vector<int32_t> lh(slots, -1), lw(slots, -1);
  for (int64_t i = 0; i < n_img; ++i) img_off[(size_t)i + 1] = img_off[(size_t)i] + (int64_t)hs[(size_t)i] * ws[(size_t)i] + (i % 3);
  const int why = pyr_plan_sizes(n_img, hs.data(), ws.data(), n_levels, num, den, off.data(), lh.data(), lw.data());
  if (why) return fail("sizes refused", why, (long)n_img);
  int64_t at = 0;
  for (int64_t i = 0; i < n_img; ++i)
    for (int l = 0; l < n_levels; ++l) {
      const size_t s = (size_t)(i * n_levels + l);
      if (off[s] != at) return fail("slot does not follow the one before", (long)s, (long)off[s]);
      at += (int64_t)lh[s] * lw[s];
      if (l == 0) {
        if (lh[s] != hs[(size_t)i] || lw[s] != ws[(size_t)i]) return fail("level 0 is not the image", (long)i, 0);
        continue;
      }
      const int32_t side[2][2] = {{lh[s - 1], lh[s]}, {lw[s - 1], lw[s]}};
      for (auto& p : side) {
        if (p[1] > p[0]) return fail("a level grows", p[0], p[1]);
        if (p[0] >= 33 && p[1] >= p[0]) return fail("a side of at least 33 does not shrink", p[0], p[1]);
        if (p[0] >= 1 && p[1] < 1) return fail("a side vanishes", p[0], p[1]);
        if (p[0] == 0 && p[1] != 0) return fail("an empty side grows", p[0], p[1]);
        const int64_t want = p[0] == 0 ? 0 : std::max<int64_t>(1, (2 * (int64_t)p[0] * den + num) / (2 * num));
        if (p[1] != want) return fail("size rule", p[0], p[1]);
      }
    }
  if (off[slots] != at) return fail("lvl_off does not end at the sum", (long)off[slots], (long)at);
  const pyr_plan P = pyr_plan_tiles(n_img, img_off.data(), n_levels, off.data(), lh.data(), lw.data());
  if (P.pixels != at || (int64_t)P.entry.size() != n_img * n_levels) return fail("plan extent", (long)P.pixels, (long)at);
  for (int l = 0; l < n_levels; ++l) {
    int64_t tile = 0;
    for (int64_t i = 0; i < n_img; ++i) {
      const pyr_entry& e = P.entry[(size_t)(l * n_img + i)];
      const size_t s = (size_t)(i * n_levels + l);
      if (e.tile0 != tile) return fail("tile0", l, (long)i);
      if (e.dst != off[s] || e.hd != lh[s] || e.wd != lw[s]) return fail("entry destination", l, (long)i);
      if (e.dst + (int64_t)e.hd * e.wd > off[s + 1]) return fail("level leaves its slot", l, (long)i);
      if (l == 0) {
        if (e.src != img_off[(size_t)i] || e.hs != e.hd || e.ws != e.wd) return fail("level 0 source", 0, (long)i);
        const int64_t n = (int64_t)e.hd * e.wd;
        if ((int64_t)e.tiles_x * PYR_COPY_CHUNK < n || ((int64_t)e.tiles_x - 1) * PYR_COPY_CHUNK >= n + (n == 0))
          return fail("copy chunks", (long)n, e.tiles_x);
        if (e.src + n > img_off[(size_t)i + 1]) return fail("copy leaves the image slot", 0, (long)i);
        tile += e.tiles_x;
        continue;
      }
      if (e.src != off[s - 1] || e.hs != lh[s - 1] || e.ws != lw[s - 1]) return fail("entry source", l, (long)i);
      const int64_t ty = e.tiles_x ? (e.hd + PYR_TILE_H - 1) / PYR_TILE_H : 0;
      if (e.hd > 0 && e.wd > 0) {
        if ((int64_t)e.tiles_x * PYR_TILE_W < e.wd || ((int64_t)e.tiles_x - 1) * PYR_TILE_W >= e.wd) return fail("tiles_x", e.wd, e.tiles_x);
        if (ty * PYR_TILE_H < e.hd || (ty - 1) * PYR_TILE_H >= e.hd) return fail("tiles_y", e.hd, (long)ty);
        if (e.hs < e.hd || e.ws < e.wd) return fail("source smaller than destination", l, (long)i);
        if (taps && (check_taps(e.wd, e.ws, e.wd < 4096) || check_taps(e.hd, e.hs, e.hd < 4096))) return 1;
      } else if (e.tiles_x != 0) {
        return fail("tiles of an empty level", l, (long)i);
      }
      tile += (int64_t)e.tiles_x * ty;
    }
    if (P.tiles[(size_t)l] != tile) return fail("tiles of a level", l, (long)tile);
  }
  ++*cases;
  return 0;
}

static int check_layouts(int64_t n_img, int64_t n_levels) {
  const pyr_layout A = pyr_plan_layout(n_img, n_levels);
  if (A.table % 256 != 0 || A.table + n_img * n_levels * (int64_t)sizeof(pyr_entry) > A.bytes) return fail("pyramid layout", (long)n_img, (long)n_levels);
  const merge_layout L = merge_plan_layout(n_img, n_levels);
  struct { int64_t at, bytes; } part[] = {{L.dims, n_img * n_levels * 8}, {L.cut, n_img * 8}, {L.cnt, (n_img + 1) * 4}};
  int64_t end = 0;
  for (auto& p : part) {
    if (p.at % 256 != 0) return fail("alignment", (long)n_img, (long)p.at);
    if (p.at < end) return fail("overlap", (long)n_img, (long)p.at);
    end = p.at + p.bytes;
  }
  if (end > L.bytes) return fail("bytes", (long)end, (long)L.bytes);
  return 0;
}

static int check_values(const char* path, long* cases) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return fail("cannot open the value file", 0, 0);
  int32_t n = 0;
  if (std::fread(&n, 4, 1, f) != 1) { std::fclose(f); return fail("value file header", 0, 0); }
  for (int32_t c = 0; c < n; ++c) {
    int32_t hdr[5];
    if (std::fread(hdr, 4, 5, f) != 5) { std::fclose(f); return fail("value file case header", c, 0); }
    const int32_t hs = hdr[0], ws = hdr[1], hd = hdr[2], wd = hdr[3];
    if (hs < 1 || ws < 1 || hd < 1 || wd < 1 || hd > hs || wd > ws || hs > 4096 || ws > 4096) { std::fclose(f); return fail("value file sizes", c, 0); }
    std::vector<uint8_t> src((size_t)hs * ws), want((size_t)hd * wd), got((size_t)hd * wd);
    if (std::fread(src.data(), 1, src.size(), f) != src.size() || std::fread(want.data(), 1, want.size(), f) != want.size()) {
      std::fclose(f);
      return fail("value file body", c, 0);
    }
    pyr_resample_host(src.data(), hs, ws, got.data(), hd, wd, hdr[4] != 0);
    for (size_t k = 0; k < got.size(); ++k)
      if (got[k] != want[k]) { std::fclose(f); return fail("resampled value", c, (long)k); }
    ++*cases;
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  std::mt19937_64 rng(argc > 1 ? std::atoll(argv[1]) : 1);
  long cases = 0;
  // ---- options
  std::vector<std::pair<int, int>> scales;
  for (int n_levels = -1; n_levels <= 18; ++n_levels)
    for (int num = -1; num <= 34; ++num)
      for (int den = -1; den <= 18; ++den) {
        const int why = pyr_check_options(n_levels, num, den);
        if ((why == 0) != allowed(n_levels, num, den)) return fail("options", num, den);
        if (why && !pyr_rule_text(why)[0]) return fail("no text for a rule", why, 0);
        if (!why && n_levels == 2) scales.push_back({num, den});
        ++cases;
      }
  if (pyr_check_options(1, 6, 5) != 1 || pyr_check_options(17, 6, 5) != 1 || pyr_check_options(8, 5, 5) != 2 ||
      pyr_check_options(8, 11, 5) != 2 || pyr_check_options(8, 17, 9) != 3 || pyr_check_options(8, 10, 9) != 4)
    return fail("rule numbers", 0, 0);
  // ---- sizes, tiles and taps: the named sizes at every allowed scale and at 2 and 16 levels
  const std::vector<int32_t> named = {0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 34, 35, 63, 64, 65, PYR_TILE_H - 1, PYR_TILE_H + 1,
                                      2 * PYR_TILE_H, PYR_TILE_W - 1, PYR_TILE_W, PYR_TILE_W + 1, 2 * PYR_TILE_W - 1, 2 * PYR_TILE_W,
                                      2 * PYR_TILE_W + 1, FEAT_TILE_W - 1, FEAT_TILE_W + 1, 240, 1200, 1600};
  for (auto& sc : scales)
    for (int n_levels : {2, 16}) {
      std::vector<int32_t> hs, ws;
      for (size_t k = 0; k < named.size(); ++k) {
        hs.push_back(named[k]); ws.push_back(named[(k * 7 + 3) % named.size()]);
        hs.push_back(named[k]); ws.push_back(1);
        hs.push_back(1); ws.push_back(named[k]);
      }
      if (check_batch(hs, ws, n_levels, sc.first, sc.second, sc.first - sc.second <= 1 || sc.first == 2 * sc.second, &cases)) return 1;
    }
  {
    std::vector<int32_t> none;
    if (check_batch(none, none, 8, 6, 5, true, &cases)) return 1;
    int64_t off1[1] = {-1};
    if (pyr_plan_sizes(0, nullptr, nullptr, 8, 6, 5, off1, nullptr, nullptr) != 0 || off1[0] != 0) return fail("zero images", 0, 0);
    int32_t neg[1] = {-1}, one[1] = {1}, lh[8], lw[8];
    int64_t off[9];
    if (pyr_plan_sizes(1, neg, one, 8, 6, 5, off, lh, lw) != 7 || pyr_plan_sizes(1, one, neg, 8, 6, 5, off, lh, lw) != 7) return fail("negative size accepted", 0, 0);
    if (pyr_plan_sizes(1, one, one, 8, 6, 5, nullptr, lh, lw) != 6 || pyr_plan_sizes(1, nullptr, one, 8, 6, 5, off, lh, lw) != 6) return fail("null accepted", 0, 0);
    if (pyr_plan_sizes(-1, one, one, 8, 6, 5, off, lh, lw) != 5) return fail("negative n_img accepted", 0, 0);
    int32_t big[1] = {1 << 16};
    int64_t boff[3];
    int32_t bh[2], bw[2];
    if (pyr_plan_sizes(1, big, big, 2, 9, 8, boff, bh, bw) != 8) return fail("more than 2^32 pixels accepted", 0, 0);
  }
  // ---- random batches
  for (int it = 0; it < 40; ++it) {
    const auto sc = scales[rng() % scales.size()];
    const int n_levels = 2 + (int)(rng() % 15), n_img = (int)(rng() % 6);
    std::vector<int32_t> hs, ws;
    for (int i = 0; i < n_img; ++i) {
      const int kind = (int)(rng() % 4);
      hs.push_back(kind == 0 ? (int32_t)(rng() % 4) : kind == 1 ? 30 + (int32_t)(rng() % 8) : 1 + (int32_t)(rng() % 700));
      ws.push_back(kind == 0 ? (int32_t)(rng() % 70) : kind == 1 ? 30 + (int32_t)(rng() % 8) : 1 + (int32_t)(rng() % 900));
    }
    if (check_batch(hs, ws, n_levels, sc.first, sc.second, true, &cases)) return 1;
  }
  // ---- taps at the extremes: the largest sides, where only the 64-bit branch applies, and the switch between the two
  for (auto& sc : scales) {
    for (int32_t ns : {2147483647, 1 << 30, (1 << 23) + 1, 1 << 23, (1 << 23) - 1, 46341, 65536}) {
      const int32_t nd = pyr_next_size(ns, sc.first, sc.second);
      if (nd < 1 || nd > ns) return fail("next size", ns, nd);
      if (check_taps(nd, ns, false)) return 1;
      ++cases;
    }
  }
  // ---- the coordinate map
  for (int32_t n0 : {1, 33, 240, 1600, 1 << 20}) {
    for (int x = 0; x < n0 && x < 5000; ++x)
      if (pyr_map(x, n0, n0) != (float)x) return fail("map at level 0", n0, x);
    int32_t nl = n0;
    for (int l = 1; l < 8; ++l) {
      nl = pyr_next_size(nl, 6, 5);
      float before = -1.0f;
      for (int x = 0; x < nl; ++x) {
        const float v = pyr_map(x, n0, nl);
        if (!(v >= -0.5f && v <= (float)n0 - 0.5f)) return fail("map outside the image", n0, x);
        if (!(v >= before)) return fail("map not monotone", n0, x);
        before = v;
      }
      ++cases;
    }
  }
  // ---- layouts
  for (int64_t n_img : {0, 1, 2, 36, 1000})
    for (int64_t n_levels : {2, 8, 16}) {
      if (check_layouts(n_img, n_levels)) return 1;
      ++cases;
    }
  if (argc > 2 && check_values(argv[2], &cases)) return 1;
  std::printf("ok %ld\n", cases);
  return 0;
}
