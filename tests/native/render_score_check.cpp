// Host replay of the render score: render_score_rule.h and render_score_plan.h as render_score.hip uses them, one tile and
// one "thread" at a time, with every index checked.  Built by tests/test_render_score_reference.py, plain and with
// -fsanitize=address,undefined, and run stand-alone.
//   render_score_check plan              the argument checks, the tiles, the halos and the workspace over sizes 0, 1, W - 1, W,
//                                        tile - 1, tile, tile + 1, 2 tile + 3: every pixel produced exactly once, no staged
//                                        word and no offset outside its buffer; prints "ok <pixels walked>"
//   render_score_check score IN OUT      IN: int64 [6] n_view, channels, window, has_mask, has_depth, want_maps; double rel_tol;
//                                        int32 heights [n_view], widths [n_view]; color, triangle, depth, photos, then mask,
//                                        view_depth, view_keep where the header says so, views back to back.
//                                        OUT: stats int64 [n_view][16], then abs_error and ssim_map (float32 bits) if wanted
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "render_score_rule.h"
#include "render_score_plan.h"

#define REQUIRE(c)                                                        \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);          \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

namespace {

struct Inputs {
  int channels, window;
  double rel_tol;
  const uint8_t* color;
  const int32_t* triangle;
  const float* depth;
  const uint8_t* photos;
  const uint8_t* mask;
  const float* view_depth;
  const uint8_t* view_keep;
};

template <int CH, int W>
int window_of(const std::vector<uint32_t>& sr, const std::vector<uint32_t>& sp, int stride, int at, double* s) {
  REQUIRE(at >= 0 && at + (W - 1) * stride + (W - 1) < (int)sr.size());
  return render_score::window_ssim<CH, W>(sr.data(), sp.data(), stride, at, s);
}

template <int CH>
int window_any(int window, const std::vector<uint32_t>& sr, const std::vector<uint32_t>& sp, int stride, int at, double* s) {
  switch (window) {
    case 3: return window_of<CH, 3>(sr, sp, stride, at, s);
    case 5: return window_of<CH, 5>(sr, sp, stride, at, s);
    case 7: return window_of<CH, 7>(sr, sp, stride, at, s);
    case 9: return window_of<CH, 9>(sr, sp, stride, at, s);
    default: return window_of<CH, 11>(sr, sp, stride, at, s);
  }
}

// one view as the kernel walks it; produced counts how often a pixel was written.  n_elems: the pixels of all views
void score_view(const Inputs& in, const TsdfView& view, int64_t n_elems, int64_t* row, uint8_t* abs_error, uint32_t* ssim_map, std::vector<int>& produced) {
  const int w = view.w, h = view.h, CH = in.channels, W = in.window, R = W / 2;
  const int64_t tiles = render_score_tiles(h, w);
  std::vector<uint32_t> sr(RENDER_SCORE_STAGE_WORDS), sp(RENDER_SCORE_STAGE_WORDS);
  for (int k = 0; k < RENDER_SCORE_COLUMNS; ++k) row[k] = 0;
  row[RS_N_PIXELS] = (int64_t)h * w;
  for (int64_t t = 0; t < tiles; ++t) {
    const RenderScoreTile T = render_score_tile(t, w, W);
    REQUIRE(T.sw == RENDER_SCORE_TILE_W + 2 * R && T.sh == RENDER_SCORE_TILE_H + 2 * R && T.sw * T.sh <= RENDER_SCORE_STAGE_WORDS);
    REQUIRE(T.x0 >= 0 && T.x0 < w && T.y0 >= 0 && T.y0 < h);
    for (int i = 0; i < T.sw * T.sh; ++i) {
      const int x = T.sx0 + i % T.sw, y = T.sy0 + i / T.sw;
      uint32_t r = 0, p = 0;
      if (x >= 0 && x < w && y >= 0 && y < h) {
        const int64_t at = view.out_off + (int64_t)y * w + x;
        REQUIRE(at >= 0 && at < n_elems);
        const int covered = in.triangle[at] >= 0;
        const int compared = covered && (!in.mask || in.mask[at] > 0);
        const uint8_t* c = in.color + at * CH;
        const uint8_t* q = in.photos + at * CH;
        r = render_score::pack(c[0], CH == 3 ? c[1] : 0, CH == 3 ? c[2] : 0, (compared ? RENDER_SCORE_COMPARED : 0) | (covered ? RENDER_SCORE_COVERED : 0));
        p = render_score::pack(q[0], CH == 3 ? q[1] : 0, CH == 3 ? q[2] : 0, 0);
      }
      sr.at((size_t)i) = r;
      sp.at((size_t)i) = p;
    }
    for (int thread = 0; thread < RENDER_SCORE_BLOCK; ++thread) {
      const int lx = thread % RENDER_SCORE_TILE_W, ly = thread / RENDER_SCORE_TILE_W;
      const int x = T.x0 + lx, y = T.y0 + ly;
      if (!(x < w && y < h)) continue;
      const int64_t at = view.out_off + (int64_t)y * w + x;
      REQUIRE(at >= 0 && at < n_elems);
      produced.at((size_t)at) += 1;
      const uint32_t rc = sr.at((size_t)((ly + R) * T.sw + lx + R)), pc = sp.at((size_t)((ly + R) * T.sw + lx + R));
      const int f = render_score::flags(rc);
      const int compared = f & RENDER_SCORE_COMPARED;
      row[RS_N_COMPARED] += compared ? 1 : 0;
      for (int k = 0; k < CH; ++k) {
        const int e = render_score::channel(rc, k) - render_score::channel(pc, k);
        const int a = compared ? (e < 0 ? -e : e) : 0;
        row[RS_SAD + k] += a;
        row[RS_SSE + k] += a * a;
        if (abs_error) abs_error[at * CH + k] = (uint8_t)a;
      }
      uint32_t bits = RENDER_SCORE_NAN_BITS;
      if (compared && x >= R && x + R < w && y >= R && y + R < h) {
        double s;
        const int has = CH == 1 ? window_any<1>(W, sr, sp, T.sw, ly * T.sw + lx, &s) : window_any<3>(W, sr, sp, T.sw, ly * T.sw + lx, &s);
        if (has) {
          row[RS_N_SSIM] += 1;
          row[RS_Q_SSIM] += render_score::quantise(s);
          const float fl = (float)s;
          std::memcpy(&bits, &fl, 4);
        }
      }
      if (ssim_map) ssim_map[at] = bits;
      if (in.view_depth) {
        const float dv = in.view_depth[at];
        const int covered = (f & RENDER_SCORE_COVERED) != 0, seen = render_score::seen(in.view_keep[at], dv);
        if (covered && seen) {
          int agree;
          int64_t q;
          render_score::depth_term(in.depth[at], dv, in.rel_tol, &agree, &q);
          row[RS_N_BOTH] += 1;
          row[RS_N_AGREE] += agree;
          row[RS_Q_REL] += q;
        }
        row[RS_N_RENDER_ONLY] += covered && !seen;
        row[RS_N_VIEW_ONLY] += seen && !covered;
      }
    }
  }
}

int plan() {
  // the argument checks, branch by branch
  int32_t hs[3] = {3, 0, 9}, ws[3] = {5, 4, 70};
  TsdfView views[4];
  int64_t n_pix = -1, most = -1;
  REQUIRE(render_score_check_views(3, hs, ws, views, &n_pix, &most) == 0 && n_pix == 15 + 630 && most == 3 * 2);
  REQUIRE(views[0].out_off == 0 && views[1].out_off == 15 && views[2].out_off == 15 && views[3].out_off == 645 && views[2].h == 9 && views[2].w == 70);
  REQUIRE(render_score_check_views(0, nullptr, nullptr, views, &n_pix, &most) == 0 && n_pix == 0 && most == 0);
  REQUIRE(render_score_check_views(-1, hs, ws, nullptr, nullptr, nullptr) == 1 && render_score_check_views(65536, hs, ws, nullptr, nullptr, nullptr) == 1);
  REQUIRE(render_score_check_views(3, nullptr, ws, nullptr, nullptr, nullptr) == 8 && render_score_check_views(3, hs, nullptr, nullptr, nullptr, nullptr) == 8);
  int32_t bad_h[1] = {-1}, big_w[1] = {32769}, edge[1] = {32768};
  REQUIRE(render_score_check_views(1, bad_h, ws, nullptr, nullptr, nullptr) == 2 && render_score_check_views(1, hs, big_w, nullptr, nullptr, nullptr) == 2);
  REQUIRE(render_score_check_views(1, edge, edge, nullptr, &n_pix, &most) == 0 && n_pix == (1LL << 30) && most == 1024LL * 4096LL);
  const char one = 0;
  const void* there = &one;
  REQUIRE(render_score_check_options(1, 7, 0.02, nullptr, nullptr) == 0 && render_score_check_options(3, 3, 0.0, there, there) == 0);
  REQUIRE(render_score_check_options(3, 11, 1.0, nullptr, nullptr) == 0);
  REQUIRE(render_score_check_options(2, 7, 0.02, nullptr, nullptr) == 3 && render_score_check_options(0, 7, 0.02, nullptr, nullptr) == 3);
  REQUIRE(render_score_check_options(1, 1, 0.02, nullptr, nullptr) == 4 && render_score_check_options(1, 13, 0.02, nullptr, nullptr) == 4);
  REQUIRE(render_score_check_options(1, 6, 0.02, nullptr, nullptr) == 4 && render_score_check_options(1, -7, 0.02, nullptr, nullptr) == 4);
  REQUIRE(render_score_check_options(1, 7, -0.01, nullptr, nullptr) == 5 && render_score_check_options(1, 7, NAN, nullptr, nullptr) == 5);
  REQUIRE(render_score_check_options(1, 7, INFINITY, nullptr, nullptr) == 5);
  REQUIRE(render_score_check_options(1, 7, 0.02, there, nullptr) == 6 && render_score_check_options(1, 7, 0.02, nullptr, there) == 6);
  for (int64_t n = 0; n <= 65535; n += 4369) {
    const RenderScoreLayout L = render_score_layout(n);
    REQUIRE(L.views == 0 && L.views + (n + 1) * (int64_t)sizeof(TsdfView) <= L.bytes && L.bytes % 256 == 0);
    REQUIRE(render_score_check_buffers(n, 1, L.bytes, there, there, there, there, there, there, L.bytes) == 0);
    REQUIRE(render_score_check_buffers(n, 1, L.bytes, there, there, there, there, there, there, L.bytes - 1) == 7);
    REQUIRE(render_score_check_buffers(n, 1, L.bytes, there, there, there, there, there, nullptr, L.bytes) == 7);
  }
  REQUIRE(render_score_check_buffers(1, 0, 8, nullptr, nullptr, nullptr, nullptr, there, there, 8) == 0);
  REQUIRE(render_score_check_buffers(0, 0, 8, nullptr, nullptr, nullptr, nullptr, nullptr, there, 8) == 0);
  REQUIRE(render_score_check_buffers(1, 0, 8, nullptr, nullptr, nullptr, nullptr, nullptr, there, 8) == 8);
  REQUIRE(render_score_check_buffers(1, 1, 8, nullptr, there, there, there, there, there, 8) == 8 && render_score_check_buffers(1, 1, 8, there, nullptr, there, there, there, there, 8) == 8);
  REQUIRE(render_score_check_buffers(1, 1, 8, there, there, nullptr, there, there, there, 8) == 8 && render_score_check_buffers(1, 1, 8, there, there, there, nullptr, there, there, 8) == 8);

  // the tiles and their halos: every pixel once, every staged word and every window inside the staged arrays
  int64_t walked = 0;
  for (int window = RENDER_SCORE_MIN_WINDOW; window <= RENDER_SCORE_MAX_WINDOW; window += 2) {
    const int wide[] = {0, 1, window - 1, window, window + 1, RENDER_SCORE_TILE_W - 1, RENDER_SCORE_TILE_W, RENDER_SCORE_TILE_W + 1, 2 * RENDER_SCORE_TILE_W + 3};
    const int high[] = {0, 1, window - 1, window, window + 1, RENDER_SCORE_TILE_H - 1, RENDER_SCORE_TILE_H, RENDER_SCORE_TILE_H + 1, 2 * RENDER_SCORE_TILE_H + 3};
    for (int w : wide) {
      for (int h : high) {
        for (int ch = 1; ch <= 3; ch += 2) {
          const int64_t lead = 7;                                  // a view in front, so that out_off is not 0
          int32_t hh[2] = {1, h}, ww[2] = {(int32_t)lead, w};
          TsdfView v[3];
          int64_t n = 0;
          REQUIRE(render_score_check_views(2, hh, ww, v, &n, nullptr) == 0 && n == lead + (int64_t)h * w);
          std::vector<uint8_t> color((size_t)n * ch, 100), photos((size_t)n * ch, 90), err((size_t)n * ch, 0xAB);
          std::vector<int32_t> tri((size_t)n, 4);
          std::vector<float> depth((size_t)n, 2.0f), vd((size_t)n, 2.0f);
          std::vector<uint8_t> keep((size_t)n, 1);
          std::vector<uint32_t> map((size_t)n, 0xABABABABu);
          std::vector<int> produced((size_t)n, 0);
          Inputs in = {ch, window, 0.02, color.data(), tri.data(), depth.data(), photos.data(), nullptr, vd.data(), keep.data()};
          int64_t row[RENDER_SCORE_COLUMNS];
          score_view(in, v[1], n, row, err.data(), map.data(), produced);
          for (int64_t p = 0; p < n; ++p) REQUIRE(produced[(size_t)p] == (p < lead ? 0 : 1));
          for (int64_t p = 0; p < lead; ++p) REQUIRE(map[(size_t)p] == 0xABABABABu && err[(size_t)p * ch] == 0xAB);
          const int64_t windows = (h >= window && w >= window) ? (int64_t)(h - window + 1) * (w - window + 1) : 0;
          REQUIRE(row[RS_N_PIXELS] == (int64_t)h * w && row[RS_N_COMPARED] == (int64_t)h * w && row[RS_N_SSIM] == windows);
          REQUIRE(row[RS_SAD] == 10LL * h * w && row[RS_SSE] == 100LL * h * w && row[RS_N_BOTH] == (int64_t)h * w && row[RS_N_AGREE] == (int64_t)h * w);
          REQUIRE(row[RS_SAD + 2] == (ch == 3 ? 10LL * h * w : 0) && row[RS_Q_REL] == 0 && row[15] == 0);
          walked += (int64_t)h * w;
        }
      }
    }
  }
  std::printf("ok %lld\n", (long long)walked);
  return 0;
}

std::vector<char> read_all(const char* path) {
  FILE* f = std::fopen(path, "rb");
  REQUIRE(f != nullptr);
  std::vector<char> out;
  char buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
  std::fclose(f);
  return out;
}

template <class T>
std::vector<T> take(const std::vector<char>& raw, size_t& at, size_t n) {
  REQUIRE(at + n * sizeof(T) <= raw.size());
  std::vector<T> out(n + 1);                                       // one spare element: data() of an empty array is still a pointer
  if (n) std::memcpy(out.data(), raw.data() + at, n * sizeof(T));
  at += n * sizeof(T);
  return out;
}

int score(const char* fin, const char* fout) {
  const std::vector<char> raw = read_all(fin);
  size_t at = 0;
  const std::vector<int64_t> head = take<int64_t>(raw, at, 6);
  const std::vector<double> tol = take<double>(raw, at, 1);
  const int64_t n_view = head[0];
  const int ch = (int)head[1], window = (int)head[2];
  const std::vector<int32_t> hs = take<int32_t>(raw, at, (size_t)n_view), ws = take<int32_t>(raw, at, (size_t)n_view);
  std::vector<TsdfView> views((size_t)n_view + 1);
  int64_t n = 0;
  REQUIRE(render_score_check_views(n_view, hs.data(), ws.data(), views.data(), &n, nullptr) == 0);
  const std::vector<uint8_t> color = take<uint8_t>(raw, at, (size_t)n * ch);
  const std::vector<int32_t> tri = take<int32_t>(raw, at, (size_t)n);
  const std::vector<float> depth = take<float>(raw, at, (size_t)n);
  const std::vector<uint8_t> photos = take<uint8_t>(raw, at, (size_t)n * ch);
  std::vector<uint8_t> mask, keep;
  std::vector<float> vd;
  if (head[3]) mask = take<uint8_t>(raw, at, (size_t)n);
  if (head[4]) { vd = take<float>(raw, at, (size_t)n); keep = take<uint8_t>(raw, at, (size_t)n); }
  REQUIRE(at == raw.size());
  REQUIRE(render_score_check_options(ch, window, tol[0], head[4] ? vd.data() : nullptr, head[4] ? keep.data() : nullptr) == 0);
  Inputs in = {ch, window, tol[0], color.data(), tri.data(), depth.data(), photos.data(), head[3] ? mask.data() : nullptr,
               head[4] ? vd.data() : nullptr, head[4] ? keep.data() : nullptr};
  std::vector<int64_t> stats((size_t)n_view * RENDER_SCORE_COLUMNS + 1);
  std::vector<uint8_t> err((size_t)n * ch + 1);
  std::vector<uint32_t> map((size_t)n + 1);
  std::vector<int> produced((size_t)n + 1, 0);
  for (int64_t v = 0; v < n_view; ++v)
    score_view(in, views[(size_t)v], n, stats.data() + v * RENDER_SCORE_COLUMNS, head[5] ? err.data() : nullptr, head[5] ? map.data() : nullptr, produced);
  for (int64_t p = 0; p < n; ++p) REQUIRE(produced[(size_t)p] == 1);
  FILE* f = std::fopen(fout, "wb");
  REQUIRE(f != nullptr);
  std::fwrite(stats.data(), 8, (size_t)n_view * RENDER_SCORE_COLUMNS, f);
  if (head[5]) {
    std::fwrite(err.data(), 1, (size_t)n * ch, f);
    std::fwrite(map.data(), 4, (size_t)n, f);
  }
  std::fclose(f);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "plan")) return plan();
  if (argc == 4 && !std::strcmp(argv[1], "score")) return score(argv[2], argv[3]);
  std::printf("usage: render_score_check plan | score IN OUT\n");
  return 2;
}
