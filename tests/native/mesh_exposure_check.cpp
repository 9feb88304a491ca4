// Host build of the exposure rule and plan (sfm_amd/csrc/mesh_exposure_rule.h, mesh_exposure_plan.h) for
// tests/test_mesh_exposure_reference.py.
//   mesh_exposure_check scene IN OUT  IN: the scene file of mesh_color_check (int64 n_ref, channels, n_vertices, has_keep, fill;
//                                     double tol, min_cos; int32 heights, widths; double proj, centres; float depth; uint8 keep
//                                     (when has_keep); uint8 pixels; double vertices; float normals).
//                                     OUT: uint8 seen[n_ref][nv], uint8 samples[n_ref][channels][nv], int64 overlap[n_ref][n_ref],
//                                     int64 sums[n_ref][n_ref][channels].  The tables are made the way k_exposure_gram makes
//                                     them: tile by tile and chunk by chunk from the 0 / 1 and the signed operand words, an
//                                     int32 sum per workgroup, sums = product + 128 * overlap.
//   mesh_exposure_check rule IN OUT   IN: int64 n_s, n_g, n_w; double s[n_s]; double g[n_g]; uint8 value[n_g]; uint32
//                                     seen4[n_w], q4[n_w].  OUT: uint8 quantise(s)[n_s], uint8 gain(value, g)[n_g], uint32
//                                     flags01[n_w], uint32 signed4[n_w].
//   mesh_exposure_check plan          every branch of the argument checks, the tiles and chunks, the windows of the gain pass;
//                                     prints "ok <cases>"
// Build with -ffp-contract=off (the headers' pragma is clang's).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "mesh_exposure_plan.h"
#include "mesh_exposure_rule.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

template <typename T>
static std::vector<T> read_n(std::FILE* f, int64_t n) {
  std::vector<T> v((size_t)n);
  REQUIRE(n == 0 || std::fread(v.data(), sizeof(T), (size_t)n, f) == (size_t)n);
  return v;
}

template <typename T>
static void write_all(std::FILE* f, const std::vector<T>& v) {
  REQUIRE(v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size());
}

// the 16 bytes load16 of mesh_exposure.hip gives: zeros past the row's end
static void load16(const uint8_t* row, int64_t n, int64_t v, uint32_t w[4]) {
  w[0] = w[1] = w[2] = w[3] = 0u;
  for (int k = 0; k < 16; ++k)
    if (v + k < n) w[k >> 2] |= (uint32_t)row[v + k] << (8 * (k & 3));
}

// the sum over 16 k of (int8)a * (int8)b, as the matrix core forms it
static int32_t dot16(const uint32_t a[4], const uint32_t b[4]) {
  int32_t s = 0;
  for (int k = 0; k < 16; ++k) s += (int32_t)(int8_t)(a[k >> 2] >> (8 * (k & 3))) * (int32_t)(int8_t)(b[k >> 2] >> (8 * (k & 3)));
  return s;
}

// k_exposure_gram on the host: every workgroup of the plan, its int32 tile, then the int64 tables
static void gram(int n_ref, int ch, int64_t nv, const uint8_t* seen, const uint8_t* samples, std::vector<int64_t>& overlap, std::vector<int64_t>& sums) {
  const int T = MESH_EXPOSURE_TILE;
  const int64_t tiles = mesh_exposure_tiles(n_ref), chunks = mesh_exposure_chunks(nv);
  for (int64_t c = 0; c < chunks; ++c)
    for (int64_t tp = 0; tp < tiles * tiles; ++tp) {
      const int ti = (int)(tp / tiles), tj = (int)(tp % tiles);
      const int64_t c0 = c * MESH_EXPOSURE_CHUNK, c1 = c0 + MESH_EXPOSURE_CHUNK < nv ? c0 + MESH_EXPOSURE_CHUNK : nv;
      for (int r = 0; r < T; ++r)
        for (int q = 0; q < T; ++q) {
          const int gi = ti * T + r, gj = tj * T + q;
          if (gi >= n_ref || gj >= n_ref) continue;
          int64_t o = 0, s[3] = {0, 0, 0};
          for (int64_t v = c0; v < c1; v += 16) {
            uint32_t fi[4], fj[4], a01[4], b01[4];
            load16(seen + (int64_t)gi * nv, nv, v, fi);
            load16(seen + (int64_t)gj * nv, nv, v, fj);
            for (int w = 0; w < 4; ++w) { a01[w] = mesh_exposure::flags01(fi[w]); b01[w] = mesh_exposure::flags01(fj[w]); }
            o += dot16(a01, b01);
            for (int k = 0; k < ch; ++k) {
              uint32_t qw[4], sw[4];
              load16(samples + ((int64_t)gi * ch + k) * nv, nv, v, qw);
              for (int w = 0; w < 4; ++w) sw[w] = mesh_exposure::signed4(qw[w], a01[w]);
              s[k] += dot16(sw, b01);
            }
          }
          REQUIRE(o >= 0 && o <= MESH_EXPOSURE_CHUNK);
          for (int k = 0; k < ch; ++k) REQUIRE(s[k] >= -128LL * MESH_EXPOSURE_CHUNK && s[k] <= 127LL * MESH_EXPOSURE_CHUNK);      // an int32 holds it
          overlap[(size_t)((int64_t)gi * n_ref + gj)] += o;
          for (int k = 0; k < ch; ++k) {
            REQUIRE(s[k] + 128 * o >= 0);
            sums[(size_t)(((int64_t)gi * n_ref + gj) * ch + k)] += s[k] + 128 * o;
          }
        }
    }
}

static int run_scene(const char* in, const char* out) {
  std::FILE* fi = std::fopen(in, "rb");
  REQUIRE(fi);
  const std::vector<int64_t> head = read_n<int64_t>(fi, 5);
  const int n_ref = (int)head[0], ch = (int)head[1];
  const int64_t nv = head[2];
  const bool has_keep = head[3] != 0;
  const std::vector<double> scal = read_n<double>(fi, 2);
  const std::vector<int32_t> heights = read_n<int32_t>(fi, n_ref), widths = read_n<int32_t>(fi, n_ref);
  REQUIRE(mesh_exposure_check(n_ref, ch, nv) == 0 && mesh_color_check(ch, nv, scal[0], scal[1], 0) == 0);
  std::vector<int32_t> refs((size_t)n_ref);
  for (int r = 0; r < n_ref; ++r) refs[(size_t)r] = r;
  std::vector<TsdfView> views((size_t)n_ref + 1);
  REQUIRE(tsdf_check_views(n_ref, heights.data(), widths.data(), n_ref, refs.data(), views.data()) == 0);
  int64_t n_out = 0;
  for (int r = 0; r < n_ref; ++r) n_out += (int64_t)heights[(size_t)r] * widths[(size_t)r];
  views[(size_t)n_ref] = TsdfView{n_out, 0, 0};
  const std::vector<double> proj = read_n<double>(fi, (int64_t)n_ref * 12), centres = read_n<double>(fi, (int64_t)n_ref * 3);
  const std::vector<float> depth = read_n<float>(fi, n_out);
  const std::vector<uint8_t> keep = read_n<uint8_t>(fi, has_keep ? n_out : 0);
  const std::vector<uint8_t> pixels = read_n<uint8_t>(fi, n_out * ch);
  const std::vector<double> X = read_n<double>(fi, nv * 3);
  const std::vector<float> N = read_n<float>(fi, nv * 3);
  std::fclose(fi);
  std::vector<uint8_t> seen((size_t)(n_ref * nv), 0xAB), samples((size_t)(n_ref * nv * ch), 0xAB);
  for (int64_t i = 0; i < nv; ++i) {
    const double n[3] = {(double)N[(size_t)(3 * i)], (double)N[(size_t)(3 * i + 1)], (double)N[(size_t)(3 * i + 2)]};
    for (int v = 0; v < n_ref; ++v) {
      const TsdfView view = views[(size_t)v];
      const mesh_color::Projection p = mesh_color::project(proj.data() + (int64_t)v * 12, X[(size_t)(3 * i)], X[(size_t)(3 * i + 1)], X[(size_t)(3 * i + 2)], view.w, view.h);
      bool use = false;
      double wgt = 0.0;
      if (p.valid) {
        const int64_t e = view.out_off + (int64_t)p.yi * view.w + p.xi;
        REQUIRE(e >= view.out_off && e < views[(size_t)v + 1].out_off);
        use = mesh_color::sees((double)depth[(size_t)e], has_keep ? keep[(size_t)e] != 0 : 1, p.q2, scal[0]) &&
              mesh_color::weight(centres.data() + (int64_t)v * 3, X.data() + 3 * i, n, scal[1], &wgt);
      }
      seen[(size_t)((int64_t)v * nv + i)] = use ? 1 : 0;
      mesh_color::Taps t = {};
      if (use) {
        t = mesh_color::taps(p.u, p.v, view.w, view.h);
        REQUIRE(t.x0 >= 0 && t.x0 <= t.x1 && t.x1 < view.w && t.y0 >= 0 && t.y0 <= t.y1 && t.y1 < view.h);
      }
      const uint8_t* img = pixels.data() + view.out_off * ch;
      for (int k = 0; k < ch; ++k) {
        uint8_t q = 0;
        if (use) {
          const double a = (double)img[((int64_t)t.y0 * view.w + t.x0) * ch + k], b = (double)img[((int64_t)t.y0 * view.w + t.x1) * ch + k];
          const double c = (double)img[((int64_t)t.y1 * view.w + t.x0) * ch + k], d = (double)img[((int64_t)t.y1 * view.w + t.x1) * ch + k];
          q = mesh_exposure::quantise(mesh_color::bilinear(a, b, c, d, t.fx, t.fy));
        }
        samples[(size_t)(((int64_t)v * ch + k) * nv + i)] = q;
      }
    }
  }
  std::vector<int64_t> overlap((size_t)n_ref * (size_t)n_ref, 0), sums((size_t)n_ref * (size_t)n_ref * (size_t)ch, 0);
  gram(n_ref, ch, nv, seen.data(), samples.data(), overlap, sums);
  std::FILE* fo = std::fopen(out, "wb");
  REQUIRE(fo);
  write_all(fo, seen);
  write_all(fo, samples);
  write_all(fo, overlap);
  write_all(fo, sums);
  std::fclose(fo);
  return 0;
}

static int run_rule(const char* in, const char* out) {
  std::FILE* fi = std::fopen(in, "rb");
  REQUIRE(fi);
  const std::vector<int64_t> head = read_n<int64_t>(fi, 3);
  const std::vector<double> s = read_n<double>(fi, head[0]), g = read_n<double>(fi, head[1]);
  const std::vector<uint8_t> value = read_n<uint8_t>(fi, head[1]);
  const std::vector<uint32_t> seen4 = read_n<uint32_t>(fi, head[2]), q4 = read_n<uint32_t>(fi, head[2]);
  std::fclose(fi);
  std::vector<uint8_t> qs(s.size()), gs(g.size());
  std::vector<uint32_t> f(seen4.size()), sg(seen4.size());
  for (size_t i = 0; i < s.size(); ++i) qs[i] = mesh_exposure::quantise(s[i]);
  for (size_t i = 0; i < g.size(); ++i) {
    REQUIRE(mesh_exposure::gain_ok(g[i]));
    gs[i] = mesh_exposure::gain(value[i], g[i]);
  }
  for (size_t i = 0; i < seen4.size(); ++i) {
    f[i] = mesh_exposure::flags01(seen4[i]);
    sg[i] = mesh_exposure::signed4(q4[i], f[i]);
    for (int k = 0; k < 4; ++k) {                                  // byte by byte against the plain statement
      const uint32_t sb = (seen4[i] >> (8 * k)) & 255u, qb = (q4[i] >> (8 * k)) & 255u;
      REQUIRE(((f[i] >> (8 * k)) & 255u) == (sb != 0 ? 1u : 0u));
      REQUIRE((int)(int8_t)(sg[i] >> (8 * k)) == (sb != 0 ? (int)qb - 128 : 0));
    }
  }
  std::FILE* fo = std::fopen(out, "wb");
  REQUIRE(fo);
  write_all(fo, qs);
  write_all(fo, gs);
  write_all(fo, f);
  write_all(fo, sg);
  std::fclose(fo);
  return 0;
}

static int run_plan() {
  int cases = 0;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // sizes
  REQUIRE(mesh_exposure_check(0, 1, 0) == 0 && mesh_exposure_check(1024, 3, 0x7FFFFFFFLL) == 0);
  REQUIRE(mesh_exposure_check(-1, 3, 5) == 1 && mesh_exposure_check(1025, 3, 5) == 1);
  REQUIRE(mesh_exposure_check(2, 0, 5) == 2 && mesh_exposure_check(2, 2, 5) == 2 && mesh_exposure_check(2, 4, 5) == 2);
  REQUIRE(mesh_exposure_check(2, 3, -1) == 3 && mesh_exposure_check(2, 3, 0x80000000LL) == 3);
  cases += 9;
  // the workspace holds the view table
  for (int64_t n : {0, 1, 36, 1024}) {
    REQUIRE(mesh_exposure_workspace_bytes(n) >= (n + 1) * (int64_t)sizeof(TsdfView) && mesh_exposure_workspace_bytes(n) % 256 == 0);
    ++cases;
  }
  // buffers
  int x = 0;
  const void* p = &x;
  const int64_t need = mesh_exposure_workspace_bytes(3);
  REQUIRE(mesh_exposure_check_sample_buffers(3, 10, 5, p, p, p, p, p, p, p, p, p, need) == 0);
  REQUIRE(mesh_exposure_check_sample_buffers(3, 10, 5, p, p, p, p, p, p, p, p, nullptr, need) == 4);
  REQUIRE(mesh_exposure_check_sample_buffers(3, 10, 5, p, p, p, p, p, p, p, p, p, need - 1) == 4);
  REQUIRE(mesh_exposure_check_sample_buffers(3, 10, 5, nullptr, p, p, p, p, p, p, p, p, need) == 5);
  REQUIRE(mesh_exposure_check_sample_buffers(3, 10, 5, p, nullptr, p, p, p, p, p, p, p, need) == 5);
  REQUIRE(mesh_exposure_check_sample_buffers(3, 10, 5, p, p, nullptr, p, p, p, p, p, p, need) == 5);
  REQUIRE(mesh_exposure_check_sample_buffers(3, 10, 5, p, p, p, nullptr, p, p, p, p, p, need) == 5);
  REQUIRE(mesh_exposure_check_sample_buffers(3, 10, 5, p, p, p, p, nullptr, p, p, p, p, need) == 5);
  REQUIRE(mesh_exposure_check_sample_buffers(3, 10, 5, p, p, p, p, p, nullptr, p, p, p, need) == 5);
  REQUIRE(mesh_exposure_check_sample_buffers(3, 10, 5, p, p, p, p, p, p, nullptr, p, p, need) == 5);
  REQUIRE(mesh_exposure_check_sample_buffers(3, 10, 5, p, p, p, p, p, p, p, nullptr, p, need) == 5);
  REQUIRE(mesh_exposure_check_sample_buffers(3, 0, 0, p, p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, p, need) == 0);
  REQUIRE(mesh_exposure_check_sample_buffers(0, 0, 5, nullptr, nullptr, nullptr, nullptr, p, p, nullptr, nullptr, p, need) == 0);
  REQUIRE(mesh_exposure_check_gram_buffers(3, 5, p, p, p, p, p, need) == 0 && mesh_exposure_check_gram_buffers(3, 5, p, p, p, p, nullptr, need) == 4);
  REQUIRE(mesh_exposure_check_gram_buffers(3, 5, p, p, p, p, p, 8) == 4 && mesh_exposure_check_gram_buffers(3, 5, nullptr, p, p, p, p, need) == 5);
  REQUIRE(mesh_exposure_check_gram_buffers(3, 5, p, nullptr, p, p, p, need) == 5 && mesh_exposure_check_gram_buffers(3, 5, p, p, nullptr, p, p, need) == 5);
  REQUIRE(mesh_exposure_check_gram_buffers(3, 5, p, p, p, nullptr, p, need) == 5 && mesh_exposure_check_gram_buffers(3, 0, nullptr, nullptr, p, p, p, need) == 0);
  REQUIRE(mesh_exposure_check_gram_buffers(0, 5, nullptr, nullptr, nullptr, nullptr, p, need) == 0);
  cases += 22;
  // tiles, chunks and what the plan call reports
  REQUIRE(mesh_exposure_tiles(0) == 0 && mesh_exposure_tiles(1) == 1 && mesh_exposure_tiles(32) == 1 && mesh_exposure_tiles(33) == 2 && mesh_exposure_tiles(1024) == 32);
  REQUIRE(mesh_exposure_chunks(0) == 0 && mesh_exposure_chunks(1) == 1 && mesh_exposure_chunks(MESH_EXPOSURE_CHUNK) == 1 &&
          mesh_exposure_chunks(MESH_EXPOSURE_CHUNK + 1) == 2 && mesh_exposure_chunks(0x7FFFFFFFLL) == 0x7FFFFFFFLL / MESH_EXPOSURE_CHUNK + 1);
  int32_t out[4];
  mesh_exposure_plan(36, 106866, out);
  REQUIRE(out[0] == 32 && out[1] == 32 && out[2] == MESH_EXPOSURE_CHUNK && out[3] == 4 * (int32_t)mesh_exposure_chunks(106866));
  mesh_exposure_plan(1024, 0x7FFFFFFFLL, out);
  REQUIRE(out[3] > 0);
  cases += 4;
  // the images of the gain pass
  {
    const int32_t hs[3] = {3, 0, 5}, ws[3] = {4, 7, 1}, bad_h[3] = {3, -1, 5}, big_w[3] = {4, 32769, 1};
    const double g[9] = {0.0, 1.0, 0.5, 1.5, 2.0, 0.25, 1e300, 3.0, 1.0};
    int64_t off[4] = {-1, -1, -1, -1};
    REQUIRE(mesh_exposure_check_images(3, hs, ws, 3, g, off) == 0 && off[0] == 0 && off[1] == 12 && off[2] == 12 && off[3] == 17);
    REQUIRE(mesh_exposure_check_images(3, hs, ws, 1, g, nullptr) == 0 && mesh_exposure_check_images(0, nullptr, nullptr, 1, nullptr, off) == 0 && off[0] == 0);
    REQUIRE(mesh_exposure_check_images(-1, hs, ws, 3, g, nullptr) == 7 && mesh_exposure_check_images(3, hs, ws, 2, g, nullptr) == 2);
    REQUIRE(mesh_exposure_check_images(3, nullptr, ws, 3, g, nullptr) == 5 && mesh_exposure_check_images(3, hs, nullptr, 3, g, nullptr) == 5 &&
            mesh_exposure_check_images(3, hs, ws, 3, nullptr, nullptr) == 5);
    REQUIRE(mesh_exposure_check_images(3, bad_h, ws, 3, g, nullptr) == 6 && mesh_exposure_check_images(3, hs, big_w, 3, g, nullptr) == 6);
    for (double bad : {-1e-300, -1.0, nan, inf, -inf}) {
      double h[9];
      std::memcpy(h, g, sizeof(g));
      h[8] = bad;
      REQUIRE(mesh_exposure_check_images(3, hs, ws, 3, h, nullptr) == 8 && mesh_exposure_check_images(3, hs, ws, 1, h, nullptr) == 0);
      REQUIRE(!mesh_exposure::gain_ok(bad));
      ++cases;
    }
    REQUIRE(mesh_exposure::gain_ok(0.0) && mesh_exposure::gain_ok(1e300));
    cases += 10;
  }
  // the windows: they cut [b0, b1) into pieces in order, without a gap, each inside one 16-byte block of the address
  for (int mis = 0; mis < 16; ++mis)
    for (int64_t b0 = 0; b0 < 40; ++b0)
      for (int64_t b1 = b0; b1 < b0 + 70; ++b1) {
        const int64_t n = mesh_exposure_windows(b0, b1, mis);
        REQUIRE((b1 == b0) == (n == 0));
        int64_t at = b0;
        for (int64_t t = 0; t < n; ++t) {
          const MeshExposureWindow w = mesh_exposure_window(b0, b1, mis, t);
          REQUIRE(w.lo == at && w.hi > w.lo && w.hi <= b1 && w.hi - w.lo <= 16);
          REQUIRE((w.lo + mis) / 16 == (w.hi - 1 + mis) / 16);
          REQUIRE(w.hi - w.lo < 16 || (w.lo + mis) % 16 == 0);     // a whole window starts on the boundary
          REQUIRE(t == 0 || (w.lo + mis) % 16 == 0);
          at = w.hi;
        }
        REQUIRE(at == b1);
        const int64_t blocks = mesh_exposure_gain_blocks(n);
        REQUIRE(blocks * MESH_EXPOSURE_GAIN_BLOCK >= n && (blocks == 0 || (blocks - 1) * MESH_EXPOSURE_GAIN_BLOCK < n));
        ++cases;
      }
  // the gain rule at its corners
  REQUIRE(mesh_exposure::gain(255, 0.0) == 0 && mesh_exposure::gain(255, 1.0) == 255 && mesh_exposure::gain(200, 1.5) == 255 && mesh_exposure::gain(255, 1e300) == 255);
  // the largest double below 0.5 plus 0.5 rounds to 1: the rule is floor(x + 0.5) in doubles, as NumPy computes it
  REQUIRE(mesh_exposure::gain(1, 0.5) == 1 && mesh_exposure::gain(3, 0.5) == 2 && mesh_exposure::gain(0, 1e300) == 0 && mesh_exposure::gain(1, 0.49999999999999994) == 1);
  REQUIRE(mesh_exposure::quantise(0.0) == 0 && mesh_exposure::quantise(0.49999999999999994) == 1 && mesh_exposure::quantise(0.5) == 1 &&
          mesh_exposure::quantise(0.25) == 0 && mesh_exposure::quantise(254.5) == 255 && mesh_exposure::quantise(255.0) == 255);
  cases += 13;
  std::printf("ok %d\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::strcmp(argv[1], "scene") == 0) return run_scene(argv[2], argv[3]);
  if (argc == 4 && std::strcmp(argv[1], "rule") == 0) return run_rule(argv[2], argv[3]);
  if (argc == 2 && std::strcmp(argv[1], "plan") == 0) return run_plan();
  std::fprintf(stderr, "usage: mesh_exposure_check scene IN OUT | rule IN OUT | plan\n");
  return 2;
}
