// Host build of the dense-depth rule and plan (sfm_amd/csrc/depth_rule.h, depth_plan.h) for tests/test_depth_reference.py.
//   depth_check sample IN OUT   IN: int64 n, then n records of { double W[12]; double x, y, d; int32 ws, hs }
//                               OUT: n records of { int32 valid, xi, yi, pad; double q2 }
//   depth_check refine IN OUT   IN: int64 n, then n records of { int32 best, n_planes, sm, s0, sp, pad; double dm, d0, dp }
//                               OUT: n float32
//   depth_check cost IN OUT     IN: int64 n, then n pairs of uint64; OUT: n int32
//   depth_check plan SEED       the thread map of tile plus halo for every radius and image sizes around the tile constants
//                               (every slot written exactly once, every pixel inside the image, every window slot inside tile
//                               plus halo), the tables, the searches, the layout and the checks; prints "ok <cases>"
// Build with -ffp-contract=off (the header's pragma is clang's).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "depth_plan.h"
#include "depth_rule.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct SampleIn { double W[12]; double x, y, d; int32_t ws, hs; };
struct SampleOut { int32_t valid, xi, yi, pad; double q2; };
struct RefineIn { int32_t best, n_planes, sm, s0, sp, pad; double dm, d0, dp; };

template <typename In, typename Out, typename F>
static int run_records(const char* in, const char* out, F f) {
  std::FILE* fi = std::fopen(in, "rb");
  REQUIRE(fi);
  int64_t n = 0;
  REQUIRE(std::fread(&n, 8, 1, fi) == 1 && n >= 0);
  std::vector<In> rec((size_t)n);
  REQUIRE(n == 0 || std::fread(rec.data(), sizeof(In), (size_t)n, fi) == (size_t)n);
  std::fclose(fi);
  std::vector<Out> res((size_t)n);
  for (int64_t i = 0; i < n; ++i) res[(size_t)i] = f(rec[(size_t)i]);
  std::FILE* fo = std::fopen(out, "wb");
  REQUIRE(fo);
  REQUIRE(n == 0 || std::fwrite(res.data(), sizeof(Out), (size_t)n, fo) == (size_t)n);
  std::fclose(fo);
  return 0;
}

static uint64_t rng_state;
static uint64_t rnd() {
  rng_state += 0x9E3779B97F4A7C15ull;
  uint64_t z = rng_state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the sweep's thread map on one w x h image at radius r: what the kernel writes to and reads from its LDS plane
static void check_tiles(int w, int h, int r) {
  const int count = depth_halo_count(r), rounds = depth_halo_rounds(r);
  REQUIRE(rounds * DEPTH_THREADS >= count && (rounds - 1) * DEPTH_THREADS < count);
  std::vector<int> owner((size_t)w * h, 0);
  for (int64_t ty = 0; ty < depth_tiles_y(h); ++ty) {
    for (int64_t tx = 0; tx < depth_tiles_x(w); ++tx) {
      const int x0 = (int)tx * DEPTH_TW, y0 = (int)ty * DEPTH_TH;
      REQUIRE(x0 < w && y0 < h);                              // no workgroup without a pixel
      std::vector<int> written((size_t)count, 0);
      std::vector<int> lds((size_t)count, -1);                // the image pixel behind every slot
      for (int tid = 0; tid < DEPTH_THREADS; ++tid) {
        for (int j = 0; j < rounds; ++j) {
          const int slot = tid + j * DEPTH_THREADS;
          if (slot >= count) continue;
          int px, py;
          depth_halo_pixel(slot, r, x0, y0, w, h, &px, &py);
          REQUIRE(px >= 0 && px < w && py >= 0 && py < h);    // nothing reads outside the image
          written[(size_t)slot]++;
          lds[(size_t)slot] = py * w + px;
        }
      }
      for (int s = 0; s < count; ++s) REQUIRE(written[(size_t)s] == 1);
      for (int tid = 0; tid < DEPTH_THREADS; ++tid) {
        const int px = tid % DEPTH_TW;
        for (int q = 0; q < 2; ++q) {
          const int py = 2 * (tid / DEPTH_TW) + q;
          REQUIRE(py < DEPTH_TH);
          for (int dy = -r; dy <= r; ++dy) {
            for (int dx = -r; dx <= r; ++dx) {
              const int slot = depth_halo_slot(px, py, dx, dy, r);
              REQUIRE(slot >= 0 && slot < count);
              if (x0 + px < w && y0 + py < h)                 // the slot holds the clamped neighbour of an image pixel
                REQUIRE(lds[(size_t)slot] == depth_clamp(y0 + py + dy, h - 1) * w + depth_clamp(x0 + px + dx, w - 1));
            }
          }
          if (x0 + px < w && y0 + py < h) owner[(size_t)(y0 + py) * w + x0 + px]++;
        }
      }
    }
  }
  for (int v : owner) REQUIRE(v == 1);                        // every pixel of the image has exactly one owner
}

static void check_tables(const std::vector<int32_t>& hs, const std::vector<int32_t>& ws, const std::vector<int32_t>& refs,
                         const std::vector<std::vector<int32_t>>& srcs, int n_planes) {
  const int64_t n_img = (int64_t)hs.size(), n_ref = (int64_t)refs.size();
  std::vector<int64_t> off((size_t)n_img + 1, 0);
  for (int64_t i = 0; i < n_img; ++i) off[(size_t)i + 1] = off[(size_t)i] + (int64_t)hs[(size_t)i] * ws[(size_t)i] + (i % 2 ? 3 : 0);
  std::vector<int64_t> src_ptr(1, 0), plane_ptr(1, 0);
  std::vector<int32_t> src_image;
  for (auto& s : srcs) { for (int32_t v : s) src_image.push_back(v); src_ptr.push_back((int64_t)src_image.size()); plane_ptr.push_back(plane_ptr.back() + n_planes); }
  REQUIRE(depth_check_images(n_img, off.data(), hs.data(), ws.data()) == 0);
  REQUIRE(depth_check_views(n_img, n_ref, refs.data(), src_ptr.data(), src_image.data(), plane_ptr.data(), 2) == 0);
  const DepthPlan p = depth_plan(n_img, off.data(), hs.data(), ws.data(), n_ref, refs.data(), src_ptr.data(), plane_ptr.data());
  REQUIRE((int64_t)p.images.size() == n_img + 1 && (int64_t)p.views.size() == n_ref + 1);
  int64_t out = 0, tiles = 0, blocks = 0;
  for (int64_t r = 0; r < n_ref; ++r) {
    const DepthView& v = p.views[(size_t)r];
    const int64_t n = (int64_t)hs[(size_t)refs[(size_t)r]] * ws[(size_t)refs[(size_t)r]];
    REQUIRE(v.out_off == out && v.tile_first == tiles && v.pix_block_first == blocks && v.image == refs[(size_t)r]);
    REQUIRE(v.n_src == (int32_t)srcs[(size_t)r].size() && v.n_planes == n_planes && v.plane_first == r * n_planes);
    REQUIRE(p.ref_of_image[(size_t)v.image] == r);
    const int64_t nt = n > 0 ? (int64_t)v.tiles_x * v.tiles_y : 0;
    for (int64_t t = 0; t < nt; ++t) REQUIRE(depth_find_view(p.views.data(), (int)n_ref, tiles + t, DEPTH_BY_TILE) == r);
    for (int64_t b = 0; b < depth_pixel_blocks(n); ++b) REQUIRE(depth_find_view(p.views.data(), (int)n_ref, blocks + b, DEPTH_BY_PIXEL_BLOCK) == r);
    out += n; tiles += nt; blocks += depth_pixel_blocks(n);
  }
  REQUIRE(p.n_out == out && p.n_tiles == tiles && p.n_pix_blocks == blocks);
  for (int64_t i = 0; i < n_img; ++i) {                       // every element of a slot finds its image
    for (int64_t e = off[(size_t)i]; e < off[(size_t)i + 1]; e += (off[(size_t)i + 1] - off[(size_t)i] > 40 ? 13 : 1)) {
      const int k = depth_find_image(p.images.data(), (int)n_img, e);
      REQUIRE(p.images[(size_t)k].off <= e && e < p.images[(size_t)k + 1].off && p.images[(size_t)k].off == off[(size_t)i]);
    }
  }
  const DepthLayout L = depth_layout(n_img, n_ref, (int64_t)src_image.size());
  const int64_t at[] = {L.images, L.views, L.src_image, L.ref_of_image, L.max_cost, L.bytes};
  const int64_t len[] = {(n_img + 1) * (int64_t)sizeof(DepthImage), (n_ref + 1) * (int64_t)sizeof(DepthView), (int64_t)src_image.size() * 4, n_img * 4, n_ref * 4};
  for (int k = 0; k < 5; ++k) { REQUIRE(at[k] % 256 == 0); REQUIRE(at[k] + len[k] <= at[k + 1]); }
  std::vector<unsigned char> wsp((size_t)L.bytes);            // an image of the workspace can be written end to end
  std::memcpy(wsp.data() + L.images, p.images.data(), p.images.size() * sizeof(DepthImage));
  std::memcpy(wsp.data() + L.views, p.views.data(), p.views.size() * sizeof(DepthView));
  if (!src_image.empty()) std::memcpy(wsp.data() + L.src_image, src_image.data(), src_image.size() * 4);
  if (n_img) std::memcpy(wsp.data() + L.ref_of_image, p.ref_of_image.data(), (size_t)n_img * 4);
}

static int run_plan(uint64_t seed) {
  rng_state = seed;
  int cases = 0;
  const int sizes[] = {1, 2, 3, 7, 8, 9, DEPTH_TH - 1, DEPTH_TH, DEPTH_TH + 1, DEPTH_TW - 1, DEPTH_TW, DEPTH_TW + 1, 2 * DEPTH_TW + 1};
  for (int r = 0; r <= DEPTH_MAX_RADIUS; ++r) {
    for (int w : sizes) for (int h : sizes) { check_tiles(w, h, r); ++cases; }
    for (int rep = 0; rep < 6; ++rep) { check_tiles(1 + (int)(rnd() % 100), 1 + (int)(rnd() % 60), r); ++cases; }
  }
  check_tables({}, {}, {}, {}, 1); ++cases;
  check_tables({5, 7}, {4, 9}, {}, {}, 1); ++cases;
  check_tables({5, 0, 7}, {4, 3, 0}, {1, 0, 2}, {{0}, {}, {0, 1}}, 3); ++cases;                  // views without a pixel between live ones
  check_tables({16, 17, 33}, {32, 31, 65}, {2, 0}, {{0, 1}, {1, 2}}, 1024); ++cases;
  for (int rep = 0; rep < 100; ++rep) {
    const int n_img = 1 + (int)(rnd() % 6);
    std::vector<int32_t> hs, ws, refs;
    for (int i = 0; i < n_img; ++i) { hs.push_back((int32_t)(rnd() % 5 == 0 ? 0 : rnd() % 70)); ws.push_back((int32_t)(rnd() % 70)); }
    std::vector<std::vector<int32_t>> srcs;
    for (int i = n_img - 1; i >= 0; --i) {
      if (rnd() % 3 == 0) continue;
      refs.push_back(i);
      std::vector<int32_t> s;
      const int ns = n_img > 1 ? (int)(rnd() % (DEPTH_MAX_SOURCES + 1)) : 0;
      for (int k = 0; k < ns; ++k) { const int32_t v = (int32_t)(rnd() % n_img); if (v != i) s.push_back(v); }
      srcs.push_back(s);
    }
    check_tables(hs, ws, refs, srcs, 1 + (int)(rnd() % 40)); ++cases;
  }
  {  // what the checks refuse
    const int64_t off[] = {0, 12, 40}, bad_off[] = {0, 12, 11};
    const int32_t hs[] = {3, 4}, ws[] = {4, 7}, big[] = {4, 8};
    const int32_t refs[] = {0, 1}, twice[] = {1, 1}, out_of_range[] = {0, 2};
    const int64_t sp[] = {0, 1, 2}, pp[] = {0, 5, 6}, none[] = {0, 5, 5}, many[] = {0, 5, 1030}, sp9[] = {0, 9, 9};
    const int32_t si[] = {1, 0}, self[] = {0, 0}, far[] = {1, 5}, nine[] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
    REQUIRE(depth_check_images(2, off, hs, ws) == 0);
    REQUIRE(depth_check_images(2, bad_off, hs, ws) != 0);
    REQUIRE(depth_check_images(2, off, hs, big) != 0);
    REQUIRE(depth_check_images(2, nullptr, hs, ws) != 0);
    REQUIRE(depth_check_images(-1, off, hs, ws) != 0);
    REQUIRE(depth_check_views(2, 2, refs, sp, si, pp, 4) == 0);
    REQUIRE(depth_check_views(2, 2, refs, sp, si, pp, 5) != 0);
    REQUIRE(depth_check_views(2, 2, refs, sp, si, pp, -1) != 0);
    REQUIRE(depth_check_views(2, 2, twice, sp, si, pp, 2) != 0);
    REQUIRE(depth_check_views(2, 2, out_of_range, sp, si, pp, 2) != 0);
    REQUIRE(depth_check_views(2, 2, refs, sp, self, pp, 2) != 0);
    REQUIRE(depth_check_views(2, 2, refs, sp, far, pp, 2) != 0);
    REQUIRE(depth_check_views(2, 2, refs, sp9, nine, pp, 2) != 0);
    REQUIRE(depth_check_views(2, 2, refs, sp, si, none, 2) != 0);
    REQUIRE(depth_check_views(2, 2, refs, sp, si, many, 2) != 0);
    REQUIRE(depth_check_views(2, 3, refs, sp, si, pp, 2) != 0);
    REQUIRE(depth_check_views(2, 2, refs, nullptr, si, pp, 2) != 0);
    cases += 17;
  }
  std::printf("ok %d\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "sample"))
    return run_records<SampleIn, SampleOut>(argv[2], argv[3], [](const SampleIn& r) {
      const depth::Sample s = depth::sample(r.W, r.x, r.y, r.d, r.ws, r.hs);
      REQUIRE(!s.valid || (s.xi >= 0 && s.xi < r.ws && s.yi >= 0 && s.yi < r.hs));
      return SampleOut{s.valid, s.xi, s.yi, 0, s.q2};
    });
  if (argc == 4 && !std::strcmp(argv[1], "refine"))
    return run_records<RefineIn, float>(argv[2], argv[3], [](const RefineIn& r) {
      return depth::refine(r.best, r.n_planes, r.sm, r.s0, r.sp, r.dm, r.d0, r.dp);
    });
  if (argc == 4 && !std::strcmp(argv[1], "cost")) {
    struct Pair { uint64_t a, b; };
    return run_records<Pair, int32_t>(argv[2], argv[3], [](const Pair& r) { return (int32_t)depth::cost(r.a, r.b); });
  }
  if (argc == 3 && !std::strcmp(argv[1], "plan")) return run_plan(std::strtoull(argv[2], nullptr, 10));
  std::fprintf(stderr, "usage: depth_check sample|refine|cost IN OUT | depth_check plan SEED\n");
  return 2;
}
