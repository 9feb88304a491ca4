// Host build of the mesh texture rule and plan (sfm_amd/csrc/mesh_texture_rule.h, mesh_texture_plan.h) for
// tests/test_mesh_texture_reference.py.
//   mesh_texture_check scene IN OUT   IN: int64 n_ref, channels, n_vertices, n_triangles, texels, cells_per_row, has_keep,
//                                     fill; double tol, min_cos; int32 heights[n_ref], widths[n_ref]; double
//                                     proj[n_ref][12], centres[n_ref][3]; float depth[n_out]; uint8 keep[n_out] (when
//                                     has_keep); uint8 pixels[n_out][channels]; double vertices[n_vertices][3]; float
//                                     normals[n_vertices][3]; int32 triangles[n_triangles][3]
//                                     OUT: uint8 texture[H][W][channels], uint8 views[H][W], float uv[n_triangles][3][2],
//                                     then per texel int64 tri (-1: none), int32 numerators[3], double X[3], double
//                                     normal[3] (zeros where the texel has no triangle or its triangle a bad index).
//                                     k_mesh_texture texel by texel, one view at a time; every index is checked before it
//                                     is read through.
//   mesh_texture_check plan           the size of the atlas, every branch of the argument checks, the grid, and the map and
//                                     its inverse over small layouts; prints "ok <cases>"
// Build with -ffp-contract=off (the headers' pragma is clang's).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mesh_texture_plan.h"
#include "mesh_texture_rule.h"

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

static int run_scene(const char* in, const char* out) {
  std::FILE* fi = std::fopen(in, "rb");
  REQUIRE(fi);
  const std::vector<int64_t> head = read_n<int64_t>(fi, 8);
  const std::vector<double> scalars = read_n<double>(fi, 2);
  const int64_t n_ref = head[0], ch = head[1], nv = head[2], nt = head[3], s = head[4], cpr = head[5], has_keep = head[6], fill = head[7];
  const double tol = scalars[0], min_cos = scalars[1];
  REQUIRE(n_ref >= 0 && n_ref <= TSDF_MAX_VIEWS);
  REQUIRE(mesh_color_check(ch, nv, tol, min_cos, fill) == 0);
  int32_t W = 0, H = 0;
  REQUIRE(mesh_texture_size(nt, s, cpr, &W, &H) == 0);
  const std::vector<int32_t> heights = read_n<int32_t>(fi, n_ref), widths = read_n<int32_t>(fi, n_ref);
  std::vector<int32_t> ref_image((size_t)n_ref);
  for (int64_t r = 0; r < n_ref; ++r) ref_image[(size_t)r] = (int32_t)r;
  std::vector<TsdfView> views((size_t)n_ref + 1);
  REQUIRE(tsdf_check_views(n_ref, heights.data(), widths.data(), n_ref, ref_image.data(), views.data()) == 0);
  int64_t n_out = 0;
  for (int64_t r = 0; r < n_ref; ++r) n_out += (int64_t)views[(size_t)r].h * views[(size_t)r].w;
  views[(size_t)n_ref] = TsdfView{n_out, 0, 0};
  REQUIRE((int64_t)(views.size() * sizeof(TsdfView)) <= mesh_texture_workspace_bytes(n_ref));
  const std::vector<double> proj = read_n<double>(fi, n_ref * 12), centres = read_n<double>(fi, n_ref * 3);
  const std::vector<float> depth = read_n<float>(fi, n_out);
  const std::vector<uint8_t> keep = read_n<uint8_t>(fi, has_keep ? n_out : 0), pixels = read_n<uint8_t>(fi, n_out * ch);
  const std::vector<double> vertices = read_n<double>(fi, nv * 3);
  const std::vector<float> normals = read_n<float>(fi, nv * 3);
  const std::vector<int32_t> triangles = read_n<int32_t>(fi, nt * 3);
  std::fclose(fi);
  const int64_t n_texels = (int64_t)H * W;
  std::vector<uint8_t> texture((size_t)(n_texels * ch)), n_views((size_t)n_texels);
  std::vector<float> uv((size_t)(nt * 6));
  std::vector<int64_t> tri((size_t)n_texels);
  std::vector<int32_t> nums((size_t)(n_texels * 3));
  std::vector<double> points((size_t)(n_texels * 3)), unit_normals((size_t)(n_texels * 3));
  // the launch covers the atlas
  REQUIRE(mesh_texture_tiles_x(W) * MESH_TEXTURE_TILE_X >= W && mesh_texture_tiles_y(H) * MESH_TEXTURE_TILE_Y >= H);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int64_t at = (int64_t)y * W + x;
      const mesh_texture::Texel tx = mesh_texture::texel_of(x, y, (int)s, (int)cpr, nt);
      REQUIRE(tx.tri >= -1 && tx.tri < nt);
      double acc[3] = {0.0, 0.0, 0.0};
      mesh_color::Tally tally = mesh_color::empty_tally();
      tri[(size_t)at] = tx.tri;
      bool owned = tx.tri >= 0;
      int64_t corner[3] = {0, 0, 0};
      if (owned) {
        int bx, by;
        mesh_texture::texel_at(tx.tri, tx.i, tx.j, (int)s, (int)cpr, &bx, &by);
        REQUIRE(bx == x && by == y && tx.i >= 0 && tx.j >= 0 && tx.i + tx.j <= s + 1);
        for (int k = 0; k < 3; ++k) {
          corner[k] = triangles[(size_t)(3 * tx.tri + k)];
          owned = owned && corner[k] >= 0 && corner[k] < nv;
        }
      }
      if (owned) {
        const mesh_texture::Numerators n = mesh_texture::numerators(tx.i, tx.j, (int)s);
        REQUIRE(n.n0 >= 0 && n.n1 >= 0 && n.n2 >= 0 && n.n0 + n.n1 + n.n2 == 2 * s);
        double m[3][3], X[3], normal[3];
        for (int k = 0; k < 3; ++k)
          for (int a = 0; a < 3; ++a) m[k][a] = (double)normals[(size_t)(3 * corner[k] + a)];
        mesh_texture::point_and_normal(n, &vertices[(size_t)(3 * corner[0])], &vertices[(size_t)(3 * corner[1])], &vertices[(size_t)(3 * corner[2])],
                                       m[0], m[1], m[2], (int)s, X, normal);
        nums[(size_t)(3 * at)] = n.n0; nums[(size_t)(3 * at + 1)] = n.n1; nums[(size_t)(3 * at + 2)] = n.n2;
        for (int a = 0; a < 3; ++a) { points[(size_t)(3 * at + a)] = X[a]; unit_normals[(size_t)(3 * at + a)] = normal[a]; }
        for (int v = 0; v < n_ref; ++v) {
          const TsdfView view = views[(size_t)v];
          const mesh_color::Projection p = mesh_color::project(&proj[(size_t)v * 12], X[0], X[1], X[2], view.w, view.h);
          if (!p.valid) continue;
          const int64_t e = view.out_off + (int64_t)p.yi * view.w + p.xi;
          REQUIRE(e >= view.out_off && e < views[(size_t)v + 1].out_off);
          if (!mesh_color::sees((double)depth[(size_t)e], has_keep ? keep[(size_t)e] != 0 : 1, p.q2, tol)) continue;
          double wgt = 0.0;
          if (!mesh_color::weight(&centres[(size_t)v * 3], X, normal, min_cos, &wgt)) continue;
          const mesh_color::Taps t = mesh_color::taps(p.u, p.v, view.w, view.h);
          REQUIRE(t.x0 >= 0 && t.x0 <= t.x1 && t.x1 < view.w && t.y0 >= 0 && t.y0 <= t.y1 && t.y1 < view.h);
          const uint8_t* img = pixels.data() + view.out_off * ch;
          for (int k = 0; k < ch; ++k) {
            const double a = (double)img[((int64_t)t.y0 * view.w + t.x0) * ch + k], b = (double)img[((int64_t)t.y0 * view.w + t.x1) * ch + k];
            const double c = (double)img[((int64_t)t.y1 * view.w + t.x0) * ch + k], d = (double)img[((int64_t)t.y1 * view.w + t.x1) * ch + k];
            acc[k] = mesh_color::add_sample(acc[k], wgt, mesh_color::bilinear(a, b, c, d, t.fx, t.fy));
          }
          mesh_color::add_view(&tally, wgt, v);
        }
      }
      for (int k = 0; k < ch; ++k) texture[(size_t)(at * ch + k)] = mesh_color::finish(acc[k], tally, (int)fill);
      n_views[(size_t)at] = mesh_color::finish_views(tally);
    }
  for (int64_t t = 0; t < nt; ++t)
    for (int k = 0; k < 3; ++k) mesh_texture::corner_uv(t, k, (int)s, (int)cpr, W, H, &uv[(size_t)(6 * t + 2 * k)]);
  std::FILE* fo = std::fopen(out, "wb");
  REQUIRE(fo);
  write_all(fo, texture);
  write_all(fo, n_views);
  write_all(fo, uv);
  write_all(fo, tri);
  write_all(fo, nums);
  write_all(fo, points);
  write_all(fo, unit_normals);
  std::fclose(fo);
  return 0;
}

static int check_plan() {
  int cases = 0;
  int32_t W = -1, H = -1;
  // the size of the atlas
  REQUIRE(mesh_texture_size(0, 8, 1, &W, &H) == 0 && W == 11 && H == 0);
  REQUIRE(mesh_texture_size(1, 1, 1, &W, &H) == 0 && W == 4 && H == 4);
  REQUIRE(mesh_texture_size(5, 3, 2, &W, &H) == 0 && W == 12 && H == 12);
  REQUIRE(mesh_texture_size(4, 3, 2, &W, &H) == 0 && W == 12 && H == 6);
  REQUIRE(mesh_texture_size(211428, 8, 326, &W, &H) == 0 && W == 3586 && H == 3575);
  REQUIRE(mesh_texture_size(2, 64, 489, &W, &H) == 0 && W == 32763 && H == 67);
  REQUIRE(mesh_texture_size(2 * 489 * 489, 64, 489, &W, &H) == 0 && W == 32763 && H == 32763);
  REQUIRE(mesh_texture_size(5, 3, 2, nullptr, nullptr) == 0);
  cases += 8;
  for (int64_t s : {(int64_t)0, (int64_t)-1, (int64_t)65, (int64_t)1 << 40}) { REQUIRE(mesh_texture_size(4, s, 2, &W, &H) == 1); ++cases; }
  for (int64_t c : {(int64_t)0, (int64_t)-3}) { REQUIRE(mesh_texture_size(4, 3, c, &W, &H) == 2); ++cases; }
  REQUIRE(mesh_texture_size(4, 64, 490, &W, &H) == 3);                         // too wide
  REQUIRE(mesh_texture_size(4, 1, 0x7FFFFFFF, &W, &H) == 3);
  REQUIRE(mesh_texture_size(2 * 489 * 489 + 1, 64, 489, &W, &H) == 3);         // too high
  REQUIRE(mesh_texture_size(MESH_TEXTURE_MAX_TRIANGLES, 1, 1, &W, &H) == 3);
  REQUIRE(mesh_texture_size(-1, 3, 2, &W, &H) == 4 && mesh_texture_size(MESH_TEXTURE_MAX_TRIANGLES + 1, 3, 2, &W, &H) == 4);
  cases += 6;
  for (int k = 1; k <= 6; ++k) REQUIRE(std::strlen(MESH_TEXTURE_WHY[k]) > 0);
  // the buffers: p stands for any pointer; each may be missing only where nothing is read or written through it
  {
    const char byte = 0;
    const void* p = &byte;
    const void* z = nullptr;
    const int64_t need = mesh_texture_workspace_bytes(2);
    REQUIRE(need == mesh_color_workspace_bytes(2) && need >= 3 * (int64_t)sizeof(TsdfView));
    REQUIRE(mesh_texture_check_buffers(2, 9, 5, 4, p, p, p, p, p, p, p, p, p, p, p, need) == 0);
    REQUIRE(mesh_texture_check_buffers(2, 9, 5, 4, p, p, p, p, p, p, p, p, p, p, z, need) == 5);
    REQUIRE(mesh_texture_check_buffers(2, 9, 5, 4, p, p, p, p, p, p, p, p, p, p, p, need - 1) == 5);
    for (int missing = 0; missing < 10; ++missing) {
      const void* a[10];
      for (int k = 0; k < 10; ++k) a[k] = k == missing ? z : p;
      REQUIRE(mesh_texture_check_buffers(2, 9, 5, 4, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], p, need) == 6);
    }
    REQUIRE(mesh_texture_check_buffers(2, 0, 5, 4, p, p, z, z, p, p, p, p, p, p, p, need) == 0);                                   // no pixel
    REQUIRE(mesh_texture_check_buffers(2, 9, 0, 4, p, p, p, p, z, z, p, p, p, p, p, need) == 0);                                   // no vertex
    REQUIRE(mesh_texture_check_buffers(2, 9, 5, 0, p, p, p, p, p, p, z, z, z, z, p, need) == 0);                                   // no triangle
    REQUIRE(mesh_texture_check_buffers(0, 0, 5, 4, z, z, z, z, p, p, p, p, p, p, p, mesh_texture_workspace_bytes(0)) == 0);        // no view
    cases += 17;
  }
  // the grid: every texel has a thread, the last tile of a row and of a column is not empty, the largest atlas fits a launch
  for (int64_t side : {(int64_t)1, (int64_t)3, (int64_t)4, (int64_t)5, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)3586, (int64_t)MESH_TEXTURE_MAX_SIDE}) {
    const int64_t tx = mesh_texture_tiles_x(side), ty = mesh_texture_tiles_y(side);
    REQUIRE(tx * MESH_TEXTURE_TILE_X >= side && (tx - 1) * MESH_TEXTURE_TILE_X < side && tx <= 0x7FFFFFFFLL);
    REQUIRE(ty * MESH_TEXTURE_TILE_Y >= side && (ty - 1) * MESH_TEXTURE_TILE_Y < side && ty <= 65535);
    ++cases;
  }
  REQUIRE(mesh_texture_tiles_y(0) == 0 && mesh_texture_uv_blocks(0) == 0 && mesh_texture_uv_blocks(257) == 2);
  REQUIRE(mesh_texture_uv_blocks(MESH_TEXTURE_MAX_TRIANGLES) <= 0x7FFFFFFFLL && MESH_TEXTURE_BATCH >= 1);
  // the map and its inverse over small layouts: every (t, i, j) has a texel of its own inside the atlas, the inverse map
  // returns it, and the texels that are left belong to nothing
  for (int s : {1, 2, 3, 5, 8, 64})
    for (int64_t nt : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)7, (int64_t)10})
      for (int cpr : {1, 2, 3, 7}) {
        REQUIRE(mesh_texture_size(nt, s, cpr, &W, &H) == 0);
        std::vector<int64_t> owner((size_t)W * (size_t)H, -1);
        for (int64_t t = 0; t < nt; ++t)
          for (int i = 0; i <= s + 1; ++i)
            for (int j = 0; i + j <= s + 1; ++j) {
              int x, y;
              mesh_texture::texel_at(t, i, j, s, cpr, &x, &y);
              REQUIRE(x >= 0 && x < W && y >= 0 && y < H);
              REQUIRE(owner[(size_t)y * W + x] == -1);
              owner[(size_t)y * W + x] = t;
              const mesh_texture::Texel back = mesh_texture::texel_of(x, y, s, cpr, nt);
              REQUIRE(back.tri == t && back.i == i && back.j == j);
              const mesh_texture::Numerators n = mesh_texture::numerators(i, j, s);
              REQUIRE(n.n0 >= 0 && n.n1 >= 0 && n.n2 >= 0 && n.n0 + n.n1 + n.n2 == 2 * s && (i + j <= s || n.n0 == 0));
            }
        int64_t owned = 0;
        for (int y = 0; y < H; ++y)
          for (int x = 0; x < W; ++x) {
            const mesh_texture::Texel tx = mesh_texture::texel_of(x, y, s, cpr, nt);
            REQUIRE(tx.tri == owner[(size_t)y * W + x]);
            owned += tx.tri >= 0;
          }
        REQUIRE(owned == nt * (int64_t)((s + 2) * (s + 3) / 2));
        // the corners sit on texel centres inside the atlas
        for (int64_t t = 0; t < nt; ++t)
          for (int k = 0; k < 3; ++k) {
            float q[2];
            mesh_texture::corner_uv(t, k, s, cpr, W, H, q);
            REQUIRE(q[0] > 0.0f && q[0] < 1.0f && q[1] > 0.0f && q[1] < 1.0f);
          }
        ++cases;
      }
  std::printf("ok %d\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "scene")) return run_scene(argv[2], argv[3]);
  if (argc == 2 && !std::strcmp(argv[1], "plan")) return check_plan();
  std::fprintf(stderr, "usage: mesh_texture_check scene IN OUT | plan\n");
  return 2;
}
