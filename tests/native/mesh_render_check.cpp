// Host build of the mesh render rule and plan (sfm_amd/csrc/mesh_render_rule.h, mesh_render_plan.h) for
// tests/test_mesh_render_reference.py.
//   mesh_render_check scene IN OUT    IN: int64 n_cam, n_vertices, n_triangles, color_mode, channels, atlas_w, atlas_h, fill;
//                                     int32 heights[n_cam], widths[n_cam]; double proj[n_cam][12]; double
//                                     vertices[n_vertices][3]; int32 triangles[n_triangles][3]; then by color_mode uint8
//                                     vertex_colors[n_vertices][channels], or float uv[n_triangles][3][2] and uint8
//                                     atlas[atlas_h][atlas_w][channels]
//                                     OUT: float depth[n_pix], int32 triangle[n_pix], float bary[n_pix][3], uint8
//                                     color[n_pix][channels] (with a colour), int64 the boxes of more than 64 pixels.
//                                     The kernels of mesh_render.hip one after the other inside a workspace laid out by the
//                                     plan: project, raster with the small boxes walked and the large ones listed, the list
//                                     walked, resolve; every index is checked before it is read or written through.
//   mesh_render_check records IN OUT  IN: int64 n; per record double ua, va, qa, ub, vb, qb, uc, vc, qc, x, y and int64 tri
//                                     OUT: per record double w0, w1, w2, A, uint64 key, double b0, b1, b2
//   mesh_render_check plan            every branch of the argument checks, the layout and the grids; prints "ok <cases>"
// Build with -ffp-contract=off (the headers' pragma is clang's).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mesh_render_plan.h"
#include "mesh_render_rule.h"

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

using mesh_render::Vertex;

struct HostMesh {
  int64_t nv, nt;
  const int32_t* triangles;
  const double* projected;                               // of one camera
};

static bool load_triangle(const HostMesh& m, int64_t t, int w, int h, Vertex& a, Vertex& b, Vertex& c, mesh_render::Box& bx) {
  REQUIRE(t >= 0 && t < m.nt);
  const int64_t idx[3] = {m.triangles[3 * t], m.triangles[3 * t + 1], m.triangles[3 * t + 2]};
  for (int k = 0; k < 3; ++k) if (idx[k] < 0 || idx[k] >= m.nv) return false;
  Vertex p[3];
  for (int k = 0; k < 3; ++k) { p[k].u = m.projected[3 * idx[k]]; p[k].v = m.projected[3 * idx[k] + 1]; p[k].q2 = m.projected[3 * idx[k] + 2]; }
  a = p[0]; b = p[1]; c = p[2];
  if (!mesh_render::usable(a, b, c)) return false;
  bx = mesh_render::box(a, b, c, w, h);
  if (!bx.empty) REQUIRE(bx.x0 >= 0 && bx.x0 <= bx.x1 && bx.x1 < w && bx.y0 >= 0 && bx.y0 <= bx.y1 && bx.y1 < h);
  return !bx.empty;
}

static void draw(const Vertex& a, const Vertex& b, const Vertex& c, int x, int y, int64_t t, uint64_t* keys, const TsdfView& view, int64_t n_pix) {
  const uint64_t k = mesh_render::claim(a, b, c, x, y, t);
  if (k == MESH_RENDER_NO_KEY) return;
  const int64_t at = view.out_off + (int64_t)y * view.w + x;
  REQUIRE(x >= 0 && x < view.w && y >= 0 && y < view.h && at >= 0 && at < n_pix);
  if (k < keys[at]) keys[at] = k;
}

static int run_scene(const char* in, const char* out) {
  std::FILE* fi = std::fopen(in, "rb");
  REQUIRE(fi);
  const std::vector<int64_t> head = read_n<int64_t>(fi, 8);
  const int64_t n_cam = head[0], nv = head[1], nt = head[2], mode = head[3], ch = head[4], aw = head[5], ah = head[6], fill = head[7];
  REQUIRE(n_cam >= 0 && n_cam <= MESH_RENDER_MAX_CAMERAS);
  const std::vector<int32_t> heights = read_n<int32_t>(fi, n_cam), widths = read_n<int32_t>(fi, n_cam);
  std::vector<TsdfView> cams((size_t)n_cam + 1);
  int64_t n_pix = 0, max_pix = 0;
  REQUIRE(mesh_render_check_cameras(n_cam, heights.data(), widths.data(), cams.data(), &n_pix, &max_pix) == 0);
  REQUIRE(mesh_render_check_mesh(nv, nt) == 0 && mesh_render_check_color(mode, ch, fill, nt, aw, ah) == 0);
  const std::vector<double> proj = read_n<double>(fi, n_cam * 12), vertices = read_n<double>(fi, nv * 3);
  const std::vector<int32_t> triangles = read_n<int32_t>(fi, nt * 3);
  std::vector<uint8_t> vcol, atlas;
  std::vector<float> uv;
  if (mode == MESH_RENDER_VERTEX) vcol = read_n<uint8_t>(fi, nv * ch);
  if (mode == MESH_RENDER_ATLAS) { uv = read_n<float>(fi, nt * 6); atlas = read_n<uint8_t>(fi, ah * aw * ch); }
  std::fclose(fi);
  // the workspace as the plan lays it out: every array inside it, none overlapping the next
  const MeshRenderLayout L = mesh_render_layout(n_cam, n_pix, nv, nt);
  REQUIRE(L.count == 0 && L.cameras >= 8 && L.keys >= L.cameras + (n_cam + 1) * (int64_t)sizeof(TsdfView) && L.projected >= L.keys + n_pix * 8);
  REQUIRE(L.list >= L.projected + n_cam * nv * 24 && L.bytes >= L.list + L.list_capacity * 8 && L.list_capacity == n_cam * nt);
  REQUIRE(L.cameras % 256 == 0 && L.keys % 256 == 0 && L.projected % 256 == 0 && L.list % 256 == 0);
  std::vector<uint64_t> keys((size_t)n_pix, MESH_RENDER_NO_KEY), list((size_t)L.list_capacity);
  std::vector<double> projected((size_t)(n_cam * nv * 3));
  int64_t n_list = 0;
  REQUIRE(mesh_render_blocks(nv) * MESH_BLOCK >= nv && mesh_render_blocks(nt) * MESH_BLOCK >= nt && mesh_render_blocks(max_pix) * MESH_BLOCK >= max_pix);
  for (int64_t cam = 0; cam < n_cam; ++cam)                                       // k_render_project
    for (int64_t i = 0; i < nv; ++i) {
      const Vertex p = mesh_render::project(&proj[(size_t)cam * 12], vertices[(size_t)(3 * i)], vertices[(size_t)(3 * i + 1)], vertices[(size_t)(3 * i + 2)]);
      double* o = &projected[(size_t)((cam * nv + i) * 3)];
      o[0] = p.u; o[1] = p.v; o[2] = p.q2;
    }
  for (int64_t cam = 0; cam < n_cam; ++cam) {                                     // k_render_raster
    const TsdfView view = cams[(size_t)cam];
    const HostMesh m{nv, nt, triangles.data(), projected.data() + cam * nv * 3};
    for (int64_t t = 0; t < nt; ++t) {
      Vertex a, b, c;
      mesh_render::Box bx;
      if (!load_triangle(m, t, view.w, view.h, a, b, c, bx)) continue;
      if (mesh_render::box_pixels(bx) > MESH_RENDER_SMALL_BOX) {
        REQUIRE(n_list < L.list_capacity);
        list[(size_t)n_list++] = ((uint64_t)cam << 32) | (uint64_t)t;
        continue;
      }
      for (int y = bx.y0; y <= bx.y1; ++y)
        for (int x = bx.x0; x <= bx.x1; ++x) draw(a, b, c, x, y, t, keys.data(), view, n_pix);
    }
  }
  for (int64_t e = n_list - 1; e >= 0; --e) {                                     // k_render_raster_large, in another order
    const int64_t cam = (int64_t)(list[(size_t)e] >> 32), t = (int64_t)(list[(size_t)e] & 0xFFFFFFFFull);
    REQUIRE(cam < n_cam && t < nt);
    const TsdfView view = cams[(size_t)cam];
    const HostMesh m{nv, nt, triangles.data(), projected.data() + cam * nv * 3};
    Vertex a, b, c;
    mesh_render::Box bx;
    REQUIRE(load_triangle(m, t, view.w, view.h, a, b, c, bx));
    const int bw = bx.x1 - bx.x0 + 1;
    const int64_t n = mesh_render::box_pixels(bx);
    for (int64_t p = 0; p < n; ++p) draw(a, b, c, bx.x0 + (int)(p % bw), bx.y0 + (int)(p / bw), t, keys.data(), view, n_pix);
  }
  std::vector<float> depth((size_t)n_pix), bary((size_t)(n_pix * 3));
  std::vector<int32_t> triangle((size_t)n_pix);
  std::vector<uint8_t> color((size_t)(mode == MESH_RENDER_NONE ? 0 : n_pix * ch));
  for (int64_t cam = 0; cam < n_cam; ++cam) {                                     // k_render_resolve
    const TsdfView view = cams[(size_t)cam];
    const double* cp = projected.data() + cam * nv * 3;
    for (int64_t p = 0; p < (int64_t)view.h * view.w; ++p) {
      const int64_t at = view.out_off + p;
      REQUIRE(at < cams[(size_t)cam + 1].out_off);
      const uint64_t k = keys[(size_t)at];
      if (k == MESH_RENDER_NO_KEY) {
        const uint32_t nan_bits = MESH_RENDER_NAN_BITS;
        std::memcpy(&depth[(size_t)at], &nan_bits, 4);
        triangle[(size_t)at] = -1;
        for (int j = 0; j < 3; ++j) bary[(size_t)(3 * at + j)] = 0.0f;
        if (mode != MESH_RENDER_NONE) for (int j = 0; j < ch; ++j) color[(size_t)(at * ch + j)] = (uint8_t)fill;
        continue;
      }
      const int64_t t = mesh_render::key_triangle(k);
      REQUIRE(t >= 0 && t < nt);
      int64_t idx[3];
      Vertex q[3];
      for (int j = 0; j < 3; ++j) {
        idx[j] = triangles[(size_t)(3 * t + j)];
        REQUIRE(idx[j] >= 0 && idx[j] < nv);
        q[j].u = cp[3 * idx[j]]; q[j].v = cp[3 * idx[j] + 1]; q[j].q2 = cp[3 * idx[j] + 2];
      }
      double bk[3];
      mesh_render::bary(q[0], q[1], q[2], (int)(p % view.w), (int)(p / view.w), bk);
      const uint32_t db = mesh_render::key_depth_bits(k);
      std::memcpy(&depth[(size_t)at], &db, 4);
      triangle[(size_t)at] = (int32_t)t;
      for (int j = 0; j < 3; ++j) bary[(size_t)(3 * at + j)] = (float)bk[j];
      if (mode == MESH_RENDER_VERTEX)
        for (int j = 0; j < ch; ++j)
          color[(size_t)(at * ch + j)] = mesh_render::shade(bk, (double)vcol[(size_t)(idx[0] * ch + j)], (double)vcol[(size_t)(idx[1] * ch + j)],
                                                            (double)vcol[(size_t)(idx[2] * ch + j)]);
      if (mode == MESH_RENDER_ATLAS) {
        const float* u = &uv[(size_t)(6 * t)];
        const double px = mesh_render::atlas_pos(bk, u[0], u[2], u[4], (int)aw), py = mesh_render::atlas_pos(bk, u[1], u[3], u[5], (int)ah);
        const mesh_color::Taps tp = mesh_render::taps(px, py, (int)aw, (int)ah);
        REQUIRE(tp.x0 >= 0 && tp.x0 < aw && tp.x1 >= 0 && tp.x1 < aw && tp.y0 >= 0 && tp.y0 < ah && tp.y1 >= 0 && tp.y1 < ah);
        for (int j = 0; j < ch; ++j)
          color[(size_t)(at * ch + j)] = mesh_render::sample((double)atlas[(size_t)(((int64_t)tp.y0 * aw + tp.x0) * ch + j)],
                                                             (double)atlas[(size_t)(((int64_t)tp.y0 * aw + tp.x1) * ch + j)],
                                                             (double)atlas[(size_t)(((int64_t)tp.y1 * aw + tp.x0) * ch + j)],
                                                             (double)atlas[(size_t)(((int64_t)tp.y1 * aw + tp.x1) * ch + j)], tp);
      }
    }
  }
  std::FILE* fo = std::fopen(out, "wb");
  REQUIRE(fo);
  write_all(fo, depth);
  write_all(fo, triangle);
  write_all(fo, bary);
  write_all(fo, color);
  write_all(fo, std::vector<int64_t>{n_list});
  std::fclose(fo);
  return 0;
}

static int run_records(const char* in, const char* out) {
  std::FILE* fi = std::fopen(in, "rb");
  REQUIRE(fi);
  const int64_t n = read_n<int64_t>(fi, 1)[0];
  REQUIRE(n >= 0 && n < (1 << 24));
  std::FILE* fo = std::fopen(out, "wb");
  REQUIRE(fo);
  for (int64_t r = 0; r < n; ++r) {
    const std::vector<double> d = read_n<double>(fi, 11);
    const int64_t tri = read_n<int64_t>(fi, 1)[0];
    const Vertex a{d[0], d[1], d[2]}, b{d[3], d[4], d[5]}, c{d[6], d[7], d[8]};
    const mesh_render::Edges e = mesh_render::edges(a, b, c, d[9], d[10]);
    const uint64_t key = mesh_render::claim(a, b, c, (int)d[9], (int)d[10], tri);
    double bk[3];
    mesh_render::bary(a, b, c, (int)d[9], (int)d[10], bk);
    write_all(fo, std::vector<double>{e.w0, e.w1, e.w2, e.A});
    write_all(fo, std::vector<uint64_t>{key});
    write_all(fo, std::vector<double>{bk[0], bk[1], bk[2]});
  }
  std::fclose(fi);
  std::fclose(fo);
  return 0;
}

static int check_plan() {
  int cases = 0;
  const int32_t hs[3] = {3, 0, 32768}, ws[3] = {5, 4, 32768};
  TsdfView cams[4];
  int64_t n_pix = -1, most = -1;
  REQUIRE(mesh_render_check_cameras(3, hs, ws, cams, &n_pix, &most) == 0 && n_pix == 15 + (int64_t)32768 * 32768 && most == (int64_t)32768 * 32768);
  REQUIRE(cams[0].out_off == 0 && cams[1].out_off == 15 && cams[2].out_off == 15 && cams[3].out_off == n_pix && cams[1].h == 0 && cams[1].w == 4);
  REQUIRE(mesh_render_check_cameras(0, nullptr, nullptr, cams, &n_pix, &most) == 0 && n_pix == 0 && most == 0 && cams[0].out_off == 0);
  REQUIRE(mesh_render_check_cameras(2, hs, ws, nullptr, nullptr, nullptr) == 0);
  REQUIRE(mesh_render_check_cameras(-1, hs, ws, nullptr, nullptr, nullptr) == 1 && mesh_render_check_cameras(65536, hs, ws, nullptr, nullptr, nullptr) == 1);
  REQUIRE(mesh_render_check_cameras(1, nullptr, ws, nullptr, nullptr, nullptr) == 10 && mesh_render_check_cameras(1, hs, nullptr, nullptr, nullptr, nullptr) == 10);
  {
    const int32_t bad_h[2] = {3, -1}, bad_w[2] = {32769, 2}, ok[2] = {3, 2};
    REQUIRE(mesh_render_check_cameras(2, bad_h, ok, nullptr, nullptr, nullptr) == 2 && mesh_render_check_cameras(2, ok, bad_w, nullptr, nullptr, nullptr) == 2);
  }
  cases += 9;
  REQUIRE(mesh_render_check_mesh(0, 0) == 0 && mesh_render_check_mesh(MESH_RENDER_MAX_ITEMS, MESH_RENDER_MAX_ITEMS) == 0);
  REQUIRE(mesh_render_check_mesh(-1, 0) == 3 && mesh_render_check_mesh(MESH_RENDER_MAX_ITEMS + 1, 0) == 3);
  REQUIRE(mesh_render_check_mesh(0, -1) == 4 && mesh_render_check_mesh(0, MESH_RENDER_MAX_ITEMS + 1) == 4);
  cases += 6;
  REQUIRE(mesh_render_check_color(0, 0, 0, 5, 0, 0) == 0 && mesh_render_check_color(1, 1, 255, 5, 0, 0) == 0 && mesh_render_check_color(2, 3, 7, 5, 1, 32768) == 0);
  REQUIRE(mesh_render_check_color(2, 3, 7, 0, 0, 0) == 0);                      // no triangle: no texel is read
  REQUIRE(mesh_render_check_color(3, 1, 0, 5, 4, 4) == 5 && mesh_render_check_color(-1, 1, 0, 5, 4, 4) == 5);
  REQUIRE(mesh_render_check_color(1, 2, 0, 5, 4, 4) == 6 && mesh_render_check_color(2, 0, 0, 5, 4, 4) == 6 && mesh_render_check_color(1, 4, 0, 5, 4, 4) == 6);
  REQUIRE(mesh_render_check_color(0, 1, -1, 5, 4, 4) == 7 && mesh_render_check_color(1, 1, 256, 5, 4, 4) == 7);
  REQUIRE(mesh_render_check_color(2, 1, 0, 5, 0, 4) == 8 && mesh_render_check_color(2, 1, 0, 5, 4, 0) == 8 && mesh_render_check_color(2, 1, 0, 5, 32769, 4) == 8 &&
          mesh_render_check_color(2, 1, 0, 5, 4, 32769) == 8);
  cases += 15;
  for (int k = 1; k <= 10; ++k) REQUIRE(std::strlen(MESH_RENDER_WHY[k]) > 0);
  // the layout: in order, aligned, and the largest call still counts in int64
  {
    const MeshRenderLayout L = mesh_render_layout(36, 36 * (int64_t)786432, 106866, 211428);
    REQUIRE(L.count == 0 && L.cameras == 256 && L.keys > L.cameras && L.projected == L.keys + 36 * (int64_t)786432 * 8 && L.list_capacity == 36 * (int64_t)211428);
    REQUIRE(L.bytes == L.list + mesh_align(L.list_capacity * 8) + 256);
    const MeshRenderLayout Z = mesh_render_layout(0, 0, 0, 0);
    REQUIRE(Z.bytes > 0 && Z.list_capacity == 0 && Z.keys == Z.projected);
    const MeshRenderLayout B = mesh_render_layout(MESH_RENDER_MAX_CAMERAS, MESH_RENDER_MAX_CAMERAS * ((int64_t)1 << 30), MESH_RENDER_MAX_ITEMS, MESH_RENDER_MAX_ITEMS);
    REQUIRE(B.bytes > B.list && B.list > B.projected && B.projected > B.keys && B.list_capacity > 0);
    cases += 3;
  }
  // the buffers: p stands for any pointer; each may be missing only where nothing is read or written through it
  {
    const char byte = 0;
    const void* p = &byte;
    const void* z = nullptr;
    REQUIRE(mesh_render_check_buffers(2, 9, 5, 4, 2, 100, p, p, p, z, p, p, p, p, p, p, p, 100) == 0);
    REQUIRE(mesh_render_check_buffers(2, 9, 5, 4, 1, 100, p, p, p, p, z, z, p, p, p, p, p, 100) == 0);
    REQUIRE(mesh_render_check_buffers(2, 9, 5, 4, 0, 100, p, p, p, z, z, z, p, p, p, z, p, 100) == 0);
    REQUIRE(mesh_render_check_buffers(2, 9, 5, 4, 0, 100, p, p, p, z, z, z, p, p, p, z, z, 100) == 9);
    REQUIRE(mesh_render_check_buffers(2, 9, 5, 4, 0, 100, p, p, p, z, z, z, p, p, p, z, p, 99) == 9);
    for (int missing = 0; missing < 10; ++missing) {
      const void* a[10];
      for (int k = 0; k < 10; ++k) a[k] = k == missing ? z : p;
      for (int mode = 0; mode < 3; ++mode) {
        const bool needed = missing < 3 || (missing == 3 && mode == 1) || ((missing == 4 || missing == 5) && mode == 2) || (missing >= 6 && missing <= 8) ||
                            (missing == 9 && mode != 0);
        REQUIRE(mesh_render_check_buffers(2, 9, 5, 4, mode, 100, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], p, 100) == (needed ? 10 : 0));
      }
    }
    REQUIRE(mesh_render_check_buffers(0, 0, 5, 4, 1, 100, z, p, p, p, z, z, z, z, z, z, p, 100) == 0);        // no camera: no pixel
    REQUIRE(mesh_render_check_buffers(2, 9, 0, 4, 1, 100, p, z, p, z, z, z, p, p, p, p, p, 100) == 0);        // no vertex
    REQUIRE(mesh_render_check_buffers(2, 9, 5, 0, 2, 100, p, p, z, z, z, z, p, p, p, p, p, 100) == 0);        // no triangle
    REQUIRE(mesh_render_check_buffers(2, 0, 5, 4, 2, 100, p, p, p, z, p, p, z, z, z, z, p, 100) == 0);        // no pixel
    cases += 39;
  }
  // the grids
  for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)MESH_RENDER_MAX_ITEMS, (int64_t)32768 * 32768}) {
    const int64_t b = mesh_render_blocks(n);
    REQUIRE(b * MESH_BLOCK >= n && (b == 0 || (b - 1) * MESH_BLOCK < n) && b <= 0x7FFFFFFFLL);
    const int64_t g = mesh_render_clear_groups(n);
    REQUIRE(g >= 1 && g <= MESH_RENDER_CLEAR_GROUPS && (g == MESH_RENDER_CLEAR_GROUPS || g * MESH_BLOCK >= n));
    ++cases;
  }
  REQUIRE(MESH_RENDER_LARGE_GROUPS >= 1 && MESH_RENDER_LARGE_GROUPS <= 65535);
  // the rule's corners: the box of a triangle far outside, on the border, and with coordinates no int holds
  {
    const Vertex a{-1e300, 1e300, 1.0}, b{2.5, 0.5, 1.0}, c{1e300, -1e300, 1.0};
    const mesh_render::Box bx = mesh_render::box(a, b, c, 5, 3);
    REQUIRE(!bx.empty && bx.x0 == 0 && bx.x1 == 4 && bx.y0 == 0 && bx.y1 == 2 && mesh_render::box_pixels(bx) == 15);
    REQUIRE(mesh_render::box(a, b, c, 0, 3).empty && mesh_render::box(a, b, c, 5, 0).empty);
    const Vertex d{5.0, 1.0, 1.0}, e{6.0, 1.0, 1.0}, f{5.5, 2.0, 1.0};
    REQUIRE(mesh_render::box(d, e, f, 5, 3).empty && !mesh_render::box(d, e, f, 6, 3).empty);
    REQUIRE(mesh_render::claim(a, b, c, 2, 1, 7) == MESH_RENDER_NO_KEY || mesh_render::key_triangle(mesh_render::claim(a, b, c, 2, 1, 7)) == 7);
    REQUIRE(mesh_render::tap(NAN, 4) == 0 && mesh_render::tap(-1e300, 4) == 0 && mesh_render::tap(1e300, 4) == 3 && mesh_render::tap(2.0, 4) == 2);
    REQUIRE(mesh_render::round_u8(NAN) == 255 && mesh_render::round_u8(-3.0) == 0 && mesh_render::round_u8(254.4) == 254 && mesh_render::round_u8(1e300) == 255);
    REQUIRE(mesh_render::key(1.0f, 5) == 0x3F80000000000005ull && mesh_render::key(1.0f, 0x7FFFFFFF) < mesh_render::key(1.5f, 0));
    REQUIRE(!mesh_render::drawn(0.0f) && !mesh_render::drawn(-1.0f) && !mesh_render::drawn(NAN) && !mesh_render::drawn(INFINITY) && mesh_render::drawn(1e-40f));
    cases += 8;
  }
  std::printf("ok %d\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "scene")) return run_scene(argv[2], argv[3]);
  if (argc == 4 && !std::strcmp(argv[1], "records")) return run_records(argv[2], argv[3]);
  if (argc == 2 && !std::strcmp(argv[1], "plan")) return check_plan();
  std::fprintf(stderr, "usage: mesh_render_check scene IN OUT | records IN OUT | plan\n");
  return 2;
}
