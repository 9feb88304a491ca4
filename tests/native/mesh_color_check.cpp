// Host build of the mesh colouring rule and plan (sfm_amd/csrc/mesh_color_rule.h, mesh_color_plan.h) for
// tests/test_mesh_color_reference.py.
//   mesh_color_check scene IN OUT   IN: int64 n_ref, channels, n_vertices, has_keep, fill; double tol, min_cos; int32
//                                   heights[n_ref], widths[n_ref]; double proj[n_ref][12], centres[n_ref][3]; float
//                                   depth[n_out]; uint8 keep[n_out] (when has_keep); uint8 pixels[n_out][channels];
//                                   double vertices[n_vertices][3]; float normals[n_vertices][3]
//                                   OUT: uint8 colors[n_vertices][channels], uint8 n_views[n_vertices], int32
//                                   best_view[n_vertices].  The views go through tsdf_check_views as the entry point
//                                   sends them, every view its own image.
//   mesh_color_check plan           the workspace, the launch size and every branch of the argument checks; prints "ok <cases>"
// Build with -ffp-contract=off (the headers' pragma is clang's).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mesh_color_plan.h"
#include "mesh_color_rule.h"

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

// k_mesh_colors for one vertex, one view at a time
static void color_vertex(const TsdfView* views, int n_ref, const double* proj, const double* centres, const float* depth, const uint8_t* keep,
                         const uint8_t* pixels, int ch, const double* X, const float* nf, double tol, double min_cos, int fill,
                         uint8_t* colors, uint8_t* n_views, int32_t* best_view) {
  const double n[3] = {(double)nf[0], (double)nf[1], (double)nf[2]};
  double acc[3] = {0.0, 0.0, 0.0};
  mesh_color::Tally tally = mesh_color::empty_tally();
  for (int v = 0; v < n_ref; ++v) {
    const TsdfView view = views[v];
    const mesh_color::Projection p = mesh_color::project(proj + (int64_t)v * 12, X[0], X[1], X[2], view.w, view.h);
    const tsdf::Projection q = tsdf::project(proj + (int64_t)v * 12, X[0], X[1], X[2], view.w, view.h);
    REQUIRE(p.valid == q.valid && p.xi == q.xi && p.yi == q.yi);          // the widened projection is the integration's
    if (!p.valid) continue;
    REQUIRE(std::memcmp(&p.q2, &q.q2, 8) == 0);
    const int64_t e = view.out_off + (int64_t)p.yi * view.w + p.xi;
    REQUIRE(e >= view.out_off && e < views[v + 1].out_off);
    if (!mesh_color::sees((double)depth[e], keep ? keep[e] != 0 : 1, p.q2, tol)) continue;
    double wgt = 0.0;
    if (!mesh_color::weight(centres + (int64_t)v * 3, X, n, min_cos, &wgt)) continue;
    const mesh_color::Taps t = mesh_color::taps(p.u, p.v, view.w, view.h);
    REQUIRE(t.x0 >= 0 && t.x0 <= t.x1 && t.x1 < view.w && t.y0 >= 0 && t.y0 <= t.y1 && t.y1 < view.h);
    const uint8_t* img = pixels + view.out_off * ch;
    for (int k = 0; k < ch; ++k) {
      const double a = (double)img[((int64_t)t.y0 * view.w + t.x0) * ch + k], b = (double)img[((int64_t)t.y0 * view.w + t.x1) * ch + k];
      const double c = (double)img[((int64_t)t.y1 * view.w + t.x0) * ch + k], d = (double)img[((int64_t)t.y1 * view.w + t.x1) * ch + k];
      acc[k] = mesh_color::add_sample(acc[k], wgt, mesh_color::bilinear(a, b, c, d, t.fx, t.fy));
    }
    mesh_color::add_view(&tally, wgt, v);
  }
  for (int k = 0; k < ch; ++k) colors[k] = mesh_color::finish(acc[k], tally, fill);
  *n_views = mesh_color::finish_views(tally);
  *best_view = tally.best;
}

static int run_scene(const char* in, const char* out) {
  std::FILE* fi = std::fopen(in, "rb");
  REQUIRE(fi);
  const std::vector<int64_t> head = read_n<int64_t>(fi, 5);
  const std::vector<double> scalars = read_n<double>(fi, 2);
  const int64_t n_ref = head[0], ch = head[1], nv = head[2], has_keep = head[3], fill = head[4];
  REQUIRE(n_ref >= 0 && n_ref <= TSDF_MAX_VIEWS);
  REQUIRE(mesh_color_check(ch, nv, scalars[0], scalars[1], fill) == 0);
  const std::vector<int32_t> heights = read_n<int32_t>(fi, n_ref), widths = read_n<int32_t>(fi, n_ref);
  std::vector<int32_t> ref_image((size_t)n_ref);
  for (int64_t r = 0; r < n_ref; ++r) ref_image[(size_t)r] = (int32_t)r;
  std::vector<TsdfView> views((size_t)n_ref + 1);
  REQUIRE(tsdf_check_views(n_ref, heights.data(), widths.data(), n_ref, ref_image.data(), views.data()) == 0);
  int64_t n_out = 0;
  for (int64_t r = 0; r < n_ref; ++r) n_out += (int64_t)views[(size_t)r].h * views[(size_t)r].w;
  views[(size_t)n_ref] = TsdfView{n_out, 0, 0};
  REQUIRE((int64_t)(views.size() * sizeof(TsdfView)) <= mesh_color_workspace_bytes(n_ref));
  const std::vector<double> proj = read_n<double>(fi, n_ref * 12), centres = read_n<double>(fi, n_ref * 3);
  const std::vector<float> depth = read_n<float>(fi, n_out);
  const std::vector<uint8_t> keep = read_n<uint8_t>(fi, has_keep ? n_out : 0), pixels = read_n<uint8_t>(fi, n_out * ch);
  const std::vector<double> vertices = read_n<double>(fi, nv * 3);
  const std::vector<float> normals = read_n<float>(fi, nv * 3);
  std::fclose(fi);
  std::vector<uint8_t> colors((size_t)(nv * ch)), n_views((size_t)nv);
  std::vector<int32_t> best((size_t)nv);
  for (int64_t i = 0; i < nv; ++i)
    color_vertex(views.data(), (int)n_ref, proj.data(), centres.data(), depth.data(), has_keep ? keep.data() : nullptr, pixels.data(), (int)ch,
                 vertices.data() + 3 * i, normals.data() + 3 * i, scalars[0], scalars[1], (int)fill, colors.data() + i * ch,
                 n_views.data() + i, best.data() + i);
  std::FILE* fo = std::fopen(out, "wb");
  REQUIRE(fo);
  write_all(fo, colors);
  write_all(fo, n_views);
  write_all(fo, best);
  std::fclose(fo);
  return 0;
}

static int check_plan() {
  int cases = 0;
  const double nan = std::nan(""), inf = 1.0 / 0.0;
  REQUIRE(mesh_color_check(1, 0, 0.0, 1.0, 0) == 0 && mesh_color_check(3, MESH_COLOR_MAX_VERTICES, 0.5, 0.35, 255) == 0);
  for (int64_t ch : {0, 2, 4, -1}) { REQUIRE(mesh_color_check(ch, 10, 0.1, 0.35, 0) == 1); ++cases; }
  for (int64_t nv : {(int64_t)-1, (int64_t)(MESH_COLOR_MAX_VERTICES + 1)}) { REQUIRE(mesh_color_check(3, nv, 0.1, 0.35, 0) == 2); ++cases; }
  for (double tol : {-0.1, nan, inf, -inf}) { REQUIRE(mesh_color_check(3, 10, tol, 0.35, 0) == 3); ++cases; }
  for (double mc : {0.0, -0.5, 1.5, nan, inf}) { REQUIRE(mesh_color_check(3, 10, 0.1, mc, 0) == 4); ++cases; }
  for (int64_t fill : {-1, 256}) { REQUIRE(mesh_color_check(3, 10, 0.1, 0.35, fill) == 5); ++cases; }
  for (int k = 1; k <= 7; ++k) REQUIRE(std::strlen(MESH_COLOR_WHY[k]) > 0);
  // the buffers: p stands for any pointer; each may be missing only where nothing is read or written through it
  {
    const char byte = 0;
    const void* p = &byte;
    const int64_t need = mesh_color_workspace_bytes(2);
    REQUIRE(mesh_color_check_buffers(2, 9, 5, p, p, p, p, p, p, p, p, p, p, need) == 0);
    REQUIRE(mesh_color_check_buffers(2, 9, 5, p, p, p, p, p, p, p, p, p, nullptr, need) == 6);
    REQUIRE(mesh_color_check_buffers(2, 9, 5, p, p, p, p, p, p, p, p, p, p, need - 1) == 6);
    REQUIRE(mesh_color_check_buffers(2, 9, 5, nullptr, p, p, p, p, p, p, p, p, p, need) == 7);
    REQUIRE(mesh_color_check_buffers(2, 9, 5, p, nullptr, p, p, p, p, p, p, p, p, need) == 7);
    REQUIRE(mesh_color_check_buffers(2, 9, 5, p, p, nullptr, p, p, p, p, p, p, p, need) == 7);
    REQUIRE(mesh_color_check_buffers(2, 9, 5, p, p, p, nullptr, p, p, p, p, p, p, need) == 7);
    REQUIRE(mesh_color_check_buffers(2, 9, 5, p, p, p, p, nullptr, p, p, p, p, p, need) == 7);
    REQUIRE(mesh_color_check_buffers(2, 9, 5, p, p, p, p, p, nullptr, p, p, p, p, need) == 7);
    REQUIRE(mesh_color_check_buffers(2, 9, 5, p, p, p, p, p, p, nullptr, p, p, p, need) == 7);
    REQUIRE(mesh_color_check_buffers(2, 9, 5, p, p, p, p, p, p, p, nullptr, p, p, need) == 7);
    REQUIRE(mesh_color_check_buffers(2, 9, 5, p, p, p, p, p, p, p, p, nullptr, p, need) == 7);
    REQUIRE(mesh_color_check_buffers(2, 0, 5, p, p, nullptr, nullptr, p, p, p, p, p, p, need) == 0);          // no pixel
    REQUIRE(mesh_color_check_buffers(2, 9, 0, p, p, p, p, nullptr, nullptr, nullptr, nullptr, nullptr, p, need) == 0);      // no vertex
    REQUIRE(mesh_color_check_buffers(0, 0, 5, nullptr, nullptr, nullptr, nullptr, p, p, p, p, p, p, mesh_color_workspace_bytes(0)) == 0);      // no view
    cases += 15;
  }
  // the workspace holds n_ref records and the one that closes the list
  for (int64_t n_ref : {0, 1, 3, 300, TSDF_MAX_VIEWS}) {
    REQUIRE(mesh_color_workspace_bytes(n_ref) >= (n_ref + 1) * (int64_t)sizeof(TsdfView));
    REQUIRE(mesh_color_workspace_bytes(n_ref) == tsdf_workspace_bytes(n_ref));
    ++cases;
  }
  // the launch: every vertex has a thread, the last block is not empty, the largest mesh fits a launch
  for (int64_t nv : {(int64_t)1, (int64_t)255, (int64_t)256, (int64_t)257, (int64_t)1000, (int64_t)MESH_COLOR_MAX_VERTICES}) {
    const int64_t nb = mesh_color_blocks(nv);
    REQUIRE(nb * MESH_BLOCK >= nv && (nb - 1) * MESH_BLOCK < nv && nb < 0x7FFFFFFFLL);
    ++cases;
  }
  REQUIRE(mesh_color_blocks(0) == 0);
  REQUIRE(MESH_COLOR_BATCH >= 1);
  // the views the entry point refuses are those of the integration
  const int32_t hs[2] = {3, 4}, ws[2] = {5, 6}, neg[2] = {3, -4}, refs[2] = {1, 0}, twice[2] = {1, 1}, far[1] = {2};
  TsdfView views[2];
  REQUIRE(tsdf_check_views(2, hs, ws, 2, refs, views) == 0 && views[1].out_off == 24 && views[1].h == 3);
  REQUIRE(tsdf_check_views(2, neg, ws, 1, refs, nullptr) == 7 && tsdf_check_views(2, hs, ws, 2, twice, nullptr) == 9);
  REQUIRE(tsdf_check_views(2, hs, ws, 1, far, nullptr) == 8 && tsdf_check_views(2, hs, ws, 3, refs, nullptr) == 9);
  // the taps never leave the image, whatever a valid (u, v) is
  const double us[] = {-0.5, -0.25, -1e-300, 0.0, 0.5, 3.0, 3.999999, 4.0, 4.49999999};
  for (double u : us)
    for (double v : us) {
      for (int w : {5, 1}) {
        const mesh_color::Taps t = mesh_color::taps(w == 1 ? (u > 0.49 ? 0.49 : u) : u, v, w, 5);
        REQUIRE(t.x0 >= 0 && t.x1 < w && t.x0 <= t.x1 && t.y0 >= 0 && t.y1 < 5 && t.y0 <= t.y1);
        REQUIRE(t.fx >= 0.0 && t.fx <= 1.0 && t.fy >= 0.0 && t.fy <= 1.0);
        ++cases;
      }
    }
  std::printf("ok %d\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "scene")) return run_scene(argv[2], argv[3]);
  if (argc == 2 && !std::strcmp(argv[1], "plan")) return check_plan();
  std::fprintf(stderr, "usage: mesh_color_check scene IN OUT | plan\n");
  return 2;
}
