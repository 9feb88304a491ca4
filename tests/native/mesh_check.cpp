// Host build of the meshing rule and plan (sfm_amd/csrc/tsdf_rule.h, mesh_rule.h, mesh_plan.h) for tests/test_mesh_reference.py.
//   mesh_check table             derives the 6 x 16 cases from the geometric rule (tetrahedra of the Kuhn split, the two
//                                triangle patterns, the orientation by n . D) and compares with MESH_CASE / MESH_TET_CORNER;
//                                prints "ok <cases>"
//   mesh_check vertex IN OUT     IN: int64 n, then n records of { double fa, fb, XA[3], XB[3], gA[3], gB[3] }
//                                OUT: n records of { double V[3]; float n[3]; int32 pad }
//   mesh_check gradient IN OUT   IN: n records of { double f0, fp, fm; int32 kp, km }      OUT: n records of { double g }
//   mesh_check node IN OUT       IN: n records of { double P[12], X[3], ds, trunc, acc; int32 w, h, kept, pad }
//                                OUT: n records of { int32 valid, xi, yi, counted; double q2, acc }
//   mesh_check finish IN OUT     IN: n records of { double acc; int32 w, pad }             OUT: n records of { uint32 bits, pad }
//   mesh_check plan SEED         the ranks of the nodes of a block, the node record, the two-level scan as the kernels walk
//                                it and the first slots it gives against running sums, for small grids and for block counts
//                                around the chunk size and above MESH_BLOCK chunks; the layout; the checks; prints "ok <cases>"
// Build with -ffp-contract=off (the headers' pragma is clang's).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mesh_plan.h"
#include "mesh_rule.h"
#include "tsdf_rule.h"
#include "scan_replay.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct VertexIn { double fa, fb, XA[3], XB[3], gA[3], gB[3]; };
struct VertexOut { double V[3]; float n[3]; int32_t pad; };
struct GradientIn { double f0, fp, fm; int32_t kp, km; };
struct GradientOut { double g; };
struct NodeIn { double P[12], X[3], ds, trunc, acc; int32_t w, h, kept, pad; };
struct NodeOut { int32_t valid, xi, yi, counted; double q2, acc; };
struct FinishIn { double acc; int32_t w, pad; };
struct FinishOut { uint32_t bits, pad; };

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

// ---- the table from the geometric rule ----
struct V3 { int x, y, z; };
static V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V3 mul(int s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
static V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static int dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static int corner_of(V3 a) { return a.x + 2 * a.y + 4 * a.z; }

static int check_table() {
  static const int perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  static const V3 dirs[7] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 0}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1}};
  for (int d = 0; d < 7; ++d) REQUIRE(MESH_DIR_CORNER(d) == corner_of(dirs[d]));
  int cases = 0;
  for (int T = 0; T < 6; ++T) {
    V3 off[4] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {1, 1, 1}};
    int e1[3] = {0, 0, 0}, e2[3] = {0, 0, 0};
    e1[perms[T][0]] = 1;
    e2[perms[T][1]] = 1;
    off[1] = V3{e1[0], e1[1], e1[2]};
    off[2] = add(off[1], V3{e2[0], e2[1], e2[2]});
    for (int n = 0; n < 4; ++n) REQUIRE(MESH_TET_CORNER[T][n] == corner_of(off[n]));
    for (int c = 0; c < 16; ++c) {
      int ins[4], out[4], ni = 0, no = 0;
      for (int n = 0; n < 4; ++n) { if ((c >> n) & 1) ins[ni++] = n; else out[no++] = n; }
      int tri[2][3][2], nt = 0;                                // triangle, vertex, the two local nodes of the edge
      if (ni == 1 || no == 1) {
        const int p = ni == 1 ? ins[0] : out[0];
        int k = 0;
        for (int n = 0; n < 4; ++n) if (n != p) { tri[0][k][0] = p; tri[0][k][1] = n; ++k; }
        nt = 1;
      } else if (ni == 2) {
        const int p = ins[0], q = ins[1], r = out[0], s = out[1];
        const int a[3][2] = {{p, r}, {p, s}, {q, s}}, b[3][2] = {{p, r}, {q, s}, {q, r}};
        std::memcpy(tri[0], a, sizeof(a));
        std::memcpy(tri[1], b, sizeof(b));
        nt = 2;
      }
      V3 so{0, 0, 0}, si{0, 0, 0};
      for (int n = 0; n < no; ++n) so = add(so, off[out[n]]);
      for (int n = 0; n < ni; ++n) si = add(si, off[ins[n]]);
      const V3 D = sub(mul(ni, so), mul(no, si));
      const uint8_t* row = MESH_CASE[T][c];
      REQUIRE(row[0] == nt);
      REQUIRE(mesh::tet_case(T, 0) == 0 && mesh::tet_case(T, 255) == 15);
      for (int t = 0; t < 2; ++t) {
        if (t >= nt) { REQUIRE(row[1 + 3 * t] == 0 && row[2 + 3 * t] == 0 && row[3 + 3 * t] == 0); continue; }
        V3 m[3];
        for (int v = 0; v < 3; ++v) m[v] = add(off[tri[t][v][0]], off[tri[t][v][1]]);
        const int nd = dot(cross(sub(m[1], m[0]), sub(m[2], m[0])), D);
        REQUIRE(nd != 0);
        const int order[3] = {0, nd < 0 ? 2 : 1, nd < 0 ? 1 : 2};
        for (int v = 0; v < 3; ++v) {
          const int a = tri[t][order[v]][0], b = tri[t][order[v]][1], lo = a < b ? a : b, hi = a < b ? b : a;
          const V3 dv = sub(off[hi], off[lo]);
          int d = -1;
          for (int k = 0; k < 7; ++k) if (dirs[k].x == dv.x && dirs[k].y == dv.y && dirs[k].z == dv.z) d = k;
          REQUIRE(d >= 0);
          REQUIRE(row[1 + 3 * t + v] == ((corner_of(off[lo]) << 3) | d));
        }
      }
      ++cases;
    }
  }
  // the cells of an edge: every corner the node can be of a cell that shares no axis with the direction
  for (int d = 0; d < 7; ++d)
    for (int c = 0; c < 8; ++c) REQUIRE((((mesh::edge_cells(d) >> c) & 1) != 0) == ((c & corner_of(dirs[d])) == 0));
  int most = 0;
  for (int i8 = 0; i8 < 256; ++i8) { const int n = mesh::cell_triangles(i8); REQUIRE(n >= 0 && n <= MESH_MAX_CELL_TRIANGLES); most = n > most ? n : most; }
  REQUIRE(most == MESH_MAX_CELL_TRIANGLES && mesh::cell_triangles(0) == 0 && mesh::cell_triangles(255) == 0);
  std::printf("ok %d\n", cases);
  return 0;
}

// ---- the plan ----
static uint64_t rng_state;
static uint64_t rnd() {
  rng_state += 0x9E3779B97F4A7C15ull;
  uint64_t z = rng_state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// k_mesh_scan_chunks and k_mesh_scan_top on the host (the shared replay of scan_replay.h): blk holds the packed counts on
// entry and the packed sums within a chunk on return, chunk_base two sums per chunk; totals[2] is what goes to counts
static void mesh_scan(std::vector<uint64_t>& blk, std::vector<int64_t>& chunk_base, int64_t* totals) {
  std::vector<int64_t> packed;
  scan_replay::chunk_counts(blk, packed);
  const int64_t n_chunks = (int64_t)packed.size();
  chunk_base.assign((size_t)n_chunks * 2, 0);
  for (int64_t c = 0; c < n_chunks; ++c) {
    chunk_base[(size_t)(2 * c)] = packed[(size_t)c] & 0xFFFFFFFFll;
    chunk_base[(size_t)(2 * c + 1)] = packed[(size_t)c] >> 32;
  }
  for (int half = 0; half < 2; ++half) totals[half] = scan_replay::chunk_totals(chunk_base.data() + half, n_chunks, 2);
}

static int check_plan(uint64_t seed) {
  rng_state = seed;
  int cases = 0;
  // per node: small grids, every node with random counts (or the largest ones), the record and the slots it gives
  const int grids[][3] = {{2, 2, 2}, {3, 2, 2}, {5, 4, 6}, {2, 2, 64}, {2, 2, 65}, {5, 5, 11}, {64, 64, 9}, {65, 64, 64}};
  for (const auto& g : grids) {
    for (int full = 0; full < 2; ++full) {
      REQUIRE(mesh_check_grid(g[0], g[1], g[2]) == 0);
      const int64_t n = mesh_nodes(g[0], g[1], g[2]), nb = mesh_blocks(n);
      REQUIRE(mesh_node(g[0] - 1, g[1] - 1, g[2] - 1, g[0], g[1]) == n - 1 && mesh_node(1, 0, 0, g[0], g[1]) == 1);
      std::vector<int> mask((size_t)n), tris((size_t)n);
      std::vector<uint32_t> record((size_t)n);
      std::vector<uint64_t> blk((size_t)nb);
      for (int64_t i = 0; i < n; ++i) {
        mask[(size_t)i] = full ? 127 : (int)(rnd() % 128);
        tris[(size_t)i] = full ? MESH_MAX_CELL_TRIANGLES : (int)(rnd() % (MESH_MAX_CELL_TRIANGLES + 1));
      }
      for (int64_t b = 0; b < nb; ++b) {                          // k_mesh_mark: the packed pair, scanned over the block
        int run = 0;
        for (int tid = 0; tid < MESH_BLOCK; ++tid) {
          const int64_t i = b * MESH_BLOCK + tid;
          if (i >= n) continue;
          const int v = __builtin_popcount((unsigned)mask[(size_t)i]) | (tris[(size_t)i] << 16);
          const uint32_t r = mesh_record(mask[(size_t)i], run & 0xFFFF, run >> 16, (int)(i & 1));
          REQUIRE(mesh_record_mask(r) == mask[(size_t)i] && mesh_record_vrank(r) == (run & 0xFFFF) && mesh_record_trank(r) == (run >> 16));
          REQUIRE(mesh_record_active(r) == (int)(i & 1));
          record[(size_t)i] = r;
          run += v;
          REQUIRE((run & 0xFFFF) <= MESH_BLOCK * 7 && (run >> 16) <= MESH_BLOCK * MESH_MAX_CELL_TRIANGLES);
        }
        blk[(size_t)b] = mesh_count_pack((uint32_t)(run & 0xFFFF), (uint32_t)(run >> 16));
      }
      std::vector<int64_t> chunk_base;
      int64_t totals[2];
      mesh_scan(blk, chunk_base, totals);
      int64_t nv = 0, nt = 0;
      for (int64_t i = 0; i < n; ++i) {
        const int64_t b = i / MESH_BLOCK;
        REQUIRE(mesh_vertex_base(chunk_base.data(), blk.data(), b) + mesh_record_vrank(record[(size_t)i]) == nv);
        REQUIRE(mesh_triangle_base(chunk_base.data(), blk.data(), b) + mesh_record_trank(record[(size_t)i]) == nt);
        nv += __builtin_popcount((unsigned)mask[(size_t)i]);
        nt += tris[(size_t)i];
      }
      REQUIRE(totals[0] == nv && totals[1] == nt);
      // the layout: nothing overlaps, all inside
      const MeshLayout L = mesh_layout(n);
      REQUIRE(L.flags == 0 && L.record >= n && L.record % 256 == 0 && L.blk >= L.record + n * 4 && L.blk % 256 == 0);
      REQUIRE(L.chunk_base >= L.blk + nb * 8 && L.chunk_base % 256 == 0 && L.bytes >= L.chunk_base + scan_chunks(nb) * 16);
      ++cases;
    }
  }
  // per block: block counts around the chunk size and above MESH_BLOCK chunks
  const int64_t sizes[] = {1, SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 3 * SCAN_CHUNK + 7,
                           (int64_t)MESH_BLOCK * SCAN_CHUNK + 5, (int64_t)(MESH_BLOCK + 1) * SCAN_CHUNK + 1};
  for (int64_t nb : sizes) {
    for (int full = 0; full < 2; ++full) {
      std::vector<uint64_t> blk((size_t)nb), counts;
      for (auto& c : blk)
        c = full ? mesh_count_pack(MESH_BLOCK * 7, MESH_BLOCK * MESH_MAX_CELL_TRIANGLES)
                 : mesh_count_pack((uint32_t)(rnd() % (MESH_BLOCK * 7 + 1)), (uint32_t)(rnd() % (MESH_BLOCK * MESH_MAX_CELL_TRIANGLES + 1)));
      counts = blk;
      std::vector<int64_t> chunk_base;
      int64_t totals[2], nv = 0, nt = 0;
      mesh_scan(blk, chunk_base, totals);
      for (int64_t b = 0; b < nb; ++b) {
        REQUIRE(mesh_vertex_base(chunk_base.data(), blk.data(), b) == nv && mesh_triangle_base(chunk_base.data(), blk.data(), b) == nt);
        nv += (int64_t)(counts[(size_t)b] & 0xFFFFFFFFull);
        nt += (int64_t)(counts[(size_t)b] >> 32);
      }
      REQUIRE(totals[0] == nv && totals[1] == nt);
      ++cases;
    }
  }
  // the largest grid: the blocks fit a launch, the layout 64 bits
  REQUIRE(mesh_blocks(mesh_nodes(MESH_MAX_DIM, MESH_MAX_DIM, MESH_MAX_DIM)) < 0x7FFFFFFFLL);
  REQUIRE(mesh_layout(mesh_nodes(MESH_MAX_DIM, MESH_MAX_DIM, MESH_MAX_DIM)).bytes > 5LL * 1024 * 1024 * 1024);
  // the checks
  const double nan = std::nan(""), inf = 1.0 / 0.0, o[3] = {0.0, -1.0, 2.0}, o_nan[3] = {0.0, nan, 0.0}, o_inf[3] = {inf, 0.0, 0.0};
  REQUIRE(mesh_check_grid(2, 2, 2) == 0 && mesh_check_grid(1024, 1024, 1024) == 0);
  REQUIRE(mesh_check_grid(1, 2, 2) == 1 && mesh_check_grid(2, 1025, 2) == 1 && mesh_check_grid(2, 2, -5) == 1);
  REQUIRE(mesh_check_frame(o, 0.5) == 0 && mesh_check_frame(nullptr, 0.5) == 2 && mesh_check_frame(o_nan, 0.5) == 3 && mesh_check_frame(o_inf, 0.5) == 3);
  REQUIRE(mesh_check_frame(o, 0.0) == 4 && mesh_check_frame(o, -1.0) == 4 && mesh_check_frame(o, nan) == 4 && mesh_check_frame(o, inf) == 4);
  REQUIRE(tsdf_check_trunc(0.1) == 0 && tsdf_check_trunc(0.0) == 5 && tsdf_check_trunc(-1.0) == 5 && tsdf_check_trunc(nan) == 5);
  const int32_t hs[3] = {3, 4, 0}, ws[3] = {5, 6, 7}, neg[3] = {3, -4, 0}, refs[3] = {2, 0, 1}, twice[2] = {1, 1}, far[1] = {3};
  TsdfView views[3];
  REQUIRE(tsdf_check_views(3, hs, ws, 3, refs, views) == 0);
  REQUIRE(views[0].out_off == 0 && views[0].h == 0 && views[0].w == 7 && views[1].out_off == 0 && views[1].h == 3 && views[1].w == 5);
  REQUIRE(views[2].out_off == 15 && views[2].h == 4 && views[2].w == 6);
  REQUIRE(tsdf_check_views(0, nullptr, nullptr, 0, nullptr, nullptr) == 0);
  REQUIRE(tsdf_check_views(3, neg, ws, 1, refs, nullptr) == 7 && tsdf_check_views(3, hs, ws, 2, twice, nullptr) == 9);
  REQUIRE(tsdf_check_views(3, hs, ws, 1, far, nullptr) == 8 && tsdf_check_views(3, hs, ws, 4, refs, nullptr) == 9);
  REQUIRE(tsdf_check_views(3, hs, ws, -1, refs, nullptr) == 9 && tsdf_check_views(-1, hs, ws, 0, refs, nullptr) == 10);
  REQUIRE(tsdf_check_views(70000, hs, ws, TSDF_MAX_VIEWS + 1, refs, nullptr) == 6 && tsdf_check_views(3, nullptr, ws, 1, refs, nullptr) == 2);
  REQUIRE(tsdf_workspace_bytes(3) >= 4 * (int64_t)sizeof(TsdfView));
  // the table the four per-view calls put into the workspace: the records of the check, n_out and the closing record
  ViewTable table;
  REQUIRE(view_table_build(3, hs, ws, 3, refs, &table) == 0 && table.views.size() == 4 && table.n_out == 39);
  for (int r = 0; r < 3; ++r) REQUIRE(table.views[r].out_off == views[r].out_off && table.views[r].h == views[r].h && table.views[r].w == views[r].w);
  REQUIRE(table.views[3].out_off == 39 && table.views[3].h == 0 && table.views[3].w == 0);
  REQUIRE(view_table_build(3, hs, ws, 1, refs, &table) == 0 && table.views.size() == 2 && table.n_out == 0 && table.views[1].out_off == 0);
  REQUIRE(view_table_build(0, nullptr, nullptr, 0, nullptr, &table) == 0 && table.views.size() == 1 && table.n_out == 0);
  // an n_ref out of range sizes nothing by itself, and the index is the check's own
  REQUIRE(view_table_build(3, hs, ws, -1, refs, &table) == 9 && table.views.size() == 1);
  REQUIRE(view_table_build(0x7FFFFFFFLL, hs, ws, 0x7FFFFFFFLL, refs, &table) == 6 && table.views.size() == 1);
  REQUIRE(view_table_build(3, hs, ws, 4, refs, &table) == 9 && view_table_build(3, hs, ws, 2, twice, &table) == 9);
  REQUIRE(view_table_build(3, neg, ws, 1, refs, &table) == 7 && view_table_build(3, hs, ws, 1, far, &table) == 8);
  REQUIRE(view_table_build(-1, hs, ws, 0, refs, &table) == 10 && view_table_build(3, nullptr, ws, 1, refs, &table) == 2);
  const int x = 0;
  REQUIRE(view_pointers_ok(0, 0, nullptr, nullptr, nullptr, nullptr) && view_pointers_ok(2, 5, &x, &x, &x, &x));
  REQUIRE(view_pointers_ok(2, 0, &x, &x, nullptr, nullptr) && view_pointers_ok(0, 5, nullptr, nullptr, &x, &x));
  REQUIRE(!view_pointers_ok(2, 0, nullptr, &x, &x, &x) && !view_pointers_ok(2, 0, &x, nullptr, &x, &x));
  REQUIRE(!view_pointers_ok(0, 5, &x, &x, nullptr, &x) && !view_pointers_ok(0, 5, &x, &x, &x, nullptr));
  for (int k = 1; k <= 11; ++k) REQUIRE(std::strlen(MESH_WHY[k]) > 0);
  std::printf("ok %d\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "table")) return check_table();
  if (argc == 4 && !std::strcmp(argv[1], "vertex"))
    return run_records<VertexIn, VertexOut>(argv[2], argv[3], [](const VertexIn& r) {
      VertexOut o;
      const double t = mesh::cut(r.fa, r.fb);
      for (int a = 0; a < 3; ++a) o.V[a] = mesh::lerp(r.XA[a], r.XB[a], t);
      mesh::normal(r.gA, r.gB, t, o.n);
      o.pad = 0;
      return o;
    });
  if (argc == 4 && !std::strcmp(argv[1], "gradient"))
    return run_records<GradientIn, GradientOut>(argv[2], argv[3], [](const GradientIn& r) {
      return GradientOut{mesh::gradient(r.f0, r.fp, r.fm, r.kp, r.km)};
    });
  if (argc == 4 && !std::strcmp(argv[1], "node"))
    return run_records<NodeIn, NodeOut>(argv[2], argv[3], [](const NodeIn& r) {
      NodeOut o;
      const tsdf::Projection p = tsdf::project(r.P, r.X[0], r.X[1], r.X[2], r.w, r.h);
      o.valid = p.valid; o.xi = p.xi; o.yi = p.yi; o.q2 = p.q2;
      o.acc = r.acc;
      o.counted = p.valid ? tsdf::add_view(r.ds, r.kept, p.q2, r.trunc, &o.acc) : 0;
      return o;
    });
  if (argc == 4 && !std::strcmp(argv[1], "finish"))
    return run_records<FinishIn, FinishOut>(argv[2], argv[3], [](const FinishIn& r) { return FinishOut{tsdf::finish_bits(r.acc, r.w), 0u}; });
  if (argc == 3 && !std::strcmp(argv[1], "plan")) return check_plan(std::strtoull(argv[2], nullptr, 10));
  std::fprintf(stderr, "usage: mesh_check table | vertex|gradient|node|finish IN OUT | plan SEED\n");
  return 2;
}
