// Host build of the rule and the launch plan of mesh smoothing (sfm_amd/csrc/mesh_smooth_rule.h, mesh_smooth_plan.h) for
// tests/test_mesh_smooth_reference.py.
//   mesh_smooth_check rule FILE  FILE holds one case as the restatement wrote it: "nv nt iterations has_mu pin_boundary
//                                has_pinned", lam and mu as the 16 hex digits of their float64 bits, nv lines "x y z [pinned]"
//                                (float64 bits), nt lines "a b c".  The program builds the adjacency on the host with the
//                                functions of the rule - the keys sorted, a run of equal keys one entry -, the states, the
//                                steps through the two buffers in the order the plan gives, and the normals over the corners
//                                in ascending h; it prints "A entries boundary isolated unsound", "S pinned_boundary
//                                pinned_given unsound isolated", per entry "e j", per vertex "v ptr flags state x y z nx ny nz"
//                                (bits in hex) and "p ptr[nv]"
//   mesh_smooth_check plan       the argument checks branch by branch and in their firing order; the workspace layouts over
//                                a grid of sizes - aligned, ascending, disjoint, within bytes; the bits and the order of the
//                                keys; where every step writes; the entries per block through the two-level scan; prints
//                                "ok <checks>"
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "mesh_smooth_plan.h"
#include "mesh_smooth_rule.h"
#include "scan_replay.h"

#define REQUIRE(c) SCAN_REPLAY_REQUIRE(c)

static double read_f64(std::FILE* f) {
  uint64_t b = 0;
  REQUIRE(std::fscanf(f, "%" SCNx64, &b) == 1);
  double v;
  std::memcpy(&v, &b, 8);
  return v;
}
static uint64_t bits64(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }
static uint32_t bits32(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }

static int run_rule(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  REQUIRE(f != nullptr);
  long long nv = 0, nt = 0, iterations = 0;
  int has_mu = 0, pin_boundary = 0, has_pinned = 0;
  REQUIRE(std::fscanf(f, "%lld %lld %lld %d %d %d", &nv, &nt, &iterations, &has_mu, &pin_boundary, &has_pinned) == 6 && nv >= 0 && nt >= 0);
  const double lam = read_f64(f), mu = read_f64(f);
  std::vector<double> x((size_t)nv * 3 + 3);
  std::vector<uint8_t> pinned((size_t)nv + 1, 0);
  for (long long i = 0; i < nv; ++i) {
    for (int a = 0; a < 3; ++a) x[(size_t)(3 * i + a)] = read_f64(f);
    if (has_pinned) { int p; REQUIRE(std::fscanf(f, "%d", &p) == 1); pinned[(size_t)i] = (uint8_t)p; }
  }
  std::vector<int32_t> tri((size_t)nt * 3);
  for (int32_t& v : tri) { int y; REQUIRE(std::fscanf(f, "%d", &y) == 1); v = y; }
  std::fclose(f);
  REQUIRE(smo_check_counts(nv, nt) == 0);

  // adjacency: two keys per live half-edge, sorted; a run of equal keys is one entry and its length the uses
  std::vector<uint64_t> keys;
  long long unsound_triangles = 0;
  for (long long t = 0; t < nt; ++t) {
    const int32_t* w = &tri[(size_t)(3 * t)];
    if (!mesh_clean::sound(w[0], w[1], w[2], nv)) ++unsound_triangles;
    for (int k = 0; k < 3; ++k) {
      int32_t a, b;
      const int live = mesh_smooth::halfedge(w, k, nv, &a, &b);
      keys.push_back(live ? mesh_smooth::edge_key(a, b) : MESH_ADJ_DEAD_KEY);
      keys.push_back(live ? mesh_smooth::edge_key(b, a) : MESH_ADJ_DEAD_KEY);
    }
  }
  REQUIRE((long long)keys.size() == 6 * nt);
  const int bits = smo_key_bits(nv);
  const uint64_t mask = (1ull << bits) - 1ull;                      // the sort sees these bits only
  std::sort(keys.begin(), keys.end(), [&](uint64_t a, uint64_t b) { return (a & mask) < (b & mask); });
  std::vector<uint64_t> entry_key;
  std::vector<int32_t> index, uses;
  for (size_t s = 0; s < keys.size(); ++s) {
    if (keys[s] == MESH_ADJ_DEAD_KEY) { for (size_t r = s; r < keys.size(); ++r) REQUIRE(keys[r] == MESH_ADJ_DEAD_KEY); break; }
    if (s > 0 && keys[s - 1] == keys[s]) { ++uses.back(); continue; }
    REQUIRE(s == 0 || keys[s - 1] < keys[s]);
    entry_key.push_back(keys[s]);
    index.push_back(mesh_smooth::key_neighbour(keys[s]));
    uses.push_back(1);
  }
  std::vector<int32_t> ptr((size_t)nv + 1);
  std::vector<uint8_t> flags((size_t)nv + 1, 0), state((size_t)nv + 1, 0);
  long long n_boundary = 0, n_isolated = 0, c_state[4] = {0, 0, 0, 0};
  for (long long v = 0; v <= nv; ++v)
    ptr[(size_t)v] = (int32_t)(std::lower_bound(entry_key.begin(), entry_key.end(), (uint64_t)v << 32) - entry_key.begin());
  for (long long v = 0; v < nv; ++v) {
    bool odd = false;
    for (int32_t e = ptr[(size_t)v]; e < ptr[(size_t)v + 1]; ++e) {
      REQUIRE(mesh_smooth::key_vertex(entry_key[(size_t)e]) == v);
      odd = odd || uses[(size_t)e] != 2;
    }
    flags[(size_t)v] = mesh_smooth::vertex_flags(ptr[(size_t)v + 1] - ptr[(size_t)v], odd);
    n_boundary += (flags[(size_t)v] & MESH_ADJ_BOUNDARY) != 0;
    n_isolated += (flags[(size_t)v] & MESH_ADJ_ISOLATED) != 0;
    state[(size_t)v] = mesh_smooth::vertex_state(flags[(size_t)v], pinned[(size_t)v] != 0, pin_boundary != 0, &x[(size_t)(3 * v)]);
    for (int b = 0; b < 4; ++b) c_state[b] += (state[(size_t)v] >> b) & 1;
  }

  // the steps: the input, the workspace and the output as the plan walks them
  REQUIRE(smo_check_smooth(nv, (int64_t)index.size(), iterations, lam, mu, has_mu, x.data(), ptr.data(), index.empty() ? nullptr : index.data(), flags.data(),
                           state.data() /* any other pointer */, state.data(), state.data()) == 0);
  std::vector<double> out(x), second(x.size(), -7.0);
  const int64_t n_steps = smo_steps(iterations, has_mu);
  const double* src = x.data();
  for (int64_t i = 0; i < n_steps; ++i) {
    double* dst = smo_step_writes_out(n_steps, i) ? out.data() : second.data();
    REQUIRE(dst != src);
    const double fct = smo_step_factor(i, lam, mu, has_mu);
    for (long long v = 0; v < nv; ++v) {
      double* o = dst + 3 * v;
      const double* me = src + 3 * v;
      o[0] = me[0]; o[1] = me[1]; o[2] = me[2];
      if (state[(size_t)v] != 0) continue;
      double s[3] = {0.0, 0.0, 0.0};
      int64_t n = 0;
      for (int32_t e = ptr[(size_t)v]; e < ptr[(size_t)v + 1]; ++e) {
        const int32_t j = index[(size_t)e];
        REQUIRE(j >= 0 && j < nv);
        if (state[(size_t)j] & MESH_SMOOTH_UNSOUND) continue;
        mesh_smooth::add_neighbour(src + 3 * (int64_t)j, s);
        ++n;
      }
      if (n > 0) mesh_smooth::move(me, s, n, fct, o);
    }
    src = dst;
  }
  REQUIRE(n_steps == 0 || src == out.data());

  // normals: the stable order of (vertex, h)
  std::vector<int32_t> corner;
  for (long long h = 0; h < 3 * nt; ++h) {
    const int32_t* w = &tri[(size_t)(3 * (h / 3))];
    if (mesh_clean::sound(w[0], w[1], w[2], nv)) corner.push_back((int32_t)h);
  }
  std::stable_sort(corner.begin(), corner.end(), [&](int32_t a, int32_t b) { return tri[(size_t)a] < tri[(size_t)b]; });
  std::vector<double> ns((size_t)nv * 3 + 3, 0.0);
  std::vector<float> nrm((size_t)nv * 3 + 3, 0.0f);
  for (int32_t h : corner) {
    const int32_t* w = &tri[(size_t)(3 * (h / 3))];
    double n[3];
    mesh_smooth::face_normal(&out[(size_t)(3 * (int64_t)w[0])], &out[(size_t)(3 * (int64_t)w[1])], &out[(size_t)(3 * (int64_t)w[2])], n);
    mesh_smooth::add_face(n, &ns[(size_t)(3 * (int64_t)tri[(size_t)h])]);
  }
  for (long long v = 0; v < nv; ++v) mesh_smooth::unit_normal(&ns[(size_t)(3 * v)], &nrm[(size_t)(3 * v)]);

  std::printf("A %zu %lld %lld %lld\n", index.size(), n_boundary, n_isolated, unsound_triangles);
  std::printf("S %lld %lld %lld %lld\n", c_state[0], c_state[1], c_state[2], c_state[3]);
  for (int32_t j : index) std::printf("e %d\n", j);
  for (long long v = 0; v < nv; ++v)
    std::printf("v %d %d %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %08x %08x %08x\n", ptr[(size_t)v], flags[(size_t)v], state[(size_t)v],
                bits64(out[(size_t)(3 * v)]), bits64(out[(size_t)(3 * v + 1)]), bits64(out[(size_t)(3 * v + 2)]), bits32(nrm[(size_t)(3 * v)]),
                bits32(nrm[(size_t)(3 * v + 1)]), bits32(nrm[(size_t)(3 * v + 2)]));
  std::printf("p %d\n", ptr[(size_t)nv]);
  return 0;
}

static int checks = 0;
#define SAME(a, b) do { REQUIRE((a) == (b)); ++checks; } while (0)

static void check_layouts(int64_t nv, int64_t nt, int64_t sort_bytes) {
  {
    const AdjLayout L = adj_layout(nt, sort_bytes);
    const int64_t n = 6 * nt, nb = smo_blocks(n);
    REQUIRE(nb * SMO_BLOCK >= n && (nb == 0 || (nb - 1) * SMO_BLOCK < n));
    const int64_t off[] = {L.key_in, L.key_out, L.uses, L.blk, L.chunk, L.sort, L.bytes};
    const int64_t len[] = {n * 8, n * 8, n * 4, nb * 4, scan_chunks(nb) * 8, sort_bytes};
    for (int i = 0; i < 6; ++i) { REQUIRE(off[i] % 256 == 0 && off[i] + len[i] <= off[i + 1]); ++checks; }
    REQUIRE(L.key_in == 0 && L.bytes >= 256 && adj_layout(nt, sort_bytes + 4096).bytes == L.bytes + 4096);
  }
  {
    const NrmLayout L = nrm_layout(nt, sort_bytes);
    const int64_t n = 3 * nt;
    const int64_t off[] = {L.key_in, L.key_out, L.val_in, L.val_out, L.sort, L.bytes};
    const int64_t len[] = {n * 4, n * 4, n * 4, n * 4, sort_bytes};
    for (int i = 0; i < 5; ++i) { REQUIRE(off[i] % 256 == 0 && off[i] + len[i] <= off[i + 1]); ++checks; }
    REQUIRE(L.key_in == 0 && L.bytes >= 256);
  }
  REQUIRE(smo_layout_bytes(nv) >= nv * 24 + 256 && smo_layout_bytes(nv) % 256 == 0);
  ++checks;
}

static uint64_t rng_state = 23;
static uint64_t rnd() {
  rng_state += 0x9E3779B97F4A7C15ull;
  uint64_t z = rng_state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the entries per block through the two-level scan as k_adj_scan_chunks / k_adj_scan_top / k_adj_scatter walk it
static void check_scan(int64_t n) {
  const int64_t nb = smo_blocks(n);
  std::vector<uint32_t> blk((size_t)nb), counts;
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t in = std::min<int64_t>(std::max<int64_t>(n - b * SMO_BLOCK, 0), SMO_BLOCK);
    blk[(size_t)b] = b % 3 == 0 ? (uint32_t)in : (uint32_t)(rnd() % (uint64_t)(in + 1));
  }
  counts = blk;
  std::vector<int64_t> chunk;
  scan_replay::chunk_counts(blk, chunk);
  chunk.push_back(0);
  const int64_t all = scan_replay::chunk_totals(chunk.data(), scan_chunks(nb), 1);
  int64_t run = 0;
  for (int64_t b = 0; b < nb; ++b) {
    REQUIRE(scan_base(chunk.data(), 1, 0, b, (int64_t)blk[(size_t)b]) == run);
    run += counts[(size_t)b];
  }
  REQUIRE(all == run && run <= n);
  ++checks;
}

static int run_plan() {
  const int64_t bigv = SMO_MAX_VERTICES, bigt = SMO_MAX_TRIANGLES;
  int x = 0, y = 0;
  const void *p = &x, *q = &y;
  const double nan = std::nan("");
  REQUIRE(6 * bigt <= 0x7FFFFFFFLL && 6 * (bigt + 1) > 0x7FFFFFFFLL);
  SAME(smo_check_counts(0, 0), 0); SAME(smo_check_counts(bigv, bigt), 0);
  SAME(smo_check_counts(-1, 0), 1); SAME(smo_check_counts(0, -1), 1); SAME(smo_check_counts(bigv + 1, 0), 1); SAME(smo_check_counts(0, bigt + 1), 1);
  SAME(smo_check_workspace(nullptr, 100, 10), 8); SAME(smo_check_workspace(p, 9, 10), 8); SAME(smo_check_workspace(p, 10, 10), 0);
  // sfm_mesh_adjacency: sizes, then pointers
  SAME(smo_check_adjacency(5, 2, p, p, p, p, p), 0); SAME(smo_check_adjacency(0, 0, nullptr, p, nullptr, nullptr, p), 0);
  SAME(smo_check_adjacency(5, 0, nullptr, p, nullptr, p, p), 0); SAME(smo_check_adjacency(0, 2, p, p, p, nullptr, p), 0);
  SAME(smo_check_adjacency(-1, 2, nullptr, nullptr, p, p, p), 1); SAME(smo_check_adjacency(5, bigt + 1, nullptr, p, p, p, p), 1);
  SAME(smo_check_adjacency(5, 2, nullptr, p, p, p, p), 2); SAME(smo_check_adjacency(5, 2, p, nullptr, p, p, p), 2); SAME(smo_check_adjacency(5, 2, p, p, nullptr, p, p), 2);
  SAME(smo_check_adjacency(5, 2, p, p, p, nullptr, p), 2); SAME(smo_check_adjacency(5, 2, p, p, p, p, nullptr), 2);
  SAME(smo_check_adjacency(0, 0, nullptr, nullptr, nullptr, nullptr, p), 2);
  // sfm_mesh_smooth: sizes, n_index, iterations, lam, mu, pointers, the two vertex arrays
  auto smooth = [&](int64_t nv, int64_t ni, int64_t it, double lam, double mu, int has_mu, const void* vin = nullptr, const void* vout = nullptr, int hole = -1) {
    const void* a[7];
    for (int i = 0; i < 7; ++i) a[i] = i == hole ? nullptr : p;
    a[0] = hole == 0 ? nullptr : (vin ? vin : p);
    a[4] = hole == 4 ? nullptr : (vout ? vout : q);
    return smo_check_smooth(nv, ni, it, lam, mu, has_mu, a[0], a[1], a[2], a[3], a[4], a[5], a[6]);
  };
  SAME(smooth(5, 12, 10, 0.5, -0.53, 1), 0); SAME(smooth(5, 12, 0, 1.0, -2.0, 1), 0); SAME(smooth(5, 12, 1000, 1e-300, nan, 0), 0);
  SAME(smooth(5, 12, 10, 0.5, 7.0, 0), 0); SAME(smooth(0, 0, 10, 0.5, -0.53, 1, p, p), 0); SAME(smooth(5, 0, 10, 0.5, -0.53, 1, nullptr, nullptr, 2), 0);
  SAME(smooth(-1, -1, -1, 0.0, 0.0, 1, p, p, 0), 1); SAME(smooth(bigv + 1, 12, 10, 0.5, -0.53, 1), 1);
  SAME(smooth(5, -1, -1, 0.0, 0.0, 1, p, p, 0), 6); SAME(smooth(5, bigv + 1, 10, 0.5, -0.53, 1), 6);
  SAME(smooth(5, 12, -1, 0.0, 0.0, 1, p, p, 0), 3); SAME(smooth(5, 12, 1001, 0.5, -0.53, 1), 3);
  SAME(smooth(5, 12, 10, 0.0, 0.0, 1, p, p, 0), 4); SAME(smooth(5, 12, 10, -0.5, -0.53, 1), 4); SAME(smooth(5, 12, 10, 1.0000001, -1.5, 1), 4);
  SAME(smooth(5, 12, 10, nan, -0.53, 1), 4); SAME(smooth(5, 12, 10, INFINITY, -0.53, 1), 4);
  SAME(smooth(5, 12, 10, 0.5, -0.5, 1, p, p, 0), 5); SAME(smooth(5, 12, 10, 0.5, -0.4, 1), 5); SAME(smooth(5, 12, 10, 0.5, 0.53, 1), 5);
  SAME(smooth(5, 12, 10, 0.5, -2.0000001, 1), 5); SAME(smooth(5, 12, 10, 0.5, nan, 1), 5); SAME(smooth(5, 12, 10, 0.5, -INFINITY, 1), 5);
  for (int hole = 0; hole < 7; ++hole) SAME(smooth(5, 12, 10, 0.5, -0.53, 1, p, p, hole), 2);
  SAME(smooth(5, 12, 10, 0.5, -0.53, 1, p, p), 7); SAME(smooth(5, 12, 10, 0.5, -0.53, 1, q, q), 7);
  // sfm_mesh_vertex_normals
  SAME(smo_check_normals(5, 2, p, p, p), 0); SAME(smo_check_normals(0, 0, nullptr, nullptr, nullptr), 0); SAME(smo_check_normals(5, 0, p, nullptr, p), 0);
  SAME(smo_check_normals(0, 2, nullptr, p, nullptr), 0);
  SAME(smo_check_normals(-1, 2, nullptr, p, p), 1); SAME(smo_check_normals(5, bigt + 1, nullptr, p, p), 1);
  SAME(smo_check_normals(5, 2, nullptr, p, p), 2); SAME(smo_check_normals(5, 2, p, nullptr, p), 2); SAME(smo_check_normals(5, 2, p, p, nullptr), 2);
  for (int why = 1; why <= 8; ++why) REQUIRE(SMO_WHY[why][0] != 0);
  // the bits of a vertex and the order of the keys under the bits the sort walks
  SAME(smo_vertex_bits(0), 1); SAME(smo_vertex_bits(1), 1); SAME(smo_vertex_bits(2), 2); SAME(smo_vertex_bits(255), 8); SAME(smo_vertex_bits(256), 9);
  SAME(smo_vertex_bits(bigv), 31); SAME(smo_key_bits(256), 41); SAME(smo_key_bits(bigv), 63);
  for (int64_t nv : {(int64_t)1, (int64_t)3, (int64_t)255, (int64_t)256, (int64_t)70000, bigv}) {
    const int bits = smo_key_bits(nv);
    const uint64_t mask = (1ull << bits) - 1ull;
    REQUIRE((1ll << (bits - 32)) - 1 >= nv);                       // all ones stays above every vertex
    for (int i = 0; i < 200; ++i) {
      const int32_t a = (int32_t)(rnd() % (uint64_t)nv), b = (int32_t)(rnd() % (uint64_t)nv), c = i % 4 == 0 ? a : (int32_t)(rnd() % (uint64_t)nv),
                    d = (int32_t)(rnd() % (uint64_t)nv);
      const uint64_t ka = mesh_smooth::edge_key(a, b), kb = mesh_smooth::edge_key(c, d);
      REQUIRE(((ka & mask) < (kb & mask)) == (a < c || (a == c && b < d)) && (ka & mask) == ka && (ka & mask) < (MESH_ADJ_DEAD_KEY & mask));
      REQUIRE(mesh_smooth::key_vertex(ka) == a && mesh_smooth::key_neighbour(ka) == b);
      ++checks;
    }
  }
  // where the steps write: the last one the output, never the buffer they read
  for (int has_mu = 0; has_mu < 2; ++has_mu)
    for (int64_t it : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)3, (int64_t)10, (int64_t)1000}) {
      const int64_t n = smo_steps(it, has_mu);
      SAME(n, it * (has_mu ? 2 : 1));
      int before = -1;                                             // the input
      for (int64_t i = 0; i < n; ++i) {
        const int w = smo_step_writes_out(n, i);
        REQUIRE(w != before && (w == 0 || w == 1));
        SAME(smo_step_factor(i, 0.5, -0.53, has_mu), (has_mu && i % 2 == 1) ? -0.53 : 0.5);
        before = w;
      }
      REQUIRE(n == 0 || before == 1);
    }
  // the rule's small functions
  {
    const int32_t t[3] = {4, 4, 7}, u[3] = {1, 2, 9};
    int32_t a, b;
    SAME(mesh_smooth::halfedge(t, 0, 8, &a, &b), 0); SAME(mesh_smooth::halfedge(t, 1, 8, &a, &b), 1); REQUIRE(a == 4 && b == 7);
    SAME(mesh_smooth::halfedge(t, 2, 8, &a, &b), 1); REQUIRE(a == 7 && b == 4);
    SAME(mesh_smooth::halfedge(t, 1, 7, &a, &b), 0); SAME(mesh_smooth::halfedge(u, 0, 9, &a, &b), 0); SAME(mesh_smooth::halfedge(u, 0, 10, &a, &b), 1);
    SAME(mesh_smooth::vertex_flags(0, false), MESH_ADJ_ISOLATED); SAME(mesh_smooth::vertex_flags(3, false), 0); SAME(mesh_smooth::vertex_flags(3, true), MESH_ADJ_BOUNDARY);
    const double fine[3] = {1.0, -2.0, 1e308}, bad[3] = {1.0, nan, 0.0}, inf[3] = {INFINITY, 0.0, 0.0};
    SAME(mesh_smooth::vertex_state(0, false, true, fine), 0); SAME(mesh_smooth::vertex_state(1, false, true, fine), 1); SAME(mesh_smooth::vertex_state(1, false, false, fine), 0);
    SAME(mesh_smooth::vertex_state(0, true, false, fine), 2); SAME(mesh_smooth::vertex_state(0, false, true, bad), 4); SAME(mesh_smooth::vertex_state(0, false, true, inf), 4);
    SAME(mesh_smooth::vertex_state(2, false, true, fine), 8); SAME(mesh_smooth::vertex_state(3, true, true, bad), 15);
  }
  // layouts and scans around every seam: the block (256), the chunk (262,144) and one past
  const int64_t seam[] = {0, 1, 42, 43, 255, 256, 257, 1023, 1025, 43690, 43691, 262143, 262144, 262145, 600000};
  for (int64_t nv : seam)
    for (int64_t nt : seam)
      for (int64_t sort_bytes : {(int64_t)0, (int64_t)1, (int64_t)1234567}) check_layouts(nv, nt, sort_bytes);
  for (int64_t n : seam) check_scan(6 * n);
  check_layouts(bigv, bigt, (int64_t)1 << 33);
  REQUIRE(adj_layout(bigt, 0).bytes > bigt * 120);
  std::printf("ok %d\n", checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "rule")) return run_rule(argv[2]);
  if (argc == 2 && !std::strcmp(argv[1], "plan")) return run_plan();
  std::fprintf(stderr, "usage: mesh_smooth_check rule FILE | plan\n");
  return 2;
}
