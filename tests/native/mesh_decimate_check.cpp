// Host build of the rule and the launch plan of decimation by vertex clustering (sfm_amd/csrc/mesh_decimate_rule.h,
// mesh_decimate_plan.h) for tests/test_mesh_decimate_reference.py.
//   mesh_decimate_check rule FILE  FILE holds one mesh as the restatement wrote it: "nv nt placement has_normals", the
//                                  origin and the cell as the 16 hex digits of their float64 bits, nv lines "x y z [nx ny nz]"
//                                  (float64 bits, then float32 bits), nt lines "a b c".  The program decimates it on the host
//                                  with the functions of the rule - keys, members in ascending index, corners in ascending
//                                  h, the solve, the duplicate rule - and prints "C nc unsound", "M kept unsound degenerate
//                                  dropped", the cluster of every vertex, per cluster "first size placed x y z nx ny nz" (bits
//                                  in hex) and per kept triangle "t c0 c1 c2"
//   mesh_decimate_check plan       the argument checks branch by branch and in their firing order; the workspace layout
//                                  over a grid of sizes - aligned, ascending, disjoint, within bytes, the part the calls hand
//                                  on at offsets that do not depend on the sort; the bits, the passes and the order of the
//                                  triple keys; the kept triangles per block through the two-level scan; prints "ok <checks>"
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <tuple>
#include <vector>

#include "mesh_decimate_plan.h"
#include "mesh_decimate_rule.h"
#include "scan_replay.h"

#define REQUIRE(c) SCAN_REPLAY_REQUIRE(c)

static double read_f64(std::FILE* f) {
  uint64_t b = 0;
  REQUIRE(std::fscanf(f, "%" SCNx64, &b) == 1);
  double v;
  std::memcpy(&v, &b, 8);
  return v;
}
static float read_f32(std::FILE* f) {
  uint32_t b = 0;
  REQUIRE(std::fscanf(f, "%" SCNx32, &b) == 1);
  float v;
  std::memcpy(&v, &b, 4);
  return v;
}
static uint64_t bits64(double v) { uint64_t b; std::memcpy(&b, &v, 8); return b; }
static uint32_t bits32(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; }

static int run_rule(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  REQUIRE(f != nullptr);
  long long nv = 0, nt = 0;
  int placement = 0, has_normals = 0;
  REQUIRE(std::fscanf(f, "%lld %lld %d %d", &nv, &nt, &placement, &has_normals) == 4 && nv >= 0 && nt >= 0);
  double origin[3];
  for (double& o : origin) o = read_f64(f);
  const double cell = read_f64(f);
  REQUIRE(dec_check_grid(origin, cell) == 0);
  std::vector<double> v((size_t)nv * 3);
  std::vector<float> nrm((size_t)nv * 3);
  for (long long i = 0; i < nv; ++i) {
    for (int a = 0; a < 3; ++a) v[(size_t)(3 * i + a)] = read_f64(f);
    if (has_normals) for (int a = 0; a < 3; ++a) nrm[(size_t)(3 * i + a)] = read_f32(f);
  }
  std::vector<int32_t> tri((size_t)nt * 3);
  for (int32_t& x : tri) { int y; REQUIRE(std::fscanf(f, "%d", &y) == 1); x = y; }
  std::fclose(f);

  // clusters: the stable order of (key, vertex)
  std::vector<uint64_t> key((size_t)nv);
  std::vector<int64_t> cellidx((size_t)nv * 3);
  for (long long i = 0; i < nv; ++i) key[(size_t)i] = mesh_decimate::vertex_key(&v[(size_t)(3 * i)], origin, cell, &cellidx[(size_t)(3 * i)]);
  std::vector<int32_t> order((size_t)nv);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return key[(size_t)a] < key[(size_t)b]; });
  std::vector<int32_t> vc((size_t)nv, -1), start;
  long long live = 0;
  for (long long s = 0; s < nv; ++s) {
    const uint64_t k = key[(size_t)order[(size_t)s]];
    if (k == MESH_DEC_DEAD_KEY) break;
    if (s == 0 || key[(size_t)order[(size_t)(s - 1)]] != k) start.push_back((int32_t)s);
    vc[(size_t)order[(size_t)s]] = (int32_t)start.size() - 1;
    ++live;
  }
  const long long nc = (long long)start.size();
  start.push_back((int32_t)live);
  std::vector<double> mean((size_t)nc * 3), x((size_t)nc * 3), A((size_t)nc * 6, 0.0), g((size_t)nc * 3, 0.0);
  std::vector<float> outn((size_t)nc * 3, 0.0f);
  std::vector<int> placed((size_t)nc, 0);
  for (long long c = 0; c < nc; ++c) {
    double s[3] = {0, 0, 0}, ns[3] = {0, 0, 0};
    for (int32_t i = start[(size_t)c]; i < start[(size_t)c + 1]; ++i) {
      const int32_t m = order[(size_t)i];
      mesh_decimate::add_member(i - start[(size_t)c], &v[(size_t)(3 * m)], has_normals ? &nrm[(size_t)(3 * m)] : nullptr, s, ns);
    }
    mesh_decimate::mean(s, start[(size_t)c + 1] - start[(size_t)c], &mean[(size_t)(3 * c)]);
    if (has_normals) mesh_decimate::unit_normal(ns, &outn[(size_t)(3 * c)]);
  }
  // triangles: corners in ascending h, the groups of equal triples
  long long unsound = 0, degenerate = 0, alive = 0;
  struct Group { int64_t n_even = 0, n_odd = 0, first_even = -1, first_odd = -1; };
  std::map<std::tuple<int32_t, int32_t, int32_t>, Group> groups;
  for (long long t = 0; t < nt; ++t) {
    const int32_t* w = &tri[(size_t)(3 * t)];
    int32_t c[3] = {-1, -1, -1};
    bool ok = mesh_clean::sound(w[0], w[1], w[2], nv);
    for (int k = 0; ok && k < 3; ++k) { c[k] = vc[(size_t)w[k]]; }
    ok = ok && c[0] >= 0 && c[1] >= 0 && c[2] >= 0;
    if (!ok) { ++unsound; continue; }
    for (int k = 0; k < 3; ++k)
      mesh_decimate::add_corner(&v[(size_t)(3 * w[0])], &v[(size_t)(3 * w[1])], &v[(size_t)(3 * w[2])], &mean[(size_t)(3 * c[k])], &A[(size_t)(6 * c[k])],
                                &g[(size_t)(3 * c[k])]);
    int32_t s[3];
    int odd;
    if (!mesh_decimate::sort_triple(c[0], c[1], c[2], s, &odd)) { ++degenerate; continue; }
    ++alive;
    Group& G = groups[std::make_tuple(s[0], s[1], s[2])];
    if (odd) { if (G.n_odd++ == 0) G.first_odd = t; } else { if (G.n_even++ == 0) G.first_even = t; }
  }
  for (long long c = 0; c < nc; ++c) {
    const int32_t first = order[(size_t)start[(size_t)c]];
    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
      lo[a] = mesh_decimate::cell_lo(origin[a], cell, cellidx[(size_t)(3 * first + a)]);
      hi[a] = mesh_decimate::cell_hi(origin[a], cell, cellidx[(size_t)(3 * first + a)]);
    }
    if (placement == 1) placed[(size_t)c] = mesh_decimate::place(&A[(size_t)(6 * c)], &g[(size_t)(3 * c)], &mean[(size_t)(3 * c)], lo, hi, &x[(size_t)(3 * c)]);
    else for (int a = 0; a < 3; ++a) x[(size_t)(3 * c + a)] = mean[(size_t)(3 * c + a)];
  }
  std::vector<int64_t> kept;
  for (const auto& kv : groups) {
    const int64_t pick = mesh_decimate::duplicate_pick(kv.second.n_even, kv.second.n_odd, kv.second.first_even, kv.second.first_odd);
    if (pick >= 0) kept.push_back(pick);
  }
  std::sort(kept.begin(), kept.end());
  std::printf("C %lld %lld\n", nc, nv - live);
  std::printf("M %zu %lld %lld %lld\n", kept.size(), unsound, degenerate, alive - (long long)kept.size());
  for (long long i = 0; i < nv; ++i) std::printf("v %d\n", vc[(size_t)i]);
  for (long long c = 0; c < nc; ++c)
    std::printf("c %d %d %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %08x %08x %08x\n", order[(size_t)start[(size_t)c]],
                start[(size_t)c + 1] - start[(size_t)c], placed[(size_t)c], bits64(x[(size_t)(3 * c)]), bits64(x[(size_t)(3 * c + 1)]),
                bits64(x[(size_t)(3 * c + 2)]), bits32(outn[(size_t)(3 * c)]), bits32(outn[(size_t)(3 * c + 1)]), bits32(outn[(size_t)(3 * c + 2)]));
  for (int64_t t : kept)
    std::printf("t %" PRId64 " %d %d %d\n", t, vc[(size_t)tri[(size_t)(3 * t)]], vc[(size_t)tri[(size_t)(3 * t + 1)]], vc[(size_t)tri[(size_t)(3 * t + 2)]]);
  return 0;
}

static int checks = 0;
#define SAME(a, b) do { REQUIRE((a) == (b)); ++checks; } while (0)

static void check_layout(int64_t nv, int64_t nt, int64_t sort_bytes) {
  const DecLayout L = dec_layout(nv, nt, sort_bytes);
  const int64_t n = 3 * nt, vb = dec_blocks(nv), tb = dec_blocks(nt);
  REQUIRE(vb * DEC_BLOCK >= nv && (vb == 0 || (vb - 1) * DEC_BLOCK < nv));
  const int64_t off[] = {L.sorted_vertex, L.corner_key, L.corner_val, L.tri_blk, L.tri_chunk, L.vkey_in, L.vkey_out, L.vval_in, L.vblk, L.vchunk,
                         L.ckey_in, L.cval_in, L.tkey_in, L.tkey_out, L.tlow_in, L.tlow_out, L.tval_a, L.tval_b, L.sort, L.bytes};
  const int64_t len[] = {nv * 4, n * 4, n * 4, tb * 4, scan_chunks(tb) * 8, nv * 8, nv * 8, nv * 4, vb * 4, scan_chunks(vb) * 8,
                         n * 4, n * 4, nt * 8, nt * 8, nt * 4, nt * 4, nt * 4, nt * 4, sort_bytes};
  for (int i = 0; i < 19; ++i) {
    REQUIRE(off[i] % 256 == 0 && off[i] + len[i] <= off[i + 1]);
    ++checks;
  }
  REQUIRE(L.sorted_vertex == 0 && L.bytes >= 256);
  // what one call hands to the next does not move with the storage of the sorts; a sizing call and the call it sizes get
  // the same layout from the same three numbers
  const DecLayout M = dec_layout(nv, nt, sort_bytes + 4096);
  REQUIRE(M.sorted_vertex == L.sorted_vertex && M.corner_key == L.corner_key && M.corner_val == L.corner_val && M.tri_blk == L.tri_blk &&
          M.tri_chunk == L.tri_chunk && M.sort == L.sort && M.bytes == L.bytes + 4096);
  const DecLayout S = dec_layout(nv, nt, sort_bytes);
  REQUIRE(std::memcmp(&S, &L, sizeof(L)) == 0);
  ++checks;
}

static uint64_t rng_state = 17;
static uint64_t rnd() {
  rng_state += 0x9E3779B97F4A7C15ull;
  uint64_t z = rng_state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// kept triangles per block through the two-level scan as k_dec_scan_chunks / k_dec_scan_top / k_dec_emit_triangles walk it
static void check_scan(int64_t nt) {
  const int64_t nb = dec_blocks(nt);
  std::vector<uint32_t> blk((size_t)nb), counts;
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t in = std::min<int64_t>(std::max<int64_t>(nt - b * DEC_BLOCK, 0), DEC_BLOCK);
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
  REQUIRE(all == run && run <= nt);
  ++checks;
}

static int run_plan() {
  const int64_t bigv = DEC_MAX_VERTICES, bigt = DEC_MAX_TRIANGLES;
  int x = 0;
  const void* p = &x;
  const double o[3] = {0.0, -1.5, 1e9}, nan_o[3] = {0.0, std::nan(""), 0.0}, inf_o[3] = {INFINITY, 0.0, 0.0};
  REQUIRE(3 * bigt <= 0x7FFFFFFFLL && 3 * (bigt + 1) > 0x7FFFFFFFLL);
  SAME(dec_check_counts(0, 0), 0); SAME(dec_check_counts(bigv, bigt), 0);
  SAME(dec_check_counts(-1, 0), 1); SAME(dec_check_counts(0, -1), 1); SAME(dec_check_counts(bigv + 1, 0), 1); SAME(dec_check_counts(0, bigt + 1), 1);
  SAME(dec_check_grid(o, 1.0), 0); SAME(dec_check_grid(o, 1e-300), 0); SAME(dec_check_grid(nullptr, 1.0), 5);
  SAME(dec_check_grid(nan_o, 1.0), 3); SAME(dec_check_grid(inf_o, 1.0), 3); SAME(dec_check_grid(o, 0.0), 3); SAME(dec_check_grid(o, -1.0), 3);
  SAME(dec_check_grid(o, std::nan("")), 3); SAME(dec_check_grid(o, INFINITY), 3);
  SAME(dec_check_workspace(nullptr, 100, 10), 7); SAME(dec_check_workspace(p, 9, 10), 7); SAME(dec_check_workspace(p, 10, 10), 0);
  // sfm_mesh_decimate_cluster: sizes, then pointers, then the grid
  SAME(dec_check_cluster(5, 2, p, o, 1.0, p, p, p, p, p), 0);
  SAME(dec_check_cluster(0, 0, nullptr, o, 1.0, nullptr, p, nullptr, nullptr, p), 0);
  SAME(dec_check_cluster(-1, 2, nullptr, nan_o, 0.0, p, p, p, p, p), 1); SAME(dec_check_cluster(5, bigt + 1, p, o, 1.0, p, p, p, p, p), 1);
  SAME(dec_check_cluster(5, 2, nullptr, nan_o, 1.0, p, p, p, p, p), 5); SAME(dec_check_cluster(5, 2, p, nullptr, 1.0, p, p, p, p, p), 5);
  SAME(dec_check_cluster(5, 2, p, o, 1.0, nullptr, p, p, p, p), 5); SAME(dec_check_cluster(5, 2, p, o, 1.0, p, nullptr, p, p, p), 5);
  SAME(dec_check_cluster(0, 0, nullptr, o, 1.0, nullptr, nullptr, nullptr, nullptr, p), 5);
  SAME(dec_check_cluster(5, 2, p, o, 1.0, p, p, nullptr, p, p), 5); SAME(dec_check_cluster(5, 2, p, o, 1.0, p, p, p, nullptr, p), 5);
  SAME(dec_check_cluster(5, 2, p, o, 1.0, p, p, p, p, nullptr), 5);
  SAME(dec_check_cluster(5, 2, p, nan_o, 1.0, p, p, p, p, p), 3); SAME(dec_check_cluster(5, 2, p, o, 0.0, p, p, p, p, p), 3);
  // sfm_mesh_decimate_mark
  SAME(dec_check_mark(5, 2, 3, p, p, p, p), 0); SAME(dec_check_mark(5, 2, 0, p, p, p, p), 0); SAME(dec_check_mark(5, 2, 5, p, p, p, p), 0);
  SAME(dec_check_mark(5, 0, 3, nullptr, nullptr, nullptr, p), 0); SAME(dec_check_mark(0, 2, 0, p, nullptr, p, p), 0);
  SAME(dec_check_mark(-1, 2, 9, nullptr, p, p, p), 1); SAME(dec_check_mark(5, bigt + 1, 3, p, p, p, p), 1);
  SAME(dec_check_mark(5, 2, -1, nullptr, p, p, p), 2); SAME(dec_check_mark(5, 2, 6, p, p, p, p), 2);
  SAME(dec_check_mark(5, 2, 3, nullptr, p, p, p), 5); SAME(dec_check_mark(5, 2, 3, p, nullptr, p, p), 5); SAME(dec_check_mark(5, 2, 3, p, p, nullptr, p), 5);
  SAME(dec_check_mark(5, 2, 3, p, p, p, nullptr), 5);
  // sfm_mesh_decimate_emit: sizes, clusters, capacities, placement, grid
  SAME(dec_check_emit_counts(5, 2, 3, 3, 2, 1, o, 1.0), 0); SAME(dec_check_emit_counts(5, 2, 3, 0, 0, 0, o, 1.0), 0);
  SAME(dec_check_emit_counts(0, 0, 0, bigv, bigv, 1, o, 1.0), 0);
  SAME(dec_check_emit_counts(bigv + 1, 2, 9, -1, 2, 7, nan_o, 1.0), 1); SAME(dec_check_emit_counts(5, 2, 6, -1, 2, 7, nan_o, 1.0), 2);
  SAME(dec_check_emit_counts(5, 2, -1, 3, 2, 1, o, 1.0), 2);
  SAME(dec_check_emit_counts(5, 2, 3, -1, 2, 7, nan_o, 1.0), 6); SAME(dec_check_emit_counts(5, 2, 3, 3, -1, 1, o, 1.0), 6);
  SAME(dec_check_emit_counts(5, 2, 3, bigv + 1, 2, 1, o, 1.0), 6); SAME(dec_check_emit_counts(5, 2, 3, 3, bigv + 1, 1, o, 1.0), 6);
  SAME(dec_check_emit_counts(5, 2, 3, 3, 2, 2, nan_o, 1.0), 4); SAME(dec_check_emit_counts(5, 2, 3, 3, 2, -1, o, 1.0), 4);
  SAME(dec_check_emit_counts(5, 2, 3, 3, 2, 1, nullptr, 1.0), 5); SAME(dec_check_emit_counts(5, 2, 3, 3, 2, 1, nan_o, 1.0), 3);
  SAME(dec_check_emit_counts(5, 2, 3, 3, 2, 0, o, -2.0), 3);
  SAME(dec_check_emit_pointers(2, 3, 2, p, p, p, p, p, p, p, p, p, p, p), 0);
  SAME(dec_check_emit_pointers(2, 3, 2, p, nullptr, p, p, p, p, p, nullptr, p, p, p), 0);
  SAME(dec_check_emit_pointers(2, 0, 2, nullptr, nullptr, p, p, nullptr, p, nullptr, nullptr, nullptr, p, p), 0);
  SAME(dec_check_emit_pointers(2, 3, 0, p, p, p, p, p, nullptr, p, p, p, nullptr, nullptr), 0);
  SAME(dec_check_emit_pointers(0, 3, 0, p, p, nullptr, nullptr, p, nullptr, p, p, p, nullptr, nullptr), 0);
  for (int hole = 0; hole < 11; ++hole) {
    if (hole == 1) continue;                                           // normals may be null
    const void* a[11];
    for (int i = 0; i < 11; ++i) a[i] = i == hole ? nullptr : p;
    SAME(dec_check_emit_pointers(2, 3, 2, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10]), 5);
  }
  for (int why = 1; why <= 7; ++why) REQUIRE(DEC_WHY[why][0] != 0);
  // the bits of a cluster number, the passes and the order of the keys
  SAME(dec_cluster_bits(0), 1); SAME(dec_cluster_bits(1), 1); SAME(dec_cluster_bits(2), 2); SAME(dec_cluster_bits(255), 8); SAME(dec_cluster_bits(256), 9);
  SAME(dec_cluster_bits(bigv), 31);
  SAME(dec_triple_passes(0), 1); SAME(dec_triple_passes((1 << 21) - 1), 1); SAME(dec_triple_passes(1 << 21), 2); SAME(dec_triple_passes(bigv), 2);
  for (int64_t nc : {(int64_t)3, (int64_t)255, (int64_t)256, (int64_t)70000, (int64_t)(1 << 21) - 1, (int64_t)1 << 21, bigv}) {
    const int bits = dec_cluster_bits(nc);
    REQUIRE((1ll << bits) > nc - 1 && (1ll << bits) - 1 >= nc);      // every number fits and all ones stays above them
    for (int i = 0; i < 200; ++i) {
      int32_t a[3], b[3];
      for (int k = 0; k < 3; ++k) { a[k] = (int32_t)(rnd() % (uint64_t)nc); b[k] = i % 4 == 0 && k < 2 ? a[k] : (int32_t)(rnd() % (uint64_t)nc); }
      std::sort(a, a + 3); std::sort(b, b + 3);
      const bool less = std::lexicographical_compare(a, a + 3, b, b + 3);
      if (dec_triple_passes(nc) == 1) {
        const uint64_t ka = dec_triple_key(a[0], a[1], a[2], bits), kb = dec_triple_key(b[0], b[1], b[2], bits);
        REQUIRE((ka < kb) == less && ka < (1ull << (3 * bits)) && ka != MESH_DEC_DEAD_KEY);
      } else {
        const auto ka = std::make_pair(dec_pair_key(a[0], a[1]), (uint32_t)a[2]), kb = std::make_pair(dec_pair_key(b[0], b[1]), (uint32_t)b[2]);
        REQUIRE((ka < kb) == less && ka.first < (1ull << (32 + bits)));
      }
      ++checks;
    }
  }
  // the cell of a coordinate and the key
  SAME(mesh_decimate::cell_index(0.0, 0.0, 1.0), 0); SAME(mesh_decimate::cell_index(-0.0, 0.0, 1.0), 0); SAME(mesh_decimate::cell_index(-1e-300, 0.0, 1.0), -1);
  SAME(mesh_decimate::cell_index(2097151.5, 0.0, 1.0), 2097151); SAME(mesh_decimate::cell_index(2097152.0, 0.0, 1.0), -1);
  SAME(mesh_decimate::cell_index(std::nan(""), 0.0, 1.0), -1); SAME(mesh_decimate::cell_index(INFINITY, 0.0, 1.0), -1);
  SAME(mesh_decimate::cell_index(1e308, -1e308, 1.0), -1); SAME(mesh_decimate::cell_index(3.0, 1.0, 2.0), 1); SAME(mesh_decimate::cell_index(1e300, 0.0, 1e-300), -1);
  {
    const double top[3] = {2097151.5, 2097151.5, 2097151.5}, zero[3] = {0, 0, 0}, mixed[3] = {1.5, 2.5, 3.5}, bad[3] = {1.5, std::nan(""), 3.5};
    int64_t idx[3];
    SAME(mesh_decimate::vertex_key(top, zero, 1.0, idx), 0x7FFFFFFFFFFFFFFFull);
    SAME(mesh_decimate::vertex_key(mixed, zero, 1.0, idx), (3ull << 42) | (2ull << 21) | 1ull);
    SAME(mesh_decimate::vertex_key(bad, zero, 1.0, idx), MESH_DEC_DEAD_KEY);
  }
  // the duplicate rule and the parity of the six orders
  {
    const int32_t perm[6][3] = {{1, 2, 3}, {2, 3, 1}, {3, 1, 2}, {2, 1, 3}, {1, 3, 2}, {3, 2, 1}};
    for (int i = 0; i < 6; ++i) {
      int32_t s[3];
      int odd;
      SAME(mesh_decimate::sort_triple(perm[i][0], perm[i][1], perm[i][2], s, &odd), 1);
      REQUIRE(s[0] == 1 && s[1] == 2 && s[2] == 3 && odd == (i >= 3));
    }
    int32_t s[3];
    int odd;
    SAME(mesh_decimate::sort_triple(4, 4, 5, s, &odd), 0); SAME(mesh_decimate::sort_triple(5, 4, 4, s, &odd), 0); SAME(mesh_decimate::sort_triple(4, 5, 4, s, &odd), 0);
    SAME(mesh_decimate::duplicate_pick(2, 0, 7, -1), 7); SAME(mesh_decimate::duplicate_pick(2, 1, 7, 3), 7); SAME(mesh_decimate::duplicate_pick(1, 2, 7, 3), 3);
    SAME(mesh_decimate::duplicate_pick(1, 1, 7, 3), -1); SAME(mesh_decimate::duplicate_pick(0, 1, -1, 3), 3);
  }
  // layouts and scans around every seam: the block (256), the chunk (262,144) and one past
  const int64_t seam[] = {0, 1, 255, 256, 257, 1023, 1025, 262143, 262144, 262145, 600000};
  for (int64_t nv : seam)
    for (int64_t nt : seam) {
      for (int64_t sort_bytes : {(int64_t)0, (int64_t)1, (int64_t)1234567}) check_layout(nv, nt, sort_bytes);
    }
  for (int64_t nt : seam) check_scan(nt);
  check_layout(bigv, bigt, (int64_t)1 << 33);
  REQUIRE(dec_layout(bigv, bigt, 0).bytes > bigv * 28 + bigt * 60);
  std::printf("ok %d\n", checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "rule")) return run_rule(argv[2]);
  if (argc == 2 && !std::strcmp(argv[1], "plan")) return run_plan();
  std::fprintf(stderr, "usage: mesh_decimate_check rule FILE | plan\n");
  return 2;
}
