// Host build of the rule and the launch plan of the edge table and of hole filling (sfm_amd/csrc/mesh_fill_rule.h,
// mesh_fill_plan.h) for tests/test_mesh_fill_reference.py.
//   mesh_fill_check walk SEED   mesh_fill::split on random closed walks of at most 64 edges that pass vertices several times
//                               (cycles hung into cycles), with random half-edge numbers: the sub-loops partition the walk,
//                               each is closed, has distinct vertices and at least 3 edges, is named by its smallest
//                               half-edge, and there are as many as cycles were hung in; against the same split done by
//                               cutting out the stretch that closes first; the hand cases; open walks leave the stack
//                               non-empty; mesh_fill::patch against sums over the listed members; the keys and the
//                               half-edge arithmetic; prints "ok <cases>"
//   mesh_fill_check patch FILE  FILE holds one loop: n, then n lines "h a x y z" in next order from the leader, the
//                               coordinates of vertex a as the 16 hex digits of their float64 bits; prints per sub-loop in
//                               ascending order of the names "name len cx cy cz nx ny nz", the bits in hex
//   mesh_fill_check plan        the argument checks branch by branch; the two workspace layouts around every block and chunk
//                               seam - aligned, ascending, disjoint, within bytes; the packed block counts through the
//                               two-level scan as the kernels walk it; prints "ok <checks>"
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "mesh_fill_plan.h"
#include "mesh_fill_rule.h"
#include "scan_replay.h"

#define REQUIRE(c) SCAN_REPLAY_REQUIRE(c)

static uint64_t rng_state;
static uint64_t rnd() {
  rng_state += 0x9E3779B97F4A7C15ull;
  uint64_t z = rng_state;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Split { std::vector<int32_t> name, len, succ; int ok; };

static Split run_split(const std::vector<int32_t>& a, const std::vector<int32_t>& b, const std::vector<int32_t>& h) {
  const int n = (int)a.size();
  Split s;
  std::vector<int32_t> stack((size_t)n + 1, 77);
  s.name.assign((size_t)n + 1, 77); s.len.assign((size_t)n + 1, 77); s.succ.assign((size_t)n + 1, 77);
  s.ok = mesh_fill::split(n, a.data(), b.data(), h.data(), stack.data(), s.name.data(), s.len.data(), s.succ.data());
  REQUIRE(stack[(size_t)n] == 77 && s.name[(size_t)n] == 77 && s.len[(size_t)n] == 77 && s.succ[(size_t)n] == 77);
  return s;
}

// the same without a stack: cut out, again and again, the stretch of what is left that closes first
static std::vector<std::vector<int>> split_by_cutting(const std::vector<int32_t>& a, const std::vector<int32_t>& b) {
  std::vector<int> rest(a.size());
  for (size_t i = 0; i < rest.size(); ++i) rest[i] = (int)i;
  std::vector<std::vector<int>> out;
  while (!rest.empty()) {
    bool cut = false;
    for (size_t j = 0; j < rest.size() && !cut; ++j)
      for (size_t i = 0; i <= j && !cut; ++i)
        if (a[(size_t)rest[i]] == b[(size_t)rest[j]]) {
          out.emplace_back(rest.begin() + (long)i, rest.begin() + (long)j + 1);
          rest.erase(rest.begin() + (long)i, rest.begin() + (long)j + 1);
          cut = true;
        }
    if (!cut) break;
  }
  return out;
}

static int check_walk(const std::vector<int32_t>& verts, int cycles, const std::vector<double>& xyz) {
  const int n = (int)verts.size();
  std::vector<int32_t> a((size_t)n), b((size_t)n), h((size_t)n);
  // distinct half-edge numbers, the smallest in front as the leader is
  std::set<int32_t> used;
  while ((int)used.size() < n) used.insert((int32_t)(rnd() % 100000));
  std::vector<int32_t> numbers(used.begin(), used.end());
  for (int i = n - 1; i > 1; --i) std::swap(numbers[(size_t)i], numbers[1 + (size_t)(rnd() % (uint64_t)i)]);
  for (int i = 0; i < n; ++i) { a[(size_t)i] = verts[(size_t)i]; b[(size_t)i] = verts[(size_t)((i + 1) % n)]; h[(size_t)i] = numbers[(size_t)i]; }
  const Split s = run_split(a, b, h);
  REQUIRE(s.ok == 1);
  const std::vector<std::vector<int>> want = split_by_cutting(a, b);
  REQUIRE((int)want.size() == cycles);
  std::vector<char> seen((size_t)n, 0);
  for (const std::vector<int>& sub : want) {
    const int m = (int)sub.size();
    REQUIRE(m >= 3);
    int32_t low = h[(size_t)sub[0]];
    std::set<int32_t> distinct;
    for (int e : sub) { low = std::min(low, h[(size_t)e]); distinct.insert(a[(size_t)e]); REQUIRE(!seen[(size_t)e]); seen[(size_t)e] = 1; }
    REQUIRE((int)distinct.size() == m);
    for (int j = 0; j < m; ++j) {
      const int e = sub[(size_t)j], f = sub[(size_t)((j + 1) % m)];
      REQUIRE(s.name[(size_t)e] == low && s.len[(size_t)e] == m && s.succ[(size_t)e] == f && b[(size_t)e] == a[(size_t)f]);
    }
    // the patch from the entry of the name: against sums over the members listed from there
    int at = 0;
    for (int j = 0; j < m; ++j) if (h[(size_t)sub[(size_t)j]] == low) at = j;
    double c[3], sum[3] = {0, 0, 0};
    float normal[3];
    mesh_fill::patch(m, sub[(size_t)at], s.succ.data(), a.data(), xyz.data(), c, normal);
    for (int j = 0; j < m; ++j)
      for (int x = 0; x < 3; ++x) {
        const double v = xyz[3 * (size_t)a[(size_t)sub[(size_t)((at + j) % m)]] + (size_t)x];
        sum[x] = j == 0 ? v : sum[x] + v;
      }
    for (int x = 0; x < 3; ++x) REQUIRE(c[x] == sum[x] / (double)m || (std::isnan(c[x]) && std::isnan(sum[x])));
    const double l2 = ((double)normal[0] * normal[0] + (double)normal[1] * normal[1]) + (double)normal[2] * normal[2];
    REQUIRE(l2 == 0.0 || (l2 > 0.999999 && l2 < 1.000001));
  }
  for (int i = 0; i < n; ++i) REQUIRE(seen[(size_t)i]);
  // an open walk: the last edge ends somewhere new
  if (n >= 2) {
    std::vector<int32_t> bo = b;
    bo[(size_t)n - 1] = 1000000;
    REQUIRE(run_split(a, bo, h).ok == 0);
  }
  return 1;
}

static int run_walk(uint64_t seed) {
  rng_state = seed;
  int cases = 0;
  for (int h = 0; h < 300; ++h) {
    const int g = mesh_fill::next_in_triangle(h);
    REQUIRE(g / 3 == h / 3 && g % 3 == (h % 3 + 1) % 3 && mesh_fill::next_in_triangle(mesh_fill::next_in_triangle(g)) == h);
    ++cases;
  }
  {
    int32_t a, b;
    mesh_fill::ends(5, 6, 7, 0, &a, &b); REQUIRE(a == 5 && b == 6);
    mesh_fill::ends(5, 6, 7, 1, &a, &b); REQUIRE(a == 6 && b == 7);
    mesh_fill::ends(5, 6, 7, 2, &a, &b); REQUIRE(a == 7 && b == 5);
    REQUIRE(mesh_fill::edge_key(5, 6, 7, 0, 8) == ((5ull << 32) | 6ull) && mesh_fill::edge_key(5, 6, 7, 2, 8) == ((5ull << 32) | 7ull));
    REQUIRE(mesh_fill::edge_key(6, 5, 7, 0, 8) == ((5ull << 32) | 6ull));
    REQUIRE(mesh_fill::edge_key(5, 5, 7, 0, 8) == MESH_FILL_DEAD_KEY && mesh_fill::edge_key(5, 5, 7, 1, 8) == ((5ull << 32) | 7ull));
    REQUIRE(mesh_fill::edge_key(5, 6, 8, 0, 8) == MESH_FILL_DEAD_KEY && mesh_fill::edge_key(-1, 6, 7, 1, 8) == MESH_FILL_DEAD_KEY);
    REQUIRE(mesh_fill::edge_key(0x7FFFFFFE, 0x7FFFFFFD, 0, 0, 0x7FFFFFFF) == ((0x7FFFFFFDull << 32) | 0x7FFFFFFEull));
    REQUIRE(mesh_fill::filled(3, 3) && !mesh_fill::filled(2, 64) && !mesh_fill::filled(17, 16) && mesh_fill::filled(64, 64) && !mesh_fill::filled(3, 1));
    cases += 5;
  }
  // hand cases: a triangle; two quads that touch in vertex 0; a figure of three triangles about one vertex
  {
    std::vector<double> xyz(3 * 16);
    for (double& v : xyz) v = (double)(rnd() % 1000) / 7.0;
    cases += check_walk({0, 1, 2}, 1, xyz);
    cases += check_walk({0, 1, 2, 3, 0, 4, 5, 6}, 2, xyz);
    cases += check_walk({0, 1, 2, 0, 3, 4, 0, 5, 6}, 3, xyz);
    cases += check_walk({1, 2, 0, 3, 4, 0, 5, 6, 0}, 3, xyz);
    cases += check_walk({0, 1, 2, 3, 4, 2, 5, 6}, 2, xyz);            // a cycle hung into the middle of another
  }
  for (int round = 0; round < 400; ++round) {
    // cycles of at least 3 edges, hung into the walk at a random place, 64 edges at the most
    const int budget = round % 7 == 0 ? 64 : 3 + (int)(rnd() % 62);
    std::vector<int32_t> walk;
    int32_t fresh = 0;
    int cycles = 0;
    while ((int)walk.size() + 3 <= budget) {
      const int room = budget - (int)walk.size();
      const int len = round % 7 == 0 && cycles == 0 && rnd() % 2 ? room : 3 + (int)(rnd() % (uint64_t)std::min(room - 2, 12));
      if (walk.empty()) {
        for (int i = 0; i < len; ++i) walk.push_back(fresh++);
      } else {
        const size_t at = (size_t)(rnd() % walk.size());
        std::vector<int32_t> hung{walk[at]};
        for (int i = 1; i < len; ++i) hung.push_back(fresh++);
        walk.insert(walk.begin() + (long)at, hung.begin(), hung.end());
      }
      ++cycles;
      if (rnd() % 3 == 0) break;
    }
    std::vector<double> xyz(3 * (size_t)fresh);
    for (double& v : xyz) v = ((double)(int64_t)(rnd() % 2000001) - 1000000.0) / 977.0;
    if (round % 11 == 0) xyz[(size_t)(rnd() % xyz.size())] = std::nan("");
    cases += check_walk(walk, cycles, xyz);
  }
  std::printf("ok %d\n", cases);
  return 0;
}

static int run_patch(const char* path) {
  std::FILE* f = std::fopen(path, "r");
  REQUIRE(f != nullptr);
  int n = 0;
  REQUIRE(std::fscanf(f, "%d", &n) == 1 && n >= 1 && n <= MESH_FILL_WAVE);
  std::vector<int32_t> a((size_t)n), b((size_t)n), h((size_t)n);
  std::map<int32_t, int32_t> local;
  std::vector<double> xyz;
  for (int i = 0; i < n; ++i) {
    int hh, aa;
    uint64_t bits[3];
    REQUIRE(std::fscanf(f, "%d %d %" SCNx64 " %" SCNx64 " %" SCNx64, &hh, &aa, &bits[0], &bits[1], &bits[2]) == 5);
    if (!local.count(aa)) {
      local[aa] = (int32_t)(xyz.size() / 3);
      for (int x = 0; x < 3; ++x) { double v; std::memcpy(&v, &bits[x], 8); xyz.push_back(v); }
    }
    h[(size_t)i] = hh; a[(size_t)i] = local[aa];
  }
  std::fclose(f);
  for (int i = 0; i < n; ++i) b[(size_t)i] = a[(size_t)((i + 1) % n)];
  const Split s = run_split(a, b, h);
  REQUIRE(s.ok == 1);
  std::map<int32_t, int> names;
  for (int i = 0; i < n; ++i) if (s.name[(size_t)i] == h[(size_t)i]) names[h[(size_t)i]] = i;
  for (const auto& kv : names) {
    double c[3];
    float normal[3];
    mesh_fill::patch(s.len[(size_t)kv.second], kv.second, s.succ.data(), a.data(), xyz.data(), c, normal);
    uint64_t cb[3];
    uint32_t nb[3];
    std::memcpy(cb, c, 24); std::memcpy(nb, normal, 12);
    std::printf("%d %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %08x %08x %08x\n", kv.first, s.len[(size_t)kv.second], cb[0], cb[1], cb[2], nb[0],
                nb[1], nb[2]);
  }
  return 0;
}

static int checks = 0;
#define SAME(a, b) do { REQUIRE((a) == (b)); ++checks; } while (0)

static void check_layouts(int64_t nt, int64_t sort_bytes) {
  const int64_t n = 3 * nt, nb = fill_blocks(n);
  REQUIRE(nb * FILL_BLOCK >= n && (nb == 0 || (nb - 1) * FILL_BLOCK < n));
  const EdgesLayout E = edges_layout(nt, sort_bytes);
  const int64_t e_off[] = {E.keys_in, E.keys_out, E.vals_in, E.vals_out, E.lead, E.blk, E.chunk_base, E.sort, E.bytes};
  const int64_t e_len[] = {n * 8, n * 8, n * 4, n * 4, n * 4, nb * 4, scan_chunks(nb) * 8, sort_bytes};
  for (int i = 0; i < 8; ++i) {
    REQUIRE(e_off[i] % 256 == 0 && e_off[i] + e_len[i] <= e_off[i + 1]);
    ++checks;
  }
  REQUIRE(E.keys_in == 0 && E.bytes >= 256);
  const FillLayout L = fill_layout(nt);
  const int64_t l_off[] = {L.sub_name, L.rank, L.blk, L.chunk_base, L.bytes};
  const int64_t l_len[] = {n * 4, n * 4, nb * 8, scan_chunks(nb) * 16};
  for (int i = 0; i < 4; ++i) {
    REQUIRE(l_off[i] % 256 == 0 && l_off[i] + l_len[i] <= l_off[i + 1]);
    ++checks;
  }
}

// names and fill triangles per block, packed, through the two-level scan as k_fill_scan_chunks / k_fill_scan_top walk it
static void check_scan(int64_t nt) {
  const int64_t n = 3 * nt, nb = fill_blocks(n);
  std::vector<uint64_t> blk((size_t)nb), counts;
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t in = std::min<int64_t>(std::max<int64_t>(n - b * FILL_BLOCK, 0), FILL_BLOCK);
    const uint32_t tris = (b % 3 == 0) ? (uint32_t)in : (uint32_t)(rnd() % (uint64_t)(in + 1));
    const uint32_t names = (uint32_t)(rnd() % (uint64_t)(tris / 3 + 1));
    blk[(size_t)b] = fill_count_pack(names, tris);
  }
  counts = blk;
  std::vector<int64_t> packed, chunk_base;
  scan_replay::chunk_counts(blk, packed);
  const int64_t n_chunks = scan_chunks(nb);
  chunk_base.assign((size_t)n_chunks * 2 + 1, 0);
  for (int64_t c = 0; c < n_chunks; ++c) {
    chunk_base[(size_t)(2 * c)] = packed[(size_t)c] & 0xFFFFFFFFll;
    chunk_base[(size_t)(2 * c + 1)] = packed[(size_t)c] >> 32;
  }
  int64_t totals[2], lo = 0, hi = 0;
  for (int half = 0; half < 2; ++half) totals[half] = scan_replay::chunk_totals(chunk_base.data() + half, n_chunks, 2);
  for (int64_t b = 0; b < nb; ++b) {
    REQUIRE(fill_name_base(chunk_base.data(), blk.data(), b) == lo && fill_triangle_base(chunk_base.data(), blk.data(), b) == hi);
    lo += (int64_t)(counts[(size_t)b] & 0xFFFFFFFFull);
    hi += (int64_t)(counts[(size_t)b] >> 32);
  }
  REQUIRE(totals[0] == lo && totals[1] == hi && hi <= n && lo <= hi);
  ++checks;
}

static int run_plan() {
  rng_state = 13;
  const int64_t bigv = FILL_MAX_VERTICES, bigt = FILL_MAX_TRIANGLES;
  int x = 0;
  const void* p = &x;
  REQUIRE(3 * bigt <= 0x7FFFFFFFLL && 3 * (bigt + 1) > 0x7FFFFFFFLL);
  SAME(fill_check_counts(0, 0), 0); SAME(fill_check_counts(bigv, bigt), 0);
  SAME(fill_check_counts(-1, 0), 1); SAME(fill_check_counts(0, -1), 1); SAME(fill_check_counts(bigv + 1, 0), 1); SAME(fill_check_counts(0, bigt + 1), 1);
  SAME(fill_check_workspace(nullptr, 100, 10), 6); SAME(fill_check_workspace(p, 9, 10), 6); SAME(fill_check_workspace(p, 10, 10), 0);
  // sfm_mesh_edges
  SAME(edges_check(5, 2, p, p, p, p, p, p, p, p), 0);
  SAME(edges_check(5, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, p), 0);
  SAME(edges_check(0, 2, p, p, p, p, p, p, p, p), 0);
  SAME(edges_check(-1, 2, p, p, p, p, p, p, p, p), 1); SAME(edges_check(5, bigt + 1, p, p, p, p, p, p, p, p), 1);
  for (int hole = 0; hole < 8; ++hole) {
    const void* a[8];
    for (int i = 0; i < 8; ++i) a[i] = i == hole ? nullptr : p;
    SAME(edges_check(5, 2, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]), 4);
  }
  // sfm_mesh_fill_mark
  SAME(fill_check_mark(5, 2, 1, 16, p, p, p, p, p), 0); SAME(fill_check_mark(5, 2, 2, 1, p, p, p, p, p), 0); SAME(fill_check_mark(5, 2, 0, 64, p, p, nullptr, p, p), 0);
  SAME(fill_check_mark(0, 0, 0, 16, nullptr, nullptr, nullptr, nullptr, p), 0);
  SAME(fill_check_mark(-1, 2, 1, 16, p, p, p, p, p), 1); SAME(fill_check_mark(5, bigt + 1, 1, 16, p, p, p, p, p), 1);
  SAME(fill_check_mark(5, 2, -1, 16, p, p, p, p, p), 2); SAME(fill_check_mark(5, 2, 3, 16, p, p, p, p, p), 2);
  SAME(fill_check_mark(5, 2, 1, 0, p, p, p, p, p), 3); SAME(fill_check_mark(5, 2, 1, 65, p, p, p, p, p), 3); SAME(fill_check_mark(5, 2, 1, -4, p, p, p, p, p), 3);
  for (int hole = 0; hole < 5; ++hole) {
    const void* a[5];
    for (int i = 0; i < 5; ++i) a[i] = i == hole ? nullptr : p;
    SAME(fill_check_mark(5, 2, 1, 16, a[0], a[1], a[2], a[3], a[4]), 4);
  }
  // sfm_mesh_fill_emit
  SAME(fill_check_emit_counts(5, 2, 1, 1, 3), 0); SAME(fill_check_emit_counts(5, 2, 1, 0, 0), 0); SAME(fill_check_emit_counts(0, 0, 0, bigv, bigv), 0);
  SAME(fill_check_emit_counts(bigv + 1, 2, 1, 1, 3), 1); SAME(fill_check_emit_counts(5, 2, 3, 1, 3), 2); SAME(fill_check_emit_counts(5, 2, -1, 1, 3), 2);
  SAME(fill_check_emit_counts(5, 2, 1, -1, 3), 5); SAME(fill_check_emit_counts(5, 2, 1, 1, -1), 5);
  SAME(fill_check_emit_counts(5, 2, 1, bigv + 1, 3), 5); SAME(fill_check_emit_counts(5, 2, 1, 1, bigv + 1), 5);
  SAME(fill_check_emit_pointers(5, 2, 1, 1, 3, p, p, p, p, p, p, p, p, p, p), 0);
  SAME(fill_check_emit_pointers(5, 2, 1, 0, 3, p, p, p, p, nullptr, nullptr, nullptr, nullptr, p, p), 0);
  SAME(fill_check_emit_pointers(5, 2, 1, 1, 0, p, p, p, p, p, p, p, p, nullptr, nullptr), 0);
  SAME(fill_check_emit_pointers(0, 2, 0, 1, 0, p, p, nullptr, p, nullptr, p, p, p, nullptr, nullptr), 0);
  for (int hole = 0; hole < 10; ++hole) {
    const void* a[10];
    for (int i = 0; i < 10; ++i) a[i] = i == hole ? nullptr : p;
    SAME(fill_check_emit_pointers(5, 2, 1, 1, 3, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]), 4);
  }
  for (int why = 1; why <= 6; ++why) REQUIRE(FILL_WHY[why][0] != 0);
  SAME(fill_loop_blocks(0), 0); SAME(fill_loop_blocks(1), 1); SAME(fill_loop_blocks(FILL_WAVES), 1); SAME(fill_loop_blocks(FILL_WAVES + 1), 2);
  REQUIRE(edges_budget(bigt) > bigt && edges_budget(0) > 0);
  // layouts and scans around every seam of 3 nt: the block (256), the chunk (262,144) and one past
  const int64_t seam[] = {0, 1, 85, 86, 341, 342, 87381, 87382, 87383, 174763, 200000};
  for (int64_t nt : seam) {
    for (int64_t sort_bytes : {(int64_t)0, (int64_t)1, (int64_t)4096, (int64_t)1234567}) check_layouts(nt, sort_bytes);
    check_scan(nt);
  }
  check_layouts(bigt, (int64_t)1 << 33);
  REQUIRE(fill_layout(bigt).bytes > bigt * 24 && edges_layout(bigt, 0).bytes > bigt * 84);
  std::printf("ok %d\n", checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "walk")) return run_walk(std::strtoull(argv[2], nullptr, 10));
  if (argc == 3 && !std::strcmp(argv[1], "patch")) return run_patch(argv[2]);
  if (argc == 2 && !std::strcmp(argv[1], "plan")) return run_plan();
  std::fprintf(stderr, "usage: mesh_fill_check walk SEED | patch FILE | plan\n");
  return 2;
}
