// Host build of the selection rule and the launch plan of mesh cleaning (sfm_amd/csrc/mesh_clean_rule.h, mesh_clean_plan.h)
// for tests/test_mesh_clean_reference.py.
//   mesh_clean_check cut SEED   mesh_clean::select against a stable sort on random sizes with many ties: sizes from a few
//                               values, from the full 31 bits, all equal, with every min_triangles / keep_largest around the
//                               candidates' number; the radix step on hand-made histograms; prints "ok <cases>"
//   mesh_clean_check plan       the argument checks branch by branch; the two workspace layouts for sizes around every
//                               block and chunk seam - aligned, ascending, disjoint, within bytes; the packed block counts
//                               through the two-level scan as the kernels walk it, the bases against running sums; the
//                               gather's unit and grid; prints "ok <checks>"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "mesh_clean_plan.h"
#include "mesh_clean_rule.h"
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

// the rule by a stable sort: the candidates, largest first, equal sizes in component order, the first k of them
static std::vector<uint8_t> select_by_sort(const std::vector<int32_t>& sizes, int64_t min_triangles, int64_t k) {
  std::vector<int64_t> cand;
  for (size_t c = 0; c < sizes.size(); ++c)
    if ((int64_t)sizes[c] >= min_triangles) cand.push_back((int64_t)c);
  if (k > 0 && (int64_t)cand.size() > k) {
    std::stable_sort(cand.begin(), cand.end(), [&](int64_t a, int64_t b) { return sizes[(size_t)a] > sizes[(size_t)b]; });
    cand.resize((size_t)k);
  }
  std::vector<uint8_t> keep(sizes.size(), 0);
  for (int64_t c : cand) keep[(size_t)c] = 1;
  return keep;
}

static int check_select(const std::vector<int32_t>& sizes, int64_t min_triangles, int64_t k) {
  std::vector<uint8_t> got(sizes.size() + 1, 7);
  const int64_t kept = mesh_clean::select(sizes.data(), (int64_t)sizes.size(), min_triangles, k, got.data());
  const std::vector<uint8_t> want = select_by_sort(sizes, min_triangles, k);
  REQUIRE(got[sizes.size()] == 7);
  REQUIRE(std::equal(want.begin(), want.end(), got.begin()));
  REQUIRE(kept == std::accumulate(want.begin(), want.end(), (int64_t)0));
  return 1;
}

static int run_cut(uint64_t seed) {
  rng_state = seed;
  int cases = 0;
  // the radix step: the bin of the k-th largest and what is left for it
  {
    int32_t hist[MESH_CLEAN_RADIX_BINS] = {0};
    hist[200] = 3; hist[17] = 4; hist[0] = 2;
    const int64_t left[] = {1, 3, 4, 7, 8, 9}, bin[] = {200, 200, 17, 17, 0, 0}, after[] = {1, 3, 1, 4, 1, 2};
    for (int i = 0; i < 6; ++i) {
      mesh_clean::Cut cut{0u, left[i]};
      mesh_clean::radix_step(hist, 3, &cut);
      REQUIRE((int64_t)cut.prefix == bin[i] && cut.left == after[i]);
      mesh_clean::Cut top{0u, left[i]};
      mesh_clean::radix_step(hist, 0, &top);
      REQUIRE(top.prefix == (uint32_t)bin[i] << 24 && top.left == after[i]);
      ++cases;
    }
    REQUIRE(mesh_clean::radix_match(0x12345678u, 0x12340000u, 2) && !mesh_clean::radix_match(0x12355678u, 0x12340000u, 2));
    REQUIRE(mesh_clean::radix_match(0xFFFFFFFFu, 0u, 0) && mesh_clean::radix_bin(0x12345678u, 0) == 0x12 && mesh_clean::radix_bin(0x12345678u, 3) == 0x78);
  }
  for (int round = 0; round < 60; ++round) {
    const int64_t n = round < 4 ? round : (int64_t)(rnd() % (round < 40 ? 600 : 5000));
    std::vector<int32_t> sizes((size_t)n);
    const int kind = round % 5;
    for (auto& s : sizes) {
      if (kind == 0) s = (int32_t)(rnd() % 4);                                  // {0, 1, 2, 3}: almost only ties
      else if (kind == 1) s = (int32_t)(rnd() & 0x7FFFFFFFull);                // every byte of the radix in use
      else if (kind == 2) s = 5;                                               // all equal
      else if (kind == 3) s = (int32_t)((rnd() % 3) << (8 * (rnd() % 4)));     // ties that differ in one byte only
      else s = (int32_t)(rnd() % 300);
    }
    if (kind == 1 && n > 2) { sizes[0] = 0x7FFFFFFF; sizes[(size_t)n - 1] = 0x7FFFFFFF; sizes[(size_t)n / 2] = 0; }
    for (int64_t min_triangles : {(int64_t)0, (int64_t)1, (int64_t)2, (int64_t)4, (int64_t)6, (int64_t)0x7FFFFFFF}) {
      int64_t n_cand = 0;
      for (int32_t s : sizes) n_cand += s >= min_triangles;
      for (int64_t k : {(int64_t)0, (int64_t)1, (int64_t)2, n_cand / 2, n_cand - 1, n_cand, n_cand + 1, (int64_t)0x7FFFFFFF})
        if (k >= 0) cases += check_select(sizes, min_triangles, k);
    }
  }
  // the cases of the GPU test: 300 components with sizes from {1, 2, 3} plus one of 50
  std::vector<int32_t> sizes(301);
  for (auto& s : sizes) s = 1 + (int32_t)(rnd() % 3);
  sizes[137] = 50;
  for (int64_t k = 0; k <= 303; ++k) cases += check_select(sizes, 1, k) + check_select(sizes, 2, k);
  cases += check_select(sizes, 51, 0);
  std::printf("ok %d\n", cases);
  return 0;
}

static int checks = 0;
#define SAME(a, b) do { REQUIRE((a) == (b)); ++checks; } while (0)

static void check_layouts(int64_t nv, int64_t nt) {
  const CcLayout C = cc_layout(nv);
  const int64_t nbv = clean_blocks(nv);
  REQUIRE(nbv * CLEAN_BLOCK >= nv && (nbv == 0 || (nbv - 1) * CLEAN_BLOCK < nv));
  const int64_t c_off[] = {C.parent, C.number, C.blk, C.chunk_base, C.bytes};
  const int64_t c_len[] = {nv * 4, nv * 4, nbv * 4, scan_chunks(nbv) * 8};
  for (int i = 0; i < 4; ++i) {
    REQUIRE(c_off[i] % 256 == 0 && c_off[i] + c_len[i] <= c_off[i + 1]);
    ++checks;
  }
  REQUIRE(C.parent == 0 && C.bytes >= 256);
  const CleanLayout L = clean_layout(nv, nt);
  const int64_t nb = clean_scan_blocks(nv, nt);
  REQUIRE(nb == clean_blocks(nv > nt ? nv : nt) && nb >= clean_blocks(nv) && nb >= clean_blocks(nt));
  const int64_t l_off[] = {L.sel, L.new_index, L.blk, L.chunk_base, L.bytes};
  const int64_t l_len[] = {CLEAN_SEL_WORDS * 8, nv * 4, nb * 8, scan_chunks(nb) * 16};
  for (int i = 0; i < 4; ++i) {
    REQUIRE(l_off[i] % 256 == 0 && l_off[i] + l_len[i] <= l_off[i + 1]);
    ++checks;
  }
}

// kept vertices and triangles per block, packed, through the two-level scan as k_clean_scan_chunks / k_clean_scan_top walk it
static void check_scan(int64_t nv, int64_t nt) {
  const int64_t nb = clean_scan_blocks(nv, nt);
  std::vector<uint64_t> blk((size_t)nb), counts;
  for (int64_t b = 0; b < nb; ++b) {
    const int64_t in_v = std::min<int64_t>(std::max<int64_t>(nv - b * CLEAN_BLOCK, 0), CLEAN_BLOCK);
    const int64_t in_t = std::min<int64_t>(std::max<int64_t>(nt - b * CLEAN_BLOCK, 0), CLEAN_BLOCK);
    const uint32_t v = (b % 3 == 0) ? (uint32_t)in_v : (uint32_t)(rnd() % (uint64_t)(in_v + 1));
    const uint32_t t = (b % 5 == 0) ? (uint32_t)in_t : (uint32_t)(rnd() % (uint64_t)(in_t + 1));
    blk[(size_t)b] = clean_count_pack(v, t);
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
    REQUIRE(clean_vertex_base(chunk_base.data(), blk.data(), b) == lo && clean_triangle_base(chunk_base.data(), blk.data(), b) == hi);
    lo += (int64_t)(counts[(size_t)b] & 0xFFFFFFFFull);
    hi += (int64_t)(counts[(size_t)b] >> 32);
  }
  REQUIRE(totals[0] == lo && totals[1] == hi && lo <= nv && hi <= nt);
  ++checks;
}

static int run_plan() {
  rng_state = 11;
  const int64_t big = CLEAN_MAX_COUNT;
  int x = 0;
  const void* p = &x;
  // counts
  SAME(clean_check_counts(0, 0), 0); SAME(clean_check_counts(big, big), 0);
  SAME(clean_check_counts(-1, 0), 1); SAME(clean_check_counts(0, -1), 1); SAME(clean_check_counts(big + 1, 0), 1); SAME(clean_check_counts(0, big + 1), 1);
  SAME(clean_check_workspace(nullptr, 100, 10), 8); SAME(clean_check_workspace(p, 9, 10), 8); SAME(clean_check_workspace(p, 10, 10), 0);
  // sfm_mesh_components
  SAME(cc_check(5, 2, p, p, p, p, p, p, p), 0);
  SAME(cc_check(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, p), 0);
  SAME(cc_check(5, 0, nullptr, p, nullptr, p, p, p, p), 0);
  SAME(cc_check(0, 2, p, nullptr, p, nullptr, nullptr, nullptr, p), 0);
  SAME(cc_check(-1, 2, p, p, p, p, p, p, p), 1); SAME(cc_check(5, big + 1, p, p, p, p, p, p, p), 1);
  SAME(cc_check(5, 2, p, p, p, p, p, p, nullptr), 4);
  SAME(cc_check(5, 2, nullptr, p, p, p, p, p, p), 4); SAME(cc_check(5, 2, p, p, nullptr, p, p, p, p), 4);
  SAME(cc_check(5, 2, p, nullptr, p, p, p, p, p), 4); SAME(cc_check(5, 2, p, p, p, nullptr, p, p, p), 4);
  SAME(cc_check(5, 2, p, p, p, p, nullptr, p, p), 4); SAME(cc_check(5, 2, p, p, p, p, p, nullptr, p), 4);
  // sfm_mesh_clean_mark
  SAME(clean_check_mark(5, 2, 3, 1, 0, p, p, p, p, p), 0);
  SAME(clean_check_mark(0, 0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, p), 0);
  SAME(clean_check_mark(5, 2, 5, big, big, p, p, p, p, p), 0);
  SAME(clean_check_mark(-1, 2, 0, 1, 0, p, p, p, p, p), 1); SAME(clean_check_mark(5, -2, 3, 1, 0, p, p, p, p, p), 1);
  SAME(clean_check_mark(5, 2, -1, 1, 0, p, p, p, p, p), 2); SAME(clean_check_mark(5, 2, 6, 1, 0, p, p, p, p, p), 2);
  SAME(clean_check_mark(5, 2, 3, -1, 0, p, p, p, p, p), 3); SAME(clean_check_mark(5, 2, 3, 1, -1, p, p, p, p, p), 3);
  SAME(clean_check_mark(5, 2, 3, 1, 0, p, p, p, p, nullptr), 4); SAME(clean_check_mark(5, 2, 3, 1, 0, nullptr, p, p, p, p), 4);
  SAME(clean_check_mark(5, 2, 3, 1, 0, p, nullptr, p, p, p), 4); SAME(clean_check_mark(5, 2, 3, 1, 0, p, p, nullptr, p, p), 4);
  SAME(clean_check_mark(5, 2, 3, 1, 0, p, p, p, nullptr, p), 4);
  // sfm_mesh_clean_emit
  SAME(clean_check_emit_counts(5, 2, 3, 5, 2), 0); SAME(clean_check_emit_counts(5, 2, 3, 0, 0), 0); SAME(clean_check_emit_counts(0, 0, 0, big, big), 0);
  SAME(clean_check_emit_counts(big + 1, 2, 3, 5, 2), 1); SAME(clean_check_emit_counts(5, 2, 6, 5, 2), 2);
  SAME(clean_check_emit_counts(5, 2, 3, -1, 2), 5); SAME(clean_check_emit_counts(5, 2, 3, 5, -1), 5);
  SAME(clean_check_emit_counts(5, 2, 3, big + 1, 2), 5); SAME(clean_check_emit_counts(5, 2, 3, 5, big + 1), 5);
  SAME(clean_check_emit_pointers(5, 2, 3, 5, 2, p, p, p, p, p, p, p, p, p, p, p), 0);
  SAME(clean_check_emit_pointers(5, 2, 3, 0, 2, p, p, p, p, nullptr, nullptr, nullptr, p, p, nullptr, nullptr), 0);
  SAME(clean_check_emit_pointers(5, 2, 3, 5, 0, p, p, p, p, p, p, p, nullptr, nullptr, p, p), 0);
  for (int hole = 0; hole < 11; ++hole) {
    const void* a[11];
    for (int i = 0; i < 11; ++i) a[i] = i == hole ? nullptr : p;
    SAME(clean_check_emit_pointers(5, 2, 3, 5, 2, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10]), 4);
  }
  // sfm_mesh_gather_rows
  SAME(clean_check_gather(1, 0, nullptr, nullptr, nullptr), 0); SAME(clean_check_gather(24, 7, p, p, p), 0);
  SAME(clean_check_gather(0, 7, p, p, p), 6); SAME(clean_check_gather(-3, 7, p, p, p), 6);
  SAME(clean_check_gather(4, -1, p, p, p), 7); SAME(clean_check_gather(4, big + 1, p, p, p), 7);
  SAME(clean_check_gather(4, 7, nullptr, p, p), 4); SAME(clean_check_gather(4, 7, p, nullptr, p), 4); SAME(clean_check_gather(4, 7, p, p, nullptr), 4);
  for (int why = 1; why <= 8; ++why) REQUIRE(CLEAN_WHY[why][0] != 0);
  SAME(clean_gather_unit(1, 0, 0), 1); SAME(clean_gather_unit(3, 0, 0), 1); SAME(clean_gather_unit(4, 256, 512), 4); SAME(clean_gather_unit(12, 256, 512), 4);
  SAME(clean_gather_unit(24, 256, 512), 8); SAME(clean_gather_unit(32, 256, 512), 16); SAME(clean_gather_unit(32, 264, 512), 8);
  SAME(clean_gather_unit(32, 256, 516), 4); SAME(clean_gather_unit(32, 257, 512), 1); SAME(clean_gather_unit(2, 256, 512), 1);
  SAME(clean_gather_blocks(0), 0); SAME(clean_gather_blocks(1), 1); SAME(clean_gather_blocks(257), 2);
  SAME(clean_gather_blocks((int64_t)CLEAN_GATHER_MAX_BLOCKS * CLEAN_BLOCK + 1), (int64_t)CLEAN_GATHER_MAX_BLOCKS);
  SAME(clean_gather_blocks(big * 24), (int64_t)CLEAN_GATHER_MAX_BLOCKS);
  REQUIRE(cc_budget(big) > big && cc_budget(0) > 0);
  // layouts and scans around every seam: the block (256), the chunk (1,024 blocks = 262,144) and one past
  const int64_t seam[] = {0, 1, 255, 256, 257, 1023, 1024, 1025, 262143, 262144, 262145, 524289};
  for (int64_t nv : seam)
    for (int64_t nt : seam) {
      check_layouts(nv, nt);
      if (nv + nt <= 262145 + 1025 || nv == nt) check_scan(nv, nt);
    }
  check_layouts(big, big);
  REQUIRE(clean_layout(big, big).bytes > big * 4 && cc_layout(big).bytes > big * 8);
  std::printf("ok %d\n", checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "cut")) return run_cut(std::strtoull(argv[2], nullptr, 10));
  if (argc == 2 && !std::strcmp(argv[1], "plan")) return run_plan();
  std::fprintf(stderr, "usage: mesh_clean_check cut SEED | plan\n");
  return 2;
}
