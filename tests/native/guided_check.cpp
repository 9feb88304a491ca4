// Host build of the guided-matching rule and plan (sfm_amd/csrc/guided_rule.h, guided_plan.h) for tests/test_guided_reference.py.
//   guided_check gate IN OUT   IN: int64 n, then n records of { double F[9]; double thr; float x1, y1, x2, y2 }
//                              OUT: n bytes, the gate of every record - once through the one-call form and once through
//                              the per-point halves, which must agree
//   guided_check plan SEED     segment tables, degenerate ones first (no pair, empty sides, one keypoint, no output row),
//                              through the checks, the table, the layout and the segment search; prints "ok <cases>"
// Build with -ffp-contract=off (the header's pragma is clang's).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "guided_plan.h"
#include "guided_rule.h"

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

struct Record { double F[9]; double thr; float x1, y1, x2, y2; };

static int run_gate(const char* in, const char* out) {
  std::FILE* fi = std::fopen(in, "rb");
  REQUIRE(fi);
  int64_t n = 0;
  REQUIRE(std::fread(&n, 8, 1, fi) == 1 && n >= 0);
  std::vector<Record> rec((size_t)n);
  REQUIRE(n == 0 || std::fread(rec.data(), sizeof(Record), (size_t)n, fi) == (size_t)n);
  std::fclose(fi);
  std::vector<unsigned char> res((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const Record& r = rec[(size_t)i];
    const bool g = guided::gate(r.F, r.x1, r.y1, r.x2, r.y2, r.thr);
    const guided::Side1 p = guided::side1(r.F, r.x1, r.y1);
    const guided::Side2 q = guided::side2(r.F, r.x2, r.y2);
    REQUIRE(g == guided::gate(p.a, p.b, p.c, p.den, q.x, q.y, q.den, r.thr * r.thr));
    res[(size_t)i] = g ? 1 : 0;
  }
  std::FILE* fo = std::fopen(out, "wb");
  REQUIRE(fo);
  REQUIRE(n == 0 || std::fwrite(res.data(), 1, (size_t)n, fo) == (size_t)n);
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

// one table of image sizes and pairs through everything the host does with it
static void check_table(const std::vector<int64_t>& sizes, const std::vector<std::pair<int, int>>& pairs) {
  std::vector<int64_t> ptr(sizes.size() + 1, 0);
  for (size_t i = 0; i < sizes.size(); ++i) ptr[i + 1] = ptr[i] + sizes[i];
  const int64_t n_rows = ptr.back(), n_seg = (int64_t)pairs.size();
  std::vector<int64_t> qb, qe, tb, te;
  for (auto& p : pairs) { qb.push_back(ptr[p.first]); qe.push_back(ptr[p.first + 1]); tb.push_back(ptr[p.second]); te.push_back(ptr[p.second + 1]); }
  const int64_t* a = n_seg ? qb.data() : nullptr; const int64_t* b = n_seg ? qe.data() : nullptr;
  const int64_t* c = n_seg ? tb.data() : nullptr; const int64_t* d = n_seg ? te.data() : nullptr;
  REQUIRE(guided_check_segments(n_seg, a, b, c, d, n_rows) == 0);
  const GuidedPlan p = guided_plan(n_seg, a, b, c, d);
  REQUIRE((int64_t)p.segs.size() == n_seg + 1);
  int64_t n_out = 0, n_rev = 0, tiles = 0, rtiles = 0;
  for (int64_t s = 0; s < n_seg; ++s) {
    const GuidedSeg& r = p.segs[(size_t)s];
    REQUIRE(r.out_first == n_out && r.rev_first == n_rev && r.tile_first == tiles && r.rev_tile_first == rtiles);
    const int64_t nq = r.q_end - r.q_beg, nt = r.t_end - r.t_beg;
    REQUIRE(nq >= 0 && nt >= 0);
    // every output row, forward tile and reverse tile finds its segment
    for (int64_t o = 0; o < nq; o += (nq > 64 ? nq / 7 + 1 : 1)) REQUIRE(guided_find(p.segs.data(), (int)n_seg, n_out + o, GUIDED_BY_OUT) == s);
    if (nq > 0) REQUIRE(guided_find(p.segs.data(), (int)n_seg, n_out + nq - 1, GUIDED_BY_OUT) == s);
    for (int64_t t = 0; t < guided_tiles(nq); ++t) {
      REQUIRE(guided_find(p.segs.data(), (int)n_seg, tiles + t, GUIDED_BY_TILE) == s);
      REQUIRE(r.q_beg + t * GUIDED_QT < r.q_end);           // no workgroup without a query
    }
    for (int64_t t = 0; t < guided_tiles(nt); ++t) REQUIRE(guided_find(p.segs.data(), (int)n_seg, rtiles + t, GUIDED_BY_REV_TILE) == s);
    n_out += nq; n_rev += nt; tiles += guided_tiles(nq); rtiles += guided_tiles(nt);
  }
  REQUIRE(p.n_out == n_out && p.n_rev == n_rev && p.n_tiles == tiles && p.n_rev_tiles == rtiles);
  REQUIRE(p.segs[(size_t)n_seg].out_first == n_out);
  const GuidedLayout L = guided_layout(n_seg, n_out, n_rev);
  // the arrays follow each other without overlap, 256-byte aligned, inside the reported size
  const int64_t off[] = {L.segs, L.idx1, L.d1, L.d2, L.ncand, L.rev, L.keep, L.blk_cnt, L.blk_off, L.bytes};
  const int64_t len[] = {(n_seg + 1) * (int64_t)sizeof(GuidedSeg), n_out * 4, n_out * 4, n_out * 4, n_out * 4, n_rev * 4, n_out,
                         (guided_blocks(n_out) + 1) * 4, (guided_blocks(n_out) + 1) * 4};
  for (int k = 0; k < 9; ++k) { REQUIRE(off[k] % 256 == 0); REQUIRE(off[k] + len[k] <= off[k + 1]); }
  // a table image of the layout can be written end to end
  std::vector<unsigned char> ws((size_t)L.bytes);
  std::memcpy(ws.data() + L.segs, p.segs.data(), p.segs.size() * sizeof(GuidedSeg));
  REQUIRE(n_out >> 8 <= guided_blocks(n_out));             // the block a segment's first row falls in has a blk_off entry
}

static int run_plan(uint64_t seed) {
  rng_state = seed;
  int cases = 0;
  // degenerate tables
  check_table({}, {}); ++cases;                                                   // no image, no pair
  check_table({5, 7}, {}); ++cases;                                               // a zero-pair batch
  check_table({0, 0}, {{0, 1}, {1, 0}}); ++cases;                                 // both sides empty: n_out = 0
  check_table({0, 9}, {{0, 1}}); ++cases;                                         // no query: n_out = 0 with train rows
  check_table({9, 0}, {{0, 1}}); ++cases;                                         // no train row
  check_table({1, 1}, {{0, 1}, {1, 0}}); ++cases;                                 // one keypoint a side
  check_table({3, 0, 1, 0, 40}, {{1, 0}, {0, 1}, {0, 2}, {3, 4}, {4, 3}, {4, 0}, {1, 3}}); ++cases;   // empties between live pairs
  for (int64_t n : {GUIDED_QT - 1, GUIDED_QT, GUIDED_QT + 1, GUIDED_CHUNK - 1, GUIDED_CHUNK, GUIDED_CHUNK + 1, 255, 256, 257}) {
    check_table({n, 2}, {{0, 1}, {1, 0}}); ++cases;
  }
  // bad tables are refused
  {
    const int64_t qb[] = {0}, qe[] = {4}, tb[] = {4}, te[] = {9};
    REQUIRE(guided_check_segments(1, qb, qe, tb, te, 9) == 0);
    REQUIRE(guided_check_segments(1, qb, qe, tb, te, 8) != 0);
    REQUIRE(guided_check_segments(-1, qb, qe, tb, te, 9) != 0);
    REQUIRE(guided_check_segments(1, nullptr, qe, tb, te, 9) != 0);
    REQUIRE(guided_check_segments(1, qe, qb, tb, te, 9) != 0);
    REQUIRE(guided_check_segments(1, qb, qe, te, tb, 9) != 0);
    REQUIRE(guided_check_segments(0, nullptr, nullptr, nullptr, nullptr, 0) == 0);
    REQUIRE(guided_check_segments(0, nullptr, nullptr, nullptr, nullptr, -1) != 0);
    cases += 8;
  }
  for (int rep = 0; rep < 200; ++rep) {
    const int n_img = 1 + (int)(rnd() % 6);
    std::vector<int64_t> sizes;
    for (int i = 0; i < n_img; ++i) { const uint64_t k = rnd() % 8; sizes.push_back(k < 2 ? 0 : (k == 2 ? 1 : (int64_t)(rnd() % 700))); }
    std::vector<std::pair<int, int>> pairs;
    const int n_pairs = (int)(rnd() % 9);
    for (int k = 0; k < n_pairs; ++k) pairs.push_back({(int)(rnd() % n_img), (int)(rnd() % n_img)});
    check_table(sizes, pairs); ++cases;
  }
  std::printf("ok %d\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "gate")) return run_gate(argv[2], argv[3]);
  if (argc == 3 && !std::strcmp(argv[1], "plan")) return run_plan(std::strtoull(argv[2], nullptr, 10));
  std::fprintf(stderr, "usage: guided_check gate IN OUT | guided_check plan SEED\n");
  return 2;
}
