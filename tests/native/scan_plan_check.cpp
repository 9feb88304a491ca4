// Host build of the scan plan (sfm_amd/csrc/scan_plan.h) for tests/test_scan_plan_reference.py.
//   scan_plan_check SEED     for the block counts 0, 1, 255, 256, 257, 1,023, 1,024, 1,025, 256 x 1,024 - 1, 256 x 1,024,
//                            256 x 1,024 + 1 and random ones, with random counts and with the largest counts:
//                            - the runs scan_run gives 256 (and 1,024) threads tile [0, n), beg <= end <= n;
//                            - the one-workgroup scan as scan_counts walks it, out of place and in place, against a
//                              running sum;
//                            - level one and level two of the chunk scan as the kernels walk them, for one total per
//                              chunk (stride 1, uint32 counts) and two packed halves (stride 2, uint64 counts), the bases
//                              from scan_base against running sums;
//                            prints "ok <cases>"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scan_plan.h"
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

static void check_runs(int64_t n, int n_threads) {
  const int64_t per = (n + n_threads - 1) / n_threads;
  int64_t next = 0;
  for (int tid = 0; tid < n_threads; ++tid) {
    int64_t beg = -1, end = -1;
    scan_run(n, tid, n_threads, &beg, &end);
    REQUIRE(0 <= beg && beg <= end && end <= n && end - beg <= per);
    REQUIRE(beg == next);                                        // no gap, no overlap
    next = end;
  }
  REQUIRE(next == n);
}

static void check_counts(int64_t n, int full) {
  const int most = 256;
  std::vector<int> in((size_t)n), out((size_t)n + 1, -7), same;
  for (auto& c : in) c = full ? most : (int)(rnd() % (most + 1));
  same = in;
  const int64_t total = scan_replay::counts(256, n, in.data(), out.data());
  const int64_t total_in_place = scan_replay::counts(256, n, same.data(), same.data());
  int64_t run = 0;
  for (int64_t i = 0; i < n; ++i) {
    REQUIRE(out[(size_t)i] == run && same[(size_t)i] == run);
    run += in[(size_t)i];
  }
  REQUIRE(total == run && total_in_place == run);
  REQUIRE(out[(size_t)n] == -7);                                 // entry n is the caller's, where it has one
}

// one total per chunk: uint32 counts, stride 1
static void check_chunks_one(int64_t nb, int full) {
  const uint32_t most = 256;
  std::vector<uint32_t> blk((size_t)nb), counts;
  for (auto& c : blk) c = full ? most : (uint32_t)(rnd() % (most + 1));
  counts = blk;
  std::vector<int64_t> chunk_base;
  scan_replay::chunk_counts(blk, chunk_base);
  REQUIRE((int64_t)chunk_base.size() == scan_chunks(nb));
  const int64_t total = scan_replay::chunk_totals(chunk_base.data(), scan_chunks(nb), 1);
  int64_t run = 0;
  for (int64_t b = 0; b < nb; ++b) {
    REQUIRE(scan_base(chunk_base.data(), 1, 0, b, (int64_t)blk[(size_t)b]) == run);
    run += counts[(size_t)b];
  }
  REQUIRE(total == run);
}

// two packed halves: uint64 counts, stride 2
static void check_chunks_two(int64_t nb, int full) {
  const uint32_t most_lo = 256 * 7, most_hi = 256 * 12;
  std::vector<uint64_t> blk((size_t)nb), counts;
  for (auto& c : blk)
    c = full ? ((uint64_t)most_lo | ((uint64_t)most_hi << 32)) : ((rnd() % (most_lo + 1)) | ((rnd() % (most_hi + 1)) << 32));
  counts = blk;
  std::vector<int64_t> packed, chunk_base;
  scan_replay::chunk_counts(blk, packed);
  const int64_t n_chunks = scan_chunks(nb);
  chunk_base.assign((size_t)n_chunks * 2, 0);
  for (int64_t c = 0; c < n_chunks; ++c) {
    chunk_base[(size_t)(2 * c)] = packed[(size_t)c] & 0xFFFFFFFFll;
    chunk_base[(size_t)(2 * c + 1)] = packed[(size_t)c] >> 32;
  }
  int64_t totals[2] = {0, 0}, lo = 0, hi = 0;
  for (int half = 0; half < 2; ++half) totals[half] = scan_replay::chunk_totals(chunk_base.data() + half, n_chunks, 2);
  for (int64_t b = 0; b < nb; ++b) {
    REQUIRE(scan_base(chunk_base.data(), 2, 0, b, (int64_t)(blk[(size_t)b] & 0xFFFFFFFFull)) == lo);
    REQUIRE(scan_base(chunk_base.data(), 2, 1, b, (int64_t)(blk[(size_t)b] >> 32)) == hi);
    lo += (int64_t)(counts[(size_t)b] & 0xFFFFFFFFull);
    hi += (int64_t)(counts[(size_t)b] >> 32);
  }
  REQUIRE(totals[0] == lo && totals[1] == hi);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: scan_plan_check SEED\n");
    return 2;
  }
  rng_state = std::strtoull(argv[1], nullptr, 10);
  static_assert(SCAN_ITEMS == 4 && SCAN_CHUNK == SCAN_THREADS * SCAN_ITEMS, "chunk = threads x items");
  std::vector<int64_t> sizes = {0, 1, 255, 256, 257, 1023, 1024, 1025, 256 * 1024 - 1, 256 * 1024, 256 * 1024 + 1};
  for (int k = 0; k < 12; ++k) sizes.push_back((int64_t)(rnd() % (k < 8 ? 5000 : 300000)));
  int cases = 0;
  for (int64_t n : sizes) {
    check_runs(n, 256);
    check_runs(n, 1024);
    for (int full = 0; full < 2; ++full) {
      check_counts(n, full);
      check_chunks_one(n, full);
      check_chunks_two(n, full);
      ++cases;
    }
  }
  // the largest n a stage passes: the products stay in 64 bits
  check_runs(0x7FFFFFFFLL, 256);
  std::printf("ok %d\n", cases);
  return 0;
}
