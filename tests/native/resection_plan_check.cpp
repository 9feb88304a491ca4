// Host-only check of sfm_amd/csrc/resection_plan.h, built with -fsanitize=address,undefined by
// tests/test_incremental_reference.py.
//   layout   the two arrays of the workspace are 256-byte aligned, lie inside `bytes`, do not overlap and hold what the
//            kernels index: one 64-bit word per wavefront of every workgroup, one int per workgroup plus the total.  For
//            the sizes that fit, a buffer of `bytes` is written at the first and the last entry of both arrays.
//   sizes    resect_check_sizes accepts 2^31 - 1 nodes and rejects 2^31, a negative size and nodes without images
// Prints "ok <sizes>" or a diagnostic and exits 1.
#include "resection_plan.h"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static int fail(const char* what, long a, long b) { std::printf("FAIL %s %ld %ld\n", what, a, b); return 1; }

int main(int argc, char** argv) {
  std::mt19937_64 rng(argc > 1 ? std::atoll(argv[1]) : 1);
  std::vector<int64_t> sizes = {0, 1, 63, 64, 65, 255, 256, 257, 1000, 65535, 65536, 65537, 12345678, ((int64_t)1 << 31) - 1};
  for (int k = 0; k < 50; ++k) sizes.push_back((int64_t)(rng() % 5000000));
  for (int64_t n : sizes) {
    const resect_layout L = resect_plan_layout(n);
    const int64_t blocks = resect_blocks(n);
    if (blocks * RESECT_BLOCK < n || (blocks > 0 && (blocks - 1) * RESECT_BLOCK >= n)) return fail("blocks", (long)n, (long)blocks);
    const int64_t words = blocks * RESECT_WAVES, sums = blocks + 1;
    if (words * 64 < n) return fail("words", (long)n, (long)words);
    struct { int64_t at, bytes; } part[] = {{L.mask, words * 8}, {L.blk, sums * 4}};
    int64_t end = 0;
    for (auto& p : part) {
      if (p.at % 256 != 0) return fail("alignment", (long)n, (long)p.at);
      if (p.at < end) return fail("overlap", (long)n, (long)p.at);
      end = p.at + p.bytes;
    }
    if (end > L.bytes) return fail("bytes", (long)end, (long)L.bytes);
    if (L.bytes <= ((int64_t)1 << 26)) {
      std::vector<char> ws((size_t)L.bytes);
      unsigned long long* mask = (unsigned long long*)(ws.data() + L.mask);
      int* blk = (int*)(ws.data() + L.blk);
      if (words) { mask[0] = ~0ull; mask[words - 1] = ~0ull; }
      blk[0] = 1; blk[sums - 1] = 2;
      if (words && (mask[0] != ~0ull || mask[words - 1] != ~0ull)) return fail("clobbered", (long)n, 0);
    }
    if (resect_check_sizes(n ? 1 : 0, n, 0, 0) != 0) return fail("sizes accepted", (long)n, 0);
  }
  if (resect_check_sizes(1, (int64_t)1 << 31, 1, 1) != 2) return fail("2^31", 0, 0);
  if (resect_check_sizes(0, 10, 1, 1) != 3) return fail("images", 0, 0);
  if (resect_check_sizes(-1, 0, 0, 0) != 1 || resect_check_sizes(1, -1, 0, 0) != 1 || resect_check_sizes(1, 1, -1, 0) != 1 ||
      resect_check_sizes(1, 1, 0, -1) != 1)
    return fail("negative", 0, 0);
  std::printf("ok %ld\n", (long)sizes.size());
  return 0;
}
