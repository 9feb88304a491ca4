// Host-only check of sfm_amd/csrc/tracks_plan.h, built with -fsanitize=address,undefined by tests/test_tracks_reference.py.
//   layout   the arrays of the workspace are 256-byte aligned, lie inside `bytes`, do not overlap and hold what the
//            kernels index (n_nodes, cap_tracks + 1, cap_long, scan blocks + 1 entries)
//   route    lane / LDS / global on each side of both thresholds; the long list holds every component it can get
//   sizes    tracks_check_sizes accepts the bounds n_nodes / 2 and n_nodes and rejects anything below, min_len < 2, 2^31
//   network  the comparators of tracks_bitonic_mirror / _step, run in order with j >= len skipped, sort every length from
//            1 to 300, lengths around the powers of two up to 2^13 and around TRACKS_LDS_MAX; every comparator has
//            i < j, and within a step no index occurs twice (the lanes of a step do not race)
// Prints "ok <comparators>" or a diagnostic and exits 1.
#include "tracks_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

static int fail(const char* what, long a, long b) { std::printf("FAIL %s %ld %ld\n", what, a, b); return 1; }

static long comparators = 0;

static int run_step(std::vector<int>& a, std::vector<char>& seen, unsigned len, unsigned lp, unsigned lk, int ld) {
  std::fill(seen.begin(), seen.end(), 0);
  for (unsigned t = 0; t < (1u << (lp - 1)); ++t) {
    unsigned i, j;
    if (ld < 0) tracks_bitonic_mirror(t, lk, i, j); else tracks_bitonic_step(t, (unsigned)ld, i, j);
    if (!(i < j) || j >= (1u << lp)) return fail("comparator range", (long)i, (long)j);
    if (j >= len) continue;
    if (seen[i] || seen[j]) return fail("index twice in a step", (long)i, (long)j);
    seen[i] = seen[j] = 1;
    ++comparators;
    if (a[i] > a[j]) std::swap(a[i], a[j]);
  }
  return 0;
}

static int check_sort(std::mt19937_64& rng, unsigned len, int kind) {
  std::vector<int> a(len), ref;
  for (unsigned k = 0; k < len; ++k)
    a[k] = kind == 0 ? (int)(rng() % 0x7fffffffu) : kind == 1 ? (int)(len - k) : kind == 2 ? (int)(rng() % 4) : (int)k;
  ref = a;
  std::sort(ref.begin(), ref.end());
  const unsigned lp = tracks_bitonic_levels(len);
  if (lp < 1 || (1u << lp) < len || (lp > 1 && (1u << (lp - 1)) >= len)) return fail("levels", (long)len, (long)lp);
  std::vector<char> seen(len);
  for (unsigned lk = 1; lk <= lp; ++lk) {
    if (run_step(a, seen, len, lp, lk, -1)) return 1;
    for (int ld = (int)lk - 2; ld >= 0; --ld)
      if (run_step(a, seen, len, lp, lk, ld)) return 1;
  }
  if (a != ref) return fail("not sorted", (long)len, kind);
  return 0;
}

int main(int argc, char** argv) {
  std::mt19937_64 rng(argc > 1 ? std::atoll(argv[1]) : 1);
  // layout
  std::vector<int64_t> sizes = {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 17500, 40000, 200000, 12345678, ((int64_t)1 << 31) - 1};
  for (int k = 0; k < 50; ++k) sizes.push_back((int64_t)(rng() % 5000000));
  for (int64_t n : sizes) {
    const tracks_layout L = tracks_plan_layout(n);
    const int64_t cand = tracks_cap_tracks(n) + 1;
    struct { int64_t at, bytes; } part[] = {
        {L.ctr, TRACKS_CTR_COUNT * 8}, {L.parent, n * 4}, {L.label, n * 4}, {L.size, n * 4}, {L.cidx, n * 4}, {L.members, n * 4},
        {L.cand_root, cand * 4}, {L.cand_off, cand * 4}, {L.cand_len, cand * 4}, {L.cand_cur, cand * 4}, {L.cand_conf, cand * 4},
        {L.cand_tid, cand * 4}, {L.cand_obs, cand * 4}, {L.long_list, tracks_cap_long(n) * 4},
        {L.blk_a, (tracks_scan_blocks(n) + 1) * 4}, {L.blk_b, (tracks_scan_blocks(n) + 1) * 4}};
    int64_t end = 0;
    for (auto& p : part) {
      if (p.at % 256 != 0) return fail("alignment", (long)n, (long)p.at);
      if (p.at < end) return fail("overlap", (long)n, (long)p.at);
      end = p.at + p.bytes;
    }
    if (end > L.bytes) return fail("bytes", (long)end, (long)L.bytes);
    // every long component has more than TRACKS_SHORT_MAX nodes: at most n / (TRACKS_SHORT_MAX + 1) of them
    if (tracks_cap_long(n) < n / (TRACKS_SHORT_MAX + 1)) return fail("cap_long", (long)n, (long)tracks_cap_long(n));
    if (tracks_scan_blocks(n) * 256 < n) return fail("scan blocks", (long)n, 0);
    if (tracks_check_sizes(n ? 1 : 0, n, 1, 1, 2, 0, n / 2, n) != 0) return fail("sizes accepted", (long)n, 0);
    if (n >= 2 && tracks_check_sizes(1, n, 1, 1, 2, 0, n / 2 - 1, n) == 0) return fail("cap_tracks", (long)n, 0);
    if (n >= 1 && tracks_check_sizes(1, n, 1, 1, 2, 0, n / 2, n - 1) == 0) return fail("cap_obs", (long)n, 0);
  }
  if (tracks_check_sizes(1, (int64_t)1 << 31, 1, 1, 2, 0, (int64_t)1 << 31, (int64_t)1 << 31) == 0) return fail("2^31", 0, 0);
  if (tracks_check_sizes(1, 10, 1, 1, 1, 0, 5, 10) == 0) return fail("min_len", 0, 0);
  if (tracks_check_sizes(1, 10, 1, 1, 2, 2, 5, 10) == 0) return fail("policy", 0, 0);
  if (tracks_check_sizes(0, 10, 1, 1, 2, 0, 5, 10) == 0) return fail("images", 0, 0);
  if (tracks_check_sizes(1, 10, 1, -1, 2, 0, 5, 10) == 0) return fail("negative", 0, 0);
  // route
  if (tracks_route(2) != TRACKS_ROUTE_LANE || tracks_route(TRACKS_SHORT_MAX) != TRACKS_ROUTE_LANE ||
      tracks_route(TRACKS_SHORT_MAX + 1) != TRACKS_ROUTE_LDS || tracks_route(TRACKS_LDS_MAX) != TRACKS_ROUTE_LDS ||
      tracks_route(TRACKS_LDS_MAX + 1) != TRACKS_ROUTE_GLOBAL || tracks_route(((int64_t)1 << 31) - 1) != TRACKS_ROUTE_GLOBAL)
    return fail("route", 0, 0);
  // network
  std::vector<unsigned> lens;
  for (unsigned n = 1; n <= 300; ++n) lens.push_back(n);
  for (unsigned p = 9; p <= 13; ++p)
    for (int d = -1; d <= 1; ++d) lens.push_back((1u << p) + d);
  lens.push_back(3000);
  lens.push_back(TRACKS_LDS_MAX + 2);
  lens.push_back(5000 + (unsigned)(rng() % 3000));
  for (unsigned len : lens)
    for (int kind = 0; kind < 4; ++kind)
      if (check_sort(rng, len, kind)) return 1;
  std::printf("ok %ld\n", comparators);
  return 0;
}
