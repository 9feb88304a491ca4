// Host-only check of sfm_amd/csrc/match_plan.h, built with -fsanitize=address,undefined by tests/test_host_logic.py.
// Random segment tables -> plan_segments: every (query row, train row) of every segment must be covered by exactly one
// piece, pieces stay inside their segment, splits are whole 128-row chunks except the last, output rows are the
// segment's query rows in order; pick_nsplit respects its limits; match_u8_kernel picks the expected uint8 kernel, filter
// and split weights on each side of its thresholds.  Prints "ok <pieces>" or a diagnostic and exits 1.
#define SFM_MATCH_PLAN_STANDALONE 1
#include "match_plan.h"
#include <cstdio>
#include <random>

static int fail(const char* what, long a, long b) { std::printf("FAIL %s %ld %ld\n", what, a, b); return 1; }

int main(int argc, char** argv) {
  std::mt19937_64 rng(argc > 1 ? std::atoll(argv[1]) : 1);
  long total_pieces = 0;
  for (int round = 0; round < 200; ++round) {
    const int n_seg = 1 + (int)(rng() % 40);
    const int metric = (int)(rng() % 3);
    const int dim = metric == SFM_METRIC_HAMMING ? 32 : (int[]){32, 64, 128}[rng() % 3];
    std::vector<int64_t> img_ptr(1, 0);
    const int n_img = 2 + (int)(rng() % 12);
    for (int i = 0; i < n_img; ++i) {
      const int kind = (int)(rng() % 5);
      const int64_t sz = kind == 0 ? 0 : kind == 1 ? 2 + (int64_t)(rng() % 40) : kind == 2 ? 200 + (int64_t)(rng() % 3000)
                                                   : kind == 3 ? 2048 + (int64_t)(rng() % 9000) : 511 + (int64_t)(rng() % 3);
      img_ptr.push_back(img_ptr.back() + sz);
    }
    std::vector<int64_t> qb(n_seg), qe(n_seg), tb(n_seg), te(n_seg);
    for (int s = 0; s < n_seg; ++s) {
      const int i = (int)(rng() % n_img), j = (int)(rng() % n_img);
      qb[s] = img_ptr[i]; qe[s] = img_ptr[i + 1]; tb[s] = img_ptr[j]; te[s] = img_ptr[j + 1];
    }
    std::vector<MatchWG> wgs; std::vector<int64_t> out_ptr;
    plan_segments(metric, dim, n_seg, qb.data(), qe.data(), tb.data(), te.data(), &wgs, &out_ptr);
    total_pieces += (long)wgs.size();
    size_t k = 0;
    for (int s = 0; s < n_seg; ++s) {
      const int64_t nq = qe[s] - qb[s], nt = te[s] - tb[s];
      if (out_ptr[s + 1] - out_ptr[s] != nq) return fail("out_ptr", s, (long)nq);
      if (nq <= 0) continue;
      const int64_t qpw = match_qpw(metric, dim, nq, true);
      for (int64_t q0 = 0; q0 < nq; q0 += qpw) {
        int64_t covered = 0; int split = 0;
        while (k < wgs.size() && wgs[k].q_first == qb[s] + q0 && wgs[k].t_seg == tb[s] && wgs[k].out_first == out_ptr[s] + q0) {
          const MatchWG& r = wgs[k];
          if (r.q_end != qe[s] || r.split != split) return fail("piece header", s, split);
          if (r.t_first != tb[s] + covered) return fail("split start", (long)r.t_first, (long)(tb[s] + covered));
          if (r.t_end > te[s] || r.t_end < r.t_first) return fail("split end", (long)r.t_end, (long)te[s]);
          if (r.t_end != te[s] && metric == SFM_METRIC_L2_U8 && (r.t_end - r.t_first) % 128 != 0) return fail("chunk multiple", s, split);
          covered += r.t_end - r.t_first; ++split; ++k;
          if (split > 8) return fail("more than 8 splits", s, split);
          if (covered == nt) break;
        }
        if (covered != nt && nt > 0) return fail("train rows covered", (long)covered, (long)nt);
        if (nt <= 0 && split != 1) return fail("empty train set pieces", s, split);
      }
    }
    if (k != wgs.size()) return fail("stray pieces", (long)k, (long)wgs.size());
  }
  for (int64_t nt : {2L, 511L, 512L, 1024L, 4095L, 50000L, 1000000L})
    for (int64_t nqb : {1L, 7L, 98L, 196L, 4000L}) {
      const int ns = pick_nsplit(nt, nqb);
      if (ns < 1 || ns > 8 || (ns > 1 && nt / ns < 512)) return fail("pick_nsplit", (long)nt, ns);
    }
  // the uint8 distance kernel on each side of every threshold of match_u8_kernel, for one pair planned as sfm_match_knn2
  // plans it (nsplit / grid checked where given: they decide the split weights)
  struct KernelCase { int64_t nq, nt; int dim; MatchU8Kernel kernel; bool filter; int w_first, w_second, nsplit; int64_t grid; };
  const KernelCase cases[] = {
      {50000, 50000, 128, MATCH_U8_DIRECT4, false, MATCH_W_FIRST, MATCH_W_SECOND, 5, 490},   // one round of two workgroups per CU
      {50000, 10240, 128, MATCH_U8_DIRECT4, false, MATCH_W_FIRST, MATCH_W_SECOND, 5, 490},   // 2,048 train rows per split
      {131072, 8192, 128, MATCH_U8_DIRECT4, false, MATCH_W_FIRST, MATCH_W_SECOND, 2, 512},   // 512 workgroups, two splits
      {50000, 10000, 128, MATCH_U8_DIRECT4, false, 0, 0, 5, 490},                            // 2,000 per split: even
      {150000, 600, 128, MATCH_U8_DIRECT4, false, 0, 0, 1, 293},                             // one split: even
      {28672, 2000, 128, MATCH_U8_DIRECT4, false, 0, 0, 3, 168},                             // 256 workgroups or fewer: even
      {300000, 50000, 128, MATCH_U8_DIRECT4, false, 0, 0, 6, 3516},                          // more than 512 workgroups: even
      {28671, 2000, 128, MATCH_U8_DIRECT2, false, 0, 0, 0, 0},                               // below 28,672 queries: two query blocks
      {20000, 20000, 128, MATCH_U8_DIRECT2, false, 0, 0, 6, 474},                            // weights only for four query blocks
      {20000, 400, 128, MATCH_U8_DIRECT2, false, 0, 0, 0, 0},                                // 8e6 distances
      {20000, 399, 128, MATCH_U8_LDS, false, 0, 0, 0, 0},                                    // below 8e6: the LDS kernel
      {20001, 3, 128, MATCH_U8_LDS, false, 0, 0, 0, 0},
      {2000, 2300, 128, MATCH_U8_LDS, true, 0, 0, 0, 0},                                     // the filter from 2,048 train rows
      {2000, 2048, 128, MATCH_U8_LDS, true, 0, 0, 0, 0},
      {2000, 2047, 128, MATCH_U8_LDS, false, 0, 0, 0, 0},
      {30000, 30000, 256, MATCH_U8_DIRECT2_KS8, false, 0, 0, 0, 0},                          // dim 256 (ORB over unpacked bits)
      {2000, 4000, 256, MATCH_U8_DIRECT2_KS8, false, 0, 0, 0, 0},
      {2000, 3999, 256, MATCH_U8_LDS, true, 0, 0, 0, 0},
      {30000, 30000, 64, MATCH_U8_LDS, true, 0, 0, 0, 0},                                    // dims below 128: always the LDS kernel
      {30000, 30000, 32, MATCH_U8_LDS, true, 0, 0, 0, 0},
  };
  for (const KernelCase& e : cases) {
    const int64_t qpw = match_qpw(SFM_METRIC_L2_U8, e.dim, e.nq, false);
    int nsplit; int64_t rps;
    match_tiling(SFM_METRIC_L2_U8, e.nq, qpw, e.nt, &nsplit, &rps);
    const int64_t grid = (e.nq + qpw - 1) / qpw * nsplit;
    const MatchU8Choice c = match_u8_kernel(e.dim, e.nq, e.nt, qpw, false, e.nt, grid, nsplit);
    if (c.kernel != e.kernel || c.filter != e.filter) return fail("kernel", (long)e.nq, (long)e.nt);
    if (c.w_first != e.w_first || c.w_second != e.w_second) return fail("split weights", (long)e.nq, (long)e.nt);
    if (e.nsplit && (nsplit != e.nsplit || grid != e.grid)) return fail("tiling", nsplit, (long)grid);
  }
  // a batched plan takes the LDS kernel whatever its size; the filter follows the longest segment
  for (int64_t longest : {2047L, 2048L, 30000L}) {
    const int64_t qb[2] = {0, 30000}, qe[2] = {30000, 60000}, tb[2] = {0, 1000}, te[2] = {1000, 1000 + longest};
    std::vector<MatchWG> wgs; std::vector<int64_t> out_ptr;
    plan_segments(SFM_METRIC_L2_U8, 128, 2, qb, qe, tb, te, &wgs, &out_ptr);
    const MatchU8Choice c = match_u8_kernel(128, 60000, 1000 + longest, 256, true, longest, (int64_t)wgs.size(), 1);
    if (c.kernel != MATCH_U8_LDS || c.filter != (longest >= 2048) || c.w_first || c.w_second) return fail("batched kernel", (long)longest, c.kernel);
  }
  std::printf("ok %ld\n", total_pieces);
  return 0;
}
