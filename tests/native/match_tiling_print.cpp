// Host-only: prints what sfm_amd/csrc/match_plan.h plans for ONE pair, so that tests place their rows at the split
// seams the library really uses (tests/matcher_truth.py: match_tiling).  Arguments: metric nq nt dim; output:
// "<queries per workgroup> <splits> <train rows per split>".
#define SFM_MATCH_PLAN_STANDALONE 1
#include "match_plan.h"
#include <cstdio>

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  const int metric = std::atoi(argv[1]), dim = std::atoi(argv[4]);
  const int64_t nq = std::atoll(argv[2]), nt = std::atoll(argv[3]);
  const int64_t qpw = match_qpw(metric, dim, nq, false);
  int nsplit; int64_t rps;
  match_tiling(metric, nq, qpw, nt, &nsplit, &rps);
  std::printf("%lld %d %lld\n", (long long)qpw, nsplit, (long long)rps);
  return 0;
}
