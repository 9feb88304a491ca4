// The sample generator every RANSAC stage shares (draw_distinct<3> and draw_distinct<7> of
// sfm_amd/csrc/ransac_common.h) built for the host, so that the CPU tests can set it against the NumPy generator index
// for index (tests/test_pnp_reference.py).
//   ransac_common_check IN OUT:  IN holds records of 5 uint64 (sample size 3 or 7, seed, segment, M >= size, hypotheses);
//   OUT gets hypotheses x size int32 per record.
#include <cstdio>
#include "ransac_common.h"

template <int N>
static bool draw(const uint64_t* rec, FILE* out) {
  bool ok = rec[3] >= (uint64_t)N;
  for (int hyp = 0; ok && hyp < (int)rec[4]; ++hyp) {
    int idx[N];
    draw_distinct<N>(rec[1], (int)rec[2], hyp, (int)rec[3], idx);
    ok = fwrite(idx, sizeof(int), N, out) == (size_t)N;
  }
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  uint64_t rec[5];
  while (fread(rec, sizeof(uint64_t), 5, in) == 5)
    if (!(rec[0] == 3 ? draw<3>(rec, out) : rec[0] == 7 && draw<7>(rec, out))) return 3;
  fclose(in);
  fclose(out);
  return 0;
}
