// The P3P solver of the PnP RANSAC kernel (sfm_amd/csrc/pnp_solve.h) built for the host, so that the CPU tests can
// set it against the NumPy reference sample by sample (tests/test_pnp_reference.py).
//   pnp_solve_check IN OUT:  IN holds records of 18 doubles (P [3][3] world points, f [3][3] unit bearings);
//   OUT gets 49 doubles per record: the bit mask of the filled candidate slots, then Rt [4][12].
#include <cstdio>
#include <vector>
#include "pnp_solve.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  double rec[18];
  while (fread(rec, sizeof(double), 18, in) == 18) {
    double P[3][3], f[3][3], Rt[4][12], o[49];
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 3; ++k) { P[i][k] = rec[3 * i + k]; f[i][k] = rec[9 + 3 * i + k]; }
    o[0] = (double)p3p::solve(P, f, Rt);
    for (int c = 0; c < 4; ++c)
      for (int e = 0; e < 12; ++e) o[1 + 12 * c + e] = Rt[c][e];
    if (fwrite(o, sizeof(double), 49, out) != 49) return 3;
  }
  fclose(in);
  fclose(out);
  return 0;
}
