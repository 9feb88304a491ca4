// The five-point solver of the essential-matrix RANSAC kernel (sfm_amd/csrc/essential_solve.h) built for the host, so
// that the CPU tests can set it against the NumPy reference sample by sample (tests/test_essential_reference.py).
//   essential_solve_check IN OUT:  IN holds records of 24 doubles (five matches as u1, v1, u2, v2 - float32 values - then
//   fx, fy, cx, cy); OUT gets 91 doubles per record: the number of filled slots, then E [10][9], packed to the front as the kernel
//   packs them (zero past that number).
#include <cstdio>
#include "essential_solve.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  double rec[24];
  while (fread(rec, sizeof(double), 24, in) == 24) {
    float px[5][4];
    for (int k = 0; k < 5; ++k)
      for (int e = 0; e < 4; ++e) px[k][e] = (float)rec[4 * k + e];
    double store[fivept::WS_DOUBLES], Bs[4][9], o[91];
    const fivept::strided<1> ws{store};
    const int nc = fivept::solve_sample(px, rec[20], rec[21], rec[22], rec[23], ws, Bs);
    if (nc < 0 || nc > fivept::MAX_CANDIDATES) return 4;
    for (int e = 0; e < 91; ++e) o[e] = 0.0;
    int filled = 0;                                        // as k_ess_solve packs them: only the candidates that are finite
    for (int k = 0; k < nc; ++k) {
      double E[9];
      if (!fivept::candidate(Bs, ws, k, E)) continue;
      for (int e = 0; e < 9; ++e) o[1 + 9 * filled + e] = E[e];
      ++filled;
    }
    o[0] = (double)filled;
    if (fwrite(o, sizeof(double), 91, out) != 91) return 3;
  }
  fclose(in);
  fclose(out);
  return 0;
}
