// The Jacobi routines of the two-view kernels (sfm_amd/csrc/pose_solve.h) built for the host, so that the CPU tests can
// set them against LAPACK (tests/test_pose_reference.py).
//   pose_solve_check essential IN OUT:  IN holds records of 9 doubles (E row-major); OUT gets 49 doubles per record:
//                                       1 or 0 (a model or none), then Rt [4][12].
//   pose_solve_check null4 IN OUT:      IN holds records of 16 doubles (a 4 x 4, row-major); OUT gets the 4 doubles of
//                                       the right singular vector of its smallest singular value.
#include <cstdio>
#include <cstring>
#include "pose_solve.h"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const bool essential = !strcmp(argv[1], "essential");
  if (!essential && strcmp(argv[1], "null4")) return 2;
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 2;
  if (essential) {
    double E[9];
    while (fread(E, sizeof(double), 9, in) == 9) {
      double Rt[4][12], o[49];
      for (int c = 0; c < 4; ++c)
        for (int e = 0; e < 12; ++e) Rt[c][e] = 0.0;
      o[0] = jacobi::decompose_essential(E, Rt) ? 1.0 : 0.0;
      for (int c = 0; c < 4; ++c)
        for (int e = 0; e < 12; ++e) o[1 + 12 * c + e] = Rt[c][e];
      if (fwrite(o, sizeof(double), 49, out) != 49) return 3;
    }
  } else {
    double rec[16];
    while (fread(rec, sizeof(double), 16, in) == 16) {
      double U[4][4], v[4];
      for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) U[r][k] = rec[4 * r + k];
      jacobi::null4(U, v);
      if (fwrite(v, sizeof(double), 4, out) != 4) return 3;
    }
  }
  fclose(in);
  fclose(out);
  return 0;
}
