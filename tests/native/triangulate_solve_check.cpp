// The N-view triangulation of the device (sfm_amd/csrc/triangulate_solve.h) built for the host, so that the CPU tests can
// set it against the NumPy restatement (tests/test_triangulate_reference.py).  All numbers are doubles.
//   triangulate_solve_check solve IN OUT:  IN holds tracks: n_raw, min_views, refine_iters, max_error, check_angle,
//                                          cos_min_angle, then n_raw observations of 15: used (0 / 1), P [12], x, y.
//                                          OUT gets 6 per track: status, n_views, X [3], max_err.
//   triangulate_solve_check dlt2 IN OUT:   IN holds records of 28: P0 [12], P1 [12], x0, y0, x1, y1; OUT gets
//                                          v[:3] / v[3] of jacobi::dlt2, 3 per record.
//   triangulate_solve_check centre IN OUT: IN holds records of 12 (P); OUT gets the camera centre, 3 per record.
#include <cstdio>
#include <cstring>
#include <vector>
#include "triangulate_solve.h"

struct HostSrc {
  const std::vector<tri::Obs>* obs;
  const std::vector<char>* used;
  bool get(int k, tri::Obs& o) const {
    if (!(*used)[k]) return false;
    o = (*obs)[k];
    return true;
  }
  bool centre(int k, double (&C)[3]) const {
    if (!(*used)[k]) return false;
    for (int e = 0; e < 3; ++e) C[e] = (*obs)[k].C[e];
    return true;
  }
};

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 2;
  if (!strcmp(argv[1], "solve")) {
    double head[6];
    while (fread(head, sizeof(double), 6, in) == 6) {
      const int n_raw = (int)head[0];
      std::vector<tri::Obs> obs(n_raw);
      std::vector<char> used(n_raw);
      for (int k = 0; k < n_raw; ++k) {
        double rec[15];
        if (fread(rec, sizeof(double), 15, in) != 15) return 3;
        used[k] = rec[0] != 0.0;
        for (int e = 0; e < 12; ++e) obs[k].P[e] = rec[1 + e];
        obs[k].x = rec[13]; obs[k].y = rec[14];
        tri::camera_centre(obs[k].P, obs[k].C);
      }
      HostSrc src{&obs, &used};
      double X[3], max_err, o[6];
      int n_views;
      o[0] = tri::solve(src, n_raw, (int)head[1], (int)head[2], head[3], head[4] != 0.0, head[5], X, n_views, max_err);
      o[1] = n_views; o[2] = X[0]; o[3] = X[1]; o[4] = X[2]; o[5] = max_err;
      if (fwrite(o, sizeof(double), 6, out) != 6) return 3;
    }
  } else if (!strcmp(argv[1], "dlt2")) {
    double rec[28];
    while (fread(rec, sizeof(double), 28, in) == 28) {
      double P0[12], P1[12], v[4], o[3];
      for (int e = 0; e < 12; ++e) { P0[e] = rec[e]; P1[e] = rec[12 + e]; }
      jacobi::dlt2(P0, P1, rec[24], rec[25], rec[26], rec[27], v);
      for (int e = 0; e < 3; ++e) o[e] = v[e] / v[3];
      if (fwrite(o, sizeof(double), 3, out) != 3) return 3;
    }
  } else if (!strcmp(argv[1], "centre")) {
    double P[12], C[3];
    while (fread(P, sizeof(double), 12, in) == 12) {
      tri::camera_centre(P, C);
      if (fwrite(C, sizeof(double), 3, out) != 3) return 3;
    }
  } else {
    return 2;
  }
  fclose(in);
  fclose(out);
  return 0;
}
