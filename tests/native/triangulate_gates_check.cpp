// The gates of the N-view triangulation at a given point (tri::judge / tri::gates / tri::reproj of
// sfm_amd/csrc/triangulate_solve.h) built for the host, so that the CPU tests can set them against the NumPy restatement
// (tests/test_incremental_reference.py).  All numbers are doubles.
//   triangulate_gates_check IN OUT:  IN holds tracks: n_raw, min_views, max_error, check_angle, cos_min_angle, X [3], then
//                                    n_raw observations of 15: used (0 / 1), P [12], x, y.  OUT gets 3 + n_raw per track:
//                                    status, n_views, max_err of tri::judge, then the reprojection error of every
//                                    observation (tri::reproj; NaN when not used).
#include <cstdio>
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
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  double head[8];
  while (fread(head, sizeof(double), 8, in) == 8) {
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
    const double X[3] = {head[5], head[6], head[7]};
    double max_err;
    int n_views;
    std::vector<double> o(3 + n_raw);
    o[0] = tri::judge(src, n_raw, (int)head[1], X, head[2], head[3] != 0.0, head[4], n_views, max_err);
    o[1] = n_views; o[2] = max_err;
    for (int k = 0; k < n_raw; ++k) {
      double hw, e2;
      o[3 + k] = used[k] ? tri::reproj(obs[k], X, hw, e2) : NAN;
    }
    if (fwrite(o.data(), sizeof(double), o.size(), out) != o.size()) return 3;
  }
  fclose(in);
  fclose(out);
  return 0;
}
