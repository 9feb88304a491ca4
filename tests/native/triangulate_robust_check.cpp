// The robust triangulation of the device (sfm_amd/csrc/triangulate_robust.h) built for the host, so that the CPU tests can
// set it against the NumPy restatement (tests/test_triangulate_robust_reference.py).  All numbers are doubles.
//   triangulate_robust_check robust IN OUT:    IN holds tracks: n_raw, min_views, refine_iters, max_error, check_angle,
//                                              cos_min_angle, then n_raw observations of 15: used (0 / 1), P [12], x, y.
//                                              OUT gets per track: status, n_views, n_inliers, X [3], max_err, then the
//                                              n_raw flags of tri::solve_robust.
//   triangulate_robust_check classify IN OUT:  the same records with X [3] appended to the head (9 numbers).  OUT gets per
//                                              track: status, n_inliers, max_err, then the n_raw flags of
//                                              tri::flag_inliers at X.
//   triangulate_robust_check pairs IN OUT:     IN holds values of s; OUT gets per s: hypotheses(s), then for every h < 64
//                                              the pair number, a and b of tri::pair_of (-1 for h >= hypotheses(s)).
#include <cstdio>
#include <cstring>
#include <vector>
#include "triangulate_robust.h"

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

static bool read_track(FILE* in, int n_raw, std::vector<tri::Obs>& obs, std::vector<char>& used) {
  obs.resize(n_raw);
  used.resize(n_raw);
  for (int k = 0; k < n_raw; ++k) {
    double rec[15];
    if (fread(rec, sizeof(double), 15, in) != 15) return false;
    used[k] = rec[0] != 0.0;
    for (int e = 0; e < 12; ++e) obs[k].P[e] = rec[1 + e];
    obs[k].x = rec[13]; obs[k].y = rec[14];
    tri::camera_centre(obs[k].P, obs[k].C);
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 2;
  std::vector<tri::Obs> obs;
  std::vector<char> used;
  if (!strcmp(argv[1], "robust")) {
    double head[6];
    while (fread(head, sizeof(double), 6, in) == 6) {
      const int n_raw = (int)head[0];
      if (!read_track(in, n_raw, obs, used)) return 3;
      HostSrc src{&obs, &used};
      std::vector<uint8_t> flags(n_raw + 1, 7);
      double X[3], max_err;
      int n_views, n_inliers;
      std::vector<double> o(7 + n_raw);
      o[0] = tri::solve_robust(src, n_raw, (int)head[1], (int)head[2], head[3], head[4] != 0.0, head[5], X, n_views, n_inliers,
                               max_err, flags.data());
      o[1] = n_views; o[2] = n_inliers; o[3] = X[0]; o[4] = X[1]; o[5] = X[2]; o[6] = max_err;
      for (int k = 0; k < n_raw; ++k) o[7 + k] = flags[k];
      if (fwrite(o.data(), sizeof(double), o.size(), out) != o.size()) return 3;
    }
  } else if (!strcmp(argv[1], "classify")) {
    double head[9];
    while (fread(head, sizeof(double), 9, in) == 9) {
      const int n_raw = (int)head[0];
      if (!read_track(in, n_raw, obs, used)) return 3;
      HostSrc src{&obs, &used};
      std::vector<uint8_t> flags(n_raw + 1, 7);
      const double X[3] = {head[6], head[7], head[8]};
      double max_err;
      int n_inliers;
      std::vector<double> o(3 + n_raw);
      o[0] = tri::classify(src, n_raw, (int)head[1], X, head[3], head[4] != 0.0, head[5], n_inliers, max_err);
      o[1] = n_inliers; o[2] = max_err;
      tri::flag_inliers(src, n_raw, X, head[3], flags.data());
      for (int k = 0; k < n_raw; ++k) o[3 + k] = flags[k];
      if (fwrite(o.data(), sizeof(double), o.size(), out) != o.size()) return 3;
    }
  } else if (!strcmp(argv[1], "pairs")) {
    double sv;
    while (fread(&sv, sizeof(double), 1, in) == 1) {
      const int s = (int)sv, n = tri::hypotheses(s);
      double o[1 + 3 * SFM_TRI_ROBUST_PAIRS];
      o[0] = n;
      for (int h = 0; h < SFM_TRI_ROBUST_PAIRS; ++h) {
        int a = -1, b = -1;
        const double pair = h < n ? (double)tri::pair_of(h, s, a, b) : -1.0;
        o[1 + 3 * h] = pair; o[2 + 3 * h] = a; o[3 + 3 * h] = b;
      }
      if (fwrite(o, sizeof(double), 1 + 3 * SFM_TRI_ROBUST_PAIRS, out) != 1 + 3 * SFM_TRI_ROBUST_PAIRS) return 3;
    }
  } else {
    return 2;
  }
  fclose(in);
  fclose(out);
  return 0;
}
