// The solver and the error rule of the fundamental-matrix RANSAC kernels (sfm_amd/csrc/fundamental_solve.h,
// fundamental_rule.h) built for the host, so that the CPU tests can set them against the NumPy reference hypothesis by
// hypothesis (tests/test_fundamental_reference.py).
//   fundamental_solve_check IN OUT:  IN holds doubles: M, H, threshold, the segment's transforms {sc1, cx1, cy1, sc2,
//   cx2, cy2}, then M matches as u1, v1, u2, v2 (float32 values), then H samples of 7 indices.  OUT gets 33 doubles per
//   hypothesis: for each of the three candidates 1 if the slot holds a model, then their F [3][9] (zero without one), then
//   their three inlier counts over the M matches as k_fund_hypotheses counts them (a match with a non-finite coordinate
//   is staged as NaN).  A sample with an index outside [0, M) gives no model and reads no match.
#include <cstdio>
#include <vector>
#include "fundamental_rule.h"
#include "fundamental_solve.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  double head[9];
  if (fread(head, sizeof(double), 9, in) != 9) return 3;
  const int M = (int)head[0], H = (int)head[1];
  const double thr2 = head[2] * head[2];
  if (M < 0 || H < 0) return 3;
  std::vector<double> pts(4 * (size_t)M), smp(7 * (size_t)H);
  if (fread(pts.data(), sizeof(double), pts.size(), in) != pts.size()) return 3;
  if (fread(smp.data(), sizeof(double), smp.size(), in) != smp.size()) return 3;
  for (int hyp = 0; hyp < H; ++hyp) {
    float px[7][4];
    bool ok = true;
    for (int k = 0; k < 7; ++k) {
      const long id = (long)smp[7 * (size_t)hyp + k];
      ok = ok && id >= 0 && id < M;
    }
    for (int k = 0; k < 7; ++k)
      for (int e = 0; e < 4; ++e) px[k][e] = ok ? (float)pts[4 * (size_t)smp[7 * (size_t)hyp + k] + e] : 0.0f;
    double Fc[3][9], o[33];
    sevenpt::solve_matches([&](int i, bool, float (&m)[4]) {
      for (int e = 0; e < 4; ++e) m[e] = px[i][e];
      return ok;
    }, head + 3, Fc);
    int count[3] = {0, 0, 0};
    for (int i = 0; i < M; ++i) {
      const double* p = &pts[4 * (size_t)i];
      const bool fin = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3]);
      const double nan = std::nan("");
      for (int k = 0; k < 3; ++k)
        count[k] += fund_inlier(Fc[k], fin ? p[0] : nan, fin ? p[1] : nan, fin ? p[2] : nan, fin ? p[3] : nan, thr2) ? 1 : 0;
    }
    for (int k = 0; k < 3; ++k) {
      bool model = false;
      for (int e = 0; e < 9; ++e) { model = model || Fc[k][e] != 0.0; o[3 + 9 * k + e] = Fc[k][e]; }
      o[k] = model ? 1.0 : 0.0;
      o[30 + k] = (double)count[k];
    }
    if (fwrite(o, sizeof(double), 33, out) != 33) return 4;
  }
  fclose(in);
  fclose(out);
  return 0;
}
