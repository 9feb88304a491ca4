// The solver and the error rule of the homography RANSAC kernels (sfm_amd/csrc/homography_solve.h, homography_rule.h)
// built for the host, so that the CPU tests can set them against the NumPy reference hypothesis by hypothesis
// (tests/test_homography_reference.py).
//   homography_solve_check IN OUT:  IN holds doubles: M, H, threshold, the segment's transforms {sc1, cx1, cy1, sc2, cx2,
//   cy2}, then M matches as u1, v1, u2, v2 (float32 values), then H samples of 4 indices.  OUT gets 11 doubles per
//   hypothesis: 1 if the sample gave a model, its H [9] (zero without one), and its inlier count over the M matches as
//   k_hom_hypotheses counts it (a match with a non-finite coordinate is staged as NaN).
#include <cstdio>
#include <vector>
#include "homography_rule.h"
#include "homography_solve.h"

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
  std::vector<double> pts(4 * (size_t)M), smp(4 * (size_t)H);
  if (fread(pts.data(), sizeof(double), pts.size(), in) != pts.size()) return 3;
  if (fread(smp.data(), sizeof(double), smp.size(), in) != smp.size()) return 3;
  for (int hyp = 0; hyp < H; ++hyp) {
    float px[4][4];
    bool ok = true;
    for (int k = 0; k < 4; ++k) {
      const long id = (long)smp[4 * (size_t)hyp + k];
      ok = ok && id >= 0 && id < M;
      for (int e = 0; e < 4; ++e) px[k][e] = ok ? (float)pts[4 * (size_t)id + e] : 0.0f;
    }
    double h[9], o[11];
    const bool good = ok && homog::solve_sample(px, head + 3, h);
    int count = 0;
    for (int e = 0; e < 9; ++e) h[e] = good ? h[e] : 0.0;
    for (int i = 0; i < M; ++i) {
      const double* p = &pts[4 * (size_t)i];
      const bool fin = std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(p[3]);
      const double nan = std::nan("");
      count += hom_inlier(h, fin ? p[0] : nan, fin ? p[1] : nan, fin ? p[2] : nan, fin ? p[3] : nan, thr2) ? 1 : 0;
    }
    o[0] = good ? 1.0 : 0.0;
    for (int e = 0; e < 9; ++e) o[1 + e] = h[e];
    o[10] = (double)count;
    if (fwrite(o, sizeof(double), 11, out) != 11) return 4;
  }
  fclose(in);
  fclose(out);
  return 0;
}
