// Fundamental-matrix RANSAC for every image pair of a driver step in one call (gfx950 only): the step between
// match_features and geometric_verification in the reference's pair loop, cv2.findFundamentalMat(pts1, pts2,
// cv2.FM_RANSAC, 3.0) at find_matches.py:282.
//
// Structure as OpenCV's FM_RANSAC is RECALLED (its source is not pinned here, like the matcher's rules): minimal
// samples of 7, the 7-point solver with up to three real solutions per sample, error of a match = the larger of its
// two squared point-to-epipolar-line distances, inlier when that is <= threshold^2, best model = most inliers, F
// scaled to F[2][2] = 1.  Deviations, on purpose: a FIXED number of hypotheses (no early exit on confidence) and an
// own, stateless sample generator, so that the result is a function of (points, seed) alone and a NumPy reference
// can follow the device hypothesis by hypothesis (tests/fundamental_reference.py).
//
// The 7-point solver is in fundamental_solve.h and the error rule in fundamental_rule.h; both compile for the host too.
// The sample kernel (k_ransac_samples<7, 7>), the Hartley normalisation, the workspace layout, the block sums, the
// whole-segment count, the winner rule and the refit's normal matrix and keep rule are shared with the other stages
// (ransac_kernels.h), the scoring loop with essential.hip and homography.hip (epipolar_rule.h).  The generator's rule
// stands above draw_distinct<N> in ransac_common.h and is restated in NumPy by the tests (tests/ransac_reference.py);
// its fallback after 256 draws is never reached in practice: 7 * (6/7)^256 = 5e-17 at M = 7.
//
// All arithmetic in float64.  Points arrive as float32 pixels [n][2] with a device seg_ptr[n_seg+1] (int64), the
// convention of sfm_epipolar_errors.  A match with a NaN or infinite coordinate is left out of the Hartley
// statistics and is staged as NaN for the scoring, so it fails every comparison; a sample that holds one gives no
// model.  Sample indices are range-checked on the device before they index anything.
#include "ransac_kernels.h"
#include "epipolar_rule.h"
#include "fundamental_solve.h"

namespace {

// --------------------------------------------------------------------------------------------- hypotheses
// One lane per (segment, hypothesis); a workgroup covers 256 hypotheses of ONE segment, so the scoring loop's points
// are wave-uniform: fetched from global memory once per workgroup and chunk into LDS, read back as broadcasts.
__global__ __launch_bounds__(256) void k_fund_hypotheses(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                         const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                         const int* __restrict__ samples, int H, int nblk, double thr2,
                                                         const double* __restrict__ T, int* __restrict__ hyp_count,
                                                         double* __restrict__ hyp_F) {
  __shared__ double2 s_pt[2 * FUND_CHUNK];
  const int s = blockIdx.x / nblk;
  const int hyp = (blockIdx.x % nblk) * 256 + threadIdx.x;
  const bool active = hyp < H;
  const int64_t slot = (int64_t)s * H + hyp;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  if (M < 7) {                                           // uniform over the workgroup
    if (active) {
      hyp_count[slot] = 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) hyp_F[slot * 9 + k] = 0.0;
    }
    return;
  }
  const double* t = T + 6 * (int64_t)s;
  double Fc[3][9];
  {
    bool in_range = active;
    int idx[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      idx[k] = active ? samples[slot * 7 + k] : 0;
      in_range = in_range && idx[k] >= 0 && idx[k] < M;
    }
    sevenpt::solve_matches([&](int i, bool ok, float (&m)[4]) {
      const int id = (ok && in_range) ? idx[i] : 0;
      const float2 p = pts1[b + id], q = pts2[b + id];
      m[0] = p.x; m[1] = p.y; m[2] = q.x; m[3] = q.y;
      return in_range;
    }, t, Fc);
  }
  // scoring: every lane walks all points of the segment with its (up to) three candidates in registers
  int cnt0 = 0, cnt1 = 0, cnt2 = 0;
  for_each_staged_point(s_pt, pts1, pts2, b, M, [&](double2 p, double2 q) {
    cnt0 += fund_inlier(Fc[0], p.x, p.y, q.x, q.y, thr2) ? 1 : 0;
    cnt1 += fund_inlier(Fc[1], p.x, p.y, q.x, q.y, thr2) ? 1 : 0;
    cnt2 += fund_inlier(Fc[2], p.x, p.y, q.x, q.y, thr2) ? 1 : 0;
  });
  if (!active) return;
  int best = cnt0;
  const bool use1 = cnt1 > best;
  best = use1 ? cnt1 : best;
  const bool use2 = cnt2 > best;
  best = use2 ? cnt2 : best;
  hyp_count[slot] = best;
#pragma unroll
  for (int e = 0; e < 9; ++e) hyp_F[slot * 9 + e] = use2 ? Fc[2][e] : (use1 ? Fc[1][e] : Fc[0][e]);
}

// ---------------------------------------------------------------------------------------------- selection
// winner per segment (ransac_winner): its F scaled to F[2][2] = 1, its mask and its count
__global__ __launch_bounds__(256) void k_fund_select(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                     const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                     int H, double thr2, const int* __restrict__ hyp_count,
                                                     const double* __restrict__ hyp_F, double* __restrict__ F,
                                                     uint8_t* __restrict__ mask, int* __restrict__ n_inliers,
                                                     int* __restrict__ status, int* __restrict__ refined) {
  const int s = blockIdx.x;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  int hp;
  const int st = ransac_winner(hyp_count, s, H, M, 7, hp);
  double f[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) f[e] = 0.0;
  int count = 0;
  if (st == 0) {                                         // uniform over the workgroup
#pragma unroll
    for (int e = 0; e < 9; ++e) f[e] = hyp_F[((int64_t)s * H + hp) * 9 + e];
    scale_last_to_one(f);
    count = fund_count(f, pts1, pts2, b, M, thr2, mask);
  }
  ransac_store_winner(s, st, b, M, f, count, F, mask, n_inliers, status, refined);
}

// -------------------------------------------------------------------------------------------------- refit
// Normalised 8-point least squares over the winner's inliers (the segment's Hartley transforms), one workgroup per
// segment: the 9 x 9 normal matrix summed by the workgroup in a fixed order, its smallest eigenvector by cyclic
// Jacobi in LDS (lanes 0..8 rotate one row / column entry each), rank 2 by zeroing the smallest singular value of the
// 3 x 3 (one-sided Jacobi in registers, as k_triangulate2 does its 4 x 4), then re-scored with the same error rule.
// The refit replaces the winner only if its inlier count is not lower.
__global__ __launch_bounds__(256) void k_fund_refit(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                    const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                    double thr2, const double* __restrict__ T, double* __restrict__ F,
                                                    uint8_t* __restrict__ mask, int* __restrict__ n_inliers,
                                                    const int* __restrict__ status, int* __restrict__ refined) {
  __shared__ double s_red[4][45];
  __shared__ double s_A[9][9], s_V[9][9];
  const int s = blockIdx.x, tid = threadIdx.x;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  const int have = n_inliers[s];
  if (status[s] != 0 || have < 8) return;                // uniform; refined[s] stays 0
  const double* t = T + 6 * (int64_t)s;
  double acc[45];
#pragma unroll
  for (int k = 0; k < 45; ++k) acc[k] = 0.0;
  for (int i = tid; i < M; i += 256) {
    if (!mask[b + i]) continue;
    const float2 p = pts1[b + i], q = pts2[b + i];
    const double xa = ((double)p.x - t[1]) * t[0], xb = ((double)p.y - t[2]) * t[0];
    const double xc = ((double)q.x - t[4]) * t[3], xd = ((double)q.y - t[5]) * t[3];
    const double r[9] = {xc * xa, xc * xb, xc, xd * xa, xd * xb, xd, xa, xb, 1.0};
    int k = 0;
#pragma unroll
    for (int u = 0; u < 9; ++u)
#pragma unroll
      for (int v = u; v < 9; ++v) acc[k++] += r[u] * r[v];
  }
  normal9_eigen(acc, s_red, s_A, s_V);
  const int kmin = smallest_diagonal9(s_A);
  double U[3][3], V[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) { U[r][c] = s_V[3 * r + c][kmin]; V[r][c] = (r == c) ? 1.0 : 0.0; }
  double fn[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) fn[3 * r + c] = U[r][c];
  const double eps = 10.0 * DBL_EPSILON;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool changed = false;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        double a = 0.0, bq = 0.0, g = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) { a += U[r][p] * U[r][p]; bq += U[r][q] * U[r][q]; g += U[r][p] * U[r][q]; }
        if (fabs(g) > eps * sqrt(a * bq)) {
          changed = true;
          const double zeta = (bq - a) / (2.0 * g);
          const double tt = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + tt * tt), sn = c * tt;
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            const double up = U[r][p], uq = U[r][q];
            U[r][p] = c * up - sn * uq; U[r][q] = sn * up + c * uq;
            const double vp = V[r][p], vq = V[r][q];
            V[r][p] = c * vp - sn * vq; V[r][q] = sn * vp + c * vq;
          }
        }
      }
    if (!changed) break;
  }
  // Fn = U V^T (U's columns carry the singular values); drop the column pair of the smallest one
  double nrm[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) nrm[k] = U[0][k] * U[0][k] + U[1][k] * U[1][k] + U[2][k] * U[2][k];
  const bool m1 = nrm[1] < nrm[0];
  const double n01 = m1 ? nrm[1] : nrm[0];
  const bool m2 = nrm[2] < n01;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double ur = m2 ? U[r][2] : (m1 ? U[r][1] : U[r][0]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double vc = m2 ? V[c][2] : (m1 ? V[c][1] : V[c][0]);
      fn[3 * r + c] -= ur * vc;
    }
  }
  double f[9];
  sevenpt::denormalise(fn, t, f);
  bool good = true;
#pragma unroll
  for (int e = 0; e < 9; ++e) good = good && isfinite(f[e]);
  if (!good) return;                                     // uniform: every thread computed the same f
  scale_last_to_one(f);
  ransac_keep_refit(s, have, f, [&](uint8_t* m) { return fund_count(f, pts1, pts2, b, M, thr2, m); }, F, mask, n_inliers,
                    refined);
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int sfm_fund_workspace_bytes(int64_t n_points, int32_t n_seg, int32_t n_hyp, int64_t* bytes_host) {
  if (!bytes_host || n_points < 0 || n_seg < 0 || n_hyp < 1) return SFM_ERR_ARG;
  *bytes_host = model9_layout(nullptr, n_seg, n_hyp).bytes;
  return SFM_OK;
}

extern "C" int sfm_fund_draw_samples(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, int32_t n_hyp, uint64_t seed,
                                     int32_t* samples) {
  return ransac_draw_samples<7, 7>(h, "sfm_fund_draw_samples", seg_ptr, n_seg, n_hyp, seed, samples);
}

extern "C" int sfm_fund_ransac(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, const float* pts1, const float* pts2,
                               int64_t n, const int32_t* samples, int32_t n_hyp, double threshold, int32_t refine,
                               double* F, uint8_t* mask, int32_t* n_inliers, int32_t* status, int32_t* hyp_count,
                               int32_t* refined, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  if (ransac_bad_args(n, n_seg, n_hyp, threshold)) return sfm_fail(h, SFM_ERR_ARG, "sfm_fund_ransac", "bad argument");
  if (n == 0 || n_seg == 0) return SFM_OK;
  if (!seg_ptr || !pts1 || !pts2 || !samples || !F || !mask || !n_inliers || !status || !workspace)
    return sfm_fail(h, SFM_ERR_ARG, "sfm_fund_ransac", "null pointer");
  const model9_ws w = model9_layout(workspace, n_seg, n_hyp);
  if (workspace_bytes < w.bytes) return sfm_fail(h, SFM_ERR_WORKSPACE, "sfm_fund_ransac", "workspace too small");
  int* counts = hyp_count ? hyp_count : w.hyp_count;
  const double thr2 = threshold * threshold;
  const float2* p1 = (const float2*)pts1;
  const float2* p2 = (const float2*)pts2;
  const int nblk = (n_hyp + 255) / 256;
  SFM_HIP(h, hipMemsetAsync(mask, 0, (size_t)n, h->stream));    // matches outside every segment
  hipLaunchKernelGGL(k_hartley_normalise<256>, dim3(n_seg), dim3(256), 0, h->stream, seg_ptr, n, p1, p2, w.T);
  sfm_prof_begin(h, SFM_PROF_FUND_HYP);
  hipLaunchKernelGGL(k_fund_hypotheses, dim3((unsigned)n_seg * nblk), dim3(256), 0, h->stream, seg_ptr, n, p1, p2,
                     samples, n_hyp, nblk, thr2, (const double*)w.T, counts, w.hyp_model);
  sfm_prof_end(h, SFM_PROF_FUND_HYP);
  hipLaunchKernelGGL(k_fund_select, dim3(n_seg), dim3(256), 0, h->stream, seg_ptr, n, p1, p2, n_hyp, thr2,
                     (const int*)counts, (const double*)w.hyp_model, F, mask, n_inliers, status, refined);
  if (refine)
    hipLaunchKernelGGL(k_fund_refit, dim3(n_seg), dim3(256), 0, h->stream, seg_ptr, n, p1, p2, thr2,
                       (const double*)w.T, F, mask, n_inliers, (const int*)status, refined);
  SFM_LAUNCH_CHECK(h, "sfm_fund_ransac");
  return SFM_OK;
}
