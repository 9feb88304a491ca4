// Homography RANSAC for every image pair of a step in one call (gfx950 only): cv2.findHomography(pts1, pts2, cv2.RANSAC,
// 3.0), the one two-view call of the usual set that twoview.hip (F), essential.hip (E) and pose.hip (recoverPose) left
// out.  Its first consumer is the guard of the incremental loop's initial pair: a pair whose matches lie on a plane, or
// whose cameras share a centre, has no defined F, and a homography explains nearly all of its matches.
//
// Structure as OpenCV's is RECALLED (its source is not pinned here): minimal samples of 4, a subset check that turns
// down collinear and orientation-reversing samples, the DLT on normalised coordinates, the forward transfer error
// |H x1 - x2|^2 <= threshold^2, most inliers wins, H scaled to H[2][2] = 1.  Deviations, on purpose: a FIXED number of
// hypotheses (no early exit on confidence); the stateless hash sampler of the other stages with 4 slots
// (k_ransac_samples<4, 4>); the error rule without its division (homography_rule.h); the refit is the normalised DLT
// over the winner's inliers and NO Levenberg-Marquardt step follows it, where OpenCV polishes the reprojection error.
// So the result is a function of (points, samples) alone, bitwise, run to run and independent of the batch, and a
// NumPy reference can follow the device hypothesis by hypothesis (tests/homography_reference.py).
//
// The kernels mirror twoview.hip's one for one:
//   k_hartley_normalise  (ransac_kernels.h, shared with sfm_fund_ransac) the segment's transforms over its finite matches
//   k_hom_hypotheses     one lane per (segment, hypothesis), 256 hypotheses of ONE segment per workgroup: the sample
//                        rule and the solver of homography_solve.h, one candidate per lane in registers, the segment's
//                        matches staged through LDS and read back as broadcasts (for_each_staged_point, epipolar_rule.h)
//   k_hom_select         the winner (ransac_winner, 4 minimum points), scaled, its mask and count
//   k_hom_refit          refine != 0 and at least 4 inliers: both rows of every inlier go into the 45 unique entries of
//                        the 9 x 9 normal matrix, smallest eigenvector (normal9_eigen), denormalised, scaled,
//                        re-scored with the same rule; it replaces the winner only if its count is not lower
//
// All arithmetic in float64.  Points arrive as float32 pixels [n][2] with a device seg_ptr[n_seg+1] (int64).  A match
// with a NaN or infinite coordinate is left out of the Hartley statistics and is staged as NaN for the scoring, so it
// fails every comparison; a sample that holds one gives no model.  Sample indices are range-checked on the device
// before they index anything.  Nothing synchronises the host.
#include "ransac_kernels.h"
#include "epipolar_rule.h"
#include "homography_rule.h"
#include "homography_solve.h"

namespace {

constexpr int HOM_MIN = 4;

__global__ __launch_bounds__(256) void k_hom_hypotheses(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                        const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                        const int* __restrict__ samples, int H, int nblk, double thr2,
                                                        const double* __restrict__ T, int* __restrict__ hyp_count,
                                                        double* __restrict__ hyp_H) {
  __shared__ double2 s_pt[2 * FUND_CHUNK];
  const int s = blockIdx.x / nblk;
  const int hyp = (blockIdx.x % nblk) * 256 + threadIdx.x;
  const bool active = hyp < H;
  const int64_t slot = (int64_t)s * H + hyp;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  if (M < HOM_MIN) {                                     // uniform over the workgroup
    if (active) {
      hyp_count[slot] = 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) hyp_H[slot * 9 + k] = 0.0;
    }
    return;
  }
  double Hc[9];
  {
    float px[4][4];
    const bool ok = load_sample<4>(samples, slot, active, M, b, pts1, pts2, px);
    double h[9];
    const bool good = homog::solve_sample(px, T + 6 * (int64_t)s, h) && ok;
#pragma unroll
    for (int e = 0; e < 9; ++e) Hc[e] = good ? h[e] : 0.0;
  }
  // scoring: every lane walks all points of the segment with its candidate in registers
  int count = 0;
  for_each_staged_point(s_pt, pts1, pts2, b, M, [&](double2 p, double2 q) {
    count += hom_inlier(Hc, p.x, p.y, q.x, q.y, thr2) ? 1 : 0;
  });
  if (!active) return;
  hyp_count[slot] = count;
#pragma unroll
  for (int e = 0; e < 9; ++e) hyp_H[slot * 9 + e] = Hc[e];
}

// ---------------------------------------------------------------------------------------------- selection
// inliers of h over the whole segment (every thread takes its own points); writes the mask when `mask` is not null
__device__ __forceinline__ int hom_count(const double (&h)[9], const float2* __restrict__ pts1,
                                         const float2* __restrict__ pts2, int64_t b, int M, double thr2,
                                         uint8_t* __restrict__ mask) {
  return segment_count(b, M, mask, [&](int64_t i) {
    const float2 p = pts1[i], q = pts2[i];
    return finite4(p, q) && hom_inlier(h, (double)p.x, (double)p.y, (double)q.x, (double)q.y, thr2);
  });
}

// winner per segment (ransac_winner): its H scaled to H[2][2] = 1, its mask and its count
__global__ __launch_bounds__(256) void k_hom_select(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                    const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                    int H, double thr2, const int* __restrict__ hyp_count,
                                                    const double* __restrict__ hyp_H, double* __restrict__ Hout,
                                                    uint8_t* __restrict__ mask, int* __restrict__ n_inliers,
                                                    int* __restrict__ status, int* __restrict__ refined) {
  const int s = blockIdx.x;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  int hp;
  const int st = ransac_winner(hyp_count, s, H, M, HOM_MIN, hp);
  double h[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) h[e] = 0.0;
  int count = 0;
  if (st == 0) {                                         // uniform over the workgroup
#pragma unroll
    for (int e = 0; e < 9; ++e) h[e] = hyp_H[((int64_t)s * H + hp) * 9 + e];
    scale_last_to_one(h);
    count = hom_count(h, pts1, pts2, b, M, thr2, mask);
  }
  ransac_store_winner(s, st, b, M, h, count, Hout, mask, n_inliers, status, refined);
}

// -------------------------------------------------------------------------------------------------- refit
// Normalised DLT over the winner's inliers (the segment's Hartley transforms), one workgroup per segment: the 9 x 9
// normal matrix of the two rows of every inlier summed by the workgroup in a fixed order, its smallest eigenvector by
// cyclic Jacobi in LDS, denormalised, scaled, then re-scored with the same error rule.  The refit replaces the winner
// only if its inlier count is not lower.
__global__ __launch_bounds__(256) void k_hom_refit(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                   const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                   double thr2, const double* __restrict__ T, double* __restrict__ Hout,
                                                   uint8_t* __restrict__ mask, int* __restrict__ n_inliers,
                                                   const int* __restrict__ status, int* __restrict__ refined) {
  __shared__ double s_red[4][45];
  __shared__ double s_A[9][9], s_V[9][9];
  const int s = blockIdx.x, tid = threadIdx.x;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  const int have = n_inliers[s];
  if (status[s] != 0 || have < HOM_MIN) return;          // uniform; refined[s] stays 0
  const double* t = T + 6 * (int64_t)s;
  double acc[45];
#pragma unroll
  for (int k = 0; k < 45; ++k) acc[k] = 0.0;
  for (int i = tid; i < M; i += 256) {
    if (!mask[b + i]) continue;
    const float2 p = pts1[b + i], q = pts2[b + i];
    const double xa = ((double)p.x - t[1]) * t[0], xb = ((double)p.y - t[2]) * t[0];
    const double xc = ((double)q.x - t[4]) * t[3], xd = ((double)q.y - t[5]) * t[3];
    const double r0[9] = {xa, xb, 1.0, 0.0, 0.0, 0.0, -xc * xa, -xc * xb, -xc};
    const double r1[9] = {0.0, 0.0, 0.0, xa, xb, 1.0, -xd * xa, -xd * xb, -xd};
    int k = 0;
#pragma unroll
    for (int u = 0; u < 9; ++u)
#pragma unroll
      for (int v = u; v < 9; ++v) acc[k++] += r0[u] * r0[v] + r1[u] * r1[v];
  }
  normal9_eigen(acc, s_red, s_A, s_V);
  const int kmin = smallest_diagonal9(s_A);
  double hn[9], h[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) hn[e] = s_V[e][kmin];
  homog::denormalise(hn, t, h);
  bool good = true;
#pragma unroll
  for (int e = 0; e < 9; ++e) good = good && isfinite(h[e]);
  if (!good) return;                                     // uniform: every thread computed the same h
  scale_last_to_one(h);
  ransac_keep_refit(s, have, h, [&](uint8_t* m) { return hom_count(h, pts1, pts2, b, M, thr2, m); }, Hout, mask,
                    n_inliers, refined);
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int sfm_hom_workspace_bytes(int64_t n_points, int32_t n_seg, int32_t n_hyp, int64_t* bytes_host) {
  if (!bytes_host || n_points < 0 || n_seg < 0 || n_hyp < 1) return SFM_ERR_ARG;
  *bytes_host = model9_layout(nullptr, n_seg, n_hyp).bytes;
  return SFM_OK;
}

extern "C" int sfm_hom_draw_samples(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, int32_t n_hyp, uint64_t seed,
                                    int32_t* samples) {
  return ransac_draw_samples<4, 4>(h, "sfm_hom_draw_samples", seg_ptr, n_seg, n_hyp, seed, samples);
}

extern "C" int sfm_hom_ransac(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, const float* pts1, const float* pts2,
                              int64_t n, const int32_t* samples, int32_t n_hyp, double threshold, int32_t refine,
                              double* H, uint8_t* mask, int32_t* n_inliers, int32_t* status, int32_t* hyp_count,
                              int32_t* refined, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  if (ransac_bad_args(n, n_seg, n_hyp, threshold)) return sfm_fail(h, SFM_ERR_ARG, "sfm_hom_ransac", "bad argument");
  if (n == 0 || n_seg == 0) return SFM_OK;
  if (!seg_ptr || !pts1 || !pts2 || !samples || !H || !mask || !n_inliers || !status || !workspace)
    return sfm_fail(h, SFM_ERR_ARG, "sfm_hom_ransac", "null pointer");
  const model9_ws w = model9_layout(workspace, n_seg, n_hyp);
  if (workspace_bytes < w.bytes) return sfm_fail(h, SFM_ERR_WORKSPACE, "sfm_hom_ransac", "workspace too small");
  int* counts = hyp_count ? hyp_count : w.hyp_count;
  const double thr2 = threshold * threshold;
  const float2* p1 = (const float2*)pts1;
  const float2* p2 = (const float2*)pts2;
  const int nblk = (n_hyp + 255) / 256;
  SFM_HIP(h, hipMemsetAsync(mask, 0, (size_t)n, h->stream));    // matches outside every segment
  hipLaunchKernelGGL(k_hartley_normalise<256>, dim3(n_seg), dim3(256), 0, h->stream, seg_ptr, n, p1, p2, w.T);
  sfm_prof_begin(h, SFM_PROF_HOM_HYP);
  hipLaunchKernelGGL(k_hom_hypotheses, dim3((unsigned)n_seg * nblk), dim3(256), 0, h->stream, seg_ptr, n, p1, p2,
                     samples, n_hyp, nblk, thr2, (const double*)w.T, counts, w.hyp_model);
  sfm_prof_end(h, SFM_PROF_HOM_HYP);
  hipLaunchKernelGGL(k_hom_select, dim3(n_seg), dim3(256), 0, h->stream, seg_ptr, n, p1, p2, n_hyp, thr2,
                     (const int*)counts, (const double*)w.hyp_model, H, mask, n_inliers, status, refined);
  if (refine)
    hipLaunchKernelGGL(k_hom_refit, dim3(n_seg), dim3(256), 0, h->stream, seg_ptr, n, p1, p2, thr2,
                       (const double*)w.T, H, mask, n_inliers, (const int*)status, refined);
  SFM_LAUNCH_CHECK(h, "sfm_hom_ransac");
  return SFM_OK;
}
