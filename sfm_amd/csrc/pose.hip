// Relative-pose recovery for every image pair of a step in one call (gfx950 only): the
// cv2.recoverPose(E, pts1, pts2, K) call of the reference's find_best_initial_pair / initialize_reconstruction
// (sfm_reconstruction.py:61-155) and the cv2.triangulatePoints call that follows it for the winner.
//
// Semantics as opencv-python 4.11's recoverPose / decomposeEssentialMat are RECALLED (their source is not pinned here;
// what pins this row is the reference's own shipped run, tests/pose_reference.py):
//   points      float32 pixels, widened to double and normalised with the inverse of K = (fx, fy, cx, cy), skew 0:
//               x = (u - cx) / fx, y = (v - cy) / fy
//   decompose   E = U S V^T, det U = det V^T = +1, R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2]; four candidates
//               [R1|t], [R2|t], [R1|-t], [R2|-t] (jacobi::decompose_essential, pose_solve.h).  Their order follows the sign
//               choices of the decomposition: it is this kernel's own, not cv2's, so a TIE between candidates may be
//               resolved differently from cv2.
//   vote        every point is triangulated against P0 = [I|0] and the candidate by the DLT of k_triangulate2
//               (jacobi::dlt2); good <=> Q.z Q.w > 0 and X.z < dist and 0 < z2 < dist with X = Q / Q.w and z2 the depth of
//               X in the second camera, and the point's byte of mask_in is not zero.  A point with a NaN or infinite
//               coordinate is never good (anything non-finite compares false).
//   winner      the first candidate with the largest count.
// One segment is one image pair: seg_ptr [n_seg+1] device int64 (the convention of sfm_fund_ransac), pts1 / pts2 [n][2]
// float32 pixels, EorF [n_seg][9] float64 row-major, Kseg [n_seg][4] float64 as sfm_pnp_ransac takes it.  Nothing goes
// back to the host between the stages.  No FMA contraction anywhere in this file.
#include "ransac_kernels.h"
#include "pose_solve.h"

#pragma clang fp contract(off)

namespace {

// largest s in [0, n_seg) with ptr[s] <= i (skips empty segments); the caller checks i against seg_range(s)
__device__ __forceinline__ int pose_seg_of(const int64_t* __restrict__ ptr, int n_seg, int64_t i) {
  int lo = 0, hi = n_seg;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ptr[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------- decompose
// One lane per segment: E (or K^T F K), its four [R|t] into cand_pose, the status.  A segment without a model gets NaN
// poses, so that every comparison of the vote is false for it; its counts stay 0.
__global__ __launch_bounds__(256) void k_pose_decompose(const int64_t* __restrict__ seg_ptr, int n_seg, int64_t n,
                                                        const double* __restrict__ EorF, int is_fundamental,
                                                        const double* __restrict__ Kseg, double* __restrict__ cand_pose,
                                                        int* __restrict__ cand_count, int* __restrict__ status) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_seg) return;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  double E[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) E[k] = EorF[9 * (int64_t)s + k];
  if (is_fundamental) {                                  // E = K^T F K, K = [[fx,0,cx],[0,fy,cy],[0,0,1]]
    const auto [fx, fy, cx, cy] = load_k4(Kseg, s);
    double G[9];                                         // G = K^T F
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      G[c] = fx * E[c];
      G[3 + c] = fy * E[3 + c];
      G[6 + c] = cx * E[c] + cy * E[3 + c] + E[6 + c];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      E[3 * r] = G[3 * r] * fx;
      E[3 * r + 1] = G[3 * r + 1] * fy;
      E[3 * r + 2] = G[3 * r] * cx + G[3 * r + 1] * cy + G[3 * r + 2];
    }
  }
  double Rt[4][12];
  const double nan = __builtin_nan("");
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int e = 0; e < 12; ++e) Rt[c][e] = nan;
  const bool ok = jacobi::decompose_essential(E, Rt);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
#pragma unroll
    for (int e = 0; e < 12; ++e) cand_pose[((int64_t)s * 4 + c) * 12 + e] = Rt[c][e];
    cand_count[4 * (int64_t)s + c] = 0;
  }
  status[s] = (M == 0) ? 1 : (ok ? 0 : 2);
}

// --------------------------------------------------------------------------------------------------- vote
// One lane per point of the whole batch, all four candidates of its segment in turn.  good4[i] gets one bit per
// candidate; the counts are integer sums into cand_count [n_seg][4] (zeroed by k_pose_decompose): a wave whose lanes all
// belong to one segment adds its four population counts with one atomicAdd each, a wave that straddles a segment
// boundary adds lane by lane.  Integer sums: the result does not depend on the order.
__global__ __launch_bounds__(256) void k_pose_vote(const int64_t* __restrict__ seg_ptr, int n_seg, int64_t n,
                                                   const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                   const double* __restrict__ Kseg, const uint8_t* __restrict__ mask_in,
                                                   double dist, const double* __restrict__ cand_pose,
                                                   int* __restrict__ cand_count, uint8_t* __restrict__ good4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int s = -1;
  bool active = i < n;
  if (active) {
    s = pose_seg_of(seg_ptr, n_seg, i);
    int64_t b; int M;
    seg_range(seg_ptr, s, n, b, M);
    active = i >= b && i < b + M;                        // a point outside every segment takes no part
    if (!active) s = -1;
  }
  unsigned bits = 0;
  if (active) {
    const auto [fx, fy, cx, cy] = load_k4(Kseg, s);
    const float2 a = pts1[i], c2 = pts2[i];
    const double x0 = ((double)a.x - cx) / fx, y0 = ((double)a.y - cy) / fy;
    const double x1 = ((double)c2.x - cx) / fx, y1 = ((double)c2.y - cy) / fy;
    const bool use = isfinite(x0) && isfinite(y0) && isfinite(x1) && isfinite(y1) && (!mask_in || mask_in[i] != 0);
    const double P0[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    if (use) {
      for (int c = 0; c < 4; ++c) {
        const double* __restrict__ src = cand_pose + ((int64_t)s * 4 + c) * 12;
        double P1[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) P1[e] = src[e];
        double q[4];
        jacobi::dlt2(P0, P1, x0, y0, x1, y1, q);
        const double Xx = q[0] / q[3], Xy = q[1] / q[3], Xz = q[2] / q[3];
        const double z2 = P1[8] * Xx + P1[9] * Xy + P1[10] * Xz + P1[11];
        const bool good = (q[2] * q[3] > 0.0) && (Xz < dist) && (z2 > 0.0) && (z2 < dist);
        bits |= (good ? 1u : 0u) << c;
      }
    }
    good4[i] = (uint8_t)bits;
  }
  // s = -1 marks a lane without a point; a wave whose lane 0 has none adds lane by lane
  const int s0 = __shfl(s, 0);
  const bool uniform = __all(!active || s == s0) && s0 >= 0;
  if (uniform) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int cnt = __popcll(__ballot((bits >> c) & 1u));
      if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&cand_count[4 * (int64_t)s0 + c], cnt);
    }
  } else if (active) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if ((bits >> c) & 1u) atomicAdd(&cand_count[4 * (int64_t)s + c], 1);
  }
}

// ------------------------------------------------------------------------------------------------- select
// One lane per segment: the first candidate with the largest count, its pose and count.  Without a model (or without
// points) the pose is zero, the count 0 and the winner 0.
__global__ __launch_bounds__(256) void k_pose_select(int n_seg, const int* __restrict__ cand_count,
                                                     const double* __restrict__ cand_pose, const int* __restrict__ status,
                                                     double* __restrict__ R, double* __restrict__ t,
                                                     int* __restrict__ n_good, int* __restrict__ winner) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_seg) return;
  int best = cand_count[4 * (int64_t)s], w = 0;
#pragma unroll
  for (int c = 1; c < 4; ++c) {
    const int v = cand_count[4 * (int64_t)s + c];
    if (v > best) { best = v; w = c; }
  }
  const bool ok = status[s] == 0;
  if (!ok) { best = 0; w = 0; }
  const double* __restrict__ src = cand_pose + ((int64_t)s * 4 + w) * 12;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) R[9 * (int64_t)s + 3 * r + c] = ok ? src[4 * r + c] : 0.0;
    t[3 * (int64_t)s + r] = ok ? src[4 * r + 3] : 0.0;
  }
  n_good[s] = best;
  winner[s] = w;
}

// ------------------------------------------------------------------------------------------------- finish
// One lane per point: the winner's mask byte (255 / 0, as OpenCV's comparison writes it) and, when X is given, the
// winner's good points triangulated again in PIXEL coordinates with K [I|0] and K [R|t] - what the reference's
// initialize_reconstruction stores.  The DLT is not invariant to the scaling of its rows, so this is not the point of
// the vote.  Points outside the mask, or outside every segment, get NaN.
__global__ __launch_bounds__(256) void k_pose_finish(const int64_t* __restrict__ seg_ptr, int n_seg, int64_t n,
                                                     const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                     const double* __restrict__ Kseg, const uint8_t* __restrict__ good4,
                                                     const int* __restrict__ winner, const int* __restrict__ status,
                                                     const double* __restrict__ cand_pose, uint8_t* __restrict__ mask_out,
                                                     double* __restrict__ X) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = pose_seg_of(seg_ptr, n_seg, i);
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  const bool inside = i >= b && i < b + M;
  const int w = winner[s] & 3;
  const bool good = inside && status[s] == 0 && ((good4[i] >> w) & 1);
  mask_out[i] = good ? 255 : 0;
  if (!X) return;
  const double nan = __builtin_nan("");
  double Xx = nan, Xy = nan, Xz = nan;
  if (good) {
    const auto [fx, fy, cx, cy] = load_k4(Kseg, s);
    const double* __restrict__ src = cand_pose + ((int64_t)s * 4 + w) * 12;
    const double P0[12] = {fx, 0.0, cx, 0.0, 0.0, fy, cy, 0.0, 0.0, 0.0, 1.0, 0.0};
    double P1[12];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      P1[e] = fx * src[e] + cx * src[8 + e];
      P1[4 + e] = fy * src[4 + e] + cy * src[8 + e];
      P1[8 + e] = src[8 + e];
    }
    const float2 a = pts1[i], c2 = pts2[i];
    double q[4];
    jacobi::dlt2(P0, P1, (double)a.x, (double)a.y, (double)c2.x, (double)c2.y, q);
    Xx = q[0] / q[3]; Xy = q[1] / q[3]; Xz = q[2] / q[3];
  }
  X[3 * i] = Xx; X[3 * i + 1] = Xy; X[3 * i + 2] = Xz;
}

struct pose_ws {
  double* cand_pose;
  int* cand_count;
  int* winner;
  uint8_t* good4;
  int64_t bytes;
};

pose_ws pose_layout(void* workspace, int64_t n, int32_t n_seg) {
  ws_carve c{(char*)workspace};
  pose_ws w;
  w.cand_pose = c.take<double>((int64_t)n_seg * 4 * 12);
  w.cand_count = c.take<int>((int64_t)n_seg * 4);
  w.winner = c.take<int>(n_seg);
  w.good4 = c.take<uint8_t>(n);
  w.bytes = c.bytes();
  return w;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int sfm_pose_workspace_bytes(int64_t n_points, int32_t n_seg, int64_t* bytes_host) {
  if (!bytes_host || n_points < 0 || n_seg < 0) return SFM_ERR_ARG;
  *bytes_host = pose_layout(nullptr, n_points, n_seg).bytes;
  return SFM_OK;
}

extern "C" int sfm_pose_recover(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, const float* pts1, const float* pts2,
                                int64_t n, const double* EorF, int32_t is_fundamental, const double* Kseg,
                                const uint8_t* mask_in, double dist, double* R, double* t, int32_t* n_good,
                                int32_t* status, uint8_t* mask_out, double* X, int32_t* cand_count, double* cand_pose,
                                int32_t* winner, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  if (n < 0 || n_seg < 0 || dist != dist) return sfm_fail(h, SFM_ERR_ARG, "sfm_pose_recover", "bad argument");
  if (n_seg == 0) return SFM_OK;
  if (!seg_ptr || !EorF || !Kseg || !R || !t || !n_good || !status || !workspace ||
      (n > 0 && (!pts1 || !pts2 || !mask_out)))
    return sfm_fail(h, SFM_ERR_ARG, "sfm_pose_recover", "null pointer");
  const pose_ws w = pose_layout(workspace, n, n_seg);
  if (workspace_bytes < w.bytes) return sfm_fail(h, SFM_ERR_WORKSPACE, "sfm_pose_recover", "workspace too small");
  int* counts = cand_count ? cand_count : w.cand_count;
  double* poses = cand_pose ? cand_pose : w.cand_pose;
  int* win = winner ? winner : w.winner;
  const float2* p1 = (const float2*)pts1;
  const float2* p2 = (const float2*)pts2;
  hipLaunchKernelGGL(k_pose_decompose, dim3(cdiv(n_seg, 256)), dim3(256), 0, h->stream, seg_ptr, n_seg, n, EorF,
                     (int)is_fundamental, Kseg, poses, counts, status);
  if (n > 0) {
    sfm_prof_begin(h, SFM_PROF_POSE_VOTE);
    hipLaunchKernelGGL(k_pose_vote, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, seg_ptr, n_seg, n, p1, p2, Kseg, mask_in,
                       dist, (const double*)poses, counts, w.good4);
    sfm_prof_end(h, SFM_PROF_POSE_VOTE);
  }
  hipLaunchKernelGGL(k_pose_select, dim3(cdiv(n_seg, 256)), dim3(256), 0, h->stream, n_seg, (const int*)counts,
                     (const double*)poses, (const int*)status, R, t, n_good, win);
  if (n > 0)
    hipLaunchKernelGGL(k_pose_finish, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, seg_ptr, n_seg, n, p1, p2, Kseg,
                       (const uint8_t*)w.good4, (const int*)win, (const int*)status, (const double*)poses, mask_out, X);
  SFM_LAUNCH_CHECK(h, "sfm_pose_recover");
  return SFM_OK;
}
