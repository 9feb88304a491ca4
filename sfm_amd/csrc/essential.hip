// Essential-matrix RANSAC for every image pair of a step in one call (gfx950 only): cv2.findEssentialMat(pts1, pts2, K,
// cv2.RANSAC, threshold = 3.0), the calibrated counterpart of twoview.hip.  K is known everywhere in this project, and
// E = K^T F K of a 7-point F is not an essential matrix (its two singular values differ by up to a factor of two on the
// shipped pairs): a pose taken from it leaves reprojection errors of many pixels.
//
// Structure as OpenCV's is RECALLED (its source is not pinned here): minimal samples of 5 solved by Nister's five-point
// algorithm (essential_solve.h, up to 10 candidates per sample), most inliers wins.  Deviations, on purpose: the error
// rule is that of twoview.hip, in PIXELS on F = K^-T E K^-1 (fund_inlier, epipolar_rule.h: the larger of the two
// squared point-to-epipolar-line distances <= threshold^2), not a Sampson distance in normalised coordinates; a FIXED
// number of hypotheses; the stateless hash sampler of the other stages with 5 slots (k_ransac_samples<5, 5>) - so the
// result is a function of (points, K, samples) alone, bitwise, run to run and independent of the batch, and a NumPy
// reference can follow the device hypothesis by hypothesis (tests/essential_reference.py).
//
//   k_ess_solve   one lane per (segment, hypothesis), workgroups of ONE wave: the 10 x 20 system of the solver lies in
//                 LDS, lane-interleaved as [element][lane] (a wave's ds_read_b64 covers 512 contiguous bytes), 100 KiB.
//                 The candidates go to the workspace as E (normalised coordinates, |E|_F = sqrt(2), sign fixed), packed
//                 to the front of the hypothesis's 10 slots, with their number cand_n beside them.  Slots at or past
//                 cand_n are never written and never read: what the workspace holds there is undefined.
//   k_ess_score   a workgroup of 256 lanes serves ONE segment: 25 hypotheses x 10 slots, one lane each, F = K^-T E K^-1
//                 in registers, the segment's matches staged through LDS in chunks and read back as broadcasts (as
//                 k_fund_hypotheses does).  A slot past the hypothesis's number holds F = 0 and never counts.  The count
//                 of a hypothesis is the largest of its slots, ties to the lowest slot.
//   k_ess_select  per segment the winner (ransac_winner: most inliers, ties to the lowest hypothesis), its mask and count.
//   k_ess_refit   refine != 0: the same solver over ALL inliers of the winner.  The 45 entries of A^T A are summed in a
//                 fixed order, the four eigenvectors of its smallest eigenvalues (normal9_eigen, shared with
//                 k_fund_refit) stand in for the null space, lane 0 runs steps 4 to 7, every candidate is scored
//                 over the whole segment by the workgroup, and the best (ties: the first) replaces the winner only if
//                 its count is not lower; refined[s] = 1 then.
//
// Rules.  All arithmetic in float64; points arrive as float32 pixels [n][2] with a device seg_ptr[n_seg+1] (int64), Kseg
// [n_seg][4] = (fx, fy, cx, cy).  Segments with fewer than 5 matches get status 1.  A hypothesis gives no model if its
// sample holds a non-finite coordinate or an index outside the segment, or if two matches of its sample share a pixel
// in image 1 or share a pixel in image 2 (float32 == on both coordinates; see essential_solve.h for why).  A match with
// a non-finite coordinate is never an inlier.  Status 2: no hypothesis gave an inlier.  Status 1 / 2 segments get E = 0,
// an all-zero mask and count 0.  The returned E is in normalised coordinates, |E|_F = sqrt(2), its entry of largest
// magnitude (the first on a tie) positive.
#include "ransac_kernels.h"
#include "epipolar_rule.h"
#include "essential_solve.h"

namespace {

constexpr int ESS_SLOTS = fivept::MAX_CANDIDATES;
constexpr int ESS_HYP_PER_BLOCK = 25;                      // k_ess_score: 25 x 10 = 250 of the 256 lanes
static_assert(ESS_HYP_PER_BLOCK * ESS_SLOTS <= 256, "one lane per (hypothesis, slot)");

// F = K^-T E K^-1, K = [fx 0 cx; 0 fy cy; 0 0 1]; written out so that the three kernels that form it round alike
__device__ __forceinline__ void make_F(double fx, double fy, double cx, double cy, const double (&E)[9], double (&F)[9]) {
#pragma clang fp contract(off)
  const double a = 1.0 / fx, b = 1.0 / fy, c = -cx / fx, d = -cy / fy;
  double G[9];                                             // E K^-1
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    G[3 * r] = E[3 * r] * a;
    G[3 * r + 1] = E[3 * r + 1] * b;
    G[3 * r + 2] = fma(E[3 * r], c, fma(E[3 * r + 1], d, E[3 * r + 2]));
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    F[j] = a * G[j];
    F[3 + j] = b * G[3 + j];
    F[6 + j] = fma(c, G[j], fma(d, G[3 + j], G[6 + j]));
  }
}

// ------------------------------------------------------------------------------------------------- solve
__global__ __launch_bounds__(64) void k_ess_solve(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                  const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                  const double* __restrict__ Kseg, const int* __restrict__ samples, int H,
                                                  int64_t total, int* __restrict__ cand_n, double* __restrict__ cand_E) {
  __shared__ double s_ws[fivept::WS_DOUBLES * 64];
  const int64_t g = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (g >= total) return;                                  // no barrier in this kernel
  const int s = (int)(g / H);
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  const fivept::strided<64> ws{s_ws + threadIdx.x};
  double Bs[4][9];
  int nc = 0;
  if (M >= 5) {
    float px[5][4];
    const bool ok = load_sample<5>(samples, g, true, M, b, pts1, pts2, px);
    const auto [fx, fy, cx, cy] = load_k4(Kseg, s);
    if (ok) nc = fivept::solve_sample(px, fx, fy, cx, cy, ws, Bs);
  }
  int filled = 0;
  for (int k = 0; k < nc; ++k) {
    double E[9];
    if (!fivept::candidate(Bs, ws, k, E)) continue;
#pragma unroll
    for (int e = 0; e < 9; ++e) cand_E[(g * ESS_SLOTS + filled) * 9 + e] = E[e];
    ++filled;
  }
  cand_n[g] = filled;
}

// ------------------------------------------------------------------------------------------------- score
__global__ __launch_bounds__(256) void k_ess_score(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                   const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                   const double* __restrict__ Kseg, int H, int nblk, double thr2,
                                                   const int* __restrict__ cand_n, const double* __restrict__ cand_E,
                                                   int* __restrict__ hyp_count, int* __restrict__ hyp_cand) {
  __shared__ double2 s_pt[2 * FUND_CHUNK];
  __shared__ int s_cnt[256];
  const int s = blockIdx.x / nblk, tid = threadIdx.x;
  const int hl = tid / ESS_SLOTS, slot = tid - ESS_SLOTS * hl;
  const int hyp = (blockIdx.x % nblk) * ESS_HYP_PER_BLOCK + hl;
  const bool lane = hl < ESS_HYP_PER_BLOCK && hyp < H;
  const int64_t g = (int64_t)s * H + hyp;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  if (M < 5) {                                             // uniform over the workgroup
    if (lane && slot == 0) { hyp_count[g] = 0; hyp_cand[g] = 0; }
    return;
  }
  double F[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) F[e] = 0.0;
  if (lane && slot < cand_n[g]) {
    double E[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = cand_E[(g * ESS_SLOTS + slot) * 9 + e];
    const auto [fx, fy, cx, cy] = load_k4(Kseg, s);
    make_F(fx, fy, cx, cy, E, F);
  }
  int cnt = 0;
  for_each_staged_point(s_pt, pts1, pts2, b, M, [&](double2 p, double2 q) {
    cnt += fund_inlier(F, p.x, p.y, q.x, q.y, thr2) ? 1 : 0;
  });
  s_cnt[tid] = cnt;
  __syncthreads();
  if (lane && slot == 0) {
    int best = cnt, cand = 0;                              // ties: the lowest slot
    for (int k = 1; k < ESS_SLOTS; ++k) {
      const int c = s_cnt[tid + k];
      if (c > best) { best = c; cand = k; }
    }
    hyp_count[g] = best;
    hyp_cand[g] = cand;
  }
}

// ---------------------------------------------------------------------------------------------- selection
__global__ __launch_bounds__(256) void k_ess_select(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                    const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                    const double* __restrict__ Kseg, int H, double thr2,
                                                    const int* __restrict__ hyp_count, const int* __restrict__ hyp_cand,
                                                    const double* __restrict__ cand_E, double* __restrict__ E_out,
                                                    uint8_t* __restrict__ mask, int* __restrict__ n_inliers,
                                                    int* __restrict__ status, int* __restrict__ refined) {
  const int s = blockIdx.x;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  int hp;
  const int st = ransac_winner(hyp_count, s, H, M, 5, hp);
  double E[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) E[e] = 0.0;
  int count = 0;
  if (st == 0) {                                           // uniform over the workgroup
    const int64_t g = (int64_t)s * H + hp;
    const int cand = hyp_cand[g];                          // a winner has a count > 0, so its slot lies below cand_n[g]
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = cand_E[(g * ESS_SLOTS + cand) * 9 + e];
    const auto [fx, fy, cx, cy] = load_k4(Kseg, s);
    double F[9];
    make_F(fx, fy, cx, cy, E, F);
    count = fund_count(F, pts1, pts2, b, M, thr2, mask);
  }
  ransac_store_winner(s, st, b, M, E, count, E_out, mask, n_inliers, status, refined);
}

// -------------------------------------------------------------------------------------------------- refit
__global__ __launch_bounds__(256) void k_ess_refit(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                   const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                   const double* __restrict__ Kseg, double thr2, double* __restrict__ E_out,
                                                   uint8_t* __restrict__ mask, int* __restrict__ n_inliers,
                                                   const int* __restrict__ status, int* __restrict__ refined) {
  __shared__ double s_red[4][45];
  __shared__ double s_A[9][9], s_V[9][9];
  __shared__ double s_ws[fivept::WS_DOUBLES];
  __shared__ double s_E[ESS_SLOTS][9];
  __shared__ int s_nc;
  const int s = blockIdx.x, tid = threadIdx.x;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  const int have = n_inliers[s];
  if (status[s] != 0 || have < 5) return;                  // uniform; refined[s] stays 0
  const auto [fx, fy, cx, cy] = load_k4(Kseg, s);
  double acc[45];
#pragma unroll
  for (int k = 0; k < 45; ++k) acc[k] = 0.0;
  for (int i = tid; i < M; i += 256) {
    if (!mask[b + i]) continue;
    const float2 p = pts1[b + i], q = pts2[b + i];
    const double xa = ((double)p.x - cx) / fx, xb = ((double)p.y - cy) / fy;
    const double xc = ((double)q.x - cx) / fx, xd = ((double)q.y - cy) / fy;
    const double r[9] = {xc * xa, xc * xb, xc, xd * xa, xd * xb, xd, xa, xb, 1.0};
    int k = 0;
#pragma unroll
    for (int u = 0; u < 9; ++u)
#pragma unroll
      for (int v = u; v < 9; ++v) acc[k++] += r[u] * r[v];
  }
  normal9_eigen(acc, s_red, s_A, s_V);
  if (tid == 0) {
    // the eigenvectors of the four smallest eigenvalues (ties: the lowest index), then steps 4 to 7 on one lane
    double Bs[4][9];
    unsigned used = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      int kmin = -1;
      for (int k = 0; k < 9; ++k)
        if (!((used >> k) & 1u) && (kmin < 0 || s_A[k][k] < s_A[kmin][kmin])) kmin = k;
      used |= 1u << kmin;
#pragma unroll
      for (int e = 0; e < 9; ++e) Bs[v][e] = s_V[e][kmin];
    }
    const fivept::strided<1> ws{s_ws};
    const int nc = fivept::solve_basis(Bs, ws);
    int filled = 0;
    for (int k = 0; k < nc; ++k) {
      double E[9];
      if (!fivept::candidate(Bs, ws, k, E)) continue;
#pragma unroll
      for (int e = 0; e < 9; ++e) s_E[filled][e] = E[e];
      ++filled;
    }
    s_nc = filled;
  }
  __syncthreads();
  const int nc = s_nc;
  int best = -1, bk = 0;
  double E[9], F[9];
  for (int k = 0; k < nc; ++k) {                           // uniform: every thread scores every candidate
#pragma unroll
    for (int e = 0; e < 9; ++e) E[e] = s_E[k][e];
    make_F(fx, fy, cx, cy, E, F);
    const int c = fund_count(F, pts1, pts2, b, M, thr2, nullptr);
    if (c > best) { best = c; bk = k; }
  }
  if (best < have) return;
#pragma unroll
  for (int e = 0; e < 9; ++e) E[e] = s_E[bk][e];
  make_F(fx, fy, cx, cy, E, F);
  (void)fund_count(F, pts1, pts2, b, M, thr2, mask);
  ransac_store_refit(s, E, best, E_out, n_inliers, refined);
}

struct ess_ws {
  double* cand_E;
  int* cand_n;
  int* hyp_count;
  int* hyp_cand;
  int64_t bytes;
};

ess_ws ess_layout(void* workspace, int32_t n_seg, int32_t n_hyp) {
  ws_carve c{(char*)workspace};
  ess_ws w;
  w.cand_E = c.take<double>((int64_t)n_seg * n_hyp * ESS_SLOTS * 9);
  w.cand_n = c.take<int>((int64_t)n_seg * n_hyp);
  w.hyp_count = c.take<int>((int64_t)n_seg * n_hyp);
  w.hyp_cand = c.take<int>((int64_t)n_seg * n_hyp);
  w.bytes = c.bytes();
  return w;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int sfm_ess_workspace_bytes(int64_t n_points, int32_t n_seg, int32_t n_hyp, int64_t* bytes_host) {
  if (!bytes_host || n_points < 0 || n_seg < 0 || n_hyp < 1) return SFM_ERR_ARG;
  *bytes_host = ess_layout(nullptr, n_seg, n_hyp).bytes;
  return SFM_OK;
}

extern "C" int sfm_ess_draw_samples(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, int32_t n_hyp, uint64_t seed,
                                    int32_t* samples) {
  return ransac_draw_samples<5, 5>(h, "sfm_ess_draw_samples", seg_ptr, n_seg, n_hyp, seed, samples);
}

extern "C" int sfm_ess_ransac(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, const float* pts1, const float* pts2,
                              int64_t n, const double* Kseg, const int32_t* samples, int32_t n_hyp, double threshold,
                              int32_t refine, double* E, uint8_t* mask, int32_t* n_inliers, int32_t* status,
                              int32_t* hyp_count, int32_t* refined, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  const int nblk = n_hyp >= 1 ? (n_hyp + ESS_HYP_PER_BLOCK - 1) / ESS_HYP_PER_BLOCK : 0;
  // the score grid is n_seg x ceil(n_hyp / 25) workgroups, the largest of the four
  if (ransac_bad_args(n, n_seg, n_hyp, threshold) || (int64_t)n_seg * nblk > 0x7fffffffLL)
    return sfm_fail(h, SFM_ERR_ARG, "sfm_ess_ransac", "bad argument");
  if (n == 0 || n_seg == 0) return SFM_OK;
  if (!seg_ptr || !pts1 || !pts2 || !Kseg || !samples || !E || !mask || !n_inliers || !status || !workspace)
    return sfm_fail(h, SFM_ERR_ARG, "sfm_ess_ransac", "null pointer");
  const ess_ws w = ess_layout(workspace, n_seg, n_hyp);
  if (workspace_bytes < w.bytes) return sfm_fail(h, SFM_ERR_WORKSPACE, "sfm_ess_ransac", "workspace too small");
  int* counts = hyp_count ? hyp_count : w.hyp_count;
  const double thr2 = threshold * threshold;
  const float2* p1 = (const float2*)pts1;
  const float2* p2 = (const float2*)pts2;
  const int64_t total = (int64_t)n_seg * n_hyp;
  SFM_HIP(h, hipMemsetAsync(mask, 0, (size_t)n, h->stream));    // matches outside every segment
  sfm_prof_begin(h, SFM_PROF_ESS_SOLVE);
  hipLaunchKernelGGL(k_ess_solve, dim3(cdiv(total, 64)), dim3(64), 0, h->stream, seg_ptr, n, p1, p2, Kseg, samples, n_hyp,
                     total, w.cand_n, w.cand_E);
  sfm_prof_end(h, SFM_PROF_ESS_SOLVE);
  sfm_prof_begin(h, SFM_PROF_ESS_SCORE);
  hipLaunchKernelGGL(k_ess_score, dim3((unsigned)n_seg * nblk), dim3(256), 0, h->stream, seg_ptr, n, p1, p2, Kseg, n_hyp,
                     nblk, thr2, (const int*)w.cand_n, (const double*)w.cand_E, counts, w.hyp_cand);
  sfm_prof_end(h, SFM_PROF_ESS_SCORE);
  hipLaunchKernelGGL(k_ess_select, dim3(n_seg), dim3(256), 0, h->stream, seg_ptr, n, p1, p2, Kseg, n_hyp, thr2,
                     (const int*)counts, (const int*)w.hyp_cand, (const double*)w.cand_E, E, mask, n_inliers, status,
                     refined);
  if (refine)
    hipLaunchKernelGGL(k_ess_refit, dim3(n_seg), dim3(256), 0, h->stream, seg_ptr, n, p1, p2, Kseg, thr2, E, mask,
                       n_inliers, (const int*)status, refined);
  SFM_LAUNCH_CHECK(h, "sfm_ess_ransac");
  return SFM_OK;
}
