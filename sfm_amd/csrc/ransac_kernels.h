// The device side of a batched, replayable RANSAC, shared by twoview.hip, essential.hip, homography.hip and pnp.hip
// (and, for load_k4, pose.hip): the sample kernel and the gather of a sample's matches, the block sums, the Hartley
// normalisation of twoview.hip and homography.hip, the whole-segment inlier count, the winner rule, the rule by which a
// refit replaces the winner and the 9 x 9 normal matrix and Jacobi of the two-view refits, for workgroups of 256 threads.
// Included by .hip files only; what also compiles for the host stays in ransac_common.h.
#pragma once
#include "common.h"
#include "ransac_common.h"
#include <cfloat>

// One lane per (segment, hypothesis): N distinct indices, or -1 in all N slots of a segment under MIN_POINTS points
template <int N, int MIN_POINTS>
__global__ __launch_bounds__(256) void k_ransac_samples(const int64_t* __restrict__ seg_ptr, int n_seg, int H, int64_t n,
                                                        uint64_t seed, int* __restrict__ samples) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)n_seg * H) return;
  const int s = (int)(g / H), hyp = (int)(g % H);
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  int idx[N];
#pragma unroll
  for (int k = 0; k < N; ++k) idx[k] = -1;
  if (M >= MIN_POINTS) draw_distinct<N>(seed, s, hyp, M, idx);
#pragma unroll
  for (int k = 0; k < N; ++k) samples[g * N + k] = idx[k];
}

// what stands behind every sfm_*_draw_samples; `what` names the entry point in the error string
template <int N, int MIN_POINTS>
int ransac_draw_samples(sfm_handle h, const char* what, const int64_t* seg_ptr, int32_t n_seg, int32_t n_hyp,
                        uint64_t seed, int32_t* samples) {
  if (!h) return SFM_ERR_ARG;
  if (n_seg < 0 || n_hyp < 1 || (int64_t)n_seg * n_hyp > 0x7fffffffLL * 64) return sfm_fail(h, SFM_ERR_ARG, what, "bad argument");
  if (n_seg == 0) return SFM_OK;
  if (!seg_ptr || !samples) return sfm_fail(h, SFM_ERR_ARG, what, "null pointer");
  const int64_t total = (int64_t)n_seg * n_hyp;
  // the segment's extent comes from seg_ptr alone here: no clamp to a point count (INT64_MAX passes every segment)
  hipLaunchKernelGGL((k_ransac_samples<N, MIN_POINTS>), dim3(cdiv(total, 256)), dim3(256), 0, h->stream, seg_ptr, n_seg,
                     n_hyp, (int64_t)0x7fffffffffffffffLL, (uint64_t)seed, samples);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}

// the scalar arguments every sfm_*_ransac turns down (the grid is n_seg x ceil(n_hyp / 256) workgroups)
inline bool ransac_bad_args(int64_t n, int32_t n_seg, int32_t n_hyp, double threshold) {
  return n < 0 || n_seg < 0 || n_hyp < 1 || !(threshold >= 0.0) || !(threshold < DBL_MAX) ||
         (int64_t)n_seg * ((n_hyp + 255) / 256) > 0x7fffffffLL;
}

// the workspace of twoview.hip and homography.hip: the segments' Hartley transforms, one 3 x 3 model and one count per
// hypothesis
struct model9_ws {
  double* T;
  double* hyp_model;
  int* hyp_count;
  int64_t bytes;
};

inline model9_ws model9_layout(void* workspace, int32_t n_seg, int32_t n_hyp) {
  ws_carve c{(char*)workspace};
  model9_ws w;
  w.T = c.take<double>((int64_t)n_seg * 6);
  w.hyp_model = c.take<double>((int64_t)n_seg * n_hyp * 9);
  w.hyp_count = c.take<int>((int64_t)n_seg * n_hyp);
  w.bytes = c.bytes();
  return w;
}

// --------------------------------------------------------------------------------------------- block sums
// Fixed order (deterministic): the lanes of a wave by butterfly d = 32..1, then the four waves as (s0 + s1) + (s2 + s3)
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// one value per thread (double or int); every thread gets the total
template <typename T>
__device__ __forceinline__ T block_sum(T v) {
  __shared__ T s_w[4];
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

// K values per thread: the four wave sums go to s_red, and block_total(s_red, k) is total k for every thread.  The
// totals stay in LDS on purpose: a caller that picks k at run time reads LDS, where a register array would go to scratch.
template <int K>
__device__ __forceinline__ void block_sum_wide(double (&acc)[K], double (*s_red)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = wave_sum(acc[k]);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
}

template <int K>
__device__ __forceinline__ double block_total(const double (*s_red)[K], int k) {
  return (s_red[0][k] + s_red[1][k]) + (s_red[2][k] + s_red[3][k]);
}

__device__ __forceinline__ bool finite4(float2 p, float2 q) {
  return isfinite(p.x) && isfinite(p.y) && isfinite(q.x) && isfinite(q.y);
}

// The sample of hypothesis `slot` of a two-view stage as px[k] = (x1, y1, x2, y2), float32 pixels.  False, with match 0
// (M >= 1) in every px[k], for an idle lane or an index outside [0, M): checked before anything is indexed.  Not for
// k_fund_hypotheses: 28 floats live across its elimination cost 32 VGPRs, so its solver is handed one match per row.
template <int N>
__device__ __forceinline__ bool load_sample(const int* __restrict__ samples, int64_t slot, bool active, int M, int64_t b,
                                            const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                            float (&px)[N][4]) {
  bool ok = active;
  int idx[N];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    idx[k] = active ? samples[slot * N + k] : 0;
    ok = ok && idx[k] >= 0 && idx[k] < M;
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int id = ok ? idx[k] : 0;
    const float2 p = pts1[b + id], q = pts2[b + id];
    px[k][0] = p.x; px[k][1] = p.y; px[k][2] = q.x; px[k][3] = q.y;
  }
  return ok;
}

// ------------------------------------------------------------------------------------------ normalisation
// Hartley transform per segment and image, over the finite matches (twoview.hip and homography.hip): x' = sc * (x - c),
// centroid c, mean distance sqrt(2) after scaling.
// T[s] = {sc1, cx1, cy1, sc2, cx2, cy2}: the 2 x 3 upper rows [sc 0 -sc*cx; 0 sc -sc*cy] in factored form.  A template
// only so that the kernel exists in the files that launch it; BLOCK is the workgroup size, 256.
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_hartley_normalise(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                             const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                                             double* __restrict__ T) {
  static_assert(BLOCK == 256, "block_sum adds four waves");
  const int s = blockIdx.x, tid = threadIdx.x;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  double sx1 = 0, sy1 = 0, sx2 = 0, sy2 = 0, cnt = 0;
  for (int i = tid; i < M; i += 256) {
    const float2 p = pts1[b + i], q = pts2[b + i];
    if (finite4(p, q)) { sx1 += p.x; sy1 += p.y; sx2 += q.x; sy2 += q.y; cnt += 1.0; }
  }
  cnt = block_sum(cnt);
  const double inv = cnt > 0 ? 1.0 / cnt : 0.0;
  const double cx1 = block_sum(sx1) * inv, cy1 = block_sum(sy1) * inv;
  const double cx2 = block_sum(sx2) * inv, cy2 = block_sum(sy2) * inv;
  double d1 = 0, d2 = 0;
  for (int i = tid; i < M; i += 256) {
    const float2 p = pts1[b + i], q = pts2[b + i];
    if (finite4(p, q)) {
      const double ax = p.x - cx1, ay = p.y - cy1, bx = q.x - cx2, by = q.y - cy2;
      d1 += sqrt(ax * ax + ay * ay); d2 += sqrt(bx * bx + by * by);
    }
  }
  d1 = block_sum(d1) * inv; d2 = block_sum(d2) * inv;
  if (tid == 0) {
    double* t = T + 6 * (int64_t)s;
    t[0] = d1 > 0 ? sqrt(2.0) / d1 : 1.0; t[1] = cx1; t[2] = cy1;
    t[3] = d2 > 0 ? sqrt(2.0) / d2 : 1.0; t[4] = cx2; t[5] = cy2;
  }
}

// ---------------------------------------------------------------------------------------------- selection
// a 3 x 3 model m as m / m[8] when that is finite (m[8] / m[8] == 1 exactly), m as it is otherwise: F[2][2] = 1 of
// k_fund_select, H[2][2] = 1 of k_hom_select
__device__ __forceinline__ void scale_last_to_one(double (&f)[9]) {
  const double d = f[8];
  bool ok = d != 0.0;
  double g[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) { g[e] = f[e] / d; ok = ok && isfinite(g[e]); }
#pragma unroll
  for (int e = 0; e < 9; ++e) f[e] = ok ? g[e] : f[e];
}

// inliers of a model over the whole segment [b, b + M), counted by the workgroup (every thread takes its own points);
// inlier(i) is the stage's rule for point i of the batch.  Writes the mask when `mask` is not null.
template <typename Inlier>
__device__ __forceinline__ int segment_count(int64_t b, int M, uint8_t* __restrict__ mask, Inlier inlier) {
  int c = 0;
  for (int i = threadIdx.x; i < M; i += 256) {
    const bool in = inlier(b + i);
    if (mask) mask[b + i] = in ? 1 : 0;
    c += in ? 1 : 0;
  }
  return block_sum(c);
}

// winner of segment s: largest count, ties to the lowest hypothesis index, as one integer key
// (count << 32 | ~hypothesis) reduced by a tree.  Returns the status (1: fewer than min_points points, 2: no
// hypothesis with an inlier, 0: `hyp` is the winner), uniform over the workgroup.
__device__ __forceinline__ int ransac_winner(const int* __restrict__ hyp_count, int s, int H, int M, int min_points, int& hyp) {
  __shared__ unsigned long long s_key[256];
  const int tid = threadIdx.x;
  unsigned long long key = 0;
  if (M >= min_points)
    for (int hp = tid; hp < H; hp += 256) {
      const int c = hyp_count[(int64_t)s * H + hp];
      const unsigned long long k = ((unsigned long long)(unsigned)(c < 0 ? 0 : c) << 32) | (0xFFFFFFFFu - (unsigned)hp);
      key = k > key ? k : key;
    }
  s_key[tid] = key;
  __syncthreads();
#pragma unroll
  for (int d = 128; d >= 1; d >>= 1) {
    if (tid < d) { const unsigned long long o = s_key[tid + d]; if (o > s_key[tid]) s_key[tid] = o; }
    __syncthreads();
  }
  key = s_key[0];
  hyp = (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu));
  return (M < min_points) ? 1 : ((int)(key >> 32) == 0 ? 2 : 0);
}

// what a select kernel leaves for segment s: the model's W doubles (zero without a model), count, status, refined = 0;
// a segment without a model gets a zero mask
template <int W>
__device__ __forceinline__ void ransac_store_winner(int s, int st, int64_t b, int M, const double (&model)[W], int count,
                                                    double* __restrict__ out, uint8_t* __restrict__ mask,
                                                    int* __restrict__ n_inliers, int* __restrict__ status,
                                                    int* __restrict__ refined) {
  if (st != 0)
    for (int i = threadIdx.x; i < M; i += 256) mask[b + i] = 0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int e = 0; e < W; ++e) out[W * (int64_t)s + e] = model[e];
    n_inliers[s] = count;
    status[s] = st;
    if (refined) refined[s] = 0;
  }
}

// what a refit leaves for segment s when its model is kept: the model's W doubles, its count, refined = 1
template <int W>
__device__ __forceinline__ void ransac_store_refit(int s, const double (&model)[W], int count, double* __restrict__ out,
                                                   int* __restrict__ n_inliers, int* __restrict__ refined) {
  if (threadIdx.x == 0) {
#pragma unroll
    for (int e = 0; e < W; ++e) out[W * (int64_t)s + e] = model[e];
    n_inliers[s] = count;
    if (refined) refined[s] = 1;
  }
}

// A refit replaces the winner only if its inlier count is not lower than `have`, the winner's.  count(mask) is the
// stage's whole-segment count of the refitted model (segment_count behind it): first without a mask, and only a model
// that is kept writes its mask.
template <int W, typename Count>
__device__ __forceinline__ void ransac_keep_refit(int s, int have, const double (&model)[W], Count count,
                                                  double* __restrict__ out, uint8_t* __restrict__ mask,
                                                  int* __restrict__ n_inliers, int* __restrict__ refined) {
  const int c = count((uint8_t*)nullptr);
  if (c < have) return;
  (void)count(mask);
  ransac_store_refit(s, model, c, out, n_inliers, refined);
}

// ------------------------------------------------------------------------------------------- 9 x 9 Jacobi
// Cyclic Jacobi on the symmetric s_A [9][9] in LDS, run by a whole workgroup (lanes 0..8 rotate one row / column entry
// each): on return the diagonal of s_A holds the eigenvalues and the columns of s_V, which must enter as the identity,
// the eigenvectors.  Every thread reads the same values, so the control flow is uniform.
__device__ __forceinline__ void jacobi9_lds(double (*s_A)[9], double (*s_V)[9]) {
  const int tid = threadIdx.x;
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int u = 0; u < 9; ++u)
      for (int v = 0; v < 9; ++v) { const double a = s_A[u][v]; if (u == v) diag += a * a; else off += a * a; }
    if (!(off > 1e-30 * diag)) break;                    // uniform: every thread read the same values
    for (int p = 0; p < 8; ++p)
      for (int q = p + 1; q < 9; ++q) {
        const double app = s_A[p][p], aqq = s_A[q][q], apq = s_A[p][q];
        double c = 1.0, sn = 0.0;
        if (fabs(apq) > DBL_EPSILON * 1e-3 * sqrt(fabs(app * aqq)) && apq != 0.0) {
          const double zeta = (aqq - app) / (2.0 * apq);
          const double tt = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          c = 1.0 / sqrt(1.0 + tt * tt); sn = c * tt;
        }
        __syncthreads();
        if (tid < 9) {                                   // A <- A J, V <- V J (columns p, q)
          const double ap = s_A[tid][p], aq = s_A[tid][q];
          s_A[tid][p] = c * ap - sn * aq; s_A[tid][q] = sn * ap + c * aq;
          const double vp = s_V[tid][p], vq = s_V[tid][q];
          s_V[tid][p] = c * vp - sn * vq; s_V[tid][q] = sn * vp + c * vq;
        }
        __syncthreads();
        if (tid < 9) {                                   // A <- J^T A (rows p, q)
          const double ap = s_A[p][tid], aq = s_A[q][tid];
          s_A[p][tid] = c * ap - sn * aq; s_A[q][tid] = sn * ap + c * aq;
        }
        __syncthreads();
      }
  }
}

// The refits of twoview.hip, essential.hip and homography.hip: acc holds a thread's share of the 45 unique entries
// (upper triangle, row by row) of a 9 x 9 normal matrix.  Summed by the workgroup in a fixed order into s_A, then
// jacobi9_lds: on return s_A's diagonal holds the eigenvalues and s_V's columns the eigenvectors, for every thread.
__device__ __forceinline__ void normal9_eigen(double (&acc)[45], double (*s_red)[45], double (*s_A)[9], double (*s_V)[9]) {
  const int tid = threadIdx.x;
  block_sum_wide(acc, s_red);
  if (tid < 81) {
    const int u = tid / 9, v = tid % 9;
    const int lo = u < v ? u : v, hi = u < v ? v : u;
    const int k = lo * 9 - lo * (lo - 1) / 2 + (hi - lo);
    s_A[u][v] = block_total(s_red, k);
    s_V[u][v] = (u == v) ? 1.0 : 0.0;
  }
  __syncthreads();
  jacobi9_lds(s_A, s_V);
}

// index of the smallest eigenvalue (ties: the lowest index)
__device__ __forceinline__ int smallest_diagonal9(const double (*s_A)[9]) {
  int kmin = 0;
  for (int k = 1; k < 9; ++k) if (s_A[k][k] < s_A[kmin][kmin]) kmin = k;
  return kmin;
}

// Kseg [n_seg][4] = (fx, fy, cx, cy) of segment s
struct k4 { double fx, fy, cx, cy; };
__device__ __forceinline__ k4 load_k4(const double* __restrict__ Kseg, int64_t s) {
  return {Kseg[4 * s], Kseg[4 * s + 1], Kseg[4 * s + 2], Kseg[4 * s + 3]};
}
