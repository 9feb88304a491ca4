// Absolute-pose (PnP) RANSAC for every candidate image of a registration step in one call (gfx950 only): the
// cv2.solvePnPRansac(points3D, points2D, K, None, iterationsCount=1000, reprojectionError=8.0,
// flags=cv2.SOLVEPNP_ITERATIVE) call of the reference's add_new_image (`pnp_ransac`).
//
// Structure as OpenCV's solvePnPRansac is RECALLED (its source is not pinned here): minimal samples of 5 solved by
// EPnP inside the loop, reprojection error against the threshold in pixels, most inliers wins, then the ITERATIVE
// (Levenberg-Marquardt) solver over the inliers.  Deviations, on purpose: minimal samples of 3 solved by closed-form
// P3P with ALL of its (up to four) roots scored; a FIXED number of hypotheses (no early exit on confidence); the
// stateless hash sampler of twoview.hip with 3 slots (k_ransac_samples<3, 4>; draw_distinct<3>, ransac_common.h) - so
// the result is a function of (points, K, samples) alone and a NumPy reference can follow the device hypothesis by
// hypothesis (tests/pnp_reference.py).  The sample kernel, the block sums, the whole-segment count and the winner rule
// are those of the fundamental-matrix RANSAC (ransac_kernels.h).
//
// One segment is one candidate image: seg_ptr[n_seg+1] device int64 (the convention of sfm_fund_ransac), X [n][3]
// float64 world points, uv [n][2] float32 pixels, Kseg [n_seg][4] float64 (fx, fy, cx, cy).  All arithmetic in
// float64.  The inlier rule has no division:  p = K [R|t] [X; 1],  inlier <=> p2 > 0 and
// (p0 - u p2)^2 + (p1 - v p2)^2 <= thr^2 p2^2,  written with explicit fma so that the three kernels that apply it
// round alike.  A point with a NaN or infinite coordinate is never an inlier; a sample that holds one, or whose
// triangle has no area (pnp_solve.h), gives no model.  Sample indices are range-checked before they index anything.
#include "ransac_kernels.h"
#include "pnp_solve.h"

namespace {

constexpr int PNP_CHUNK = 512;       // points per LDS stage of the scoring loop: 512 x 5 doubles = 20 KiB

__device__ __forceinline__ bool finite_point(const double* __restrict__ x, float2 p) {
  return isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]) && isfinite(p.x) && isfinite(p.y);
}

// P = K [R|t], row-major 3 x 4
__device__ __forceinline__ void make_P(double fx, double fy, double cx, double cy, const double (&Rt)[12], double (&P)[12]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    P[e] = fma(fx, Rt[e], cx * Rt[8 + e]);
    P[4 + e] = fma(fy, Rt[4 + e], cy * Rt[8 + e]);
    P[8 + e] = Rt[8 + e];
  }
}

// NaN fails every comparison; P = 0 (the empty candidate slot) gives p2 = 0 and never counts
__device__ __forceinline__ bool pnp_inlier(const double (&P)[12], double x, double y, double z, double u, double v, double thr2) {
#pragma clang fp contract(off)
  const double p0 = fma(P[0], x, fma(P[1], y, fma(P[2], z, P[3])));
  const double p1 = fma(P[4], x, fma(P[5], y, fma(P[6], z, P[7])));
  const double p2 = fma(P[8], x, fma(P[9], y, fma(P[10], z, P[11])));
  const double e0 = fma(-u, p2, p0), e1 = fma(-v, p2, p1);
  return (p2 > 0.0) && (fma(e0, e0, e1 * e1) <= thr2 * (p2 * p2));
}

// --------------------------------------------------------------------------------------------- hypotheses
// One lane per (segment, hypothesis); a workgroup covers 256 hypotheses of ONE segment, so the scoring loop's points
// are wave-uniform: fetched from global memory once per workgroup and chunk into LDS, read back as broadcasts.  The
// (up to) four candidates of the lane's sample stay in registers as P = K [R|t] while every point of the segment is
// scored; their [R|t] wait in the workspace (cand_Rt) for k_pnp_select, which needs one of them per segment.
__global__ __launch_bounds__(256) void k_pnp_hypotheses(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                        const double* __restrict__ X, const float2* __restrict__ uv,
                                                        const double* __restrict__ Kseg, const int* __restrict__ samples,
                                                        int H, int nblk, double thr2, int* __restrict__ hyp_count,
                                                        int* __restrict__ hyp_cand, double* __restrict__ cand_Rt) {
  __shared__ double s_pt[5 * PNP_CHUNK];
  const int s = blockIdx.x / nblk;
  const int hyp = (blockIdx.x % nblk) * 256 + threadIdx.x;
  const bool active = hyp < H;
  const int64_t slot = (int64_t)s * H + hyp;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  if (M < 4) {                                           // uniform over the workgroup
    if (active) {
      hyp_count[slot] = 0; hyp_cand[slot] = 0;
#pragma unroll
      for (int e = 0; e < 48; ++e) cand_Rt[slot * 48 + e] = 0.0;         // "no model", as the other stages leave it
    }
    return;
  }
  const auto [fx, fy, cx, cy] = load_k4(Kseg, s);
  double Pc[4][12];
  {
    bool ok = active;
    int idx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      idx[k] = active ? samples[slot * 3 + k] : 0;
      ok = ok && idx[k] >= 0 && idx[k] < M;
    }
    double Pw[3][3], f[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int64_t id = b + (ok ? idx[k] : 0);
      const float2 p = uv[id];
#pragma unroll
      for (int c = 0; c < 3; ++c) Pw[k][c] = X[3 * id + c];
      ok = ok && finite_point(&X[3 * id], p);
      const double bx = ((double)p.x - cx) / fx, by = ((double)p.y - cy) / fy;
      const double inv = 1.0 / sqrt(bx * bx + by * by + 1.0);
      f[k][0] = bx * inv; f[k][1] = by * inv; f[k][2] = inv;
    }
    double Rt[4][12];
    const int solved = p3p::solve(Pw, f, Rt);
    const int filled = ok ? solved : 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool good = (filled >> c) & 1;
#pragma unroll
      for (int e = 0; e < 12; ++e) Rt[c][e] = good ? Rt[c][e] : 0.0;
      make_P(fx, fy, cx, cy, Rt[c], Pc[c]);
      if (active) {
#pragma unroll
        for (int e = 0; e < 12; ++e) cand_Rt[(slot * 4 + c) * 12 + e] = Rt[c][e];
      }
    }
  }
  // scoring: every lane walks all points of the segment with its candidates in registers
  int cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0;
  for (int base = 0; base < M; base += PNP_CHUNK) {
    const int cnt = (M - base < PNP_CHUNK) ? (M - base) : PNP_CHUNK;
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += 256) {       // a non-finite point is staged as NaN in all five
      const int64_t id = b + base + t;
      const float2 p = uv[id];
      const bool fin = finite_point(&X[3 * id], p);
      const double nan = __builtin_nan("");
      s_pt[5 * t] = fin ? X[3 * id] : nan; s_pt[5 * t + 1] = fin ? X[3 * id + 1] : nan;
      s_pt[5 * t + 2] = fin ? X[3 * id + 2] : nan;
      s_pt[5 * t + 3] = fin ? (double)p.x : nan; s_pt[5 * t + 4] = fin ? (double)p.y : nan;
    }
    __syncthreads();
    for (int i = 0; i < cnt; ++i) {
      const double x = s_pt[5 * i], y = s_pt[5 * i + 1], z = s_pt[5 * i + 2], u = s_pt[5 * i + 3], v = s_pt[5 * i + 4];
      cnt0 += pnp_inlier(Pc[0], x, y, z, u, v, thr2) ? 1 : 0;
      cnt1 += pnp_inlier(Pc[1], x, y, z, u, v, thr2) ? 1 : 0;
      cnt2 += pnp_inlier(Pc[2], x, y, z, u, v, thr2) ? 1 : 0;
      cnt3 += pnp_inlier(Pc[3], x, y, z, u, v, thr2) ? 1 : 0;
    }
  }
  if (!active) return;
  int best = cnt0, cand = 0;                             // ties: the lowest candidate slot
  if (cnt1 > best) { best = cnt1; cand = 1; }
  if (cnt2 > best) { best = cnt2; cand = 2; }
  if (cnt3 > best) { best = cnt3; cand = 3; }
  hyp_count[slot] = best;
  hyp_cand[slot] = cand;
}

// ---------------------------------------------------------------------------------------------- selection
// inliers of P over the whole segment; writes the mask when `mask` is not null
__device__ __forceinline__ int pnp_count(const double (&P)[12], const double* __restrict__ X,
                                         const float2* __restrict__ uv, int64_t b, int M, double thr2,
                                         uint8_t* __restrict__ mask) {
  return segment_count(b, M, mask, [&](int64_t id) {
    const float2 p = uv[id];
    return finite_point(&X[3 * id], p) &&
           pnp_inlier(P, X[3 * id], X[3 * id + 1], X[3 * id + 2], (double)p.x, (double)p.y, thr2);
  });
}

// winner per segment (ransac_winner; ties between the candidates of one hypothesis were settled in k_pnp_hypotheses,
// to the lowest slot): its [R|t], its mask and its count
__global__ __launch_bounds__(256) void k_pnp_select(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                    const double* __restrict__ X, const float2* __restrict__ uv,
                                                    const double* __restrict__ Kseg, int H, double thr2,
                                                    const int* __restrict__ hyp_count, const int* __restrict__ hyp_cand,
                                                    const double* __restrict__ cand_Rt, double* __restrict__ Rt_out,
                                                    uint8_t* __restrict__ mask, int* __restrict__ n_inliers,
                                                    int* __restrict__ status, int* __restrict__ refined) {
  const int s = blockIdx.x;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  int hp;
  const int st = ransac_winner(hyp_count, s, H, M, 4, hp);
  double Rt[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) Rt[e] = 0.0;
  int count = 0;
  if (st == 0) {                                         // uniform over the workgroup
    const int64_t slot = (int64_t)s * H + hp;
    const int cand = hyp_cand[slot] & 3;
#pragma unroll
    for (int e = 0; e < 12; ++e) Rt[e] = cand_Rt[(slot * 4 + cand) * 12 + e];
    const auto [fx, fy, cx, cy] = load_k4(Kseg, s);
    double P[12];
    make_P(fx, fy, cx, cy, Rt, P);
    count = pnp_count(P, X, uv, b, M, thr2, mask);
  }
  ransac_store_winner(s, st, b, M, Rt, count, Rt_out, mask, n_inliers, status, refined);
}

// ------------------------------------------------------------------------------------------------- refine
// R = I + a [w]x + b [w]x^2 (Rodrigues), the series for small |w| as sfm_amd/rotation.py has them
__device__ __forceinline__ void rodrigues(double w0, double w1, double w2, double (&R)[9]) {
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
  double a, bq;
  if (th2 < 1e-4) {
    a = 1.0 - th2 / 6.0 + th2 * th2 / 120.0;
    bq = 0.5 - th2 / 24.0 + th2 * th2 / 720.0;
  } else {
    const double th = sqrt(th2);
    a = sin(th) / th;
    bq = (1.0 - cos(th)) / th2;
  }
  R[0] = 1.0 - bq * (w1 * w1 + w2 * w2); R[1] = -a * w2 + bq * w0 * w1;      R[2] = a * w1 + bq * w0 * w2;
  R[3] = a * w2 + bq * w0 * w1;          R[4] = 1.0 - bq * (w0 * w0 + w2 * w2); R[5] = -a * w0 + bq * w1 * w2;
  R[6] = -a * w1 + bq * w0 * w2;         R[7] = a * w0 + bq * w1 * w2;       R[8] = 1.0 - bq * (w0 * w0 + w1 * w1);
}

constexpr int PNP_SUMS = 28;         // 21 entries of the normal matrix (upper triangle, row by row), 6 of the gradient, the cost
constexpr int PNP_LM_ITERS = 30;

// Levenberg-Marquardt on the pose over the winner's inlier set (held fixed), one workgroup per segment.  The unknowns
// are (rvec, t) with the rotation vector taken about the current rotation, R <- exp([w]x) R: the 2 x 6 Jacobian of a
// pixel is then  d(pixel)/dY [ -[R X]x | I ]  in closed form, and no iterate comes near the vector's singularity at
// an angle of pi.  The 6 x 6 normal matrix, the gradient and the cost are summed in a fixed order (lanes by
// butterfly, the four waves in one expression); every thread then takes the same damped Cholesky step in registers,
// so the control flow is uniform.  A step is kept only if the cost drops; the loop ends when
// |step| <= 1e-12 (1 + |(angle(R), t)|) or after 30 steps.  The refined pose replaces the winner only if its inlier
// count over ALL points is not lower.
__global__ __launch_bounds__(256) void k_pnp_refine(const int64_t* __restrict__ seg_ptr, int64_t n,
                                                    const double* __restrict__ X, const float2* __restrict__ uv,
                                                    const double* __restrict__ Kseg, double thr2,
                                                    double* __restrict__ Rt_out, uint8_t* __restrict__ mask,
                                                    int* __restrict__ n_inliers, const int* __restrict__ status,
                                                    int* __restrict__ refined) {
  __shared__ double s_red[4][PNP_SUMS];
  const int s = blockIdx.x, tid = threadIdx.x;
  int64_t b; int M;
  seg_range(seg_ptr, s, n, b, M);
  const int have = n_inliers[s];
  if (status[s] != 0 || have < 3) return;                // uniform; refined[s] stays 0
  const auto [fx, fy, cx, cy] = load_k4(Kseg, s);
  double R[9], t[3], Rn[9], tn[3];                       // the accepted pose and the trial
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Rn[3 * r + c] = R[3 * r + c] = Rt_out[12 * (int64_t)s + 4 * r + c];
    tn[r] = t[r] = Rt_out[12 * (int64_t)s + 4 * r + 3];
  }
  double Hc[PNP_SUMS];                                   // the sums at the accepted pose
#pragma unroll
  for (int k = 0; k < PNP_SUMS; ++k) Hc[k] = 0.0;
  double mu = 1e-3;
  for (int it = 0; it <= PNP_LM_ITERS; ++it) {
    double acc[PNP_SUMS];
#pragma unroll
    for (int k = 0; k < PNP_SUMS; ++k) acc[k] = 0.0;
    for (int i = tid; i < M; i += 256) {
      const int64_t id = b + i;
      if (!mask[id]) continue;
      const double x = X[3 * id], y = X[3 * id + 1], z = X[3 * id + 2];
      const float2 p = uv[id];
      const double q0 = Rn[0] * x + Rn[1] * y + Rn[2] * z, q1 = Rn[3] * x + Rn[4] * y + Rn[5] * z;
      const double q2 = Rn[6] * x + Rn[7] * y + Rn[8] * z;                        // R X
      const double y0 = q0 + tn[0], y1 = q1 + tn[1], y2 = q2 + tn[2];
      const double iz = 1.0 / y2;
      const double ru = fx * y0 * iz + cx - (double)p.x, rv = fy * y1 * iz + cy - (double)p.y;
      const double a0 = fx * iz, a2 = -fx * y0 * iz * iz, c1 = fy * iz, c2 = -fy * y1 * iz * iz;
      const double ju[6] = {a2 * q1, a0 * q2 - a2 * q0, -a0 * q1, a0, 0.0, a2};
      const double jv[6] = {c2 * q1 - c1 * q2, -c2 * q0, c1 * q0, 0.0, c1, c2};
      int k = 0;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) acc[k++] += ju[r] * ju[c] + jv[r] * jv[c];
#pragma unroll
      for (int r = 0; r < 6; ++r) acc[21 + r] += ju[r] * ru + jv[r] * rv;
      acc[27] += ru * ru + rv * rv;
    }
    block_sum_wide(acc, s_red);
#pragma unroll
    for (int k = 0; k < PNP_SUMS; ++k) acc[k] = block_total(s_red, k);
    // from here on every thread holds the same numbers
    if (it == 0 || acc[27] < Hc[27]) {
#pragma unroll
      for (int k = 0; k < PNP_SUMS; ++k) Hc[k] = acc[k];
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = tn[k];
      if (it > 0) mu = fmax(mu * 0.1, 1e-12);
    } else {
      mu *= 10.0;
    }
    if (it == PNP_LM_ITERS || !(Hc[27] == Hc[27])) break;
    // (H + mu diag H) d = -g by Cholesky, H = L L^T
    double L[6][6], d[6];
    bool pd = true;
    {
      int k = 0;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = r; c < 6; ++c) { L[c][r] = Hc[k] * (r == c ? 1.0 + mu : 1.0); ++k; }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      double dj = L[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k];
      pd = pd && (dj > 0.0);
      const double lj = sqrt(dj);
      L[j][j] = lj;
#pragma unroll
      for (int i = j + 1; i < 6; ++i) {
        double v = L[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
        L[i][j] = v / lj;
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double v = -Hc[21 + i];
#pragma unroll
      for (int k = 0; k < i; ++k) v -= L[i][k] * d[k];
      d[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
      double v = d[i];
#pragma unroll
      for (int k = i + 1; k < 6; ++k) v -= L[k][i] * d[k];
      d[i] = v / L[i][i];
    }
    double dn = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) dn += d[i] * d[i];
    if (!pd || !isfinite(dn)) break;
    const double vx = R[7] - R[5], vy = R[2] - R[6], vz = R[3] - R[1];
    const double ang = atan2(0.5 * sqrt(vx * vx + vy * vy + vz * vz), 0.5 * (R[0] + R[4] + R[8] - 1.0));
    const double xn = sqrt(ang * ang + t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    if (sqrt(dn) <= 1e-12 * (1.0 + xn)) break;
    double dR[9];
    rodrigues(d[0], d[1], d[2], dR);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) Rn[3 * r + c] = dR[3 * r] * R[c] + dR[3 * r + 1] * R[3 + c] + dR[3 * r + 2] * R[6 + c];
      tn[r] = t[r] + d[3 + r];
    }
  }
  double Rt[12], P[12];
  bool good = true;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { Rt[4 * r + c] = R[3 * r + c]; good = good && isfinite(R[3 * r + c]); }
    Rt[4 * r + 3] = t[r]; good = good && isfinite(t[r]);
  }
  if (!good) return;                                     // uniform: every thread holds the same pose
  make_P(fx, fy, cx, cy, Rt, P);
  ransac_keep_refit(s, have, Rt, [&](uint8_t* m) { return pnp_count(P, X, uv, b, M, thr2, m); }, Rt_out, mask, n_inliers,
                    refined);
}

struct pnp_ws {
  double* cand_Rt;
  int* hyp_count;
  int* hyp_cand;
  int64_t bytes;
};

pnp_ws pnp_layout(void* workspace, int32_t n_seg, int32_t n_hyp) {
  ws_carve c{(char*)workspace};
  pnp_ws w;
  w.cand_Rt = c.take<double>((int64_t)n_seg * n_hyp * 4 * 12);
  w.hyp_count = c.take<int>((int64_t)n_seg * n_hyp);
  w.hyp_cand = c.take<int>((int64_t)n_seg * n_hyp);
  w.bytes = c.bytes();
  return w;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int sfm_pnp_workspace_bytes(int64_t n_points, int32_t n_seg, int32_t n_hyp, int64_t* bytes_host) {
  if (!bytes_host || n_points < 0 || n_seg < 0 || n_hyp < 1) return SFM_ERR_ARG;
  *bytes_host = pnp_layout(nullptr, n_seg, n_hyp).bytes;
  return SFM_OK;
}

extern "C" int sfm_pnp_draw_samples(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, int32_t n_hyp, uint64_t seed,
                                    int32_t* samples) {
  return ransac_draw_samples<3, 4>(h, "sfm_pnp_draw_samples", seg_ptr, n_seg, n_hyp, seed, samples);
}

extern "C" int sfm_pnp_ransac(sfm_handle h, const int64_t* seg_ptr, int32_t n_seg, const double* X, const float* uv,
                              int64_t n, const double* Kseg, const int32_t* samples, int32_t n_hyp, double threshold,
                              int32_t refine, double* Rt, uint8_t* mask, int32_t* n_inliers, int32_t* status,
                              int32_t* hyp_count, int32_t* refined, void* workspace, int64_t workspace_bytes) {
  if (!h) return SFM_ERR_ARG;
  if (ransac_bad_args(n, n_seg, n_hyp, threshold)) return sfm_fail(h, SFM_ERR_ARG, "sfm_pnp_ransac", "bad argument");
  if (n == 0 || n_seg == 0) return SFM_OK;
  if (!seg_ptr || !X || !uv || !Kseg || !samples || !Rt || !mask || !n_inliers || !status || !workspace)
    return sfm_fail(h, SFM_ERR_ARG, "sfm_pnp_ransac", "null pointer");
  const pnp_ws w = pnp_layout(workspace, n_seg, n_hyp);
  if (workspace_bytes < w.bytes) return sfm_fail(h, SFM_ERR_WORKSPACE, "sfm_pnp_ransac", "workspace too small");
  int* counts = hyp_count ? hyp_count : w.hyp_count;
  const double thr2 = threshold * threshold;
  const float2* p2 = (const float2*)uv;
  const int nblk = (n_hyp + 255) / 256;
  SFM_HIP(h, hipMemsetAsync(mask, 0, (size_t)n, h->stream));    // points outside every segment
  sfm_prof_begin(h, SFM_PROF_PNP_HYP);
  hipLaunchKernelGGL(k_pnp_hypotheses, dim3((unsigned)n_seg * nblk), dim3(256), 0, h->stream, seg_ptr, n, X, p2, Kseg,
                     samples, n_hyp, nblk, thr2, counts, w.hyp_cand, w.cand_Rt);
  sfm_prof_end(h, SFM_PROF_PNP_HYP);
  hipLaunchKernelGGL(k_pnp_select, dim3(n_seg), dim3(256), 0, h->stream, seg_ptr, n, X, p2, Kseg, n_hyp, thr2,
                     (const int*)counts, (const int*)w.hyp_cand, (const double*)w.cand_Rt, Rt, mask, n_inliers, status,
                     refined);
  if (refine)
    hipLaunchKernelGGL(k_pnp_refine, dim3(n_seg), dim3(256), 0, h->stream, seg_ptr, n, X, p2, Kseg, thr2, Rt, mask,
                       n_inliers, (const int*)status, refined);
  SFM_LAUNCH_CHECK(h, "sfm_pnp_ransac");
  return SFM_OK;
}
