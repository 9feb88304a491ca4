// Bundle adjustment, the implicit-Schur PCG (sfm_ba_solve_pcg).  (Data layout: ba.hip.)
#include "ba_internal.h"
#include "ba_device.h"

// ------------------------------------------------------------------------------------ implicit-Schur PCG
// The damped camera system S y = r,  S = B + alpha I - W (C + alpha I)^-1 W^T, WITHOUT forming or factoring S
// (SURVEY.md section 7 hard part 4 / 4b): for systems of many cameras (1000 cameras: S is 800 MB and its replicated
// factorisation 13.8 ms per damped solve) and for the multi-rank split, where the dense route all-reduces n^2/2
// doubles per solve and factors on every rank while this route exchanges ONE vector of n doubles per iteration.
//   S v = (B + alpha I) v - sum_{k in camera} G_k u_{pt(k)},   u_j = sum_{k in track j} G_k^T v_{cam(k)}
// (the same two passes over G the back-substitution makes), preconditioned with the exact diagonal blocks
// M_c = B_c + alpha I - sum_{k in c} G_k G_k^T (d x d per camera, inverted explicitly).  All CG scalars live on the
// device (one fused single-workgroup kernel per iteration: alpha, x, r, z = M^-1 r, beta, p); the host only reads
// ||r||^2 every few iterations.  Vectors of length n are replicated on every rank, sums over observations are
// rank-local and reduced through the caller's hook - so every rank runs the identical recurrence.

__global__ __launch_bounds__(256) void k_track_sum(int P, const int* __restrict__ pt_ptr, const double* __restrict__ tmp3,
                                                   double* __restrict__ u) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= P) return;
  double u0 = 0.0, u1 = 0.0, u2 = 0.0;
#pragma unroll 5
  for (int k = pt_ptr[j]; k < pt_ptr[j + 1]; ++k) { u0 += tmp3[(size_t)k * 3]; u1 += tmp3[(size_t)k * 3 + 1]; u2 += tmp3[(size_t)k * 3 + 2]; }
  u[(size_t)j * 3] = u0; u[(size_t)j * 3 + 1] = u1; u[(size_t)j * 3 + 2] = u2;
}
// out[c] = B_c v_c - sum over the camera's chunks of the partial sums of k_cam_reduce_chunks (this rank's part of S v - alpha v)
template <int D>
__global__ void k_cam_reduce_final_bv(int C, const int* __restrict__ cch_ptr, const double* __restrict__ part,
                                      const double* __restrict__ B, const double* __restrict__ v, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C * D) return;
  const int c = i / D, a = i - c * D;
  double t = 0.0;
  for (int ch = cch_ptr[c]; ch < cch_ptr[c + 1]; ++ch) t += part[(size_t)ch * 16 + a];
  double bv = 0.0;
#pragma unroll
  for (int b = 0; b < D; ++b) bv += B[(size_t)c * D * D + a * D + b] * v[c * D + b];
  out[i] = bv - t;
}
// per chunk of one camera's observations: sum_k G_k G_k^T (D x D), thread (a, b) per entry, fixed order
template <int D, typename TG, int GS>
__global__ __launch_bounds__(128) void k_cam_gg_chunks(const int* __restrict__ cch_beg, const int* __restrict__ cch_end,
                                                       const int* __restrict__ cam_obs, const TG* __restrict__ G,
                                                       double* __restrict__ part) {
  const int ch = blockIdx.x, e = threadIdx.x;
  if (e >= D * D) return;
  const int a = e / D, b = e - a * D;
  double acc = 0.0;
  for (int i = cch_beg[ch]; i < cch_end[ch]; ++i) {
    const TG* g = G + (size_t)cam_obs[i] * GS;
    acc += (double)g[a] * (double)g[b] + (double)g[D + a] * (double)g[D + b] + (double)g[2 * D + a] * (double)g[2 * D + b];
  }
  part[(size_t)ch * (D * D) + e] = acc;
}
template <int D>
__global__ void k_cam_gg_final(int C, const int* __restrict__ cch_ptr, const double* __restrict__ part,
                               const double* __restrict__ B, double* __restrict__ M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C * D * D) return;
  const int c = i / (D * D), e = i - c * D * D;
  double t = 0.0;
  for (int ch = cch_ptr[c]; ch < cch_ptr[c + 1]; ++ch) t += part[(size_t)ch * (D * D) + e];
  M[i] = B[i] - t;
}
// Minv_c = (M_c + alpha I)^-1 by Cholesky, one thread per camera (D <= 10: 100 doubles of registers / scratch)
template <int D>
__global__ __launch_bounds__(64) void k_precond_invert(int C, const double* __restrict__ M, double alpha, double* __restrict__ Minv,
                                 double* __restrict__ scal) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double L[D][D], X[D][D];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) L[i][j] = 0.5 * (M[(size_t)c * D * D + i * D + j] + M[(size_t)c * D * D + j * D + i]) + (i == j ? alpha : 0.0);
  const bool bad = !small_chol_inverse<D>(L, X);      // X = L^-1, then Minv = X^T X
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) sum += X[k][i] * X[k][j];
      Minv[(size_t)c * D * D + i * D + j] = sum;
    }
  if (bad) scal[CG_FAIL] = 1.0;
}

// z = Minv r per camera block (thread i owns row i of its block)
template <int D>
__device__ __forceinline__ double precond_row(const double* __restrict__ Minv, const double* __restrict__ r, int i) {
  const int c = i / D, a = i - c * D;
  const double* m = Minv + (size_t)c * D * D + a * D;
  double z = 0.0;
#pragma unroll
  for (int b = 0; b < D; ++b) z += m[b] * r[c * D + b];
  return z;
}
// start: x = 0, r = rhs, z = M^-1 r, p = z; scalars rz, rr, rr0
template <int D>
__global__ __launch_bounds__(1024) void k_cg_init(int n, const double* __restrict__ rhs, const double* __restrict__ Minv,
                                                  double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                  double* __restrict__ pv, double* __restrict__ scal) {
  __shared__ double s_red[17];
  double rz = 0.0, rr = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) { x[i] = 0.0; r[i] = rhs[i]; }
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 1024) {
    const double zi = precond_row<D>(Minv, rhs, i);
    z[i] = zi; pv[i] = zi;
    rz += rhs[i] * zi; rr += rhs[i] * rhs[i];
  }
  rz = block_sum1024(rz, s_red);
  rr = block_sum1024(rr, s_red);
  if (threadIdx.x == 0) { scal[CG_RZ] = rz; scal[CG_RR] = rr; scal[CG_RR0] = rr; scal[CG_ITER] = 0.0; }
}
// one CG iteration after the product: Ap = (reduced B p - W C^-1 W^T p) + alpha p
template <int D>
__global__ __launch_bounds__(1024) void k_cg_step(int n, double alpha, double* __restrict__ Ap, double* __restrict__ pv,
                                                  double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                  const double* __restrict__ Minv, double* __restrict__ scal) {
  __shared__ double s_red[17];
  const double rz = scal[CG_RZ];
  double pAp = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) { const double ap = Ap[i] + alpha * pv[i]; Ap[i] = ap; pAp += pv[i] * ap; }
  pAp = block_sum1024(pAp, s_red);
  if (!(pAp > 0.0) || rz == 0.0) {            // S is not positive definite (or the residual vanished exactly): stop moving
    if (threadIdx.x == 0) { if (!(pAp > 0.0) && rz != 0.0) scal[CG_FAIL] = 2.0; scal[CG_RR] = (rz == 0.0) ? 0.0 : scal[CG_RR]; }
    return;
  }
  const double a = rz / pAp;
  for (int i = threadIdx.x; i < n; i += 1024) { x[i] += a * pv[i]; r[i] -= a * Ap[i]; }
  __syncthreads();                              // r complete before the block-wise preconditioner reads it
  double rz_new = 0.0, rr = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) {
    const double zi = precond_row<D>(Minv, r, i);
    z[i] = zi;
    rz_new += r[i] * zi; rr += r[i] * r[i];
  }
  rz_new = block_sum1024(rz_new, s_red);
  rr = block_sum1024(rr, s_red);
  const double beta = rz_new / rz;
  for (int i = threadIdx.x; i < n; i += 1024) pv[i] = z[i] + beta * pv[i];
  if (threadIdx.x == 0) { scal[CG_RZ] = rz_new; scal[CG_RR] = rr; scal[CG_ITER] += 1.0; }
}

namespace {
struct Pcg {
  sfm_ctx* h; sfm_ba_problem p; Lay L; double* ws; double alpha, rtol; int max_iter;
  sfm_reduce_fn reduce; void* user;
  int iters;
  bool stalled = false;      // a system ran out of iterations above rtol

  int red(double* ptr, int64_t count) {
    if (!reduce) return SFM_OK;
    return reduce(user, ptr, count, 0) ? sfm_fail(h, SFM_ERR_HIP, "sfm_ba_solve_pcg", "the reduce hook failed") : SFM_OK;
  }
  // this rank's part of (S - alpha I) v -> cg_Ap, reduced over the ranks
  int matvec(const double* v) {
    const int C = p->n_cams, P = p->n_pts, D = p->cam_dim, n = C * D;
    launch_obs_Gtp(h, p, L, v);
    hipLaunchKernelGGL(k_track_sum, dim3(cdiv(P, 256)), dim3(256), 0, h->stream, P, p->pt_ptr, WS(L, tmp3), WS(L, v));
    launch_cam_reduce_chunks(h, p, L, WS(L, v));
    DISPATCH_D(D, hipLaunchKernelGGL(k_cam_reduce_final_bv<DD>, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, C, p->cch_ptr, WS(L, cch_part),
                                     WS(L, B), v, WS(L, cg_Ap)));
    return red(WS(L, cg_Ap), n);
  }
  // x = S^-1 rhs (x, rhs: device vectors of n doubles, distinct from the cg_* work vectors)
  int solve(const double* rhs, double* x) {
    const int D = p->cam_dim, n = p->n_cams * D;
    DISPATCH_D(D, hipLaunchKernelGGL(k_cg_init<DD>, dim3(1), dim3(1024), 0, h->stream, n, rhs, WS(L, cg_Minv), x, WS(L, cg_r), WS(L, cg_z),
                                     WS(L, cg_p), WS(L, cg_scal)));
    const int check_every = 8;
    bool settled = false;                            // converged, or a failure the scalars already carry
    for (int it = 0; it < max_iter; ++it) {
      int rc = matvec(WS(L, cg_p)); if (rc) return rc;
      DISPATCH_D(D, hipLaunchKernelGGL(k_cg_step<DD>, dim3(1), dim3(1024), 0, h->stream, n, alpha, WS(L, cg_Ap), WS(L, cg_p), x, WS(L, cg_r),
                                       WS(L, cg_z), WS(L, cg_Minv), WS(L, cg_scal)));
      ++iters;
      if ((it + 1) % check_every == 0 || it + 1 == max_iter) {
        SFM_HIP(h, hipMemcpyAsync(h->pinned, WS(L, cg_scal), 8 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        SFM_HIP(h, hipStreamSynchronize(h->stream));
        const double rr = h->pinned[CG_RR], rr0 = h->pinned[CG_RR0];
        if (h->pinned[CG_FAIL] != 0.0 || !(rr == rr)) { settled = true; break; }     // reported through the scalars
        if (rr <= rtol * rtol * rr0) { settled = true; break; }
      }
    }
    // max_iter iterations without reaching rtol (the last look above was at it + 1 == max_iter): an inexact p and
    // p^T (H + alpha I)^-1 p would silently steer More's alpha update.  Measured on the goldens: near convergence of the
    // outer loop (alpha ~ 1e-3, S nearly singular along the 7 gauge directions) block-Jacobi PCG stalls at a relative
    // residual of 1e-2 .. 1e-4.  The caller (sfm_ba_solve_pcg) then solves THIS damped system by the formed-S route, as the
    // explicit-S CG falls back to its factorisation.
    if (!settled) {
      const double rr = h->pinned[CG_RR], rr0 = h->pinned[CG_RR0];
      const double rel = rr0 > 0.0 ? std::sqrt(rr / rr0) : 0.0;
      if (rel > p->pcg_worst_relres) p->pcg_worst_relres = rel;
      if (getenv("SFM_PCG_DEBUG")) fprintf(stderr, "sfm_amd pcg: alpha %.3e: %d iterations, relative residual %.3e (rtol %.1e): formed-S fallback\n", alpha, max_iter, rel, rtol);
      stalled = true;
    }
    SFM_LAUNCH_CHECK(h, "sfm_ba_solve_pcg");
    return SFM_OK;
  }
};
}  // namespace

// The damped system by the formed-S route (what the trust-region loop does with SFM_SOLVER_DENSE), for a system the
// implicit-Schur PCG could not bring to its tolerance.
static int pcg_fallback_dense(sfm_ctx* h, sfm_ba_problem p, const Lay& L, double alpha, int want_q, sfm_reduce_fn reduce, void* user) {
  char* base = (char*)p->workspace;
  sfm_ba_layout lay; sfm_ba_get_layout(p, &lay);
  auto red = [&](int64_t off, int64_t count) -> int {
    if (!reduce) return SFM_OK;
    return reduce(user, base + off, count, 0) ? sfm_fail(h, SFM_ERR_HIP, "sfm_ba_solve_pcg", "the reduce hook failed") : SFM_OK;
  };
  int rc;
  p->pcg_fallbacks++;
  if ((rc = sfm_ba_schur_build(h, p, alpha))) return rc;
  if (reduce) {
    if ((rc = sfm_ba_pack_system(h, p))) return rc;
    if ((rc = red(lay.reduce_Sp_off, lay.reduce_Sp_count))) return rc;
    if ((rc = sfm_ba_unpack_system(h, p))) return rc;
  }
  if ((rc = sfm_ba_schur_solve(h, p, alpha, want_q))) return rc;
  if ((rc = red(lay.reduce_q_off, lay.reduce_q_count))) return rc;
  return sfm_ba_finish_solve(h, p, want_q);
}

extern "C" int sfm_ba_solve_pcg(sfm_handle h, sfm_ba_problem p, double alpha, int want_q, double rtol, int32_t max_iter,
                                sfm_reduce_fn reduce, void* reduce_user, int32_t* iters_host) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  if (!(alpha > 0.0) || !(rtol > 0.0) || max_iter < 1) return sfm_fail(h, SFM_ERR_ARG, "sfm_ba_solve_pcg", "alpha, rtol > 0 and max_iter >= 1");
  double* ws = (double*)p->workspace;
  const int C = p->n_cams, D = p->cam_dim, n = C * D;
  Pcg cg{h, p, L, ws, alpha, rtol, max_iter, reduce, reduce_user, 0};
  if (reduce) p->sharded = 1;          // the formed-S fallback below solves a replicated camera system: same route on every rank
  SFM_HIP(h, hipMemsetAsync(WS(L, cg_scal), 0, CG_SCAL_WORDS * sizeof(double), h->stream));
  // point factors, G, and this rank's part of the right-hand side r = g_c - W C_a^-1 g_p and of the diagonal blocks
  sfm_prof_begin(h, SFM_PROF_BUILD_G);
  launch_build_G(h, p, L, alpha, nullptr);
  sfm_prof_end(h, SFM_PROF_BUILD_G);
  sfm_prof_begin(h, SFM_PROF_SCHUR);
  launch_cam_reduce_chunks(h, p, L, WS(L, e));
  DISPATCH_DT(D, p->precision, {
    if (p->n_cchunks > 0)
      hipLaunchKernelGGL((k_cam_gg_chunks<DD, double, GG>), dim3((unsigned)p->n_cchunks), dim3(128), 0, h->stream, p->cch_beg, p->cch_end,
                         p->cam_obs, WS(L, G), WS(L, cbl_part));
    launch_cam_reduce_final(h, p, L, WS(L, gc), WS(L, tvec), false);
    hipLaunchKernelGGL(k_cam_gg_final<DD>, dim3(cdiv((int64_t)n * DD, 256)), dim3(256), 0, h->stream, C, p->cch_ptr, WS(L, cbl_part),
                       WS(L, B), WS(L, cg_M));
  });
  sfm_prof_end(h, SFM_PROF_SCHUR);
  if ((rc = cg.red(WS(L, tvec), n))) return rc;
  if ((rc = cg.red(WS(L, cg_M), (int64_t)n * D))) return rc;
  sfm_prof_begin(h, SFM_PROF_CHOL);            // the slot of the camera solve: here the CG iterations
  DISPATCH_D(D, hipLaunchKernelGGL(k_precond_invert<DD>, dim3(cdiv(C, 64)), dim3(64), 0, h->stream, C, WS(L, cg_M), alpha, WS(L, cg_Minv),
                                   WS(L, cg_scal)));
  // y = S^-1 r ; p_c = -y
  if ((rc = cg.solve(WS(L, tvec), WS(L, y)))) return rc;
  if (cg.stalled) {
    sfm_prof_end(h, SFM_PROF_CHOL);
    if (iters_host) *iters_host = cg.iters;
    return pcg_fallback_dense(h, p, L, alpha, want_q, reduce, reduce_user);
  }
  ba_copy_neg(h, WS(L, y), WS(L, pc), n, -1.0);
  sfm_prof_end(h, SFM_PROF_CHOL);
  sfm_prof_begin(h, SFM_PROF_BACKSUB);
  // (not launch_backsub: here the point sums are always a launch of their own, ahead of the camera-wise pass, and
  // k_cam_reduce_final runs without its extra workgroup)
  launch_obs_Gtp(h, p, L, WS(L, pc));
  launch_backsub_points(h, p, L);
  ba_sum_partials(h, WS(L, part_pt), (int)L.nblk_pt, 2, WS(L, red_q) + n);
  if (want_q) {
    launch_cam_reduce_chunks(h, p, L, WS(L, v));
    launch_cam_reduce_final(h, p, L, nullptr, WS(L, red_q), false);
  }
  sfm_prof_end(h, SFM_PROF_BACKSUB);
  if ((rc = cg.red(WS(L, red_q), n + 2))) return rc;
  if (want_q) {
    // rhs2 = p_c - W C_a^-1 p_p ;  p^T (H + alpha I)^-1 p = rhs2^T S^-1 rhs2 + sum ||v||^2
    sfm_prof_begin(h, SFM_PROF_TRSV);
    ba_add_vec(h, WS(L, pc), WS(L, red_q), WS(L, tvec), n);
    if ((rc = cg.solve(WS(L, tvec), WS(L, y)))) return rc;
    if (cg.stalled) {
      sfm_prof_end(h, SFM_PROF_TRSV);
      if (iters_host) *iters_host = cg.iters;
      return pcg_fallback_dense(h, p, L, alpha, want_q, reduce, reduce_user);
    }
    ba_dot(h, n, WS(L, tvec), WS(L, y), WS(L, cg_scal) + CG_DOT);
    sfm_prof_end(h, SFM_PROF_TRSV);
  }
  launch_finish_solve_pcg(h, p, L, want_q, WS(L, cg_scal) + CG_DOT, WS(L, cg_scal) + CG_FAIL);
  SFM_LAUNCH_CHECK(h, "sfm_ba_solve_pcg");
  if (iters_host) *iters_host = cg.iters;
  return SFM_OK;
}
