// Bundle-adjustment stages for gfx950 (MI355X): residual + analytic Jacobian + Huber row
// scaling, block accumulation, damped Schur-complement solve.  fp64 throughout.  Here: the workspace layout, the Schur stage, shared
// vector kernels, the scalar read-back; ba_model.hip: the camera model (linearise, step, cost); ba_camera_cg.hip: the formed camera
// system; ba_pcg.hip: the implicit-Schur PCG; ba_device.h: device helpers; ba_stages.h: what one unit calls in another.
//
// What is computed (and for which reference lines) is documented in include/sfm_amd.h and
// DESIGN.md; the arithmetic mirrors oracle/ba_oracle.py statement by statement where the
// order of operations matters (Rodrigues coefficients, Huber scaling).
//
// Data layout in HBM (all inside the caller's workspace, see ba_layout()):
//   recA   [N][2D]    per observation, point-major: Jc~ rows (2xD)
//   recB   [N][8]     per observation: Jp~ rows (2x3), f~ (2)
//   G      [N][GS]    per observation, per alpha: W_k L_j^-T as [3][D]  (L_j L_j^T = C_j + alpha I)
// These three are the bulk of the traffic.  SFM_BA_MIXED stores the Jacobian records recA / recB in float32 (the
// "mixed-precision Jacobian" of BASELINE.json config 5); everything derived from them - B, C, g, G, S, the step - is
// computed and kept in float64 FROM THE ROUNDED ROWS, so S stays the exact Schur complement of a (slightly
// perturbed) Jacobian and therefore positive definite for every alpha > 0.  G itself must not be rounded: with G in
// float32 S = B - sum G G^T loses definiteness in the 7 gauge directions (eigenvalue alpha) as soon as
// alpha < ~1e-7 max diag(H) - measured: the zero-noise goldens then fail in the factorisation (the kernels keep the
// storage type of G as a template parameter; only double is instantiated).
//   S | r  [(n+1)][n] reduced camera system with its right-hand side as a bordered row
// Observations of one point (a track) are contiguous; cameras are reached through cam_obs.
#include "ba_internal.h"
#include "ba_device.h"
#include <atomic>

// ------------------------------------------------------------------------------------ layout
// Stride of a G block in doubles.  D = 10: 32 = 256 bytes, so that a block is exactly two whole 128-byte lines - the Schur
// gather is bound by the lines it pulls through the fabric, and a 240-byte block at 16-byte alignment straddles 2.75 on
// average: k_schur_items 357 -> 305 us, fabric traffic 2.34 -> 1.94 GB per launch (round 3, profiles/).  D = 6: 18 doubles =
// 144 bytes straddle exactly two lines at any 16-byte offset already.  The strides DISPATCH_DT instantiates (GG) must match.
static int64_t g_stride(int64_t D) { return D == 10 ? 32 : 3 * D; }
Lay ba_layout(int64_t C, int64_t P, int64_t N, int64_t D, int64_t n_items, int64_t n_cchunks, int precision) {
  Lay L;
  int64_t o = 0, n = C * D;
  auto take = [&](int64_t cnt) { int64_t r = o; o = align_up(o + cnt, 32); return r; };
  // record arrays: float64, or float32 in mixed precision (sized in doubles either way)
  const int64_t es = precision == SFM_BA_MIXED ? 4 : 8;
  auto take_rec = [&](int64_t elems) { return take((elems * es + 7) / 8); };
  L.nblk_obs = (N + 255) / 256;
  L.nblk_pt = (P + 255) / 256;
  L.recA = take_rec(N * 2 * D);
  L.recB = take_rec(N * 8);
  L.campre = take(C * CAMPRE);
  L.campre2 = take(C * CAMPRE);
  L.B = take(C * D * D);
  L.gc = take(n);
  L.Cp = take(P * 6);
  L.gp = take(P * 3);
  L.Linv = take(P * 6);
  L.e = take(P * 3);
  L.v = take(P * 3);
  L.tmp3 = take(N * 3);
  L.G = take(N * g_stride(D));                     // always float64 (see the header of this file)
  L.eobs = take(N * 3);                 // e_j = M g_pj copied per observation (read with the G row by the diagonal Schur items)
  L.red_lin = take(2 * n + 2);
  L.gmax = take(2);
  L.red_S = take(n * n + n);
  L.red_q = take(n + 2);
  L.red_step = take(8);
  L.pc = take(n);
  L.pp = take(P * 3);
  L.y = take(n);
  L.tvec = take(n);
  L.scalars = take(SFM_SC_COUNT);
  L.part_obs = take(L.nblk_obs * 2 * 4 + 4);
  L.part_pt = take(L.nblk_pt * 4);
  L.part_x = take(((n + 3 * P + 255) / 256) * 2 + 2);
  L.cost_reg = take(C * 4);
  L.regrec = take(C * 20);
  L.dense = take(dense_ws_doubles((int)n));
  L.sch_part = take(n_items * D * D);
  L.cch_part = take(n_cchunks * 16);
  L.cbl_part = take(n_cchunks * (D * D + D));
  // implicit-Schur PCG (sfm_ba_solve_pcg): residual, preconditioned residual, direction, S p; block-Jacobi blocks
  L.cg_r = take(n); L.cg_z = take(n); L.cg_p = take(n); L.cg_Ap = take(n);
  L.cg_M = take(C * D * D); L.cg_Minv = take(C * D * D);
  L.cg_scal = take(CG_SCAL_WORDS);       // status words of the camera CG
  L.cg_mail = take(4 * n);               // k_cgs_persist: two slots of n doubles as pairs of 8-byte {tag, half} granules
  L.total = o;
  return L;
}

extern "C" int sfm_ba_get_layout(sfm_ba_problem p, sfm_ba_layout* out) {
  if (!p || !out) return SFM_ERR_ARG;
  const Lay& L = p->L;
  const int64_t n = (int64_t)p->n_cams * p->cam_dim;
  const int64_t es = p->precision == SFM_BA_MIXED ? 4 : 8;
  out->total_bytes = L.total * 8;
  out->rec_off = L.recA * 8; out->rec_stride = 2 * p->cam_dim * es;
  out->recB_off = L.recB * 8;
  out->B_off = L.B * 8; out->gc_off = L.gc * 8;
  out->Cp_off = L.Cp * 8; out->gp_off = L.gp * 8;
  out->reduce_lin_off = L.red_lin * 8; out->reduce_lin_count = 2 * n + 2;
  out->gmax_off = L.gmax * 8;
  out->reduce_S_off = L.red_S * 8; out->reduce_S_count = n * n + n;
  out->reduce_Sp_off = (L.dense + dense_ws_lm_offset((int)n)) * 8;   // the factor's buffer: free until the factorisation
  out->reduce_Sp_count = n * (n + 1) / 2 + n;
  out->reduce_q_off = L.red_q * 8; out->reduce_q_count = n + 2;
  out->reduce_step_off = L.red_step * 8; out->reduce_step_count = 5;
  out->pc_off = L.pc * 8; out->pp_off = L.pp * 8;
  out->scalars_off = L.scalars * 8;
  out->G_off = L.G * 8;
  out->cg_Ap_off = L.cg_Ap * 8; out->cg_M_off = L.cg_M * 8;
  return SFM_OK;
}

// ------------------------------------------------------------------------------------ damped solve: point side
// L_j L_j^T = C_j + alpha I ; stores M = L_j^-1 (lower, packed m00 m10 m11 m20 m21 m22) and e_j = M g_pj.
// M = L^-1 (packed m00 m10 m11 m20 m21 m22) of L L^T = C_j + alpha I, and e_j = M g_pj: the SAME statements wherever a kernel needs
// them (k_build_G forms them per observation instead of fetching what a kernel of its own had stored)
__device__ __forceinline__ void point_factor_vals(const double* __restrict__ c, const double* __restrict__ g, double alpha,
                                                  double (&m)[6], double (&ev)[3]) {
  const double a00 = c[0] + alpha, a10 = c[1], a20 = c[2], a11 = c[3] + alpha, a21 = c[4], a22 = c[5] + alpha;
  const double l00 = sqrt(a00), l10 = a10 / l00, l20 = a20 / l00;
  const double l11 = sqrt(a11 - l10 * l10), l21 = (a21 - l20 * l10) / l11;
  const double l22 = sqrt(a22 - l20 * l20 - l21 * l21);
  const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
  const double m10 = -l10 * m00 * m11, m21 = -l21 * m11 * m22;
  const double m20 = -(l20 * m00 + l21 * m10) * m22;
  m[0] = m00; m[1] = m10; m[2] = m11; m[3] = m20; m[4] = m21; m[5] = m22;
  const double g0 = g[0], g1 = g[1], g2 = g[2];
  ev[0] = m00 * g0;
  ev[1] = m10 * g0 + m11 * g1;
  ev[2] = m20 * g0 + m21 * g1 + m22 * g2;
}

// G_k[m][a] = sum_r Jc~[r][a] * V[r][m],  V = Jp~ M^T (2x3); e_j copied next to the observation (k_schur_items, diagonal
// items).  One thread per observation, 256 observations per workgroup, and - as in k_lin_obs - both directions pass through
// LDS so that HBM only sees contiguous streams: the Jacobian rows of the 256 observations come in as one flat coalesced
// read, every thread picks its 2 D + 6 values out of LDS (odd row stride: no bank conflicts), gathers its point's M (six
// doubles; the ten observations of a track share them) and leaves its GS outputs in the same LDS buffer, which then goes
// out as 16-byte stores, 64 KB contiguous per workgroup (GS = 32: the padding doubles are written as zeros).
// Round 2's form (16 lanes per observation, three 8-byte stores per lane 80 bytes apart) moved the same bytes at 3.3 TB/s.
template <int D, typename T, typename TG, int GS>
__global__ __launch_bounds__(256) void k_build_G(int64_t N, const int* __restrict__ pt_idx,
                                                 const T* __restrict__ recA, const T* __restrict__ recB,
                                                 double* __restrict__ Linv, TG* __restrict__ G,
                                                 double* __restrict__ e, double* __restrict__ eobs,
                                                 const double* __restrict__ Cp, const double* __restrict__ gp, double alpha, int P,
                                                 unsigned nblk_obs, double* __restrict__ cg_scal /* may be null */) {
  static_assert(GS % 2 == 0 && GS >= 3 * D, "G blocks are written as 16-byte pieces");
  // the status words of the camera CG that follows start from zero: cleared HERE, by the first kernel of
  // sfm_ba_schur_build, instead of by a memset between two kernels of the chain (a fill kernel of its own, ~5 us with its
  // boundaries) - and before k_schur_assemble, whose diagonal-block workgroups may RAISE the failure word
  if (cg_scal && blockIdx.x == 0 && threadIdx.x < CG_SCAL_WORDS) cg_scal[threadIdx.x] = 0.0;
  // The point factors M_j = L_j^-1 and e_j = M_j g_pj for the kernels further down the chain (k_backsub, the camera-wise passes)
  // are the work of the LAST cdiv(P, 256) workgroups of this launch - a kernel of its own until round 4 (k_point_factor: 6 us
  // and a boundary in front of every damped solve).  The observation workgroups do not wait for them: every observation forms
  // its point's M and e itself, from the same six + three doubles by the same statements (point_factor_vals).
  if (blockIdx.x >= nblk_obs) {
    const int j = (int)(blockIdx.x - nblk_obs) * 256 + (int)threadIdx.x;
    if (j < P) {
      double m[6], ev[3];
      point_factor_vals(Cp + (size_t)j * 6, gp + (size_t)j * 3, alpha, m, ev);
#pragma unroll
      for (int q = 0; q < 6; ++q) Linv[(size_t)j * 6 + q] = m[q];
#pragma unroll
      for (int q = 0; q < 3; ++q) e[(size_t)j * 3 + q] = ev[q];
    }
    return;
  }
  constexpr int WA = 2 * D, LDA = WA + 1, LDB = 9, LDG = GS + 1;
  constexpr int VE = 16 / (int)sizeof(T);                // elements per 16-byte load
  constexpr int NA = WA / VE, NB = 8 / VE;               // 16-byte loads per thread for the two record arrays of 256 observations
  static_assert(WA % VE == 0 && 8 % VE == 0, "record rows are whole 16-byte pieces");
  constexpr int IN_DOUBLES = 256 * (LDA + LDB), OUT_DOUBLES = 256 * LDG;
  __shared__ double s_buf[IN_DOUBLES > OUT_DOUBLES ? IN_DOUBLES : OUT_DOUBLES];
  double* s_jp = s_buf + 256 * LDA;                       // recB records, stride 9
  typedef T vec_t __attribute__((ext_vector_type(VE)));
  const int tid = threadIdx.x;
  const int64_t k0 = (int64_t)blockIdx.x * 256;
  const int nvalid = (int)((N - k0) < 256 ? (N - k0) : 256);
  const bool live = tid < nvalid;
  // every global load of the workgroup is issued before anything waits: the point id first (the M / e gathers depend on it),
  // then the flat, coalesced 16-byte pieces of the two record arrays, then the gathers
  const int64_t k = k0 + tid;
  const int64_t pj = live ? pt_idx[k] : 0;
  vec_t la[NA], lb[NB];
  {
    const vec_t* inA = (const vec_t*)(recA + (size_t)k0 * WA);
    const vec_t* inB = (const vec_t*)(recB + (size_t)k0 * 8);
#pragma unroll
    for (int j = 0; j < NA; ++j) { const int i = tid + 256 * j; la[j] = i * VE < nvalid * WA ? inA[i] : (vec_t)(T)0; }
#pragma unroll
    for (int j = 0; j < NB; ++j) { const int i = tid + 256 * j; lb[j] = i * VE < nvalid * 8 ? inB[i] : (vec_t)(T)0; }
  }
  double cpj[6], gpj[3];
#pragma unroll
  for (int q = 0; q < 6; ++q) cpj[q] = Cp[(size_t)pj * 6 + q];
#pragma unroll
  for (int q = 0; q < 3; ++q) gpj[q] = gp[(size_t)pj * 3 + q];
#pragma unroll
  for (int j = 0; j < NA; ++j)
#pragma unroll
    for (int v = 0; v < VE; ++v) { const int i = (tid + 256 * j) * VE + v, t = i / WA, q = i - t * WA; s_buf[t * LDA + q] = (double)la[j][v]; }
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int v = 0; v < VE; ++v) { const int i = (tid + 256 * j) * VE + v; s_jp[(i >> 3) * LDB + (i & 7)] = (double)lb[j][v]; }
  __syncthreads();
  double mq[6], eq[3];
  point_factor_vals(cpj, gpj, alpha, mq, eq);
  const double m00 = mq[0], m10 = mq[1], m11 = mq[2], m20 = mq[3], m21 = mq[4], m22 = mq[5];
  const double e0 = eq[0], e1 = eq[1], e2 = eq[2];
  double g[3 * D];
  {
    const double* jp = &s_jp[tid * LDB];
    const double j0 = jp[0], j1 = jp[1], j2 = jp[2], j3 = jp[3], j4 = jp[4], j5 = jp[5];
    // V[r][m] = sum_q Jp~[r][q] M[m][q]  (M lower triangular)
    const double v00 = j0 * m00, v01 = j0 * m10 + j1 * m11, v02 = j0 * m20 + j1 * m21 + j2 * m22;
    const double v10 = j3 * m00, v11 = j3 * m10 + j4 * m11, v12 = j3 * m20 + j4 * m21 + j5 * m22;
    const double* my = &s_buf[tid * LDA];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      const double c0 = my[a], c1 = my[D + a];
      g[a] = c0 * v00 + c1 * v10;
      g[D + a] = c0 * v01 + c1 * v11;
      g[2 * D + a] = c0 * v02 + c1 * v12;
    }
  }
  if (live) { eobs[k * 3] = e0; eobs[k * 3 + 1] = e1; eobs[k * 3 + 2] = e2; }
  __syncthreads();                                      // everybody has its inputs in registers: the buffer becomes the output stage
  {
    double* my = &s_buf[tid * LDG];
#pragma unroll
    for (int q = 0; q < 3 * D; ++q) my[q] = g[q];
#pragma unroll
    for (int q = 3 * D; q < GS; ++q) my[q] = 0.0;       // padding of the block (read as part of a 16-byte chunk, never used)
  }
  __syncthreads();
  {
    typedef TG pair_t __attribute__((ext_vector_type(2)));
    pair_t* outp = (pair_t*)(G + (size_t)k0 * GS);
    constexpr int HP = GS / 2;
#pragma unroll
    for (int j = 0; j < HP; ++j) {
      const int i = tid + 256 * j;
      if (i < nvalid * HP) {
        const int t = i / HP, q = 2 * (i - t * HP);
        pair_t v; v.x = (TG)s_buf[t * LDG + q]; v.y = (TG)s_buf[t * LDG + q + 1];
        outp[i] = v;
      }
    }
  }
}

// Reduced camera system  S[c][c2] = [c == c2] B_c - sum_{(k,k2) on a shared track} G_k G_k2^T  (c <= c2, mirrored).
// The pair list of a block is cut into work items of <= 256 pairs (sfm_amd/structure.py; the items of a block of >= 3 items
// interleaved pair by pair, so that all items of a block row walk the row camera's observation list in step: k_item_desc); ONE wavefront per
// item accumulates its 16x16 tile on v_mfma_f64_16x16x4_f64 as a K = 4 (3 used) x n_pairs contraction:
// lane l feeds A[row l&15][k l>>4] = G_k[m = l>>4][row], B likewise from G_k2; C/D: col = l&15,
// row = (l>>4) + 4*reg.  Pair ids are loaded 64 at a time (coalesced) and broadcast with v_readlane so the
// 16 gathers of 8 pairs are in flight together.  k_schur_assemble then sums the items of each block in
// order (bitwise reproducible), adds B_c on the diagonal and writes the block and its mirror.
// build-time tuning knobs of the gather: waves per SIMD the register budget is cut for, and 16-byte chunk loads in flight per
// operand and wave.  Measured (round 3, tools/exp_schur_occupancy.sh; us per launch):
//   (waves, loads)     d = 10 random   d = 6 random   d = 10 coherent scene
//   (5, 8)                  312             349              335
//   (6, 6)                  312             325              342
//   (7, 5)                  307             313              346
//   (8, 4)                  306             309              351
// More waves hide the LDS / MFMA phases of each other - decisive for d = 6, whose 7-block slabs and 63 loader lanes leave
// more of those - but they also widen the set of lines in flight per XCD and cost L2 hits on the k side (31 % -> 28 % of the
// line requests on the random scene, 19 % -> 14 % on the coherent one).  Shipped: (5, 8) for d = 10, (8, 4) for d = 6.
#ifndef SFM_SCHUR_WAVES_D10
#define SFM_SCHUR_WAVES_D10 5
#endif
#ifndef SFM_SCHUR_U_D10
#define SFM_SCHUR_U_D10 8
#endif
#ifndef SFM_SCHUR_WAVES_D6
#define SFM_SCHUR_WAVES_D6 8
#endif
#ifndef SFM_SCHUR_U_D6
#define SFM_SCHUR_U_D6 4
#endif
#ifdef SFM_SCHUR_WAVES          /* one setting for both block sizes (the experiment scripts) */
#undef SFM_SCHUR_WAVES_D10
#undef SFM_SCHUR_WAVES_D6
#define SFM_SCHUR_WAVES_D10 SFM_SCHUR_WAVES
#define SFM_SCHUR_WAVES_D6 SFM_SCHUR_WAVES
#endif
#ifdef SFM_SCHUR_U
#undef SFM_SCHUR_U_D10
#undef SFM_SCHUR_U_D6
#define SFM_SCHUR_U_D10 SFM_SCHUR_U
#define SFM_SCHUR_U_D6 SFM_SCHUR_U
#endif
// Diagnostic build only (-DSFM_SCHUR_STAMPS=1, tools/exp_schur_lifetimes.sh): begin / end of every wave of k_schur_items on the
// 100 MHz constant clock, with its item's pair count and the place it ran.  The shipped library executes no stamp.
#ifndef SFM_SCHUR_STAMPS
#define SFM_SCHUR_STAMPS 0
#endif
#if SFM_SCHUR_STAMPS
constexpr int SCHUR_STAMP_WAVES = 1 << 16;
__device__ unsigned long long g_schur_stamps[SCHUR_STAMP_WAVES * 4];
extern "C" int sfm_debug_schur_stamps(unsigned long long* dst, int n_words) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_schur_stamps), (size_t)n_words * 8, 0, hipMemcpyDeviceToHost);
}
#define SCHUR_STAMP_BEGIN() const unsigned long long stamp_t0 = __builtin_amdgcn_s_memrealtime()
#define SCHUR_STAMP_END(npairs, isdiag) do { const unsigned wv = blockIdx.x * SFM_SCHUR_WG_WAVES + (threadIdx.x >> 6); if ((threadIdx.x & 63) == 0 && wv < SCHUR_STAMP_WAVES) { \
    unsigned long long* o = g_schur_stamps + (size_t)wv * 4; \
    o[0] = stamp_t0; o[1] = __builtin_amdgcn_s_memrealtime(); \
    o[2] = ((unsigned long long)(unsigned)(npairs) << 32) | (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4); \
    o[3] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 20) | ((unsigned long long)((isdiag) ? 1 : 0) << 32); } } while (0)
#else
#define SCHUR_STAMP_BEGIN() do {} while (0)
#define SCHUR_STAMP_END(npairs, isdiag) do {} while (0)
#endif
// waves per workgroup of k_schur_items (its waves never meet: no barrier, wave-private LDS).  ONE: a wave slot is handed back
// when its wave ends, not when the slowest of four does.  Wave begin / end stamps (tools/exp_schur_lifetimes.sh, cfg4): with
// four waves per workgroup 4,400-4,800 of the 5,120 wave slots were occupied through the bulk of the launch, with one 4,850-
// 5,050; span 309-311 -> 302-303 us (a wave lives 53 -> 55 us: the gather is bandwidth-bound, the gain is the filled slots).
#ifndef SFM_SCHUR_WG_WAVES
#define SFM_SCHUR_WG_WAVES 1
#endif
template <int D, typename T, int GS>
__global__ __launch_bounds__(64 * SFM_SCHUR_WG_WAVES) __attribute__((amdgpu_waves_per_eu(D == 6 ? SFM_SCHUR_WAVES_D6 : SFM_SCHUR_WAVES_D10, D == 6 ? SFM_SCHUR_WAVES_D6 : SFM_SCHUR_WAVES_D10))) void k_schur_items(const int* __restrict__ xcd_ptr, const int* __restrict__ xcd_items,
                                                     const int* __restrict__ it_first,
                                                     const int* __restrict__ it_stride,
                                                     const int* __restrict__ it_cnt,
                                                     const int* __restrict__ pair_k, const int* __restrict__ pair_k2,
                                                     const T* __restrict__ G, double* __restrict__ part,
                                                     const int* __restrict__ cam_idx,
                                                     const int* __restrict__ item_ptr, const int* __restrict__ cch_ptr, int n_cams,
                                                     const double* __restrict__ eobs, double* __restrict__ cch_part,
                                                     int fuse_rhs) {
  // Gathers are latency-bound (about 5 us under load), so what counts is useful bytes in flight per register:
  // a G block is BB bytes = CH 16-byte chunks, one lane fetches one chunk (global_load_dwordx4) and one
  // instruction fetches BPL whole blocks (float64 D = 10: 4 blocks on 60 lanes, D = 6: 7 on 63; float32 D = 10:
  // 8 blocks = 8 full 128-byte lines on 64 lanes, D = 6: 12 on 60) - at least twice the bytes per VGPR of a
  // one-element-per-lane gather that only 30 of 64 lanes take part in.  The blocks then pass through a
  // wave-private LDS slab to reach the MFMA operand layout (lane = (row, m)), widened to float64 there.
  //
  // Items of a DIAGONAL block (c, c) hold only self-pairs (k, k): one gather serves both operands, and the product's
  // spare column D carries the right-hand side with it - B operand column D = e_j (the point's M g_p), so the same MFMA
  // leaves sum_k G_k e_j in accumulator column D.  It goes to the chunk partials k_cam_reduce_final turns into
  // r_c = g_c - sum (item piece i of block (c, c) <-> observation chunk i of camera c: both cut the camera's list by 256),
  // which spares the separate pass over G for the right-hand side (72 us, a gather by camera, per damped solve).
  typedef int chunk_t __attribute__((ext_vector_type(4)));
  constexpr int BB = GS * (int)sizeof(T);      // bytes per G block
  static_assert(BB % 16 == 0, "a G block must be a whole number of 16-byte chunks");
  static_assert(D < 16, "column D of the 16 x 16 product is the right-hand side");
  constexpr int CH = BB / 16;                  // 16-byte chunks per block
  constexpr int BPL = 64 / CH;                 // blocks per load instruction
  constexpr int UMAX = D == 6 ? SFM_SCHUR_U_D6 : SFM_SCHUR_U_D10;
  constexpr int U = (64 + BPL - 1) / BPL < UMAX ? (64 + BPL - 1) / BPL : UMAX;   // load instructions in flight per operand
  constexpr int PB = U * BPL;                  // pairs per batch
  constexpr int WGW = SFM_SCHUR_WG_WAVES;
  __shared__ __attribute__((aligned(16))) char s_stage[WGW][2][BPL * BB + 16];   // + a slot that always reads as zero
  __shared__ double s_e[WGW][64][3];           // diagonal items: e_j of the 64 pairs whose ids the wave holds
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // workgroup b serves item group b % 8 (a set of whole block rows, problem.hip): with the round-robin XCD placement one
  // XCD sees every item of a camera's block row, so that camera's G blocks (1.2 MB at 5,000 observations) are
  // re-read from its 4 MB L2 instead of the fabric (speed only - any placement gives the same result)
  const int grp = blockIdx.x & 7;
  const int pos = xcd_ptr[grp] + (blockIdx.x >> 3) * WGW + w;
  if (pos >= xcd_ptr[grp + 1]) return;
  SCHUR_STAMP_BEGIN();
  // (the item and its bounds are the same for the whole wave: in SGPRs, so that every loop bound below is scalar - as per-lane
  // loads they put the trip count of the MFMA loop into a VGPR and an exec-mask dance around every MFMA)
  const int it = __builtin_amdgcn_readfirstlane(xcd_items[pos]);
  // the item walks pairs first + j * stride, j < n (problem.hip, k_item_desc: stride 1, or the item count of an interleaved block -
  // then the lanes' id loads are strided, over lines the block's other items ask for at the same time)
  const int first = __builtin_amdgcn_readfirstlane(it_first[it]), stride = __builtin_amdgcn_readfirstlane(it_stride[it]);
  const int n = __builtin_amdgcn_readfirstlane(it_cnt[it]);
  const int row = lane & 15, m = lane >> 4;
  const int lb = lane / CH, lc = lane - lb * CH;          // this lane's block / chunk within a load
  const bool loader = lb < BPL;
  char* sA = s_stage[w][0];
  char* sB = s_stage[w][1];
  const char* Gb = (const char*)G;
  v4d acc = {0.0, 0.0, 0.0, 0.0};
  const int k_first = __builtin_amdgcn_readfirstlane(pair_k[first]), k2_first = __builtin_amdgcn_readfirstlane(pair_k2[first]);
  // wave-uniform.  A diagonal block holds nothing but self-pairs UNLESS a camera appears twice on a track (fuse_rhs == 0,
  // sfm_ba_prob::has_dup): then it is processed like any other block and the right-hand side comes from k_cam_reduce_chunks
  const bool diag = fuse_rhs && k_first == k2_first;
  // K-packed form (see the MFMA loop): slot s = 4 j + m of MFMA j -> pair s / 3 of the slab, point coordinate s % 3
  constexpr int NM = (3 * BPL + 3) / 4;                   // MFMAs per full slab (3 for 4 pairs, 6 for 7)
  const bool krow = row < D, ke_lane = row == D;
  // LDS element of this lane's slot in MFMA j; lanes without one (row >= D, or a slot beyond the slab) read the slab's ZERO SLOT:
  // an unconditional ds_read where a predicated one cost an exec-masked block with its zero fill per operand
  constexpr int ZSLOT = BPL * GS;
  int koff[NM];
#pragma unroll
  for (int j = 0; j < NM; ++j) {
    const int sl = 4 * j + m, pi = (sl * 11) >> 5;        // sl / 3 for sl < 32
    koff[j] = (pi < BPL && krow) ? pi * GS + (sl - 3 * pi) * D + row : ZSLOT;
  }
  if (lane < 2) { ((double*)sA)[ZSLOT + lane] = 0.0; ((double*)sB)[ZSLOT + lane] = 0.0; }
  // two instantiations of the item loop (the off-diagonal one is the kernel as it was: nothing of the diagonal path in it)
  auto run = [&](auto diag_c) __attribute__((always_inline)) {
    constexpr bool DIAG = decltype(diag_c)::value;
    // (the pair ids of the NEXT 64 pairs are asked for while the present 64 are worked on)
    int kk_n = lane < n ? pair_k[first + lane * stride] : 0;
    int kk2_n = DIAG ? kk_n : (lane < n ? pair_k2[first + lane * stride] : 0);
    for (int base = 0; base < n; base += 64) {
      const int kk = kk_n, kk2 = kk2_n;
      if (base + 64 < n) {                                 // wave-uniform
        const int jn = base + 64 + lane;
        kk_n = jn < n ? pair_k[first + jn * stride] : 0;
        kk2_n = DIAG ? kk_n : (jn < n ? pair_k2[first + jn * stride] : 0);
      }
      const int cnt = (n - base) < 64 ? (n - base) : 64;
      if (DIAG) {
        // e_j of this lane's pair (the per-observation copy k_build_G leaves) -> LDS, in flight together with the G loads
        // of the batch below
        const double* ej = eobs + (size_t)kk * 3;
        const double e0 = ej[0], e1 = ej[1], e2 = ej[2];
        s_e[w][lane][0] = e0; s_e[w][lane][1] = e1; s_e[w][lane][2] = e2;
      }
      for (int u0 = 0; u0 < cnt; u0 += PB) {
        chunk_t ra[U], rb[U];
        // (Measured and not kept: every lane loading unconditionally, surplus lanes fetching the item's last pair again - 292
        // against 287 us; G through a buffer resource with 32-bit offsets and zeros beyond the end, all 16 loads back to back -
        // 295: tools/experiments/README.md.)
        if (u0 + PB <= cnt) {
          // a FULL batch (the usual case: every batch of a 256-pair item but perhaps its last): every pair exists, so no load
          // needs its predicate - no exec-masked block around each of the 16 loads (the one lane beyond the last block of a
          // load, d = 6, fetches that block's neighbour once more and does not store it)
#pragma unroll
          for (int t = 0; t < U; ++t) {
            const int p = u0 + t * BPL + (loader ? lb : BPL - 1);
            ra[t] = *(const chunk_t*)(Gb + (size_t)(unsigned)__shfl(kk, p, 64) * BB + 16 * lc);
            if (!DIAG) rb[t] = *(const chunk_t*)(Gb + (size_t)(unsigned)__shfl(kk2, p, 64) * BB + 16 * lc);
          }
        } else
#pragma unroll
        for (int t = 0; t < U; ++t) {
          const int p = u0 + t * BPL + lb;                  // pair this lane fetches a chunk of
          const int k = __shfl(kk, p & 63, 64);
          const bool ok = loader && p < cnt;
          ra[t] = ok ? *(const chunk_t*)(Gb + (size_t)k * BB + 16 * lc) : (chunk_t){0, 0, 0, 0};
          if (!DIAG) {
            const int k2 = __shfl(kk2, p & 63, 64);
            rb[t] = ok ? *(const chunk_t*)(Gb + (size_t)k2 * BB + 16 * lc) : (chunk_t){0, 0, 0, 0};
          }
        }
#pragma unroll
        for (int t = 0; t < U; ++t) {
          if (u0 + t * BPL >= cnt) break;                   // wave-uniform
          if (loader) {
            *(chunk_t*)(sA + lb * BB + 16 * lc) = ra[t];
            if (!DIAG) *(chunk_t*)(sB + lb * BB + 16 * lc) = rb[t];
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          // the contraction index of a slab is (pair, m): 3 nb slots for nb pairs, 4 per MFMA - four pairs = 12 slots = 3 FULL
          // v_mfma_f64_16x16x4 instead of 4 with K = 3 of 4 used.  Slot s = 4 j + (lane >> 4) of MFMA j reads pair s / 3,
          // m = s % 3 (offsets precomputed per lane: koff[j]); pairs past the end of the item were stored as zeros.
          // ALL operands of the slab are read before the first MFMA (one LDS latency per slab, not one per MFMA).
          const int nb = (cnt - (u0 + t * BPL)) < BPL ? (cnt - (u0 + t * BPL)) : BPL;
          const int nm = (3 * nb + 3) >> 2;
          // (d = 6 runs at 8 waves per SIMD on 64 registers: its six MFMAs per slab take their operands one at a time)
          constexpr int PFN = D == 6 ? 1 : NM;
#pragma unroll
          for (int j0 = 0; j0 < NM; j0 += PFN) {
            if (j0 >= nm) break;                            // wave-uniform
            double av[PFN], bv[PFN];
#pragma unroll
            for (int q = 0; q < PFN; ++q) {
              const int j = j0 + q;
              if (j < NM) {
                const int ko = koff[j];
                av[q] = (double)((const T*)sA)[ko];
                if (DIAG) {
                  const int sl = 4 * j + m, pi = (sl * 11) >> 5;
                  bv[q] = ko != ZSLOT ? av[q] : ((ke_lane && pi < nb) ? s_e[w][u0 + t * BPL + pi][sl - 3 * pi] : 0.0);
                } else bv[q] = (double)((const T*)sB)[ko];
              }
            }
#pragma unroll
            for (int q = 0; q < PFN; ++q) {
              if (j0 + q >= nm || j0 + q >= NM) break;      // wave-uniform
              acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[q], bv[q], acc, 0, 0, 0);
            }
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // the slab is rewritten by the next t
        }
      }
    }
  };
  if (diag) run(std::true_type{}); else run(std::false_type{});
  const int col = lane & 15;
  if (col < D) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = (lane >> 4) + 4 * i;
      if (rr < D) part[(size_t)it * (D * D) + rr * D + col] = acc[i];
    }
  } else if (diag && col == D) {
    // piece number of this item inside block (c, c) = chunk number inside camera c
    const int c = cam_idx[k_first];
    const int64_t blk = (int64_t)c * n_cams - (int64_t)c * (c - 1) / 2;
    const int ch = cch_ptr[c] + (it - item_ptr[blk]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rr = (lane >> 4) + 4 * i;
      if (rr < D) cch_part[(size_t)ch * 16 + rr] = acc[i];
    }
  }
  SCHUR_STAMP_END(n, diag);
}

// grid (C, ceil(C / ASM_NB)), 128 threads: workgroup (r, y) sums the item tiles of the blocks (r, c), c = ASM_NB y .. <= r, of the
// LOWER triangle of S - thread e < D * D owns element (e / D, e % D) of every one of them - and writes its strip as whole rows of
// up to ASM_NB D doubles through LDS.  ONLY THE LOWER TRIANGLE of S is ever read (k_diag_einv, k_scale_system, the multi-rank
// exchange sfm_ba_pack_system, the factorisation: test_upper_triangle_of_S_is_never_read poisons the rest), so nothing else is
// written; the items hold the UPPER blocks (c, r), c <= r, so element (rr, col) of block (r, c) is the transposed element of the
// item tiles.  (The first form wrote each block by itself, and its mirror: 80-byte row segments, 0.42 ms at 1000 cameras.)
// E_r = chol(S_rr + alpha I) and E_r^-1 by the first D lanes of a wave: lane i owns row i of L and, afterwards, column i of L^-1;
// what another lane holds comes by shuffle.  blk: the block's element (0, 0) in LDS (row stride ld; only its lower triangle is
// read).  The same operations in the same order as small_chol_inverse: bit for bit the factors k_diag_einv produces.
template <int D>
__device__ __forceinline__ void diag_block_factor_lanes(const double* blk, int ld, double alpha, int i, int r,
                                                        double* __restrict__ Einv, double* __restrict__ Efac, double* __restrict__ cg_scal) {
  double Lr[D], Xc[D];
#pragma unroll
  for (int k = 0; k < D; ++k) Lr[k] = (k <= i) ? blk[i * ld + k] + (i == k ? alpha : 0.0) : 0.0;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    double sum = Lr[j];
#pragma unroll
    for (int k = 0; k < j; ++k) sum = fma(-Lr[k], Lr[k], sum);  // (lane j's value is the pivot's)
    double piv = __shfl(sum, j, 64);
    if (!(piv > 0.0)) { ok = false; piv = 1.0; }
    const double l = sqrt(piv);
    double t = Lr[j];
#pragma unroll
    for (int k = 0; k < j; ++k) t = fma(-Lr[k], __shfl(Lr[k], j, 64), t);
    Lr[j] = (i == j) ? l : (i > j ? t / l : Lr[j]);
  }
  // column i of X = L^-1:  X[rw][i] = ([rw == i] - sum_{i <= k < rw} L[rw][k] X[k][i]) / L[rw][rw]
#pragma unroll
  for (int rw = 0; rw < D; ++rw) {
    double sum = (rw == i) ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < rw; ++k) {
      const double lrk = __shfl(Lr[k], rw, 64);
      // (a fused multiply-add where k_diag_einv's unrolled `sum -= L[r][k] * X[k][t]` gets one: a product rounded on its own -
      // what a select between product and zero compiles to - differs in the last bit)
      sum = (k >= i) ? fma(-lrk, Xc[k], sum) : sum;
    }
    const double lrr = __shfl(Lr[rw], rw, 64);
    Xc[rw] = (rw >= i) ? sum / lrr : 0.0;
  }
#pragma unroll
  for (int k = 0; k < D; ++k) {
    Efac[(size_t)r * D * D + i * D + k] = k <= i ? Lr[k] : 0.0;
    Einv[(size_t)r * D * D + k * D + i] = Xc[k];
  }
  if (!ok) cg_scal[CGS_FAIL] = 1.0;
}
// v[j] = -(sum of the item tiles of block (r, c_0 + j)) (+ B_r on the diagonal block), j < nv, for element e of the block (the
// transposed element of the tiles for c < r: the items hold the upper blocks).  The item ranges of all blocks are fetched first and
// the tiles then walked ROUND BY ROUND - round i adds item i of every block that has one - so that up to ASM_NB loads are in
// flight where a block-by-block walk waited for each block's chain (range, then tiles) in turn: 8 dependent round trips per
// workgroup, which the launch covered with occupancy alone (198 us at 1000 cameras).  Every block's sum in the same order.
template <int D, int ASM_NB>
__device__ __forceinline__ void strip_item_sums(int C, int r, int c_0, int nv, int e, const int* __restrict__ item_ptr,
                                                const double* __restrict__ part, const double* __restrict__ B, double (&v)[ASM_NB]) {
  const int rr = e / D, col = e - rr * D;
  const int eT = col * D + rr;
  int ib[ASM_NB], ie[ASM_NB], mx = 0;
#pragma unroll
  for (int j = 0; j < ASM_NB; ++j) {
    ib[j] = ie[j] = 0;
    if (j < nv) {
      const int c = c_0 + j;
      const int64_t blk = (int64_t)c * C - (int64_t)c * (c - 1) / 2 + (r - c);
      ib[j] = item_ptr[blk]; ie[j] = item_ptr[blk + 1];
    }
  }
#pragma unroll
  for (int j = 0; j < ASM_NB; ++j) { v[j] = 0.0; mx = (ie[j] - ib[j]) > mx ? (ie[j] - ib[j]) : mx; }
  for (int i = 0; i < mx; ++i) {
#pragma unroll
    for (int j = 0; j < ASM_NB; ++j)
      if (ib[j] + i < ie[j]) v[j] += part[(size_t)(ib[j] + i) * (D * D) + ((c_0 + j == r) ? e : eT)];
  }
#pragma unroll
  for (int j = 0; j < ASM_NB; ++j) {
    v[j] = -v[j];
    if (j < nv && c_0 + j == r) v[j] += B[(size_t)r * D * D + e];
  }
}
// <ASM_NB blocks per workgroup, ROUNDS> by camera count: schur_assemble_shape (ba_plan.h)
template <int D, int ASM_NB, bool ROUNDS>
__global__ __launch_bounds__(128) void k_schur_assemble(int C, const int* __restrict__ item_ptr,
                                                        const double* __restrict__ part,
                                                        const double* __restrict__ B, double* __restrict__ S, double* __restrict__ cg_scal,
                                                        const int* __restrict__ cch_ptr, const double* __restrict__ cch_part,
                                                        const double* __restrict__ gc, double* __restrict__ rhs_out,
                                                        double alpha, double* __restrict__ Einv /* null: no factors */, double* __restrict__ Efac) {
  // the right-hand side r_c = g_c - sum over the camera's chunk partials of sum_k G_k e_j (they came out of the
  // diagonal-block items, or of the camera-wise pass): the first workgroup of a block row adds them up, four slots of chunks
  // side by side as k_cam_reduce_final does - that kernel was a launch of its own here (4.8 us plus a boundary)
  if (blockIdx.y == 0 && threadIdx.x < 64) {
    const int cc = blockIdx.x, lane = threadIdx.x, sl = lane >> 4, a = lane & 15;
    double t = 0.0;
    for (int ch = cch_ptr[cc] + sl; ch < cch_ptr[cc + 1]; ch += 4) t += cch_part[(size_t)ch * 16 + a];
    const double t1 = __shfl(t, a + 16, 64), t2 = __shfl(t, a + 32, 64), t3 = __shfl(t, a + 48, 64);
    if (sl == 0 && a < D) rhs_out[cc * D + a] = gc[cc * D + a] - ((t + t1) + (t2 + t3));
  }
  __shared__ double sOut[D][ASM_NB * D + 1];
  const int r = blockIdx.x, c_0 = blockIdx.y * ASM_NB;
  if (c_0 > r) return;                                   // (workgroup-uniform) right of the diagonal
  const int nv = (r - c_0 + 1) < ASM_NB ? (r - c_0 + 1) : ASM_NB;
  const int e = threadIdx.x;
  if (e < D * D) {
    const int rr = e / D, col = e - rr * D;
    if (ROUNDS) {
      double v[ASM_NB];
      strip_item_sums<D, ASM_NB>(C, r, c_0, nv, e, item_ptr, part, B, v);
#pragma unroll
      for (int j = 0; j < ASM_NB; ++j)
        if (j < nv) sOut[rr][j * D + col] = v[j];
    } else {                                             // block by block (few cameras: 22.1 us at 200 against 24.8 round by round)
      const int eT = col * D + rr;
#pragma unroll
      for (int j = 0; j < ASM_NB; ++j)
        if (j < nv) {
          const int c = c_0 + j;
          const int64_t blk = (int64_t)c * C - (int64_t)c * (c - 1) / 2 + (r - c);
          const int src = (c == r) ? e : eT;
          double s = 0.0;
          for (int it = item_ptr[blk]; it < item_ptr[blk + 1]; ++it) s += part[(size_t)it * (D * D) + src];
          double v = -s;
          if (c == r) v += B[(size_t)c * D * D + e];
          sOut[rr][j * D + col] = v;
        }
    }
  }
  __syncthreads();
  // The workgroup that holds the DIAGONAL block (r, r) also factors it for the camera CG: E_r = chol(S_rr + alpha I) and
  // E_r^-1 - what k_diag_einv did as a launch of its own between this kernel and k_scale_system (11 us + a boundary per damped
  // solve, one thread per camera with a 10 x 10 factorisation in 400 registers).  Here: the first D lanes of wave 0
  // (diag_block_factor_lanes).  Unsharded problems only - a rank's S is a partial sum until the exchange (sfm_ba_schur_solve runs
  // k_diag_einv then).
  if (Einv && r < c_0 + ASM_NB && e < D)                  // (c_0 <= r holds here)
    diag_block_factor_lanes<D>(&sOut[0][(r - c_0) * D], ASM_NB * D + 1, alpha, e, r, Einv, Efac, cg_scal);
  const int n = C * D, W = nv * D;
  constexpr int WMAX = ASM_NB * D, NST = (D * WMAX + 127) / 128;
#pragma unroll
  for (int t = 0; t < NST; ++t) {
    const int idx = e + 128 * t;
    const int rr = idx / WMAX, col = idx - rr * WMAX;              // whole rows of the strip
    if (rr < D && col < W) S[(size_t)(r * D + rr) * n + c_0 * D + col] = sOut[rr][col];
  }
}

// ---- The tile-streaming route (n > 2,048, unsharded): S~ = E^-1 (S + alpha I) E^-T straight from the item tiles.
// k_schur_assemble wrote S (400 MB at 1000 cameras) only for k_scale_system_lower to read it back and write S~ (another 400 MB,
// 0.25-0.34 ms per damped solve): with the diagonal blocks' factors known BEFOREHAND (k_schur_diag: one small workgroup per
// camera, the same sums in the same order as k_schur_assemble's, the same factor lanes) the assembling workgroup can scale its
// strip in LDS and write S~ alone.  S itself is then not formed; the few consumers that need it (the factorisation a system falls
// back to, sfm_ba_pack_system) run k_schur_assemble on the same item tiles first (schur_materialise_S).
template <int D>
__global__ __launch_bounds__(128) void k_schur_diag(int C, const int* __restrict__ item_ptr, const double* __restrict__ part,
                                                    const double* __restrict__ B, double alpha, double* __restrict__ Einv,
                                                    double* __restrict__ Efac, double* __restrict__ cg_scal) {
  __shared__ double sBlk[D][D + 1];
  const int r = blockIdx.x, e = threadIdx.x;
  if (e < D * D) {
    const int rr = e / D, col = e - rr * D;
    const int64_t blk = (int64_t)r * C - (int64_t)r * (r - 1) / 2;
    double s = 0.0;
#pragma unroll 4
    for (int it = item_ptr[blk]; it < item_ptr[blk + 1]; ++it) s += part[(size_t)it * (D * D) + e];      // (a diagonal block holds ~20 items at 1000 cameras)
    double v = -s;
    v += B[(size_t)r * D * D + e];
    sBlk[rr][col] = v;
  }
  __syncthreads();
  if (e < D) diag_block_factor_lanes<D>(&sBlk[0][0], D + 1, alpha, e, r, Einv, Efac, cg_scal);
}
// grid and strips as k_schur_assemble.  Writes, of S~: the strip's blocks (r, c), c <= r, as whole rows; the transposes (c, r) of
// the blocks with r - c <= SCALED_BAND (the 128 x 128 diagonal tiles of the tile kernel reach above the diagonal: a tile spans at
// most 128 / D + 2 cameras) - exact transposes, so the diagonal tiles are symmetric to the bit; r~ = E^-1 r (and r itself, which
// the launch-per-iteration routes and the factorisation read).
template <int D, int ASM_NB>
__global__ __launch_bounds__(128) void k_schur_assemble_scaled(int C, const int* __restrict__ item_ptr, const double* __restrict__ part,
                                                               const double* __restrict__ B, double* __restrict__ St,
                                                               const int* __restrict__ cch_ptr, const double* __restrict__ cch_part,
                                                               const double* __restrict__ gc, double* __restrict__ rhs_out,
                                                               double* __restrict__ rhs_t, double alpha, const double* __restrict__ Einv) {
  constexpr int SCALED_BAND = 128 / D + 2;
  if (blockIdx.y == 0 && threadIdx.x < 64) {
    const int cc = blockIdx.x, lane = threadIdx.x, sl = lane >> 4, a = lane & 15;
    double t = 0.0;
    for (int ch = cch_ptr[cc] + sl; ch < cch_ptr[cc + 1]; ch += 4) t += cch_part[(size_t)ch * 16 + a];
    const double t1 = __shfl(t, a + 16, 64), t2 = __shfl(t, a + 32, 64), t3 = __shfl(t, a + 48, 64);
    const double rv = (sl == 0 && a < D) ? gc[cc * D + a] - ((t + t1) + (t2 + t3)) : 0.0;
    double ts = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) ts += Einv[(size_t)cc * D * D + (a < D ? a : 0) * D + k] * __shfl(rv, k, 64);
    if (sl == 0 && a < D) { rhs_out[cc * D + a] = rv; rhs_t[cc * D + a] = ts; }
  }
  __shared__ double sOut[D][ASM_NB * D + 1];
  __shared__ double sE1[D * D], sE2[ASM_NB][D * D];
  const int r = blockIdx.x, c_0 = blockIdx.y * ASM_NB;
  if (c_0 > r) return;                                   // (workgroup-uniform) right of the diagonal
  const int nv = (r - c_0 + 1) < ASM_NB ? (r - c_0 + 1) : ASM_NB;
  const int e = threadIdx.x;
  const int a = e / D, b = e - a * D;
  if (e < D * D) {
    double ev[ASM_NB + 1];
    ev[ASM_NB] = Einv[(size_t)r * D * D + e];
#pragma unroll
    for (int j = 0; j < ASM_NB; ++j) ev[j] = j < nv ? Einv[(size_t)(c_0 + j) * D * D + e] : 0.0;
    double v[ASM_NB];
    strip_item_sums<D, ASM_NB>(C, r, c_0, nv, e, item_ptr, part, B, v);
    sE1[e] = ev[ASM_NB];
#pragma unroll
    for (int j = 0; j < ASM_NB; ++j)
      if (j < nv) { sOut[a][j * D + b] = v[j]; sE2[j][e] = ev[j]; }
  }
  __syncthreads();
  // The two small products per block, T = E_r^-1 X and T E_c^-T, by ROW OWNERS: thread (j, h) forms row h of block j - its row of
  // T stays in registers between the two products (one thread per output passes T through LDS and a barrier: k_scale_system_lower's
  // form).  The terms of every sum in the same order as there.
  // (the diagonal block first: its lower triangle mirrored - only that triangle of S is ever meant - and alpha on its diagonal)
  const bool has_diag = r < c_0 + ASM_NB;                 // (workgroup-uniform)
  const int jd = (r - c_0) * D;
  double dv = 0.0;
  if (has_diag && e < D * D) dv = (b <= a ? sOut[a][jd + b] : sOut[b][jd + a]) + (a == b ? alpha : 0.0);
  __syncthreads();
  if (has_diag && e < D * D) sOut[a][jd + b] = dv;
  __syncthreads();
  // (one row per thread: 300 us per launch at 1000 cameras; two rows per thread - half the LDS reads, twice the chain - 348)
  constexpr int RPT = 1;                                  // rows per thread
  constexpr int RH = D / RPT;
  const int oj = e / RH, oh = e - oj * RH;                // block of the strip, first row
  const bool owner = e < ASM_NB * RH && oj < nv;
  double out[RPT][D];
  if (owner) {
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int ra = oh + q * RH;
      double tr[D];
#pragma unroll
      for (int bb = 0; bb < D; ++bb) tr[bb] = 0.0;
      // tr[bb] = sum_k E1[ra][k] X[k][bb], k ascending in every sum: one row of X per step
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double e1 = sE1[ra * D + k];
#pragma unroll
        for (int bb = 0; bb < D; ++bb) tr[bb] = fma(e1, sOut[k][oj * D + bb], tr[bb]);
        __builtin_amdgcn_sched_barrier(0);                // (left to itself the scheduler hoists all 200 LDS loads: 310 spilled registers)
      }
#pragma unroll
      for (int bb = 0; bb < D; ++bb) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) t = fma(tr[k], sE2[oj][bb * D + k], t);
        out[q][bb] = t;
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  }
  __syncthreads();                                        // every owner has read its block before any of it is overwritten
  if (owner) {
#pragma unroll
    for (int q = 0; q < RPT; ++q)
#pragma unroll
      for (int bb = 0; bb < D; ++bb) sOut[oh + q * RH][oj * D + bb] = out[q][bb];
  }
  __syncthreads();
  const int n = C * D, W = nv * D;
  constexpr int WMAX = ASM_NB * D, NST = (D * WMAX + 127) / 128;
#pragma unroll
  for (int t = 0; t < NST; ++t) {
    const int idx = e + 128 * t;
    const int rr = idx / WMAX, col = idx - rr * WMAX;              // whole rows of the strip
    if (rr < D && col < W) St[(size_t)(r * D + rr) * n + c_0 * D + col] = sOut[rr][col];
  }
  if (e < D * D) {
#pragma unroll
    for (int j = 0; j < ASM_NB; ++j) {
      const int c = c_0 + j;
      if (j < nv && c < r && r - c <= SCALED_BAND)                 // block (c, r) = the transpose: element (a, b) = S~_rc (b, a)
        St[(size_t)(c * D + a) * n + r * D + b] = sOut[b][j * D + a];
    }
  }
}

// out[c][a] = (base ? base[c][a] : 0) - sum_{k in camera c} sum_m G_k[m][a] vec[pt(k)][m]
// Camera lists are cut into chunks of <= 256 observations: one workgroup per chunk.  A G block is fetched as 16-byte pieces,
// one per lane - 16 lanes take one whole block in ONE load instruction (GS = 32: 256 contiguous bytes = two full lines; the
// round-2 form issued three 8-byte loads per lane, 80 bytes apart, for the same block) - so a wavefront covers four
// observations per trip.  Lane l16 of a group holds the elements e = 2 l16, 2 l16 + 1 of the block, i.e. (m, a), (m, a + 1)
// with m = e / D, a = e % D (D is even: a pair never straddles two m), multiplies them with vec[pt][m] and keeps its two
// running sums; at the end the sums of equal a are added over m, the four groups and the four wavefronts in fixed order.
template <int D, typename T, int GS>
__global__ __launch_bounds__(256) void k_cam_reduce_chunks(const int* __restrict__ cch_beg, const int* __restrict__ cch_end,
                                                           const int* __restrict__ cam_obs, const int* __restrict__ cam_pt,
                                                           const T* __restrict__ G, const double* __restrict__ vec,
                                                           double* __restrict__ part) {
  static_assert(D % 2 == 0 && GS % 2 == 0 && GS <= 32, "16-byte pieces of a block: one per lane of a 16-lane group");
  typedef T pair_t __attribute__((ext_vector_type(2)));
  __shared__ double s[4][4][32];                      // [wave][group][element]
  const int ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int grp = lane >> 4, l16 = lane & 15;
  const int e0 = 2 * l16;
  const bool live = e0 < 3 * D;
  const int m = live ? e0 / D : 0;
  double acc0 = 0.0, acc1 = 0.0;
  const int beg = cch_beg[ch], end = cch_end[ch];
  // A trip was a chain of three dependent loads (observation id -> its point -> the point's vector, the G piece beside the point
  // id; now two: the point comes from cam_pt beside the id), and with a run-time trip count each trip waited for the one before: 16 chains one after the other per 256-observation
  // chunk - the launch was as long as that (60 us at 200 cameras for 256 MB).  Four trips' loads are now issued level by level;
  // the products are still added in trip order (the same bits).
  constexpr int UNR = 4;                               // (eight: 53.8 us against 50.4)
  for (int i0 = beg + w * 4 + grp; i0 < end; i0 += 16 * UNR) {
    int k[UNR], pj[UNR];
    pair_t g[UNR];
    double vm[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) { const int i = i0 + 16 * u; k[u] = i < end ? cam_obs[i] : -1; pj[u] = i < end ? cam_pt[i] : 0; }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      g[u] = (k[u] >= 0 && live) ? *(const pair_t*)(G + (size_t)k[u] * GS + e0) : (pair_t){(T)0, (T)0};
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) vm[u] = k[u] >= 0 ? vec[(size_t)pj[u] * 3 + m] : 0.0;
#pragma unroll
    for (int u = 0; u < UNR; ++u)
      if (k[u] >= 0 && live) { acc0 += (double)g[u].x * vm[u]; acc1 += (double)g[u].y * vm[u]; }
  }
  s[w][grp][e0] = acc0; s[w][grp][e0 + 1] = acc1;
  __syncthreads();
  if (tid < 16) {
    double t = 0.0;
    if (tid < D) {
#pragma unroll
      for (int mm = 0; mm < 3; ++mm)
#pragma unroll
        for (int ww = 0; ww < 4; ++ww)
#pragma unroll
          for (int gg = 0; gg < 4; ++gg) t += s[ww][gg][mm * D + tid];
    }
    part[(size_t)ch * 16 + tid] = t;
  }
}
// One wavefront per camera: lane = (slot s = lane >> 4, a = lane & 15); slot s adds the chunks s, s + 4, s + 8, ... in order and
// the four slot sums are combined in fixed order - 5 dependent loads for a camera of 20 chunks where one thread per output
// entry walked all 20 (11 us per call for 2,000 numbers, twice per damped solve).
template <int D>
__global__ __launch_bounds__(256) void k_cam_reduce_final(int C, const int* __restrict__ cch_ptr, const double* __restrict__ part,
                                                          const double* __restrict__ base, double* __restrict__ out,
                                                          const double* __restrict__ sum_part = nullptr, int sum_nblk = 0, int sum_cnt = 0,
                                                          double* __restrict__ sum_dst = nullptr) {
  // (one workgroup more than the cameras need, when asked: the sums of another kernel's per-block partials - k_sum_partials as a
  // launch of its own was 4.6 us plus a kernel boundary in the chain of every damped solve)
  if (sum_part && blockIdx.x == gridDim.x - 1) {
    __shared__ double s_red[4];
    for (int q = 0; q < sum_cnt; ++q) {
      double t = 0.0;
      for (int i = threadIdx.x; i < sum_nblk; i += 256) t += sum_part[(size_t)i * sum_cnt + q];
      const double tt = block_sum256(t, s_red);
      if (threadIdx.x == 0) sum_dst[q] = tt;
    }
    return;
  }
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= C) return;
  const int lane = threadIdx.x & 63, s = lane >> 4, a = lane & 15;
  double t = 0.0;
  for (int ch = cch_ptr[c] + s; ch < cch_ptr[c + 1]; ch += 4) t += part[(size_t)ch * 16 + a];
  const double t1 = __shfl(t, a + 16, 64), t2 = __shfl(t, a + 32, 64), t3 = __shfl(t, a + 48, 64);
  if (s == 0 && a < D) out[c * D + a] = (base ? base[c * D + a] : 0.0) - ((t + t1) + (t2 + t3));
}

// tmp3[k][m] = sum_a G_k[m][a] p_c[cam(k)][a]
// 16 lanes per observation, each with one 16-byte piece of the block (see k_cam_reduce_chunks): the whole block in one
// coalesced load, p_c[cam] as 16-byte pieces too; the D / 2 products of equal m are summed through LDS in fixed order.
constexpr int GTP_OBS = 64;                           // observations per workgroup of k_obs_Gtp (four trips of 16)
template <int D, typename T, int GS>
__global__ __launch_bounds__(256) void k_obs_Gtp(int64_t N, const int* __restrict__ cam_idx,
                                                 const T* __restrict__ G,
                                                 const double* __restrict__ pc, double* __restrict__ tmp3) {
  static_assert(D % 2 == 0 && GS % 2 == 0 && GS <= 32, "16-byte pieces of a block: one per lane of a 16-lane group");
  typedef T pair_t __attribute__((ext_vector_type(2)));
  __shared__ double s[GTP_OBS][17];                   // [observation of the workgroup][lane of its group]
  const int tid = threadIdx.x, slot = tid >> 4, l16 = tid & 15;
  const int64_t k0 = (int64_t)blockIdx.x * GTP_OBS;
  const int e0 = 2 * l16;
  const int a = e0 % D;
  const bool live = e0 < 3 * D;
  pair_t g[GTP_OBS / 16];
  int cam[GTP_OBS / 16];
#pragma unroll
  for (int it = 0; it < GTP_OBS / 16; ++it) {           // every load of the workgroup in flight before the first use
    const int64_t k = k0 + it * 16 + slot;
    const bool ok = live && k < N;
    g[it] = ok ? *(const pair_t*)(G + (size_t)k * GS + e0) : (pair_t)(T)0;
    cam[it] = ok ? cam_idx[k] : 0;
  }
#pragma unroll
  for (int it = 0; it < GTP_OBS / 16; ++it) {
    const double2 p = *(const double2*)(pc + (size_t)cam[it] * D + a);
    s[it * 16 + slot][l16] = (double)g[it].x * p.x + (double)g[it].y * p.y;
  }
  __syncthreads();
  if (tid < 3 * GTP_OBS) {                            // GTP_OBS x 3 values, one contiguous run
    const int sl = tid / 3, mm = tid - 3 * sl;
    const int64_t kk = k0 + sl;
    if (kk < N) {
      double u = 0.0;
#pragma unroll
      for (int j = 0; j < D / 2; ++j) u += s[sl][mm * (D / 2) + j];
      tmp3[kk * 3 + mm] = u;
    }
  }
}

// p_pj = -M^T (e_j + sum_track tmp3),  v_j = M p_pj ; block partials of ||p_p||^2 and ||v||^2.
__global__ __launch_bounds__(256) void k_backsub(int P, const int* __restrict__ pt_ptr,
                                                 const double* __restrict__ tmp3,
                                                 const double* __restrict__ Linv,
                                                 const double* __restrict__ e, double* __restrict__ pp,
                                                 double* __restrict__ v, double* __restrict__ part) {
  __shared__ double s_red[4];
  const int j = blockIdx.x * 256 + threadIdx.x;
  double p2 = 0.0, v2 = 0.0;
  if (j < P) {
    double u0 = e[(size_t)j * 3], u1 = e[(size_t)j * 3 + 1], u2 = e[(size_t)j * 3 + 2];
    // (a track's ~10 rows: with a run-time trip count every row waited for the one before; five in flight, added in order)
#pragma unroll 5
    for (int k = pt_ptr[j]; k < pt_ptr[j + 1]; ++k) {
      u0 += tmp3[(size_t)k * 3]; u1 += tmp3[(size_t)k * 3 + 1]; u2 += tmp3[(size_t)k * 3 + 2];
    }
    const double* M = Linv + (size_t)j * 6;
    const double q0 = -(M[0] * u0 + M[1] * u1 + M[3] * u2);
    const double q1 = -(M[2] * u1 + M[4] * u2);
    const double q2 = -(M[5] * u2);
    pp[(size_t)j * 3] = q0; pp[(size_t)j * 3 + 1] = q1; pp[(size_t)j * 3 + 2] = q2;
    const double w0 = M[0] * q0, w1 = M[1] * q0 + M[2] * q1, w2 = M[3] * q0 + M[4] * q1 + M[5] * q2;
    v[(size_t)j * 3] = w0; v[(size_t)j * 3 + 1] = w1; v[(size_t)j * 3 + 2] = w2;
    p2 = q0 * q0 + q1 * q1 + q2 * q2;
    v2 = w0 * w0 + w1 * w1 + w2 * w2;
  }
  double a = block_sum256(p2, s_red);
  double b = block_sum256(v2, s_red);
  if (threadIdx.x == 0) { part[blockIdx.x * 2] = a; part[blockIdx.x * 2 + 1] = b; }
}

// ------------------------------------------------------------------------------------ small vector helpers
__global__ void k_copy_neg(const double* __restrict__ src, double* __restrict__ dst, int n, double sgn) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = sgn * src[i];
}
__global__ void k_add_vec(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = a[i] + b[i];
}
// dst[0..cnt) = fixed-order sums of `cnt` interleaved partial columns (stride = cnt).
__global__ __launch_bounds__(256) void k_sum_partials(const double* __restrict__ part, int nblk, int cnt,
                                                      double* __restrict__ dst) {
  __shared__ double s_red[4];
  for (int q = 0; q < cnt; ++q) {
    double t = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) t += part[(size_t)i * cnt + q];
    double tt = block_sum256(t, s_red);
    if (threadIdx.x == 0) dst[q] = tt;
  }
}
__global__ __launch_bounds__(1024) void k_dot(int n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out) {
  __shared__ double s_red[17];
  double t = 0.0;
  for (int i = threadIdx.x; i < n; i += 1024) t += a[i] * b[i];
  t = block_sum1024(t, s_red);
  if (threadIdx.x == 0) *out = t;
}
// (the launches the other units make of these: ba_stages.h)
void ba_copy_neg(sfm_ctx* h, const double* src, double* dst, int n, double sgn) { hipLaunchKernelGGL(k_copy_neg, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, src, dst, n, sgn); }
void ba_add_vec(sfm_ctx* h, const double* a, const double* b, double* dst, int n) { hipLaunchKernelGGL(k_add_vec, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, a, b, dst, n); }
void ba_dot(sfm_ctx* h, int n, const double* a, const double* b, double* out) { hipLaunchKernelGGL(k_dot, dim3(1), dim3(1024), 0, h->stream, n, a, b, out); }
void ba_sum_partials(sfm_ctx* h, const double* part, int nblk, int cnt, double* dst) { hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, h->stream, part, nblk, cnt, dst); }

// ------------------------------------------------------------------------------------ host stages
int check_problem(sfm_ctx* h, sfm_ba_problem p, Lay* L) {
  if (!h) return SFM_ERR_ARG;
  if (!p) return sfm_fail(h, SFM_ERR_ARG, "sfm_ba", "null problem");
  if (!p->workspace) return sfm_fail(h, SFM_ERR_WORKSPACE, "sfm_ba", "no workspace bound (sfm_ba_bind_workspace)");
  *L = p->L;
  return SFM_OK;
}

extern "C" int sfm_ba_set_sharded(sfm_handle h, sfm_ba_problem p, int sharded) {
  if (!h) return SFM_ERR_ARG;
  if (!p) return sfm_fail(h, SFM_ERR_ARG, "sfm_ba_set_sharded", "null problem");
  p->sharded = sharded ? 1 : 0;
  return SFM_OK;
}

// the launches of the Schur stage that other units make too (what they enqueue: ba_stages.h)
void launch_build_G(sfm_ctx* h, sfm_ba_problem p, const Lay& L, double alpha, double* cg_scal) {
  double* ws = (double*)p->workspace; const int64_t N = p->n_obs, P = p->n_pts;
  DISPATCH_DT(p->cam_dim, p->precision,
    hipLaunchKernelGGL((k_build_G<DD, TT, double, GG>), dim3(cdiv(N, 256) + cdiv(P, 256)), dim3(256), 0, h->stream, N, p->pt_idx, WST(L, recA),
                       WST(L, recB), WS(L, Linv), WS(L, G), WS(L, e), WS(L, eobs), WS(L, Cp), WS(L, gp), alpha, (int)P, (unsigned)cdiv(N, 256),
                       cg_scal));
}
void launch_obs_Gtp(sfm_ctx* h, sfm_ba_problem p, const Lay& L, const double* vc) {
  double* ws = (double*)p->workspace; const int64_t N = p->n_obs;
  DISPATCH_D(p->cam_dim, hipLaunchKernelGGL((k_obs_Gtp<DD, double, GG>), dim3(cdiv(N, GTP_OBS)), dim3(256), 0, h->stream, N, p->cam_idx, WS(L, G), vc, WS(L, tmp3)));
}
void launch_backsub_points(sfm_ctx* h, sfm_ba_problem p, const Lay& L) {
  double* ws = (double*)p->workspace;
  hipLaunchKernelGGL(k_backsub, dim3((unsigned)L.nblk_pt), dim3(256), 0, h->stream, p->n_pts, p->pt_ptr, WS(L, tmp3),
                     WS(L, Linv), WS(L, e), WS(L, pp), WS(L, v), WS(L, part_pt));
}
void launch_cam_reduce_chunks(sfm_ctx* h, sfm_ba_problem p, const Lay& L, const double* vec) {
  double* ws = (double*)p->workspace;
  if (p->n_cchunks > 0)
    DISPATCH_D(p->cam_dim, hipLaunchKernelGGL((k_cam_reduce_chunks<DD, double, GG>), dim3((unsigned)p->n_cchunks), dim3(256), 0, h->stream, p->cch_beg,
                                              p->cch_end, p->cam_obs, p->cam_pt, WS(L, G), vec, WS(L, cch_part)));
}
void launch_cam_reduce_final(sfm_ctx* h, sfm_ba_problem p, const Lay& L, const double* base, double* out, bool point_sums) {
  double* ws = (double*)p->workspace; const int C = p->n_cams, s = point_sums ? 1 : 0;
  // (+ 1 workgroup: the two sums over the point pass's per-block partials, sum ||p_p||^2 and sum ||v||^2; else the kernel's defaults)
  DISPATCH_D(p->cam_dim, hipLaunchKernelGGL(k_cam_reduce_final<DD>, dim3(cdiv(C, 4) + s), dim3(256), 0, h->stream, C, p->cch_ptr, WS(L, cch_part),
                                            base, out, s ? WS(L, part_pt) : (const double*)nullptr, s ? (int)L.nblk_pt : 0, s ? 2 : 0,
                                            s ? WS(L, red_q) + C * p->cam_dim : (double*)nullptr));
}

// S (red_S) and its right-hand side from the item tiles; einv_out / m_out: the diagonal blocks' factors of S + alpha I for the
// camera CG as well (null: not wanted)
static void launch_schur_assemble(sfm_ctx* h, sfm_ba_problem p, const Lay& L, double alpha, double* einv_out, double* m_out) {
  double* ws = (double*)p->workspace;
  const int C = p->n_cams, D = p->cam_dim, n = C * D;
  const AsmShape shape = schur_assemble_shape(C);
#define ASM_LAUNCH(NB, ROUNDS)                                                                                                  \
  hipLaunchKernelGGL((k_schur_assemble<DD, NB, ROUNDS>), dim3(C, cdiv(C, NB)), dim3(128), 0, h->stream, C, p->item_ptr,          \
                     WS(L, sch_part), WS(L, B), WS(L, red_S), WS(L, cg_scal), p->cch_ptr, WS(L, cch_part), WS(L, gc),             \
                     WS(L, red_S) + (size_t)n * n, alpha, einv_out, m_out)
  DISPATCH_D(D, {
    if (shape.rounds) ASM_LAUNCH(8, true);
    else if (shape.nb == 8) ASM_LAUNCH(8, false);
    else ASM_LAUNCH(2, false);
  });
#undef ASM_LAUNCH
}
// the scaled system S~ (lower triangle) and r~ instead, behind the diagonal blocks' factors (k_schur_diag)
static void launch_schur_assemble_scaled(sfm_ctx* h, sfm_ba_problem p, const Lay& L, double alpha, double* St) {
  double* ws = (double*)p->workspace;
  const int C = p->n_cams, D = p->cam_dim, n = C * D;
#define ASM_LAUNCH(NB)                                                                                                          \
  hipLaunchKernelGGL((k_schur_assemble_scaled<DD, NB>), dim3(C, cdiv(C, NB)), dim3(128), 0, h->stream, C, p->item_ptr,           \
                     WS(L, sch_part), WS(L, B), St, p->cch_ptr, WS(L, cch_part), WS(L, gc), WS(L, red_S) + (size_t)n * n,         \
                     WS(L, cg_r), alpha, WS(L, cg_Minv))
  DISPATCH_D(D, {
    hipLaunchKernelGGL(k_schur_diag<DD>, dim3(C), dim3(128), 0, h->stream, C, p->item_ptr, WS(L, sch_part), WS(L, B), alpha,
                       WS(L, cg_Minv), WS(L, cg_M), WS(L, cg_scal));
    if (schur_assemble_scaled_nb(C) == 4) ASM_LAUNCH(4);
    else ASM_LAUNCH(2);
  });
#undef ASM_LAUNCH
}

extern "C" int sfm_ba_schur_build(sfm_handle h, sfm_ba_problem p, double alpha) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  if (!(alpha > 0.0)) return sfm_fail(h, SFM_ERR_ARG, "sfm_ba_schur_build", "alpha must be > 0");
  double* ws = (double*)p->workspace;
  const int C = p->n_cams, D = p->cam_dim, n = C * D;
  const BaSwitches sw = ba_switches_from_env();
  const CamPlan plan = cam_plan(n, p->camera_solver, h->cgs_persist_off != 0, sw);
  sfm_prof_begin(h, SFM_PROF_BUILD_G);
  launch_build_G(h, p, L, alpha, WS(L, cg_scal));
  sfm_prof_end(h, SFM_PROF_BUILD_G);
  sfm_prof_begin(h, SFM_PROF_SCHUR);
  DISPATCH_DT(D, p->precision, {
    if (p->n_items > 0) { // 8 groups x ceil(largest group / 4) workgroups
      sfm_prof_begin(h, SFM_PROF_SCHUR_ITEMS);
      hipLaunchKernelGGL((k_schur_items<DD, double, GG>), dim3(8 * cdiv(p->xcd_max_items, SFM_SCHUR_WG_WAVES)),
                         dim3(64 * SFM_SCHUR_WG_WAVES), 0, h->stream,
                         p->xcd_ptr, p->xcd_items, p->it_first, p->it_stride, p->it_cnt, p->pair_k, p->pair_k2, WS(L, G), WS(L, sch_part),
                         p->cam_idx, p->item_ptr, p->cch_ptr, C, WS(L, eobs), WS(L, cch_part), p->has_dup ? 0 : 1);
      sfm_prof_end(h, SFM_PROF_SCHUR_ITEMS);
    }
  });
  if (p->has_dup) launch_cam_reduce_chunks(h, p, L, WS(L, e));      // the chunk partials of sum_k G_k e_j by the camera-wise pass over G
  // what the solve of this system will consume decides what is left for it: S (with the diagonal blocks' factors), or S~ alone
  // (S is then formed on demand only: schur_materialise_S)
  const BuildFusion fuse = build_fusion(plan, p->sharded != 0, p->camera_solver, n, sw);
  p->st_alpha = -1.0;
  p->s_valid = fuse.scale ? 0 : 1;
  if (fuse.scale) {
    DenseWs dw; dense_ws_carve(WS(L, dense), n, &dw);
    launch_schur_assemble_scaled(h, p, L, alpha, dw.Lm);
    p->st_alpha = alpha;
  } else
    launch_schur_assemble(h, p, L, alpha, fuse.einv ? WS(L, cg_Minv) : (double*)nullptr, WS(L, cg_M));
  p->cg_scal_clean = 1;
  p->einv_alpha = fuse.einv ? alpha : -1.0;
  sfm_prof_end(h, SFM_PROF_SCHUR);
  SFM_LAUNCH_CHECK(h, "sfm_ba_schur_build");
  return SFM_OK;
}

// S (red_S) from the item tiles of the last sfm_ba_schur_build, for the consumers that need the unscaled system after a build
// that formed S~ only: the factorisation (a system the CG is not given, or did not finish) and sfm_ba_pack_system.
int schur_materialise_S(sfm_ctx* h, sfm_ba_problem p, const Lay& L) {
  if (p->s_valid) return SFM_OK;
  launch_schur_assemble(h, p, L, 0.0, nullptr, nullptr);
  p->s_valid = 1;
  SFM_LAUNCH_CHECK(h, "schur_materialise_S");
  return SFM_OK;
}

// rows 0..n of [S | r] ([n+1][n]): row r keeps its first min(r + 1, n) entries, packed back to back
__global__ __launch_bounds__(256) void k_pack_lower(const double* __restrict__ S, int n, double* __restrict__ Sp, int unpack_dir) {
  const int r = blockIdx.x;
  const int len = r < n ? r + 1 : n;
  const size_t off = (size_t)r * (r + 1) / 2;
  double* full = const_cast<double*>(S) + (size_t)r * n;
  for (int c = threadIdx.x; c < len; c += 256) {
    if (unpack_dir) full[c] = Sp[off + c];
    else Sp[off + c] = full[c];
  }
}

static int pack_S(sfm_handle h, sfm_ba_problem p, int unpack_dir, const char* what) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  double* ws = (double*)p->workspace;
  const int n = p->n_cams * p->cam_dim;
  DenseWs dw; dense_ws_carve(WS(L, dense), n, &dw);
  if ((rc = schur_materialise_S(h, p, L))) return rc;
  p->st_alpha = -1.0;                                  // the packed copy goes where S~ would be
  hipLaunchKernelGGL(k_pack_lower, dim3(n + 1), dim3(256), 0, h->stream, WS(L, red_S), n, dw.Lm, unpack_dir);
  SFM_LAUNCH_CHECK(h, what);
  return SFM_OK;
}
extern "C" int sfm_ba_pack_system(sfm_handle h, sfm_ba_problem p) { return pack_S(h, p, 0, "sfm_ba_pack_system"); }
extern "C" int sfm_ba_unpack_system(sfm_handle h, sfm_ba_problem p) { return pack_S(h, p, 1, "sfm_ba_unpack_system"); }

// point back-substitution for the p_c in the workspace, and (want_q) the pieces of rhs2 = p_c - W C_a^-1 p_p
void launch_backsub(sfm_ctx* h, sfm_ba_problem p, const Lay& L, int want_q) {
  double* ws = (double*)p->workspace;
  sfm_prof_begin(h, SFM_PROF_BACKSUB);
  launch_obs_Gtp(h, p, L, WS(L, pc));
  launch_backsub_points(h, p, L);
  if (want_q) launch_cam_reduce_chunks(h, p, L, WS(L, v));
  if (want_q) launch_cam_reduce_final(h, p, L, nullptr, WS(L, red_q), true);
  else ba_sum_partials(h, WS(L, part_pt), (int)L.nblk_pt, 2, WS(L, red_q) + p->n_cams * p->cam_dim);
  sfm_prof_end(h, SFM_PROF_BACKSUB);
}

// The host's wait for a ticket in pinned memory (sfm_ba_read_scalars, cgs_solve_big).  Every few thousand spins the stream is asked as
// well: a drained stream ends the wait whatever was published (a path that publishes nothing, or a failure the caller's synchronisation reports)
bool ba_wait_for_word(sfm_ctx* h, const volatile double* word, double want) {
  constexpr unsigned SPIN_QUERY = 4096;
  bool seen = false;
  for (unsigned spins = 1; ; ++spins) {
    if (*word == want) { seen = true; break; }
    if ((spins % SPIN_QUERY) == 0 && hipStreamQuery(h->stream) != hipErrorNotReady) break;
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return seen;
}

extern "C" int sfm_ba_read_scalars(sfm_handle h, sfm_ba_problem p, double* out_host) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  // every kernel that writes one of the scalars writes it into the problem's pinned host mirror too (p->host_sc; the 128-byte
  // device-to-host copy was a blit kernel of its own in front of every wait), and the finishing kernel of a stage publishes its
  // ticket behind them: the host spins on the ticket word (ba_wait_for_word) and sees the scalars ~1 us after the kernel's last store,
  // where a stream synchronisation returns only after the kernel has been retired and its completion signal processed.
  // SFM_POLL_SCALARS=0: wait for the stream.
  static const bool poll_on = !(getenv("SFM_POLL_SCALARS") && getenv("SFM_POLL_SCALARS")[0] == '0');
  const bool seen = poll_on && p->look_pending && ba_wait_for_word(h, p->host_sc + SFM_HSC_SEQ, p->look_seq);
  p->look_pending = 0;
  if (!seen) SFM_HIP(h, hipStreamSynchronize(h->stream));
  if (p->cg2_pending && (rc = cgs_second_system_verdict(h, p, L))) return rc;
  memcpy(out_host, p->host_sc, SFM_SC_COUNT * sizeof(double));
  return SFM_OK;
}
