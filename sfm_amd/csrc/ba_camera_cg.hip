// Bundle adjustment, the camera system once it is formed: block-Jacobi-scaled CG in three forms (launch per iteration, persistent,
// tile-streaming), the factorisation fallback, and the host stages sfm_ba_schur_solve / sfm_ba_finish_solve.  (Data layout: ba.hip.)
#include "ba_internal.h"
#include "ba_device.h"
#include <atomic>
#include <chrono>

// ------------------------------------------------------------------------------------ CG on the explicit reduced system
// Once S has been formed (and, multi-rank, all-reduced) the replicated camera solve is a latency chain in the dense
// Cholesky (n / 64 dependent steps, 0.9 ms at n = 2000) - but with its own d x d diagonal blocks as preconditioner
// S needs only ~25 conjugate-gradient iterations to a relative residual of 1e-13, each ONE launch that streams S once
// from L2.  The system is scaled symmetrically with the Cholesky factors E_c of its diagonal blocks,
// S~ = E^-1 (S + alpha I) E^-T (unit diagonal blocks), so that plain CG on S~ IS block-Jacobi PCG on S and the
// recurrences need no preconditioner application.  k_cgs_iter: every workgroup first repeats the vector
// recurrences of the previous iteration from r, p and the full S~ p (3 n doubles from L2, fixed-order block sums:
// all workgroups obtain bit-identical scalars and vectors, so no grid-wide reduction or second launch is needed),
// keeps the new direction in LDS and multiplies its own rows of S~ with it.  r, p, S~ p are double-buffered
// (workgroup 0 publishes iteration k's vectors while others may still read iteration k-1's).  Rows are dealt to
// workgroups so that one XCD owns a contiguous eighth of S~ (4 MB at n = 2000: stays in its L2 across iterations).
// The host reads ||r||^2 every few launches.  If CG has not converged after CGS_MAX_ITER iterations, or meets a
// direction of non-positive curvature, the caller falls back to the Cholesky route: S itself is left untouched.
// (CGS_MAX_N, CGS_MAX_ITER and the budget of the tile-streaming route: ba_plan.h)
// ||r|| <= CGS_RTOL ||r_0|| on the scaled system.  SFM_CGS_RTOL overrides it - a DIAGNOSTIC knob (tools/exp_cg_fixed_cost.py
// sets 1.0: zero iterations, what remains is the fixed cost of a system), never set by the product
static double cgs_rtol() { static const double v = getenv("SFM_CGS_RTOL") ? atof(getenv("SFM_CGS_RTOL")) : 1e-13; return v; }
#define CGS_RTOL cgs_rtol()

// E_c = chol(S_cc + alpha I); Einv[c] = E_c^-1 (lower, zeros above).  One thread per camera.
template <int D>
__global__ __launch_bounds__(64) void k_diag_einv(int C, const double* __restrict__ S, int n, double alpha, double* __restrict__ Einv,
                            double* __restrict__ Efac /* E_c itself (lower) */, double* __restrict__ scal) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double L[D][D], X[D][D];
  const double* blk = S + (size_t)c * D * n + c * D;
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) L[i][j] = (j <= i) ? blk[(size_t)i * n + j] + (i == j ? alpha : 0.0) : 0.0;
  const bool bad = !small_chol_inverse<D>(L, X);
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      Einv[(size_t)c * D * D + i * D + j] = X[i][j];
      Efac[(size_t)c * D * D + i * D + j] = j <= i ? L[i][j] : 0.0;
    }
  if (bad) scal[CGS_FAIL] = 1.0;
}
// St[c][c2] = Einv_c (S[c][c2] + alpha [c == c2]) Einv_c2^T.  One workgroup (128 threads, thread e < D*D owns element e of a
// block) per block row c and SCALE_NB consecutive columns c2; only the blocks c2 >= c are computed, each is written twice
// (St is symmetric: the block and its transpose).  All blocks of a workgroup move through each stage together: three
// barriers per workgroup, not per block.  (One workgroup per block pair, 40,000 at 200 cameras: 22 us, dispatch-bound.)
// (blocks per workgroup, us per launch at 200 cameras: 16: 29.9, 8: 21.8, 4: 18.4, 2: 18.0)
constexpr int SCALE_NB = 4;
template <int D>
__global__ __launch_bounds__(128) void k_scale_system(int n, int C, const double* __restrict__ S, double alpha,
                                                      const double* __restrict__ Einv, double* __restrict__ St,
                                                      const double* __restrict__ rhs, double* __restrict__ rhs_t) {
  __shared__ double sB[SCALE_NB][D * D], sT[SCALE_NB][D * D], sE2[SCALE_NB][D * D], sE1[D * D];
  const int c = blockIdx.x, e = threadIdx.x;
  const int a = e / D, b = e - a * D;
  const int c2_0 = blockIdx.y * SCALE_NB;
  // rhs~_c = E_c^-1 rhs_c for the CG that follows (the first workgroup of the block row does it, once for everybody: the
  // persistent kernel used to form all of rhs~ in every one of its workgroups)
  if (rhs_t && blockIdx.y == 0 && e < D) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) t += Einv[(size_t)c * D * D + e * D + k] * rhs[c * D + k];     // E^-1 lower: stored zeros above
    rhs_t[c * D + e] = t;
  }
  if (c2_0 + SCALE_NB <= c) return;                      // (workgroup-uniform) nothing at or right of the diagonal here
  const int nb = (C - c2_0) < SCALE_NB ? (C - c2_0) : SCALE_NB;
  if (e < D * D) {
    sE1[e] = Einv[(size_t)c * D * D + e];
#pragma unroll
    for (int j = 0; j < SCALE_NB; ++j)
      if (j < nb && c2_0 + j >= c) {
        // block (c, c2 >= c) of S from its LOWER triangle - the part the multi-rank exchange carries (sfm_ba_pack_system):
        // S[c][c2][a][b] = S[c2 D + b][c D + a]
        const int c2 = c2_0 + j, row = c * D + a, col = c2 * D + b;
        sB[j][e] = (col <= row ? S[(size_t)row * n + col] : S[(size_t)col * n + row]) + ((c == c2 && a == b) ? alpha : 0.0);
        sE2[j][e] = Einv[(size_t)c2 * D * D + e];
      }
  }
  __syncthreads();
  if (e < D * D) {
#pragma unroll
    for (int j = 0; j < SCALE_NB; ++j)
      if (j < nb && c2_0 + j >= c) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) t += sE1[a * D + k] * sB[j][k * D + b];    // Einv_c is lower: entries k > a are stored zeros
        sT[j][e] = t;
      }
  }
  __syncthreads();
  if (e < D * D) {
#pragma unroll
    for (int j = 0; j < SCALE_NB; ++j)
      if (j < nb && c2_0 + j >= c) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) t += sT[j][a * D + k] * sE2[j][b * D + k];
        const int c2 = c2_0 + j;
        St[(size_t)(c * D + a) * n + c2 * D + b] = t;
        if (c2 != c) St[(size_t)(c2 * D + b) * n + c * D + a] = t;
      }
  }
}
// The same for the tile-streaming CG (n > 2,048), which reads the 128 x 128 tiles (I, J <= I) of St only - the lower triangle
// plus, inside the diagonal tiles, the entries above the diagonal: blocks (c, c2) with c2 <= c and the band c < c2 <= c + BAND
// (a 128-wide tile spans at most 128 / D + 2 cameras).  Every block is read from the lower triangle of S and written ONCE, in
// its own rows (80-byte row segments): half the bytes of k_scale_system and none of its column-strided mirror writes
// (0.53 -> 0.35 ms at 1000 cameras).  A form that moves whole 640-byte rows of the strip through LDS (every workgroup computing all
// its blocks, the transposes bit-identical) was built and measured SLOWER: 35 against 21 us at 200 cameras, +0.1 ms at 1000 - the
// kernel is bound by the latency of its few dependent stages per workgroup, not by the width of its accesses.
template <int D>
__global__ __launch_bounds__(128) void k_scale_system_lower(int n, int C, const double* __restrict__ S, double alpha,
                                                            const double* __restrict__ Einv, double* __restrict__ St,
                                                            const double* __restrict__ rhs, double* __restrict__ rhs_t) {
  constexpr int BAND = 128 / D + 2;
  __shared__ double sB[SCALE_NB][D * D], sT[SCALE_NB][D * D], sE2[SCALE_NB][D * D], sE1[D * D];
  // descending strips and rows: what k_schur_assemble wrote last is read first - still in the memory-side cache at 1000 cameras
  const int c = (int)(gridDim.x - 1u - blockIdx.x), e = threadIdx.x;
  const int a = e / D, b = e - a * D;
  const int by = (int)(gridDim.y - 1u - blockIdx.y);
  const int c2_0 = by * SCALE_NB;
  if (rhs_t && by == 0 && e < D) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) t += Einv[(size_t)c * D * D + e * D + k] * rhs[c * D + k];
    rhs_t[c * D + e] = t;
  }
  if (c2_0 > c + BAND) return;                           // (workgroup-uniform) nothing left of the band's end here
  const int last = (c + BAND) < (C - 1) ? (c + BAND) : (C - 1);
  if (e < D * D) {
    sE1[e] = Einv[(size_t)c * D * D + e];
#pragma unroll
    for (int j = 0; j < SCALE_NB; ++j)
      if (c2_0 + j <= last) {
        const int c2 = c2_0 + j, row = c * D + a, col = c2 * D + b;
        sB[j][e] = (col <= row ? S[(size_t)row * n + col] : S[(size_t)col * n + row]) + ((c == c2 && a == b) ? alpha : 0.0);
        sE2[j][e] = Einv[(size_t)c2 * D * D + e];
      }
  }
  __syncthreads();
  if (e < D * D) {
#pragma unroll
    for (int j = 0; j < SCALE_NB; ++j)
      if (c2_0 + j <= last) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) t += sE1[a * D + k] * sB[j][k * D + b];
        sT[j][e] = t;
      }
  }
  __syncthreads();
  if (e < D * D) {
#pragma unroll
    for (int j = 0; j < SCALE_NB; ++j)
      if (c2_0 + j <= last) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) t += sT[j][a * D + k] * sE2[j][b * D + k];
        St[(size_t)(c * D + a) * n + (c2_0 + j) * D + b] = t;
      }
  }
}
// out_c = Einv_c v_c (transpose 0) or Einv_c^T v_c (transpose 1), optionally negated
template <int D>
__global__ void k_block_mv(int C, const double* __restrict__ Einv, const double* __restrict__ v, double* __restrict__ out,
                           int transpose, double sgn, const double* __restrict__ v2 = nullptr /* added to v when given */) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C * D) return;
  const int c = i / D, a = i - c * D;
  const double* E = Einv + (size_t)c * D * D;
  double t = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) t += (transpose ? E[k * D + a] : E[a * D + k]) * (v[c * D + k] + (v2 ? v2[c * D + k] : 0.0));
  out[i] = sgn * t;
}
// state 0 of the recurrence: x = 0, r = p = rhs; rr0
__global__ __launch_bounds__(256) void k_cgs_init(int n, const double* __restrict__ rhs, double* __restrict__ x,
                                                  double* __restrict__ r0, double* __restrict__ p0, double* __restrict__ scal) {
  __shared__ double s_red[4];
  double rr = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) { const double v = rhs[i]; x[i] = 0.0; r0[i] = v; p0[i] = v; rr += v * v; }
  rr = block_sum256(rr, s_red);
  if (threadIdx.x == 0) {
    scal[CGS_RR0] = rr; scal[CGS_RR] = rr; scal[CGS_ITER] = 0.0; scal[CGS_DONE] = 0.0;
    scal[CGS_RR_SLOT] = rr; scal[CGS_RR_SLOT + 1] = rr;
  }
}
// One CG iteration on S~ per launch.  it == 0: only the product S~ p_0.  vec: [2 states][r | p | Ap], n doubles each.
// NC = ceil(n / 512) column chunks per thread, ROWS rows of S~ per workgroup.  The workgroup's slice of S~ does not
// depend on the recurrences, so it is fetched into registers FIRST (ROWS x NC 16-byte loads per thread in flight)
// and the vector recurrences run in the shadow of that latency; measured 12.8 -> ... us per launch.
template <int NC, int ROWS>
__global__ __launch_bounds__(256) void k_cgs_iter(int n, int it, double rtol2, const double* __restrict__ St,
                                                  double* __restrict__ vec, double* __restrict__ x, double* __restrict__ scal) {
  __shared__ double s_p[NC * 512];
  __shared__ double s_red[4];
  __shared__ double s_row[ROWS][4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // rows of this workgroup: XCD x = blockIdx % 8 owns rows [x * per_xcd, (x + 1) * per_xcd)
  const int per_xcd = (int)(gridDim.x / 8) * ROWS;
  const int row0 = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3) * ROWS;
  double2 sv[ROWS][NC];
#pragma unroll
  for (int q = 0; q < ROWS; ++q)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int row = row0 + q, jc = 2 * tid + 512 * c;            // n is even: jc < n implies jc + 1 < n
      sv[q][c] = (row < n && jc < n) ? *(const double2*)(St + (size_t)row * n + jc) : make_double2(0.0, 0.0);
    }
  const size_t sz = (size_t)3 * n;
  const double* in = vec + (size_t)((it + 1) & 1) * sz;        // state written by launch it - 1 (it == 0: state 0 below)
  double* out = vec + (size_t)(it & 1) * sz;
  if (it == 0) {
    in = vec;                                                  // k_cgs_init left r_0 = p_0 in state 0
    for (int i = tid; i < NC * 512; i += 256) s_p[i] = i < n ? in[n + i] : 0.0;
  } else {
    const double *r = in, *pv = in + n, *Ap = in + 2 * n;
    constexpr int PER = 2 * NC;
    double rv[PER], pvv[PER], av[PER];
    double pAp = 0.0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int i = tid + 256 * q;
      rv[q] = i < n ? r[i] : 0.0; pvv[q] = i < n ? pv[i] : 0.0; av[q] = i < n ? Ap[i] : 0.0;
      pAp += pvv[q] * av[q];
    }
    pAp = block_sum256(pAp, s_red);
    // ||r||^2 as workgroup 0 of the previous launch left it.  It writes the new value to the OTHER slot: workgroups of
    // this launch that run later must still find the old one
    const double rr_old = scal[CGS_RR_SLOT + ((it + 1) & 1)], rr0 = scal[CGS_RR0];
    const bool done = rr_old <= rtol2 * rr0;
    const bool broken = !done && !(pAp > 0.0);                 // non-positive curvature (or NaN): S~ is not positive definite
    if (done || broken) {
      // carry the state forward unchanged so that later launches of this batch see it again (and stop again)
      if (blockIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < PER; ++q) { const int i = tid + 256 * q; if (i < n) { out[i] = rv[q]; out[n + i] = pvv[q]; out[2 * n + i] = av[q]; } }
        if (tid == 0) { scal[CGS_RR_SLOT + (it & 1)] = rr_old; scal[CGS_DONE] = 1.0; if (broken) scal[CGS_FAIL] = 2.0; }
      }
      return;
    }
    const double a = rr_old / pAp;
    double rr_new = 0.0;
#pragma unroll
    for (int q = 0; q < PER; ++q) { rv[q] -= a * av[q]; rr_new += rv[q] * rv[q]; }
    rr_new = block_sum256(rr_new, s_red);
    const double beta = rr_new / rr_old;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int i = tid + 256 * q;
      const double pn = rv[q] + beta * pvv[q];
      s_p[i] = i < n ? pn : 0.0;
      if (i < n && blockIdx.x == 0) { x[i] += a * pvv[q]; out[i] = rv[q]; out[n + i] = pn; }
    }
    if (blockIdx.x == 0 && tid == 0) { scal[CGS_RR_SLOT + (it & 1)] = rr_new; scal[CGS_RR] = rr_new; scal[CGS_ITER] = (double)it; }
  }
  __syncthreads();
  double acc[ROWS];
#pragma unroll
  for (int q = 0; q < ROWS; ++q) acc[q] = 0.0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const double p0 = s_p[2 * tid + 512 * c], p1 = s_p[2 * tid + 512 * c + 1];
#pragma unroll
    for (int q = 0; q < ROWS; ++q) acc[q] += sv[q][c].x * p0 + sv[q][c].y * p1;
  }
#pragma unroll
  for (int q = 0; q < ROWS; ++q) {
    const double t = wave_sum(acc[q]);
    if (lane == 0) s_row[q][w] = t;
  }
  __syncthreads();
  if (tid < ROWS && row0 + tid < n) out[2 * n + row0 + tid] = (s_row[tid][0] + s_row[tid][1]) + (s_row[tid][2] + s_row[tid][3]);
}

// ------------------------------------------------------------------------------------ persistent form of the same CG
// ONE launch per system instead of one per iteration (k_cgs_iter above: ~7 us per iteration, of which the kernel boundary
// and the re-read of S~ from L2 are most).  Workgroup b owns the PR_ROWS rows [8 b, 8 b + 8) of S~ and holds them IN
// REGISTERS for the whole solve (thread t: the columns 2t + 512 c, c < NC -> 8 x NC x 2 doubles = 128 VGPRs at n = 2048:
// the kernel runs one wave per SIMD), together with its columns of x, r, p.  Per iteration a workgroup multiplies its rows
// with p (64 FMAs per thread, wave sums, four partials through LDS: fixed order), PUBLISHES its 8 entries of S~ p and
// GATHERS all n of them: the all-gather is the only exchange between workgroups.  It uses self-validating 8-byte granules
// (cdna_hip_programming.md, Guideline 16, form R2: {tag, 32-bit half of the double} written by ONE relaxed agent-scope
// atomic store = global_store_dwordx2 sc1, polled with relaxed agent-scope atomic loads = sc1: no flag, no fence; a double
// is two granules).  tag = salt (a per-launch counter: no hipGraph replay here) * 256 + iteration + 1, two slots by
// iteration parity: a workgroup can be at most one iteration ahead of the slowest (its product of iteration i + 1 needs
// every entry of iteration i), so when it overwrites slot i & 1 with iteration i + 2 everybody has read iteration i.
// The vector recurrences and the two dot products are then computed REDUNDANTLY by every workgroup from identical data in
// identical order (block sums), so all take the same branch at the same iteration and no second exchange is needed.
// Placement-independent: nothing assumes a dispatch order or a workgroup -> XCD map; every spin is bounded, a workgroup that
// gives up posts the launch's salt in the abort word, which the others poll beside their granules, and the host then takes
// the per-launch kernel (and stops using this one for the handle: a grid that is not co-resident - CUs taken by another
// process - would pay the timeout on every solve otherwise).
// Diagnostic build only (-DSFM_CGS_STAMPS=1, tools/exp_cgs_phases.sh): per-iteration phase stamps of workgroup 0 / thread 0 of
// k_cgs_persist on the 100 MHz constant clock.  The shipped library executes no stamp.
#ifndef SFM_CGS_STAMPS
#define SFM_CGS_STAMPS 0
#endif
#if SFM_CGS_STAMPS
constexpr int CGS_STAMP_SLOTS = 1 << 16;
__device__ unsigned long long g_cgs_stamps[CGS_STAMP_SLOTS];
__device__ unsigned int g_cgs_stamp_pos;
extern "C" int sfm_debug_cgs_stamps(unsigned long long* dst, int n_words, unsigned int* n_used) {
  if (hipMemcpyFromSymbol(n_used, HIP_SYMBOL(g_cgs_stamp_pos), 4, 0, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_cgs_stamps), (size_t)n_words * 8, 0, hipMemcpyDeviceToHost);
}
// record (tag, time): tag 0 = launch start, 1 = rows in registers, 2 = product + wave sums done (publish), 3 = gather complete,
// 4 = recurrences done (end of iteration), 5 = epilogue done
#define CGS_STAMP(tag) do { if (stamp_on) { const unsigned q_ = atomicAdd(&g_cgs_stamp_pos, 2u); \
    if (q_ + 1 < CGS_STAMP_SLOTS) { g_cgs_stamps[q_] = (tag); g_cgs_stamps[q_ + 1] = __builtin_amdgcn_s_memrealtime(); } } } while (0)
#else
#define CGS_STAMP(tag) do {} while (0)
#endif
constexpr int PR_ROWS = 8;
constexpr unsigned PR_SPIN_LIMIT = 1u << 17;      // passes over a thread's granules (~1 us each) before giving up
typedef unsigned long long pr_u64;
#define PR_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// What used to be separate 4-us launches around a system, folded into the persistent kernel (all optional):
struct PrFuse {
  const double* Einv;      // non-null: the right-hand side arrives UNSCALED and rhs~ = E^-1 (rhs + rhs_b) is formed in the prologue
  const double* rhs_b;     //   second summand (system of the q term: p_c + W C_a^-1 p_p pieces), may be null
  double* pc_out;          // non-null (step system): p_c = -E^-T x~ is written here by workgroup 0 on convergence
  const double* fin_pc;    // non-null (q system): the scalars of the damped solve are finished here on convergence
  const double* fin_redq;  //   [n + 2]: ... | sum ||p_p||^2 | sum ||v||^2
  double* fin_sc;          //   SFM_SC_PNORM2, SFM_SC_PQ, SFM_SC_CHOL_FAIL
  double* fin_hsc;         //   the same three in the problem's pinned host mirror of the scalars (sfm_ba_read_scalars)
  int rhs_scaled;          // 1: `rhs` is rhs~ already (k_scale_system / k_block_mv formed it; Einv then only serves the epilogue).  Forming
                           //    it in the prologue - every workgroup all n entries, ~200 eight-byte loads per thread - took 17-19 us per
                           //    launch by in-kernel stamps, more than seven iterations
  double fin_seq;          // (q system) the ticket sfm_ba_read_scalars waits for - published whatever the verdict: the host then looks at it
};

template <int NC, int D>
__global__ __launch_bounds__(256, 1) void k_cgs_persist(int n, double rtol2, int max_iter, unsigned salt,
                                                        const double* __restrict__ St, const double* __restrict__ rhs,
                                                        double* __restrict__ x_out, pr_u64* mail /* [2][n][2] granules */,
                                                        pr_u64* abort_w, double* __restrict__ scal, PrFuse f, int sabotage,
                                                        double* __restrict__ host_status /* pinned host memory, device-mapped: 8 words */) {
  __shared__ double s_part[PR_ROWS][4];
  __shared__ double s_red[4];
  __shared__ int s_ok[4];
  __shared__ double s_x[PR_MAX_N];                  // workgroup 0, epilogue: x~ for the block-wise back-transformation
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int blk = (int)blockIdx.x;
  // test hook (SFM_CGS_SABOTAGE=1): workgroup 1 never publishes, as if it had not become resident - the others must run into
  // their spin bound, post the abort word and leave; the host then takes the launch-per-iteration route
  if (sabotage > 0 && blk == 1) return;
  const int row0 = blk * PR_ROWS;
#if SFM_CGS_STAMPS
  const bool stamp_on = blk == 0 && tid == 0;
#endif
  CGS_STAMP(0);
  // this thread's slice of the workgroup's rows: registers for the whole solve
  double2 sv[PR_ROWS][NC];
#pragma unroll
  for (int q = 0; q < PR_ROWS; ++q)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int row = row0 + q, col = 2 * tid + 512 * c;            // n is even: col < n implies col + 1 < n
      sv[q][c] = (row < n && col < n) ? *(const double2*)(St + (size_t)row * n + col) : make_double2(0.0, 0.0);
    }
  double xv[2 * NC], rv[2 * NC], pv[2 * NC], bv[2 * NC];     // bv: the right-hand side itself (the q system's r~ . x~)
#if SFM_CGS_STAMPS
  { double keep_ = 0.0;
#pragma unroll
    for (int q = 0; q < PR_ROWS; ++q) keep_ += sv[q][0].x;
    asm volatile("" :: "v"(keep_)); }      // (the stamp below must not be scheduled ahead of the row loads)
#endif
  CGS_STAMP(1);
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int col = 2 * tid + 512 * c;
    const bool in = col < n;
    if (f.Einv && !f.rhs_scaled) {
      // rhs~_i = sum_k E^-1[cam][a][k] (rhs + rhs_b)[cam D + k]   (E^-1 lower triangular: the stored zeros above cost nothing here)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        double t = 0.0;
        if (in) {
          const int i = col + u, cam = i / D, a = i - cam * D;
          const double* e = f.Einv + (size_t)cam * D * D + a * D;
          const double* r = rhs + cam * D;
#pragma unroll
          for (int k = 0; k < D; ++k) t += e[k] * (r[k] + (f.rhs_b ? f.rhs_b[cam * D + k] : 0.0));
        }
        rv[2 * c + u] = t;
      }
    } else {
      rv[2 * c] = in ? rhs[col] : 0.0; rv[2 * c + 1] = in ? rhs[col + 1] : 0.0;
    }
    bv[2 * c] = rv[2 * c]; bv[2 * c + 1] = rv[2 * c + 1];
    xv[2 * c] = 0.0; xv[2 * c + 1] = 0.0;
  }
  double rr0;
  {
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < 2 * NC; ++i) t += rv[i] * rv[i];
    rr0 = block_sum256_fast(t, s_red);                 // ||rhs||^2 (every thread gets it): the tolerance is relative to the right-hand side
  }

  // one round: y = S~ v for this workgroup's rows, published and gathered; returns false when the launch is abandoned
  double yv[2 * NC];
  // (dot: v . y over the whole vector, in every thread - its four wave parts travel through LDS together with the waves'
  // verdicts on the gather, one barrier pair for both; meaningless when the round is abandoned)
  auto exchange = [&](const double (&v)[2 * NC], int round, double& dot) -> bool {
    double acc[PR_ROWS];
#pragma unroll
    for (int q = 0; q < PR_ROWS; ++q) {
      double t = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) t += sv[q][c].x * v[2 * c] + sv[q][c].y * v[2 * c + 1];
      acc[q] = t;
    }
    // the eight row sums over the wave by ONE halving exchange (lane_rows8_sum: 10 additions and 22 cross-lane moves) instead of
    // eight full wave sums (48 and 96): in-kernel stamps put "product + wave sums" at 1.8 us of a 5.1-us iteration at n = 2,000
    // (one wave per SIMD: every dependent step of the reduction is exposed)
    {
      const double t = lane_rows8_sum(acc, lane);
      if ((lane & 7) == 0) s_part[((lane >> 5) << 2) | (((lane >> 4) & 1) << 1) | ((lane >> 3) & 1)][w] = t;
    }
    __syncthreads();
    CGS_STAMP(2);
    const unsigned tag = salt * 256u + (unsigned)round + 1u;
    pr_u64* slot = mail + (size_t)(round & 1) * 2 * n;
    if (tid < PR_ROWS && row0 + tid < n) {
      const double y = (s_part[tid][0] + s_part[tid][1]) + (s_part[tid][2] + s_part[tid][3]);
      const pr_u64 bits = (pr_u64)__double_as_longlong(y);
      // the two granules of the entry in ONE 16-byte device-scope store (the workgroup's eight entries = one whole 128-byte line
      // from one instruction); each 8-byte half carries its own tag, so the store need not be atomic as a whole
      typedef unsigned pr_st4 __attribute__((ext_vector_type(4)));
      const pr_st4 pk = {(unsigned)(bits & 0xFFFFFFFFull), tag, (unsigned)(bits >> 32), tag};
      asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(slot + 2 * (size_t)(row0 + tid)), "v"(pk) : "memory");
    }
    // gather this thread's columns: 4 granules per chunk (two doubles), re-read until every tag matches
    // ... but not at once: nothing can have arrived before the slowest workgroup's store has crossed the fabric, and a pass that
    // comes too early is not free - 250 workgroups x 32 KB of L1-bypassing loads compete with the very stores they wait for,
    // and the lines they pull are invalidated again a moment later.  In-kernel stamps (tools/exp_cgs_phases.sh, n = 2,000):
    // publish -> gather complete 2.83 us polling at once, 1.78 with s_sleep 8 (x 64 clocks) in front, 1.56-1.59 with 24, 1.91
    // with 40, 2.57 with 64; n = 500 (63 workgroups, one chunk per thread): 0.98 at once, 1.08 with 8, 1.31 with 24.
    constexpr int FIRST_SLEEP = NC == 1 ? 0 : 6 * NC - 4;          // 8 / 14 / 20 for two / three / four chunks per thread
    if (FIRST_SLEEP > 0) __builtin_amdgcn_s_sleep(FIRST_SLEEP);
    bool ok = false;
    for (unsigned spins = 0; spins < PR_SPIN_LIMIT; ++spins) {
      pr_u64 g[4 * NC];
      // a thread's four granules of a chunk (two doubles) are 32 contiguous, 32-byte aligned bytes: TWO 16-byte device-scope loads
      // instead of four 8-byte ones (8-byte accesses run at 0.54-0.70 of the 16-byte rate, MI355X_MICROARCH.md).  Every 8-byte
      // half carries its own tag, so a 16-byte load that saw its two halves at different times is still read correctly.  The
      // compiler does not see these loads: the wait below is theirs.
      typedef unsigned pr_u32x4 __attribute__((ext_vector_type(4)));
      pr_u32x4 q[2 * NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = 2 * tid + 512 * c;
        const pr_u64* gp = slot + 2 * (size_t)(col < n ? col : 0);
        asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(q[2 * c]) : "v"(gp) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off offset:16 sc1" : "=v"(q[2 * c + 1]) : "v"(gp) : "memory");
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
      for (int c = 0; c < 2 * NC; ++c) {
        // (the wait must sit between the loads and the first use of ANY of their registers: tie them to it)
        asm volatile("" : "+v"(q[c]));
        g[2 * c] = (pr_u64)q[c].x | ((pr_u64)q[c].y << 32);
        g[2 * c + 1] = (pr_u64)q[c].z | ((pr_u64)q[c].w << 32);
      }
      bool all = true;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const bool in = 2 * tid + 512 * c < n;
#pragma unroll
        for (int i = 0; i < 4; ++i) all &= !in || (unsigned)(g[4 * c + i] >> 32) == tag;
        yv[2 * c] = in ? __longlong_as_double((long long)((g[4 * c] & 0xFFFFFFFFull) | (g[4 * c + 1] << 32))) : 0.0;
        yv[2 * c + 1] = in ? __longlong_as_double((long long)((g[4 * c + 2] & 0xFFFFFFFFull) | (g[4 * c + 3] << 32))) : 0.0;
      }
      if (__all(all)) { ok = true; break; }
      if ((spins & 31u) == 31u && __hip_atomic_load(abort_w, PR_RLX_AGENT) == (pr_u64)salt) break;     // somebody gave up
      __builtin_amdgcn_s_sleep(2);                    // (polling without the sleep measured the same: 135.1 / 100.1 us per system)
    }
    CGS_STAMP(3);
    double td = 0.0;
#pragma unroll
    for (int i = 0; i < 2 * NC; ++i) td += v[i] * yv[i];
    td = wave_sum_all(td);
    // (s_red / s_ok were last READ before the barrier above - the one behind the s_part writes - so they can be written here
    // without another one in front; their next writer, the block sum of r . r, starts with a barrier of its own)
    if (lane == 0) { s_red[w] = td; s_ok[w] = ok ? 1 : 0; }
    __syncthreads();
    const bool all_ok = (s_ok[0] & s_ok[1] & s_ok[2] & s_ok[3]) != 0;
    dot = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    if (!all_ok && tid == 0) __hip_atomic_store(abort_w, (pr_u64)salt, PR_RLX_AGENT);
    return all_ok;
  };
  // done: 1 = the recurrence ended (converged, or broken: fail 2), 0 = out of iterations, -1 = the launch was abandoned.
  // CGS_FAIL may already hold k_diag_einv's 1 (a diagonal block is not positive definite): it is only ever raised here.
  auto finish = [&](double rr, int it, double done, double fail) {
    if (blk != 0) return;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int col = 2 * tid + 512 * c;
      if (col < n) { x_out[col] = xv[2 * c]; x_out[col + 1] = xv[2 * c + 1]; }
    }
    if (tid == 0) {
      scal[CGS_RR0] = rr0; scal[CGS_RR] = rr; scal[CGS_ITER] = (double)it; scal[CGS_DONE] = done;
      const double fail_now = scal[CGS_FAIL] != 0.0 ? scal[CGS_FAIL] : fail;
      if (fail != 0.0 && scal[CGS_FAIL] == 0.0) scal[CGS_FAIL] = fail;
      // the host's copy of the verdict, written straight into its pinned page (visible when the launch has ended: an event
      // behind the launch is all the host waits for) - a separate 64-byte device-to-host copy is a blit kernel of its own, ~4 us
      // plus two kernel boundaries between this system and the back-substitution that waits behind it
      host_status[CGS_RR0] = rr0; host_status[CGS_RR] = rr; host_status[CGS_ITER] = (double)it;
      host_status[CGS_FAIL] = fail_now; host_status[CGS_DONE] = done;
    }
    const bool converged = done == 1.0 && fail == 0.0 && rr <= rtol2 * rr0;
    if (!converged && f.fin_sc && tid == 0) publish_ticket(f.fin_hsc, f.fin_seq);      // (no scalars: the verdict is what the host finds)
    if (!converged || !(f.pc_out || f.fin_sc)) return;          // (workgroup-uniform)
    if (f.pc_out) {
      // p_c = -E^-T x~: entry (cam, a) needs the whole x~ block of its camera -> through LDS
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = 2 * tid + 512 * c;
        if (col < n) { s_x[col] = xv[2 * c]; s_x[col + 1] = xv[2 * c + 1]; }
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = 2 * tid + 512 * c;
        if (col < n) {
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int i = col + u, cam = i / D, a = i - cam * D;
            const double* e = f.Einv + (size_t)cam * D * D;
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) t += e[k * D + a] * s_x[cam * D + k];
            f.pc_out[i] = -t;
          }
        }
      }
    }
    if (f.fin_sc) {
      // the scalars of the damped solve (k_finish_solve_pcg): p^T (H + alpha I)^-1 p = rhs2~ . x~2 + sum ||v||^2
      double t = 0.0, t2 = 0.0;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int col = 2 * tid + 512 * c;
        if (col < n) {
          t += bv[2 * c] * xv[2 * c] + bv[2 * c + 1] * xv[2 * c + 1];
          const double p0 = f.fin_pc[col], p1 = f.fin_pc[col + 1];
          t2 += p0 * p0 + p1 * p1;
        }
      }
      const double dot = block_sum256_fast(t, s_red);
      const double pc2 = block_sum256_fast(t2, s_red);
      if (tid == 0) {
        const double pn2 = pc2 + f.fin_redq[n], pq = dot + f.fin_redq[n + 1];
        f.fin_sc[SFM_SC_PNORM2] = f.fin_hsc[SFM_SC_PNORM2] = pn2; f.fin_sc[SFM_SC_PQ] = f.fin_hsc[SFM_SC_PQ] = pq;
        double fl = scal[CGS_FAIL] != 0.0 ? 1.0 : 0.0;
        if (fl == 0.0 && !(isfinite(pn2) && isfinite(pq))) fl = 3.0;
        f.fin_sc[SFM_SC_CHOL_FAIL] = f.fin_hsc[SFM_SC_CHOL_FAIL] = fl;
        publish_ticket(f.fin_hsc, f.fin_seq);
      }
    }
  };

  int round = 0;
  double rr = rr0;                                  // x = 0: r = p = rhs
#pragma unroll
  for (int i = 0; i < 2 * NC; ++i) pv[i] = rv[i];
  if (!(rr0 > 0.0)) {                               // zero right-hand side: x = 0; NaN / Inf in it: not a system CG can solve (fail 2 ->
    if (rr0 == 0.0) finish(0.0, 0, 1.0, 0.0);       // the caller's factorisation route reports the non-finite step)
    else finish(rr0, 0, 1.0, 2.0);
    return;
  }
  int it = 0;
  for (; it < max_iter; ++it) {
    if (rr <= rtol2 * rr0) { finish(rr, it, 1.0, 0.0); return; }
    double pAp;
    if (!exchange(pv, round++, pAp)) { finish(rr, it, -1.0, 0.0); return; }
    if (!(pAp > 0.0)) { finish(rr, it, 1.0, 2.0); return; }       // non-positive curvature (or NaN): S~ is not positive definite
    const double a = rr / pAp;
    double t2 = 0.0;
#pragma unroll
    for (int i = 0; i < 2 * NC; ++i) { xv[i] += a * pv[i]; rv[i] -= a * yv[i]; t2 += rv[i] * rv[i]; }
    const double rr_new = block_sum256_fast(t2, s_red);
    const double beta = rr_new / rr;
#pragma unroll
    for (int i = 0; i < 2 * NC; ++i) pv[i] = rv[i] + beta * pv[i];
    rr = rr_new;
    CGS_STAMP(4);
  }
  finish(rr, it, rr <= rtol2 * rr0 ? 1.0 : 0.0, 0.0);
}

// One persistent launch for a system (k_cgs_persist), in two halves so that the host never idles the GPU on its status:
// cgs_persist_launch enqueues the kernel and the copy of its 8 status words into pinned memory (slot pin: SFM_PIN_CG1 /
// the problem's own slot for the second system) (which systems take it: cam_plan);
// cgs_persist_status interprets the copy once the caller knows it has arrived (an event behind it, or a later stream
// synchronisation).  *ran = 0: the launch was abandoned - the caller takes the launch-per-iteration route (cgs_solve) with its
// separate pre / post kernels; *status = 0: converged (and whatever `fuse` asked for has been done by workgroup 0).
// The salt of a launch's granule tags comes from ONE process-wide counter (24 bits, never 0 = what cleared memory reads as),
// started from the clock: a handle that is destroyed and created again, or two handles sharing a workspace over time, can never
// replay a salt whose granules still sit in a mailbox (a per-handle counter restarting at 1 could: the reader would then take
// stale entries for fresh ones - silently).  sfm_ba_bind_workspace clears the mailbox of a caller-owned workspace besides.
static unsigned cgs_next_salt() {
  static std::atomic<unsigned> seq{(unsigned)(std::chrono::steady_clock::now().time_since_epoch().count() >> 10)};
  unsigned s;
  do { s = (seq.fetch_add(1u, std::memory_order_relaxed) + 1u) & 0xFFFFFFu; } while (s == 0u);
  return s;
}
struct PrLaunch {      // everything a (re)launch of one system needs
  int n, D; const double* St; const double* rhs; double* x_t; double* mail; double* scal; double rtol; PrFuse fuse;
  double* pin;         // pinned host words the kernel writes its verdict to
};
static int cgs_persist_launch(sfm_ctx* h, const PrLaunch& a) {
  const int n = a.n, D = a.D;
  const unsigned grid = (unsigned)cdiv(n, PR_ROWS);
  const int nc = (int)cdiv(n, 512);
  pr_u64* abort_w = (pr_u64*)(a.scal + 12);
  const unsigned salt = cgs_next_salt();
  const double rtol2 = a.rtol * a.rtol;
  const int sabotage = (getenv("SFM_CGS_SABOTAGE") && getenv("SFM_CGS_SABOTAGE")[0] == '1' && grid > 1) ? 1 : 0;
  a.pin[CGS_DONE] = -1.0;                          // what a launch that never wrote its verdict reads as: abandoned
#define PR_LAUNCH(NC, DD_) hipLaunchKernelGGL((k_cgs_persist<NC, DD_>), dim3(grid), dim3(256), 0, h->stream, n, rtol2, CGS_MAX_ITER, salt, a.St, a.rhs, a.x_t, (pr_u64*)a.mail, abort_w, a.scal, a.fuse, sabotage, a.pin)
  if (D == 10) { if (nc <= 1) PR_LAUNCH(1, 10); else if (nc == 2) PR_LAUNCH(2, 10); else if (nc == 3) PR_LAUNCH(3, 10); else PR_LAUNCH(4, 10); }
  else { if (nc <= 1) PR_LAUNCH(1, 6); else if (nc == 2) PR_LAUNCH(2, 6); else if (nc == 3) PR_LAUNCH(3, 6); else PR_LAUNCH(4, 6); }
#undef PR_LAUNCH
  SFM_LAUNCH_CHECK(h, "cgs_persist_launch");
  return SFM_OK;
}
static void cgs_persist_read(const double* st, int* iters_out, int* status, int* ran) {
  *ran = 0; *status = 1;
  if (st[CGS_DONE] == -1.0) return;                 // the launch was abandoned (a spin ran out)
  *ran = 1;
  *iters_out += (int)st[CGS_ITER];
  if (st[CGS_FAIL] == 0.0 && st[CGS_DONE] != 0.0) *status = 0;
}
// The verdict of a launch has arrived (an event or a stream synchronisation behind it).  An abandoned launch is dealt with here:
//   * `sharded` (the problem is one rank's shard): every rank must take the SAME route through the camera solve - the
//     launch-per-iteration kernel sums in another order, and a rank that switched on its own would hold a replicated camera step
//     that differs from its peers' in the last bits and, sooner or later, a different trial history and a different sequence of
//     collectives.  So: the same kernel again, up to CGS_SHARDED_RETRIES times, then the solve fails loudly;
//   * otherwise: *ran = 0, the handle stops using the persistent kernel and the caller takes the launch-per-iteration route.
// *relaunched tells the caller that work enqueued behind the first launch on the assumption that it converged must be redone.
constexpr int CGS_SHARDED_RETRIES = 3;
static int cgs_persist_verdict(sfm_ctx* h, const PrLaunch& a, int sharded, int* iters_out, int* status, int* ran, int* relaunched) {
  *relaunched = 0;
  cgs_persist_read(a.pin, iters_out, status, ran);
  if (*ran) return SFM_OK;
  auto again = [&]() -> int {
    *relaunched = 1;
    SFM_HIP(h, hipMemsetAsync(a.scal, 0, CG_SCAL_WORDS * sizeof(double), h->stream));
    int rc = cgs_persist_launch(h, a); if (rc) return rc;
    SFM_HIP(h, hipStreamSynchronize(h->stream));
    cgs_persist_read(a.pin, iters_out, status, ran);
    return SFM_OK;
  };
  if (sharded) {
    for (int attempt = 1; attempt <= CGS_SHARDED_RETRIES && !*ran; ++attempt) {
      fprintf(stderr, "sfm_amd: the persistent CG launch of a sharded solve was abandoned; launching it again (%d of %d)\n", attempt, CGS_SHARDED_RETRIES);
      int rc = again(); if (rc) return rc;
    }
    if (!*ran)
      return sfm_fail(h, SFM_ERR_HIP, "camera CG",
                      "the persistent kernel could not run on this rank (its grid was not co-resident) and a sharded solve must take the "
                      "same route on every rank: set SFM_CGS_PERSIST=0 on ALL ranks");
    return SFM_OK;
  }
  h->cgs_persist_off = 1;
  fprintf(stderr, "sfm_amd: the persistent CG launch was abandoned (grid not co-resident?); using one launch per iteration from now on\n");
  return SFM_OK;
}

// Launches until the host's next look at the residual: where it should be small enough by the average rate so far (CG converges close to
// linearly here) - a look costs a wait on the stream, a launch past convergence 3-4 us.  pad: launches beyond the iterations, cap: largest batch
static int cgs_next_batch(double rr, double rr0, double its, double rtol2, int pad, int cap) {
  const double rate = rr0 > 0.0 ? std::log(rr / rr0) / (its > 1.0 ? its : 1.0) : 0.0;      // < 0 when converging
  if (!(rate < -1e-3 && rr > 0.0)) return 8;
  const double need = std::log(rtol2 * rr0 / rr) / rate;
  return need < 2.0 ? pad : (need > cap ? cap : (int)need + pad);
}
// x~ = S~^-1 rhs~ by CG, one launch per iteration (k_cgs_iter); returns 0 converged / 1 not converged or broken (caller falls
// back to the factorisation)
static int cgs_solve(sfm_ctx* h, int n, const double* St, const double* rhs_t, double* x_t, double* vec, double* scal,
                     double rtol, int* iters_out, int* status) {
  const double rtol2 = rtol * rtol;
  *status = 1;
  // (column chunks per thread, rows per workgroup): 128 registers of prefetched matrix per thread in the two larger shapes
  // four rows per workgroup: at n = 2000 that is 512 workgroups (two per CU) - 8 rows / 256 workgroups measured 6 % slower per
  // iteration, 2 rows / 1,024 workgroups 9 % slower (twice the redundant vector work).
  constexpr int ROWS = 4;
  const unsigned grid = 8u * (unsigned)cdiv(cdiv(n, 8), ROWS);
  hipLaunchKernelGGL(k_cgs_init, dim3(1), dim3(256), 0, h->stream, n, rhs_t, x_t, vec, vec + n, scal);
  int it = 0;
  int batch = 13;                                                  // launch 0 only multiplies: first look after 12 iterations
  while (it <= CGS_MAX_ITER) {
    for (int b = 0; b < batch; ++b, ++it)
      if (n <= 1024) hipLaunchKernelGGL((k_cgs_iter<2, ROWS>), dim3(grid), dim3(256), 0, h->stream, n, it, rtol2, St, vec, x_t, scal);
      else if (n <= 2048) hipLaunchKernelGGL((k_cgs_iter<4, ROWS>), dim3(grid), dim3(256), 0, h->stream, n, it, rtol2, St, vec, x_t, scal);
      else hipLaunchKernelGGL((k_cgs_iter<8, ROWS>), dim3(grid), dim3(256), 0, h->stream, n, it, rtol2, St, vec, x_t, scal);
    SFM_HIP(h, hipMemcpyAsync(h->pinned, scal, 8 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    SFM_HIP(h, hipStreamSynchronize(h->stream));
    if (h->pinned[CGS_FAIL] != 0.0) break;
    const double rr = h->pinned[CGS_RR], rr0 = h->pinned[CGS_RR0];
    if (h->pinned[CGS_DONE] != 0.0 || rr <= rtol2 * rr0) { *status = 0; break; }
    batch = cgs_next_batch(rr, rr0, h->pinned[CGS_ITER], rtol2, 2, 32);
  }
  *iters_out += (int)h->pinned[CGS_ITER];
  SFM_LAUNCH_CHECK(h, "cgs_solve");
  return SFM_OK;
}

// ------------------------------------------------------------------------------------ the same CG for large systems
// n > 2,048 (1000 cameras: n = 10,000, S~ = 800 MB).  Little of S~ stays in a cache between iterations, so an iteration is
// a stream over the matrix and what counts is how many bytes of it are read: S~ is symmetric, and a 128 x 128 tile (I, J),
// J < I, of its lower triangle serves BOTH products it takes part in - rows I of S~ p get A_IJ p_J, rows J get A_IJ^T p_I -
// so an iteration reads n^2 / 2 entries (414 MB at n = 10,000 against 800 MB; the factorisation it replaces: 14 ms per damped
// solve, ~50 iterations of this per system).  One workgroup per tile (3,160 at n = 10,000); wave w owns 32 of its rows, a lane
// two of its columns (one 16-byte load per row and lane: a row of the tile is one contiguous KiB).  The column sums stay in
// the lane (two accumulators over the wave's rows, the four waves added in fixed order through LDS); the row sums of 16 rows
// at a time are reduced over the 64 lanes by a halving exchange (lane_rows16_sum: 15 + 2 shuffles instead of 16 x 6).  Every
// tile writes its partial sums to a slot of its own, P[k][i] with k = J for the row sums of (I, J) and k = I for its column
// sums - each (k, i) is written exactly once per iteration - and k_cgs_big_reduce adds the nb = ceil(n / 128) slots of an
// entry in fixed order: no atomics, bitwise reproducible.  The recurrences run in ONE workgroup (k_cgs_big_update: 5 vectors
// of n doubles, ~6 us); three launches per iteration, ~15 us of them around the ~75 us stream.  State in the factor's
// transposed-copy buffer (free on this route): r | p | S~p | dots[nb] | P[nb][n].
constexpr int SY_T = 128;

// v[q] = this lane's part of the sum of row q; returns (in every lane) the sum over the 64 lanes of row (lane >> 2)
__device__ __forceinline__ double lane_rows16_sum(double (&v)[16], int lane) {
  // halving exchanges without LDS round trips (the ds_bpermute form of this function, 17 dependent shuffles per call, was
  // ~0.8 us at the end of every 16-row batch of a tile): across the half-waves and across neighbouring rows by
  // v_permlane32_swap / v_permlane16_swap, inside a row of 16 lanes by row / half-row mirrors (DPP)
  double u[8], x[4];
#pragma unroll
  for (int k = 0; k < 8; ++k) u[k] = swap32_add(v[k], v[k + 8]);        // upper half keeps rows + 8
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = swap16_add(u[k], u[k + 4]);        // odd rows of 16 lanes keep rows + 4
  double y[2];
  {
    const bool hi = (lane & 8) != 0;                                    // lanes 8..15 of a row keep rows + 2
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double send = hi ? x[k] : x[k + 2], keep = hi ? x[k + 2] : x[k];
      y[k] = keep + dpp_f64<0x140>(send);                               // row_mirror: lane i <-> lane 15 - i
    }
  }
  double t;
  {
    const bool hi = (lane & 4) != 0;                                    // bit 2 keeps rows + 1
    const double send = hi ? y[0] : y[1], keep = hi ? y[1] : y[0];
    t = keep + dpp_f64<0x141>(send);                                    // row_half_mirror: lane i <-> lane 7 - i of its eight
  }
  t += dpp_f64<0xB1>(t);                                                // the four lanes of a quad
  t += dpp_f64<0x4E>(t);
  return t;
}

// The recurrences in the Chronopoulos - Gear arrangement, which needs ONE global reduction point per iteration (gamma = r.r and
// delta = (S~ r).r, both from the product that has just been formed) where the textbook form has two (p.S~p, then r'.r'):
//     beta = gamma / gamma_prev;  alpha = gamma / (delta - beta gamma / alpha_prev)
//     p = r + beta p;  s = w + beta s  (= S~ p);  x += alpha p;  r -= alpha s;  w = S~ r
// So an iteration is TWO launches: the tile kernel - whose prologue sums the per-block dot products of the previous launch (every
// tile the same 2 nb numbers in the same order: identical scalars everywhere, no broadcast), forms the new r on its own two
// 128-entry ranges in LDS and multiplies - and the slot reduction, which also leaves the two dot products per block.  The third
// launch of the first form (a single workgroup running the vector updates over all n entries: 13 us of a ~100-us iteration at
// n = 10,000, plus its boundary) is gone: the DIAGONAL tile of a range writes that range's r, p, s, x, into the other of two
// buffer sets (the off-diagonal tiles of the same launch still read the old ones).  Convergence is seen one launch late - the
// launch whose prologue finds gamma <= rtol^2 gamma_0 copies x out and multiplies nothing.
// State in the factor's transposed-copy buffer (free on this route): [2][r | p | s | x] | w | dots[2][nbp] | P[nb][n].
__global__ __launch_bounds__(256) void k_cgb_init(int n, int nbp, const double* __restrict__ rhs, double* __restrict__ vec,
                                                  double* __restrict__ dots, double* __restrict__ scal) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    vec[i] = rhs[i];                                                                  // r_0 (set 0)
    vec[(size_t)1 * n + i] = 0.0; vec[(size_t)2 * n + i] = 0.0; vec[(size_t)3 * n + i] = 0.0;     // p, s (times beta = 0 in launch 1), x_0
  }
  if (i < 2 * nbp) dots[i] = 0.0;
  if (i == 0) { scal[CGS_RR0] = 0.0; scal[CGS_RR] = 0.0; scal[CGS_ITER] = 0.0; scal[CGS_DONE] = 0.0; scal[5] = scal[6] = scal[7] = scal[8] = 0.0; }
}
__global__ __launch_bounds__(256) void k_cgb_symv(int n, int nb, int nbp, int it, double rtol2, const double* __restrict__ St,
                                                  double* __restrict__ vec, const double* __restrict__ wv, const double* __restrict__ dots,
                                                  double* __restrict__ P, double* __restrict__ scal, double* __restrict__ x_out, int flip,
                                                  double* __restrict__ hst /* pinned host words */, double seq) {
  // CGS_DONE holds 1 + the index of the launch that saw the end (converged or broken).  Only an EARLIER launch's verdict stops
  // this one: the tiles of the deciding launch itself all reach the same verdict from the same numbers, and each still has its
  // range of x to copy out - a tile that started late must not take tile 0's freshly written flag for yesterday's
  { const double dn = scal[CGS_DONE]; if (dn != 0.0 && dn <= (double)it) return; }
  __shared__ double s_r[2][SY_T];                   // the new r on the tile's row range (I) and column range (J)
  __shared__ double s_col[4][SY_T];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // t -> (I, J), J <= I: I = floor((sqrt(8 t + 1) - 1) / 2), corrected for the rounding of the root
  const int t = flip ? (int)(gridDim.x - 1u - blockIdx.x) : (int)blockIdx.x;
  int I = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((I + 1) * (I + 2) / 2 <= t) ++I;
  while (I * (I + 1) / 2 > t) --I;
  const int J = t - I * (I + 1) / 2;
  const int r0 = I * SY_T, c0 = J * SY_T;
  const size_t N4 = (size_t)4 * n;
  double* cur = vec + (size_t)((it + 1) & 1) * N4;     // launch it - 1 left r_{it-1}, p_{it-2}, s_{it-2}, x_{it-1} here (it = 0: unused)
  double* nxt = vec + (size_t)(it & 1) * N4;           // launch 0 reads r_0 from set 0
  // Loads return in issue order.  The few small ones the prologue needs (the dot products, the scalars, this thread's entries of
  // r, s, w, p, x) therefore go FIRST and the 32 matrix loads per thread behind them: the prologue's arithmetic then runs while
  // the tile streams in.  (With the matrix loads in front, every small load waited for all of them and the launch was 10 us
  // longer than the plain product it replaces: 70.8 against 61.2 us at n = 10,000.)
  const int half = tid >> 7, li = tid & 127;        // threads 0..127: range I, 128..255: range J
  const int gi = (half ? c0 : r0) + li;
  const bool own = I == J && half == 0;             // the range's diagonal tile keeps the vectors
  double g = 0.0, dl = 0.0, g_prev = 0.0, a_prev = 0.0, g0s = 0.0;
  double v_r = 0.0, v_s = 0.0, v_w = 0.0, v_p = 0.0, v_x = 0.0;
  if (it == 0) {
    v_r = gi < n ? nxt[gi] : 0.0;
  } else {
    for (int bb = lane; bb < nb; bb += 64) { g += dots[bb]; dl += dots[nbp + bb]; }
    g_prev = scal[CGB_PAIR + 1 + 2 * ((it + 1) & 1)]; a_prev = scal[CGB_PAIR + 2 * ((it + 1) & 1)]; g0s = scal[CGS_RR0];
    if (gi < n) {
      v_r = cur[gi]; v_s = cur[(size_t)2 * n + gi]; v_w = wv[gi];
      if (own) { v_p = cur[(size_t)n + gi]; v_x = cur[(size_t)3 * n + gi]; }
    }
  }
  const int jc = c0 + 2 * lane;                     // n is even: jc < n implies jc + 1 < n
  const bool col_ok = jc < n;
  double2 a[2][16];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int row = r0 + w * 32 + b * 16 + q;
      a[b][q] = (col_ok && row < n) ? *(const double2*)(St + (size_t)row * n + jc) : make_double2(0.0, 0.0);
    }
  if (it == 0) {
    s_r[half][li] = v_r;
  } else {
    // gamma_{it-1}, delta_{it-1}: the per-block parts, summed by every wave of every tile in the same order
    g = wave_sum_all(g); dl = wave_sum_all(dl);
    const double g0 = it == 1 ? g : g0s;
    const bool converged = g <= rtol2 * g0;          // (a zero right-hand side: 0 <= 0, x = 0)
    const double beta = it == 1 ? 0.0 : g / g_prev;
    const double den = it == 1 ? dl : dl - beta * g / a_prev;
    const bool broken = !converged && !(den > 0.0);  // non-positive curvature, or NaN anywhere: S~ is not positive definite
    if (t == 0 && tid == 0) {
      if (it == 1) scal[CGS_RR0] = g;
      scal[CGS_RR] = g; scal[CGS_ITER] = (double)(it - 1);
      if (converged || broken) scal[CGS_DONE] = (double)(it + 1);
      if (broken) scal[CGS_FAIL] = 2.0;
      // the host's copy, straight into its pinned page: where the solve stands (every launch) and, from the launch that sees the
      // end, the verdict with the system's ticket behind it - cgs_solve_big spins on the ticket and goes on enqueuing while the
      // launches it had queued blind behind this one are still returning
      const double fl = broken ? 2.0 : scal[CGS_FAIL];
      hst[CGS_RR0] = g0; hst[CGS_RR] = g; hst[CGS_ITER] = (double)(it - 1); hst[CGS_FAIL] = fl;
      if (converged || broken) {
        hst[CGS_DONE] = (double)(it + 1);
        publish_word(hst + 7, seq);
      }
    }
    if (converged) {                                 // (uniform over the whole grid) x_{it-1} is the answer
      if (own && gi < n) x_out[gi] = v_x;
      return;
    }
    if (broken) return;
    const double al = g / den;
    if (t == 0 && tid == 0) { scal[CGB_PAIR + 2 * (it & 1)] = al; scal[CGB_PAIR + 1 + 2 * (it & 1)] = g; }
    double rn = 0.0;
    if (gi < n) {
      const double sn = v_w + beta * v_s;
      rn = v_r - al * sn;
      if (own) {
        const double pn = v_r + beta * v_p;
        nxt[gi] = rn; nxt[(size_t)n + gi] = pn; nxt[(size_t)2 * n + gi] = sn; nxt[(size_t)3 * n + gi] = v_x + al * pn;
      }
    }
    s_r[half][li] = rn;
  }
  __syncthreads();
  const double pj0 = col_ok ? s_r[1][2 * lane] : 0.0, pj1 = col_ok ? s_r[1][2 * lane + 1] : 0.0;
  double cs0 = 0.0, cs1 = 0.0;
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    double v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const double pi = s_r[0][w * 32 + b * 16 + q];
      v[q] = a[b][q].x * pj0 + a[b][q].y * pj1;
      cs0 += a[b][q].x * pi; cs1 += a[b][q].y * pi;
    }
    const double rs = lane_rows16_sum(v, lane);
    const int row = r0 + w * 32 + b * 16 + (lane >> 2);
    if ((lane & 3) == 0 && row < n) P[(size_t)J * n + row] = rs;
  }
  if (I != J) {                                      // (workgroup-uniform) the diagonal tile is stored whole: row sums only
    s_col[w][2 * lane] = cs0; s_col[w][2 * lane + 1] = cs1;
    __syncthreads();
    if (tid < SY_T && c0 + tid < n) P[(size_t)I * n + c0 + tid] = (s_col[0][tid] + s_col[1][tid]) + (s_col[2][tid] + s_col[3][tid]);
  }
}
// w = S~ r = sum over the nb slots (fixed order); the block's parts of gamma = r.r and delta = w.r.  One workgroup of 128 per
// block of 128 entries.  r is the one launch `it` of the tile kernel has just formed (set it & 1).
__global__ __launch_bounds__(128) void k_cgb_reduce(int n, int nb, int nbp, int it, const double* __restrict__ P, const double* __restrict__ vec,
                                                    double* __restrict__ wv, double* __restrict__ dots, const double* __restrict__ scal) {
  if (scal[CGS_DONE] != 0.0) return;
  __shared__ double s_w[2][2];
  const int i = (int)blockIdx.x * SY_T + threadIdx.x;
  const double* r = vec + (size_t)(it & 1) * 4 * n;
  double sum = 0.0, ri = 0.0;
  if (i < n) {
    ri = r[i];
    // 79 slots at n = 10,000 and only 79 workgroups: the launch is as long as a thread's chain of loads.  32 of them in flight
    // at a time (the additions in slot order all the same): 8.9 -> 6.0 us per launch
    for (int k0 = 0; k0 < nb; k0 += 32) {
      double t[32];
#pragma unroll
      for (int q = 0; q < 32; ++q) t[q] = (k0 + q < nb) ? P[(size_t)(k0 + q) * n + i] : 0.0;
#pragma unroll
      for (int q = 0; q < 32; ++q) sum = (k0 + q < nb) ? sum + t[q] : sum;
    }
    wv[i] = sum;
  }
  const double g = wave_sum_all(ri * ri), d = wave_sum_all(sum * ri);
  if ((threadIdx.x & 63) == 0) { s_w[0][threadIdx.x >> 6] = g; s_w[1][threadIdx.x >> 6] = d; }
  __syncthreads();
  if (threadIdx.x == 0) { dots[blockIdx.x] = s_w[0][0] + s_w[0][1]; dots[nbp + blockIdx.x] = s_w[1][0] + s_w[1][1]; }
}

// its_hint: iterations the last converged system of this problem took (0: unknown) - the first batch of launches is sized for it
// (a batch is enqueued blind and the host looks at the residual behind it; launches past convergence return at once but still
// cost ~3 us each: at 14 iterations per system, 30 of the fixed first batch of 72 launches were such)
static int cgs_solve_big(sfm_ctx* h, int n, const double* St, const double* rhs_t, double* x_t, double* buf, double* scal,
                         double rtol, int budget, int* iters_out, int* status, int its_hint) {
  const double rtol2 = rtol * rtol;
  *status = 1;
  const int nb = (int)cdiv(n, SY_T), nbp = (nb + 127) & ~127;
  const unsigned n_tiles = (unsigned)((int64_t)nb * (nb + 1) / 2);
  double *vec = buf, *wv = buf + 8 * (size_t)n, *dots = wv + n, *P = dots + 2 * (size_t)nbp;
  hipLaunchKernelGGL(k_cgb_init, dim3(cdiv(n > 2 * nbp ? n : 2 * nbp, 256)), dim3(256), 0, h->stream, n, nbp, rhs_t, vec, dots, scal);
  // launch `it` forms r_it (it >= 1: from the dot products launch it - 1 left) and multiplies; launch it = k + 1 is the one that
  // sees iterate k converged and copies it out, so a system of k iterations takes k + 2 launch pairs
  // The triangle (405 MB at n = 10,000) is larger than the memory-side cache (256 MB): walked in the same direction every
  // iteration, nothing of it is ever found there (a cyclic walk is LRU's worst case); walked back and forth, the tail of the
  // previous pass is.  Odd launches therefore take the tiles in descending order: 1,361 -> 1,215 us per second system at cfg5
  // (tools/experiments/README.md).  Which tile a workgroup takes changes nothing in the arithmetic: every tile's partial sums go
  // to its own slot.
  int it = 0;
  int batch = its_hint > 0 ? (its_hint + 4 > 48 ? 48 : its_hint + 4) : 24;
  // The verdict comes through the pinned page (k_cgb_symv): the host spins on this system's ticket (ba_wait_for_word), which also
  // ends when the stream has drained (a batch that ended without a verdict).  No status copy, no stream synchronisation
  // on the way of a system that converges within its batch - and the caller's next launches queue up behind the blind launches
  // still returning.  (No launch of an earlier system can write here: all of them return at their first instruction.)
  volatile double* hst = h->pinned + SFM_PIN_CGB;
  h->cgb_seq += 1.0;
  const double seq = h->cgb_seq;
  for (int q = 0; q < 7; ++q) hst[q] = 0.0;
  while (it < budget + 2) {
    for (int b = 0; b < batch && it < budget + 2; ++b, ++it) {
      hipLaunchKernelGGL(k_cgb_symv, dim3(n_tiles), dim3(256), 0, h->stream, n, nb, nbp, it, rtol2, St, vec, wv, dots, P, scal, x_t, it & 1,
                         h->pinned + SFM_PIN_CGB, seq);
      hipLaunchKernelGGL(k_cgb_reduce, dim3(nb), dim3(128), 0, h->stream, n, nb, nbp, it, P, vec, wv, dots, scal);
    }
    bool seen = ba_wait_for_word(h, hst + 7, seq);
    if (!seen) {
      SFM_HIP(h, hipStreamSynchronize(h->stream));
      seen = hst[7] == seq;                           // (the verdict of the batch's last launches)
    }
    if (seen && hst[CGS_FAIL] != 0.0) break;
    if (seen) { *status = 0; break; }                 // (the launch that saw the end has copied x out)
    if (hst[CGS_FAIL] != 0.0) break;                  // a diagonal block was not positive definite (raised before the first launch)
    const double rr = hst[CGS_RR], rr0 = hst[CGS_RR0];
    batch = cgs_next_batch(rr, rr0, hst[CGS_ITER], rtol2, 3, 48);
  }
  *iters_out += (int)hst[CGS_ITER];
  SFM_LAUNCH_CHECK(h, "cgs_solve_big");
  return SFM_OK;
}

// S~ x~ = r~ (r~ in cg_r, x~ into cg_z) by the plan's launch-per-iteration CG
static int cgs_solve_per_launch(sfm_ctx* h, sfm_ba_problem p, const Lay& L, const DenseWs& dw, const CamPlan& plan, int* status, int its_hint) {
  double* ws = (double*)p->workspace;
  const int n = p->n_cams * p->cam_dim;
  if (plan.per_launch == CAM_CG_TILES)
    return cgs_solve_big(h, n, dw.Lm, WS(L, cg_r), WS(L, cg_z), dw.LmT, WS(L, cg_scal), CGS_RTOL, plan.budget, &p->cg_iters, status, its_hint);
  return cgs_solve(h, n, dw.Lm, WS(L, cg_r), WS(L, cg_z), dw.LmT, WS(L, cg_scal), CGS_RTOL, &p->cg_iters, status);
}

__global__ void k_add_diag(double* __restrict__ A, int n, double alpha) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) A[(size_t)i * n + i] += alpha;
}
// S + alpha I = L L^T into the factor's buffer, where S~ was (S is formed from the item tiles first if the build left S~ only);
// row n of [S | r]: r -> L^-1 r
static int factor_system(sfm_ctx* h, sfm_ba_problem p, const Lay& L, const DenseWs& dw, double alpha) {
  double* ws = (double*)p->workspace;
  const int n = p->n_cams * p->cam_dim;
  int rc = schur_materialise_S(h, p, L); if (rc) return rc;
  p->st_alpha = -1.0;
  SFM_HIP(h, hipMemsetAsync(dw.flag, 0, sizeof(int), h->stream));       // the factorisation's failure flag (k_finish_solve reads it)
  hipLaunchKernelGGL(k_add_diag, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, WS(L, red_S), n, alpha);
  return dense_cholesky(h, WS(L, red_S), n, n + 1, dw);
}

// scalars after the solve: PNORM2 = ||p_c||^2 + sum ||p_p||^2 ; PQ = sum ||v||^2 + ||y||^2
__global__ __launch_bounds__(256) void k_finish_solve(int n, const double* __restrict__ pc,
                                                      const double* __restrict__ red_q,
                                                      const double* __restrict__ y, int want_q,
                                                      const int* __restrict__ flag, double* __restrict__ sc, double* __restrict__ hsc,
                                                      double seq) {
  __shared__ double s_red[4];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    a += pc[i] * pc[i];
    if (want_q) b += y[i] * y[i];
  }
  double at = block_sum256(a, s_red);
  double bt = block_sum256(b, s_red);
  if (threadIdx.x == 0) {
    const double pn2 = at + red_q[n], pq = want_q ? (bt + red_q[n + 1]) : 0.0;
    sc[SFM_SC_PNORM2] = hsc[SFM_SC_PNORM2] = pn2;
    sc[SFM_SC_PQ] = hsc[SFM_SC_PQ] = pq;
    // 1: non-positive pivot, 2: a triangular solve stalled, 3: the step is not finite (NaN/Inf in the system)
    int f = *flag;
    if (f == 0 && !(isfinite(pn2) && isfinite(pq))) f = 3;
    sc[SFM_SC_CHOL_FAIL] = hsc[SFM_SC_CHOL_FAIL] = (double)f;
    publish_ticket(hsc, seq);
  }
}
// scalars after a PCG solve: PNORM2 = ||p_c||^2 + sum ||p_p||^2, PQ = rhs2^T S^-1 rhs2 + sum ||v||^2, failure code
__global__ __launch_bounds__(256) void k_finish_solve_pcg(int n, const double* __restrict__ pc, const double* __restrict__ red_q,
                                                          int want_q, const double* __restrict__ dotp, const double* __restrict__ failp,
                                                          double* __restrict__ sc, double* __restrict__ hsc, double seq) {
  __shared__ double s_red[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) a += pc[i] * pc[i];
  const double at = block_sum256(a, s_red);
  if (threadIdx.x == 0) {
    const double pn2 = at + red_q[n], pq = want_q ? (*dotp + red_q[n + 1]) : 0.0;
    sc[SFM_SC_PNORM2] = hsc[SFM_SC_PNORM2] = pn2; sc[SFM_SC_PQ] = hsc[SFM_SC_PQ] = pq;
    double f = *failp != 0.0 ? 1.0 : 0.0;                   // 1: a block or S itself is not positive definite
    if (f == 0.0 && !(isfinite(pn2) && isfinite(pq))) f = 3.0;
    sc[SFM_SC_CHOL_FAIL] = hsc[SFM_SC_CHOL_FAIL] = f;
    publish_ticket(hsc, seq);
  }
}
void launch_finish_solve_pcg(sfm_ctx* h, sfm_ba_problem p, const Lay& L, int want_q, const double* dotp, const double* failp) {
  double* ws = (double*)p->workspace;
  hipLaunchKernelGGL(k_finish_solve_pcg, dim3(1), dim3(256), 0, h->stream, p->n_cams * p->cam_dim, WS(L, pc), WS(L, red_q), want_q, dotp,
                     failp, WS(L, scalars), p->host_sc, next_ticket(p));
}

extern "C" int sfm_ba_schur_solve(sfm_handle h, sfm_ba_problem p, double alpha, int want_q) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  double* ws = (double*)p->workspace;
  const int C = p->n_cams, D = p->cam_dim, n = C * D;
  double* S = WS(L, red_S);
  DenseWs dw; dense_ws_carve(WS(L, dense), n, &dw);
  p->cg_state = 0;
  p->cg2_pending = 0;
  p->cg_alpha = alpha;
  const BaSwitches sw = ba_switches_from_env();
  const CamPlan plan = cam_plan(n, p->camera_solver, h->cgs_persist_off != 0, sw);
  // AUTO only: a system predicted to exhaust the CG's budget goes to the factorisation at once (CgPredictor)
  const double hdiag = p->host_sc[SFM_SC_HDIAG];
  const double arel = hdiag > 0.0 ? alpha / hdiag : 0.0;
  const bool hopeless = p->camera_solver == SFM_CAMERA_SOLVER_AUTO && arel > 0.0 && sw.predict && p->cgp.hopeless(arel, plan.budget);
  if (hopeless) p->cg_fallbacks++;
  if (plan.route != CAM_FACTOR && !hopeless) {
    const int its_before = p->cg_iters;
    // S~ = E^-1 (S + alpha I) E^-T into the factor's buffer (S stays as it is: the fallback below needs it), r~ = E^-1 r
    sfm_prof_begin(h, SFM_PROF_CHOL);
    // (cleared by k_schur_assemble when this solve follows its own sfm_ba_schur_build, as it does in every loop of this library)
    if (!p->cg_scal_clean) { SFM_HIP(h, hipMemsetAsync(WS(L, cg_scal), 0, CG_SCAL_WORDS * sizeof(double), h->stream)); p->einv_alpha = -1.0; }
    p->cg_scal_clean = 0;
    const bool have_einv = p->einv_alpha == alpha && !p->sharded;      // k_schur_assemble of THIS system left them
    p->einv_alpha = -1.0;
    // ... or the scaled system itself (tile-streaming route: k_schur_assemble_scaled)
    const bool have_st = have_einv && p->st_alpha == alpha && plan.lower_only;
    if (!have_st && (rc = schur_materialise_S(h, p, L))) return rc;
    if (!have_st) DISPATCH_D(D, {
      if (!have_einv)
        hipLaunchKernelGGL(k_diag_einv<DD>, dim3(cdiv(C, 64)), dim3(64), 0, h->stream, C, S, n, alpha, WS(L, cg_Minv), WS(L, cg_M), WS(L, cg_scal));
      if (plan.lower_only)
        hipLaunchKernelGGL(k_scale_system_lower<DD>, dim3(C, cdiv(C, SCALE_NB)), dim3(128), 0, h->stream, n, C, S, alpha, WS(L, cg_Minv), dw.Lm,
                           S + (size_t)n * n, WS(L, cg_r));
      else
        hipLaunchKernelGGL(k_scale_system<DD>, dim3(C, cdiv(C, SCALE_NB)), dim3(128), 0, h->stream, n, C, S, alpha, WS(L, cg_Minv), dw.Lm,
                           S + (size_t)n * n, WS(L, cg_r));
    });
    int status = 1, ran = 0;
    if (plan.route == CAM_CG_PERSIST) {
      // ONE persistent launch: r~ = E^-1 r in its prologue, p_c = -E^-T x~ in its epilogue.  The host needs its verdict
      // (converged / fall back) but must not idle the GPU for it: the status words are copied to pinned memory, an event is
      // recorded behind the copy, the back-substitution is enqueued on the assumption that the solve converged (it does: 0
      // fallbacks in the bench schedules), and only then the host waits - for the event, not for the stream.
      PrFuse fuse = {WS(L, cg_Minv), nullptr, WS(L, pc), nullptr, nullptr, nullptr, nullptr, 1, 0.0};      // rhs~ = cg_r (k_scale_system)
      const PrLaunch pl = {n, D, dw.Lm, WS(L, cg_r), WS(L, cg_z), WS(L, cg_mail), WS(L, cg_scal), CGS_RTOL, fuse, h->pinned + SFM_PIN_CG1};
      rc = cgs_persist_launch(h, pl);
      if (rc) return rc;
      SFM_HIP(h, hipEventRecord(h->cg_event, h->stream));
      sfm_prof_end(h, SFM_PROF_CHOL);
      launch_backsub(h, p, L, want_q);
      SFM_HIP(h, hipEventSynchronize(h->cg_event));
      int relaunched = 0;
      rc = cgs_persist_verdict(h, pl, p->sharded, &p->cg_iters, &status, &ran, &relaunched);
      if (rc) return rc;
      if (relaunched && ran && status == 0) launch_backsub(h, p, L, want_q);      // the first one ran on an unfinished p_c
      if (ran && status == 0) {
        p->cg_state = 1;
        p->cgp.note_ok(arel, p->cg_iters - its_before);
        SFM_LAUNCH_CHECK(h, "sfm_ba_schur_solve");
        return SFM_OK;
      }
      sfm_prof_begin(h, SFM_PROF_CHOL);             // not converged or abandoned: the routes below, then the back-substitution again
    }
    if (!ran) {                                       // plan.per_launch: one launch (pair) per iteration, with the scaling of r and of the solution as kernels of their own
      DISPATCH_D(D, hipLaunchKernelGGL(k_block_mv<DD>, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, C, WS(L, cg_Minv), S + (size_t)n * n, WS(L, cg_r), 0, 1.0));
      rc = cgs_solve_per_launch(h, p, L, dw, plan, &status, p->cgp.ok_its[0]);
      if (rc) return rc;
      p->cg_its_sys1 = p->cg_iters - its_before;
      if (status == 0)
        DISPATCH_D(D, hipLaunchKernelGGL(k_block_mv<DD>, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, C, WS(L, cg_Minv), WS(L, cg_z),
                                         WS(L, pc), 1, -1.0));                      // p_c = -E^-T x~
    }
    if (status == 0) {
      p->cg_state = 1;
      p->cgp.note_ok(arel, p->cg_iters - its_before);
    } else {
      p->cg_fallbacks++;
      p->cgp.note_out_of_budget(arel, p->cg_iters - its_before, plan.budget);
    }
    sfm_prof_end(h, SFM_PROF_CHOL);
  }
  if (p->cg_state == 0) {
    sfm_prof_begin(h, SFM_PROF_CHOL);
    rc = factor_system(h, p, L, dw, alpha); if (rc) return rc;
    sfm_prof_end(h, SFM_PROF_CHOL);
    sfm_prof_begin(h, SFM_PROF_TRSV);
    // p_c = -L^-T (L^-1 r)
    ba_copy_neg(h, dw.Lm + (size_t)n * n, WS(L, tvec), n, -1.0);
    rc = dense_trsv(h, n, dw, WS(L, tvec), WS(L, pc), 1); if (rc) return rc;
    sfm_prof_end(h, SFM_PROF_TRSV);
  }
  launch_backsub(h, p, L, want_q);
  SFM_LAUNCH_CHECK(h, "sfm_ba_schur_solve");
  return SFM_OK;
}

// the q term from the factorisation (S intact in red_S): used when the CG on the second system did not converge
static int finish_solve_by_factor(sfm_ctx* h, sfm_ba_problem p, const Lay& L, double* ws, int want_q, bool factor_first) {
  const int n = p->n_cams * p->cam_dim;
  DenseWs dw; dense_ws_carve(WS(L, dense), n, &dw);
  int rc;
  if (factor_first) {
    p->cg_fallbacks++;
    p->cg_state = 0;
    rc = factor_system(h, p, L, dw, p->cg_alpha); if (rc) return rc;
  }
  if (want_q) {
    // rhs2 = p_c - W C_a^-1 p_p ;  y = L^-1 rhs2
    sfm_prof_begin(h, SFM_PROF_TRSV);
    ba_add_vec(h, WS(L, pc), WS(L, red_q), WS(L, tvec), n);
    rc = dense_trsv(h, n, dw, WS(L, tvec), WS(L, y), 0); if (rc) return rc;
    sfm_prof_end(h, SFM_PROF_TRSV);
  }
  hipLaunchKernelGGL(k_finish_solve, dim3(1), dim3(256), 0, h->stream, n, WS(L, pc), WS(L, red_q), WS(L, y),
                     want_q, (const int*)dw.flag, WS(L, scalars), p->host_sc, next_ticket(p));
  SFM_LAUNCH_CHECK(h, "sfm_ba_finish_solve");
  return SFM_OK;
}

extern "C" int sfm_ba_finish_solve(sfm_handle h, sfm_ba_problem p, int want_q) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  double* ws = (double*)p->workspace;
  const int n = p->n_cams * p->cam_dim;
  DenseWs dw; dense_ws_carve(WS(L, dense), n, &dw);
  const CamPlan plan = cam_plan(n, p->camera_solver, h->cgs_persist_off != 0, ba_switches_from_env());
  if (p->cg_state == 1) {
    // the camera system was solved by CG on the scaled system S~ (still in dw.Lm): p^T (H + alpha I)^-1 p needs
    // rhs2^T S^-1 rhs2 = r~2^T x~2 with r~2 = E^-1 rhs2, S~ x~2 = r~2
    const int C = p->n_cams, D = p->cam_dim;
    int status = 0;
    if (want_q) {
      sfm_prof_begin(h, SFM_PROF_TRSV);
      if (plan.route == CAM_CG_PERSIST) {
        // ONE persistent launch: r~2 = E^-1 (p_c + rhs2 pieces) in its prologue, r~2 . x~2 and the scalars of the solve in its
        // epilogue.  Its verdict travels to pinned memory with the copy enqueued behind it and is looked at where the host
        // synchronises anyway: in sfm_ba_read_scalars, which redoes this step from the factorisation if it has to.
        // rhs~2 = E^-1 (p_c + rhs2 pieces) by one small launch (in the CG kernel's prologue every workgroup formed all of it)
        DISPATCH_D(D, hipLaunchKernelGGL(k_block_mv<DD>, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, C, WS(L, cg_Minv), WS(L, pc),
                                         WS(L, cg_r), 0, 1.0, WS(L, red_q)));
        PrFuse fuse = {WS(L, cg_Minv), nullptr, nullptr, WS(L, pc), WS(L, red_q), WS(L, scalars), p->host_sc, 1, next_ticket(p)};
        const PrLaunch pl = {n, D, dw.Lm, WS(L, cg_r), WS(L, cg_z), WS(L, cg_mail), WS(L, cg_scal), CGS_RTOL, fuse, p->host_sc + SFM_HSC_CG2};
        rc = cgs_persist_launch(h, pl);
        if (rc) return rc;
        p->cg2_pending = 1;
        sfm_prof_end(h, SFM_PROF_TRSV);
        return SFM_OK;
      }
      ba_add_vec(h, WS(L, pc), WS(L, red_q), WS(L, tvec), n);
      DISPATCH_D(D, hipLaunchKernelGGL(k_block_mv<DD>, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, C, WS(L, cg_Minv), WS(L, tvec),
                                       WS(L, cg_r), 0, 1.0));
      // (the q system of a damped solve takes about as many iterations as its step system just did)
      rc = cgs_solve_per_launch(h, p, L, dw, plan, &status, p->cg_its_sys1);
      if (rc) return rc;
      if (status == 0)
        ba_dot(h, n, WS(L, cg_r), WS(L, cg_z), WS(L, cg_scal) + 8);
      sfm_prof_end(h, SFM_PROF_TRSV);
    }
    if (status == 0) {
      launch_finish_solve_pcg(h, p, L, want_q, WS(L, cg_scal) + 8, WS(L, cg_scal) + CGS_FAIL);
      SFM_LAUNCH_CHECK(h, "sfm_ba_finish_solve");
      return SFM_OK;
    }
    // the second system did not converge: factor after all (S is intact) and take the q term from the factor
    return finish_solve_by_factor(h, p, L, ws, want_q, true);
  }
  return finish_solve_by_factor(h, p, L, ws, want_q, false);
}

// The verdict of the persistent CG on the second system of the last damped solve has arrived with the wait of sfm_ba_read_scalars; if it
// did not converge - or was abandoned - the q term is redone from the factorisation now (no exchange between ranks: red_q is reduced already)
int cgs_second_system_verdict(sfm_ctx* h, sfm_ba_problem p, const Lay& L) {
  double* ws = (double*)p->workspace;
  p->cg2_pending = 0;
  int status = 1, ran = 0, relaunched = 0;
  const int D = p->cam_dim, n = p->n_cams * D;      // (a relaunch finds the same inputs: r~2 is still in cg_r, S~ in the factor's buffer)
  DenseWs dw; dense_ws_carve(WS(L, dense), n, &dw);
  PrFuse fuse = {WS(L, cg_Minv), nullptr, nullptr, WS(L, pc), WS(L, red_q), WS(L, scalars), p->host_sc, 1, p->look_seq};
  const PrLaunch pl = {n, D, dw.Lm, WS(L, cg_r), WS(L, cg_z), WS(L, cg_mail), WS(L, cg_scal), CGS_RTOL, fuse, p->host_sc + SFM_HSC_CG2};
  int rc = cgs_persist_verdict(h, pl, p->sharded, &p->cg_iters, &status, &ran, &relaunched);
  if (rc) return rc;
  if (!(ran && status == 0)) {
    if ((rc = finish_solve_by_factor(h, p, L, ws, 1, true))) return rc;
    SFM_HIP(h, hipStreamSynchronize(h->stream));
  }
  return SFM_OK;
}
