// Device helpers, constants and host dispatch macros shared by the bundle-adjustment units (ba*.hip).  Every function here is
// __forceinline__: a kernel's code does not depend on the unit that instantiates it.  (block_sum1024 is here because k_dot in
// ba.hip uses it besides the PCG; g_stride and GTP_OBS have one user each and stay with it in ba.hip.)
#pragma once
#include "ba_internal.h"
#include <cstdlib>
#include <cmath>

typedef double v4d __attribute__((ext_vector_type(4)));
// a ticket into a pinned host word, BEHIND everything this thread has written before (the host spins on the word); seq 0: none
__device__ __forceinline__ void publish_word(double* word, double seq) {
  if (seq > 0.0) {
    __threadfence_system();
    *(volatile double*)word = seq;
  }
}
// the ticket of a finished stage into the problem's pinned page, behind the scalars (sfm_ba_read_scalars)
__device__ __forceinline__ void publish_ticket(double* hsc, double seq) { publish_word(hsc + SFM_HSC_SEQ, seq); }

#define EPS_D 2.220446049250313e-16
#define SQRT_EPS_D 1.4901161193847656e-08
#define CAMPRE 16   // r[3] t[3] fx fy cx cy  a b a1 b1 (Rodrigues coefficients)  |r|^2 pad

// The same sums without a trip through LDS per step (__shfl_* is ds_bpermute: ~100 cycles each, six in a row per wave_sum - in
// the persistent CG, one wave per SIMD, that latency is the iteration): quad permutes and row mirrors (DPP) inside a row of 16
// lanes, v_permlane16_swap / v_permlane32_swap across rows.  Every step adds a value and its partner's in the same order on both
// sides, so ALL lanes end with bit-identical totals.  Measured (cfg4, 20 outer iterations after 5): camera-solve slots 155 + 123
// -> 140 + 104 us per damped solve, 310 -> 322 LM-iterations/s.
template <int CTRL> __device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
// {a, b} -> (swap16: rows 1, 3 of a <-> rows 0, 2 of b; swap32: upper half of a <-> lower half of b), then a + b: with a = b = v
// the sum of v over the two rows / halves in every lane, with two different registers one step of a halving exchange (the
// even rows / lower half end with a's sum, the odd rows / upper half with b's)
__device__ __forceinline__ double swap16_add(double a, double b) {
  const auto rlo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const auto rhi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  return __hiloint2double((int)rhi[0], (int)rlo[0]) + __hiloint2double((int)rhi[1], (int)rlo[1]);
}
__device__ __forceinline__ double swap32_add(double a, double b) {
  const auto rlo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const auto rhi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  return __hiloint2double((int)rhi[0], (int)rlo[0]) + __hiloint2double((int)rhi[1], (int)rlo[1]);
}
__device__ __forceinline__ double wave_sum_all(double v) {
  v += dpp_f64<0xB1>(v);          // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);          // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);         // row_half_mirror
  v += dpp_f64<0x140>(v);         // row_mirror: every lane of a row holds the row's sum
  v = swap16_add(v, v);           // rows 0 + 1, rows 2 + 3
  return swap32_add(v, v);        // both halves
}
// (every lane gets the total; the callers that say "valid in lane 0" predate the DPP form)
__device__ __forceinline__ double wave_sum(double v) { return wave_sum_all(v); }
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
  return v;
}
// v[q] = this lane's part of the sum of row q (8 rows); returns, in every lane, the sum over the 64 lanes of row
// 4 (lane >> 5) + 2 ((lane >> 4) & 1) + ((lane >> 3) & 1): the halves of the wave, then neighbouring rows of 16 lanes, then the two
// halves of a row of 16 each pass HALF of what they hold to their partner and keep the other half (4 + 2 + 1 additions), the
// last eight lanes are summed by mirrors / quad permutes (3 additions).  Fixed order: the same bits on every workgroup.
__device__ __forceinline__ double lane_rows8_sum(double (&v)[8], int lane) {
  double u[4], x[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) u[k] = swap32_add(v[k], v[k + 4]);        // upper half keeps rows + 4
#pragma unroll
  for (int k = 0; k < 2; ++k) x[k] = swap16_add(u[k], u[k + 2]);        // odd rows of 16 lanes keep rows + 2
  const bool hi = (lane & 8) != 0;                                      // lanes 8..15 of a row keep rows + 1
  const double send = hi ? x[0] : x[1], keep = hi ? x[1] : x[0];
  double t = keep + dpp_f64<0x140>(send);                               // row_mirror: lane i <-> lane 15 - i
  t += dpp_f64<0x141>(t);                                               // row_half_mirror: lane i <-> lane 7 - i of its eight
  t += dpp_f64<0xB1>(t);                                                // the four lanes of a quad
  t += dpp_f64<0x4E>(t);
  return t;
}
// Sum over a 256-thread block, fixed order, in every thread.  s: >= 4 doubles of LDS.
__device__ __forceinline__ double block_sum256_fast(double v, double* s) {
  v = wave_sum_all(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s[0] + s[1]) + (s[2] + s[3]);
}
// Sum over a 256-thread block, fixed order; result valid in thread 0.  s: >= 4 doubles of LDS.
__device__ __forceinline__ double block_sum256(double v, double* s) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  return s[0] + s[1] + s[2] + s[3];
}
__device__ __forceinline__ double block_max256(double v, double* s) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(s[0], s[1]), fmax(s[2], s[3]));
}

// Huber, per scalar residual, exactly as scipy least_squares.py:169-178 + common.py:720-731:
// returns rho0; scale = sqrt(max(rho1 + 2 rho2 f^2, EPS)); ft = f * rho1 / scale.
__device__ __forceinline__ double huber_row(double f, double& scale, double& ft) {
  double z = f * f;
  if (z <= 1.0) { scale = 1.0; ft = f; return z; }
  double sz = sqrt(z);
  // rho1 + 2*rho2*z with rho2 = -0.5 z^-1.5 is 0 up to rounding -> clamped to EPS
  scale = SQRT_EPS_D;
  // f rho1 = f / |f| is sign(f): taken as such, ft = +-2^26 exactly.  (f * (1.0 / sz) rounds to 1 - 2^-53 for about one f in
  // seven.)  f * 0.0 adds nothing to a finite f and keeps a non-finite one poisoning the gradient as the product did.
  ft = f * 0.0 + copysign(1.0 / SQRT_EPS_D, f);
  return 2.0 * sz - 1.0;
}
__device__ __forceinline__ double huber_rho0(double f) {
  double z = f * f;
  return z <= 1.0 ? z : 2.0 * sqrt(z) - 1.0;
}

__device__ __forceinline__ void mat3_mul(const double* A, const double* Bm, double* Cm) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      Cm[i * 3 + j] = A[i * 3] * Bm[j] + A[i * 3 + 1] * Bm[3 + j] + A[i * 3 + 2] * Bm[6 + j];
}

// Sum over a 1024-thread block, fixed order; every thread gets the result.  s: >= 17 doubles of LDS.
__device__ __forceinline__ double block_sum1024(double v, double* s) {
  v = wave_sum_all(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < 16; ++w) t += s[w];
  return t;
}

// In-register Cholesky of a small SPD block and the inverse of its factor (one thread per block; D <= 10):
// L (lower part valid on entry) <- chol(L), X <- L^-1 (lower, zeros above).  Returns false on a non-positive pivot.
template <int D>
__device__ __forceinline__ bool small_chol_inverse(double (&L)[D][D], double (&X)[D][D]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    // (explicit fused multiply-adds: the cooperative form of this routine in k_schur_assemble must round exactly alike, and what
    // the compiler contracts on its own depends on the code around it)
    double sum = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) sum = fma(-L[j][k], L[j][k], sum);
    if (!(sum > 0.0)) { ok = false; sum = 1.0; }
    const double l = sqrt(sum);
    L[j][j] = l;
#pragma unroll
    for (int i = j + 1; i < D; ++i) {
      double t = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) t = fma(-L[i][k], L[j][k], t);
      L[i][j] = t / l;
    }
  }
#pragma unroll
  for (int t = 0; t < D; ++t)
#pragma unroll
    for (int r = 0; r < D; ++r) {
      double sum = (r == t) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < r; ++k) sum = (k >= t) ? fma(-L[r][k], X[k][t], sum) : sum;
      X[r][t] = (r >= t) ? sum / L[r][r] : 0.0;
    }
  return ok;
}

#define WS(L, field) (ws + (L).field)
// camera block width DD and G block stride GG (doubles; G is always float64; = g_stride in ba.hip) ...
#define DISPATCH_D(D, ...)                                                           \
  do {                                                                               \
    if ((D) == 10) { constexpr int DD = 10; constexpr int GG = 32; __VA_ARGS__; }    \
    else { constexpr int DD = 6; constexpr int GG = 18; __VA_ARGS__; }               \
  } while (0)
// ... and the storage type TT of the Jacobian records as well
#define DISPATCH_DT(D, PREC, ...)                                                    \
  do {                                                                               \
    if ((PREC) == SFM_BA_MIXED) { typedef float TT; DISPATCH_D(D, __VA_ARGS__); }    \
    else { typedef double TT; DISPATCH_D(D, __VA_ARGS__); }                          \
  } while (0)
#define WST(L, field) ((TT*)(ws + (L).field))
