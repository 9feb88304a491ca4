// Bundle adjustment, everything that evaluates the camera model: per-camera precompute, linearisation, block accumulation,
// trial step and cost, reprojection errors.  (Data layout: ba.hip.)
#include "ba_internal.h"
#include "ba_device.h"

// ------------------------------------------------------------------------------------ per-camera precompute
// Rodrigues coefficients of R = I + a[r]x + b[r]x^2 and of dR/dr_i (same series / closed-form split as the
// oracle's _rod_coeffs).  Only 14 doubles per camera are kept; R X and (dR/dr_i) X are rebuilt per observation
// from cross products (cam_apply below) - gathering a 3x3 R and three 3x3 dR per observation cost more L1/TA
// traffic than the kernel's whole HBM stream.
template <int D>
__device__ __forceinline__ void campre_row(const double (&p)[D], double fx0, double fy0, double cx0, double cy0, double* __restrict__ o) {
  const double th2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
  double a, b, a1, b1;
  if (th2 < 1e-4) {
    double z = th2;
    a = 1.0 - z / 6.0 + z * z / 120.0;
    b = 0.5 - z / 24.0 + z * z / 720.0;
    a1 = -1.0 / 3.0 + z / 30.0 - z * z / 840.0;
    b1 = -1.0 / 12.0 + z / 180.0 - z * z / 6720.0;
  } else {
    double t = sqrt(th2), s, co;
    sincos(t, &s, &co);
    a = s / t;
    b = (1.0 - co) / th2;
    a1 = (t * co - s) / (th2 * t);
    b1 = (t * s - 2.0 * (1.0 - co)) / (th2 * th2);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) o[i] = p[i];
  if (D == 10) { o[6] = p[6]; o[7] = p[7]; o[8] = p[8]; o[9] = p[9]; }
  else { o[6] = fx0; o[7] = fy0; o[8] = cx0; o[9] = cy0; }
  o[10] = a; o[11] = b; o[12] = a1; o[13] = b1; o[14] = th2; o[15] = 0.0;
}
template <int D>
__global__ void k_campre(const double* __restrict__ cams, int C, double fx0, double fy0, double cx0,
                         double cy0, double* __restrict__ out) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double p[D];
#pragma unroll
  for (int i = 0; i < D; ++i) p[i] = cams[(size_t)c * D + i];
  campre_row<D>(p, fx0, fy0, cx0, cy0, out + (size_t)c * CAMPRE);
}

// Y = R X + t  with  R X = X + a (r x X) + b (r x (r x X))
__device__ __forceinline__ void cam_project(const double* __restrict__ cp, double X0, double X1, double X2,
                                            double& Y0, double& Y1, double& Y2) {
  const double r0 = cp[0], r1 = cp[1], r2 = cp[2], a = cp[10], b = cp[11];
  const double c0 = r1 * X2 - r2 * X1, c1 = r2 * X0 - r0 * X2, c2 = r0 * X1 - r1 * X0;       // r x X
  const double e0 = r1 * c2 - r2 * c1, e1 = r2 * c0 - r0 * c2, e2 = r0 * c1 - r1 * c0;       // r x (r x X)
  Y0 = X0 + a * c0 + b * e0 + cp[3];
  Y1 = X1 + a * c1 + b * e1 + cp[4];
  Y2 = X2 + a * c2 + b * e2 + cp[5];
}

// ------------------------------------------------------------------------------------ linearise: per observation
// One thread per observation (point-major).  Residual (sfm_reconstruction.py:453-470,486), analytic
// 2x(D+3) Jacobian, Huber row scaling.  The two record arrays are transposed through
// LDS one after the other (43 KB instead of 59 KB: 3 workgroups per CU) so the doubles of 256 observations
// leave the CU as contiguous, fully coalesced streams.
template <int D, typename T>
__global__ __launch_bounds__(256) void k_lin_obs(int64_t N, const int* __restrict__ cam_idx,
                                                 const int* __restrict__ pt_idx,
                                                 const double* __restrict__ uv,
                                                 const double* __restrict__ pts,
                                                 const double* __restrict__ campre,
                                                 T* __restrict__ recA, T* __restrict__ recB,
                                                 double* __restrict__ part) {
  constexpr int WA = 2 * D, LDA = WA + 1, WB = 8, LDB = WB + 1;
  __shared__ double s_rec[256 * LDA];
  __shared__ double s_red[4];
  const int tid = threadIdx.x;
  const int64_t k0 = (int64_t)blockIdx.x * 256;
  const int64_t k = k0 + tid;
  double cost = 0.0;
  double jb[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) jb[q] = 0.0;
  if (k < N) {
    const int c = cam_idx[k], j = pt_idx[k];
    const double* cp = campre + (size_t)c * CAMPRE;
    const double X0 = pts[3 * (size_t)j], X1 = pts[3 * (size_t)j + 1], X2 = pts[3 * (size_t)j + 2];
    const double r0 = cp[0], r1 = cp[1], r2 = cp[2];
    const double fx = cp[6], fy = cp[7], cx = cp[8], cy = cp[9];
    const double a = cp[10], b = cp[11], a1 = cp[12], b1 = cp[13], th2 = cp[14];
    const double c0 = r1 * X2 - r2 * X1, c1 = r2 * X0 - r0 * X2, c2 = r0 * X1 - r1 * X0;       // r x X
    const double e0 = r1 * c2 - r2 * c1, e1 = r2 * c0 - r0 * c2, e2 = r0 * c1 - r1 * c0;       // r x (r x X)
    const double Y0 = X0 + a * c0 + b * e0 + cp[3], Y1 = X1 + a * c1 + b * e1 + cp[4], Y2 = X2 + a * c2 + b * e2 + cp[5];
    const double iz = 1.0 / Y2, xn = Y0 * iz, yn = Y1 * iz;
    const double f0 = fx * xn + cx - uv[2 * k], f1 = fy * yn + cy - uv[2 * k + 1];
    double s0, s1, ft0, ft1;
    cost = 0.5 * (huber_row(f0, s0, ft0) + huber_row(f1, s1, ft1));
    // Pi = d(u,v)/d(x,y,z), already multiplied by the robust row scale
    const double p00 = s0 * fx * iz, p02 = -s0 * fx * xn * iz;
    const double p11 = s1 * fy * iz, p12 = -s1 * fy * yn * iz;
    double* my = &s_rec[tid * LDA];
    // (dR/dr_i) X = a (e_i x X) + b (r X_i + e_i (r.X) - 2 r_i X) + r_i (a1 (r x X) + b1 (r x (r x X)))
    const double rx = r0 * X0 + r1 * X1 + r2 * X2;
    const double w0 = a1 * c0 + b1 * e0, w1 = a1 * c1 + b1 * e1, w2 = a1 * c2 + b1 * e2;
    {
      const double d0 = b * (r0 * X0 + rx - 2.0 * r0 * X0) + r0 * w0;
      const double d1 = a * (-X2) + b * (r1 * X0 - 2.0 * r0 * X1) + r0 * w1;
      const double d2 = a * (X1) + b * (r2 * X0 - 2.0 * r0 * X2) + r0 * w2;
      my[0] = p00 * d0 + p02 * d2; my[D] = p11 * d1 + p12 * d2;
    }
    {
      const double d0 = a * (X2) + b * (r0 * X1 - 2.0 * r1 * X0) + r1 * w0;
      const double d1 = b * (r1 * X1 + rx - 2.0 * r1 * X1) + r1 * w1;
      const double d2 = a * (-X0) + b * (r2 * X1 - 2.0 * r1 * X2) + r1 * w2;
      my[1] = p00 * d0 + p02 * d2; my[D + 1] = p11 * d1 + p12 * d2;
    }
    {
      const double d0 = a * (-X1) + b * (r0 * X2 - 2.0 * r2 * X0) + r2 * w0;
      const double d1 = a * (X0) + b * (r1 * X2 - 2.0 * r2 * X1) + r2 * w1;
      const double d2 = b * (r2 * X2 + rx - 2.0 * r2 * X2) + r2 * w2;
      my[2] = p00 * d0 + p02 * d2; my[D + 2] = p11 * d1 + p12 * d2;
    }
    my[3] = p00; my[4] = 0.0; my[5] = p02;
    my[D + 3] = 0.0; my[D + 4] = p11; my[D + 5] = p12;
    if (D == 10) {
      my[6] = s0 * xn; my[7] = 0.0; my[8] = s0; my[9] = 0.0;
      my[D + 6] = 0.0; my[D + 7] = s1 * yn; my[D + 8] = 0.0; my[D + 9] = s1;
    }
    // R[p][q] = delta_pq + a (r x e_q)[p] + b (r_p r_q - delta_pq |r|^2);  Jp = Pi R needs rows 0, 1, 2
    const double R00 = 1.0 + b * (r0 * r0 - th2), R01 = -a * r2 + b * r0 * r1, R02 = a * r1 + b * r0 * r2;
    const double R10 = a * r2 + b * r1 * r0, R11 = 1.0 + b * (r1 * r1 - th2), R12 = -a * r0 + b * r1 * r2;
    const double R20 = -a * r1 + b * r2 * r0, R21 = a * r0 + b * r2 * r1, R22 = 1.0 + b * (r2 * r2 - th2);
    jb[0] = p00 * R00 + p02 * R20; jb[1] = p00 * R01 + p02 * R21; jb[2] = p00 * R02 + p02 * R22;
    jb[3] = p11 * R10 + p12 * R20; jb[4] = p11 * R11 + p12 * R21; jb[5] = p11 * R12 + p12 * R22;
    jb[6] = ft0; jb[7] = ft1;
  }
  double tot = block_sum256(cost, s_red);   // contains the barrier that publishes s_rec
  if (tid == 0) part[blockIdx.x] = tot;
  const int nvalid = (int)((N - k0) < 256 ? (N - k0) : 256);
  {
    T* outp = recA + (size_t)k0 * WA;
    for (int i = tid; i < nvalid * WA; i += 256) {
      const int t = i / WA, q = i - t * WA;
      outp[i] = (T)s_rec[t * LDA + q];
    }
  }
  __syncthreads();
  {
    double* my = &s_rec[tid * LDB];
#pragma unroll
    for (int q = 0; q < 8; ++q) my[q] = jb[q];
  }
  __syncthreads();
  {
    T* outp = recB + (size_t)k0 * WB;
    for (int i = tid; i < nvalid * WB; i += 256) {
      const int t = i >> 3, q = i & 7;
      outp[i] = (T)s_rec[t * LDB + q];
    }
  }
}

// per point: C_j = sum Jp~^T Jp~ (packed xx,xy,xz,yy,yz,zz), g_pj = sum Jp~^T f~ ; block partials of
// ||g_p||^2 and max|g_p|.
// (the work of workgroup `blk` of 256 points; launched as part of k_point_cam_blocks)
template <typename T>
__device__ __forceinline__ void point_blocks_wg(int blk, int P, const int* __restrict__ pt_ptr,
                                                const T* __restrict__ recB,
                                                double* __restrict__ Cp, double* __restrict__ gp,
                                                double* __restrict__ part) {
  __shared__ double s_red[4];
  const int j = blk * 256 + threadIdx.x;
  double g2 = 0.0, gm = 0.0, cm = 0.0;
  if (j < P) {
    double c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, g0 = 0, g1 = 0, g2v = 0;
    for (int k = pt_ptr[j]; k < pt_ptr[j + 1]; ++k) {       // (`#pragma unroll 5`, which pays in k_backsub: 17.5 -> 19.9 us here)
      const T* r = recB + (size_t)k * 8;
      const double a0 = r[0], a1 = r[1], a2 = r[2], b0 = r[3], b1 = r[4], b2 = r[5], f0 = r[6], f1 = r[7];
      c0 += a0 * a0 + b0 * b0; c1 += a0 * a1 + b0 * b1; c2 += a0 * a2 + b0 * b2;
      c3 += a1 * a1 + b1 * b1; c4 += a1 * a2 + b1 * b2; c5 += a2 * a2 + b2 * b2;
      g0 += a0 * f0 + b0 * f1; g1 += a1 * f0 + b1 * f1; g2v += a2 * f0 + b2 * f1;
    }
    double* co = Cp + (size_t)j * 6;
    co[0] = c0; co[1] = c1; co[2] = c2; co[3] = c3; co[4] = c4; co[5] = c5;
    gp[(size_t)j * 3] = g0; gp[(size_t)j * 3 + 1] = g1; gp[(size_t)j * 3 + 2] = g2v;
    g2 = g0 * g0 + g1 * g1 + g2v * g2v;
    gm = fmax(fabs(g0), fmax(fabs(g1), fabs(g2v)));
    cm = fmax(c0, fmax(c3, c5));
  }
  double t2 = block_sum256(g2, s_red);
  double tm = block_max256(gm, s_red);
  double tc = block_max256(cm, s_red);
  if (threadIdx.x == 0) { part[blk * 4] = t2; part[blk * 4 + 1] = tm; part[blk * 4 + 2] = tc; }
}

// per camera: B_c = sum Jc~^T Jc~ (DxD), g_c = sum Jc~^T f~ over the camera's observations.
// One workgroup per chunk of <= 256 observations of one camera: the chunk's Jc~ rows and f~ are gathered into
// LDS and contracted on the matrix cores; the chunks of a camera are added in fixed order (k_cam_blocks_final).
// (the work of the workgroup of chunk `ch`; launched as part of k_point_cam_blocks)
template <int D, typename T>
__device__ __forceinline__ void cam_blocks_chunk_wg(int ch, const int* __restrict__ cch_beg, const int* __restrict__ cch_end,
                                                    const int* __restrict__ cam_obs,
                                                    const T* __restrict__ recA,
                                                    const T* __restrict__ recB, double* __restrict__ part) {
  // [B | g] = M^T M restricted to rows < D, with M = [Jc~ | f~] (2 rows per observation, D + 1 columns): one 16x16
  // tile of v_mfma_f64_16x16x4_f64 per wavefront, K = (observation, residual row), both operands the same LDS rows.
  // Each wavefront takes a quarter of the chunk; the four partial tiles are added in fixed order.
  constexpr int W = 2 * D + 2, LDW = W + 1, NE = D * D + D;
  __shared__ double s[256 * LDW];
  __shared__ double s_tile[4][16 * 17];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int beg = cch_beg[ch], cnt = cch_end[ch] - beg;
  // gather of the chunk's rows: 16 lanes per observation, each one PAIR of values (16 bytes in float64) - the D pairs of the
  // Jc~ rows and the pair f~ - so a row arrives in one load instruction per wavefront of four observations, and the loads of
  // four trips are in flight together.  (One value per thread, 22 threads per observation: 150 us per linearisation at cfg4
  // for 176 MB - a quarter of the rate of the other passes over the records.)
  {
    typedef T pair_t __attribute__((ext_vector_type(2)));
    const int slot = tid >> 4, l16 = tid & 15;
    const bool live = l16 <= D;                              // pairs 0 .. D-1: Jc~, pair D: f~
    // all 16 trips of a full chunk in flight: first the 16 observation ids, then the 16 row pieces
    int kk[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int o = it * 16 + slot;
      kk[it] = (live && o < cnt) ? cam_obs[beg + o] : -1;
    }
    pair_t v[16];
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      v[it] = (pair_t)(T)0;
      if (kk[it] >= 0)
        v[it] = l16 < D ? *(const pair_t*)(recA + (size_t)kk[it] * (2 * D) + 2 * l16) : *(const pair_t*)(recB + (size_t)kk[it] * 8 + 6);
    }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int o = it * 16 + slot;
      if (kk[it] >= 0) { s[o * LDW + 2 * l16] = (double)v[it].x; s[o * LDW + 2 * l16 + 1] = (double)v[it].y; }
    }
  }
  __syncthreads();
  const int col = lane & 15, kq = lane >> 4;             // operand column (0..D-1: Jc~, D: f~), k slot
  const int rrow = kq & 1;                               // residual row of this k slot
  const int q = col < D ? rrow * D + col : 2 * D + rrow; // position inside an observation's staged record
  const bool live = col <= D;
  const int per = (cnt + 3) / 4;
  // (the wave's range in SGPRs - w comes from threadIdx, so the compiler kept the trip count in a VGPR and wrapped every MFMA
  // in an exec-mask save / restore - and four steps' operands read ahead of their MFMAs: one LDS wait per four, not per one)
  const int wu = __builtin_amdgcn_readfirstlane(w);
  const int o0 = wu * per, o1 = (o0 + per) < cnt ? (o0 + per) : cnt;
  v4d acc = {0.0, 0.0, 0.0, 0.0};
  for (int o = o0; o < o1; o += 8) {                     // k slots of a step: (o, row 0), (o, row 1), (o + 1, row 0), (o + 1, row 1)
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int oo = o + 2 * u + (kq >> 1);
      v[u] = (live && oo < o1) ? s[oo * LDW + q] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (o + 2 * u >= o1) break;                          // wave-uniform
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], v[u], acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) s_tile[w][(kq + 4 * i) * 17 + col] = acc[i];      // C/D: row = kq + 4 i, column = col
  __syncthreads();
  if (tid < NE) {
    const int a = tid < D * D ? tid / D : tid - D * D;
    const int b = tid < D * D ? tid - a * D : D;
    part[(size_t)ch * NE + tid] = ((s_tile[0][a * 17 + b] + s_tile[1][a * 17 + b]) + s_tile[2][a * 17 + b]) + s_tile[3][a * 17 + b];
  }
}
// The point blocks and the chunk sums of the camera blocks in ONE launch: both only read the records k_lin_obs left and neither
// reads what the other writes.  The first nblk_pt workgroups walk the tracks of 256 points each - chains of dependent loads that
// move 64 MB in the time the gather of the chunks moves 384 MB - and the chunk workgroups fill the CUs around them.  As two
// launches the track walk ran alone, at a fifth of the memory system's rate, with the chunk gather waiting behind it.
template <int D, typename T>
__global__ __launch_bounds__(256) void k_point_cam_blocks(int P, const int* __restrict__ pt_ptr, const T* __restrict__ recB,
                                                          double* __restrict__ Cp, double* __restrict__ gp,
                                                          double* __restrict__ part_pt, unsigned nblk_pt,
                                                          const int* __restrict__ cch_beg, const int* __restrict__ cch_end,
                                                          const int* __restrict__ cam_obs, const T* __restrict__ recA,
                                                          double* __restrict__ cbl_part) {
  if (blockIdx.x < nblk_pt) point_blocks_wg<T>((int)blockIdx.x, P, pt_ptr, recB, Cp, gp, part_pt);
  else cam_blocks_chunk_wg<D, T>((int)(blockIdx.x - nblk_pt), cch_beg, cch_end, cam_obs, recA, recB, cbl_part);
}
// Regulariser rows of sfm_reconstruction.py:489-499 (cam_dim 10) of one camera: residual, Jacobian w.r.t.
// (fx,fy,cx,cy), Huber scaling; adds into B_c / g_c, keeps the scaled rows for the step stage.
__device__ __forceinline__ void cam_reg_rows(const double* __restrict__ p, double fx0, double cx0, double cy0,
                                             double width, double height, double w, double* Bc, double* gcc,
                                             double* __restrict__ cost_reg, double* __restrict__ rr) {
  const double fx = p[6], fy = p[7], cx = p[8], cy = p[9];
  double f[4] = {(fx - fx0) / fx0 * w, (fy - fx) / fx * w, (cx - cx0) / width * w, (cy - cy0) / height * w};
  double J[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) J[i] = 0.0;
  J[0] = w / fx0;
  J[4] = -w * fy / (fx * fx); J[5] = w / fx;
  J[10] = w / width;
  J[15] = w / height;
  double cost = 0.0, ft[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double sc;
    cost += huber_row(f[r], sc, ft[r]);
#pragma unroll
    for (int q = 0; q < 4; ++q) J[r * 4 + q] *= sc;
  }
  *cost_reg = 0.5 * cost;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double g = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) g += J[r * 4 + i] * ft[r];
    gcc[6 + i] += g;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double hsum = 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) hsum += J[r * 4 + i] * J[r * 4 + q];
      Bc[(6 + i) * 10 + 6 + q] += hsum;
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) rr[i] = J[i];
#pragma unroll
  for (int r = 0; r < 4; ++r) rr[16 + r] = ft[r];
}

// One workgroup per camera: thread e adds the chunk partials of element e of [B_c | g_c] in chunk order (eight loads in flight,
// the additions in their order), then - cam_dim 10 with the regulariser - one thread adds the regulariser rows to the sums in
// LDS: the order of additions into B and g_c that two launches (chunk sums, then k_cam_reg) had.
template <int D>
__global__ __launch_bounds__(128) void k_cam_blocks_final(const int* __restrict__ cch_ptr, const double* __restrict__ part,
                                                          double* __restrict__ B, double* __restrict__ gc, int with_reg,
                                                          const double* __restrict__ cams, double fx0, double cx0, double cy0,
                                                          double width, double height, double w,
                                                          double* __restrict__ cost_reg, double* __restrict__ regrec) {
  constexpr int NE = D * D + D;
  static_assert(NE <= 128, "one thread per element of [B_c | g_c]");
  __shared__ double s_v[NE];
  const int c = blockIdx.x, e = threadIdx.x;
  if (e < NE) {
    double t = 0.0;
    const int ch1 = cch_ptr[c + 1];
#pragma unroll 8
    for (int ch = cch_ptr[c]; ch < ch1; ++ch) t += part[(size_t)ch * NE + e];
    s_v[e] = t;
  }
  if constexpr (D == 10) {
    if (with_reg) {
      __syncthreads();
      if (e == 0) cam_reg_rows(cams + (size_t)c * 10, fx0, cx0, cy0, width, height, w, s_v, s_v + 100, cost_reg + c, regrec + (size_t)c * 20);
    }
  }
  __syncthreads();
  if (e < D * D) B[(size_t)c * D * D + e] = s_v[e];
  else if (e < NE) gc[(size_t)c * D + (e - D * D)] = s_v[e];
}

// Fixed-order sum of block partials -> reduce_lin = [gc copy | cost | ||gp||^2 | diag(B)], gmax = [max|gp|, max diag C].
// Workgroups 0..3 each sum one column (cost, ||gp||^2, max|gp|, max diag C) with the loop and the block tree a single workgroup
// used for all four one after the other; workgroups 4.. copy gc and diag(B), one element per thread.
constexpr int LIN_FINALIZE_COLS = 4;
__global__ __launch_bounds__(256) void k_lin_finalize(int n, int D, const double* __restrict__ gc,
                                                      const double* __restrict__ B,
                                                      const double* __restrict__ part_obs, int nblk_obs,
                                                      const double* __restrict__ part_pt, int nblk_pt,
                                                      const double* __restrict__ cost_reg, int n_reg,
                                                      double* __restrict__ red_lin, double* __restrict__ gmax) {
  __shared__ double s_red[4];
  const int tid = threadIdx.x, col = blockIdx.x;
  if (col >= LIN_FINALIZE_COLS) {
    const int i = (col - LIN_FINALIZE_COLS) * 256 + tid;
    if (i < n) {
      red_lin[i] = gc[i];
      const int cam = i / D, a = i - cam * D;
      red_lin[n + 2 + i] = B[(size_t)cam * D * D + a * D + a];
    }
    return;
  }
  if (col == 0) {
    double c = 0.0;
    #pragma unroll 8
    for (int i = tid; i < nblk_obs; i += 256) c += part_obs[i];
    #pragma unroll 8
    for (int i = tid; i < n_reg; i += 256) c += cost_reg[i];
    const double ct = block_sum256(c, s_red);
    if (tid == 0) red_lin[n] = ct;
  } else if (col == 1) {
    double g2 = 0.0;
    #pragma unroll 8
    for (int i = tid; i < nblk_pt; i += 256) g2 += part_pt[4 * i];
    const double g2t = block_sum256(g2, s_red);
    if (tid == 0) red_lin[n + 1] = g2t;
  } else {
    double m = 0.0;
    #pragma unroll 8
    for (int i = tid; i < nblk_pt; i += 256) m = fmax(m, part_pt[4 * i + col - 1]);
    const double mt = block_max256(m, s_red);
    if (tid == 0) gmax[col - 2] = mt;
  }
}

__global__ __launch_bounds__(256) void k_finish_linearize(int n, const double* __restrict__ red_lin,
                                                          const double* __restrict__ gmax,
                                                          double* __restrict__ sc, double* __restrict__ hsc, double seq) {
  __shared__ double s_red[4];
  double g2 = 0.0, gm = 0.0, hm = 0.0;
  #pragma unroll 8
  for (int i = threadIdx.x; i < n; i += 256) {
    double v = red_lin[i]; g2 += v * v; gm = fmax(gm, fabs(v));
    hm = fmax(hm, red_lin[n + 2 + i]);
  }
  double g2t = block_sum256(g2, s_red);
  double gmt = block_max256(gm, s_red);
  double hmt = block_max256(hm, s_red);
  if (threadIdx.x == 0) {
    sc[SFM_SC_COST] = hsc[SFM_SC_COST] = red_lin[n];
    sc[SFM_SC_GNORM2] = hsc[SFM_SC_GNORM2] = g2t + red_lin[n + 1];
    sc[SFM_SC_GINF] = hsc[SFM_SC_GINF] = fmax(gmt, gmax[0]);
    sc[SFM_SC_HDIAG] = hsc[SFM_SC_HDIAG] = fmax(hmt, gmax[1]);
    publish_ticket(hsc, seq);
  }
}

// ------------------------------------------------------------------------------------ step + cost
// regulariser rows at x_new (cost) and their share of J~ s, f~ J~ s
__device__ __forceinline__ void reg_step_rows(const double* p /* camera row of x_new */, const double* __restrict__ s /* pc + 10 c + 6 */,
                                              double scale, const double* __restrict__ rr, double fx0, double cx0, double cy0,
                                              double width, double height, double w, int with_lin,
                                              double* __restrict__ out /* cost, js2, gts */) {
  const double fx = p[6], fy = p[7], cx = p[8], cy = p[9];
  const double f[4] = {(fx - fx0) / fx0 * w, (fy - fx) / fx * w, (cx - cx0) / width * w, (cy - cy0) / height * w};
  double cost = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) cost += huber_rho0(f[r]);
  double js2 = 0.0, gts = 0.0;
  if (with_lin) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double t = scale * (rr[r * 4] * s[0] + rr[r * 4 + 1] * s[1] + rr[r * 4 + 2] * s[2] + rr[r * 4 + 3] * s[3]);
      js2 += t * t;
      gts += rr[16 + r] * t;
    }
  }
  out[0] = 0.5 * cost;
  out[1] = js2;
  out[2] = gts;
}
__global__ void k_reg_step(int C, const double* __restrict__ cams_new, const double* __restrict__ pc,
                           double scale, const double* __restrict__ regrec, double fx0, double cx0, double cy0,
                           double width, double height, double w, int with_lin,
                           double* __restrict__ cost_reg /*[C][4]: cost, js2, gts*/) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  reg_step_rows(cams_new + (size_t)c * 10, pc + (size_t)c * 10 + 6, scale, regrec + (size_t)c * 20, fx0, cx0, cy0, width, height, w,
                with_lin, cost_reg + (size_t)c * 4);
}

// x_new = x + scale p, stated as the fused multiply-add it has always compiled to: the camera workgroups below form the same
// rows a second time and must get the same bits.
__device__ __forceinline__ double axpy_val(double x, double scale, double p) { return fma(scale, p, x); }
// Workgroups 0 .. nblk_x - 1: x_new and the block partials of ||s||^2, ||x_new||^2 over the points.  Workgroups nblk_x ..: one
// thread per camera - the camera's row of x_new once more, in registers, and from it what k_campre (first cdiv(C, 256)
// workgroups) and k_reg_step (as many again, if the regulariser applies) would make of the stored row (campre2, cost_reg):
// two launches, each waiting for this one, that the trial step no longer has.
template <int D>
__global__ __launch_bounds__(256) void k_axpy_step(int64_t n_c, int64_t n_total, const double* __restrict__ x,
                                                   const double* __restrict__ pc, const double* __restrict__ pp,
                                                   double scale, double* __restrict__ x_new,
                                                   double* __restrict__ part, unsigned nblk_x, int C, double fx0, double fy0,
                                                   double cx0, double cy0, double* __restrict__ campre2,
                                                   const double* __restrict__ regrec, double width, double height, double w,
                                                   double* __restrict__ cost_reg) {
  if (blockIdx.x >= nblk_x) {
    const unsigned nblk_c = (unsigned)(C + 255) / 256, b = blockIdx.x - nblk_x;      // campre workgroups, then regulariser workgroups
    const int c = (int)(b < nblk_c ? b : b - nblk_c) * 256 + (int)threadIdx.x;
    if (c >= C) return;
    double p[D];
#pragma unroll
    for (int i = 0; i < D; ++i) p[i] = axpy_val(x[(size_t)c * D + i], scale, pc[(size_t)c * D + i]);
    if (b < nblk_c) campre_row<D>(p, fx0, fy0, cx0, cy0, campre2 + (size_t)c * CAMPRE);
    else if constexpr (D == 10)
      reg_step_rows(p, pc + (size_t)c * 10 + 6, scale, regrec + (size_t)c * 20, fx0, cx0, cy0, width, height, w, 1, cost_reg + (size_t)c * 4);
    return;
  }
  __shared__ double s_red[4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double s2 = 0.0, x2 = 0.0;
  if (i < n_total) {
    const bool is_cam = i < n_c;
    const double pv = is_cam ? pc[i] : pp[i - n_c];
    const double s = scale * pv;
    const double xn = axpy_val(x[i], scale, pv);
    x_new[i] = xn;
    if (!is_cam) { s2 = s * s; x2 = xn * xn; }
  }
  double a = block_sum256(s2, s_red);
  double b = block_sum256(x2, s_red);
  if (threadIdx.x == 0) { part[blockIdx.x * 2] = a; part[blockIdx.x * 2 + 1] = b; }
}

// Trial step, one pass over the observations: (J~ s) for both rows -> block partials of (J~ s)^2 and f~ (J~ s), and the Huber
// cost at x_new.  256 observations per workgroup.  The two record arrays come in as in k_build_G - flat, coalesced 16-byte
// loads, transposed through LDS (odd row strides) - but one after the other through the same buffer, as in k_lin_obs: 51 KB
// and three workgroups per CU instead of 69 KB and two.  (One thread per (observation, row) with 8-byte loads 80 bytes apart
// moved the same 224 MB at 4.4 TB/s, and the cost was a second pass.)
// The partial sums keep the grouping and the trees they had as two kernels:
//   part[4 b' + 0/1], b' = 2 b, 2 b + 1: sums over the 256 (observation, row) lanes of 128 observations - t^2 and f~ t go to
//     LDS in that lane order, lane i then holds (observation i / 2, row i % 2) of its half;
//   part[4 b + 2]: the cost of the 256 observations, thread i holding observation i (the statements of k_cost_obs).
// The five sums are block_sum256's - wave_sum, then the four waves' totals added in order by thread 0 - behind ONE pair of
// barriers instead of five: a workgroup that spends its last microsecond in ten barriers keeps a third of a CU's loads waiting.
template <int D, typename T>
__global__ __launch_bounds__(256) void k_step_cost_obs(int64_t N, const int* __restrict__ cam_idx,
                                                       const int* __restrict__ pt_idx, const double* __restrict__ uv,
                                                       const T* __restrict__ recA, const T* __restrict__ recB,
                                                       const double* __restrict__ pc, const double* __restrict__ pp,
                                                       double scale, const double* __restrict__ pts_new,
                                                       const double* __restrict__ campre2, double* __restrict__ part) {
  constexpr int WA = 2 * D, LDA = WA + 1, LDB = 9;
  constexpr int VE = 16 / (int)sizeof(T);                // elements per 16-byte load
  constexpr int NA = WA / VE, NB = 8 / VE;               // 16-byte loads per thread for the two record arrays of 256 observations
  static_assert(WA % VE == 0 && 8 % VE == 0, "record rows are whole 16-byte pieces");
  __shared__ double s_buf[256 * LDA];                     // recB records (stride 9) first, then recA records (stride LDA)
  __shared__ double s_j2[512], s_gt[512];
  __shared__ double s_red[5][4];
  typedef T vec_t __attribute__((ext_vector_type(VE)));
  const int tid = threadIdx.x;
  const int64_t k0 = (int64_t)blockIdx.x * 256;
  const int nvalid = (int)((N - k0) < 256 ? (N - k0) : 256);
  const bool live = tid < nvalid;
  const int64_t k = k0 + tid;
  // every global load is issued before anything waits: the two ids (the gathers depend on them), the flat pieces of the
  // records, the observation's uv, then the gathers
  const size_t cam = live ? cam_idx[k] : 0, pj = live ? pt_idx[k] : 0;
  vec_t la[NA], lb[NB];
  {
    const vec_t* inA = (const vec_t*)(recA + (size_t)k0 * WA);
    const vec_t* inB = (const vec_t*)(recB + (size_t)k0 * 8);
#pragma unroll
    for (int j = 0; j < NB; ++j) { const int i = tid + 256 * j; lb[j] = i * VE < nvalid * 8 ? inB[i] : (vec_t)(T)0; }
#pragma unroll
    for (int j = 0; j < NA; ++j) { const int i = tid + 256 * j; la[j] = i * VE < nvalid * WA ? inA[i] : (vec_t)(T)0; }
  }
  const double u0 = live ? uv[2 * k] : 0.0, u1 = live ? uv[2 * k + 1] : 0.0;
  double c[D], q[3], cp[CAMPRE - 1], X[3];
#pragma unroll
  for (int a = 0; a < D; ++a) c[a] = pc[cam * D + a];
#pragma unroll
  for (int a = 0; a < 3; ++a) q[a] = pp[pj * 3 + a];
#pragma unroll
  for (int a = 0; a < CAMPRE - 1; ++a) cp[a] = campre2[cam * CAMPRE + a];
#pragma unroll
  for (int a = 0; a < 3; ++a) X[a] = pts_new[pj * 3 + a];
#pragma unroll
  for (int j = 0; j < NB; ++j)
#pragma unroll
    for (int v = 0; v < VE; ++v) { const int i = (tid + 256 * j) * VE + v; s_buf[(i >> 3) * LDB + (i & 7)] = (double)lb[j][v]; }
  __syncthreads();
  double jb[8];                                           // Jp~ rows and f~ of this thread's observation
#pragma unroll
  for (int e = 0; e < 8; ++e) jb[e] = s_buf[tid * LDB + e];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NA; ++j)
#pragma unroll
    for (int v = 0; v < VE; ++v) { const int i = (tid + 256 * j) * VE + v, t = i / WA, e = i - t * WA; s_buf[t * LDA + e] = (double)la[j][v]; }
  __syncthreads();
  double cost = 0.0;
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    double t = 0.0, fr = 0.0;
    if (live) {
      const double* jc = &s_buf[tid * LDA + row * D];
      const double* jp = &jb[row * 3];
      t = jp[0] * q[0] + jp[1] * q[1] + jp[2] * q[2];
#pragma unroll
      for (int a = 0; a < D; ++a) t += jc[a] * c[a];
      t *= scale;
      fr = jb[6 + row];
    }
    // the products, not t and f~: summed from LDS their first addition is an addition (t * t next to it would be fused into it)
    s_j2[2 * tid + row] = t * t;
    s_gt[2 * tid + row] = fr * t;
  }
  if (live) {
    double Y0, Y1, Y2;
    cam_project(cp, X[0], X[1], X[2], Y0, Y1, Y2);
    const double iz = 1.0 / Y2;
    const double f0 = cp[6] * (Y0 * iz) + cp[8] - u0;
    const double f1 = cp[7] * (Y1 * iz) + cp[9] - u1;
    cost = 0.5 * (huber_rho0(f0) + huber_rho0(f1));
  }
  __syncthreads();                                        // s_j2 / s_gt are whole
  double w[5] = {s_j2[tid], s_gt[tid], cost, s_j2[256 + tid], s_gt[256 + tid]};
#pragma unroll
  for (int e = 0; e < 5; ++e) w[e] = wave_sum(w[e]);
  if ((tid & 63) == 0)
#pragma unroll
    for (int e = 0; e < 5; ++e) s_red[e][tid >> 6] = w[e];
  __syncthreads();
  if (tid == 0) {
    double tot[5];
#pragma unroll
    for (int e = 0; e < 5; ++e) tot[e] = s_red[e][0] + s_red[e][1] + s_red[e][2] + s_red[e][3];
    const size_t b = blockIdx.x;
    part[8 * b] = tot[0]; part[8 * b + 1] = tot[1];
    part[4 * b + 2] = tot[2];
    if (nvalid > 128) { part[8 * b + 4] = tot[3]; part[8 * b + 5] = tot[4]; }     // (the last workgroup may have no second block of 256 rows)
  }
}

// Huber cost of the reprojection rows at the parameters behind `campre` / `pts`.
__global__ __launch_bounds__(256) void k_cost_obs(int64_t N, const int* __restrict__ cam_idx,
                                                  const int* __restrict__ pt_idx,
                                                  const double* __restrict__ uv, const double* __restrict__ pts,
                                                  const double* __restrict__ campre,
                                                  double* __restrict__ part, int part_stride, int part_col,
                                                  double* __restrict__ err_out) {
  __shared__ double s_red[4];
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double cost = 0.0;
  if (k < N) {
    const double* cp = campre + (size_t)cam_idx[k] * CAMPRE;
    const size_t j = (size_t)pt_idx[k] * 3;
    const double X0 = pts[j], X1 = pts[j + 1], X2 = pts[j + 2];
    double Y0, Y1, Y2;
    cam_project(cp, X0, X1, X2, Y0, Y1, Y2);
    const double iz = 1.0 / Y2;
    const double f0 = cp[6] * (Y0 * iz) + cp[8] - uv[2 * k];
    const double f1 = cp[7] * (Y1 * iz) + cp[9] - uv[2 * k + 1];
    cost = 0.5 * (huber_rho0(f0) + huber_rho0(f1));
    if (err_out) err_out[k] = sqrt(f0 * f0 + f1 * f1);
  }
  double t = block_sum256(cost, s_red);
  if (threadIdx.x == 0 && part) part[(size_t)blockIdx.x * part_stride + part_col] = t;
}

// red_step = [ js2, gts, cost_new, s_pts2, xnew_pts2 ] (this rank's partial sums, fixed order).
// The single-workgroup sums of this kernel and of k_lin_finalize / k_finish_step / k_finish_linearize walk ~4,000 block partials,
// 16 per thread: with a run-time trip count the loop waited for every load before issuing the next (12-14 us per kernel);
// `#pragma unroll 8` lets eight loads be in flight while the additions keep their order (the same bits).
// One workgroup per column q of red_step (grid 5): the column's loops in their order, then its block tree.
__global__ __launch_bounds__(256) void k_step_finalize(const double* __restrict__ part_obs, int nblk_obs,
                                                       int nblk_rows, const double* __restrict__ part_x, int nblk_x,
                                                       const double* __restrict__ cost_reg, int n_reg,
                                                       int with_lin, double* __restrict__ red_step) {
  __shared__ double s_red[4];
  const int q = blockIdx.x;
  double v = 0.0;
  if (q == 2) {
    #pragma unroll 8
    for (int i = threadIdx.x; i < nblk_obs; i += 256) v += part_obs[(size_t)i * 4 + 2];
    #pragma unroll 8
    for (int i = threadIdx.x; i < n_reg; i += 256) v += cost_reg[(size_t)i * 4];
  } else if (q < 2) {
    if (with_lin)
      #pragma unroll 8
      for (int i = threadIdx.x; i < nblk_rows; i += 256) v += part_obs[(size_t)i * 4 + q];
    #pragma unroll 8
    for (int i = threadIdx.x; i < n_reg; i += 256) v += cost_reg[(size_t)i * 4 + 1 + q];
  } else if (with_lin) {
    #pragma unroll 8
    for (int i = threadIdx.x; i < nblk_x; i += 256) v += part_x[(size_t)i * 2 + (q - 3)];
  }
  const double t = block_sum256(v, s_red);
  if (threadIdx.x == 0) red_step[q] = t;
}

__global__ __launch_bounds__(256) void k_finish_step(int n_c, const double* __restrict__ pc, double scale,
                                                     const double* __restrict__ x_new,
                                                     const double* __restrict__ red_step,
                                                     double* __restrict__ sc, double* __restrict__ hsc, double seq) {
  __shared__ double s_red[4];
  double s2 = 0.0, x2 = 0.0;
  #pragma unroll 8
  for (int i = threadIdx.x; i < n_c; i += 256) {
    const double s = scale * pc[i];
    s2 += s * s;
    x2 += x_new[i] * x_new[i];
  }
  double a = block_sum256(s2, s_red);
  double b = block_sum256(x2, s_red);
  if (threadIdx.x == 0) {
    sc[SFM_SC_JS2] = hsc[SFM_SC_JS2] = red_step[0]; sc[SFM_SC_GTS] = hsc[SFM_SC_GTS] = red_step[1];
    sc[SFM_SC_COST_NEW] = hsc[SFM_SC_COST_NEW] = red_step[2];
    sc[SFM_SC_SNORM2] = hsc[SFM_SC_SNORM2] = a + red_step[3]; sc[SFM_SC_XNEW_NORM2] = hsc[SFM_SC_XNEW_NORM2] = b + red_step[4];
    publish_ticket(hsc, seq);
  }
}

__global__ void k_set_intrinsics(int C, double fx, double fy, double cx, double cy, double* __restrict__ cp) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double* o = cp + (size_t)c * CAMPRE;
  o[6] = fx; o[7] = fy; o[8] = cx; o[9] = cy;
}

// The reprojection of x = [cams | pts]: k_campre into `campre` ((fx, fy, cx, cy): the intrinsics of cameras that carry none),
// k_set_intrinsics when every camera is to project with these (shared_k), then k_cost_obs (grid cdiv(N, 256) = Lay::nblk_obs) -> part, err_out.
static void launch_projection(sfm_ctx* h, int C, int D, int64_t N, const int* cam_idx, const int* pt_idx, const double* uv,
                              const double* x, double fx, double fy, double cx, double cy, int shared_k, double* campre,
                              double* part, int part_stride, int part_col, double* err_out) {
  DISPATCH_D(D, hipLaunchKernelGGL(k_campre<DD>, dim3(cdiv(C, 64)), dim3(64), 0, h->stream, x, C, fx, fy, cx, cy, campre));
  if (shared_k) hipLaunchKernelGGL(k_set_intrinsics, dim3(cdiv(C, 64)), dim3(64), 0, h->stream, C, fx, fy, cx, cy, campre);
  hipLaunchKernelGGL(k_cost_obs, dim3(cdiv(N, 256)), dim3(256), 0, h->stream, N, cam_idx, pt_idx, uv, x + (size_t)C * D, campre,
                     part, part_stride, part_col, err_out);
}

static int launch_cost(sfm_ctx* h, sfm_ba_problem p, const Lay& L, double* ws, const double* x,
                       const double* pc_for_reg, double scale, int with_lin, double* err_out) {
  const int C = p->n_cams;
  launch_projection(h, p->n_cams, p->cam_dim, p->n_obs, p->cam_idx, p->pt_idx, p->uv, x, p->fx0, p->fy0, p->cx0, p->cy0, 0, WS(L, campre2),
                    WS(L, part_obs), 4, 2, err_out);
  if (p->cam_dim == 10 && p->apply_reg)
    hipLaunchKernelGGL(k_reg_step, dim3(cdiv(C, 64)), dim3(64), 0, h->stream, C, x, pc_for_reg, scale, WS(L, regrec), p->fx0, p->cx0,
                       p->cy0, p->width, p->height, p->reg_weight, with_lin, WS(L, cost_reg));
  SFM_LAUNCH_CHECK(h, "launch_cost");
  return SFM_OK;
}

extern "C" int sfm_ba_cost(sfm_handle h, sfm_ba_problem p, const double* x) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  double* ws = (double*)p->workspace;
  rc = launch_cost(h, p, L, ws, x, nullptr, 0.0, 0, nullptr); if (rc) return rc;
  const int nreg = (p->cam_dim == 10 && p->apply_reg) ? p->n_cams : 0;
  hipLaunchKernelGGL(k_step_finalize, dim3(5), dim3(256), 0, h->stream, WS(L, part_obs), (int)L.nblk_obs, 0,
                     (const double*)nullptr, 0, WS(L, cost_reg), nreg, 0, WS(L, red_step));
  SFM_LAUNCH_CHECK(h, "sfm_ba_cost");
  return SFM_OK;
}

// (shared_k: compute_reconstruction_stats projects with the ONE shared self.K, sfm_reconstruction.py:601)
extern "C" int sfm_ba_reproj_errors(sfm_handle h, sfm_ba_problem p, const double* x, int shared_k,
                                    double* err_out) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  if (!err_out) return sfm_fail(h, SFM_ERR_ARG, "sfm_ba_reproj_errors", "null output");
  launch_projection(h, p->n_cams, p->cam_dim, p->n_obs, p->cam_idx, p->pt_idx, p->uv, x, p->fx0, p->fy0, p->cx0, p->cy0, shared_k,
                    (double*)p->workspace + L.campre2, nullptr, 0, 0, err_out);
  SFM_LAUNCH_CHECK(h, "sfm_ba_reproj_errors");
  return SFM_OK;
}

// block partials of ||v||^2 (the residual norm below; ||x||^2 for the trust-region loop's initial radius, Delta_0 = ||x_0||, scipy trf.py:422-430)
__global__ __launch_bounds__(256) void k_sq_partials(int64_t n, const double* __restrict__ v, double* __restrict__ part) {
  __shared__ double s_red[4];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double t = i < n ? v[i] * v[i] : 0.0;
  const double a = block_sum256(t, s_red);
  if (threadIdx.x == 0) part[blockIdx.x] = a;
}
// sum over this problem's observations of ||proj - uv||^2 at x, to the host: what bundle_adjust logs before and after the
// solve (sfm_reconstruction.py:522-524 prints ||objective(x)||_2).  In the library so that the drop-in's write-back needs no
// torch kernel: on a fresh box the first use of a torch elementwise / reduction kernel pages its code object in from disk,
// ~0.1 s of the 0.15 s the round-2 driver run saw in `log_norms_and_write_back`.
extern "C" int sfm_ba_residual_norm2(sfm_handle h, sfm_ba_problem p, const double* x, int shared_k, double* out_host) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  if (!x || !out_host) return sfm_fail(h, SFM_ERR_ARG, "sfm_ba_residual_norm2", "null argument");
  double* ws = (double*)p->workspace;
  launch_projection(h, p->n_cams, p->cam_dim, p->n_obs, p->cam_idx, p->pt_idx, p->uv, x, p->fx0, p->fy0, p->cx0, p->cy0, shared_k, WS(L, campre2),
                    nullptr, 0, 0, WS(L, tmp3));
  hipLaunchKernelGGL(k_sq_partials, dim3((unsigned)L.nblk_obs), dim3(256), 0, h->stream, p->n_obs, WS(L, tmp3), WS(L, part_obs));
  ba_sum_partials(h, WS(L, part_obs), (int)L.nblk_obs, 1, WS(L, red_step) + 6);
  SFM_HIP(h, hipMemcpyAsync(h->pinned + 48, WS(L, red_step) + 6, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  SFM_HIP(h, hipStreamSynchronize(h->stream));
  SFM_LAUNCH_CHECK(h, "sfm_ba_residual_norm2");
  *out_host = h->pinned[48];
  return SFM_OK;
}

extern "C" int sfm_reproj_errors(sfm_handle h, int32_t n_cams, int32_t cam_dim, int64_t n_obs, const int32_t* cam_idx,
                                 const int32_t* pt_idx, const double* uv, const double* x, double fx, double fy, double cx,
                                 double cy, int shared_k, double* err_out) {
  if (!h) return SFM_ERR_ARG;
  if (n_cams < 1 || n_obs < 1 || (cam_dim != 6 && cam_dim != 10) || !cam_idx || !pt_idx || !uv || !x || !err_out)
    return sfm_fail(h, SFM_ERR_ARG, "sfm_reproj_errors", "bad argument");
  double* campre = (double*)sfm_scratch(h, (size_t)n_cams * CAMPRE * sizeof(double));
  if (!campre) return sfm_fail(h, SFM_ERR_HIP, "sfm_reproj_errors", "scratch allocation failed");
  launch_projection(h, n_cams, cam_dim, n_obs, cam_idx, pt_idx, uv, x, fx, fy, cx, cy, shared_k, campre, nullptr, 0, 0, err_out);
  SFM_LAUNCH_CHECK(h, "sfm_reproj_errors");
  return SFM_OK;
}

extern "C" int sfm_ba_linearize(sfm_handle h, sfm_ba_problem p, const double* x) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  double* ws = (double*)p->workspace;
  const int C = p->n_cams, P = p->n_pts, D = p->cam_dim, n = C * D;
  const int64_t N = p->n_obs;
  const double* pts = x + (size_t)n;
  const int nreg = (D == 10 && p->apply_reg) ? C : 0;
  p->cgp.fail_rel *= 0.8;                             // a new linearisation: what was hopeless for the camera CG may not be here, let it try lower again
  DISPATCH_DT(D, p->precision, {
    hipLaunchKernelGGL(k_campre<DD>, dim3(cdiv(C, 64)), dim3(64), 0, h->stream, x, C, p->fx0, p->fy0, p->cx0,
                       p->cy0, WS(L, campre));
    sfm_prof_begin(h, SFM_PROF_LIN_OBS);
    hipLaunchKernelGGL((k_lin_obs<DD, TT>), dim3((unsigned)L.nblk_obs), dim3(256), 0, h->stream, N, p->cam_idx,
                       p->pt_idx, p->uv, pts, WS(L, campre), WST(L, recA), WST(L, recB), WS(L, part_obs));
    sfm_prof_end(h, SFM_PROF_LIN_OBS);
    sfm_prof_begin(h, SFM_PROF_LIN_REST);
    hipLaunchKernelGGL((k_point_cam_blocks<DD, TT>), dim3((unsigned)L.nblk_pt + (unsigned)p->n_cchunks), dim3(256), 0, h->stream, P,
                       p->pt_ptr, WST(L, recB), WS(L, Cp), WS(L, gp), WS(L, part_pt), (unsigned)L.nblk_pt, p->cch_beg, p->cch_end,
                       p->cam_obs, WST(L, recA), WS(L, cbl_part));
    hipLaunchKernelGGL(k_cam_blocks_final<DD>, dim3(C), dim3(128), 0, h->stream, p->cch_ptr, WS(L, cbl_part), WS(L, B), WS(L, gc),
                       nreg > 0, x, p->fx0, p->cx0, p->cy0, p->width, p->height, p->reg_weight, WS(L, cost_reg), WS(L, regrec));
  });
  // cost_reg is [C][4] in the step stage and [C] here: use stride 1 in both by writing column 0 only
  hipLaunchKernelGGL(k_lin_finalize, dim3(LIN_FINALIZE_COLS + cdiv(n, 256)), dim3(256), 0, h->stream, n, D, WS(L, gc), WS(L, B), WS(L, part_obs),
                     (int)L.nblk_obs, WS(L, part_pt), (int)L.nblk_pt, WS(L, cost_reg), nreg, WS(L, red_lin),
                     WS(L, gmax));
  sfm_prof_end(h, SFM_PROF_LIN_REST);
  SFM_LAUNCH_CHECK(h, "sfm_ba_linearize");
  return SFM_OK;
}
extern "C" int sfm_ba_finish_linearize(sfm_handle h, sfm_ba_problem p) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  double* ws = (double*)p->workspace;
  hipLaunchKernelGGL(k_finish_linearize, dim3(1), dim3(256), 0, h->stream, p->n_cams * p->cam_dim,
                     WS(L, red_lin), WS(L, gmax), WS(L, scalars), p->host_sc, next_ticket(p));
  SFM_LAUNCH_CHECK(h, "sfm_ba_finish_linearize");
  return SFM_OK;
}

extern "C" int sfm_ba_step(sfm_handle h, sfm_ba_problem p, const double* x, double scale, double* x_new) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  double* ws = (double*)p->workspace;
  const int C = p->n_cams, P = p->n_pts, D = p->cam_dim, n = C * D;
  const int64_t N = p->n_obs, ntot = (int64_t)n + 3 * (int64_t)P;
  double* part_x = WS(L, part_x);
  sfm_prof_begin(h, SFM_PROF_STEP);
  const unsigned nblk_x = cdiv(ntot, 256), nblk_rows = cdiv(2 * N, 256);
  const int nreg = (D == 10 && p->apply_reg) ? C : 0;
  // x_new, and in the same launch campre2 / cost_reg at x_new (per camera); one pass over the observations; the five sums
  DISPATCH_D(D, hipLaunchKernelGGL(k_axpy_step<DD>, dim3(nblk_x + cdiv(C, 256) * (nreg > 0 ? 2 : 1)), dim3(256), 0, h->stream, (int64_t)n, ntot, x, WS(L, pc),
                                   WS(L, pp), scale, x_new, part_x, nblk_x, C, p->fx0, p->fy0, p->cx0, p->cy0, WS(L, campre2),
                                   WS(L, regrec), p->width, p->height, p->reg_weight, WS(L, cost_reg)));
  DISPATCH_DT(D, p->precision, hipLaunchKernelGGL((k_step_cost_obs<DD, TT>), dim3((unsigned)L.nblk_obs), dim3(256), 0, h->stream, N,
                                                  p->cam_idx, p->pt_idx, p->uv, WST(L, recA), WST(L, recB), WS(L, pc), WS(L, pp), scale,
                                                  x_new + (size_t)n, WS(L, campre2), WS(L, part_obs)));
  hipLaunchKernelGGL(k_step_finalize, dim3(5), dim3(256), 0, h->stream, WS(L, part_obs), (int)L.nblk_obs,
                     (int)nblk_rows, part_x, (int)nblk_x, WS(L, cost_reg), nreg, 1, WS(L, red_step));
  sfm_prof_end(h, SFM_PROF_STEP);
  SFM_LAUNCH_CHECK(h, "sfm_ba_step");
  return SFM_OK;
}

extern "C" int sfm_ba_finish_step(sfm_handle h, sfm_ba_problem p, const double* x, double scale,
                                  const double* x_new) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  double* ws = (double*)p->workspace;
  (void)x;
  hipLaunchKernelGGL(k_finish_step, dim3(1), dim3(256), 0, h->stream, p->n_cams * p->cam_dim, WS(L, pc), scale,
                     x_new, WS(L, red_step), WS(L, scalars), p->host_sc, next_ticket(p));
  SFM_LAUNCH_CHECK(h, "sfm_ba_finish_step");
  return SFM_OK;
}

__global__ __launch_bounds__(256) void k_xnorm_finish(int n_c, const double* __restrict__ x, const double* __restrict__ red_step,
                                                      double* __restrict__ sc, double* __restrict__ hsc, double seq) {
  __shared__ double s_red[4];
  double a = 0.0;
  for (int i = threadIdx.x; i < n_c; i += 256) a += x[i] * x[i];
  const double t = block_sum256(a, s_red);
  if (threadIdx.x == 0) { sc[SFM_SC_XNEW_NORM2] = hsc[SFM_SC_XNEW_NORM2] = t + red_step[4]; publish_ticket(hsc, seq); }
}
int ba_xnorm_partial(sfm_ctx* h, sfm_ba_problem p, const double* x) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  double* ws = (double*)p->workspace;
  const int64_t n = (int64_t)p->n_cams * p->cam_dim, np3 = 3 * (int64_t)p->n_pts;
  const unsigned nb = cdiv(np3, 256);       // part_x holds ((n + 3P + 255) / 256) * 2 + 2 doubles: enough
  hipLaunchKernelGGL(k_sq_partials, dim3(nb), dim3(256), 0, h->stream, np3, x + n, WS(L, part_x));
  ba_sum_partials(h, WS(L, part_x), (int)nb, 1, WS(L, red_step) + 4);
  SFM_LAUNCH_CHECK(h, "ba_xnorm_partial");
  return SFM_OK;
}
int ba_xnorm_finish(sfm_ctx* h, sfm_ba_problem p, const double* x) {
  Lay L; int rc = check_problem(h, p, &L); if (rc) return rc;
  double* ws = (double*)p->workspace;
  hipLaunchKernelGGL(k_xnorm_finish, dim3(1), dim3(256), 0, h->stream, p->n_cams * p->cam_dim, x, WS(L, red_step), WS(L, scalars), p->host_sc, next_ticket(p));
  SFM_LAUNCH_CHECK(h, "ba_xnorm_finish");
  return SFM_OK;
}
