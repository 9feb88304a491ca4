// The rule of the render score (render_score.hip), written so that it also compiles for the host
// (tests/native/render_score_check.cpp) and so that NumPy reproduces it operation for operation
// (tests/render_score_reference.py).  include/sfm_amd.h states the whole stage; this header holds its arithmetic: integers,
// and float64 without FMA contraction for the SSIM quotient and the depth ratio.  Every statistic is an integer sum, so
// no order of summation exists.
//
// A staged pixel is one 32-bit word per image: the channels in bytes 0 .. 2 (a gray image uses byte 0), and for the render
// the flags in byte 3 - bit 0 compared (covered and, with a mask, mask > 0), bit 1 covered (triangle >= 0).
//   ssim_channel():  a = 2 Sx Sy, b = Sx Sx + Sy Sy, cv = 2 (n Sxy - Sx Sy), vr = (n Sxx - Sx Sx) + (n Syy - Sy Sy) in int64,
//                    c1 = (double)(n n) * 6.5025, c2 = (double)(n n) * 58.5225,
//                    s = (((double)a + c1) * ((double)cv + c2)) / (((double)b + c1) * ((double)vr + c2))
//   window_ssim():   the five sums per channel over W x W staged pixels and the number of compared ones among them; a window
//                    iff that number is W W; s = s_0 or ((s_0 + s_1) + s_2) / 3.0
//   quantise():      (int64)floor(v * 16777216.0 + 0.5)
//   seen():          keep != 0 and the view's depth finite
//   depth_term():    r = |(double)dr - (double)dv|; a NaN r agrees with nothing and adds 0; otherwise agree = r <= rel_tol dv
//                    and the ratio is min(r / dv, 1.0) for dv > 0; for dv <= 0, where r / dv is no relative error, the ratio
//                    is 0.0 when r == 0 and 1.0 otherwise (so such a pixel agrees only when dr == dv == 0)
// The sums of a window fit 32 bits (n <= 121: Sx <= 30,855, Sxx <= 7,868,025); the products are taken in int64.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RENDER_SCORE_HD __host__ __device__ __forceinline__
#else
#define RENDER_SCORE_HD inline
#endif

#pragma clang fp contract(off)

#define RENDER_SCORE_NAN_BITS 0x7FC00000u
#define RENDER_SCORE_COMPARED 1
#define RENDER_SCORE_COVERED 2
#define RENDER_SCORE_COLUMNS 16
// the columns of the statistics table
#define RS_N_PIXELS 0
#define RS_N_COMPARED 1
#define RS_SAD 2
#define RS_SSE 5
#define RS_N_SSIM 8
#define RS_Q_SSIM 9
#define RS_N_BOTH 10
#define RS_N_AGREE 11
#define RS_Q_REL 12
#define RS_N_RENDER_ONLY 13
#define RS_N_VIEW_ONLY 14

namespace render_score {

RENDER_SCORE_HD uint32_t pack(int c0, int c1, int c2, int flags) {
  return (uint32_t)c0 | ((uint32_t)c1 << 8) | ((uint32_t)c2 << 16) | ((uint32_t)flags << 24);
}
RENDER_SCORE_HD int channel(uint32_t p, int k) { return (int)((p >> (8 * k)) & 255u); }
RENDER_SCORE_HD int flags(uint32_t p) { return (int)(p >> 24); }

RENDER_SCORE_HD double ssim_channel(int64_t n, int64_t Sx, int64_t Sy, int64_t Sxx, int64_t Syy, int64_t Sxy) {
  const int64_t a = 2 * Sx * Sy;
  const int64_t b = Sx * Sx + Sy * Sy;
  const int64_t cv = 2 * (n * Sxy - Sx * Sy);
  const int64_t vr = (n * Sxx - Sx * Sx) + (n * Syy - Sy * Sy);
  const double c1 = (double)(n * n) * 6.5025;
  const double c2 = (double)(n * n) * 58.5225;
  return (((double)a + c1) * ((double)cv + c2)) / (((double)b + c1) * ((double)vr + c2));
}

RENDER_SCORE_HD int64_t quantise(double v) { return (int64_t)floor(v * 16777216.0 + 0.5); }

// the window whose first staged pixel is sr[at] / sp[at], rows `stride` words apart: 1 and *s when all W W pixels are compared
template <int CH, int W>
RENDER_SCORE_HD int window_ssim(const uint32_t* sr, const uint32_t* sp, int stride, int at, double* s) {
  int32_t sx[CH], sy[CH], sxx[CH], syy[CH], sxy[CH];
  for (int k = 0; k < CH; ++k) { sx[k] = 0; sy[k] = 0; sxx[k] = 0; syy[k] = 0; sxy[k] = 0; }
  int full = 0;
  for (int dy = 0; dy < W; ++dy) {
    for (int dx = 0; dx < W; ++dx) {
      const uint32_t r = sr[at + dy * stride + dx], p = sp[at + dy * stride + dx];
      full += flags(r) & RENDER_SCORE_COMPARED;
      for (int k = 0; k < CH; ++k) {
        const int32_t x = channel(r, k), y = channel(p, k);
        sx[k] += x; sy[k] += y; sxx[k] += x * x; syy[k] += y * y; sxy[k] += x * y;
      }
    }
  }
  if (full != W * W) return 0;
  double v[CH];
  for (int k = 0; k < CH; ++k) v[k] = ssim_channel(W * W, sx[k], sy[k], sxx[k], syy[k], sxy[k]);
  *s = CH == 1 ? v[0] : ((v[0] + v[CH > 1 ? 1 : 0]) + v[CH > 2 ? 2 : 0]) / 3.0;
  return 1;
}

RENDER_SCORE_HD int seen(int keep, float dv) {
  const double d = (double)dv;
  return keep != 0 && (d - d == 0.0);
}

RENDER_SCORE_HD void depth_term(float dr, float dv, double rel_tol, int* agree, int64_t* q) {
  const double v = (double)dv;
  const double r = fabs((double)dr - v);
  if (!(r == r)) { *agree = 0; *q = 0; return; }
  *agree = r <= rel_tol * v ? 1 : 0;
  double t;
  if (v > 0.0) {
    t = r / v;
    t = t < 1.0 ? t : 1.0;
  } else {
    t = r == 0.0 ? 0.0 : 1.0;
  }
  *q = quantise(t);
}

}  // namespace render_score
