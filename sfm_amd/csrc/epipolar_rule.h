// The error rule of twoview.hip (fundamental matrix) and essential.hip (essential matrix) with its whole-segment count,
// so that both count an inlier alike, bit for bit, and the staging of a segment's matches for the scoring loops of those
// two and of homography.hip.  Included by .hip files only; the rule itself is in fundamental_rule.h, which the host
// compiles too.
#pragma once
#include "ransac_kernels.h"
#include "fundamental_rule.h"

constexpr int FUND_CHUNK = 512;      // points per LDS stage of the scoring loop: 512 x 4 doubles = 16 KiB

// stage points [c0, c0 + cnt) of a segment into LDS as doubles; a non-finite match becomes NaN in all four
__device__ __forceinline__ void stage_points(double2* s_pt, const float2* __restrict__ pts1, const float2* __restrict__ pts2,
                                             int64_t base, int cnt, int nthreads) {
  for (int t = threadIdx.x; t < cnt; t += nthreads) {
    const float2 p = pts1[base + t], q = pts2[base + t];
    const bool ok = finite4(p, q);
    const double nan = __builtin_nan("");
    s_pt[2 * t] = ok ? make_double2((double)p.x, (double)p.y) : make_double2(nan, nan);
    s_pt[2 * t + 1] = ok ? make_double2((double)q.x, (double)q.y) : make_double2(nan, nan);
  }
}

// The scoring loop of a workgroup of 256 lanes that serves ONE segment [b, b + M): its matches go through s_pt
// [2 * FUND_CHUNK] in pieces of FUND_CHUNK, fetched from global memory once per workgroup, and point(p, q) sees every
// one of them as a broadcast read.  Every lane of the workgroup must call it.
template <typename Point>
__device__ __forceinline__ void for_each_staged_point(double2* s_pt, const float2* __restrict__ pts1,
                                                      const float2* __restrict__ pts2, int64_t b, int M, Point point) {
  for (int base = 0; base < M; base += FUND_CHUNK) {
    const int cnt = (M - base < FUND_CHUNK) ? (M - base) : FUND_CHUNK;
    __syncthreads();
    stage_points(s_pt, pts1, pts2, b + base, cnt, 256);
    __syncthreads();
    for (int i = 0; i < cnt; ++i) point(s_pt[2 * i], s_pt[2 * i + 1]);
  }
}

// inliers of f over the whole segment (not staged: every thread takes its own points); writes the mask when `mask` is
// not null
__device__ __forceinline__ int fund_count(const double (&f)[9], const float2* __restrict__ pts1,
                                          const float2* __restrict__ pts2, int64_t b, int M, double thr2,
                                          uint8_t* __restrict__ mask) {
  return segment_count(b, M, mask, [&](int64_t i) {
    const float2 p = pts1[i], q = pts2[i];
    return finite4(p, q) && fund_inlier(f, (double)p.x, (double)p.y, (double)q.x, (double)q.y, thr2);
  });
}
