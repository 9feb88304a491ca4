// What the batched RANSAC stages (twoview.hip, essential.hip, homography.hip, pnp.hip, pose.hip) and their solver
// headers share and the host can compile too: the segment convention, the stateless sample generator, the closed-form
// cubic and the numbering of the Givens rotations.  The functions marked SFM_HD build with g++, so that the generator
// and the minimal solvers built on them can be checked on a CPU (tests/native/).  The device-only part - kernels, block
// sums, the winner rule - is in ransac_kernels.h.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SFM_HD __host__ __device__ __forceinline__
#else
#define SFM_HD inline
#endif

constexpr int RANSAC_MAX_DRAWS = 256;

SFM_HD uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// segment s as [b, b + M) inside [0, n): seg_ptr is trusted to ascend, the clamps keep a bad one inside the arrays
SFM_HD void seg_range(const int64_t* __restrict__ seg_ptr, int s, int64_t n, int64_t& b, int& M) {
  int64_t lo = seg_ptr[s], hi = seg_ptr[s + 1];
  hi = hi < 0 ? 0 : (hi > n ? n : hi);
  lo = lo < 0 ? 0 : (lo > hi ? hi : lo);
  const int64_t m = hi - lo;
  b = lo;
  M = (int)(m > 0x7fffffffLL ? 0x7fffffffLL : m);
}

// N distinct indices of [0, M), M >= N, for (seed, segment s, hypothesis hyp).  All arithmetic is uint64, wrapping,
// and mix is mix64 above (the splitmix64 finaliser):
//   key  = mix(mix(mix(seed) ^ s) ^ hyp);  draw d = 0, 1, 2, ...:  index = ((mix(key ^ d) >> 32) * M) >> 32
// The slots are filled in order; a draw equal to an earlier slot is discarded and the next d is taken.  After
// RANSAC_MAX_DRAWS draws a slot takes the lowest unused index.
template <int N>
SFM_HD void draw_distinct(uint64_t seed, int s, int hyp, int M, int (&idx)[N]) {
  const uint64_t key = mix64(mix64(mix64(seed) ^ (uint64_t)s) ^ (uint64_t)hyp);
  uint64_t d = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    int v = -1;
    while (d < (uint64_t)RANSAC_MAX_DRAWS) {
      const int c = (int)(((mix64(key ^ d) >> 32) * (uint64_t)M) >> 32);
      ++d;
      bool dup = false;
#pragma unroll
      for (int j = 0; j < N; ++j) dup |= (j < k) && (idx[j] == c);
      if (!dup) { v = c; break; }
    }
    if (v < 0) {                                     // lowest unused index (at most N - 1 are taken, M >= N)
      for (int c = 0; c < N && v < 0; ++c) {
        bool dup = false;
#pragma unroll
        for (int j = 0; j < N; ++j) dup |= (j < k) && (idx[j] == c);
        if (!dup) v = c;
      }
    }
    idx[k] = v;
  }
}

// Real roots of the monic cubic x^3 + A x^2 + B x + C in closed form (trigonometric / Cardano): three, ascending,
// or one (root[1] = root[2] = 0 then).  Returns their number.
SFM_HD int cubic_roots_monic(double A, double B, double Cc, double (&root)[3]) {
  const double Q = (A * A - 3.0 * B) / 9.0, R = (2.0 * A * A * A - 9.0 * A * B + 27.0 * Cc) / 54.0;
  const double Q3 = Q * Q * Q;
  if (R * R < Q3) {
    const double sq = sqrt(Q);
    double ct = R / (sq * sq * sq);
    ct = ct < -1.0 ? -1.0 : (ct > 1.0 ? 1.0 : ct);
    const double th = acos(ct);
    const double two_pi = 6.283185307179586476925286766559;
    root[0] = -2.0 * sq * cos(th / 3.0) - A / 3.0;                 // ascending for th in [0, pi]
    root[1] = -2.0 * sq * cos((th + 2.0 * two_pi) / 3.0) - A / 3.0;
    root[2] = -2.0 * sq * cos((th + two_pi) / 3.0) - A / 3.0;
    return 3;
  }
  const double e = cbrt(fabs(R) + sqrt(R * R - Q3));
  const double aa = R > 0.0 ? -e : e;
  const double bb = aa != 0.0 ? Q / aa : 0.0;
  root[0] = aa + bb - A / 3.0; root[1] = 0.0; root[2] = 0.0;
  return 1;
}

// two Newton steps on the monic cubic from x; a step that is not finite is not taken
SFM_HD double cubic_newton2(double x, double A, double B, double Cc) {
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const double fx = ((x + A) * x + B) * x + Cc, dx = (3.0 * x + 2.0 * A) * x + B;
    const double xn = x - fx / dx;
    x = (dx != 0.0 && std::isfinite(xn)) ? xn : x;
  }
  return x;
}

// The Givens eliminations of fundamental_solve.h (7 x 9, 35 rotations) and homography_solve.h (8 x 9, 36) number their
// rotations alike: rotation k acts on columns (i, j), j > i, with k = i*8 - i*(i-1)/2 + (j - i - 1)
SFM_HD constexpr int rot_index(int i, int j) { return i * 8 - i * (i - 1) / 2 + (j - i - 1); }
