// The calibrated minimal solver of the essential-matrix RANSAC (essential.hip): Nister's five-point algorithm
// ("An efficient solution to the five-point relative pose problem", PAMI 2004), for the device and - SFM_HD - for the
// host, so that the CPU tests can set it against NumPy sample by sample (tests/native/essential_solve_check.cpp).
//
//   1. x = (u - cx) / fx, y = (v - cy) / fy from float32 pixels widened to double
//   2. the 5 x 9 system, row = x2 (x) x1 (E row-major, x2^T E x1 = 0)
//   3. its null space X, Y, Z, W: Givens rotations of column pairs from the right, A G = [L 0]; the last four columns
//      of G are an orthonormal basis (the scheme of k_fund_hypotheses: no pivot, every index a constant).  E = xX + yY + zZ + W
//   4. det E = 0 and E E^T E - tr(E E^T) E / 2 = 0 as a 10 x 20 matrix in Nister's monomial order
//        x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
//   5. Gauss-Jordan with row pivoting on the left ten columns (rows 0..3 are not reduced further once they have served
//      as pivots: only rows 4..9 are read); k = e - z f, l = g - z h, m = i - z j give B(z), det B(z) has degree 10
//   6. its real roots, ascending: the real roots of p^(k) separate those of p^(k-1), so from the linear p^(9) upwards
//      every level brackets its roots between the roots of the level below (and -+ the Cauchy bound of p, which holds
//      every root of every derivative: Gauss-Lucas) and bisects where the sign changes; the roots of p itself then get
//      two Newton steps.  The coefficients of the level at work sit in registers.  No complex arithmetic, no division chain, and the same roots whatever ran before.  A double root
//      changes no sign and is not found: such a sample is at the edge between two counts of real roots anyway.
//      A polynomial with a non-finite coefficient, a zero leading one or a non-finite bound gives no model.
//   7. per root (x, y, w) = the cross product of two rows of B(z): of the pairs (k,l), (k,m), (l,m) the one with the
//      largest |w|, the first on a tie; w == 0 gives no candidate.  (x, y, z) then take three Gauss-Newton steps on the
//      nine cubic constraints themselves (polish() says why).  E = xX + yY + zZ + W, scaled to |E|_F = sqrt(2), the
//      entry of largest magnitude (the first on a tie) positive.
//
// A sample gives no model if it holds a non-finite coordinate, or if two of its matches share a pixel in image 1 or share
// a pixel in image 2 (float32 == on both coordinates): the doubled match leaves the system with rank 4 and the "null
// space" arbitrary - and matchers do repeat keypoints.
//
// Working storage: the 10 x 20 system is more than a lane's registers, and its elimination indexes rows at run time, so
// everything that is indexed at run time lives behind an accessor ws(e), e < WS_DOUBLES: a lane-interleaved LDS column
// on the device (strided<64>), a plain array on the host (strided<1>).  Register arrays are indexed by constants only.
#pragma once
#include <cfloat>
#include <cmath>
#include "ransac_common.h"

namespace fivept {

constexpr int WS_DOUBLES = 200;      // the 10 x 20 system; after the elimination the same storage holds:
constexpr int WS_ROOTS = 66;         //   [0, 66) p^(k) / k!, k = 0..10, at deriv_at(k); two root lists of 10
constexpr int WS_XYZ = 86;           //   (x, y, z) of up to 10 candidates
constexpr int MAX_CANDIDATES = 10;

template <int STRIDE>
struct strided {
  double* p;
  SFM_HD double& operator()(int e) const { return p[e * STRIDE]; }
};

SFM_HD constexpr int deriv_at(int k) { return k * 11 - k * (k - 1) / 2; }
static_assert(deriv_at(10) + 1 <= WS_ROOTS && WS_ROOTS + 2 * 10 <= WS_XYZ && WS_XYZ + 3 * MAX_CANDIDATES <= WS_DOUBLES,
              "the overlays of the working storage: derivative table, two root lists, candidates");
SFM_HD constexpr int rot_at(int i, int j) { return i * 8 - i * (i - 1) / 2 + (j - i - 1); }      // 30 rotations
SFM_HD constexpr int pair_at(int a, int b) { return a * 4 - a * (a - 1) / 2 + (b - a); }        // a <= b < 4
SFM_HD constexpr int sym3_at(int i, int j) { return i < j ? i * 3 - i * (i - 1) / 2 + (j - i) : j * 3 - j * (j - 1) / 2 + (i - j); }

// column of the monomial x^ex y^ey z^ez in Nister's order
SFM_HD constexpr int mono3(int ex, int ey, int ez) {
  const int key = ex * 16 + ey * 4 + ez;
  return key == 48 ? 0 : key == 12 ? 1 : key == 36 ? 2 : key == 24 ? 3 : key == 33 ? 4 : key == 32 ? 5 : key == 9 ? 6 :
         key == 8 ? 7 : key == 21 ? 8 : key == 20 ? 9 : key == 18 ? 10 : key == 17 ? 11 : key == 16 ? 12 : key == 6 ? 13 :
         key == 5 ? 14 : key == 4 ? 15 : key == 3 ? 16 : key == 2 ? 17 : key == 1 ? 18 : 19;
}

// polynomials in (x, y, z) by variable index 0, 1, 2 and 3 for the constant: degree <= 1 as [4], degree <= 2 as [10]
// (pair_at), degree <= 3 as [20] (mono3).  o += sg * p * q
SFM_HD void mul11(const double (&p)[4], const double (&q)[4], double sg, double (&o)[10]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) o[pair_at(a < b ? a : b, a < b ? b : a)] += sg * p[a] * q[b];
}

SFM_HD void mul21(const double (&q)[10], const double (&p)[4], double (&o)[20]) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = a; b < 4; ++b)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        o[mono3((a == 0) + (b == 0) + (c == 0), (a == 1) + (b == 1) + (c == 1), (a == 2) + (b == 2) + (c == 2))] +=
            q[pair_at(a, b)] * p[c];
}

// step 3.  rows [5][9]; returns false when a NaN came through
SFM_HD bool null_space(const double (&rows)[5][9], double (&Bs)[4][9]) {
  double rc[30], rs[30];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    double r[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) r[e] = rows[i][e];
#pragma unroll
    for (int ii = 0; ii < i; ++ii)
#pragma unroll
      for (int j = ii + 1; j < 9; ++j) {
        const double c = rc[rot_at(ii, j)], sn = rs[rot_at(ii, j)];
        const double u = r[ii], v = r[j];
        r[ii] = c * u + sn * v; r[j] = c * v - sn * u;
      }
#pragma unroll
    for (int j = i + 1; j < 9; ++j) {
      const double u = r[i], v = r[j];
      const double hh = sqrt(u * u + v * v);
      const bool nz = hh > 0.0;                            // NaN: (1, 0), and the NaN travels on in r
      rc[rot_at(i, j)] = nz ? u / hh : 1.0; rs[rot_at(i, j)] = nz ? v / hh : 0.0;
      r[i] = nz ? hh : u; r[j] = nz ? 0.0 : v;
    }
    ok = ok && (r[i] == r[i]);
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {                            // G e5 .. G e8: the rotations in reverse on the unit vectors
    double f[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) f[e] = (e == 5 + v) ? 1.0 : 0.0;
#pragma unroll
    for (int i = 4; i >= 0; --i)
#pragma unroll
      for (int j = 8; j > i; --j) {
        const double c = rc[rot_at(i, j)], sn = rs[rot_at(i, j)];
        const double u = f[i], w = f[j];
        f[i] = c * u - sn * w; f[j] = sn * u + c * w;
      }
#pragma unroll
    for (int e = 0; e < 9; ++e) Bs[v][e] = f[e];
  }
  return ok;
}

// step 4: row 0 = det E, rows 1..9 = the entries of (E E^T - tr(E E^T) / 2) E, into ws(20 * row + column)
template <class WS>
SFM_HD void build_constraints(const double (&Bs)[4][9], WS ws) {
  double L[9][4];
#pragma unroll
  for (int e = 0; e < 9; ++e)
#pragma unroll
    for (int v = 0; v < 4; ++v) L[e][v] = Bs[v][e];
  {
    double q0[10], q1[10], q2[10], acc[20];
#pragma unroll
    for (int m = 0; m < 10; ++m) q0[m] = q1[m] = q2[m] = 0.0;
#pragma unroll
    for (int m = 0; m < 20; ++m) acc[m] = 0.0;
    mul11(L[4], L[8], 1.0, q0); mul11(L[5], L[7], -1.0, q0);
    mul11(L[5], L[6], 1.0, q1); mul11(L[3], L[8], -1.0, q1);
    mul11(L[3], L[7], 1.0, q2); mul11(L[4], L[6], -1.0, q2);
    mul21(q0, L[0], acc); mul21(q1, L[1], acc); mul21(q2, L[2], acc);
#pragma unroll
    for (int m = 0; m < 20; ++m) ws(m) = acc[m];
  }
  double G[6][10];                                         // E E^T: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
#pragma unroll
      for (int m = 0; m < 10; ++m) G[sym3_at(i, j)][m] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) mul11(L[3 * i + k], L[3 * j + k], 1.0, G[sym3_at(i, j)]);
    }
#pragma unroll
  for (int m = 0; m < 10; ++m) {
    const double t = 0.5 * (G[0][m] + G[3][m] + G[5][m]);
    G[0][m] -= t; G[3][m] -= t; G[5][m] -= t;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double acc[20];
#pragma unroll
      for (int m = 0; m < 20; ++m) acc[m] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) mul21(G[sym3_at(i, k)], L[3 * k + j], acc);
#pragma unroll
      for (int m = 0; m < 20; ++m) ws(20 * (1 + 3 * i + j) + m) = acc[m];
    }
}

// step 5, first half.  false when a pivot is zero or not a number
template <class WS>
SFM_HD bool gauss_jordan(WS ws) {
  bool ok = true;
  for (int c = 0; c < 10; ++c) {
    int pr = c;
    double best = fabs(ws(20 * c + c));
    for (int r = c + 1; r < 10; ++r) {
      const double v = fabs(ws(20 * r + c));
      if (v > best) { best = v; pr = r; }
    }
    ok = ok && (best > 0.0);
    if (pr != c)
      for (int m = c; m < 20; ++m) { const double t = ws(20 * c + m); ws(20 * c + m) = ws(20 * pr + m); ws(20 * pr + m) = t; }
    const double inv = 1.0 / ws(20 * c + c);
    for (int m = c + 1; m < 20; ++m) ws(20 * c + m) *= inv;
    for (int r = (c < 4 ? c + 1 : 4); r < 10; ++r) {
      if (r == c) continue;
      const double f = ws(20 * r + c);
      for (int m = c + 1; m < 20; ++m) ws(20 * r + m) -= f * ws(20 * c + m);
    }
  }
  return ok;
}

// p^(k) / k! out of the table written by real_roots into registers, zero above its degree 10 - k, and its value at z:
// the leading zeros leave Horner's result as it is (0 * z + c = c for a finite z), and a bisection then costs no LDS read
template <class WS>
SFM_HD void deriv_load(WS ws, int k, double (&c)[11]) {
#pragma unroll
  for (int i = 0; i <= 10; ++i) {
    c[i] = 0.0;
    if (i <= 10 - k) c[i] = ws(deriv_at(k) + i);
  }
}

SFM_HD double horner10(const double (&c)[11], double z) {
  double acc = c[10];
#pragma unroll
  for (int i = 9; i >= 0; --i) acc = acc * z + c[i];
  return acc;
}

// step 6.  c[i] is the coefficient of z^i.  Returns the number of roots; root k is ws(WS_ROOTS + k), ascending
template <class WS>
SFM_HD int real_roots(const double (&c)[11], WS ws) {
  bool ok = c[10] != 0.0;
  double big = 0.0;
#pragma unroll
  for (int i = 0; i <= 10; ++i) ok = ok && std::isfinite(c[i]);
#pragma unroll
  for (int i = 0; i < 10; ++i) big = fmax(big, fabs(c[i] / c[10]));
  const double bound = 1.0 + big;
  if (!ok || !std::isfinite(bound)) return 0;
#pragma unroll
  for (int i = 0; i <= 10; ++i) ws(i) = c[i];
  for (int k = 0; k < 10; ++k)
    for (int i = 0; i < 10 - k; ++i) ws(deriv_at(k + 1) + i) = ws(deriv_at(k) + i + 1) * ((double)(i + 1) / (double)(k + 1));
  int m = 0, cur = 0;                                      // m roots of the level below in list cur ^ 1
  double ck[11];
  for (int d = 1; d <= 10; ++d) {
    deriv_load(ws, 10 - d, ck);
    int cnt = 0;
    double a = -bound, fa = horner10(ck, a);
    for (int j = 0; j <= m; ++j) {
      const double b = (j < m) ? ws(WS_ROOTS + 10 * (cur ^ 1) + j) : bound;
      const double fb = horner10(ck, b);
      if ((fa < 0.0) != (fb < 0.0)) {
        const bool neg = fa < 0.0;
        double lo = a, hi = b;
        for (int it = 0; it < 128; ++it) {
          const double mid = lo + 0.5 * (hi - lo);
          if (!(mid > lo && mid < hi)) break;
          if ((horner10(ck, mid) < 0.0) == neg) lo = mid; else hi = mid;
        }
        ws(WS_ROOTS + 10 * cur + cnt) = hi;
        ++cnt;
      }
      a = b; fa = fb;
    }
    m = cnt; cur ^= 1;
  }
  // ten levels: the last list written is list 1; move it to the front, polished (a step that is not finite is not
  // taken).  ck holds p; p' = p^(1) / 1!
  double c1[11];
  deriv_load(ws, 1, c1);
  for (int j = 0; j < m; ++j) {
    double z = ws(WS_ROOTS + 10 * (cur ^ 1) + j);
    for (int it = 0; it < 2; ++it) {
      const double f = horner10(ck, z), df = horner10(c1, z);
      const double zn = z - f / df;
      z = (df != 0.0 && std::isfinite(zn)) ? zn : z;
    }
    ws(WS_ROOTS + j) = z;
  }
  return m;
}

SFM_HD double horner3(const double (&p)[4], double z) { return ((p[3] * z + p[2]) * z + p[1]) * z + p[0]; }
SFM_HD double horner4(const double (&p)[5], double z) { return (((p[4] * z + p[3]) * z + p[2]) * z + p[1]) * z + p[0]; }

// steps 4 to 7 from a basis.  Returns the number of candidates; candidate k is (x, y, z) = ws(WS_XYZ + 3 k ...), by
// ascending z
template <class WS>
SFM_HD int solve_basis(const double (&Bs)[4][9], WS ws) {
  build_constraints(Bs, ws);
  if (!gauss_jordan(ws)) return 0;
  double bx[3][4], by[3][4], bc[3][5];                     // B(z) by ascending power of z
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    double e[10], f[10];
#pragma unroll
    for (int m = 0; m < 10; ++m) { e[m] = ws(20 * (4 + 2 * t) + 10 + m); f[m] = ws(20 * (5 + 2 * t) + 10 + m); }
    bx[t][0] = e[2]; bx[t][1] = e[1] - f[2]; bx[t][2] = e[0] - f[1]; bx[t][3] = -f[0];
    by[t][0] = e[5]; by[t][1] = e[4] - f[5]; by[t][2] = e[3] - f[4]; by[t][3] = -f[3];
    bc[t][0] = e[9]; bc[t][1] = e[8] - f[9]; bc[t][2] = e[7] - f[8]; bc[t][3] = e[6] - f[7]; bc[t][4] = -f[6];
  }
  double c[11];
#pragma unroll
  for (int i = 0; i <= 10; ++i) c[i] = 0.0;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int u = (t + 1) % 3, v = (t + 2) % 3;            // cofactor of (t, 2): cyclic, so the sign is +
    double co[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) co[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) co[i + j] += bx[u][i] * by[v][j] - bx[v][i] * by[u][j];
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
      for (int j = 0; j < 5; ++j) c[i + j] += co[i] * bc[t][j];
  }
  const int nr = real_roots(c, ws);
  int nc = 0;
  for (int k = 0; k < nr; ++k) {
    const double z = ws(WS_ROOTS + k);
    double X[3], Y[3], C[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) { X[t] = horner3(bx[t], z); Y[t] = horner3(by[t], z); C[t] = horner4(bc[t], z); }
    double x = 0.0, y = 0.0, w = 0.0;
#pragma unroll
    for (int pr = 0; pr < 3; ++pr) {
      const int a = pr == 2 ? 1 : 0, b = pr == 0 ? 1 : 2;
      const double cw = X[a] * Y[b] - Y[a] * X[b];
      if (pr == 0 || fabs(cw) > fabs(w)) { x = Y[a] * C[b] - C[a] * Y[b]; y = C[a] * X[b] - X[a] * C[b]; w = cw; }
    }
    x /= w; y /= w;
    if (w == 0.0 || !std::isfinite(x) || !std::isfinite(y)) continue;
    ws(WS_XYZ + 3 * nc) = x; ws(WS_XYZ + 3 * nc + 1) = y; ws(WS_XYZ + 3 * nc + 2) = z;
    ++nc;
  }
  return nc;
}

// steps 1 to 7 for one sample: px[k] = (u1, v1, u2, v2) of match k.  Returns the number of candidates (0: no model)
template <class WS>
SFM_HD int solve_sample(const float (&px)[5][4], double fx, double fy, double cx, double cy, WS ws, double (&Bs)[4][9]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int e = 0; e < 4; ++e) ok = ok && std::isfinite(px[k][e]);
#pragma unroll
  for (int k = 0; k < 5; ++k)
#pragma unroll
    for (int l = k + 1; l < 5; ++l)
      ok = ok && !((px[k][0] == px[l][0] && px[k][1] == px[l][1]) || (px[k][2] == px[l][2] && px[k][3] == px[l][3]));
  double rows[5][9];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const double x1 = ((double)px[k][0] - cx) / fx, y1 = ((double)px[k][1] - cy) / fy;
    const double x2 = ((double)px[k][2] - cx) / fx, y2 = ((double)px[k][3] - cy) / fy;
    rows[k][0] = x2 * x1; rows[k][1] = x2 * y1; rows[k][2] = x2;
    rows[k][3] = y2 * x1; rows[k][4] = y2 * y1; rows[k][5] = y2;
    rows[k][6] = x1; rows[k][7] = y1; rows[k][8] = 1.0;
  }
  if (!ok) return 0;
  if (!null_space(rows, Bs)) return 0;
  return solve_basis(Bs, ws);
}

// f = (E E^T - tr(E E^T) / 2) E, half of the nine cubic constraints, at a 3 x 3 E; returns |f|^2
SFM_HD double cubic_residual(const double (&E)[9], double (&L)[9], double (&f)[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) L[3 * i + j] = E[3 * i] * E[3 * j] + E[3 * i + 1] * E[3 * j + 1] + E[3 * i + 2] * E[3 * j + 2];
  const double h = 0.5 * (L[0] + L[4] + L[8]);
  L[0] -= h; L[4] -= h; L[8] -= h;
  double r2 = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      f[3 * i + j] = L[3 * i] * E[j] + L[3 * i + 1] * E[3 + j] + L[3 * i + 2] * E[6 + j];
      r2 += f[3 * i + j] * f[3 * i + j];
    }
  return r2;
}

SFM_HD void combine(const double (&Bs)[4][9], double x, double y, double z, double (&E)[9]) {
#pragma unroll
  for (int e = 0; e < 9; ++e) E[e] = x * Bs[0][e] + y * Bs[1][e] + z * Bs[2][e] + Bs[3][e];
}

// The root of the degree-10 polynomial carries the rounding of the elimination behind it, and (x, y) that of B(z): on
// real pairs the two singular values of E = xX + yY + zZ + W then differ by up to 1e-8.  Three Gauss-Newton steps on the
// nine cubic constraints in (x, y, z) - inside the null space, so the five epipolar constraints stay exact - take that
// out (two leave a candidate in 600 at 1e-10 where 1e-14 is there to be had: tests/solver_truth.py).  The Jacobian along a basis matrix D is (D E^T + E D^T - tr(D E^T)) E + (E E^T - tr(E E^T) / 2) D.  A step is
// kept only if it is finite and lowers |f|^2.
SFM_HD void polish(const double (&Bs)[4][9], double& x, double& y, double& z) {
  double E[9], L[9], f[9];
  combine(Bs, x, y, z, E);
  double r2 = cubic_residual(E, L, f);
  for (int it = 0; it < 3; ++it) {
    double J[3][9];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      double S[9];                                         // D E^T + E D^T - tr(D E^T) I
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          S[3 * i + j] = Bs[v][3 * i] * E[3 * j] + Bs[v][3 * i + 1] * E[3 * j + 1] + Bs[v][3 * i + 2] * E[3 * j + 2] +
                         E[3 * i] * Bs[v][3 * j] + E[3 * i + 1] * Bs[v][3 * j + 1] + E[3 * i + 2] * Bs[v][3 * j + 2];
      const double h = 0.5 * (S[0] + S[4] + S[8]);
      S[0] -= h; S[4] -= h; S[8] -= h;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          J[v][3 * i + j] = S[3 * i] * E[j] + S[3 * i + 1] * E[3 + j] + S[3 * i + 2] * E[6 + j] +
                            L[3 * i] * Bs[v][j] + L[3 * i + 1] * Bs[v][3 + j] + L[3 * i + 2] * Bs[v][6 + j];
    }
    double A[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};    // J^T J: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2); J^T f
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      A[0] += J[0][e] * J[0][e]; A[1] += J[0][e] * J[1][e]; A[2] += J[0][e] * J[2][e];
      A[3] += J[1][e] * J[1][e]; A[4] += J[1][e] * J[2][e]; A[5] += J[2][e] * J[2][e];
      g[0] += J[0][e] * f[e]; g[1] += J[1][e] * f[e]; g[2] += J[2][e] * f[e];
    }
    const double c0 = A[3] * A[5] - A[4] * A[4], c1 = A[2] * A[4] - A[1] * A[5], c2 = A[1] * A[4] - A[2] * A[3];
    const double det = A[0] * c0 + A[1] * c1 + A[2] * c2;
    const double d0 = (c0 * g[0] + c1 * g[1] + c2 * g[2]) / det;
    const double d1 = (c1 * g[0] + (A[0] * A[5] - A[2] * A[2]) * g[1] + (A[1] * A[2] - A[0] * A[4]) * g[2]) / det;
    const double d2 = (c2 * g[0] + (A[1] * A[2] - A[0] * A[4]) * g[1] + (A[0] * A[3] - A[1] * A[1]) * g[2]) / det;
    const double xn = x - d0, yn = y - d1, zn = z - d2;
    double En[9], Ln[9], fn[9];
    combine(Bs, xn, yn, zn, En);
    const double rn = cubic_residual(En, Ln, fn);
    if (!(rn < r2)) break;                                 // also a step that is not finite
    x = xn; y = yn; z = zn; r2 = rn;
#pragma unroll
    for (int e = 0; e < 9; ++e) { E[e] = En[e]; L[e] = Ln[e]; f[e] = fn[e]; }
  }
}

// step 7, second half: candidate k as E (normalised coordinates), polished, |E|_F = sqrt(2), largest entry positive.
// false, and E = 0, when it is not finite
template <class WS>
SFM_HD bool candidate(const double (&Bs)[4][9], WS ws, int k, double (&E)[9]) {
  double x = ws(WS_XYZ + 3 * k), y = ws(WS_XYZ + 3 * k + 1), z = ws(WS_XYZ + 3 * k + 2);
  polish(Bs, x, y, z);
  combine(Bs, x, y, z, E);
  double n2 = 0.0, big = 0.0, sg = 1.0;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    n2 += E[e] * E[e];
    if (fabs(E[e]) > big) { big = fabs(E[e]); sg = E[e] < 0.0 ? -1.0 : 1.0; }
  }
  const double sc = sg * sqrt(2.0 / n2);
  bool ok = n2 > 0.0;
#pragma unroll
  for (int e = 0; e < 9; ++e) { E[e] *= sc; ok = ok && std::isfinite(E[e]); }
#pragma unroll
  for (int e = 0; e < 9; ++e) E[e] = ok ? E[e] : 0.0;
  return ok;
}

}  // namespace fivept
