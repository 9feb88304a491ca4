// Robust N-view triangulation of one track: an outlier observation is dropped, not the point.  For the device
// (triangulate.hip) and - SFM_HD - for the host, so that the CPU tests can set it against the NumPy restatement
// (tests/triangulate_robust_reference.py, tests/native/triangulate_robust_check.cpp).  tri::solve of triangulate_solve.h
// is used as it is.  For one track, with u_0..u_{m-1} its used observations in track order:
//   sound        the pixel, P and C of the observation are finite
//   agrees       the observation is sound, its depth hw > 0 and its error e <= max_error at a point X (tri::reproj)
//   Consensus    a source adaptor {src, X, max_error}: get / centre answer false unless the observation agrees with X,
//                so a subset of the observations is described by a point and needs no stored mask
//   pair_of      pair number of hypothesis h over the s sound observations, and its two ranks (a < b)
//   hypothesis   (score, X_h) of hypothesis h: jacobi::dlt2 of the pair, score = observations that agree with X_h
//   finish       the refit tri::solve over Consensus{X_winner}, then the census at the refit point
//   solve_robust step 1 (tri::solve over all used observations), step 2 (the hypotheses, h on a host loop), step 3 (finish)
//   classify     the gates at a given X over the observations that agree with it: tri::judge over Consensus{X}
// Storage is constant in the track length, every walk over the observations runs in the track's own order and there is
// no FMA contraction (host builds pass -ffp-contract=off): a track's outputs depend on its used observations only.
#pragma once
#include "triangulate_solve.h"

namespace tri {

SFM_HD bool sound(const Obs& o) {
  bool f = std::isfinite(o.x) && std::isfinite(o.y) && finite3(o.C);
#pragma unroll
  for (int e = 0; e < 12; ++e) f = f && std::isfinite(o.P[e]);
  return f;
}

// e is written whenever the observation is sound (NaN or inf where the projection is)
SFM_HD bool agrees(const Obs& o, const double (&X)[3], double max_error, double& e) {
  e = NAN;
  if (!sound(o)) return false;
  double hw, e2;
  e = reproj(o, X, hw, e2);
  return hw > 0.0 && e <= max_error;
}

template <class Src>
struct Consensus {
  const Src& src;
  double X[3];
  double max_error;
  SFM_HD bool get(int k, Obs& o) const {
    if (!src.get(k, o)) return false;
    double e;
    return agrees(o, X, max_error, e);
  }
  SFM_HD bool centre(int k, double (&C)[3]) const {
    Obs o;
    if (!get(k, o)) return false;
    C[0] = o.C[0]; C[1] = o.C[1]; C[2] = o.C[2];
    return true;
  }
};

// used and sound observations of a track
template <class Src>
SFM_HD void count_views(const Src& src, int n_raw, int& n_used, int& n_sound) {
  Obs o;
  n_used = 0; n_sound = 0;
  for (int k = 0; k < n_raw; ++k) {
    if (!src.get(k, o)) continue;
    ++n_used;
    n_sound += sound(o) ? 1 : 0;
  }
}

// number of hypotheses of a track with s sound observations: min(s (s - 1) / 2, SFM_TRI_ROBUST_PAIRS)
SFM_HD int hypotheses(int s) {
  const int64_t M = (int64_t)s * (s - 1) / 2;
  return M < SFM_TRI_ROBUST_PAIRS ? (int)M : SFM_TRI_ROBUST_PAIRS;
}

// Hypothesis h (0 <= h < hypotheses(s)) uses pair number h of the M = s (s - 1) / 2 pairs (a, b), a < b, in
// lexicographic order when M <= H = SFM_TRI_ROBUST_PAIRS and pair number (h * M) / H otherwise; a and b are ranks among
// the sound observations.  Returns the pair number.  (h * M) / H is formed as h * (M / H) + (h * (M % H)) / H, the same
// integer without the large product.
SFM_HD int64_t pair_of(int h, int s, int& a, int& b) {
  const int64_t H = SFM_TRI_ROBUST_PAIRS;
  const int64_t M = (int64_t)s * (s - 1) / 2;
  const int64_t pair = M <= H ? (int64_t)h : (int64_t)h * (M / H) + ((int64_t)h * (M % H)) / H;
  int64_t p = pair;
  a = 0;
  while (a < s - 2 && p >= (int64_t)(s - 1 - a)) { p -= s - 1 - a; ++a; }
  b = a + 1 + (int)p;
  return pair;
}

// Hypothesis h of a track with s >= 2 sound observations: the point X_h of jacobi::dlt2 of its pair and its score, the
// number of used observations that agree with X_h.  A void hypothesis scores 0 and leaves X_h NaN: v[3] == 0, a point
// that is not finite, a depth <= 0 in one of the two views, or - with the angle gate on - two rays that do not pass it
// (the gate of tri::gates on this pair: cos <= cos_min_angle passes).
template <class Src>
SFM_HD int hypothesis(const Src& src, int n_raw, int s, double max_error, bool check_angle, double cos_min_angle, int h,
                      double (&Xh)[3]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  Xh[0] = NAN; Xh[1] = NAN; Xh[2] = NAN;
  int a, b;
  pair_of(h, s, a, b);
  Obs o, oa, ob;
  int rank = 0, found = 0;
  for (int k = 0; k < n_raw && found < 2; ++k) {
    if (!src.get(k, o) || !sound(o)) continue;
    if (rank == a) { oa = o; ++found; }
    if (rank == b) { ob = o; ++found; }
    ++rank;
  }
  if (found < 2) return 0;
  double v[4];
  jacobi::dlt2(oa.P, ob.P, oa.x, oa.y, ob.x, ob.y, v);
  if (v[3] == 0.0) return 0;
  const double X[3] = {v[0] / v[3], v[1] / v[3], v[2] / v[3]};
  if (!finite3(X)) return 0;
  double hwa, hwb, e2;
  reproj(oa, X, hwa, e2);
  reproj(ob, X, hwb, e2);
  if (hwa <= 0.0 || hwb <= 0.0) return 0;
  if (check_angle) {
    const double a0 = X[0] - oa.C[0], a1 = X[1] - oa.C[1], a2 = X[2] - oa.C[2];
    const double na = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
    const double b0 = X[0] - ob.C[0], b1 = X[1] - ob.C[1], b2 = X[2] - ob.C[2];
    const double nb = sqrt(b0 * b0 + b1 * b1 + b2 * b2);
    if (!((a0 * b0 + a1 * b1 + a2 * b2) / (na * nb) <= cos_min_angle)) return 0;
  }
  int score = 0;
  for (int k = 0; k < n_raw; ++k) {
    if (!src.get(k, o)) continue;
    double e;
    score += agrees(o, X, max_error, e) ? 1 : 0;
  }
  Xh[0] = X[0]; Xh[1] = X[1]; Xh[2] = X[2];
  return score;
}

// the observations that agree with X: how many, and their largest error (0 without any)
template <class Src>
SFM_HD void census(const Src& src, int n_raw, const double (&X)[3], double max_error, int& n_inliers, double& max_err) {
  Obs o;
  n_inliers = 0; max_err = 0.0;
  for (int k = 0; k < n_raw; ++k) {
    if (!src.get(k, o)) continue;
    double e;
    if (!agrees(o, X, max_error, e)) continue;
    ++n_inliers;
    max_err = e > max_err ? e : max_err;
  }
}

// Step 3.  The refit is tri::solve over the observations that agree with Xw, with min_views = max(min_views, 3) and the
// caller's refine_iters and gates.  False when its status is not OK (nothing is written then).  Otherwise X is the refit
// point, n_inliers the number of used observations that agree with X - a superset of the refit's own set - and max_err
// their largest error.
template <class Src>
SFM_HD bool finish(const Src& src, int n_raw, int min_views, int refine_iters, double max_error, bool check_angle,
                   double cos_min_angle, const double (&Xw)[3], double (&X)[3], int& n_inliers, double& max_err) {
  const Consensus<Src> c{src, {Xw[0], Xw[1], Xw[2]}, max_error};
  double Xr[3], me;
  int nv;
  if (solve(c, n_raw, min_views < 3 ? 3 : min_views, refine_iters, max_error, check_angle, cos_min_angle, Xr, nv, me) !=
      SFM_TRI_OK)
    return false;
  X[0] = Xr[0]; X[1] = Xr[1]; X[2] = Xr[2];
  census(src, n_raw, X, max_error, n_inliers, max_err);
  return true;
}

// obs_inlier[k], k < n_raw: 1 for the used observations that agree with X, 0 elsewhere
template <class Src>
SFM_HD void flag_inliers(const Src& src, int n_raw, const double (&X)[3], double max_error, uint8_t* obs_inlier) {
  Obs o;
  for (int k = 0; k < n_raw; ++k) {
    double e;
    obs_inlier[k] = (src.get(k, o) && agrees(o, X, max_error, e)) ? 1 : 0;
  }
}

// The whole rule.  Step 1: full = tri::solve over all used observations; OK returns it as it is with every used
// observation an inlier.  A failing track with fewer than 4 sound observations returns full with no inlier.  Step 2: the
// hypotheses h = 0 .. hypotheses(s) - 1; the winner has the highest score, ties go to the lowest h; below
// max(min_views, 3) full is returned.  Step 3: finish(); when the refit fails full is returned.  n_views is the number
// of used observations in every case.  obs_inlier has n_raw entries.
template <class Src>
SFM_HD int solve_robust(const Src& src, int n_raw, int min_views, int refine_iters, double max_error, bool check_angle,
                        double cos_min_angle, double (&X)[3], int& n_views, int& n_inliers, double& max_err,
                        uint8_t* obs_inlier) {
  const int full = solve(src, n_raw, min_views, refine_iters, max_error, check_angle, cos_min_angle, X, n_views, max_err);
  Obs o;
  if (full == SFM_TRI_OK) {
    for (int k = 0; k < n_raw; ++k) obs_inlier[k] = src.get(k, o) ? 1 : 0;
    n_inliers = n_views;
    return full;
  }
  for (int k = 0; k < n_raw; ++k) obs_inlier[k] = 0;
  n_inliers = 0;
  int n_used, s;
  count_views(src, n_raw, n_used, s);
  if (s < 4) return full;
  const int n_hyp = hypotheses(s);
  int best = 0;
  double Xw[3] = {NAN, NAN, NAN};
  for (int h = 0; h < n_hyp; ++h) {
    double Xh[3];
    const int score = hypothesis(src, n_raw, s, max_error, check_angle, cos_min_angle, h, Xh);
    if (score > best) { best = score; Xw[0] = Xh[0]; Xw[1] = Xh[1]; Xw[2] = Xh[2]; }
  }
  if (best < (min_views < 3 ? 3 : min_views)) return full;
  double Xr[3], me;
  int ni;
  if (!finish(src, n_raw, min_views, refine_iters, max_error, check_angle, cos_min_angle, Xw, Xr, ni, me)) return full;
  X[0] = Xr[0]; X[1] = Xr[1]; X[2] = Xr[2];
  n_inliers = ni;
  max_err = me;
  flag_inliers(src, n_raw, X, max_error, obs_inlier);
  return SFM_TRI_OK;
}

// The gates at a given X over the observations that agree with it: tri::judge over Consensus{src, X, max_error}.
// OK, TOO_FEW_VIEWS (fewer than min_views agree; a non-finite X lands here) or LOW_ANGLE.  n_inliers is the number of
// observations that agree, max_err their largest error (NaN for TOO_FEW_VIEWS).  Fed the X of solve_robust with the
// same cameras and gates, a track of status OK gets OK, the same n_inliers and the same max_err bits.
template <class Src>
SFM_HD int classify(const Src& src, int n_raw, int min_views, const double (&X)[3], double max_error, bool check_angle,
                    double cos_min_angle, int& n_inliers, double& max_err) {
  const Consensus<Src> c{src, {X[0], X[1], X[2]}, max_error};
  return judge(c, n_raw, min_views, X, max_error, check_angle, cos_min_angle, n_inliers, max_err);
}

}  // namespace tri
