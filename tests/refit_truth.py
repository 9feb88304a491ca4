"""A multi-precision truth for the REFITS that end the four batched RANSAC stages (k_fund_refit, k_hom_refit, k_ess_refit,
k_pnp_refine) and for the Hartley transforms in front of two of them, and the judge that holds a model to it
(tests/test_refit_truth.py on the CPU, tests/test_refit_truth_gpu.py on the device).  The minimal solvers have their
truth in tests/solver_truth.py; this module reuses its small mp algebra, its essential seeds and polish, its [R|t]
distance and its constants MARGIN = 8 and LEFT_OUT = 1e-6.

The truth solves each PROBLEM in mpmath at 60 digits from exact inputs (float32 pixels, float64 world points and K, a
given inlier mask and, for F and H, a given transform T = (sc1, cx1, cy1, sc2, cx2, cy2)).  It replays no kernel.

    hartley      per image, over the finite matches: the centroid and sqrt(2) / the mean distance to it
    fundamental  x' = sc (x - c); the eigenvector of the smallest eigenvalue of A^T A over the mask (mp.eigsy, every
                 eigenpair checked to a residual under 1e-40); its 3 x 3 replaced by the nearest rank-2 matrix (mp.svd_r);
                 T2^T Fn T1
    homography   the smallest eigenvector of the normal matrix of the two rows per match; T2^-1 Hn T1
    essential    the invariant subspace of the four smallest eigenvalues of A^T A in K-normalised coordinates, then all
                 real E in it with det E = 0 and 2 E E^T E - tr(E E^T) E = 0: solver_truth's seeds (det C(z) at the 11th
                 roots of unity, twice) and Gauss-Newton polish, on this basis
    pnp          the stationary point of the summed squared reprojection error over the mask: Newton on the gradient in the
                 local parametrisation R <- exp([w]x) R, seeded from pnp_reference.refit (scipy), the gradient in mpmath,
                 its Jacobian a float64 central difference held fixed (the iteration gains nine digits a step), until the
                 gradient norm is under 1e-40.  The seed's rotation is first made orthogonal in mpmath (Newton's polar
                 iteration).

Condition.  kappa: all inputs of the problem (the masked pixels, world points, K, T) multiplied at once by 1 +- 2^-40,
independent signs, three fixed-seed draws, re-solved; kappa = max distance / 2^-40.

Distances.  F, H, E: the sine of the angle between the 9-vectors.  [R|t]: solver_truth's, max(|R - R*|_F,
|t - t*| / max(|t*|, extent)) with extent the largest distance of a masked world point from their centroid.  T: the larger,
over the two images, of |sc - sc*| / sc* and |c - c*| sc* / sqrt(2) (the centre's error against the mean distance).

The judge.  ratio = distance / unit with unit = kappa 2^-53; for PnP the kernel promises a stop at
|step| <= 1e-12 (1 + |x|), x = (angle(R), t), not at rounding, so its unit is kappa 2^-53 + 1e-12 (1 + |x|).  C_REF is the
worst ratio of the NumPy references (fr.refit, hr.refit, er.refit, pr.lm_refit - the kernel's LM replayed in float64 -
and fr.hartley) over the scenes below; the references hold 1 x C_REF and the device MARGIN x C_REF.  A scene whose bound
MARGIN C_REF kappa 2^-53 passes LEFT_OUT = 1e-6 may not be in the list at all: nothing is left out of the judged set.

Scenes (segments(stage)): noise 0.3 px; M = minimum + 1 and + 2 without outliers (8 and 9 for F: the first sizes at which
the winner's count passes the refit's gate; one thread holds one match), M = 40, 255, 256, 257, 513, 1025 with the first
int(0.3 M) matches outliers (255 .. 257 and 513 straddle the 256-thread stride, so a thread takes one or two matches
and all four waves add to the block sums; whole waves skip on the mask), one segment of 42 with two non-finite matches,
and one segment at noise 1.5 px whose reference refit LOSES (the first seed of 0 .. 499 where fewer matches pass under
the refit than under the winner and no squared error lies within 1e-6 of threshold^2).  The homography scenes are
hr.planar, and hr.rotation (whose noise is its own 0.5 px) at M = 40 and 257.  Then the edge segments: every match
non-finite, one finite match, one segment under the stage's minimum and, for F, M = 7 (a winner with 7 < 8 inliers).
Samples: ransac_reference.draw_samples(SEED, segment, M, 64, ...).

Measured (CPU: the references on their own winner masks; device = MI355X, on the mask and T of its own refine = 0 call;
left out = scenes whose bound passes 1e-6; time = CPU seconds of the stage's truths here):

    stage         segments   C_REF   bound 8 x C_REF   worst device   left out   time
    hartley       12 + 11    10.91   87.28             11.8           0          1 s
    fundamental   9          17.76   142.1             8.82           0          2 s
    homography    9          24.28   194.2             16.2           0          2 s
    essential     9          286.7   2294              14.3           0          3 s
    pnp           9          9.646   77.17             0.278          0          5 s

(segments = the judged ones; each stage's call also holds the segment whose refit loses - seeds 31, 30 and 10 for F, H and
E; PnP has no such seed in 0 .. 499 and goes without that segment - and the edge segments.)  The essential scene at
M = 513 is seed 361 (RESEED): at seed 360 the best root of the truth counts 362 matches where the winner counts 363, so
that refit legitimately loses.  C_REF of the essential refit is large for the reason solver_truth gives for its own:
kappa is that of the problem, while both the reference and the kernel go through A^T A in K-normalised coordinates,
whose eigenvectors feel the square of the spread of the singular values.

What the bounds found when they were first run: no defect on the device; every stage lies under its bound by a factor
of ten or more, and PnP by 280.  PnP's C_REF comes from ONE view (M = 257): four LM steps bring the float64 replay to
2.5e-11 of the stationary point, where the cost no longer drops in float64 (it is flat to 1e-21 relative), so every
further step is refused, mu grows tenfold six times and the loop ends by its step rule on the DAMPED step - ten times the
1e-12 (1 + |x|) it promises.  The kernel has the same rule and meets the same end on other views (its worst, 0.278 of the
unit, is M = 255); all other views of both end within 0.02 of the unit.  A stop taken from the undamped step would be
the tighter rule; the bound does not ask for it.
"""
import functools
import time

import numpy as np

import essential_reference as er
import fundamental_reference as fr
import homography_reference as hr
import pnp_reference as pr
import ransac_reference
from solver_truth import (K4_REF, LEFT_OUT, MARGIN, MP, RES_MAX, U40, U53, _cof, _dot, _draws, _epi_rows, _ess_model, _ess_polish,
                          _ess_seeds, _hom_rows, _mat, _merge, _mp, _norm, _perturb, _rt_distance, _sine, _to_ld, _tr,
                          _unit, mpf, ws_regions)  # noqa: F401
from test_solver_truth_gpu import THR

STAGES = ("fundamental", "homography", "essential", "pnp")
SEED = 17
N_HYP = 64
SAMPLE = {"fundamental": (7, 7), "homography": (4, 4), "essential": (5, 5), "pnp": (3, 4)}       # (size, least points)
GATE = {"fundamental": 8, "homography": 4, "essential": 5, "pnp": 3}                                # least count for a refit
SIZES = (40, 255, 256, 257, 513, 1025)
# the seed of the segment whose reference refit loses (find_dropped(); None: no seed of 0 .. 499 has one)
DROPPED_SEED = {"fundamental": 31, "homography": 30, "essential": 10, "pnp": None}
# the worst ratio of the NumPy references against this truth, measured by test_refit_truth.measure_c()
C_REF = {"hartley": 10.91, "fundamental": 17.76, "homography": 24.28, "essential": 286.7, "pnp": 9.646}


# --------------------------------------------------------------------------------------------------- scenes
class Segment:
    """kind: "kept" (judged against the truth), "dropped" (the reference's refit loses), or an edge: "nonfinite", "one",
    "short", "seven"."""

    def __init__(self, name, kind, data, k4=K4_REF):
        self.name, self.kind, self.data, self.k4 = name, kind, data, k4
        self.n = len(data[0])


def _scene(stage, seed, M, share, noise=0.3, rot=False):
    rng = np.random.default_rng(seed)
    if stage == "pnp":
        return pr.synth_view(rng, M, share, noise=noise)[:2]
    if stage == "homography":
        return hr.rotation(rng, M, share)[:2] if rot else hr.planar(rng, M, share, noise=noise)[:2]
    return fr.synth_pair(rng, M, share, noise=noise)[:2]


# a scene that fails a precondition of test_refit_truth.py is replaced by the next seed HERE: {(stage, M): seed}
RESEED = {("essential", 513): 361}


@functools.lru_cache(maxsize=None)
def segments(stage):
    """The segments of a stage's device call, in order - computed once, never modified."""
    least = SAMPLE[stage][1]
    first = 8 if stage == "fundamental" else least + 1
    out = []
    for k, M in enumerate((first, first + 1) + SIZES):
        rot = stage == "homography" and M in (40, 257)
        seed = RESEED.get((stage, M), 300 + 10 * k)
        out.append(Segment(f"M = {M}" + (", rotation" if rot else ""), "kept", _scene(stage, seed, M, 0.3 if M >= 40 else 0.0, rot=rot)))
    a, b = (np.array(v) for v in _scene(stage, RESEED.get((stage, 42), 390), 42, 0.3))
    a[33] = np.inf
    b[15, 1] = np.nan
    out.append(Segment("M = 42, two non-finite", "kept", (a, b)))
    if DROPPED_SEED[stage] is not None:
        out.append(Segment("noise 1.5 px, the refit loses", "dropped", _scene(stage, DROPPED_SEED[stage], 40, 0.3, noise=1.5)))
    a, b = (np.array(v[:10]) for v in out[2].data)
    out.append(Segment("every match non-finite", "nonfinite", (a, np.full_like(b, np.nan))))
    a, b = (np.array(v[-10:]) for v in out[2].data)
    a[:4], a[5:] = np.nan, np.inf
    out.append(Segment("one finite match", "one", (a, b)))
    out.append(Segment("under the minimum", "short", tuple(np.array(v[-(least - 1):]) for v in out[2].data)))
    if stage == "fundamental":
        out.append(Segment("M = 7", "seven", _scene(stage, 397, 7, 0.0)))
    return out


@functools.lru_cache(maxsize=None)
def samples(stage, s):
    size, least = SAMPLE[stage]
    return ransac_reference.draw_samples(SEED, s, segments(stage)[s].n, N_HYP, size, least)


# ------------------------------------------------------------------------- the rule, the references' own refits
def _f64(data):
    return tuple(np.asarray(v, np.float64) for v in data)


def error_ratio(stage, model, seg):
    """[M] float64: each match's squared error over threshold^2 by the stage's rule (inlier: <= 1); NaN for a non-finite
    match, inf for a point behind the camera."""
    a, b = _f64(seg.data)
    thr2 = THR[stage] ** 2
    with np.errstate(all="ignore"):
        if stage in ("fundamental", "essential"):
            F = np.asarray(model, np.float64).reshape(3, 3)
            return fr.cv_err2(er.to_pixels(F, pr.k_matrix(seg.k4)) if stage == "essential" else F, a, b) / thr2
        if stage == "homography":
            e, w2 = hr.residuals(model, a, b)
            r = np.where(w2 != 0, e / (thr2 * w2), np.inf)
        else:
            Rt = np.asarray(model, np.float64).reshape(3, 4)
            p = (a @ Rt[:, :3].T + Rt[:, 3]) @ pr.k_matrix(seg.k4).T
            e0, e1 = p[:, 0] - b[:, 0] * p[:, 2], p[:, 1] - b[:, 1] * p[:, 2]
            r = np.where(p[:, 2] > 0, (e0 * e0 + e1 * e1) / (thr2 * p[:, 2] * p[:, 2]), np.inf)
        return np.where(np.isfinite(a).all(1) & np.isfinite(b).all(1), r, np.nan)


def rule_mask(stage, model, seg):
    with np.errstate(invalid="ignore"):
        return error_ratio(stage, model, seg) <= 1.0


def band(stage, model, seg, width):
    """[M] bool: the matches whose squared error lies within `width` (relative) of threshold^2."""
    with np.errstate(invalid="ignore"):
        return np.abs(error_ratio(stage, model, seg) - 1.0) <= width


def hartley6(p1, p2):
    """fr.hartley over the finite matches of both images, in the kernel's factored form (sc1, cx1, cy1, sc2, cx2, cy2)."""
    p1, p2 = _f64((p1, p2))
    fin = np.isfinite(p1).all(1) & np.isfinite(p2).all(1)
    if not fin.any():
        return np.array([1.0, 0, 0, 1.0, 0, 0])
    out = []
    for p in (p1[fin], p2[fin]):
        T = fr.hartley(p)
        c = p.mean(0)
        out += [T[0, 0], c[0], c[1]]
    return np.array(out)


def t_matrices(T6):
    s1, x1, y1, s2, x2, y2 = (float(v) for v in T6)
    return np.array([[s1, 0, -s1 * x1], [0, s1, -s1 * y1], [0, 0, 1.0]]), np.array([[s2, 0, -s2 * x2], [0, s2, -s2 * y2], [0, 0, 1.0]])


def reference_winner(stage, s):
    """The reference's refine = 0 result for segment s: (model flat or None, mask, count, T6 or None)."""
    seg = segments(stage)[s]
    a, b = _f64(seg.data)
    K = pr.k_matrix(seg.k4)
    with np.errstate(all="ignore"):
        if stage == "fundamental":
            r = fr.ransac(a, b, samples(stage, s), THR[stage])
            m = r["F"]
        elif stage == "homography":
            r = hr.ransac(a, b, samples(stage, s), THR[stage])
            m = r["H"]
        elif stage == "essential":
            r = er.ransac(a, b, K, samples(stage, s), THR[stage])
            m = r["E"]
        else:
            r = pr.ransac(a, b, K, samples(stage, s), THR[stage])
            m = None if r["R"] is None else np.c_[r["R"], r["t"]]
    T6 = hartley6(a, b) if stage in ("fundamental", "homography") else None
    return (None if m is None else np.asarray(m, np.float64).ravel()), r["mask"], int(r["n_inliers"]), T6


def reference_refit(stage, seg, mask, T6=None, start=None):
    """The NumPy reference's refit over `mask`: the model, flat (F, H scaled to [2][2] = 1; E; [R|t] by pr.lm_refit from
    `start`), and for PnP the number of LM steps."""
    a, b = _f64(seg.data)
    K = pr.k_matrix(seg.k4)
    mask = np.asarray(mask, bool)
    if stage == "fundamental":
        return fr.refit(a, b, *t_matrices(T6), mask).ravel(), None
    if stage == "homography":
        return hr.refit(a, b, *t_matrices(T6), mask).ravel(), None
    if stage == "essential":
        E = er.refit(a, b, K, mask, THR[stage])[0]
        return (None if E is None else E.ravel()), None
    Rt =np.asarray(start, np.float64).reshape(3, 4)
    R, t, steps = pr.lm_refit(K, Rt[:, :3], Rt[:, 3], a[mask], b[mask])
    return np.c_[R, t].ravel(), steps


# ------------------------------------------------------------------------------------------------ mp algebra
def _normal(rows):
    """A^T A [9,9] (mp matrix) of rows [r][9]."""
    cols = list(zip(*rows))
    A = MP.zeros(9)
    for u in range(9):
        for v in range(u, 9):
            A[u, v] = A[v, u] = MP.fdot(cols[u], cols[v])
    return A


def _eigen(A):
    """(eigenvalues ascending, eigenvectors as lists) of the symmetric A, every pair checked to a residual under 1e-40
    of the largest eigenvalue."""
    w, Q = MP.eigsy(A)
    w = [w[k] for k in range(9)]
    vecs = [[Q[i, k] for i in range(9)] for k in range(9)]
    scale = max(abs(x) for x in w)
    for lam, v in zip(w, vecs):
        res = _norm([_dot([A[i, j] for j in range(9)], v) - lam * v[i] for i in range(9)]) / scale
        assert res < RES_MAX, res
    return w, vecs


def _t3(sc, cx, cy):
    return [sc, mpf(0), -sc * cx, mpf(0), sc, -sc * cy, mpf(0), mpf(0), mpf(1)]


def _t3_inv(sc, cx, cy):
    return [1 / sc, mpf(0), cx, mpf(0), 1 / sc, cy, mpf(0), mpf(0), mpf(1)]


def _normalised(vals, T6):
    s1, x1, y1, s2, x2, y2 = T6
    return [((vals[4 * m] - x1) * s1, (vals[4 * m + 1] - y1) * s1, (vals[4 * m + 2] - x2) * s2, (vals[4 * m + 3] - y2) * s2)
            for m in range(len(vals) // 4)]


def _fund_solve(vals, T6, pick=0, rank2=True, swap=False):
    """The unit 9-vector F of the masked matches vals (flat, x1 y1 x2 y2) under T6.  pick, rank2 and swap are the
    mutations of test_refit_truth.py: another eigenvector, no rank-2 step, T1 and T2 exchanged in the de-normalisation."""
    fn = _eigen(_normal(_epi_rows(_normalised(vals, T6))))[1][pick]
    if rank2:
        U, S, V = MP.svd_r(MP.matrix([fn[0:3], fn[3:6], fn[6:9]]))    # S descending, fn = U diag(S) V
        fn = [sum(U[i, k] * S[k] * V[k, j] for k in range(2)) for i in range(3) for j in range(3)]
    T1, T2 = _t3(*T6[:3]), _t3(*T6[3:])
    if swap:
        T1, T2 = T2, T1
    return _unit(_mat(_tr(T2), _mat(fn, T1)))


def _hom_solve(vals, T6, pick=0, rank2=True, swap=False):
    hn = _eigen(_normal(_hom_rows(_normalised(vals, T6))))[1][pick]
    a, b = (T6[3:], T6[:3]) if not swap else (T6[:3], T6[3:])
    return _unit(_mat(_t3_inv(*a), _mat(hn, _t3(*b))))


def _masked_pixels(seg, mask):
    a, b = seg.data
    idx = np.flatnonzero(np.asarray(mask, bool))
    return _mp(np.c_[np.asarray(a, np.float64)[idx], np.asarray(b, np.float64)[idx]].ravel())


class Truth:
    """roots [n][D] (mp lists; one root except for E), roots_ld, kappa [n], unit [n] (the judge's unit), seconds."""

    def __init__(self, roots, kappa, extent=1.0, floor=0.0):
        self.roots_mp = roots
        self.roots = np.stack([_to_ld(r) for r in roots])
        self.kappa = np.asarray(kappa, np.float64)
        self.extent = extent
        self.unit = self.kappa * U53 + floor


def truth_model9(stage, seg, mask, T6, **mutation):
    """Fundamental or homography: one root."""
    solve = _fund_solve if stage == "fundamental" else _hom_solve
    vals, T = _masked_pixels(seg, mask), _mp(T6)
    root = solve(vals, T, **mutation)
    worst = mpf(0)
    for signs in ([] if mutation else _draws(len(vals) + 6)):
        v2 = _perturb(vals + T, signs)
        worst = max(worst, _sine(root, solve(v2[:-6], v2[-6:])))
    return Truth([root], [float(worst) / U40])


# ------------------------------------------------------------------------------------------------- essential
def _ess_subspace(vals, k4, shift=0):
    fx, fy, cx, cy = k4
    pts = [((vals[4 * m] - cx) / fx, (vals[4 * m + 1] - cy) / fy, (vals[4 * m + 2] - cx) / fx, (vals[4 * m + 3] - cy) / fy)
           for m in range(len(vals) // 4)]
    vecs = _eigen(_normal(_epi_rows(pts)))[1]
    return vecs[:3] + [vecs[3 + shift]]


def _span_next_to(N2, N):
    """An orthonormal basis of span(N2) next to the four vectors N: their projections, by Gram-Schmidt."""
    out = []
    for v in N:
        w = [mpf(0)] * 9
        for n in N2:
            c = _dot(n, v)
            w = [x + c * y for x, y in zip(w, n)]
        for o in out:
            c = _dot(o, w)
            w = [x - c * y for x, y in zip(w, o)]
        out.append(_unit(w))
    return out


def truth_essential(seg, mask, shift=0, condition=True):
    """All real E of the four-dimensional subspace; shift = 1 is the mutation that takes the fifth eigenvector for the
    fourth."""
    vals, k4 = _masked_pixels(seg, mask), _mp(seg.k4)
    N = _ess_subspace(vals, k4, shift)
    N0 = np.array([[float(x) for x in v] for v in N])
    found = [g[0] for g in (_ess_polish(N, _mp(q)) for q in _ess_seeds(N0)) if g is not None]
    qs = _merge(found, lambda p, q: _sine(_ess_model(N, p), _ess_model(N, q)))
    roots = [_ess_model(N, q) for q in qs]
    kappa = [mpf(0)] * len(roots)
    for signs in (_draws(len(vals) + 4) if condition and not shift else []):
        v2 = _perturb(vals + k4, signs)
        N2 = _span_next_to(_ess_subspace(v2[:-4], v2[-4:]), N)
        for k, q in enumerate(qs):
            got = _ess_polish(N2, q)
            kappa[k] = max(kappa[k], _sine(roots[k], _ess_model(N2, got[0])) if got else mpf(1))
    return Truth(roots, [float(k) / U40 for k in kappa])


# ------------------------------------------------------------------------------------------------------- pnp
def _pnp_gradient(Rt, X, uv, k4):
    """The gradient [6] (mp) of half the summed squared reprojection error at w = 0 of R <- exp([w]x) R, t <- t + d:
    sum over the points of (d pixel / d y [-[q]x | I])^T residual, q = R X, y = q + t."""
    fx, fy, cx, cy = k4
    g = [mpf(0)] * 6
    R = [Rt[0:3], Rt[4:7], Rt[8:11]]
    t = [Rt[3], Rt[7], Rt[11]]
    for m in range(len(uv) // 2):
        P = X[3 * m:3 * m + 3]
        q0, q1, q2 = _dot(R[0], P), _dot(R[1], P), _dot(R[2], P)
        y0, y1, iz = q0 + t[0], q1 + t[1], 1 / (q2 + t[2])
        ru, rv = fx * y0 * iz + cx - uv[2 * m], fy * y1 * iz + cy - uv[2 * m + 1]
        a0, c1 = fx * iz, fy * iz
        a2, c2 = -a0 * y0 * iz, -c1 * y1 * iz
        du = (a0 * ru, c1 * rv, a2 * ru + c2 * rv)                        # (d pixel / d y)^T residual
        g[0] += q1 * du[2] - q2 * du[1]                                   # q x du
        g[1] += q2 * du[0] - q0 * du[2]
        g[2] += q0 * du[1] - q1 * du[0]
        g[3] += du[0]
        g[4] += du[1]
        g[5] += du[2]
    return g


def _mp_exp(w):
    """exp([w]x) row-major [9]: I + sin(th)/th [w]x + 2 sin^2(th/2)/th^2 [w]x^2 (no cancellation at small th)."""
    th = _norm(w)
    if th == 0:
        return [mpf(1), mpf(0), mpf(0), mpf(0), mpf(1), mpf(0), mpf(0), mpf(0), mpf(1)]
    a, b = MP.sin(th) / th, 2 * MP.sin(th / 2) ** 2 / (th * th)
    Kx = [mpf(0), -w[2], w[1], w[2], mpf(0), -w[0], -w[1], w[0], mpf(0)]
    K2 = _mat(Kx, Kx)
    I = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    return [i + a * x + b * y for i, x, y in zip(I, Kx, K2)]


def _pnp_moved(Rt, d):
    R = _mat(_mp_exp(d[:3]), [Rt[0], Rt[1], Rt[2], Rt[4], Rt[5], Rt[6], Rt[8], Rt[9], Rt[10]])
    return [R[0], R[1], R[2], Rt[3] + d[3], R[3], R[4], R[5], Rt[7] + d[4], R[6], R[7], R[8], Rt[11] + d[5]]


def _pnp_newton(Rt, Hinv, X, uv, k4, maxit=40):
    for _ in range(maxit):
        g = _pnp_gradient(Rt, X, uv, k4)
        if _norm(g) < RES_MAX:
            return Rt
        Rt = _pnp_moved(Rt, [-_dot(row, g) for row in Hinv])
    raise AssertionError("the PnP truth's Newton iteration did not reach a gradient under 1e-40")


def _np_gradient(K, Rt, X, uv):
    return pr.local_sums(K, Rt[:, :3], Rt[:, 3], X, uv)[1]


def truth_pnp(seg, mask, start):
    """start: a pose [12] near the optimum (the winner, or a refit of it); pnp_reference.refit polishes it first."""
    mask = np.asarray(mask, bool)
    Xf, uvf = (v[mask] for v in _f64(seg.data))
    K = pr.k_matrix(seg.k4)
    s = np.asarray(start, np.float64).reshape(3, 4)
    R0, t0 = pr.refit(K, s[:, :3], s[:, 3], Xf, uvf)
    seed = np.c_[R0, t0]
    # the Jacobian of the local gradient at the seed by central differences in float64, held fixed: each Newton step
    # then leaves about 1e-9 of the error
    Hm, h = np.zeros((6, 6)), 1e-5
    for j in range(6):
        d = np.zeros(6)
        d[j] = h
        plus = np.c_[pr._exp_so3(d[:3]) @ R0, t0 + d[3:]]
        minus = np.c_[pr._exp_so3(-d[:3]) @ R0, t0 - d[3:]]
        Hm[:, j] = (_np_gradient(K, plus, Xf, uvf) - _np_gradient(K, minus, Xf, uvf)) / (2 * h)
    Hinv = [_mp(r) for r in np.linalg.inv(0.5 * (Hm + Hm.T))]
    Rt = _mp(seed.ravel())
    R = [Rt[0], Rt[1], Rt[2], Rt[4], Rt[5], Rt[6], Rt[8], Rt[9], Rt[10]]
    for _ in range(5):                                                    # polar iteration: R <- (R + R^-T) / 2
        c = _cof(R)
        det = _dot(c[:3], R[:3])
        R = [(x + y / det) / 2 for x, y in zip(R, c)]
    Rt = [R[0], R[1], R[2], Rt[3], R[3], R[4], R[5], Rt[7], R[6], R[7], R[8], Rt[11]]
    X, uv, k4 = _mp(Xf.ravel()), _mp(uvf.ravel()), _mp(seg.k4)
    root = _pnp_newton(Rt, Hinv, X, uv, k4)
    extent = mpf(float(np.linalg.norm(Xf - Xf.mean(0), axis=1).max()))
    worst = mpf(0)
    for signs in _draws(len(X) + len(uv) + 4):
        v2 = _perturb(X + uv + k4, signs)
        got = _pnp_newton(root, Hinv, v2[:len(X)], v2[len(X):-4], v2[-4:])
        worst = max(worst, _rt_distance(got, root, extent))
    r = [float(x) for x in root]
    v = np.array([r[9] - r[6], r[2] - r[8], r[4] - r[1]])
    ang = np.arctan2(0.5 * np.linalg.norm(v), 0.5 * (r[0] + r[5] + r[10] - 1.0))
    xn = np.sqrt(ang * ang + r[3] ** 2 + r[7] ** 2 + r[11] ** 2)
    return Truth([root], [float(worst) / U40], float(extent), 1e-12 * (1.0 + xn))


# ---------------------------------------------------------------------------------------------------- hartley
def _hartley_solve(vals):
    """vals: the finite matches, flat (x1 y1 x2 y2), mp -> [sc1, cx1, cy1, sc2, cx2, cy2]."""
    n = len(vals) // 4
    out = []
    for o in (0, 2):
        xs, ys = vals[o::4], vals[o + 1::4]
        cx, cy = MP.fsum(xs) / n, MP.fsum(ys) / n
        d = MP.fsum(MP.sqrt((x - cx) ** 2 + (y - cy) ** 2) for x, y in zip(xs, ys)) / n
        out += [MP.sqrt(2) / d if d > 0 else mpf(1), cx, cy]
    return out


def _hartley_distance(T, ref):
    worst = mpf(0)
    for o in (0, 3):
        dc = MP.sqrt((T[o + 1] - ref[o + 1]) ** 2 + (T[o + 2] - ref[o + 2]) ** 2) * ref[o] / MP.sqrt(2)
        worst = max(worst, abs(T[o] - ref[o]) / ref[o], dc)
    return worst


def truth_hartley(seg):
    """(T [6] mp, kappa) over the finite matches of the segment (at least two distinct ones)."""
    a, b = _f64(seg.data)
    fin = np.isfinite(a).all(1) & np.isfinite(b).all(1)
    vals = _mp(np.c_[a[fin], b[fin]].ravel())
    T = _hartley_solve(vals)
    worst = mpf(0)
    for signs in _draws(len(vals)):
        worst = max(worst, _hartley_distance(_hartley_solve(_perturb(vals, signs)), T))
    return T, float(worst) / U40


def hartley_ratio(T6, truth):
    T, kappa = truth
    return float(_hartley_distance(_mp(T6), T)) / (kappa * U53)


# ------------------------------------------------------------------------------------------------- the judge
@functools.lru_cache(maxsize=None)
def _truth_cached(stage, s, mask_bytes, extra_bytes):
    seg = segments(stage)[s]
    mask = np.frombuffer(mask_bytes, np.uint8).astype(bool)
    extra = np.frombuffer(extra_bytes, np.float64)
    t0 = time.process_time()
    if stage in ("fundamental", "homography"):
        tr = truth_model9(stage, seg, mask, extra)
    elif stage == "essential":
        tr = truth_essential(seg, mask)
    else:
        tr = truth_pnp(seg, mask, extra)
    tr.seconds = time.process_time() - t0
    return tr


def truth(stage, s, mask, extra=()):
    """The truth of segment s over `mask`; extra: T6 for F and H, a start pose [12] for PnP.  Computed once per distinct
    input, never modified."""
    return _truth_cached(stage, s, np.asarray(mask, bool).astype(np.uint8).tobytes(), np.asarray(extra, np.float64).tobytes())


def distances(stage, model, tr):
    """[n] float64: the distance of one model to each root of the truth, taken in long double."""
    c = np.asarray(model, np.float64).ravel().astype(np.longdouble)
    r = tr.roots
    if stage == "pnp":
        rot = [0, 1, 2, 4, 5, 6, 8, 9, 10]
        dR = np.sqrt(((c[rot] - r[:, rot]) ** 2).sum(-1))
        dt = np.sqrt(((c[3::4] - r[:, 3::4]) ** 2).sum(-1))
        nt = np.maximum(np.sqrt((r[:, 3::4] ** 2).sum(-1)), np.longdouble(tr.extent))
        return np.maximum(dR, dt / nt).astype(np.float64)
    c = c / np.sqrt((c * c).sum())
    dots = r @ c
    perp = c[None] - dots[:, None] * r
    return np.sqrt((perp * perp).sum(-1)).astype(np.float64)


def ratios(stage, model, tr):
    """[n]: distance / unit against every root."""
    return distances(stage, model, tr) / tr.unit


def root_counts(stage, tr, seg, factor=1.0):
    """The inlier count of every truth root over the whole segment, at threshold x factor."""
    with np.errstate(invalid="ignore"):
        return np.array([int((error_ratio(stage, r.astype(np.float64), seg) <= factor * factor).sum()) for r in tr.roots])


# ------------------------------------------------------------------------------------- the dropped-refit search
def find_dropped(stage):
    """The first seed of 0 .. 499 (noise 1.5 px, M = 40, outlier share 0.3) whose reference refit counts fewer matches than
    the winner, with no squared error of either model within 1e-6 (relative) of threshold^2; None if there is none."""
    size, least = SAMPLE[stage]
    at = len(SIZES) + 3                                                   # the segment's place in the call
    smp = ransac_reference.draw_samples(SEED, at, 40, N_HYP, size, least)
    for seed in range(500):
        seg = Segment("", "dropped", _scene(stage, seed, 40, 0.3, noise=1.5))
        a, b = _f64(seg.data)
        K = pr.k_matrix(seg.k4)
        with np.errstate(all="ignore"):
            if stage == "fundamental":
                r = fr.ransac(a, b, smp, THR[stage])
                m = r["F"]
            elif stage == "homography":
                r = hr.ransac(a, b, smp, THR[stage])
                m = r["H"]
            elif stage == "essential":
                r = er.ransac(a, b, K, smp, THR[stage])
                m = r["E"]
            else:
                r = pr.ransac(a, b, K, smp, THR[stage])
                m = None if r["R"] is None else np.c_[r["R"], r["t"]]
        if m is None or r["n_inliers"] < GATE[stage]:
            continue
        got, _ = reference_refit(stage, seg, r["mask"], hartley6(a, b), m)
        if got is not None and int(rule_mask(stage, got, seg).sum()) < r["n_inliers"] and not band(stage, got, seg, 1e-6).any() \
                and not band(stage, np.ravel(m), seg, 1e-6).any():
            return seed
    return None
