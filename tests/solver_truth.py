"""A multi-precision truth for the four minimal problems behind the batched RANSAC stages, and the judge that holds a
solver's models to it (tests/test_solver_truth.py on the CPU, tests/test_solver_truth_gpu.py on the device).

The truth solves each minimal PROBLEM in mpmath at 60 digits; it replays no kernel.  Inputs are taken exactly: float32
pixels, float64 world points and K are binary rationals.

    homography   the null vector of the 8 x 9 system in pixel coordinates (no Hartley transform)
    fundamental  the null space of the 7 x 9 system in pixel coordinates, the real roots of det(a F1 + F2): all real F
    essential    all real E = sum q_k N_k (N the null space of the 5 x 9 system of the normalised points, |q| = 1) with
                 det E = 0 and 2 E E^T E - tr(E E^T) E = 0
    p3p          all depth triples l > 0 of |l_i f_i - l_j f_j|^2 = |P_i - P_j|^2, then [R|t]

Route.  A float64 seed, then the exact step in mpmath: null spaces are a NumPy basis projected onto the null space by
one 60-digit solve; the cubic of F is expanded by polynomial products of the linear entries and solved by
mp.polyroots, the count of its real roots decided by the discriminant; the seeds of E hide one unknown of the ten
constraints - polynomials kept as arrays indexed by exponent, no monomial order - take det C(z) at the 11th roots of
unity, and read (x, y) off the null vector of C(z), twice, the second time in a rotated basis; the seeds of P3P eliminate
one depth ratio from two conics by a numeric resultant, once per cyclic order of the points.  Every root is then
polished by Newton (Gauss-Newton for E's ten equations) in mpmath on the defining equations until the residual is
below 1e-40, and roots closer than 1e-25 are merged.  Nothing here is shared with the *_solve.h headers or with
essential_reference's product tables.

Completeness.  A candidate that matches no listed root is polished on the same equations (Sample.guard): if it converges
to a root the truth does not list, TruthIncomplete is raised - a failure of the truth, not of the candidate.  (A
candidate within a listed root's bound lands on that root; only the unmatched ones need the polish.)

Condition.  kappa of a root: all inputs of the sample (pixels, world points, K) multiplied at once by 1 +- 2^-40,
independent signs, three fixed-seed draws; the root re-polished; kappa = max |delta model| / 2^-40.

Distances.  F, H, E: the sine of the angle between the 9-vectors.  [R|t]: max(|R - R*|_F, |t - t*| / max(|t*|, the
longest side of the world triangle)).

The judge.  Under a constant C a truth root with C kappa 2^-53 > 1e-6 is left out: neither required nor forbidden, and
a candidate within that distance of it is not spurious.  Every other root must be the nearest root of exactly one
candidate, within C kappa 2^-53; every candidate must lie within the bound of a root.  C is C_REF, the worst ratio
error / (kappa 2^-53) of the NumPy references over the sample sets below, for the references themselves, and 8 x C_REF for
the host builds of the headers and for the device (MARGIN).

Measured (the sample sets of scenes(), seed SEED; ratios are error / (kappa 2^-53); host = tests/native/*_solve_check.cpp
by g++ -ffp-contract=off / -ffp-contract=fast -mfma; device = MI355X; left out = share of the roots outside the
degenerate scenes whose bound at 8 x C_REF passes 1e-6; time = CPU seconds of truth(solver) here):

    solver        samples  roots   C_REF   bound 8 x C_REF   worst host off / fast   worst device   left out   time
    fundamental   160      404     109.2   873.6             21.7 / 6.2              1.63           0.56 %     5 s
    homography    240      240     3.68    29.44             2.13 / 3.57             3.53           0 %        3 s
    essential     128      602     93.5    748               6.9 / 4.42              3.08           0 %        18 s
    pnp           120      278     5.70    45.6              4.92 / 3.06             4.14           0.90 %     3 s

C_REF of the fundamental and essential references is large because kappa is often below 1 there (the sine between
9-vectors in pixels is ruled by the few large entries), while a float64 model cannot be nearer than 2^-53 or so.
The device's fundamental and homography figures are those of the one stored model per hypothesis.  P3P's left-out
share is one sample of the near-collinear scene: its triangle is flattened to a sine of 1.5e-10, the float32 pixels
leave it a complex pair of depth triples 1e-7 off the real axis and no real root, and the device returns the pair's
two near-roots (residual 1e-15 of the squared side) - such a sample, Newton stalling below a residual of 1e-12, counts
as undetermined and nothing in it is judged.

What the bounds found when they were first run: pnp_solve.h took its Newton residuals as l_i^2 + l_j^2 - 2 b_ij l_i l_j
- a_ij, which cancels from the size of the squared depths to that of the squared side: worst host ratio 729 (errors
of 2e-10 at kappa 3e3), 4.92 with the residuals taken from the difference vectors.  essential_solve.h's two
Gauss-Newton steps left one candidate of 602 at 6.5e-11 (ratio 1.6e4, in the -ffp-contract=fast build only); a third
step brings it to 1.1.  essential_reference.from_basis had no polish at all (ratios up to 2.8e8, which would have been
its C_REF): it now takes step 7's Gauss-Newton too, by np.linalg.pinv.
"""
import functools
import time

import mpmath
import numpy as np

import essential_reference as er
import fundamental_reference as fr
import homography_reference as hr
import pnp_reference as pr
import ransac_reference

MP = mpmath.mp.clone()
MP.dps = 60
mpf = MP.mpf
RES_MAX = mpf("1e-40")
MERGE = mpf("1e-25")
U40, U53 = 2.0 ** -40, 2.0 ** -53
LEFT_OUT = 1e-6
MARGIN = 8.0
SEED = 11
ROOT_CAP = {"fundamental": 3, "homography": 1, "essential": 10, "pnp": 4}
# the worst ratio error / (kappa 2^-53) of the NumPy references, measured by measure_c() - see the table above
C_REF = {"fundamental": 109.2, "homography": 3.68, "essential": 93.5, "pnp": 5.70}


class TruthIncomplete(AssertionError):
    """A candidate polished onto a root of the problem that the truth does not list."""


# ------------------------------------------------------------------------------------------ small mp algebra
def _mp(v):
    return [mpf(float(x)) if not isinstance(x, mpf) else x for x in v]


def _solve(A, B):
    """A [n][n], B [n][m] (lists of mpf) -> X [n][m]: Gaussian elimination with row pivoting."""
    n, m = len(A), len(B[0])
    M = [list(A[i]) + list(B[i]) for i in range(n)]
    for c in range(n):
        p = max(range(c, n), key=lambda r: abs(M[r][c]))
        M[c], M[p] = M[p], M[c]
        piv = M[c][c]
        for r in range(c + 1, n):
            f = M[r][c] / piv
            if f:
                Mr, Mc = M[r], M[c]
                for k in range(c, n + m):
                    Mr[k] -= f * Mc[k]
    X = [[mpf(0)] * m for _ in range(n)]
    for r in range(n - 1, -1, -1):
        for k in range(m):
            s = M[r][n + k]
            for c in range(r + 1, n):
                s -= M[r][c] * X[c][k]
            X[r][k] = s / M[r][r]
    return X


def _dot(a, b):
    return MP.fdot(a, b)


def _norm(a):
    return MP.sqrt(_dot(a, a))


def _unit(a):
    n = _norm(a)
    return [x / n for x in a]


def _sine(a, b):
    """The sine of the angle between two vectors (the sign of either is free)."""
    a, b = _unit(a), _unit(b)
    c = _dot(a, b)
    return _norm([x - c * y for x, y in zip(a, b)])


def _project_null(A, vecs):
    """vecs (a list of 9-vectors) moved onto the null space of A [r][9] by one solve: v - A^T (A A^T)^-1 A v."""
    G = [[_dot(ri, rj) for rj in A] for ri in A]
    rhs = [[_dot(ri, v) for v in vecs] for ri in A]
    Y = _solve(G, rhs)
    out = []
    for k, v in enumerate(vecs):
        w = list(v)
        for i, ri in enumerate(A):
            y = Y[i][k]
            w = [wj - y * rj for wj, rj in zip(w, ri)]
        out.append(w)
    return out


def _null_residual(A, v):
    nv = _norm(v)
    return max(abs(_dot(r, v)) / (_norm(r) * nv) for r in A)


def _to_ld(v):
    """mpf list -> longdouble array, from the two leading float64 parts."""
    hi = [float(x) for x in v]
    lo = [float(x - mpf(h)) for x, h in zip(v, hi)]
    return np.asarray(hi, np.longdouble) + np.asarray(lo, np.longdouble)


def _draws(n):
    """Three fixed-seed draws of n signs: the inputs' relative perturbations are sign * 2^-40."""
    return [np.random.default_rng(101 + d).choice([-1.0, 1.0], size=n) for d in range(3)]


def _perturb(vals, signs):
    return [v * (1 + mpf(float(s)) * mpf(U40)) for v, s in zip(vals, signs)]


def _merge(roots, dist):
    out = []
    for r in roots:
        if all(dist(r, o) > MERGE for o in out):
            out.append(r)
    return out


class Sample:
    """One sample's truth: `roots` [n][D] longdouble (unit 9-vectors, or [R|t] row-major), `kappa` [n], `residual` (the
    largest defining-equation residual over the roots), `extent` (P3P: the longest side of the world triangle) and
    `guard(candidate)`: None if the polished candidate is no root, else the index of the listed root it lands on
    (TruthIncomplete if it lands on an unlisted one)."""

    def __init__(self, roots_mp, kappa, residual, guard, extent=1.0, undetermined=False):
        self.roots_mp = roots_mp
        self.undetermined = undetermined       # rank-deficient, or within 1e-6 of a double root (P3P): nothing is judged
        D = len(roots_mp[0]) if roots_mp else 0
        self.roots = np.stack([_to_ld(r) for r in roots_mp]) if roots_mp else np.zeros((0, D), np.longdouble)
        self.kappa = np.asarray(kappa, np.float64)
        self.residual = residual
        self.guard = guard
        self.extent = extent


# ------------------------------------------------------------------------------------------------ homography
def _hom_rows(px):
    rows = []
    for x, y, u, v in px:
        rows.append([x, y, mpf(1), mpf(0), mpf(0), mpf(0), -u * x, -u * y, -u])
        rows.append([mpf(0), mpf(0), mpf(0), x, y, mpf(1), -v * x, -v * y, -v])
    return rows


def truth_homography(px):
    """px [4][4] = (x, y, u, v) in pixels (float32 values, or mpf).  One root."""
    vals = _mp(np.asarray(px, object).ravel())
    A = _hom_rows([vals[4 * m:4 * m + 4] for m in range(4)])
    seed = np.linalg.svd(np.array([[float(a) for a in r] for r in A]))[2][8]
    h = _unit(_project_null(A, [_mp(seed)])[0])
    worst = mpf(0)
    for signs in _draws(16):
        v2 = _perturb(vals, signs)
        h2 = _project_null(_hom_rows([v2[4 * m:4 * m + 4] for m in range(4)]), [h])[0]
        worst = max(worst, _sine(h, h2))
    return Sample([h], [float(worst) / U40], _null_residual(A, h), lambda cand: 0)


# ----------------------------------------------------------------------------------------------- fundamental
def _epi_rows(pts):
    return [[c * a, c * b, c, d * a, d * b, d, a, b, mpf(1)] for a, b, c, d in pts]


def _padd(p, q):
    n = max(len(p), len(q))
    return [(p[i] if i < len(p) else 0) + (q[i] if i < len(q) else 0) for i in range(n)]


def _pmul(p, q):
    out = [mpf(0)] * (len(p) + len(q) - 1)
    for i, a in enumerate(p):
        for j, b in enumerate(q):
            out[i + j] += a * b
    return out


def _det_pencil(F1, F2):
    """Coefficients c[0..3] (ascending in a) of det(a F1 + F2), by products of the linear entries."""
    e = lambda i, j: [F2[3 * i + j], F1[3 * i + j]]
    neg = lambda p: [-x for x in p]
    m = lambda i, j, k, l: _padd(_pmul(e(1, i), e(2, j)), neg(_pmul(e(1, k), e(2, l))))
    return _padd(_padd(_pmul(e(0, 0), m(1, 2, 2, 1)), neg(_pmul(e(0, 1), m(0, 2, 2, 0)))), _pmul(e(0, 2), m(0, 1, 1, 0)))


def _poly_newton(c, a):
    """Newton on the polynomial c (ascending) from a, until the step no longer moves a; returns (a, |p(a)| scaled)."""
    for _ in range(200):
        p = dp = mpf(0)
        for ck in reversed(c):
            dp = dp * a + p
            p = p * a + ck
        if dp == 0:
            break
        step = p / dp
        a -= step
        if abs(step) <= mpf("1e-58") * (1 + abs(a)):
            break
    p, scale = mpf(0), mpf(0)
    for k, ck in enumerate(c):
        p += ck * a ** k
        scale += abs(ck) * abs(a) ** k
    return a, abs(p) / scale


def _fund_model(F1, F2, a):
    return _unit([a * x + y for x, y in zip(F1, F2)])


def _fund_basis(A, near):
    """An orthogonal pair spanning the null space of A, next to the pair `near`."""
    F1, F2 = _project_null(A, near)
    F1 = _unit(F1)
    c = _dot(F1, F2)
    return F1, _unit([y - c * x for x, y in zip(F1, F2)])


def truth_fundamental(pts):
    """pts [7][4] = (x1, y1, x2, y2) in pixels.  Up to three roots."""
    vals = _mp(np.asarray(pts, object).ravel())
    A = _epi_rows([vals[4 * m:4 * m + 4] for m in range(7)])
    Vt = np.linalg.svd(np.array([[float(a) for a in r] for r in A]))[2]
    F1, F2 = _fund_basis(A, [_mp(Vt[7]), _mp(Vt[8])])
    c = _det_pencil(F1, F2)
    c0, c1, c2, c3 = c
    disc = 18 * c3 * c2 * c1 * c0 - 4 * c2 ** 3 * c0 + c2 * c2 * c1 * c1 - 4 * c3 * c1 ** 3 - 27 * c3 * c3 * c0 * c0
    z = sorted(MP.polyroots(c[::-1], maxsteps=2000, extraprec=1000), key=lambda r: abs(MP.im(r)))
    params, residual = [], _null_residual(A, F1)
    for r in z[:3 if disc > 0 else 1]:
        a, res = _poly_newton(c, MP.re(r))
        params.append(a)
        residual = max(residual, res)
    params = sorted(_merge(params, lambda p, q: _sine(_fund_model(F1, F2, p), _fund_model(F1, F2, q))))
    roots = [_fund_model(F1, F2, a) for a in params]
    kappa = [mpf(0)] * len(roots)
    for signs in _draws(28):
        v2 = _perturb(vals, signs)
        A2 = _epi_rows([v2[4 * m:4 * m + 4] for m in range(7)])
        G1, G2 = _fund_basis(A2, [F1, F2])
        c2_ = _det_pencil(G1, G2)
        for k, a in enumerate(params):
            a2, _ = _poly_newton(c2_, a)
            kappa[k] = max(kappa[k], _sine(roots[k], _fund_model(G1, G2, a2)))

    def guard(cand):
        f = _mp(np.asarray(cand, np.float64).ravel())
        x, y = _dot(f, F1), _dot(f, F2)
        if y == 0:
            return None
        a, res = _poly_newton(c, x / y)
        if not res < RES_MAX:
            return None
        m = _fund_model(F1, F2, a)
        for k, r in enumerate(roots):
            if _sine(m, r) <= MERGE:
                return k
        raise TruthIncomplete("a fundamental candidate polished onto an unlisted root")
    return Sample(roots, [float(k) / U40 for k in kappa], residual, guard)


# ------------------------------------------------------------------------------------------------- essential
def _mat(A, B):
    return [A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j] for i in range(3) for j in range(3)]


def _tr(A):
    return [A[0], A[3], A[6], A[1], A[4], A[7], A[2], A[5], A[8]]


def _cof(E):
    a, b, c, d, e, f, g, h, i = E
    return [e * i - f * h, f * g - d * i, d * h - e * g, c * h - b * i, a * i - c * g, b * g - a * h,
            b * f - c * e, c * d - a * f, a * e - b * d]


def _ess_residual(N, q):
    """The ten constraints at E = sum q_k N_k, and |q|^2 - 1: residuals [11], and the parts the Jacobian shares."""
    E = [sum(q[k] * N[k][e] for k in range(4)) for e in range(9)]
    EEt = _mat(E, _tr(E))
    t = EEt[0] + EEt[4] + EEt[8]
    EEtE = _mat(EEt, E)
    cof = _cof(E)
    r = [2 * x - t * y for x, y in zip(EEtE, E)] + [_dot(cof[:3], E[:3]), _dot(q, q) - 1]
    return r, (E, EEt, t, cof)


def _ess_jacobian(N, q, parts):
    """[11][4]: along N_k, 2 (B E^T E + E B^T E + E E^T B) - 2 tr(B E^T) E - tr(E E^T) B, tr(cof(E)^T B) and 2 q_k."""
    E, EEt, t, cof = parts
    EtE = _mat(_tr(E), E)
    J = [[None] * 4 for _ in range(11)]
    for k in range(4):
        B = N[k]
        d = [x + y + z for x, y, z in zip(_mat(B, EtE), _mat(_mat(E, _tr(B)), E), _mat(EEt, B))]
        tb = 2 * _dot(B, E)
        for e in range(9):
            J[e][k] = 2 * d[e] - tb * E[e] - t * B[e]
        J[9][k] = _dot(cof, B)
        J[10][k] = 2 * q[k]
    return J


def _ess_polish(N, q, maxit=16):
    """Gauss-Newton from q, the Jacobian kept while the residual falls by 1e-3 a step and formed again when it does
    not; (q, residual) with the residual under RES_MAX, or None."""
    q = list(q)
    J = JtJ = None
    last = None
    for _ in range(maxit):
        r, parts = _ess_residual(N, q)
        res = max(abs(x) for x in r)
        if res < RES_MAX:
            return q, res
        if J is None or not res < last * mpf("1e-3"):
            J = _ess_jacobian(N, q, parts)
            cols = [[J[e][a] for e in range(11)] for a in range(4)]
            JtJ = [[_dot(cols[a], cols[b]) for b in range(4)] for a in range(4)]
        last = res
        try:
            step = _solve(JtJ, [[_dot(cols[a], r)] for a in range(4)])
        except ZeroDivisionError:
            return None
        q = [x - s[0] for x, s in zip(q, step)]
        if max(abs(x) for x in q) > 10:
            return None
    return None


_EXP2 = [(i, j) for i in range(4) for j in range(4 - i)]                 # the ten (x, y) exponents of degree <= 3
_ROT4 = np.linalg.qr(np.random.default_rng(4).standard_normal((4, 4)))[0]


def _p3mul(A, B):
    """Product of two polynomials in three unknowns, kept as [4,4,4] arrays indexed by exponent (total degree <= 3)."""
    out = np.zeros((4, 4, 4))
    for i, j, k in np.argwhere(B != 0):
        out[i:, j:, k:] += B[i, j, k] * A[:4 - i, :4 - j, :4 - k]
    return out


def _ess_seeds_one(N):
    """float64: N [4,9] -> q [n,4] (not normalised), the real solutions with q[3] = 1, hiding q[2]."""
    L = np.zeros((3, 3, 4, 4, 4))
    L[:, :, 1, 0, 0], L[:, :, 0, 1, 0], L[:, :, 0, 0, 1], L[:, :, 0, 0, 0] = (N[k].reshape(3, 3) for k in range(4))
    EEt = [[sum(_p3mul(L[i, k], L[j, k]) for k in range(3)) for j in range(3)] for i in range(3)]
    t = EEt[0][0] + EEt[1][1] + EEt[2][2]
    eqs = [sum(_p3mul(2 * EEt[i][k] - (t if i == k else 0), L[k, j]) for k in range(3)) for i in range(3) for j in range(3)]
    minor = lambda a, b: _p3mul(L[1, a], L[2, b]) - _p3mul(L[1, b], L[2, a])
    eqs.append(_p3mul(minor(1, 2), L[0, 0]) - _p3mul(minor(0, 2), L[0, 1]) + _p3mul(minor(0, 1), L[0, 2]))
    C = np.array([[[P[i, j, k] for (i, j) in _EXP2] for P in eqs] for k in range(4)])          # [4][10][10] by power of z
    C = C / np.abs(C).max()
    w = np.exp(2j * np.pi * np.arange(11) / 11)
    dets = np.linalg.det(sum(C[k][None] * (w ** k)[:, None, None] for k in range(4)))
    co = np.fft.fft(dets) / 11                                           # ascending coefficients of det C(z)
    if not np.isfinite(co).all() or np.abs(co).max() == 0:
        return np.zeros((0, 4))
    out = []
    for z in np.roots(co[::-1]):
        if abs(z.imag) > 1e-4 * (1 + abs(z.real)):
            continue
        z = z.real
        v = np.linalg.svd(sum(C[k] * z ** k for k in range(4)))[2][-1]
        one = v[_EXP2.index((0, 0))]
        if abs(one) < 1e-9:
            continue
        out.append([v[_EXP2.index((1, 0))] / one, v[_EXP2.index((0, 1))] / one, z, 1.0])
    return np.array(out).reshape(-1, 4)


def _ess_seeds(N):
    a = _ess_seeds_one(N)
    b = _ess_seeds_one(_ROT4 @ N) @ _ROT4                                # q' N' = q' Q N: q = q' Q
    q = np.concatenate([a, b])
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    keep = []                                                            # a root both runs found is polished once
    for v in q:
        if all(min(np.abs(v - o).max(), np.abs(v + o).max()) > 1e-9 for o in keep):
            keep.append(v)
    return np.array(keep).reshape(-1, 4)


def _ess_rows(vals, k4):
    fx, fy, cx, cy = k4
    pts = [((vals[4 * m] - cx) / fx, (vals[4 * m + 1] - cy) / fy, (vals[4 * m + 2] - cx) / fx, (vals[4 * m + 3] - cy) / fy)
           for m in range(5)]
    return _epi_rows(pts)


def _ess_basis(A, near):
    """An orthonormal basis (Gram-Schmidt) of the null space of A [5][9], next to the four vectors `near`."""
    out = []
    for v in _project_null(A, near):
        for o in out:
            c = _dot(o, v)
            v = [x - c * y for x, y in zip(v, o)]
        out.append(_unit(v))
    return out


def _ess_model(N, q):
    return _unit([sum(q[k] * N[k][e] for k in range(4)) for e in range(9)])


def truth_essential(pts, k4):
    """pts [5][4] = (u1, v1, u2, v2) in pixels, k4 = (fx, fy, cx, cy).  Up to ten roots, unit 9-vectors (normalised
    coordinates)."""
    vals, k4 = _mp(np.asarray(pts, object).ravel()), _mp(k4)
    A = _ess_rows(vals, k4)
    N0 = np.linalg.svd(np.array([[float(a) for a in r] for r in A]))[2][5:9]
    N = _ess_basis(A, [_mp(v) for v in N0])
    found, residual = [], _null_residual(A, N[0])
    for q in _ess_seeds(N0):
        got = _ess_polish(N, _mp(q))
        if got is not None:
            found.append(got)
            residual = max(residual, got[1])
    qs = _merge([g[0] for g in found], lambda p, q: _sine(_ess_model(N, p), _ess_model(N, q)))
    roots = [_ess_model(N, q) for q in qs]
    kappa = [mpf(0)] * len(roots)
    for signs in _draws(24):
        v2 = _perturb(vals + k4, signs)
        N2 = _ess_basis(_ess_rows(v2[:20], v2[20:]), N)
        for k, q in enumerate(qs):
            got = _ess_polish(N2, q)
            kappa[k] = max(kappa[k], _sine(roots[k], _ess_model(N2, got[0])) if got else mpf(1))

    def guard(cand):
        e = np.asarray(cand, np.float64).ravel()
        q = N0 @ e
        if not np.isfinite(q).all() or not np.linalg.norm(q) > 0:
            return None
        got = _ess_polish(N, _mp(q / np.linalg.norm(q)))
        if got is None:
            return None
        m = _ess_model(N, got[0])
        for k, r in enumerate(roots):
            if _sine(m, r) <= MERGE:
                return k
        raise TruthIncomplete("an essential candidate polished onto an unlisted root")
    return Sample(roots, [float(k) / U40 for k in kappa], residual, guard)


# ------------------------------------------------------------------------------------------------------- p3p
def _p3p_problem(P, uv, k4):
    """a = (a01, a02, a12), b = (b01, b02, b12), the unit bearings f [3][3]."""
    fx, fy, cx, cy = k4
    f = [_unit([(uv[2 * i] - cx) / fx, (uv[2 * i + 1] - cy) / fy, mpf(1)]) for i in range(3)]
    d = lambda i, j: [P[3 * i + k] - P[3 * j + k] for k in range(3)]
    a = [_dot(d(i, j), d(i, j)) for i, j in ((0, 1), (0, 2), (1, 2))]
    b = [_dot(f[i], f[j]) for i, j in ((0, 1), (0, 2), (1, 2))]
    return a, b, f


def _p3p_newton(a, b, l, maxit=60, floor=None):
    """Newton on the three distance equations from l; (l, residual relative to the largest a) or None.  floor: a list
    that receives the smallest residual met on the way."""
    l = list(l)
    amax = max(a)
    for _ in range(maxit):
        r = [l[0] * l[0] + l[1] * l[1] - 2 * b[0] * l[0] * l[1] - a[0], l[0] * l[0] + l[2] * l[2] - 2 * b[1] * l[0] * l[2] - a[1],
             l[1] * l[1] + l[2] * l[2] - 2 * b[2] * l[1] * l[2] - a[2]]
        res = max(abs(x) for x in r) / amax
        if floor is not None:
            floor[:] = [min(floor + [res])]
        J = [[2 * (l[0] - b[0] * l[1]), 2 * (l[1] - b[0] * l[0]), mpf(0)], [2 * (l[0] - b[1] * l[2]), mpf(0), 2 * (l[2] - b[1] * l[0])],
             [mpf(0), 2 * (l[1] - b[2] * l[2]), 2 * (l[2] - b[2] * l[1])]]
        try:
            step = _solve(J, [[x] for x in r])
        except ZeroDivisionError:
            return None
        if res < mpf("1e-55") or (res < RES_MAX and max(abs(s[0]) for s in step) < mpf("1e-45") * max(l)):
            return l, res
        l = [x - s[0] for x, s in zip(l, step)]
        if not all(abs(x) < mpf("1e30") for x in l):
            return None
    return None


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _frame(p0, p1, p2):
    e1 = _unit([x - y for x, y in zip(p1, p0)])
    e3 = _unit(_cross(e1, [x - y for x, y in zip(p2, p0)]))
    return e1, _cross(e3, e1), e3


def _p3p_pose(P, f, l):
    """[R|t] row-major with l_i f_i = R P_i + t: the rigid motion taking the world triangle's frame to the camera's."""
    w = _frame(P[0:3], P[3:6], P[6:9])
    y = [[l[i] * x for x in f[i]] for i in range(3)]
    c = _frame(*y)
    R = [[sum(c[m][r] * w[m][k] for m in range(3)) for k in range(3)] for r in range(3)]
    t = [y[0][r] - _dot(R[r], P[0:3]) for r in range(3)]
    return [x for r in range(3) for x in R[r] + [t[r]]]


def _rt_distance(m, ref, extent):
    R = lambda v: [v[4 * r + k] for r in range(3) for k in range(3)]
    t = lambda v: [v[4 * r + 3] for r in range(3)]
    dR = _norm([x - y for x, y in zip(R(m), R(ref))])
    dt = _norm([x - y for x, y in zip(t(m), t(ref))]) / max(_norm(t(ref)), extent)
    return max(dR, dt)


def _p3p_seeds(a, b):
    """float64 depth triples: with u = l1 / l0 and v = l2 / l0 the equations leave two conics whose v^2 terms agree, so
    their difference is linear in v; substituted back, a quartic in u by polynomial products (np.polymul)."""
    a01, a02, a12 = a
    b01, b02, b12 = b
    s = np.array([1.0, -2 * b01, 1.0])                                   # 1 + u^2 - 2 b01 u, descending
    C1 = np.polysub(a02 * s, [a01])
    C2 = np.polysub(a12 * s, [a01, 0.0, 0.0])
    B1, B2 = np.array([2 * a01 * b02]), np.array([2 * a01 * b12, 0.0])
    num, den = np.polysub(C2, C1), np.polysub(B1, B2)                    # v = num / den
    quartic = np.polyadd(np.polyadd(-a01 * np.polymul(num, num), np.polymul(np.polymul(B1, num), den)),
                         np.polymul(C1, np.polymul(den, den)))
    out = []
    if not np.isfinite(quartic).all() or not np.any(quartic):
        return out
    for u in np.roots(quartic):
        if abs(u.imag) > 1e-4 * (1 + abs(u.real)):
            continue
        u = u.real
        dn, sv = np.polyval(den, u), np.polyval(s, u)
        if dn == 0 or sv <= 0:
            continue
        v = np.polyval(num, u) / dn
        l0 = np.sqrt(a01 / sv)
        out.append([l0, u * l0, v * l0])
    return out


_CYCLES = ((0, 1, 2), (1, 2, 0), (2, 0, 1))
_PAIR = {(0, 1): 0, (1, 0): 0, (0, 2): 1, (2, 0): 1, (1, 2): 2, (2, 1): 2}


def truth_pnp(P, uv, k4):
    """P [3][3] world points (float64), uv [3][2] pixels (float32), k4 = (fx, fy, cx, cy).  Up to four [R|t] [12]."""
    Pv, uvv, kv = _mp(np.asarray(P, object).ravel()), _mp(np.asarray(uv, object).ravel()), _mp(k4)
    a, b, f = _p3p_problem(Pv, uvv, kv)
    extent = MP.sqrt(max(a))
    af, bf = [float(x) for x in a], [float(x) for x in b]
    found, residual, near_double = [], mpf(0), False
    for cyc in _CYCLES:
        pa = [af[_PAIR[cyc[0], cyc[1]]], af[_PAIR[cyc[0], cyc[2]]], af[_PAIR[cyc[1], cyc[2]]]]
        pb = [bf[_PAIR[cyc[0], cyc[1]]], bf[_PAIR[cyc[0], cyc[2]]], bf[_PAIR[cyc[1], cyc[2]]]]
        for s in _p3p_seeds(pa, pb):
            l = [0.0] * 3
            for k in range(3):
                l[cyc[k]] = s[k]
            if not (np.isfinite(l).all() and min(l) > 0):
                continue
            floor = []
            got = _p3p_newton(a, b, _mp(l), floor=floor)
            if got is not None and min(got[0]) > 0:
                found.append(got[0])
                residual = max(residual, got[1])
            # Newton that stalls at a residual of delta^2 circles a complex pair delta off the real axis: under
            # delta = 1e-6 (LEFT_OUT) the sample's count of real roots is not settled at the judge's resolution
            near_double = near_double or (got is None and floor[0] < mpf(LEFT_OUT) ** 2)
    ls = _merge(found, lambda p, q: max(abs(x - y) for x, y in zip(p, q)) / max(q))
    roots = [_p3p_pose(Pv, f, l) for l in ls]
    kappa = [mpf(0)] * len(roots)
    for signs in _draws(19):
        v2 = _perturb(Pv + uvv + kv, signs)
        a2, b2, f2 = _p3p_problem(v2[:9], v2[9:15], v2[15:])
        for k, l in enumerate(ls):
            got = _p3p_newton(a2, b2, l)
            kappa[k] = max(kappa[k], _rt_distance(_p3p_pose(v2[:9], f2, got[0]), roots[k], extent) if got else mpf(1))

    def guard(cand):
        m = _mp(np.asarray(cand, np.float64).ravel())
        l = [_norm([_dot(m[4 * r:4 * r + 3], Pv[3 * i:3 * i + 3]) + m[4 * r + 3] for r in range(3)]) for i in range(3)]
        R = [m[4 * r + k] for r in range(3) for k in range(3)]
        if _dot(_cof(R)[:3], R[:3]) < 0:
            return None                                                   # a mirror image: no rigid motion
        got = _p3p_newton(a, b, l)
        if got is None or min(got[0]) <= 0:
            return None
        for k, o in enumerate(ls):
            if max(abs(x - y) for x, y in zip(got[0], o)) / max(o) <= MERGE:
                return k
        raise TruthIncomplete("a P3P candidate polished onto an unlisted root")
    return Sample(roots, [float(k) / U40 for k in kappa], residual, guard, float(extent), undetermined=near_double)


# ------------------------------------------------------------------------------------------------- the judge
def distances(solver, cands, sample):
    """[m, n] float64: the distance of each candidate [m, D] (float64) to each truth root, taken in long double."""
    r = sample.roots
    if len(cands) == 0 or len(r) == 0:
        return np.zeros((len(cands), len(r)))
    c = np.asarray(cands, np.float64).reshape(len(cands), -1).astype(np.longdouble)
    if solver == "pnp":
        rot = [0, 1, 2, 4, 5, 6, 8, 9, 10]
        dR = np.sqrt(((c[:, None, rot] - r[None, :, rot]) ** 2).sum(-1))
        dt = np.sqrt(((c[:, None, 3::4] - r[None, :, 3::4]) ** 2).sum(-1))
        nt = np.maximum(np.sqrt((r[:, 3::4] ** 2).sum(-1)), np.longdouble(sample.extent))
        return np.maximum(dR, dt / nt[None]).astype(np.float64)
    c = c / np.sqrt((c * c).sum(-1, keepdims=True))
    dots = c @ r.T
    perp = c[:, None, :] - dots[:, :, None] * r[None]
    return np.sqrt((perp * perp).sum(-1)).astype(np.float64)


def judge(solver, cands, sample, C, single=False, degenerate=False):
    """The failures (strings; none = passed) of a candidate set [m, D] against a sample's truth under the constant C, and
    the ratios error / (kappa 2^-53) of the judged roots' matches.  single: the set is one stored best model (the
    device's fundamental and homography stages): it must match one root, the others are not required.  degenerate: the
    scene is one of the deliberately degenerate ones: no root is required, and a candidate passes if it lies within the
    bound of a root or the guard accepts it.  An unmatched candidate goes to the sample's guard first, which raises TruthIncomplete if the candidate is a root the truth lacks."""
    if sample.undetermined:
        return [], []
    d = distances(solver, cands, sample)
    tol = C * sample.kappa * U53
    judged = tol <= LEFT_OUT
    fails, ratios = [], []
    taken = np.zeros(len(tol), int)
    for m in range(d.shape[0]):
        if d.shape[1] == 0:
            fails.append(f"candidate {m}: the problem has no root")
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            k = int(np.argmin(np.where(tol > 0, d[m] / tol, np.inf)))
        if d[m, k] <= tol[k]:
            taken[k] += 1
            if judged[k]:
                ratios.append(d[m, k] / (sample.kappa[k] * U53))
            continue
        k = int(np.argmin(d[m]))
        landed = sample.guard(cands[m])                                   # TruthIncomplete passes through
        if degenerate and landed is not None:
            continue
        fails.append(f"candidate {m}: nearest root {k} at {d[m, k]:.3e}, {d[m, k] / (sample.kappa[k] * U53):.3g} x kappa 2^-53"
                     f" (kappa {sample.kappa[k]:.3g}); polished it lands on " + ("no root" if landed is None else f"root {landed}"))
    for k in np.flatnonzero(judged & (not degenerate)):
        if taken[k] > 1:
            fails.append(f"root {k} matched by {taken[k]} candidates")
        if taken[k] == 0 and not single:
            fails.append(f"root {k} (kappa {sample.kappa[k]:.3g}) matched by no candidate")
    if single and d.shape[0] != 1:
        fails.append(f"{d.shape[0]} models where one is stored")
    return fails, ratios


def measure_c(pairs):
    """The smallest self-consistent C over (kappa, error) pairs: C = max error / (kappa 2^-53) over the roots that C
    itself leaves in (C kappa 2^-53 <= 1e-6)."""
    kappa, err = (np.asarray(v, np.float64) for v in zip(*pairs))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(kappa > 0, err / (kappa * U53), np.inf)
    best = None
    for c in np.sort(ratio[np.isfinite(ratio)]):
        inside = kappa * U53 * c <= LEFT_OUT
        if inside.any() and ratio[inside].max() <= c:
            best = float(c)
            break
    return best


# ---------------------------------------------------------------------------------------------------- scenes
K4_REF = (1228.0, 1228.0, 512.0, 384.0)
N_HYP = {"fundamental": 257, "homography": 257, "essential": 65, "pnp": 257}
SAMPLE = {"fundamental": (7, 7), "homography": (4, 4), "essential": (5, 5), "pnp": (3, 4)}       # (size, least points)
# the judged hypotheses of a scene: the first lanes and the last ones, which end in the partial workgroup (essential: 16
# where the others have 20, which keeps its truth under 30 CPU seconds)
JUDGED = {"fundamental": list(range(0, 10)) + list(range(247, 257)), "homography": list(range(0, 10)) + list(range(247, 257)),
          "essential": list(range(0, 8)) + list(range(57, 65)), "pnp": list(range(0, 10)) + list(range(247, 257))}


class Scene:
    def __init__(self, name, data, k4=K4_REF, degenerate=False):
        self.name, self.data, self.k4, self.degenerate = name, data, k4, degenerate
        self.n = len(data[0])


def _pair(seed, noise=0.5, yaw=0.25, t=(-1.5, 0.1, 0.3), M=40):
    p1, p2, _ = fr.synth_pair(np.random.default_rng(seed), M, 0.0, noise=noise, yaw=yaw, t=t)
    return p1, p2


def _shift(pair, by):
    return tuple((p.astype(np.float64) + by).astype(np.float32) for p in pair)


def _collinear(passes):
    """Five matches of a plane scene whose first three lie almost on a line in image 1: a^2 = 1.2e-6 d1 d2 (kept) or
    0.8e-6 d1 d2 (no model by triple_ok's 1e-6 rule) for the triple (0, 1, 2)."""
    p1, p2, _ = hr.planar(np.random.default_rng(61), 5, 0.0, noise=0.0)
    p1, p2 = p1.astype(np.float64), p2.astype(np.float64)
    d = p1[1] - p1[0]
    nrm = np.array([-d[1], d[0]]) / np.hypot(*d)
    e1, e2 = p2[1] - p2[0], p2[2] - p2[0]
    side = np.sign(e1[0] * e2[1] - e1[1] * e2[0])                # keep the turn of image 2
    sine = np.sqrt((1.2 if passes else 0.8) * 1e-6)
    p1[2] = p1[0] + 1.7 * d + side * sine * 1.7 * np.hypot(*d) * nrm
    return p1.astype(np.float32), p2.astype(np.float32)


@functools.lru_cache(maxsize=None)
def scenes(solver):
    """The scenes of a solver, in the order of the device call's segments - computed once, never modified."""
    if solver == "pnp":
        return _pnp_scenes()
    bunny = er.shipped_pairs()
    far = 3500.0
    out = [Scene("noise-free", _pair(1, noise=0.0)), Scene("noise 0.5 px, wide baseline", _pair(2)),
           Scene("baseline 1 % of the depth", _pair(3, yaw=0.02, t=(0.06, 0.0, 0.0))),
           Scene("forward motion", _pair(4, yaw=0.03, t=(0.02, -0.01, -1.0))),
           Scene("pixels near 4000", _shift(_pair(5), far), (1228.0, 1228.0, 512.0 + far, 384.0 + far)),
           Scene("shipped pair 0", (bunny[0][0], bunny[0][1])), Scene("shipped pair 78", (bunny[78][0], bunny[78][1]))]
    if solver == "essential":
        p1, p2 = (p.astype(np.float64) for p in _pair(6))
        sq = lambda p: np.c_[p[:, 0], 384.0 + 1.25 * (p[:, 1] - 384.0)].astype(np.float32)
        out.append(Scene("fx != fy", (sq(p1), sq(p2)), (1228.0, 1535.0, 512.0, 384.0)))
    if solver == "fundamental":
        out.append(Scene("planar (degenerate)", hr.planar(np.random.default_rng(7), 40, noise=0.0)[:2], degenerate=True))
    if solver == "homography":
        out += [Scene("plane, noise-free", hr.planar(np.random.default_rng(8), 40, noise=0.0)[:2]),
                Scene("plane, noise 0.5 px", hr.planar(np.random.default_rng(9), 40)[:2]),
                Scene("rotation", hr.rotation(np.random.default_rng(10), 40)[:2]),
                Scene("triple past the collinearity rule", _collinear(True)),
                Scene("triple short of the collinearity rule", _collinear(False))]
    return out


def _pnp_scenes():
    R, t = None, None

    def view(seed, noise=0.5, M=40):
        nonlocal R, t
        X, uv, R, t = pr.synth_view(np.random.default_rng(seed), M, 0.0, noise=noise)
        return X, uv

    def project(X):
        x = (X @ R.T + t) @ fr.K_REF.T
        return (x[:, :2] / x[:, 2:]).astype(np.float32)

    out = [Scene("noise-free", view(21, noise=0.0)), Scene("noise 0.5 px", view(22))]
    X, uv = view(23)
    out.append(Scene("world offset 1e3, extent 1", (X + 1e3, uv)))
    # six points, two of whose triples are flattened: the first judged sample of this segment to a sine of 1.5e-10 at its
    # first vertex (at most twice that at the others: past the area rule |n|^2 > 1e-20 d1^2 d2^2), the first judged
    # sample that shares no point with it to 0.4e-10 (short of the rule at every vertex: no model)
    X, _ = view(24, noise=0.0, M=6)
    drawn = ransac_reference.draw_samples(SEED, len(out), 6, N_HYP["pnp"], 3, 4)[JUDGED["pnp"]]
    past = drawn[0]
    short = next(r for r in drawn if not set(r) & set(past))
    for (i, j, k), sine in ((past, 1.5e-10), (short, 0.4e-10)):
        d = X[j] - X[i]
        nrm = np.cross(d, [0.3, -0.5, 0.8])
        X[k] = X[i] + 2.0 * d + sine * 2.0 * np.linalg.norm(d) * nrm / np.linalg.norm(nrm)
    out.append(Scene("near-collinear triangles", (X, project(X))))
    rng = np.random.default_rng(25)
    cam = np.c_[rng.uniform(-1, 1, (40, 2)), np.full(40, 6.0)]
    X = (cam - t) @ R                                                     # R^T (cam - t): every point at depth 6
    out.append(Scene("equal depth", (X, (project(X).astype(np.float64) + rng.normal(size=(40, 2)) * 0.5).astype(np.float32))))
    # the danger cylinder: world points on a circle, the camera centre 1e-7 off the cylinder over it
    th = rng.uniform(0, 2 * np.pi, 40)
    X = np.c_[np.cos(th), np.sin(th), np.full(40, 6.0)]
    x = (X - [1.0 + 1e-7, 0.0, 0.0]) @ fr.K_REF.T
    out.append(Scene("danger cylinder (degenerate)", (X, (x[:, :2] / x[:, 2:]).astype(np.float32)), degenerate=True))
    return out


@functools.lru_cache(maxsize=None)
def samples(solver, segment):
    """[N_HYP, size] int32: the samples of scene `segment`, as the device call draws them for that segment."""
    size, least = SAMPLE[solver]
    return ransac_reference.draw_samples(SEED, segment, scenes(solver)[segment].n, N_HYP[solver], size, least)


def sample_inputs(solver, scene, idx):
    """What the truth_* function of the solver takes for the sample idx of a scene."""
    if solver == "pnp":
        return scene.data[0][idx], scene.data[1][idx], scene.k4
    px = np.c_[scene.data[0][idx], scene.data[1][idx]]
    return (px, scene.k4) if solver == "essential" else (px,)


TRUTH = {"fundamental": truth_fundamental, "homography": truth_homography, "essential": truth_essential, "pnp": truth_pnp}


@functools.lru_cache(maxsize=None)
def truth(solver):
    """({(segment, hypothesis): Sample} over the judged hypotheses of every scene, CPU seconds) - computed once per
    session, never modified."""
    t0 = time.process_time()
    out = {}
    for s, sc in enumerate(scenes(solver)):
        for h in JUDGED[solver]:
            try:
                out[s, h] = TRUTH[solver](*sample_inputs(solver, sc, samples(solver, s)[h]))
            except ZeroDivisionError:                                     # a repeated match: the system has lost a rank
                out[s, h] = Sample([], [], mpf(0), lambda cand: None, undetermined=True)
    return out, time.process_time() - t0


def left_out_shares(solver, C):
    """(share of the roots left out under C over the scenes that are not degenerate, {scene name: share})."""
    tr, _ = truth(solver)
    per, tot = {}, [0, 0]
    for s, sc in enumerate(scenes(solver)):
        kap = np.concatenate([tr[s, h].kappa if not tr[s, h].undetermined else np.r_[tr[s, h].kappa, np.inf] * np.inf
                              for h in JUDGED[solver]])
        out = int((C * kap * U53 > LEFT_OUT).sum())
        per[sc.name] = out / max(len(kap), 1)
        if not sc.degenerate:
            tot[0] += out
            tot[1] += len(kap)
    return tot[0] / max(tot[1], 1), per


# ------------------------------------------------------------------------- what the solvers are expected to do
def voided(solver, scene, idx):
    """True where the stage's own sample rule gives no model for the sample idx (its slots must then hold none)."""
    if solver == "homography":
        return bool(hr.voided(scene.data[0], scene.data[1], idx[None])[0])
    if solver == "essential":
        return bool(er.voided(scene.data[0], scene.data[1], idx[None])[0])
    if solver == "pnp":
        return bool(pr.degenerate(scene.data[0][idx]))
    return False


def hartley_pair(scene):
    p1, p2 = (np.asarray(p, np.float64) for p in scene.data)
    return fr.hartley(p1), fr.hartley(p2)


def reference_candidates(solver, scene, idx):
    """The candidates [m, D] of the NumPy reference (fr.seven_point, hr.four_point, er.five_point, pr.p3p) for one
    sample, in the coordinates of the truth: F and H in pixels, E normalised, [R|t] row-major."""
    if voided(solver, scene, idx):                                        # the references' ransac() applies the rule first
        return np.zeros((0, 12 if solver == "pnp" else 9))
    if solver == "pnp":
        f = pr.bearings(scene.data[1][idx], pr.k_matrix(scene.k4))
        got = pr.p3p(scene.data[0][idx], f)
        return np.array([np.c_[R, t].ravel() for R, t in got]).reshape(-1, 12)
    p1, p2 = (np.asarray(p, np.float64) for p in scene.data)
    if solver == "essential":
        K = pr.k_matrix(scene.k4)
        E, ok = er.five_point(er.normalise(p1[idx], K)[None], er.normalise(p2[idx], K)[None])
        return E[0][ok[0]].reshape(-1, 9)
    T1, T2 = hartley_pair(scene)
    n1 = (np.c_[p1[idx], np.ones(len(idx))] @ T1.T)[None, :, :2]
    n2 = (np.c_[p2[idx], np.ones(len(idx))] @ T2.T)[None, :, :2]
    if solver == "fundamental":
        Fn, ok = fr.seven_point(n1, n2)
        return np.array([T2.T @ F @ T1 for F in Fn[0][ok[0]]]).reshape(-1, 9)
    Hn, ok = hr.four_point(n1, n2)
    return (np.linalg.inv(T2) @ Hn[0] @ T1).reshape(-1, 9)[:int(ok[0])]


def sample_failures(solver, cands, sample, scene, idx, C):
    """judge() for the sample idx of a scene - after the stage's own sample rule: where that gives no model, any model
    is a failure."""
    if voided(solver, scene, idx):
        return (["a model where the sample rule gives none"] if len(cands) else []), []
    return judge(solver, cands, sample, C, degenerate=scene.degenerate)


def model_count(solver, model, scene, threshold):
    """The inlier count of one 3 x 3 model over the scene's matches, by the references' rules."""
    p1, p2 = (np.asarray(p, np.float64) for p in scene.data)
    M = np.asarray(model, np.float64).reshape(3, 3)
    if solver == "fundamental":
        return int(fr.inliers(M, p1, p2, threshold).sum())
    return int(hr.inliers(M, p1, p2, threshold).sum())


def best_model_failures(solver, model, hyp_count, sample, scene, C, threshold, stable):
    """The device's fundamental and homography stages keep one model per hypothesis, the best.  It must match one truth
    root (judge(single=True)); and where the hypothesis is `stable`, the count of the root it matched, recomputed by
    the reference's rule, must equal hyp_count - a stored model that is a root, but not the one that was counted, fails here."""
    fails, ratios = judge(solver, np.asarray(model).reshape(1, 9), sample, C, single=True, degenerate=scene.degenerate)
    if not fails and stable and not scene.degenerate and not sample.undetermined:
        d = distances(solver, np.asarray(model).reshape(1, 9), sample)[0]
        with np.errstate(divide="ignore", invalid="ignore"):
            k = int(np.argmin(d / (C * sample.kappa * U53)))
        want = model_count(solver, sample.roots[k].astype(np.float64), scene, threshold)
        if want != hyp_count:
            fails.append(f"hyp_count {hyp_count}, but the matched root {k} counts {want}")
    return fails, ratios


def count_is_stable(solver, sample, scene, threshold):
    """fundamental_reference has no stable(): a fundamental hypothesis is taken as stable when no root's count changes
    between threshold (1 - 1e-3) and threshold (1 + 1e-3) - a model within the judge's bound (at most 1e-6 in the sine)
    moves no match across the gate then."""
    return all(model_count(solver, r.astype(np.float64), scene, threshold * (1 - 1e-3)) ==
               model_count(solver, r.astype(np.float64), scene, threshold * (1 + 1e-3)) for r in sample.roots)


def ws_regions(total_bytes, *regions):
    """Byte offsets of a workspace's leading arrays: each region (count, itemsize) is rounded up to 256 bytes, in order
    (ws_carve::take in sfm_amd/csrc/common.h), and the sum plus 256 is what sfm_*_workspace_bytes reports.  The
    regions must be ALL of the layout: a layout change fails here and does not read the wrong bytes."""
    off, at = [], 0
    for count, itemsize in regions:
        off.append(at)
        at += (count * itemsize + 255) // 256 * 256
    assert at + 256 == total_bytes, (at + 256, total_bytes)
    return off
