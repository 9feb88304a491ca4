"""A multi-precision truth for the geometric code that runs after the minimal solvers - camera centres, the linear and
the refined point of a track, the gate quantities, the four poses of an essential matrix - and the judge that holds
tests/triangulate_reference.py, tests/pose_reference.py, the host builds of triangulate_solve.h, triangulate_robust.h and
pose_solve.h (tests/test_geometry_truth.py) and the device (tests/test_geometry_truth_gpu.py) to it.

The truth solves each PROBLEM in mpmath at 60 digits with the small algebra of tests/solver_truth.py; it replays no kernel
and shares no routine with the three headers or with triangulate_reference, triangulate_robust_reference and
pose_reference (those modules appear below as the references under judgement and as builders of scenes only).  Inputs
are taken exactly as the float64 or float32 numbers they are.

    centre      C solves M C = -p4 (P = [M | p4]) by Gaussian elimination
    linear X    the eigenvector of the smallest eigenvalue of A^T A, A the 2n x 4 matrix of the rows x P[2] - P[0] and
                y P[2] - P[1] in pixels: MP.eigsy, then inverse iteration until |A^T A v - lambda v| < 1e-40 |v|;
                dehomogenised.  Two views are the same problem with four rows (jacobi::dlt2, sfm_triangulate2).
    refined X   the stationary point of the sum of squared reprojection errors reached from the linear truth by full
                Newton (analytic gradient and Hessian) until the gradient is below 1e-40; the Hessian there is positive
                definite.  A track where Newton does not get there in 60 steps is undetermined: nothing of it is judged.
    gates       at a given X: the depths P[2].(X,1), the reprojection errors and their maximum, the cost, the cosines of
                the pairs of viewing directions X - C
    poses       from E: V from the eigenvectors of E^T E, u_k = E v_k / sigma_k for the two large singular values (also
                eigenvectors of E E^T), u_3 = u_1 x u_2, v_3 signed for det V = +1; R = U W V^T and U W^T V^T,
                t = +- u_3: a set of four.  R^T R - I, det R - 1 and the eigen relations hold to 1e-40.

Condition.  As in solver_truth.py: all inputs of a case (the entries of the used cameras' P and the pixels; the nine
entries of E) multiplied at once by 1 +- 2^-40 with independent signs, three fixed-seed draws, kappa = the largest
relative change of the output / 2^-40.  The change of X is relative to |X - centroid of the used views' centres| (with
|X| a world far from the origin would flatter every method), that of a centre to |C|, that of max_err and of the cost
to max_err and the cost, that of [R|t] is solver_truth's distance.

The judge.  An output must lie within C kappa 2^-53 of the truth; a case whose bound at 8 x C passes 1e-6 is left out,
neither required nor forbidden.  C = C_REF per quantity for the references, 8 x C_REF (solver_truth.MARGIN) for the host
builds and the device; C_REF is the worst ratio of the float64 NumPy restatements over scenes(), by measure_c().  The
cost (the 5-step assertions) takes twice the constant of max_err: it is a sum of squares of the errors max_err is the
largest of.  Left-out plus undetermined cases: at most 2 % per scene and quantity outside the degenerate scene.  In the
exact scene max_err is zero by construction, so "relative to max_err" says nothing there: its max_err is judged by the
same ratio error / (kappa 2^-53) taken in pixels, and left out when that bound passes 1e-6 px.

Status.  The status the truth's gate quantities give must be the device's wherever every deciding quantity (the
smallest depth from 0, max_err from max_error, the smallest cosine from cos_min) is further from its threshold than its
own bound (8 x C_REF of the point's kind x its own kappa in absolute units x 2^-53); inside that band either neighbour
is accepted.

Measured (scenes() and essentials(), seed SEED; ratios are error / (kappa 2^-53); host = tests/native/
triangulate_solve_check.cpp, triangulate_robust_check.cpp and pose_solve_check.cpp by g++ -ffp-contract=off /
-ffp-contract=fast -mfma; device = MI355X; left out = share of the cases outside the degenerate scene whose bound at
8 x C_REF passes 1e-6 or whose truth is undetermined, the worst scene; time = CPU seconds of truth() / pose_truths()):

    quantity    cases   C_REF   bound 8 x C_REF   worst host off / fast   worst device   left out   time
    centre      882     2.23    17.84             2.23 / 1.52             2.23           0 %        1 s
    linear X    734     99.6    796.8             99.5 / 92.4             99.5           0 %        54 s, all three
    refined X   734     2.2     17.6              2.16 / 3.03             2.16           0 %
    max_err     1468    16.1    128.8             16.0 / 15.6             16.0           0 %
    pose        320     46.2    369.6             6.57 / 8.92             6.57           0 %        1.5 s

C_REF of the linear point is set by the 24 long tracks alone (every other scene stays below 8.2): there kappa is at
most 0.33 - hundreds of views average the perturbation out - while the streaming Givens accumulation of 128 to 1026 rows
collects a relative error of up to about 3.6e-15, some 30 x 2^-53.  That is the growth of a backward-stable QR with the number of
rows, not a lost digit; the refined point of the same tracks is at 2.15.  C_REF of the poses is LAPACK's (pose_reference):
kappa is below 1 there (0.13 to 2), and the one-sided Jacobi of pose_solve.h is nearer the truth than LAPACK is.  The
exact scene sets C_REF of max_err (16.0, in pixels; 12.4 elsewhere).

The shipped default of 5 Gauss-Newton steps: judged as the stationary point on every scene but the narrow arcs and the
principal-plane scene (worst 1.95, host and device alike).  On those three it is measured: the distance to the
stationary point in units of the bound 8 x C_REF is 0.076 (arc of 0.04 rad), 0.073 (arc of 0.01 rad) and 0.10 (depth
1e-3 of the others) on the device and the -ffp-contract=off host build, 0.085 / 0.065 / 0.066 with fma: 5 steps have
converged on all of them.  The cost of the 5-step point never exceeds the linear truth's by more than 0.0011 kappa 2^-53.

What the bounds found when they were first run: nothing in the headers.  Two things in the first draft of the scenes
and the test: full Newton does not reach a stationary point from the linear point when one view is 1000 times nearer
than the others and the other views carry 0.002 px of noise or more (the Hessian there is indefinite; Gauss-Newton,
which the header runs, does get there), so that scene is nearly noise-free; and sfm_tracks_evaluate needs the condition
number of its own problem (evaluate_case), in which the point is an input and does not follow a perturbation.
"""
import functools
import time

import numpy as np

import pose_reference as pr
import solver_truth as st
import triangulate_reference as tr
from solver_truth import MP, _dot, _sine, _solve, _to_ld  # noqa: F401  (the algebra the truth is written in)

mpf = MP.mpf
RES_MAX = st.RES_MAX
U40, U53, LEFT_OUT, MARGIN = st.U40, st.U53, st.LEFT_OUT, st.MARGIN
SEED = 23
NEWTON_STEPS = 60
QUANTITIES = ("centre", "linear", "refined", "max_err", "pose")
# the worst ratio error / (kappa 2^-53) of the float64 NumPy restatements over scenes(), measured by measure_c() in
# tests/test_geometry_truth.py::test_references_define_c - see the table above
C_REF = {"centre": 2.23, "linear": 99.6, "refined": 2.2, "max_err": 16.1, "pose": 46.2}
C_COST = 2.0



# --------------------------------------------------------------------------------------------------- the truth
def _mp(v):
    return st._mp(np.asarray(v, dtype=object).ravel())


def centre_truth(P):
    """P [12] -> C [3] (mpf)."""
    P = _mp(P)
    return [r[0] for r in _solve([P[0:3], P[4:7], P[8:11]], [[-P[3]], [-P[7]], [-P[11]]])]


def _ata(obs):
    G = [[mpf(0)] * 4 for _ in range(4)]
    for P, x, y in obs:
        for r in ([x * P[8 + k] - P[k] for k in range(4)], [y * P[8 + k] - P[4 + k] for k in range(4)]):
            for i in range(4):
                for j in range(i, 4):
                    G[i][j] += r[i] * r[j]
    for i in range(4):
        for j in range(i):
            G[i][j] = G[j][i]
    return G


def _matvec(G, v):
    return [_dot(r, v) for r in G]


def linear_truth(obs):
    """obs [(P [12], x, y)] (mpf) -> (X [3], v [4] unit, lambda, |A^T A v - lambda v| / |v|)."""
    G = _ata(obs)
    _, Q = MP.eigsy(MP.matrix(G))
    v = st._unit([Q[i, 0] for i in range(4)])
    shift = mpf("1e-25") * (G[0][0] + G[1][1] + G[2][2] + G[3][3])
    lam = res = None
    for _ in range(6):
        lam = _dot(v, _matvec(G, v))
        w = _solve([[G[i][j] - ((lam - shift) if i == j else 0) for j in range(4)] for i in range(4)], [[x] for x in v])
        v = st._unit([x[0] for x in w])
        lam = _dot(v, _matvec(G, v))
        res = st._norm([a - lam * b for a, b in zip(_matvec(G, v), v)])
        if res < RES_MAX:
            break
    return [v[k] / v[3] for k in range(3)], v, lam, res


def _derivatives(obs, X):
    """(cost, gradient [3], Hessian [3][3]) of the sum of squared reprojection errors at X."""
    g = [mpf(0)] * 3
    H = [[mpf(0)] * 3 for _ in range(3)]
    cost = mpf(0)
    for P, x, y in obs:
        iw = 1 / (P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11])
        u = (P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3]) * iw
        v = (P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7]) * iw
        du, dv = u - x, v - y
        cost += du * du + dv * dv
        ju = [(P[k] - u * P[8 + k]) * iw for k in range(3)]
        jv = [(P[4 + k] - v * P[8 + k]) * iw for k in range(3)]
        a = [ju[k] * du + jv[k] * dv for k in range(3)]        # the second derivatives of u and v are -(ju p2^T + p2 ju^T) / hw
        for i in range(3):
            g[i] += a[i]
            for j in range(i, 3):
                H[i][j] += ju[i] * ju[j] + jv[i] * jv[j] - (a[i] * P[8 + j] + P[8 + i] * a[j]) * iw
    for i in range(3):
        for j in range(i):
            H[i][j] = H[j][i]
    return cost, [2 * x for x in g], [[2 * x for x in r] for r in H]


def _positive_definite(H):
    a = H[0][0]
    b = H[0][0] * H[1][1] - H[0][1] * H[1][0]
    c = (H[0][0] * (H[1][1] * H[2][2] - H[1][2] * H[2][1]) - H[0][1] * (H[1][0] * H[2][2] - H[1][2] * H[2][0])
         + H[0][2] * (H[1][0] * H[2][1] - H[1][1] * H[2][0]))
    return a > 0 and b > 0 and c > 0


def _gradient(obs, X):
    g = [mpf(0)] * 3
    for P, x, y in obs:
        iw = 1 / (P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11])
        u = (P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3]) * iw
        v = (P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7]) * iw
        du, dv = (u - x) * iw, (v - y) * iw
        for k in range(3):
            g[k] += (P[k] - u * P[8 + k]) * du + (P[4 + k] - v * P[8 + k]) * dv
    return [2 * x for x in g]


def refined_truth(obs, X0, steps=NEWTON_STEPS, keep=None):
    """Full Newton from X0: (X, |gradient|, Hessian) with the gradient below 1e-40 and a positive definite Hessian, or
    None.  keep: X0 is the stationary point of inputs 2^-40 away and `keep` the Hessian there, which is kept (it is 1e-12
    off) so that a step needs the gradient only; the stationary point does not depend on the route."""
    X = list(X0)
    H = keep
    for _ in range(steps):
        try:
            if keep is not None:
                g = _gradient(obs, X)
            else:
                _, g, H = _derivatives(obs, X)
            gn = st._norm(g)
            if gn < RES_MAX:
                return (X, gn, H) if keep is not None or _positive_definite(H) else None
            step = _solve(H, [[x] for x in g])
        except ZeroDivisionError:
            return None
        X = [a - s[0] for a, s in zip(X, step)]
        if not all(abs(a) < mpf("1e30") for a in X):
            return None
    return None


def gate_truth(obs, centres, X):
    """At X (mpf [3]): (errors [n], depths [n], cost, smallest cosine over the pairs of views or None for one view)."""
    err, depth, cost = [], [], mpf(0)
    for P, x, y in obs:
        hw = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11]
        du = (P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3]) / hw - x
        dv = (P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7]) / hw - y
        cost += du * du + dv * dv
        err.append(MP.sqrt(du * du + dv * dv))
        depth.append(hw)
    d = [st._unit([a - b for a, b in zip(X, C)]) for C in centres]
    cos = None
    if len(d) > 1:                                             # the pair is found in long double, its cosine taken in mp
        D = np.stack([_to_ld(v) for v in d])
        c = D @ D.T + 4 * np.eye(len(d), dtype=np.longdouble)
        i, j = np.unravel_index(int(np.argmin(c)), c.shape)
        cos = _dot(d[i], d[j])
    return err, depth, cost, cos


class Point:
    """One point of a track's truth: X (long double [3]) and X_mp, kappa of X, and the gate quantities with their kappa
    in absolute units: max_err, cost, min_depth, min_cos (None for a single view), err [n] with k_err [n]."""


def _point(obs, centres, X, scale):
    p = Point()
    p.X_mp, p.X = X, _to_ld(X)
    err, depth, cost, cos = gate_truth(obs, centres, X)
    p.err = np.array([float(e) for e in err])
    p.max_err_mp, p.cost_mp, p.min_depth_mp, p.min_cos_mp = max(err), cost, min(depth), cos
    p.scale_mp = scale
    p.d = {"X": mpf(0), "max_err": mpf(0), "cost": mpf(0), "min_depth": mpf(0), "min_cos": mpf(0)}
    p.err_mp, p.d_err = err, [mpf(0)] * len(err)
    return p


def _perturbed(p, obs, centres, X):
    err, depth, cost, cos = gate_truth(obs, centres, X)
    ch = {"X": st._norm([a - b for a, b in zip(X, p.X_mp)]) / p.scale_mp, "max_err": abs(max(err) - p.max_err_mp),
          "cost": abs(cost - p.cost_mp), "min_depth": abs(min(depth) - p.min_depth_mp),
          "min_cos": abs(cos - p.min_cos_mp) if cos is not None else mpf(0)}
    for k, v in ch.items():
        p.d[k] = max(p.d[k], v)
    p.d_err = [max(d, abs(a - b)) for d, a, b in zip(p.d_err, err, p.err_mp)]


def _finish(p):
    p.kappa = float(p.d["X"]) / U40
    p.max_err, p.cost, p.min_depth = float(p.max_err_mp), float(p.cost_mp), float(p.min_depth_mp)
    p.min_cos = None if p.min_cos_mp is None else float(p.min_cos_mp)
    p.k_max_err, p.k_cost = float(p.d["max_err"]) / U40, float(p.d["cost"]) / U40
    p.k_min_depth, p.k_min_cos = float(p.d["min_depth"]) / U40, float(p.d["min_cos"]) / U40
    p.scale = float(p.scale_mp)
    p.k_err = np.array([float(d) for d in p.d_err]) / U40          # per observation, in pixels
    del p.d, p.d_err


class TrackTruth:
    """linear, refined: Point (refined None where Newton did not get there: undetermined); residual: the eigen
    residual of the linear stage; gradient: |gradient| at the refined point."""


def track_truth(P_list, cams, xy):
    """P_list {camera: [12]} of the used cameras, cams [n] the camera of each observation, xy [n,2] -> TrackTruth."""
    keys = sorted(P_list)
    vals = [v for k in keys for v in _mp(P_list[k])] + _mp(xy)

    def unpack(vals):
        Pm = {k: vals[12 * i:12 * i + 12] for i, k in enumerate(keys)}
        px = vals[12 * len(keys):]
        obs = [(Pm[c], px[2 * i], px[2 * i + 1]) for i, c in enumerate(cams)]
        cen = {k: centre_truth(Pm[k]) for k in keys}
        return obs, [cen[c] for c in cams]

    obs, centres = unpack(vals)
    T = TrackTruth()
    T.obs, T.centres = obs, centres
    Xl, _, _, T.residual = linear_truth(obs)
    mid = [sum(C[k] for C in centres) / len(centres) for k in range(3)]
    T.linear = _point(obs, centres, Xl, st._norm([a - b for a, b in zip(Xl, mid)]))
    got = refined_truth(obs, Xl)
    T.refined, T.gradient, hessian = None, None, None
    if got is not None:
        T.refined, T.gradient = _point(obs, centres, got[0], st._norm([a - b for a, b in zip(got[0], mid)])), got[1]
        hessian = got[2]
    for signs in st._draws(len(vals)):
        obs2, cen2 = unpack(st._perturb(vals, signs))
        _perturbed(T.linear, obs2, cen2, linear_truth(obs2)[0])
        if T.refined is not None:
            got = refined_truth(obs2, T.refined.X_mp, steps=12, keep=hessian)
            if got is None:
                T.refined = None
            else:
                _perturbed(T.refined, obs2, cen2, got[0])
    _finish(T.linear)
    if T.refined is not None:
        _finish(T.refined)
    return T


def centre_case(P):
    """(C long double [3], kappa relative to |C|)."""
    vals = _mp(P)
    C = centre_truth(vals)
    n = st._norm(C)
    worst = mpf(0)
    for signs in st._draws(12):
        C2 = centre_truth(st._perturb(vals, signs))
        worst = max(worst, st._norm([a - b for a, b in zip(C, C2)]) / n if n else mpf(0))
    return _to_ld(C), float(worst) / U40


def _col(M, k):
    return [M[r][k] for r in range(3)]


def _poses_mp(E):
    """E [9] (mpf) -> ([4][12] row-major [R|t] in the order R1 t, R2 t, R1 -t, R2 -t; residual), or None (rank < 2)."""
    Em = [E[0:3], E[3:6], E[6:9]]
    EtE = [[sum(Em[r][i] * Em[r][j] for r in range(3)) for j in range(3)] for i in range(3)]
    lam, Q = MP.eigsy(MP.matrix(EtE))
    order = sorted(range(3), key=lambda k: -lam[k])
    V = [st._unit([Q[r, k] for r in range(3)]) for k in order]            # v_1, v_2, v_3 by descending eigenvalue
    if not lam[order[1]] > 0:
        return None
    Ev = [[_dot(Em[r], V[k]) for r in range(3)] for k in range(2)]
    sig = [st._norm(x) for x in Ev]
    U = [[x / s for x in e] for e, s in zip(Ev, sig)]
    U.append(st._cross(U[0], U[1]))
    if _dot(st._cross(V[0], V[1]), V[2]) < 0:
        V[2] = [-x for x in V[2]]
    scale = sig[0] * sig[0]
    res = max(st._norm([a - lam[order[k]] * b for a, b in zip(_matvec(EtE, V[k]), V[k])]) for k in range(3)) / scale
    EEt = [[_dot(Em[i], Em[j]) for j in range(3)] for i in range(3)]
    res = max([res] + [st._norm([a - sig[k] * sig[k] * b for a, b in zip(_matvec(EEt, U[k]), U[k])]) / scale for k in range(2)])
    UW = ([-x for x in U[1]], U[0], U[2])                                  # the columns of U W and of U W^T
    UWt = (U[1], [-x for x in U[0]], U[2])
    out = []
    for cols in (UW, UWt):
        R = [[sum(cols[k][r] * V[k][c] for k in range(3)) for c in range(3)] for r in range(3)]
        RtR = [_dot(_col(R, i), _col(R, j)) - (1 if i == j else 0) for i in range(3) for j in range(3)]
        res = max([res, abs(_dot(st._cross(R[0], R[1]), R[2]) - 1)] + [abs(x) for x in RtR])
        out.append(R)
    t = U[2]
    return [[x for r in range(3) for x in R[r] + [s * t[r]]] for s in (1, -1) for R in out], res


class PoseTruth:
    """poses [4,12] long double (a set), kappa [4], residual; none: E gives no model (rank < 2)."""


def pose_truth(E):
    vals = _mp(E)
    T = PoseTruth()
    got = _poses_mp(vals)
    T.none = got is None
    if T.none:
        return T
    poses, T.residual = got
    worst = [mpf(0)] * 4
    for signs in st._draws(9):
        got2 = _poses_mp(st._perturb(vals, signs))
        for k, p in enumerate(poses):
            worst[k] = max(worst[k], min(st._rt_distance(q, p, mpf(1)) for q in got2[0]) if got2 else mpf(1))
    T.poses_mp = poses
    T.poses = np.stack([_to_ld(p) for p in poses])
    T.kappa = np.array([float(w) / U40 for w in worst])
    return T


# ---------------------------------------------------------------------------------------------------- the judge
def ratio_points(X, point):
    """|X - X*| / scale / (kappa 2^-53) of a float64 X [3] (inf where kappa is 0 and X differs)."""
    d = np.asarray(X, np.float64).astype(np.longdouble) - point.X
    e = float(np.sqrt((d * d).sum())) / point.scale
    return _ratio(e, point.kappa)


def _ratio(e, kappa):
    if not np.isfinite(e):
        return np.inf
    if kappa == 0:
        return 0.0 if e == 0 else np.inf
    return e / (kappa * U53)


def left_out(kappa, C, unit=1.0):
    """The bound at MARGIN x C_REF passes 1e-6 (relative; `unit` turns an absolute kappa into a relative one)."""
    return not MARGIN * C * kappa * U53 <= LEFT_OUT * unit


def ratio_max_err(e, point):
    return _ratio(abs(float(np.longdouble(e) - np.longdouble(point.max_err))), point.k_max_err)


def max_err_left_out(point, exact):
    return left_out(point.k_max_err, C_REF["max_err"], 1.0 if exact else point.max_err)


def pose_distances(cands, T):
    """[4 candidates, 4 truths]: solver_truth's [R|t] distance with extent 1 (t is a unit vector)."""
    c = np.asarray(cands, np.float64).reshape(4, 12).astype(np.longdouble)
    rot = [0, 1, 2, 4, 5, 6, 8, 9, 10]
    dR = np.sqrt(((c[:, None, rot] - T.poses[None, :, rot]) ** 2).sum(-1))
    dt = np.sqrt(((c[:, None, 3::4] - T.poses[None, :, 3::4]) ** 2).sum(-1))
    return np.maximum(dR, dt).astype(np.float64)


def judge_poses(cands, T, C):
    """(failures, ratios): the four candidates must match the truth's four as a set - pr.match_candidates applied to the
    truth - each within C kappa 2^-53."""
    fails, ratios = [], []
    cands = np.asarray(cands, np.float64).reshape(4, 3, 4)
    if not np.isfinite(cands).all():
        return ["a candidate is not finite"], []
    d = pose_distances(cands, T)
    try:
        perm, _ = pr.match_candidates([(c[:, :3], c[:, 3]) for c in cands],
                                      [(p.reshape(3, 4)[:, :3].astype(np.float64), p.reshape(3, 4)[:, 3].astype(np.float64)) for p in T.poses])
    except AssertionError:
        return [f"pose: the candidates are no permutation of the truth's four (nearest distances {d.min(0)})"], []
    for k in range(4):
        if left_out(T.kappa[k], C_REF["pose"]):
            continue
        r = _ratio(d[perm[k], k], T.kappa[k])
        ratios.append(r)
        if not r <= C:
            fails.append(f"pose: candidate {perm[k]} lies {d[perm[k], k]:.3e} from truth {k}, {r:.3g} x kappa 2^-53 (kappa {T.kappa[k]:.3g})")
    return fails, ratios


def allowed_statuses(point, kind, n_views, min_views=2, max_error=4.0, min_angle_deg=0.0):
    """(the set of statuses the band rule accepts at this truth point, in_band); kind: "linear" or "refined", whose
    constant bounds the depth and the cosine."""
    if n_views < min_views:
        return {tr.TOO_FEW_VIEWS}, False

    def sides(value, kappa, thr, C):
        return {value <= thr} if abs(value - thr) > MARGIN * C * kappa * U53 else {True, False}

    out = set()
    cos_min = float(np.cos(np.float64(min_angle_deg) * (np.pi / 180.0)))
    for behind in sides(point.min_depth, point.k_min_depth, 0.0, C_REF[kind]):
        for wide in ({True} if not min_angle_deg > 0 else sides(point.min_cos, point.k_min_cos, cos_min, C_REF[kind])):
            for low in sides(point.max_err, point.k_max_err, max_error, C_REF["max_err"]):
                out.add(tr.BEHIND if behind else tr.LOW_ANGLE if not wide else tr.OK if low else tr.HIGH_ERROR)
    return out, len(out) > 1


measure_c = st.measure_c


def cost_at(T, X):
    """The sum of squared reprojection errors of a float64 X over the track's observations, in mp."""
    return _derivatives(T.obs, _mp(X))[0]


def _errors(obs, X):
    out = []
    for P, x, y in obs:
        hw = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11]
        du = (P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3]) / hw - x
        dv = (P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7]) / hw - y
        out.append(MP.sqrt(du * du + dv * dv))
    return out


def evaluate_case(T, X):
    """The problem of sfm_tracks_evaluate: the errors of a track's observations at a GIVEN X (float64 [3]).  Its inputs
    are P, the pixels and X, all perturbed as everywhere; the point does not follow the perturbation as the stationary
    point does.  (errors [n] mpf, kappa [n] of each, kappa of their maximum), the kappas in pixels."""
    cams, where = [], []
    for P, _, _ in T.obs:
        k = next((i for i, Q in enumerate(cams) if Q is P), None)
        if k is None:
            k = len(cams)
            cams.append(P)
        where.append(k)
    vals = [v for P in cams for v in P] + [v for _, x, y in T.obs for v in (x, y)] + _mp(X)

    def errors(vals):
        px = vals[12 * len(cams):-3]
        return _errors([(vals[12 * k:12 * k + 12], px[2 * i], px[2 * i + 1]) for i, k in enumerate(where)], vals[-3:])

    err = errors(vals)
    d, dm = [mpf(0)] * len(err), mpf(0)
    for signs in st._draws(len(vals)):
        e2 = errors(st._perturb(vals, signs))
        d = [max(a, abs(b - c)) for a, b, c in zip(d, e2, err)]
        dm = max(dm, abs(max(e2) - max(err)))
    return err, np.array([float(x) for x in d]) / U40, float(dm) / U40


def judge_tracks(X, max_err, kind, mult, what, only=None):
    """A call's X [T,3] and max_err [T] over the tracks of flat() against the truth's `kind` point ("linear" or
    "refined") under mult x C_REF: (failures - each names the quantity -, {scene: worst ratio of X}, {scene: worst ratio of
    max_err}).  Degenerate scenes, undetermined tracks and left-out cases are not judged.  only: the scene names to judge."""
    tracks = truth()[0]
    scene_of = flat()[7]
    fails, wx, we = [], {}, {}
    for i, T in enumerate(tracks):
        sc = scenes()[scene_of[i]]
        if T is None or (only is not None and sc.name not in only):
            continue
        p = getattr(T, kind)
        wx.setdefault(sc.name, 0.0); we.setdefault(sc.name, 0.0)
        if p is None:
            continue
        if not left_out(p.kappa, C_REF[kind]):
            r = ratio_points(X[i], p)
            wx[sc.name] = max(wx[sc.name], r)
            if not r <= mult * C_REF[kind]:
                fails.append(f"{what}, {sc.name}, track {i}: {kind} X is {r:.3g} x kappa 2^-53 off (kappa {p.kappa:.3g}, bound {mult * C_REF[kind]:.4g})")
        if max_err is not None and not max_err_left_out(p, sc.exact):
            r = ratio_max_err(max_err[i], p)
            we[sc.name] = max(we[sc.name], r)
            if not r <= mult * C_REF["max_err"]:
                fails.append(f"{what}, {sc.name}, track {i}: max_err at the {kind} point is {r:.3g} x kappa 2^-53 off "
                             f"(bound {mult * C_REF['max_err']:.4g})")
    return fails, wx, we


def judge_status(status, kind, what, **gates):
    """(failures, share of the tracks outside the degenerate scene that lie in the band)."""
    tracks = truth()[0]
    nv = n_views()
    fails, band, n = [], 0, 0
    for i, T in enumerate(tracks):
        if T is None or getattr(T, kind) is None:
            continue
        allowed, inside = allowed_statuses(getattr(T, kind), kind, int(nv[i]), **gates)
        n += 1
        band += inside
        if int(status[i]) not in allowed:
            fails.append(f"{what}, track {i}: status {int(status[i])}, the truth's gate quantities give {sorted(allowed)}")
    return fails, band / max(n, 1)


def judge_centres(C, mult, what):
    """(failures, worst ratio) of camera centres [n_cams,3] over the cameras of flat()."""
    fails, worst = [], 0.0
    for i, (c, kappa) in enumerate(truth()[1]):
        d = np.asarray(C[i], np.float64).astype(np.longdouble) - c
        n = float(np.sqrt((c * c).sum()))
        if left_out(kappa, C_REF["centre"]):
            continue
        r = _ratio(float(np.sqrt((d * d).sum())) / n if n else float(np.sqrt((d * d).sum())), kappa)
        worst = max(worst, r)
        if not r <= mult * C_REF["centre"]:
            fails.append(f"{what}, camera {i}: centre is {r:.3g} x kappa 2^-53 off (kappa {kappa:.3g}, bound {mult * C_REF['centre']:.4g})")
    return fails, worst


def caps():
    """{scene: {quantity: share left out or undetermined}} under MARGIN x C_REF, outside the degenerate scene."""
    tracks = truth()[0]
    scene_of = flat()[7]
    out = {}
    for s, sc in enumerate(scenes()):
        if sc.degenerate:
            continue
        T = [tracks[i] for i in np.flatnonzero(scene_of == s)]
        n = len(T)
        out[sc.name] = {
            "linear": sum(left_out(t.linear.kappa, C_REF["linear"]) for t in T) / n,
            "refined": sum(t.refined is None or left_out(t.refined.kappa, C_REF["refined"]) for t in T) / n,
            "max_err": sum(t.refined is None or max_err_left_out(t.refined, sc.exact) or max_err_left_out(t.linear, sc.exact) for t in T) / n}
    return out


# --------------------------------------------------------------------------------------------------- the scenes
K_EXACT = np.array([[1024.0, 0, 512], [0, 1024.0, 384], [0, 0, 1]])
N_TRACKS = 50


class Scene:
    """name; proj [n,12]; tracks [(cams [m] int, xy [m,2] float64)]; five: how the 5-step point is treated ("judge",
    "measure"); degenerate: outside the caps, only a status is asked; exact: max_err is zero by construction."""

    def __init__(self, name, proj, tracks, five="judge", degenerate=False, exact=False):
        self.name, self.proj, self.tracks = name, np.ascontiguousarray(proj, np.float64).reshape(-1, 12), tracks
        self.five, self.degenerate, self.exact = five, degenerate, exact


def _cameras(K, n, span, radius=6.0):
    _, Rs, ts, cs = tr.arc_cameras(n, radius=radius, span=span)
    return np.stack([K @ np.hstack([R, t[:, None]]) for R, t in zip(Rs, ts)]), Rs, cs


def _observe(rng, proj, X, cams, noise):
    out = []
    for p, c in zip(X, cams):
        c = np.asarray(c, np.int64)
        h = proj[c].reshape(-1, 3, 4) @ np.append(p, 1.0)
        out.append((c, h[:, :2] / h[:, 2:3] + rng.normal(size=(len(c), 2)) * noise))
    return out


def _subsets(rng, n_cams, lo, hi, n):
    return [np.sort(rng.choice(n_cams, int(rng.integers(lo, hi + 1)), replace=False)) for _ in range(n)]


def _arc_scene(name, seed, K=tr.K_SFM, span=2.0, noise=0.5, lo=2, hi=12, shift=None, away=None, five="judge"):
    rng = np.random.default_rng(seed)
    proj, Rs, cs = _cameras(K, 12, span)
    X = rng.uniform(0, 1, (N_TRACKS, 3))
    if away is not None:                                        # along the middle of the arc's viewing directions
        d = np.array([0.5, 0.5, 0.5]) - cs.mean(axis=0)
        X = 0.5 + away * d / np.linalg.norm(d) + rng.uniform(-1, 1, (N_TRACKS, 3)) * away / 12.0
    tracks = _observe(rng, proj, X, _subsets(rng, 12, lo, hi, N_TRACKS), noise)
    if shift is not None:                                       # P' = P [I | -shift]: the pixels stay
        s = shift * np.array([1.0, 0.7, -0.3])
        proj = proj.copy()
        proj[:, :, 3] -= proj[:, :, :3] @ s
    return Scene(name, proj, tracks, five)


def _long_scene():
    rng = np.random.default_rng(SEED + 20)
    proj, _, _ = _cameras(tr.K_SFM, 600, 2.0)
    lengths = [64] * 6 + [65] * 6 + [300] * 6 + [513] * 6
    cams = [np.sort(rng.choice(600, n, replace=False)) for n in lengths]
    return Scene("tracks of 64, 65, 300, 513 views", proj, _observe(rng, proj, rng.uniform(0, 1, (24, 3)), cams, 0.5))


def _principal_plane_scene():
    """Every track has a camera of its own whose principal plane lies 6e-3 in front of the point: 1e-3 of the depth in
    the arc's cameras.  Noise 5e-4 px: the arc's noise moves the linear point sideways, which the near camera sees a
    thousand times larger, and from 0.002 px on the Hessian at the linear point is indefinite and full Newton leaves
    (8 of 12 tracks; at 0.05 px, where the linear point is 40 px off in the near view, 49 of 50)."""
    rng = np.random.default_rng(SEED + 21)
    proj, Rs, _ = _cameras(tr.K_SFM, 12, 2.0)
    X = rng.uniform(0, 1, (N_TRACKS, 3))
    extra, cams = [], []
    for k, p in enumerate(X):
        R = Rs[int(rng.integers(0, 12))]
        c = p - R.T @ np.array([rng.uniform(-2e-3, 2e-3), rng.uniform(-2e-3, 2e-3), 6e-3])
        extra.append(tr.K_SFM @ np.hstack([R, (-R @ c)[:, None]]))
        arc = np.sort(rng.choice(12, int(rng.integers(2, 7)), replace=False))
        cams.append(np.insert(arc, int(rng.integers(0, len(arc) + 1)), 12 + k))
    proj = np.concatenate([proj, np.stack(extra)])
    return Scene("depth 1e-3 of the others in one view", proj, _observe(rng, proj, X, cams, 5e-4), five="measure")


def _repeated_scene():
    rng = np.random.default_rng(SEED + 22)
    proj, _, _ = _cameras(tr.K_SFM, 12, 2.0)
    cams = []
    for _ in range(N_TRACKS):
        c = rng.permutation(12)[:int(rng.integers(3, 9))]
        c[1] = c[0]                                             # the same camera twice, two observations of its own
        cams.append(c)
    return Scene("a camera seen twice", proj, _observe(rng, proj, rng.uniform(0, 1, (N_TRACKS, 3)), cams, 0.5))


def _zero_rows_scene():
    """Every track has an axis-aligned camera of its own with the point on its axis and the pixel at the principal point:
    its two DLT rows hold exact zeros, so that fold_row's b != 0 skip is taken - first, inside and last in the track."""
    rng = np.random.default_rng(SEED + 23)
    proj, _, _ = _cameras(tr.K_SFM, 12, 2.0)
    X = rng.uniform(0, 1, (N_TRACKS, 3))
    extra, cams = [], []
    for k, p in enumerate(X):
        c = np.array([p[0], p[1], -6.0])
        extra.append(tr.K_SFM @ np.hstack([np.eye(3), -c[:, None]]))
        arc = np.sort(rng.choice(12, int(rng.integers(2, 7)), replace=False))
        cams.append(np.insert(arc, (0, len(arc) // 2, len(arc))[k % 3], 12 + k))
    proj = np.concatenate([proj, np.stack(extra)])
    tracks = _observe(rng, proj, X, cams, 0.5)
    for c, xy in tracks:
        xy[c >= 12] = [512.0, 384.0]
    return Scene("exact zeros in the DLT rows", proj, tracks)


def _two_view_scene():
    rng = np.random.default_rng(SEED + 24)
    proj, _, _ = _cameras(tr.K_SFM, 12, 2.0)
    cams = [np.sort(rng.choice(12, 2, replace=False)) for _ in range(50)]
    projs = [proj]
    for k, deg in enumerate(np.geomspace(0.2, 2.0, 10)):        # ten pairs of their own, 0.2 to 2 degrees of parallax
        projs.append(_cameras(tr.K_SFM, 2, np.deg2rad(deg))[0])
        cams.append(np.array([12 + 2 * k, 13 + 2 * k]))
    proj = np.concatenate(projs)
    X = rng.uniform(0, 1, (60, 3))
    return Scene("two views", proj, _observe(rng, proj, X[:50], cams[:50], 0.5) + _observe(rng, proj, X[50:], cams[50:], 0.1))


def _exact_scene():
    """Three axis-aligned cameras at integer centres, f = 1024, and points with coordinates in {-2, 0, 4, 12}: every depth
    is a power of two and every pixel an exact float64, so the truth is the construction itself."""
    rng = np.random.default_rng(SEED + 25)
    Rs = [np.eye(3), np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]]), np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])]
    cs = [np.array([0.0, 0, -4]), np.array([-4.0, 0, 0]), np.array([0.0, -4, 0])]
    proj = np.stack([K_EXACT @ np.hstack([R, (-R @ c)[:, None]]) for R, c in zip(Rs, cs)])
    grid = np.array([[x, y, z] for x in (-2.0, 0, 4, 12) for y in (-2.0, 0, 4, 12) for z in (-2.0, 0, 4, 12)])
    X = grid[rng.permutation(64)[:N_TRACKS]]
    cams = [np.array(((0, 1, 2), (0, 1), (1, 2), (0, 2))[k % 4]) for k in range(N_TRACKS)]
    sc = Scene("exact", proj, _observe(rng, proj, X, cams, 0.0), exact=True)
    sc.X = X
    return sc


def _degenerate_scene():
    """Pure forward motion with the point on the baseline: both rays are the baseline itself."""
    c = [np.array([0.5, 0.5, -6.0]), np.array([0.5, 0.5, -5.0]), np.array([0.5, 0.5, -3.0])]
    proj = np.stack([tr.K_SFM @ np.hstack([np.eye(3), -x[:, None]]) for x in c])
    X = np.array([[0.5, 0.5, z] for z in (0.5, 2.0, 10.0, -2.0, 300.0)])
    cams = [np.array([0, 1]), np.array([0, 1]), np.array([0, 2]), np.array([0, 1, 2]), np.array([1, 2])]
    return Scene("forward motion, point on the baseline (degenerate)", proj, _observe(np.random.default_rng(0), proj, X, cams, 0.0),
                 degenerate=True)


@functools.lru_cache(maxsize=None)
def scenes():
    """The scenes, in the order of the device call - computed once, never modified."""
    K300 = np.array([[300.0, 0, 187], [0, 300.0, 95], [0, 0, 1]])
    K6000 = np.array([[6000.0, 0, 3310], [0, 6000.0, 1790], [0, 0, 1]])
    return [_arc_scene("baseline", SEED),
            _arc_scene("world shifted by 1e3", SEED + 1, shift=1e3), _arc_scene("world shifted by 1e5", SEED + 2, shift=1e5, lo=4),     # at 2 and 3 views max_err is small enough for its relative bound to pass 1e-6
            _arc_scene("arc of 0.04 rad", SEED + 3, span=0.04, five="measure"),
            _arc_scene("arc of 0.01 rad", SEED + 4, span=0.01, noise=0.05, five="measure"),
            _arc_scene("points 300 away", SEED + 5, away=300.0), _arc_scene("points 3000 away", SEED + 6, away=3000.0, noise=0.05),
            _long_scene(), _principal_plane_scene(),
            _arc_scene("f = 300", SEED + 7, K=K300), _arc_scene("f = 6000", SEED + 8, K=K6000),
            _repeated_scene(), _zero_rows_scene(), _two_view_scene(), _exact_scene(), _degenerate_scene()]


@functools.lru_cache(maxsize=None)
def flat():
    """(args of tr.triangulate / triangulate_tracks_raw for all scenes in one call, scene_of_track [T], first camera of
    each scene): camera = image, every observation a keypoint of its own."""
    projs, cams, xys, lens, scene_of, first = [], [], [], [], [], []
    base = 0
    for s, sc in enumerate(scenes()):
        first.append(base)
        projs.append(sc.proj)
        for c, xy in sc.tracks:
            cams.append(c + base); xys.append(xy); lens.append(len(c)); scene_of.append(s)
        base += len(sc.proj)
    return _flat(np.concatenate(projs), cams, xys) + (np.array(scene_of), np.array(first))


def _flat(proj, cams, xys):
    obs_image = np.concatenate(cams).astype(np.int32)
    uv = np.concatenate(xys)
    n_img = len(proj)
    counts = np.bincount(obs_image, minlength=n_img)
    kp_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    order = np.argsort(obs_image, kind="stable")
    obs_kp = np.empty(len(obs_image), np.int32)
    obs_kp[order] = (np.arange(len(obs_image)) - kp_ptr[obs_image[order]]).astype(np.int32)
    kp_xy = np.empty((len(obs_image), 2))
    kp_xy[kp_ptr[obs_image] + obs_kp] = uv
    track_ptr = np.concatenate([[0], np.cumsum([len(c) for c in cams])]).astype(np.int64)
    return (np.ascontiguousarray(proj).reshape(-1, 12), np.arange(n_img, dtype=np.int32), kp_ptr, kp_xy, track_ptr, obs_image, obs_kp)


def flat_args():
    return flat()[:7]


@functools.lru_cache(maxsize=None)
def truth():
    """([TrackTruth or None (degenerate scene)] per track of flat(), [(C, kappa)] per camera, CPU seconds) - computed
    once per session, never modified."""
    t0 = time.process_time()
    tracks = []
    for sc in scenes():
        for c, xy in sc.tracks:
            tracks.append(None if sc.degenerate else track_truth({int(k): sc.proj[k] for k in set(c.tolist())}, c.tolist(), xy))
    centres = [centre_case(P) for sc in scenes() for P in sc.proj]
    return tracks, centres, time.process_time() - t0


def n_views():
    return np.diff(flat()[4])


# ------------------------------------------------------------------------------------------- essential matrices
def _rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def _essential(R, t):
    t = np.asarray(t, np.float64) / np.linalg.norm(t)
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R


@functools.lru_cache(maxsize=None)
def essentials():
    """[(name, E [3,3])], 80 matrices - computed once, never modified."""
    rng = np.random.default_rng(SEED + 40)
    base = []
    for _ in range(10):
        R = pr.random_rotation(rng)
        base.append((R, rng.normal(size=3)))
    out = []
    for k, (R, t) in enumerate(base):
        E = _essential(R, t)
        out += [(f"essential {k}", E), (f"essential {k} x 1e-6", E * 1e-6), (f"essential {k} x 1e6", E * 1e6)]
    for k, (R, t) in enumerate(base):
        E = _essential(R, t)
        out.append((f"essential {k} rounded to float32", E.astype(np.float32).astype(np.float64)))
        out.append((f"essential {k} with 1e-3 noise", E * (1 + 1e-3 * rng.normal(size=(3, 3)))))
    for k in range(2):
        t = rng.normal(size=3)
        for name, a in (("0", 0.0), ("1e-8", 1e-8), ("pi - 1e-8", np.pi - 1e-8)):
            out.append((f"rotation by {name} about baseline {k}", _essential(_rot(t, a), t)))
    for k, axis in enumerate(np.eye(3)):
        out.append((f"t along axis {k}", _essential(base[k][0], axis)))
        out.append((f"t along axis {k}, negative", _essential(base[3 + k][0], -axis)))
    for k in range(5):
        E = _essential(*base[k])
        out += [(f"essential {k} transposed", E.T.copy()), (f"essential {k} negated", -E)]
    import essential_reference as er
    pairs = er.shipped_pairs()
    for i in er.SHIPPED[:8]:
        out.append((f"shipped pair {i}", pr.essential_from_fundamental(pairs[i][2], pr.K_REF)))
    assert len(out) == 80
    return out


@functools.lru_cache(maxsize=None)
def pose_truths():
    t0 = time.process_time()
    out = [pose_truth(E) for _, E in essentials()]
    return out, time.process_time() - t0
