"""NumPy float64 reference of the batched PnP RANSAC (sfm_amd/csrc/pnp.hip), taking the samples as input, plus the
sample generator (tests/ransac_reference.py at 3 slots) and the synthetic views the tests share.

It is a reference for the tests, not a second implementation to fall back to, and not the kernel's algebra restated:
the kernel intersects the conics of the depth pencil (one cubic root, two quadratics, Newton polish, frame-to-frame
pose); here the depths come from Grunert's quartic through np.roots and the pose from a rigid alignment of the three
points by SVD.

    bearings   f = normalise(K^-1 [u, v, 1])
    inlier     p = K [R|t] [X; 1]:  p2 > 0  and  (p0 - u p2)^2 + (p1 - v p2)^2 <= thr^2 p2^2     (no division)
    degenerate sample (no model):  |(P1-P0) x (P2-P0)|^2 <= 1e-20 |P1-P0|^2 |P2-P0|^2, or a non-finite coordinate
"""
import numpy as np

import ransac_reference
from fundamental_reference import K_REF


def draw_samples(seed, segment, n_points, n_hyp):
    """[n_hyp, 3] int32: the samples drawn for segment `segment` holding `n_points` points (all -1 under 4)."""
    return ransac_reference.draw_samples(seed, segment, n_points, n_hyp, 3, 4)


# ------------------------------------------------------------------------------------------------ geometry
def k_matrix(k4):
    fx, fy, cx, cy = (float(v) for v in k4)
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def bearings(uv, K):
    """Unit rays of pixels uv [M,2] through K."""
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    f = np.stack([(uv[:, 0] - K[0, 2]) / K[0, 0], (uv[:, 1] - K[1, 2]) / K[1, 1], np.ones(len(uv))], 1)
    with np.errstate(invalid="ignore"):
        return f / np.linalg.norm(f, axis=1)[:, None]


def degenerate(P):
    """The rule of the kernel: a triangle without area, or a non-finite coordinate, gives no model."""
    with np.errstate(invalid="ignore", over="ignore"):
        d1, d2 = P[1] - P[0], P[2] - P[0]
        n = np.cross(d1, d2)
        return not (n @ n > 1e-20 * (d1 @ d1) * (d2 @ d2))


def _polish_depths(s, P, f):
    """Three Newton steps on |s_i f_i - s_j f_j|^2 = |P_i - P_j|^2 (np.linalg.solve).  The quartic's roots lose
    digits when the triangle is small against its distance (all four roots crowd near 1: the shipped scene), and the
    congruence test below would then drop a correct pose."""
    pairs = ((0, 1), (0, 2), (1, 2))
    for _ in range(3):
        g = np.array([((s[i] * f[i] - s[j] * f[j]) ** 2).sum() - ((P[i] - P[j]) ** 2).sum() for i, j in pairs])
        J = np.zeros((3, 3))
        for r, (i, j) in enumerate(pairs):
            J[r, i] = 2 * (s[i] - (f[i] @ f[j]) * s[j])
            J[r, j] = 2 * (s[j] - (f[i] @ f[j]) * s[i])
        try:
            step = np.linalg.solve(J, g)
        except np.linalg.LinAlgError:
            break
        if not np.isfinite(step).all():
            break
        s = s - step
    return s


def p3p(P, f):
    """P [3,3] world points, f [3,3] unit bearings -> list of up to four (R, t) with depth_i f_i = R P_i + t.
    Grunert's quartic in v = s3 / s1 (as in Haralick et al., "Review and analysis of solutions of the three point
    perspective pose estimation problem", 1994), u = s2 / s1 from v, the depths polished by Newton on the three
    distance equations, then the rigid motion of the three points.  A root is taken as real when
    |imag| <= 1e-7 (1 + |real|); a candidate is kept when both ratios and the depths are positive and the aligned
    triangle meets the three camera points within 1e-6 of their size."""
    P = np.asarray(P, dtype=np.float64)
    f = np.asarray(f, dtype=np.float64)
    if not (np.isfinite(P).all() and np.isfinite(f).all()) or degenerate(P):
        return []
    a2, b2, c2 = ((P[1] - P[2]) ** 2).sum(), ((P[0] - P[2]) ** 2).sum(), ((P[0] - P[1]) ** 2).sum()
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    k1, k2, k3, k4 = (a2 - c2) / b2, (a2 + c2) / b2, (b2 - c2) / b2, (b2 - a2) / b2
    A4 = (k1 - 1) ** 2 - 4 * c2 / b2 * ca * ca
    A3 = 4 * (k1 * (1 - k1) * cb - (1 - k2) * ca * cg + 2 * c2 / b2 * ca * ca * cb)
    A2 = 2 * (k1 * k1 - 1 + 2 * k1 * k1 * cb * cb + 2 * k3 * ca * ca - 4 * k2 * ca * cb * cg + 2 * k4 * cg * cg)
    A1 = 4 * (-k1 * (1 + k1) * cb + 2 * a2 / b2 * cg * cg * cb - (1 - k2) * ca * cg)
    A0 = (1 + k1) ** 2 - 4 * a2 / b2 * cg * cg
    co = np.array([A4, A3, A2, A1, A0])
    if not np.isfinite(co).all() or abs(A4) < 1e-14 * np.abs(co).max():
        return []
    out = []
    for v in np.roots(co):
        if abs(v.imag) > 1e-7 * (1 + abs(v.real)):
            continue
        v = v.real
        den = 2 * (cg - v * ca)
        if v <= 0 or den == 0:
            continue
        u = ((k1 - 1) * v * v - 2 * k1 * cb * v + 1 + k1) / den
        d = 1 + v * v - 2 * v * cb
        if u <= 0 or d <= 0:
            continue
        s1 = np.sqrt(b2 / d)
        s = _polish_depths(np.array([s1, u * s1, v * s1]), P, f)
        if not (s > 0).all():
            continue
        Q = f * s[:, None]
        pc, qc = P.mean(0), Q.mean(0)
        U, _, Vt = np.linalg.svd((Q - qc).T @ (P - pc))                 # Kabsch: the points are coplanar, so the
        R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt           # third direction is fixed by det = +1
        t = qc - R @ pc
        if np.abs(P @ R.T + t - Q).max() > 1e-6 * np.abs(Q).max():
            continue
        out.append((R, t))
    return out[:4]


def projection(K, R, t):
    return K @ np.c_[R, np.asarray(t, dtype=np.float64).reshape(3)]


def inliers(K, R, t, X, uv, threshold):
    """The kernel's rule, without division; a non-finite point fails it."""
    Pm = projection(K, R, t)
    with np.errstate(invalid="ignore", over="ignore"):
        p = X @ Pm[:, :3].T + Pm[:, 3]
        e0, e1 = p[:, 0] - uv[:, 0] * p[:, 2], p[:, 1] - uv[:, 1] * p[:, 2]
        return (p[:, 2] > 0) & (e0 * e0 + e1 * e1 <= threshold * threshold * p[:, 2] * p[:, 2])


def residuals(x, K, X, uv):
    """Reprojection residuals [2k] of the pose x = (rvec, t) in pixels."""
    from sfm_amd.rotation import rodrigues
    p = X @ rodrigues(x[:3]).T + x[3:6]
    return np.r_[K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2] - uv[:, 0], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2] - uv[:, 1]]


def cost(K, R, t, X, uv):
    """Summed squared reprojection error of (R, t) over the given points."""
    from sfm_amd.rotation import log_so3
    return float((residuals(np.r_[log_so3(R), np.asarray(t).reshape(3)], K, X, uv) ** 2).sum())


def refit(K, R, t, X, uv):
    from scipy.optimize import least_squares
    from sfm_amd.rotation import log_so3, rodrigues
    o = least_squares(residuals, np.r_[log_so3(R), np.asarray(t).reshape(3)], args=(K, X, uv), method="lm",
                      xtol=1e-14, ftol=1e-14)
    return rodrigues(o.x[:3]), o.x[3:6].copy()


def _exp_so3(w):
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-2:
        a, b = 1 - th * th / 6 + th ** 4 / 120, 0.5 - th * th / 24 + th ** 4 / 720
    else:
        a, b = np.sin(th) / th, (1 - np.cos(th)) / (th * th)
    return np.eye(3) + a * Kx + b * (Kx @ Kx)


def local_sums(K, R, t, X, uv):
    """(J^T J [6,6], J^T r [6], r^T r) of the reprojection residuals in pixels, for the unknowns (w, t) of the local
    parametrisation R <- exp([w]x) R taken at w = 0: d(pixel)/dy [-[R X]x | I] with y = R X + t."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    q = X @ R.T
    y = q + t
    iz = 1.0 / y[:, 2]
    ru, rv = fx * y[:, 0] * iz + cx - uv[:, 0], fy * y[:, 1] * iz + cy - uv[:, 1]
    a0, a2, c1, c2 = fx * iz, -fx * y[:, 0] * iz * iz, fy * iz, -fy * y[:, 1] * iz * iz
    z = np.zeros_like(iz)
    ju = np.stack([a2 * q[:, 1], a0 * q[:, 2] - a2 * q[:, 0], -a0 * q[:, 1], a0, z, a2], 1)
    jv = np.stack([c2 * q[:, 1] - c1 * q[:, 2], -c2 * q[:, 0], c1 * q[:, 0], z, c1, c2], 1)
    return ju.T @ ju + jv.T @ jv, ju.T @ ru + jv.T @ rv, float(ru @ ru + rv @ rv)


LM_ITERS = 30


def lm_refit(K, R, t, X, uv, max_steps=LM_ITERS):
    """The kernel's Levenberg-Marquardt (k_pnp_refine) in float64 NumPy over the given points: the same update
    R <- exp([w]x) R, t <- t + d, the same damping (H + mu diag H, mu from 1e-3, x 0.1 on a step that lowers the cost and
    never under 1e-12, x 10 otherwise) and the same stop, |step| <= 1e-12 (1 + |(angle(R), t)|) or max_steps steps.
    Returns (R, t, the number of steps tried)."""
    X, uv = np.asarray(X, np.float64).reshape(-1, 3), np.asarray(uv, np.float64).reshape(-1, 2)
    R, t = np.array(R, np.float64), np.array(t, np.float64).reshape(3)
    Rn, tn, mu, have, it = R, t, 1e-3, None, 0
    for it in range(max_steps + 1):
        with np.errstate(all="ignore"):
            got = local_sums(K, Rn, tn, X, uv)
        if it == 0 or got[2] < have[2]:
            have, R, t = got, Rn, tn
            if it > 0:
                mu = max(mu * 0.1, 1e-12)
        else:
            mu *= 10.0
        if it == max_steps or not np.isfinite(have[2]):
            break
        Hm, g, _ = have
        try:
            L = np.linalg.cholesky(Hm + mu * np.diag(np.diag(Hm)))
        except np.linalg.LinAlgError:
            break
        d = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        if not np.isfinite(d).all():
            break
        v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        ang = np.arctan2(0.5 * np.linalg.norm(v), 0.5 * (np.trace(R) - 1.0))
        if np.linalg.norm(d) <= 1e-12 * (1.0 + np.sqrt(ang * ang + t @ t)):
            break
        Rn, tn = _exp_so3(d[:3]) @ R, t + d[3:]
    return R, t, it


def ransac(X, uv, K, samples, threshold=8.0, refine=False):
    """Follows the device for one segment on given samples [H,3].  Returns a dict: `hyp_count` [H] (best candidate
    count per hypothesis), `status` (0 ok, 1 fewer than 4 points, 2 no model), `R`, `t` (or None), `mask` [M] bool,
    `n_inliers`, `refined`, `winner` (hypothesis index) and `cand_count` [H,4]."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    K = np.asarray(K, dtype=np.float64)
    M, H = len(X), len(samples)
    res = {"hyp_count": np.zeros(H, np.int32), "status": 1, "R": None, "t": None, "mask": np.zeros(M, bool),
           "n_inliers": 0, "refined": False, "winner": -1, "cand_count": np.zeros((H, 4), np.int32)}
    if M < 4:
        return res
    f = bearings(uv, K)
    cnt = np.zeros((H, 4), np.int32)
    best = (0, None)
    for h, s in enumerate(np.asarray(samples, dtype=np.int64)):
        for k, (R, t) in enumerate(p3p(X[s], f[s])):
            cnt[h, k] = inliers(K, R, t, X, uv, threshold).sum()
            if cnt[h, k] > best[0]:                      # first maximum: lowest hypothesis, then lowest candidate
                best = (int(cnt[h, k]), (h, R, t))
    res["cand_count"] = cnt
    res["hyp_count"] = cnt.max(1).astype(np.int32)
    res["status"] = 2
    if best[0] == 0:
        return res
    h, R, t = best[1]
    mask = inliers(K, R, t, X, uv, threshold)
    res.update(status=0, R=R, t=t, mask=mask, n_inliers=int(mask.sum()), winner=int(h))
    if refine and mask.sum() >= 3:                       # 6 residuals for 6 unknowns, as the kernel asks
        Rr, tr = refit(K, R, t, X[mask], uv[mask])
        if np.isfinite(Rr).all() and np.isfinite(tr).all():
            mr = inliers(K, Rr, tr, X, uv, threshold)
            if mr.sum() >= mask.sum():
                res.update(R=Rr, t=tr, mask=mr, n_inliers=int(mr.sum()), refined=True)
    return res


def stable(X, uv, K, samples, threshold=8.0):
    """[H] bool: True where hyp_count does not change when X is replaced by X (1 + 1e-13 N(0,1)), for two fixed-seed
    replays.  A hypothesis near a double root gains or loses a candidate under such a change; comparing it with the
    device would compare rounding."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    base = ransac(X, uv, K, samples, threshold)["hyp_count"]
    ok = np.ones(len(samples), bool)
    for rep in range(2):
        rng = np.random.default_rng(77 + rep)
        ok &= ransac(X * (1 + 1e-13 * rng.standard_normal(X.shape)), uv, K, samples, threshold)["hyp_count"] == base
    return ok


# ---------------------------------------------------------------------------------------- synthetic views
CASES = [(3, 0.0), (4, 0.0), (40, 0.3), (300, 0.3), (300, 0.6), (2000, 0.5)]       # (M, outlier share), ONE batch


def synth_view(rng, M, outlier_share=0.0, noise=0.5):
    """Points in a box in front of a camera with the reference's K; the first int(M * outlier_share) pixels are
    replaced by uniform ones.  Returns X [M,3] float64, uv [M,2] float32 and the true R, t."""
    X = rng.uniform(-1, 1, (M, 3)) + [0, 0, 6.0]
    yaw = 0.25
    R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    t = np.array([-1.5, 0.1, 0.3])
    x = (X @ R.T + t) @ K_REF.T
    x = x[:, :2] / x[:, 2:]
    if noise:
        x = x + rng.normal(size=x.shape) * noise
    k = int(M * outlier_share)
    x[:k] = rng.uniform(0, 1, (k, 2)) * [1024, 768]
    return X, x.astype(np.float32), R, t


def synth_batch():
    out = [synth_view(np.random.default_rng(1000 * M + int(100 * share)), M, share) for M, share in CASES]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], [o[3] for o in out]
