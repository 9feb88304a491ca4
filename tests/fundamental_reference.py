"""NumPy float64 restatement of the batched fundamental-matrix RANSAC (sfm_amd/csrc/twoview.hip), taking the samples
as input, plus its sample generator (tests/ransac_reference.py at 7 slots) and the synthetic two-view scenes the tests share.

It is a reference for the tests, not a second implementation to fall back to: null space by np.linalg.svd, the cubic
through four determinant evaluations and np.roots, where the kernel rotates columns and solves in closed form.

    row of the system for x1=(a,b), x2=(c,d):  [c*a, c*b, c, d*a, d*b, d, a, b, 1]
    err(F, x1, x2) = max( s^2/((F x1)_0^2 + (F x1)_1^2), s^2/((F^T x2)_0^2 + (F^T x2)_1^2) ),  s = x2^T F x1
"""
import functools

import numpy as np

import ransac_reference
from ransac_reference import mix64  # noqa: F401


def draw_samples(seed, segment, n_points, n_hyp):
    """[n_hyp, 7] int32: the samples drawn for segment `segment` holding `n_points` matches (all -1 under 7)."""
    return ransac_reference.draw_samples(seed, segment, n_points, n_hyp, 7, 7)


# ------------------------------------------------------------------------------------------------ geometry
def hartley(p):
    """3x3 transform: centroid to the origin, mean distance sqrt(2), over the finite rows of p."""
    c = p.mean(0)
    d = np.sqrt(((p - c) ** 2).sum(1)).mean()
    s = np.sqrt(2.0) / d if d > 0 else 1.0
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def system_rows(x1, x2):
    a, b = x1[..., 0], x1[..., 1]
    c, d = x2[..., 0], x2[..., 1]
    return np.stack([c * a, c * b, c, d * a, d * b, d, a, b, np.ones_like(a)], -1)


def seven_point(x1, x2):
    """x1, x2 [H,7,2] normalised.  Returns F [H,3,3,3] (root slot, ascending real roots) and valid [H,3]."""
    H = x1.shape[0]
    A = system_rows(x1, x2)
    out = np.zeros((H, 3, 3, 3))
    ok = np.zeros((H, 3), bool)
    fin = np.isfinite(A).all(axis=(1, 2))
    Vt = np.zeros((H, 9, 9))
    if fin.any():
        Vt[fin] = np.linalg.svd(A[fin])[2]
    F1 = Vt[:, 7].reshape(H, 3, 3)
    F2 = Vt[:, 8].reshape(H, 3, 3)
    lam = np.array([-1.0, 0.0, 1.0, 2.0])
    dets = np.stack([np.linalg.det(l * F1 + (1 - l) * F2) for l in lam], -1)
    co = np.linalg.solve(np.vander(lam, 4, increasing=True), dets.T).T        # c0..c3
    for h in np.flatnonzero(fin):
        cc = co[h]
        if not np.all(np.isfinite(cc)) or abs(cc[3]) < 1e-14 * np.abs(cc).max():
            continue
        r = np.roots(cc[::-1])
        r = np.sort(r[np.abs(r.imag) < 1e-9 * (1 + np.abs(r.real))].real)
        for k, l in enumerate(r[:3]):
            out[h, k] = l * F1[h] + (1 - l) * F2[h]
            ok[h, k] = True
    return out, ok


def cv_err2(F, p1, p2):
    """The larger of the two squared point-line distances.  F [...,3,3], p [M,2] -> [...,M]; NaN where undefined."""
    x1 = np.c_[p1, np.ones(len(p1))]
    x2 = np.c_[p2, np.ones(len(p2))]
    l2 = np.einsum("...ij,mj->...mi", F, x1)          # F x1
    l1 = np.einsum("...ji,mj->...mi", F, x2)          # F^T x2
    s = (l2 * x2).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d2 = s * s / (l2[..., 0] ** 2 + l2[..., 1] ** 2)
        d1 = s * s / (l1[..., 0] ** 2 + l1[..., 1] ** 2)
        e = np.maximum(d1, d2)
    bad = ~(np.isfinite(p1).all(1) & np.isfinite(p2).all(1))
    e = np.where(bad, np.nan, e)
    return e


def inliers(F, p1, p2, threshold):
    with np.errstate(invalid="ignore"):
        return cv_err2(F, p1, p2) <= threshold * threshold


def sym_err(F, p1, p2):
    """The reference's verification metric (find_matches.py:160-174) in float64: mean of the two point-line distances."""
    x1 = np.c_[p1, np.ones(len(p1))]
    x2 = np.c_[p2, np.ones(len(p2))]
    l2 = x1 @ F.T
    l1 = x2 @ F
    e1 = np.abs((l1 * x1).sum(1)) / np.hypot(l1[:, 0], l1[:, 1])
    e2 = np.abs((l2 * x2).sum(1)) / np.hypot(l2[:, 0], l2[:, 1])
    return (e1 + e2) / 2


def _scale(F):
    with np.errstate(divide="ignore", invalid="ignore"):
        G = F / F[2, 2]
    return G if F[2, 2] != 0 and np.isfinite(G).all() else F


def refit(p1, p2, T1, T2, mask):
    """Normalised 8-point least squares over mask (the segment's transforms), rank 2 enforced; None if not finite."""
    x1 = (np.c_[p1[mask], np.ones(mask.sum())] @ T1.T)[:, :2]
    x2 = (np.c_[p2[mask], np.ones(mask.sum())] @ T2.T)[:, :2]
    A = system_rows(x1, x2)
    w, V = np.linalg.eigh(A.T @ A)
    U, sv, Vt = np.linalg.svd(V[:, 0].reshape(3, 3))
    sv[2] = 0.0
    F = T2.T @ (U @ np.diag(sv) @ Vt) @ T1
    return _scale(F) if np.isfinite(F).all() else None


def ransac(p1, p2, samples, threshold=3.0, refine=False):
    """Follows the device for one pair on given samples [H,7].  Returns a dict: `hyp_count` [H] (best candidate count per
    hypothesis), `status` (0 ok, 1 fewer than 7 matches, 2 no model), `F` (scaled to F[2,2] = 1, or None), `mask` [M] bool,
    `n_inliers`, `refined`, `winner` (hypothesis index) and `cand_count` [H,3]."""
    p1 = np.asarray(p1, dtype=np.float64).reshape(-1, 2)
    p2 = np.asarray(p2, dtype=np.float64).reshape(-1, 2)
    M, H = len(p1), len(samples)
    res = {"hyp_count": np.zeros(H, np.int32), "status": 1, "F": None, "mask": np.zeros(M, bool), "n_inliers": 0,
           "refined": False, "winner": -1, "cand_count": np.zeros((H, 3), np.int32)}
    if M < 7:
        return res
    fin = np.isfinite(p1).all(1) & np.isfinite(p2).all(1)
    if fin.any():
        T1, T2 = hartley(p1[fin]), hartley(p2[fin])
    else:
        T1 = T2 = np.eye(3)
    with np.errstate(invalid="ignore", over="ignore"):
        n1 = (np.c_[p1, np.ones(M)] @ T1.T)[:, :2]
        n2 = (np.c_[p2, np.ones(M)] @ T2.T)[:, :2]
    n1[~fin] = np.nan
    n2[~fin] = np.nan
    idx = np.asarray(samples, dtype=np.int64)
    Fn, ok = seven_point(n1[idx], n2[idx])
    F = np.einsum("ji,hkjl,lm->hkim", T2, Fn, T1)     # T2^T Fn T1
    ok &= np.isfinite(F).all(axis=(2, 3))
    F[~ok] = 0.0
    with np.errstate(invalid="ignore"):
        cnt = ((cv_err2(F, p1, p2) <= threshold * threshold) & ok[..., None]).sum(-1)      # [H,3]
    res["cand_count"] = cnt.astype(np.int32)
    res["hyp_count"] = cnt.max(1).astype(np.int32)
    res["status"] = 2
    if cnt.max() == 0:
        return res
    h, k = np.unravel_index(np.argmax(cnt), cnt.shape)        # first maximum: lowest hypothesis, then lowest root
    Fw = _scale(F[h, k])
    mask = inliers(Fw, p1, p2, threshold)
    res.update(status=0, F=Fw, mask=mask, n_inliers=int(mask.sum()), winner=int(h))
    if refine and mask.sum() >= 8:
        Fr = refit(p1, p2, T1, T2, mask)
        if Fr is not None:
            mr = inliers(Fr, p1, p2, threshold)
            if mr.sum() >= mask.sum():
                res.update(F=Fr, mask=mr, n_inliers=int(mr.sum()), refined=True)
    return res


# ---------------------------------------------------------------------------------------- synthetic scenes
K_REF = np.array([[1228.0, 0, 512], [0, 1228.0, 384], [0, 0, 1]])


def true_fundamental(R, t, K=K_REF):
    """K^-T [t]x R K^-1 scaled to F[2,2] = 1, for X2 = R X1 + t."""
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return F / F[2, 2]


def synth_pair(rng, M, outlier_share=0.0, noise=0.5, float32=True, yaw=0.25, t=(-1.5, 0.1, 0.3)):
    """Points in a box in front of two cameras with the reference's K; the first int(M * outlier_share) matches get a
    uniform random second point.  Returns pts1, pts2 [M,2] (float32-rounded unless float32=False) and the true F."""
    X = rng.uniform(-1, 1, (M, 3)) + [0, 0, 6.0]
    R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    t = np.asarray(t, dtype=np.float64)
    x1 = X @ K_REF.T
    x1 = x1[:, :2] / x1[:, 2:]
    x2 = (X @ R.T + t) @ K_REF.T
    x2 = x2[:, :2] / x2[:, 2:]
    if noise:
        x1 = x1 + rng.normal(size=x1.shape) * noise
        x2 = x2 + rng.normal(size=x2.shape) * noise
    k = int(M * outlier_share)
    x2[:k] = rng.uniform(0, 1, (k, 2)) * [1024, 768]
    if float32:
        x1, x2 = x1.astype(np.float32), x2.astype(np.float32)
    return x1, x2, true_fundamental(R, t)


CASES = [(7, 0.0), (8, 0.0), (40, 0.3), (300, 0.3), (300, 0.6), (2000, 0.5)]       # (M, outlier share), ONE batch


@functools.lru_cache(maxsize=None)
def synth_batch():
    """(pts1 list, pts2 list, true F list) of CASES - computed once, never modified."""
    out = []
    for M, share in CASES:
        rng = np.random.default_rng(1000 * M + int(100 * share))
        out.append(synth_pair(rng, M, share, noise=0.5))
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]
