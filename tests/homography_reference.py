"""NumPy float64 restatement of the batched homography RANSAC (sfm_amd/csrc/homography.hip), taking the samples as
input, plus its sample generator (tests/ransac_reference.py at 4 slots) and the scenes the tests share: a general one, a
pure rotation and a plane.

It is a reference for the tests, not a second implementation to fall back to: null space by np.linalg.svd where the
kernel rotates columns, the refit's eigenvector by np.linalg.eigh where the kernel runs a cyclic Jacobi.

    sample rule   per triple (i, j, k) of (0,1,2), (0,1,3), (0,2,3), (1,2,3) and image, on the float32 pixels as double:
                  a = (xj-xi)(yk-yi) - (yj-yi)(xk-xi), d1 = |pj-pi|^2, d2 = |pk-pi|^2; no model unless a^2 > 1e-6 d1 d2 in
                  both images, none if (a1 > 0) != (a2 > 0), none on a non-finite coordinate
    rows          [x, y, 1, 0, 0, 0, -u x, -u y, -u], [0, 0, 0, x, y, 1, -v x, -v y, -v] on Hartley-normalised coordinates
    inlier        X = (h0 x + h1 y) + h2, Y = (h3 x + h4 y) + h5, W = (h6 x + h7 y) + h8:
                  W != 0 and (X - u W)^2 + (Y - v W)^2 <= thr^2 W^2
"""
import numpy as np

import fundamental_reference as fr
import ransac_reference

MIN_SAMPLE = 4
TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))


def draw_samples(seed, segment, n_points, n_hyp):
    """[n_hyp, 4] int32: the samples drawn for segment `segment` holding `n_points` matches (all -1 under 4)."""
    return ransac_reference.draw_samples(seed, segment, n_points, n_hyp, 4, 4)


def voided(p1, p2, samples):
    """[H] bool: the samples that give no model by the sample rule."""
    idx = np.asarray(samples, dtype=np.int64)
    a = np.asarray(p1, dtype=np.float32)[idx].astype(np.float64)          # [H,4,2]
    b = np.asarray(p2, dtype=np.float32)[idx].astype(np.float64)
    bad = ~(np.isfinite(a).all(axis=(1, 2)) & np.isfinite(b).all(axis=(1, 2)))
    with np.errstate(invalid="ignore", over="ignore"):
        for i, j, k in TRIPLES:
            pos = []
            for p in (a, b):
                e1, e2 = p[:, j] - p[:, i], p[:, k] - p[:, i]
                ar = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
                bad |= ~(ar * ar > 1e-6 * (e1 * e1).sum(1) * (e2 * e2).sum(1))
                pos.append(ar > 0)
            bad |= pos[0] != pos[1]
    return bad


def system_rows(x1, x2):
    """x1, x2 [...,2] -> [...,2,9]: the two rows of each match."""
    x, y, u, v = x1[..., 0], x1[..., 1], x2[..., 0], x2[..., 1]
    o, z = np.ones_like(x), np.zeros_like(x)
    return np.stack([np.stack([x, y, o, z, z, z, -u * x, -u * y, -u], -1),
                     np.stack([z, z, z, x, y, o, -v * x, -v * y, -v], -1)], -2)


def four_point(x1, x2):
    """x1, x2 [H,4,2] normalised -> Hn [H,3,3] (zero where the system is not finite) and ok [H]."""
    n = x1.shape[0]
    A = system_rows(x1, x2).reshape(n, 8, 9)
    fin = np.isfinite(A).all(axis=(1, 2))
    out = np.zeros((n, 3, 3))
    if fin.any():
        out[fin] = np.linalg.svd(A[fin])[2][:, 8].reshape(-1, 3, 3)
    return out, fin


def inlier_counts(Hm, p1, p2, threshold):
    """[...,M] bool for Hm [...,3,3]: the rule, bracketed as the kernel brackets it.  Non-finite matches never count."""
    h = Hm.reshape(Hm.shape[:-2] + (9, 1))
    x, y, u, v = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    with np.errstate(all="ignore"):
        X = (h[..., 0, :] * x + h[..., 1, :] * y) + h[..., 2, :]
        Y = (h[..., 3, :] * x + h[..., 4, :] * y) + h[..., 5, :]
        W = (h[..., 6, :] * x + h[..., 7, :] * y) + h[..., 8, :]
        dx, dy = X - u * W, Y - v * W
        ok = (W != 0) & (dx * dx + dy * dy <= threshold * threshold * (W * W))
    return ok & np.isfinite(p1).all(1) & np.isfinite(p2).all(1)


def residuals(Hm, p1, p2):
    """(e, w2) [M] each of one H [3,3]: the two sides of the rule, e = (X - u W)^2 + (Y - v W)^2 and w2 = W^2."""
    h = np.asarray(Hm, dtype=np.float64).reshape(9)
    p1 = np.asarray(p1, dtype=np.float64).reshape(-1, 2)
    p2 = np.asarray(p2, dtype=np.float64).reshape(-1, 2)
    x, y, u, v = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    with np.errstate(all="ignore"):
        X, Y, W = (h[0] * x + h[1] * y) + h[2], (h[3] * x + h[4] * y) + h[5], (h[6] * x + h[7] * y) + h[8]
        dx, dy = X - u * W, Y - v * W
        return dx * dx + dy * dy, W * W


def inliers(Hm, p1, p2, threshold):
    p1 = np.asarray(p1, dtype=np.float64).reshape(-1, 2)
    p2 = np.asarray(p2, dtype=np.float64).reshape(-1, 2)
    return inlier_counts(np.asarray(Hm, dtype=np.float64).reshape(3, 3), p1, p2, threshold)


def _scale(Hm):
    with np.errstate(divide="ignore", invalid="ignore"):
        G = Hm / Hm[2, 2]
    return G if Hm[2, 2] != 0 and np.isfinite(G).all() else Hm


def transforms(p1, p2):
    fin = np.isfinite(p1).all(1) & np.isfinite(p2).all(1)
    if fin.any():
        return fr.hartley(p1[fin]), fr.hartley(p2[fin]), fin
    return np.eye(3), np.eye(3), fin


def refit(p1, p2, T1, T2, mask):
    """Normalised DLT over mask (the segment's transforms); None if not finite."""
    x1 = (np.c_[p1[mask], np.ones(mask.sum())] @ T1.T)[:, :2]
    x2 = (np.c_[p2[mask], np.ones(mask.sum())] @ T2.T)[:, :2]
    A = system_rows(x1, x2).reshape(-1, 9)
    w, V = np.linalg.eigh(A.T @ A)
    Hm = np.linalg.inv(T2) @ V[:, 0].reshape(3, 3) @ T1
    return _scale(Hm) if np.isfinite(Hm).all() else None


def ransac(p1, p2, samples, threshold=3.0, refine=False, scale=None):
    """Follows the device for one pair on given samples [H,4].  Returns a dict: `hyp_count` [H], `status` (0 ok, 1 fewer
    than 4 matches, 2 no hypothesis with an inlier), `H` (scaled to H[2,2] = 1, or None), `mask` [M] bool, `n_inliers`,
    `refined`, `winner` (hypothesis index) and `voided` [H].
    scale: optional ([M,2], [M,2]) factors on the normalised coordinates the solver sees (`stable`)."""
    p1 = np.asarray(p1, dtype=np.float64).reshape(-1, 2)
    p2 = np.asarray(p2, dtype=np.float64).reshape(-1, 2)
    M, n = len(p1), len(samples)
    res = {"hyp_count": np.zeros(n, np.int32), "status": 1, "H": None, "mask": np.zeros(M, bool), "n_inliers": 0,
           "refined": False, "winner": -1, "voided": np.ones(n, bool)}
    if M < MIN_SAMPLE:
        return res
    idx = np.asarray(samples, dtype=np.int64)
    void = voided(p1, p2, idx)
    T1, T2, fin = transforms(p1, p2)
    with np.errstate(invalid="ignore", over="ignore"):
        n1 = (np.c_[p1, np.ones(M)] @ T1.T)[:, :2]
        n2 = (np.c_[p2, np.ones(M)] @ T2.T)[:, :2]
        if scale is not None:
            n1, n2 = n1 * scale[0], n2 * scale[1]
    n1[~fin] = np.nan
    n2[~fin] = np.nan
    live = np.flatnonzero(~void)
    Hs, ok = np.zeros((n, 3, 3)), np.zeros(n, bool)
    if len(live):
        Hn, ok[live] = four_point(n1[idx[live]], n2[idx[live]])
        Hs[live] = np.linalg.inv(T2) @ Hn @ T1
    ok &= np.isfinite(Hs).all(axis=(1, 2))
    Hs[~ok] = 0.0
    cnt = inlier_counts(Hs, p1, p2, threshold).sum(-1)
    res["hyp_count"] = cnt.astype(np.int32)
    res["voided"] = void
    res["status"] = 2
    if cnt.max() == 0:
        return res
    h = int(np.argmax(cnt))                                              # first maximum: the lowest hypothesis
    Hw = _scale(Hs[h])
    mask = inliers(Hw, p1, p2, threshold)
    res.update(status=0, H=Hw, mask=mask, n_inliers=int(mask.sum()), winner=h)
    if refine and mask.sum() >= MIN_SAMPLE:
        Hr = refit(p1, p2, T1, T2, mask)
        if Hr is not None:
            mr = inliers(Hr, p1, p2, threshold)
            if mr.sum() >= mask.sum():
                res.update(H=Hr, mask=mr, n_inliers=int(mr.sum()), refined=True)
    return res


def stable(p1, p2, samples, threshold=3.0):
    """[H] bool: True where hyp_count does not change when the normalised coordinates are multiplied by
    1 + 1e-13 N(0,1), for two fixed-seed replays.  A hypothesis with a match on the edge of the gate gains or loses it
    under such a change; comparing it with the device would compare rounding."""
    M = len(np.asarray(p1).reshape(-1, 2))
    base = ransac(p1, p2, samples, threshold)["hyp_count"]
    ok = np.ones(len(samples), bool)
    for rep in range(2):
        rng = np.random.default_rng(77 + rep)
        sc = (1 + 1e-13 * rng.standard_normal((M, 2)), 1 + 1e-13 * rng.standard_normal((M, 2)))
        ok &= ransac(p1, p2, samples, threshold, scale=sc)["hyp_count"] == base
    return ok


# ------------------------------------------------------------------------------------------------- scenes
K_REF = fr.K_REF
YAW = 0.25


def _yaw(yaw):
    return np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])


def general(rng, M, outlier_share=0.0):
    """fundamental_reference.synth_pair as it is: points in a box, a baseline.  Returns (pts1, pts2, None)."""
    p1, p2, _ = fr.synth_pair(rng, M, outlier_share)
    return p1, p2, None


def rotation(rng, M, outlier_share=0.0):
    """The scene of synth_pair with t = 0: both cameras share a centre.  Returns (pts1, pts2, K R K^-1)."""
    with np.errstate(invalid="ignore", divide="ignore"):                 # the true F of t = 0 is 0 / 0: not used
        p1, p2, _ = fr.synth_pair(rng, M, outlier_share, t=(0.0, 0.0, 0.0))
    Ht = K_REF @ _yaw(YAW) @ np.linalg.inv(K_REF)
    return p1, p2, Ht / Ht[2, 2]


def planar(rng, M, outlier_share=0.0, noise=0.5, t=(-1.5, 0.1, 0.3)):
    """synth_pair's cameras and noise, with every point on the plane n . X = d of camera 1's frame.  Returns
    (pts1, pts2, K (R + t n^T / d) K^-1), the plane-induced homography."""
    nrm, d = np.array([0.3, 0.2, 1.0]), 6.0
    xy = rng.uniform(-1, 1, (M, 2))
    X = np.c_[xy, (d - xy @ nrm[:2]) / nrm[2]]
    R, t = _yaw(YAW), np.asarray(t, dtype=np.float64)
    x1 = X @ K_REF.T
    x1 = x1[:, :2] / x1[:, 2:]
    x2 = (X @ R.T + t) @ K_REF.T
    x2 = x2[:, :2] / x2[:, 2:]
    x1 = x1 + rng.normal(size=x1.shape) * noise
    x2 = x2 + rng.normal(size=x2.shape) * noise
    k = int(M * outlier_share)
    x2[:k] = rng.uniform(0, 1, (k, 2)) * [1024, 768]
    Ht = K_REF @ (R + np.outer(t, nrm) / d) @ np.linalg.inv(K_REF)
    return x1.astype(np.float32), x2.astype(np.float32), Ht / Ht[2, 2]


SCENES = {"general": general, "rotation": rotation, "planar": planar}
# (scene, M, outlier share), ONE batch: M around the sample size and around FUND_CHUNK = 512, the LDS stage of the
# scoring loop; outlier shares 0 and 0.3
CASES = [("general", 3, 0.0), ("planar", 4, 0.0), ("rotation", 5, 0.0), ("planar", 5, 0.3), ("general", 40, 0.0),
         ("rotation", 40, 0.3), ("planar", 300, 0.0), ("general", 300, 0.3), ("rotation", 511, 0.3), ("planar", 512, 0.0),
         ("general", 512, 0.3), ("planar", 513, 0.3)]
SHIPPED = list(range(0, 148, 13))                                       # pairs 0, 13, ..., 143 of tests/golden/bunny_pairs.npz


def scene(kind, M, share):
    """(pts1, pts2, true H or None) of one case, from a generator seeded by the case."""
    return SCENES[kind](np.random.default_rng(1000 * M + int(100 * share) + 7 * sorted(SCENES).index(kind)), M, share)


def synth_batch():
    out = [scene(*c) for c in CASES]
    return [o[0] for o in out], [o[1] for o in out]


def shipped_pairs():
    """[(pts1, pts2, F)] of the 148 shipped pairs (all matched points, float32 pixels; F as shipped)."""
    import essential_reference
    return essential_reference.shipped_pairs()
