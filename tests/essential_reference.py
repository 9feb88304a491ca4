"""NumPy float64 reference of the batched essential-matrix RANSAC (sfm_amd/csrc/essential.hip), taking the samples as
input, plus its sample generator (tests/ransac_reference.py at 5 slots).

It is a reference for the tests, not a second implementation to fall back to.  The algorithm is the kernel's (Nister's
five-point solver, the steps are listed in sfm_amd/csrc/essential_solve.h); the means are not: null space by
np.linalg.svd where the kernel rotates columns, the elimination by np.linalg.solve, the real roots as the eigenvalues
with a zero imaginary part of the companion matrix (batched over the hypotheses) where the kernel brackets and bisects.
The two null-space bases differ, so the candidates of a sample come in another order; its best count does not.

    normalised  x = (u - cx) / fx,  y = (v - cy) / fy
    row of the system for x1 = (a, b), x2 = (c, d):  [c*a, c*b, c, d*a, d*b, d, a, b, 1]   (x2^T E x1 = 0, E row-major)
    inlier      fundamental_reference.cv_err2(K^-T E K^-1, p1, p2) <= threshold^2 in pixels
    no model    a sample with a non-finite coordinate, or with two matches that share a pixel in image 1 or in image 2
"""
import itertools

import numpy as np

import fundamental_reference as fr
import ransac_reference

MIN_SAMPLE = 5
# Nister's order: x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1, as exponents of (x, y, z)
MONO3 = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
         (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
MONO1 = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
MONO2 = sorted({tuple(np.add(a, b)) for a in MONO1 for b in MONO1}, reverse=True)


def _product_table(left, right, out):
    T = np.zeros((len(left), len(right), len(out)))
    for (i, a), (j, b) in itertools.product(enumerate(left), enumerate(right)):
        T[i, j, out.index(tuple(np.add(a, b)))] = 1.0
    return T


T11, T21 = _product_table(MONO1, MONO1, MONO2), _product_table(MONO2, MONO1, MONO3)


def draw_samples(seed, segment, n_points, n_hyp):
    """[n_hyp, 5] int32: the samples drawn for segment `segment` holding `n_points` matches (all -1 under 5)."""
    return ransac_reference.draw_samples(seed, segment, n_points, n_hyp, 5, 5)


def k4_of(K):
    K = np.asarray(K, dtype=np.float64)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def normalise(p, K):
    fx, fy, cx, cy = k4_of(K)
    p = np.asarray(p, dtype=np.float64).reshape(-1, 2)
    return np.stack([(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy], 1)


def to_pixels(E, K):
    """K^-T E K^-1 for E [...,3,3]."""
    Ki = np.linalg.inv(np.asarray(K, dtype=np.float64))
    return Ki.T @ E @ Ki


def scaled(E):
    """E [...,9] with |E|_F = sqrt(2) and its entry of largest magnitude (the first on a tie) positive."""
    with np.errstate(invalid="ignore", divide="ignore"):
        E = E * (np.sqrt(2.0) / np.sqrt((E * E).sum(-1)))[..., None]
    big = np.take_along_axis(E, np.argmax(np.abs(E), -1)[..., None], -1)
    return np.where(big < 0, -E, E)


def _polymul(a, b):
    """Batched product of polynomials by ascending power: a [H,n], b [H,m] -> [H,n+m-1]."""
    out = np.zeros((a.shape[0], a.shape[1] + b.shape[1] - 1))
    for i in range(a.shape[1]):
        out[:, i:i + b.shape[1]] += a[:, i:i + 1] * b
    return out


def _polyval(c, z):
    """c [H,n] by ascending power at z [H,R] -> [H,R]."""
    acc = np.zeros_like(z)
    for i in range(c.shape[1] - 1, -1, -1):
        acc = acc * z + c[:, i:i + 1]
    return acc


def _cubic(E):
    """(E E^T - tr(E E^T) / 2) E for E [...,3,3]: the nine cubic constraints, halved."""
    L = E @ np.swapaxes(E, -1, -2)
    L = L - 0.5 * np.trace(L, axis1=-2, axis2=-1)[..., None, None] * np.eye(3)
    return L @ E, L


def polish(basis, x, y, z, steps=4):
    """Step 7's Gauss-Newton on the nine cubic constraints in (x, y, z), inside the null space: basis [H,4,9], x, y, z
    [H,R].  By np.linalg.pinv of the 9 x 3 Jacobian, all candidates at once; a candidate keeps a step only if it is
    finite and lowers |f|^2.  Without it the roots carry the rounding of the elimination and of the companion matrix
    (errors of 1e-7 to 1e-12 in E, measured against tests/solver_truth.py), which the kernel's polish takes out."""
    B = basis.reshape(-1, 1, 4, 3, 3)
    q = np.stack([x, y, z], -1)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            E = (q[..., None, None] * B[:, :, :3]).sum(2) + B[:, :, 3]
            f, L = _cubic(E)
            J = []
            for v in range(3):
                D = np.broadcast_to(B[:, :, v], E.shape)
                S = D @ np.swapaxes(E, -1, -2)
                S = S + np.swapaxes(S, -1, -2)
                S = S - 0.5 * np.trace(S, axis1=-2, axis2=-1)[..., None, None] * np.eye(3)
                J.append((S @ E + L @ D).reshape(E.shape[:-2] + (9,)))
            J = np.stack(J, -1)                                          # [H,R,9,3]
            ok = np.isfinite(J).all(axis=(-1, -2)) & np.isfinite(f).all(axis=(-1, -2))
            step = np.zeros_like(q)
            if ok.any():
                step[ok] = (np.linalg.pinv(J[ok]) @ f[ok].reshape(-1, 9, 1))[..., 0]
            qn = q - step
            fn, _ = _cubic((qn[..., None, None] * B[:, :, :3]).sum(2) + B[:, :, 3])
            better = ok & ((fn * fn).sum(axis=(-1, -2)) < (f * f).sum(axis=(-1, -2)))
            q = np.where(better[..., None], qn, q)
    return q[..., 0], q[..., 1], q[..., 2]


def from_basis(basis):
    """Steps 4 to 7: basis [H,4,9] (X, Y, Z, W) -> E [H,10,3,3] (slot = ascending real root; scaled()) and valid [H,10]."""
    H = basis.shape[0]
    E_out, valid = np.zeros((H, 10, 3, 3)), np.zeros((H, 10), bool)
    if H == 0:
        return E_out, valid
    L = basis.transpose(0, 2, 1)                                        # [H,9,4]: entry e of E as a linear polynomial
    m11 = lambda p, q: np.einsum("ha,hb,abk->hk", p, q, T11)
    m21 = lambda q, p: np.einsum("hk,hc,kcm->hm", q, p, T21)
    ent = lambda i, j: L[:, 3 * i + j]
    det = (m21(m11(ent(1, 1), ent(2, 2)) - m11(ent(1, 2), ent(2, 1)), ent(0, 0))
           - m21(m11(ent(1, 0), ent(2, 2)) - m11(ent(1, 2), ent(2, 0)), ent(0, 1))
           + m21(m11(ent(1, 0), ent(2, 1)) - m11(ent(1, 1), ent(2, 0)), ent(0, 2)))
    EEt = [[sum(m11(ent(i, k), ent(j, k)) for k in range(3)) for j in range(3)] for i in range(3)]
    tr = EEt[0][0] + EEt[1][1] + EEt[2][2]
    rows = [det]
    for i in range(3):
        for j in range(3):
            rows.append(sum(m21(2.0 * EEt[i][k] - (tr if i == k else 0.0), ent(k, j)) for k in range(3)))
    M = np.stack(rows, 1)                                               # [H,10,20]
    ok = np.isfinite(M).all(axis=(1, 2))
    R = np.zeros((H, 10, 10))
    try:
        R[ok] = np.linalg.solve(M[ok][:, :, :10], M[ok][:, :, 10:])
    except np.linalg.LinAlgError:                                       # a singular left block somewhere: one by one
        for h in np.flatnonzero(ok):
            try:
                R[h] = np.linalg.solve(M[h, :, :10], M[h, :, 10:])
            except np.linalg.LinAlgError:
                ok[h] = False
    ok &= np.isfinite(R).all(axis=(1, 2))
    R[~ok] = 0.0
    # rows e..j (leading x^2z, x^2, y^2z, y^2, xyz, xy): k = e - z f, l = g - z h, m = i - z j as polynomials in z
    bx, by, bc = [], [], []
    for t in range(3):
        e, f = R[:, 4 + 2 * t], R[:, 5 + 2 * t]
        bx.append(np.stack([e[:, 2], e[:, 1] - f[:, 2], e[:, 0] - f[:, 1], -f[:, 0]], 1))
        by.append(np.stack([e[:, 5], e[:, 4] - f[:, 5], e[:, 3] - f[:, 4], -f[:, 3]], 1))
        bc.append(np.stack([e[:, 9], e[:, 8] - f[:, 9], e[:, 7] - f[:, 8], e[:, 6] - f[:, 7], -f[:, 6]], 1))
    c = np.zeros((H, 11))
    for t in range(3):
        u, v = (t + 1) % 3, (t + 2) % 3
        c += _polymul(_polymul(bx[u], by[v]) - _polymul(bx[v], by[u]), bc[t])
    ok &= np.isfinite(c).all(1) & (c[:, 10] != 0)
    c[~ok] = 0.0
    c[~ok, 10] = 1.0
    comp = np.zeros((H, 10, 10))
    comp[:, 0, :] = -(c[:, :10] / c[:, 10:])[:, ::-1]
    comp[:, np.arange(1, 10), np.arange(9)] = 1.0
    ok &= np.isfinite(comp).all(axis=(1, 2))
    comp[~ok] = 0.0
    ev = np.linalg.eigvals(comp)
    z = np.sort(np.where((ev.imag == 0) & ok[:, None], ev.real, np.inf), 1)
    valid = np.isfinite(z)
    z = np.where(valid, z, 0.0)
    rows3 = np.stack([np.stack([_polyval(bx[t], z), _polyval(by[t], z), _polyval(bc[t], z)], -1) for t in range(3)], 2)
    cr = np.stack([np.cross(rows3[:, :, a], rows3[:, :, b]) for a, b in ((0, 1), (0, 2), (1, 2))], 2)     # [H,10,3,3]
    pick = np.argmax(np.abs(cr[..., 2]), -1)                             # the first of equal ones
    xyw = np.take_along_axis(cr, pick[..., None, None], 2)[:, :, 0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x, y = xyw[..., 0] / xyw[..., 2], xyw[..., 1] / xyw[..., 2]
        x, y, z = polish(basis, x, y, z)
        E = (x[..., None] * basis[:, None, 0] + y[..., None] * basis[:, None, 1] + z[..., None] * basis[:, None, 2]
             + basis[:, None, 3])
        E = scaled(E)
    valid &= (xyw[..., 2] != 0) & np.isfinite(E).all(-1)
    E_out[valid] = E[valid].reshape(-1, 3, 3)
    return E_out, valid


def five_point(x1, x2):
    """x1, x2 [H,5,2] normalised.  Returns E [H,10,3,3] and valid [H,10]; the filled slots are those of the ascending
    real roots, so they need not be the first ones."""
    H = x1.shape[0]
    A = fr.system_rows(x1, x2)
    fin = np.isfinite(A).all(axis=(1, 2))
    basis = np.zeros((H, 4, 9))
    if fin.any():
        basis[fin] = np.linalg.svd(A[fin])[2][:, 5:9]
    E, valid = from_basis(basis)
    valid &= fin[:, None]
    E[~valid] = 0.0
    return E, valid


def voided(p1, p2, samples):
    """[H] bool: the samples that give no model by rule (a non-finite coordinate, a repeated pixel in either image)."""
    idx = np.asarray(samples, dtype=np.int64)
    a, b = np.asarray(p1, dtype=np.float32)[idx], np.asarray(p2, dtype=np.float32)[idx]          # [H,5,2]
    bad = ~(np.isfinite(a).all(axis=(1, 2)) & np.isfinite(b).all(axis=(1, 2)))
    for k, l in itertools.combinations(range(5), 2):
        bad |= (a[:, k] == a[:, l]).all(1) | (b[:, k] == b[:, l]).all(1)
    return bad


def counts(E, ok, K, p1, p2, threshold):
    """Inlier counts [..] of E [..,3,3] (ok [..]) over the pair: fundamental_reference.cv_err2's rule on K^-T E K^-1,
    written as matrix products over the valid candidates, in blocks."""
    out = np.zeros(ok.shape, np.int64)
    F = to_pixels(E[ok], K)                                             # [N,3,3]
    x1, x2 = np.c_[p1, np.ones(len(p1))].T, np.c_[p2, np.ones(len(p2))].T        # [3,M]
    got = np.zeros(len(F), np.int64)
    with np.errstate(all="ignore"):
        for at in range(0, len(F), 256):
            l2, l1 = F[at:at + 256] @ x1, F[at:at + 256].transpose(0, 2, 1) @ x2  # F x1, F^T x2: [n,3,M]
            s2 = (l2 * x2).sum(1) ** 2
            e = np.maximum(s2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2), s2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2))
            got[at:at + 256] = (e <= threshold * threshold).sum(1)
    out[ok] = got
    return out


def inliers(E, K, p1, p2, threshold):
    p1 = np.asarray(p1, dtype=np.float64).reshape(-1, 2)
    p2 = np.asarray(p2, dtype=np.float64).reshape(-1, 2)
    return fr.inliers(to_pixels(np.asarray(E, dtype=np.float64).reshape(3, 3), K), p1, p2, threshold)


def refit(p1, p2, K, mask, threshold):
    """The solver over all inliers: the four eigenvectors of A^T A with the smallest eigenvalues stand in for the null
    space.  Returns (E, count) of the best candidate (the first of equal ones) or (None, 0)."""
    A = fr.system_rows(normalise(p1[mask], K), normalise(p2[mask], K))
    w, V = np.linalg.eigh(A.T @ A)
    E, ok = from_basis(V[:, :4].T[None])
    cnt = counts(E[0], ok[0], K, p1, p2, threshold)
    if cnt.max() == 0:
        return None, 0
    k = int(np.argmax(cnt))
    return E[0, k], int(cnt[k])


def ransac(p1, p2, K, samples, threshold=3.0, refine=False, scale=None):
    """Follows the device for one pair on given samples [H,5].  Returns a dict: `hyp_count` [H] (best candidate count per
    hypothesis), `status` (0 ok, 1 fewer than 5 matches, 2 no model), `E` (normalised coordinates, scaled(), or None),
    `mask` [M] bool, `n_inliers`, `refined`, `winner` (hypothesis index), `cand_count` [H,10] and `voided` [H].
    scale: optional ([M,2], [M,2]) factors on the normalised coordinates the solver sees (`stable`)."""
    p1 = np.asarray(p1, dtype=np.float64).reshape(-1, 2)
    p2 = np.asarray(p2, dtype=np.float64).reshape(-1, 2)
    M, H = len(p1), len(samples)
    res = {"hyp_count": np.zeros(H, np.int32), "status": 1, "E": None, "mask": np.zeros(M, bool), "n_inliers": 0,
           "refined": False, "winner": -1, "cand_count": np.zeros((H, 10), np.int32), "voided": np.ones(H, bool)}
    if M < MIN_SAMPLE:
        return res
    idx = np.asarray(samples, dtype=np.int64)
    void = voided(p1, p2, idx)
    with np.errstate(invalid="ignore", over="ignore"):
        n1, n2 = normalise(p1, K), normalise(p2, K)
        if scale is not None:
            n1, n2 = n1 * scale[0], n2 * scale[1]
    live = np.flatnonzero(~void)
    E, ok = np.zeros((H, 10, 3, 3)), np.zeros((H, 10), bool)
    E[live], ok[live] = five_point(n1[idx[live]], n2[idx[live]])
    cnt = counts(E, ok, K, p1, p2, threshold)
    res["cand_count"] = cnt.astype(np.int32)
    res["hyp_count"] = cnt.max(1).astype(np.int32)
    res["voided"] = void
    res["status"] = 2
    if cnt.max() == 0:
        return res
    h, k = np.unravel_index(np.argmax(cnt), cnt.shape)                  # first maximum: lowest hypothesis, then lowest slot
    Ew = E[h, k]
    mask = inliers(Ew, K, p1, p2, threshold)
    res.update(status=0, E=Ew, mask=mask, n_inliers=int(mask.sum()), winner=int(h))
    if refine and mask.sum() >= MIN_SAMPLE:
        Er, _ = refit(p1, p2, K, mask, threshold)
        if Er is not None:
            mr = inliers(Er, K, p1, p2, threshold)
            if mr.sum() >= mask.sum():
                res.update(E=Er, mask=mr, n_inliers=int(mr.sum()), refined=True)
    return res


def stable(p1, p2, K, samples, threshold=3.0):
    """[H] bool: True where hyp_count does not change when the normalised coordinates are multiplied by
    1 + 1e-13 N(0,1), for two fixed-seed replays.  A hypothesis whose polynomial is near a double root gains or loses a
    pair of candidates under such a change; comparing it with the device would compare rounding."""
    M = len(np.asarray(p1).reshape(-1, 2))
    base = ransac(p1, p2, K, samples, threshold)["hyp_count"]
    ok = np.ones(len(samples), bool)
    for rep in range(2):
        rng = np.random.default_rng(77 + rep)
        sc = (1 + 1e-13 * rng.standard_normal((M, 2)), 1 + 1e-13 * rng.standard_normal((M, 2)))
        ok &= ransac(p1, p2, K, samples, threshold, scale=sc)["hyp_count"] == base
    return ok


# ------------------------------------------------------------------------------------------- shared inputs
CASES = [(4, 0.0), (5, 0.0), (6, 0.0), (40, 0.3), (300, 0.3), (300, 0.6), (2000, 0.5)]       # (M, outlier share), ONE batch
SHIPPED = list(range(0, 148, 13))                                       # pairs 0, 13, ..., 143 of tests/golden/bunny_pairs.npz


def synth_batch():
    out = [fr.synth_pair(np.random.default_rng(1000 * M + int(100 * share)), M, share) for M, share in CASES]
    return [o[0] for o in out], [o[1] for o in out]


def shipped_pairs():
    """[(pts1, pts2, F)] of the 148 shipped pairs (all matched points, float32 pixels; F as shipped)."""
    import os
    bp = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bunny_pairs.npz"), allow_pickle=False)
    off = bp["offsets"]
    return [(bp["pts1"][off[i]:off[i + 1]], bp["pts2"][off[i]:off[i + 1]], bp["F"][i]) for i in range(len(off) - 1)]


def reprojection_errors(K, R, t, X, p1, p2):
    """[M]: the larger of the two pixel errors of X under K [I|0] and K [R|t]."""
    K = np.asarray(K, dtype=np.float64)
    a, b = X @ K.T, (X @ np.asarray(R).T + np.reshape(t, 3)) @ K.T
    with np.errstate(all="ignore"):
        e1 = np.hypot(*(a[:, :2] / a[:, 2:] - p1).T)
        e2 = np.hypot(*(b[:, :2] / b[:, 2:] - p2).T)
    return np.maximum(e1, e2)


def pose_quality(E, mask, p1, p2, K, max_error=4.0):
    """What a pose taken from E is worth: E -> pose_reference.recover_pose over `mask` -> two-view triangulation of its
    good points in pixels.  Returns (number of good points, share of them within max_error in both views, median error)."""
    import pose_reference
    p1 = np.asarray(p1, dtype=np.float64).reshape(-1, 2)
    p2 = np.asarray(p2, dtype=np.float64).reshape(-1, 2)
    rp = pose_reference.recover_pose(E, p1, p2, K, mask=np.asarray(mask).reshape(-1))
    good = rp["mask"] != 0
    if rp["R"] is None or not good.any():
        return 0, 0.0, float("nan")
    X = pose_reference.triangulate_pixels(K, rp["R"], rp["t"], p1[good], p2[good])
    err = reprojection_errors(K, rp["R"], rp["t"], X, p1[good], p2[good])
    with np.errstate(invalid="ignore"):
        return int(good.sum()), float((err <= max_error).mean()), float(np.median(err))
