"""NumPy restatement of sfm_amd/csrc/triangulate_solve.h (N-view triangulation of tracks), generic over the dtype so that
it runs in float64 - operation for operation what the header does, no fused multiply-adds - and in np.longdouble, whose
80-bit result stands in for the exact value when a tolerance is worked out.

All tracks advance in lockstep: the loops run over the position of an observation inside its track and every operation is
element-wise over the tracks, so each track still sums over its own used observations in their order.
"""
import numpy as np

OK, TOO_FEW_VIEWS, DEGENERATE, BEHIND, LOW_ANGLE, HIGH_ERROR = range(6)


def camera_centres(proj, dtype=np.float64):
    """C = -M^-1 p4 by cofactors, as tri::camera_centre."""
    P = np.asarray(proj).reshape(-1, 12).astype(dtype)
    m00, m01, m02, p0, m10, m11, m12, p1, m20, m21, m22, p2 = (P[:, k] for k in range(12))
    c00, c01, c02 = m11 * m22 - m12 * m21, m12 * m20 - m10 * m22, m10 * m21 - m11 * m20
    det = (m00 * c00 + m01 * c01) + m02 * c02
    a01, a02 = m02 * m21 - m01 * m22, m01 * m12 - m02 * m11
    a11, a12 = m00 * m22 - m02 * m20, m02 * m10 - m00 * m12
    a21, a22 = m01 * m20 - m00 * m21, m00 * m11 - m01 * m10
    with np.errstate(all="ignore"):
        return np.stack([-((c00 * p0 + a01 * p1) + a02 * p2) / det, -((c01 * p0 + a11 * p1) + a12 * p2) / det,
                         -((c02 * p0 + a21 * p1) + a22 * p2) / det], axis=1)


def null4(U):
    """jacobi::null4 of pose_solve.h on a stack [T,4,4]: the right singular vector of the smallest singular value by
    Hestenes sweeps on the columns, eps = 10 * machine epsilon of the dtype, at most 30 sweeps."""
    U = U.copy()
    dtype = U.dtype
    T = U.shape[0]
    V = np.zeros((T, 4, 4), dtype)
    for k in range(4):
        V[:, k, k] = 1
    eps = dtype.type(10) * np.finfo(dtype).eps
    one, two = dtype.type(1), dtype.type(2)
    with np.errstate(all="ignore"):
        for _ in range(30):
            changed = False
            for p in range(3):
                for q in range(p + 1, 4):
                    a = np.zeros(T, dtype); b = np.zeros(T, dtype); g = np.zeros(T, dtype)
                    for r in range(4):
                        a = a + U[:, r, p] * U[:, r, p]; b = b + U[:, r, q] * U[:, r, q]; g = g + U[:, r, p] * U[:, r, q]
                    rot = np.abs(g) > eps * np.sqrt(a * b)
                    if not rot.any():
                        continue
                    changed = True
                    zeta = (b - a) / (two * g)
                    tt = np.copysign(one, zeta) / (np.abs(zeta) + np.sqrt(one + zeta * zeta))
                    c = one / np.sqrt(one + tt * tt)
                    s = c * tt
                    for M in (U, V):
                        mp, mq = M[:, :, p].copy(), M[:, :, q].copy()
                        M[:, :, p] = np.where(rot[:, None], c[:, None] * mp - s[:, None] * mq, mp)
                        M[:, :, q] = np.where(rot[:, None], s[:, None] * mp + c[:, None] * mq, mq)
            if not changed:
                break
    nk = np.zeros((T, 4), dtype)
    for r in range(4):
        nk = nk + U[:, r, :] * U[:, r, :]
    best = np.argmin(nk, axis=1)                      # the first of equal ones
    return V[np.arange(T), :, best]


def gather(proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp, dtype=np.float64):
    """The used observations of every track, padded to the longest: P [T,L,12], C [T,L,3], xy [T,L,2] in `dtype`, mask
    [T,L], n_views [T].  An image or camera index out of range is not registered; a keypoint outside its image is NaN."""
    proj = np.asarray(proj, dtype=np.float64).reshape(-1, 12)
    cam_of_image = np.asarray(cam_of_image, dtype=np.int64).reshape(-1)
    kp_ptr = np.asarray(kp_ptr, dtype=np.int64)
    kp_xy = np.asarray(kp_xy, dtype=np.float64).reshape(-1, 2)
    track_ptr = np.asarray(track_ptr, dtype=np.int64)
    obs_image = np.asarray(obs_image, dtype=np.int64); obs_kp = np.asarray(obs_kp, dtype=np.int64)
    T, n_obs, n_img, n_cams, n_nodes = len(track_ptr) - 1, len(obs_image), len(cam_of_image), len(proj), len(kp_xy)
    img_ok = (obs_image >= 0) & (obs_image < n_img)
    img = np.where(img_ok, obs_image, 0)
    cam = cam_of_image[img] if n_img else np.full(n_obs, -1)
    used = img_ok & (cam >= 0) & (cam < n_cams)
    cam = np.where(used, cam, 0)
    trk = np.repeat(np.arange(T), np.diff(track_ptr))
    n_views = np.bincount(trk[used], minlength=T).astype(np.int32) if n_obs else np.zeros(T, np.int32)
    L = max(int(n_views.max()) if T else 0, 1)
    sel = np.flatnonzero(used)
    first = np.concatenate([[0], np.cumsum(n_views)])[:-1]
    pos = np.arange(len(sel)) - first[trk[sel]]                       # rank of a used observation inside its track
    mask = np.zeros((T, L), bool)
    P = np.zeros((T, L, 12), dtype); C = np.zeros((T, L, 3), dtype); xy = np.zeros((T, L, 2), dtype)
    if len(sel):
        lo, hi = kp_ptr[img[sel]], kp_ptr[img[sel] + 1]
        node = lo + obs_kp[sel]
        ok = (obs_kp[sel] >= 0) & (node < hi) & (node < n_nodes)
        px = np.where(ok[:, None], kp_xy[np.where(ok, node, 0)] if n_nodes else np.nan, np.nan)
        centres = camera_centres(proj, dtype)
        mask[trk[sel], pos] = True
        P[trk[sel], pos] = proj[cam[sel]].astype(dtype)
        C[trk[sel], pos] = centres[cam[sel]]
        xy[trk[sel], pos] = px.astype(dtype)
    return P, C, xy, mask, n_views


def _project(P, X):
    hx = P[:, 0] * X[:, 0] + P[:, 1] * X[:, 1] + P[:, 2] * X[:, 2] + P[:, 3]
    hy = P[:, 4] * X[:, 0] + P[:, 5] * X[:, 1] + P[:, 6] * X[:, 2] + P[:, 7]
    hw = P[:, 8] * X[:, 0] + P[:, 9] * X[:, 1] + P[:, 10] * X[:, 2] + P[:, 11]
    return hx, hy, hw


def dlt_rows(P, xy):
    """[..., 2, 4]: x P[2] - P[0] and y P[2] - P[1]."""
    return np.stack([xy[..., 0:1] * P[..., 8:12] - P[..., 0:4], xy[..., 1:2] * P[..., 8:12] - P[..., 4:8]], axis=-2)


def linear_stage(P, xy, mask, n_views):
    """Homogeneous v [T,4]: streaming Givens QR of the rows and null4 of the factor; dlt2 for two-view tracks."""
    T, L = mask.shape
    dtype = P.dtype
    rows = dlt_rows(P, xy)                                            # [T,L,2,4]
    R = np.zeros((T, 4, 4), dtype)
    with np.errstate(all="ignore"):
        for l in range(L):
            for half in range(2):
                r = rows[:, l, half].copy()
                for j in range(4):
                    b = r[:, j]
                    act = mask[:, l] & (b != 0)
                    a = R[:, j, j]
                    h = np.sqrt(a * a + b * b)
                    hs = np.where(act, h, 1)
                    c, s = a / hs, b / hs
                    R[:, j, j] = np.where(act, h, a)
                    for k in range(j + 1, 4):
                        rk, xk = R[:, j, k].copy(), r[:, k].copy()
                        R[:, j, k] = np.where(act, c * rk + s * xk, rk)
                        r[:, k] = np.where(act, c * xk - s * rk, xk)
        U = R
        two = n_views == 2
        if two.any() and L >= 2:
            U = np.where(two[:, None, None], rows[:, :2].reshape(T, 4, 4), R)
        return null4(U)


def evaluate(P, xy, mask, X, max_error):
    """(cost, max_err, behind, high, err [T,L]) at X, sums in observation order."""
    T, L = mask.shape
    dtype = P.dtype
    cost = np.zeros(T, dtype); max_err = np.zeros(T, dtype)
    behind = np.zeros(T, bool); high = np.zeros(T, bool)
    err = np.full((T, L), np.nan, dtype)
    with np.errstate(all="ignore"):
        for l in range(L):
            m = mask[:, l]
            hx, hy, hw = _project(P[:, l], X)
            du, dv = hx / hw - xy[:, l, 0], hy / hw - xy[:, l, 1]
            e2 = du * du + dv * dv
            e = np.sqrt(e2)
            cost = np.where(m, cost + e2, cost)
            max_err = np.where(m & ((e > max_err) | (e != e)), e, max_err)
            behind |= m & (hw <= 0)
            high |= m & (e > dtype.type(max_error))
            err[:, l] = np.where(m, e, np.nan)
    return cost, max_err, behind, high, err


def refine(P, xy, mask, X0, iters):
    """`iters` Gauss-Newton steps from X0; returns (X, cost at X0).  A track whose pivot is not positive or whose new
    point is not finite keeps its last good point and takes no further step."""
    T, L = mask.shape
    dtype = P.dtype
    X = X0.copy()
    alive = np.ones(T, bool)
    cost0 = np.zeros(T, dtype)
    with np.errstate(all="ignore"):
        for it in range(iters):
            A = {k: np.zeros(T, dtype) for k in ("00", "10", "11", "20", "21", "22")}
            g = [np.zeros(T, dtype) for _ in range(3)]
            cost = np.zeros(T, dtype)
            for l in range(L):
                m = mask[:, l]
                Pl = P[:, l]
                hx, hy, hw = _project(Pl, X)
                pu, pv = hx / hw, hy / hw
                du, dv = pu - xy[:, l, 0], pv - xy[:, l, 1]
                cost = np.where(m, cost + (du * du + dv * dv), cost)
                ju = [(Pl[:, k] - pu * Pl[:, 8 + k]) / hw for k in range(3)]
                jv = [(Pl[:, 4 + k] - pv * Pl[:, 8 + k]) / hw for k in range(3)]
                for key in A:
                    i, j = int(key[0]), int(key[1])
                    A[key] = np.where(m, A[key] + (ju[i] * ju[j] + jv[i] * jv[j]), A[key])
                for k in range(3):
                    g[k] = np.where(m, g[k] + (ju[k] * du + jv[k] * dv), g[k])
            if it == 0:
                cost0 = cost
            ok = alive & (A["00"] > 0)
            l00 = np.sqrt(A["00"])
            l10, l20 = A["10"] / l00, A["20"] / l00
            d1 = A["11"] - l10 * l10
            ok &= d1 > 0
            l11 = np.sqrt(d1)
            l21 = (A["21"] - l20 * l10) / l11
            d2 = A["22"] - l20 * l20 - l21 * l21
            ok &= d2 > 0
            l22 = np.sqrt(d2)
            y0 = g[0] / l00
            y1 = (g[1] - l10 * y0) / l11
            y2 = (g[2] - l20 * y0 - l21 * y1) / l22
            z2 = y2 / l22
            z1 = (y1 - l21 * z2) / l11
            z0 = (y0 - l10 * z1 - l20 * z2) / l00
            Xn = np.stack([X[:, 0] - z0, X[:, 1] - z1, X[:, 2] - z2], axis=1)
            ok &= np.isfinite(Xn).all(axis=1)
            alive = ok
            X = np.where(ok[:, None], Xn, X)
    return X, cost0


def wide_pair(C, mask, X, cos_min):
    """[T] bool: some pair of used views has d_i.d_j / (|d_i||d_j|) <= cos_min, d = X - C."""
    T, L = mask.shape
    with np.errstate(all="ignore"):
        d = X[:, None, :] - C
        n = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
        wide = np.zeros(T, bool)
        for i in range(L - 1):
            dot = d[:, i, None, 0] * d[:, i + 1:, 0] + d[:, i, None, 1] * d[:, i + 1:, 1] + d[:, i, None, 2] * d[:, i + 1:, 2]
            c = dot / (n[:, i, None] * n[:, i + 1:])
            wide |= (mask[:, i, None] & mask[:, i + 1:] & (c <= cos_min)).any(axis=1)
    return wide


def triangulate(proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp, min_views=2, refine_iters=5, max_error=4.0,
                min_angle_deg=0.0, dtype=np.float64):
    """{X [T,3], status, n_views int32, max_err [T], counts [6] int64} in `dtype`, plus "linear" (the linear stage's X)."""
    dtype = np.dtype(dtype)
    P, C, xy, mask, n_views = gather(proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp, dtype)
    T = len(n_views)
    status = np.zeros(T, np.int32)
    nan = dtype.type(np.nan)

    def fail(cond, code):
        status[(status == OK) & cond] = code

    fail(n_views < min_views, TOO_FEW_VIEWS)
    finite = (np.isfinite(P).all(axis=2) & np.isfinite(C).all(axis=2) & np.isfinite(xy).all(axis=2)) | ~mask
    fail(~finite.all(axis=1), DEGENERATE)
    v = linear_stage(P, xy, mask, n_views)
    with np.errstate(all="ignore"):
        Xl = v[:, :3] / v[:, 3:4]
    fail(v[:, 3] == 0, DEGENERATE)
    fail(~np.isfinite(Xl).all(axis=1), DEGENERATE)
    X = Xl
    if refine_iters > 0:
        Xr, cost_lin = refine(P, xy, mask, Xl, refine_iters)
        cost = evaluate(P, xy, mask, Xr, max_error)[0]
        with np.errstate(all="ignore"):
            X = np.where((cost > cost_lin)[:, None], Xl, Xr)
    _, max_err, behind, high, _ = evaluate(P, xy, mask, X, max_error)
    fail(behind, BEHIND)
    if min_angle_deg > 0:
        cos_min = dtype.type(np.cos(np.float64(min_angle_deg) * (np.pi / 180.0)))
        fail(~wide_pair(C, mask, X, cos_min), LOW_ANGLE)
    fail(high, HIGH_ERROR)
    dead = (status == TOO_FEW_VIEWS) | (status == DEGENERATE)
    X = np.where(dead[:, None], nan, X)
    max_err = np.where(dead, nan, max_err)
    return {"X": X, "status": status, "n_views": n_views, "max_err": max_err,
            "counts": np.bincount(status, minlength=6).astype(np.int64), "linear": np.where(dead[:, None], nan, Xl)}


def gate_quantities(proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp, X, dtype=np.float64):
    """Every quantity a gate compares, without early exit: err [T,L] and depth [T,L] per used view (NaN elsewhere) and
    cos [T,L,L] of every pair of used views i < j (NaN elsewhere)."""
    dtype = np.dtype(dtype)
    P, C, xy, mask, _ = gather(proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp, dtype)
    X = np.asarray(X).astype(dtype)
    T, L = mask.shape
    err = evaluate(P, xy, mask, X, np.inf)[4]
    with np.errstate(all="ignore"):
        depth = np.stack([np.where(mask[:, l], _project(P[:, l], X)[2], np.nan) for l in range(L)], axis=1)
        d = X[:, None, :] - C
        n = np.sqrt((d * d).sum(axis=2))
        cos = (d[:, :, None, :] * d[:, None, :, :]).sum(axis=3) / (n[:, :, None] * n[:, None, :])
    pair = mask[:, :, None] & mask[:, None, :] & np.triu(np.ones((L, L), bool), 1)[None]
    return err, depth, np.where(pair, cos, np.nan)


# ------------------------------------------------------------------------------------------------ scenes for the tests
K_SFM = np.array([[1228.0, 0, 512], [0, 1228.0, 384], [0, 0, 1]])        # StructureFromMotion.K


def arc_cameras(n=12, radius=6.0, span=2.0, height=1.5, target=(0.5, 0.5, 0.5)):
    """n cameras on an arc of `span` radians around the unit cube, looking at its centre: (proj [n,3,4], R, t, centres)."""
    target = np.asarray(target, dtype=np.float64)
    Rs, ts, cs = [], [], []
    for a in np.linspace(-span / 2, span / 2, n):
        c = target + [radius * np.sin(a), height, -radius * np.cos(a)]
        z = (target - c) / np.linalg.norm(target - c)
        x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        Rs.append(R); ts.append(-R @ c); cs.append(c)
    Rs, ts = np.stack(Rs), np.stack(ts)
    proj = np.stack([K_SFM @ np.hstack([R, t[:, None]]) for R, t in zip(Rs, ts)])
    return proj, Rs, ts, np.stack(cs)


def project_points(proj, X):
    """Pixels [n_cams, n_pts, 2] of points X [n_pts,3]."""
    h = np.einsum("cij,pj->cpi", np.asarray(proj).reshape(-1, 3, 4), np.hstack([X, np.ones((len(X), 1))]))
    return h[..., :2] / h[..., 2:3]


def make_tracks(rng, proj, X, lengths, noise=0.5, repeat=False, cams=None, uniform=False):
    """Flat arrays for points X seen by lengths[p] cameras each (distinct and ascending unless repeat; or the cameras
    cams[p]): every camera is an image of its own, every observation a keypoint of its own, images numbered as the
    cameras.  noise: pixels, one figure or one per point; Gaussian, or uniform in [-noise, noise] per coordinate.
    Returns (kp_ptr, kp_xy, track_ptr, obs_image, obs_kp)."""
    n_cams = len(proj)
    px = project_points(proj, X)
    if cams is None:
        cams = [np.sort(rng.choice(n_cams, int(n), replace=False)) if not repeat else rng.integers(0, n_cams, int(n))
                for n in lengths]
    obs_image = np.concatenate(cams).astype(np.int32) if len(cams) else np.zeros(0, np.int32)
    pt = np.repeat(np.arange(len(X)), [len(c) for c in cams])
    draw = rng.uniform(-1, 1, (len(pt), 2)) if uniform else rng.normal(size=(len(pt), 2))
    uv = px[obs_image, pt] + draw * np.broadcast_to(np.asarray(noise, dtype=np.float64), (len(X),))[pt, None]
    order = np.argsort(obs_image, kind="stable")                            # keypoints grouped by image
    obs_kp = np.empty(len(pt), np.int32)
    counts = np.bincount(obs_image, minlength=n_cams)
    kp_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    obs_kp[order] = (np.arange(len(pt)) - kp_ptr[obs_image[order]]).astype(np.int32)
    kp_xy = np.empty((len(pt), 2))
    kp_xy[kp_ptr[obs_image] + obs_kp] = uv
    track_ptr = np.concatenate([[0], np.cumsum([len(c) for c in cams])]).astype(np.int64)
    return kp_ptr, kp_xy, track_ptr, obs_image, obs_kp
