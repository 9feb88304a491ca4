"""NumPy restatement of the exposure compensation (sfm_amd/csrc/mesh_exposure.hip; include/sfm_amd.h states the rule): what
every view sees of every vertex as one byte per channel, the two integer tables, the solve of the gains and the gain applied
to an image, operation for operation - float64 with every product and sum rounded on its own - so that the device's output
bytes can be compared with these.  The sample twice: on arrays (`sample`) and in plain loops (`sample_loops`); the tables as
matrix products (`tables`) and by counting (`tables_loops`).  Nothing here imports the package: `solve_gains` restates
sfm_amd.exposure.solve_gains pair by pair.  Also the gained sphere scene the tests share and what the rule is worth on it."""
import numpy as np

import mesh_color_reference as cr
import mesh_reference as mr


# ------------------------------------------------------------------------------------------- the sample on arrays
def sample(vertices, normals, proj, centres, depth, keep, images, tol, min_cos=0.35, channels=None):
    """(seen uint8 [n,nv], samples uint8 [n,ch,nv]): steps 1 to 4 of the colouring per view, the sample quantised."""
    X = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    n = np.asarray(normals, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    proj = np.asarray(proj, dtype=np.float64).reshape(-1, 12)
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    ch = cr.channels_of(images, channels)
    nv = len(X)
    tol, min_cos = np.float64(tol), np.float64(min_cos)
    seen = np.zeros((len(depth), nv), np.uint8)
    samples = np.zeros((len(depth), ch, nv), np.uint8)
    zero_normal = (n == 0).all(axis=1)
    for v, d in enumerate(depth):
        d = np.asarray(d, dtype=np.float32)
        h, w = d.shape
        if h == 0 or w == 0 or nv == 0:
            continue
        P = proj[v]
        valid, xi, yi, q2 = mr.project(P, X, w, h)
        with np.errstate(all="ignore"):
            q0 = ((P[0] * X[:, 0] + P[1] * X[:, 1]) + P[2] * X[:, 2]) + P[3]
            q1 = ((P[4] * X[:, 0] + P[5] * X[:, 1]) + P[6] * X[:, 2]) + P[7]
            u, vv = q0 / q2, q1 / q2
            ds = d[yi, xi].astype(np.float64)
            ok = valid & np.isfinite(ds)
            if keep is not None:
                ok &= np.asarray(keep[v])[yi, xi] != 0
            dd = ds - q2
            ok &= (dd >= -tol) & (dd <= tol)
            g = centres[v][None, :] - X
            l2 = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
            ok &= np.isfinite(l2) & (l2 > 0)
            c = np.where(zero_normal, 1.0, ((n[:, 0] * g[:, 0] + n[:, 1] * g[:, 1]) + n[:, 2] * g[:, 2]) / np.sqrt(l2))
            ok &= c >= min_cos
            u, vv = np.where(ok, u, 0.0), np.where(ok, vv, 0.0)
            x0, y0 = np.floor(u), np.floor(vv)
            fx, fy = u - x0, vv - y0
            xa, xb = np.clip(x0.astype(np.int64), 0, w - 1), np.clip(x0.astype(np.int64) + 1, 0, w - 1)
            ya, yb = np.clip(y0.astype(np.int64), 0, h - 1), np.clip(y0.astype(np.int64) + 1, 0, h - 1)
            img = np.asarray(images[v], dtype=np.uint8).reshape(h, w, ch)
            for k in range(ch):
                a, b = img[ya, xa, k].astype(np.float64), img[ya, xb, k].astype(np.float64)
                e, f = img[yb, xa, k].astype(np.float64), img[yb, xb, k].astype(np.float64)
                top = a + fx * (b - a)
                bot = e + fx * (f - e)
                s = top + fy * (bot - top)
                r = np.floor(s + 0.5)
                samples[v, k] = np.where(ok, np.where(r < 255.0, r, 255.0), 0.0).astype(np.uint8)
        seen[v] = ok
    return seen, samples


# ------------------------------------------------------------------------------------------- the sample in plain loops
def sample_loops(vertices, normals, proj, centres, depth, keep, images, tol, min_cos=0.35, channels=None):
    """The same outputs vertex by vertex and view by view, every number a scalar: a second formulation."""
    F = np.float64
    X = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    N = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    proj = np.asarray(proj, dtype=np.float64).reshape(-1, 12)
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    ch = cr.channels_of(images, channels)
    tol, min_cos = F(tol), F(min_cos)
    seen = np.zeros((len(depth), len(X)), np.uint8)
    samples = np.zeros((len(depth), ch, len(X)), np.uint8)
    with np.errstate(all="ignore"):
        for i in range(len(X)):
            x = [F(t) for t in X[i]]
            n = [F(t) for t in N[i]]
            for v in range(len(depth)):
                h, w = depth[v].shape
                P = proj[v]
                q = [((P[4 * r] * x[0] + P[4 * r + 1] * x[1]) + P[4 * r + 2] * x[2]) + P[4 * r + 3] for r in range(3)]
                u, vv = q[0] / q[2], q[1] / q[2]
                if not (q[2] > 0 and u >= -0.5 and u < F(w) - 0.5 and vv >= -0.5 and vv < F(h) - 0.5):
                    continue
                xi, yi = min(int(np.floor(u + 0.5)), w - 1), min(int(np.floor(vv + 0.5)), h - 1)
                ds = F(depth[v][yi, xi])
                if not np.isfinite(ds) or (keep is not None and keep[v][yi, xi] == 0):
                    continue
                d = ds - q[2]
                if not (d >= -tol and d <= tol):
                    continue
                g = [F(centres[v][a]) - x[a] for a in range(3)]
                l2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
                if not (np.isfinite(l2) and l2 > 0):
                    continue
                c = F(1.0) if (n[0] == 0 and n[1] == 0 and n[2] == 0) else ((n[0] * g[0] + n[1] * g[1]) + n[2] * g[2]) / np.sqrt(l2)
                if not c >= min_cos:
                    continue
                x0, y0 = np.floor(u), np.floor(vv)
                fx, fy = u - x0, vv - y0
                cols = [min(max(int(x0) + t, 0), w - 1) for t in (0, 1)]
                rows = [min(max(int(y0) + t, 0), h - 1) for t in (0, 1)]
                img = images[v].reshape(h, w, ch)
                seen[v, i] = 1
                for k in range(ch):
                    a, b = F(img[rows[0], cols[0], k]), F(img[rows[0], cols[1], k])
                    e, f = F(img[rows[1], cols[0], k]), F(img[rows[1], cols[1], k])
                    top = a + fx * (b - a)
                    bot = e + fx * (f - e)
                    r = np.floor((top + fy * (bot - top)) + 0.5)
                    samples[v, k, i] = int(r) if r < 255 else 255
    return seen, samples


# ------------------------------------------------------------------------------------------- the tables
def tables(seen, samples):
    """(overlap int64 [n,n], sums int64 [n,n,ch]): overlap = F F^T and sums_k = (Q_k F) F^T with F = (seen != 0)."""
    F = (np.asarray(seen) != 0).astype(np.int64)
    Q = np.asarray(samples).astype(np.int64)
    n, ch = F.shape[0], Q.shape[1]
    overlap = F @ F.T
    sums = np.zeros((n, n, ch), np.int64)
    for k in range(ch):
        sums[:, :, k] = (Q[:, k, :] * F) @ F.T
    return overlap, sums


def tables_loops(seen, samples):
    """The same by counting, vertex by vertex."""
    n, ch, nv = np.asarray(samples).shape
    overlap, sums = np.zeros((n, n), np.int64), np.zeros((n, n, ch), np.int64)
    for x in range(nv):
        who = [i for i in range(n) if seen[i][x] != 0]
        for i in who:
            for j in who:
                overlap[i, j] += 1
                for k in range(ch):
                    sums[i, j, k] += int(samples[i][k][x])
    return overlap, sums


# ------------------------------------------------------------------------------------------- the gains
def solve_gains(overlap, sums, sigma_n=10.0, sigma_g=1.0, min_overlap=1):
    """float64 [n,ch]: the statement of include/sfm_amd.h pair by pair."""
    overlap, sums = np.asarray(overlap), np.asarray(sums)
    n, ch = overlap.shape[0], sums.shape[2]
    use = lambda i, j: i != j and overlap[i, j] >= min_overlap and overlap[i, j] > 0
    active = [i for i in range(n) if any(use(i, j) for j in range(n))]
    pos = {i: p for p, i in enumerate(active)}
    gains = np.ones((n, ch))
    if not active:
        return gains
    for k in range(ch):
        A, rhs = np.zeros((len(active), len(active))), np.zeros(len(active))
        for i in active:
            for j in active:
                if not use(i, j):
                    continue
                N = float(overlap[i, j])
                a, b = float(sums[i, j, k]) / N, float(sums[j, i, k]) / N
                A[pos[i], pos[i]] += N * (a * a / sigma_n ** 2 + 1.0 / sigma_g ** 2)
                A[pos[j], pos[j]] += N * b * b / sigma_n ** 2
                A[pos[i], pos[j]] -= N * a * b / sigma_n ** 2
                A[pos[j], pos[i]] -= N * a * b / sigma_n ** 2
                rhs[pos[i]] += N / sigma_g ** 2
        gains[active, k] = np.linalg.solve(A, rhs)
    return gains


def apply_gain(image, gain):
    """uint8 like image: min(floor(I * g + 0.5), 255) per pixel; gain a number or one per channel of an [h,w,3] image."""
    p = np.asarray(image, dtype=np.uint8).astype(np.float64) * np.asarray(gain, dtype=np.float64)
    r = np.floor(p + 0.5)
    return np.where(r < 255.0, r, 255.0).astype(np.uint8)


def apply_gains(images, gains):
    gains = np.asarray(gains, dtype=np.float64).reshape(len(images), -1)
    return [apply_gain(a, g if np.ndim(a) == 3 else g[0]) for a, g in zip(images, gains)]


def spread(seen, samples):
    """float64 [nv,ch]: per vertex and channel the largest minus the smallest sample over the vertex's views; NaN with fewer
    than 2 views."""
    seen = np.asarray(seen) != 0
    q = np.asarray(samples).astype(np.int64)
    out = np.full((seen.shape[1], q.shape[1]), np.nan)
    for x in np.flatnonzero(seen.sum(axis=0) >= 2):
        mine = q[seen[:, x], :, x]                                 # [views of x, channels]
        out[x] = mine.max(axis=0) - mine.min(axis=0)
    return out


# ------------------------------------------------------------------------------------------- the gained sphere
def true_gains(n=14, seed=0):
    return np.round(np.random.default_rng(seed).uniform(0.6, 1.1, n), 3)


def gained_sphere_scene():
    """`colour_sphere_scene()` with every image multiplied by its gain of `true_gains()` and rounded half up.
    Returns (proj, depth, origin, voxel, shape, trunc, centres, images as rendered, gained images, g_true)."""
    proj, depth, origin, voxel, shape, trunc, centres, images = cr.colour_sphere_scene()
    g = true_gains(len(images))
    gained = [apply_gain(a, gk) for a, gk in zip(images, g)]
    return proj, depth, origin, voxel, shape, trunc, centres, images, gained, g


def worth(vertices, normals, proj, centres, depth, trunc, rendered, gained, g_true, sigma_g, sigma_n=10.0, compensated=None):
    """One row of the worth table for the gained images compensated with sigma_g: {gains, error (median, p95, max), spread
    (median, p95), agreement per channel}.  `compensated`: the corrected images where something else than `apply_gains`
    made them (the device)."""
    seen, q = sample(vertices, normals, proj, centres, depth, None, gained, trunc, 0.35)
    g_est = solve_gains(*tables(seen, q), sigma_n, sigma_g, 1)
    fixed = apply_gains(gained, g_est) if compensated is None else compensated
    col, n_views, best = cr.colors(vertices, normals, proj, centres, depth, None, fixed, trunc, 0.35, 0)
    prod = g_est * np.asarray(g_true)[:, None]
    return dict(gains=g_est, error=scaled_error(col, n_views, vertices, float(prod.mean())),
                spread=spread_summary(*sample(vertices, normals, proj, centres, depth, None, fixed, trunc, 0.35)),
                agreement=(prod.max(axis=0) - prod.min(axis=0)) / prod.mean(axis=0))


def scaled_error(col, n_views, vertices, s):
    """(median, p95, max) of |colour / s - texture at the radial foot point| over the seen vertices."""
    X = np.asarray(vertices, dtype=np.float64)
    truth = cr.sphere_texture(X / np.linalg.norm(X, axis=1, keepdims=True))
    err = np.abs(np.asarray(col, dtype=np.float64) / s - truth)[np.asarray(n_views) > 0]
    return float(np.median(err)), float(np.percentile(err, 95)), float(err.max())


def spread_summary(seen, samples):
    sp = spread(seen, samples)
    sp = sp[np.isfinite(sp)]
    return float(np.median(sp)), float(np.percentile(sp, 95))
