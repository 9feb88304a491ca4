"""NumPy restatement of the mesh colouring (sfm_amd/csrc/mesh_color.hip; include/sfm_amd.h states the rule): per vertex a
blend over the views that see it, operation for operation - float64 with every product and sum rounded on its own - so
that the device's output bytes can be compared with these.  Twice: on arrays (`colors`) and in plain per-vertex loops
(`colors_loops`).  Also the hand cases, the random scenes and the coloured sphere scene the tests share."""
import numpy as np

import mesh_reference as mr


class Scene:
    """Views (proj [n,12], centres [n,3], depth / keep / images: one array per view, keep may be None), vertices, normals and
    the three scalars; `args()` is what both restatements and `sfm_amd.mesh_vertex_colors` take."""

    def __init__(self, proj, centres, depth, keep, images, vertices, normals, tol, min_cos=0.35, fill=0, channels=None):
        self.proj = np.asarray(proj, dtype=np.float64).reshape(-1, 12)
        self.centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
        self.depth = [np.asarray(d, dtype=np.float32) for d in depth]
        self.keep = None if keep is None else [np.asarray(k, dtype=np.uint8) for k in keep]
        self.images = [np.asarray(a, dtype=np.uint8) for a in images]
        self.vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.normals = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
        self.tol, self.min_cos, self.fill = tol, min_cos, fill
        self.channels = channels if channels is not None else (3 if self.images and self.images[0].ndim == 3 else 1)

    def args(self):
        return (self.vertices, self.normals, self.proj, self.centres, self.depth, self.keep, self.images, self.tol, self.min_cos, self.fill)


def channels_of(images, channels=None):
    if channels is not None:
        return int(channels)
    return 3 if len(images) and np.ndim(images[0]) == 3 else 1


# ------------------------------------------------------------------------------------------- the rule on arrays
def colors(vertices, normals, proj, centres, depth, keep, images, tol, min_cos=0.35, fill=0, channels=None):
    """(colors uint8 [nv] or [nv,3], n_views uint8 [nv], best_view int32 [nv]).  depth: one float32 [h,w] per view; keep: one
    uint8 [h,w] per view, or None; images: one uint8 [h,w] or [h,w,3] per VIEW."""
    X = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    n = np.asarray(normals, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    proj = np.asarray(proj, dtype=np.float64).reshape(-1, 12)
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    ch = channels_of(images, channels)
    nv = len(X)
    tol, min_cos = np.float64(tol), np.float64(min_cos)
    acc, W, bw = np.zeros((nv, ch)), np.zeros(nv), np.zeros(nv)
    m, best = np.zeros(nv, np.int64), np.full(nv, -1, np.int64)
    zero_normal = (n == 0).all(axis=1)
    for v, d in enumerate(depth):
        d = np.asarray(d, dtype=np.float32)
        h, w = d.shape
        if h == 0 or w == 0:
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
            wgt = c * c
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
                acc[:, k] = np.where(ok, acc[:, k] + wgt * s, acc[:, k])
            W = np.where(ok, W + wgt, W)
            m += ok
            better = ok & (wgt > bw)
            bw = np.where(better, wgt, bw)
            best = np.where(better, v, best)
    has = (m > 0) & (W > 0)
    with np.errstate(all="ignore"):
        r = np.floor(acc / np.where(has, W, 1.0)[:, None] + 0.5)
        col = np.where(r < 255.0, r, 255.0)
    out = np.where(has[:, None], col, float(fill)).astype(np.uint8)
    return (out[:, 0] if ch == 1 else out), np.minimum(m, 255).astype(np.uint8), best.astype(np.int32)


# ------------------------------------------------------------------------------------------- the rule in plain loops
def colors_loops(vertices, normals, proj, centres, depth, keep, images, tol, min_cos=0.35, fill=0, channels=None):
    """The same outputs vertex by vertex and view by view, every number a scalar: a second formulation."""
    F = np.float64
    X = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    N = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    proj = np.asarray(proj, dtype=np.float64).reshape(-1, 12)
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    ch = channels_of(images, channels)
    tol, min_cos = F(tol), F(min_cos)
    out = np.zeros((len(X), ch), np.uint8)
    n_views, best_view = np.zeros(len(X), np.uint8), np.zeros(len(X), np.int32)
    with np.errstate(all="ignore"):
        for i in range(len(X)):
            x = [F(t) for t in X[i]]
            n = [F(t) for t in N[i]]
            acc, W, m, best, bw = [F(0.0)] * ch, F(0.0), 0, -1, F(0.0)
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
                wgt = c * c
                x0, y0 = np.floor(u), np.floor(vv)
                fx, fy = u - x0, vv - y0
                cols = [min(max(int(x0) + t, 0), w - 1) for t in (0, 1)]
                rows = [min(max(int(y0) + t, 0), h - 1) for t in (0, 1)]
                img = images[v].reshape(h, w, ch)
                for k in range(ch):
                    a, b = F(img[rows[0], cols[0], k]), F(img[rows[0], cols[1], k])
                    e, f = F(img[rows[1], cols[0], k]), F(img[rows[1], cols[1], k])
                    top = a + fx * (b - a)
                    bot = e + fx * (f - e)
                    acc[k] = acc[k] + wgt * (top + fy * (bot - top))
                W = W + wgt
                m += 1
                if wgt > bw:
                    bw, best = wgt, v
            for k in range(ch):
                if m > 0 and W > 0:
                    r = np.floor(acc[k] / W + 0.5)
                    out[i, k] = int(r) if r < 255 else 255
                else:
                    out[i, k] = fill
            n_views[i], best_view[i] = min(m, 255), best
    return (out[:, 0] if ch == 1 else out), n_views, best_view


def assert_same(got, want, what=""):
    for name, g, w in zip(("colors", "n_views", "best_view"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))[:5])


# ------------------------------------------------------------------------------------------- cameras and hand cases
def camera(centre, w, h, f=2.0, back=False):
    """(proj [12], centre) of a camera at `centre` that looks along +z (along -z with back=True), principal point in the
    middle of w x h pixels.  With f = 2 a point at distance 2 in front of it falls on u = x - centre_x + (w - 1) / 2."""
    C = np.asarray(centre, dtype=np.float64)
    R = np.diag([1.0, -1.0, -1.0]) if back else np.eye(3)
    K = np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1.0]])
    return np.c_[K @ R, -K @ R @ C].reshape(12), C


HAND_TOL, HAND_MIN_COS, HAND_FILL = 0.25, 0.5, 7


def ramp(w, h):
    """img[y, x] = 10 x + 40 y + 10: linear, so a bilinear sample is the ramp at (u, v)."""
    y, x = np.mgrid[0:h, 0:w]
    return (10 * x + 40 * y + 10).astype(np.uint8)


def hand_cases():
    """[(name, Scene with gray images, expected colours, expected n_views, expected best_view)]: every expectation is worked
    out by hand.  All share tol 0.25, min_cos 0.5 and fill 7; all cameras have f = 2 and 5 x 3 pixels, so a vertex (x, y, 2)
    in front of a camera at the origin falls on (u, v) = (x + 2, y + 1)."""
    front, origin = camera((0, 0, 0), 5, 3)
    flat = lambda d: np.full((3, 5), d, np.float32)
    const = lambda g: np.full((3, 5), g, np.uint8)
    ones = np.ones((3, 5), np.uint8)
    zero, towards = (0, 0, 0), (0, 0, -1)
    S = lambda views, vertices, normals: Scene([p for p, c, d, k, i in views], [c for p, c, d, k, i in views], [d for p, c, d, k, i in views],
                                               [k for p, c, d, k, i in views], [i for p, c, d, k, i in views], vertices, normals,
                                               HAND_TOL, HAND_MIN_COS, HAND_FILL)
    cases = []
    cases.append(("a pixel centre returns that pixel", S([(front, origin, flat(2), ones, ramp(5, 3))], [(1, 0, 2), (-2, -1, 2), (2, 1, 2)], [zero] * 3),
                  [80, 10, 130], [1, 1, 1], [0, 0, 0]))
    cases.append(("half-way between two pixels returns their mean", S([(front, origin, flat(2), ones, ramp(5, 3))], [(0.5, 0, 2), (0, 0.5, 2)], [zero] * 2),
                  [75, 90], [1, 1], [0, 0]))
    cases.append(("two views of weight 1 holding 10 and 11 return 11",
                  S([(front, origin, flat(2), ones, const(10)), (front, origin, flat(2), ones, const(11))], [(0, 0, 2)], [zero]), [11], [2], [0]))
    cases.append(("a constant image returns the constant", S([(front, origin, flat(2), ones, const(200))], [(0.3, 0.2, 2), (-1.9, 0.77, 2)], [towards] * 2),
                  [200, 200], [1, 1], [0, 0]))
    # occlusion: the vertex lies on the back plane z = 3; view A has a nearer surface (depth 2) at that pixel, view B sees 3
    side, side_c = camera((0.5, 0, 0), 5, 3)
    cases.append(("a view with a nearer depth at the pixel is not used", S([(front, origin, flat(2), ones, const(30)), (side, side_c, flat(3), ones, const(90))],
                                                                            [(0, 0, 3)], [towards]), [90], [1], [1]))
    # a view behind the surface: it sits at z = 4 and looks back; the depth agrees, the normal points away from it
    behind, behind_c = camera((0, 0, 4), 5, 3, back=True)
    cases.append(("a view behind the surface is not used", S([(front, origin, flat(2), ones, const(50)), (behind, behind_c, flat(2), ones, const(150))],
                                                              [(0, 0, 2)], [towards]), [50], [1], [0]))
    # d = ds - q2 = +0.25, -0.25 (both count) and +0.5 (does not)
    cases.append(("d == +-tol still counts", S([(front, origin, flat(2.25), ones, const(40)), (front, origin, flat(1.75), ones, const(60)),
                                                (front, origin, flat(2.5), ones, const(250))], [(0, 0, 2)], [zero]), [50], [2], [0]))
    # g = (0, 0, -2), sqrt(l2) = 2: n = (0, 0, -0.5) gives c = 0.5 exactly; one float32 step less does not pass
    below = np.nextafter(np.float32(-0.5), np.float32(0))
    cases.append(("c == min_cos still counts", S([(front, origin, flat(2), ones, const(99))], [(0, 0, 2), (0, 0, 2)], [(0, 0, -0.5), (0, 0, below)]),
                  [99, 7], [1, 0], [0, -1]))
    # skipped views: the centre handed in is the vertex itself (l2 = 0), a NaN vertex, depths that are not finite, keep = 0
    cases.append(("a vertex at the centre is skipped", S([(front, (0, 0, 2), flat(2), ones, const(99))], [(0, 0, 2)], [towards]), [7], [0], [-1]))
    cases.append(("a NaN vertex is skipped", S([(front, origin, flat(2), ones, const(99))], [(np.nan, 0, 2), (0, 0, np.nan)], [zero] * 2),
                  [7, 7], [0, 0], [-1, -1]))
    bad_depth = flat(2)
    bad_depth[1, 2], bad_depth[1, 3], bad_depth[1, 4] = np.nan, np.inf, -np.inf
    cases.append(("a depth that is not finite is skipped", S([(front, origin, bad_depth, ones, const(99))], [(0, 0, 2), (1, 0, 2), (2, 0, 2), (-1, 0, 2)], [zero] * 4),
                  [7, 7, 7, 99], [0, 0, 0, 1], [-1, -1, -1, 0]))
    some = ones.copy()
    some[1, 2] = 0
    cases.append(("keep = 0 is skipped", S([(front, origin, flat(2), some, const(99))], [(0, 0, 2), (1, 0, 2)], [zero] * 2), [7, 99], [0, 1], [-1, 0]))
    # outside the image, and behind the camera: no view at all
    cases.append(("a vertex with no view gets fill", S([(front, origin, flat(2), ones, const(99))], [(2.5, 0, 2), (0, 0, -2), (0, -1.51, 2)], [zero] * 3),
                  [7, 7, 7], [0, 0, 0], [-1, -1, -1]))
    return [(name, s, np.array(c, np.uint8), np.array(m, np.uint8), np.array(b, np.int32)) for name, s, c, m, b in cases]


def many_views(n=300, n_vertices=1, seed=0):
    """n views of 2 x 2 pixels, all at the origin with f = 2, that all see the vertices on the plane z = 2 (zero normals)."""
    rng = np.random.default_rng(seed)
    p, c = camera((0, 0, 0), 2, 2)
    images = [rng.integers(0, 256, (2, 2), dtype=np.uint8) for _ in range(n)]
    vertices = np.c_[rng.uniform(-0.45, 0.45, (n_vertices, 2)), np.full(n_vertices, 2.0)]
    return Scene([p] * n, [c] * n, [np.full((2, 2), 2.0, np.float32)] * n, None, images, vertices, np.zeros((n_vertices, 3), np.float32),
                 HAND_TOL, HAND_MIN_COS, HAND_FILL)


def merged_hand_cases(channels=1):
    """Every hand case in one scene: case j is moved by (128 j, 0, 0), which changes no number of its own arithmetic beyond
    exact shifts and puts it outside every other case's images.  Returns (Scene, colours, n_views, best_view) expected."""
    proj, centres, depth, keep, images, vertices, normals, col, cnt, best = [], [], [], [], [], [], [], [], [], []
    for j, (name, s, c, m, b) in enumerate(hand_cases()):
        shift = np.array([128.0 * j, 0.0, 0.0])
        first = len(proj)
        for v in range(len(s.proj)):
            P = s.proj[v].reshape(3, 4).copy()
            P[:, 3] = P[:, 3] - P[:, :3] @ shift
            proj.append(P.reshape(12))
            centres.append(s.centres[v] + shift)
        depth += s.depth
        keep += s.keep
        images += s.images
        vertices.append(s.vertices + shift)
        normals.append(s.normals)
        col.append(c); cnt.append(m); best.append(np.where(b >= 0, b + first, -1).astype(np.int32))
    col = np.concatenate(col)
    if channels == 3:
        # two more channels that keep every hand-made blend an exact shift of the first: + 100 (- 100 from 128), + 50 (- 150 from 200)
        second = lambda a: np.where(a < 128, a.astype(np.int16) + 100, a.astype(np.int16) - 100).astype(np.uint8)
        third = lambda a: np.where(a < 200, a.astype(np.int16) + 50, a.astype(np.int16) - 150).astype(np.uint8)
        seen = np.concatenate(cnt) > 0
        images = [np.stack([a, second(a), third(a)], axis=-1) for a in images]
        col = np.stack([col, np.where(seen, second(col), col), np.where(seen, third(col), col)], axis=-1)
    return (Scene(proj, centres, depth, keep, images, np.concatenate(vertices), np.concatenate(normals), HAND_TOL, HAND_MIN_COS, HAND_FILL),
            col, np.concatenate(cnt), np.concatenate(best))


# ------------------------------------------------------------------------------------------- random scenes
def random_views(rng, sizes, channels):
    """Cameras around the origin that look at it from the -z side, within 0.3 rad per axis, with depth maps near the plane
    through the origin that faces them (so that many vertices near the origin pass the occlusion test), a tenth of the depths
    not finite, a fifth of the keep flags zero.  sizes: (h, w) per view; a view may have no pixel."""
    proj, centres, depth, keep, images = [], [], [], [], []
    for h, w in sizes:
        a, b = rng.uniform(-0.3, 0.3, 2)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        R = Rx @ Ry
        dist = rng.uniform(2.0, 3.0)
        C = -R.T @ np.array([0.0, 0.0, dist])
        f = 0.8 * max(w, h, 1)
        K = np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1.0]])
        proj.append(np.c_[K @ R, -K @ R @ C].reshape(12))
        centres.append(C)
        d = (dist + rng.normal(0, 0.08, (h, w))).astype(np.float32)
        bad = rng.random((h, w)) < 0.1
        d[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
        depth.append(d)
        keep.append((rng.random((h, w)) < 0.8).astype(np.uint8))
        images.append(rng.integers(0, 256, (h, w) if channels == 1 else (h, w, 3), dtype=np.uint8))
    return proj, centres, depth, keep, images


def random_vertices(rng, n):
    """Vertices near the plane z = 0 in front of the cameras of `random_views`; normals towards -z with noise, some zero, some
    turned away, one in twenty vertices with a NaN coordinate."""
    X = np.c_[rng.uniform(-0.7, 0.7, (n, 2)), rng.normal(0, 0.08, n)]
    N = np.c_[rng.normal(0, 0.4, (n, 2)), -np.ones(n)]
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    kind = rng.integers(0, 20, n)
    N[kind < 3] = 0.0
    N[kind == 3] *= -1.0
    X[kind == 4, rng.integers(0, 3)] = np.nan
    return X, N.astype(np.float32)


def random_scene(seed, n_vertices, sizes, channels, with_keep=True, tol=0.25, min_cos=0.35, fill=3):
    rng = np.random.default_rng(seed)
    proj, centres, depth, keep, images = random_views(rng, sizes, channels)
    X, N = random_vertices(rng, n_vertices)
    return Scene(proj, centres, depth, keep if with_keep else None, images, X, N, tol, min_cos, fill, channels)


# ------------------------------------------------------------------------------------------- the coloured sphere
def sphere_texture(X):
    """float64 [..., 3]: 127.5 + 100 sin(3 X_k) per channel."""
    return 127.5 + 100.0 * np.sin(3.0 * np.asarray(X, dtype=np.float64))


def colour_sphere_scene(n_cams=14, size=64, f=90.0):
    """`sphere_scene()` defaults plus the camera centres and one size x size x 3 image per camera: a pixel whose ray hits the
    unit sphere at X holds floor(127.5 + 100 sin(3 X_k) + 0.5) in channel k, a pixel that misses holds 0.
    Returns (proj, depth, origin, voxel, shape, trunc, centres, images)."""
    proj, depth, origin, voxel, shape, trunc = mr.sphere_scene(n_cams=n_cams, size=size, f=f)
    centres, images = [], []
    for c in mr.sphere_cameras()[:n_cams]:
        P, R, t, K = mr.look_at(c, f, size)
        yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
        ray = np.stack([(xx - K[0, 2]) / f, (yy - K[1, 2]) / f, np.ones_like(xx)], axis=-1) @ R
        C = np.asarray(c, dtype=np.float64)
        a = (ray * ray).sum(-1)
        b = 2.0 * (ray @ C)
        disc = b * b - 4 * a * (C @ C - 1.0)
        with np.errstate(all="ignore"):
            d = np.where(disc >= 0, (-b - np.sqrt(disc)) / (2 * a), np.nan)
        hit = np.isfinite(d)
        X = C + np.where(hit, d, 0.0)[..., None] * ray
        img = np.where(hit[..., None], np.floor(sphere_texture(X) + 0.5), 0.0).astype(np.uint8)
        centres.append(C)
        images.append(img)
    return proj, depth, origin, voxel, shape, trunc, np.array(centres), images


def nearest_pixel_of_best_view(vertices, best_view, proj, images):
    """The cloud recipe on a mesh: per vertex the nearest pixel of its best view alone (uint8 [nv, ch]; zeros without a view)."""
    X = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    ch = channels_of(images)
    out = np.zeros((len(X), ch), np.uint8)
    for v in np.unique(best_view[best_view >= 0]):
        sel = best_view == v
        h, w = images[v].shape[:2]
        valid, xi, yi, q2 = mr.project(proj[v], X[sel], w, h)
        out[sel] = images[v].reshape(h, w, ch)[yi, xi]
    return out


def error_summary(col, vertices):
    """(median, p95, max) of the absolute error in grey levels against the texture at the vertex's radial foot point."""
    X = np.asarray(vertices, dtype=np.float64)
    truth = sphere_texture(X / np.linalg.norm(X, axis=1, keepdims=True))
    err = np.abs(np.asarray(col, dtype=np.float64) - truth)
    return float(np.median(err)), float(np.percentile(err, 95)), float(err.max())
