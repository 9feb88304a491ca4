"""NumPy restatement of the mesh render (sfm_amd/csrc/mesh_render.hip; include/sfm_amd.h states the rule): the mesh drawn
through a camera, operation for operation - float64 with every product and sum rounded on its own, the winner of a pixel
the smallest (depth as float32, triangle) - so that the device's output bytes can be compared with these.  Twice: triangle
by triangle over its box with a minimum per pixel (`render`), and in plain loops pixel by pixel over all triangles with a
lexicographic comparison (`render_loops`)."""
import numpy as np

import mesh_color_reference as cr
import mesh_reference as mr
import mesh_texture_reference as tr

NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
NAN_BITS = np.uint32(0x7FC00000)
SMALL_BOX = 64                                                    # the device walks a larger box in its second pass
F = np.float64


# ------------------------------------------------------------------------------------------- the steps on arrays
def project(P, X):
    """Step 1: (u, v, q2) float64 [n] each; zeros where the vertex is not usable."""
    P = np.asarray(P, dtype=np.float64).reshape(12)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        q0 = ((P[0] * X[:, 0] + P[1] * X[:, 1]) + P[2] * X[:, 2]) + P[3]
        q1 = ((P[4] * X[:, 0] + P[5] * X[:, 1]) + P[6] * X[:, 2]) + P[7]
        q2 = ((P[8] * X[:, 0] + P[9] * X[:, 1]) + P[10] * X[:, 2]) + P[11]
        u, v = q0 / q2, q1 / q2
        ok = (q2 > 0) & np.isfinite(u) & np.isfinite(v) & np.isfinite(q2)
    return np.where(ok, u, 0.0), np.where(ok, v, 0.0), np.where(ok, q2, 0.0)


def span(a, b, c, n):
    """Step 2 on one axis: (first, last, not empty) of ceil(min) .. floor(max) cut to 0 .. n - 1."""
    lo = np.ceil(np.minimum(np.minimum(a, b), c))
    hi = np.floor(np.maximum(np.maximum(a, b), c))
    lo = np.where(lo > 0.0, lo, 0.0)
    hi = np.where(hi < F(n - 1), hi, F(n - 1))
    ok = lo <= hi
    return np.where(ok, lo, 0.0).astype(np.int64), np.where(ok, hi, -1.0).astype(np.int64), ok


def edge_functions(ua, va, ub, vb, uc, vc, x, y):
    """Step 3: (w0, w1, w2, A)."""
    with np.errstate(all="ignore"):
        w0 = (ub - x) * (vc - y) - (vb - y) * (uc - x)
        w1 = (uc - x) * (va - y) - (vc - y) * (ua - x)
        w2 = (ua - x) * (vb - y) - (va - y) * (ub - x)
        return w0, w1, w2, (w0 + w1) + w2


def claims(corners, x, y, tri):
    """Steps 3 to 5 for triangles (corners = 9 arrays ua, va, qa, ub, ...) at the pixel centres (x, y): the uint64 key, NO_KEY
    where the triangle does not draw there."""
    ua, va, qa, ub, vb, qb, uc, vc, qc = corners
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    w0, w1, w2, A = edge_functions(ua, va, ub, vb, uc, vc, x, y)
    with np.errstate(all="ignore"):
        inside = (A != 0.0) & (((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0)))
        s = (w0 / qa + w1 / qb) + w2 / qc
        d = (A / s).astype(np.float32)
        ok = inside & np.isfinite(d) & (d > 0)
    key = (np.ascontiguousarray(d).view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(tri).astype(np.uint64)
    return np.where(ok, key, NO_KEY)


def rasterise(vertices, triangles, P, w, h):
    """Steps 1 to 5 for one camera: (keys uint64 [h,w], (u, v, q2) of the vertices, boxes of more than SMALL_BOX pixels)."""
    X = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    nv = len(X)
    u, v, q2 = project(P, X)
    keys = np.full(h * w, NO_KEY, np.uint64)
    good = ((T >= 0) & (T < nv)).all(axis=1)
    idx = np.where(good[:, None], T, 0)
    if nv == 0 or len(T) == 0 or h == 0 or w == 0:
        return keys.reshape(h, w), (u, v, q2), 0
    good &= (q2[idx] > 0).all(axis=1)
    ua, ub, uc = (u[idx[:, k]] for k in range(3))
    va, vb, vc = (v[idx[:, k]] for k in range(3))
    x0, x1, okx = span(ua, ub, uc, w)
    y0, y1, oky = span(va, vb, vc, h)
    good &= okx & oky
    t = np.nonzero(good)[0]
    x0, x1, y0, y1 = x0[t], x1[t], y0[t], y1[t]
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    n_large = int((bw * bh > SMALL_BOX).sum())
    corner = lambda sel: tuple(a[idx[sel, k]] for k in range(3) for a in (u, v, q2))
    # boxes of at most 8 x 8: all of them at once, offset by offset
    small = (bw <= 8) & (bh <= 8)
    ts = t[small]
    if len(ts):
        sx0, sy0, sbw, sbh = x0[small], y0[small], bw[small], bh[small]
        for dy in range(int(sbh.max())):
            for dx in range(int(sbw.max())):
                sel = (sbw > dx) & (sbh > dy)
                if sel.any():
                    x, y = sx0[sel] + dx, sy0[sel] + dy
                    np.minimum.at(keys, y * w + x, claims(corner(ts[sel]), x, y, ts[sel]))
    # the rest one by one over its box
    for j in np.nonzero(~small)[0]:
        y, x = np.mgrid[y0[j]:y1[j] + 1, x0[j]:x1[j] + 1]
        c = tuple(F(a[idx[t[j], k]]) for k in range(3) for a in (u, v, q2))
        np.minimum.at(keys, (y * w + x).ravel(), claims(c, x, y, np.full(x.shape, t[j])).ravel())
    return keys.reshape(h, w), (u, v, q2), n_large


def round_u8(x):
    with np.errstate(all="ignore"):
        r = np.floor(x + 0.5)
        return np.where(r < 255.0, np.where(r > 0.0, r, 0.0), 255.0).astype(np.uint8)


def tap(t, n):
    with np.errstate(all="ignore"):
        return np.where(t >= 0.0, np.where(t <= F(n - 1), t, F(n - 1)), 0.0).astype(np.int64)


def resolve(keys, projected, triangles, vertex_colors=None, uv=None, atlas=None, fill=0):
    """Step 6: (depth float32 [h,w], triangle int32 [h,w], bary float32 [h,w,3], color uint8 [h,w] / [h,w,3] or None)."""
    h, w = keys.shape
    u, v, q2 = projected
    T = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    drawn = keys != NO_KEY
    tri = np.where(drawn, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1)
    depth = np.where(drawn, (keys >> np.uint64(32)).astype(np.uint32), NAN_BITS).astype(np.uint32).view(np.float32)
    bary = np.zeros((h, w, 3), np.float32)
    color = None
    ch = 1
    if vertex_colors is not None:
        vertex_colors = np.asarray(vertex_colors, dtype=np.uint8)
        ch = 3 if vertex_colors.ndim == 2 else 1
    if atlas is not None:
        atlas = np.asarray(atlas, dtype=np.uint8)
        ch = 3 if atlas.ndim == 3 else 1
    if vertex_colors is not None or atlas is not None:
        color = np.full((h, w, ch), fill, np.uint8)
    ys, xs = np.nonzero(drawn)
    if len(ys):
        t = tri[ys, xs]
        idx = T[t]
        ua, ub, uc = (u[idx[:, k]] for k in range(3))
        va, vb, vc = (v[idx[:, k]] for k in range(3))
        qa, qb, qc = (q2[idx[:, k]] for k in range(3))
        w0, w1, w2, A = edge_functions(ua, va, ub, vb, uc, vc, xs.astype(np.float64), ys.astype(np.float64))
        with np.errstate(all="ignore"):
            r0, r1, r2 = w0 / qa, w1 / qb, w2 / qc
            s = (r0 + r1) + r2
            b0, b1, b2 = r0 / s, r1 / s, r2 / s
        bary[ys, xs] = np.stack([b0, b1, b2], axis=-1).astype(np.float32)
        if vertex_colors is not None:
            col = vertex_colors.reshape(len(vertex_colors), ch).astype(np.float64)
            for k in range(ch):
                with np.errstate(all="ignore"):
                    color[ys, xs, k] = round_u8((b0 * col[idx[:, 0], k] + b1 * col[idx[:, 1], k]) + b2 * col[idx[:, 2], k])
        elif atlas is not None:
            H, W = atlas.shape[:2]
            U = np.asarray(uv, dtype=np.float32).reshape(-1, 3, 2).astype(np.float64)[t]
            with np.errstate(all="ignore"):
                px = ((b0 * U[:, 0, 0] + b1 * U[:, 1, 0]) + b2 * U[:, 2, 0]) * F(W) - 0.5
                py = ((b0 * U[:, 0, 1] + b1 * U[:, 1, 1]) + b2 * U[:, 2, 1]) * F(H) - 0.5
                x0, y0 = np.floor(px), np.floor(py)
                fx, fy = px - x0, py - y0
                xa, xb, ya, yb = tap(x0, W), tap(x0 + 1.0, W), tap(y0, H), tap(y0 + 1.0, H)
                img = atlas.reshape(H, W, ch)
                for k in range(ch):
                    a, b = img[ya, xa, k].astype(np.float64), img[ya, xb, k].astype(np.float64)
                    e, f = img[yb, xa, k].astype(np.float64), img[yb, xb, k].astype(np.float64)
                    top = a + fx * (b - a)
                    bot = e + fx * (f - e)
                    color[ys, xs, k] = round_u8(top + fy * (bot - top))
    if color is not None and ch == 1:
        color = color[:, :, 0]
    return depth, tri.astype(np.int32), bary, color


class Render:
    """Per camera the four outputs, and n_large: the boxes of more than SMALL_BOX pixels over all cameras."""

    def __init__(self):
        self.depth, self.triangle, self.bary, self.color, self.n_large = [], [], [], [], 0

    @property
    def coverage(self):
        return [float((t >= 0).mean()) if t.size else 0.0 for t in self.triangle]


def render(vertices, triangles, proj, sizes, vertex_colors=None, uv=None, atlas=None, fill=0):
    """The rule on arrays.  proj float64 [n,12], sizes [(width, height)] per camera."""
    out = Render()
    for P, (w, h) in zip(np.asarray(proj, dtype=np.float64).reshape(-1, 12), sizes):
        keys, projected, n_large = rasterise(vertices, triangles, P, w, h)
        d, t, b, c = resolve(keys, projected, triangles, vertex_colors, uv, atlas, fill)
        out.depth.append(d); out.triangle.append(t); out.bary.append(b); out.color.append(c)
        out.n_large += n_large
    if vertex_colors is None and atlas is None:
        out.color = None
    return out


# ------------------------------------------------------------------------------------------- the rule in plain loops
def render_loops(vertices, triangles, proj, sizes, vertex_colors=None, uv=None, atlas=None, fill=0):
    """The same outputs pixel by pixel over all triangles, every number a scalar: a second formulation."""
    X = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    nv = len(X)
    out = Render()
    ch = 0
    if vertex_colors is not None:
        vertex_colors = np.asarray(vertex_colors)
        ch = 3 if vertex_colors.ndim == 2 else 1
        vcol = vertex_colors.reshape(nv, ch)
    if atlas is not None:
        atlas = np.asarray(atlas)
        ch = 3 if atlas.ndim == 3 else 1
        H, W = atlas.shape[:2]
        img = atlas.reshape(H, W, ch)
        uv = np.asarray(uv, dtype=np.float32).reshape(-1, 3, 2)
    clampi = lambda t, n: 0 if not t >= 0 else (int(t) if t <= n - 1 else n - 1)
    rnd = lambda x: int(min(max(np.floor(x + 0.5), 0.0), 255.0)) if np.floor(x + 0.5) < 255.0 else 255
    with np.errstate(all="ignore"):
        for P, (w, h) in zip(np.asarray(proj, dtype=np.float64).reshape(-1, 12), sizes):
            pv = []
            for i in range(nv):
                q = [((P[4 * r] * X[i, 0] + P[4 * r + 1] * X[i, 1]) + P[4 * r + 2] * X[i, 2]) + P[4 * r + 3] for r in range(3)]
                a, b = q[0] / q[2], q[1] / q[2]
                pv.append((a, b, q[2]) if (q[2] > 0 and np.isfinite(a) and np.isfinite(b) and np.isfinite(q[2])) else None)
            live = []
            for t in range(len(T)):
                if all(0 <= int(i) < nv for i in T[t]) and all(pv[int(i)] is not None for i in T[t]):
                    a, b, c = (pv[int(i)] for i in T[t])
                    if (np.ceil(min(a[0], b[0], c[0])) <= np.floor(max(a[0], b[0], c[0])) and
                            np.ceil(min(a[1], b[1], c[1])) <= np.floor(max(a[1], b[1], c[1]))):
                        live.append((t, a, b, c))
            depth = np.full((h, w), NAN_BITS, np.uint32).view(np.float32)
            tri, bary = np.full((h, w), -1, np.int32), np.zeros((h, w, 3), np.float32)
            color = np.full((h, w, ch), fill, np.uint8) if ch else None
            n_large = 0
            for t, a, b, c in live:
                bw = min(np.floor(max(a[0], b[0], c[0])), w - 1) - max(np.ceil(min(a[0], b[0], c[0])), 0) + 1
                bh = min(np.floor(max(a[1], b[1], c[1])), h - 1) - max(np.ceil(min(a[1], b[1], c[1])), 0) + 1
                n_large += bool(bw > 0 and bh > 0 and bw * bh > SMALL_BOX)
            for y in range(h):
                for x in range(w):
                    best = None
                    fx_, fy_ = F(x), F(y)
                    for t, a, b, c in live:
                        if not (np.ceil(min(a[0], b[0], c[0])) <= x <= np.floor(max(a[0], b[0], c[0])) and
                                np.ceil(min(a[1], b[1], c[1])) <= y <= np.floor(max(a[1], b[1], c[1]))):
                            continue
                        w0 = (b[0] - fx_) * (c[1] - fy_) - (b[1] - fy_) * (c[0] - fx_)
                        w1 = (c[0] - fx_) * (a[1] - fy_) - (c[1] - fy_) * (a[0] - fx_)
                        w2 = (a[0] - fx_) * (b[1] - fy_) - (a[1] - fy_) * (b[0] - fx_)
                        A = (w0 + w1) + w2
                        if A == 0 or not ((w0 >= 0 and w1 >= 0 and w2 >= 0) or (w0 <= 0 and w1 <= 0 and w2 <= 0)):
                            continue
                        r = (w0 / a[2], w1 / b[2], w2 / c[2])
                        s = (r[0] + r[1]) + r[2]
                        d = np.float32(A / s)
                        if not (np.isfinite(d) and d > 0):
                            continue
                        if best is None or (d, t) < best[:2]:
                            best = (d, t, (r[0] / s, r[1] / s, r[2] / s))
                    if best is None:
                        continue
                    d, t, bk = best
                    depth[y, x], tri[y, x], bary[y, x] = d, t, [np.float32(v) for v in bk]
                    i0, i1, i2 = (int(i) for i in T[t])
                    for k in range(ch):
                        if vertex_colors is not None:
                            color[y, x, k] = rnd((bk[0] * F(vcol[i0, k]) + bk[1] * F(vcol[i1, k])) + bk[2] * F(vcol[i2, k]))
                        else:
                            px = ((bk[0] * F(uv[t, 0, 0]) + bk[1] * F(uv[t, 1, 0])) + bk[2] * F(uv[t, 2, 0])) * F(W) - 0.5
                            py = ((bk[0] * F(uv[t, 0, 1]) + bk[1] * F(uv[t, 1, 1])) + bk[2] * F(uv[t, 2, 1])) * F(H) - 0.5
                            x0, y0 = np.floor(px), np.floor(py)
                            gx, gy = px - x0, py - y0
                            xa, xb, ya, yb = clampi(x0, W), clampi(x0 + 1.0, W), clampi(y0, H), clampi(y0 + 1.0, H)
                            p, q, e, f = F(img[ya, xa, k]), F(img[ya, xb, k]), F(img[yb, xa, k]), F(img[yb, xb, k])
                            top = p + gx * (q - p)
                            bot = e + gx * (f - e)
                            color[y, x, k] = rnd(top + gy * (bot - top))
            out.depth.append(depth); out.triangle.append(tri); out.bary.append(bary)
            out.color.append(color[:, :, 0] if ch == 1 else color)
            out.n_large += n_large
    if not ch:
        out.color = None
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what=""):
    """Every output byte, camera by camera: depth and bary as float32 bits, triangle, color.  got may be a `MeshRender`."""
    assert len(got.depth) == len(want.depth), (what, len(got.depth), len(want.depth))
    for c in range(len(want.depth)):
        for name in ("triangle", "depth", "bary", "color"):
            g, w = getattr(got, name), getattr(want, name)
            if w is None or g is None:
                assert w is None and g is None, (what, name)
                continue
            g, w = np.asarray(g[c]), np.asarray(w[c])
            assert g.dtype == w.dtype and g.shape == w.shape, (what, c, name, g.dtype, w.dtype, g.shape, w.shape)
            if name in ("depth", "bary"):
                g, w = bits(g), bits(w)
            assert np.array_equal(g, w), (what, c, name, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())


# ------------------------------------------------------------------------------------------- scenes
class Scene:
    """What both restatements, `sfm_amd.render_mesh` and the host build take: `args()` in front, `kwargs()` behind."""

    def __init__(self, vertices, triangles, proj, sizes, vertex_colors=None, uv=None, atlas=None, fill=0):
        self.vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.triangles = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
        self.proj = np.asarray(proj, dtype=np.float64).reshape(-1, 12)
        self.sizes = [(int(w), int(h)) for w, h in sizes]
        self.vertex_colors, self.uv, self.atlas, self.fill = vertex_colors, uv, atlas, fill

    def args(self):
        return self.vertices, self.triangles, self.proj, self.sizes

    def kwargs(self):
        return dict(vertex_colors=self.vertex_colors, uv=self.uv, atlas=self.atlas, fill=self.fill)


def reference(scene):
    return render(*scene.args(), **scene.kwargs())


def random_scene(seed, n_vertices, n_triangles, sizes, source=None, channels=1, wild_uv=False, fill=9):
    """Cameras and vertices of `mesh_color_reference` (vertices near the plane z = 0 in front of the cameras, one in twenty
    with a NaN coordinate) at sizes [(width, height)]; even triangles take three random vertices and span much of an image,
    odd ones a vertex and two of its nearest neighbours; one triangle in ten has an index of -1 or n_vertices.  source: None,
    "vertex" or "atlas" (the layout of the texture at texels 2 with random texels; wild_uv puts some uv outside the atlas and
    one at NaN)."""
    rng = np.random.default_rng(seed)
    proj = cr.random_views(rng, [(h, w) for w, h in sizes], 1)[0]
    X = cr.random_vertices(rng, n_vertices)[0]
    T = rng.integers(0, max(n_vertices, 1), (n_triangles, 3)).astype(np.int32)
    if n_vertices >= 3:
        P = np.nan_to_num(X, nan=1e3)
        for t in range(1, n_triangles, 2):
            near = np.argsort(((P - P[T[t, 0]]) ** 2).sum(axis=1))[1:4]
            T[t, 1:] = rng.permutation(near)[:2]
    for t in range(n_triangles):
        if rng.random() < 0.1:
            T[t, rng.integers(0, 3)] = rng.choice([-1, n_vertices])
    vcol = uv = atlas = None
    if source == "vertex":
        vcol = rng.integers(0, 256, n_vertices if channels == 1 else (n_vertices, 3), dtype=np.uint8)
    elif source == "atlas":
        cpr = tr.default_cells_per_row(n_triangles)
        W, H = tr.atlas_size(n_triangles, 2, cpr)
        uv = tr.corner_uv(n_triangles, 2, cpr)
        atlas = rng.integers(0, 256, (max(H, 1), W) if channels == 1 else (max(H, 1), W, 3), dtype=np.uint8)
        if wild_uv and n_triangles:
            k = rng.integers(0, n_triangles, max(n_triangles // 4, 1))
            uv[k] = rng.uniform(-0.5, 1.5, (len(k), 3, 2)).astype(np.float32)
            uv[k[0], 0, 0] = np.nan
    return Scene(X, T, proj, sizes, vcol, uv, atlas, fill)


def close_up_scene(seed=5, n=12, size=(48, 40)):
    """A grid of (n - 1)^2 * 2 small triangles on the plane z = 3 and four that are several times larger, seen by one
    camera at the origin so that the small ones take boxes of a few pixels and the large ones of hundreds: both raster
    passes of the device draw into the one image."""
    rng = np.random.default_rng(seed)
    w, h = size
    g = np.linspace(-1.0, 1.0, n)
    gx, gy = np.meshgrid(g, g)
    X = np.c_[gx.ravel() + rng.normal(0, 0.01, n * n), gy.ravel() + rng.normal(0, 0.01, n * n), 3.0 + rng.normal(0, 0.05, n * n)]
    T = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            T += [(a, a + 1, a + n), (a + 1, a + n + 1, a + n)]
    big = np.array([[-0.9, -0.8, 2.5], [0.7, -0.6, 2.6], [-0.5, 0.9, 2.4], [0.8, 0.8, 3.5], [-0.8, 0.2, 3.6], [0.1, -0.9, 3.4]])
    T += [(n * n, n * n + 1, n * n + 2), (n * n + 3, n * n + 4, n * n + 5), (n * n + 2, n * n + 1, n * n + 3), (0, n * n - 1, n * n + 4)]
    X = np.concatenate([X, big])
    f = 0.9 * w
    P = np.array([f, 0, (w - 1) / 2.0, 0, 0, f, (h - 1) / 2.0, 0, 0, 0, 1.0, 0])
    vcol = rng.integers(0, 256, (len(X), 3), dtype=np.uint8)
    return Scene(X, np.array(T, np.int32), [P], [size], vcol, None, None, 4)


# ------------------------------------------------------------------------------------------- hand cases
UNIT = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])        # u = X / Z, v = Y / Z, depth Z


def at(u, v, z):
    """The point that the camera UNIT sees at (u, v) with the depth z; exact for the z used here (powers of two)."""
    return (u * z, v * z, z)


def hand_cases():
    """(name, vertices, triangles, (width, height)) seen through UNIT; tests/test_mesh_render_reference.py holds what each
    must give."""
    cases = []
    # A at depth 4 covers the image's left part; B at depth 2 covers a part of that
    cases.append(("overlap", [at(0, 0, 4), at(4, 0, 4), at(0, 4, 4), at(0, 0, 2), at(2, 0, 2), at(0, 2, 2)], [(0, 1, 2), (3, 4, 5)], (6, 5)))
    # the square 0 .. 4 cut along its diagonal at one depth: the pixels (k, k) lie on the shared edge
    cases.append(("shared edge", [at(0, 0, 2), at(4, 0, 2), at(4, 4, 2), at(0, 4, 2)], [(0, 1, 2), (0, 2, 3)], (6, 6)))
    cases.append(("vertex on a pixel centre", [at(2, 1, 2), at(2.5, 1.25, 2), at(2.25, 1.5, 2)], [(0, 1, 2)], (5, 3)))
    cases.append(("between pixel centres", [at(2.125, 1.125, 2), at(2.875, 1.125, 2), at(2.125, 1.875, 2)], [(0, 1, 2)], (5, 3)))
    cases.append(("zero area", [at(0, 0, 2), at(2, 2, 2), at(4, 4, 2)], [(0, 1, 2)], (6, 6)))
    cases.append(("a corner behind the camera", [at(0, 0, 2), at(4, 0, 2), (0.0, -8.0, -2.0)], [(0, 1, 2)], (6, 6)))
    cases.append(("NaN vertex and bad indices", [at(0, 0, 2), at(4, 0, 2), at(0, 4, 2), (np.nan, 0.0, 2.0)],
                  [(0, 1, 3), (0, 1, 4), (0, -1, 2), (0, 1, 2)], (6, 6)))
    cases.append(("both orientations", [at(0, 0, 2), at(4, 0, 2), at(0, 4, 2), at(0, 0, 4), at(4, 0, 4), at(0, 4, 4)], [(0, 2, 1), (3, 4, 5)], (6, 6)))
    cases.append(("larger than the image", [at(-100, -100, 4), at(300, -100, 4), at(-100, 300, 4)], [(0, 1, 2)], (5, 3)))
    cases.append(("one pixel", [at(-100, -100, 4), at(300, -100, 4), at(-100, 300, 4)], [(0, 1, 2)], (1, 1)))
    cases.append(("no pixel", [at(-100, -100, 4), at(300, -100, 4), at(-100, 300, 4)], [(0, 1, 2)], (0, 4)))
    return [(name, np.array(V, dtype=np.float64), np.array(T, dtype=np.int32), size) for name, V, T, size in cases]


def merged_hand_scene(source="vertex", channels=3):
    """Every hand case in one mesh, drawn through the camera of every case at that case's size."""
    V, T, sizes, first = [], [], [], 0
    for name, v, t, size in hand_cases():
        V.append(v)
        T.append(np.where((t >= 0) & (t < len(v)), t + first, -1))
        sizes.append(size)
        first += len(v)
    V, T = np.concatenate(V), np.concatenate(T).astype(np.int32)
    rng = np.random.default_rng(77)
    vcol = uv = atlas = None
    if source == "vertex":
        vcol = rng.integers(0, 256, len(V) if channels == 1 else (len(V), 3), dtype=np.uint8)
    elif source == "atlas":
        cpr = tr.default_cells_per_row(len(T))
        W, H = tr.atlas_size(len(T), 3, cpr)
        uv, atlas = tr.corner_uv(len(T), 3, cpr), rng.integers(0, 256, (H, W) if channels == 1 else (H, W, 3), dtype=np.uint8)
    return Scene(V, T, [UNIT] * len(sizes), sizes, vcol, uv, atlas, 200)


# ------------------------------------------------------------------------------------------- the textured sphere
NOVEL_CAMERA = (2.9, 1.6, 1.1)                                     # none of `mesh_reference.sphere_cameras()`


def analytic_sphere_view(centre, f, size, w):
    """(hit bool [size,size], depth float64, colour float64 [size,size,3], cosine between the viewing ray and the normal) of
    the unit sphere with the texture `fine_texture` through `look_at(centre)`."""
    P, R, t, K = mr.look_at(centre, f, size)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    ray = np.stack([(xx - K[0, 2]) / f, (yy - K[1, 2]) / f, np.ones_like(xx)], axis=-1) @ R
    C = np.asarray(centre, dtype=np.float64)
    a = (ray * ray).sum(-1)
    b = 2.0 * (ray @ C)
    disc = b * b - 4 * a * (C @ C - 1.0)
    with np.errstate(all="ignore"):
        d = np.where(disc >= 0, (-b - np.sqrt(disc)) / (2 * a), np.nan)
    hit = np.isfinite(d)
    X = C + np.where(hit, d, 0.0)[..., None] * ray
    cosine = np.where(hit, -(ray * X).sum(-1) / np.sqrt(a), 0.0)
    return P, hit, d, tr.fine_texture(X, w), cosine


def sphere_worth(size, f, w, texels):
    """The mesh of the textured sphere (`mesh_texture_reference.textured_sphere_scene`) drawn through its 14 cameras and
    through NOVEL_CAMERA, with the atlas and with the vertex colours, against the analytic image and depth.  Returns
    dict(pixels=compared, atlas=(median, p95, max), vertex=(median, p95, max) in grey levels, depth=largest error in voxels
    over the pixels whose ray meets the sphere at a cosine of at least 0.5, novel=the same three for NOVEL_CAMERA alone,
    unseen=texels without a view among those of the triangles NOVEL_CAMERA draws)."""
    proj, depth, origin, voxel, shape, trunc, centres, images = tr.textured_sphere_scene(size, f, w)
    tsdf, weight = mr.integrate(proj, depth, None, origin, voxel, shape, trunc)
    m = mr.mesh(tsdf, weight, origin, voxel, shape, 1)
    T = np.asarray(m.triangles, dtype=np.int64)
    cpr = tr.default_cells_per_row(len(T))
    atlas, views, uv = tr.texture(m.vertices, m.normals, T, proj, centres, depth, None, images, trunc, texels, 0.35, 0, cpr)
    vcol = cr.colors(m.vertices, m.normals, proj, centres, depth, None, images, trunc, 0.35, 0)[0]
    cams = list(mr.sphere_cameras()) + [NOVEL_CAMERA]
    truth = [analytic_sphere_view(c, f, size, w) for c in cams]
    P = [t[0] for t in truth]
    sizes = [(size, size)] * len(cams)
    ra = render(m.vertices, T, P, sizes, uv=uv, atlas=atlas)
    rv = render(m.vertices, T, P, sizes, vertex_colors=vcol)
    e_atlas, e_vertex, e_depth, per = [], [], [], []
    for c, (_, hit, d, colour, cosine) in enumerate(truth):
        both = hit & (ra.triangle[c] >= 0)
        ea, ev = np.abs(ra.color[c][both].astype(np.float64) - colour[both]), np.abs(rv.color[c][both].astype(np.float64) - colour[both])
        steep = both & (cosine >= 0.5)
        ed = np.abs(ra.depth[c][steep].astype(np.float64) - d[steep]) / voxel
        e_atlas.append(ea.ravel()); e_vertex.append(ev.ravel()); e_depth.append(ed)
        per.append((tr.error_summary(ea), tr.error_summary(ev), float(ed.max())))
    tri_map = tr.inverse_map(len(T), texels, cpr)[0]
    drawn = np.unique(ra.triangle[-1][ra.triangle[-1] >= 0])
    unseen = int((views[np.isin(tri_map, drawn)] == 0).sum())
    return dict(triangles=len(T), pixels=int(sum(len(e) for e in e_depth)), atlas=tr.error_summary(np.concatenate(e_atlas)),
                vertex=tr.error_summary(np.concatenate(e_vertex)), depth=float(np.concatenate(e_depth).max()), novel=per[-1], unseen=unseen,
                coverage=ra.coverage)


# ------------------------------------------------------------------------------------------- the default scene
def default_scene_render(resolution):
    """The default scene of `depth_reference` through the restatements alone - sweep, filter, box at `resolution`, TSDF, mesh -
    drawn through its three views with the plain mean of the corner colours left out: (scene, proj, mesh, Render, true
    depth per view)."""
    import depth_reference as dr
    from sfm_amd.mesh import bounding_grid, projections_from_backprojections
    from test_depth_fuse_reference import scene_maps
    s, (refs, sources, warps, backproj, planes), maps = scene_maps(0)
    f = dr.filter_views(s.images, refs, sources, warps, backproj, maps, 0.02, [12 * len(src) * 25 for src in sources], 1)
    keep, xyz, depth = [v[1] for v in f], [v[2] for v in f], [m[2] for m in maps]
    origin, voxel, shape = bounding_grid(np.concatenate([x[k != 0] for x, k in zip(xyz, keep)]), resolution, 0.05)
    proj = projections_from_backprojections(backproj)
    tsdf, weight = mr.integrate(proj, depth, keep, origin, voxel, shape, 3.0 * voxel)
    m = mr.mesh(tsdf, weight, origin, voxel, shape, 1)
    sizes = [(d.shape[1], d.shape[0]) for d in depth]
    return s, proj, m, render(m.vertices, m.triangles, proj, sizes), [s.depth[r] for r in refs], voxel
