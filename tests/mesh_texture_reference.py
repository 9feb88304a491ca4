"""NumPy restatement of the mesh texture (sfm_amd/csrc/mesh_texture.hip; include/sfm_amd.h states the rule): one patch of
texels per triangle in an atlas, every texel the blend of `sfm_mesh_colors` at the texel's point, operation for operation -
float64 with every product and sum rounded on its own - so that the device's output bytes can be compared with these.
Twice: on arrays (`texture`: the points and normals of all texels by the layout, then the blend on them) and in plain
loops over the texels through the inverse map (`texture_loops`).

The blend is that of tests/mesh_color_reference.py with one difference in its input: the normal of a texel stays float64,
while `mesh_color_reference.colors` narrows the normals it is given to float32 as `sfm_mesh_colors` reads them.  So the
per-view steps stand here once more for float64 normals (`blend`, `blend_one`), and the tests hold them to
`mesh_color_reference.colors` on normals that float32 holds exactly."""
import math

import numpy as np

import mesh_color_reference as cr
import mesh_reference as mr

MAX_SIDE = 32768


# ------------------------------------------------------------------------------------------- the layout
def default_cells_per_row(n_triangles):
    cells = (int(n_triangles) + 1) // 2
    r = math.isqrt(cells)
    return max(r + (r * r < cells), 1)


def atlas_size(n_triangles, texels, cells_per_row):
    """(W, H)."""
    P = texels + 3
    cells = (n_triangles + 1) // 2
    return cells_per_row * P, -(-cells // cells_per_row) * P


def texel_at(t, i, j, texels, cells_per_row):
    """The map: (x, y) of local (i, j) of triangle t; arrays or scalars."""
    t, i, j = np.asarray(t, dtype=np.int64), np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    P = texels + 3
    c = t >> 1
    x0, y0 = (c % cells_per_row) * P, (c // cells_per_row) * P
    odd = (t & 1) == 1
    return np.where(odd, x0 + P - 1 - i, x0 + i), np.where(odd, y0 + P - 1 - j, y0 + j)


def inverse_map(n_triangles, texels, cells_per_row):
    """The inverse map on the whole atlas: (tri int64 [H,W], -1 where the texel belongs to no triangle; i, j int64 [H,W])."""
    s, P = texels, texels + 3
    W, H = atlas_size(n_triangles, texels, cells_per_row)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    lx, ly = x % P, y % P
    c = (y // P) * cells_per_row + x // P
    lower, upper = lx + ly <= s + 1, lx + ly >= s + 3
    tri = np.where(lower, 2 * c, np.where(upper, 2 * c + 1, -1))
    i = np.where(lower, lx, P - 1 - lx)
    j = np.where(lower, ly, P - 1 - ly)
    none = (tri < 0) | (tri >= n_triangles)
    return np.where(none, -1, tri), np.where(none, 0, i), np.where(none, 0, j)


def numerators(i, j, texels):
    """(n0, n1, n2) over 2 s; arrays or scalars."""
    i, j, s = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64), texels
    inner = i + j <= s
    g1 = np.clip(2 * i - 1, 0, 2 * s)
    n1 = np.where(inner, 2 * i, g1)
    n2 = np.where(inner, 2 * j, 2 * s - g1)
    return np.where(inner, 2 * s - n1 - n2, 0), n1, n2


def corner_uv(n_triangles, texels, cells_per_row):
    """float32 [nt,3,2]: ((x + 0.5) / W, (y + 0.5) / H) of the texel of every corner, computed in double, rounded once."""
    W, H = atlas_size(n_triangles, texels, cells_per_row)
    t = np.arange(n_triangles, dtype=np.int64)[:, None]
    x, y = texel_at(t, np.array([0, texels, 0])[None, :], np.array([0, 0, texels])[None, :], texels, cells_per_row)
    with np.errstate(all="ignore"):
        return np.stack([(x.astype(np.float64) + 0.5) / np.float64(W), (y.astype(np.float64) + 0.5) / np.float64(max(H, 1))], axis=-1).astype(np.float32)


def interpolate(n0, n1, n2, a0, a1, a2, texels):
    with np.errstate(all="ignore"):
        return ((n0 * a0 + n1 * a1) + n2 * a2) / np.float64(2 * texels)


def points_of(tri, i, j, vertices, normals, triangles, texels):
    """(good bool [...], X float64 [...,3], normal float64 [...,3]) of the texels (tri, i, j): good where the texel has a
    triangle whose three indices are in range; elsewhere X and the normal are zeros and mean nothing."""
    V = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    M = np.asarray(normals, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    T = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    nv = len(V)
    owned = tri >= 0
    idx = T[np.where(owned, tri, 0)] if len(T) else np.zeros(tri.shape + (3,), np.int64)
    good = owned & ((idx >= 0) & (idx < nv)).all(axis=-1)
    idx = np.where(good[..., None], idx, 0)
    V, M = np.concatenate([V, np.zeros((1, 3))]), np.concatenate([M, np.zeros((1, 3))])          # nv may be 0
    n0, n1, n2 = (n.astype(np.float64)[..., None] for n in numerators(i, j, texels))
    X = interpolate(n0, n1, n2, V[idx[..., 0]], V[idx[..., 1]], V[idx[..., 2]], texels)
    g = interpolate(n0, n1, n2, M[idx[..., 0]], M[idx[..., 1]], M[idx[..., 2]], texels)
    with np.errstate(all="ignore"):
        l2 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
        has = np.isfinite(l2) & (l2 > 0)
        normal = np.where(has[..., None], g / np.sqrt(np.where(has, l2, 1.0))[..., None], 0.0)
    return good, np.where(good[..., None], X, 0.0), np.where(good[..., None], normal, 0.0)


# ------------------------------------------------------------------------------------------- the blend, float64 normals
def blend(X, normal, proj, centres, depth, keep, images, tol, min_cos, fill, channels):
    """Steps 1 to 5 of `sfm_mesh_colors` and its finish for the points X [n,3] with the float64 normals [n,3]:
    (colours uint8 [n,ch], views uint8 [n])."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    n = np.asarray(normal, dtype=np.float64).reshape(-1, 3)
    proj = np.asarray(proj, dtype=np.float64).reshape(-1, 12)
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    ch, nv = channels, len(X)
    tol, min_cos = np.float64(tol), np.float64(min_cos)
    acc, W, m = np.zeros((nv, ch)), np.zeros(nv), np.zeros(nv, np.int64)
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
                acc[:, k] = np.where(ok, acc[:, k] + wgt * (top + fy * (bot - top)), acc[:, k])
            W = np.where(ok, W + wgt, W)
            m += ok
    has = (m > 0) & (W > 0)
    with np.errstate(all="ignore"):
        r = np.floor(acc / np.where(has, W, 1.0)[:, None] + 0.5)
    col = np.where(has[:, None], np.where(r < 255.0, r, 255.0), float(fill)).astype(np.uint8)
    return col, np.minimum(m, 255).astype(np.uint8)


def blend_one(x, n, proj, centres, depth, keep, images, tol, min_cos, fill, ch):
    """The same for one point, every number a scalar: ([ch] colours, views)."""
    F = np.float64
    acc, W, m = [F(0.0)] * ch, F(0.0), 0
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
    if m > 0 and W > 0:
        out = []
        for k in range(ch):
            r = np.floor(acc[k] / W + 0.5)
            out.append(int(r) if r < 255 else 255)
        return out, min(m, 255)
    return [fill] * ch, 0


# ------------------------------------------------------------------------------------------- the rule on arrays
def texture(vertices, normals, triangles, proj, centres, depth, keep, images, tol, texels=8, min_cos=0.35, fill=0, cells_per_row=None,
            channels=None):
    """(image uint8 [H,W] or [H,W,3], views uint8 [H,W], uv float32 [nt,3,2])."""
    T = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    nt = len(T)
    cpr = default_cells_per_row(nt) if cells_per_row is None else cells_per_row
    ch = cr.channels_of(images, channels)
    W, H = atlas_size(nt, texels, cpr)
    tri, i, j = inverse_map(nt, texels, cpr)
    good, X, normal = points_of(tri, i, j, vertices, normals, T, texels)
    image, views = np.full((H, W, ch), fill, np.uint8), np.zeros((H, W), np.uint8)
    col, m = blend(X[good], normal[good], proj, centres, depth, keep, images, tol, min_cos, fill, ch)
    image[good], views[good] = col, m
    return (image[:, :, 0] if ch == 1 else image), views, corner_uv(nt, texels, cpr)


# ------------------------------------------------------------------------------------------- the rule in plain loops
def texture_loops(vertices, normals, triangles, proj, centres, depth, keep, images, tol, texels=8, min_cos=0.35, fill=0, cells_per_row=None,
                  channels=None):
    """The same outputs texel by texel through the inverse map, every number a scalar: a second formulation."""
    F = np.float64
    V = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    M = np.asarray(normals, dtype=np.float32).reshape(-1, 3)
    T = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    proj = np.asarray(proj, dtype=np.float64).reshape(-1, 12)
    centres = np.asarray(centres, dtype=np.float64).reshape(-1, 3)
    depth = [np.asarray(d, dtype=np.float32) for d in depth]
    nt, nv, s, P = len(T), len(V), texels, texels + 3
    cpr = default_cells_per_row(nt) if cells_per_row is None else cells_per_row
    ch = cr.channels_of(images, channels)
    cells = (nt + 1) // 2
    W, H = cpr * P, ((cells + cpr - 1) // cpr) * P
    image, views = np.zeros((H, W, ch), np.uint8), np.zeros((H, W), np.uint8)
    tol, min_cos = F(tol), F(min_cos)
    with np.errstate(all="ignore"):
        for y in range(H):
            for x in range(W):
                lx, ly = x % P, y % P
                c = (y // P) * cpr + x // P
                if lx + ly <= s + 1:
                    t, i, j = 2 * c, lx, ly
                elif lx + ly >= s + 3:
                    t, i, j = 2 * c + 1, P - 1 - lx, P - 1 - ly
                else:
                    t = -1
                image[y, x], views[y, x] = fill, 0
                if t < 0 or t >= nt or not all(0 <= int(a) < nv for a in T[t]):
                    continue
                if i + j <= s:
                    n1, n2 = 2 * i, 2 * j
                    n0 = 2 * s - n1 - n2
                else:
                    n1 = min(max(2 * i - 1, 0), 2 * s)
                    n0, n2 = 0, 2 * s - n1
                n0, n1, n2 = F(n0), F(n1), F(n2)
                a0, a1, a2 = (int(a) for a in T[t])
                pt = [((n0 * V[a0, a] + n1 * V[a1, a]) + n2 * V[a2, a]) / F(2 * s) for a in range(3)]
                g = [((n0 * F(M[a0, a]) + n1 * F(M[a1, a])) + n2 * F(M[a2, a])) / F(2 * s) for a in range(3)]
                l2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]
                if np.isfinite(l2) and l2 > 0:
                    l = np.sqrt(l2)
                    n = [g[0] / l, g[1] / l, g[2] / l]
                else:
                    n = [F(0.0)] * 3
                image[y, x], views[y, x] = blend_one(pt, n, proj, centres, depth, keep, images, tol, min_cos, fill, ch)
    uv = np.zeros((nt, 3, 2), np.float32)
    for t in range(nt):
        c = t >> 1
        x0, y0 = (c % cpr) * P, (c // cpr) * P
        for k, (i, j) in enumerate(((0, 0), (s, 0), (0, s))):
            x, y = (x0 + P - 1 - i, y0 + P - 1 - j) if t & 1 else (x0 + i, y0 + j)
            uv[t, k] = np.float32((F(x) + 0.5) / F(W)), np.float32((F(y) + 0.5) / F(H))
    return (image[:, :, 0] if ch == 1 else image), views, uv


def assert_same(got, want, what=""):
    """image and views byte for byte, uv as float32 bits."""
    for name, g, w in zip(("image", "views", "uv"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        g, w = (g.view(np.uint32), w.view(np.uint32)) if name == "uv" else (g, w)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())


# ------------------------------------------------------------------------------------------- scenes
class Scene:
    """A `mesh_color_reference.Scene` and triangles over its vertices; `args()` is what both restatements and
    `sfm_amd.mesh_texture` take in front of texels."""

    def __init__(self, scene, triangles):
        self.s, self.triangles = scene, np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
        self.channels, self.tol, self.min_cos, self.fill = scene.channels, scene.tol, scene.min_cos, scene.fill

    def args(self):
        s = self.s
        return (s.vertices, s.normals, self.triangles, s.proj, s.centres, s.depth, s.keep, s.images, s.tol)

    def kwargs(self, texels, cells_per_row=None):
        return dict(texels=texels, min_cos=self.min_cos, fill=self.fill, cells_per_row=cells_per_row)


def random_scene(seed, n_vertices, n_triangles, sizes, channels, with_keep=True, bad=()):
    """`mesh_color_reference.random_scene` (views with depths that are not finite and keep = 0, vertices with NaN and zero
    normals) with random triangles over its vertices; bad: (triangle, corner, index) to overwrite."""
    s = cr.random_scene(seed, n_vertices, sizes, channels, with_keep)
    rng = np.random.default_rng(seed + 1000)
    T = rng.integers(0, max(n_vertices, 1), (n_triangles, 3)).astype(np.int32)
    for t, k, value in bad:
        T[t, k] = value
    return Scene(s, T)


def reference(scene, texels, cells_per_row=None):
    return texture(*scene.args(), channels=scene.channels, **scene.kwargs(texels, cells_per_row))


def bilinear_taps(uv, W, H):
    """The four taps of a bilinear lookup at uv [n,2] in an atlas whose texel (x, y) has its centre at ((x + 0.5) / W,
    (y + 0.5) / H): (x int64 [n,4], y int64 [n,4], weight float64 [n,4])."""
    px, py = uv[:, 0].astype(np.float64) * W - 0.5, uv[:, 1].astype(np.float64) * H - 0.5
    x0, y0 = np.floor(px), np.floor(py)
    fx, fy = px - x0, py - y0
    x = np.stack([x0, x0 + 1, x0, x0 + 1], axis=1).astype(np.int64)
    y = np.stack([y0, y0, y0 + 1, y0 + 1], axis=1).astype(np.int64)
    return x, y, np.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], axis=1)


# ------------------------------------------------------------------------------------------- the textured sphere
def fine_texture(X, w):
    """float64 [..., 3]: 127.5 + 100 sin(w X_k) per channel."""
    return 127.5 + 100.0 * np.sin(w * np.asarray(X, dtype=np.float64))


def textured_sphere_scene(size, f, w, n_cams=14):
    """`mesh_color_reference.colour_sphere_scene` at size x size pixels with the texture 127.5 + 100 sin(w X_k):
    (proj, depth, origin, voxel, shape, trunc, centres, images)."""
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
        images.append(np.where(hit[..., None], np.floor(fine_texture(X, w) + 0.5), 0.0).astype(np.uint8))
        centres.append(C)
    return proj, depth, origin, voxel, shape, trunc, np.array(centres), images


def error_summary(err):
    return float(np.median(err)), float(np.percentile(err, 95)), float(err.max())


def sphere_worth(size, f, w, texels):
    """The atlas against the vertex colours interpolated across the triangles, on the textured sphere: the absolute error in
    grey levels against the texture at the radial foot point over the interior texels (i + j <= s) of every triangle.
    Returns dict(texels=count, unseen=count, atlas=(median, p95, max), interpolated=(median, p95, max), rms=(atlas, interpolated))."""
    proj, depth, origin, voxel, shape, trunc, centres, images = textured_sphere_scene(size, f, w)
    tsdf, weight = mr.integrate(proj, depth, None, origin, voxel, shape, trunc)
    m = mr.mesh(tsdf, weight, origin, voxel, shape, 1)
    T = np.asarray(m.triangles, dtype=np.int64)
    nt, cpr = len(T), default_cells_per_row(len(T))
    image, views, uv = texture(m.vertices, m.normals, T, proj, centres, depth, None, images, trunc, texels, 0.35, 0, cpr)
    tri, i, j = inverse_map(nt, texels, cpr)
    inner = (tri >= 0) & (i + j <= texels)
    good, X, normal = points_of(tri, i, j, m.vertices, m.normals, T, texels)
    assert good[inner].all()
    X = X[inner]
    truth = fine_texture(X / np.linalg.norm(X, axis=1, keepdims=True), w)
    vcol = cr.colors(m.vertices, m.normals, proj, centres, depth, None, images, trunc, 0.35, 0)[0].astype(np.float64)
    n0, n1, n2 = (n.astype(np.float64)[inner][:, None] for n in numerators(i, j, texels))
    idx = T[tri[inner]]
    lerp = interpolate(n0, n1, n2, vcol[idx[:, 0]], vcol[idx[:, 1]], vcol[idx[:, 2]], texels)
    e_atlas, e_lerp = np.abs(image[inner].astype(np.float64) - truth), np.abs(lerp - truth)
    return dict(texels=int(inner.sum()), triangles=nt, unseen=int((views[inner] == 0).sum()), atlas=error_summary(e_atlas),
                interpolated=error_summary(e_lerp), rms=(float(np.sqrt((e_atlas ** 2).mean())), float(np.sqrt((e_lerp ** 2).mean()))))
