"""NumPy restatement of the render score (include/sfm_amd.h, "score of a render against the photographs"): `score_view` in
array operations, `score_view_loops` in plain Python loops for tiny inputs, the figures the host forms from the integer
table, the cases the tests share and the worth of the score on the textured sphere.  Every statistic is an integer sum; the
two quotients are float64, which NumPy and Python evaluate one operation at a time."""
import math

import numpy as np

COLUMNS = 16
(N_PIXELS, N_COMPARED, SAD, SSE, N_SSIM, Q_SSIM, N_BOTH, N_AGREE, Q_REL, N_RENDER_ONLY, N_VIEW_ONLY) = (0, 1, 2, 5, 8, 9, 10, 11, 12, 13, 14)
Q = 16777216.0
NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def box(a, W):
    """The sums of `a` (int64 [h,w]) over every W x W window inside it: [h - W + 1, w - W + 1]; needs h, w >= W."""
    h, w = a.shape
    c = np.zeros((h + 1, w + 1), np.int64)
    c[1:, 1:] = a.cumsum(0).cumsum(1)
    return c[W:, W:] - c[:-W, W:] - c[W:, :-W] + c[:-W, :-W]


def ssim_channel(n, Sx, Sy, Sxx, Syy, Sxy):
    a = 2 * Sx * Sy
    b = Sx * Sx + Sy * Sy
    cv = 2 * (n * Sxy - Sx * Sy)
    vr = (n * Sxx - Sx * Sx) + (n * Syy - Sy * Sy)
    c1 = np.float64(n * n) * 6.5025
    c2 = np.float64(n * n) * 58.5225
    return ((a.astype(np.float64) + c1) * (cv.astype(np.float64) + c2)) / ((b.astype(np.float64) + c1) * (vr.astype(np.float64) + c2))


def quantise(v):
    return np.floor(v * Q + 0.5).astype(np.int64)


def score_view(color, triangle, depth, photo, mask=None, view_depth=None, view_keep=None, window=7, rel_tol=0.02):
    """One view: (stats int64 [16], abs_error uint8 shaped like color, ssim_map float32 [h,w])."""
    color, photo = np.asarray(color), np.asarray(photo)
    assert color.dtype == np.uint8 and photo.dtype == np.uint8 and color.shape == photo.shape
    h, w = color.shape[:2]
    ch = 1 if color.ndim == 2 else 3
    W, r = int(window), int(window) // 2
    x = color.reshape(h, w, ch).astype(np.int64)
    y = photo.reshape(h, w, ch).astype(np.int64)
    covered = np.asarray(triangle).reshape(h, w) >= 0
    compared = covered if mask is None else covered & (np.asarray(mask).reshape(h, w) > 0)
    stats = np.zeros(COLUMNS, np.int64)
    stats[N_PIXELS], stats[N_COMPARED] = h * w, int(compared.sum())
    e = np.where(compared[..., None], np.abs(x - y), 0)
    stats[SAD:SAD + ch] = e.sum((0, 1))
    stats[SSE:SSE + ch] = (e * e).sum((0, 1))
    abs_error = e.astype(np.uint8).reshape(color.shape)
    ssim_map = np.full((h, w), NAN32, np.float32)
    if h >= W and w >= W:
        n = W * W
        has = box(compared.astype(np.int64), W) == n
        s_k = [ssim_channel(n, box(x[..., k], W), box(y[..., k], W), box(x[..., k] * x[..., k], W), box(y[..., k] * y[..., k], W),
                            box(x[..., k] * y[..., k], W)) for k in range(ch)]
        s = s_k[0] if ch == 1 else ((s_k[0] + s_k[1]) + s_k[2]) / 3.0
        inner = ssim_map[r:h - r, r:w - r]
        inner[has] = s[has].astype(np.float32)
        stats[N_SSIM] = int(has.sum())
        stats[Q_SSIM] = int(quantise(s[has]).sum())
    if view_depth is not None:
        dv32 = np.asarray(view_depth, dtype=np.float32).reshape(h, w)
        dv = dv32.astype(np.float64)
        dr = np.asarray(depth, dtype=np.float32).reshape(h, w).astype(np.float64)
        seen = (np.asarray(view_keep).reshape(h, w) != 0) & np.isfinite(dv)
        both = covered & seen
        with np.errstate(all="ignore"):
            rr = np.abs(dr - dv)
            known = both & ~np.isnan(rr)
            agree = known & (rr <= rel_tol * dv)
            t = np.where(dv > 0.0, np.minimum(rr / dv, 1.0), np.where(rr == 0.0, 0.0, 1.0))
        stats[N_BOTH], stats[N_AGREE] = int(both.sum()), int(agree.sum())
        stats[Q_REL] = int(quantise(t[known]).sum())
        stats[N_RENDER_ONLY], stats[N_VIEW_ONLY] = int((covered & ~seen).sum()), int((seen & ~covered).sum())
    return stats, abs_error, ssim_map


def score_view_loops(color, triangle, depth, photo, mask=None, view_depth=None, view_keep=None, window=7, rel_tol=0.02):
    """`score_view` pixel by pixel with Python's integers and floats: for tiny inputs."""
    color, photo = np.asarray(color), np.asarray(photo)
    h, w = color.shape[:2]
    ch = 1 if color.ndim == 2 else 3
    W, r = int(window), int(window) // 2
    n = W * W
    X, Y = color.reshape(h, w, ch).tolist(), photo.reshape(h, w, ch).tolist()
    tri = np.asarray(triangle).reshape(h, w).tolist()
    msk = None if mask is None else np.asarray(mask).reshape(h, w).tolist()
    covered = [[tri[i][j] >= 0 for j in range(w)] for i in range(h)]
    compared = [[covered[i][j] and (msk is None or msk[i][j] > 0) for j in range(w)] for i in range(h)]
    stats = [0] * COLUMNS
    stats[N_PIXELS] = h * w
    abs_error = np.zeros((h, w, ch), np.uint8)
    ssim_map = np.full((h, w), NAN32, np.float32)
    c1, c2 = float(n * n) * 6.5025, float(n * n) * 58.5225
    for i in range(h):
        for j in range(w):
            if compared[i][j]:
                stats[N_COMPARED] += 1
                for k in range(ch):
                    e = abs(X[i][j][k] - Y[i][j][k])
                    stats[SAD + k] += e
                    stats[SSE + k] += e * e
                    abs_error[i, j, k] = e
            if i - r < 0 or i + r >= h or j - r < 0 or j + r >= w:
                continue
            cells = [(a, b) for a in range(i - r, i + r + 1) for b in range(j - r, j + r + 1)]
            if not all(compared[a][b] for a, b in cells):
                continue
            s_k = []
            for k in range(ch):
                Sx = sum(X[a][b][k] for a, b in cells)
                Sy = sum(Y[a][b][k] for a, b in cells)
                Sxx = sum(X[a][b][k] ** 2 for a, b in cells)
                Syy = sum(Y[a][b][k] ** 2 for a, b in cells)
                Sxy = sum(X[a][b][k] * Y[a][b][k] for a, b in cells)
                a_, b_ = 2 * Sx * Sy, Sx * Sx + Sy * Sy
                cv, vr = 2 * (n * Sxy - Sx * Sy), (n * Sxx - Sx * Sx) + (n * Syy - Sy * Sy)
                s_k.append(((float(a_) + c1) * (float(cv) + c2)) / ((float(b_) + c1) * (float(vr) + c2)))
            s = s_k[0] if ch == 1 else ((s_k[0] + s_k[1]) + s_k[2]) / 3.0
            ssim_map[i, j] = np.float32(s)
            stats[N_SSIM] += 1
            stats[Q_SSIM] += math.floor(s * Q + 0.5)
    if view_depth is not None:
        dv_all = np.asarray(view_depth, dtype=np.float32).reshape(h, w).astype(np.float64).tolist()
        dr_all = np.asarray(depth, dtype=np.float32).reshape(h, w).astype(np.float64).tolist()
        keep = np.asarray(view_keep).reshape(h, w).tolist()
        for i in range(h):
            for j in range(w):
                dv, dr = dv_all[i][j], dr_all[i][j]
                seen = keep[i][j] != 0 and math.isfinite(dv)
                if covered[i][j] and not seen:
                    stats[N_RENDER_ONLY] += 1
                if seen and not covered[i][j]:
                    stats[N_VIEW_ONLY] += 1
                if not (covered[i][j] and seen):
                    continue
                stats[N_BOTH] += 1
                rr = abs(dr - dv)
                if math.isnan(rr):
                    continue
                if rr <= rel_tol * dv:
                    stats[N_AGREE] += 1
                if dv > 0.0:
                    t = min(rr / dv, 1.0) if not math.isinf(rr) else 1.0
                else:
                    t = 0.0 if rr == 0.0 else 1.0
                stats[Q_REL] += math.floor(t * Q + 0.5)
    return np.array(stats, np.int64), abs_error.reshape(color.shape), ssim_map


class Score:
    """stats int64 [n,16], abs_error and ssim_map as lists per view."""

    def __init__(self, stats, abs_error, ssim_map, channels):
        self.stats, self.abs_error, self.ssim_map, self.channels = stats, abs_error, ssim_map, channels


def opt(arrays, v):
    return None if arrays is None else arrays[v]


def score(colors, triangles, depths, photos, masks=None, view_depths=None, view_keeps=None, window=7, rel_tol=0.02, fn=score_view):
    out = [fn(colors[v], triangles[v], depths[v], photos[v], opt(masks, v), opt(view_depths, v), opt(view_keeps, v), window, rel_tol)
           for v in range(len(colors))]
    ch = 3 if (len(colors) and np.asarray(colors[0]).ndim == 3) else 1
    stats = np.array([o[0] for o in out], np.int64).reshape(-1, COLUMNS)
    return Score(stats, [o[1] for o in out], [o[2] for o in out], ch)


def figures(stats, channels):
    """What the host forms from one row of the table, or from the sum of several: dict(n_compared, mae [c], mse [c], psnr, ssim,
    n_ssim, depth_both, depth_agree, depth_rel, render_only, view_only); a mean over nothing is NaN."""
    s = [int(v) for v in np.asarray(stats).reshape(-1, COLUMNS).sum(0)]
    n = s[N_COMPARED]
    div = lambda a, b: a / b if b else float("nan")
    sse = sum(s[SSE:SSE + channels])
    if n == 0:
        psnr = float("nan")
    elif sse == 0:
        psnr = float("inf")
    else:
        psnr = 10.0 * math.log10(65025.0 * n * channels / sse)
    return dict(n_compared=n, mae=[div(s[SAD + k], n) for k in range(channels)], mse=[div(s[SSE + k], n) for k in range(channels)], psnr=psnr,
                ssim=div(s[Q_SSIM], Q * s[N_SSIM]), n_ssim=s[N_SSIM], depth_both=s[N_BOTH], depth_agree=div(s[N_AGREE], s[N_BOTH]),
                depth_rel=div(s[Q_REL], Q * s[N_BOTH]), render_only=s[N_RENDER_ONLY], view_only=s[N_VIEW_ONLY])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what=""):
    """Every output byte: the table, the error maps, the SSIM maps as float32 bits (the NaN is the quiet NaN 0x7FC00000)."""
    gs, ws = np.asarray(got.stats), np.asarray(want.stats)
    assert gs.dtype == np.int64 and gs.shape == ws.shape, (what, gs.dtype, gs.shape, ws.shape)
    assert np.array_equal(gs, ws), (what, "stats", gs.tolist(), ws.tolist())
    assert len(got.abs_error) == len(want.abs_error) and len(got.ssim_map) == len(want.ssim_map), what
    for v, (g, w) in enumerate(zip(got.abs_error, want.abs_error)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), (what, "abs_error", v)
    for v, (g, w) in enumerate(zip(got.ssim_map, want.ssim_map)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == np.float32 and g.shape == w.shape and np.array_equal(bits(g), bits(w)), (what, "ssim_map", v, int((bits(g) != bits(w)).sum()))


# ------------------------------------------------------------------------------------------- cases
PATTERNS = ("all", "none", "checker", "middle", "corner", "random")


def coverage(pattern, h, w, rng, tile=(32, 8)):
    """triangle int32 [h,w]: -1 where the pattern leaves a pixel uncovered.  `middle` drops one pixel in the middle of the
    first tile, `corner` the pixel on the far corner of the first tile (or of the image, if that is smaller)."""
    t = rng.integers(0, 1000, (h, w)).astype(np.int32)
    if pattern == "none":
        t[:] = -1
    elif pattern == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        t[(yy + xx) % 2 == 1] = -1
    elif pattern == "middle" and h and w:
        t[min(tile[1] // 2, h - 1), min(tile[0] // 2, w - 1)] = -1
    elif pattern == "corner" and h and w:
        t[min(tile[1] - 1, h - 1), min(tile[0] - 1, w - 1)] = -1
    elif pattern == "random":
        t[rng.random((h, w)) >= 0.9] = -1
    return t


class Case:
    """One view's inputs; args() in the order of `score_view`."""

    def __init__(self, color, triangle, depth, photo, mask=None, view_depth=None, view_keep=None):
        self.color, self.triangle, self.depth, self.photo, self.mask, self.view_depth, self.view_keep = color, triangle, depth, photo, mask, view_depth, view_keep

    def args(self):
        return self.color, self.triangle, self.depth, self.photo, self.mask, self.view_depth, self.view_keep


def random_case(seed, h, w, channels, pattern="random", mask=False, with_depth=True, tile=(32, 8)):
    """A smooth render, a photograph that is the render plus noise (so that SSIM takes values over its range), depths that sit
    on both sides of the threshold, NaN and non-positive depths, keep flags that drop a tenth."""
    rng = np.random.default_rng(seed)
    shape = (h, w) if channels == 1 else (h, w, 3)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 90 * np.sin(0.37 * xx + 0.21 * yy)
    base = base if channels == 1 else np.stack([base, 255 - base, 0.5 * base + 40], axis=-1)
    color = np.clip(base + rng.normal(0, 12, shape), 0, 255).astype(np.uint8)
    photo = np.clip(color.astype(np.float64) * rng.choice([1.0, 0.7, -1.0], 1)[0] % 256 + rng.normal(0, rng.choice([0.0, 3.0, 25.0]), shape), 0, 255).astype(np.uint8)
    tri = coverage(pattern, h, w, rng, tile)
    depth = np.where(tri >= 0, rng.uniform(1.0, 4.0, (h, w)), np.nan).astype(np.float32)
    m = (rng.random((h, w)) < 0.98).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8) if mask else None
    vd = vk = None
    if with_depth:
        rel = rng.choice([0.0, 0.01, 0.02, 0.03, 0.5, 3.0], (h, w))
        vd = (np.where(tri >= 0, depth, 2.0) / (1.0 + rel * rng.choice([-1.0, 1.0], (h, w)).clip(-0.3, 1))).astype(np.float32)
        kind = rng.random((h, w))
        vd[kind < 0.08] = np.nan
        vd[(kind >= 0.08) & (kind < 0.11)] = 0.0
        vd[(kind >= 0.11) & (kind < 0.14)] = -1.5
        vd[(kind >= 0.14) & (kind < 0.16)] = np.inf
        vk = (rng.random((h, w)) < 0.9).astype(np.uint8) * rng.integers(1, 256, (h, w)).astype(np.uint8)
    return Case(color, tri, depth, photo, m, vd, vk)


# ------------------------------------------------------------------------------------------- the textured sphere
def sphere_renders(size=128, f=180.0, w=24.0, texels=6):
    """The mesh of the textured sphere (`mesh_texture_reference.textured_sphere_scene`) through the restatements, drawn through
    its own 14 cameras with the atlas and with the vertex colours: (atlas render, vertex-colour render, images, depth)."""
    import mesh_color_reference as cr
    import mesh_reference as mr
    import mesh_render_reference as rr
    import mesh_texture_reference as tr
    proj, depth, origin, voxel, shape, trunc, centres, images = tr.textured_sphere_scene(size, f, w)
    tsdf, weight = mr.integrate(proj, depth, None, origin, voxel, shape, trunc)
    m = mr.mesh(tsdf, weight, origin, voxel, shape, 1)
    T = np.asarray(m.triangles, dtype=np.int64)
    cpr = tr.default_cells_per_row(len(T))
    atlas, views, uv = tr.texture(m.vertices, m.normals, T, proj, centres, depth, None, images, trunc, texels, 0.35, 0, cpr)
    vcol = cr.colors(m.vertices, m.normals, proj, centres, depth, None, images, trunc, 0.35, 0)[0]
    sizes = [(size, size)] * len(proj)
    ra = rr.render(m.vertices, T, proj, sizes, uv=uv, atlas=atlas)
    rv = rr.render(m.vertices, T, proj, sizes, vertex_colors=vcol)
    return ra, rv, images, depth


def worth_of(ra, rv, images, depth, score_fn):
    """score_fn(render, photos, view_depths or None) -> stats [n,16].  dict(atlas=figures, vertex=figures, per_view=[figures],
    own=[ssim per view against its photograph], next=[against the photograph of the next view], covered=(min, max),
    finite=(min, max), agree=(min, max) share of the pixels with both depths within 1 %)."""
    n = len(images)
    sa = score_fn(ra, images, depth)
    sv = score_fn(rv, images, depth)
    nxt = score_fn(ra, [images[(v + 1) % n] for v in range(n)], None)
    one = score_fn(ra, images, depth, 0.01)
    covered = [int((t >= 0).sum()) for t in ra.triangle]
    finite = [int(np.isfinite(d).sum()) for d in depth]
    share = [one[v, N_AGREE] / one[v, N_BOTH] for v in range(n)]
    return dict(atlas=figures(sa, 3), vertex=figures(sv, 3), per_view=[figures(sa[v], 3) for v in range(n)],
                own=[figures(sa[v], 3)["ssim"] for v in range(n)], next=[figures(nxt[v], 3)["ssim"] for v in range(n)],
                covered=(min(covered), max(covered)), finite=(min(finite), max(finite)), agree=(min(share), max(share)))


def reference_score_fn(render, photos, view_depths, rel_tol=0.02):
    keeps = None if view_depths is None else [np.ones(d.shape, np.uint8) for d in view_depths]
    return score(render.color, render.triangle, render.depth, photos, None, view_depths, keeps, 7, rel_tol).stats


# measured with this restatement on textured_sphere_scene(128, 180, 24) at texels 6, 14 views, three channels, window 7,
# pooled over the views: (MAE in grey levels over the channels, PSNR in dB, SSIM)
ATLAS_MEASURED = (12.233, 18.364, 0.9748)
VERTEX_MEASURED = (16.510, 18.023, 0.9497)


def assert_worth(r):
    mean = lambda v: sum(v) / len(v)
    a, v = r["atlas"], r["vertex"]
    assert mean(a["mae"]) <= ATLAS_MEASURED[0] + 0.5, a
    assert a["ssim"] >= ATLAS_MEASURED[2] - 0.005, a
    assert mean(a["mae"]) < mean(v["mae"]) and a["psnr"] > v["psnr"] and a["ssim"] > v["ssim"], (a, v)
    for k, (own, other) in enumerate(zip(r["own"], r["next"])):
        assert own > other, (k, own, other)
