"""NumPy restatement of the dense-depth stage (include/sfm_amd.h, "dense depth maps"): census, sweep, filter and
back-projection, vectorised, every floating-point operation in the order the header states it (float64, no FMA: NumPy has
none).  The device must equal it bit for bit.  Also the synthetic scene the quality figures are measured on."""
import numpy as np

ABSENT_COST = 24
OFFSETS = [(dy, dx) for dy in range(-3, 4) for dx in range(-3, 4) if (dy, dx) != (0, 0)]


def census(img):
    """[h,w] uint64: bit k = I(clamp(p + o_k)) < I(p) over the 48 offsets."""
    I = np.asarray(img).astype(np.int32)
    h, w = I.shape
    ys, xs = np.arange(h), np.arange(w)
    out = np.zeros((h, w), dtype=np.uint64)
    for k, (dy, dx) in enumerate(OFFSETS):
        nb = I[np.clip(ys + dy, 0, h - 1)][:, np.clip(xs + dx, 0, w - 1)]
        out |= (nb < I).astype(np.uint64) << np.uint64(k)
    return out


def popcount(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=-1).astype(np.int32)


def sample(W, x, y, d, ws, hs):
    """The sample rule on arrays: (valid, xi, yi, q2); xi / yi are 0 where the sample is not valid."""
    W = np.asarray(W, dtype=np.float64).reshape(12)
    x, y, d = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(d, dtype=np.float64)
    with np.errstate(all="ignore"):
        a0 = (W[0] * x + W[1] * y) + W[2]
        a1 = (W[4] * x + W[5] * y) + W[6]
        a2 = (W[8] * x + W[9] * y) + W[10]
        q0 = d * a0 + W[3]
        q1 = d * a1 + W[7]
        q2 = d * a2 + W[11]
        u, v = q0 / q2, q1 / q2
        valid = (q2 > 0) & (u >= -0.5) & (u < float(ws) - 0.5) & (v >= -0.5) & (v < float(hs) - 0.5)
        xi = np.where(valid, np.minimum(np.floor(np.where(valid, u, 0.0) + 0.5), ws - 1), 0).astype(np.int64)
        yi = np.where(valid, np.minimum(np.floor(np.where(valid, v, 0.0) + 0.5), hs - 1), 0).astype(np.int64)
    return valid, xi, yi, q2


def plane_costs(cen_ref, sources, d):
    """c_k [h,w] int32 of one plane: sources is a list of (census of the source, warp)."""
    h, w = cen_ref.shape
    y, x = np.mgrid[0:h, 0:w]
    c = np.zeros((h, w), dtype=np.int32)
    for cen_s, W in sources:
        hs, ws = cen_s.shape
        if hs == 0 or ws == 0:
            c += ABSENT_COST
            continue
        valid, xi, yi, _ = sample(W, x, y, d, ws, hs)
        c += np.where(valid, popcount(cen_ref ^ cen_s[yi, xi]), ABSENT_COST).astype(np.int32)
    return c


def box_sum(c, r):
    h, w = c.shape
    cp = np.pad(c, r, mode="edge")
    S = np.zeros((h, w), dtype=np.int32)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            S += cp[dy:dy + h, dx:dx + w]
    return S


def refine(best, S, planes):
    """depth float32 [h,w] of the winners: the sub-plane step where it applies, the plane's depth elsewhere."""
    D = len(planes)
    planes = np.asarray(planes, dtype=np.float64)
    Sl = S.astype(np.int64)
    take = lambda k: np.take_along_axis(Sl, np.clip(k, 0, D - 1)[None], axis=0)[0]
    sm, s0, sp = take(best - 1), take(best), take(best + 1)
    den = sm - 2 * s0 + sp
    ok = (best > 0) & (best < D - 1) & (den > 0)
    with np.errstate(all="ignore"):
        off = (sm - sp).astype(np.float64) / (2 * np.where(ok, den, 1)).astype(np.float64)
        j = np.clip(np.where(off >= 0, best + 1, best - 1), 0, D - 1)
        f = np.abs(off)
        w0 = 1.0 / planes[best]
        wv = w0 + f * (1.0 / planes[j] - w0)
        return np.where(ok, (1.0 / wv).astype(np.float32), planes[best].astype(np.float32))


def sweep_view(cen_ref, sources, planes, r, want_volume=False):
    """(plane int32, cost uint16, depth float32) of one reference view."""
    S = np.stack([box_sum(plane_costs(cen_ref, sources, d), r) for d in np.asarray(planes, dtype=np.float64)])
    best = np.argmin(S, axis=0).astype(np.int32)                  # the first minimum: the lowest k
    cost = np.take_along_axis(S, best[None].astype(np.int64), axis=0)[0].astype(np.uint16)
    out = (best, cost, refine(best.astype(np.int64), S, planes))
    return out + (S,) if want_volume else out


def sweep(images, refs, sources, warps, planes, r):
    """The batch: images (all of the set), refs (reference image per view), sources / warps (per view a list of images and
    an [n,12] array), planes (per view).  Returns one (plane, cost, depth) per view."""
    cen = [census(a) if a.size else np.zeros(a.shape, np.uint64) for a in images]
    return [sweep_view(cen[ref], [(cen[s], W) for s, W in zip(sources[v], np.asarray(warps[v]).reshape(-1, 12))], planes[v], r)
            for v, ref in enumerate(refs)]


def filter_views(images, refs, sources, warps, backproj, maps, rel_tol, max_cost, min_consistent):
    """Per view (n_consistent uint8, keep uint8, xyz float64 [h,w,3]).  maps: per view (plane, cost, depth); max_cost: None
    or one int per view."""
    view_of = {ref: v for v, ref in enumerate(refs)}
    out = []
    for v, ref in enumerate(refs):
        h, w = images[ref].shape
        y, x = np.mgrid[0:h, 0:w]
        d = maps[v][2].astype(np.float64)
        finite = np.isfinite(d)
        n = np.zeros((h, w), dtype=np.int32)
        for s, W in zip(sources[v], np.asarray(warps[v]).reshape(-1, 12)):
            if s not in view_of:
                continue
            hs, ws = images[s].shape
            if hs == 0 or ws == 0:
                continue
            valid, xi, yi, q2 = sample(W, x, y, d, ws, hs)
            ds = maps[view_of[s]][2].astype(np.float64)[yi, xi]
            with np.errstate(all="ignore"):
                n += (finite & valid & np.isfinite(ds) & (np.abs(ds - q2) <= rel_tol * q2)).astype(np.int32)
        cost_ok = np.ones((h, w), bool) if max_cost is None else maps[v][1].astype(np.int64) <= int(max_cost[v])
        keep = (finite & cost_ok & (n >= min_consistent)).astype(np.uint8)
        M = np.asarray(backproj[v], dtype=np.float64).reshape(3, 4)
        xf, yf = x.astype(np.float64), y.astype(np.float64)
        with np.errstate(all="ignore"):
            xyz = np.stack([d * ((M[i, 0] * xf + M[i, 1] * yf) + M[i, 2]) + M[i, 3] for i in range(3)], axis=-1)
        xyz[~finite] = np.nan
        out.append((n.astype(np.uint8), keep, xyz))
    return out


# ------------------------------------------------------------------------------------------------------------ the scene
class Scene:
    pass


def _texture(rng, n):
    """[n,n] float64 in 0 .. 1: white noise smoothed by two 3 x 3 box passes, stretched to the full range."""
    t = rng.random((n, n))
    for _ in range(2):
        p = np.pad(t, 1, mode="wrap")
        t = sum(p[dy:dy + n, dx:dx + n] for dy in range(3) for dx in range(3)) / 9.0
    return (t - t.min()) / (t.max() - t.min())


def _lookup(tex, X, Y, cell):
    """Bilinear lookup of the periodic texture at world (X, Y), one texel per `cell` world units."""
    n = tex.shape[0]
    gx, gy = X / cell, Y / cell
    x0, y0 = np.floor(gx).astype(np.int64), np.floor(gy).astype(np.int64)
    fx, fy = gx - x0, gy - y0
    t = lambda yy, xx: tex[yy % n, xx % n]
    return (t(y0, x0) * (1 - fx) + t(y0, x0 + 1) * fx) * (1 - fy) + (t(y0 + 1, x0) * (1 - fx) + t(y0 + 1, x0 + 1) * fx) * fy


def make_scene(n_cams=3, width=96, height=72, f=100.0, baseline=0.8, z_front=3.2, z_back=4.0, d_min=2.5, d_max=5.0, seed=0):
    """Pinhole cameras on a line along x, all looking down +z at a textured back plane z = z_back with a raised textured
    rectangle z = z_front in front of it, ray-cast analytically to uint8.  Returns a Scene with images, K, poses
    {i: (R, t)}, depth (true depth per pixel and camera), d_min / d_max."""
    rng = np.random.default_rng(seed)
    s = Scene()
    s.K = np.array([[f, 0, (width - 1) / 2.0], [0, f, (height - 1) / 2.0], [0, 0, 1.0]])
    s.size, s.d_min, s.d_max, s.z_front, s.z_back = (width, height), d_min, d_max, z_front, z_back
    tex_back, tex_front = _texture(rng, 256), _texture(rng, 256)
    cell = 0.6 * z_front / f                                     # a texel is a little smaller than a pixel's footprint
    half_w, half_h = 0.3 * width * z_back / f * 0.5, 0.3 * height * z_back / f * 0.5      # the rectangle, centred
    s.rect = (-half_w, half_w, -half_h, half_h)
    y, x = np.mgrid[0:height, 0:width].astype(np.float64)
    s.images, s.depth, s.poses = [], [], {}
    for i in range(n_cams):
        cx = baseline * (i - (n_cams - 1) / 2.0)
        s.poses[i] = (np.eye(3), np.array([-cx, 0.0, 0.0]))
        dx, dy = (x - s.K[0, 2]) / f, (y - s.K[1, 2]) / f
        Xf, Yf = cx + z_front * dx, z_front * dy
        hit = (Xf >= -half_w) & (Xf <= half_w) & (Yf >= -half_h) & (Yf <= half_h)
        Xb, Yb = cx + z_back * dx, z_back * dy
        val = np.where(hit, _lookup(tex_front, Xf + 7.0, Yf + 3.0, cell), _lookup(tex_back, Xb, Yb, cell * z_back / z_front))
        s.images.append(np.clip(np.rint(val * 255.0), 0, 255).astype(np.uint8))
        s.depth.append(np.where(hit, z_front, z_back))
    return s


_DEFAULT = {}


def default_scene():
    """The default scene, built once and shared (treat it as read-only)."""
    if "s" not in _DEFAULT:
        _DEFAULT["s"] = make_scene()
    return _DEFAULT["s"]
