"""Dense depth maps by plane-sweep stereo on the device (`sfm_depth_census` / `sfm_depth_sweep` / `sfm_depth_filter`,
sfm_amd/csrc/depth.hip; include/sfm_amd.h states the rule completely): per reference view a census transform, a sweep over
fronto-parallel planes with winner-take-all and a sub-plane step, then a cross-view consistency filter that also
back-projects every pixel.  The planes are chosen here (`plane_depths`): the rule works only when adjacent planes move a
pixel by about one pixel in the source images.  No CPU fallback: without the library or a GPU the calls raise.
"""
from __future__ import annotations

import ctypes as C
from numbers import Real

import numpy as np

from . import _lib

MAX_SOURCES, MAX_RADIUS, MAX_PLANES = 8, 4, 1024
MAX_NORMAL_STEP = 4


def _K_of(K, image):
    K = K[image] if isinstance(K, (dict, list, tuple)) else K
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("K must be 3 x 3 (or one 3 x 3 per image)")
    return K


def _pose_of(poses, image):
    try:
        R, t = poses[image]
    except (KeyError, IndexError, TypeError):
        raise ValueError(f"image {image} has no pose") from None
    R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64).reshape(-1)
    if R.shape != (3, 3) or t.shape != (3,):
        raise ValueError(f"pose of image {image}: R must be 3 x 3 and t have 3 elements")
    return R, t


def view_warps(K, poses, ref, sources):
    """[len(sources), 12] float64: per source the row-major [A | b] with A = K_s R_s R_r^T K_r^-1 and
    b = K_s (t_s - R_s R_r^T t_r), so that [A | b] applied to d * (x, y, 1) is the source's K_s (R_s X + t_s) of the point
    at depth d behind reference pixel (x, y).  poses: {image: (R, t)} with x_cam = R X + t; K: one matrix or one per image."""
    Rr, tr = _pose_of(poses, ref)
    Kr_inv = np.linalg.inv(_K_of(K, ref))
    out = np.zeros((len(sources), 12))
    for k, s in enumerate(sources):
        Rs, ts = _pose_of(poses, s)
        Ks = _K_of(K, s)
        Rrel = Rs @ Rr.T
        out[k] = np.c_[Ks @ Rrel @ Kr_inv, Ks @ (ts - Rrel @ tr)].reshape(12)
    return out


def view_backprojection(K, poses, ref):
    """[12] float64: the row-major [M | c], M = R_r^T K_r^-1, c = -R_r^T t_r: X = d * M (x, y, 1) + c."""
    Rr, tr = _pose_of(poses, ref)
    return np.c_[Rr.T @ np.linalg.inv(_K_of(K, ref)), -Rr.T @ tr].reshape(12)


def _corner_tracks(inv_depths, warps, size):
    """[n_warps * 4, n_planes, 2]: where the four image corners land in every source at every plane (NaN behind it)."""
    w, h = size
    corners = np.array([[0.0, 0.0], [w - 1.0, 0.0], [0.0, h - 1.0], [w - 1.0, h - 1.0]])
    W = np.asarray(warps, dtype=np.float64).reshape(-1, 3, 4)
    ray = np.einsum("sij,cj->sci", W[:, :, :3], np.c_[corners, np.ones(4)])             # [s, c, 3]
    with np.errstate(all="ignore"):
        q = ray[:, :, None, :] / inv_depths[None, None, :, None] + W[:, None, None, :, 3]
        uv = q[..., :2] / np.where(q[..., 2:] > 0, q[..., 2:], np.nan)
    return uv.reshape(-1, len(inv_depths), 2)


def plane_depths(d_min, d_max, warps, size, max_planes=256):
    """Plane depths for one reference view of `size` = (width, height): uniform in inverse depth from d_min (plane 0) to
    d_max, as few as keep the largest displacement between adjacent planes - taken at the four image corners over the
    given warps - at or below 1 px, and at most max_planes.  Without a warp (or with every corner behind every source)
    there is nothing to measure: max_planes planes."""
    if not (isinstance(d_min, Real) and isinstance(d_max, Real) and 0 < d_min <= d_max < float("inf")):
        raise ValueError("depth range must satisfy 0 < d_min <= d_max < inf")
    if not (isinstance(max_planes, (int, np.integer)) and 1 <= max_planes <= MAX_PLANES):
        raise ValueError(f"max_planes must be 1 .. {MAX_PLANES}")
    if len(size) != 2 or min(size) < 1:
        raise ValueError("size must be (width, height)")
    warps = np.asarray(warps, dtype=np.float64).reshape(-1, 12)
    if d_min == d_max:
        return np.array([float(d_min)])

    def planes(n):
        return 1.0 / np.linspace(1.0 / d_min, 1.0 / d_max, n)

    def step(n):
        uv = _corner_tracks(1.0 / planes(n), warps, size)
        d = np.linalg.norm(np.diff(uv, axis=1), axis=2)
        return np.nanmax(d) if np.isfinite(d).any() else np.nan

    if len(warps) == 0 or max_planes < 2:
        return planes(int(max_planes))
    total = step(2)
    if not np.isfinite(total):
        return planes(int(max_planes))
    n = int(min(max(np.ceil(total - 1e-9) + 1, 2), max_planes))
    while n < max_planes and step(n) > 1.0 + 1e-9:          # a rotation between the views makes the motion non-uniform
        n += 1
    return planes(n)


def _registered_observations(rec):
    """(image, track) of every observation of a track with a point in a registered image (inlier ones under robust tracks)."""
    tr = rec.tracks
    trk = np.repeat(np.arange(len(tr)), tr.lengths())
    sel = np.flatnonzero(rec.has_point[trk] & (rec.cam_of_image()[tr.image] >= 0)) if tr.n_obs else np.zeros(0, np.int64)
    if rec.obs_inlier is not None:
        sel = sel[np.asarray(rec.obs_inlier)[sel]]
    return np.asarray(tr.image)[sel], trk[sel]


def select_sources(rec, n_sources=4):
    """{registered image: the up to n_sources registered images that share the most points with it} (most first; ties go to
    the lower image position; images that share no point are not sources)."""
    if not (isinstance(n_sources, (int, np.integer)) and 1 <= n_sources <= MAX_SOURCES):
        raise ValueError(f"n_sources must be 1 .. {MAX_SOURCES}")
    img, trk = _registered_observations(rec)
    n_img = len(rec.tracks.kp_ptr) - 1
    A = np.zeros((len(rec.tracks), n_img), dtype=np.float32)
    A[trk, img] = 1.0
    common = np.rint(A.T @ A).astype(np.int64)
    out = {}
    for i in sorted(rec.order):
        c = common[i].copy()
        c[i] = 0
        cand = [j for j in np.lexsort((np.arange(n_img), -c)) if c[j] > 0 and j in rec.poses]
        out[int(i)] = [int(j) for j in cand[:n_sources]]
    return out


def depth_ranges(rec, margin=0.2):
    """{registered image: (d_min, d_max)}: the smallest and largest positive depth of the points it observes, widened to
    d_min * (1 - margin) and d_max * (1 + margin).  An image that observes no point in front of it is left out."""
    if not (isinstance(margin, Real) and 0 <= margin < 1):
        raise ValueError("margin must be in [0, 1)")
    img, trk = _registered_observations(rec)
    out = {}
    for i in sorted(rec.order):
        R, t = _pose_of(rec.poses, i)
        z = (rec.X[trk[img == i]] @ R.T + t)[:, 2]
        z = z[np.isfinite(z) & (z > 0)]
        if len(z):
            out[int(i)] = (float(z.min() * (1.0 - margin)), float(z.max() * (1.0 + margin)))
    return out


def check_arguments(images, K, poses, sources, planes, radius=2):
    """Everything about a depth_maps call that can be judged without a device.  Returns (gray uint8 images, the reference
    views in order, src_ptr, src_image, warps [n_entries,12], backproj [n_ref,12], plane_ptr, plane depths).  ValueError says
    what is wrong."""
    from .features import _gray
    imgs = [np.ascontiguousarray(_gray(a)) for a in images]
    n_img = len(imgs)
    if not (isinstance(radius, (int, np.integer)) and 0 <= radius <= MAX_RADIUS):
        raise ValueError(f"radius must be an integer 0 .. {MAX_RADIUS}")
    if not isinstance(sources, dict) or not isinstance(planes, dict):
        raise ValueError("sources and planes must be dictionaries keyed by the reference image")
    refs = [int(r) for r in sources]
    if len(set(refs)) != len(refs):
        raise ValueError("a reference image is listed twice")
    src_ptr, src_image, plane_ptr, depth_list, warps, backproj = [0], [], [0], [], [], []
    for r, key in zip(refs, sources):
        if not 0 <= r < n_img:
            raise ValueError(f"reference {r} names an image outside 0..{n_img - 1}")
        src = [int(s) for s in sources[key]]
        if len(src) > MAX_SOURCES:
            raise ValueError(f"view {r}: at most {MAX_SOURCES} sources")
        for s in src:
            if not 0 <= s < n_img:
                raise ValueError(f"view {r}: source {s} names an image outside 0..{n_img - 1}")
            if s == r:
                raise ValueError(f"view {r}: a source is its own reference")
        if key not in planes:
            raise ValueError(f"view {r} has no planes")
        d = np.asarray(planes[key], dtype=np.float64).reshape(-1)
        if not 1 <= len(d) <= MAX_PLANES:
            raise ValueError(f"view {r}: 1 .. {MAX_PLANES} planes, not {len(d)}")
        if not (np.isfinite(d) & (d > 0)).all():
            raise ValueError(f"view {r}: every plane depth must be finite and > 0")
        warps.append(view_warps(K, poses, r, src))
        backproj.append(view_backprojection(K, poses, r))
        src_image += src
        src_ptr.append(len(src_image))
        depth_list.append(d)
        plane_ptr.append(plane_ptr[-1] + len(d))
    return (imgs, refs, np.array(src_ptr, dtype=np.int64), np.array(src_image, dtype=np.int32),
            np.concatenate(warps).reshape(-1, 12) if warps else np.zeros((0, 12)),
            np.array(backproj, dtype=np.float64).reshape(-1, 12), np.array(plane_ptr, dtype=np.int64),
            np.concatenate(depth_list) if depth_list else np.zeros(0))


class DepthMaps:
    """What `depth_maps` returns.  views: the reference images in order; depth (float32), plane (int32), cost (uint16): one
    [h,w] array per view; after `.filter(...)` also n_consistent, keep (uint8) and xyz (float64 [h,w,3])."""

    def __init__(self, state):
        self._s = state
        self.views = list(state["refs"])
        self.shapes = [state["imgs"][r].shape for r in self.views]
        self.radius = state["radius"]
        self.n_sources = np.diff(state["src_ptr"]).tolist()
        self.n_consistent = self.keep = self.xyz = None
        self._host = {}

    def _split(self, name, tail=()):
        if name not in self._host:
            flat = self._s[name].cpu().numpy()
            if name == "cost":
                flat = flat.view(np.uint16)                   # held as int16 on the device side: torch has no uint16 indexing
            out, o = [], 0
            for h, w in self.shapes:
                out.append(flat[o:o + h * w].reshape((h, w) + tail))
                o += h * w
            self._host[name] = out
        return self._host[name]

    depth = property(lambda self: self._split("depth"))
    plane = property(lambda self: self._split("plane"))
    cost = property(lambda self: self._split("cost"))

    def filter(self, rel_tol=0.01, max_cost=None, min_consistent=2):
        """Cross-view check and back-projection on the device.  rel_tol: a source agrees when its own depth at the pixel the
        point falls on differs from the point's depth in that source by at most rel_tol of it; max_cost: None, or the
        largest MEAN census cost per sample (0 .. 48) a kept pixel may have - the device compares the pixel's cost with
        floor(max_cost * sources * window) of its view; min_consistent: agreeing sources a kept pixel needs.  Fills
        n_consistent, keep, xyz and returns self."""
        import torch
        if not (isinstance(rel_tol, Real) and rel_tol >= 0):
            raise ValueError("rel_tol must be a number >= 0")
        if max_cost is not None and not (isinstance(max_cost, Real) and max_cost >= 0):
            raise ValueError("max_cost must be None or a number >= 0")
        if not (isinstance(min_consistent, (int, np.integer)) and 0 <= min_consistent <= MAX_SOURCES):
            raise ValueError(f"min_consistent must be an integer 0 .. {MAX_SOURCES}")
        s = self._s
        limit = None if max_cost is None else self.cost_limits(max_cost)
        n = max(s["n_out"], 1)
        dev = s["depth"].device
        s["n_consistent"] = torch.empty(n, dtype=torch.uint8, device=dev)
        s["keep"] = torch.empty(n, dtype=torch.uint8, device=dev)
        s["xyz"] = torch.empty((n, 3), dtype=torch.float64, device=dev)
        dp = lambda t: C.c_void_p(t.data_ptr())
        hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        h = _lib.get_handle(dev.index)
        h.call("sfm_depth_filter", hp(s["off"]), hp(s["heights"]), hp(s["widths"]), len(s["imgs"]), len(self.views), hp(s["ref_image"]),
               hp(s["src_ptr"]), hp(s["src_image"]), dp(s["warps"]), dp(s["backproj"]), dp(s["depth"]), dp(s["cost"]), hp(limit),
               C.c_double(float(rel_tol)), int(min_consistent), dp(s["n_consistent"]), dp(s["keep"]), dp(s["xyz"]), dp(s["ws"]),
               s["ws"].numel())
        for name in ("n_consistent", "keep", "xyz"):
            self._host.pop(name, None)
        self.n_consistent, self.keep = self._split("n_consistent"), self._split("keep")
        self.xyz = self._split("xyz", (3,))
        self._rel_tol = float(rel_tol)
        return self

    def fuse(self, rel_tol=None, normal_step=2, normal_jump=0.05):
        """The kept pixels of all views fused into one cloud with normals on the device (`sfm_depth_fuse_mark` /
        `sfm_depth_fuse_gather`; include/sfm_amd.h states the rule): a surface point is kept once, by the earliest view that
        sees it, as the mean of the views that agree on it.  rel_tol: the agreement of two views' depths, None for the value
        of the last `.filter()`; normal_step: the normal of a pixel comes from its neighbours this many pixels away, 1 .. 4;
        normal_jump: a neighbour whose depth differs by more than this share of the pixel's is across an edge, and the pixel
        gets no normal.  Needs `.filter()` first.  Returns a `FusedCloud`."""
        import torch
        if self.keep is None:
            raise ValueError("fuse() needs filter() first")
        rel_tol = self._rel_tol if rel_tol is None else rel_tol
        if not (isinstance(rel_tol, Real) and rel_tol >= 0):
            raise ValueError("rel_tol must be None or a number >= 0")
        if not (isinstance(normal_step, (int, np.integer)) and 1 <= normal_step <= MAX_NORMAL_STEP):
            raise ValueError(f"normal_step must be an integer 1 .. {MAX_NORMAL_STEP}")
        if not (isinstance(normal_jump, Real) and normal_jump >= 0):
            raise ValueError("normal_jump must be a number >= 0")
        s = self._s
        n, n_ref, n_img = max(s["n_out"], 1), len(self.views), len(s["imgs"])
        dev = s["depth"].device
        h = _lib.get_handle(dev.index)
        need = C.c_int64()
        h.check(h.lib.sfm_depth_fuse_workspace_bytes(n_img, n_ref, len(s["src_image"]), s["n_out"], C.byref(need)),
                "sfm_depth_fuse_workspace_bytes")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        f = {"view_normals": torch.empty((n, 3), dtype=torch.float32, device=dev),
             "agree_mask": torch.empty(n, dtype=torch.uint8, device=dev), "owner": torch.empty(n, dtype=torch.uint8, device=dev),
             "pt_ptr": torch.empty(n_ref + 1, dtype=torch.int64, device=dev)}
        dp = lambda t: C.c_void_p(t.data_ptr())
        hp = lambda a: C.c_void_p(a.ctypes.data)
        views = (hp(s["off"]), hp(s["heights"]), hp(s["widths"]), n_img, n_ref, hp(s["ref_image"]), hp(s["src_ptr"]), hp(s["src_image"]),
                 dp(s["warps"]))
        h.call("sfm_depth_fuse_mark", *views, dp(s["backproj"]), dp(s["depth"]), dp(s["keep"]), dp(s["xyz"]), C.c_double(float(rel_tol)),
               int(normal_step), C.c_double(float(normal_jump)), dp(f["view_normals"]), dp(f["agree_mask"]), dp(f["owner"]),
               dp(f["pt_ptr"]), dp(ws), need.value)
        pt_ptr = f["pt_ptr"].cpu().numpy()                       # waits for the mark call: the number of points sizes the outputs
        m = int(pt_ptr[-1])
        f["points"] = torch.empty((max(m, 1), 3), dtype=torch.float64, device=dev)
        f["normals"] = torch.empty((max(m, 1), 3), dtype=torch.float32, device=dev)
        f["n_views"] = torch.empty(max(m, 1), dtype=torch.uint8, device=dev)
        f["index"] = torch.empty((max(m, 1), 3), dtype=torch.int32, device=dev)
        h.call("sfm_depth_fuse_gather", *views, dp(s["depth"]), dp(s["xyz"]), dp(f["view_normals"]), dp(f["agree_mask"]), dp(f["owner"]),
               dp(f["pt_ptr"]), m, dp(f["points"]), dp(f["normals"]), dp(f["n_views"]), dp(f["index"]), dp(ws), need.value)
        return FusedCloud(f, pt_ptr, self)

    def tsdf(self, origin=None, voxel=None, shape=None, resolution=256, margin=0.05, trunc=None, min_weight=1):
        """The kept pixels of all views integrated into a truncated signed distance volume on the device
        (`sfm_tsdf_integrate`; include/sfm_amd.h states the rule).  origin (3 numbers), voxel and shape = (nx, ny, nz) nodes,
        each 2 .. 1024, come together; without them the box is, per axis, the 1st to 99th percentile of the kept pixels' xyz
        widened by margin of its length on both sides, with cubic voxels so that the longest side has `resolution` nodes.
        trunc: the truncation distance, None for 3 voxels; min_weight: what `.mesh()` of the volume takes by default.  Every
        view weighs the same, and space that no kept pixel looks through stays unknown.  Needs `.filter()` first.  Returns a
        `TsdfVolume`."""
        from .mesh import integrate_depth_maps
        return integrate_depth_maps(self, origin, voxel, shape, resolution, margin, trunc, min_weight)

    def cost_limits(self, max_cost):
        """int32 per view: floor(max_cost * sources * window), what `filter(max_cost=...)` hands to the device."""
        win = (2 * self.radius + 1) ** 2
        return np.array([min(int(np.floor(max_cost * ns * win)), 65535) for ns in self.n_sources], dtype=np.int32)

    def point_cloud(self, colors=None):
        """(points float64 [m,3], index int64 [m,3] as (view position, y, x)) of the kept pixels in (view, row-major) order;
        with colors - one [h,w] or [h,w,3] array per IMAGE - also the colour of every point.  Needs `.filter()` first."""
        import torch
        if self.keep is None:
            raise ValueError("point_cloud() needs filter() first")
        s = self._s
        idx = torch.nonzero(s["keep"][:s["n_out"]], as_tuple=False).reshape(-1)          # compaction is torch indexing
        pts = s["xyz"][idx].cpu().numpy()
        flat = idx.cpu().numpy()
        first = np.cumsum([0] + [h * w for h, w in self.shapes])
        view = np.searchsorted(first, flat, side="right") - 1
        index = np.zeros((len(flat), 3), dtype=np.int64)
        if len(flat):
            local = flat - first[view]
            widths = np.array([w for _, w in self.shapes], dtype=np.int64)[view]
            index = np.stack([view, local // widths, local % widths], axis=1).astype(np.int64)
        if colors is None:
            return pts, index
        if len(colors) != len(s["imgs"]):
            raise ValueError("colors: one array per image")
        col = [np.asarray(colors[r]) for r in self.views]
        tail = col[0].shape[2:] if col else ()
        out = np.zeros((len(flat),) + tail, dtype=col[0].dtype if col else np.uint8)
        for v in range(len(self.views)):
            m = index[:, 0] == v
            out[m] = col[v][index[m, 1], index[m, 2]]
        return pts, index, out


class FusedCloud:
    """What `DepthMaps.fuse` returns; the arrays stay on the device until they are asked for.  points float64 [m,3], normals
    float32 [m,3] (zeros where no agreeing view has a normal), n_views uint8 [m] (the views a point is the mean of), index
    int32 [m,3] as (view position, y, x) of the owning pixel, in (view, row-major) order; pt_ptr int64 [views + 1]: the points
    of view v are pt_ptr[v] .. pt_ptr[v+1]; view_normals (float32 [h,w,3]), owner and agree_mask (uint8 [h,w]): one per view."""

    def __init__(self, state, pt_ptr, maps):
        self._f = state
        self._maps = maps
        self.pt_ptr = pt_ptr
        self._host = {}

    def __len__(self):
        return int(self.pt_ptr[-1])

    def _flat(self, name):
        if name not in self._host:
            self._host[name] = self._f[name].cpu().numpy()[:len(self)]
        return self._host[name]

    def _per_view(self, name, tail=()):
        if name not in self._host:
            flat, out, o = self._f[name].cpu().numpy(), [], 0
            for h, w in self._maps.shapes:
                out.append(flat[o:o + h * w].reshape((h, w) + tail))
                o += h * w
            self._host[name] = out
        return self._host[name]

    points = property(lambda self: self._flat("points"))
    normals = property(lambda self: self._flat("normals"))
    n_views = property(lambda self: self._flat("n_views"))
    index = property(lambda self: self._flat("index"))
    view_normals = property(lambda self: self._per_view("view_normals", (3,)))
    owner = property(lambda self: self._per_view("owner"))
    agree_mask = property(lambda self: self._per_view("agree_mask"))

    def colors(self, images):
        """The colour of every point from its owning pixel: images is one [h,w] or [h,w,3] array per IMAGE of the set."""
        maps = self._maps
        if len(images) != len(maps._s["imgs"]):
            raise ValueError("colors: one array per image")
        col = [np.asarray(images[r]) for r in maps.views]
        index = self.index
        tail = col[0].shape[2:] if col else ()
        out = np.zeros((len(index),) + tail, dtype=col[0].dtype if col else np.uint8)
        for v in range(len(col)):
            m = index[:, 0] == v
            out[m] = col[v][index[m, 1], index[m, 2]]
        return out


def depth_maps(images, K, poses, sources, planes, radius=2, device=0):
    """Depth maps of the reference views named by `sources`.

    images: every image of the set, [h,w] uint8 (or [h,w,3] BGR, converted like the feature stage does), sizes may differ;
    K: one 3 x 3 matrix or one per image; poses: {image position: (R, t)} with x_cam = R X + t; sources: {reference image:
    [source images]} (at most 8 each, an empty list is allowed); planes: {reference image: plane depths} (1 .. 1024,
    finite, > 0; `plane_depths` chooses them); radius: the aggregation window is (2 radius + 1)^2, 0 .. 4.
    Returns `DepthMaps` (outputs stay on the device until they are asked for)."""
    return depth_maps_raw(*check_arguments(images, K, poses, sources, planes, radius), radius=radius, device=device)


def depth_maps_raw(imgs, refs, src_ptr, src_image, warps, backproj, plane_ptr, depths, radius=2, device=0):
    """The census and the sweep on arrays in the shapes of the ABI (what `check_arguments` returns): the warps and the
    back-projections are taken as given."""
    import torch
    from .features import _upload_images
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    n_img, n_ref = len(imgs), len(refs)
    heights = np.array([a.shape[0] for a in imgs], dtype=np.int32)
    widths = np.array([a.shape[1] for a in imgs], dtype=np.int32)
    d_img, off = _upload_images(imgs, dev)
    ref_image = np.array(refs, dtype=np.int32)
    need = C.c_int64()
    h.check(h.lib.sfm_depth_workspace_bytes(n_img, n_ref, len(src_image), C.byref(need)), "sfm_depth_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    n_out = int(sum(imgs[r].size for r in refs))
    st = {"imgs": imgs, "refs": refs, "radius": int(radius), "off": off, "heights": heights, "widths": widths, "ref_image": ref_image,
          "src_ptr": src_ptr, "src_image": src_image, "n_out": n_out, "ws": ws,
          "warps": torch.from_numpy(np.ascontiguousarray(warps)).to(dev) if len(warps) else torch.zeros((1, 12), dtype=torch.float64, device=dev),
          "backproj": torch.from_numpy(np.ascontiguousarray(backproj)).to(dev) if n_ref else torch.zeros((1, 12), dtype=torch.float64, device=dev),
          "census": torch.empty(max(int(off[-1]), 1), dtype=torch.int64, device=dev),
          "plane": torch.empty(max(n_out, 1), dtype=torch.int32, device=dev),
          "cost": torch.empty(max(n_out, 1), dtype=torch.int16, device=dev),
          "depth": torch.empty(max(n_out, 1), dtype=torch.float32, device=dev)}
    d_planes = torch.from_numpy(depths).to(dev) if len(depths) else torch.zeros(1, dtype=torch.float64, device=dev)
    dp = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: C.c_void_p(a.ctypes.data)
    h.call("sfm_depth_census", dp(d_img), hp(off), hp(heights), hp(widths), n_img, dp(st["census"]), dp(ws), need.value)
    h.call("sfm_depth_sweep", dp(st["census"]), hp(off), hp(heights), hp(widths), n_img, n_ref, hp(ref_image), hp(src_ptr), hp(src_image),
           dp(st["warps"]), hp(plane_ptr), dp(d_planes), int(radius), dp(st["plane"]), dp(st["cost"]), dp(st["depth"]), dp(ws), need.value)
    return DepthMaps(st)


def depth_maps_from_arrays(shapes, refs, src_ptr, src_image, warps, backproj, depth, keep, xyz, rel_tol=0.01, device=0):
    """A `DepthMaps` around maps that were made and filtered elsewhere, for `.fuse()`: shapes is the (height, width) of every
    image of the set, refs / src_ptr / src_image / warps / backproj are as `check_arguments` returns them, and depth
    (float32 [h,w]), keep (uint8 [h,w]) and xyz (float64 [h,w,3]) hold one array per view in the order of refs.  plane, cost
    and n_consistent are zeros.  rel_tol is what `.fuse(rel_tol=None)` takes."""
    import torch
    shapes = [(int(h), int(w)) for h, w in shapes]
    refs = [int(r) for r in refs]
    if len(set(refs)) != len(refs) or any(not 0 <= r < len(shapes) for r in refs):
        raise ValueError("refs must name different images of the set")
    if not (len(depth) == len(keep) == len(xyz) == len(refs)):
        raise ValueError("depth, keep and xyz need one array per view")
    for v, r in enumerate(refs):
        if np.shape(depth[v]) != shapes[r] or np.shape(keep[v]) != shapes[r] or np.shape(xyz[v]) != shapes[r] + (3,):
            raise ValueError(f"view {v}: the maps must have the shape of image {r}")
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    n_img, n_ref = len(shapes), len(refs)
    src_ptr, src_image = np.ascontiguousarray(src_ptr, dtype=np.int64), np.ascontiguousarray(src_image, dtype=np.int32)
    off = np.zeros(n_img + 1, dtype=np.int64)
    np.cumsum([hh * ww for hh, ww in shapes], out=off[1:])
    need = C.c_int64()
    h.check(h.lib.sfm_depth_workspace_bytes(n_img, n_ref, len(src_image), C.byref(need)), "sfm_depth_workspace_bytes")
    n_out = int(sum(shapes[r][0] * shapes[r][1] for r in refs))

    def up(arrays, dtype, tail=()):
        """The views' arrays back to back on the device (one element where there is no pixel: a pointer must exist)."""
        if not n_out:
            return torch.from_numpy(np.zeros((1,) + tail, dtype)).to(dev)
        flat = np.concatenate([np.asarray(a, dtype=dtype).reshape((-1,) + tail) for a in arrays])
        return torch.from_numpy(np.ascontiguousarray(flat)).to(dev)

    def table(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev) if len(a) else torch.zeros((1, 12), dtype=torch.float64, device=dev)

    warps = np.asarray(warps, dtype=np.float64).reshape(-1, 12)
    backproj = np.asarray(backproj, dtype=np.float64).reshape(-1, 12)
    st = {"imgs": [np.zeros(sh, np.uint8) for sh in shapes], "refs": refs, "radius": 0, "off": off,
          "heights": np.array([sh[0] for sh in shapes], dtype=np.int32), "widths": np.array([sh[1] for sh in shapes], dtype=np.int32),
          "ref_image": np.array(refs, dtype=np.int32), "src_ptr": src_ptr, "src_image": src_image, "n_out": n_out,
          "ws": torch.empty(need.value, dtype=torch.uint8, device=dev),
          "warps": table(warps), "backproj": table(backproj),
          "plane": torch.zeros(max(n_out, 1), dtype=torch.int32, device=dev),
          "cost": torch.zeros(max(n_out, 1), dtype=torch.int16, device=dev),
          "n_consistent": torch.zeros(max(n_out, 1), dtype=torch.uint8, device=dev),
          "depth": up(depth, np.float32), "keep": up(keep, np.uint8), "xyz": up(xyz, np.float64, (3,))}
    maps = DepthMaps(st)
    maps.n_consistent, maps.keep, maps.xyz = maps._split("n_consistent"), maps._split("keep"), maps._split("xyz", (3,))
    maps._rel_tol = float(rel_tol)
    return maps


def dense_from_reconstruction(rec, images, n_sources=4, margin=0.2, max_planes=256, radius=2, rel_tol=0.01, max_cost=None,
                              min_consistent=2, colors=None, device=0, fuse=False, mesh=False, texture=None,
                              min_triangles=None, keep_largest=None, fill_holes=None, decimate=None, smooth=None):
    """The chain on a `Reconstruction`: sources by shared points (`select_sources`), the depth interval of every view from
    its sparse points (`depth_ranges`), planes at most one pixel apart (`plane_depths`), `depth_maps`, `.filter`,
    `.point_cloud`.  images: one per image position of rec.tracks.  Returns (points, index, DepthMaps) - or (points, index,
    colours, DepthMaps) with colors.  With fuse=True the last step is `.fuse()` in place of `.point_cloud`, and the result
    is (FusedCloud, DepthMaps); the colours are then `FusedCloud.colors(colors)`.  With mesh=True the surface of the kept
    pixels, `maps.tsdf().mesh()`, is appended to whichever of those is returned; with colors (uint8 images) it is coloured
    by `Mesh.colors(colors)`, and with texture (an integer, the texels per triangle leg) it also gets the atlas of
    `Mesh.texture(colors, texels=texture)` as `Mesh.atlas`; the tuple keeps its shape.  With min_triangles or keep_largest
    (both None: nothing changes) the mesh is `Mesh.clean(min_triangles, keep_largest)` of that surface - min_triangles None
    is 1 then - cleaned before it is coloured.  With fill_holes (None: nothing changes; otherwise max_edges, 1 .. 64) the
    mesh is then `Mesh.fill_holes(fill_holes)` of that: filled after the cleaning and before it is coloured.  With decimate
    (None: nothing changes; otherwise a factor, a finite number > 0) the mesh is then `Mesh.decimate(factor=decimate)` of that:
    clustered on cells of that many voxels after the cleaning and the filling and before it is coloured.  With smooth (None:
    nothing changes; otherwise an iteration count, 0 .. 1000) the mesh is `Mesh.smooth(smooth)` after the cleaning and the
    filling and before the decimation, so that the quadrics see the smoothed faces."""
    if smooth is not None:
        from .mesh_smooth import check_smooth_arguments
        if not mesh:
            raise ValueError("smooth needs mesh=True")
        check_smooth_arguments(smooth)
    if decimate is not None:
        if not mesh:
            raise ValueError("decimate needs mesh=True")
        if not (isinstance(decimate, Real) and not isinstance(decimate, bool) and np.isfinite(decimate) and decimate > 0):
            raise ValueError("decimate must be None or a factor, a finite number > 0")
    if fill_holes is not None:
        from .mesh_fill import check_fill_arguments
        if not mesh:
            raise ValueError("fill_holes needs mesh=True")
        check_fill_arguments(fill_holes)
    cleaning = min_triangles is not None or keep_largest is not None
    if cleaning:
        from .mesh_clean import check_clean_arguments
        if not mesh:
            raise ValueError("min_triangles and keep_largest need mesh=True")
        min_triangles = 1 if min_triangles is None else min_triangles
        check_clean_arguments(min_triangles, keep_largest)
    if texture is not None:
        if not (isinstance(texture, (int, np.integer)) and 1 <= texture <= 64):
            raise ValueError("texture must be None or the texels per triangle leg, an integer 1 .. 64")
        if not mesh or colors is None:
            raise ValueError("texture needs mesh=True and colors: the images the atlas is blended from")
    n_img = len(rec.tracks.kp_ptr) - 1
    if len(images) != n_img:
        raise ValueError(f"{len(images)} images for {n_img} image positions")
    src = select_sources(rec, n_sources)
    rng = depth_ranges(rec, margin)
    src = {r: s for r, s in src.items() if r in rng}
    planes = {}
    for r, s in src.items():
        size = (int(np.asarray(images[r]).shape[1]), int(np.asarray(images[r]).shape[0]))
        planes[r] = plane_depths(rng[r][0], rng[r][1], view_warps(rec.K, rec.poses, r, s), size, max_planes)
    maps = depth_maps(images, rec.K, rec.poses, src, planes, radius, device)
    maps.filter(rel_tol, max_cost, min_consistent)
    surface = (maps.tsdf().mesh(),) if mesh else ()
    if cleaning:
        surface = (surface[0].clean(min_triangles, keep_largest),)
    if fill_holes is not None:
        surface = (surface[0].fill_holes(int(fill_holes)),)
    if smooth is not None:
        surface = (surface[0].smooth(int(smooth)),)
    if decimate is not None:
        surface = (surface[0].decimate(factor=float(decimate)),)
    if mesh and colors is not None:
        surface[0].colors(colors)
        if texture is not None:
            surface[0].texture(colors, texels=int(texture))
    if fuse:
        return (maps.fuse(), maps) + surface
    return maps.point_cloud(colors) + (maps,) + surface
