"""Exposure compensation between the views of a mesh: one gain per view and channel, estimated from the vertices that several
views see (`sfm_mesh_exposure_sample`, `sfm_mesh_exposure_gram`: sfm_amd/csrc/mesh_exposure.hip) and applied to the images
(`sfm_images_gain`) before they go to `Mesh.colors`, `Mesh.texture` and `Mesh.score`; include/sfm_amd.h states the rule
completely.  The device makes the samples and two integer tables, the solve of the gains is float64 NumPy here
(`solve_gains`).  No CPU fallback: without the library or a GPU the device calls raise.
"""
from __future__ import annotations

import ctypes as C
from numbers import Real

import numpy as np

from . import _lib
from ._lib import dp, hp
from ._views import ViewSet, centres_from_projections, check_color_images, workspace  # noqa: F401

MAX_VIEWS = 1024


def check_exposure_arguments(tol, min_cos, sigma_n=10.0, sigma_g=1.0, min_overlap=1, n_views=0):
    """The checks of `Mesh.exposure` and `mesh_exposure_tables` that need no device; ValueError says what is wrong."""
    from .mesh import check_color_scalars
    check_color_scalars(tol, min_cos, 0)
    for name, s in (("sigma_n", sigma_n), ("sigma_g", sigma_g)):
        if not (isinstance(s, Real) and not isinstance(s, bool) and np.isfinite(s) and s > 0):
            raise ValueError(f"{name} must be a finite number > 0")
    if not (isinstance(min_overlap, (int, np.integer)) and not isinstance(min_overlap, bool) and min_overlap >= 1):
        raise ValueError("min_overlap must be an integer >= 1")
    if not 0 <= n_views <= MAX_VIEWS:
        raise ValueError(f"at most {MAX_VIEWS} views")


def check_gains(gains, n_images, channels):
    """float64 [n_images, channels] from gains, each finite and >= 0, or ValueError."""
    g = np.asarray(gains, dtype=np.float64)
    if g.shape == (n_images,) and channels == 1:
        g = g.reshape(n_images, 1)
    if g.shape != (n_images, channels):
        raise ValueError(f"gains must be [{n_images}, {channels}]: one per image and channel")
    if not (np.isfinite(g).all() and (g >= 0).all()):
        raise ValueError("every gain must be finite and >= 0")
    return np.ascontiguousarray(g)


def solve_gains(overlap, sums, sigma_n=10.0, sigma_g=1.0, min_overlap=1):
    """The gains float64 [n, channels] from overlap int [n, n] and sums int [n, n, channels] (include/sfm_amd.h, "Gains"):
    per channel the minimum of sum over ordered pairs i != j of N ((g_i a - g_j b)^2 / sigma_n^2 + (1 - g_i)^2 / sigma_g^2)
    with N = overlap[i][j], a = sums[i][j] / N, b = sums[j][i] / N.  Pairs with fewer than min_overlap common vertices are
    ignored; a view without a pair gets the gain 1."""
    check_exposure_arguments(0.0, 1.0, sigma_n, sigma_g, min_overlap)
    overlap, sums = np.asarray(overlap), np.asarray(sums)
    n = overlap.shape[0] if overlap.ndim == 2 else -1
    if overlap.ndim != 2 or overlap.shape != (n, n) or sums.ndim != 3 or sums.shape[:2] != (n, n) or sums.shape[2] not in (1, 3):
        raise ValueError("overlap must be [n, n] and sums [n, n, channels], channels 1 or 3")
    if overlap.dtype.kind not in "iu" or sums.dtype.kind not in "iu":
        raise ValueError("overlap and sums must hold integers")
    channels = sums.shape[2]
    gains = np.ones((n, channels))
    N = overlap.astype(np.float64)
    N[(overlap < min_overlap) | np.eye(n, dtype=bool)] = 0.0
    pair = N > 0
    active = pair.sum(axis=1) > 0
    if not active.any():
        return gains
    Nd = np.where(pair, N, 1.0)
    in2, ig2 = 1.0 / (float(sigma_n) * float(sigma_n)), 1.0 / (float(sigma_g) * float(sigma_g))
    for k in range(channels):
        S = sums[:, :, k].astype(np.float64)
        a = np.where(pair, S / Nd, 0.0)                            # a of the ordered pair (i, j)
        b = np.where(pair, S.T / Nd, 0.0)                          # b of the ordered pair (i, j)
        off = N * a * b * in2
        A = -(off + off.T)
        A[np.diag_indices(n)] = (N * (a * a * in2 + ig2)).sum(axis=1) + (N * b * b * in2).sum(axis=0)
        rhs = N.sum(axis=1) * ig2
        gains[active, k] = np.linalg.solve(A[np.ix_(active, active)], rhs[active])
    return gains


class ExposureGains:
    """What `Mesh.exposure` returns.  gains float64 [n_views, channels], overlap int64 [n_views, n_views], sums int64
    [n_views, n_views, channels]; seen uint8 [n_views, nv] and samples uint8 [n_views, channels, nv] stay on the device until
    they are asked for.  views: the image of the set behind every view."""

    def __init__(self, state, gains, overlap, sums, n_vertices, channels, views, n_images):
        self._m, self.gains, self.overlap, self.sums = state, gains, overlap, sums
        self.n_vertices, self.channels, self.views, self.n_images = int(n_vertices), int(channels), [int(v) for v in views], int(n_images)
        self._host = {}

    def _get(self, name, shape):
        if name not in self._host:
            n = int(np.prod(shape, dtype=np.int64))
            self._host[name] = self._m[name].cpu().numpy().reshape(-1)[:n].reshape(shape)
        return self._host[name]

    seen = property(lambda self: self._get("seen", (len(self.views), self.n_vertices)))
    samples = property(lambda self: self._get("samples", (len(self.views), self.channels, self.n_vertices)))

    def spread(self):
        """float64 [nv, channels]: per vertex and channel the largest minus the smallest sample over the views that see the
        vertex; NaN for a vertex with fewer than 2 views."""
        return sample_spread(self.seen, self.samples)

    def image_gains(self):
        """float64 [n_images, channels]: the gain of every image of the set, 1 for an image that is no view."""
        g = np.ones((self.n_images, self.channels))
        g[self.views] = self.gains
        return g

    def apply(self, images):
        """The images with their gains applied on the device (`sfm_images_gain`): one uint8 array per IMAGE of the set, as
        `Mesh.exposure` took them; returns the corrected arrays in the same order, ready for `Mesh.colors`, `Mesh.texture`
        and `Mesh.score`."""
        if len(images) != self.n_images:
            raise ValueError("images: one array per image of the set")
        dev = self._m["seen"].device
        return apply_gains(images, self.image_gains(), dev.index or 0)


def sample_spread(seen, samples):
    """What `ExposureGains.spread` computes, on host arrays."""
    seen = np.asarray(seen) != 0
    q = np.asarray(samples).astype(np.int64)
    if len(seen) == 0:
        return np.full((seen.shape[1], q.shape[1]), np.nan)
    hi = np.where(seen[:, None, :], q, -1).max(axis=0)             # [channels, nv]
    lo = np.where(seen[:, None, :], q, 256).min(axis=0)
    return np.where(seen.sum(axis=0) >= 2, (hi - lo).astype(np.float64), np.nan).T


def _tables(views, n_vertices, d_vertices, d_normals, tol, min_cos):
    """The two device calls: a `ViewSet` with its pixels; the vertices and the normals on the device.  Returns the device
    state: seen, samples, overlap, sums."""
    import torch
    dev = views.depth.device
    h = _lib.get_handle(dev.index)
    n_ref, channels, nv = views.n_ref, views.channels, int(n_vertices)
    ws, ws_bytes = workspace(h, dev, "sfm_mesh_exposure_workspace_bytes", n_ref, channels, nv)
    out = {"seen": torch.empty(max(n_ref * nv, 1), dtype=torch.uint8, device=dev),
           "samples": torch.empty(max(n_ref * channels * nv, 1), dtype=torch.uint8, device=dev),
           "overlap": torch.empty(max(n_ref * n_ref, 1), dtype=torch.int64, device=dev),
           "sums": torch.empty(max(n_ref * n_ref * channels, 1), dtype=torch.int64, device=dev)}
    h.call("sfm_mesh_exposure_sample", *views.args(), nv, dp(d_vertices), dp(d_normals), C.c_double(float(tol)), C.c_double(float(min_cos)),
           dp(out["seen"]), dp(out["samples"]), dp(ws), ws_bytes)
    h.call("sfm_mesh_exposure_gram", n_ref, channels, nv, dp(out["seen"]), dp(out["samples"]), dp(out["overlap"]), dp(out["sums"]),
           dp(ws), ws_bytes)
    out["held"] = (ws, d_vertices, d_normals) + views.alive()       # alive while the calls may still run
    return out


def _host_tables(state, n_ref, channels):
    overlap = state["overlap"].cpu().numpy()[:n_ref * n_ref].reshape(n_ref, n_ref)
    sums = state["sums"].cpu().numpy()[:n_ref * n_ref * channels].reshape(n_ref, n_ref, channels)
    return overlap, sums


def mesh_exposure_tables(vertices, normals, proj, centres, depth, keep, images, tol, min_cos=0.35, device=0):
    """`sfm_mesh_exposure_sample` and `sfm_mesh_exposure_gram` on arrays that were made elsewhere; the arguments are those of
    `mesh_vertex_colors`.  Returns (seen uint8 [n,nv], samples uint8 [n,channels,nv], overlap int64 [n,n], sums int64
    [n,n,channels])."""
    from .mesh import check_mesh_arrays, upload_rows
    check_exposure_arguments(tol, min_cos)
    vertices, normals, _ = check_mesh_arrays(vertices, normals)
    views = ViewSet.from_arrays(proj, centres, depth, keep, MAX_VIEWS, images).to(device)
    dev, n, nv, channels = views.depth.device, views.n_ref, len(vertices), views.channels
    st = _tables(views, nv, upload_rows(vertices, dev), upload_rows(normals, dev), tol, min_cos)
    overlap, sums = _host_tables(st, n, channels)
    return (st["seen"].cpu().numpy()[:n * nv].reshape(n, nv), st["samples"].cpu().numpy()[:n * channels * nv].reshape(n, channels, nv),
            overlap, sums)


def apply_gains(images, gains, device=0):
    """`sfm_images_gain`: images one uint8 [h,w] or [h,w,3] array each, all with the same channel count, gains float64
    [n, channels], each finite and >= 0.  Returns the arrays with out = min(floor(in * g + 0.5), 255) per pixel and channel."""
    import torch
    arrays = [np.asarray(a) for a in images]
    flat, channels = check_color_images(arrays, [a.shape[:2] for a in arrays])
    g = check_gains(gains, len(arrays), channels)
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    heights = np.array([a.shape[0] for a in arrays] + [0], dtype=np.int32)
    widths = np.array([a.shape[1] for a in arrays] + [0], dtype=np.int32)
    d_in = torch.from_numpy(flat).to(dev)
    d_out = torch.empty_like(d_in)
    gp = np.concatenate([g.reshape(-1), np.ones(1)])               # one element more: a pointer must exist
    h.call("sfm_images_gain", hp(heights), hp(widths), len(arrays), int(channels), hp(gp), dp(d_in), dp(d_out))
    host = d_out.cpu().numpy()                                     # waits for the call: gp and d_in may go
    out, o = [], 0
    for a in arrays:
        out.append(host[o:o + a.size].reshape(a.shape).copy())
        o += a.size
    return out


def mesh_exposure(mesh, images, maps=None, tol=None, min_cos=0.35, sigma_n=10.0, sigma_g=1.0, min_overlap=1):
    """What `Mesh.exposure` does."""
    tol = mesh._tol("exposure", tol)
    check_exposure_arguments(tol, min_cos, sigma_n, sigma_g, min_overlap)
    views = mesh._views("exposure", maps, images, arrays_too=True)
    check_exposure_arguments(tol, min_cos, n_views=views.n_ref)
    st = _tables(views, mesh.n_vertices, mesh._m["vertices"], mesh._m["normals"], tol, min_cos)
    overlap, sums = _host_tables(st, views.n_ref, views.channels)
    return ExposureGains(st, solve_gains(overlap, sums, sigma_n, sigma_g, min_overlap), overlap, sums, mesh.n_vertices, views.channels, views.views,
                         views.n_images)
