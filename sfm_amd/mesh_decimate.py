"""Decimation of a mesh by vertex clustering on the device: `sfm_mesh_decimate_cluster`, `sfm_mesh_decimate_mark` and
`sfm_mesh_decimate_emit` (sfm_amd/csrc/mesh_decimate.hip); include/sfm_amd.h states the rule completely.  The vertices are
sorted into the cells of a uniform grid; every cell that holds some becomes one vertex, at the mean of its members or - the
default - where the planes of the triangles that touch the cell meet, pulled towards that mean and kept inside the cell;
a triangle stays when its three vertices land in three cells, and of several on one triple of cells the first of the
prevailing orientation stays, none when the orientations balance.  A function of its inputs, the same from run to run: no
priority queue, no target count.  No CPU fallback: without the library or a GPU the calls raise.
"""
from __future__ import annotations

import ctypes as C
from numbers import Real

import numpy as np

from . import _lib
from ._lib import dp as _dp, hp as _hp
from .mesh_clean import _up, check_clean_arguments

MAX_TRIANGLES = 0x7FFFFFFF // 3
AXIS_CELLS = 1 << 21
PLACEMENTS = {"mean": 0, "quadric": 1}


def check_decimate_arguments(cell=1.0, origin=None, placement="quadric", n_vertices=None, triangles=None, vertices=None, normals=None):
    """What `Mesh.decimate` and `decimate_mesh` check before the device: (cell float, origin float64 [3] or None, placement
    0 / 1, n_vertices, triangles int32 [nt,3], vertices float64 [nv,3], normals float32 [nv,3]) or ValueError.  The arrays
    stay None where they are not given; n_vertices is taken from vertices when those are given."""
    if not (isinstance(cell, Real) and not isinstance(cell, bool) and np.isfinite(cell) and cell > 0):
        raise ValueError("cell must be a finite number > 0")
    if origin is not None:
        try:
            origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("origin must be None or 3 finite numbers") from None
        if origin.shape != (3,) or not np.isfinite(origin).all():
            raise ValueError("origin must be None or 3 finite numbers")
    if not (isinstance(placement, str) and placement in PLACEMENTS):
        raise ValueError('placement must be "quadric" or "mean"')
    _, _, n_vertices, triangles, vertices, normals = check_clean_arguments(1, None, n_vertices, triangles, vertices, normals)
    if triangles is not None and len(triangles) > MAX_TRIANGLES:
        raise ValueError("at most (2^31 - 1) / 3 triangles")
    return float(cell), origin, PLACEMENTS[placement], n_vertices, triangles, vertices, normals


def _default_origin(d_vertices, n_vertices, cell):
    """The per-axis minimum of the finite coordinates, taken on the device (zeros when there is none); ValueError when their
    extent over cell reaches 2^21 on an axis."""
    import torch
    if n_vertices == 0:
        return np.zeros(3)
    v = d_vertices.reshape(-1)[:3 * n_vertices].reshape(-1, 3)
    finite = torch.isfinite(v)
    inf = torch.full_like(v, float("inf"))
    lo = torch.where(finite, v, inf).amin(0).cpu().numpy()
    hi = torch.where(finite, v, -inf).amax(0).cpu().numpy()
    lo = np.where(np.isfinite(lo), lo, 0.0)
    hi = np.where(np.isfinite(hi), hi, 0.0)
    with np.errstate(over="ignore"):
        if not (np.floor((hi - lo) / cell) < AXIS_CELLS).all():
            raise ValueError("the extent of the vertices over cell reaches 2^21 on an axis: a larger cell")
    return np.ascontiguousarray(lo, dtype=np.float64)


def _decimate(dev, n_vertices, n_triangles, d_vertices, d_normals, d_triangles, cell, origin, placement):
    """The three device calls: (state, n_clusters, n_kept, counts) with counts = dict(n_unsound_vertices, n_unsound_triangles,
    n_degenerate, n_cancelled); the state holds vertices, normals, triangles, vertex_cluster, cluster_start, cluster_first,
    cluster_size, cluster_placed, triangle_keep and triangle_map on the device."""
    import torch
    h = _lib.get_handle(dev.index)
    nv, nt = int(n_vertices), int(n_triangles)
    origin = np.ascontiguousarray(origin, dtype=np.float64)
    need = C.c_int64()
    h.call("sfm_mesh_decimate_workspace_bytes", nv, nt, C.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    per = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    m = {"vertex_cluster": per(nv), "cluster_start": per(nv + 1), "cluster_first": per(nv), "cluster_size": per(nv),
         "triangle_keep": torch.empty(max(nt, 1), dtype=torch.uint8, device=dev)}
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    h.call("sfm_mesh_decimate_cluster", nv, nt, _dp(d_vertices), _hp(origin), C.c_double(cell), _dp(m["vertex_cluster"]), _dp(m["cluster_start"]),
           _dp(m["cluster_first"]), _dp(m["cluster_size"]), _dp(counts), _dp(ws), need.value)
    nc, bad_vertices = (int(c) for c in counts.cpu().numpy())    # waits for the call: the count sizes the sorts of the next
    marks = torch.empty(5, dtype=torch.int64, device=dev)
    h.call("sfm_mesh_decimate_mark", nv, nt, nc, _dp(d_triangles), _dp(m["vertex_cluster"]), _dp(m["triangle_keep"]), _dp(marks), _dp(ws), need.value)
    kept, bad_triangles, degenerate, dropped, status = (int(c) for c in marks.cpu().numpy())       # the counts size the outputs
    if status != 0:
        raise RuntimeError("sfm_mesh_decimate_mark: vertex_cluster is not that of sfm_mesh_decimate_cluster")
    m.update({"vertices": torch.empty((max(nc, 1), 3), dtype=torch.float64, device=dev),
              "normals": torch.zeros((max(nc, 1), 3), dtype=torch.float32, device=dev),
              "cluster_placed": torch.empty(max(nc, 1), dtype=torch.uint8, device=dev),
              "triangles": torch.empty((max(kept, 1), 3), dtype=torch.int32, device=dev), "triangle_map": per(kept)})
    h.call("sfm_mesh_decimate_emit", nv, nt, nc, _dp(d_vertices), _dp(d_normals), _dp(d_triangles), _dp(m["vertex_cluster"]), _dp(m["cluster_start"]),
           _dp(m["triangle_keep"]), _hp(origin), C.c_double(cell), int(placement), nc, kept, _dp(m["vertices"]), _dp(m["normals"]),
           _dp(m["cluster_placed"]), _dp(m["triangles"]), _dp(m["triangle_map"]), _dp(ws), need.value)
    m["decimate_ws"] = (ws, d_vertices, d_normals, d_triangles)   # alive while the call may still run
    return m, nc, kept, dict(n_unsound_vertices=bad_vertices, n_unsound_triangles=bad_triangles, n_degenerate=degenerate, n_cancelled=dropped)


def _decimated_mesh(m, nc, kept, counts, n_source_vertices, cell, origin, volume):
    from .mesh import Mesh
    out = Mesh(m, nc, kept, volume)
    out.n_source_vertices = int(n_source_vertices)
    out.n_unsound_vertices, out.n_unsound_triangles = counts["n_unsound_vertices"], counts["n_unsound_triangles"]
    out.n_degenerate, out.n_cancelled = counts["n_degenerate"], counts["n_cancelled"]
    out.cell, out.origin = float(cell), np.array(origin, dtype=np.float64)
    return out


def decimate(mesh, cell=None, factor=2.0, origin=None, placement="quadric"):
    """What `Mesh.decimate` does."""
    if cell is None:
        if not (isinstance(factor, Real) and not isinstance(factor, bool) and np.isfinite(factor) and factor > 0):
            raise ValueError("factor must be a finite number > 0")
        if mesh._volume is None:
            raise ValueError("decimate() needs cell: the mesh has no volume")
        cell = float(factor) * float(mesh._volume.voxel)
    cell, origin, placement = check_decimate_arguments(cell, origin, placement)[:3]
    src = mesh._m
    dev = src["vertices"].device
    if origin is None:
        origin = _default_origin(src["vertices"], mesh.n_vertices, cell)
    m, nc, kept, counts = _decimate(dev, mesh.n_vertices, mesh.n_triangles, src["vertices"], src["normals"], src["triangles"], cell, origin, placement)
    m["decimate_src"] = src
    return _decimated_mesh(m, nc, kept, counts, mesh.n_vertices, cell, origin, mesh._volume)


def decimate_mesh(vertices, triangles, normals=None, cell=None, origin=None, placement="quadric", device=0):
    """The three decimation calls on arrays that were made elsewhere: vertices float64 [nv,3], triangles int32 [nt,3], normals
    float32 [nv,3] or None (zeros), cell (required), origin [3] or None (the per-axis minimum of the finite coordinates; with
    an origin of the caller's a vertex outside the 2^21 cells of an axis is unsound, with None such an extent is a
    ValueError).  Returns a `Mesh` without a volume, with vertex_cluster, cluster_first, cluster_size, cluster_placed,
    triangle_map, the four counts, cell and origin."""
    import torch
    if vertices is None:
        raise ValueError("vertices must be [nv,3]")
    if cell is None:
        raise ValueError("cell must be a finite number > 0")
    cell, origin, placement, nv, tri, vertices, normals = check_decimate_arguments(
        cell, origin, placement, None, np.zeros((0, 3), np.int32) if triangles is None else triangles, vertices, normals)
    if normals is None:
        normals = np.zeros((nv, 3), np.float32)
    _lib.get_handle(device)
    dev = torch.device("cuda", device)
    d_v, d_n, d_t = _up(dev, vertices), _up(dev, normals), _up(dev, tri)
    if origin is None:
        origin = _default_origin(d_v, nv, cell)
    m, nc, kept, counts = _decimate(dev, nv, len(tri), d_v, d_n, d_t, cell, origin, placement)
    return _decimated_mesh(m, nc, kept, counts, nv, cell, origin, None)
