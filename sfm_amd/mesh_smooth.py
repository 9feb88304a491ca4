"""The vertex adjacency of a mesh, Taubin smoothing over it and area-weighted vertex normals on the device:
`sfm_mesh_adjacency`, `sfm_mesh_smooth` and `sfm_mesh_vertex_normals` (sfm_amd/csrc/mesh_smooth.hip); include/sfm_amd.h
states the rule completely.  The neighbours of a vertex are the other ends of its live half-edges in ascending index; a
vertex with an edge that is not used exactly twice is a boundary vertex.  One iteration moves every free vertex towards the
mean of its neighbours by lam and then, with mu, away from the new mean by |mu| (Taubin's lambda | mu pair, which keeps the
volume a plain Laplacian loses); boundary vertices, the caller's pinned ones, vertices that are not finite and vertices
without a neighbour stay.  The normals are the unit of the area-weighted sum of the face normals about each vertex.  A
function of its inputs, the same from run to run.  No CPU fallback: without the library or a GPU the calls raise.
"""
from __future__ import annotations

import ctypes as C
from numbers import Real

import numpy as np

from . import _lib
from ._lib import dp as _dp
from .mesh_clean import _up, _whole, check_clean_arguments

MAX_TRIANGLES = 0x7FFFFFFF // 6
MAX_ITERATIONS = 1000
NORMALS = ("recompute", "keep")


def check_smooth_arguments(iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, pinned=None, normals="recompute", n_vertices=None, triangles=None,
                           vertices=None, vertex_normals=None):
    """What `Mesh.smooth`, `smooth_mesh`, `mesh_adjacency` and `mesh_vertex_normals` check before the device: (iterations, lam,
    mu or None, pin_boundary bool, pinned uint8 [nv] or None, normals, n_vertices, triangles int32 [nt,3], vertices float64
    [nv,3], vertex_normals float32 [nv,3]) or ValueError.  The arrays stay None where they are not given; n_vertices is taken
    from vertices when those are given."""
    if not (_whole(iterations) and 0 <= iterations <= MAX_ITERATIONS):
        raise ValueError(f"iterations must be an integer 0 .. {MAX_ITERATIONS}")
    number = lambda x: isinstance(x, Real) and not isinstance(x, bool) and np.isfinite(x)
    if not (number(lam) and 0 < lam <= 1):
        raise ValueError("lam must be a finite number with 0 < lam <= 1")
    if mu is not None and not (number(mu) and -2 <= mu < -lam):
        raise ValueError("mu must be None or a finite number with -2 <= mu < -lam")
    if not (isinstance(normals, str) and normals in NORMALS):
        raise ValueError('normals must be "recompute" or "keep"')
    _, _, n_vertices, triangles, vertices, vertex_normals = check_clean_arguments(1, None, n_vertices, triangles, vertices, vertex_normals)
    if triangles is not None and len(triangles) > MAX_TRIANGLES:
        raise ValueError("at most (2^31 - 1) / 6 triangles")
    if pinned is not None:
        try:
            pinned = np.asarray(pinned)
        except (TypeError, ValueError):
            raise ValueError("pinned must be None or uint8 / bool [nv]") from None
        if pinned.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)) or pinned.ndim != 1 or (n_vertices is not None and len(pinned) != n_vertices):
            raise ValueError("pinned must be None or uint8 / bool [nv]")
        pinned = np.ascontiguousarray(pinned).astype(np.uint8)
    return int(iterations), float(lam), None if mu is None else float(mu), bool(pin_boundary), pinned, normals, n_vertices, triangles, vertices, vertex_normals


class MeshAdjacency:
    """What `Mesh.adjacency` and `mesh_adjacency` return; the arrays stay on the device until they are asked for.  ptr int32
    [nv + 1], index int32 [n_entries] - the neighbours of v are index[ptr[v] : ptr[v + 1]], ascending -, vertex_flags uint8
    [nv] (bit 0: boundary, bit 1: isolated); n_entries, n_boundary_vertices, n_isolated, n_unsound_triangles."""

    def __init__(self, state, n_mesh_vertices, n_mesh_triangles, counts):
        self._m = state
        self.n_mesh_vertices, self.n_mesh_triangles = int(n_mesh_vertices), int(n_mesh_triangles)
        self.n_entries, self.n_boundary_vertices, self.n_isolated, self.n_unsound_triangles = (int(c) for c in counts[:4])
        self._host = {}

    def _get(self, name, n):
        if name not in self._host:
            self._host[name] = self._m[name].cpu().numpy()[:n]
        return self._host[name]

    ptr = property(lambda self: self._get("ptr", self.n_mesh_vertices + 1))
    index = property(lambda self: self._get("index", self.n_entries))
    vertex_flags = property(lambda self: self._get("vertex_flags", self.n_mesh_vertices))


def _adjacency(dev, n_vertices, n_triangles, d_triangles):
    """The device call: the triangles on the device.  Returns a `MeshAdjacency`."""
    import torch
    h = _lib.get_handle(dev.index)
    nv, nt = int(n_vertices), int(n_triangles)
    need = C.c_int64()
    h.call("sfm_mesh_adjacency_workspace_bytes", nv, nt, C.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    m = {"ptr": torch.empty(nv + 1, dtype=torch.int32, device=dev), "index": torch.empty(max(6 * nt, 1), dtype=torch.int32, device=dev),
         "vertex_flags": torch.empty(max(nv, 1), dtype=torch.uint8, device=dev), "counts": torch.empty(4, dtype=torch.int64, device=dev)}
    h.call("sfm_mesh_adjacency", nv, nt, _dp(d_triangles), _dp(m["ptr"]), _dp(m["index"]), _dp(m["vertex_flags"]), _dp(m["counts"]), _dp(ws), need.value)
    counts = [int(c) for c in m["counts"].cpu().numpy()]          # waits for the call
    m["held"] = (ws, d_triangles)
    return MeshAdjacency(m, nv, nt, counts)


def _smooth(dev, adjacency, n_vertices, d_vertices, iterations, lam, mu, pin_boundary, d_pinned):
    """The device call: (new vertices, vertex_state, counts) with counts = [n_pinned_boundary, n_pinned_given,
    n_unsound_vertices, n_isolated]."""
    import torch
    h = _lib.get_handle(dev.index)
    nv = int(n_vertices)
    need = C.c_int64()
    h.call("sfm_mesh_smooth_workspace_bytes", nv, C.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    out = torch.empty((max(nv, 1), 3), dtype=torch.float64, device=dev)
    state = torch.empty(max(nv, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(5, dtype=torch.int64, device=dev)
    a = adjacency._m
    h.call("sfm_mesh_smooth", nv, _dp(d_vertices), _dp(a["ptr"]), _dp(a["index"]), int(adjacency.n_entries), _dp(a["vertex_flags"]),
           None if d_pinned is None else _dp(d_pinned), 1 if pin_boundary else 0, C.c_double(lam), C.c_double(0.0 if mu is None else mu),
           0 if mu is None else 1, int(iterations), _dp(out), _dp(state), _dp(counts), _dp(ws), need.value)
    got = [int(c) for c in counts.cpu().numpy()]                  # waits for the call
    if got[4] != 0:
        raise ValueError("sfm_mesh_smooth: the adjacency is not that of these triangles")
    return out, state, got[:4], (ws, d_vertices, d_pinned, adjacency)


def _normals(dev, n_vertices, n_triangles, d_vertices, d_triangles):
    """The device call: normals float32 [max(nv, 1), 3] on the device."""
    import torch
    h = _lib.get_handle(dev.index)
    nv, nt = int(n_vertices), int(n_triangles)
    need = C.c_int64()
    h.call("sfm_mesh_vertex_normals_workspace_bytes", nv, nt, C.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    out = torch.zeros((max(nv, 1), 3), dtype=torch.float32, device=dev)
    h.call("sfm_mesh_vertex_normals", nv, nt, _dp(d_vertices), _dp(d_triangles), _dp(out), _dp(ws), need.value)
    return out, (ws, d_vertices, d_triangles)


def _check_adjacency(n_vertices, n_triangles, adjacency):
    if not isinstance(adjacency, MeshAdjacency) or (adjacency.n_mesh_vertices, adjacency.n_mesh_triangles) != (n_vertices, n_triangles):
        raise ValueError("adjacency must be the MeshAdjacency of this mesh")


def adjacency_of(mesh):
    """What `Mesh.adjacency` does."""
    return _adjacency(mesh._m["vertices"].device, mesh.n_vertices, mesh.n_triangles, mesh._m["triangles"])


def _smoothed_mesh(dev, src, nv, nt, adjacency, iterations, lam, mu, pin_boundary, d_pinned, normals, volume):
    from .mesh import Mesh
    out, state, counts, held = _smooth(dev, adjacency, nv, src["vertices"], iterations, lam, mu, pin_boundary, d_pinned)
    m = {"vertices": out, "triangles": src["triangles"], "vertex_state": state, "smooth_held": held, "smooth_src": src}
    if normals == "keep":
        m["normals"] = src["normals"]
    else:
        m["normals"], m["normals_held"] = _normals(dev, nv, nt, out, src["triangles"])
    mesh = Mesh(m, nv, nt, volume)
    mesh.n_pinned_boundary, mesh.n_pinned_given, mesh.n_unsound_vertices, mesh.n_isolated = counts
    mesh.adjacency_before = adjacency
    return mesh


def smooth(mesh, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, pinned=None, normals="recompute", adjacency=None):
    """What `Mesh.smooth` does."""
    import torch
    iterations, lam, mu, pin_boundary, pinned, normals = check_smooth_arguments(iterations, lam, mu, pin_boundary, pinned, normals, mesh.n_vertices)[:6]
    if adjacency is None:
        adjacency = adjacency_of(mesh)
    else:
        _check_adjacency(mesh.n_vertices, mesh.n_triangles, adjacency)
    src = mesh._m
    dev = src["vertices"].device
    d_pinned = None if pinned is None else torch.from_numpy(np.concatenate([pinned, np.zeros(1, np.uint8)])).to(dev)
    return _smoothed_mesh(dev, src, mesh.n_vertices, mesh.n_triangles, adjacency, iterations, lam, mu, pin_boundary, d_pinned, normals, mesh._volume)


def recompute_normals(mesh):
    """What `Mesh.recompute_normals` does."""
    from .mesh import Mesh
    src = mesh._m
    dev = src["vertices"].device
    m = {"vertices": src["vertices"], "triangles": src["triangles"], "normals_src": src}
    m["normals"], m["normals_held"] = _normals(dev, mesh.n_vertices, mesh.n_triangles, src["vertices"], src["triangles"])
    return Mesh(m, mesh.n_vertices, mesh.n_triangles, mesh._volume)


def mesh_adjacency(triangles, n_vertices, device=0):
    """`sfm_mesh_adjacency` on an array that was made elsewhere: triangles int32 [nt,3], n_vertices.  Returns a
    `MeshAdjacency`; a triangle with an index outside 0 .. n_vertices - 1 has no live half-edge and is counted in its
    n_unsound_triangles."""
    import torch
    if n_vertices is None:
        raise ValueError("n_vertices must be an integer 0 .. 2^31 - 1")
    got = check_smooth_arguments(n_vertices=n_vertices, triangles=np.zeros((0, 3), np.int32) if triangles is None else triangles)
    n_vertices, tri = got[6], got[7]
    _lib.get_handle(device)
    dev = torch.device("cuda", device)
    return _adjacency(dev, n_vertices, len(tri), _up(dev, tri))


def mesh_vertex_normals(vertices, triangles, device=0):
    """`sfm_mesh_vertex_normals` on arrays that were made elsewhere: vertices float64 [nv,3], triangles int32 [nt,3].  Returns
    normals float32 [nv,3] on the host: unit, area-weighted, zeros where the sum has no finite positive length."""
    import torch
    if vertices is None:
        raise ValueError("vertices must be [nv,3]")
    got = check_smooth_arguments(triangles=np.zeros((0, 3), np.int32) if triangles is None else triangles, vertices=vertices)
    nv, tri, vertices = got[6], got[7], got[8]
    _lib.get_handle(device)
    dev = torch.device("cuda", device)
    out, _ = _normals(dev, nv, len(tri), _up(dev, vertices), _up(dev, tri))
    return out.cpu().numpy()[:nv]


def smooth_mesh(vertices, triangles, normals=None, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, pinned=None, normals_mode="recompute", device=0):
    """`sfm_mesh_adjacency`, `sfm_mesh_smooth` and `sfm_mesh_vertex_normals` on arrays that were made elsewhere: vertices
    float64 [nv,3], triangles int32 [nt,3], normals float32 [nv,3] or None (zeros; they matter with normals_mode = "keep" only),
    pinned uint8 / bool [nv] or None.  Returns a `Mesh` without a volume, with vertex_state, the four counts and
    adjacency_before."""
    import torch
    if vertices is None:
        raise ValueError("vertices must be [nv,3]")
    iterations, lam, mu, pin_boundary, pinned, normals_mode, nv, tri, vertices, normals = check_smooth_arguments(
        iterations, lam, mu, pin_boundary, pinned, normals_mode, None, np.zeros((0, 3), np.int32) if triangles is None else triangles, vertices, normals)
    if pinned is not None and len(pinned) != nv:
        raise ValueError("pinned must be None or uint8 / bool [nv]")
    if normals is None:
        normals = np.zeros((nv, 3), np.float32)
    _lib.get_handle(device)
    dev = torch.device("cuda", device)
    from .mesh import upload_rows
    src = {"vertices": upload_rows(vertices, dev), "normals": upload_rows(normals, dev), "triangles": upload_rows(tri, dev)}       # one row more
    adjacency = _adjacency(dev, nv, len(tri), src["triangles"])
    d_pinned = None if pinned is None else _up(dev, pinned)
    return _smoothed_mesh(dev, src, nv, len(tri), adjacency, iterations, lam, mu, pin_boundary, d_pinned, normals_mode, None)
