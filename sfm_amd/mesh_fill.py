"""The edge table of a mesh, its boundary loops and the filling of the small holes on the device: `sfm_mesh_edges` and
`sfm_mesh_fill_mark` / `sfm_mesh_fill_emit` (sfm_amd/csrc/mesh_fill.hip); include/sfm_amd.h states the rule completely.
Half-edge h = 3 t + k of triangle t runs from tri[t][k] to tri[t][(k + 1) % 3]; an edge is boundary when one live half-edge
uses it, inconsistent when two use it in the same direction, non-manifold when more than two do.  A boundary half-edge's
successor is found by rotating about its end inside the surface; a cycle of at most 64 successors is a short loop; a loop
that passes a vertex twice - two holes that touch - is split there; every sub-loop of 3 .. max_edges edges is closed by a
fan about the mean of its vertices.  Longer boundary cycles - an outline is one - stay open and are counted by their edges.
The outline of a lone fragment is a short loop too: `Mesh.clean` first.  No CPU fallback: without the library or a GPU the
calls raise.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import dp as _dp
from .mesh_clean import _up, _whole, check_clean_arguments

MAX_EDGES = 64
MAX_TRIANGLES = 0x7FFFFFFF // 3


def check_fill_arguments(max_edges=16, n_vertices=None, triangles=None, vertices=None, normals=None):
    """What `Mesh.fill_holes`, `fill_mesh_holes` and `mesh_edges` check before the device: (max_edges, n_vertices, triangles
    int32 [nt,3], vertices float64 [nv,3], normals float32 [nv,3]) or ValueError.  The arrays stay None where they are not
    given; n_vertices is taken from vertices when those are given."""
    if not (_whole(max_edges) and 1 <= max_edges <= MAX_EDGES):
        raise ValueError(f"max_edges must be an integer 1 .. {MAX_EDGES}")
    _, _, n_vertices, triangles, vertices, normals = check_clean_arguments(1, None, n_vertices, triangles, vertices, normals)
    if triangles is not None and len(triangles) > MAX_TRIANGLES:
        raise ValueError("at most (2^31 - 1) / 3 triangles")
    return int(max_edges), n_vertices, triangles, vertices, normals


class MeshEdges:
    """What `Mesh.edges` and `mesh_edges` return; the arrays stay on the device until they are asked for.  n_edges (distinct
    live edges), n_boundary_edges, n_inconsistent_edges, n_nonmanifold_edges, n_loops (short loops: boundary cycles of at
    most 64 edges), n_long_boundary_edges (boundary half-edges on no short loop), n_unsound (triangles with an index outside
    0 .. nv - 1); halfedge_uses, halfedge_twin, halfedge_next and halfedge_loop int32 [3 nt]; loop_leader and loop_edges int32
    [n_loops]."""

    def __init__(self, state, n_mesh_vertices, n_mesh_triangles, counts, triangles=None):
        self._m = state
        self.n_mesh_vertices, self.n_mesh_triangles = int(n_mesh_vertices), int(n_mesh_triangles)
        (self.n_edges, self.n_boundary_edges, self.n_inconsistent_edges, self.n_nonmanifold_edges, self.n_loops, self.n_long_boundary_edges,
         self.n_unsound) = (int(c) for c in counts[:7])
        self._triangles = triangles                                # a callable: the triangles on the host, for euler
        self._host = {}

    def _get(self, name, n):
        if name not in self._host:
            self._host[name] = self._m[name].cpu().numpy()[:n]
        return self._host[name]

    halfedge_uses = property(lambda self: self._get("halfedge_uses", 3 * self.n_mesh_triangles))
    halfedge_twin = property(lambda self: self._get("halfedge_twin", 3 * self.n_mesh_triangles))
    halfedge_next = property(lambda self: self._get("halfedge_next", 3 * self.n_mesh_triangles))
    halfedge_loop = property(lambda self: self._get("halfedge_loop", 3 * self.n_mesh_triangles))
    loop_leader = property(lambda self: self._get("loop_leader", self.n_loops))
    loop_edges = property(lambda self: self._get("loop_edges", self.n_loops))

    @property
    def is_closed(self):
        """No boundary, no inconsistent and no non-manifold edge, and no unsound triangle."""
        return self.n_boundary_edges == 0 and self.n_inconsistent_edges == 0 and self.n_nonmanifold_edges == 0 and self.n_unsound == 0

    @property
    def euler(self):
        """V - E + F: V the vertices that some sound triangle uses (counted on the host), E the distinct live edges, F the
        sound triangles."""
        if "euler" not in self._host:
            tri = np.asarray(self._triangles(), dtype=np.int64).reshape(-1, 3)
            ok = ((tri >= 0) & (tri < self.n_mesh_vertices)).all(axis=1)
            self._host["euler"] = int(len(np.unique(tri[ok])) - self.n_edges + int(ok.sum()))
        return self._host["euler"]


def _edges(dev, n_vertices, n_triangles, d_triangles, host_triangles):
    """The device call: the triangles on the device.  Returns a `MeshEdges`."""
    import torch
    h = _lib.get_handle(dev.index)
    nv, nt = int(n_vertices), int(n_triangles)
    need = C.c_int64()
    h.call("sfm_mesh_edges_workspace_bytes", nt, C.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    per = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    m = {"halfedge_uses": per(3 * nt), "halfedge_twin": per(3 * nt), "halfedge_next": per(3 * nt), "halfedge_loop": per(3 * nt),
         "loop_leader": per(nt), "loop_edges": per(nt), "counts": torch.empty(8, dtype=torch.int64, device=dev)}
    h.call("sfm_mesh_edges", nv, nt, _dp(d_triangles), _dp(m["halfedge_uses"]), _dp(m["halfedge_twin"]), _dp(m["halfedge_next"]),
           _dp(m["halfedge_loop"]), _dp(m["loop_leader"]), _dp(m["loop_edges"]), _dp(m["counts"]), _dp(ws), need.value)
    counts = [int(c) for c in m["counts"].cpu().numpy()]          # waits for the call
    if counts[7] != 0:
        raise RuntimeError("sfm_mesh_edges: a rotation about a vertex ran out of its step budget")
    m["held"] = (ws, d_triangles)
    return MeshEdges(m, nv, nt, counts, host_triangles)


def _fill(dev, edges, n_vertices, n_triangles, d_triangles, d_vertices, max_edges):
    """The two device calls on a mesh with its edge table: (state, n_filled, n_fill_triangles, n_open); the state holds
    halfedge_fill, fill_vertices, fill_normals, fill_name, fill_triangles and fill_triangle_halfedge on the device."""
    import torch
    h = _lib.get_handle(dev.index)
    nv, nt, nl = int(n_vertices), int(n_triangles), int(edges.n_loops)
    need = C.c_int64()
    h.check(h.lib.sfm_mesh_fill_workspace_bytes(nt, C.byref(need)), "sfm_mesh_fill_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    flags = torch.empty(max(3 * nt, 1), dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    e = edges._m
    h.call("sfm_mesh_fill_mark", nv, nt, _dp(d_triangles), _dp(e["halfedge_next"]), nl, _dp(e["loop_leader"]), int(max_edges), _dp(flags), _dp(counts),
           _dp(ws), need.value)
    filled, n_tri, n_open, status = (int(c) for c in counts.cpu().numpy())       # waits for the mark call: the counts size the outputs
    if status != 0:
        raise ValueError("sfm_mesh_fill_mark: the edge table is not that of these triangles")
    if nv + filled > 0x7FFFFFFF:
        raise ValueError("the filled mesh would have more than 2^31 - 1 vertices")
    m = {"halfedge_fill": flags, "fill_vertices": torch.empty((max(filled, 1), 3), dtype=torch.float64, device=dev),
         "fill_normals": torch.empty((max(filled, 1), 3), dtype=torch.float32, device=dev),
         "fill_name": torch.empty(max(filled, 1), dtype=torch.int32, device=dev),
         "fill_triangles": torch.empty((max(n_tri, 1), 3), dtype=torch.int32, device=dev),
         "fill_triangle_halfedge": torch.empty(max(n_tri, 1), dtype=torch.int32, device=dev)}
    h.call("sfm_mesh_fill_emit", nv, nt, _dp(d_triangles), _dp(e["halfedge_next"]), nl, _dp(e["loop_leader"]), _dp(flags), _dp(d_vertices), filled, n_tri,
           _dp(m["fill_vertices"]), _dp(m["fill_normals"]), _dp(m["fill_name"]), _dp(m["fill_triangles"]), _dp(m["fill_triangle_halfedge"]), _dp(ws),
           need.value)
    m["fill_ws"] = (ws, d_triangles, d_vertices, edges)            # alive while the call may still run
    return m, filled, n_tri, n_open


def _check_edges(mesh, edges):
    if not isinstance(edges, MeshEdges) or (edges.n_mesh_vertices, edges.n_mesh_triangles) != (mesh.n_vertices, mesh.n_triangles):
        raise ValueError("edges must be the MeshEdges of this mesh")


def edges_of(mesh):
    """What `Mesh.edges` does."""
    return _edges(mesh._m["vertices"].device, mesh.n_vertices, mesh.n_triangles, mesh._m["triangles"], lambda: mesh.triangles)


def _filled_mesh(dev, src, nv, nt, m, filled, n_tri, n_open, volume, edges):
    """The `Mesh` of the old arrays with the patches behind them."""
    import torch
    from .mesh import Mesh
    out = dict(m)
    for name, new, old_n, new_n in (("vertices", "fill_vertices", nv, filled), ("normals", "fill_normals", nv, filled),
                                    ("triangles", "fill_triangles", nt, n_tri)):
        joined = torch.cat([src[name].reshape(-1)[:3 * old_n].reshape(-1, 3), m[new][:new_n]])
        out[name] = joined if len(joined) else torch.zeros((1, 3), dtype=joined.dtype, device=dev)
    out["fill_src"] = src                                          # alive while the copies may still run
    mesh = Mesh(out, nv + filled, nt + n_tri, volume)
    mesh.fill_vertex_start, mesh.fill_triangle_start, mesh.n_filled, mesh.n_fill_triangles, mesh.n_open = nv, nt, filled, n_tri, n_open
    mesh.edges_before = edges
    return mesh


def fill_holes(mesh, max_edges=16, edges=None):
    """What `Mesh.fill_holes` does."""
    max_edges = check_fill_arguments(max_edges)[0]
    if edges is None:
        edges = edges_of(mesh)
    else:
        _check_edges(mesh, edges)
    src = mesh._m
    dev = src["vertices"].device
    m, filled, n_tri, n_open = _fill(dev, edges, mesh.n_vertices, mesh.n_triangles, src["triangles"], src["vertices"], max_edges)
    return _filled_mesh(dev, src, mesh.n_vertices, mesh.n_triangles, m, filled, n_tri, n_open, mesh._volume, edges)


def mesh_edges(triangles, n_vertices, device=0):
    """`sfm_mesh_edges` on an array that was made elsewhere: triangles int32 [nt,3], n_vertices.  Returns a `MeshEdges`; a
    triangle with an index outside 0 .. n_vertices - 1 has no live half-edge and is counted in its n_unsound."""
    import torch
    if n_vertices is None:
        raise ValueError("n_vertices must be an integer 0 .. 2^31 - 1")
    _, n_vertices, tri, _, _ = check_fill_arguments(n_vertices=n_vertices, triangles=np.zeros((0, 3), np.int32) if triangles is None else triangles)
    _lib.get_handle(device)
    dev = torch.device("cuda", device)
    return _edges(dev, n_vertices, len(tri), _up(dev, tri), lambda: tri)


def fill_mesh_holes(vertices, triangles, normals=None, max_edges=16, device=0):
    """`sfm_mesh_edges` and `sfm_mesh_fill_mark` / `sfm_mesh_fill_emit` on arrays that were made elsewhere: vertices float64
    [nv,3], triangles int32 [nt,3], normals float32 [nv,3] or None (zeros).  Returns a `Mesh` without a volume: the old
    arrays with the patches behind them, with fill_vertex_start, fill_triangle_start, n_filled, n_fill_triangles,
    fill_triangle_halfedge and edges_before."""
    import torch
    if vertices is None:
        raise ValueError("vertices must be [nv,3]")
    max_edges, nv, tri, vertices, normals = check_fill_arguments(max_edges, None, np.zeros((0, 3), np.int32) if triangles is None else triangles,
                                                                 vertices, normals)
    if normals is None:
        normals = np.zeros((nv, 3), np.float32)
    _lib.get_handle(device)
    dev = torch.device("cuda", device)
    nt = len(tri)
    src = {"vertices": _up(dev, vertices), "normals": _up(dev, normals), "triangles": _up(dev, tri)}      # flat, one element more
    edges = _edges(dev, nv, nt, src["triangles"], lambda: tri)
    m, filled, n_tri, n_open = _fill(dev, edges, nv, nt, src["triangles"], src["vertices"], max_edges)
    return _filled_mesh(dev, src, nv, nt, m, filled, n_tri, n_open, None, edges)
