"""The connected components of a mesh and the removal of the small ones on the device: `sfm_mesh_components`,
`sfm_mesh_clean_mark` / `sfm_mesh_clean_emit` and `sfm_mesh_gather_rows` (sfm_amd/csrc/mesh_clean.hip); include/sfm_amd.h
states the rule completely.  Vertices are the nodes and every triangle joins its three; components are numbered by their
smallest vertex; a component stays when it has at least min_triangles triangles and, with keep_largest, is among that many
with the most triangles (ties go to the lower component number); kept vertices and triangles keep their order.  Integers
only: every output byte is a function of the inputs.  No CPU fallback: without the library or a GPU the calls raise.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import dp as _dp

MAX_COUNT = 0x7FFFFFFF


def _whole(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def check_clean_arguments(min_triangles=1, keep_largest=None, n_vertices=None, triangles=None, vertices=None, normals=None):
    """What `Mesh.clean`, `clean_mesh` and `mesh_components` check before the device: (min_triangles, keep_largest with None
    as 0, n_vertices, triangles int32 [nt,3], vertices float64 [nv,3], normals float32 [nv,3]) or ValueError.  The arrays
    stay None where they are not given; n_vertices is taken from vertices when those are given."""
    if not (_whole(min_triangles) and 0 <= min_triangles <= MAX_COUNT):
        raise ValueError("min_triangles must be an integer 0 .. 2^31 - 1")
    if keep_largest is not None and not (_whole(keep_largest) and 1 <= keep_largest <= MAX_COUNT):
        raise ValueError("keep_largest must be None or an integer 1 .. 2^31 - 1")
    if vertices is not None:
        try:
            vertices = np.ascontiguousarray(vertices, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("vertices must be [nv,3]") from None
        if vertices.ndim != 2 or vertices.shape[1] != 3:
            raise ValueError("vertices must be [nv,3]")
        if n_vertices is not None and n_vertices != len(vertices):
            raise ValueError("n_vertices is not the number of vertices")
        n_vertices = len(vertices)
    if n_vertices is not None and not (_whole(n_vertices) and 0 <= n_vertices <= MAX_COUNT):
        raise ValueError("n_vertices must be an integer 0 .. 2^31 - 1")
    if normals is not None:
        try:
            normals = np.ascontiguousarray(normals, dtype=np.float32)
        except (TypeError, ValueError):
            raise ValueError("normals must be [nv,3]") from None
        if vertices is None or normals.shape != vertices.shape:
            raise ValueError("normals must be [nv,3], one row per vertex")
    if triangles is not None:
        try:
            tri = np.asarray(triangles)
        except (TypeError, ValueError):
            raise ValueError("triangles must be [nt,3] integers that fit int32") from None
        if tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu" or (tri.size and (tri.min() < -0x80000000 or tri.max() > 0x7FFFFFFF)):
            raise ValueError("triangles must be [nt,3] integers that fit int32")
        if len(tri) > MAX_COUNT:
            raise ValueError("at most 2^31 - 1 triangles")
        triangles = np.ascontiguousarray(tri, dtype=np.int32)
    return int(min_triangles), 0 if keep_largest is None else int(keep_largest), None if n_vertices is None else int(n_vertices), triangles, vertices, normals


class MeshComponents:
    """What `Mesh.components` and `mesh_components` return; the arrays stay on the device until they are asked for.
    n_components; vertex_component int32 [nv] and triangle_component int32 [nt] (-1 for an unsound triangle, one with an index
    outside 0 .. nv - 1); per component root (its smallest vertex, ascending), n_vertices and n_triangles, int32
    [n_components]; n_unsound, the unsound triangles the call counted."""

    def __init__(self, state, n_mesh_vertices, n_mesh_triangles, n_components, n_unsound):
        self._m = state
        self.n_mesh_vertices, self.n_mesh_triangles = int(n_mesh_vertices), int(n_mesh_triangles)
        self.n_components, self.n_unsound = int(n_components), int(n_unsound)
        self._host = {}

    def _get(self, name, n):
        if name not in self._host:
            self._host[name] = self._m[name].cpu().numpy()[:n]
        return self._host[name]

    vertex_component = property(lambda self: self._get("vertex_component", self.n_mesh_vertices))
    triangle_component = property(lambda self: self._get("triangle_component", self.n_mesh_triangles))
    root = property(lambda self: self._get("comp_root", self.n_components))
    n_vertices = property(lambda self: self._get("comp_vertices", self.n_components))
    n_triangles = property(lambda self: self._get("comp_triangles", self.n_components))

    def largest(self, k=1):
        """The numbers of the k components with the most triangles, largest first; equal sizes in component order."""
        if not (_whole(k) and k >= 0):
            raise ValueError("k must be an integer >= 0")
        order = np.argsort(-self.n_triangles.astype(np.int64), kind="stable")
        return [int(c) for c in order[:k]]


def _components(dev, n_vertices, n_triangles, d_triangles):
    """The device call: the triangles on the device.  Returns a `MeshComponents`."""
    import torch
    h = _lib.get_handle(dev.index)
    need = C.c_int64()
    h.check(h.lib.sfm_mesh_components_workspace_bytes(int(n_vertices), C.byref(need)), "sfm_mesh_components_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    nv, nt = max(int(n_vertices), 1), max(int(n_triangles), 1)
    m = {"vertex_component": torch.empty(nv, dtype=torch.int32, device=dev), "triangle_component": torch.empty(nt, dtype=torch.int32, device=dev),
         "comp_root": torch.empty(nv, dtype=torch.int32, device=dev), "comp_vertices": torch.empty(nv, dtype=torch.int32, device=dev),
         "comp_triangles": torch.empty(nv, dtype=torch.int32, device=dev), "counts": torch.empty(3, dtype=torch.int64, device=dev)}
    h.call("sfm_mesh_components", int(n_vertices), int(n_triangles), _dp(d_triangles), _dp(m["vertex_component"]), _dp(m["triangle_component"]),
           _dp(m["comp_root"]), _dp(m["comp_vertices"]), _dp(m["comp_triangles"]), _dp(m["counts"]), _dp(ws), need.value)
    n_components, n_unsound, _ = (int(c) for c in m["counts"].cpu().numpy())
    m["held"] = (ws, d_triangles)
    return MeshComponents(m, n_vertices, n_triangles, n_components, n_unsound)


def _gather(dev, d_src, row_bytes, d_map, n):
    """`sfm_mesh_gather_rows`: the rows d_map[0 .. n) of d_src, as a tensor shaped and typed like d_src with n rows (at least
    one is allocated)."""
    import torch
    h = _lib.get_handle(dev.index)
    out = torch.empty((max(int(n), 1),) + tuple(d_src.shape[1:]), dtype=d_src.dtype, device=dev)
    h.call("sfm_mesh_gather_rows", _dp(d_src), int(row_bytes), _dp(d_map), int(n), _dp(out))
    return out


def _clean(dev, comps, n_vertices, n_triangles, d_triangles, d_vertices, d_normals, min_triangles, keep_largest):
    """The two device calls on a labelled mesh: (state, n_vertices, n_triangles, n_kept_components); the state holds
    vertices, normals, triangles, vertex_map, triangle_map and comp_keep on the device."""
    import torch
    h = _lib.get_handle(dev.index)
    nv, nt, nc = int(n_vertices), int(n_triangles), int(comps.n_components)
    need = C.c_int64()
    h.check(h.lib.sfm_mesh_clean_workspace_bytes(nv, nt, C.byref(need)), "sfm_mesh_clean_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    keep = torch.empty(max(nc, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    c = comps._m
    h.call("sfm_mesh_clean_mark", nv, nt, nc, _dp(c["vertex_component"]), _dp(c["triangle_component"]), _dp(c["comp_triangles"]), int(min_triangles),
           int(keep_largest), _dp(keep), _dp(counts), _dp(ws), need.value)
    kept, nv2, nt2 = (int(v) for v in counts.cpu().numpy())        # waits for the mark call: the counts size the outputs
    m = {"vertices": torch.empty((max(nv2, 1), 3), dtype=torch.float64, device=dev),
         "normals": torch.empty((max(nv2, 1), 3), dtype=torch.float32, device=dev),
         "triangles": torch.empty((max(nt2, 1), 3), dtype=torch.int32, device=dev),
         "vertex_map": torch.empty(max(nv2, 1), dtype=torch.int32, device=dev),
         "triangle_map": torch.empty(max(nt2, 1), dtype=torch.int32, device=dev), "comp_keep": keep}
    h.call("sfm_mesh_clean_emit", nv, nt, nc, _dp(c["vertex_component"]), _dp(c["triangle_component"]), _dp(keep), _dp(d_triangles), _dp(d_vertices),
           _dp(d_normals), nv2, nt2, _dp(m["vertex_map"]), _dp(m["triangle_map"]), _dp(m["triangles"]), _dp(m["vertices"]), _dp(m["normals"]),
           _dp(ws), need.value)
    m["clean_ws"] = (ws, d_triangles, d_vertices, d_normals)      # alive while the call may still run
    return m, nv2, nt2, kept


def components_of(mesh):
    """What `Mesh.components` does."""
    comps = _components(mesh._m["vertices"].device, mesh.n_vertices, mesh.n_triangles, mesh._m["triangles"])
    if comps.n_unsound:
        raise ValueError(f"{comps.n_unsound} triangles have an index outside 0 .. n_vertices - 1")
    return comps


def clean(mesh, min_triangles=1, keep_largest=None, components=None):
    """What `Mesh.clean` does."""
    from .mesh import Mesh
    min_triangles, keep_largest = check_clean_arguments(min_triangles, keep_largest)[:2]
    if components is None:
        components = components_of(mesh)
    elif not isinstance(components, MeshComponents) or (components.n_mesh_vertices, components.n_mesh_triangles) != (mesh.n_vertices, mesh.n_triangles):
        raise ValueError("components must be the MeshComponents of this mesh")
    src = mesh._m
    dev = src["vertices"].device
    m, nv, nt, _ = _clean(dev, components, mesh.n_vertices, mesh.n_triangles, src["triangles"], src["vertices"], src["normals"], min_triangles,
                          keep_largest)
    for name in ("vertex_colors", "n_views", "best_view"):
        if name in src:
            t = src[name]
            m[name] = _gather(dev, t, t.element_size() * (t.shape[1] if t.ndim == 2 else 1), m["vertex_map"], nv)
    m["clean_src"] = src                                           # alive while the gathers may still run
    out = Mesh(m, nv, nt, mesh._volume)
    out.components_before = components
    return out


def _up(dev, a):
    """A host array on the device with one element more: a pointer must exist."""
    import torch
    return torch.from_numpy(np.concatenate([a.reshape(-1), np.zeros(1, a.dtype)])).to(dev)


def mesh_components(triangles, n_vertices, device=0):
    """`sfm_mesh_components` on an array that was made elsewhere: triangles int32 [nt,3], n_vertices.  Returns a
    `MeshComponents`; a triangle with an index outside 0 .. n_vertices - 1 joins nothing, is labelled -1 and is counted in
    its n_unsound."""
    import torch
    if n_vertices is None:
        raise ValueError("n_vertices must be an integer 0 .. 2^31 - 1")
    _, _, n_vertices, tri, _, _ = check_clean_arguments(n_vertices=n_vertices, triangles=np.zeros((0, 3), np.int32) if triangles is None else triangles)
    _lib.get_handle(device)
    dev = torch.device("cuda", device)
    return _components(dev, n_vertices, len(tri), _up(dev, tri))


def clean_mesh(vertices, triangles, normals=None, min_triangles=1, keep_largest=None, device=0):
    """`sfm_mesh_clean_mark` / `sfm_mesh_clean_emit` on arrays that were made elsewhere: vertices float64 [nv,3], triangles
    int32 [nt,3], normals float32 [nv,3] or None (zeros).  An unsound triangle is dropped.  Returns a `Mesh` without a volume,
    with vertex_map, triangle_map and components_before."""
    import torch
    from .mesh import Mesh
    if vertices is None:
        raise ValueError("vertices must be [nv,3]")
    min_triangles, keep_largest, nv, tri, vertices, normals = check_clean_arguments(
        min_triangles, keep_largest, None, np.zeros((0, 3), np.int32) if triangles is None else triangles, vertices, normals)
    if normals is None:
        normals = np.zeros((nv, 3), np.float32)
    _lib.get_handle(device)
    dev = torch.device("cuda", device)
    d_tri = _up(dev, tri)
    comps = _components(dev, nv, len(tri), d_tri)
    m, nv2, nt2, _ = _clean(dev, comps, nv, len(tri), d_tri, _up(dev, vertices), _up(dev, normals), min_triangles, keep_largest)
    out = Mesh(m, nv2, nt2, None)
    out.components_before = comps
    return out
