"""The connected components of a mesh and the removal of the small ones, restated for the tests (include/sfm_amd.h states the
rule): the labelling twice, independently - SciPy's connected_components over the triangle edges, renumbered by smallest
vertex, and a plain union-find in loops - and the selection and the compaction in NumPy.  Integers only."""
from collections import namedtuple

import numpy as np

Components = namedtuple("Components", "n_components vertex_component triangle_component root n_vertices n_triangles n_unsound")
Cleaned = namedtuple("Cleaned", "keep vertex_map triangle_map triangles vertices normals")


def sound_mask(triangles, n_vertices):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return ((t >= 0) & (t < n_vertices)).all(axis=1)


def _tables(n_vertices, tri, ok, label_of_vertex):
    """Components from any labelling of the vertices (equal label = same component): renumbered by smallest vertex."""
    first = np.full(int(label_of_vertex.max()) + 1 if n_vertices else 0, n_vertices, np.int64)
    np.minimum.at(first, label_of_vertex, np.arange(n_vertices))
    roots = np.sort(first[first < n_vertices])
    number = np.full(n_vertices + 1, -1, np.int64)
    number[roots] = np.arange(len(roots))
    vc = number[first[label_of_vertex]] if n_vertices else np.zeros(0, np.int64)
    tc = np.full(len(tri), -1, np.int64)
    tc[ok] = vc[tri[ok, 0]]
    return Components(len(roots), vc.astype(np.int32), tc.astype(np.int32), roots.astype(np.int32),
                      np.bincount(vc, minlength=len(roots)).astype(np.int32), np.bincount(tc[ok], minlength=len(roots)).astype(np.int32),
                      int((~ok).sum()))


def components(triangles, n_vertices):
    """SciPy's connected_components over the edges (a, b) and (a, c) of every sound triangle."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    ok = sound_mask(tri, n_vertices)
    if n_vertices == 0:
        return _tables(0, tri, ok, np.zeros(0, np.int64))
    s = tri[ok]
    rows, cols = np.concatenate([s[:, 0], s[:, 0]]), np.concatenate([s[:, 1], s[:, 2]])
    graph = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n_vertices, n_vertices))
    _, labels = connected_components(graph, directed=False)
    return _tables(n_vertices, tri, ok, labels.astype(np.int64))


def components_loops(triangles, n_vertices):
    """A plain union-find, the larger root under the smaller, then everything counted in loops."""
    tri = [tuple(int(v) for v in t) for t in np.asarray(triangles, dtype=np.int64).reshape(-1, 3)]
    parent = list(range(n_vertices))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v

    ok = [all(0 <= v < n_vertices for v in t) for t in tri]
    for t, good in zip(tri, ok):
        if good:
            for other in t[1:]:
                a, b = find(t[0]), find(other)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    roots = [v for v in range(n_vertices) if find(v) == v]
    number = {r: c for c, r in enumerate(roots)}
    vc = [number[find(v)] for v in range(n_vertices)]
    tc = [vc[t[0]] if good else -1 for t, good in zip(tri, ok)]
    nv, nt = [0] * len(roots), [0] * len(roots)
    for c in vc:
        nv[c] += 1
    for c in tc:
        if c >= 0:
            nt[c] += 1
    i32 = lambda a: np.array(a, dtype=np.int32).reshape(-1)
    return Components(len(roots), i32(vc), i32(tc), i32(roots), i32(nv), i32(nt), ok.count(False))


def assert_same_components(a, b, what=""):
    assert a.n_components == b.n_components and a.n_unsound == b.n_unsound, (what, a.n_components, b.n_components, a.n_unsound, b.n_unsound)
    for name in ("vertex_component", "triangle_component", "root", "n_vertices", "n_triangles"):
        x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
        assert x.dtype == y.dtype == np.int32 and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), (what, name, int((x != y).sum()))


def select(n_triangles, min_triangles=1, keep_largest=None):
    """comp_keep uint8 [n_components]: the candidates, and with more than keep_largest of them the k largest by a stable sort -
    which is the cut: all above the k-th size, and the first of those at it in component order."""
    sizes = np.asarray(n_triangles, dtype=np.int64)
    cand = np.flatnonzero(sizes >= min_triangles)
    if keep_largest is not None and keep_largest > 0 and len(cand) > keep_largest:
        cand = cand[np.argsort(-sizes[cand], kind="stable")[:keep_largest]]
    keep = np.zeros(len(sizes), np.uint8)
    keep[cand] = 1
    return keep


def clean(comps, triangles, vertices=None, normals=None, min_triangles=1, keep_largest=None):
    """The selection and the compaction on a labelled mesh: a `Cleaned`."""
    tri = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    keep = select(comps.n_triangles, min_triangles, keep_largest)
    kv = keep[comps.vertex_component].astype(bool) if len(comps.vertex_component) else np.zeros(0, bool)
    tc = comps.triangle_component
    kt = np.zeros(len(tri), bool)
    kt[tc >= 0] = keep[tc[tc >= 0]].astype(bool)
    vertex_map = np.flatnonzero(kv).astype(np.int32)
    triangle_map = np.flatnonzero(kt).astype(np.int32)
    new_index = np.full(len(kv), -1, np.int32)
    new_index[vertex_map] = np.arange(len(vertex_map), dtype=np.int32)
    new_tri = new_index[tri[triangle_map].astype(np.int64)].reshape(-1, 3).astype(np.int32)
    v = None if vertices is None else np.ascontiguousarray(vertices, dtype=np.float64)[vertex_map]
    n = None if normals is None else np.ascontiguousarray(normals, dtype=np.float32)[vertex_map]
    return Cleaned(keep, vertex_map, triangle_map, new_tri, v, n)


# ------------------------------------------------------------------------------------------- cases
def hand_cases():
    """{name: (n_vertices, triangles, the vertex sets of the components in order, triangles per component)}."""
    return {
        "one triangle": (3, [(0, 1, 2)], [{0, 1, 2}], [1]),
        "two that share a vertex only": (5, [(0, 1, 2), (2, 3, 4)], [{0, 1, 2, 3, 4}], [2]),
        "two that share an edge": (4, [(0, 1, 2), (2, 1, 3)], [{0, 1, 2, 3}], [2]),
        "two that are disjoint": (6, [(3, 4, 5), (2, 0, 1)], [{0, 1, 2}, {3, 4, 5}], [1, 1]),
        "an isolated vertex": (5, [(0, 4, 2)], [{0, 2, 4}, {1}, {3}], [1, 0, 0]),
        "a repeated index": (4, [(2, 2, 3), (1, 1, 1), (0, 1, 0)], [{0, 1}, {2, 3}], [2, 1]),
    }


def random_soup(seed, n_vertices, n_triangles, spread=None):
    """Triangles whose indices lie within `spread` of a random centre: many components of many sizes, and loose vertices."""
    rng = np.random.default_rng(seed)
    if n_vertices == 0 or n_triangles == 0:
        return np.zeros((0, 3), np.int32)
    spread = max(n_vertices // 50, 2) if spread is None else spread
    centre = rng.integers(0, n_vertices, n_triangles)
    tri = (centre[:, None] // spread) * spread + rng.integers(0, spread, (n_triangles, 3))
    return np.minimum(tri, n_vertices - 1).astype(np.int32)


def strip(n_vertices):
    """Triangle i = (i, i + 1, i + 2): one component whose vertex numbers ascend."""
    i = np.arange(n_vertices - 2, dtype=np.int32)
    return np.stack([i, i + 1, i + 2], axis=1)


def two_sphere_field(shape=(40, 24, 24), centres=((11.3, 11.6, 11.4), (29.2, 12.1, 11.8)), radii=(7.3, 5.1)):
    """float32 [n_nodes]: the distance in voxels to the nearer of two spheres that do not touch, negative inside."""
    import mesh_reference as mr
    return np.minimum(mr.sphere_field(shape, centres[0], radii[0]), mr.sphere_field(shape, centres[1], radii[1])), shape


_DEFAULT = {}


def default_scene_mesh(min_consistent, min_weight):
    """The reference mesh of the default scene (96 x 72, 3 cameras, rel_tol 0.02, mean cost <= 12, resolution 64) through the
    restatements of every stage, as tests/test_mesh_reference.py builds it."""
    key = (min_consistent, min_weight)
    if key not in _DEFAULT:
        import depth_reference as dr
        import mesh_reference as mr
        from sfm_amd.mesh import bounding_grid, projections_from_backprojections
        from test_depth_fuse_reference import scene_maps
        if ("field", min_consistent) not in _DEFAULT:
            s, (refs, sources, warps, backproj, planes), maps = scene_maps(0)
            f = dr.filter_views(s.images, refs, sources, warps, backproj, maps, 0.02, [12 * len(src) * 25 for src in sources], min_consistent)
            keep, xyz, depth = [v[1] for v in f], [v[2] for v in f], [m[2] for m in maps]
            origin, voxel, shape = bounding_grid(np.concatenate([x[k != 0] for x, k in zip(xyz, keep)]), 64, 0.05)
            proj = projections_from_backprojections(backproj)
            _DEFAULT[("field", min_consistent)] = (mr.integrate(proj, depth, keep, origin, voxel, shape, 3.0 * voxel), origin, voxel, shape)
        (tsdf, weight), origin, voxel, shape = _DEFAULT[("field", min_consistent)]
        _DEFAULT[key] = mr.mesh(tsdf, weight, origin, voxel, shape, min_weight)
    return _DEFAULT[key]
