"""NumPy restatement of the smoothing rule of include/sfm_amd.h (sfm_mesh_adjacency, sfm_mesh_smooth,
sfm_mesh_vertex_normals), operation for operation: float64, every product and every sum rounding on its own, every sum in
the order the rule states.  The adjacency and the normals are restated twice: vectorised (`adjacency`, `vertex_normals`) and
in plain loops and dicts (`adjacency_loops`, `vertex_normals_loops`).  The measures of the README's table are here too."""
import numpy as np

import mesh_decimate_reference as dr
import mesh_reference as mr
from mesh_reference import bits  # noqa: F401

BOUNDARY, ISOLATED = 1, 2
PIN_BOUNDARY, PIN_GIVEN, UNSOUND, STATE_ISOLATED = 1, 2, 4, 8


class Adjacency:
    """ptr int32 [nv + 1], index int32 [n_entries], vertex_flags uint8 [nv], counts [n_entries, n_boundary_vertices,
    n_isolated, n_unsound_triangles]."""


class Smoothed:
    """vertices float64 [nv,3], vertex_state uint8 [nv], counts [n_pinned_boundary, n_pinned_given, n_unsound_vertices,
    n_isolated], normals float32 [nv,3] (recomputed), adjacency."""


# ------------------------------------------------------------------------------------------- adjacency
def _sound(t, nv):
    return ((t >= 0) & (t < nv)).all(axis=1) if len(t) else np.zeros(0, bool)


def adjacency(triangles, n_vertices):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    nv = int(n_vertices)
    sound = _sound(t, nv)
    a, b = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)               # half-edge 3 t + k
    live = np.repeat(sound, 3) & (a != b)
    a, b = a[live], b[live]
    keys = np.concatenate([(a << 32) | b, (b << 32) | a])
    uniq, uses = np.unique(keys, return_counts=True)
    src, dst = uniq >> 32, uniq & 0xFFFFFFFF
    out = Adjacency()
    out.ptr = np.searchsorted(src, np.arange(nv + 1)).astype(np.int32)
    out.index = dst.astype(np.int32)
    boundary = np.zeros(nv, bool)
    boundary[src[uses != 2]] = True
    isolated = np.diff(out.ptr) == 0
    out.vertex_flags = (boundary * BOUNDARY + isolated * ISOLATED).astype(np.uint8)
    out.counts = [len(uniq), int(boundary.sum()), int(isolated.sum()), int((~sound).sum())]
    return out


def adjacency_loops(triangles, n_vertices):
    nv = int(n_vertices)
    uses, unsound = {}, 0
    for tri in np.asarray(triangles).reshape(-1, 3).tolist():
        if not all(0 <= x < nv for x in tri):
            unsound += 1
            continue
        for k in range(3):
            a, b = tri[k], tri[(k + 1) % 3]
            if a != b:
                pair = (min(a, b), max(a, b))
                uses[pair] = uses.get(pair, 0) + 1
    neighbours = [set() for _ in range(nv)]
    for a, b in uses:
        neighbours[a].add(b)
        neighbours[b].add(a)
    ptr, index, flags = [0], [], []
    for v in range(nv):
        mine = sorted(neighbours[v])
        index += mine
        ptr.append(len(index))
        odd = any(uses[(min(v, j), max(v, j))] != 2 for j in mine)
        flags.append((BOUNDARY if odd else 0) | (0 if mine else ISOLATED))
    out = Adjacency()
    out.ptr, out.index, out.vertex_flags = np.array(ptr, np.int32), np.array(index, np.int32), np.array(flags, np.uint8)
    out.counts = [len(index), sum(1 for f in flags if f & BOUNDARY), sum(1 for f in flags if f & ISOLATED), unsound]
    return out


def assert_same_adjacency(a, b, what=""):
    assert list(a.counts) == list(b.counts), (what, a.counts, b.counts)
    for name in ("ptr", "index", "vertex_flags"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (what, name)


# ------------------------------------------------------------------------------------------- the steps
def vertex_state(adj, vertices, pin_boundary=True, pinned=None):
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = adj.vertex_flags
    state = np.zeros(len(v), np.uint8)
    if pin_boundary:
        state |= ((f & BOUNDARY) != 0).astype(np.uint8) * PIN_BOUNDARY
    if pinned is not None:
        state |= (np.asarray(pinned) != 0).astype(np.uint8) * PIN_GIVEN
    state |= (~np.isfinite(v).all(axis=1)).astype(np.uint8) * UNSOUND
    state |= ((f & ISOLATED) != 0).astype(np.uint8) * STATE_ISOLATED
    return state


def _rounds(adj, state):
    """Per rank r among the sound neighbours of the free vertices: (vertices, their r-th sound neighbour); and the number of
    sound neighbours per vertex."""
    ptr, index = adj.ptr.astype(np.int64), adj.index.astype(np.int64)
    nv = len(state)
    owner = np.repeat(np.arange(nv), np.diff(ptr))
    take = ((state[index] & UNSOUND) == 0) & (state[owner] == 0) if len(index) else np.zeros(0, bool)
    owner, other = owner[take], index[take]                        # still (vertex, neighbour ascending)
    n = np.bincount(owner, minlength=nv)
    first = np.concatenate([[0], np.cumsum(n)])[:-1]
    rank = np.arange(len(owner)) - first[owner]
    rounds = []
    for r in range(int(rank.max()) + 1 if len(rank) else 0):
        sel = rank == r
        rounds.append((owner[sel], other[sel]))
    return rounds, n


def step(x, rounds, n, f):
    s = np.zeros_like(x)
    with np.errstate(all="ignore"):
        for vs, js in rounds:
            s[vs] = s[vs] + x[js]
        move = n > 0
        count = n[move].astype(np.float64)[:, None]
        m = s[move] / count
        out = x.copy()
        out[move] = x[move] + f * (m - x[move])
    return out


def smooth(vertices, triangles, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, pinned=None, adj=None, normals=True):
    x = np.array(vertices, dtype=np.float64).reshape(-1, 3)
    tri = np.asarray(triangles, np.int32).reshape(-1, 3)
    if adj is None:
        adj = adjacency(tri, len(x))
    out = Smoothed()
    out.adjacency = adj
    out.vertex_state = state = vertex_state(adj, x, pin_boundary, pinned)
    out.counts = [int(((state & b) != 0).sum()) for b in (PIN_BOUNDARY, PIN_GIVEN, UNSOUND, STATE_ISOLATED)]
    rounds, n = _rounds(adj, state)
    for _ in range(int(iterations)):
        x = step(x, rounds, n, lam)
        if mu is not None:
            x = step(x, rounds, n, mu)
    out.vertices = x
    out.triangles = tri
    out.normals = vertex_normals(x, tri) if normals else None
    return out


# ------------------------------------------------------------------------------------------- normals
def face_normals(vertices, triangles):
    """(p1 - p0) x (p2 - p0) per triangle, every product rounding on its own."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e1, e2 = v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]
        return np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)


def vertex_normals(vertices, triangles):
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    nv = len(v)
    sound = _sound(t, nv)
    fn = np.zeros((len(t), 3))
    fn[sound] = face_normals(v, t[sound])
    h = np.flatnonzero(np.repeat(sound, 3))                         # the corners of the sound triangles, ascending
    owner = t.reshape(-1)[h]
    order = np.argsort(owner, kind="stable")
    h, owner = h[order], owner[order]
    n = np.bincount(owner, minlength=nv)
    first = np.concatenate([[0], np.cumsum(n)])[:-1]
    rank = np.arange(len(owner)) - first[owner]
    ns = np.zeros((nv, 3))
    with np.errstate(all="ignore"):
        for r in range(int(rank.max()) + 1 if len(rank) else 0):
            sel = rank == r
            ns[owner[sel]] = ns[owner[sel]] + fn[h[sel] // 3]
    return mr.unit(ns).reshape(-1, 3)


def vertex_normals_loops(vertices, triangles):
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    nv = len(v)
    ns = [[0.0, 0.0, 0.0] for _ in range(nv)]
    corners = [[] for _ in range(nv)]
    tris = np.asarray(triangles).reshape(-1, 3).tolist()
    for t, tri in enumerate(tris):
        if all(0 <= x < nv for x in tri):
            for k in range(3):
                corners[tri[k]].append(3 * t + k)
    out = np.zeros((nv, 3), np.float32)
    with np.errstate(all="ignore"):
        for i in range(nv):
            for h in corners[i]:                                   # ascending by construction
                p0, p1, p2 = (v[x] for x in tris[h // 3])
                e1, e2 = p1 - p0, p2 - p0
                n = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
                for a in range(3):
                    ns[i][a] = ns[i][a] + n[a]
            x, y, z = (np.float64(c) for c in ns[i])
            l2 = (x * x + y * y) + z * z
            if np.isfinite(l2) and l2 > 0:
                l = np.sqrt(l2)
                out[i] = (np.float32(x / l), np.float32(y / l), np.float32(z / l))
    return out


# ------------------------------------------------------------------------------------------- measures
def face_angle_rms(vertices, triangles, centre):
    """The rms over the triangles with an area of the angle, in degrees, between the face normal and the direction from the
    centre to the face's centroid."""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles, np.int64)
    fn = face_normals(v, t)
    length = np.linalg.norm(fn, axis=1)
    ok = length > 0
    radius = v[t].mean(axis=1) - np.asarray(centre, np.float64)
    cos = (fn[ok] * radius[ok]).sum(axis=1) / (length[ok] * np.linalg.norm(radius[ok], axis=1))
    angle = np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))
    return float(np.sqrt((angle ** 2).mean()))


def radial_error(vertices, triangles, centre, radius, voxel):
    """(rms, signed mean) over the referenced vertices of |x - centre| - radius, in voxels; the mean is the bias."""
    used = np.unique(np.asarray(triangles))
    e = (np.linalg.norm(np.asarray(vertices, np.float64)[used] - np.asarray(centre, np.float64), axis=1) - radius) / voxel
    return float(np.sqrt((e ** 2).mean())), float(e.mean())


_MESHES = {}


def noisy_scene_sphere(amplitude=1.0, seed=7, n_cams=14):
    """(mesh, voxel) of `sphere_scene(n_cams)` with uniform noise of +-amplitude voxels on every depth map."""
    key = (amplitude, seed, n_cams)
    if key not in _MESHES:
        proj, depth, origin, voxel, shape, trunc = mr.sphere_scene(n_cams=n_cams)
        rng = np.random.default_rng(seed)
        depth = [(d + rng.uniform(-amplitude * voxel, amplitude * voxel, size=d.shape)).astype(np.float32) for d in depth]
        tsdf, weight = mr.integrate(proj, depth, None, origin, voxel, shape, trunc)
        _MESHES[key] = (mr.mesh(tsdf, weight, origin, voxel, shape, 1), voxel)
    return _MESHES[key]


# ------------------------------------------------------------------------------------------- hand cases
def fan(n):
    """n triangles about vertex 0 on a closed ring of n vertices, the hub lifted out of the plane."""
    a = 2.0 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0.0, 0.0, 0.7]], np.stack([np.cos(a), np.sin(a), 0.1 * np.cos(5 * a)], axis=1)])
    i = np.arange(n, dtype=np.int32)
    return v, np.stack([np.zeros(n, np.int32), 1 + i, 1 + (i + 1) % n], axis=1)


def hand_cases():
    """(name, vertices, triangles, pinned or None) - the smallest shapes where the kernels can go wrong."""
    rng = np.random.default_rng(17)
    out = []
    v3 = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    out.append(("one triangle", v3, np.array([(0, 1, 2)], np.int32), None))
    v4 = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [0.2, 1.0, 0.0], [0.1, 0.3, 1.0]])
    tet = np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)], np.int32)
    out.append(("a tetrahedron", v4, tet, None))
    out.append(("two triangles on one edge", v4, np.array([(0, 1, 2), (2, 1, 3)], np.int32), None))
    out.append(("a doubled triangle", v4, np.concatenate([tet, tet[:1]]), None))
    out.append(("a doubled triangle, turned", v4, np.concatenate([tet, tet[:1, [1, 0, 2]]]), None))
    out.append(("a triangle (a, a, b)", v4, np.concatenate([tet, [(1, 1, 2)], [(3, 0, 3)]]).astype(np.int32), None))
    out.append(("an index out of range", v4, np.concatenate([tet, [(0, 1, 4)], [(-1, 1, 2)], [(0, 1 << 30, 2)]]).astype(np.int32), None))
    v5 = np.concatenate([v4, [[5.0, 5.0, 5.0]]])
    out.append(("an isolated vertex", v5, tet, None))
    s = dr.analytic_sphere()
    bad = s.vertices.copy()
    bad[100, 1] = np.nan
    bad[500, 2] = np.inf
    bad[501, 0] = -np.inf
    out.append(("a NaN and an inf vertex", bad, s.triangles, None))
    big = s.vertices.copy()
    a = adjacency(s.triangles, len(big))
    big[a.index[a.ptr[7]:a.ptr[8]]] = (1.7e308, -1.7e308, 1.7e308)  # finite, but the sum of two of them is not
    out.append(("values that overflow", big, s.triangles, None))
    out.append(("a caller's pinned", s.vertices, s.triangles, (rng.uniform(size=len(s.vertices)) < 0.2).astype(np.uint8)))
    out.append(("a fan of 1,000 triangles", *fan(1000), None))
    out.append(("nv = 0", np.zeros((0, 3)), np.zeros((0, 3), np.int32), None))
    out.append(("nt = 0 with vertices", rng.uniform(size=(5, 3)), np.zeros((0, 3), np.int32), None))
    return out
