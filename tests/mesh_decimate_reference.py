"""The rule of decimation by vertex clustering (include/sfm_amd.h, sfm_amd/csrc/mesh_decimate_rule.h) restated twice:
`decimate` in NumPy, operation for operation - np.float64 throughout, the ordered sums taken in rounds (round j adds member j
of every cluster that has one, so a cluster's sum is sequential in the rule's order), no einsum and no sum where the order is
part of the rule - and `decimate_loops` in plain Python, one cluster and one triangle at a time.  Also the meshes of the
README's table, the hand cases and the measures the table reports."""
import math

import numpy as np

import mesh_reference as mr

AXIS_CELLS = 1 << 21
DEAD = np.uint64(0xFFFFFFFFFFFFFFFF)
LAMBDA = 0.015625
bits = mr.bits


class Decimated:
    """vertex_cluster int32 [nv]; per cluster first, size (int32), placed (uint8), vertices float64 [nc,3], normals float32
    [nc,3]; triangles int32 [nt',3], triangle_map int32 [nt']; counts = [clusters, unsound vertices]; marks = [kept, unsound
    triangles, degenerate, dropped by the duplicate rule, status]."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def default_origin(vertices):
    """The per-axis minimum of the finite coordinates, zeros where there is none: what `Mesh.decimate` takes."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        lo = np.where(np.isfinite(v), v, np.inf).min(axis=0) if len(v) else np.zeros(3)
    return np.where(np.isfinite(lo), lo, 0.0)


def _rounds(start, size, values):
    """Per cluster the sequential sum of values[start + 0], values[start + 1], ... (size of them, at least one)."""
    total = values[start].copy()
    for j in range(1, int(size.max()) if len(size) else 0):
        sel = np.flatnonzero(size > j)
        total[sel] = total[sel] + values[start[sel] + j]
    return total


def decimate(vertices, triangles, normals=None, cell=1.0, origin=None, placement=1, duplicates="cancel"):
    """The NumPy restatement.  duplicates="first" keeps the first triangle of every triple whatever the orientations are -
    not the rule: what the rule is compared with."""
    v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    nv, nt = len(v), len(tri)
    origin = default_origin(v) if origin is None else np.asarray(origin, np.float64)
    cell = np.float64(cell)
    with np.errstate(all="ignore"):
        q = np.floor((v - origin) / cell)
        sound = (np.isfinite(v) & (q >= 0.0) & (q < float(AXIS_CELLS))).all(axis=1)
    qi = np.where(sound[:, None], q, 0.0).astype(np.int64)
    keys = np.where(sound, (qi[:, 2].astype(np.uint64) << np.uint64(42)) | (qi[:, 1].astype(np.uint64) << np.uint64(21)) | qi[:, 0].astype(np.uint64), DEAD)
    order = np.argsort(keys, kind="stable")
    n_live = int(sound.sum())
    live = order[:n_live]
    ks = keys[live]
    head = np.ones(n_live, bool)
    head[1:] = ks[1:] != ks[:-1]
    start = np.flatnonzero(head)
    nc = len(start)
    size = np.diff(np.r_[start, n_live]).astype(np.int64)
    vertex_cluster = np.full(nv, -1, np.int32)
    vertex_cluster[live] = (np.cumsum(head) - 1).astype(np.int32)
    first = live[start]
    with np.errstate(all="ignore"):
        m = _rounds(start, size, v[live]) / size.astype(np.float64)[:, None] if nc else np.zeros((0, 3))
        if normals is None:
            out_normals = np.zeros((nc, 3), np.float32)
        else:
            ns = _rounds(start, size, np.asarray(normals, np.float32)[live].astype(np.float64)) if nc else np.zeros((0, 3))
            l2 = (ns[:, 0] * ns[:, 0] + ns[:, 1] * ns[:, 1]) + ns[:, 2] * ns[:, 2]
            good = np.isfinite(l2) & (l2 > 0.0)
            out_normals = np.where(good[:, None], ns / np.sqrt(np.where(good, l2, 1.0))[:, None], 0.0).astype(np.float32)
    # triangles
    inside = ((tri >= 0) & (tri < nv)).all(axis=1)
    c = np.where(inside[:, None], vertex_cluster[np.where(inside[:, None], tri, 0)], -1) if nv else np.full((nt, 3), -1, np.int32)
    tri_sound = inside & (c >= 0).all(axis=1)
    x = m.copy()
    placed = np.zeros(nc, np.uint8)
    if placement == 1 and nc and tri_sound.any():
        ckey = np.where(tri_sound[:, None], c, np.int64(1) << 40).reshape(-1)
        corder = np.argsort(ckey, kind="stable")
        corder = corder[:3 * int(tri_sound.sum())]
        cc = ckey[corder]
        ct = corder // 3
        chead = np.ones(len(cc), bool)
        chead[1:] = cc[1:] != cc[:-1]
        cstart = np.flatnonzero(chead)
        csize = np.diff(np.r_[cstart, len(cc)]).astype(np.int64)
        cwho = cc[cstart]                                              # the clusters that have corners
        with np.errstate(all="ignore"):
            p0, p1, p2 = v[tri[ct, 0]], v[tri[ct, 1]], v[tri[ct, 2]]
            e1, e2 = p1 - p0, p2 - p0
            nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
            r = p0 - m[cc]
            s = (nx * r[:, 0] + ny * r[:, 1]) + nz * r[:, 2]
            terms = np.stack([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * s, ny * s, nz * s], axis=1)
            zero = np.zeros((len(cwho), 9))
            acc = zero + terms[cstart]                                 # 0.0 + the first term: A and g start at zero
            for j in range(1, int(csize.max())):
                sel = np.flatnonzero(csize > j)
                acc[sel] = acc[sel] + terms[cstart[sel] + j]
            Ag = np.zeros((nc, 9))
            Ag[cwho] = acc
            A00, A01, A02, A11, A12, A22, g0, g1, g2 = Ag.T
            tr = (A00 + A11) + A22
            lam = tr * LAMBDA
            B00, B01, B02, B11, B12, B22 = A00 + lam, A01, A02, A11 + lam, A12, A22 + lam
            d0 = B00
            l10, l20 = B01 / d0, B02 / d0
            d1 = B11 - l10 * B01
            u = B12 - l20 * B01
            l21 = u / d1
            d2 = (B22 - l20 * B02) - l21 * u
            z1 = g1 - l10 * g0
            z2 = (g2 - l20 * g0) - l21 * z1
            y2 = z2 / d2
            y1 = z1 / d1 - l21 * y2
            y0 = (g0 / d0 - l10 * y1) - l20 * y2
            cand = m + np.stack([y0, y1, y2], axis=1)
            idx = qi[first]
            lo = origin + cell * idx.astype(np.float64)
            hi = origin + cell * (idx + 1).astype(np.float64)
            ok = (tr > 0.0) & (d0 > 0.0) & (d1 > 0.0) & (d2 > 0.0) & (np.isfinite(cand) & (lo <= cand) & (cand <= hi)).all(axis=1)
        x = np.where(ok[:, None], cand, m)
        placed = ok.astype(np.uint8)
    srt = np.sort(c, axis=1)
    degenerate = tri_sound & ((srt[:, 0] == srt[:, 1]) | (srt[:, 1] == srt[:, 2]))
    alive = tri_sound & ~degenerate
    keep = np.zeros(nt, bool)
    t_alive = np.flatnonzero(alive)
    if len(t_alive):
        ca = c[t_alive].astype(np.int64)
        odd = ((ca[:, 0] > ca[:, 1]).astype(int) + (ca[:, 0] > ca[:, 2]) + (ca[:, 1] > ca[:, 2])) % 2 == 1
        sa = srt[t_alive].astype(np.int64)
        _, inv = np.unique(sa, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        ng = int(inv.max()) + 1
        n_even, n_odd = np.bincount(inv[~odd], minlength=ng), np.bincount(inv[odd], minlength=ng)
        first_even, first_odd, first_any = np.full(ng, nt, np.int64), np.full(ng, nt, np.int64), np.full(ng, nt, np.int64)
        np.minimum.at(first_even, inv[~odd], t_alive[~odd])
        np.minimum.at(first_odd, inv[odd], t_alive[odd])
        np.minimum.at(first_any, inv, t_alive)
        if duplicates == "first":
            keep[first_any] = True
        else:
            keep[first_even[n_even > n_odd]] = True
            keep[first_odd[n_odd > n_even]] = True
    kept = np.flatnonzero(keep)
    marks = [len(kept), int((~tri_sound).sum()), int(degenerate.sum()), int(alive.sum()) - len(kept), 0]
    return Decimated(vertex_cluster=vertex_cluster, cluster_first=first.astype(np.int32), cluster_size=size.astype(np.int32),
                     cluster_placed=placed, vertices=np.ascontiguousarray(x, np.float64).reshape(-1, 3), normals=out_normals,
                     triangles=np.ascontiguousarray(c[kept], np.int32).reshape(-1, 3), triangle_map=kept.astype(np.int32),
                     counts=[nc, nv - n_live], marks=marks, origin=np.array(origin, np.float64), cell=float(cell))


# ------------------------------------------------------------------------------------------- plain loops
def _cell_index(v, o, cell):
    if not math.isfinite(v):
        return -1
    d = (v - o) / cell
    if not math.isfinite(d):
        return -1
    q = math.floor(d)
    return q if 0 <= q < AXIS_CELLS else -1


def _place(A, g, m, lo, hi):
    """(x, placed) of mesh_decimate::place, in its order; a division by zero gives what IEEE gives."""
    def div(a, b):
        try:
            return a / b
        except ZeroDivisionError:
            return math.nan if (a == 0.0 or math.isnan(a)) else math.copysign(math.inf, a) * math.copysign(1.0, b)

    A00, A01, A02, A11, A12, A22 = A
    tr = (A00 + A11) + A22
    lam = tr * LAMBDA
    B00, B01, B02, B11, B12, B22 = A00 + lam, A01, A02, A11 + lam, A12, A22 + lam
    d0 = B00
    l10, l20 = div(B01, d0), div(B02, d0)
    d1 = B11 - l10 * B01
    u = B12 - l20 * B01
    l21 = div(u, d1)
    d2 = (B22 - l20 * B02) - l21 * u
    z1 = g[1] - l10 * g[0]
    z2 = (g[2] - l20 * g[0]) - l21 * z1
    y2 = div(z2, d2)
    y1 = div(z1, d1) - l21 * y2
    y0 = (div(g[0], d0) - l10 * y1) - l20 * y2
    x = [m[0] + y0, m[1] + y1, m[2] + y2]
    ok = tr > 0.0 and d0 > 0.0 and d1 > 0.0 and d2 > 0.0 and all(math.isfinite(x[a]) and lo[a] <= x[a] <= hi[a] for a in range(3))
    return (x, 1) if ok else (list(m), 0)


def decimate_loops(vertices, triangles, normals=None, cell=1.0, origin=None, placement=1):
    """The same rule one vertex, one cluster and one triangle at a time, in Python floats."""
    v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3).tolist()
    tri = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3).tolist()
    nrm = None if normals is None else [[float(a) for a in row] for row in np.asarray(normals, np.float32).reshape(-1, 3)]
    nv, nt = len(v), len(tri)
    origin = [float(a) for a in (default_origin(vertices) if origin is None else origin)]
    cell = float(cell)
    cells = {}
    index_of = {}
    for i, p in enumerate(v):
        idx = [_cell_index(p[a], origin[a], cell) for a in range(3)]
        if min(idx) < 0:
            continue
        key = (idx[2] << 42) | (idx[1] << 21) | idx[0]
        cells.setdefault(key, []).append(i)
        index_of[key] = idx
    ordered = sorted(cells)
    nc = len(ordered)
    vertex_cluster = [-1] * nv
    for c, key in enumerate(ordered):
        for i in cells[key]:
            vertex_cluster[i] = c
    means, out_normals = [], []
    for key in ordered:
        members = cells[key]
        s = list(v[members[0]])
        for i in members[1:]:
            s = [s[a] + v[i][a] for a in range(3)]
        means.append([s[a] / float(len(members)) for a in range(3)])
        if nrm is None:
            out_normals.append([0.0, 0.0, 0.0])
            continue
        n = list(nrm[members[0]])
        for i in members[1:]:
            n = [n[a] + nrm[i][a] for a in range(3)]
        l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        out_normals.append([a / math.sqrt(l2) for a in n] if (math.isfinite(l2) and l2 > 0.0) else [0.0, 0.0, 0.0])

    def clusters_of(t):
        if not all(0 <= i < nv for i in t):
            return None
        c = [vertex_cluster[i] for i in t]
        return None if min(c) < 0 else c

    quadric = [[[0.0] * 6, [0.0] * 3] for _ in range(nc)]
    unsound = degenerate = 0
    groups = {}
    for t, ids in enumerate(tri):
        c = clusters_of(ids)
        if c is None:
            unsound += 1
            continue
        p0, p1, p2 = v[ids[0]], v[ids[1]], v[ids[2]]
        e1 = [p1[a] - p0[a] for a in range(3)]
        e2 = [p2[a] - p0[a] for a in range(3)]
        n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        for k in range(3):                                            # ascending h = 3 t + k over ascending t: the rule's order
            A, g = quadric[c[k]]
            m = means[c[k]]
            r = [p0[a] - m[a] for a in range(3)]
            s = (n[0] * r[0] + n[1] * r[1]) + n[2] * r[2]
            for slot, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                A[slot] = A[slot] + n[a] * n[b]
            for a in range(3):
                g[a] = g[a] + n[a] * s
        if len(set(c)) < 3:
            degenerate += 1
            continue
        inversions = (c[0] > c[1]) + (c[0] > c[2]) + (c[1] > c[2])
        groups.setdefault(tuple(sorted(c)), [[], []])[inversions % 2].append(t)
    positions, placed = [], []
    for c, key in enumerate(ordered):
        if placement != 1:
            positions.append(means[c])
            placed.append(0)
            continue
        idx = index_of[key]
        lo = [origin[a] + cell * float(idx[a]) for a in range(3)]
        hi = [origin[a] + cell * float(idx[a] + 1) for a in range(3)]
        x, took = _place(quadric[c][0], quadric[c][1], means[c], lo, hi)
        positions.append(x)
        placed.append(took)
    kept = []
    for even, odd in groups.values():
        if len(even) > len(odd):
            kept.append(even[0])
        elif len(odd) > len(even):
            kept.append(odd[0])
    kept.sort()
    n_alive = sum(len(e) + len(o) for e, o in groups.values())
    with np.errstate(all="ignore"):
        return Decimated(vertex_cluster=np.array(vertex_cluster, np.int32).reshape(-1), cluster_first=np.array([cells[k][0] for k in ordered], np.int32).reshape(-1),
                         cluster_size=np.array([len(cells[k]) for k in ordered], np.int32).reshape(-1), cluster_placed=np.array(placed, np.uint8).reshape(-1),
                         vertices=np.array(positions, np.float64).reshape(-1, 3), normals=np.array(out_normals, np.float64).astype(np.float32).reshape(-1, 3),
                         triangles=np.array([clusters_of(tri[t]) for t in kept], np.int32).reshape(-1, 3), triangle_map=np.array(kept, np.int32).reshape(-1),
                         counts=[nc, nv - sum(len(m) for m in cells.values())], marks=[len(kept), unsound, degenerate, n_alive - len(kept), 0],
                         origin=np.array(origin, np.float64), cell=cell)


FIELDS = ("vertex_cluster", "cluster_first", "cluster_size", "cluster_placed", "vertices", "normals", "triangles", "triangle_map")


def assert_same(a, b, what=""):
    assert list(a.counts) == list(b.counts) and list(a.marks) == list(b.marks), (what, a.counts, b.counts, a.marks, b.marks)
    for name in FIELDS:
        x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        assert np.array_equal(bits(x), bits(y)), (what, name, int((bits(x) != bits(y)).sum()))


# ------------------------------------------------------------------------------------------- meshes and measures
_MESHES = {}
SPHERE_CENTRE, SPHERE_RADIUS = (6.3, 6.6, 6.4), 4.3


def analytic_sphere():
    """The mesh of the distance field of a sphere on 14^3 nodes, radius 4.3 voxels, centre off the nodes: 1,008 / 2,012."""
    if "sphere" not in _MESHES:
        f = mr.sphere_field((14, 14, 14), SPHERE_CENTRE, SPHERE_RADIUS)
        _MESHES["sphere"] = mr.mesh(f, np.ones(len(f), np.uint16), (0.0, 0.0, 0.0), 1.0, (14, 14, 14))
    return _MESHES["sphere"]


def torus():
    """The mesh of a torus on 20 x 20 x 12 nodes whose tube is 5.2 voxels thick: 2,630 / 5,260."""
    if "torus" not in _MESHES:
        f = mr.torus_field((20, 20, 12), (9.4, 9.6, 5.5), 5.5, 2.6)
        _MESHES["torus"] = mr.mesh(f, np.ones(len(f), np.uint16), (0.0, 0.0, 0.0), 1.0, (20, 20, 12))
    return _MESHES["torus"]


def scene_sphere(n_cams=14):
    """(mesh, voxel) of `sphere_scene(n_cams)` through the restatements of the integration and of the mesher."""
    key = ("scene", n_cams)
    if key not in _MESHES:
        proj, depth, origin, voxel, shape, trunc = mr.sphere_scene(n_cams=n_cams)
        tsdf, weight = mr.integrate(proj, depth, None, origin, voxel, shape, trunc)
        _MESHES[key] = (mr.mesh(tsdf, weight, origin, voxel, shape, 1), voxel)
    return _MESHES[key]


def used_vertices(triangles):
    return len(np.unique(np.asarray(triangles))) if len(triangles) else 0


def nonmanifold_edges(triangles):
    """(boundary, non-manifold) undirected edges: used once, used more than twice."""
    ec = mr.edge_counts(triangles)
    und = {}
    for (a, b), n in ec.items():
        und[(min(a, b), max(a, b))] = und.get((min(a, b), max(a, b)), 0) + n
    return sum(1 for n in und.values() if n == 1), sum(1 for n in und.values() if n > 2)


def median_radial_error(d, centre=SPHERE_CENTRE, radius=SPHERE_RADIUS):
    """The median over the referenced new vertices of | |x - centre| - radius |, in the units of the mesh."""
    used = np.unique(d.triangles)
    return float(np.median(np.abs(np.linalg.norm(d.vertices[used] - np.asarray(centre), axis=1) - radius)))


# ------------------------------------------------------------------------------------------- hand cases
def hand_cases():
    """(name, vertices, triangles, normals or None, cell, origin, what the case is about) - the smallest shapes where the
    kernels can go wrong; origin is given, so a vertex outside the grid is unsound."""
    o = np.zeros(3)
    rng = np.random.default_rng(11)
    out = []
    # vertices exactly on cell faces and at origin; one just below origin; one at cell index 2^21; NaN and infinities
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 1], [2, 2, 2], [np.nextafter(0.0, -1.0), 0.5, 0.5], [-1e-9, 0.5, 0.5],
                  [float(AXIS_CELLS), 0.5, 0.5], [np.nextafter(float(AXIS_CELLS), 0.0), 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5],
                  [0.5, 0.5, -np.inf], [3.5, 0.25, 0.25], [0.25, 3.5, 0.25], [0.25, 0.25, 3.5], [1e308, -1e308, 0.5]], np.float64)
    t = np.array([(0, 1, 2), (1, 3, 4), (0, 4, 12), (12, 13, 14), (5, 1, 2), (7, 1, 2), (8, 12, 13), (9, 1, 2), (10, 3, 4), (11, 12, 13), (15, 1, 2),
                  (0, 1, 16), (-1, 1, 2), (0, 1, 1 << 30), (3, 3, 4), (12, 13, 13)], np.int32)
    out.append(("faces, origin, the ends of the grid, NaN, indices", v, t, rng.normal(size=v.shape).astype(np.float32), 1.0, o))
    # duplicates: two equal triangles; two even and one odd; an even-odd pair; a triple with odd before even
    v = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 1.5], [1.6, 0.4, 0.5], [0.4, 1.6, 0.5], [0.6, 0.6, 0.4], [2.5, 2.5, 2.5]],
                 np.float64)
    t = np.array([(0, 1, 2), (6, 4, 5), (0, 1, 3), (1, 3, 0), (3, 1, 6), (0, 2, 3), (3, 5, 0), (2, 1, 3), (1, 3, 2), (3, 5, 4), (7, 1, 2), (2, 7, 4), (5, 1, 7)],
                 np.int32)
    out.append(("duplicates: equal, two even and one odd, an even-odd pair", v, t, None, 1.0, o))
    # all vertices in one cell
    v = rng.uniform(0.1, 0.9, size=(9, 3))
    out.append(("all in one cell", v, np.array([(0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 4, 8)], np.int32), rng.normal(size=v.shape).astype(np.float32), 1.0, o))
    # a cluster of zero-area triangles only: collinear vertices
    v = np.array([[0.2, 0.2, 0.2], [0.4, 0.4, 0.4], [0.6, 0.6, 0.6], [1.2, 1.2, 1.2], [2.4, 2.4, 2.4]], np.float64)
    out.append(("zero-area triangles only", v, np.array([(0, 1, 2), (0, 3, 4), (1, 3, 4)], np.int32), None, 1.0, o))
    # a cell whose solution leaves the box: three vertices of cell (4, 4, 4) on a cone whose apex is in the cell above
    for name, apex in (("the solution leaves the box", 1.4), ("the same cone with its apex in the box", 0.95)):
        P = np.array([0.5, 0.5, apex])
        base = np.array([[0.7, 0.5, 0.9], [0.4, 0.5 + 0.1732, 0.9], [0.4, 0.5 - 0.1732, 0.9]]) - (0.0, 0.0, 0.0 if apex > 1 else 0.6)
        far = np.array([base[i] + 4.0 * (P - base[(i + 1) % 3]) for i in range(3)])
        out.append((name, np.concatenate([base, far]), np.array([(0, 1, 3), (1, 2, 4), (2, 0, 5)], np.int32), None, 1.0, np.full(3, -4.0)))
    # nothing at all, vertices without triangles
    out.append(("nv = 0", np.zeros((0, 3)), np.zeros((0, 3), np.int32), None, 1.0, o))
    out.append(("nt = 0", np.zeros((0, 3)), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32), 0.5, o))
    v = rng.uniform(0, 4, size=(40, 3))
    out.append(("nt = 0 with vertices", v, np.zeros((0, 3), np.int32), rng.normal(size=v.shape).astype(np.float32), 1.0, o))
    # the world shifted by 1e5
    s = analytic_sphere()
    out.append(("shifted by 1e5", s.vertices + 1e5, s.triangles, s.normals, 2.0, np.full(3, 1e5)))
    return out


def strip(n_vertices, step=1.0):
    """Vertices along a zigzag, one per cell of side 1 when step is 1, and the triangles (i, i + 1, i + 2) with every second
    one turned: n_vertices - 2 triangles, all kept when no two vertices share a cell."""
    i = np.arange(n_vertices)
    v = np.stack([0.5 + step * (i // 2), 0.5 + (i % 2).astype(np.float64), np.full(n_vertices, 0.5)], axis=1)
    j = np.arange(n_vertices - 2, dtype=np.int32)
    t = np.stack([j, j + 1, j + 2], axis=1)
    t[1::2] = t[1::2][:, [1, 0, 2]]
    return v, t
