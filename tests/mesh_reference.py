"""NumPy restatement of the meshing stages (sfm_amd/csrc/tsdf.hip, mesh.hip; include/sfm_amd.h states the rule): the
integration of depth maps into a truncated signed distance volume and marching tetrahedra over the Kuhn split, operation
for operation - float64 with every product and sum rounded on its own, everything else integer - so that the device's
output bytes can be compared with these.  Also the derivation of the 6 x 16 case table from the geometric rule, the test
fields, and the measures of a mesh (edges, Euler characteristic, signed volume)."""
import numpy as np

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
QNAN_BITS = 0x7FC00000


# ------------------------------------------------------------------------------------------- the case table
def tet_nodes(T):
    """The four local nodes (x, y, z offsets) of tetrahedron T of a cell."""
    a, b, _ = PERMS[T]
    v0 = np.zeros(3, np.int64)
    v1 = v0.copy(); v1[a] += 1
    v2 = v1.copy(); v2[b] += 1
    return [v0, v1, v2, np.ones(3, np.int64)]


def case_triangles(T, case):
    """The triangles of tetrahedron T when local node i is inside iff bit i of case: a list of triangles, each three edges
    (i, j), i < j, of local nodes, in the order and the orientation of the rule."""
    off = tet_nodes(T)
    ins = [i for i in range(4) if (case >> i) & 1]
    out = [i for i in range(4) if not (case >> i) & 1]
    edge = lambda p, q: (min(p, q), max(p, q))
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1 or len(out) == 1:
        p = ins[0] if len(ins) == 1 else out[0]
        a, b, c = [i for i in range(4) if i != p]
        tris = [[edge(p, a), edge(p, b), edge(p, c)]]
    else:
        (p, q), (r, s) = ins, out
        tris = [[edge(p, r), edge(p, s), edge(q, s)], [edge(p, r), edge(q, s), edge(q, r)]]
    D = len(ins) * sum(off[i] for i in out) - len(out) * sum(off[i] for i in ins)
    res = []
    for tri in tris:
        m = [off[i] + off[j] for i, j in tri]
        n = np.cross(m[1] - m[0], m[2] - m[0])
        dot = int(n @ D)
        assert dot != 0
        res.append(tri if dot > 0 else [tri[0], tri[2], tri[1]])
    return res


def edge_code(T, e):
    """(corner, direction) of edge e = (i, j) of tetrahedron T: the corner x + 2 y + 4 z of the owning node, the direction 0 .. 6."""
    off = tet_nodes(T)
    lo, hi = off[e[0]], off[e[1]]
    return int(lo[0] + 2 * lo[1] + 4 * lo[2]), DIRS.index(tuple(int(t) for t in hi - lo))


def derive_table():
    """uint8 [6, 16, 7]: the number of triangles, then per triangle vertex the byte (corner << 3) | direction."""
    tab = np.zeros((6, 16, 7), np.uint8)
    for T in range(6):
        for case in range(16):
            tris = case_triangles(T, case)
            tab[T, case, 0] = len(tris)
            for k, tri in enumerate(tris):
                for v, e in enumerate(tri):
                    c, d = edge_code(T, e)
                    tab[T, case, 1 + 3 * k + v] = (c << 3) | d
    return tab


def tet_corners():
    """uint8 [6, 4]: the corner x + 2 y + 4 z of every local node of every tetrahedron."""
    return np.array([[int(v[0] + 2 * v[1] + 4 * v[2]) for v in tet_nodes(T)] for T in range(6)], np.uint8)


# ------------------------------------------------------------------------------------------- integration
def project(P, X, w, h):
    """The projection rule on arrays: X [..., 3] -> (valid, xi, yi, q2)."""
    P = np.asarray(P, dtype=np.float64).reshape(12)
    with np.errstate(all="ignore"):
        q = [((P[4 * i] * X[..., 0] + P[4 * i + 1] * X[..., 1]) + P[4 * i + 2] * X[..., 2]) + P[4 * i + 3] for i in range(3)]
        u, v = q[0] / q[2], q[1] / q[2]
        valid = (q[2] > 0) & (u >= -0.5) & (u < float(w) - 0.5) & (v >= -0.5) & (v < float(h) - 0.5)
        xi = np.where(valid, np.minimum(np.floor(np.where(valid, u, 0.0) + 0.5), w - 1), 0).astype(np.int64)
        yi = np.where(valid, np.minimum(np.floor(np.where(valid, v, 0.0) + 0.5), h - 1), 0).astype(np.int64)
    return valid, xi, yi, q[2]


def node_positions(origin, voxel, shape):
    """float64 [n_nodes, 3], node n = (k ny + j) nx + i at origin + voxel * (i, j, k)."""
    nx, ny, nz = shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    o, s = np.asarray(origin, dtype=np.float64), np.float64(voxel)
    return np.stack([o[a] + s * idx.astype(np.float64).ravel() for a, idx in enumerate((i, j, k))], axis=1)


def integrate(proj, depth, keep, origin, voxel, shape, trunc):
    """(tsdf float32 [n_nodes], weight uint16 [n_nodes]).  proj [n_ref, 12]; depth: one float32 [h, w] per view; keep: one
    uint8 [h, w] per view, or None."""
    X = node_positions(origin, voxel, shape)
    n = len(X)
    acc, cnt = np.zeros(n, np.float64), np.zeros(n, np.int64)
    trunc = np.float64(trunc)
    for v, d in enumerate(depth):
        d = np.asarray(d, dtype=np.float32)
        h, w = d.shape
        if h == 0 or w == 0:
            continue
        valid, xi, yi, q2 = project(np.asarray(proj, dtype=np.float64).reshape(-1, 12)[v], X, w, h)
        ds = d[yi, xi].astype(np.float64)
        with np.errstate(all="ignore"):
            ok = valid & np.isfinite(ds)
            if keep is not None:
                ok &= np.asarray(keep[v])[yi, xi] != 0
            sdf = ds - q2
            ok &= ~(sdf < -trunc)
            term = np.where(sdf < trunc, sdf, trunc) / trunc
        acc = np.where(ok, acc + np.where(ok, term, 0.0), acc)
        cnt += ok
    with np.errstate(all="ignore"):
        tsdf = (acc / cnt.astype(np.float64)).astype(np.float32)
    tsdf[cnt == 0] = np.array([QNAN_BITS], np.uint32).view(np.float32)[0]
    return tsdf, cnt.astype(np.uint16)


# ------------------------------------------------------------------------------------------- marching tetrahedra
class MeshOut:
    pass


def classify(tsdf, weight, shape, min_weight):
    nx, ny, nz = shape
    f = np.asarray(tsdf, dtype=np.float32).reshape(nz, ny, nx)
    w = np.asarray(weight, dtype=np.uint16).reshape(nz, ny, nx)
    with np.errstate(all="ignore"):
        known = (w.astype(np.int64) >= int(min_weight)) & np.isfinite(f)
        inside = f < 0
    return f, known, inside


def shifted(a, off, fill):
    """b[k, j, i] = a[k + off z, j + off y, i + off x], fill outside the grid; off = (x, y, z)."""
    nz, ny, nx = a.shape
    pad = np.full((nz + 2, ny + 2, nx + 2), fill, a.dtype)
    pad[1:-1, 1:-1, 1:-1] = a
    return pad[1 + off[2]:1 + off[2] + nz, 1 + off[1]:1 + off[1] + ny, 1 + off[0]:1 + off[0] + nx]


def gradients(f, known):
    """float64 [nz, ny, nx, 3]: per axis the central difference, else the one-sided one with the usable neighbour, else 0."""
    f64 = f.astype(np.float64)
    g = np.zeros(f.shape + (3,), np.float64)
    for a in range(3):
        e = [0, 0, 0]; e[a] = 1
        m = [0, 0, 0]; m[a] = -1
        kp, km = shifted(known, e, False), shifted(known, m, False)
        fp, fm = shifted(f64, e, 0.0), shifted(f64, m, 0.0)
        with np.errstate(all="ignore"):
            g[..., a] = np.where(kp & km, 0.5 * (fp - fm), np.where(kp, fp - f64, np.where(km, f64 - fm, 0.0)))
    return g


def unit(n):
    """n / sqrt(l2) as float32 where l2 = (n0 n0 + n1 n1) + n2 n2 is finite and > 0, else zeros."""
    n = np.asarray(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        l2 = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        ok = np.isfinite(l2) & (l2 > 0)
        out = np.where(ok[..., None], n / np.sqrt(np.where(ok, l2, 1.0))[..., None], 0.0)
    return out.astype(np.float32)


def mesh(tsdf, weight, origin, voxel, shape, min_weight=1):
    """The mesh of a field: MeshOut with vertices float64 [nv, 3], normals float32 [nv, 3], triangles int32 [nt, 3], and the
    intermediate vert_mask uint8 [n_nodes], active bool [n_nodes] (cell = its lowest node; False where there is no cell)."""
    nx, ny, nz = shape
    f, known, inside = classify(tsdf, weight, shape, min_weight)
    active = np.ones((nz, ny, nx), bool)
    for c in range(8):
        active &= shifted(known, (c & 1, (c >> 1) & 1, (c >> 2) & 1), False)
    mask = np.zeros((nz, ny, nx), np.uint8)
    for d, dv in enumerate(DIRS):
        differ = inside != shifted(inside, dv, False)
        any_cell = np.zeros((nz, ny, nx), bool)
        for c in range(8):
            back = (c & 1, (c >> 1) & 1, (c >> 2) & 1)
            if any(back[a] and dv[a] for a in range(3)):
                continue
            any_cell |= shifted(active, tuple(-b for b in back), False)
        mask |= ((differ & any_cell).astype(np.uint8) << d).astype(np.uint8)
    out = MeshOut()
    out.vert_mask, out.active = mask.ravel(), active.ravel()
    bits = ((mask.ravel()[:, None] >> np.arange(7)[None, :]) & 1).astype(bool)              # [n_nodes, 7]
    vid = (np.cumsum(bits.ravel()) - 1).reshape(-1, 7)
    node, dirn = np.nonzero(bits)
    i, j, k = node % nx, (node // nx) % ny, node // (nx * ny)
    dv = np.array(DIRS, np.int64)[dirn]
    ib, jb, kb = i + dv[:, 0], j + dv[:, 1], k + dv[:, 2]
    o, s = np.asarray(origin, dtype=np.float64), np.float64(voxel)
    g = gradients(f, known)
    with np.errstate(all="ignore"):
        fa, fb = f[k, j, i].astype(np.float64), f[kb, jb, ib].astype(np.float64)
        t = fa / (fa - fb)
        V = np.zeros((len(node), 3), np.float64)
        for a, (ia, ba) in enumerate(((i, ib), (j, jb), (k, kb))):
            xa, xb = o[a] + s * ia.astype(np.float64), o[a] + s * ba.astype(np.float64)
            V[:, a] = xa + t * (xb - xa)
        gA, gB = g[k, j, i], g[kb, jb, ib]
        out.normals = unit(gA + t[:, None] * (gB - gA)).reshape(-1, 3)
    out.vertices = V
    # triangles: active cells in cell order, tetrahedra 0 .. 5, the triangles of the case
    table, corners = derive_table().astype(np.int64), tet_corners().astype(np.int64)
    cell = np.flatnonzero(active.ravel())
    ci, cj, ck = cell % nx, (cell // nx) % ny, cell // (nx * ny)
    ins = np.stack([inside[ck + ((c >> 2) & 1), cj + ((c >> 1) & 1), ci + (c & 1)] for c in range(8)], axis=1).astype(np.int64)
    tri = np.zeros((len(cell), 6, 2, 3), np.int64)
    have = np.zeros((len(cell), 6, 2), bool)
    for T in range(6):
        case = sum(ins[:, corners[T, n]] << n for n in range(4))
        row = table[T][case]                                       # [cells, 7]
        for q in range(2):
            have[:, T, q] = row[:, 0] > q
            for v in range(3):
                code = row[:, 1 + 3 * q + v]
                c, d = code >> 3, code & 7
                owner = ((ck + ((c >> 2) & 1)) * ny + cj + ((c >> 1) & 1)) * nx + ci + (c & 1)
                tri[:, T, q, v] = vid[owner, d]
                assert (bits[owner, d] | ~have[:, T, q]).all()
    out.triangles = tri[have].astype(np.int32).reshape(-1, 3)
    return out


def mesh_loops(tsdf, weight, origin, voxel, shape, min_weight=1):
    """The same mesh in plain loops, from the geometric rule and without the table: a second formulation."""
    nx, ny, nz = shape
    f32 = np.asarray(tsdf, dtype=np.float32)
    w = np.asarray(weight)
    F = np.float64
    idx = lambda p: (p[2] * ny + p[1]) * nx + p[0]
    in_grid = lambda p: 0 <= p[0] < nx and 0 <= p[1] < ny and 0 <= p[2] < nz
    known = lambda p: in_grid(p) and int(w[idx(p)]) >= min_weight and bool(np.isfinite(f32[idx(p)]))
    inside = lambda p: bool(f32[idx(p)] < 0)
    val = lambda p: F(f32[idx(p)])
    add = lambda p, q: (p[0] + q[0], p[1] + q[1], p[2] + q[2])

    def active(p):
        if not all(0 <= p[a] < (nx, ny, nz)[a] - 1 for a in range(3)):
            return False
        return all(known(add(p, (x, y, z))) for z in (0, 1) for y in (0, 1) for x in (0, 1))

    def gradient(p):
        g = []
        for a in range(3):
            e = tuple(1 if b == a else 0 for b in range(3))
            m = tuple(-t for t in e)
            kp, km = known(add(p, e)), known(add(p, m))
            if kp and km:
                g.append(F(0.5) * (val(add(p, e)) - val(add(p, m))))
            elif kp:
                g.append(val(add(p, e)) - val(p))
            elif km:
                g.append(val(p) - val(add(p, m)))
            else:
                g.append(F(0.0))
        return g

    o, s = [F(t) for t in origin], F(voxel)
    vid, verts, normals = {}, [], []
    with np.errstate(all="ignore"):
        for k in range(nz):
            for j in range(ny):
                for i in range(nx):
                    N = (i, j, k)
                    for d, dv in enumerate(DIRS):
                        B = add(N, dv)
                        if not in_grid(B) or inside(N) == inside(B):
                            continue
                        cells = [(i - x, j - y, k - z) for z in (0, 1) for y in (0, 1) for x in (0, 1)
                                 if not (x and dv[0]) and not (y and dv[1]) and not (z and dv[2])]
                        if not any(active(c) for c in cells):
                            continue
                        vid[(N, d)] = len(verts)
                        fa, fb = val(N), val(B)
                        t = fa / (fa - fb)
                        pos = []
                        for a in range(3):
                            xa, xb = o[a] + s * F(N[a]), o[a] + s * F(B[a])
                            pos.append(xa + t * (xb - xa))
                        verts.append(pos)
                        gA, gB = gradient(N), gradient(B)
                        n = [gA[a] + t * (gB[a] - gA[a]) for a in range(3)]
                        l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
                        if np.isfinite(l2) and l2 > 0:
                            l = np.sqrt(l2)
                            normals.append([np.float32(n[a] / l) for a in range(3)])
                        else:
                            normals.append([np.float32(0)] * 3)
    tris = []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                if not active((i, j, k)):
                    continue
                for T in range(6):
                    off = [tuple(int(t) for t in v) for v in tet_nodes(T)]
                    case = sum(int(inside(add((i, j, k), off[n]))) << n for n in range(4))
                    for tri in case_triangles(T, case):
                        ids = []
                        for a, b in tri:
                            N = add((i, j, k), off[a])
                            d = DIRS.index(tuple(off[b][c] - off[a][c] for c in range(3)))
                            ids.append(vid[(N, d)])
                        tris.append(ids)
    out = MeshOut()
    out.vertices = np.array(verts, dtype=np.float64).reshape(-1, 3)
    out.normals = np.array(normals, dtype=np.float32).reshape(-1, 3)
    out.triangles = np.array(tris, dtype=np.int32).reshape(-1, 3)
    return out


# ------------------------------------------------------------------------------------------- measures of a mesh
def edge_counts(triangles):
    """{(a, b): times the directed edge a -> b is used}."""
    t = np.asarray(triangles, dtype=np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    keys, counts = np.unique(e, axis=0, return_counts=True)
    return {(int(a), int(b)): int(c) for (a, b), c in zip(keys, counts)}


def is_closed_and_oriented(triangles):
    """Every directed edge once and its reverse once."""
    ec = edge_counts(triangles)
    return all(c == 1 and ec.get((b, a), 0) == 1 for (a, b), c in ec.items())


def euler_characteristic(n_vertices, triangles):
    ec = edge_counts(triangles)
    undirected = {(min(a, b), max(a, b)) for a, b in ec}
    return n_vertices - len(undirected) + len(triangles)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(triangles, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ------------------------------------------------------------------------------------------- fields and scenes
def grid_xyz(shape, origin=(0.0, 0.0, 0.0), voxel=1.0):
    nx, ny, nz = shape
    X = node_positions(origin, voxel, shape)
    return X[:, 0].reshape(nz, ny, nx), X[:, 1].reshape(nz, ny, nx), X[:, 2].reshape(nz, ny, nx)


def sphere_field(shape, centre, radius):
    """float32 [n_nodes]: the distance to a sphere in voxels, negative inside."""
    x, y, z = grid_xyz(shape)
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - radius).astype(np.float32).ravel()


def torus_field(shape, centre, R, r):
    x, y, z = grid_xyz(shape)
    q = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2) - R
    return (np.sqrt(q ** 2 + (z - centre[2]) ** 2) - r).astype(np.float32).ravel()


def look_at(centre, f, size):
    """(P [12], R, t, K) of a camera at `centre` looking at the origin, size x size pixels."""
    centre = np.asarray(centre, dtype=np.float64)
    z = -centre / np.linalg.norm(centre)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    t = -R @ centre
    K = np.array([[f, 0, (size - 1) / 2.0], [0, f, (size - 1) / 2.0], [0, 0, 1.0]])
    return np.c_[K @ R, K @ t].reshape(12), R, t, K


def sphere_cameras():
    """The 14 camera centres of the sphere scene: six on the axes at distance 4, eight on the cube diagonals at 2.3 per axis."""
    axes = [tuple(4.0 * s if a == b else 0.0 for b in range(3)) for a in range(3) for s in (1, -1)]
    diag = [(2.3 * sx, 2.3 * sy, 2.3 * sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    return axes + diag


def sphere_scene(n_cams=14, size=64, f=90.0, nodes=32, half=1.4, trunc_voxels=3.0):
    """Rendered depth maps of the unit sphere: (proj [n, 12], depth maps, origin, voxel, shape, trunc).  A pixel whose ray
    misses the sphere has depth NaN."""
    proj, depth = [], []
    for c in sphere_cameras()[:n_cams]:
        P, R, t, K = look_at(c, f, size)
        yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
        ray = np.stack([(xx - K[0, 2]) / f, (yy - K[1, 2]) / f, np.ones_like(xx)], axis=-1) @ R        # world direction per unit depth
        C = np.asarray(c, dtype=np.float64)
        a = (ray * ray).sum(-1)
        b = 2.0 * (ray @ C)
        cc = C @ C - 1.0
        disc = b * b - 4 * a * cc
        with np.errstate(all="ignore"):
            d = np.where(disc >= 0, (-b - np.sqrt(disc)) / (2 * a), np.nan)
        proj.append(P)
        depth.append(d.astype(np.float32))
    voxel = 2.0 * half / (nodes - 1)
    return np.array(proj), depth, (-half, -half, -half), voxel, (nodes, nodes, nodes), trunc_voxels * voxel


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    b = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()
    b[np.isnan(a)] = 0                                            # the payload of a NaN is not part of the rule
    return b


def assert_same_mesh(a, b, what=""):
    for name in ("vertices", "normals", "triangles"):
        x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        assert np.array_equal(bits(x), bits(y)), (what, name, int((bits(x) != bits(y)).any(axis=-1).sum()))
