"""The edge table of a mesh, its boundary loops and the filling of the small holes, restated for the tests (include/sfm_amd.h
states the rule): the table twice, independently - NumPy over sorted keys with the walks vectorised, and plain loops over
dictionaries - the sub-loops twice - the stack of the rule, and the repeated removal of the first closed stretch - and the
centroid fan in float64, operation for operation."""
import math
from collections import namedtuple

import numpy as np

WAVE = 64
# counts of an `Edges`: distinct live edges, boundary, inconsistent, non-manifold, short loops, boundary half-edges on none, unsound, status
Edges = namedtuple("Edges", "uses twin next loop loop_leader loop_edges counts")
Fill = namedtuple("Fill", "halfedge_fill counts vertices normals name triangles triangle_halfedge")


def _ends(triangles, n_vertices):
    """(a, b, live) per half-edge h = 3 t + k: from tri[t][k] to tri[t][(k + 1) % 3]."""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    ok = ((tri >= 0) & (tri < n_vertices)).all(axis=1)
    a, b = tri.reshape(-1), tri[:, [1, 2, 0]].reshape(-1)
    return a, b, np.repeat(ok, 3) & (a != b), int((~ok).sum())


def _nx(h):
    return h - h % 3 + (h % 3 + 1) % 3


def _number_loops(lead, length):
    """loop, loop_leader, loop_edges from the leader of every half-edge (-1: on no short loop) and the loop lengths."""
    n = len(lead)
    leaders = np.flatnonzero(lead == np.arange(n))
    number = np.full(n + 1, -1, np.int64)
    number[leaders] = np.arange(len(leaders))
    return number[lead].astype(np.int32), leaders.astype(np.int32), length[leaders].astype(np.int32)


def edges(triangles, n_vertices):
    """NumPy: the runs of equal keys after a stable sort, the rotation and the loop walk on all half-edges in step."""
    a, b, live, n_unsound = _ends(triangles, n_vertices)
    n = len(a)
    uses, twin = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    hs = np.flatnonzero(live)
    key = (np.minimum(a[hs], b[hs]) << 32) | np.maximum(a[hs], b[hs])
    order = np.argsort(key, kind="stable")
    sk, sh = key[order], hs[order]
    first = np.r_[True, sk[1:] != sk[:-1]] if len(sk) else np.zeros(0, bool)
    start = np.flatnonzero(first)
    run = np.diff(np.r_[start, len(sk)])
    uses[sh] = np.repeat(run, run)
    two = start[run == 2]
    p, q = sh[two], sh[two + 1]
    opposite = a[p] == b[q]
    twin[p[opposite]], twin[q[opposite]] = q[opposite], p[opposite]
    n_inconsistent = int((~opposite).sum())
    # the successor: rotate about b inside the surface
    nxt = np.full(n, -1, np.int64)
    h = np.flatnonzero(uses == 1)
    g = _nx(h)
    steps = 0
    while len(h):
        ug = uses[g]
        done = ug == 1
        nxt[h[done]] = g[done]
        go = (ug > 1) & (twin[g] >= 0)
        h, g = h[go], _nx(twin[g[go]])
        steps += 1
        assert steps <= n // 3 + 1
    # the short loops
    lead, length = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    h = np.flatnonzero(uses == 1)
    cur, low = h.copy(), h.copy()
    for step in range(1, WAVE + 1):
        cur = nxt[cur]
        alive = cur >= 0
        h, cur, low = h[alive], cur[alive], low[alive]
        back = cur == h
        lead[h[back]], length[h[back]] = low[back], step
        h, cur, low = h[~back], cur[~back], np.minimum(low[~back], cur[~back])
    loop, loop_leader, loop_edges = _number_loops(lead, length)
    boundary = uses == 1
    counts = [len(start), int(boundary.sum()), n_inconsistent, int((run > 2).sum()), len(loop_leader), int((boundary & (lead < 0)).sum()), n_unsound, 0]
    return Edges(uses.astype(np.int32), twin.astype(np.int32), nxt.astype(np.int32), loop, loop_leader, loop_edges, counts)


def edges_loops(triangles, n_vertices):
    """Plain loops: a dictionary from the unordered pair to its half-edges, one walk at a time."""
    tri = [tuple(int(v) for v in t) for t in np.asarray(triangles, dtype=np.int64).reshape(-1, 3)]
    n = 3 * len(tri)
    ends, n_unsound = [None] * n, 0
    table = {}
    for t, c in enumerate(tri):
        if not all(0 <= v < n_vertices for v in c):
            n_unsound += 1
            continue
        for k in range(3):
            if c[k] != c[(k + 1) % 3]:
                ends[3 * t + k] = (c[k], c[(k + 1) % 3])
                table.setdefault(frozenset(ends[3 * t + k]), []).append(3 * t + k)
    uses, twin = [0] * n, [-1] * n
    n_inconsistent = n_nonmanifold = 0
    for hs in table.values():
        for h in hs:
            uses[h] = len(hs)
        if len(hs) == 2:
            if ends[hs[0]] == ends[hs[1]][::-1]:
                twin[hs[0]], twin[hs[1]] = hs[1], hs[0]
            else:
                n_inconsistent += 1
        n_nonmanifold += len(hs) > 2
    nxt = [-1] * n
    for h in range(n):
        if uses[h] != 1:
            continue
        g = _nx(h)
        while uses[g] > 1 and twin[g] >= 0:
            g = _nx(twin[g])
        nxt[h] = g if uses[g] == 1 else -1
    lead, length = [-1] * n, [0] * n
    for h in range(n):
        if uses[h] != 1:
            continue
        g, seen = h, []
        for _ in range(WAVE):
            g = nxt[g]
            if g < 0:
                break
            seen.append(g)
            if g == h:
                lead[h], length[h] = min(seen), len(seen)
                break
    loop, loop_leader, loop_edges = _number_loops(np.array(lead, np.int64).reshape(-1), np.array(length, np.int64).reshape(-1))
    counts = [len(table), uses.count(1), n_inconsistent, n_nonmanifold, len(loop_leader), sum(1 for h in range(n) if uses[h] == 1 and lead[h] < 0),
              n_unsound, 0]
    i32 = lambda v: np.array(v, dtype=np.int32).reshape(-1)
    return Edges(i32(uses), i32(twin), i32(nxt), loop, loop_leader, loop_edges, counts)


def assert_same_edges(x, y, what=""):
    assert list(x.counts) == list(y.counts), (what, x.counts, y.counts)
    for name in ("uses", "twin", "next", "loop", "loop_leader", "loop_edges"):
        p, q = np.asarray(getattr(x, name)), np.asarray(getattr(y, name))
        assert p.dtype == q.dtype == np.int32 and p.shape == q.shape, (what, name, p.dtype, q.dtype, p.shape, q.shape)
        assert p.tobytes() == q.tobytes(), (what, name, int((p != q).sum()))


def is_closed(e):
    c = e.counts
    return c[1] == 0 and c[2] == 0 and c[3] == 0 and c[6] == 0


def euler(triangles, n_vertices, e):
    """V - E + F with V the vertices some sound triangle uses and F the sound triangles."""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    ok = ((tri >= 0) & (tri < n_vertices)).all(axis=1)
    return len(np.unique(tri[ok])) - e.counts[0] + int(ok.sum())


def loop_members(e, leader):
    out, g = [], int(leader)
    while True:
        out.append(g)
        g = int(e.next[g])
        if g == leader:
            return out


def boundary_cycles(e):
    """The length of every closed boundary cycle, short or long, ascending."""
    nxt = e.next
    seen, out = set(), []
    for h in np.flatnonzero(e.uses == 1):
        h = int(h)
        if h in seen:
            continue
        g, path = h, []
        while g >= 0 and g not in seen:
            seen.add(g)
            path.append(g)
            g = int(nxt[g])
        if g == h:
            out.append(len(path))
    return sorted(out)


def sub_loops_stack(hs, a, b):
    """The rule's stack: the sub-loops of a loop given by its half-edges in next order, each a list in its stack order."""
    stack, out = [], []
    for h in hs:
        stack.append(h)
        for p in range(len(stack)):
            if a[stack[p]] == b[h]:
                out.append(stack[p:])
                del stack[p:]
                break
    assert not stack
    return out


def sub_loops_cut(hs, a, b):
    """The same without a stack: cut out, again and again, the stretch that closes first."""
    rest, out = list(hs), []
    while rest:
        for j in range(len(rest)):
            at = [i for i in range(j + 1) if a[rest[i]] == b[rest[j]]]
            if at:
                assert len(at) == 1
                out.append(rest[at[0]:j + 1])
                del rest[at[0]:j + 1]
                break
        else:
            raise AssertionError("an open stretch")
    return out


def _from_name(sub):
    i = sub.index(min(sub))
    return sub[i:] + sub[:i]


def _patch(order, a, b, v, f64):
    """The new vertex and its normal for one sub-loop, its half-edges from its name on: every operation on its own."""
    c = [f64(0.0)] * 3
    for x in range(3):
        s = f64(v[a[order[0]]][x])
        for h in order[1:]:
            s = s + f64(v[a[h]][x])
        c[x] = s / f64(len(order))
    n = [f64(0.0)] * 3
    for h in order:
        p = [f64(v[a[h]][x]) - f64(v[b[h]][x]) for x in range(3)]
        q = [c[x] - f64(v[b[h]][x]) for x in range(3)]
        cr = [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]
        n = [n[x] + cr[x] for x in range(3)]
    l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    if math.isfinite(l2) and l2 > 0.0:
        l = f64(math.sqrt(l2))
        n = [n[x] / l for x in range(3)]
    else:
        n = [0.0] * 3
    return [float(x) for x in c], n


def _finish(n, a, b, n_vertices, subs, n_open, fv, fn):
    hf = np.full(n, -1, np.int32)
    for r, sub in enumerate(subs):
        hf[sub] = r
    th = np.flatnonzero(hf >= 0)
    ft = np.stack([b[th], a[th], n_vertices + hf[th].astype(np.int64)], axis=1).astype(np.int32).reshape(-1, 3)
    return Fill(hf, [len(subs), len(th), n_open, 0], fv, fn, np.array([s[0] for s in subs], np.int32).reshape(-1), ft, th.astype(np.int32))


def loop_matrix(e):
    """int64 [n_loops, longest]: the half-edges of every short loop in next order from its leader, -1 behind its end."""
    nl = len(e.loop_leader)
    width = int(e.loop_edges.max()) if nl else 0
    M = np.full((nl, width), -1, np.int64)
    cur = e.loop_leader.astype(np.int64)
    for i in range(width):
        on = i < e.loop_edges
        M[on, i] = cur[on]
        cur = np.where(on, e.next[np.maximum(cur, 0)], -1)
    return M


def _patches(ids, a, b, v):
    """`_patch` on m sub-loops of one length at once: ids int64 [m, L], the half-edges of each from its name on."""
    A, B = a[ids], b[ids]
    L = ids.shape[1]
    c = v[A[:, 0]].copy()
    for j in range(1, L):
        c = c + v[A[:, j]]
    c = c / np.float64(L)
    n = np.zeros_like(c)
    for j in range(L):
        p, q = v[A[:, j]] - v[B[:, j]], c - v[B[:, j]]
        cr = np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], axis=1)
        n = n + cr
    l2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    good = np.isfinite(l2) & (l2 > 0.0)
    n = np.where(good[:, None], n / np.sqrt(np.where(good, l2, 1.0))[:, None], 0.0)
    return c, n.astype(np.float32)


def fill(e, triangles, n_vertices, vertices, max_edges=16):
    """The fill pair on an edge table, NumPy: a `Fill`.  vertices float64 [nv,3].  The loops whose start vertices are all
    different are their own sub-loop; only the others go through the stack; the patches are summed for all sub-loops of one
    length at once, operation for operation."""
    assert 1 <= max_edges <= WAVE
    a, b, _, _ = _ends(triangles, n_vertices)
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    M = loop_matrix(e)
    starts = np.where(M >= 0, a[np.maximum(M, 0)], -1 - np.arange(M.shape[1])[None, :]) if M.size else M
    ordered = np.sort(starts, axis=1)
    pinched = (ordered[:, 1:] == ordered[:, :-1]).any(axis=1) if M.size else np.zeros(len(M), bool)
    subs, n_open = [], 0
    for row, pinch, length in zip(M, pinched, e.loop_edges):
        members = [int(h) for h in row[:length]]
        for sub in (sub_loops_stack(members, a, b) if pinch else [members]):
            assert len(sub) >= 3
            if len(sub) <= max_edges:
                subs.append(_from_name(sub))
            else:
                n_open += 1
    subs.sort(key=lambda s: s[0])
    fv, fn = np.zeros((len(subs), 3), np.float64), np.zeros((len(subs), 3), np.float32)
    lengths = np.array([len(s) for s in subs], np.int64)
    with np.errstate(all="ignore"):
        for L in np.unique(lengths):
            rows = np.flatnonzero(lengths == L)
            fv[rows], fn[rows] = _patches(np.array([subs[r] for r in rows], np.int64), a, b, v)
    return _finish(len(a), a, b, n_vertices, subs, n_open, fv, fn)


def fill_loops(e, triangles, n_vertices, vertices, max_edges=16):
    """The same in plain loops: every loop walked on its own, the sub-loops by cutting, every patch in Python floats."""
    assert 1 <= max_edges <= WAVE
    a, b, _, _ = _ends(triangles, n_vertices)
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    subs, n_open = [], 0
    for leader in e.loop_leader:
        for sub in sub_loops_cut(loop_members(e, leader), a, b):
            assert len(sub) >= 3 and len({a[h] for h in sub}) == len(sub)
            if len(sub) <= max_edges:
                subs.append(_from_name(sub))
            else:
                n_open += 1
    subs.sort(key=lambda s: s[0])
    fv, fn = np.zeros((len(subs), 3), np.float64), np.zeros((len(subs), 3), np.float32)
    with np.errstate(all="ignore"):
        for r, sub in enumerate(subs):
            c, nrm = _patch(sub, a, b, v, float)
            fv[r] = c
            fn[r] = np.array(nrm, dtype=np.float64).astype(np.float32)
    return _finish(len(a), a, b, n_vertices, subs, n_open, fv, fn)


def bits(x):
    x = np.ascontiguousarray(x)
    if x.dtype.kind != "f":
        return x
    u = x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize]).copy()
    u[np.isnan(x)] = 0                                            # the payload of a NaN is not part of the rule
    return u


def assert_same_fill(x, y, what=""):
    assert list(x.counts) == list(y.counts), (what, x.counts, y.counts)
    for name in ("halfedge_fill", "vertices", "normals", "name", "triangles", "triangle_halfedge"):
        p, q = np.asarray(getattr(x, name)), np.asarray(getattr(y, name))
        assert p.dtype == q.dtype and p.shape == q.shape, (what, name, p.dtype, q.dtype, p.shape, q.shape)
        assert np.array_equal(bits(p), bits(q)), (what, name, int((bits(p) != bits(q)).sum()))


def filled_mesh(vertices, normals, triangles, f):
    """(vertices, normals, triangles) with the patches appended."""
    v = np.concatenate([np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3), f.vertices])
    n = np.concatenate([np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3), f.normals])
    t = np.concatenate([np.asarray(triangles, dtype=np.int32).reshape(-1, 3), f.triangles])
    return v, n, t


def fill_mesh(vertices, normals, triangles, max_edges=16):
    """(e, f, (vertices, normals, triangles) filled)."""
    e = edges(triangles, len(vertices))
    f = fill(e, triangles, len(vertices), vertices, max_edges)
    return e, f, filled_mesh(vertices, normals, triangles, f)


# ------------------------------------------------------------------------------------------- cases
def disc_fan(rim):
    """(n_vertices, triangles): the fan (centre, i, i + 1) over a closed rim of `rim` vertices; vertex 0 is the centre."""
    i = np.arange(rim, dtype=np.int64)
    return rim + 1, np.stack([np.zeros(rim, np.int64), 1 + i, 1 + (i + 1) % rim], axis=1).astype(np.int32)


def ring_vertices(rim, radius=1.0, z=0.0):
    """[rim + 1, 3]: the centre and a circle about it, the positions of `disc_fan`."""
    ang = 2.0 * np.pi * np.arange(rim) / rim
    return np.concatenate([[[0.0, 0.0, z]], np.stack([radius * np.cos(ang), radius * np.sin(ang), np.full(rim, z)], axis=1)])


def open_fan(degree):
    """(n_vertices, triangles): `degree` triangles about vertex 0 with one gap: the rotation about 0 passes every one."""
    i = np.arange(degree, dtype=np.int64)
    return degree + 2, np.stack([np.zeros(degree, np.int64), 1 + i, 2 + i], axis=1).astype(np.int32)


def quad_grid(nx, ny, punched):
    """(vertices [n,3], triangles): nx x ny quads, two triangles each, without the quads whose number y * nx + x is in
    `punched`; the outline is one long cycle, every punched quad alone a 4-loop."""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    v = np.stack([xs.ravel(), ys.ravel(), 0.25 * np.sin(xs.ravel() * 0.7) * np.cos(ys.ravel() * 0.9)], axis=1).astype(np.float64)
    q = np.setdiff1d(np.arange(nx * ny), np.asarray(punched, dtype=np.int64))
    x, y = q % nx, q // nx
    p = y * (nx + 1) + x
    tri = np.concatenate([np.stack([p, p + 1, p + nx + 2], axis=1), np.stack([p, p + nx + 2, p + nx + 1], axis=1)])
    return v, tri.astype(np.int32)


def punched_grid(n_holes):
    """A quad grid with n_holes separate one-quad holes (every third quad of every third row)."""
    per_row = 40
    rows = -(-n_holes // per_row)
    nx, ny = 3 * per_row + 1, 3 * rows + 1
    holes = [(3 * (k // per_row) + 1) * nx + 3 * (k % per_row) + 1 for k in range(n_holes)]
    return quad_grid(nx, ny, holes)


def cube_less_one_quad():
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], dtype=np.float64)
    quads = [(0, 2, 3, 1), (0, 1, 5, 4), (1, 3, 7, 5), (3, 2, 6, 7), (2, 0, 4, 6)]           # the top (4, 5, 7, 6) is missing
    tri = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return v, np.array(tri, np.int32)


def touching_blocks(w1, h1, w2, h2, margin=8):
    """A quad grid with two punched blocks of w1 x h1 and w2 x h2 quads that share one corner vertex: the surface about that
    vertex is two fans, so ONE boundary loop of 2 (w1 + h1) + 2 (w2 + h2) edges passes it twice and splits into two
    sub-loops.  touching_blocks(1, 1, 1, 1) is two one-quad holes that touch.  With the margin of 8 quads around them the
    outline has more than 64 edges and is no short loop."""
    nx, ny = w1 + w2 + 2 * margin, h1 + h2 + 2 * margin
    holes = [y * nx + x for y in range(margin, margin + h1) for x in range(margin, margin + w1)]
    holes += [y * nx + x for y in range(margin + h1, margin + h1 + h2) for x in range(margin + w1, margin + w1 + w2)]
    return quad_grid(nx, ny, holes)


def random_soup(seed, n_vertices, n_triangles):
    """Triangles over few vertices: boundary, inconsistent and non-manifold edges, repeated indices and unsound ones."""
    rng = np.random.default_rng(seed)
    if n_triangles == 0:
        return np.zeros((0, 3), np.int32)
    tri = rng.integers(0, max(n_vertices, 1), (n_triangles, 3))
    bad = rng.random(n_triangles) < 0.03
    tri[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice([-1, n_vertices, 0x7FFFFFFF, -0x80000000], int(bad.sum()))
    return tri.astype(np.int32)


def random_surface(seed, n=12, drop=0.2):
    """A quad grid with random quads and random single triangles dropped: many loops, pinches among them."""
    rng = np.random.default_rng(seed)
    v, tri = quad_grid(n, n, np.flatnonzero(rng.random(n * n) < drop))
    return v, tri[rng.random(len(tri)) > 0.05]
