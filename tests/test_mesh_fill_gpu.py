"""The edge table and the hole filling on the device against tests/mesh_fill_reference.py: every output byte of
`sfm_mesh_edges` and `sfm_mesh_fill_mark` / `sfm_mesh_fill_emit`, every call twice, on hand cases, rims around the
wavefront, pinches, the long rotation, NaN vertices, the seams of the block scan, and the device's own meshes."""
import ctypes as C

import numpy as np
import pytest

import mesh_fill_reference as fr
import mesh_reference as mr

pytestmark = pytest.mark.gpu


def assert_edges(got, want, what=""):
    mine = [got.n_edges, got.n_boundary_edges, got.n_inconsistent_edges, got.n_nonmanifold_edges, got.n_loops, got.n_long_boundary_edges, got.n_unsound]
    assert mine == list(want.counts[:7]), (what, mine, want.counts)
    for name, ref in (("halfedge_uses", want.uses), ("halfedge_twin", want.twin), ("halfedge_next", want.next), ("halfedge_loop", want.loop),
                      ("loop_leader", want.loop_leader), ("loop_edges", want.loop_edges)):
        x = getattr(got, name)
        assert x.dtype == np.int32 and x.shape == ref.shape, (what, name, x.dtype, x.shape, ref.shape)
        assert x.tobytes() == ref.tobytes(), (what, name, int((x != ref).sum()))
    assert got.is_closed == fr.is_closed(want), what


def device_edges(tri, n_vertices, what=""):
    """The device's table, checked against the reference and against a second run."""
    from sfm_amd import mesh_edges
    tri = np.asarray(tri, np.int32).reshape(-1, 3)
    got, again = mesh_edges(tri, n_vertices), mesh_edges(tri, n_vertices)
    want = fr.edges(tri, n_vertices)
    assert_edges(got, want, what)
    assert_edges(again, want, (what, "second run"))
    assert got.euler == fr.euler(tri, n_vertices, want), what
    return got, want


def assert_filled(mesh, v, n, tri, f, what=""):
    """Every output of the fill pair, and the old arrays byte for byte in front."""
    nv, nt = len(v), len(tri)
    assert (mesh.n_filled, mesh.n_fill_triangles, mesh.n_open) == tuple(f.counts[:3]), (what, mesh.n_filled, mesh.n_fill_triangles, mesh.n_open, f.counts)
    assert (mesh.fill_vertex_start, mesh.fill_triangle_start, mesh.n_vertices, mesh.n_triangles) == (nv, nt, nv + f.counts[0], nt + f.counts[1]), what
    vv, nn, tt = fr.filled_mesh(v, n, tri, f)
    for name, ref, dtype in (("vertices", vv, np.float64), ("normals", nn, np.float32), ("triangles", tt, np.int32),
                             ("fill_triangle_halfedge", f.triangle_halfedge, np.int32)):
        x = getattr(mesh, name)
        assert x.dtype == dtype and x.shape == ref.shape, (what, name, x.dtype, x.shape, ref.shape)
        assert np.array_equal(fr.bits(x), fr.bits(ref)), (what, name, int((fr.bits(x) != fr.bits(ref)).sum()))
    assert mesh.vertices[:nv].tobytes() == np.ascontiguousarray(v, np.float64).tobytes() and mesh.normals[:nv].tobytes() == n.tobytes(), what
    assert mesh.triangles[:nt].tobytes() == tri.tobytes(), what
    flags = mesh._m["halfedge_fill"].cpu().numpy()[:3 * nt]
    names = mesh._m["fill_name"].cpu().numpy()[:f.counts[0]]
    assert flags.dtype == names.dtype == np.int32 and flags.tobytes() == f.halfedge_fill.tobytes() and names.tobytes() == f.name.tobytes(), what
    assert mesh.atlas is None and mesh.vertex_colors is None and mesh.n_views is None and mesh.best_view is None


def device_fill(v, tri, max_edges=16, what="", normals=None):
    """fill_mesh_holes against the reference, twice; the table it used as well."""
    from sfm_amd import fill_mesh_holes
    tri = np.asarray(tri, np.int32).reshape(-1, 3)
    v = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
    n = np.random.default_rng(len(v)).normal(size=(len(v), 3)).astype(np.float32) if normals is None else normals
    got, again = fill_mesh_holes(v, tri, n, max_edges), fill_mesh_holes(v, tri, n, max_edges)
    e = fr.edges(tri, len(v))
    f = fr.fill(e, tri, len(v), v, max_edges)
    assert_filled(got, v, n, tri, f, what)
    assert_filled(again, v, n, tri, f, (what, "second run"))
    assert_edges(got.edges_before, e, what)
    return got, e, f


def closes(mesh):
    e = mesh.edges()
    return e.is_closed, e.euler


# ------------------------------------------------------------------------------------------- small cases
def test_empty_inputs(gpu_ready):
    none, _ = device_edges(np.zeros((0, 3), np.int32), 0)
    assert none.n_edges == 0 and none.halfedge_uses.shape == (0,) and none.loop_leader.shape == (0,) and none.is_closed and none.euler == 0
    loose, _ = device_edges(np.zeros((0, 3), np.int32), 5, "vertices without triangles")
    assert loose.n_edges == 0 and loose.euler == 0
    got, _, _ = device_fill(np.zeros((0, 3)), np.zeros((0, 3), np.int32))
    assert got.vertices.shape == (0, 3) and got.triangles.shape == (0, 3) and got.n_filled == 0
    got, _, _ = device_fill(np.arange(15.0).reshape(5, 3), np.zeros((0, 3), np.int32))
    assert got.n_vertices == 5 and got.n_triangles == 0


def test_hand_cases(gpu_ready):
    v3 = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], np.float64)
    one, e, f = device_fill(v3, [(0, 1, 2)], 16, "one triangle")
    assert one.n_filled == 1 and one.triangles.tolist() == [[0, 1, 2], [1, 0, 3], [2, 1, 3], [0, 2, 3]] and closes(one) == (True, 2)
    assert one.vertices[3].tolist() == [2 / 3, 2 / 3, 0.0] and one.normals[3].tolist() == [0.0, 0.0, -1.0]
    assert device_fill(v3, [(0, 1, 2)], 2, "one triangle, max_edges 2")[0].n_open == 1
    tet_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    tet, _, _ = device_fill(tet_v, [(0, 2, 1), (0, 1, 3), (1, 2, 3)], 16, "a tetrahedron less one face")
    assert tet.n_filled == 1 and closes(tet) == (True, 2)
    cube_v, cube_t = fr.cube_less_one_quad()
    cube, _, _ = device_fill(cube_v, cube_t, 16, "a cube less one quad")
    assert cube.n_filled == 1 and cube.n_fill_triangles == 4 and closes(cube) == (True, 2) and cube.normals[8].tolist() == [0.0, 0.0, 1.0]
    bow, e, _ = device_fill(np.random.default_rng(1).normal(size=(5, 3)), [(0, 1, 2), (2, 3, 4)], 16, "two that share a vertex only")
    assert e.counts[4] == 2 and bow.n_filled == 2 and closes(bow)[0]
    v, t = fr.touching_blocks(1, 1, 1, 1)
    touch, e, f = device_fill(v, t, 16, "two holes that touch")
    assert e.loop_edges.tolist() == [8] and f.counts == [2, 8, 0, 0] and touch.n_filled == 2
    assert device_fill(v, t, 3, "two holes that touch, max_edges 3")[0].n_open == 2
    fin_t = [(0, 1, 2), (1, 0, 3), (0, 1, 4)]
    fin, want = device_edges(fin_t, 5, "three triangles on one edge")
    assert fin.n_nonmanifold_edges == 1 and fin.halfedge_uses[[0, 3, 6]].tolist() == [3, 3, 3] and fin.halfedge_next.tolist() == [-1, 2, -1, -1, 5, -1, -1, 8, -1]
    assert device_fill(np.random.default_rng(2).normal(size=(5, 3)), fin_t, 16, "three triangles on one edge")[0].n_filled == 0
    same, _ = device_edges([(0, 1, 2), (0, 1, 3)], 4, "the same direction twice")
    assert same.n_inconsistent_edges == 1 and same.halfedge_twin.tolist() == [-1] * 6 and not same.is_closed
    odd_t = [(0, 1, 2), (2, 1, 1), (0, 2, 7), (-1, 0, 1), (3, 3, 3)]
    odd, _ = device_edges(odd_t, 4, "a repeated index and unsound triangles")
    assert odd.n_unsound == 2 and odd.n_nonmanifold_edges == 1 and not odd.is_closed
    device_fill(np.random.default_rng(3).normal(size=(4, 3)), odd_t, 16, "a repeated index and unsound triangles")
    # a hole beside them: the quad grid's hole is filled whatever stands behind it in the array
    v, t = fr.quad_grid(20, 20, [210])
    mixed = np.concatenate([t[:300], np.array([(5, 5, 6), (-1, 0, 1), (0, 1, len(v))], np.int32), t[300:]])
    got, e, f = device_fill(v, mixed, 16, "a hole beside a repeated index and unsound triangles")
    assert e.counts[6] == 2 and f.counts[0] == 1 and f.counts[1] == 4


@pytest.mark.parametrize("rim", [3, 16, 17, 63, 64, 65])
def test_disc_fans(gpu_ready, rim):
    """The fan (centre, i, i + 1) over a closed rim: the rim is the loop; 65 edges are no short loop, 17 stay open at 16."""
    nv, t = fr.disc_fan(rim)
    v = fr.ring_vertices(rim) + 0.01 * np.random.default_rng(rim).normal(size=(nv, 3))
    got, want = device_edges(t, nv, rim)
    assert got.n_loops == int(rim <= 64) and got.n_long_boundary_edges == (rim if rim > 64 else 0) and got.n_boundary_edges == rim
    for max_edges in (16, 64):
        mesh, e, f = device_fill(v, t, max_edges, (rim, max_edges))
        fills = rim <= max_edges
        assert (mesh.n_filled, mesh.n_fill_triangles) == (int(fills), rim if fills else 0) and mesh.n_open == int(rim <= 64 and not fills)
        assert closes(mesh) == (fills, 2 if fills else 1)


def test_the_long_rotation(gpu_ready):
    """1,000 triangles about vertex 0 with one gap: the successor of the half-edge that arrives at 0 passes every one."""
    nv, t = fr.open_fan(1000)
    got, want = device_edges(t, nv, "open fan")
    assert got.halfedge_next[3 * 999 + 2] == 0 and got.n_loops == 0 and got.n_long_boundary_edges == 1002
    rng = np.random.default_rng(1000)
    device_edges(t[rng.permutation(1000)], nv, "open fan, shuffled")


def test_pinches(gpu_ready):
    """Two blocks of punched quads that share a corner: one loop, two sub-loops; 64 edges split into 32 + 32, 66 are no loop."""
    v, t = fr.touching_blocks(8, 8, 8, 8)
    got, e, f = device_fill(v, t, 64, "32 + 32")
    assert e.loop_edges.tolist() == [64] and (got.n_filled, got.n_fill_triangles) == (2, 64)
    got, _, _ = device_fill(v, t, 31, "32 + 32 at 31")
    assert (got.n_filled, got.n_open) == (0, 2)
    v, t = fr.touching_blocks(8, 8, 8, 9)
    got, e, f = device_fill(v, t, 64, "32 + 34")
    assert e.counts[4] == 0 and got.n_filled == 0 and got.edges_before.n_long_boundary_edges == e.counts[1]
    v, t = fr.touching_blocks(3, 2, 1, 5)
    got, e, f = device_fill(v, t, 10, "10 + 12 at 10")
    assert e.loop_edges.tolist() == [22] and (got.n_filled, got.n_fill_triangles, got.n_open) == (1, 10, 1)
    # many holes, pinches among them, in any order of the triangles
    for seed in range(3):
        v, t = fr.random_surface(40 + seed, 24, 0.2)
        t = t[np.random.default_rng(seed).permutation(len(t))]
        for max_edges in (4, 16, 64):
            device_fill(v, t, max_edges, ("random surface", seed, max_edges))


def test_nan_and_infinite_vertices_on_a_rim(gpu_ready):
    nv, t = fr.disc_fan(7)
    v = fr.ring_vertices(7)
    v[2, 1], v[4, 0], v[6, 2] = np.nan, np.inf, -np.inf
    got, _, f = device_fill(v, t, 16, "NaN on the rim")
    assert got.n_filled == 1 and np.isinf(got.vertices[8, 0]) and np.isnan(got.vertices[8, 1]) and got.normals[8].tolist() == [0.0, 0.0, 0.0]
    v, t = fr.quad_grid(12, 12, [40, 41, 90])
    v[::5, 0], v[::7, 2] = np.nan, np.inf
    device_fill(v, t, 16, "NaN on a grid")


# ------------------------------------------------------------------------------------------- the seams of the scans
@pytest.mark.parametrize("n_holes", [255, 256, 257, 1025])
def test_seams_of_the_loop_numbers(gpu_ready, n_holes):
    """A quad grid with n_holes one-quad holes: that many short loops, sub-loops and new vertices."""
    v, t = fr.punched_grid(n_holes)
    got, e, f = device_fill(v, t, 16, n_holes)
    assert e.counts[4] == n_holes and (got.n_filled, got.n_fill_triangles) == (n_holes, 4 * n_holes) and got.edges_before.n_loops == n_holes
    after = got.edges()
    assert after.n_loops == 0 and after.n_boundary_edges == e.counts[5]


@pytest.mark.parametrize("nt", [85, 86, 341, 342])
def test_seams_of_the_half_edges(gpu_ready, nt):
    """3 nt at 255, 258, 1,023 and 1,026: disjoint triangles, so the first and the last half-edge of the array are boundary
    and every block is full of leaders; then a strip, whose outline passes the first and the last half-edge."""
    tri = np.arange(3 * nt, dtype=np.int32).reshape(-1, 3)
    v = np.random.default_rng(nt).normal(size=(3 * nt, 3))
    got, e, f = device_fill(v, tri, 16, nt)
    assert e.counts[4] == nt and got.n_filled == nt and e.uses[0] == 1 and e.uses[-1] == 1 and f.halfedge_fill[-1] == nt - 1
    i = np.arange(nt, dtype=np.int32)
    strip = np.stack([i, i + 1, i + 2], axis=1)
    strip[1::2] = strip[1::2][:, [1, 0, 2]]
    got, want = device_edges(strip, nt + 2, ("strip", nt))
    assert want.uses[0] == 1 and want.uses[-1] == 1 and got.n_inconsistent_edges == 0 and got.n_boundary_edges == nt + 2


def test_the_second_scan_level(gpu_ready):
    """87,382 disjoint triangles: 3 nt = 262,146, past the 1,024 blocks of one chunk; every outline is a loop and is filled."""
    nt = 87382
    tri = np.arange(3 * nt, dtype=np.int32).reshape(-1, 3)
    v = np.random.default_rng(nt).normal(size=(3 * nt, 3))
    got, e, f = device_fill(v, tri, 16, "262,146")
    assert e.counts[:6] == [3 * nt, 3 * nt, 0, 0, nt, 0] and (got.n_filled, got.n_fill_triangles) == (nt, 3 * nt)
    assert got.fill_triangle_halfedge[-1] == 3 * nt - 1 and got.triangles[-1].tolist() == [3 * nt - 3, 3 * nt - 1, 4 * nt - 1]


def test_nothing_depends_on_the_order(gpu_ready):
    v, t = fr.random_surface(9, 30, 0.15)
    rng = np.random.default_rng(9)
    order = rng.permutation(len(t))
    turned = np.stack([np.roll(x, k) for x, k in zip(t[order], rng.integers(0, 3, len(t)))])
    a, _ = device_edges(t, len(v), "surface")
    b, _ = device_edges(turned, len(v), "surface, shuffled")
    for name in ("n_edges", "n_boundary_edges", "n_loops", "n_long_boundary_edges", "euler"):
        assert getattr(a, name) == getattr(b, name), name
    assert sorted(a.loop_edges.tolist()) == sorted(b.loop_edges.tolist())
    x, _, _ = device_fill(v, t, 16, "surface")
    y, _, _ = device_fill(v, turned, 16, "surface, shuffled")
    assert (x.n_filled, x.n_fill_triangles, x.n_open) == (y.n_filled, y.n_fill_triangles, y.n_open)
    assert x.edges().n_boundary_edges == y.edges().n_boundary_edges


def test_entry_points_reject_bad_arguments(gpu_ready):
    """SFM_ERR_ARG (-1) before any device work: the data pointers are 1 or null throughout, so a call that got as far as a
    launch would not return -1 but fault."""
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    p, big, room = C.c_void_p(1), (1 << 31) // 3 + 1, 1 << 30
    why = lambda: lib.sfm_last_error(h._h)
    need = C.c_int64(-1)
    assert lib.sfm_mesh_edges_workspace_bytes(h._h, 0, C.byref(need)) == 0 and 0 < need.value <= 4096
    assert lib.sfm_mesh_edges_workspace_bytes(h._h, 100000, C.byref(need)) == 0 and need.value >= 100000 * 3 * 28
    for n in (-1, big):
        assert lib.sfm_mesh_edges_workspace_bytes(h._h, n, C.byref(need)) == -1
    assert lib.sfm_mesh_edges_workspace_bytes(h._h, 5, None) == -1

    def edges(nv=5, nt=2, tri=p, uses=p, twin=p, nxt=p, loop=p, leader=p, length=p, counts=p, ws=p, ws_bytes=room):
        return lib.sfm_mesh_edges(h._h, nv, nt, tri, uses, twin, nxt, loop, leader, length, counts, ws, ws_bytes)

    def mark(nv=5, nt=2, tri=p, nxt=p, nl=1, leader=p, max_edges=16, flags=p, counts=p, ws=p, ws_bytes=room):
        return lib.sfm_mesh_fill_mark(h._h, nv, nt, tri, nxt, nl, leader, max_edges, flags, counts, ws, ws_bytes)

    def emit(nv=5, nt=2, tri=p, nxt=p, nl=1, leader=p, flags=p, v=p, cap_v=1, cap_t=3, fv=p, fn=p, name=p, ft=p, fh=p, ws=p, ws_bytes=room):
        return lib.sfm_mesh_fill_emit(h._h, nv, nt, tri, nxt, nl, leader, flags, v, cap_v, cap_t, fv, fn, name, ft, fh, ws, ws_bytes)

    for call, cases in ((edges, [dict(nv=-1), dict(nt=-1), dict(nv=1 << 31), dict(nt=big), dict(tri=None), dict(uses=None), dict(twin=None), dict(nxt=None),
                                 dict(loop=None), dict(leader=None), dict(length=None), dict(counts=None), dict(ws=None), dict(ws_bytes=64)]),
                        (mark, [dict(nv=-1), dict(nt=big), dict(nl=-1), dict(nl=3), dict(max_edges=0), dict(max_edges=65), dict(tri=None), dict(nxt=None),
                                dict(leader=None), dict(flags=None), dict(counts=None), dict(ws=None), dict(ws_bytes=64)]),
                        (emit, [dict(nv=1 << 31), dict(nt=-1), dict(nl=3), dict(cap_v=-1), dict(cap_t=-1), dict(cap_v=1 << 31), dict(cap_t=1 << 31),
                                dict(tri=None), dict(nxt=None), dict(leader=None), dict(flags=None), dict(v=None), dict(fv=None), dict(fn=None),
                                dict(name=None), dict(ft=None), dict(fh=None), dict(ws=None), dict(ws_bytes=64)])):
        for kw in cases:
            assert call(**kw) == -1, (call.__name__, kw)
            null = any(v is None for k, v in kw.items() if k != "ws")
            assert why().endswith(b": null pointer") == null, (call.__name__, kw, why())
    # nothing to emit: returns at once, whatever the pointers
    assert emit(cap_v=0, cap_t=0, v=None, fv=None, fn=None, name=None, ft=None, fh=None) == 0


def test_emit_writes_nothing_at_or_above_the_capacities(gpu_ready):
    import torch
    from sfm_amd import _lib, mesh_edges
    v, t = fr.punched_grid(40)
    e = fr.edges(t, len(v))
    f = fr.fill(e, t, len(v), v)
    dev = torch.device("cuda", 0)
    h = _lib.get_handle(0)
    table = mesh_edges(t, len(v))
    d_tri, d_v = torch.from_numpy(t).to(dev), torch.from_numpy(v).to(dev)
    need = C.c_int64()
    assert h.lib.sfm_mesh_fill_workspace_bytes(len(t), C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    flags = torch.empty(3 * len(t), dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    dp = lambda x: C.c_void_p(x.data_ptr())
    m = table._m
    h.call("sfm_mesh_fill_mark", len(v), len(t), dp(d_tri), dp(m["halfedge_next"]), table.n_loops, dp(m["loop_leader"]), 16, dp(flags), dp(counts), dp(ws),
           need.value)
    assert counts.cpu().numpy().tolist() == f.counts == [40, 160, 0, 0]
    cap_v, cap_t = 17, 50
    fv = torch.full((40, 3), 7.0, dtype=torch.float64, device=dev)
    fn = torch.full((40, 3), 7.0, dtype=torch.float32, device=dev)
    name = torch.full((40,), 7, dtype=torch.int32, device=dev)
    ft = torch.full((160, 3), 7, dtype=torch.int32, device=dev)
    fh = torch.full((160,), 7, dtype=torch.int32, device=dev)
    h.call("sfm_mesh_fill_emit", len(v), len(t), dp(d_tri), dp(m["halfedge_next"]), table.n_loops, dp(m["loop_leader"]), dp(flags), dp(d_v), cap_v, cap_t,
           dp(fv), dp(fn), dp(name), dp(ft), dp(fh), dp(ws), need.value)
    fv, fn, name, ft, fh = (x.cpu().numpy() for x in (fv, fn, name, ft, fh))
    assert (fv[cap_v:] == 7.0).all() and (fn[cap_v:] == 7.0).all() and (name[cap_v:] == 7).all() and (ft[cap_t:] == 7).all() and (fh[cap_t:] == 7).all()
    assert fv[:cap_v].tobytes() == f.vertices[:cap_v].tobytes() and name[:cap_v].tobytes() == f.name[:cap_v].tobytes()
    assert fh[:cap_t].tobytes() == f.triangle_halfedge[:cap_t].tobytes()
    # a triangle whose new vertex is above the capacity of the vertices is written as -1s: never an index past the arrays
    want = f.triangles[:cap_t].copy()
    want[want[:, 2] >= len(v) + cap_v] = -1
    assert ft[:cap_t].tobytes() == want.tobytes()
    # a table that is not of these triangles raises the status word and fills nothing there
    wrong = torch.from_numpy(np.ascontiguousarray(t[::-1])).to(dev)
    h.call("sfm_mesh_fill_mark", len(v), len(t), dp(wrong), dp(m["halfedge_next"]), table.n_loops, dp(m["loop_leader"]), 16, dp(flags), dp(counts), dp(ws),
           need.value)
    got = counts.cpu().numpy().tolist()
    assert got[3] in (0, 1) and got[0] <= 40


# ------------------------------------------------------------------------------------------- the device's own meshes
def test_the_sphere_of_eight_cameras_comes_back_closed(gpu_ready):
    """sphere_scene(n_cams=8) -> tsdf -> mesh -> edges / fill_holes on the device: the README's first row."""
    from sfm_amd import MeshEdges
    from sfm_amd.mesh import tsdf_volume_from_depth_arrays
    proj, depth, origin, voxel, shape, trunc = mr.sphere_scene(n_cams=8)
    mesh = tsdf_volume_from_depth_arrays(proj, depth, None, origin, voxel, shape, trunc).mesh()
    assert (mesh.n_vertices, mesh.n_triangles) == (6943, 13776)
    table = mesh.edges()
    want = fr.edges(mesh.triangles, mesh.n_vertices)
    assert isinstance(table, MeshEdges)
    assert_edges(table, want, "sphere")
    assert (table.n_edges, table.n_boundary_edges, table.n_loops, table.n_long_boundary_edges) == (20763, 198, 28, 0) and not table.is_closed
    before = (mesh.vertices.tobytes(), mesh.normals.tobytes(), mesh.triangles.tobytes())
    out = mesh.fill_holes()
    f = fr.fill(want, mesh.triangles, mesh.n_vertices, mesh.vertices)
    assert_filled(out, mesh.vertices, mesh.normals, mesh.triangles, f, "sphere")
    assert (out.n_filled, out.n_fill_triangles, out.n_vertices, out.n_triangles) == (46, 198, 6989, 13974)
    after = out.edges()
    assert after.is_closed and after.euler == 2 and after.n_edges == 20961
    assert mr.is_closed_and_oriented(out.triangles) and mr.euler_characteristic(out.n_vertices, out.triangles) == 2
    assert round(mr.signed_volume(out.vertices, out.triangles), 4) == 4.2527
    assert out is not mesh and (mesh.vertices.tobytes(), mesh.normals.tobytes(), mesh.triangles.tobytes()) == before and mesh.n_filled is None
    assert out._volume is mesh._volume and out.edges_before.n_loops == 28
    same = mesh.fill_holes(16, edges=table)
    assert same.edges_before is table and same.triangles.tobytes() == out.triangles.tobytes() and same.vertices.tobytes() == out.vertices.tobytes()
    assert mesh.fill_holes(4).n_filled == 39 and mesh.fill_holes(3).n_filled == 0      # 19 loops of 4 edges and 20 parts of 4 of the loops that touch
    # a closed mesh comes back as it went in
    again = out.fill_holes()
    assert again.n_filled == 0 and again.triangles.tobytes() == out.triangles.tobytes() and again.vertices.tobytes() == out.vertices.tobytes()


def test_default_scene_filled_textured_and_rendered(gpu_ready):
    """depth_maps -> filter -> tsdf -> mesh -> clean -> fill_holes -> texture -> render_views on the default scene: the
    README's third row, and the coverage of no view falls."""
    from test_mesh_texture_gpu import default_scene_maps
    s, maps = default_scene_maps()
    mesh = maps.tsdf(resolution=64).mesh()
    images = list(s.images)
    table = mesh.edges()
    want = fr.edges(mesh.triangles, mesh.n_vertices)
    assert_edges(table, want, "default scene")
    assert (table.n_edges, table.n_boundary_edges) == (33689, 1042)
    out = mesh.fill_holes(16, edges=table)
    assert_filled(out, mesh.vertices, mesh.normals, mesh.triangles, fr.fill(want, mesh.triangles, mesh.n_vertices, mesh.vertices), "default scene")
    assert (out.n_filled, out.n_fill_triangles) == (4, 48) and out.edges().n_boundary_edges == 994
    mesh.texture(images, texels=2)
    base = mesh.render_views().coverage
    atlas = out.texture(images, texels=2)
    assert atlas is out.atlas and atlas.n_triangles == out.n_triangles
    render = out.render_views()
    assert render.sizes == [(96, 72)] * 3 and all(c >= b for c, b in zip(render.coverage, base))
    assert out.colors(images).shape == (out.n_vertices,)


def test_dense_from_reconstruction_fills_the_mesh(gpu_ready):
    """fill_holes of `dense_from_reconstruction`: with None the mesh is the one of before; with a number it is filled after
    the cleaning."""
    from sfm_amd import Reconstruction, Tracks, dense_from_reconstruction
    import depth_reference as dr
    s = dr.default_scene()
    ys, xs = np.mgrid[4:72:8, 4:96:8]
    ys, xs = ys.ravel(), xs.ravel()
    z = s.depth[1][ys, xs]
    X = np.stack([(xs - s.K[0, 2]) / s.K[0, 0] * z, (ys - s.K[1, 2]) / s.K[1, 1] * z, z], axis=1)
    n = len(X)
    kp = []
    for i in range(3):
        q = (X + s.poses[i][1]) @ s.K.T
        kp.append(q[:, :2] / q[:, 2:])
    tracks = Tracks(np.arange(4) * n, np.arange(n + 1) * 3, np.tile(np.arange(3), n), np.repeat(np.arange(n), 3))
    rec = Reconstruction(tracks, np.concatenate(kp), s.K)
    rec.poses, rec.order, rec.unregistered = dict(s.poses), [1, 0, 2], []
    rec.X, rec.has_point = X, np.ones(n, bool)
    kw = dict(rel_tol=0.02, max_cost=12.0, min_consistent=1, mesh=True)
    plain = dense_from_reconstruction(rec, s.images, **kw)[-1]
    none = dense_from_reconstruction(rec, s.images, fill_holes=None, **kw)[-1]
    assert none.triangles.tobytes() == plain.triangles.tobytes() and none.vertices.tobytes() == plain.vertices.tobytes() and none.n_filled is None
    filled = dense_from_reconstruction(rec, s.images, min_triangles=100, fill_holes=16, colors=list(s.images), **kw)[-1]
    cleaned = plain.clean(min_triangles=100)
    ref = cleaned.fill_holes(16)
    assert filled.triangles.tobytes() == ref.triangles.tobytes() and filled.vertices.tobytes() == ref.vertices.tobytes()
    assert filled.fill_triangle_start == cleaned.n_triangles and filled.vertex_colors.shape == (filled.n_vertices,)
