"""Decimation by vertex clustering on the device against tests/mesh_decimate_reference.py: every output byte of
`sfm_mesh_decimate_cluster`, `sfm_mesh_decimate_mark` and `sfm_mesh_decimate_emit`, every call twice, on the meshes of the
README's table, the hand cases, the seams of the block scan, the two-pass sort of the triples and the device's own meshes;
what needs no reference; the refusals and the capacities; and the chain through `dense_from_reconstruction`."""
import ctypes as C

import numpy as np
import pytest

import mesh_decimate_reference as dr
import mesh_reference as mr

pytestmark = pytest.mark.gpu

PLACEMENTS = {0: "mean", 1: "quadric"}


def assert_decimated(got, want, nv, what=""):
    """Every output of the three calls."""
    mine = [got.n_vertices, got.n_unsound_vertices, got.n_triangles, got.n_unsound_triangles, got.n_degenerate, got.n_cancelled]
    assert mine == list(want.counts) + list(want.marks[:4]), (what, mine, want.counts, want.marks)
    assert got.n_source_vertices == nv and got.cell == want.cell and got.origin.tobytes() == want.origin.tobytes(), what
    for name, dtype in (("vertex_cluster", np.int32), ("cluster_first", np.int32), ("cluster_size", np.int32), ("cluster_placed", np.uint8),
                        ("vertices", np.float64), ("normals", np.float32), ("triangles", np.int32), ("triangle_map", np.int32)):
        x, ref = getattr(got, name), getattr(want, name)
        assert x.dtype == dtype and x.shape == ref.shape, (what, name, x.dtype, x.shape, ref.shape)
        assert np.array_equal(dr.bits(x), dr.bits(ref)), (what, name, int((dr.bits(x) != dr.bits(ref)).sum()))
    assert got.atlas is None and got.vertex_colors is None and got.n_views is None and got.best_view is None


def device_decimate(v, t, n, cell, origin, placement, what=""):
    """decimate_mesh against the reference, twice."""
    from sfm_amd import decimate_mesh
    v = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
    t = np.asarray(t, np.int32).reshape(-1, 3)
    want = dr.decimate(v, t, n, cell, origin, placement)
    for run in ("first run", "second run"):
        got = decimate_mesh(v, t, n, cell=cell, origin=origin, placement=PLACEMENTS[placement])
        assert_decimated(got, want, len(v), (what, run))
    return got, want


# ------------------------------------------------------------------------------------------- the reference meshes
@pytest.mark.parametrize("cell", [1.5, 2.0, 3.0])
@pytest.mark.parametrize("placement", [0, 1])
def test_the_analytic_sphere(gpu_ready, cell, placement):
    s = dr.analytic_sphere()
    got, want = device_decimate(s.vertices, s.triangles, s.normals, cell, np.zeros(3), placement, ("sphere", cell))
    assert (got.n_vertices, got.n_triangles, got.n_cancelled) == {1.5: (140, 276, 0), 2.0: (85, 164, 4), 3.0: (44, 84, 0)}[cell]
    assert mr.is_closed_and_oriented(got.triangles) and got.edges().is_closed and got.edges().euler == 2
    device_decimate(s.vertices, s.triangles, None, cell, None, placement, ("sphere without normals, origin by default", cell))


@pytest.mark.parametrize("placement", [0, 1])
def test_the_torus_pinches(gpu_ready, placement):
    m = dr.torus()
    got, want = device_decimate(m.vertices, m.triangles, m.normals, 2.0, np.zeros(3), placement, "torus")
    assert (got.n_vertices, got.n_triangles) == (212, 432) and got.edges().n_nonmanifold_edges == 5


@pytest.mark.parametrize("placement", [0, 1])
def test_hand_cases(gpu_ready, placement):
    for name, v, t, n, cell, origin in dr.hand_cases():
        device_decimate(v, t, n, cell, origin, placement, name)


@pytest.mark.parametrize("n", [255, 256, 257, 258, 259])
def test_seams_of_the_blocks(gpu_ready, n):
    """n vertices in n cells with n - 2 triangles, all kept: 255 / 256 / 257 of each; then four vertices to a cell."""
    v, t = dr.strip(n)
    normals = np.random.default_rng(n).normal(size=v.shape).astype(np.float32)
    got, want = device_decimate(v, t, normals, 1.0, np.zeros(3), 1, ("strip", n))
    assert (got.n_vertices, got.n_triangles, got.n_degenerate) == (n, n - 2, 0) and got.triangle_map.tolist() == list(range(n - 2))
    v, t = dr.strip(n, 0.5)
    v += np.random.default_rng(n).uniform(-0.2, 0.2, size=v.shape)
    got, want = device_decimate(v, t, normals, 1.0, np.zeros(3), 1, ("strip, two to a cell", n))
    assert got.n_vertices < n and got.n_degenerate > 0


def test_the_second_scan_level(gpu_ready):
    """262,147 vertices in as many cells and 262,145 triangles: one more than the 1,024 blocks of 256 of a scan chunk, in the
    numbering of the clusters and in the compaction of the triangles."""
    n = 1024 * 256 + 3
    v, t = dr.strip(n)
    got, want = device_decimate(v, t, None, 1.0, np.zeros(3), 1, "262,147")
    assert (got.n_vertices, got.n_triangles) == (n, n - 2) and got.triangle_map[-1] == n - 3 and got.vertex_cluster[-1] >= 0


def test_more_clusters_than_three_fields_of_a_key_hold(gpu_ready):
    """2,100,000 vertices in as many cells, past 2^21: a cluster number needs 22 bits, three need 66, and the triples are
    sorted in two stable passes; duplicates of every kind among them."""
    nx, ny = 2100, 1000
    j, i = np.mgrid[0:ny, 0:nx]
    v = np.stack([i.ravel() + 0.5, j.ravel() + 0.5, np.full(nx * ny, 0.5)], axis=1)
    rng = np.random.default_rng(21)
    t = rng.integers(0, nx * ny, size=(4000, 3)).astype(np.int32)
    t[:1000] = nx * ny - 1 - rng.integers(0, 3000, size=(1000, 3))               # many share their largest cluster
    dup = t[rng.integers(0, 4000, 1500)]
    dup[::2] = dup[::2][:, [1, 0, 2]]
    dup[::3] = np.roll(dup[::3], 1, axis=1)
    t = np.concatenate([t, dup])[rng.permutation(5500)]
    got, want = device_decimate(v, t, None, 1.0, np.zeros(3), 0, "2,100,000 clusters")
    assert got.n_vertices == nx * ny > 1 << 21 and got.n_cancelled > 500 and 2000 < got.n_triangles < 4000


# ------------------------------------------------------------------------------------------- the device's own meshes
def test_the_sphere_of_eight_cameras_filled_and_decimated(gpu_ready):
    from sfm_amd.mesh import tsdf_volume_from_depth_arrays
    proj, depth, origin, voxel, shape, trunc = mr.sphere_scene(n_cams=8)
    mesh = tsdf_volume_from_depth_arrays(proj, depth, None, origin, voxel, shape, trunc).mesh().fill_holes()
    before = (mesh.vertices.tobytes(), mesh.normals.tobytes(), mesh.triangles.tobytes())
    for placement in ("quadric", "mean"):
        out = mesh.decimate(placement=placement)
        want = dr.decimate(mesh.vertices, mesh.triangles, mesh.normals, 2.0 * voxel, None, int(placement == "quadric"))
        assert_decimated(out, want, mesh.n_vertices, ("sphere of eight cameras", placement))
        assert out._volume is mesh._volume and out.cell == 2.0 * voxel and out.origin.tolist() == mesh.vertices.min(axis=0).tolist()
        assert out.n_triangles < mesh.n_triangles // 8 and out is not mesh and mesh.n_degenerate is None
    assert (mesh.vertices.tobytes(), mesh.normals.tobytes(), mesh.triangles.tobytes()) == before
    at = mesh.decimate(cell=3.0 * voxel, origin=origin)
    assert_decimated(at, dr.decimate(mesh.vertices, mesh.triangles, mesh.normals, 3.0 * voxel, np.asarray(origin, np.float64), 1), mesh.n_vertices, "cell and origin given")
    with pytest.raises(ValueError, match="2\\^21"):
        mesh.decimate(cell=1e-7)


def test_the_default_scene_mesh_at_factor_two(gpu_ready):
    """The open mesh of the default scene, with its outlines: every byte, and the stages behind accept it."""
    from test_mesh_texture_gpu import default_scene_maps
    s, maps = default_scene_maps()
    mesh = maps.tsdf(resolution=64).mesh()
    out = mesh.decimate(factor=2.0)
    want = dr.decimate(mesh.vertices, mesh.triangles, mesh.normals, 2.0 * mesh._volume.voxel, None, 1)
    assert_decimated(out, want, mesh.n_vertices, "default scene")
    assert out.n_triangles < mesh.n_triangles // 3 and out.edges().n_boundary_edges > 0
    images = list(s.images)
    assert out.colors(images).shape == (out.n_vertices,) and out.texture(images, texels=4).n_triangles == out.n_triangles
    assert out.render_views().sizes == [(96, 72)] * 3


# ------------------------------------------------------------------------------------------- what needs no reference
def test_properties_that_need_no_reference(gpu_ready):
    from sfm_amd import decimate_mesh
    m, voxel = dr.scene_sphere()
    origin = np.full(3, -1.4)
    rng = np.random.default_rng(3)
    order = rng.permutation(len(m.triangles))
    turned = np.stack([np.roll(t, k) for t, k in zip(m.triangles[order], rng.integers(0, 3, len(order)))])
    a = decimate_mesh(m.vertices, m.triangles, m.normals, cell=2 * voxel, origin=origin)
    b = decimate_mesh(m.vertices, turned, m.normals, cell=2 * voxel, origin=origin)
    again = decimate_mesh(m.vertices, m.triangles, m.normals, cell=2 * voxel, origin=origin)
    for name in ("vertices", "normals", "triangles", "triangle_map", "vertex_cluster", "cluster_placed"):
        assert getattr(a, name).tobytes() == getattr(again, name).tobytes(), name                  # two runs, equal bytes
    # the order of the triangles: the sums of the quadric walk them in another order, so the mean placement is compared
    a0 = decimate_mesh(m.vertices, m.triangles, m.normals, cell=2 * voxel, origin=origin, placement="mean")
    b0 = decimate_mesh(m.vertices, turned, m.normals, cell=2 * voxel, origin=origin, placement="mean")
    assert a0.vertices.tobytes() == b0.vertices.tobytes() and a0.normals.tobytes() == b0.normals.tobytes()
    canon = lambda t: sorted(tuple(np.roll(x, -int(np.argmin(x)))) for x in t.tolist())
    assert canon(a.triangles) == canon(b.triangles) == canon(a0.triangles) and (a.n_degenerate, a.n_cancelled) == (b.n_degenerate, b.n_cancelled)
    same = a.cluster_placed == b.cluster_placed                   # a sum that rounds otherwise may tip a box test, rarely
    assert same.mean() > 0.99 and np.abs(a.vertices - b.vertices)[same].max() < 1e-6 * voxel
    # a cell smaller than every edge: the triangles come back, the vertices in key order (the mean of one vertex is the vertex)
    s = dr.analytic_sphere()
    d = decimate_mesh(s.vertices, s.triangles, s.normals, cell=2.0 ** -16, origin=np.zeros(3), placement="mean")
    assert (d.n_vertices, d.n_triangles, d.n_degenerate, d.n_cancelled) == (len(s.vertices), len(s.triangles), 0, 0)
    assert d.triangles.tobytes() == d.vertex_cluster[s.triangles].astype(np.int32).tobytes() and d.vertices[d.vertex_cluster].tobytes() == s.vertices.tobytes()
    assert (d.cluster_size == 1).all() and d.cluster_first[d.vertex_cluster].tolist() == list(range(len(s.vertices)))
    keys = np.floor(d.vertices * 65536.0).astype(np.int64)
    assert (np.diff((keys[:, 2] << 42) | (keys[:, 1] << 21) | keys[:, 0]) > 0).all()


# ------------------------------------------------------------------------------------------- refusals and capacities
def test_entry_points_reject_bad_arguments(gpu_ready):
    """SFM_ERR_ARG (-1) before any device work: the data pointers are 1 or null throughout, so a call that got as far as a
    launch would not return -1 but fault."""
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    p, big, room = C.c_void_p(1), (1 << 31) // 3 + 1, 1 << 30
    why = lambda: lib.sfm_last_error(h._h)
    need = C.c_int64(-1)
    assert lib.sfm_mesh_decimate_workspace_bytes(h._h, 0, 0, C.byref(need)) == 0 and 0 < need.value <= 8192
    assert lib.sfm_mesh_decimate_workspace_bytes(h._h, 100000, 200000, C.byref(need)) == 0 and need.value >= 100000 * 24 + 200000 * 80
    for nv, nt in ((-1, 0), (0, -1), (1 << 31, 0), (0, big)):
        assert lib.sfm_mesh_decimate_workspace_bytes(h._h, nv, nt, C.byref(need)) == -1
    assert lib.sfm_mesh_decimate_workspace_bytes(h._h, 5, 2, None) == -1
    good = (C.c_double * 3)(0.0, 0.0, 0.0)
    hp = lambda a: C.cast(a, C.c_void_p)
    origins = {"nan": (C.c_double * 3)(0.0, float("nan"), 0.0), "inf": (C.c_double * 3)(float("inf"), 0.0, 0.0)}

    def cluster(nv=5, nt=2, v=p, origin=hp(good), cell=1.0, vc=p, start=p, first=p, size=p, counts=p, ws=p, ws_bytes=room):
        return lib.sfm_mesh_decimate_cluster(h._h, nv, nt, v, origin, cell, vc, start, first, size, counts, ws, ws_bytes)

    def mark(nv=5, nt=2, nc=3, tri=p, vc=p, keep=p, counts=p, ws=p, ws_bytes=room):
        return lib.sfm_mesh_decimate_mark(h._h, nv, nt, nc, tri, vc, keep, counts, ws, ws_bytes)

    def emit(nv=5, nt=2, nc=3, v=p, n=p, tri=p, vc=p, start=p, keep=p, origin=hp(good), cell=1.0, placement=1, cap_c=3, cap_t=2, nv_out=p, nn=p,
             placed=p, nt_out=p, tmap=p, ws=p, ws_bytes=room):
        return lib.sfm_mesh_decimate_emit(h._h, nv, nt, nc, v, n, tri, vc, start, keep, origin, cell, placement, cap_c, cap_t, nv_out, nn, placed, nt_out,
                                          tmap, ws, ws_bytes)

    grid = [dict(origin=hp(origins["nan"])), dict(origin=hp(origins["inf"])), dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf"))]
    for call, cases in ((cluster, [dict(nv=-1), dict(nt=-1), dict(nv=1 << 31), dict(nt=big), dict(v=None), dict(origin=None), dict(vc=None), dict(start=None),
                                   dict(first=None), dict(size=None), dict(counts=None), dict(ws=None), dict(ws_bytes=64)] + grid),
                        (mark, [dict(nv=-1), dict(nt=big), dict(nc=-1), dict(nc=6), dict(tri=None), dict(vc=None), dict(keep=None), dict(counts=None),
                                dict(ws=None), dict(ws_bytes=64)]),
                        (emit, [dict(nv=1 << 31), dict(nt=-1), dict(nc=6), dict(nc=-1), dict(cap_c=-1), dict(cap_t=-1), dict(cap_c=1 << 31), dict(cap_t=1 << 31),
                                dict(placement=2), dict(placement=-1), dict(v=None), dict(tri=None), dict(vc=None), dict(start=None), dict(keep=None),
                                dict(origin=None), dict(nv_out=None), dict(nn=None), dict(placed=None), dict(nt_out=None), dict(tmap=None), dict(ws=None),
                                dict(ws_bytes=64)] + grid)):
        for kw in cases:
            assert call(**kw) == -1, (call.__name__, kw)
            null = any(v is None for k, v in kw.items() if k != "ws")
            assert why().endswith(b": null pointer") == null, (call.__name__, kw, why())
    # the firing order: the sizes in front of the pointers in front of the grid in front of the workspace
    assert cluster(nv=-1, v=None, cell=0.0, ws=None) == -1 and b"n_vertices" in why()
    assert cluster(v=None, cell=0.0, ws=None) == -1 and why().endswith(b": null pointer")
    assert cluster(cell=0.0, ws=None) == -1 and b"cell" in why()
    assert emit(nc=6, cap_c=-1, placement=7, cell=0.0, ws=None) == -1 and b"n_clusters" in why()
    assert emit(cap_c=-1, placement=7, cell=0.0, ws=None) == -1 and b"capacity" in why()
    assert emit(placement=7, cell=0.0, ws=None) == -1 and b"placement" in why()
    assert emit(cell=0.0, ws=None) == -1 and b"cell" in why()
    assert emit(ws=None, v=None) == -1 and b"workspace" in why()
    # nothing to emit: returns at once, whatever the pointers; normals may be absent
    assert emit(cap_c=0, cap_t=0, v=None, n=None, tri=None, vc=None, start=None, keep=None, nv_out=None, nn=None, placed=None, nt_out=None, tmap=None) == 0


def test_emit_writes_nothing_at_or_above_the_capacities(gpu_ready):
    import torch
    from sfm_amd import _lib
    m, voxel = dr.scene_sphere()
    v, t, n = m.vertices, m.triangles, m.normals
    origin, cell = np.full(3, -1.4), 2.0 * voxel
    want = dr.decimate(v, t, n, cell, origin, 1)
    nv, nt, nc, kept = len(v), len(t), want.counts[0], want.marks[0]
    dev = torch.device("cuda", 0)
    h = _lib.get_handle(0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dp = lambda x: C.c_void_p(x.data_ptr())
    d_v, d_n, d_t = up(v), up(n), up(t)
    need = C.c_int64()
    h.call("sfm_mesh_decimate_workspace_bytes", nv, nt, C.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    guard = 64
    i32 = lambda k: torch.full((k + guard,), 7, dtype=torch.int32, device=dev)
    vc, start, first, size = i32(nv), i32(nv + 1), i32(nv), i32(nv)
    keep = torch.full((nt + guard,), 7, dtype=torch.uint8, device=dev)
    counts, marks = torch.full((2 + guard,), 7, dtype=torch.int64, device=dev), torch.full((5 + guard,), 7, dtype=torch.int64, device=dev)
    o = np.ascontiguousarray(origin)
    hp = C.c_void_p(o.ctypes.data)
    h.call("sfm_mesh_decimate_cluster", nv, nt, dp(d_v), hp, C.c_double(cell), dp(vc), dp(start), dp(first), dp(size), dp(counts), dp(ws), need.value)
    assert counts.cpu().numpy()[:2].tolist() == want.counts and (counts.cpu().numpy()[2:] == 7).all()
    h.call("sfm_mesh_decimate_mark", nv, nt, nc, dp(d_t), dp(vc), dp(keep), dp(marks), dp(ws), need.value)
    assert marks.cpu().numpy()[:5].tolist() == want.marks and (marks.cpu().numpy()[5:] == 7).all()
    vc_h, start_h, first_h, size_h, keep_h = (x.cpu().numpy() for x in (vc, start, first, size, keep))
    assert vc_h[:nv].tobytes() == want.vertex_cluster.tobytes() and (vc_h[nv:] == 7).all() and (start_h[nc + 1:] == 7).all() and start_h[nc] == nv
    assert first_h[:nc].tobytes() == want.cluster_first.tobytes() and (first_h[nc:] == 7).all() and size_h[:nc].tobytes() == want.cluster_size.tobytes()
    assert (size_h[nc:] == 7).all() and (keep_h[nt:] == 7).all() and np.flatnonzero(keep_h[:nt]).tolist() == want.triangle_map.tolist()
    for cap_c, cap_t in ((nc, kept), (nc - 75, kept - 300), (17, 0), (0, 50)):
        out_v = torch.full((nc + guard, 3), 7.0, dtype=torch.float64, device=dev)
        out_n = torch.full((nc + guard, 3), 7.0, dtype=torch.float32, device=dev)
        placed = torch.full((nc + guard,), 7, dtype=torch.uint8, device=dev)
        out_t = torch.full((kept + guard, 3), 7, dtype=torch.int32, device=dev)
        tmap = torch.full((kept + guard,), 7, dtype=torch.int32, device=dev)
        h.call("sfm_mesh_decimate_emit", nv, nt, nc, dp(d_v), dp(d_n), dp(d_t), dp(vc), dp(start), dp(keep), hp, C.c_double(cell), 1, cap_c, cap_t,
               dp(out_v), dp(out_n), dp(placed), dp(out_t), dp(tmap), dp(ws), need.value)
        out_v, out_n, placed, out_t, tmap = (x.cpu().numpy() for x in (out_v, out_n, placed, out_t, tmap))
        assert (out_v[cap_c:] == 7.0).all() and (out_n[cap_c:] == 7.0).all() and (placed[cap_c:] == 7).all() and (out_t[cap_t:] == 7).all() and (tmap[cap_t:] == 7).all()
        assert out_v[:cap_c].tobytes() == want.vertices[:cap_c].tobytes() and out_n[:cap_c].tobytes() == want.normals[:cap_c].tobytes()
        assert placed[:cap_c].tobytes() == want.cluster_placed[:cap_c].tobytes()
        assert out_t[:cap_t].tobytes() == want.triangles[:cap_t].tobytes() and tmap[:cap_t].tobytes() == want.triangle_map[:cap_t].tobytes()
    # without normals none is written
    out_v = torch.full((nc, 3), 7.0, dtype=torch.float64, device=dev)
    out_n = torch.full((nc, 3), 7.0, dtype=torch.float32, device=dev)
    placed = torch.full((nc,), 7, dtype=torch.uint8, device=dev)
    h.call("sfm_mesh_decimate_emit", nv, nt, nc, dp(d_v), None, dp(d_t), dp(vc), dp(start), dp(keep), hp, C.c_double(cell), 1, nc, 0, dp(out_v), dp(out_n),
           dp(placed), None, None, dp(ws), need.value)
    assert out_v.cpu().numpy().tobytes() == want.vertices.tobytes() and (out_n.cpu().numpy() == 7.0).all()
    # a vertex_cluster that is not the call's raises the status word and addresses nothing outside the arrays
    wrong = torch.full((nv,), nc + 5, dtype=torch.int32, device=dev)
    h.call("sfm_mesh_decimate_mark", nv, nt, nc, dp(d_t), dp(wrong), dp(keep), dp(marks), dp(ws), need.value)
    assert marks.cpu().numpy()[:5].tolist() == [0, nt, 0, 0, 1]


# ------------------------------------------------------------------------------------------- the chain
def test_dense_from_reconstruction_decimates_the_mesh(gpu_ready):
    """decimate of `dense_from_reconstruction`: with None the mesh is the one of before; with a factor it is decimated after
    the cleaning and the filling, and colors(), texture(), render_views() and score() accept it.  The scores are printed, not
    asserted."""
    from sfm_amd import Reconstruction, Tracks, dense_from_reconstruction
    import depth_reference as dref
    s = dref.default_scene()
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
    images = list(s.images)
    full = dense_from_reconstruction(rec, s.images, fill_holes=16, **kw)[-1]
    none = dense_from_reconstruction(rec, s.images, fill_holes=16, decimate=None, **kw)[-1]
    assert none.triangles.tobytes() == full.triangles.tobytes() and none.vertices.tobytes() == full.vertices.tobytes() and none.n_degenerate is None
    small = dense_from_reconstruction(rec, s.images, fill_holes=16, decimate=2.0, colors=images, texture=4, **kw)[-1]
    ref = full.decimate(factor=2.0)
    assert small.triangles.tobytes() == ref.triangles.tobytes() and small.vertices.tobytes() == ref.vertices.tobytes()
    assert small.n_triangles < full.n_triangles // 3 and small.vertex_colors.shape == (small.n_vertices,) and small.atlas.n_triangles == small.n_triangles
    full.colors(images)
    full.texture(images, texels=4)
    for name, mesh in (("full", full), ("decimated", small)):
        render = mesh.render_views()
        score = mesh.score(images)
        assert render.sizes == [(96, 72)] * 3 and len(score.psnr) == 3 and (score.n_compared > 0).all()
        print(name, mesh.n_vertices, mesh.n_triangles, "coverage", np.round(render.coverage, 4).tolist(), "psnr", np.round(score.psnr, 2).tolist(),
              "ssim", np.round(score.ssim, 4).tolist(), "mae", np.round(score.mae.reshape(-1), 2).tolist(), "depth_agree", np.round(score.depth_agree, 4).tolist())
