"""Mesh smoothing on the device against tests/mesh_smooth_reference.py: every output byte of `sfm_mesh_adjacency`,
`sfm_mesh_smooth` and `sfm_mesh_vertex_normals`, every call twice, on the meshes of the README's table, the hand cases, the
seams of the blocks, the second level of the scan and the device's own meshes; what needs no reference; the refusals, the
capacities and the status word; and the chain through `dense_from_reconstruction`."""
import ctypes as C

import numpy as np
import pytest

import mesh_decimate_reference as dr
import mesh_reference as mr
import mesh_smooth_reference as sr

pytestmark = pytest.mark.gpu


def same(x, ref, what):
    assert x.dtype == ref.dtype and x.shape == ref.shape, (what, x.dtype, ref.dtype, x.shape, ref.shape)
    assert np.array_equal(sr.bits(x), sr.bits(ref)), (what, int((sr.bits(x) != sr.bits(ref)).sum()))


def assert_adjacency(got, want, what=""):
    assert [got.n_entries, got.n_boundary_vertices, got.n_isolated, got.n_unsound_triangles] == list(want.counts), (what, want.counts)
    for name in ("ptr", "index", "vertex_flags"):
        same(getattr(got, name), getattr(want, name), (what, name))


def assert_smoothed(got, want, src_triangles, what=""):
    """Every output of the three calls."""
    assert [got.n_pinned_boundary, got.n_pinned_given, got.n_unsound_vertices, got.n_isolated] == list(want.counts), (what, want.counts)
    assert_adjacency(got.adjacency_before, want.adjacency, what)
    same(got.vertices, want.vertices, (what, "vertices"))
    same(got.vertex_state, want.vertex_state, (what, "vertex_state"))
    same(got.normals, want.normals, (what, "normals"))
    assert got.triangles.tobytes() == np.ascontiguousarray(src_triangles, np.int32).tobytes(), what
    assert got.atlas is None and got.vertex_colors is None and got.n_views is None and got.best_view is None


def device_smooth(v, t, iterations=10, lam=0.5, mu=-0.53, pin_boundary=True, pinned=None, what=""):
    """smooth_mesh against the reference, twice."""
    from sfm_amd import smooth_mesh
    v = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
    t = np.asarray(t, np.int32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        want = sr.smooth(v, t, iterations, lam, mu, pin_boundary, pinned)
    for run in ("first run", "second run"):
        got = smooth_mesh(v, t, None, iterations, lam, mu, pin_boundary, pinned)
        assert_smoothed(got, want, t, (what, run))
    return got, want


# ------------------------------------------------------------------------------------------- the reference meshes
@pytest.mark.parametrize("iterations", [1, 2, 10])
@pytest.mark.parametrize("mu", [-0.53, None])
def test_the_analytic_sphere(gpu_ready, iterations, mu):
    s = dr.analytic_sphere()
    got, want = device_smooth(s.vertices, s.triangles, iterations, 0.5, mu, what=("sphere", iterations, mu))
    assert got.n_vertices == 1008 and got.adjacency_before.n_boundary_vertices == 0 and (got.vertex_state == 0).all()
    assert (got.vertices != s.vertices).any(axis=1).all()


@pytest.mark.parametrize("iterations", [1, 2, 10])
@pytest.mark.parametrize("mu", [-0.53, None])
def test_the_torus(gpu_ready, iterations, mu):
    m = dr.torus()
    got, want = device_smooth(m.vertices, m.triangles, iterations, 0.5, mu, what=("torus", iterations, mu))
    assert got.adjacency_before.n_entries == 2 * (2630 + 5260)


def test_other_factors_and_zero_iterations(gpu_ready):
    m = dr.torus()
    device_smooth(m.vertices, m.triangles, 3, 0.63, -0.67, what="0.63 | -0.67")
    device_smooth(m.vertices, m.triangles, 1, 1.0, -2.0, what="1 | -2")
    device_smooth(m.vertices, m.triangles, 2, 1.0, None, what="to the mean")
    for mu in (-0.53, None):
        got, want = device_smooth(m.vertices, m.triangles, 0, 0.5, mu, what="zero iterations")
        assert got.vertices.tobytes() == m.vertices.tobytes()


def test_hand_cases(gpu_ready):
    for name, v, t, pinned in sr.hand_cases():
        for pin_boundary in (True, False):
            got, want = device_smooth(v, t, 2, pinned=pinned, pin_boundary=pin_boundary, what=(name, pin_boundary))
            if name == "one triangle" and pin_boundary:
                assert got.vertices.tobytes() == v.tobytes() and got.n_pinned_boundary == 3
            if name == "a NaN and an inf vertex":
                rest = np.setdiff1d(np.arange(len(v)), [100, 500, 501])
                assert np.isfinite(got.vertices[rest]).all() and got.n_unsound_vertices == 3
            if name == "a fan of 1,000 triangles":
                assert got.adjacency_before.ptr[1] == 1000 and (got.vertices[0] != v[0]).any()
    name, v, t, pinned = sr.hand_cases()[-4]
    assert name == "a caller's pinned"
    got, want = device_smooth(v, t, 10, pinned=pinned.astype(bool), what="pinned as bool")
    assert got.n_pinned_given == int(pinned.sum()) and got.vertices[pinned != 0].tobytes() == v[pinned != 0].tobytes()


@pytest.mark.parametrize("n", [255, 256, 257, 258, 259])
def test_seams_of_the_blocks(gpu_ready, n):
    """A strip of n vertices: 6 (n - 2) keys, 4 n - 6 entries, n + 1 lanes of ptr; every vertex is on the outline, so the
    steps run with pin_boundary off."""
    v, t = dr.strip(n)
    v[:, 2] += np.random.default_rng(n).uniform(-0.3, 0.3, n)
    got, want = device_smooth(v, t, 2, pin_boundary=False, what=("strip", n))
    assert got.adjacency_before.n_entries == 4 * n - 6 and got.adjacency_before.n_boundary_vertices == n and (got.vertices != v).any(axis=1).all()
    got, want = device_smooth(v, t, 2, what=("strip, pinned", n))
    assert got.vertices.tobytes() == v.tobytes() and got.n_pinned_boundary == n


def test_the_second_scan_level(gpu_ready):
    """43,693 vertices and 43,691 triangles: 262,146 keys, one block more than the 1,024 blocks of 256 of a scan chunk, in the
    ranking of the entries."""
    n = 43693
    assert 6 * (n - 2) > 1024 * 256 >= 6 * (n - 3)
    v, t = dr.strip(n)
    v[:, 2] += np.random.default_rng(5).uniform(-0.3, 0.3, n)
    got, want = device_smooth(v, t, 1, pin_boundary=False, what="262,146 keys")
    assert got.adjacency_before.n_entries == 4 * n - 6 and got.adjacency_before.index[-1] == n - 2


# ------------------------------------------------------------------------------------------- the device's own meshes
def test_the_sphere_of_eight_cameras(gpu_ready):
    """Pin-holes where no camera looks: boundary vertices.  With pin_boundary on and off, against `Mesh.edges()`."""
    from sfm_amd.mesh import tsdf_volume_from_depth_arrays
    proj, depth, origin, voxel, shape, trunc = mr.sphere_scene(n_cams=8)
    mesh = tsdf_volume_from_depth_arrays(proj, depth, None, origin, voxel, shape, trunc).mesh(min_weight=1)
    before = (mesh.vertices.tobytes(), mesh.normals.tobytes(), mesh.triangles.tobytes())
    adj = mesh.adjacency()
    assert_adjacency(adj, sr.adjacency(mesh.triangles, mesh.n_vertices), "eight cameras")
    assert adj.n_boundary_vertices > 0 and adj.n_mesh_vertices == mesh.n_vertices
    # a vertex is boundary-flagged iff it ends a half-edge whose edge is not used exactly twice
    edges = mesh.edges()
    odd = np.flatnonzero(edges.halfedge_uses != 2)
    tri = mesh.triangles.reshape(-1)
    ends = np.zeros(mesh.n_vertices, bool)
    ends[tri[odd]] = True
    ends[mesh.triangles[:, [1, 2, 0]].reshape(-1)[odd]] = True
    assert np.array_equal((adj.vertex_flags & 1) != 0, ends) and adj.n_boundary_vertices == int(ends.sum())
    for pin_boundary in (True, False):
        want = sr.smooth(mesh.vertices, mesh.triangles, 10, pin_boundary=pin_boundary)
        for given in (None, adj):
            out = mesh.smooth(pin_boundary=pin_boundary, adjacency=given)
            assert_smoothed(out, want, mesh.triangles, ("eight cameras", pin_boundary))
            assert out._volume is mesh._volume and out is not mesh and (given is None or out.adjacency_before is adj)
        assert out.n_pinned_boundary == (adj.n_boundary_vertices if pin_boundary else 0)
        assert (out.vertices[ends].tobytes() == mesh.vertices[ends].tobytes()) == pin_boundary
    assert (mesh.vertices.tobytes(), mesh.normals.tobytes(), mesh.triangles.tobytes()) == before and mesh.vertex_state is None
    kept = mesh.smooth(3, normals="keep")
    assert kept.normals.tobytes() == mesh.normals.tobytes() and kept.vertices.tobytes() == sr.smooth(mesh.vertices, mesh.triangles, 3, normals=False).vertices.tobytes()
    from sfm_amd import mesh_adjacency
    for other in (mesh_adjacency(mesh.triangles[:-1], mesh.n_vertices), mesh_adjacency(mesh.triangles, mesh.n_vertices + 1), mesh.edges()):
        with pytest.raises(ValueError, match="MeshAdjacency of this mesh"):
            mesh.smooth(adjacency=other)


def test_recomputed_normals_point_where_the_gradient_points(gpu_ready):
    from sfm_amd import mesh_vertex_normals
    from sfm_amd.mesh import tsdf_volume_from_arrays
    f = mr.sphere_field((14, 14, 14), dr.SPHERE_CENTRE, dr.SPHERE_RADIUS)
    mesh = tsdf_volume_from_arrays(f.reshape(14, 14, 14), np.ones((14, 14, 14), np.uint16), (0.0, 0.0, 0.0), 1.0).mesh()
    s = dr.analytic_sphere()
    assert mesh.vertices.tobytes() == s.vertices.tobytes() and mesh.triangles.tobytes() == s.triangles.tobytes()
    out = mesh.recompute_normals()
    want = sr.vertex_normals(s.vertices, s.triangles)
    same(out.normals, want, "recompute_normals")
    same(mesh_vertex_normals(s.vertices, s.triangles), want, "mesh_vertex_normals")
    assert out.vertices.tobytes() == s.vertices.tobytes() and out.triangles.tobytes() == s.triangles.tobytes() and out._volume is mesh._volume
    cos = (out.normals.astype(np.float64) * mesh.normals).sum(axis=1)
    worst = float(np.degrees(np.arccos(np.clip(cos.min(), -1, 1))))
    print("worst angle between the area-weighted and the gradient normal, degrees:", round(worst, 2))
    assert cos.min() > 0.0                                          # the same side of the surface everywhere
    # a mesh without normals gets them
    from sfm_amd import decimate_mesh
    bare = decimate_mesh(s.vertices, s.triangles, None, cell=2.0)
    assert (bare.normals == 0).all()
    same(bare.recompute_normals().normals, sr.vertex_normals(bare.vertices, bare.triangles), "after decimate_mesh")


def test_properties_that_need_no_reference(gpu_ready):
    from sfm_amd import mesh_adjacency, smooth_mesh
    m = dr.scene_sphere()[0]
    rng = np.random.default_rng(3)
    order = rng.permutation(len(m.triangles))
    turned = np.stack([np.roll(t, k) for t, k in zip(m.triangles[order], rng.integers(0, 3, len(order)))])
    a, again, b = smooth_mesh(m.vertices, m.triangles), smooth_mesh(m.vertices, m.triangles), smooth_mesh(m.vertices, turned)
    for name in ("vertices", "normals", "vertex_state"):
        assert getattr(a, name).tobytes() == getattr(again, name).tobytes(), name                  # two runs, equal bytes
    # the order of the triangles: the vertices' bytes do not depend on it; the normals' bytes are claimed for a fixed order only
    assert a.vertices.tobytes() == b.vertices.tobytes() and np.abs(a.normals.astype(np.float64) - b.normals).max() < 1e-6
    adj = mesh_adjacency(m.triangles, len(m.vertices))
    assert adj.n_boundary_vertices == 0 and adj.n_isolated == 0 and (adj.vertex_flags == 0).all()     # a closed mesh has no boundary vertex
    assert adj.ptr[0] == 0 and adj.ptr[-1] == adj.n_entries == 2 * (len(m.vertices) + len(m.triangles) - 2)
    kept = smooth_mesh(m.vertices, m.triangles, m.normals, 2, normals_mode="keep")
    assert kept.normals.tobytes() == m.normals.tobytes()
    # the figures of the table from the device's vertices
    assert round(sr.face_angle_rms(a.vertices, m.triangles, (0, 0, 0)), 2) == 9.60 and round(mr.signed_volume(a.vertices, m.triangles), 4) == 4.2586


# ------------------------------------------------------------------------------------------- refusals and capacities
def test_entry_points_reject_bad_arguments(gpu_ready):
    """SFM_ERR_ARG (-1) before any device work: the data pointers are 1, 2 or null throughout, so a call that got as far as a
    launch would not return -1 but fault."""
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    p, q, big, room = C.c_void_p(1), C.c_void_p(2), (1 << 31) // 6 + 1, 1 << 40
    why = lambda: lib.sfm_last_error(h._h)
    need = C.c_int64(-1)
    assert lib.sfm_mesh_adjacency_workspace_bytes(h._h, 0, 0, C.byref(need)) == 0 and 0 < need.value <= 8192
    assert lib.sfm_mesh_adjacency_workspace_bytes(h._h, 100000, 200000, C.byref(need)) == 0 and need.value >= 200000 * 120
    assert lib.sfm_mesh_vertex_normals_workspace_bytes(h._h, 100000, 200000, C.byref(need)) == 0 and need.value >= 200000 * 48
    assert lib.sfm_mesh_smooth_workspace_bytes(h._h, 100000, C.byref(need)) == 0 and 2400000 <= need.value <= 2400000 + 512
    for nv, nt in ((-1, 0), (0, -1), (1 << 31, 0), (0, big)):
        assert lib.sfm_mesh_adjacency_workspace_bytes(h._h, nv, nt, C.byref(need)) == -1
        assert lib.sfm_mesh_vertex_normals_workspace_bytes(h._h, nv, nt, C.byref(need)) == -1
    assert lib.sfm_mesh_smooth_workspace_bytes(h._h, -1, C.byref(need)) == -1 and lib.sfm_mesh_smooth_workspace_bytes(h._h, 1 << 31, C.byref(need)) == -1
    assert lib.sfm_mesh_adjacency_workspace_bytes(h._h, 5, 2, None) == -1 and lib.sfm_mesh_smooth_workspace_bytes(h._h, 5, None) == -1
    assert lib.sfm_mesh_vertex_normals_workspace_bytes(h._h, 5, 2, None) == -1

    def adjacency(nv=5, nt=2, tri=p, ptr=p, index=p, flags=p, counts=p, ws=p, ws_bytes=room):
        return lib.sfm_mesh_adjacency(h._h, nv, nt, tri, ptr, index, flags, counts, ws, ws_bytes)

    def smooth(nv=5, vin=p, ptr=p, index=p, ni=12, flags=p, pinned=None, pin=1, lam=0.5, mu=-0.53, has_mu=1, it=10, vout=q, state=p, counts=p, ws=p, ws_bytes=room):
        return lib.sfm_mesh_smooth(h._h, nv, vin, ptr, index, ni, flags, pinned, pin, lam, mu, has_mu, it, vout, state, counts, ws, ws_bytes)

    def normals(nv=5, nt=2, v=p, tri=p, out=p, ws=p, ws_bytes=room):
        return lib.sfm_mesh_vertex_normals(h._h, nv, nt, v, tri, out, ws, ws_bytes)

    nan, inf = float("nan"), float("inf")
    for call, cases in ((adjacency, [dict(nv=-1), dict(nt=-1), dict(nv=1 << 31), dict(nt=big), dict(tri=None), dict(ptr=None), dict(index=None), dict(flags=None),
                                     dict(counts=None), dict(ws=None), dict(ws_bytes=64)]),
                        (smooth, [dict(nv=-1), dict(nv=1 << 31), dict(ni=-1), dict(ni=1 << 31), dict(it=-1), dict(it=1001), dict(lam=0.0), dict(lam=-0.5), dict(lam=1.5),
                                  dict(lam=nan), dict(lam=inf), dict(mu=-0.5), dict(mu=0.3), dict(mu=-2.5), dict(mu=nan), dict(mu=-inf), dict(vin=None), dict(ptr=None),
                                  dict(index=None), dict(flags=None), dict(vout=None), dict(state=None), dict(counts=None), dict(vout=p), dict(ws=None), dict(ws_bytes=64)]),
                        (normals, [dict(nv=-1), dict(nt=-1), dict(nv=1 << 31), dict(nt=big), dict(v=None), dict(tri=None), dict(out=None), dict(ws=None),
                                   dict(ws_bytes=64)])):
        for kw in cases:
            assert call(**kw) == -1, (call.__name__, kw)
            null = any(v is None for k, v in kw.items() if k != "ws")
            assert why().endswith(b": null pointer") == null, (call.__name__, kw, why())
    # the firing order of sfm_mesh_smooth: the sizes, n_index, iterations, lam, mu, the pointers, the two arrays, the workspace
    assert smooth(nv=-1, ni=-1, it=-1, lam=0.0, mu=0.0, vin=None, ws=None) == -1 and b"n_vertices" in why()
    assert smooth(ni=-1, it=-1, lam=0.0, mu=0.0, vin=None, ws=None) == -1 and b"n_index" in why()
    assert smooth(it=-1, lam=0.0, mu=0.0, vin=None, ws=None) == -1 and b"iterations" in why()
    assert smooth(lam=0.0, mu=0.0, vin=None, ws=None) == -1 and b"lam must" in why()
    assert smooth(mu=0.0, vin=None, ws=None) == -1 and b"mu must" in why()
    assert smooth(vin=None, vout=None, ws=None) == -1 and why().endswith(b": null pointer")
    assert smooth(vout=p, ws=None) == -1 and b"vertices_out" in why()
    assert smooth(ws=None) == -1 and b"workspace" in why()
    # without mu its value is not looked at; pinned may be null; index may be null without entries
    import torch
    counts = torch.full((5,), 7, dtype=torch.int64, device="cuda:0")
    ws = torch.empty(256, dtype=torch.uint8, device="cuda:0")
    assert smooth(nv=0, has_mu=0, mu=nan, vin=None, index=None, ni=0, flags=None, vout=None, state=None, counts=C.c_void_p(counts.data_ptr()),
                  ws=C.c_void_p(ws.data_ptr()), ws_bytes=256) == 0
    assert counts.cpu().tolist() == [0] * 5


def test_nothing_is_written_beyond_the_capacities_and_a_foreign_table_raises_the_status(gpu_ready):
    import torch
    from sfm_amd import _lib
    m = dr.scene_sphere(8)[0]
    v, t = m.vertices, m.triangles
    nv, nt = len(v), len(t)
    want = sr.smooth(v, t, 3)
    adj = want.adjacency
    ne = adj.counts[0]
    assert adj.counts[1] > 0
    dev = torch.device("cuda", 0)
    h = _lib.get_handle(0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dp = lambda x: C.c_void_p(x.data_ptr())
    d_v, d_t = up(v), up(t)
    guard = 64
    full = lambda n, dtype, value=7: torch.full((n + guard,), value, dtype=dtype, device=dev)
    need = C.c_int64()
    h.call("sfm_mesh_adjacency_workspace_bytes", nv, nt, C.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    ptr, index, flags, counts = full(nv + 1, torch.int32), full(6 * nt, torch.int32), full(nv, torch.uint8), full(4, torch.int64)
    h.call("sfm_mesh_adjacency", nv, nt, dp(d_t), dp(ptr), dp(index), dp(flags), dp(counts), dp(ws), need.value)
    ptr_h, index_h, flags_h, counts_h = (x.cpu().numpy() for x in (ptr, index, flags, counts))
    assert counts_h[:4].tolist() == adj.counts and (counts_h[4:] == 7).all()
    assert ptr_h[:nv + 1].tobytes() == adj.ptr.tobytes() and (ptr_h[nv + 1:] == 7).all()
    assert index_h[:ne].tobytes() == adj.index.tobytes() and (index_h[ne:] == 7).all()                 # nothing behind the entries
    assert flags_h[:nv].tobytes() == adj.vertex_flags.tobytes() and (flags_h[nv:] == 7).all()

    h.call("sfm_mesh_smooth_workspace_bytes", nv, C.byref(need))
    ws2 = torch.empty(need.value, dtype=torch.uint8, device=dev)

    def smooth(d_ptr, d_index, n_index, iterations=3):
        out = torch.full((nv + guard, 3), 7.0, dtype=torch.float64, device=dev)
        state, c = full(nv, torch.uint8), full(5, torch.int64)
        h.call("sfm_mesh_smooth", nv, dp(d_v), dp(d_ptr), dp(d_index), n_index, dp(flags), None, 1, C.c_double(0.5), C.c_double(-0.53), 1, iterations,
               dp(out), dp(state), dp(c), dp(ws2), need.value)
        out, state, c = (x.cpu().numpy() for x in (out, state, c))
        assert (out[nv:] == 7.0).all() and (state[nv:] == 7).all() and (c[5:] == 7).all()
        return out[:nv], state[:nv], c[:5].tolist()

    for n_index in (ne, 6 * nt):                                    # the entries, or the capacity
        out, state, c = smooth(ptr, index, n_index)
        assert out.tobytes() == want.vertices.tobytes() and state.tobytes() == want.vertex_state.tobytes() and c == want.counts + [0]
    out, state, c = smooth(ptr, index, ne, iterations=0)
    assert out.tobytes() == v.tobytes() and c == want.counts + [0]
    d_n = torch.full((nv + guard, 3), 7.0, dtype=torch.float32, device=dev)
    h.call("sfm_mesh_vertex_normals_workspace_bytes", nv, nt, C.byref(need))
    ws3 = torch.empty(need.value, dtype=torch.uint8, device=dev)
    h.call("sfm_mesh_vertex_normals", nv, nt, dp(up(want.vertices)), dp(d_t), dp(d_n), dp(ws3), need.value)
    d_n = d_n.cpu().numpy()
    assert d_n[:nv].tobytes() == want.normals.tobytes() and (d_n[nv:] == 7.0).all()

    # tables that are not of these triangles: the status word, finite vertices, and no address outside the arrays
    free = int(np.flatnonzero(want.vertex_state == 0)[0])
    for what, bad_ptr, bad_index, n_index in (
            ("an entry at n_vertices", adj.ptr, np.where(np.arange(ne) == adj.ptr[free], nv, adj.index), ne),
            ("a negative entry", adj.ptr, np.where(np.arange(ne) == adj.ptr[free], -5, adj.index), ne),
            ("an entry of 2^31 - 1", adj.ptr, np.where(np.arange(ne) == adj.ptr[free] + 1, 0x7FFFFFFF, adj.index), ne),
            ("a decreasing ptr", np.where(np.arange(nv + 1) == free + 1, adj.ptr[free] - 1, adj.ptr), adj.index, ne),
            ("a ptr past the entries", np.where(np.arange(nv + 1) == nv, ne + 1000000, adj.ptr), adj.index, ne),
            ("a negative ptr", np.where(np.arange(nv + 1) == free, -3, adj.ptr), adj.index, ne),
            ("fewer entries than ptr says", adj.ptr, adj.index, ne - 1)):
        out, state, c = smooth(up(bad_ptr.astype(np.int32)), up(bad_index.astype(np.int32)), n_index)
        assert c[4] == 1 and c[:4] == want.counts and np.isfinite(out).all(), what
    # the Python layer turns the status word into an error
    from sfm_amd import mesh_adjacency
    from sfm_amd.mesh_smooth import _smooth
    wrong = mesh_adjacency(t, nv)
    wrong._m["ptr"] = up(np.where(np.arange(nv + 1) == free + 1, adj.ptr[free] - 1, adj.ptr).astype(np.int32))
    with pytest.raises(ValueError, match="not that of these triangles"):
        _smooth(dev, wrong, nv, d_v, 1, 0.5, -0.53, True, None)


# ------------------------------------------------------------------------------------------- the chain
def test_dense_from_reconstruction_smooths_the_mesh(gpu_ready):
    """smooth of `dense_from_reconstruction`: with None the mesh is the one of before; with an iteration count it is smoothed
    after the cleaning and the filling and before the decimation, and colors(), texture(), render_views() and score() accept
    it.  The scores are printed beside those of the unsmoothed chain, not asserted."""
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
    filled = dense_from_reconstruction(rec, s.images, fill_holes=16, **kw)[-1]
    none = dense_from_reconstruction(rec, s.images, fill_holes=16, smooth=None, **kw)[-1]
    assert none.triangles.tobytes() == filled.triangles.tobytes() and none.vertices.tobytes() == filled.vertices.tobytes() and none.vertex_state is None
    plain = dense_from_reconstruction(rec, s.images, fill_holes=16, decimate=2.0, colors=images, texture=4, **kw)[-1]
    smooth = dense_from_reconstruction(rec, s.images, fill_holes=16, smooth=10, decimate=2.0, colors=images, texture=4, **kw)[-1]
    between = filled.smooth(10)
    same(between.vertices, sr.smooth(filled.vertices, filled.triangles, 10).vertices, "the filled mesh, smoothed")
    ref = between.decimate(factor=2.0)
    assert smooth.triangles.tobytes() == ref.triangles.tobytes() and smooth.vertices.tobytes() == ref.vertices.tobytes()
    assert smooth.vertex_colors.shape == (smooth.n_vertices,) and smooth.atlas.n_triangles == smooth.n_triangles
    for name, mesh in (("decimated", plain), ("smoothed and decimated", smooth)):
        render = mesh.render_views()
        score = mesh.score(images)
        assert render.sizes == [(96, 72)] * 3 and len(score.psnr) == 3 and (score.n_compared > 0).all()
        print(name, mesh.n_vertices, mesh.n_triangles, "coverage", np.round(render.coverage, 4).tolist(), "psnr", np.round(score.psnr, 2).tolist(),
              "ssim", np.round(score.ssim, 4).tolist(), "mae", np.round(score.mae.reshape(-1), 2).tolist(), "depth_agree", np.round(score.depth_agree, 4).tolist())
