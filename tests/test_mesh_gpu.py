"""The TSDF integration and marching tetrahedra on the device against tests/mesh_reference.py: every output byte - tsdf,
weight, vertices, normals, triangles - on grids of a few to a few hundred thousand nodes, then the chain from the sweep on
the default scene to a PLY file.

The float32 normals and the float64 vertices are compared bit for bit like everything else: sqrt and / in float64 are
correctly rounded on the device."""
import numpy as np
import pytest

import depth_reference as dr
import mesh_reference as mr
from test_mesh_reference import PLANE_SHARE, plane_share, read_ply_mesh

pytestmark = pytest.mark.gpu


def device_mesh(f, w, origin, voxel, shape, min_weight=1):
    from sfm_amd import tsdf_volume_from_arrays
    nx, ny, nz = shape
    vol = tsdf_volume_from_arrays(np.asarray(f, np.float32).reshape(nz, ny, nx), np.asarray(w, np.uint16).reshape(nz, ny, nx), origin, voxel)
    return vol.mesh(min_weight)


def assert_mesh_equal(f, w, origin, voxel, shape, min_weight=1, what=""):
    got = device_mesh(f, w, origin, voxel, shape, min_weight)
    want = mr.mesh(f, w, origin, voxel, shape, min_weight)
    assert got.n_vertices == len(want.vertices) and got.n_triangles == len(want.triangles), (what, got.n_vertices, got.n_triangles)
    mr.assert_same_mesh(got, want, what)
    return got, want


def random_field(rng, shape, unknown=0.1, zeros=0.1, nan=0.03):
    """Values around zero, some exactly zero, some nodes without weight, some NaN or infinite at nodes with weight."""
    n = shape[0] * shape[1] * shape[2]
    f = rng.normal(0, 1, n).astype(np.float32)
    f[rng.random(n) < zeros] = 0.0
    f[rng.random(n) < zeros / 4] = -0.0
    w = np.where(rng.random(n) < unknown, 0, rng.integers(1, 5, n)).astype(np.uint16)
    bad = rng.random(n) < nan
    f[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
    return f, w


def test_single_cell_in_all_256_sign_patterns(gpu_ready):
    rng = np.random.default_rng(80)
    total = 0
    for pattern in range(256):
        f = rng.uniform(0.1, 1.0, 8).astype(np.float32)
        f[[(pattern >> c) & 1 == 1 for c in range(8)]] *= -1
        got, want = assert_mesh_equal(f, np.ones(8, np.uint16), (0.5, -1.0, 2.0), 0.75, (2, 2, 2), what=f"pattern {pattern}")
        total += got.n_triangles
        if pattern in (0, 255):
            assert got.n_vertices == 0 and got.n_triangles == 0 and got.vertices.shape == (0, 3) and got.triangles.shape == (0, 3)
    assert total > 1500


@pytest.mark.parametrize("shape", [(3, 2, 2), (2, 2, 64), (2, 2, 65), (5, 5, 11)])
def test_small_grids_around_the_block(gpu_ready, shape):
    """Node counts of 12, 256, 260 and 275: below, at and above one block of 256 nodes.  Random fields with exact zeros,
    nodes without weight, NaN and infinite values at nodes with weight, min_weight 1 and 3."""
    rng = np.random.default_rng(81 + shape[2])
    n_tri = n_zero_area = 0
    for rep in range(6):
        f, w = random_field(rng, shape, unknown=0.05 * rep)
        for mw in (1, 3):
            got, want = assert_mesh_equal(f, w, (0.1, 0.2, -0.3), 0.37, shape, mw, f"{shape} rep {rep} min_weight {mw}")
            n_tri += got.n_triangles
            v = want.vertices[want.triangles]
            n_zero_area += int((np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1) == 0).sum()) if len(v) else 0
    assert n_tri >= 40 and (n_zero_area > 0 or shape == (3, 2, 2))      # the fields are not trivial ones


@pytest.mark.parametrize("shape", [(64, 64, 64), (65, 64, 64)])
def test_sphere_around_one_scan_chunk(gpu_ready, shape):
    """1,024 blocks are one chunk of the scan; 65 x 64 x 64 nodes are 1,040 blocks.  The mesh of the sphere is closed."""
    f = mr.sphere_field(shape, (31.3, 30.6, 32.45), 24.3)
    got, want = assert_mesh_equal(f, np.ones(len(f), np.uint16), (-1.0, -1.0, -1.0), 2.0 / 63, shape, what=str(shape))
    assert got.n_triangles > 20000 and mr.is_closed_and_oriented(got.triangles)
    assert mr.euler_characteristic(got.n_vertices, got.triangles) == 2 and mr.signed_volume(got.vertices, got.triangles) > 0
    again = device_mesh(f, np.ones(len(f), np.uint16), (-1.0, -1.0, -1.0), 2.0 / 63, shape)
    for name in ("vertices", "normals", "triangles"):
        assert getattr(got, name).tobytes() == getattr(again, name).tobytes(), name


def test_fields_without_a_surface_and_with_holes(gpu_ready):
    shape = (7, 6, 9)
    n = 7 * 6 * 9
    f = mr.sphere_field(shape, (3.2, 2.6, 4.1), 2.2)
    ones = np.ones(n, np.uint16)
    for what, ff, ww, mw in (("all outside", np.abs(f) + 0.5, ones, 1), ("all inside", -np.abs(f) - 0.5, ones, 1),
                             ("all unknown", f, np.zeros(n, np.uint16), 1), ("all NaN", np.full(n, np.nan, np.float32), ones, 1),
                             ("min_weight above every weight", f, ones * 7, 8), ("min_weight 65536", f, ones * 65535, 65536)):
        got, want = assert_mesh_equal(ff, ww, (0, 0, 0), 1.0, shape, mw, what)
        assert got.n_vertices == 0 and got.n_triangles == 0, what
    got, want = assert_mesh_equal(f, ones * 7, (0, 0, 0), 1.0, shape, 7, "min_weight at the weight")
    assert got.n_triangles > 50 and mr.is_closed_and_oriented(got.triangles)
    got, want = assert_mesh_equal(f, ones, (0, 0, 0), 1.0, shape, 0, "min_weight 0")
    assert got.n_triangles > 50
    # half of the nodes unknown: an open mesh whose edges are still used at most twice
    w = ones.copy().reshape(9, 6, 7)
    w[:, :, 4:] = 0
    got, want = assert_mesh_equal(f, w.ravel(), (0, 0, 0), 1.0, shape, 1, "half known")
    ec = mr.edge_counts(got.triangles)
    assert got.n_triangles > 20 and max(ec.values()) == 1 and any((b, a) not in ec for a, b in ec)
    # a NaN at a node with weight, next to the surface: its 8 cells fall out
    g = f.copy().reshape(9, 6, 7)
    g[4, 2, 1] = np.nan
    got, want = assert_mesh_equal(g.ravel(), ones, (0, 0, 0), 1.0, shape, 1, "NaN at a node with weight")
    assert 0 < got.n_triangles and not mr.is_closed_and_oriented(got.triangles)
    # exact zeros: zero-area triangles are kept, the mesh stays closed
    z = f.copy()
    z[np.abs(z) < 0.3] = 0.0
    got, want = assert_mesh_equal(z, ones, (0, 0, 0), 1.0, shape, 1, "exact zeros")
    assert mr.is_closed_and_oriented(got.triangles) and mr.euler_characteristic(got.n_vertices, got.triangles) == 2


# ------------------------------------------------------------------------------------------- integration
def device_integrate(proj, depth, keep, origin, voxel, shape, trunc):
    from sfm_amd.mesh import tsdf_volume_from_depth_arrays
    return tsdf_volume_from_depth_arrays(proj, depth, keep, origin, voxel, shape, trunc)


def assert_volume_equal(proj, depth, keep, origin, voxel, shape, trunc, what=""):
    vol = device_integrate(proj, depth, keep, origin, voxel, shape, trunc)
    tsdf, weight = mr.integrate(proj, depth, keep, origin, voxel, shape, trunc)
    assert vol.tsdf.dtype == np.float32 and vol.weight.dtype == np.uint16
    assert np.array_equal(vol.weight.ravel(), weight), (what, int((vol.weight.ravel() != weight).sum()))
    assert np.array_equal(vol.tsdf.ravel().view(np.uint32), tsdf.view(np.uint32)), (what, int((vol.tsdf.ravel().view(np.uint32) != tsdf.view(np.uint32)).sum()))
    return vol, tsdf, weight


def hand_made_views(rng):
    """Three views of different sizes in front of a 9 x 7 x 5 grid over [-1, 1] x [-0.75, 0.75] x [1.5, 2.5] (voxel 0.25, all
    coordinates exact): view 0 looks down +z from the origin at a constant depth of 2, so that with trunc 0.5 the nodes of
    the first layer sit exactly at sdf = trunc and those of the last at sdf = -trunc; view 1 is shifted and has a focal
    length that puts part of the grid outside the image; view 2 looks from the side."""
    sizes = ((12, 16), (9, 11), (20, 15))
    K = [np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1.0]]) for (h, w), f in zip(sizes, (6.0, 8.0, 7.0))]
    c, s = np.cos(0.5), np.sin(0.5)
    R = [np.eye(3), np.eye(3), np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])]
    t = [np.zeros(3), np.array([0.125, -0.25, 0.5]), np.array([1.0, 0.0, 0.25])]
    proj = np.array([np.c_[K[v] @ R[v], K[v] @ t[v]].reshape(12) for v in range(3)])
    depth = [np.full(sizes[0], 2.0, np.float32), rng.uniform(1.8, 3.2, sizes[1]).astype(np.float32), rng.uniform(1.5, 3.0, sizes[2]).astype(np.float32)]
    keep = [(rng.random(sz) < 0.7).astype(np.uint8) for sz in sizes]
    return proj, depth, keep


GRID = ((-1.0, -0.75, 1.5), 0.25, (9, 7, 5), 0.5)


def test_integration_of_hand_made_views(gpu_ready):
    rng = np.random.default_rng(90)
    proj, depth, keep = hand_made_views(rng)
    vol, tsdf, weight = assert_volume_equal(proj[:1], depth[:1], None, *GRID, what="view 0 alone")
    t3 = tsdf.reshape(5, 7, 9)
    assert (weight == 1).all() and (t3[0] == 1.0).all() and (t3[4] == -1.0).all() and (t3[2] == 0.0).all()      # sdf = trunc, -trunc, 0
    # behind -trunc a view is skipped: at trunc 0.25 the layer at sdf = -0.25 still counts and the one at -0.5 does not
    vol, tsdf, weight = assert_volume_equal(proj[:1], depth[:1], None, GRID[0], GRID[1], GRID[2], 0.25, what="trunc 0.25")
    assert (weight.reshape(5, 7, 9)[4] == 0).all() and (weight.reshape(5, 7, 9)[3] == 1).all()
    assert (tsdf.view(np.uint32).reshape(5, 7, 9)[4] == mr.QNAN_BITS).all()
    vol, tsdf, weight = assert_volume_equal(proj, depth, None, *GRID, what="keep NULL")
    assert weight.max() == 3 and weight.min() < 3
    vol, tsdf, kept_weight = assert_volume_equal(proj, depth, keep, *GRID, what="keep given")
    assert (kept_weight <= weight).all() and (kept_weight < weight).any() and (kept_weight == 0).any()
    # a view behind the grid, and one whose projection holds a NaN: neither counts anywhere
    behind = proj.copy()
    behind[2] = np.c_[np.diag([7.0, 7.0, 1.0]) @ np.diag([1.0, -1.0, -1.0]), [0.0, 0.0, 1.0]].reshape(12)
    vol, tsdf, w_behind = assert_volume_equal(behind, depth, None, *GRID, what="a view behind the grid")
    nan = proj.copy()
    nan[2, 5] = np.nan
    vol, tsdf, w_nan = assert_volume_equal(nan, depth, None, *GRID, what="NaN in proj")
    two = mr.integrate(proj[:2], depth[:2], None, *GRID)[1]
    assert np.array_equal(w_behind, two) and np.array_equal(w_nan, two)
    # depths that are not finite
    bad = [d.copy() for d in depth]
    bad[0][::2, ::3] = np.nan
    bad[1][1::2] = np.inf
    bad[2][:, ::2] = -np.inf
    vol, tsdf, w_bad = assert_volume_equal(proj, bad, keep, *GRID, what="depths that are not finite")
    assert (w_bad <= kept_weight).all() and (w_bad < kept_weight).any()
    # no view at all, and the same call twice
    vol, tsdf, weight = assert_volume_equal(np.zeros((0, 12)), [], None, *GRID, what="no view")
    assert (weight == 0).all()
    a, b = device_integrate(proj, bad, keep, *GRID), device_integrate(proj, bad, keep, *GRID)
    assert a.tsdf.tobytes() == b.tsdf.tobytes() and a.weight.tobytes() == b.weight.tobytes()


def test_sphere_from_14_cameras(gpu_ready):
    """The scene of tests/test_mesh_reference.py: 14 rendered depth maps of the unit sphere into 32^3 nodes, then the mesh."""
    proj, depth, origin, voxel, shape, trunc = mr.sphere_scene()
    vol, tsdf, weight = assert_volume_equal(proj, depth, None, origin, voxel, shape, trunc, "sphere")
    got = vol.mesh(1)
    want = mr.mesh(tsdf, weight, origin, voxel, shape, 1)
    mr.assert_same_mesh(got, want, "sphere")
    assert mr.is_closed_and_oriented(got.triangles) and mr.euler_characteristic(got.n_vertices, got.triangles) == 2
    radial = np.abs(np.linalg.norm(got.vertices, axis=1) - 1.0) / voxel
    assert radial.max() <= 1.0
    open_mesh = vol.mesh(2)
    mr.assert_same_mesh(open_mesh, mr.mesh(tsdf, weight, origin, voxel, shape, 2), "sphere, min_weight 2")
    assert not mr.is_closed_and_oriented(open_mesh.triangles)


def test_entry_points_reject_bad_arguments(gpu_ready):
    """SFM_ERR_ARG (-1) before any device work: the data pointers are null throughout, so a call that got as far as a launch
    would not return -1 but fault."""
    import ctypes as C
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    import view_calls as vc
    hp, f64 = vc.hp, (lambda *v: np.array(v, dtype=np.float64))
    good = dict(vc.GOOD, o=f64(0, 0, 0), s=0.5, nx=4, ny=5, nz=6, trunc=1.0, mw=1, nv=10, nt=10, ws_bytes=1 << 20)
    nan, inf = float("nan"), float("inf")
    bad_grid = [dict(nx=1), dict(ny=1025), dict(nz=0), dict(nx=-4)]
    bad_frame = [dict(o=f64(0, nan, 0)), dict(o=f64(inf, 0, 0)), dict(s=0.0), dict(s=-1.0), dict(s=nan), dict(s=inf), dict(o=None)]
    bad_views = vc.BAD_SIZES + [dict(trunc=0.0), dict(trunc=-1.0), dict(trunc=nan)]
    def integrate(a):
        return lib.sfm_tsdf_integrate(h._h, hp(a["hs"]), hp(a["ws"]), a["n_img"], a["n_ref"], hp(a["refs"]), None, None, None, hp(a["o"]),
                                      a["s"], a["nx"], a["ny"], a["nz"], a["trunc"], None, None, C.c_void_p(1), a["ws_bytes"])

    def mark(a):
        return lib.sfm_mesh_mark(h._h, None, None, a["nx"], a["ny"], a["nz"], a["mw"], None, C.c_void_p(1), a["ws_bytes"])

    def emit(a):
        return lib.sfm_mesh_emit(h._h, None, a["nx"], a["ny"], a["nz"], hp(a["o"]), a["s"], a["nv"], a["nt"], None, None, None,
                                 C.c_void_p(1), a["ws_bytes"])

    # the good calls get through every check on sizes and parameters and are stopped by their null data pointers, also -1 but
    # with another message: the bad ones must each name their own reason
    for call in (integrate, mark, emit):
        assert call(good) == -1 and lib.sfm_last_error(h._h).endswith(b": null pointer"), call.__name__
    for call, cases in ((integrate, bad_grid + bad_frame + bad_views + [dict(ws_bytes=64)]), (mark, bad_grid + [dict(mw=-1), dict(ws_bytes=64)]),
                        (emit, bad_grid + bad_frame + [dict(nv=-1), dict(nt=-1), dict(nv=1 << 31), dict(nt=1 << 31), dict(ws_bytes=64)])):
        for kw in cases:
            assert call(dict(good, **kw)) == -1, (call.__name__, kw)
            assert "o" in kw and kw["o"] is None or not lib.sfm_last_error(h._h).endswith(b": null pointer"), (call.__name__, kw)
    assert emit(dict(good, nv=0, nt=0)) == 0                      # nothing to emit: returns at once
    need = C.c_int64()
    assert lib.sfm_mesh_workspace_bytes(4, 5, 6, C.byref(need)) == 0 and 120 * 5 < need.value < (1 << 20)
    assert lib.sfm_mesh_workspace_bytes(4, 5, 1, C.byref(need)) == -1 and lib.sfm_mesh_workspace_bytes(4, 5, 6, None) == -1
    assert lib.sfm_tsdf_workspace_bytes(2, C.byref(need)) == 0 and 0 < need.value < (1 << 20)
    assert lib.sfm_tsdf_workspace_bytes(65536, C.byref(need)) == -1 and lib.sfm_tsdf_workspace_bytes(-1, C.byref(need)) == -1


def test_default_scene_from_depth_maps_to_a_ply_file(gpu_ready, tmp_path):
    """depth_maps -> filter -> tsdf -> mesh -> save_ply_mesh on the default scene (96 x 72, 3 cameras): the restatement's
    bytes on the device's own maps, the file read back, and the share of the vertices within one voxel of the nearer true
    plane against the figure the restatement gives on the CPU's maps (tests/test_mesh_reference.py)."""
    from sfm_amd import depth as dm
    from sfm_amd import Mesh, TsdfVolume, depth_maps, save_ply_mesh
    s = dr.default_scene()
    refs, sources = [0, 1, 2], [[1, 2], [0, 2], [0, 1]]
    warps = [dm.view_warps(s.K, s.poses, r, src) for r, src in zip(refs, sources)]
    planes = {r: dm.plane_depths(s.d_min, s.d_max, warps[r], s.size) for r in refs}
    maps = depth_maps(s.images, s.K, s.poses, {r: src for r, src in zip(refs, sources)}, planes, radius=2)
    with pytest.raises(ValueError, match="filter"):
        maps.tsdf()
    maps.filter(rel_tol=0.02, max_cost=12.0, min_consistent=1)
    vol = maps.tsdf(resolution=64)
    assert isinstance(vol, TsdfVolume) and max(vol.shape) == 64 and vol.trunc == 3.0 * vol.voxel
    want_proj = np.array([np.c_[s.K @ s.poses[r][0], s.K @ s.poses[r][1]].reshape(12) for r in refs])
    assert np.allclose(vol.proj, want_proj, rtol=1e-9, atol=1e-9)
    tsdf, weight = mr.integrate(vol.proj, maps.depth, maps.keep, vol.origin, vol.voxel, vol.shape, vol.trunc)
    assert np.array_equal(vol.weight.ravel(), weight) and np.array_equal(vol.tsdf.ravel().view(np.uint32), tsdf.view(np.uint32))
    mesh = vol.mesh()
    assert isinstance(mesh, Mesh)
    want = mr.mesh(tsdf, weight, vol.origin, vol.voxel, vol.shape, 1)
    mr.assert_same_mesh(mesh, want, "default scene")
    share = plane_share(mesh.vertices, s, vol.voxel)
    print(f"default scene: {mesh.n_vertices} vertices, {mesh.n_triangles} triangles, share within one voxel {share:.4f}")
    assert mesh.n_triangles > 1000 and share >= PLANE_SHARE - 0.02
    path = tmp_path / "mesh.ply"
    save_ply_mesh(mesh.vertices, mesh.triangles, path, normals=mesh.normals)
    v, n, t = read_ply_mesh(path)
    assert np.array_equal(v, mesh.vertices.astype(np.float32)) and np.array_equal(n, mesh.normals) and np.array_equal(t, mesh.triangles)
    # an explicit box, and the three box arguments only together
    box = maps.tsdf(origin=vol.origin, voxel=vol.voxel, shape=vol.shape, trunc=vol.trunc)
    assert box.tsdf.tobytes() == vol.tsdf.tobytes() and box.weight.tobytes() == vol.weight.tobytes()
    with pytest.raises(ValueError):
        maps.tsdf(origin=vol.origin)


def test_dense_from_reconstruction_with_a_mesh(gpu_ready):
    """The chain from a `Reconstruction` with mesh=True, on the scene of tests/test_depth_fuse_gpu.py: the mesh comes last,
    behind whatever the call returned before, and lies on the two planes."""
    from sfm_amd import FusedCloud, Mesh, Reconstruction, Tracks, dense_from_reconstruction
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
    kw = dict(rel_tol=0.02, max_cost=12.0, min_consistent=1)
    pts, index, maps, mesh = dense_from_reconstruction(rec, s.images, mesh=True, **kw)
    assert isinstance(mesh, Mesh) and mesh.n_triangles > 10000 and mesh.triangles.max() == mesh.n_vertices - 1
    share = plane_share(mesh.vertices, s, 0.1)                     # 256 nodes on the longest side: a voxel is far below the depth noise
    print(f"dense_from_reconstruction: {mesh.n_vertices} vertices, {mesh.n_triangles} triangles, share within 0.1 of a plane {share:.4f}")
    # 0.1: the p95 z error of a view's depth on this scene is 0.05 (README, "Fusion") and a vertex lies within the truncation,
    # 3 voxels = 0.044, of a depth it was made from; 0.9 leaves the step between the two planes and the 5 % beyond p95
    assert share >= 0.9
    assert (mesh.normals[:, 2] < 0).mean() > 0.7                   # the surface looks at the cameras
    cloud, maps2, mesh2 = dense_from_reconstruction(rec, s.images, fuse=True, mesh=True, **kw)
    assert isinstance(cloud, FusedCloud) and mesh2.vertices.tobytes() == mesh.vertices.tobytes()
    assert mesh2.triangles.tobytes() == mesh.triangles.tobytes()
    assert len(dense_from_reconstruction(rec, s.images, **kw)) == 3 and len(pts) == sum(int(k.sum()) for k in maps.keep)


def test_emit_writes_nothing_at_or_above_its_capacities(gpu_ready):
    """Capacities below the counts of the mark call: the slots below them hold what they should, the rest of the buffers
    keeps its fill."""
    import ctypes as C
    import torch
    from sfm_amd import _lib
    shape = (9, 8, 7)
    f = mr.sphere_field(shape, (4.2, 3.6, 3.1), 2.6)
    w = np.ones(len(f), np.uint16)
    origin = np.array([0.5, 0.25, -1.0])
    want = mr.mesh(f, w, origin, 0.5, shape, 1)
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    d_f, d_w = torch.from_numpy(f).to(dev), torch.from_numpy(w.view(np.int16)).to(dev)
    need = C.c_int64()
    h.check(h.lib.sfm_mesh_workspace_bytes(*shape, C.byref(need)), "sfm_mesh_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    dp = lambda t: C.c_void_p(t.data_ptr())
    h.call("sfm_mesh_mark", dp(d_f), dp(d_w), *shape, 1, dp(counts), dp(ws), need.value)
    nv, nt = (int(c) for c in counts.cpu().numpy())
    assert (nv, nt) == (len(want.vertices), len(want.triangles)) and nv > 100 and nt > 200
    for cap_v, cap_t in ((nv // 2, nt // 3), (0, nt), (nv, 0), (1, 1), (nv, nt)):
        V = torch.full((nv + 8, 3), -7.0, dtype=torch.float64, device=dev)
        N = torch.full((nv + 8, 3), -7.0, dtype=torch.float32, device=dev)
        T = torch.full((nt + 8, 3), -7, dtype=torch.int32, device=dev)
        h.call("sfm_mesh_emit", dp(d_f), *shape, C.c_void_p(origin.ctypes.data), C.c_double(0.5), cap_v, cap_t, dp(V), dp(N), dp(T),
               dp(ws), need.value)
        V, N, T = V.cpu().numpy(), N.cpu().numpy(), T.cpu().numpy()
        assert V[:cap_v].tobytes() == want.vertices[:cap_v].tobytes() and (V[cap_v:] == -7.0).all(), (cap_v, cap_t)
        assert N[:cap_v].tobytes() == want.normals[:cap_v].tobytes() and (N[cap_v:] == -7.0).all(), (cap_v, cap_t)
        assert T[:cap_t].tobytes() == want.triangles[:cap_t].tobytes() and (T[cap_t:] == -7).all(), (cap_v, cap_t)
