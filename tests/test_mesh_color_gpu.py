"""The mesh colouring on the device against tests/mesh_color_reference.py: every output byte - colors, n_views, best_view -
for vertex counts around the workgroup, view counts around the batch, the hand cases, the coloured sphere from the device's
own mesh, then the chain from the sweep on the default scene to a coloured PLY file."""
import ctypes as C

import numpy as np
import pytest

import depth_reference as dr
import mesh_color_reference as cr
import view_calls as vc
from test_mesh_color_reference import SEEN_SHARE, read_ply_coloured_mesh

pytestmark = pytest.mark.gpu

HAND_SIZES = [(7, 5), (1, 1), (16, 9), (0, 4)]                    # (h, w): three views with pixels and one of height 0


def device_colors(s):
    from sfm_amd import mesh_vertex_colors
    return mesh_vertex_colors(*s.args())


def assert_scene_equal(s, what=""):
    want = cr.colors(*s.args(), channels=s.channels)
    got = device_colors(s)
    cr.assert_same(got, want, what)
    return want


@pytest.mark.parametrize("n_vertices", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_vertex_counts_around_the_wave_and_the_workgroup(gpu_ready, n_vertices):
    """Random vertices and normals around three views of 7 x 5, 1 x 1 and 16 x 9 pixels and one of height 0; gray and three
    channels, keep given and NULL."""
    seen = 0
    for channels in (1, 3):
        for with_keep in (True, False):
            s = cr.random_scene(100 + n_vertices, n_vertices, HAND_SIZES, channels, with_keep)
            want = assert_scene_equal(s, (n_vertices, channels, with_keep))
            assert want[0].shape == ((n_vertices,) if channels == 1 else (n_vertices, 3))
            seen += int((want[1] > 0).sum())
    assert seen > 0 or n_vertices <= 1


@pytest.mark.parametrize("n_views", [1, 3, 4, 5, 8, 9])
def test_view_counts_around_the_batch(gpu_ready, n_views):
    """65 vertices; the thread takes four views at a time."""
    sizes = [[(7, 5), (9, 16), (12, 20)][v % 3] for v in range(n_views)]
    for channels in (1, 3):
        s = cr.random_scene(200 + n_views, 65, sizes, channels, with_keep=bool(n_views % 2))
        want = assert_scene_equal(s, (n_views, channels))
        assert want[1].max() >= min(n_views, 2) and want[2].max() >= min(n_views, 3) - 1


def test_no_view_and_300_views(gpu_ready):
    s = cr.random_scene(7, 65, [], 1)
    col, n_views, best = assert_scene_equal(s, "no view")
    assert (col == s.fill).all() and (n_views == 0).all() and (best == -1).all()
    s = cr.many_views(300, 65)
    col, n_views, best = assert_scene_equal(s, "300 views")
    assert (n_views == 255).all() and (best == 0).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_hand_cases(gpu_ready, channels):
    s, col, n_views, best = cr.merged_hand_cases(channels)
    cr.assert_same(device_colors(s), (col, n_views, best), "hand cases")


def raw_call(s, n_vertices, rows, fill_byte=0xAB):
    """sfm_mesh_colors on a scene with outputs of `rows` rows that hold fill_byte before the call; the three outputs whole."""
    import torch
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    ch = s.channels
    up = lambda arrays, dtype: torch.from_numpy(np.concatenate([np.asarray(a, dtype=dtype).reshape(-1) for a in arrays] + [np.zeros(1, dtype)])).to(dev)
    heights = np.array([d.shape[0] for d in s.depth], dtype=np.int32)
    widths = np.array([d.shape[1] for d in s.depth], dtype=np.int32)
    refs = np.arange(len(s.depth), dtype=np.int32)
    d = dict(proj=torch.from_numpy(s.proj).to(dev), centres=torch.from_numpy(s.centres).to(dev), depth=up(s.depth, np.float32),
             keep=up(s.keep, np.uint8), pixels=up(s.images, np.uint8), V=torch.from_numpy(s.vertices).to(dev), N=torch.from_numpy(s.normals).to(dev),
             colors=torch.full((rows, ch), fill_byte, dtype=torch.uint8, device=dev), n_views=torch.full((rows,), fill_byte, dtype=torch.uint8, device=dev),
             best=torch.full((rows,), -77, dtype=torch.int32, device=dev))
    need = C.c_int64()
    h.check(h.lib.sfm_mesh_colors_workspace_bytes(len(refs), C.byref(need)), "sfm_mesh_colors_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    dp = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: C.c_void_p(a.ctypes.data)
    h.call("sfm_mesh_colors", hp(heights), hp(widths), len(refs), len(refs), hp(refs), dp(d["proj"]), dp(d["centres"]), dp(d["depth"]), dp(d["keep"]),
           dp(d["pixels"]), ch, n_vertices, dp(d["V"]), dp(d["N"]), C.c_double(s.tol), C.c_double(s.min_cos), s.fill, dp(d["colors"]),
           dp(d["n_views"]), dp(d["best"]), dp(ws), need.value)
    return d["colors"].cpu().numpy(), d["n_views"].cpu().numpy(), d["best"].cpu().numpy()


@pytest.mark.parametrize("n_vertices", [0, 1, 200, 256, 300])
def test_nothing_is_written_at_or_above_n_vertices(gpu_ready, n_vertices):
    """Outputs with 64 rows past n_vertices keep their fill there; the scene has 300 vertices, so the rows past n_vertices
    belong to vertices the call was not asked for."""
    s = cr.random_scene(31, 300, HAND_SIZES, 3)
    want = cr.colors(*s.args(), channels=3)
    col, n_views, best = raw_call(s, n_vertices, n_vertices + 64)
    assert np.array_equal(col[:n_vertices], want[0][:n_vertices]) and (col[n_vertices:] == 0xAB).all()
    assert np.array_equal(n_views[:n_vertices], want[1][:n_vertices]) and (n_views[n_vertices:] == 0xAB).all()
    assert np.array_equal(best[:n_vertices], want[2][:n_vertices]) and (best[n_vertices:] == -77).all()


def test_coloured_sphere_from_the_device_mesh(gpu_ready):
    """The coloured sphere scene: TSDF and mesh on the device, then the colours of its 7,006 vertices from 14 views."""
    from sfm_amd import mesh_vertex_colors
    from sfm_amd.mesh import tsdf_volume_from_depth_arrays
    proj, depth, origin, voxel, shape, trunc, centres, images = cr.colour_sphere_scene()
    mesh = tsdf_volume_from_depth_arrays(proj, depth, None, origin, voxel, shape, trunc).mesh()
    got = mesh_vertex_colors(mesh.vertices, mesh.normals, proj, centres, depth, None, images, trunc)
    want = cr.colors(mesh.vertices, mesh.normals, proj, centres, depth, None, images, trunc, 0.35, 0)
    cr.assert_same(got, want, "coloured sphere")
    assert mesh.n_vertices > 5000 and got[1].min() >= 2 and cr.error_summary(got[0], mesh.vertices)[1] < 2.2


def test_entry_point_rejects_bad_arguments(gpu_ready):
    """SFM_ERR_ARG (-1) before any device work: the data pointers are null throughout, so a call that got as far as a launch
    would not return -1 but fault."""
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    hp, one = vc.hp, vc.ONE
    good = dict(vc.GOOD, ch=3, nv=10, tol=0.1, min_cos=0.35, fill=0, ws_bytes=1 << 20, workspace=one, V=one, N=one, colors=one, n_views=one,
                best=one)
    nan, inf = float("nan"), float("inf")

    def call(a):
        return lib.sfm_mesh_colors(h._h, hp(a["hs"]), hp(a["ws"]), a["n_img"], a["n_ref"], hp(a["refs"]), a["proj"], a["centres"], a["depth"],
                                   a["keep"], a["pixels"], a["ch"], a["nv"], a["V"], a["N"], a["tol"], a["min_cos"], a["fill"], a["colors"],
                                   a["n_views"], a["best"], a["workspace"], a["ws_bytes"])

    why = lambda: lib.sfm_last_error(h._h)
    bad_scalars = [dict(ch=0), dict(ch=2), dict(ch=4), dict(nv=-1), dict(nv=1 << 31), dict(tol=-0.1), dict(tol=nan), dict(tol=inf),
                   dict(min_cos=0.0), dict(min_cos=-0.2), dict(min_cos=1.01), dict(min_cos=nan), dict(min_cos=inf), dict(fill=-1), dict(fill=256)]
    for kw in vc.BAD_VIEWS + bad_scalars + [dict(ws_bytes=8), dict(workspace=None)]:
        assert call(dict(good, **kw)) == -1, kw
        assert not why().endswith(b": null pointer") or kw in vc.NULL_ARRAYS, (kw, why())
    for name in vc.VIEW_POINTERS + ("V", "N", "colors", "n_views", "best"):
        assert call(dict(good, **{name: None})) == -1 and why().endswith(b": null pointer"), name
    assert lib.sfm_mesh_colors(None, *[None] * 2, 0, 0, *[None] * 6, 3, 0, None, None, 0.1, 0.35, 0, None, None, None, None, 0) == -1
    # nothing to do: returns at once, with every pointer that has nothing behind it null
    none = dict(V=None, N=None, colors=None, n_views=None, best=None)
    assert call(dict(good, nv=0, **none)) == 0
    assert call(dict(good, nv=0, **vc.NO_VIEW, **none)) == 0 and call(dict(good, nv=0, **vc.NO_PIXEL, **none)) == 0
    need = C.c_int64()
    assert lib.sfm_mesh_colors_workspace_bytes(2, C.byref(need)) == 0 and 3 * 16 <= need.value < (1 << 20)
    assert lib.sfm_mesh_colors_workspace_bytes(65536, C.byref(need)) == -1 and lib.sfm_mesh_colors_workspace_bytes(-1, C.byref(need)) == -1
    assert lib.sfm_mesh_colors_workspace_bytes(2, None) == -1


def default_scene_maps():
    from sfm_amd import depth as dm
    from sfm_amd import depth_maps
    s = dr.default_scene()
    refs, sources = [0, 1, 2], [[1, 2], [0, 2], [0, 1]]
    warps = [dm.view_warps(s.K, s.poses, r, src) for r, src in zip(refs, sources)]
    planes = {r: dm.plane_depths(s.d_min, s.d_max, warps[r], s.size) for r in refs}
    maps = depth_maps(s.images, s.K, s.poses, {r: src for r, src in zip(refs, sources)}, planes, radius=2)
    return s, maps.filter(rel_tol=0.02, max_cost=12.0, min_consistent=1)


@pytest.mark.parametrize("channels", [1, 3])
def test_default_scene_from_depth_maps_to_a_coloured_ply_file(gpu_ready, tmp_path, channels):
    """depth_maps -> filter -> tsdf -> mesh -> colors -> save on the default scene (96 x 72, 3 cameras): the restatement's
    bytes on the device's own maps and mesh, the file read back, and the share of the vertices with a view against the figure
    the restatement gives on the CPU's maps (tests/test_mesh_color_reference.py)."""
    from sfm_amd import tsdf_volume_from_arrays
    s, maps = default_scene_maps()
    images = list(s.images) if channels == 1 else [np.stack([a, 255 - a, a // 2 + 17], axis=-1) for a in s.images]
    vol = maps.tsdf(resolution=64)
    mesh = vol.mesh()
    assert mesh.vertex_colors is None and mesh.n_views is None and mesh.best_view is None
    col = mesh.colors(images)
    assert col is mesh.vertex_colors and col.dtype == np.uint8 and col.shape == ((mesh.n_vertices,) if channels == 1 else (mesh.n_vertices, 3))
    centres = maps._s["backproj"].cpu().numpy().reshape(-1, 3, 4)[:, :, 3]
    assert np.allclose(centres, [-s.poses[r][0].T @ s.poses[r][1] for r in maps.views], atol=1e-12)
    want = cr.colors(mesh.vertices, mesh.normals, vol.proj, centres, maps.depth, maps.keep, [images[r] for r in maps.views], vol.trunc, 0.35, 0)
    cr.assert_same((col, mesh.n_views, mesh.best_view), want, "default scene")
    share = float((mesh.n_views >= 1).mean())
    print(f"default scene: {mesh.n_vertices} vertices, share with a view {share:.4f}")
    assert mesh.n_vertices > 5000 and share >= SEEN_SHARE - 0.02
    path = tmp_path / "mesh.ply"
    mesh.save(path)
    v, n, c, t = read_ply_coloured_mesh(path)
    assert np.array_equal(v, mesh.vertices.astype(np.float32)) and np.array_equal(n, mesh.normals) and np.array_equal(t, mesh.triangles)
    assert np.array_equal(c, np.repeat(col[:, None], 3, axis=1) if channels == 1 else col[:, ::-1])
    # the maps handed in, other scalars, and a mesh whose volume has no maps
    again = mesh.colors(images, maps, tol=vol.trunc, min_cos=0.35, fill=0)
    assert again.tobytes() == col.tobytes()
    other = mesh.colors(images, tol=0.5 * vol.trunc, min_cos=0.8, fill=200)
    want = cr.colors(mesh.vertices, mesh.normals, vol.proj, centres, maps.depth, maps.keep, [images[r] for r in maps.views], 0.5 * vol.trunc, 0.8, 200)
    cr.assert_same((other, mesh.n_views, mesh.best_view), want, "other scalars")
    assert (mesh.n_views == 0).any() and (other[mesh.n_views == 0] == 200).all()
    bare = tsdf_volume_from_arrays(vol.tsdf, vol.weight, vol.origin, vol.voxel).mesh()
    with pytest.raises(ValueError, match="DepthMaps.tsdf"):
        bare.colors(images)
    assert bare.colors(images, maps).tobytes() == col.tobytes()     # tol: 3 voxels of the volume, the default truncation


def test_dense_from_reconstruction_with_a_coloured_mesh(gpu_ready):
    """The chain from a `Reconstruction` with mesh=True and colors: the tuple keeps its shape, the mesh carries the colours
    that `mesh.colors(images)` gives; without colors the mesh has none."""
    from sfm_amd import Mesh, Reconstruction, Tracks, dense_from_reconstruction
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
    images = list(s.images)
    out = dense_from_reconstruction(rec, images, mesh=True, colors=images, **kw)
    assert len(out) == 5 and isinstance(out[4], Mesh)
    pts, index, point_colors, maps, mesh = out
    col = mesh.vertex_colors
    print(f"dense_from_reconstruction: {mesh.n_vertices} vertices, share with a view {(mesh.n_views >= 1).mean():.4f}")
    assert col is not None and col.shape == (mesh.n_vertices,) and (mesh.n_views >= 1).any()
    kept = col.copy()
    assert mesh.colors(images).tobytes() == kept.tobytes()
    plain = dense_from_reconstruction(rec, images, mesh=True, **kw)
    assert len(plain) == 4 and plain[3].vertex_colors is None and plain[3].vertices.tobytes() == mesh.vertices.tobytes()
    assert plain[0].tobytes() == pts.tobytes() and plain[1].tobytes() == index.tobytes()
