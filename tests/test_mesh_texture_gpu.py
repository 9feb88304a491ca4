"""The mesh texture on the device against tests/mesh_texture_reference.py: every output byte - texture, views and uv as
float32 bits - for triangle counts around the cell, the tile and the workgroup, patch sizes 1 to 64, atlas widths on both
sides of the tile, view counts around a batch of four, bad indices, over-allocated outputs, the textured sphere from the device's
own mesh, then the chain from the sweep on the default scene to OBJ, MTL and PNG files."""
import ctypes as C

import numpy as np
import pytest

import depth_reference as dr
import mesh_color_reference as cr
import mesh_texture_reference as tr
import view_calls as vc
from test_mesh_color_gpu import default_scene_maps
from test_mesh_texture_reference import assert_obj_files

pytestmark = pytest.mark.gpu

# measured with the restatements on the default scene from the CPU's maps (the box at resolution 32, 4,886 triangles, texels 4,
# tol = 3 voxels, min_cos 0.35): the share of the triangles' texels that at least one view sees; the device's own maps
# differ from those in a few pixels, so the test asks for five percentage points less
SEEN_SHARE = 0.927
SIZES = [(7, 5), (3, 5), (16, 9), (0, 4), (30, 40)]               # (h, w): 5 x 3 to 40 x 30 pixels and one view of height 0


def device_texture(s, texels, cells_per_row=None):
    from sfm_amd import mesh_texture
    t = mesh_texture(*s.args(), **s.kwargs(texels, cells_per_row))
    return t, (t.image, t.views, t.uv)


def assert_scene_equal(s, texels, cells_per_row=None, what=""):
    want = tr.reference(s, texels, cells_per_row)
    t, got = device_texture(s, texels, cells_per_row)
    tr.assert_same(got, want, what)
    nt = len(s.triangles)
    cpr = tr.default_cells_per_row(nt) if cells_per_row is None else cells_per_row
    assert t.size == tr.atlas_size(nt, texels, cpr) and t.texels == texels and t.cells_per_row == cpr
    return want


@pytest.mark.parametrize("n_triangles", [0, 1, 2, 3, 63, 64, 65, 257])
def test_triangle_counts(gpu_ready, n_triangles):
    """Random triangles over 50 random vertices (NaN coordinates, zero normals) at texels 3, so a patch is 6 texels: gray and
    three channels, keep given and NULL; the default atlas is 6 to 72 texels wide: below, at and above a tile."""
    seen = 0
    for channels in (1, 3):
        for with_keep in (True, False):
            s = tr.random_scene(300 + n_triangles, 50, n_triangles, SIZES, channels, with_keep)
            want = assert_scene_equal(s, 3, None, (n_triangles, channels, with_keep))
            seen += int((want[1] > 0).sum())
    assert seen > 0 or n_triangles == 0


@pytest.mark.parametrize("texels", [1, 2, 8, 64])
def test_patch_sizes(gpu_ready, texels):
    """5 triangles: an odd count, so the last cell has an empty half."""
    for channels in (1, 3):
        s = tr.random_scene(400 + texels, 50, 5, SIZES, channels)
        want = assert_scene_equal(s, texels, None, (texels, channels))
        assert (want[1] >= 2).sum() > texels


@pytest.mark.parametrize("cells_per_row,n_triangles,texels", [(1, 9, 3), (2, 9, 3), (7, 40, 3), (7, 30, 6), (8, 20, 5), (11, 45, 3), (13, 60, 2),
                                                              (3, 7, 64)])
def test_cells_per_row_and_widths_off_the_tile(gpu_ready, cells_per_row, n_triangles, texels):
    """Atlases of W x H = 6 x 30, 12 x 18, 42 x 18, 63 x 27, 64 x 16, 66 x 18, 65 x 15 and 201 x 134 texels under tiles of
    64 x 4: narrower than a tile, one texel short of it, exactly one, one and two texels over it, several tiles with a rest;
    heights that are and are not a multiple of 4."""
    s = tr.random_scene(500 + cells_per_row, 50, n_triangles, SIZES, 3)
    want = assert_scene_equal(s, texels, cells_per_row, (cells_per_row, n_triangles, texels))
    assert want[1].shape[::-1] == tr.atlas_size(n_triangles, texels, cells_per_row) and (want[1] > 0).any()


@pytest.mark.parametrize("n_views", [0, 1, 3, 4, 5, 9])
def test_view_counts_around_a_batch(gpu_ready, n_views):
    """33 triangles; without a view there is no image to take three channels from, so that case is gray."""
    sizes = [[(7, 5), (9, 16), (30, 40)][v % 3] for v in range(n_views)]
    for channels in (1, 3) if n_views else (1,):
        s = tr.random_scene(600 + n_views, 50, 33, sizes, channels, with_keep=bool(n_views % 2))
        want = assert_scene_equal(s, 4, 5, (n_views, channels))
        assert want[1].max() >= min(n_views, 2)
        if n_views == 0:
            assert (want[0] == s.fill).all() and (want[1] == 0).all()


def test_bad_indices(gpu_ready):
    """A triangle with the index -1 and one with n_vertices: fill and 0, their uv as ever, their neighbours untouched; and a
    mesh without a vertex, where every index is bad."""
    nv = 50
    s = tr.random_scene(700, nv, 11, SIZES, 3, bad=[(2, 0, -1), (7, 2, nv)])
    want = assert_scene_equal(s, 5, 3, "bad indices")
    tri = tr.inverse_map(11, 5, 3)[0]
    for t in (2, 7):
        assert (want[0][tri == t] == s.fill).all() and (want[1][tri == t] == 0).all()
    assert (want[1][tri == 3] > 0).any() and (want[1][tri == 6] > 0).any()
    clean = tr.random_scene(700, nv, 11, SIZES, 3)
    assert np.array_equal(tr.reference(clean, 5, 3)[2], want[2])
    none = tr.random_scene(701, 0, 4, SIZES, 1)
    want = assert_scene_equal(none, 3, 2, "no vertex")
    assert (want[0] == none.fill).all()


def raw_call(s, n_triangles, texels, cells_per_row, spare, fill_byte=0xAB):
    """sfm_mesh_texture on the first n_triangles of a scene with outputs that have `spare` elements more than the call needs
    and hold fill_byte before it; the three outputs whole, and (W, H)."""
    import torch
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    c, ch = s.s, s.channels
    up = lambda arrays, dtype: torch.from_numpy(np.concatenate([np.asarray(a, dtype=dtype).reshape(-1) for a in arrays] + [np.zeros(1, dtype)])).to(dev)
    heights = np.array([d.shape[0] for d in c.depth], dtype=np.int32)
    widths = np.array([d.shape[1] for d in c.depth], dtype=np.int32)
    refs = np.arange(len(c.depth), dtype=np.int32)
    W, H = tr.atlas_size(n_triangles, texels, cells_per_row)
    d = dict(proj=torch.from_numpy(c.proj).to(dev), centres=torch.from_numpy(c.centres).to(dev), depth=up(c.depth, np.float32),
             keep=up(c.keep, np.uint8), pixels=up(c.images, np.uint8), V=torch.from_numpy(c.vertices).to(dev), N=torch.from_numpy(c.normals).to(dev),
             T=torch.from_numpy(np.ascontiguousarray(s.triangles)).to(dev),
             image=torch.full((H * W * ch + spare,), fill_byte, dtype=torch.uint8, device=dev),
             views=torch.full((H * W + spare,), fill_byte, dtype=torch.uint8, device=dev),
             uv=torch.full((n_triangles * 6 + spare,), -77.0, dtype=torch.float32, device=dev))
    need = C.c_int64()
    h.check(h.lib.sfm_mesh_texture_workspace_bytes(len(refs), C.byref(need)), "sfm_mesh_texture_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    dp = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: C.c_void_p(a.ctypes.data)
    h.call("sfm_mesh_texture", hp(heights), hp(widths), len(refs), len(refs), hp(refs), dp(d["proj"]), dp(d["centres"]), dp(d["depth"]), dp(d["keep"]),
           dp(d["pixels"]), ch, len(c.vertices), dp(d["V"]), dp(d["N"]), n_triangles, dp(d["T"]), texels, cells_per_row, C.c_double(s.tol),
           C.c_double(s.min_cos), s.fill, dp(d["image"]), dp(d["views"]), dp(d["uv"]), dp(ws), need.value)
    return d["image"].cpu().numpy(), d["views"].cpu().numpy(), d["uv"].cpu().numpy(), (W, H)


@pytest.mark.parametrize("n_triangles,cells_per_row", [(0, 3), (1, 1), (10, 3), (37, 5), (40, 11)])
def test_nothing_is_written_past_the_outputs(gpu_ready, n_triangles, cells_per_row):
    """Outputs with 4,096 elements past H * W * channels, H * W and n_triangles * 6 keep what they held there; the scene has
    40 triangles, so what lies past the atlas of the first n_triangles belongs to triangles the call was not asked for."""
    s = tr.random_scene(800, 50, 40, SIZES, 3)
    image, views, uv, (W, H) = raw_call(s, n_triangles, 3, cells_per_row, 4096)
    part = tr.Scene(s.s, s.triangles[:n_triangles])
    want = tr.reference(part, 3, cells_per_row)
    n = H * W
    assert np.array_equal(image[:n * 3].reshape(H, W, 3), want[0]) and (image[n * 3:] == 0xAB).all() and len(image) == n * 3 + 4096
    assert np.array_equal(views[:n].reshape(H, W), want[1]) and (views[n:] == 0xAB).all()
    assert np.array_equal(uv[:n_triangles * 6].view(np.uint32), want[2].reshape(-1).view(np.uint32)) and (uv[n_triangles * 6:] == -77.0).all()


def test_textured_sphere_from_the_device_mesh(gpu_ready):
    """The coloured sphere scene (14 views of 64 x 64): TSDF and mesh on the device, then the atlas of its 14,008 triangles
    at texels 4."""
    from sfm_amd import mesh_texture
    from sfm_amd.mesh import tsdf_volume_from_depth_arrays
    proj, depth, origin, voxel, shape, trunc, centres, images = cr.colour_sphere_scene()
    mesh = tsdf_volume_from_depth_arrays(proj, depth, None, origin, voxel, shape, trunc).mesh()
    t = mesh_texture(mesh.vertices, mesh.normals, mesh.triangles, proj, centres, depth, None, images, trunc, texels=4)
    want = tr.texture(mesh.vertices, mesh.normals, mesh.triangles, proj, centres, depth, None, images, trunc, 4, 0.35, 0)
    tr.assert_same((t.image, t.views, t.uv), want, "textured sphere")
    tri = tr.inverse_map(mesh.n_triangles, 4, t.cells_per_row)[0]
    assert mesh.n_triangles > 10000 and t.views[tri >= 0].min() >= 1 and (t.views[tri < 0] == 0).all()


def test_default_scene_from_depth_maps_to_obj_files(gpu_ready, tmp_path):
    """depth_maps -> filter -> tsdf -> mesh -> texture -> save_obj on the default scene (96 x 72, 3 cameras), gray and BGR:
    the restatement's bytes on the device's own maps and mesh, and the three files read back."""
    from sfm_amd import MeshTexture
    s, maps = default_scene_maps()
    vol = maps.tsdf(resolution=32)
    mesh = vol.mesh()
    assert mesh.atlas is None and mesh.n_triangles > 1000
    centres = maps._s["backproj"].cpu().numpy().reshape(-1, 3, 4)[:, :, 3]
    for channels in (1, 3):
        images = list(s.images) if channels == 1 else [np.stack([a, 255 - a, a // 2 + 17], axis=-1) for a in s.images]
        t = mesh.texture(images, texels=4)
        assert t is mesh.atlas and isinstance(t, MeshTexture) and t.image.shape == (t.size[::-1] if channels == 1 else t.size[::-1] + (3,))
        want = tr.texture(mesh.vertices, mesh.normals, mesh.triangles, vol.proj, centres, maps.depth, maps.keep, [images[r] for r in maps.views],
                          vol.trunc, 4, 0.35, 0)
        tr.assert_same((t.image, t.views, t.uv), want, ("default scene", channels))
        tri = tr.inverse_map(mesh.n_triangles, 4, t.cells_per_row)[0]
        share = float((t.views[tri >= 0] > 0).mean())
        print(f"default scene: {mesh.n_triangles} triangles, atlas {t.size}, share of the triangles' texels with a view {share:.4f}")
        assert share >= SEEN_SHARE - 0.05
        path = tmp_path / f"mesh{channels}.obj"
        mesh.save_obj(path)
        assert_obj_files(path, mesh.vertices, mesh.normals, mesh.triangles, t.uv, t.image)
    # other scalars and another layout; the vertex colours are untouched by it
    other = mesh.texture(images, texels=2, tol=0.5 * vol.trunc, min_cos=0.8, fill=200, cells_per_row=100)
    want = tr.texture(mesh.vertices, mesh.normals, mesh.triangles, vol.proj, centres, maps.depth, maps.keep, [images[r] for r in maps.views],
                      0.5 * vol.trunc, 2, 0.8, 200, 100)
    tr.assert_same((other.image, other.views, other.uv), want, "other scalars")
    assert other.size[0] == 500 and (other.views == 0).any() and (other.image[other.views == 0] == 200).all() and mesh.vertex_colors is None


def test_dense_from_reconstruction_with_a_textured_mesh(gpu_ready):
    """The chain from a `Reconstruction` with mesh=True, colors and texture=4: the tuple keeps its shape and the mesh carries
    the atlas that `mesh.texture(images, texels=4)` gives; without texture the mesh has none."""
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
    out = dense_from_reconstruction(rec, images, mesh=True, colors=images, texture=4, **kw)
    assert len(out) == 5 and isinstance(out[4], Mesh)
    mesh = out[4]
    atlas = mesh.atlas
    assert atlas is not None and atlas.texels == 4 and atlas.uv.shape == (mesh.n_triangles, 3, 2) and (atlas.views > 0).any()
    assert mesh.vertex_colors is not None
    kept = (atlas.image.copy(), atlas.views.copy(), atlas.uv.copy())
    again = mesh.texture(images, texels=4)
    tr.assert_same((again.image, again.views, again.uv), kept, "texture() again")
    plain = dense_from_reconstruction(rec, images, mesh=True, colors=images, **kw)
    assert len(plain) == 5 and plain[4].atlas is None and plain[4].vertex_colors.tobytes() == mesh.vertex_colors.tobytes()


def test_entry_point_rejects_bad_arguments(gpu_ready):
    """SFM_ERR_ARG (-1) before any device work: the data pointers are null or stand-ins throughout, so a call that got as far
    as a launch would not return -1 but fault."""
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    hp, one = vc.hp, vc.ONE
    good = dict(vc.GOOD, ch=3, nv=10, nt=6, s=8, cpr=2, tol=0.1, min_cos=0.35, fill=0, ws_bytes=1 << 20, workspace=one, V=one, N=one, T=one,
                image=one, views=one, uv=one)
    nan, inf = float("nan"), float("inf")

    def call(a):
        return lib.sfm_mesh_texture(h._h, hp(a["hs"]), hp(a["ws"]), a["n_img"], a["n_ref"], hp(a["refs"]), a["proj"], a["centres"], a["depth"],
                                    a["keep"], a["pixels"], a["ch"], a["nv"], a["V"], a["N"], a["nt"], a["T"], a["s"], a["cpr"], a["tol"],
                                    a["min_cos"], a["fill"], a["image"], a["views"], a["uv"], a["workspace"], a["ws_bytes"])

    why = lambda: lib.sfm_last_error(h._h)
    bad_scalars = [dict(ch=0), dict(ch=2), dict(ch=4), dict(nv=-1), dict(nv=1 << 31), dict(tol=-0.1), dict(tol=nan), dict(tol=inf),
                   dict(min_cos=0.0), dict(min_cos=1.01), dict(min_cos=nan), dict(fill=-1), dict(fill=256)]
    bad_layout = [dict(s=0), dict(s=65), dict(s=-1), dict(cpr=0), dict(cpr=-1), dict(s=64, cpr=490), dict(s=64, cpr=489, nt=2 * 489 * 489 + 1),
                  dict(nt=-1), dict(nt=1 << 31, cpr=32768, s=1)]
    for kw in vc.BAD_VIEWS + bad_scalars + bad_layout + [dict(ws_bytes=8), dict(workspace=None)]:
        assert call(dict(good, **kw)) == -1, kw
        assert not why().endswith(b": null pointer") or kw in vc.NULL_ARRAYS, (kw, why())
    for name in vc.VIEW_POINTERS + ("V", "N", "T", "image", "views", "uv"):
        assert call(dict(good, **{name: None})) == -1 and why().endswith(b": null pointer"), name
    assert lib.sfm_mesh_texture(None, *[None] * 2, 0, 0, *[None] * 6, 3, 0, None, None, 0, None, 8, 1, 0.1, 0.35, 0, None, None, None, None, 0) == -1
    # nothing to do: returns at once, with every pointer that has nothing behind it null
    none = dict(T=None, image=None, views=None, uv=None)
    assert call(dict(good, nt=0, **none)) == 0
    assert call(dict(good, nt=0, nv=0, V=None, N=None, **none)) == 0
    assert call(dict(good, nt=0, **vc.NO_VIEW, **none)) == 0 and call(dict(good, nt=0, **vc.NO_PIXEL, **none)) == 0
    W, H = C.c_int32(), C.c_int32()
    assert lib.sfm_mesh_texture_size(6, 8, 2, C.byref(W), C.byref(H)) == 0 and (W.value, H.value) == (22, 22)
    assert lib.sfm_mesh_texture_size(6, 65, 2, C.byref(W), C.byref(H)) == -1
    need = C.c_int64()
    assert lib.sfm_mesh_texture_workspace_bytes(2, C.byref(need)) == 0 and 3 * 16 <= need.value < (1 << 20)
    assert lib.sfm_mesh_texture_workspace_bytes(65536, C.byref(need)) == -1 and lib.sfm_mesh_texture_workspace_bytes(2, None) == -1
