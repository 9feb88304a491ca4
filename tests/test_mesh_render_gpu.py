"""The mesh render on the device against tests/mesh_render_reference.py: every output byte - depth and barycentrics as float32
bits, triangle, colour - for the hand cases in one scene, triangle counts around the wavefront and the workgroup, one to five
cameras of mixed sizes, every source of colour, a close-up whose boxes take both raster passes, batches against single
calls, over-allocated outputs, the sphere from the device's own mesh and atlas, then the chain from the sweep on the default
scene to PNG files."""
import ctypes as C

import numpy as np
import pytest

import mesh_color_reference as cr
import mesh_render_reference as rr
from test_mesh_texture_gpu import default_scene_maps
from test_mesh_texture_reference import read_png

pytestmark = pytest.mark.gpu

# measured with the restatements on the default scene from the CPU's maps (`mesh_render_reference.default_scene_render(32)`:
# the box at resolution 32, 2,662 vertices, 4,886 triangles): the share of drawn pixels of the three views of 96 x 72; the
# device's own maps differ from those in a few pixels, so the test allows five percentage points either way
COVERAGE = (0.6073, 0.7264, 0.6043)
SIZES = [(5, 3), (9, 16), (4, 0), (40, 30)]                        # (width, height): one camera without a pixel
SOURCES = [(None, 1, False), ("vertex", 1, False), ("vertex", 3, False), ("atlas", 1, True), ("atlas", 3, False)]


def device_render(s):
    from sfm_amd import render_mesh
    return render_mesh(*s.args(), **s.kwargs())


def assert_scene_equal(s, what=""):
    want = rr.reference(s)
    got = device_render(s)
    rr.assert_same(got, want, what)
    assert got.sizes == s.sizes and got.n_large == want.n_large and got.coverage == want.coverage
    return want


@pytest.mark.parametrize("source,channels", [(None, 1), ("vertex", 1), ("vertex", 3), ("atlas", 1), ("atlas", 3)])
def test_hand_cases_in_one_scene(gpu_ready, source, channels):
    """The hand cases of tests/test_mesh_render_reference.py as one mesh, drawn through each case's camera at its size (a
    1 x 1 and a 0 x 4 image among them): overlap, a shared edge, a vertex on a pixel centre, a triangle between pixel centres,
    zero area, a corner behind the camera, a NaN vertex, bad indices, both orientations, a triangle larger than the image."""
    want = assert_scene_equal(rr.merged_hand_scene(source, channels), ("hand", source, channels))
    # the triangles larger than the image lie behind every other case and fill what those leave open
    assert sum(int((t >= 0).sum()) for t in want.triangle) > 100 and len(np.unique(np.concatenate([t.ravel() for t in want.triangle]))) >= 3


@pytest.mark.parametrize("n_triangles", [0, 1, 2, 63, 64, 65, 257])
def test_triangle_counts(gpu_ready, n_triangles):
    """Random meshes over 50 vertices with NaN coordinates and bad indices: one to five cameras in a call, sizes 5 x 3, 9 x 16,
    4 x 0 and 40 x 30, gray and three channels, vertex colours, atlas (some uv outside it, one NaN) and no colour."""
    drawn = large = 0
    for case, (source, channels, wild) in enumerate(SOURCES):
        sizes = (SIZES + SIZES[:1])[:case + 1] if case else SIZES[3:]           # 1 (the largest), 2, 3, 4, 5 cameras
        s = rr.random_scene(1000 + 10 * n_triangles + case, 50, n_triangles, sizes, source, channels, wild)
        want = assert_scene_equal(s, (n_triangles, case))
        drawn += sum(int((t >= 0).sum()) for t in want.triangle)
        large += want.n_large
    assert (drawn > 100 and large > 0) or n_triangles < 63


def test_close_up_takes_both_raster_passes(gpu_ready):
    """One camera close to a grid of 242 small triangles and four large ones: the CPU counts four boxes of more than 64 pixels
    and 242 of fewer, both kinds show in the image, and the device's list holds four entries."""
    s = rr.close_up_scene()
    want = rr.reference(s)
    nt = len(s.triangles)
    assert want.n_large == 4 and nt == 246
    seen = np.unique(want.triangle[0])
    assert (seen >= nt - 4).sum() >= 2 and ((seen >= 0) & (seen < nt - 4)).sum() > 100
    got = device_render(s)
    rr.assert_same(got, want, "close-up")
    assert got.n_large == 4


def test_a_batch_equals_its_cameras_one_by_one(gpu_ready):
    s = rr.random_scene(31, 50, 80, [(40, 30), (9, 16)], "atlas", 3)
    both = device_render(s)
    rr.assert_same(both, rr.reference(s), "batch")
    for c in range(2):
        one = device_render(rr.Scene(s.vertices, s.triangles, s.proj[c:c + 1], s.sizes[c:c + 1], **s.kwargs()))
        for name in ("depth", "triangle", "bary", "color"):
            assert getattr(one, name)[0].tobytes() == getattr(both, name)[c].tobytes(), (c, name)


def raw_call(s, spare, guard=0xAB):
    """sfm_mesh_render with outputs that have `spare` elements more than the call needs and hold `guard` bytes before it."""
    import torch
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    heights = np.array([hh for w, hh in s.sizes], dtype=np.int32)
    widths = np.array([w for w, hh in s.sizes], dtype=np.int32)
    n = int(sum(w * hh for w, hh in s.sizes))
    ch = 3 if s.vertex_colors.ndim == 2 else 1
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = dict(proj=up(s.proj), V=up(s.vertices), T=up(s.triangles), col=up(s.vertex_colors))
    out = {name: torch.full((n * k + spare,), guard, dtype=torch.uint8, device=dev).view(dt) if dt != torch.uint8
           else torch.full((n * k + spare,), guard, dtype=torch.uint8, device=dev)
           for name, k, dt in (("depth", 4, torch.float32), ("triangle", 4, torch.int32), ("bary", 12, torch.float32), ("color", ch, torch.uint8))}
    hp = lambda a: C.c_void_p(a.ctypes.data)
    dp = lambda t: C.c_void_p(t.data_ptr())
    need = C.c_int64()
    h.check(h.lib.sfm_mesh_render_workspace_bytes(len(heights), hp(heights), hp(widths), len(s.vertices), len(s.triangles), C.byref(need)), "workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    h.call("sfm_mesh_render", len(heights), hp(heights), hp(widths), dp(d["proj"]), len(s.vertices), dp(d["V"]), len(s.triangles), dp(d["T"]), 1, ch,
           dp(d["col"]), None, None, 0, 0, s.fill, dp(out["depth"]), dp(out["triangle"]), dp(out["bary"]), dp(out["color"]), dp(ws), need.value)
    return {k: v.cpu().numpy() for k, v in out.items()}, n, ch


@pytest.mark.parametrize("sizes", [[(4, 0)], [(5, 3)], [(9, 16), (4, 0), (40, 30)]])
def test_nothing_is_written_past_the_outputs(gpu_ready, sizes):
    """Outputs with 4,096 bytes past what the cameras need keep what they held there."""
    s = rr.random_scene(52, 50, 70, sizes, "vertex", 3)
    got, n, ch = raw_call(s, 4096)
    want = rr.reference(s)
    flat = lambda arrays: np.concatenate([np.asarray(a).reshape(-1) for a in arrays])
    for name, k in (("depth", 1), ("triangle", 1), ("bary", 3), ("color", ch)):
        w = flat(getattr(want, name))
        g = got[name]
        assert g[:n * k].tobytes() == w.tobytes(), name
        tail = g[n * k:].view(np.uint8)
        assert len(tail) == 4096 and (tail == 0xAB).all(), name


def test_sphere_from_the_device_mesh_and_atlas(gpu_ready):
    """The coloured sphere scene: TSDF, mesh, vertex colours and atlas on the device, then its 14 cameras at 64 x 64."""
    from sfm_amd import mesh_texture, mesh_vertex_colors, render_mesh
    from sfm_amd.mesh import tsdf_volume_from_depth_arrays
    proj, depth, origin, voxel, shape, trunc, centres, images = cr.colour_sphere_scene()
    mesh = tsdf_volume_from_depth_arrays(proj, depth, None, origin, voxel, shape, trunc).mesh()
    t = mesh_texture(mesh.vertices, mesh.normals, mesh.triangles, proj, centres, depth, None, images, trunc, texels=4)
    vcol = mesh_vertex_colors(mesh.vertices, mesh.normals, proj, centres, depth, None, images, trunc)[0]
    sizes = [(64, 64)] * len(proj)
    for kw in (dict(uv=t.uv, atlas=t.image), dict(vertex_colors=vcol)):
        got = render_mesh(mesh.vertices, mesh.triangles, proj, sizes, **kw)
        want = rr.render(mesh.vertices, mesh.triangles, proj, sizes, **kw)
        rr.assert_same(got, want, ("sphere", list(kw)))
    assert mesh.n_triangles > 10000 and min(want.coverage) > 0.3 and got.n_large == 0
    # the render of an input view is close to that view where both have the sphere
    err = np.abs(want.color[0].astype(np.float64) - images[0])[(want.triangle[0] >= 0) & np.isfinite(depth[0])]
    assert np.median(err) < 3.0


def test_default_scene_from_depth_maps_to_png_files(gpu_ready, tmp_path):
    """depth_maps -> filter -> tsdf -> mesh -> texture -> render_views -> save_png on the default scene (96 x 72, 3 cameras),
    gray and BGR: the restatement's bytes on the device's own mesh and atlas, the PNG read back, the coverage beside the
    restatement's on the CPU's maps; then the vertex colours, no colour, and a novel camera given as K with (R, t)."""
    from sfm_amd import MeshRender
    s, maps = default_scene_maps()
    vol = maps.tsdf(resolution=32)
    mesh = vol.mesh()
    assert mesh.n_triangles > 1000
    plain = mesh.render_views()                                    # neither atlas nor vertex colours yet: geometry only
    assert plain.color is None and plain.sizes == [(96, 72)] * 3
    sizes = [(96, 72)] * 3
    for channels in (1, 3):
        images = list(s.images) if channels == 1 else [np.stack([a, 255 - a, a // 2 + 17], axis=-1) for a in s.images]
        t = mesh.texture(images, texels=4)
        r = mesh.render_views()
        assert isinstance(r, MeshRender) and r.sizes == sizes and r.color[0].shape == ((72, 96) if channels == 1 else (72, 96, 3))
        want = rr.render(mesh.vertices, mesh.triangles, vol.proj, sizes, uv=t.uv, atlas=t.image)
        rr.assert_same(r, want, ("default scene", channels))
        print(f"default scene: {mesh.n_triangles} triangles, coverage {[round(c, 4) for c in r.coverage]}")
        for c in range(3):
            assert abs(r.coverage[c] - COVERAGE[c]) <= 0.05
            r.save_png(tmp_path / f"view{c}.png", camera=c)
            png = read_png(tmp_path / f"view{c}.png")
            assert np.array_equal(png, r.color[c][:, :, ::-1] if channels == 3 else r.color[c])
        for name in ("depth", "triangle", "bary"):                 # the geometry does not depend on the colour
            assert all(a.tobytes() == b.tobytes() for a, b in zip(getattr(r, name), getattr(plain, name)))
    # the vertex colours, asked for by name and with another fill
    vcol = mesh.colors(images)
    r = mesh.render_views(colors="vertex", fill=200)
    rr.assert_same(r, rr.render(mesh.vertices, mesh.triangles, vol.proj, sizes, vertex_colors=vcol, fill=200), "vertex colours")
    assert (r.color[0][r.triangle[0] < 0] == 200).all() and mesh.render_views(colors=None).color is None
    # a camera that is none of the views, as K with (R, t), at another size
    K = s.K.copy()
    K[:2] *= 0.5
    R, tt = s.poses[1]
    novel = (K, (R, tt + np.array([0.05, -0.02, 0.1])))
    r = mesh.render(novel, (48, 36))
    P = (K @ np.c_[R, tt + np.array([0.05, -0.02, 0.1])]).reshape(1, 12)
    rr.assert_same(r, rr.render(mesh.vertices, mesh.triangles, P, [(48, 36)], uv=t.uv, atlas=t.image), "novel camera")
    assert r.coverage[0] > 0.3


def test_entry_point_rejects_bad_arguments(gpu_ready):
    """SFM_ERR_ARG (-1) before any device work: the data pointers are null or stand-ins throughout, so a call that got as far
    as a launch would not return -1 but fault."""
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    one = C.c_void_p(1)                                            # stands for a pointer that is there; never followed
    good = dict(n_cam=2, hs=i32(3, 4), ws=i32(4, 7), proj=one, nv=10, V=one, nt=6, T=one, mode=2, ch=3, col=None, uv=one, atlas=one, aw=8, ah=8, fill=0,
                depth=one, tri=one, bary=one, color=one, workspace=one, ws_bytes=1 << 20)

    def call(a):
        return lib.sfm_mesh_render(h._h, a["n_cam"], hp(a["hs"]), hp(a["ws"]), a["proj"], a["nv"], a["V"], a["nt"], a["T"], a["mode"], a["ch"], a["col"],
                                   a["uv"], a["atlas"], a["aw"], a["ah"], a["fill"], a["depth"], a["tri"], a["bary"], a["color"], a["workspace"],
                                   a["ws_bytes"])

    why = lambda: lib.sfm_last_error(h._h)
    bad = [dict(n_cam=-1), dict(n_cam=65536), dict(hs=i32(3, -1)), dict(ws=i32(4, 32769)), dict(nv=-1), dict(nv=1 << 31), dict(nt=-1), dict(nt=1 << 31),
           dict(mode=3), dict(mode=-1), dict(ch=2), dict(ch=0), dict(fill=-1), dict(fill=256), dict(aw=0), dict(ah=0), dict(aw=32769), dict(ws_bytes=64),
           dict(workspace=None)]
    for kw in bad:
        assert call(dict(good, **kw)) == -1, kw
        assert not why().endswith(b": null pointer"), (kw, why())
    for name in ("hs", "ws", "proj", "V", "T", "uv", "atlas", "depth", "tri", "bary", "color"):
        assert call(dict(good, **{name: None})) == -1 and why().endswith(b": null pointer"), name
    assert call(dict(good, mode=1, uv=None, atlas=None)) == -1 and why().endswith(b": null pointer")          # vertex colours asked for, none given
    need = C.c_int64()
    assert lib.sfm_mesh_render_workspace_bytes(2, hp(good["hs"]), hp(good["ws"]), 10, 6, C.byref(need)) == 0 and need.value < (1 << 20)
    assert call(dict(good, ws_bytes=need.value - 1)) == -1 and why().endswith(b"too small")
