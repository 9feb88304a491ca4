"""The render score on the device against tests/render_score_reference.py: every output byte - the table, abs_error, ssim_map as
float32 bits - over sizes around the window and the tile (read from the library), both channel counts, windows 3, 7 and 11,
the coverage patterns with and without a mask, with and without the views' depth, a batch against its views one by one,
guard bytes behind every output, NULL map pointers, then the chain from the sweep on the default scene to PNG files, the
textured sphere from the device's own mesh and atlas, and the entry point's refusals."""
import ctypes as C

import numpy as np
import pytest

import mesh_texture_reference as tr
import render_score_reference as sr
from test_mesh_texture_gpu import default_scene_maps
from test_mesh_texture_reference import read_png

pytestmark = pytest.mark.gpu


def tile():
    from sfm_amd.mesh import score_tile
    return score_tile()


def reference(cases, window=7, rel_tol=0.02):
    out = [sr.score_view(*c.args(), window, rel_tol) for c in cases]
    return sr.Score(np.array([o[0] for o in out], np.int64).reshape(-1, 16), [o[1] for o in out], [o[2] for o in out], 3 if cases[0].color.ndim == 3 else 1)


def device_score(cases, window=7, rel_tol=0.02):
    from sfm_amd import score_render
    pick = lambda name: None if getattr(cases[0], name) is None else [getattr(c, name) for c in cases]
    return score_render(pick("color"), pick("triangle"), pick("depth"), pick("photo"), pick("view_depth"), pick("view_keep"), pick("mask"), window, rel_tol)


@pytest.mark.parametrize("window", [3, 7, 11])
@pytest.mark.parametrize("channels", [1, 3])
def test_sizes_around_the_window_and_the_tile(gpu_ready, channels, window):
    """Widths and heights from 1, W - 1, W, W + 1, T - 1, T, T + 1 and 2 T + 3 with T the tile's side in that direction: all 64
    images as the views of one call, every pixel covered but one, with the views' depth."""
    tw, th = tile()
    widths = [1, window - 1, window, window + 1, tw - 1, tw, tw + 1, 2 * tw + 3]
    heights = [1, window - 1, window, window + 1, th - 1, th, th + 1, 2 * th + 3]
    cases = [sr.random_case(1000 * window + 100 * channels + 8 * i + j, h, w, channels, "middle", False, True, (tw, th))
             for i, h in enumerate(heights) for j, w in enumerate(widths)]
    want = reference(cases, window)
    got = device_score(cases, window)
    at = heights.index(th + 1) * 8 + widths.index(window)          # the T + 1 by W view: two tiles high, one window wide
    assert got.stats[at].tolist() == want.stats[at].tolist()
    sr.assert_same(got, want, (channels, window))
    assert got.sizes == [(c.triangle.shape[1], c.triangle.shape[0]) for c in cases]
    assert want.stats[:, sr.N_SSIM].sum() > 500 and (want.stats[:, sr.N_SSIM] == 0).sum() >= 15 and want.stats[:, sr.Q_SSIM].min() < 0


@pytest.mark.parametrize("pattern", sr.PATTERNS)
def test_coverage_patterns(gpu_ready, pattern):
    """All, none, a checkerboard, one uncovered pixel in the middle of a tile, one on a tile's corner, about 90 % at random: each
    with and without a mask, gray and three channels, windows 3 and 7, over more than one tile in both directions."""
    tw, th = tile()
    h, w = 2 * th + 3, 2 * tw + 3
    for k, (mask, channels, window) in enumerate([(False, 1, 7), (True, 3, 7), (True, 1, 3), (False, 3, 3)]):
        cases = [sr.random_case(500 + 10 * sr.PATTERNS.index(pattern) + k, h, w, channels, pattern, mask, True, (tw, th))]
        want = reference(cases, window)
        sr.assert_same(device_score(cases, window), want, (pattern, mask, channels, window))
        covered = int((cases[0].triangle >= 0).sum())
        assert covered == {"all": h * w, "none": 0, "middle": h * w - 1, "corner": h * w - 1}.get(pattern, covered)
        assert (want.stats[0, sr.N_COMPARED] < covered) == (mask and covered > 0)
        if pattern == "corner" and not mask:                       # the hole is far enough inside for all W W windows that hold it to exist
            assert want.stats[0, sr.N_SSIM] == (h - window + 1) * (w - window + 1) - window * window


@pytest.mark.parametrize("with_depth", [False, True])
def test_a_batch_equals_its_views_one_by_one(gpu_ready, with_depth):
    """Three views of different sizes, one with a side of 0, with and without the views' depth."""
    tw, th = tile()
    cases = [sr.random_case(60 + k, h, w, 3, "random", True, with_depth, (tw, th)) for k, (h, w) in enumerate([(th + 5, 2 * tw + 1), (0, 9), (3 * th, tw - 3)])]
    both = device_score(cases, 5, 0.03)
    sr.assert_same(both, reference(cases, 5, 0.03), "batch")
    assert (both.stats[:, sr.N_BOTH:].any()) == with_depth and both.stats[1].tolist() == [0] * 16
    for v in range(3):
        alone = device_score(cases[v:v + 1], 5, 0.03)
        assert alone.stats[0].tolist() == both.stats[v].tolist(), v
        assert alone.abs_error[0].tobytes() == both.abs_error[v].tobytes() and alone.ssim_map[0].tobytes() == both.ssim_map[v].tobytes(), v


def raw_call(cases, window, rel_tol, spare, maps=True, guard=0xAB):
    """sfm_render_score with outputs that have `spare` bytes more than the call needs, holding `guard`, and a table with a spare
    row in front of which the call's rows end; maps=False passes NULL for abs_error and ssim_map."""
    import torch
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    ch = 3 if cases[0].color.ndim == 3 else 1
    heights = np.array([c.triangle.shape[0] for c in cases], dtype=np.int32)
    widths = np.array([c.triangle.shape[1] for c in cases], dtype=np.int32)
    n = int(sum(c.triangle.size for c in cases))
    cat = lambda name, dt: torch.from_numpy(np.concatenate([np.ascontiguousarray(getattr(c, name), dtype=dt).reshape(-1) for c in cases] + [np.zeros(1, dt)])).to(dev)
    opt = lambda name, dt: None if getattr(cases[0], name) is None else cat(name, dt)
    d = dict(color=cat("color", np.uint8), tri=cat("triangle", np.int32), depth=cat("depth", np.float32), photo=cat("photo", np.uint8),
             mask=opt("mask", np.uint8), vd=opt("view_depth", np.float32), vk=opt("view_keep", np.uint8))
    full = lambda nbytes: torch.full((nbytes + spare,), guard, dtype=torch.uint8, device=dev)
    out = dict(stats=full(len(cases) * 128), abs_error=full(n * ch), ssim_map=full(n * 4))
    hp = lambda a: C.c_void_p(a.ctypes.data)
    dp = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    need = C.c_int64()
    h.check(h.lib.sfm_render_score_workspace_bytes(len(cases), hp(heights), hp(widths), C.byref(need)), "workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    h.call("sfm_render_score", len(cases), hp(heights), hp(widths), ch, dp(d["color"]), dp(d["tri"]), dp(d["depth"]), dp(d["photo"]), dp(d["mask"]), dp(d["vd"]),
           dp(d["vk"]), window, C.c_double(rel_tol), dp(out["stats"]), dp(out["abs_error"]) if maps else None, dp(out["ssim_map"]) if maps else None,
           dp(ws), need.value)
    return {k: v.cpu().numpy() for k, v in out.items()}, n, ch


@pytest.mark.parametrize("shapes", [[(0, 4)], [(3, 5)], [(9, 16), (4, 0), (19, 67)]])
def test_nothing_is_written_past_the_outputs_and_null_maps_change_no_statistic(gpu_ready, shapes):
    """Outputs with 4,096 bytes past what the views need keep what they held there; the table is cleared by the call itself; with
    NULL for both maps the table is the same and the maps' buffers are untouched."""
    cases = [sr.random_case(80 + k, h, w, 3, "all", False, True) for k, (h, w) in enumerate(shapes)]
    want = reference(cases, 7, 0.02)
    got, n, ch = raw_call(cases, 7, 0.02, 4096)
    flat = lambda arrays: np.concatenate([np.asarray(a).reshape(-1) for a in arrays]).view(np.uint8)
    for name, w in (("stats", want.stats.reshape(-1).view(np.uint8)), ("abs_error", flat(want.abs_error)), ("ssim_map", flat(want.ssim_map))):
        g = got[name]
        assert g[:len(w)].tobytes() == w.tobytes(), name
        assert len(g) - len(w) == 4096 and (g[len(w):] == 0xAB).all(), name
    bare = raw_call(cases, 7, 0.02, 4096, maps=False)[0]
    assert bare["stats"].tobytes() == got["stats"].tobytes()
    assert (bare["abs_error"] == 0xAB).all() and (bare["ssim_map"] == 0xAB).all()


def test_python_layer_without_maps_and_without_depth(gpu_ready):
    from sfm_amd import mesh as mm
    cases = [sr.random_case(90, 21, 40, 1, "random", False, True)]
    want = reference(cases, 3)
    got = device_score(cases, 3)
    sr.assert_same(got, want, "with depth")
    assert got.pooled() == sr.figures(want.stats, 1) and got.window == 3 and got.channels == 1
    for c in cases:
        c.view_depth = c.view_keep = None
    bare = device_score(cases, 3)
    assert bare.stats[0, :sr.N_BOTH].tolist() == want.stats[0, :sr.N_BOTH].tolist() and not bare.stats[0, sr.N_BOTH:].any()
    # view_keep None with view_depth keeps every pixel
    depth = cases[0].depth
    vd = np.where(np.isnan(depth), 1.0, depth * 1.01).astype(np.float32)
    r = mm.score_render([cases[0].color], [cases[0].triangle], [depth], [cases[0].photo], [vd])
    want = sr.score_view(cases[0].color, cases[0].triangle, depth, cases[0].photo, None, vd, np.ones(vd.shape, np.uint8))
    assert r.stats[0].tolist() == want[0].tolist() and r.depth_agree[0] == 1.0 and r.view_only[0] == int((cases[0].triangle < 0).sum())


def test_default_scene_from_depth_maps_to_png_files(gpu_ready, tmp_path):
    """depth_maps -> filter -> tsdf -> mesh -> texture -> score on the default scene (96 x 72, 3 cameras) at resolution 32, gray and
    BGR: the restatement applied to the device's own render bytes, and the PNG files read back."""
    from sfm_amd import RenderScore
    s, maps = default_scene_maps()
    mesh = maps.tsdf(resolution=32).mesh()
    assert mesh.n_triangles > 1000
    with pytest.raises(ValueError, match="colour"):
        mesh.score(list(s.images))                                 # neither atlas nor vertex colours yet
    for channels in (1, 3):
        images = list(s.images) if channels == 1 else [np.stack([a, 255 - a, a // 2 + 17], axis=-1) for a in s.images]
        mesh.texture(images, texels=4)
        score = mesh.score(images)
        r = mesh.render_views()
        photos = [images[v] for v in maps.views]
        want = sr.score(r.color, r.triangle, r.depth, photos, None, maps.depth, maps.keep, 7, 0.02)
        assert isinstance(score, RenderScore) and score.sizes == [(96, 72)] * 3 and score.channels == channels
        sr.assert_same(score, want, ("default scene", channels))
        f = score.pooled()
        print(f"default scene, {channels} channel(s): MAE {np.mean(f['mae']):.3f} PSNR {f['psnr']:.3f} SSIM {f['ssim']:.4f} over {f['n_ssim']} windows; "
              f"depth within 2 % {f['depth_agree']:.4f} of {f['depth_both']}, render only {f['render_only']}, view only {f['view_only']}")
        assert f == sr.figures(want.stats, channels) and f["n_ssim"] > 1000 and f["depth_both"] > 1000 and 0.0 < f["ssim"] <= 1.0
        assert score.worst(3) == [int(i) for i in np.argsort(score.ssim, kind="stable")]
        for c in range(3):
            score.save_png(tmp_path / f"error{c}.png", camera=c)
            png = read_png(tmp_path / f"error{c}.png")
            assert np.array_equal(png, want.abs_error[c][:, :, ::-1] if channels == 3 else want.abs_error[c])
            score.save_png(tmp_path / f"ssim{c}.png", camera=c, what="ssim")
            m = want.ssim_map[c].astype(np.float64)
            gray = np.where(np.isnan(m), 0, np.floor((np.nan_to_num(m) + 1.0) * 127.5 + 0.5)).astype(np.uint8)
            assert np.array_equal(read_png(tmp_path / f"ssim{c}.png"), gray)
    # the render compared by hand with masks, other options and the statistics alone; the vertex colours by name
    masks = [(np.arange(72 * 96).reshape(72, 96) % 5 > 0).astype(np.uint8) * 9 for _ in range(3)]
    other = r.compare(photos, maps, masks=masks, window=5, rel_tol=0.005, keep_maps=False)
    want = sr.score(r.color, r.triangle, r.depth, photos, masks, maps.depth, maps.keep, 5, 0.005)
    assert np.array_equal(other.stats, want.stats) and other.abs_error is None and other.ssim_map is None
    plain = r.compare(photos)
    assert not plain.stats[:, sr.N_BOTH:].any() and np.array_equal(plain.stats[:, :sr.N_BOTH], score.stats[:, :sr.N_BOTH])
    mesh.colors(images)
    vertex = mesh.score(images, colors="vertex", window=3)
    rv = mesh.render_views(colors="vertex")
    sr.assert_same(vertex, sr.score(rv.color, rv.triangle, rv.depth, photos, None, maps.depth, maps.keep, 3, 0.02), "vertex colours")


def test_sphere_from_the_device_mesh_and_atlas_meets_the_worth_bounds(gpu_ready):
    """The textured sphere of the worth test (128 x 128, 14 views, texels 6): TSDF, mesh, atlas, vertex colours, render and score
    all on the device, held to the bounds of tests/test_render_score_reference.py."""
    from sfm_amd import mesh_texture, mesh_vertex_colors, render_mesh, score_render
    from sfm_amd.mesh import tsdf_volume_from_depth_arrays
    proj, depth, origin, voxel, shape, trunc, centres, images = tr.textured_sphere_scene(128, 180.0, 24.0)
    mesh = tsdf_volume_from_depth_arrays(proj, depth, None, origin, voxel, shape, trunc).mesh()
    t = mesh_texture(mesh.vertices, mesh.normals, mesh.triangles, proj, centres, depth, None, images, trunc, texels=6)
    vcol = mesh_vertex_colors(mesh.vertices, mesh.normals, proj, centres, depth, None, images, trunc)[0]
    sizes = [(128, 128)] * len(proj)
    ra = render_mesh(mesh.vertices, mesh.triangles, proj, sizes, uv=t.uv, atlas=t.image)
    rv = render_mesh(mesh.vertices, mesh.triangles, proj, sizes, vertex_colors=vcol)
    on_device = lambda render, photos, view_depths, rel_tol=0.02: score_render(render.color, render.triangle, render.depth, photos, view_depths, None, None, 7, rel_tol).stats
    r = sr.worth_of(ra, rv, images, depth, on_device)
    a, v = r["atlas"], r["vertex"]
    print(f"sphere on the device: atlas MAE {np.mean(a['mae']):.3f} PSNR {a['psnr']:.3f} SSIM {a['ssim']:.4f}; vertex colours {np.mean(v['mae']):.3f} "
          f"{v['psnr']:.3f} {v['ssim']:.4f}; covered {r['covered']}, within 1 % {r['agree'][0]:.4f} .. {r['agree'][1]:.4f}")
    sr.assert_worth(r)
    assert np.array_equal(on_device(ra, images, depth), sr.reference_score_fn(ra, images, depth))


def test_entry_point_rejects_bad_arguments(gpu_ready):
    """SFM_ERR_ARG (-1) before any device work: the data pointers are null or stand-ins throughout, so a call that got as far
    as a launch would not return -1 but fault."""
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    i32 = lambda *v: np.array(v, dtype=np.int32)
    one = C.c_void_p(1)                                            # stands for a pointer that is there; never followed
    good = dict(n=2, hs=i32(3, 4), ws=i32(4, 7), ch=3, color=one, tri=one, depth=one, photos=one, mask=None, vd=one, vk=one, window=7, tol=0.02, stats=one,
                err=None, ssim=None, workspace=one, ws_bytes=1 << 20)

    def call(a):
        return lib.sfm_render_score(h._h, a["n"], hp(a["hs"]), hp(a["ws"]), a["ch"], a["color"], a["tri"], a["depth"], a["photos"], a["mask"], a["vd"], a["vk"],
                                    a["window"], a["tol"], a["stats"], a["err"], a["ssim"], a["workspace"], a["ws_bytes"])

    why = lambda: lib.sfm_last_error(h._h)
    bad = [dict(n=-1), dict(n=65536), dict(hs=i32(3, -1)), dict(ws=i32(4, 32769)), dict(ch=2), dict(ch=0), dict(ch=4), dict(window=1), dict(window=13),
           dict(window=6), dict(window=-7), dict(tol=-0.5), dict(tol=float("nan")), dict(tol=float("inf")), dict(vd=None), dict(vk=None), dict(ws_bytes=64),
           dict(workspace=None)]
    for kw in bad:
        assert call(dict(good, **kw)) == -1, kw
        assert not why().endswith(b": null pointer"), (kw, why())
    for name in ("hs", "ws", "color", "tri", "depth", "photos", "stats"):
        assert call(dict(good, **{name: None})) == -1 and why().endswith(b": null pointer"), name
    need = C.c_int64()
    assert lib.sfm_render_score_workspace_bytes(2, hp(good["hs"]), hp(good["ws"]), C.byref(need)) == 0 and need.value < (1 << 20)
    assert call(dict(good, ws_bytes=need.value - 1)) == -1 and why().endswith(b"too small")
    assert lib.sfm_render_score(None, 0, None, None, 1, None, None, None, None, None, None, None, 7, 0.02, None, None, None, None, 0) == -1
