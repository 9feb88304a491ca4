"""The mesh colouring without a device: the restatement on arrays of tests/mesh_color_reference.py against the one in plain
loops, the hand cases, the rule and plan headers built for the host (bit for bit against NumPy, and under the sanitizers as
a stand-alone program), what the rule is worth on the coloured sphere, the argument checks and the PLY writer."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mesh_color_reference as cr
import mesh_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "mesh_color_check.cpp")
MIXED_SIZES = [(7, 5), (1, 1), (16, 9), (0, 4), (12, 20)]         # (h, w): one view of a single pixel, one without a pixel


# ------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("channels", [1, 3])
def test_the_two_restatements_agree(channels):
    """200 random vertices, 5 views of mixed sizes, with and without keep: every byte."""
    for seed, with_keep in ((11, True), (12, False)):
        s = cr.random_scene(seed + channels, 200, MIXED_SIZES, channels, with_keep)
        got = cr.colors(*s.args(), channels=channels)
        cr.assert_same(cr.colors_loops(*s.args(), channels=channels), got, (seed, channels))
        assert got[0].shape == ((200,) if channels == 1 else (200, 3))
        # the scene is not a trivial one: unseen vertices, vertices with several views, at least three views the best of some
        assert (got[1] == 0).sum() > 10 and (got[1] >= 2).sum() > 40 and len(set(got[2]) - {-1}) >= 3 and 3 not in got[2]
        assert ((got[2] == -1) == (got[1] == 0)).all() and (got[0][got[1] == 0] == s.fill).all()


def test_no_view_at_all():
    s = cr.random_scene(3, 10, [], 3)
    for fn in (cr.colors, cr.colors_loops):
        col, n_views, best = fn(*s.args(), channels=3)
        assert col.shape == (10, 3) and (col == s.fill).all() and (n_views == 0).all() and (best == -1).all()


# ------------------------------------------------------------------------------------------- hand cases
def test_hand_cases():
    names = []
    for name, s, col, n_views, best in cr.hand_cases():
        for fn in (cr.colors, cr.colors_loops):
            cr.assert_same(fn(*s.args()), (col, n_views, best), (name, fn.__name__))
        names.append(name)
    assert len(names) == 13
    for channels in (1, 3):
        s, col, n_views, best = cr.merged_hand_cases(channels)
        for fn in (cr.colors, cr.colors_loops):
            cr.assert_same(fn(*s.args()), (col, n_views, best), ("merged", channels, fn.__name__))
        assert len(s.vertices) == 25 and (best >= 0).sum() == 14 and len(s.proj) == 18 and best.max() == 16


def test_300_views_saturate_n_views():
    s = cr.many_views(300, 2)
    col, n_views, best = cr.colors(*s.args())
    cr.assert_same(cr.colors_loops(*s.args()), (col, n_views, best), "300 views")
    assert (n_views == 255).all() and (best == 0).all()            # every weight is 1: the tie goes to the first view
    few = cr.many_views(254, 2)
    assert (cr.colors(*few.args())[1] == 254).all()


# ------------------------------------------------------------------------------------------- what the rule is worth
# measured with the restatement on the coloured sphere scene (`sphere_scene()` defaults, 14 rendered views of 64 x 64, the
# analytic texture 127.5 + 100 sin(3 X_k); tol = 3 voxels, min_cos 0.35): (median, p95, max) of the absolute error in grey
# levels against the texture at the vertex's radial foot point, for the blend and for the nearest pixel of best_view alone
BLEND_MEASURED = (0.28, 1.11, 8.42)
SINGLE_MEASURED = (0.98, 4.55, 13.68)
_SPHERE = {}


def coloured_sphere():
    """The scene, the restatement's mesh of it and the restatement's colours, made once."""
    if not _SPHERE:
        proj, depth, origin, voxel, shape, trunc, centres, images = cr.colour_sphere_scene()
        tsdf, weight = mr.integrate(proj, depth, None, origin, voxel, shape, trunc)
        _SPHERE["scene"] = (proj, depth, origin, voxel, shape, trunc, centres, images)
        _SPHERE["mesh"] = mr.mesh(tsdf, weight, origin, voxel, shape, 1)
        _SPHERE["colors"] = cr.colors(_SPHERE["mesh"].vertices, _SPHERE["mesh"].normals, proj, centres, depth, None, images, trunc, 0.35, 0)
    return _SPHERE["scene"], _SPHERE["mesh"], _SPHERE["colors"]


def test_coloured_sphere_scene():
    proj, depth, origin, voxel, shape, trunc, centres, images = cr.colour_sphere_scene()
    ref = mr.sphere_scene()
    assert np.array_equal(proj, ref[0]) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(depth, ref[1])) and trunc == ref[5]
    assert len(images) == 14 and all(a.shape == (64, 64, 3) and a.dtype == np.uint8 for a in images)
    for d, img, C, P in zip(depth, images, centres, proj):
        hit = np.isfinite(d)
        assert (img[~hit] == 0).all() and hit.sum() > 1000 and img[hit].min() >= 27 and img[hit].max() <= 228
        assert np.allclose(P.reshape(3, 4) @ np.r_[C, 1.0], 0.0, atol=1e-9)          # the centre is the projection's
    # a pixel next to the middle of the first camera (on the +x axis, 3 in front of the sphere): its ray hits within half a
    # pixel, 0.5 / 90 * 3 = 0.017, of (1, 0, 0), which the texture's slope of at most 300 per unit turns into 5 grey levels
    assert abs(int(images[0][32, 32, 0]) - (127.5 + 100 * np.sin(3.0))) < 6 and abs(int(images[0][32, 32, 1]) - 127.5) < 6


def test_worth_on_the_coloured_sphere():
    """Measured: 7,006 vertices, each with 2 to 5 views; blend median 0.28, p95 1.11, max 8.42 grey levels; the nearest pixel
    of the single best view 0.98, 4.55, 13.68.  Asserted: no vertex is unseen; the blend's p95 at most the measured value
    plus 1 grey level (the rounding of the rendered images, and room for a changed mesh) and at most half the single view's."""
    (proj, depth, origin, voxel, shape, trunc, centres, images), m, (col, n_views, best) = coloured_sphere()
    assert n_views.min() >= 1 and (best >= 0).all()
    blend = cr.error_summary(col, m.vertices)
    single = cr.error_summary(cr.nearest_pixel_of_best_view(m.vertices, best, proj, images), m.vertices)
    print(f"coloured sphere: {len(m.vertices)} vertices, views per vertex {n_views.min()} .. {n_views.max()}, blend median / p95 / max "
          f"{blend[0]:.2f} / {blend[1]:.2f} / {blend[2]:.2f}, single view {single[0]:.2f} / {single[1]:.2f} / {single[2]:.2f}")
    assert blend[1] <= BLEND_MEASURED[1] + 1.0
    assert blend[1] <= 0.5 * single[1]


# measured with the restatements on the default scene (the maps, the box at resolution 64 and the mesh of
# tests/test_mesh_reference.py, its three gray images, tol = 3 voxels, min_cos 0.35): the share of the vertices that at least
# one view sees
SEEN_SHARE = 0.972


def test_seen_share_on_the_default_scene():
    """Measured: 11,573 vertices, 97.2 % with at least one view (319 with none, 165 with one, 5,038 with two, 6,051 with
    three).  Asserted: the share less two percentage points; an unseen vertex holds fill."""
    import depth_reference as dr
    from sfm_amd.mesh import bounding_grid, projections_from_backprojections
    from test_depth_fuse_reference import scene_maps
    s, (refs, sources, warps, backproj, planes), maps = scene_maps(0)
    f = dr.filter_views(s.images, refs, sources, warps, backproj, maps, 0.02, [12 * len(src) * 25 for src in sources], 1)
    keep, xyz, depth = [v[1] for v in f], [v[2] for v in f], [m[2] for m in maps]
    origin, voxel, shape = bounding_grid(np.concatenate([x[k != 0] for x, k in zip(xyz, keep)]), 64, 0.05)
    proj = projections_from_backprojections(backproj)
    centres = np.asarray(backproj).reshape(-1, 3, 4)[:, :, 3]
    assert np.allclose(centres, [-s.poses[r][0].T @ s.poses[r][1] for r in refs], atol=1e-12)
    tsdf, weight = mr.integrate(proj, depth, keep, origin, voxel, shape, 3.0 * voxel)
    m = mr.mesh(tsdf, weight, origin, voxel, shape, 1)
    col, n_views, best = cr.colors(m.vertices, m.normals, proj, centres, depth, keep, [s.images[r] for r in refs], 3.0 * voxel, 0.35, 9)
    share = float((n_views >= 1).mean())
    print(f"default scene: {len(m.vertices)} vertices, share with a view {share:.4f}, views per vertex {np.bincount(n_views).tolist()}")
    assert share >= SEEN_SHARE - 0.02 and (col[n_views == 0] == 9).all() and n_views.max() == 3


# ------------------------------------------------------------------------------------------- the headers on the host
def build_check(tmp_path, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"), CHECK_SRC, "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return str(exe)


def run_scene(exe, tmp_path, s, channels=None):
    """The scene through the host build of the rule: (colors, n_views, best_view) as the restatements return them."""
    ch = s.channels if channels is None else channels
    nv, n_ref = len(s.vertices), len(s.depth)
    fin, fout = tmp_path / "scene.in", tmp_path / "scene.out"
    with open(fin, "wb") as f:
        f.write(np.array([n_ref, ch, nv, s.keep is not None, s.fill], np.int64).tobytes())
        f.write(np.array([s.tol, s.min_cos], np.float64).tobytes())
        f.write(np.array([d.shape[0] for d in s.depth], np.int32).tobytes())
        f.write(np.array([d.shape[1] for d in s.depth], np.int32).tobytes())
        f.write(s.proj.tobytes())
        f.write(s.centres.tobytes())
        for arrays in (s.depth, s.keep or [], s.images):
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        f.write(s.vertices.tobytes())
        f.write(s.normals.tobytes())
    run = subprocess.run([exe, "scene", str(fin), str(fout)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    raw = np.fromfile(fout, dtype=np.uint8)
    assert len(raw) == nv * (ch + 5)
    col = raw[:nv * ch].reshape(nv, ch)
    return (col[:, 0] if ch == 1 else col), raw[nv * ch:nv * (ch + 1)], raw[nv * (ch + 1):].view(np.int32)


def check_rule(exe, tmp_path, n_vertices):
    for channels in (1, 3):
        for seed, with_keep in ((21, True), (22, False)):
            s = cr.random_scene(seed, n_vertices, MIXED_SIZES, channels, with_keep)
            want = cr.colors(*s.args(), channels=channels)
            assert (want[1] >= 2).mean() > 0.2
            cr.assert_same(run_scene(exe, tmp_path, s), want, ("random", channels, with_keep))
        s, col, n_views, best = cr.merged_hand_cases(channels)
        cr.assert_same(run_scene(exe, tmp_path, s), (col, n_views, best), ("hand cases", channels))
    s = cr.many_views(300, 3)
    cr.assert_same(run_scene(exe, tmp_path, s), cr.colors(*s.args()), "300 views")
    for s in (cr.random_scene(4, 0, MIXED_SIZES, 3), cr.random_scene(4, 9, [], 1)):          # no vertex; no view
        cr.assert_same(run_scene(exe, tmp_path, s), cr.colors(*s.args(), channels=s.channels), "empty")


def test_rule_header_equals_numpy_bit_for_bit(tmp_path):
    exe = build_check(tmp_path, ["-O2"], "mesh_color_check")
    check_rule(exe, tmp_path, 20000)
    (proj, depth, origin, voxel, shape, trunc, centres, images), m, want = coloured_sphere()
    s = cr.Scene(proj, centres, depth, None, images, m.vertices, m.normals, trunc, 0.35, 0)
    cr.assert_same(run_scene(exe, tmp_path, s), want, "coloured sphere")


def test_rule_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone: the workspace, the launch size, every
    branch of the argument checks and the taps at the borders of an image; then the rule on the random scenes and the hand
    cases, where the program itself checks every index it reads through."""
    exe = build_check(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                 "-fno-omit-frame-pointer"], "mesh_color_check_san")
    run = subprocess.run([exe, "plan"], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])
    check_rule(exe, tmp_path, 1500)


# ------------------------------------------------------------------------------------------- argument checks, no device
def test_argument_checks_without_gpu():
    import inspect
    import sfm_amd
    from sfm_amd import depth as dm
    from sfm_amd import mesh as mm
    assert sfm_amd.mesh_vertex_colors is mm.mesh_vertex_colors
    assert [p.default for p in list(inspect.signature(mm.Mesh.colors).parameters.values())[2:]] == [None, None, 0.35, 0]
    assert [p.default for p in list(inspect.signature(mm.mesh_vertex_colors).parameters.values())[8:]] == [0.35, 0, 0]
    gray, bgr = np.zeros((2, 3), np.uint8), np.zeros((2, 3, 3), np.uint8)
    maps = dm.DepthMaps({"refs": [1], "imgs": [gray, gray], "radius": 2, "src_ptr": np.array([0, 0])})
    vol = mm.TsdfVolume(None, None, np.zeros(3), 0.1, (4, 4, 4))
    mesh = mm.Mesh({}, 0, 0, vol)
    assert mesh.vertex_colors is None and mesh.n_views is None and mesh.best_view is None
    with pytest.raises(ValueError, match="DepthMaps.tsdf"):
        mesh.colors([gray, gray])                                  # the volume was not built from maps
    with pytest.raises(ValueError, match="filter"):
        mesh.colors([gray, gray], maps)
    maps.keep = [np.ones((2, 3), np.uint8)]                        # as after filter(): the checks come before the device
    from sfm_amd._views import ViewSet                            # what DepthMaps.tsdf() leaves in the volume, nothing on a device
    vol.views = ViewSet(np.array([2, 2], np.int32), np.array([3, 3], np.int32), np.array([1], np.int32), np.zeros((1, 12)), np.zeros((1, 3)),
                        None, None, maps)
    for images, kw in (([gray], {}), ([gray, gray, gray], {}), ([gray, np.zeros((3, 2), np.uint8)], {}), ([gray, gray.astype(np.float32)], {}),
                       ([gray, np.zeros((2, 3, 4), np.uint8)], {}), ([gray, np.zeros(6, np.uint8)], {}),
                       ([gray, gray], dict(tol=-1.0)), ([gray, gray], dict(tol=float("nan"))), ([gray, gray], dict(tol="x")),
                       ([gray, gray], dict(min_cos=0.0)), ([gray, gray], dict(min_cos=1.5)), ([gray, gray], dict(min_cos=float("nan"))),
                       ([gray, gray], dict(fill=-1)), ([gray, gray], dict(fill=256)), ([gray, gray], dict(fill=1.5))):
        with pytest.raises(ValueError):
            mesh.colors(images, **kw)
    with pytest.raises(ValueError, match="tol"):
        mm.Mesh({}, 0, 0).colors([gray, gray], maps)               # no volume to take the truncation from
    # two views whose images differ in their channel count
    two = dm.DepthMaps({"refs": [0, 1], "imgs": [gray, gray], "radius": 2, "src_ptr": np.array([0, 0, 0])})
    two.keep = [np.ones((2, 3), np.uint8)] * 2
    with pytest.raises(ValueError, match="all be"):
        mesh.colors([gray, bgr], two)
    # the function on arrays
    V, N = np.zeros((4, 3)), np.zeros((4, 3), np.float32)
    good = dict(vertices=V, normals=N, proj=np.zeros((1, 12)), centres=np.zeros((1, 3)), depth=[np.zeros((2, 3), np.float32)], keep=None,
                images=[gray], tol=0.1)
    for bad in (dict(vertices=np.zeros((4, 2))), dict(normals=np.zeros((3, 3), np.float32)), dict(proj=np.zeros((2, 12))), dict(centres=np.zeros((1, 2))),
                dict(depth=[np.zeros(6, np.float32)]), dict(keep=[np.zeros((3, 2), np.uint8)]), dict(images=[]), dict(images=[bgr[:1]]),
                dict(images=[gray.astype(np.int32)]), dict(tol=-0.1), dict(tol=float("inf")), dict(min_cos=0), dict(min_cos=1.01), dict(fill=300)):
        with pytest.raises(ValueError):
            mm.mesh_vertex_colors(**dict(good, **bad))
    flat, channels = mm.check_color_images([bgr, np.ones((1, 1, 3), np.uint8)], [(2, 3), (1, 1)])
    assert channels == 3 and flat.dtype == np.uint8 and len(flat) == 22 and flat[18:21].tolist() == [1, 1, 1]
    assert inspect.signature(dm.dense_from_reconstruction).parameters["colors"].default is None


def test_c_entry_points_reject_bad_calls_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    need = ctypes.c_int64(-1)
    assert lib.sfm_mesh_colors_workspace_bytes(36, ctypes.byref(need)) == 0 and need.value >= 37 * 16
    assert lib.sfm_mesh_colors_workspace_bytes(0, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.sfm_mesh_colors_workspace_bytes(-1, ctypes.byref(need)) != 0 and lib.sfm_mesh_colors_workspace_bytes(65536, ctypes.byref(need)) != 0
    assert lib.sfm_mesh_colors_workspace_bytes(3, None) != 0
    assert lib.sfm_mesh_colors(None, None, None, 0, 0, None, None, None, None, None, None, 3, 0, None, None, 0.1, 0.35, 0, None, None, None,
                               None, 0) != 0


# ------------------------------------------------------------------------------------------- the PLY file
def read_ply_coloured_mesh(path):
    """(vertices float32 [n,3], normals float32 [n,3], colours uint8 [n,3] as red, green, blue, triangles int32 [m,3]) of a
    file `save_ply_mesh` wrote with normals and colours."""
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    text = head.decode("ascii")
    props = re.findall(r"property (\w+) (\w+)\n", text[text.index("element vertex"):text.index("element face")])
    assert props == [("float", a) for a in ("x", "y", "z", "nx", "ny", "nz")] + [("uchar", c) for c in ("red", "green", "blue")]
    n = int(re.search(r"element vertex (\d+)", text).group(1))
    m = int(re.search(r"element face (\d+)", text).group(1))
    v = np.frombuffer(body[:n * 27], np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]))
    faces = np.frombuffer(body[n * 27:], np.dtype([("n", "u1"), ("v", "<i4", 3)]))
    assert len(faces) == m and (faces["n"] == 3).all()
    return v["p"], v["n"], v["c"], faces["v"]


def test_a_coloured_mesh_round_trips_through_the_ply_writer(tmp_path):
    """`Mesh.save` writes vertex_colors when it has them and is given none; an uncoloured mesh saves exactly as before."""
    from sfm_amd import Mesh, save_ply_mesh

    class Held:                                                    # what Mesh keeps per array: something with .cpu().numpy()
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    rng = np.random.default_rng(7)
    V, N = rng.normal(0, 1, (5, 3)), rng.normal(0, 1, (5, 3)).astype(np.float32)
    T = np.array([[0, 1, 2], [2, 3, 4]], np.int32)
    bgr = rng.integers(0, 256, (5, 3), dtype=np.uint8)
    gray = rng.integers(0, 256, 5, dtype=np.uint8)
    state = lambda **more: dict({"vertices": Held(V), "normals": Held(N), "triangles": Held(T)}, **more)
    plain, want = tmp_path / "plain.ply", tmp_path / "want.ply"
    Mesh(state(), 5, 2).save(plain)
    save_ply_mesh(V, T, want, normals=N)
    assert open(plain, "rb").read() == open(want, "rb").read()      # exactly as today
    path = tmp_path / "coloured.ply"
    Mesh(state(vertex_colors=Held(bgr)), 5, 2).save(path)
    v, n, c, t = read_ply_coloured_mesh(path)
    assert np.array_equal(v, V.astype(np.float32)) and np.array_equal(n, N) and np.array_equal(t, T)
    assert np.array_equal(c, bgr[:, ::-1])                         # colours are in cv2's channel order, the file in red, green, blue
    save_ply_mesh(V, T, want, normals=N, colors=bgr)
    assert open(path, "rb").read() == open(want, "rb").read()
    Mesh(state(vertex_colors=Held(gray)), 5, 2).save(path)         # a gray mesh, and colours handed in win over the mesh's own
    save_ply_mesh(V, T, want, normals=N, colors=gray)
    assert open(path, "rb").read() == open(want, "rb").read()
    assert np.array_equal(read_ply_coloured_mesh(path)[2], np.repeat(gray[:, None], 3, axis=1))
    Mesh(state(vertex_colors=Held(gray)), 5, 2).save(path, colors=bgr)
    assert np.array_equal(read_ply_coloured_mesh(path)[2], bgr[:, ::-1])
