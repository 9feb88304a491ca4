"""The mesh texture without a device: the restatement on arrays of tests/mesh_texture_reference.py against the one in plain
loops, the layout of the atlas, hand cases, what the atlas is worth on the textured sphere, the rule and plan headers built
for the host (bit for bit against NumPy, and under the sanitizers as a stand-alone program), the argument checks and the
OBJ / MTL / PNG writers."""
import ctypes
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import mesh_color_reference as cr
import mesh_texture_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "mesh_texture_check.cpp")
MIXED_SIZES = [(7, 5), (1, 1), (16, 9), (0, 4), (12, 20)]         # (h, w): one view of a single pixel, one without a pixel


# ------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("texels", [1, 2, 5, 8])
def test_the_two_restatements_agree(texels):
    """Random triangles over 40 random vertices, 5 views of mixed sizes; odd and even triangle counts, cells_per_row 1, 3 and
    the default, gray and three channels, with and without keep, one triangle with a bad index: every byte."""
    seen = several = 0
    for case, (n_triangles, cells_per_row) in enumerate(((7, 1), (6, 3), (9, None), (4, 3))):
        channels, with_keep = (1, 3)[case % 2], case < 2
        s = tr.random_scene(40 * texels + case, 40, n_triangles, MIXED_SIZES, channels, with_keep, bad=[(1, 2, 40)])
        got = tr.reference(s, texels, cells_per_row)
        tr.assert_same(tr.texture_loops(*s.args(), channels=channels, **s.kwargs(texels, cells_per_row)), got, (texels, case))
        W, H = tr.atlas_size(n_triangles, texels, tr.default_cells_per_row(n_triangles) if cells_per_row is None else cells_per_row)
        assert got[0].shape == ((H, W) if channels == 1 else (H, W, 3)) and got[1].shape == (H, W) and got[2].shape == (n_triangles, 3, 2)
        seen += int((got[1] > 0).sum())
        several += int((got[1] >= 2).sum())
    assert seen > 20 * texels and several > 10 * texels                 # not a trivial scene


def test_the_blend_is_that_of_the_colouring():
    """The per-view steps restated for float64 normals give `mesh_color_reference.colors` byte for byte on normals that
    float32 holds exactly, and so does the scalar form."""
    for channels in (1, 3):
        s = cr.random_scene(50 + channels, 300, MIXED_SIZES, channels)
        col, n_views, best = cr.colors(*s.args(), channels=channels)
        got, m = tr.blend(s.vertices, s.normals.astype(np.float64), s.proj, s.centres, s.depth, s.keep, s.images, s.tol, s.min_cos, s.fill, channels)
        assert np.array_equal(got.reshape(col.shape), col) and np.array_equal(m, n_views) and (m >= 2).sum() > 60
        for i in range(0, 300, 7):
            one, m1 = tr.blend_one([np.float64(t) for t in s.vertices[i]], [np.float64(t) for t in s.normals[i]], s.proj, s.centres, s.depth, s.keep,
                                   s.images, np.float64(s.tol), np.float64(s.min_cos), s.fill, channels)
            assert one == got[i].tolist() and m1 == m[i]


def test_no_triangle_and_no_view():
    s = tr.random_scene(3, 10, 0, MIXED_SIZES, 3)
    for fn in (tr.texture, tr.texture_loops):
        image, views, uv = fn(*s.args(), channels=3, **s.kwargs(4, 2))
        assert image.shape == (0, 14, 3) and views.shape == (0, 14) and uv.shape == (0, 3, 2) and uv.dtype == np.float32
    s = tr.random_scene(3, 10, 5, [], 3)
    for fn in (tr.texture, tr.texture_loops):
        image, views, uv = fn(*s.args(), channels=3, **s.kwargs(2))
        assert image.shape == (10, 10, 3) and (image == s.fill).all() and (views == 0).all()


# ------------------------------------------------------------------------------------------- the layout
@pytest.mark.parametrize("texels", [1, 2, 5, 8])
def test_the_map_and_its_inverse(texels):
    s = texels
    for n_triangles, cpr in ((1, 1), (2, 1), (5, 1), (6, 3), (9, 2), (10, None)):
        cpr = tr.default_cells_per_row(n_triangles) if cpr is None else cpr
        W, H = tr.atlas_size(n_triangles, s, cpr)
        tri, ii, jj = tr.inverse_map(n_triangles, s, cpr)
        assert tri.shape == (H, W)
        # the map: every (t, i, j) has a texel of its own, which the inverse map returns
        local = [(i, j) for i in range(s + 2) for j in range(s + 2 - i)]
        owner = np.full((H, W), -1)
        for t in range(n_triangles):
            for i, j in local:
                x, y = (int(a) for a in tr.texel_at(t, i, j, s, cpr))
                assert 0 <= x < W and 0 <= y < H and owner[y, x] == -1, "no texel belongs to two triangles"
                owner[y, x] = t
                assert (tri[y, x], ii[y, x], jj[y, x]) == (t, i, j)
        # the inverse map: every texel with a triangle maps back to itself; the rest belongs to nothing
        assert np.array_equal(owner, tri)
        ys, xs = np.nonzero(tri >= 0)
        bx, by = tr.texel_at(tri[ys, xs], ii[ys, xs], jj[ys, xs], s, cpr)
        assert np.array_equal(bx, xs) and np.array_equal(by, ys)
        assert (tri >= 0).sum() == n_triangles * (s + 2) * (s + 3) // 2
        y, x = np.mgrid[0:H, 0:W]
        assert (tri[(x % (s + 3)) + (y % (s + 3)) == s + 2] == -1).all()                 # the unused diagonal
        if n_triangles % 2:
            c = n_triangles // 2
            x0, y0 = (c % cpr) * (s + 3), (c // cpr) * (s + 3)
            cell = tri[y0:y0 + s + 3, x0:x0 + s + 3]
            assert (cell >= 0).sum() == (s + 2) * (s + 3) // 2 and set(np.unique(cell)) == {-1, n_triangles - 1}          # the empty half
        # numerators: non-negative, sum 2 s; the corners are the vertices; the gutter lies on the hypotenuse
        n0, n1, n2 = tr.numerators(ii, jj, s)
        assert (n0 >= 0).all() and (n1 >= 0).all() and (n2 >= 0).all() and (n0 + n1 + n2 == 2 * s).all()
        assert (n0[(ii + jj == s + 1) & (tri >= 0)] == 0).all()
        for (i, j), want in (((0, 0), (2 * s, 0, 0)), ((s, 0), (0, 2 * s, 0)), ((0, s), (0, 0, 2 * s)), ((0, s + 1), (0, 0, 2 * s)),
                             ((s + 1, 0), (0, 2 * s, 0)), ((1, s), (0, 1, 2 * s - 1))):
            assert tuple(int(n) for n in tr.numerators(i, j, s)) == want


def test_unused_texels_get_fill_and_zero():
    """The unused diagonal, the empty half of an odd count and the cells past the last triangle."""
    s = tr.random_scene(8, 30, 5, [(12, 20), (16, 9)], 3)
    s.s.fill = s.fill = 77
    image, views, uv = tr.reference(s, 5, 2)
    tri, i, j = tr.inverse_map(5, 5, 2)
    assert image.shape == (16, 16, 3) and (tri == -1).sum() == 16 * 16 - 5 * 28
    assert (image[tri == -1] == 77).all() and (views[tri == -1] == 0).all() and (views[tri >= 0] > 0).sum() > 40


def test_bilinear_taps_stay_inside_the_triangle():
    """10,000 random points inside random triangles of random layouts: the four taps of a bilinear lookup at the
    interpolated uv that have a non-zero weight all belong to that triangle.  With the uv in double - as the rule computes
    them before it rounds - for any point, edges and corners included; with the float32 uv for points whose barycentric
    coordinates are at least 1e-3, which is more than the rounding of a float32 uv moves a point here (2^-24 of an atlas
    of at most 110 texels: 7e-6 texel, 7e-6 of a barycentric coordinate at texels = 1)."""
    rng = np.random.default_rng(5)
    n_points = 0
    for case in range(100):
        s = int(rng.choice([1, 2, 3, 5, 8]))
        nt = int(rng.integers(1, 40))
        cpr = [1, 3, tr.default_cells_per_row(nt)][case % 3]
        W, H = tr.atlas_size(nt, s, cpr)
        tri, ii, jj = tr.inverse_map(nt, s, cpr)
        uv32 = tr.corner_uv(nt, s, cpr)
        t = np.arange(nt, dtype=np.int64)[:, None]
        cx, cy = tr.texel_at(t, np.array([0, s, 0])[None, :], np.array([0, 0, s])[None, :], s, cpr)
        uv64 = np.stack([(cx + 0.5) / W, (cy + 0.5) / H], axis=-1)
        assert np.array_equal(uv64.astype(np.float32), uv32)
        which = rng.integers(0, nt, 100)
        bary = rng.dirichlet([1.0, 1.0, 1.0], 100)
        bary[:10] = np.eye(3)[rng.integers(0, 3, 10)]                                    # corners
        bary[10:20, 0] = 0.0                                                             # the hypotenuse
        bary[10:20, 1:] /= bary[10:20, 1:].sum(axis=1, keepdims=True)
        bary[20:30, 1] = 0.0                                                             # the i axis
        bary[20:30] /= bary[20:30].sum(axis=1, keepdims=True)
        inner = 1e-3 + (1.0 - 3e-3) * bary
        # a weight below 1e-9 of a lookup in double is the rounding of this test's own arithmetic (1e-13), not a tap
        for uv, b, least in ((uv64, bary, 1e-9), (uv32.astype(np.float64), inner, 0.0)):
            x, y, w = tr.bilinear_taps((b[:, :, None] * uv[which]).sum(axis=1), W, H)
            w = np.where(w <= least, 0.0, w)
            used = w > 0
            assert (x[used] >= 0).all() and (x[used] < W).all() and (y[used] >= 0).all() and (y[used] < H).all()
            owner = np.where(used, tri[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], which[:, None])
            assert np.array_equal(owner, np.broadcast_to(which[:, None], owner.shape)), (case, s, nt, cpr)
            assert np.allclose(w.sum(axis=1), 1.0, atol=1e-6)
            n_points += len(which)
    assert n_points == 20000


# ------------------------------------------------------------------------------------------- hand cases
def fronto_parallel(images, normals=((0, 0, -1),) * 3, triangles=((0, 1, 2),)):
    """One camera at the origin with f = 2 and 5 x 3 pixels in front of the plane z = 2: a point (x, y, 2) falls on
    (u, v) = (x + 2, y + 1).  The triangle (-1, -0.5), (1, -0.5), (-1, 0.5) lies inside the image."""
    front, origin = cr.camera((0, 0, 0), 5, 3)
    V = [(-1.0, -0.5, 2.0), (1.0, -0.5, 2.0), (-1.0, 0.5, 2.0)]
    scene = cr.Scene([front], [origin], [np.full((3, 5), 2.0, np.float32)], [np.ones((3, 5), np.uint8)], images, V, normals,
                     cr.HAND_TOL, cr.HAND_MIN_COS, cr.HAND_FILL)
    return tr.Scene(scene, triangles)


def test_hand_cases():
    for fn in (tr.texture, tr.texture_loops):
        # a constant image gives a constant patch
        s = fronto_parallel([np.full((3, 5), 200, np.uint8)])
        image, views, uv = fn(*s.args(), **s.kwargs(4, 1))
        tri, i, j = tr.inverse_map(1, 4, 1)
        assert image.shape == (7, 7) and (image[tri == 0] == 200).all() and (views[tri == 0] == 1).all()
        assert (image[tri < 0] == cr.HAND_FILL).all() and (views[tri < 0] == 0).all() and (tri == 0).sum() == 21
        # the ramp 10 x + 40 y + 10 is linear, so a texel holds the ramp at its point: u = 2 n1 / 2s + 1, v = n2 / 2s + 0.5
        for texels in (1, 4, 5):
            s = fronto_parallel([cr.ramp(5, 3)])
            image, views, uv = fn(*s.args(), **s.kwargs(texels, 1))
            tri, i, j = tr.inverse_map(1, texels, 1)
            n0, n1, n2 = tr.numerators(i, j, texels)
            want = np.floor(10.0 * (n1 / texels + 1.0) + 40.0 * (n2 / (2.0 * texels) + 0.5) + 10.0 + 0.5)
            assert np.array_equal(image[tri == 0], want[tri == 0].astype(np.uint8)) and (views[tri == 0] == 1).all()
            # the corners sit on texel centres
            assert image[0, 0] == 40 and image[0, texels] == 60 and image[texels, 0] == 80
            assert np.array_equal(uv, (np.array([[[0.5, 0.5], [texels + 0.5, 0.5], [0.5, texels + 0.5]]]) / (texels + 3)).astype(np.float32))
        # the second triangle of a cell is the first turned by half a turn: corner 0 at the cell's last texel
        s = fronto_parallel([cr.ramp(5, 3)], triangles=((0, 1, 2), (0, 1, 2)))
        image, views, uv = fn(*s.args(), **s.kwargs(4, 1))
        tri = tr.inverse_map(2, 4, 1)[0]
        assert np.array_equal(image[::-1, ::-1][tri == 0], image[tri == 0]) and image[6, 6] == 40 and image[6, 2] == 60 and image[2, 6] == 80
        assert np.array_equal(uv[1], (np.array([[6.5, 6.5], [2.5, 6.5], [6.5, 2.5]]) / 7).astype(np.float32))
        # a triangle with a bad index gives fill, and its neighbour is untouched
        for bad in (-1, 3):
            s = fronto_parallel([cr.ramp(5, 3)], triangles=((0, bad, 2), (0, 1, 2)))
            again, views, uv2 = fn(*s.args(), **s.kwargs(4, 1))
            tri2 = tr.inverse_map(2, 4, 1)[0]
            assert (again[tri2 == 0] == cr.HAND_FILL).all() and (views[tri2 == 0] == 0).all() and np.array_equal(again[tri2 == 1], image[tri2 == 1])
            assert np.array_equal(uv2, uv)
        # a normal turned away: no view; the normal of a texel is interpolated and then normalised
        s = fronto_parallel([cr.ramp(5, 3)], normals=((0, 0, 1),) * 3)
        assert (fn(*s.args(), **s.kwargs(2, 1))[1] == 0).all()
        s = fronto_parallel([cr.ramp(5, 3)], normals=((0, 0, -4), (0, 0, -0.01), (0, 0, 0)))          # lengths do not count, zero passes
        assert (fn(*s.args(), **s.kwargs(2, 1))[1][tr.inverse_map(1, 2, 1)[0] == 0] == 1).all()


# ------------------------------------------------------------------------------------------- what the atlas is worth
# measured with the restatements on the sphere scene of `mesh_reference.sphere_scene` (14 cameras, 32^3 nodes, voxel 0.09) at
# 128 x 128 pixels with f = 180, the analytic texture 127.5 + 100 sin(24 X_k), texels = 6, tol = 3 voxels, min_cos 0.35:
# (median, p95, max) of the absolute error in grey levels against the texture at the radial foot point over the interior
# texels of every triangle, for the atlas and for the vertex colours of `sfm_mesh_colors` interpolated across the triangle
ATLAS_MEASURED = (1.54, 7.47, 33.10)
INTERPOLATED_MEASURED = (3.58, 21.01, 61.65)


def test_worth_on_the_textured_sphere():
    """Measured: 14,032 triangles, 392,896 interior texels, none unseen; atlas median 1.54, p95 7.47, max 33.10 grey levels (RMS
    3.62); interpolated vertex colours 3.58, 21.01, 61.65 (RMS 9.50).  Asserted: no interior texel is unseen; the atlas p95 at
    most the measured value plus 1 grey level and at most half of the interpolated colours' p95 (measured: 0.36 of it)."""
    r = tr.sphere_worth(128, 180.0, 24.0, 6)
    print(f"textured sphere: {r['triangles']} triangles, {r['texels']} interior texels, {r['unseen']} unseen; atlas median / p95 / max "
          f"{r['atlas'][0]:.2f} / {r['atlas'][1]:.2f} / {r['atlas'][2]:.2f} (RMS {r['rms'][0]:.2f}), interpolated "
          f"{r['interpolated'][0]:.2f} / {r['interpolated'][1]:.2f} / {r['interpolated'][2]:.2f} (RMS {r['rms'][1]:.2f})")
    assert r["unseen"] == 0 and r["texels"] == r["triangles"] * 28
    assert r["atlas"][1] <= ATLAS_MEASURED[1] + 1.0
    assert r["atlas"][1] <= 0.5 * r["interpolated"][1]


# ------------------------------------------------------------------------------------------- the headers on the host
def build_check(tmp_path, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"), CHECK_SRC, "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return str(exe)


def run_scene(exe, tmp_path, s, texels, cells_per_row):
    """The scene through the host build of the rule: ((image, views, uv), tri, numerators, points, normals)."""
    c, T = s.s, s.triangles
    ch, nv, nt, n_ref = s.channels, len(c.vertices), len(T), len(c.depth)
    fin, fout = tmp_path / "scene.in", tmp_path / "scene.out"
    with open(fin, "wb") as f:
        f.write(np.array([n_ref, ch, nv, nt, texels, cells_per_row, c.keep is not None, s.fill], np.int64).tobytes())
        f.write(np.array([s.tol, s.min_cos], np.float64).tobytes())
        f.write(np.array([d.shape[0] for d in c.depth], np.int32).tobytes())
        f.write(np.array([d.shape[1] for d in c.depth], np.int32).tobytes())
        f.write(c.proj.tobytes())
        f.write(c.centres.tobytes())
        for arrays in (c.depth, c.keep or [], c.images):
            for a in arrays:
                f.write(np.ascontiguousarray(a).tobytes())
        f.write(c.vertices.tobytes())
        f.write(c.normals.tobytes())
        f.write(np.ascontiguousarray(T, dtype=np.int32).tobytes())
    run = subprocess.run([exe, "scene", str(fin), str(fout)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    raw = open(fout, "rb").read()
    W, H = tr.atlas_size(nt, texels, cells_per_row)
    n = H * W
    sizes = [n * ch, n, nt * 24, n * 8, n * 12, n * 24, n * 24]
    assert len(raw) == sum(sizes)
    parts, at = [], 0
    for size in sizes:
        parts.append(raw[at:at + size])
        at += size
    image = np.frombuffer(parts[0], np.uint8).reshape((H, W) if ch == 1 else (H, W, 3))
    return ((image, np.frombuffer(parts[1], np.uint8).reshape(H, W), np.frombuffer(parts[2], np.float32).reshape(nt, 3, 2)),
            np.frombuffer(parts[3], np.int64).reshape(H, W), np.frombuffer(parts[4], np.int32).reshape(H, W, 3),
            np.frombuffer(parts[5], np.float64).reshape(H, W, 3), np.frombuffer(parts[6], np.float64).reshape(H, W, 3))


def check_rule(exe, tmp_path, n_triangles):
    """Random meshes: the numerators, the points, the normals, the uv and every byte of the atlas."""
    for case, (texels, cells_per_row) in enumerate(((1, 1), (2, 3), (5, None), (8, 7), (64, 2))):
        nt = 3 if texels == 64 else n_triangles + case % 2
        channels = (1, 3)[case % 2]
        cpr = tr.default_cells_per_row(nt) if cells_per_row is None else cells_per_row
        s = tr.random_scene(60 + case, 50, nt, MIXED_SIZES, channels, with_keep=case != 2, bad=[(0, 0, -1), (2, 1, 50)])
        want = tr.reference(s, texels, cpr)
        got, tri, nums, X, normal = run_scene(exe, tmp_path, s, texels, cpr)
        tr.assert_same(got, want, ("random", case))
        wtri, i, j = tr.inverse_map(nt, texels, cpr)
        good, wX, wn = tr.points_of(wtri, i, j, s.s.vertices, s.s.normals, s.triangles, texels)
        assert np.array_equal(tri, wtri) and not good[wtri == 0].any() and not good[wtri == 2].any() and good[wtri == 1].all()
        assert np.array_equal(nums[good], np.stack(tr.numerators(i, j, texels), axis=-1)[good])
        assert np.array_equal(X.view(np.uint64), wX.view(np.uint64)) and np.array_equal(normal.view(np.uint64), wn.view(np.uint64))
        assert (want[1] >= 2).mean() > 0.1 and np.isnan(wX).any() and (wn[good] == 0).all(axis=-1).any() or texels == 64
    s = tr.random_scene(4, 9, 0, MIXED_SIZES, 3)                   # no triangle
    tr.assert_same(run_scene(exe, tmp_path, s, 3, 2)[0], tr.reference(s, 3, 2), "no triangle")
    s = tr.random_scene(4, 0, 3, MIXED_SIZES, 1)                   # no vertex: every index is bad
    got = run_scene(exe, tmp_path, s, 3, 2)[0]
    tr.assert_same(got, tr.reference(s, 3, 2), "no vertex")
    assert (got[0] == s.fill).all()
    s = tr.random_scene(4, 9, 5, [], 1)                            # no view
    tr.assert_same(run_scene(exe, tmp_path, s, 3, 2)[0], tr.reference(s, 3, 2), "no view")


def test_rule_header_equals_numpy_bit_for_bit(tmp_path):
    exe = build_check(tmp_path, ["-O2"], "mesh_texture_check")
    check_rule(exe, tmp_path, 400)


def test_rule_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone: the size of the atlas, the grid, every
    branch of the argument checks and the map and its inverse over small layouts; then the rule on random meshes, where the
    program itself checks every index it reads through."""
    exe = build_check(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                 "-fno-omit-frame-pointer"], "mesh_texture_check_san")
    run = subprocess.run([exe, "plan"], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])
    check_rule(exe, tmp_path, 40)


# ------------------------------------------------------------------------------------------- argument checks, no device
def test_argument_checks_without_gpu():
    import inspect
    import sfm_amd
    from sfm_amd import depth as dm
    from sfm_amd import mesh as mm
    assert sfm_amd.mesh_texture is mm.mesh_texture and sfm_amd.MeshTexture is mm.MeshTexture
    assert [p.default for p in list(inspect.signature(mm.Mesh.texture).parameters.values())[2:]] == [8, None, None, 0.35, 0, None]
    assert [p.default for p in list(inspect.signature(mm.mesh_texture).parameters.values())[9:]] == [8, 0.35, 0, None, 0]
    assert inspect.signature(dm.dense_from_reconstruction).parameters["texture"].default is None
    # the layout in Python is that of the restatement
    for nt, s, cpr in ((0, 8, None), (1, 1, None), (5, 3, 2), (211428, 8, None), (7, 64, 1)):
        want_cpr = tr.default_cells_per_row(nt) if cpr is None else cpr
        assert mm.check_texture_layout(nt, s, cpr) == (want_cpr,) + tr.atlas_size(nt, s, want_cpr)
    assert mm.check_texture_layout(211428, 8, None) == (326, 3586, 3575)
    for nt, s, cpr in ((4, 0, None), (4, 65, None), (4, 2.0, None), (4, 8, 0), (4, 8, -1), (4, 8, 1.5), (4, 64, 490), (2 * 489 * 489 + 1, 64, 489),
                       (-1, 8, None), (1 << 31, 1, None)):
        with pytest.raises(ValueError):
            mm.check_texture_layout(nt, s, cpr)
    gray = np.zeros((2, 3), np.uint8)
    maps = dm.DepthMaps({"refs": [1], "imgs": [gray, gray], "radius": 2, "src_ptr": np.array([0, 0])})
    vol = mm.TsdfVolume(None, None, np.zeros(3), 0.1, (4, 4, 4))
    mesh = mm.Mesh({}, 0, 4, vol)
    assert mesh.atlas is None
    with pytest.raises(ValueError, match="DepthMaps.tsdf"):
        mesh.texture([gray, gray])
    with pytest.raises(ValueError, match="filter"):
        mesh.texture([gray, gray], maps=maps)
    maps.keep = [np.ones((2, 3), np.uint8)]                        # as after filter(): the checks come before the device
    from sfm_amd._views import ViewSet                            # what DepthMaps.tsdf() leaves in the volume, nothing on a device
    vol.views = ViewSet(np.array([2, 2], np.int32), np.array([3, 3], np.int32), np.array([1], np.int32), np.zeros((1, 12)), np.zeros((1, 3)),
                        None, None, maps)
    for images, kw in (([gray], {}), ([gray, np.zeros((3, 2), np.uint8)], {}), ([gray, gray.astype(np.float32)], {}),
                       ([gray, gray], dict(texels=0)), ([gray, gray], dict(texels=65)), ([gray, gray], dict(texels=4.0)),
                       ([gray, gray], dict(cells_per_row=0)), ([gray, gray], dict(texels=64, cells_per_row=490)),
                       ([gray, gray], dict(tol=-1.0)), ([gray, gray], dict(min_cos=0.0)), ([gray, gray], dict(fill=256))):
        with pytest.raises(ValueError):
            mesh.texture(images, **kw)
    with pytest.raises(ValueError, match="texture"):
        mesh.save_obj("nowhere.obj")
    assert mesh.atlas is None
    # the function on arrays
    V, N = np.zeros((4, 3)), np.zeros((4, 3), np.float32)
    good = dict(vertices=V, normals=N, triangles=np.array([[0, 1, 2]]), proj=np.zeros((1, 12)), centres=np.zeros((1, 3)),
                depth=[np.zeros((2, 3), np.float32)], keep=None, images=[gray], tol=0.1)
    for bad in (dict(vertices=np.zeros((4, 2))), dict(normals=np.zeros((3, 3), np.float32)), dict(triangles=np.zeros((1, 4), np.int32)),
                dict(triangles=np.zeros((1, 3))), dict(triangles=np.array([[0, 1, 1 << 31]])), dict(proj=np.zeros((2, 12))), dict(centres=np.zeros((1, 2))),
                dict(depth=[np.zeros(6, np.float32)]), dict(keep=[np.zeros((3, 2), np.uint8)]), dict(images=[]), dict(images=[gray.astype(np.int32)]),
                dict(tol=-0.1), dict(min_cos=0), dict(fill=300), dict(texels=0), dict(texels=65), dict(cells_per_row=0),
                dict(texels=64, cells_per_row=490)):
        with pytest.raises(ValueError):
            mm.mesh_texture(**dict(good, **bad))
    for kw in (dict(texture=0), dict(texture=65), dict(texture=2.5), dict(texture=8), dict(texture=8, mesh=True), dict(texture=8, colors=[gray])):
        with pytest.raises(ValueError, match="texture"):
            dm.dense_from_reconstruction(None, [], **kw)


def test_c_entry_points_reject_bad_calls_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    W, H = ctypes.c_int32(-1), ctypes.c_int32(-1)
    size = lambda nt, s, cpr: lib.sfm_mesh_texture_size(nt, s, cpr, ctypes.byref(W), ctypes.byref(H))
    for nt, s, cpr in ((0, 8, 1), (1, 1, 1), (5, 3, 2), (211428, 8, 326), (2 * 489 * 489, 64, 489), (7, 5, 3)):
        assert size(nt, s, cpr) == 0 and (W.value, H.value) == tr.atlas_size(nt, s, cpr), (nt, s, cpr)
    for nt, s, cpr in ((4, 0, 2), (4, 65, 2), (4, -1, 2), (4, 8, 0), (4, 8, -1), (4, 64, 490), (2 * 489 * 489 + 1, 64, 489), (-1, 8, 2), (1 << 31, 8, 40000),
                       (4, 1, 0x7FFFFFFF)):
        assert size(nt, s, cpr) == -1, (nt, s, cpr)
    assert lib.sfm_mesh_texture_size(4, 8, 2, None, ctypes.byref(H)) == -1 and lib.sfm_mesh_texture_size(4, 8, 2, ctypes.byref(W), None) == -1
    need = ctypes.c_int64(-1)
    assert lib.sfm_mesh_texture_workspace_bytes(36, ctypes.byref(need)) == 0 and need.value >= 37 * 16
    assert lib.sfm_mesh_texture_workspace_bytes(0, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.sfm_mesh_texture_workspace_bytes(-1, ctypes.byref(need)) != 0 and lib.sfm_mesh_texture_workspace_bytes(65536, ctypes.byref(need)) != 0
    assert lib.sfm_mesh_texture_workspace_bytes(3, None) != 0
    assert lib.sfm_mesh_texture(None, None, None, 0, 0, None, None, None, None, None, None, 3, 0, None, None, 0, None, 8, 1, 0.1, 0.35, 0, None,
                                None, None, None, 0) != 0


# ------------------------------------------------------------------------------------------- the OBJ, MTL and PNG files
def read_png(path):
    """uint8 [h,w] or [h,w,3] of an 8-bit gray or RGB PNG without interlace whose rows all have filter type 0."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(raw):
        n, kind = struct.unpack(">I4s", raw[at:at + 8])
        data = raw[at + 8:at + 8 + n]
        assert struct.unpack(">I", raw[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data) & 0xFFFFFFFF
        chunks.append((kind, data))
        at += 12 + n
    assert [k for k, d in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    w, h, depth, colour, compression, filtering, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, compression, filtering, interlace) == (8, 0, 0, 0) and colour in (0, 2)
    ch = 3 if colour == 2 else 1
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + w * ch)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape((h, w) if ch == 1 else (h, w, 3))


def read_obj(path):
    """(v float64 [n,3], vn [n,3], vt [m,2], faces int [f,3,3] as written (1-based v/vt/vn), mtllib, usemtl)."""
    v, vn, vt, faces, names = [], [], [], [], {}
    for line in open(path).read().splitlines():
        key, _, rest = line.partition(" ")
        if key == "v":
            v.append([float(t) for t in rest.split()])
        elif key == "vn":
            vn.append([float(t) for t in rest.split()])
        elif key == "vt":
            vt.append([float(t) for t in rest.split()])
        elif key == "f":
            faces.append([[int(t) if t else 0 for t in (corner.split("/") + ["", ""])[:3]] for corner in rest.split()])
        elif key in ("mtllib", "usemtl"):
            names[key] = rest
    return (np.array(v).reshape(-1, 3), np.array(vn).reshape(-1, 3), np.array(vt).reshape(-1, 2), np.array(faces, dtype=np.int64).reshape(-1, 3, 3),
            names.get("mtllib"), names.get("usemtl"))


def assert_obj_files(path, V, N, T, uv, image, bgr=True):
    """The three files of `save_obj_mesh` read back."""
    stem = os.path.splitext(str(path))[0]
    v, vn, vt, faces, mtllib, usemtl = read_obj(path)
    assert np.array_equal(v, V) and np.array_equal(vn.astype(np.float32), N)                  # %.17g and %.9g round-trip
    assert mtllib == os.path.basename(stem) + ".mtl" and usemtl == "atlas"
    mtl = open(stem + ".mtl").read()
    assert "newmtl atlas\n" in mtl and f"map_Kd {os.path.basename(stem)}.png\n" in mtl
    nt = len(T)
    assert faces.shape == (nt, 3, 3) and np.array_equal(faces[:, :, 0], T + 1) and np.array_equal(faces[:, :, 2], T + 1)
    assert np.array_equal(faces[:, :, 1], np.arange(3 * nt).reshape(nt, 3) + 1)
    flat = uv.reshape(-1, 2).astype(np.float64)
    assert vt.shape == (3 * nt, 2) and np.array_equal(vt[:, 0].astype(np.float32), uv.reshape(-1, 2)[:, 0])
    assert np.allclose(vt[:, 1], 1.0 - flat[:, 1], rtol=0, atol=1e-8) and (vt[:, 1] > 0.5).any() == (flat[:, 1] < 0.5).any()          # the flip
    png = read_png(stem + ".png")
    assert np.array_equal(png, image[:, :, ::-1] if (bgr and image.ndim == 3) else image)


def test_obj_mtl_and_png_round_trip(tmp_path):
    from sfm_amd import Mesh, MeshTexture, save_obj_mesh, write_png

    class Held:                                                    # what Mesh keeps per array: something with .cpu().numpy()
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    rng = np.random.default_rng(9)
    V, N = rng.normal(0, 1, (5, 3)), rng.normal(0, 1, (5, 3)).astype(np.float32)
    T = np.array([[0, 1, 2], [2, 3, 4], [4, 1, 0]], np.int32)
    uv = tr.corner_uv(3, 4, 2)
    W, H = tr.atlas_size(3, 4, 2)
    for channels in (1, 3):
        image = rng.integers(0, 256, (H, W) if channels == 1 else (H, W, 3), dtype=np.uint8)
        path = tmp_path / f"mesh{channels}.obj"
        save_obj_mesh(V, T, path, normals=N, uv=uv, texture=image)
        assert_obj_files(path, V, N, T, uv, image)
        # through Mesh.save_obj, from the atlas the mesh holds and from one handed in
        state = {"vertices": Held(V), "normals": Held(N), "triangles": Held(T)}
        atlas = MeshTexture({"image": Held(image.reshape(-1)), "views": Held(np.zeros(H * W, np.uint8)), "uv": Held(uv.reshape(-1))}, (W, H), 4, 2, channels, 3)
        assert atlas.image.shape == image.shape and atlas.views.shape == (H, W) and atlas.uv.shape == (3, 3, 2) and atlas.size == (W, H)
        mesh = Mesh(state, 5, 3)
        other = tmp_path / f"held{channels}.obj"
        mesh.save_obj(other, atlas)
        assert_obj_files(other, V, N, T, uv, image)
        mesh.atlas = atlas
        mesh.save_obj(other)
        assert open(other).read() == open(path).read().replace(f"mesh{channels}", f"held{channels}")
    rgb = tmp_path / "rgb.obj"
    save_obj_mesh(V, T, rgb, normals=N, uv=uv, texture=image, bgr=False)
    assert_obj_files(rgb, V, N, T, uv, image, bgr=False)
    # without uv and normals: plain faces and no other file
    bare = tmp_path / "bare.obj"
    save_obj_mesh(V, T, bare)
    v, vn, vt, faces, mtllib, usemtl = read_obj(bare)
    assert np.array_equal(v, V) and len(vn) == 0 and len(vt) == 0 and np.array_equal(faces[:, :, 0], T + 1) and (faces[:, :, 1:] == 0).all()
    assert mtllib is None and not os.path.exists(tmp_path / "bare.mtl") and not os.path.exists(tmp_path / "bare.png")
    save_obj_mesh(V, T, bare, normals=N)
    assert "f 1//1 2//2 3//3" in open(bare).read()
    for kw in (dict(uv=uv[:2]), dict(normals=N[:4]), dict(texture=image), dict(uv=uv, texture=image.astype(np.float32))):
        with pytest.raises(ValueError):
            save_obj_mesh(V, T, tmp_path / "bad.obj", **kw)
    with pytest.raises(ValueError):
        save_obj_mesh(V, np.array([[0, 1, 5]]), tmp_path / "bad.obj")
    # the PNG writer on its own: one pixel, a wide gray row, and what it refuses
    for image in (np.array([[7]], np.uint8), rng.integers(0, 256, (1, 300), dtype=np.uint8), rng.integers(0, 256, (17, 3, 3), dtype=np.uint8)):
        write_png(tmp_path / "one.png", image)
        assert np.array_equal(read_png(tmp_path / "one.png"), image)
    for image in (np.zeros((0, 4), np.uint8), np.zeros((2, 2, 4), np.uint8), np.zeros((2, 2), np.uint16), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError):
            write_png(tmp_path / "bad.png", image)
