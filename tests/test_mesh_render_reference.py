"""The mesh render without a device: the restatement on arrays of tests/mesh_render_reference.py against the one in plain
loops, hand cases with expectations worked out by hand, two properties, what the render is worth on the textured sphere,
the rule and plan headers built for the host (bit for bit against NumPy, and under the sanitizers as a stand-alone
program), and the argument checks."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_render_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "mesh_render_check.cpp")
SIZES = [(5, 3), (9, 16), (4, 0), (14, 11)]                        # (width, height): one camera without a pixel
SOURCES = [(None, 1, False), ("vertex", 1, False), ("vertex", 3, False), ("atlas", 1, True), ("atlas", 3, False)]


# ------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("n_triangles", [0, 1, 7, 40])
def test_the_two_restatements_agree(n_triangles):
    """Random meshes over 50 vertices (NaN coordinates, bad indices, triangles that span an image and triangles of a few
    pixels), four cameras, every source of colour: every byte, and the count of boxes above 64 pixels."""
    drawn = 0
    for case, (source, channels, wild) in enumerate(SOURCES):
        s = rr.random_scene(100 * n_triangles + case, 50, n_triangles, SIZES, source, channels, wild)
        want, got = rr.reference(s), rr.render_loops(*s.args(), **s.kwargs())
        rr.assert_same(got, want, (n_triangles, case))
        assert got.n_large == want.n_large
        assert [d.shape for d in want.depth] == [(h, w) for w, h in SIZES] and (want.color is None) == (source is None)
        drawn += sum(int((t >= 0).sum()) for t in want.triangle)
    assert drawn > 50 or n_triangles < 7                           # of 1,565 pixels: not a trivial scene


def test_the_close_up_scene_has_both_kinds_of_box():
    s = rr.close_up_scene()
    want = rr.reference(s)
    rr.assert_same(rr.render_loops(*s.args(), **s.kwargs()), want, "close-up")
    assert want.n_large == 4 and len(s.triangles) - want.n_large > 200 and want.coverage[0] > 0.3
    assert sum((want.triangle[0] == t).any() for t in range(len(s.triangles) - 4, len(s.triangles))) >= 2      # large ones in front of the grid show
    assert len(np.unique(want.triangle[0])) > 100                                                                  # and so do the small ones


# ------------------------------------------------------------------------------------------- hand cases
def hand(name):
    return next((V, T, size) for n, V, T, size in rr.hand_cases() if n == name)


@pytest.mark.parametrize("fn", [rr.render, rr.render_loops])
def test_hand_cases(fn):
    draw = lambda name, **kw: (lambda V, T, size: fn(V, T, [rr.UNIT], [size], **kw))(*hand(name))
    nan = np.isnan
    # overlap: A (depth 4) covers x + y <= 4, B (depth 2) covers x + y <= 2 of it and is in front
    r = draw("overlap")
    y, x = np.mgrid[0:5, 0:6]
    assert np.array_equal(r.triangle[0], np.where(x + y <= 2, 1, np.where(x + y <= 4, 0, -1)))
    assert np.array_equal(r.depth[0][x + y <= 4], np.where(x + y <= 2, 2.0, 4.0)[x + y <= 4].astype(np.float32)) and nan(r.depth[0][x + y > 4]).all()
    assert rr.bits(r.depth[0][x + y > 4]).tolist() == [0x7FC00000] * int((x + y > 4).sum()) and (r.bary[0][x + y > 4] == 0).all()
    # shared edge: the square's 25 pixels once each; the five on the diagonal tie in depth and go to triangle 0
    r = draw("shared edge")
    y, x = np.mgrid[0:6, 0:6]
    inside = (x <= 4) & (y <= 4)
    assert np.array_equal(r.triangle[0], np.where(inside, np.where(x >= y, 0, 1), -1)) and (r.depth[0][inside] == 2.0).all()
    assert (r.triangle[0][np.arange(5), np.arange(5)] == 0).all()
    # a vertex on the pixel centre (2, 1): that pixel alone, with the weight all on that corner
    r = draw("vertex on a pixel centre")
    assert (r.triangle[0] >= 0).sum() == 1 and r.triangle[0][1, 2] == 0 and r.depth[0][1, 2] == 2.0 and r.bary[0][1, 2].tolist() == [1.0, 0.0, 0.0]
    for name in ("between pixel centres", "zero area", "a corner behind the camera"):
        r = draw(name)
        assert (r.triangle[0] == -1).all() and nan(r.depth[0]).all() and (r.bary[0] == 0).all(), name
    # a NaN vertex, an index of n_vertices and one of -1 draw nothing; the sound triangle behind them draws as number 3
    r = draw("NaN vertex and bad indices")
    y, x = np.mgrid[0:6, 0:6]
    assert np.array_equal(r.triangle[0], np.where(x + y <= 4, 3, -1))
    # both orientations: the clockwise triangle at depth 2 hides the counter-clockwise one at depth 4
    r = draw("both orientations")
    assert np.array_equal(r.triangle[0], np.where(x + y <= 4, 0, -1)) and (r.depth[0][x + y <= 4] == 2.0).all()
    V, T, size = hand("both orientations")
    back = fn(V, T[::-1], [rr.UNIT], [size])
    assert np.array_equal(back.triangle[0], np.where(x + y <= 4, 1, -1)) and np.array_equal(rr.bits(back.depth[0]), rr.bits(r.depth[0]))
    # larger than the image: every pixel, at the plane's depth; 1 x 1 and 0 x 4 images
    r = draw("larger than the image", vertex_colors=np.array([10, 10, 10], np.uint8), fill=99)
    assert (r.triangle[0] == 0).all() and (r.depth[0] == 4.0).all() and r.depth[0].shape == (3, 5) and (r.color[0] == 10).all()
    assert np.allclose(r.bary[0].sum(axis=-1), 1.0, atol=3e-7)
    r = draw("one pixel")
    assert r.triangle[0].tolist() == [[0]] and r.depth[0].tolist() == [[4.0]] and r.coverage == [1.0]
    r = draw("no pixel", vertex_colors=np.zeros((3, 3), np.uint8))
    assert r.triangle[0].shape == (4, 0) and r.depth[0].shape == (4, 0) and r.bary[0].shape == (4, 0, 3) and r.color[0].shape == (4, 0, 3) and r.coverage == [0.0]


@pytest.mark.parametrize("fn", [rr.render, rr.render_loops])
def test_hand_colours(fn):
    """The triangle (0,0), (4,0), (0,4) at depth 2 with the vertex colours 0, 200, 100: the pixel (x, y) has the weights
    (4 - x - y, x, y) / 4, so its colour is 50 x + 25 y.  With an atlas of 4 x 4 texels holding 10 c + 40 r and the corners'
    uv on the texel centres (0,0), (2,0), (0,2), the pixel samples the atlas at (x / 2, y / 2): 5 x + 20 y."""
    V, T = np.array([rr.at(0, 0, 2), rr.at(4, 0, 2), rr.at(0, 4, 2)]), np.array([[0, 1, 2]], np.int32)
    y, x = np.mgrid[0:6, 0:6]
    inside = x + y <= 4
    r = fn(V, T, [rr.UNIT], [(6, 6)], vertex_colors=np.array([0, 200, 100], np.uint8), fill=7)
    assert np.array_equal(r.color[0], np.where(inside, 50 * x + 25 * y, 7).astype(np.uint8))
    rgb = np.array([[0, 0, 255], [200, 40, 255], [100, 80, 255]], np.uint8)
    r = fn(V, T, [rr.UNIT], [(6, 6)], vertex_colors=rgb, fill=7)
    assert np.array_equal(r.color[0], np.where(inside[..., None], np.stack([50 * x + 25 * y, 10 * x + 20 * y, 255 + 0 * x], axis=-1), 7).astype(np.uint8))
    ay, ax = np.mgrid[0:4, 0:4]
    atlas = (10 * ax + 40 * ay).astype(np.uint8)
    uv = np.array([[[0.5 / 4, 0.5 / 4], [2.5 / 4, 0.5 / 4], [0.5 / 4, 2.5 / 4]]], np.float32)
    r = fn(V, T, [rr.UNIT], [(6, 6)], uv=uv, atlas=atlas, fill=7)
    assert np.array_equal(r.color[0], np.where(inside, 5 * x + 20 * y, 7).astype(np.uint8))
    # uv outside the atlas clamp to its border texels, a NaN uv gives 255: no index leaves the atlas
    wild = np.array([[[-3.0, -3.0], [-3.0, -3.0], [-3.0, -3.0]]], np.float32)
    assert (fn(V, T, [rr.UNIT], [(6, 6)], uv=wild, atlas=atlas).color[0][inside] == 0).all()
    assert (fn(V, T, [rr.UNIT], [(6, 6)], uv=-wild, atlas=atlas).color[0][inside] == 150).all()
    assert (fn(V, T, [rr.UNIT], [(6, 6)], uv=wild * np.nan, atlas=atlas).color[0][inside] == 255).all()


# ------------------------------------------------------------------------------------------- properties
def test_permuting_the_triangles_permutes_the_indices():
    """Wherever the two nearest depths of a pixel differ, the permuted list shows the same triangle under its new number
    with the same depth and barycentrics; the scene's triangles overlap, so the property is not empty."""
    s = rr.random_scene(11, 50, 60, [(14, 11), (9, 16)], "vertex", 3)
    a = rr.reference(s)
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(s.triangles))                       # new list: triangle j is the old perm[j]
    b = rr.render(s.vertices, s.triangles[perm], s.proj, s.sizes, **s.kwargs())
    old_of_new = np.append(perm, -1)
    ties = 0
    for c in range(2):
        back = old_of_new[b.triangle[c]]
        same = back == a.triangle[c]
        assert np.array_equal(rr.bits(a.depth[c]), rr.bits(b.depth[c]))            # the depth never depends on the order
        ties += int((~same).sum())
        assert np.array_equal(rr.bits(a.bary[c][same]), rr.bits(b.bary[c][same])) and np.array_equal(a.color[c][same], b.color[c][same])
        assert (a.triangle[c] >= 0).sum() > 10
    assert ties == 0                                               # no two triangles of this scene tie in float32 at a pixel


def test_a_plane_renders_its_depth():
    """A mesh of the plane z = c in front of an axis-aligned camera: every covered pixel has depth == (float)c exactly, with
    barycentrics that sum to 1 within float32 rounding (three roundings of at most 2^-24 each, 1.8e-7)."""
    rng = np.random.default_rng(8)
    for c in (0.7, 3.0, 1e3 / 3):
        g = np.linspace(-1.0, 1.0, 6) * c
        gx, gy = np.meshgrid(g, g)
        V = np.c_[gx.ravel() + rng.normal(0, 0.02 * c, 36), gy.ravel() + rng.normal(0, 0.02 * c, 36), np.full(36, c)]
        T = np.array([t for j in range(5) for i in range(5) for t in ((j * 6 + i, j * 6 + i + 1, j * 6 + i + 6), (j * 6 + i + 1, j * 6 + i + 7, j * 6 + i + 6))])
        P = np.array([20.0, 0, 15.5, 0, 0, 20.0, 11.5, 0, 0, 0, 1.0, 0])
        r = rr.render(V, T, [P], [(32, 24)])
        on = r.triangle[0] >= 0
        assert on.sum() > 400 and (r.depth[0][on] == np.float32(c)).all()
        assert np.abs(r.bary[0][on].astype(np.float64).sum(axis=-1) - 1.0).max() <= 1.8e-7 and (r.bary[0][on] >= 0).all()


# ------------------------------------------------------------------------------------------- what the render is worth
# measured with the restatements on the textured sphere of `mesh_texture_reference.textured_sphere_scene` (14 cameras, 32^3
# nodes, voxel 0.09, 128 x 128 pixels, f = 180, texture 127.5 + 100 sin(24 X_k), texels 6), drawn through its 14 cameras and
# through one at (2.9, 1.6, 1.1) that is none of them: (median, p95, max) of the absolute error in grey levels against
# the analytic image over the covered pixels, and the largest depth error in voxels where the ray meets the sphere at a
# cosine of at least 0.5
ATLAS_MEASURED = (3.70, 31.08, 193.70)
VERTEX_MEASURED = (8.38, 37.71, 190.49)
DEPTH_MEASURED = 0.633


def test_worth_on_the_textured_sphere():
    """Measured: 14,032 triangles, 15 cameras, 42.6 to 43.3 % of the pixels covered (56.7 % for the novel camera); atlas
    render median 3.70, p95 31.08, max 193.70 grey levels; vertex-colour render 8.38, 37.71, 190.49; the novel camera alone
    3.57 / 33.28 / 192.72 against 7.17 / 36.12 / 179.10; rendered depth at most 0.633 voxel from the sphere over 77,204 pixels
    (0.597 for the novel camera).  The tails are the limb, where one pixel spans several periods of the texture and one
    sample per pixel cannot follow it.  No texel of a triangle that the novel camera draws is without a view.  Asserted: the
    atlas p95 at most the measured value plus 1 grey level and below the vertex colours'; the depth error at most the measured
    value plus 0.25 voxel, the margin the meshing test gives its radial error."""
    r = rr.sphere_worth(128, 180.0, 24.0, 6)
    print(f"rendered sphere: {r['triangles']} triangles, coverage {min(r['coverage']):.4f} .. {max(r['coverage']):.4f}; atlas median / p95 / max "
          f"{r['atlas'][0]:.2f} / {r['atlas'][1]:.2f} / {r['atlas'][2]:.2f}, vertex colours {r['vertex'][0]:.2f} / {r['vertex'][1]:.2f} / "
          f"{r['vertex'][2]:.2f}; depth {r['depth']:.4f} voxel over {r['pixels']} pixels; novel camera {r['novel']}")
    assert r["unseen"] == 0
    assert r["atlas"][1] <= ATLAS_MEASURED[1] + 1.0
    assert r["atlas"][1] < r["vertex"][1]
    assert r["depth"] <= DEPTH_MEASURED + 0.25


# ------------------------------------------------------------------------------------------- the headers on the host
def build_check(tmp_path, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"), CHECK_SRC, "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return str(exe)


def run_scene(exe, tmp_path, s):
    """The scene through the host build of the rule and the plan: a `Render`."""
    mode = 0 if (s.vertex_colors is None and s.atlas is None) else (1 if s.atlas is None else 2)
    src = s.vertex_colors if mode == 1 else s.atlas
    ch = 1 if mode == 0 else (3 if src.ndim == (2 if mode == 1 else 3) else 1)
    aw, ah = (s.atlas.shape[1], s.atlas.shape[0]) if mode == 2 else (0, 0)
    fin, fout = tmp_path / "scene.in", tmp_path / "scene.out"
    with open(fin, "wb") as f:
        f.write(np.array([len(s.sizes), len(s.vertices), len(s.triangles), mode, ch, aw, ah, s.fill], np.int64).tobytes())
        f.write(np.array([h for w, h in s.sizes], np.int32).tobytes())
        f.write(np.array([w for w, h in s.sizes], np.int32).tobytes())
        f.write(s.proj.tobytes())
        f.write(s.vertices.tobytes())
        f.write(s.triangles.tobytes())
        if mode == 1:
            f.write(np.ascontiguousarray(s.vertex_colors).tobytes())
        if mode == 2:
            f.write(np.ascontiguousarray(s.uv, dtype=np.float32).tobytes())
            f.write(np.ascontiguousarray(s.atlas).tobytes())
    run = subprocess.run([exe, "scene", str(fin), str(fout)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    raw = open(fout, "rb").read()
    n = sum(w * h for w, h in s.sizes)
    sizes = [n * 4, n * 4, n * 12, n * ch if mode else 0, 8]
    assert len(raw) == sum(sizes)
    at = np.cumsum([0] + sizes)
    flat = [np.frombuffer(raw[at[k]:at[k + 1]], dt) for k, dt in enumerate((np.float32, np.int32, np.float32, np.uint8, np.int64))]
    out, o = rr.Render(), 0
    for w, h in s.sizes:
        out.depth.append(flat[0][o:o + h * w].reshape(h, w))
        out.triangle.append(flat[1][o:o + h * w].reshape(h, w))
        out.bary.append(flat[2][3 * o:3 * (o + h * w)].reshape(h, w, 3))
        out.color.append(flat[3][ch * o:ch * (o + h * w)].reshape((h, w) if ch == 1 else (h, w, 3)) if mode else None)
        o += h * w
    if not mode:
        out.color = None
    out.n_large = int(flat[4][0])
    return out


def records(seed, n):
    """Records (ua, va, qa, ub, vb, qb, uc, vc, qc, x, y), tri: triangles with small integer and dyadic coordinates, so that
    many pixel centres lie exactly on an edge or a vertex; a third of them moved off it by one or two units in the last
    place; depths that agree to the float32 and differ in the double."""
    rng = np.random.default_rng(seed)
    R = np.zeros((n, 11))
    R[:, [0, 1, 3, 4, 6, 7]] = rng.integers(-8, 24, (n, 6)) / rng.choice([1.0, 2.0, 4.0], (n, 6))
    R[:, 9:11] = rng.integers(0, 16, (n, 2))
    onto = rng.random(n) < 0.3                                      # corner a onto the pixel centre
    R[onto, 0:2] = R[onto, 9:11]
    mid = rng.random(n) < 0.3                                       # the pixel centre onto the middle of the edge b c
    R[mid, 6:8] = 2 * R[mid, 9:11] - R[mid, 3:5]
    z = rng.choice([0.5, 1.0, 3.0, 7.25], n)
    R[:, 2], R[:, 5], R[:, 8] = z, z * rng.choice([1.0, 1.0, 1.5], n), z * rng.choice([1.0, 1.0, 0.75], n)
    off = rng.random(n) < 0.33
    for col in (0, 4, 7):
        R[off, col] = np.nextafter(R[off, col], R[off, col] + rng.choice([-1.0, 1.0], int(off.sum())))
    tie = rng.random(n) < 0.3                                       # a depth that differs below float32's resolution
    R[tie, 2] = R[tie, 2] * (1.0 + rng.choice([-1, 1, 2], int(tie.sum())) * 2.0 ** -40)
    return R, rng.integers(0, 0x7FFFFFFF, n).astype(np.int64)


def check_records(exe, tmp_path, n):
    R, tri = records(21, n)
    fin, fout = tmp_path / "records.in", tmp_path / "records.out"
    with open(fin, "wb") as f:
        f.write(np.array([n], np.int64).tobytes())
        rec = np.zeros(n, dtype=[("d", np.float64, 11), ("t", np.int64)])
        rec["d"], rec["t"] = R, tri
        f.write(rec.tobytes())
    run = subprocess.run([exe, "records", str(fin), str(fout)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    got = np.frombuffer(open(fout, "rb").read(), dtype=[("w", np.float64, 4), ("key", np.uint64), ("b", np.float64, 3)])
    assert len(got) == n
    ua, va, qa, ub, vb, qb, uc, vc, qc, x, y = R.T
    w0, w1, w2, A = rr.edge_functions(ua, va, ub, vb, uc, vc, x, y)
    same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))
    assert same(got["w"], np.stack([w0, w1, w2, A], axis=1))
    key = rr.claims((ua, va, qa, ub, vb, qb, uc, vc, qc), x, y, tri)
    assert np.array_equal(got["key"], key)
    with np.errstate(all="ignore"):
        r0, r1, r2 = w0 / qa, w1 / qb, w2 / qc
        s = (r0 + r1) + r2
        b = np.stack([r0 / s, r1 / s, r2 / s], axis=1)
    drawn = key != rr.NO_KEY
    assert same(got["b"][drawn], b[drawn])
    # the records are what they claim to be: edge functions at zero and next to it, both signs, both outcomes
    zero = (w0 == 0) | (w1 == 0) | (w2 == 0)
    tiny = ~zero & (np.minimum(np.minimum(np.abs(w0), np.abs(w1)), np.abs(w2)) < 1e-12)
    assert zero.sum() > n // 10 and tiny.sum() > n // 50 and (drawn & zero).sum() > n // 50 and (drawn & tiny).sum() > 5 and (~drawn & tiny).sum() > 5
    assert (A[drawn] > 0).any() and (A[drawn] < 0).any() and (A == 0).any()
    # depths that tie in float32 although they differ in double
    with np.errstate(all="ignore"):
        d64 = A / s
    d32 = d64.astype(np.float32)
    assert (drawn & (d32.astype(np.float64) != d64)).sum() > n // 20


def check_scenes(exe, tmp_path, n_triangles):
    for case, (source, channels, wild) in enumerate(SOURCES):
        s = rr.random_scene(40 + case, 50, n_triangles + case % 2, SIZES + [(40, 30)], source, channels, wild)
        want = rr.reference(s)
        got = run_scene(exe, tmp_path, s)
        rr.assert_same(got, want, ("random", case))
        assert got.n_large == want.n_large and want.n_large > 0 and sum(int((t >= 0).sum()) for t in want.triangle) > 100
    for source, channels in ((None, 1), ("vertex", 3), ("atlas", 1)):
        s = rr.merged_hand_scene(source, channels)
        rr.assert_same(run_scene(exe, tmp_path, s), rr.reference(s), ("hand", source))
    s = rr.close_up_scene()
    got = run_scene(exe, tmp_path, s)
    rr.assert_same(got, rr.reference(s), "close-up")
    assert got.n_large == 4
    for nv, nt, sizes in ((9, 0, SIZES), (0, 3, SIZES), (9, 5, []), (9, 5, [(0, 0)])):              # no triangle, no vertex, no camera, no pixel
        s = rr.random_scene(4, nv, nt, sizes, "vertex", 3)
        rr.assert_same(run_scene(exe, tmp_path, s), rr.reference(s), (nv, nt, sizes))


def test_rule_header_equals_numpy_bit_for_bit(tmp_path):
    exe = build_check(tmp_path, ["-O2"], "mesh_render_check")
    check_records(exe, tmp_path, 20000)
    check_scenes(exe, tmp_path, 120)


def test_rule_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone: every branch of the argument checks, the
    layout and the grids; then the rule on records and scenes, where the program itself checks every index it reads or writes
    through."""
    exe = build_check(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                 "-fno-omit-frame-pointer"], "mesh_render_check_san")
    run = subprocess.run([exe, "plan"], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])
    check_records(exe, tmp_path, 2000)
    check_scenes(exe, tmp_path, 30)


# ------------------------------------------------------------------------------------------- argument checks, no device
def test_argument_checks_without_gpu(tmp_path):
    import inspect
    import sfm_amd
    from sfm_amd import depth as dm
    from sfm_amd import mesh as mm
    assert sfm_amd.render_mesh is mm.render_mesh and sfm_amd.MeshRender is mm.MeshRender
    assert [p.default for p in list(inspect.signature(mm.Mesh.render).parameters.values())[3:]] == ["auto", 0]
    assert [p.default for p in list(inspect.signature(mm.render_mesh).parameters.values())[4:]] == [None, None, None, 0, 0]
    assert inspect.signature(mm.Mesh.render_views).parameters["maps"].default is None
    P = np.arange(12.0)
    K, R, t = np.diag([2.0, 2.0, 1.0]), np.eye(3), np.array([1.0, 2.0, 3.0])
    check = mm.check_render_arguments
    # one camera in every accepted form, one size for all
    for cam in (P, P.reshape(3, 4), P.tolist(), P.reshape(3, 4).tolist()):
        proj, hs, ws = check(cam, (5, 3))[:3]
        assert np.array_equal(proj, P[None]) and hs.tolist() == [3] and ws.tolist() == [5] and hs.dtype == np.int32
    for cam in ((K, (R, t)), (K, R, t), [K, (R, t)]):
        assert np.array_equal(check(cam, (5, 3))[0], (K @ np.c_[R, t]).reshape(1, 12))
    # a list of cameras, one size each or one for all; a camera without a pixel
    proj, hs, ws = check([P, (K, R, t), P.reshape(3, 4)], [(5, 3), (0, 4), (32768, 1)])[:3]
    assert proj.shape == (3, 12) and hs.tolist() == [3, 4, 1] and ws.tolist() == [5, 0, 32768]
    assert check(np.zeros((4, 12)), (2, 2))[1].tolist() == [2] * 4 and check(np.zeros((4, 3, 4)), [2, 2])[2].tolist() == [2] * 4
    assert check([], [])[0].shape == (0, 12) and check([], (4, 4))[1].shape == (0,)
    for cams, sizes, fill in ((np.zeros(11), (5, 3), 0), (np.zeros((3, 3)), (5, 3), 0), ([P, np.zeros(5)], (5, 3), 0), ((K, (R, t[:2])), (5, 3), 0),
                              ("camera", (5, 3), 0), (P, (5,), 0), (P, (5, 3, 1), 0), (P, (5.0, 3), 0), (P, (-1, 3), 0), (P, (5, 32769), 0), (P, 5, 0),
                              ([P, P], [(5, 3)], 0), ([P, P], [(5, 3), (5, 3), (5, 3)], 0), (P, [(5, 3), (5, 3)], 0), (P, (5, 3), -1), (P, (5, 3), 256),
                              (P, (5, 3), 1.0), (P, (True, 3), 0)):
        with pytest.raises(ValueError):
            check(cams, sizes, fill)
    # the source of colour
    assert [mm.resolve_render_colors(c, a, v) for c, a, v in (("auto", True, True), ("auto", False, True), ("auto", False, False), (None, True, True),
                                                              ("atlas", True, False), ("vertex", True, True))] == [2, 1, 0, 0, 2, 1]
    for c, a, v in (("atlas", False, True), ("vertex", True, False), ("both", True, True), (1, True, True)):
        with pytest.raises(ValueError):
            mm.resolve_render_colors(c, a, v)
    mesh = mm.Mesh({}, 0, 4)
    for kw in (dict(colors="atlas"), dict(colors="vertex"), dict(colors="rgb"), dict(fill=300)):
        with pytest.raises(ValueError):
            mesh.render(P, (5, 3), **kw)
    with pytest.raises(ValueError):
        mesh.render(np.zeros(11), (5, 3))
    with pytest.raises(ValueError, match="DepthMaps.tsdf"):
        mesh.render_views()
    # the function on arrays
    V, T = np.zeros((4, 3)), np.array([[0, 1, 2]])
    uv, atlas = np.zeros((1, 3, 2), np.float32), np.zeros((4, 4), np.uint8)
    out = check(P, (5, 3), 0, V, T, None, uv, atlas)
    assert out[3:5] == (2, 1) and out[6].dtype == np.int32 and out[8].dtype == np.float32
    assert check(P, (5, 3), 0, V, T, np.zeros((4, 3), np.uint8))[3:5] == (1, 3) and check(P, (5, 3), 0, V, T)[3:5] == (0, 1)
    good = dict(vertices=V, triangles=T, proj=P, sizes=(5, 3))
    for bad in (dict(vertices=np.zeros((4, 2))), dict(triangles=np.zeros((1, 4), np.int32)), dict(triangles=np.zeros((1, 3))), dict(triangles=np.array([[0, 1, 1 << 31]])),
                dict(proj=np.zeros(7)), dict(sizes=(5, -3)), dict(fill=256), dict(vertex_colors=np.zeros(3, np.uint8)), dict(vertex_colors=np.zeros((4, 2), np.uint8)),
                dict(vertex_colors=np.zeros(4, np.float32)), dict(uv=uv), dict(atlas=atlas), dict(uv=uv, atlas=atlas, vertex_colors=np.zeros(4, np.uint8)),
                dict(uv=np.zeros((2, 3, 2), np.float32), atlas=atlas), dict(uv=uv, atlas=np.zeros((4, 4, 2), np.uint8)), dict(uv=uv, atlas=np.zeros((0, 4), np.uint8)),
                dict(uv=uv, atlas=atlas.astype(np.int32)), dict(uv=uv.astype(np.int32), atlas=atlas)):
        with pytest.raises(ValueError):
            mm.render_mesh(**dict(good, **bad))

    # a render held on the host: the views per camera, the coverage, the PNG, BGR written as RGB
    class Held:
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a

        def __getitem__(self, k):
            return Held(self.a[k])

    from test_mesh_texture_reference import read_png
    rng = np.random.default_rng(2)
    n = 5 * 3 + 0 + 2 * 2
    tri = rng.integers(-1, 3, n).astype(np.int32)
    for ch in (1, 3):
        state = {"depth": Held(rng.random(n).astype(np.float32)), "triangle": Held(tri), "bary": Held(rng.random(n * 3).astype(np.float32)),
                 "color": Held(rng.integers(0, 256, n * ch, dtype=np.uint8)), "ws": Held(np.array([7, 0], np.uint64).view(np.uint8))}
        r = mm.MeshRender(state, [3, 4, 2], [5, 0, 2], ch, True)
        assert r.sizes == [(5, 3), (0, 4), (2, 2)] and [d.shape for d in r.depth] == [(3, 5), (4, 0), (2, 2)] and r.bary[2].shape == (2, 2, 3)
        assert [c.shape for c in r.color] == [(3, 5) + (3,) * (ch == 3), (4, 0) + (3,) * (ch == 3), (2, 2) + (3,) * (ch == 3)]
        assert r.coverage == [float((tri[:15] >= 0).mean()), 0.0, float((tri[15:] >= 0).mean())] and r.n_large == 7
        assert np.array_equal(r.triangle[2].ravel(), tri[15:]) and np.array_equal(r.color[2].ravel(), state["color"].a[15 * ch:])
        r.save_png(tmp_path / "view.png", camera=2)
        assert np.array_equal(read_png(tmp_path / "view.png"), r.color[2][:, :, ::-1] if ch == 3 else r.color[2])
        with pytest.raises(ValueError):
            r.save_png(tmp_path / "empty.png", camera=1)           # a camera without a pixel has no image to write
    bare = mm.MeshRender({"triangle": Held(tri)}, [3, 4, 2], [5, 0, 2], 1, False)
    assert bare.color is None
    with pytest.raises(ValueError, match="colour"):
        bare.save_png(tmp_path / "bare.png")


def test_c_entry_points_reject_bad_calls_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    i32 = lambda *v: np.array(v, dtype=np.int32)
    hp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    need = ctypes.c_int64(-1)
    size = lambda n_cam, hs, ws, nv, nt: lib.sfm_mesh_render_workspace_bytes(n_cam, hp(hs), hp(ws), nv, nt, ctypes.byref(need))
    assert size(2, i32(3, 4), i32(5, 0), 10, 6) == 0 and need.value >= 8 + 3 * 16 + 15 * 8 + 2 * 10 * 24 + 2 * 6 * 8
    small = need.value
    assert size(2, i32(30, 4), i32(50, 0), 10, 6) == 0 and need.value >= small + 1500 * 8 - 256      # the keys, less the alignment the small call already paid
    assert size(0, None, None, 0, 0) == 0 and need.value > 0
    assert size(36, i32(*[768] * 36), i32(*[1024] * 36), 106866, 211428) == 0 and need.value < (1 << 30)
    for n_cam, hs, ws, nv, nt in ((-1, i32(3), i32(3), 1, 1), (65536, i32(3), i32(3), 1, 1), (1, None, i32(3), 1, 1), (1, i32(3), None, 1, 1), (1, i32(-1), i32(3), 1, 1),
                                  (1, i32(3), i32(32769), 1, 1), (1, i32(3), i32(3), -1, 1), (1, i32(3), i32(3), 1 << 31, 1), (1, i32(3), i32(3), 1, -1),
                                  (1, i32(3), i32(3), 1, 1 << 31)):
        assert size(n_cam, hs, ws, nv, nt) == -1, (n_cam, nv, nt)
    assert lib.sfm_mesh_render_workspace_bytes(1, hp(i32(3)), hp(i32(3)), 1, 1, None) == -1
    assert lib.sfm_mesh_render(None, 0, None, None, None, 0, None, 0, None, 0, 1, None, None, None, 0, 0, 0, None, None, None, None, None, 0) == -1
