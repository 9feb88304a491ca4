"""The exposure compensation without a device: the two restatements of the sample and of the tables of
tests/mesh_exposure_reference.py against each other, the solve on hand-built tables and against the package's, the rule and
plan headers built for the host (bit for bit against NumPy, and under the sanitizers as a stand-alone program), the argument
checks, and what the rule is worth on the gained sphere."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_color_reference as cr
import mesh_exposure_reference as er
from test_mesh_color_reference import MIXED_SIZES, coloured_sphere

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "mesh_exposure_check.cpp")


def scene_args(s):
    """What `er.sample` takes of a `cr.Scene`."""
    return (s.vertices, s.normals, s.proj, s.centres, s.depth, s.keep, s.images, s.tol, s.min_cos)


def assert_same(got, want, what=""):
    for name, g, w in zip(("seen", "samples", "overlap", "sums"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())


# ------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("channels", [1, 3])
def test_the_two_restatements_agree(channels):
    """200 random vertices, 5 views of mixed sizes, with and without keep: every byte of seen and samples, every entry of
    the tables; and the diagonal of overlap is what single-view `colors` counts."""
    for seed, with_keep in ((11, True), (12, False)):
        s = cr.random_scene(seed + channels, 200, MIXED_SIZES, channels, with_keep)
        seen, q = er.sample(*scene_args(s), channels=channels)
        assert_same(er.sample_loops(*scene_args(s), channels=channels), (seen, q), (seed, channels))
        assert seen.shape == (5, 200) and q.shape == (5, channels, 200) and set(np.unique(seen)) == {0, 1}
        assert q.transpose(0, 2, 1)[seen == 0].max() == 0
        overlap, sums = er.tables(seen, q)
        assert_same((seen, q) + er.tables_loops(seen, q), (seen, q, overlap, sums), (seed, channels))
        assert np.array_equal(overlap, overlap.T) and (np.triu(overlap, 1) > 0).sum() >= 3 and overlap[3].max() == 0       # the view without a pixel
        for v in range(5):
            one = cr.colors(s.vertices, s.normals, s.proj[v:v + 1], s.centres[v:v + 1], s.depth[v:v + 1], None if s.keep is None else s.keep[v:v + 1],
                            s.images[v:v + 1], s.tol, s.min_cos, 0, channels)
            assert overlap[v, v] == (one[1] > 0).sum() and np.array_equal(seen[v], one[1])
            # a single view's colour is its sample, up to the division of wgt * s by wgt before the rounding
            assert np.abs(one[0].reshape(200, channels).T.astype(int) - q[v].astype(int)).max() <= 1


def test_hand_cases_and_many_views():
    names = 0
    for name, s, col, n_views, best in cr.hand_cases():
        seen, q = er.sample(*scene_args(s))
        assert_same(er.sample_loops(*scene_args(s)), (seen, q), name)
        assert np.array_equal(seen.sum(axis=0), n_views), name
        names += 1
    assert names == 13
    for channels in (1, 3):
        s, col, n_views, best = cr.merged_hand_cases(channels)
        seen, q = er.sample(*scene_args(s))
        assert_same(er.sample_loops(*scene_args(s)), (seen, q), ("merged", channels))
        assert np.array_equal(seen.sum(axis=0), n_views)
        assert_same((seen, q) + er.tables_loops(seen, q), (seen, q) + er.tables(seen, q), ("merged", channels))
    s = cr.many_views(300, 2)
    seen, q = er.sample(*scene_args(s))
    assert_same(er.sample_loops(*scene_args(s)), (seen, q), "300 views")
    overlap, sums = er.tables(seen, q)
    assert seen.all() and (overlap == 2).all() and np.array_equal(sums[:, :, 0], np.repeat(q[:, 0, :].sum(axis=1, dtype=np.int64)[:, None], 300, axis=1))
    s = cr.random_scene(3, 10, [], 3)
    for fn in (er.sample, er.sample_loops):
        seen, q = fn(*scene_args(s), channels=3)
        assert seen.shape == (0, 10) and q.shape == (0, 3, 10)
    assert er.tables(seen, q)[0].shape == (0, 0)


# ------------------------------------------------------------------------------------------- the solve
def pair_tables(n_common, a, b, extra=0):
    """Two views that share n_common vertices, view 0 holding a and view 1 holding b there (per channel), and `extra` more
    views that share nothing."""
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    n = 2 + extra
    overlap, sums = np.zeros((n, n), np.int64), np.zeros((n, n, len(a)), np.int64)
    overlap[:2, :2] = n_common
    sums[0, :2], sums[1, :2] = n_common * a, n_common * b
    for v in range(2, n):
        overlap[v, v], sums[v, v] = 50, 50 * 90
    return overlap, sums


def test_solve_on_hand_built_tables():
    from sfm_amd import solve_gains
    for solve in (er.solve_gains, solve_gains):
        # b = 2 a: the ratio of the gains approaches 2 as the prior loosens
        ratios = []
        for sigma_g in (0.1, 1.0, 10.0, 1000.0):
            g = solve(*pair_tables(400, 60, 120), 10.0, sigma_g, 1)
            assert g.shape == (2, 1) and (g > 0).all()
            ratios.append(g[0, 0] / g[1, 0])
        assert all(x < y for x, y in zip(ratios, ratios[1:])) and ratios[0] < 1.7 and abs(ratios[-1] - 2.0) < 1e-4, ratios
        # an isolated view gets exactly 1, and so does every view when min_overlap rules the only pair out
        g = solve(*pair_tables(400, [60, 80, 100], [120, 40, 100], extra=2), 10.0, 1.0, 1)
        assert g.shape == (4, 3) and (g[2:] == 1.0).all() and g[0, 0] > 1 > g[1, 0] and g[0, 1] < 1 < g[1, 1]
        assert abs(g[0, 2] - g[1, 2]) < 1e-12 and abs(g[0, 2] - 1.0) < 1e-12
        assert (solve(*pair_tables(400, 60, 120), 10.0, 1.0, 401) == 1.0).all()
        assert (solve(*pair_tables(400, 60, 120), 10.0, 1.0, 400) != 1.0).all()
        assert solve(np.zeros((0, 0), np.int64), np.zeros((0, 0, 3), np.int64), 10.0, 1.0, 1).shape == (0, 3)
        # identical images: five views that all hold the same values where they meet
        rng = np.random.default_rng(5)
        seen = (rng.random((5, 600)) < 0.6).astype(np.uint8)
        q = np.where(seen[:, None, :] != 0, rng.integers(0, 256, (1, 3, 600)), 0).astype(np.uint8)
        g = solve(*er.tables(seen, q), 10.0, 1.0, 1)
        assert np.abs(g - g[0]).max() < 1e-12 and np.abs(g - 1.0).max() < 1e-12
    # the package's solve against the restatement on random tables, with pairs below min_overlap and an isolated view
    seen[4] = 0
    seen[4, :3] = 1
    q = np.where(seen[:, None, :] != 0, rng.integers(0, 256, (5, 3, 600)), 0).astype(np.uint8)
    for min_overlap in (1, 4, 200):
        overlap, sums = er.tables(seen, q)
        assert np.abs(solve_gains(overlap, sums, 10.0, 1.0, min_overlap) - er.solve_gains(overlap, sums, 10.0, 1.0, min_overlap)).max() < 1e-12


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
    """The scene through the host build of the rule and of the gram kernel's arithmetic: (seen, samples, overlap, sums)."""
    ch = s.channels if channels is None else channels
    nv, n_ref = len(s.vertices), len(s.depth)
    fin, fout = tmp_path / "scene.in", tmp_path / "scene.out"
    with open(fin, "wb") as f:
        f.write(np.array([n_ref, ch, nv, s.keep is not None, 0], np.int64).tobytes())
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
    a, b = n_ref * nv, n_ref * nv * (1 + ch)
    assert len(raw) == b + 8 * n_ref * n_ref * (1 + ch)
    tables = raw[b:].view(np.int64)
    return (raw[:a].reshape(n_ref, nv), raw[a:b].reshape(n_ref, ch, nv), tables[:n_ref * n_ref].reshape(n_ref, n_ref),
            tables[n_ref * n_ref:].reshape(n_ref, n_ref, ch))


def reference(s, channels=None):
    seen, q = er.sample(*scene_args(s), channels=s.channels if channels is None else channels)
    return (seen, q) + er.tables(seen, q)


def boundary_records():
    """Samples and products that land on .5 and next to it; gains 0, 1, 0.5, 1.5 and random ones; every byte value."""
    rng = np.random.default_rng(17)
    half = np.arange(0, 256) + 0.5
    s = np.concatenate([rng.uniform(0, 255, 20000), half[:-1], np.nextafter(half[:-1], 0), np.nextafter(half[:-1], 300), np.arange(256.0)])
    values = np.tile(np.arange(256, dtype=np.uint8), 60)
    g = np.concatenate([np.repeat([0.0, 1.0, 0.5, 1.5, 0.25, 2.5, 1e300, 5e-324], 256), rng.uniform(0, 3, len(values) - 8 * 256)])
    # gains that put an odd value on .5 after the product: (k + 0.5) / value, the product is rounded before the sum
    odd = rng.integers(1, 256, 4000).astype(np.uint8)
    values = np.concatenate([values, odd])
    g = np.concatenate([g, (rng.integers(0, 255, 4000) + 0.5) / odd])
    word = lambda n: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    seen4 = np.concatenate([word(4000) & np.uint32(0x01010101), word(4000),
                            np.array([0, 0x01010101, 0x80808080, 0x7F7F7F7F, 0xFFFFFFFF, 0x00FF0001, 0x01000080], np.uint32)]).astype(np.uint32)
    q4 = rng.integers(0, 1 << 32, len(seen4), dtype=np.uint64).astype(np.uint32)
    q4[-7:] = [0x7F808180, 0xFF00FF00, 0x7F7F8080, 0x80807F7F, 0x00000000, 0xFFFFFFFF, 0x01FE7F80]
    return s, g, values, seen4, q4


def check_rule(exe, tmp_path, n_vertices):
    for channels in (1, 3):
        for seed, with_keep in ((21, True), (22, False)):
            s = cr.random_scene(seed, n_vertices, MIXED_SIZES, channels, with_keep)
            want = reference(s)
            assert (want[0].sum(axis=0) >= 2).mean() > 0.2
            assert_same(run_scene(exe, tmp_path, s), want, ("random", channels, with_keep))
        s = cr.merged_hand_cases(channels)[0]
        assert_same(run_scene(exe, tmp_path, s), reference(s), ("hand cases", channels))
    s = cr.many_views(300, 3)
    assert_same(run_scene(exe, tmp_path, s), reference(s), "300 views")
    for s in (cr.random_scene(4, 0, MIXED_SIZES, 3), cr.random_scene(4, 9, [], 1)):          # no vertex; no view
        assert_same(run_scene(exe, tmp_path, s), reference(s), "empty")
    # the records: quantise, gain and the two operand words
    s, g, values, seen4, q4 = boundary_records()
    fin, fout = tmp_path / "rule.in", tmp_path / "rule.out"
    with open(fin, "wb") as f:
        f.write(np.array([len(s), len(g), len(seen4)], np.int64).tobytes())
        for a in (s, g, values, seen4, q4):
            f.write(np.ascontiguousarray(a).tobytes())
    run = subprocess.run([exe, "rule", str(fin), str(fout)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    raw = np.fromfile(fout, dtype=np.uint8)
    assert len(raw) == len(s) + len(g) + 8 * len(seen4)
    r = np.floor(s + 0.5)
    assert np.array_equal(raw[:len(s)], np.where(r < 255.0, r, 255.0).astype(np.uint8))
    got = raw[len(s):len(s) + len(g)]
    want = np.array([er.apply_gain(v, k) for v, k in zip(values[:8 * 256:37], g[:8 * 256:37])], np.uint8)
    assert np.array_equal(got[:8 * 256:37], want)
    p = values.astype(np.float64) * g
    r = np.floor(p + 0.5)
    assert np.array_equal(got, np.where(r < 255.0, r, 255.0).astype(np.uint8))
    assert (np.abs(p[-4000:] - np.floor(p[-4000:]) - 0.5) < 1e-9).all()                    # those products do sit at .5
    words = raw[len(s) + len(g):].view(np.uint32)
    sb, qb = seen4.view(np.uint8), q4.view(np.uint8)
    assert np.array_equal(words[:len(seen4)].view(np.uint8), (sb != 0).astype(np.uint8))
    assert np.array_equal(words[len(seen4):].view(np.int8), np.where(sb != 0, qb.astype(np.int16) - 128, 0).astype(np.int8))


def test_rule_header_equals_numpy_bit_for_bit(tmp_path):
    exe = build_check(tmp_path, ["-O2"], "mesh_exposure_check")
    check_rule(exe, tmp_path, 9000)                                # more than two chunks of the vertex range
    (proj, depth, origin, voxel, shape, trunc, centres, images), m, _ = coloured_sphere()
    s = cr.Scene(proj, centres, depth, None, images, m.vertices, m.normals, trunc, 0.35, 0)
    assert_same(run_scene(exe, tmp_path, s), reference(s), "coloured sphere")


def test_rule_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone: every branch of the argument checks,
    the tiles and chunks, the windows of the gain pass; then the rule on the random scenes, the hand cases and the records,
    where the program itself checks every index it reads through."""
    exe = build_check(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                 "-fno-omit-frame-pointer"], "mesh_exposure_check_san")
    run = subprocess.run([exe, "plan"], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])
    check_rule(exe, tmp_path, 1500)


# ------------------------------------------------------------------------------------------- argument checks, no device
def test_argument_checks_without_gpu():
    import inspect
    import sfm_amd
    from sfm_amd import depth as dm
    from sfm_amd import exposure as ex
    from sfm_amd import mesh as mm
    for name in ("ExposureGains", "apply_gains", "check_exposure_arguments", "mesh_exposure_tables", "solve_gains"):
        assert getattr(sfm_amd, name) is getattr(ex, name)
    assert [p.default for p in list(inspect.signature(mm.Mesh.exposure).parameters.values())[2:]] == [None, None, 0.35, 10.0, 1.0, 1]
    assert [p.default for p in list(inspect.signature(ex.solve_gains).parameters.values())[2:]] == [10.0, 1.0, 1]
    nan, inf = float("nan"), float("inf")
    ex.check_exposure_arguments(0.1, 0.35)
    ex.check_exposure_arguments(0.0, 1.0, 5, 2, 3, 1024)
    for kw in (dict(tol=-1.0), dict(tol=nan), dict(tol="x"), dict(min_cos=0.0), dict(min_cos=1.5), dict(min_cos=nan), dict(sigma_n=0.0),
               dict(sigma_n=-1.0), dict(sigma_n=nan), dict(sigma_n=inf), dict(sigma_n=None), dict(sigma_g=0), dict(sigma_g=inf), dict(sigma_g="1"),
               dict(min_overlap=0), dict(min_overlap=1.5), dict(min_overlap=True), dict(n_views=1025)):
        with pytest.raises(ValueError):
            ex.check_exposure_arguments(**dict(dict(tol=0.1, min_cos=0.35), **kw))
    assert ex.check_gains([[1, 2, 3]], 1, 3).dtype == np.float64 and ex.check_gains([0.5, 0.0], 2, 1).shape == (2, 1)
    for bad, n, c in (([[1, 2]], 1, 3), ([1.0], 2, 1), ([[-0.1]], 1, 1), ([[nan]], 1, 1), ([[inf]], 1, 1), ([1.0, 2.0, 3.0], 3, 3)):
        with pytest.raises(ValueError):
            ex.check_gains(bad, n, c)
    ov, su = np.ones((2, 2), np.int64), np.ones((2, 2, 3), np.int64)
    for bad in (dict(overlap=np.ones((2, 3), np.int64)), dict(sums=np.ones((2, 2), np.int64)), dict(sums=np.ones((2, 2, 2), np.int64)),
                dict(overlap=np.ones((2, 2))), dict(sums=np.ones((3, 3, 3), np.int64)), dict(sigma_n=0.0), dict(sigma_g=nan), dict(min_overlap=0)):
        with pytest.raises(ValueError):
            ex.solve_gains(**dict(dict(overlap=ov, sums=su), **bad))
    # Mesh.exposure: what colors() refuses, before the device
    gray, bgr = np.zeros((2, 3), np.uint8), np.zeros((2, 3, 3), np.uint8)
    maps = dm.DepthMaps({"refs": [1], "imgs": [gray, gray], "radius": 2, "src_ptr": np.array([0, 0])})
    vol = mm.TsdfVolume(None, None, np.zeros(3), 0.1, (4, 4, 4))
    mesh = mm.Mesh({}, 0, 0, vol)
    with pytest.raises(ValueError, match="integrated from depth maps"):
        mesh.exposure([gray, gray])
    with pytest.raises(ValueError, match="filter"):
        mesh.exposure([gray, gray], maps)
    maps.keep = [np.ones((2, 3), np.uint8)]
    from sfm_amd._views import ViewSet                            # what DepthMaps.tsdf() leaves in the volume, nothing on a device
    vol.views = ViewSet(np.array([2, 2], np.int32), np.array([3, 3], np.int32), np.array([1], np.int32), np.zeros((1, 12)), np.zeros((1, 3)),
                        None, None, maps)
    for images, kw in (([gray], {}), ([gray, gray, gray], {}), ([gray, np.zeros((3, 2), np.uint8)], {}), ([gray, gray.astype(np.float32)], {}),
                       ([gray, gray], dict(tol=-1.0)), ([gray, gray], dict(min_cos=0.0)), ([gray, gray], dict(sigma_n=0.0)),
                       ([gray, gray], dict(sigma_g=nan)), ([gray, gray], dict(min_overlap=0))):
        with pytest.raises(ValueError):
            mesh.exposure(images, **kw)
    with pytest.raises(ValueError, match="tol"):
        mm.Mesh({}, 0, 0).exposure([gray, gray], maps)
    # the functions on arrays
    V, N = np.zeros((4, 3)), np.zeros((4, 3), np.float32)
    good = dict(vertices=V, normals=N, proj=np.zeros((1, 12)), centres=np.zeros((1, 3)), depth=[np.zeros((2, 3), np.float32)], keep=None,
                images=[gray], tol=0.1)
    for bad in (dict(vertices=np.zeros((4, 2))), dict(normals=np.zeros((3, 3), np.float32)), dict(proj=np.zeros((2, 12))), dict(centres=np.zeros((1, 2))),
                dict(depth=[np.zeros(6, np.float32)]), dict(keep=[np.zeros((3, 2), np.uint8)]), dict(images=[]), dict(images=[bgr[:1]]),
                dict(tol=-0.1), dict(min_cos=0), dict(depth=[np.zeros((1, 1), np.float32)] * 1025, proj=np.zeros((1025, 12)), centres=np.zeros((1025, 3)))):
        with pytest.raises(ValueError):
            ex.mesh_exposure_tables(**dict(good, **bad))
    for images, gains in (([gray, bgr], np.ones((2, 1))), ([gray], np.ones((2, 1))), ([bgr], np.ones((1, 1))), ([gray], [[-1.0]]), ([gray], [[nan]]),
                          ([gray.astype(np.int16)], [[1.0]])):
        with pytest.raises(ValueError):
            ex.apply_gains(images, gains)
    # what an ExposureGains does on the host
    seen = np.array([[1, 1, 0, 1], [1, 0, 0, 1], [0, 0, 0, 1]], np.uint8)
    q = np.array([[[10, 20, 0, 40]], [[13, 0, 0, 35]], [[0, 0, 0, 60]]], np.uint8)
    assert np.array_equal(ex.sample_spread(seen, q), np.array([[3.0], [nan], [nan], [25.0]]), equal_nan=True)
    assert np.array_equal(er.spread(seen, q), ex.sample_spread(seen, q), equal_nan=True)
    e = ex.ExposureGains({}, np.array([[0.5], [2.0]]), None, None, 4, 1, [2, 0], 3)
    assert np.array_equal(e.image_gains(), [[2.0], [1.0], [0.5]])
    with pytest.raises(ValueError, match="one array per image"):
        e.apply([gray])
    assert np.allclose(ex.centres_from_projections(cr.camera((1, 2, 3), 5, 3)[0][None]), [[1, 2, 3]], atol=1e-12)


def test_c_entry_points_reject_bad_calls_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    need = ctypes.c_int64(-1)
    assert lib.sfm_mesh_exposure_workspace_bytes(36, 3, 100000, ctypes.byref(need)) == 0 and need.value >= 37 * 16
    assert lib.sfm_mesh_exposure_workspace_bytes(0, 1, 0, ctypes.byref(need)) == 0 and need.value > 0
    for bad in ((-1, 3, 5), (1025, 3, 5), (2, 2, 5), (2, 3, -1), (2, 3, 1 << 31)):
        assert lib.sfm_mesh_exposure_workspace_bytes(*bad, ctypes.byref(need)) != 0, bad
    assert lib.sfm_mesh_exposure_workspace_bytes(3, 3, 5, None) != 0
    out = (ctypes.c_int32 * 4)()
    assert lib.sfm_mesh_exposure_plan(36, 3, 106866, out) == 0
    tile_i, tile_j, chunk, groups = list(out)
    assert tile_i == tile_j == 32 and chunk >= 64 and chunk % 32 == 0 and 128 * chunk < 2 ** 31 and groups == 4 * -(-106866 // chunk)
    assert lib.sfm_mesh_exposure_plan(0, 1, 0, out) == 0 and out[3] == 0
    assert lib.sfm_mesh_exposure_plan(1025, 3, 5, out) != 0 and lib.sfm_mesh_exposure_plan(3, 2, 5, out) != 0 and lib.sfm_mesh_exposure_plan(3, 3, 5, None) != 0
    assert lib.sfm_mesh_exposure_sample(None, None, None, 0, 0, None, None, None, None, None, None, 3, 0, None, None, 0.1, 0.35, None, None, None, 0) != 0
    assert lib.sfm_mesh_exposure_gram(None, 0, 3, 0, None, None, None, None, None, 0) != 0
    assert lib.sfm_images_gain(None, None, None, 0, 3, None, None, None) != 0


# ------------------------------------------------------------------------------------------- what the rule is worth
# measured with the restatement on the gained sphere scene (the coloured sphere, 14 views of 64 x 64 x 3, the mesh of its
# integration with 7,006 vertices, tol = 3 voxels, min_cos 0.35, every image multiplied by its gain of `true_gains()` and
# rounded half up).  error: (median, p95, max) of |colour / s - texture at the radial foot point|, s the mean of g_est *
# g_true; spread: (median, p95) over vertices with at least 2 views and channels of the largest minus the smallest sample;
# agreement: (max - min) / mean of g_est * g_true per channel
MEASURED = {"as rendered": ((0.28, 1.11, 8.42), (2.0, 11.0)),
            "with the gains": ((9.95, 31.62, 64.20), (28.0, 91.0)),
            0.1: ((4.87, 12.05, 19.90), (11.0, 28.0), (0.292, 0.319, 0.350)),
            1.0: ((0.73, 2.20, 7.26), (2.0, 8.0), (0.0292, 0.0297, 0.0218))}
_WORTH = {}


def gained_sphere():
    """The gained scene on the restatement's mesh of the coloured sphere, made once."""
    if not _WORTH:
        proj, depth, origin, voxel, shape, trunc, centres, images, gained, g_true = er.gained_sphere_scene()
        (_, _, _, _, _, _, _, rendered), m, _ = coloured_sphere()
        assert all(np.array_equal(a, b) for a, b in zip(images, rendered))
        _WORTH["scene"] = (m.vertices, m.normals, proj, centres, depth, trunc, images, gained, g_true)
    return _WORTH["scene"]


def assert_worth(rows, what=""):
    """The assertions of the worth table on rows = {"as rendered", "with the gains", 0.1, 1.0}, each a dict with `error` and
    `spread`, the compensated ones with `agreement` too."""
    plain, gained, tight, loose = rows["as rendered"], rows["with the gains"], rows[0.1], rows[1.0]
    for name, r in rows.items():
        print(f"{what}{name}: error median / p95 / max {r['error'][0]:.2f} / {r['error'][1]:.2f} / {r['error'][2]:.2f}, spread median / p95 "
              f"{r['spread'][0]:.1f} / {r['spread'][1]:.1f}" + (f", agreement {np.round(100 * r['agreement'], 2).tolist()} %" if "agreement" in r else ""))
    assert loose["error"][0] <= MEASURED[1.0][0][0] + 0.5
    assert loose["error"][0] <= gained["error"][0] / 5.0
    assert (loose["agreement"] <= np.array(MEASURED[1.0][2]) + 0.01).all()
    assert loose["spread"][1] <= plain["spread"][1] + 3.0
    assert tight["error"][0] > loose["error"][0] and tight["spread"][1] > loose["spread"][1] and (tight["agreement"] > loose["agreement"]).all()


def test_worth_on_the_gained_sphere():
    """Measured (the table of the README): as rendered 0.28 / 1.11 / 8.42 and spread 2 / 11; with the gains 9.95 / 31.62 / 64.20
    and 28 / 91; compensated with sigma_g 0.1: 4.87 / 12.05 / 19.90 and 11 / 28, the products g_est * g_true agreeing to
    29.2 / 31.9 / 35.0 % per channel; with sigma_g 1.0: 0.73 / 2.20 / 7.26 and 2 / 8, agreeing to 2.92 / 2.97 / 2.18 %.  The
    sample is quantised directly here, where a single-view `colors` divides wgt * s by wgt first: no printed digit differs
    from a table made that way.  Asserted: the compensated median error at most the measured value plus 0.5 grey level and at
    most a fifth of the uncompensated one; the agreement per channel at most the measured value plus one percentage point;
    the compensated spread's p95 at most the as-rendered p95 plus 3 grey levels; sigma_g 0.1 worse than 1.0 in error,
    spread and agreement."""
    V, N, proj, centres, depth, trunc, images, gained, g_true = gained_sphere()
    assert np.array_equal(g_true, [0.918, 0.735, 0.62, 0.608, 1.007, 1.056, 0.903, 0.965, 0.872, 1.068, 1.008, 0.601, 1.029, 0.617])
    assert max(int(a.max()) for a in images) <= 228 and len(V) == 7006                    # nothing saturates under a gain of at most 1.068
    rows = {}
    for name, imgs, s in (("as rendered", images, 1.0), ("with the gains", gained, float(g_true.mean()))):
        col, n_views, best = cr.colors(V, N, proj, centres, depth, None, imgs, trunc, 0.35, 0)
        rows[name] = dict(error=er.scaled_error(col, n_views, V, s), spread=er.spread_summary(*er.sample(V, N, proj, centres, depth, None, imgs, trunc, 0.35)))
    for sigma_g in (0.1, 1.0):
        rows[sigma_g] = er.worth(V, N, proj, centres, depth, trunc, images, gained, g_true, sigma_g)
    assert_worth(rows)
    for name, r in rows.items():                                   # the table as it is printed in the README
        assert np.allclose(r["error"], MEASURED[name][0], atol=0.006) and np.allclose(r["spread"], MEASURED[name][1], atol=0.3), (name, r)
    seen, q = er.sample(V, N, proj, centres, depth, None, gained, trunc, 0.35)
    overlap = er.tables(seen, q)[0]
    off = overlap[np.triu_indices(14, 1)]
    assert (off > 0).sum() == 60 and off[off > 0].min() == 9 and off.max() == 919
