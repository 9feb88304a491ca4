"""The render score without a GPU: the NumPy restatement of the rule (tests/render_score_reference.py) against its version in
plain loops, properties and hand cases, the host build of render_score_rule.h and render_score_plan.h bit for bit against NumPy
and under the sanitizers stand-alone, the argument checks of the Python layer and of the C entry points, and the worth of
the score on the textured sphere."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import render_score_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "render_score_check.cpp")
Q = 1 << 24


def one(case, window=7, rel_tol=0.02, fn=sr.score_view):
    return fn(*case.args(), window, rel_tol)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(sr.bits(a[2]), sr.bits(b[2]))


# ------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("window", [3, 5, 7])
def test_the_two_restatements_agree(channels, window):
    hits = np.zeros(sr.COLUMNS, np.int64)
    for k, (h, w, pattern, mask, with_depth) in enumerate([(9, 12, "random", False, True), (13, 8, "all", True, True), (7, 7, "all", False, False),
                                                           (10, 10, "checker", False, True), (12, 11, "middle", True, False), (2, 9, "all", False, True),
                                                           (0, 5, "all", False, True), (11, 14, "none", False, True)]):
        case = sr.random_case(100 * window + 10 * channels + k, h, w, channels, pattern, mask, with_depth, tile=(8, 8))
        a, b = one(case, window), one(case, window, fn=sr.score_view_loops)
        assert same(a, b), (k, a[0].tolist(), b[0].tolist())
        assert a[0][sr.N_PIXELS] == h * w and a[0][15] == 0 and (channels == 3 or (a[0][[3, 4, 6, 7]] == 0).all())
        hits += a[0] != 0
    assert (hits[[sr.N_COMPARED, sr.SAD, sr.SSE, sr.N_SSIM, sr.Q_SSIM, sr.N_BOTH, sr.N_AGREE, sr.Q_REL, sr.N_RENDER_ONLY, sr.N_VIEW_ONLY]] > 0).all()


@pytest.mark.parametrize("channels", [1, 3])
def test_identical_images(channels):
    """sad = sse = 0, every s exactly 1.0, q_ssim = n_ssim 2^24 and PSNR inf."""
    case = sr.random_case(3, 20, 23, channels, "middle", True, False)
    case.photo = case.color.copy()
    stats, err, ssim = one(case)
    assert stats[sr.N_COMPARED] > 100 and stats[sr.N_SSIM] > 10
    assert (stats[sr.SAD:sr.SAD + 6] == 0).all() and not err.any()
    assert (ssim[~np.isnan(ssim)] == np.float32(1.0)).all() and int((~np.isnan(ssim)).sum()) == stats[sr.N_SSIM]
    assert stats[sr.Q_SSIM] == stats[sr.N_SSIM] * Q
    f = sr.figures(stats, channels)
    assert f["psnr"] == math.inf and f["ssim"] == 1.0 and f["mae"] == [0.0] * channels


@pytest.mark.parametrize("channels", [1, 3])
def test_swapping_render_and_photo_changes_no_statistic(channels):
    case = sr.random_case(5, 18, 21, channels, "random", True, True)
    a = one(case, 3)
    case.color, case.photo = case.photo, case.color
    b = one(case, 3)
    assert same(a, b) and a[0][sr.N_SSIM] > 0 and a[0][sr.Q_SSIM] != a[0][sr.N_SSIM] * Q


def flat_case(h, w, x, y, channels=1):
    shape = (h, w) if channels == 1 else (h, w, 3)
    return sr.Case(np.full(shape, x, np.uint8), np.zeros((h, w), np.int32), np.ones((h, w), np.float32), np.full(shape, y, np.uint8))


@pytest.mark.parametrize("fn", [sr.score_view, sr.score_view_loops])
def test_hand_cases(fn):
    # a constant render x against a constant photograph y: no variance, so s = (2 x y + C1) / (x^2 + y^2 + C1) with C1 = 6.5025
    # (the factors n^2 cancel only in exact arithmetic: the rule's own value is what is asserted, the formula to 1e-15)
    x, y, W = 100, 90, 7
    stats, err, ssim = fn(*flat_case(9, 10, x, y).args(), W, 0.02)
    n = W * W
    c1, c2 = float(n * n) * 6.5025, float(n * n) * 58.5225
    s = ((float(2 * n * x * n * y) + c1) * (0.0 + c2)) / ((float((n * x) ** 2 + (n * y) ** 2) + c1) * (0.0 + c2))
    assert abs(s - (2 * x * y + 6.5025) / (x * x + y * y + 6.5025)) < 1e-15 and 0.99 < s < 1.0
    assert stats.tolist() == [90, 90, 900, 0, 0, 9000, 0, 0, 12, 12 * math.floor(s * Q + 0.5), 0, 0, 0, 0, 0, 0]
    assert (err == 10).all() and np.isnan(ssim[:3]).all() and np.isnan(ssim[:, :3]).all() and np.isnan(ssim[6:]).all() and np.isnan(ssim[:, 7:]).all()
    assert (ssim[3:6, 3:7] == np.float32(s)).all()
    assert sr.bits(ssim)[0, 0] == 0x7FC00000
    f = sr.figures(stats, 1)
    assert f["mae"] == [10.0] and f["mse"] == [100.0] and f["psnr"] == 10.0 * math.log10(65025.0 * 90 / 9000) and abs(f["ssim"] - s) < 2.0 ** -24

    # a window cut by one uncovered pixel: the W^2 windows that hold it are gone, its own error is not counted
    case = flat_case(11, 12, 100, 90)
    case.triangle[5, 6] = -1
    stats, err, ssim = fn(*case.args(), 3, 0.02)
    assert stats[sr.N_COMPARED] == 131 and stats[sr.SAD] == 1310 and err[5, 6] == 0 and stats[sr.N_SSIM] == 9 * 10 - 9
    assert np.isnan(ssim[4:7, 5:8]).all() and not np.isnan(ssim[3, 5:8]).any() and not np.isnan(ssim[4:7, 4]).any()
    # the same pixel masked out instead
    case.triangle[5, 6] = 0
    case.mask = np.full((11, 12), 7, np.uint8)
    case.mask[5, 6] = 0
    masked = fn(*case.args(), 3, 0.02)
    assert np.array_equal(masked[0], stats) and np.array_equal(sr.bits(masked[2]), sr.bits(ssim))

    # an image narrower than the window has no window, and neither has one that is lower
    for h, w in ((9, 6), (6, 9), (1, 1)):
        stats, err, ssim = fn(*flat_case(h, w, 3, 250, 3).args(), 7, 0.02)
        assert stats[sr.N_SSIM] == 0 and stats[sr.Q_SSIM] == 0 and np.isnan(ssim).all() and stats[sr.N_COMPARED] == h * w
        assert stats[sr.SAD:sr.SAD + 3].tolist() == [247 * h * w] * 3 and math.isnan(sr.figures(stats, 3)["ssim"])
    # nothing compared: PSNR is NaN
    case = flat_case(8, 8, 1, 2)
    case.triangle[:] = -1
    assert math.isnan(sr.figures(fn(*case.args(), 7, 0.02)[0], 1)["psnr"])


@pytest.mark.parametrize("fn", [sr.score_view, sr.score_view_loops])
def test_depth_hand_cases(fn):
    """At the threshold, with NaN, with keep = 0 and with dv <= 0."""
    dv = np.array([[2.0, 2.0, 2.0, 2.0, np.nan, 2.0, 0.0, 0.0, -1.0, 2.0, np.inf, 1.0]], np.float32)
    tol = 0.25                                                     # exact in binary: 0.25 * 2.0 = 0.5
    dr = np.array([[2.5, np.nextafter(np.float32(2.5), np.float32(3)), 1.5, 2.0, 2.0, 2.0, 0.0, 1.0, -1.0, np.nan, 2.0, 9.0]], np.float32)
    keep = np.array([[1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 255]], np.uint8)
    tri = np.zeros((1, 12), np.int32)
    grey = np.zeros((1, 12), np.uint8)
    stats = fn(grey, tri, dr, grey, None, dv, keep, 3, tol)[0]
    # seen: all but the NaN, the keep = 0 and the inf -> 9 pixels with both depths, 3 that only the render has
    assert stats[sr.N_BOTH] == 9 and stats[sr.N_RENDER_ONLY] == 3 and stats[sr.N_VIEW_ONLY] == 0
    # agree: 2.5 (at the threshold), 1.5 (at it from below), 2.0, dr = dv = 0; not: one ulp past it, dv = 0 with r = 1, dv = -1 with
    # r = 0 (0 <= -0.25 is false), a NaN render depth, 9 against 1
    assert stats[sr.N_AGREE] == 4
    ratio = lambda a, b: math.floor(min(abs(np.float64(np.float32(a)) - b) / b, 1.0) * Q + 0.5)
    want = ratio(2.5, 2.0) + ratio(float(dr[0, 1]), 2.0) + ratio(1.5, 2.0) + 0 + 0 + Q + 0 + 0 + Q
    #      the three near the threshold            dr=dv   0/0   1/0  r=0,dv<0  NaN  capped
    assert stats[sr.Q_REL] == want
    # a pixel the mesh does not cover, seen by the view
    tri[0, 3] = -1
    stats = fn(grey, tri, dr, grey, None, dv, keep, 3, tol)[0]
    assert stats[sr.N_BOTH] == 8 and stats[sr.N_VIEW_ONLY] == 1 and stats[sr.N_AGREE] == 3 and stats[sr.N_COMPARED] == 11
    # without the view's depth every depth column is 0
    assert (fn(grey, tri, dr, grey, None, None, None, 3, tol)[0][sr.N_BOTH:] == 0).all()
    f = sr.figures(stats, 1)
    assert f["depth_agree"] == 3 / 8 and f["depth_rel"] == stats[sr.Q_REL] / (Q * 8)


def test_pooled_figures_come_from_the_summed_integers():
    a, b = one(sr.random_case(1, 12, 40, 3, "all"))[0], one(sr.random_case(2, 30, 9, 3, "random"))[0]
    pooled = sr.figures(np.stack([a, b]), 3)
    assert pooled["n_compared"] == a[1] + b[1] and pooled["mae"][1] == (a[3] + b[3]) / (a[1] + b[1])
    assert pooled["psnr"] == 10.0 * math.log10(65025.0 * (a[1] + b[1]) * 3 / (a[5:8].sum() + b[5:8].sum()))
    assert pooled["ssim"] != (sr.figures(a, 3)["ssim"] + sr.figures(b, 3)["ssim"]) / 2


# ------------------------------------------------------------------------------------------- the headers on the host
def build_check(tmp_path, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"), CHECK_SRC, "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return str(exe)


def run_cases(exe, tmp_path, cases, window, rel_tol, want_maps=True):
    """The cases as one batch through the host build: a `Score`."""
    ch = 3 if cases[0].color.ndim == 3 else 1
    has_mask, has_depth = cases[0].mask is not None, cases[0].view_depth is not None
    fin, fout = tmp_path / "score.in", tmp_path / "score.out"
    cat = lambda name, dt: np.concatenate([np.ascontiguousarray(getattr(c, name), dtype=dt).reshape(-1) for c in cases]).tobytes()
    with open(fin, "wb") as f:
        f.write(np.array([len(cases), ch, window, has_mask, has_depth, want_maps], np.int64).tobytes())
        f.write(np.array([rel_tol], np.float64).tobytes())
        f.write(np.array([c.triangle.shape[0] for c in cases], np.int32).tobytes())
        f.write(np.array([c.triangle.shape[1] for c in cases], np.int32).tobytes())
        f.write(cat("color", np.uint8) + cat("triangle", np.int32) + cat("depth", np.float32) + cat("photo", np.uint8))
        if has_mask:
            f.write(cat("mask", np.uint8))
        if has_depth:
            f.write(cat("view_depth", np.float32) + cat("view_keep", np.uint8))
    run = subprocess.run([exe, "score", str(fin), str(fout)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    raw = open(fout, "rb").read()
    n = sum(c.triangle.size for c in cases)
    assert len(raw) == len(cases) * 128 + (n * ch + n * 4 if want_maps else 0)
    stats = np.frombuffer(raw[:len(cases) * 128], np.int64).reshape(-1, 16)
    if not want_maps:
        return sr.Score(stats, [], [], ch)
    err, ssim = np.frombuffer(raw[len(cases) * 128:len(cases) * 128 + n * ch], np.uint8), np.frombuffer(raw[len(cases) * 128 + n * ch:], np.float32)
    errs, maps, o = [], [], 0
    for c in cases:
        h, w = c.triangle.shape
        errs.append(err[o * ch:(o + h * w) * ch].reshape(c.color.shape))
        maps.append(ssim[o:o + h * w].reshape(h, w))
        o += h * w
    return sr.Score(stats, errs, maps, ch)


def reference_of(cases, window, rel_tol):
    out = [sr.score_view(*c.args(), window, rel_tol) for c in cases]
    return sr.Score(np.array([o[0] for o in out], np.int64).reshape(-1, 16), [o[1] for o in out], [o[2] for o in out], 3 if cases[0].color.ndim == 3 else 1)


def check_cases(exe, tmp_path, sizes):
    seed = 0
    for window in (3, 7, 11):
        for channels in (1, 3):
            for mask, with_depth in ((False, True), (True, False)):
                # the first, largest view keeps windows at every size of the window; the others go through the patterns
                cases = [sr.random_case(7000 + 10 * seed + k, h, w, channels, ("all", "middle", "corner")[seed % 3] if k == 0 else
                                        sr.PATTERNS[(seed + k) % len(sr.PATTERNS)], mask, with_depth) for k, (h, w) in enumerate(sizes)]
                seed += 1
                want = reference_of(cases, window, 0.02)
                sr.assert_same(run_cases(exe, tmp_path, cases, window, 0.02), want, (window, channels, mask, with_depth))
                assert np.array_equal(run_cases(exe, tmp_path, cases, window, 0.02, want_maps=False).stats, want.stats)
                assert want.stats[:, sr.N_SSIM].sum() > 0 and (want.stats[:, sr.N_BOTH].sum() > 0) == with_depth


def test_rule_header_equals_numpy_bit_for_bit_whatever_the_contraction(tmp_path):
    """Built with -ffp-contract=off and with the compiler's default (fast): the rule has no product that feeds a sum in
    floating point except v * 2^24 + 0.5, whose product is exact, so both builds give NumPy's bytes."""
    sizes = [(41, 70), (9, 33), (0, 4), (17, 11), (8, 32), (12, 5)]
    for flags, name in ((["-O2", "-ffp-contract=off"], "render_score_check"), (["-O2", "-ffp-contract=fast"], "render_score_check_fast")):
        check_cases(build_check(tmp_path, flags, name), tmp_path, sizes)


def test_rule_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone: the argument checks branch by branch, then
    the tiles, halos and workspace offsets over sizes 0, 1, W - 1, W, W + 1, tile - 1, tile, tile + 1 and 2 tile + 3 for every
    window and both channel counts - every pixel produced exactly once, no index outside its buffer - then the rule on cases."""
    exe = build_check(tmp_path, ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                 "-fno-omit-frame-pointer"], "render_score_check_san")
    run = subprocess.run([exe, "plan"], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])
    assert int(run.stdout.split()[1]) > 100000
    check_cases(exe, tmp_path, [(19, 67), (9, 33), (0, 4), (7, 7)])


# ------------------------------------------------------------------------------------------- argument checks, no device
def test_argument_checks_without_gpu(tmp_path):
    import inspect
    import sfm_amd
    from sfm_amd import mesh as mm
    assert sfm_amd.RenderScore is mm.RenderScore and sfm_amd.score_render is mm.score_render and sfm_amd.check_score_arguments is mm.check_score_arguments
    assert [p.default for p in list(inspect.signature(mm.MeshRender.compare).parameters.values())[2:]] == [None, None, 7, 0.02, True]
    assert [p.default for p in list(inspect.signature(mm.score_render).parameters.values())[4:]] == [None, None, None, 7, 0.02, 0]
    assert [p.default for p in list(inspect.signature(mm.Mesh.score).parameters.values())[2:4]] == [None, "auto"]
    assert mm.score_tile() == (32, 8) or all(v > 0 for v in mm.score_tile())
    check = mm.check_score_arguments
    hs, ws = [3, 0, 2], [5, 4, 2]
    grey = [np.zeros((h, w), np.uint8) for h, w in zip(hs, ws)]
    bgr = [np.zeros((h, w, 3), np.uint8) for h, w in zip(hs, ws)]
    photos, masks = check(hs, ws, 1, grey)
    assert photos.dtype == np.uint8 and photos.shape == (19,) and masks is None
    photos, masks = check(hs, ws, 3, bgr, grey, 11, 0.0)
    assert photos.shape == (57,) and masks.shape == (19,)
    assert check([], [], 1, [])[0].shape == (0,)
    for kw in (dict(channels=2), dict(window=6), dict(window=1), dict(window=13), dict(window=7.0), dict(window=True), dict(rel_tol=-0.1), dict(rel_tol=float("nan")),
               dict(rel_tol=float("inf")), dict(rel_tol="x"), dict(images=grey[:2]), dict(images=bgr), dict(images=[g.astype(np.float32) for g in grey]),
               dict(images=[grey[0], grey[1], np.zeros((2, 3), np.uint8)]), dict(masks=grey[:1]), dict(masks=bgr), dict(images=5), dict(heights=[3, 0, 40000])):
        args = dict(heights=hs, widths=ws, channels=1, images=grey, masks=None, window=7, rel_tol=0.02)
        args.update(kw)
        with pytest.raises(ValueError):
            check(**args)

    # a render and a score held on the host
    class Held:
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a

        def __getitem__(self, k):
            return Held(self.a[k])

    bare = mm.MeshRender({"triangle": Held(np.zeros(4, np.int32))}, [2], [2], 1, False)
    with pytest.raises(ValueError, match="colour"):
        bare.compare([np.zeros((2, 2), np.uint8)])
    with pytest.raises(ValueError, match="DepthMaps.tsdf"):
        mm.Mesh({}, 0, 4).score([np.zeros((2, 2), np.uint8)])
    for bad in (dict(color=[np.zeros((2, 2), np.float32)]), dict(photos=[np.zeros((2, 3), np.uint8)]), dict(view_keep=[np.ones((2, 2), np.uint8)]),
                dict(triangle=[np.zeros((3, 2), np.int32)]), dict(view_depth=[np.zeros((2, 3), np.float32)]), dict(window=4), dict(masks=[np.zeros((2, 2, 3), np.uint8)]),
                dict(color=[np.zeros((2, 2), np.uint8), np.zeros((2, 2, 3), np.uint8)])):
        args = dict(color=[np.zeros((2, 2), np.uint8)], triangle=[np.zeros((2, 2), np.int32)], depth=[np.ones((2, 2), np.float32)], photos=[np.zeros((2, 2), np.uint8)])
        args.update(bad)
        with pytest.raises(ValueError):
            mm.score_render(**args)

    from test_mesh_texture_reference import read_png
    cases = [sr.random_case(40 + k, h, w, 3, "random") for k, (h, w) in enumerate(((12, 15), (0, 3), (9, 10)))]
    want = reference_of(cases, 3, 0.02)
    state = {"stats": Held(want.stats.reshape(-1)), "abs_error": Held(np.concatenate([e.reshape(-1) for e in want.abs_error])),
             "ssim_map": Held(np.concatenate([m.reshape(-1) for m in want.ssim_map]))}
    score = mm.RenderScore(state, [12, 0, 9], [15, 3, 10], 3, 3, 0.02, True)
    sr.assert_same(score, want, "held")
    assert score.sizes == [(15, 12), (3, 0), (10, 9)] and score.mae.shape == (3, 3) and score.mse.shape == (3, 3) and score.psnr.shape == (3,)
    for v in (0, 2):
        f = sr.figures(want.stats[v], 3)
        assert score.n_compared[v] == f["n_compared"] and score.mae[v].tolist() == f["mae"] and score.mse[v].tolist() == f["mse"] and score.psnr[v] == f["psnr"]
        assert score.ssim[v] == f["ssim"] and score.n_ssim[v] == f["n_ssim"] and score.depth_both[v] == f["depth_both"] and score.depth_agree[v] == f["depth_agree"]
        assert score.depth_rel[v] == f["depth_rel"] and score.render_only[v] == f["render_only"] and score.view_only[v] == f["view_only"]
    assert score.n_compared[1] == 0 and np.isnan(score.psnr[1]) and np.isnan(score.ssim[1]) and np.isnan(score.mae[1]).all()
    assert score.pooled() == sr.figures(want.stats, 3)
    order = score.worst(3)
    assert sorted(order) == [0, 1, 2] and order[2] == 1 and score.ssim[order[0]] <= score.ssim[order[1]]
    assert score.worst(1, by="mae") == [int(np.nanargmax(score.mae.mean(axis=1)))] and score.worst(0) == [] and len(score.worst(5, by="depth_rel")) == 3
    with pytest.raises(ValueError):
        score.worst(by="colour")
    score.save_png(tmp_path / "error.png", camera=2)
    assert np.array_equal(read_png(tmp_path / "error.png"), want.abs_error[2][:, :, ::-1])
    score.save_png(tmp_path / "ssim.png", camera=0, what="ssim")
    png = read_png(tmp_path / "ssim.png")
    m = want.ssim_map[0].astype(np.float64)
    assert png.shape == (12, 15) and (png[np.isnan(m)] == 0).all() and np.isnan(m).any() and not np.isnan(m).all()
    assert np.array_equal(png[~np.isnan(m)], np.floor((m[~np.isnan(m)] + 1.0) * 127.5 + 0.5).astype(np.uint8))
    assert mm.ssim_to_gray(np.array([-1.0, 0.0, 1.0, np.nan], np.float32)).tolist() == [0, 128, 255, 0]
    with pytest.raises(ValueError):
        score.save_png(tmp_path / "x.png", what="depth")
    none = mm.RenderScore({"stats": Held(want.stats.reshape(-1))}, [12, 0, 9], [15, 3, 10], 3, 3, 0.02, False)
    assert none.abs_error is None and none.ssim_map is None
    with pytest.raises(ValueError, match="keep_maps"):
        none.save_png(tmp_path / "x.png")


def test_c_entry_points_reject_bad_calls_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    i32 = lambda *v: np.array(v, dtype=np.int32)
    hp = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    need = ctypes.c_int64(-1)
    size = lambda n, hs, ws: lib.sfm_render_score_workspace_bytes(n, hp(hs), hp(ws), ctypes.byref(need))
    assert size(2, i32(3, 4), i32(5, 0)) == 0 and need.value >= 3 * 16
    assert size(0, None, None) == 0 and need.value > 0
    assert size(36, i32(*[768] * 36), i32(*[1024] * 36)) == 0 and need.value < (1 << 16)
    for n, hs, ws in ((-1, i32(3), i32(3)), (65536, i32(3), i32(3)), (1, None, i32(3)), (1, i32(3), None), (1, i32(-1), i32(3)), (1, i32(3), i32(32769))):
        assert size(n, hs, ws) == -1, n
    assert lib.sfm_render_score_workspace_bytes(1, hp(i32(3)), hp(i32(3)), None) == -1
    tw, th = ctypes.c_int32(), ctypes.c_int32()
    assert lib.sfm_render_score_tile(ctypes.byref(tw), ctypes.byref(th)) == 0 and tw.value > 0 and th.value > 0
    assert lib.sfm_render_score_tile(None, ctypes.byref(th)) == -1 and lib.sfm_render_score_tile(ctypes.byref(tw), None) == -1
    assert lib.sfm_render_score(None, 0, None, None, 1, None, None, None, None, None, None, None, 7, 0.02, None, None, None, None, 0) == -1


# ------------------------------------------------------------------------------------------- worth
def test_worth_on_the_textured_sphere():
    """`textured_sphere_scene(128, 180, 24)` at texels 6 through the restatements of every stage, its 14 cameras, three channels,
    window 7, pooled over the views.  Measured: atlas MAE 12.233 grey levels, PSNR 18.364 dB, SSIM 0.9748; vertex colours
    16.510, 18.023, 0.9497; the render covers 6,979 to 7,090 pixels of a view whose own depth is finite on 6,756 to 6,836 - the
    mesh stands about one pixel outside the silhouette, and those pixels compare a surface colour with the background; of the
    pixels with both depths 91 to 94 % agree within 1 %.  Asserted: atlas MAE at most the measured value plus 0.5, atlas SSIM
    at least the measured value less 0.005, the atlas better than the vertex colours in MAE, PSNR and SSIM, and every view's
    render closer in SSIM to its own photograph than to the next view's."""
    r = sr.worth_of(*sr.sphere_renders(128, 180.0, 24.0, 6), sr.reference_score_fn)
    mean = lambda v: sum(v) / len(v)
    a, v = r["atlas"], r["vertex"]
    print(f"atlas MAE {mean(a['mae']):.3f} PSNR {a['psnr']:.3f} SSIM {a['ssim']:.4f}; vertex colours MAE {mean(v['mae']):.3f} PSNR {v['psnr']:.3f} "
          f"SSIM {v['ssim']:.4f}; covered {r['covered']}, finite {r['finite']}, within 1 % {r['agree'][0]:.4f} .. {r['agree'][1]:.4f}; "
          f"depth_rel {a['depth_rel']:.5f}, render only {a['render_only']}, view only {a['view_only']}; "
          f"own SSIM {min(r['own']):.4f} .. {max(r['own']):.4f}, next view's {min(r['next']):.4f} .. {max(r['next']):.4f}")
    sr.assert_worth(r)
