"""CPU tests of the feature stage's contract: the NumPy restatement of tests/features_reference.py against brute force and
hand-built cases, the host-only pattern functions of the library through ctypes, the planning header under the sanitizers,
the PNM reader / writer and the argument checks of the device entry points.  No GPU."""
import ctypes
import functools
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import features_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# SHA-256 of the 1,024 bytes of sfm_orb_default_pattern's table, generated once: a change of the generator is deliberate
DEFAULT_PATTERN_SHA256 = "847934b61f6ff7a2a427d52a182b601a54a7c31edf1e46c135d499ec591e9e74"


@functools.lru_cache(maxsize=None)
def default_tables():
    """(base [256,4] int8, rot [30,256,4] int8) from the library's host-only functions - never modified."""
    from sfm_amd import features
    base = features.default_pattern()
    rot = features.rotate_pattern(base)
    base.setflags(write=False)
    rot.setflags(write=False)
    return base, rot


# ------------------------------------------------------------------------------------------------------------ FAST
def test_score_formula_against_a_threshold_sweep_of_the_segment_test():
    """score = the largest threshold at which the published segment test still passes, pixel by pixel on a 40 x 40 scene."""
    img = fr.make_scene(40, 40, seed=7, noise=6)
    b = fr.fast_b(img)
    n_corners = 0
    for y in range(3, 37):
        for x in range(3, 37):
            passing = [t for t in range(0, 255) if fr.segment_test(img, y, x, t)]
            largest = max(passing) if passing else -1
            # the test passes at t iff b > t, so the largest passing threshold is b - 1 (b <= 0: it never passes)
            assert largest == (int(b[y, x]) - 1 if b[y, x] >= 1 else -1), (y, x)
            assert passing == list(range(0, largest + 1))
            n_corners += largest >= 20
    assert n_corners >= 10
    s = fr.fast_score(img, 20)
    assert (s[:3] == 0).all() and (s[-3:] == 0).all() and (s[:, :3] == 0).all() and (s[:, -3:] == 0).all()
    assert np.array_equal(s[3:-3, 3:-3] > 0, b[3:-3, 3:-3] > 20)
    assert np.array_equal(s[s > 0].astype(int), b[s > 0] - 1)


def ring(values, centre=100):
    img = np.full((7, 7), centre, dtype=np.uint8)
    for (dx, dy), v in zip(fr.CIRCLE, values):
        img[3 + dy, 3 + dx] = v
    return img


@pytest.mark.parametrize("sign", [1, -1])
def test_hand_built_arcs(sign):
    c = 100
    arc9 = [c + sign * 40] * 9 + [c] * 7
    arc8 = [c + sign * 40] * 8 + [c] * 8
    wrap = [c + sign * 40] * 4 + [c] * 7 + [c + sign * 40] * 5          # indices 11 .. 15, 0 .. 3: wraps 15 -> 0
    assert fr.fast_score(ring(arc9), 20)[3, 3] == 39
    assert fr.fast_score(ring(arc8), 20)[3, 3] == 0
    assert fr.fast_score(ring(wrap), 20)[3, 3] == 39
    assert fr.fast_score(ring(arc9), 39)[3, 3] == 39 and fr.fast_score(ring(arc9), 40)[3, 3] == 0
    uneven = [c + sign * (25 + k) for k in range(9)] + [c] * 7          # the weakest pixel of the arc decides
    assert fr.fast_score(ring(uneven), 20)[3, 3] == 24
    for start in range(16):
        rolled = np.roll(np.array(arc9), start).tolist()
        assert fr.fast_score(ring(rolled), 20)[3, 3] == 39
        assert fr.fast_score(ring(np.roll(np.array(arc8), start).tolist()), 20)[3, 3] == 0


def test_suppression_and_selection():
    s = np.zeros((9, 9), np.uint8)
    s[2, 2], s[2, 3] = 50, 50            # two equal adjacent maxima both go
    s[5, 5], s[5, 6] = 60, 59            # the larger stays
    s[0, 0] = 7                          # neighbours outside the image count as 0
    s[8, 4], s[7, 5] = 9, 9              # diagonal ties go too
    k = fr.suppress(s)
    assert sorted(zip(*np.nonzero(k))) == [(0, 0), (5, 5)] and k[5, 5] == 60 and k[0, 0] == 7
    kept = np.zeros((6, 6), np.uint8)
    kept[0, 1], kept[1, 0], kept[1, 4], kept[3, 3], kept[5, 5] = 30, 40, 30, 30, 20
    xy, sc = fr.select(kept, 0)
    assert xy.tolist() == [[1, 0], [0, 1], [4, 1], [3, 3], [5, 5]] and sc.tolist() == [30, 40, 30, 30, 20]
    xy, sc = fr.select(kept, 3)          # the cut score is 30: 40 stays, the first two 30s in row-major order stay
    assert xy.tolist() == [[1, 0], [0, 1], [4, 1]] and sc.tolist() == [30, 40, 30]
    xy, sc = fr.select(kept, 1)
    assert xy.tolist() == [[0, 1]]
    assert len(fr.select(kept, 5)[0]) == 5 and len(fr.select(kept, 9)[0]) == 5


def test_gate_counts_of_the_scenes():
    """The small scenes of the GPU tests exercise ties, a cut inside a score class and the border gate."""
    img = fr.make_scene(120, 150, seed=2, noise=20, levels=8)
    sc = fr.fast_score(img)
    nms = fr.suppress(sc)
    kept = fr.gate(nms, 16)
    assert (sc > 0).sum() > 1000 and (nms > 0).sum() > 200 and (kept > 0).sum() > 100
    assert len(np.unique(kept[kept > 0])) <= 8                       # few score classes: cuts fall inside one
    img = fr.make_scene(97, 83, seed=3)
    nms = fr.suppress(fr.fast_score(img))
    assert (fr.gate(nms, 16) > 0).sum() > (fr.gate(nms, 31) > 0).sum() >= 1


# ------------------------------------------------------------------------------------------------------------ blur
def test_blur():
    assert fr.BLUR_W.sum() == 256 and (fr.BLUR_W == fr.BLUR_W[::-1]).all()
    for v in (0, 1, 127, 255):
        assert (fr.blur(np.full((9, 13), v, np.uint8)) == v).all()
    for shape in [(1, 1), (1, 5), (2, 2), (3, 40)]:
        assert (fr.blur(np.full(shape, 200, np.uint8)) == 200).all()
    imp = np.zeros((15, 17), np.uint8)
    imp[7, 8] = 255
    want = (255 * np.outer(fr.BLUR_W, fr.BLUR_W) + 32768) >> 16
    got = fr.blur(imp)
    assert np.array_equal(got[4:11, 5:12], want) and got.sum() == want.sum()
    # reflect-101: index -1 is index 1 (the border pixel is not repeated), so an impulse at index 1 is seen through taps
    # x + k - 3 = 1 and x + k - 3 = -1: out[x] = w[4 - x] + w[2 - x]
    edge = np.zeros((8, 8), np.uint8)
    edge[1, 1] = 255
    w = fr.BLUR_W
    col = np.array([w[4] + w[2], w[3] + w[1], w[2] + w[0], w[1], w[0], 0, 0, 0])
    assert np.array_equal(fr.blur(edge), (255 * np.outer(col, col) + 32768) >> 16)


def test_orientation_bins():
    assert fr.angle_bin(0, 0) == (0, True)
    assert fr.angle_bin(5, 1) == (1, False) and fr.angle_bin(-5, -1) == (16, False) and fr.angle_bin(5, -1) == (29, False)
    assert fr.angle_bin(0, 5)[1] and fr.angle_bin(0, -5)[1]          # 90 degrees is the edge between bins 7 and 8
    img = np.zeros((31, 31), np.uint8)
    img[15, 20] = 10
    assert fr.moments(img, 15, 15) == (50, 0)
    img[3, 15] = 7                                                    # dy = -12: inside the disc
    img[0, 0] = 200                                                   # outside the disc
    assert fr.moments(img, 15, 15) == (50, -84)


# --------------------------------------------------------------------------------------------------------- pattern
def test_default_pattern_and_rotation():
    base, rot = default_tables()
    assert base.shape == (256, 4) and base.dtype == np.int8 and rot.shape == (30, 256, 4)
    assert hashlib.sha256(base.tobytes()).hexdigest() == DEFAULT_PATTERN_SHA256
    b = base.astype(int)
    assert ((b[:, 0] ** 2 + b[:, 1] ** 2) <= 169).all() and ((b[:, 2] ** 2 + b[:, 3] ** 2) <= 169).all()
    assert not ((b[:, 0] == b[:, 2]) & (b[:, 1] == b[:, 3])).any()
    both = {tuple(p) for p in b.tolist()} | {(p[2], p[3], p[0], p[1]) for p in b.tolist()}
    assert len(both) == 512                                           # no pair twice, in either direction
    assert np.array_equal(rot, fr.rotate_pattern(base))
    assert np.array_equal(rot[0], base)
    for k in range(30):
        assert np.array_equal(rot[(k + 15) % 30].astype(int), -rot[k].astype(int))
    assert np.abs(rot.astype(int)).max() <= 14
    # centre-weighted: more endpoints inside half the radius than a uniform law over the disc would put there (1/4)
    r2 = np.concatenate([b[:, 0] ** 2 + b[:, 1] ** 2, b[:, 2] ** 2 + b[:, 3] ** 2])
    assert (r2 <= 42).mean() > 0.4


def test_rotation_refuses_a_table_beyond_radius_13():
    from sfm_amd import _lib, features
    base = np.array(default_tables()[0])
    base[5] = (14, 0, 1, 1)
    with pytest.raises(ValueError):
        features.rotate_pattern(base)
    lib = _lib.load()
    rot = np.full((30, 256, 4), 77, np.int8)
    assert lib.sfm_orb_rotate_pattern(ctypes.c_void_p(base.ctypes.data), ctypes.c_void_p(rot.ctypes.data)) == -1
    assert (rot == 77).all()
    assert lib.sfm_orb_rotate_pattern(None, ctypes.c_void_p(rot.ctypes.data)) == -1
    assert lib.sfm_orb_default_pattern(None) == -1
    base[5] = (13, 0, 0, -13)
    assert np.array_equal(features.rotate_pattern(base), fr.rotate_pattern(base))


def test_features_plan_under_address_and_ub_sanitizers(tmp_path):
    """sfm_amd/csrc/features_plan.h (pattern generator and rotation, argument checks, image table, workspace layout) is plain
    C++: built with g++ -fsanitize=address,undefined and driven over degenerate and random batches."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "features_plan_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "features_plan_check.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    for seed in (1, 2):
        run = subprocess.run([str(exe), str(seed)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])


# ------------------------------------------------------------------------------------------------- descriptor bits
def test_descriptor_bit_layout():
    """Bit k of the descriptor sits in byte k / 8 at position k % 8."""
    rot = np.zeros((30, 256, 4), np.int8)
    rot[:, :, 0] = -1                                                 # a = (-1, 0), b = (1, 0) for every pair ...
    rot[:, :, 2] = 1
    rot[:, 9] = (1, 0, -1, 0)                                         # ... except pair 9, which looks the other way
    img = np.zeros((41, 41), np.uint8)
    img[:, 21:] = 200
    bl = fr.blur(img)
    bins, amb, desc = fr.describe(img, bl, np.array([[20, 20]]), rot)
    assert bins[0] == 0 and not amb[0]                                # brighter to the right: the centroid lies along +x
    want = np.full(32, 0xFF, np.uint8)
    want[1] = 0xFF ^ (1 << 1)
    assert np.array_equal(desc[0], want)


# ------------------------------------------------------------------------------------------------------------- PNM
def test_pnm_round_trip(tmp_path):
    from sfm_amd import read_pnm, write_pnm
    rng = np.random.default_rng(3)
    gray = rng.integers(0, 256, (7, 11), dtype=np.uint8)
    bgr = rng.integers(0, 256, (5, 9, 3), dtype=np.uint8)
    write_pnm(tmp_path / "a.pgm", gray)
    write_pnm(tmp_path / "a.ppm", bgr)
    write_pnm(tmp_path / "c.ppm", bgr, comment="made by a test")
    assert open(tmp_path / "a.pgm", "rb").read().startswith(b"P5\n11 7\n255\n")
    assert np.array_equal(read_pnm(tmp_path / "a.pgm"), gray) and read_pnm(tmp_path / "a.pgm").dtype == np.uint8
    assert np.array_equal(read_pnm(tmp_path / "a.ppm"), bgr)
    assert np.array_equal(read_pnm(tmp_path / "c.ppm"), bgr)
    raw = open(tmp_path / "a.ppm", "rb").read()
    assert raw[len(b"P6\n9 5\n255\n"):][:3] == bytes(bgr[0, 0, ::-1])        # the file holds RGB, the array BGR
    # comments anywhere in the header, other whitespace
    (tmp_path / "d.pgm").write_bytes(b"P5 # magic\n# a line of its own\n3\t2 # size\n255\n" + bytes(range(6)))
    assert read_pnm(tmp_path / "d.pgm").tolist() == [[0, 1, 2], [3, 4, 5]]
    (tmp_path / "t.pgm").write_bytes(b"P5\n3 2\n255\n" + bytes(range(5)))
    with pytest.raises(ValueError, match="truncated"):
        read_pnm(tmp_path / "t.pgm")
    (tmp_path / "h.pgm").write_bytes(b"P5\n3")
    with pytest.raises(ValueError):
        read_pnm(tmp_path / "h.pgm")
    (tmp_path / "m.pgm").write_bytes(b"P5\n1 1\n65535\n\x00\x00")
    with pytest.raises(ValueError):
        read_pnm(tmp_path / "m.pgm")
    (tmp_path / "p.pgm").write_bytes(b"P2\n1 1\n255\n0\n")
    with pytest.raises(ValueError):
        read_pnm(tmp_path / "p.pgm")
    with pytest.raises(ValueError):
        write_pnm(tmp_path / "f.pgm", gray.astype(np.float32))


def test_bgr_to_gray_rule():
    from sfm_amd.features import bgr_to_gray
    px = lambda b, g, r: np.array([[[b, g, r]]], dtype=np.uint8)
    assert bgr_to_gray(px(255, 255, 255))[0, 0] == 255 and bgr_to_gray(px(0, 0, 0))[0, 0] == 0
    assert bgr_to_gray(px(255, 0, 0))[0, 0] == 29 and bgr_to_gray(px(0, 255, 0))[0, 0] == 150
    assert bgr_to_gray(px(0, 0, 255))[0, 0] == 76
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    assert np.array_equal(bgr_to_gray(img), fr.bgr_to_gray(img)) and bgr_to_gray(img).dtype == np.uint8


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_without_gpu():
    from sfm_amd import _lib
    lib = _lib.load()
    off = np.array([0, 63 * 63], dtype=np.int64)
    hh, ww = np.array([63], np.int32), np.array([63], np.int32)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    need = ctypes.c_int64(-1)
    assert lib.sfm_features_workspace_bytes(1, hp(off), ctypes.byref(need)) == 0 and need.value >= 2 * 63 * 63
    assert lib.sfm_features_workspace_bytes(1, hp(off), None) == -1
    assert lib.sfm_features_workspace_bytes(1, None, ctypes.byref(need)) == -1
    assert lib.sfm_features_workspace_bytes(-1, hp(off), ctypes.byref(need)) == -1
    bad = np.array([0, 10, 5], dtype=np.int64)
    assert lib.sfm_features_workspace_bytes(2, hp(bad), ctypes.byref(need)) == -1
    zero = np.array([0], dtype=np.int64)
    assert lib.sfm_features_workspace_bytes(0, hp(zero), ctypes.byref(need)) == 0 and need.value > 0
    # a null handle is refused before anything else is looked at
    assert lib.sfm_features_detect(None, None, None, hp(off), hp(hh), hp(ww), 1, 20, 31, 0, None, None, 0) == -1
    assert lib.sfm_features_describe(None, None, hp(off), hp(hh), hp(ww), 1, None, 0, None, None, None, None, None, None,
                                     None, 0) == -1
