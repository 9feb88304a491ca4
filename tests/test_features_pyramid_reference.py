"""CPU tests of the multi-scale feature stage's contract: the NumPy restatement of tests/features_pyramid_reference.py
against a second statement in plain loops and hand-built cases, the level sizes, the mask rule, the cut over the union of
the levels, the coordinate map, what the pyramid is worth on scenes seen from two distances, and the planning header under
the sanitizers.  No GPU."""
import ctypes
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import features_reference as fr
import features_pyramid_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = [(n, d) for d in range(1, 17) for n in range(d + 1, 17) if n <= 2 * d and 8 * n >= 9 * d]


@functools.lru_cache(maxsize=None)
def rot_table():
    from sfm_amd import features
    rot = features.rotate_pattern(features.default_pattern())
    rot.setflags(write=False)
    return rot


# ------------------------------------------------------------------------------------------------------- resampling
def test_resampling_equals_a_plain_loop_statement():
    rng = np.random.default_rng(3)
    for hs, ws, hd, wd in [(7, 9, 6, 8), (13, 5, 7, 3), (5, 5, 1, 1), (1, 8, 1, 7), (9, 1, 8, 1), (12, 10, 6, 5), (20, 31, 18, 28)]:
        src = rng.integers(0, 256, size=(hs, ws), dtype=np.uint8)
        assert np.array_equal(pr.resample(src, hd, wd), pr.resample_loops(src.tolist(), hd, wd)), (hs, ws, hd, wd)


def test_resampling_properties():
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, size=(14, 22), dtype=np.uint8)
    assert np.array_equal(pr.resample(src, 14, 22), src)                      # equal sizes: the identity
    half = pr.resample(src, 14, 11)                                           # 2/1 along x, fy = 0: rounded mean of pairs
    pairs = (src[:, 0::2].astype(int) + src[:, 1::2].astype(int) + 1) >> 1
    assert np.array_equal(half, pairs)
    for hd, wd in [(12, 18), (7, 11), (13, 21), (1, 1)]:
        out = pr.resample(src, hd, wd).astype(int)
        y0, y1, _ = pr.taps(hd, 14)
        x0, x1, _ = pr.taps(wd, 22)
        four = np.stack([src[y0][:, x0], src[y0][:, x1], src[y1][:, x0], src[y1][:, x1]]).astype(int)
        assert (out >= four.min(axis=0)).all() and (out <= four.max(axis=0)).all()      # hence within [min, max] of the source
        assert out.min() >= src.min() and out.max() <= src.max()
    for v in (0, 1, 127, 254, 255):
        assert (pr.resample(np.full((9, 13), v, np.uint8), 8, 11) == v).all()


# ------------------------------------------------------------------------------------------------------------ sizes
def test_level_sizes():
    assert [s[0] for s in pr.level_sizes(240, 240, 8)] == [240, 200, 167, 139, 116, 97, 81, 68]
    assert [s[1] for s in pr.level_sizes(240, 240, 8)] == [240, 200, 167, 139, 116, 97, 81, 68]
    # a 33 x 33 image is eligible at level 0 alone: at 6/5 the rule gives 28 from level 1 on, below the 33 a keypoint needs
    sizes = pr.level_sizes(33, 33, 4)
    assert sizes[0] == (33, 33) and sizes[1] == (28, 28) and all(max(s) < 33 for s in sizes[1:])
    rot = rot_table()
    img = fr.make_scene(33, 33, 5)
    r = pr.detect_and_describe(img, rot, edge=16, n_levels=4)
    assert (r["lvl_count"][1:] == 0).all()
    assert len(SCALES) > 20 and (6, 5) in SCALES and (9, 8) in SCALES and (2, 1) in SCALES and (16, 8) in SCALES
    for num, den in SCALES:
        assert pr.check_options(8, num, den)
        n = np.arange(1, 5000)
        nxt = np.array([pr.next_size(int(v), num, den) for v in n])
        assert (nxt <= n).all() and (nxt >= 1).all()
        assert (nxt[n >= 33] < n[n >= 33]).all(), (num, den)
    assert pr.next_size(0, 6, 5) == 0
    for bad in [(1, 6, 5), (17, 6, 5), (8, 5, 5), (8, 11, 5), (8, 17, 9), (8, 10, 9)]:
        assert not pr.check_options(*bad)


# ------------------------------------------------------------------------------------------------------------- masks
def test_one_masked_source_pixel_removes_exactly_its_readers():
    for hs, ws, hd, wd in [(12, 12, 10, 10), (9, 14, 6, 7), (10, 10, 5, 5), (8, 8, 8, 8)]:
        y0, y1, _ = pr.taps(hd, hs)
        x0, x1, _ = pr.taps(wd, ws)
        for my, mx in [(0, 0), (hs - 1, ws - 1), (hs // 2, ws // 2), (3, ws - 2)]:
            mask = np.full((hs, ws), 255, np.uint8)
            mask[my, mx] = 0
            got = pr.resample_mask(mask, hd, wd)
            for y in range(hd):
                for x in range(wd):
                    reads = (my in (y0[y], y1[y])) and (mx in (x0[x], x1[x]))
                    assert got[y, x] == (0 if reads else 1), (hs, ws, my, mx, y, x)
    assert set(np.unique(pr.resample_mask(np.full((6, 6), 7, np.uint8), 5, 5))) == {1}
    lv, mk = pr.pyramid(np.zeros((40, 40), np.uint8), 3, mask=np.full((40, 40), 9, np.uint8))
    assert (mk[0] == 9).all() and (mk[1] == 1).all() and mk[2].shape == lv[2].shape


# --------------------------------------------------------------------------------------------------------------- cut
def test_cut_over_the_union_with_ties():
    rot = rot_table()
    img = fr.make_scene(160, 200, 7, levels=8)
    full = pr.detect_and_describe(img, rot, edge=16, n_levels=4)
    assert full["lvl_count"].tolist() == [188, 132, 88, 62] and len(full["xy"]) == 470
    cut = pr.detect_and_describe(img, rot, edge=16, n_levels=4, max_features=50)
    assert cut["cut"] == (127, 47, 6, 3)          # the cut score, keypoints above it, at it, and how many of those stay
    assert len(cut["xy"]) == 50 and (np.diff(cut["src"]) > 0).all()
    sc = full["score"].astype(int)
    at = np.nonzero(sc == 127)[0]
    assert set(cut["src"]) == set(np.nonzero(sc > 127)[0]) | set(at[:3])
    for m in (10, 50, 100):
        a = pr.detect_and_describe(img, rot, edge=16, n_levels=4, max_features=m)
        b = pr.detect_and_describe(img, rot, edge=16, n_levels=4, max_features=m, precut=True)
        assert len(a["xy"]) == m
        for k in ("xy", "level", "score", "angle_bin", "desc", "xy_level"):
            assert np.array_equal(a[k], b[k]), (m, k)
    big = pr.detect_and_describe(img, rot, edge=16, n_levels=4, max_features=1000)
    assert np.array_equal(big["src"], np.arange(470)) and big["cut"] == (0, 470, 0, 0)


# --------------------------------------------------------------------------------------------------------------- map
def test_coordinate_map():
    for n0 in (33, 240, 1601):
        x = np.arange(n0)
        m = pr.map_coord(x, n0, n0)
        assert m.dtype == np.float32 and np.array_equal(m, x.astype(np.float32))
        for num, den in ((6, 5), (9, 8), (2, 1), (3, 2)):
            nl = n0
            for _ in range(7):
                nl = pr.next_size(nl, num, den)
                m = pr.map_coord(np.arange(nl), n0, nl).astype(np.float64)
                assert (np.diff(m) > 0).all() and m[0] >= -0.5 and m[-1] <= n0 - 0.5


# ------------------------------------------------------------------------------------------------------------- worth
# the restatement's counts (keypoints A, keypoints B, matches, correct): 1 level, then 8 levels at 6/5.  They reproduce the
# prototype's figures of the README's table exactly.
WORTH = {(3, 2, 0): ((143, 211, 30, 19), (535, 916, 323, 311)), (3, 2, 1): ((185, 292, 33, 24), (653, 1185, 420, 414)),
         (3, 2, 2): ((150, 197, 32, 20), (486, 860, 295, 284)), (2, 1, 0): ((150, 289, 10, 1), (486, 1281, 261, 252)),
         (2, 1, 1): ((162, 255, 21, 6), (501, 1217, 246, 222)), (2, 1, 2): ((150, 258, 17, 3), (543, 1304, 281, 259))}


@pytest.mark.parametrize("zn,zd,seed", sorted(WORTH))
def test_worth_of_the_pyramid_on_a_scene_seen_from_two_distances(zn, zd, seed):
    rot = rot_table()
    one = pr.worth_case(zn, zd, seed, rot, 1)
    eight = pr.worth_case(zn, zd, seed, rot, 8)
    print(f"zoom {zn}/{zd} seed {seed}: 1 level {one}, 8 levels {eight}")
    assert eight[3] >= 5 * one[3]
    assert 10 * eight[3] >= 9 * eight[2]          # at worst 222 of 246 = 90.2 % (zoom 2, seed 1)
    assert (one, eight) == WORTH[(zn, zd, seed)]


# ------------------------------------------------------------------------------------------------------------ native
def write_value_file(path):
    """Cases for the native program's plain-loop resampling: (hs, ws, hd, wd, mask) int32, the source, what NumPy gives."""
    rng = np.random.default_rng(11)
    cases = []
    for hs, ws, num, den in [(40, 57, 6, 5), (33, 33, 9, 8), (17, 64, 2, 1), (1, 30, 3, 2), (30, 1, 6, 5), (90, 71, 16, 9)]:
        hd, wd = pr.next_size(hs, num, den), pr.next_size(ws, num, den)
        src = rng.integers(0, 256, size=(hs, ws), dtype=np.uint8)
        cases.append((hs, ws, hd, wd, 0, src, pr.resample(src, hd, wd)))
        m = (rng.random((hs, ws)) > 0.1).astype(np.uint8) * 200
        cases.append((hs, ws, hd, wd, 1, m, pr.resample_mask(m, hd, wd)))
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for hs, ws, hd, wd, mask, src, want in cases:
            f.write(struct.pack("<5i", hs, ws, hd, wd, mask))
            f.write(src.tobytes())
            f.write(want.tobytes())
    return len(cases)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_features_pyramid_plan_native(tmp_path, sanitize):
    """sfm_amd/csrc/features_pyramid_plan.h (option checks, level tables, tile tables, taps, coordinate map, workspace
    layouts, the resampling in plain loops) is plain C++: built with g++, plain and with -fsanitize=address,undefined, and
    driven over degenerate and random batches and over values NumPy computed."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "features_pyramid_check"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if sanitize else []
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + flags + ["-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "features_pyramid_check.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    values = tmp_path / "values.bin"
    n = write_value_file(values)
    assert n == 12
    for seed in (1, 2):
        run = subprocess.run([str(exe), str(seed), str(values)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])


# ------------------------------------------------------------------------------------------------- host entry points
def test_pyramid_sizes_entry_point_against_the_restatement():
    """sfm_features_pyramid_sizes is host only: the library's tables against the restatement, and its refusals."""
    from sfm_amd import _lib
    lib = _lib.load()
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    shapes = [(97, 131), (64, 129), (33, 33), (1, 70), (70, 1), (0, 5)]
    h = np.array([s[0] for s in shapes], np.int32)
    w = np.array([s[1] for s in shapes], np.int32)
    for n_levels, (num, den) in [(2, (6, 5)), (8, (6, 5)), (16, (9, 8)), (5, (2, 1)), (8, (3, 2))]:
        n = len(shapes) * n_levels
        off, lh, lw = np.full(n + 1, -1, np.int64), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        assert lib.sfm_features_pyramid_sizes(len(shapes), hp(h), hp(w), n_levels, num, den, hp(off), hp(lh), hp(lw)) == 0
        want = [s for shp in shapes for s in pr.level_sizes(shp[0], shp[1], n_levels, num, den)]
        assert list(zip(lh.tolist(), lw.tolist())) == want
        assert off.tolist() == np.concatenate([[0], np.cumsum([a * b for a, b in want])]).tolist()
    off, lh, lw = np.zeros(13, np.int64), np.zeros(12, np.int32), np.zeros(12, np.int32)
    for n_levels, num, den in [(1, 6, 5), (17, 6, 5), (8, 5, 5), (8, 11, 5), (8, 17, 9), (8, 10, 9)]:
        assert lib.sfm_features_pyramid_sizes(1, hp(h), hp(w), n_levels, num, den, hp(off), hp(lh), hp(lw)) == -1
    assert lib.sfm_features_pyramid_sizes(1, None, hp(w), 8, 6, 5, hp(off), hp(lh), hp(lw)) == -1
    need = ctypes.c_int64()
    assert lib.sfm_features_pyramid_workspace_bytes(3, 8, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.sfm_features_merge_workspace_bytes(3, 8, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.sfm_features_merge_workspace_bytes(3, 1, ctypes.byref(need)) == -1
