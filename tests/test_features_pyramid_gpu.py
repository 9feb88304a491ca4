"""The multi-scale feature stage on the device (sfm_features_pyramid, sfm_features_merge_count / _gather around the
unchanged sfm_features_detect / _describe) against the contract restated in tests/features_pyramid_reference.py: every
output byte must be EQUAL - levels, level masks, kp_ptr, xy as float32 bits, level, score, desc, src - with the one
exception of the angle bin (and with it the descriptor) of a keypoint whose atan2 falls on a bin edge, which the reference
flags.  Then the cut across levels with ties, degenerate input and the refusals, properties that need no reference, the old
path, and the chain up to tracks on a pair of images taken from two distances."""
import ctypes
import functools

import numpy as np
import pytest

import features_reference as fr
import features_pyramid_reference as pr
from test_features_reference import default_tables

pytestmark = pytest.mark.gpu

SHAPES = [(97, 131), (64, 129), (65, 257), (63, 200), (33, 33), (1, 70), (70, 1)]
KEYS = ("level", "score", "angle_bin", "desc")


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def mixed_batch():
    images = [fr.make_scene(h, w, seed=30 + i) for i, (h, w) in enumerate(SHAPES)]
    images[4][13:20, 13:20] = 50
    images[4][16, 16] = 250               # the one admissible pixel of the 33 x 33 image at edge 16 is a corner
    return tuple(frozen(a) for a in images)


def make_mask(shape, i):
    """None for every third image; else a mask with a hole, a masked band and values other than 255."""
    if i % 3 == 2:
        return None
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    m = np.full(shape, 3 + i, np.uint8)
    m[(yy - shape[0] // 2) ** 2 + (xx - shape[1] // 3) ** 2 < 60] = 0
    m[:, (xx[0] % 37) == 5] = 0
    return m


@functools.lru_cache(maxsize=None)
def mixed_masks():
    return tuple(make_mask(a.shape, i) for i, a in enumerate(mixed_batch()))


def reference(img, mask=None, **kw):
    return pr.detect_and_describe(img, default_tables()[1], mask=mask, **kw)


def raw(images, masks=None, **kw):
    from sfm_amd import features
    return features.detect_and_describe_raw(list(images), None if masks is None else list(masks), **kw)


def assert_levels(images, masks, n_levels, scale):
    from sfm_amd import pyramid_levels
    lv, mk = pyramid_levels(list(images), None if masks is None else list(masks), n_levels=n_levels, scale=scale)
    assert len(lv) == len(images) and (mk is None) == (masks is None)
    for i, img in enumerate(images):
        m = None if masks is None else (np.full(img.shape, 1, np.uint8) if masks[i] is None else (masks[i] > 0).astype(np.uint8))
        want, want_m = pr.pyramid(img, n_levels, scale[0], scale[1], m)
        assert len(lv[i]) == n_levels
        for l in range(n_levels):
            assert lv[i][l].shape == want[l].shape and lv[i][l].dtype == np.uint8, (i, l)
            assert np.array_equal(lv[i][l], want[l]), (i, l, "level")
            if masks is not None:
                assert np.array_equal(mk[i][l], want_m[l]), (i, l, "mask")


def assert_matches_reference(out, refs, n_levels, what="", refs_src=None):
    """refs: the restatement from the uncut union; refs_src: from the per-level pre-cut, whose src indexes what the device's
    level batch holds (default: refs, right without a cut)."""
    kp, lk = out["kp_ptr"], out["lvl_kp_ptr"]
    assert kp.dtype == np.int64 and kp[0] == 0 and len(kp) == len(refs) + 1 and len(lk) == len(refs) * n_levels + 1
    assert np.array_equal(np.diff(kp), [len(r["xy"]) for r in refs]), (what, np.diff(kp).tolist(), [len(r["xy"]) for r in refs])
    assert out["xy"].dtype == np.float32 and out["xy"].shape == (int(kp[-1]), 2)
    assert out["level"].dtype == np.uint8 and out["src"].dtype == np.int32 and out["desc"].shape == (int(kp[-1]), 32)
    for i, r in enumerate(refs):
        a, b = int(kp[i]), int(kp[i + 1])
        assert np.array_equal(out["xy"][a:b].view(np.uint32), r["xy"].view(np.uint32)), (what, i, "xy")
        assert np.array_equal(out["level"][a:b], r["level"]), (what, i, "level")
        assert np.array_equal(out["score"][a:b], r["score"]), (what, i, "score")
        rs = (refs_src or refs)[i]
        assert np.array_equal(out["src"][a:b] - int(lk[i * n_levels]), rs["src"]), (what, i, "src")
        sure = ~r["ambiguous"]
        assert r["ambiguous"].sum() <= 1
        assert np.array_equal(out["angle_bin"][a:b][sure], r["angle_bin"][sure]), (what, i, "angle_bin")
        assert np.array_equal(out["desc"][a:b][sure], r["desc"][sure]), (what, i, "desc")


# ---------------------------------------------------------------------------------- every output byte, the mixed batch
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("scale", [(6, 5), (3, 2), (2, 1), (9, 8)], ids=lambda s: f"{s[0]}over{s[1]}")
@pytest.mark.parametrize("n_levels", [2, 8])
def test_mixed_batch_against_the_restatement(gpu_ready, n_levels, scale, masked):
    images = mixed_batch()
    masks = mixed_masks() if masked else None
    assert_levels(images, masks, n_levels, scale)
    refs = [reference(a, None if masks is None else masks[i], edge=16, n_levels=n_levels, num=scale[0], den=scale[1])
            for i, a in enumerate(images)]
    # the reference alone: keypoints on more than one level, none on the images that cannot hold one
    assert sum((r["lvl_count"][1:] > 0).sum() for r in refs) >= 2 and sum(len(r["xy"]) for r in refs) >= 60
    assert all(len(refs[i]["xy"]) == 0 for i in (5, 6)) and (refs[4]["lvl_count"][1:] == 0).all()
    assert masked or refs[4]["xy"].tolist() == [[16.0, 16.0]]          # under the mask that pixel is masked out
    out = raw(images, masks, edge=16, n_levels=n_levels, scale=scale)
    assert_matches_reference(out, refs, n_levels, (n_levels, scale, masked))


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_sizes_around_the_resampling_tile(gpu_ready, masked):
    """The resampling tile is 256 x 16 destination pixels.  At 6/5 the images below have a level 1 of exactly two tiles each
    way (32 x 512: the width a tile multiple, every store a whole dword), one pixel more (33 x 513) and one less (31 x 511)."""
    shapes = [(38, 614), (40, 616), (37, 613)]
    assert [pr.level_sizes(h, w, 2)[1] for h, w in shapes] == [(32, 512), (33, 513), (31, 511)]
    images = [fr.make_scene(h, w, seed=50 + i) for i, (h, w) in enumerate(shapes)]
    masks = [make_mask(a.shape, i) for i, a in enumerate(images)] if masked else None
    assert_levels(images, masks, 3, (6, 5))
    refs = [reference(a, None if masks is None else masks[i], edge=16, n_levels=3) for i, a in enumerate(images)]
    assert sum(len(r["xy"]) for r in refs) >= 30
    assert_matches_reference(raw(images, masks, edge=16, n_levels=3), refs, 3, masked)


# ------------------------------------------------------------------------------------------ the cut across the levels
@functools.lru_cache(maxsize=None)
def tied_scene():
    return frozen(fr.make_scene(160, 200, 7, levels=8))


@pytest.mark.parametrize("max_features", [10, 50, 100, 1000])
def test_cut_across_levels_with_ties(gpu_ready, max_features):
    img = tied_scene()
    union = reference(img, edge=16, n_levels=4, max_features=max_features)
    precut = reference(img, edge=16, n_levels=4, max_features=max_features, precut=True)
    assert len(union["xy"]) == min(max_features, 470)
    if max_features == 50:
        assert union["cut"] == (127, 47, 6, 3)          # the cut falls inside a tied class
    out = raw([img], edge=16, n_levels=4, max_features=max_features)
    assert_matches_reference(out, [union], 4, max_features, refs_src=[precut])
    # two such images and a third in one batch: the cut is per image
    other = fr.make_scene(90, 120, seed=9)
    out3 = raw([img, other, img], edge=16, n_levels=4, max_features=max_features)
    ref_o = reference(other, edge=16, n_levels=4, max_features=max_features)
    pre_o = reference(other, edge=16, n_levels=4, max_features=max_features, precut=True)
    assert_matches_reference(out3, [union, ref_o, union], 4, max_features, refs_src=[precut, pre_o, precut])


# ------------------------------------------------------------------------------------------------------- degenerate
def test_degenerate_input(gpu_ready):
    from sfm_amd import PyramidFeatures, detect_and_describe_batched, detect_features
    flat = np.full((80, 90), 131, np.uint8)
    f = detect_and_describe_batched([flat], n_levels=8)[0]
    assert isinstance(f, PyramidFeatures) and f.xy.shape == (0, 2) and f.xy.dtype == np.float32 and f.descriptors is None
    assert f.level.shape == (0,) and f.size.shape == (0,)
    scene = fr.make_scene(97, 131, seed=30)
    some = detect_and_describe_batched([flat, scene, flat[:20, :20], scene], edge=16, n_levels=4, max_features=30)
    assert [len(g.xy) for g in some] == [0, 30, 0, 30]
    assert np.array_equal(some[1].xy, some[3].xy) and np.array_equal(some[1].descriptors, some[3].descriptors)
    zero = detect_and_describe_batched([scene, scene], [np.zeros(scene.shape, np.uint8), None], edge=16, n_levels=4)
    assert len(zero[0].xy) == 0 and len(zero[1].xy) == len(reference(scene, edge=16, n_levels=4)["xy"])
    assert detect_and_describe_batched([], n_levels=8) == []
    xy, desc = detect_features(flat, n_levels=3)
    assert xy.shape == (0, 2) and desc is None


def test_refusals_carry_the_rule(gpu_ready):
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p
    h = _lib.get_handle(0)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    heights, widths = np.array([40], np.int32), np.array([50], np.int32)
    off = np.array([0, 2000], np.int64)
    buf = lambda n: torch.zeros(n, dtype=torch.uint8, device="cuda")
    img, msk, lvl, lvl_m, ws = buf(2000), buf(2000), buf(8000), buf(8000), buf(1 << 16)

    def pyramid(n_levels=8, num=6, den=5, images=img, masks=None, lvl_masks=None, lvl_images=lvl, heights=heights,
                workspace=ws, workspace_bytes=1 << 16, handle=h._h):
        rc = h.lib.sfm_features_pyramid(handle, _p(images), _p(masks), hp(off), None if heights is None else hp(heights),
                                        hp(widths), 1, n_levels, num, den, _p(lvl_images), _p(lvl_masks), _p(workspace),
                                        workspace_bytes)
        return rc, (h.lib.sfm_last_error(h._h) or b"").decode()

    assert pyramid()[0] == 0 and pyramid(masks=msk, lvl_masks=lvl_m)[0] == 0
    for kw, text in [(dict(n_levels=1), "n_levels must be in [2, 16]"), (dict(n_levels=17), "n_levels must be in [2, 16]"),
                     (dict(num=5, den=5), "den < num <= 2 den"), (dict(num=11, den=5), "den < num <= 2 den"),
                     (dict(num=17, den=9), "at most 16"), (dict(num=10, den=9), "at least 9/8"),
                     (dict(images=None), "null pointer"), (dict(lvl_images=None), "null pointer"),
                     (dict(heights=None), "null pointer"), (dict(workspace_bytes=8), "workspace too small"),
                     (dict(workspace=None), "workspace too small"),
                     (dict(masks=msk), "both be given or both be null"), (dict(lvl_masks=lvl_m), "both be given or both be null")]:
        rc, msg = pyramid(**kw)
        assert rc == -1 and "sfm_features_pyramid" in msg and text in msg, (kw, rc, msg)
    assert pyramid(handle=None)[0] == -1
    kp_l, kp = torch.zeros(9, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda")
    score = buf(16)

    def count(n_levels=8, max_features=0, lvl_kp_ptr=kp_l, kp_ptr=kp, workspace_bytes=1 << 16):
        rc = h.lib.sfm_features_merge_count(h._h, _p(lvl_kp_ptr), _p(score), 1, n_levels, max_features, _p(kp_ptr), _p(ws),
                                            workspace_bytes)
        return rc, (h.lib.sfm_last_error(h._h) or b"").decode()

    assert count()[0] == 0
    for kw, text in [(dict(n_levels=1), "n_levels"), (dict(n_levels=17), "n_levels"), (dict(max_features=-1), "max_features"),
                     (dict(lvl_kp_ptr=None), "null pointer"), (dict(kp_ptr=None), "null pointer"),
                     (dict(workspace_bytes=8), "workspace too small")]:
        rc, msg = count(**kw)
        assert rc == -1 and "sfm_features_merge_count" in msg and text in msg, (kw, rc, msg)
    lvl_h, lvl_w = np.full(8, 40, np.int32), np.full(8, 50, np.int32)
    out4, out1 = torch.zeros(64, dtype=torch.int32, device="cuda"), buf(64)

    def gather(n_kp=1, xy=out4, workspace_bytes=1 << 16, n_levels=8):
        rc = h.lib.sfm_features_merge_gather(h._h, _p(kp_l), _p(out4), _p(score), _p(score), _p(out1), hp(lvl_h), hp(lvl_w), 1,
                                             n_levels, _p(kp), n_kp, _p(xy), _p(out1), _p(out1), _p(out1), _p(out1), _p(out4),
                                             _p(ws), workspace_bytes)
        return rc, (h.lib.sfm_last_error(h._h) or b"").decode()

    assert gather(n_kp=0)[0] == 0
    for kw, text in [(dict(n_kp=-1), "n_kp out of range"), (dict(xy=None), "null pointer"),
                     (dict(workspace_bytes=8), "workspace too small"), (dict(n_levels=1), "n_levels")]:
        rc, msg = gather(**kw)
        assert rc == -1 and "sfm_features_merge_gather" in msg and text in msg, (kw, rc, msg)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------ properties without a reference
def test_batch_independence_and_repeatability(gpu_ready):
    images = [mixed_batch()[i] for i in (0, 1, 2, 3)] + [tied_scene()]
    kw = dict(edge=16, n_levels=8, max_features=60)
    whole = raw(images, **kw)
    again = raw(images, **kw)
    for k in ("kp_ptr", "xy", "src", "lvl_kp_ptr") + KEYS:
        assert np.array_equal(whole[k], again[k]), k
    assert (np.diff(whole["kp_ptr"]) > 0).all() and np.diff(whole["kp_ptr"]).max() == 60
    for i, img in enumerate(images):
        alone = raw([img], **kw)
        a, b = int(whole["kp_ptr"][i]), int(whole["kp_ptr"][i + 1])
        assert int(alone["kp_ptr"][-1]) == b - a
        for k in ("xy",) + KEYS:
            assert np.array_equal(alone[k], whole[k][a:b]), (i, k)
        assert np.array_equal(alone["src"], whole["src"][a:b] - int(whole["lvl_kp_ptr"][i * 8]))


def test_level_0_is_the_single_scale_stage(gpu_ready):
    images = [mixed_batch()[0], mixed_batch()[2], tied_scene()]
    multi = raw(images, edge=16, n_levels=8)
    single = raw(images, edge=16)
    assert single["xy"].dtype == np.int32 and "level" not in single
    for i in range(len(images)):
        a, b = int(multi["kp_ptr"][i]), int(multi["kp_ptr"][i + 1])
        first = multi["level"][a:b] == 0
        c, d = int(single["kp_ptr"][i]), int(single["kp_ptr"][i + 1])
        assert first.sum() == d - c >= 20 and first[:d - c].all()          # level 0 comes first
        assert np.array_equal(multi["xy"][a:b][first], single["xy"][c:d].astype(np.float32))
        for k in ("score", "angle_bin", "desc"):
            assert np.array_equal(multi[k][a:b][first], single[k][c:d]), (i, k)


def test_the_single_scale_path_is_untouched(gpu_ready):
    from sfm_amd import Features, detect_and_describe_batched
    images = [mixed_batch()[0], tied_scene()]
    for f, img in zip(detect_and_describe_batched(images), images):
        r = fr.detect_and_describe(img, default_tables()[1])
        assert type(f) is Features and f._fields == ("xy", "response", "angle", "descriptors")
        assert f.xy.dtype == np.float32 and np.array_equal(f.xy, r["xy"].astype(np.float32)) and len(f.xy) >= 5
        assert np.array_equal(f.response, r["score"].astype(np.float32))
        sure = ~r["ambiguous"]
        assert np.array_equal(f.angle[sure], r["angle_bin"][sure].astype(np.float32) * 12)
        assert f.descriptors.dtype == np.uint8 and np.array_equal(f.descriptors[sure], r["desc"][sure])


def test_public_interface(gpu_ready):
    from sfm_amd import detect_and_describe_batched, detect_features
    img = mixed_batch()[0]
    r = reference(img, edge=16, n_levels=5, num=3, den=2)
    f = detect_and_describe_batched([img], edge=16, n_levels=5, scale=(3, 2))[0]
    assert f._fields == ("xy", "response", "angle", "descriptors", "level", "size")
    assert np.array_equal(f.xy, r["xy"]) and np.array_equal(f.level, r["level"])
    assert np.array_equal(f.response, r["score"].astype(np.float32)) and (f.angle % 12 == 0).all()
    widths = np.array([s[1] for s in pr.level_sizes(97, 131, 5, 3, 2)], np.float64)
    assert f.size.dtype == np.float32 and np.array_equal(f.size, (31.0 * 131 / widths[r["level"]]).astype(np.float32))
    assert len(np.unique(f.level)) >= 2 and f.size[f.level == 0].tolist() == [31.0] * int((f.level == 0).sum())
    xy, desc = detect_features(img, edge=16, n_levels=5, scale=(3, 2))
    assert np.array_equal(xy, f.xy) and np.array_equal(desc, f.descriptors)
    for bad in (dict(n_levels=17), dict(n_levels=8, scale=(5, 5)), dict(n_levels=8, scale=(10, 9))):
        with pytest.raises(Exception):
            detect_and_describe_batched([img], **bad)


# --------------------------------------------------------------------------------------------------------- the chain
def test_two_distances_match_through_the_pyramid_up_to_tracks(gpu_ready):
    """The zoom-3/2 pair of the worth measurement (seed 0) through ImageMatcher.process_images: with 8 levels the pair is
    verified with at least five times the matches of the single-scale stage (whose result may be None), and build_tracks
    takes the result."""
    from sfm_amd.matcher import ImageMatcher
    a, b = pr.zoom_pair(3, 2, 0)
    m = ImageMatcher()
    feats1, res1 = m.process_images([a, b], [(0, 1)], n_levels=1)
    feats8, res8 = m.process_images([a, b], [(0, 1)], n_levels=8)
    verified = lambda r: 0 if r is None or r.get("inlier_mask") is None else int(np.asarray(r["inlier_mask"]).sum())
    one, eight = verified(res1[0]), verified(res8[0])
    print(f"verified matches: 1 level {one}, 8 levels {eight}; keypoints {[len(f.xy) for f in feats1]} / {[len(f.xy) for f in feats8]}")
    assert res8[0] is not None and res8[0]["F"] is not None
    assert eight >= 5 * one and eight >= 5
    assert [len(f.xy) for f in feats8] == [535, 916]          # the restatement's counts of the worth table
    tracks = m.build_tracks([f.xy for f in feats8], [(0, 1)], res8)
    assert (tracks.lengths() == 2).sum() >= 5
