"""sfm_features_detect / sfm_features_describe on the device against the contract restated in tests/features_reference.py:
every output byte must be EQUAL (integers throughout, so there are no tolerances); the only exception is the angle bin - and
with it the descriptor - of a keypoint whose atan2 falls on a bin edge, which the reference flags.  Then properties that
need no reference (translation, half turn, batch independence) and the public interface up to tracks."""
import functools

import numpy as np
import pytest

import features_reference as fr
from test_features_reference import default_tables

pytestmark = pytest.mark.gpu


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def batch():
    """The seven images of the batched comparison - never modified."""
    centre = fr.make_scene(33, 33, seed=5)
    centre[13:20, 13:20] = 50
    centre[16, 16] = 250                  # the one admissible pixel at edge 16 is a corner
    return tuple(frozen(a) for a in (
        fr.make_scene(97, 83, seed=3),                        # narrower than one 128-pixel tile
        fr.make_scene(160, 211, seed=1),
        fr.make_scene(63, 63, seed=6),                        # no keypoint at edge 31: one admissible pixel
        fr.make_scene(64, 200, seed=4, noise=0, levels=4),    # almost everything is tied
        fr.make_scene(120, 150, seed=2, noise=20, levels=8),
        centre,
        np.full((70, 90), 131, np.uint8)))                    # constant


@functools.lru_cache(maxsize=None)
def reference(which, edge, max_features=0, mask_kind=None):
    img = batch()[which]
    return fr.detect_and_describe(img, default_tables()[1], mask=make_mask(img.shape, mask_kind), edge=edge,
                                  max_features=max_features)


def make_mask(shape, kind):
    if kind is None:
        return None
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    if kind == "half":
        return ((xx + yy) > (shape[0] + shape[1]) // 2).astype(np.uint8) * 255
    return (((xx + yy) & 1) * 7).astype(np.uint8)              # a checkerboard of 1-pixel cells, any value > 0 counts


def device(images, **kw):
    from sfm_amd import features
    return features.detect_and_describe_raw(list(images), want_blurred=True, **kw)


def assert_matches_reference(out, refs, what=""):
    kp = out["kp_ptr"]
    assert kp.dtype == np.int64 and kp[0] == 0 and len(kp) == len(refs) + 1
    assert np.array_equal(np.diff(kp), [len(r["xy"]) for r in refs]), (what, np.diff(kp).tolist(), [len(r["xy"]) for r in refs])
    for i, r in enumerate(refs):
        a, b = int(kp[i]), int(kp[i + 1])
        assert out["xy"].dtype == np.int32 and np.array_equal(out["xy"][a:b], r["xy"]), (what, i, "xy")
        assert np.array_equal(out["score"][a:b], r["score"]), (what, i, "score")
        assert np.array_equal(out["blurred"][i], r["blurred"]), (what, i, "blurred")
        sure = ~r["ambiguous"]
        assert np.array_equal(out["angle_bin"][a:b][sure], r["angle_bin"][sure]), (what, i, "angle_bin")
        assert np.array_equal(out["desc"][a:b][sure], r["desc"][sure]), (what, i, "desc")


# ---------------------------------------------------------------------------------- one batched call, every output byte
@pytest.mark.parametrize("edge", [16, 31])
def test_batch_against_the_reference(gpu_ready, edge):
    refs = [reference(i, edge) for i in range(len(batch()))]
    # the reference alone: the comparison is neither empty nor hollowed out by flagged keypoints
    assert all(r["ambiguous"].sum() <= 1 for r in refs)
    assert len(reference(1, 31)["xy"]) >= 20
    assert len(reference(2, 31)["xy"]) == 0 and len(reference(6, edge)["xy"]) == 0
    assert reference(5, 16)["xy"].tolist() == [[16, 16]]
    out = device(batch(), edge=edge)
    assert_matches_reference(out, refs, edge)
    assert out["desc"].shape == (int(out["kp_ptr"][-1]), 32) and out["desc"].dtype == np.uint8


def test_a_batch_of_more_rows_than_one_piece_of_the_row_scan(gpu_ready):
    """69 images of 64 x 64 and one of 300 x 64: 4,716 image rows, so the one workgroup that scans the row counts walks a
    second piece of 4,096 with its carry, and the tie scan of the tall image a second tile of 256 rows; the quota cuts
    into the tied scores of most images."""
    images = [fr.make_scene(64, 64, seed=100 + i) for i in range(69)]
    images.insert(40, fr.make_scene(300, 64, seed=7, noise=20, levels=8))
    assert sum(a.shape[0] for a in images) > 4096
    for mf in (0, 4):
        refs = [fr.detect_and_describe(a, default_tables()[1], edge=16, max_features=mf) for a in images]
        assert sum(len(r["xy"]) for r in refs) > 100 and len(refs[40]["xy"]) > 0
        assert_matches_reference(device(images, edge=16, max_features=mf), refs, mf)


def test_threshold_is_honoured(gpu_ready):
    img = batch()[1]
    for threshold in (1, 60, 254):
        r = fr.detect_and_describe(img, default_tables()[1], threshold=threshold, edge=16)
        assert_matches_reference(device([img], edge=16, threshold=threshold), [r], threshold)


# --------------------------------------------------------------------------------------------------------- selection
def test_selection(gpu_ready):
    kept = reference(4, 16)["kept"]                            # the 8-level scene: a handful of score classes
    scores, counts = np.unique(kept[kept > 0], return_counts=True)
    s = int(scores[np.argmax(counts)])
    above, ties = int((kept > s).sum()), int((kept == s).sum())
    inside = above + ties // 2
    assert ties >= 4 and above < inside < above + ties        # the cut falls inside the tied class
    total = max(len(reference(i, 16)["xy"]) for i in range(len(batch())))
    for mf in (1, 50, inside, total + 5):
        refs = [reference(i, 16, mf) for i in range(len(batch()))]
        assert all(len(r["xy"]) == min(mf, len(reference(i, 16)["xy"])) for i, r in enumerate(refs))
        assert_matches_reference(device(batch(), edge=16, max_features=mf), refs, mf)
    r = reference(4, 16, inside)
    assert (r["score"] == s).sum() == inside - above and (r["score"] > s).sum() == above


# -------------------------------------------------------------------------------------------------------------- mask
@pytest.mark.parametrize("kind", ["half", "checker"])
def test_masks(gpu_ready, kind):
    refs = [reference(i, 16, 0, kind) for i in range(len(batch()))]
    assert 0 < sum(len(r["xy"]) for r in refs) < sum(len(reference(i, 16)["xy"]) for i in range(len(batch())))
    out = device(batch(), edge=16, masks=[make_mask(a.shape, kind) for a in batch()])
    assert_matches_reference(out, refs, kind)
    # a mask for some images only
    masks = [make_mask(a.shape, kind) if i % 2 else None for i, a in enumerate(batch())]
    mixed = [reference(i, 16, 0, kind if i % 2 else None) for i in range(len(batch()))]
    assert_matches_reference(device(batch(), edge=16, masks=masks), mixed, kind)


def test_a_masked_corner_still_suppresses_its_neighbour(gpu_ready):
    img = batch()[1]
    sc = fr.fast_score(img).astype(int)
    h, w = sc.shape
    found = None
    for y in range(17, h - 17):
        for x in range(17, w - 17):
            if sc[y, x] == 0:
                continue
            nb = [(sc[y + dy, x + dx], y + dy, x + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx]
            stronger = [n for n in nb if n[0] >= sc[y, x]]
            if len(stronger) == 1 and stronger[0][0] > sc[y, x]:
                found = (y, x, stronger[0][1], stronger[0][2])       # B = (y, x) loses to A alone
                break
        if found:
            break
    assert found is not None
    by, bx, ay, ax = found
    mask = np.full(img.shape, 255, np.uint8)
    mask[ay, ax] = 0                                           # A is masked out; B is not
    out = device([img], edge=16, masks=[mask])
    pts = set(map(tuple, out["xy"].tolist()))
    assert (bx, by) not in pts and (ax, ay) not in pts
    assert_matches_reference(out, [fr.detect_and_describe(img, default_tables()[1], mask=mask, edge=16)])
    assert sc[ay, ax] > sc[by, bx] > 0                         # without A, B would be the strict maximum of its 3 x 3


# ---------------------------------------------------------------------------------------------- batch independence
def test_batch_independence_and_repeatability(gpu_ready):
    imgs = batch()
    offsets = np.cumsum([0] + [a.size for a in imgs])
    assert any(o % 16 for o in offsets[1:-1])                  # the images do not start on 16-byte boundaries
    whole = device(imgs, edge=16, max_features=40)
    again = device(imgs, edge=16, max_features=40)
    for k in ("kp_ptr", "xy", "score", "angle_bin", "desc"):
        assert np.array_equal(whole[k], again[k]), k
    kp = whole["kp_ptr"]
    for i, img in enumerate(imgs):
        # alone, and behind another neighbour at another offset
        for group, pos in (([img], 0), ([imgs[(i + 3) % len(imgs)][:, 5:], img], 1)):
            o = device(group, edge=16, max_features=40)
            a, b, c, d = int(kp[i]), int(kp[i + 1]), int(o["kp_ptr"][pos]), int(o["kp_ptr"][pos + 1])
            assert d - c == b - a, (i, pos)
            for k in ("xy", "score", "angle_bin", "desc"):
                assert np.array_equal(o[k][c:d], whole[k][a:b]), (i, pos, k)
            assert np.array_equal(o["blurred"][pos], whole["blurred"][i])


# -------------------------------------------------------------------------------------------------------- translation
def test_translation(gpu_ready):
    scene = fr.make_scene(200, 260, seed=11)
    dx, dy = 7, 5
    A, B = scene[0:190, 0:250], scene[dy:dy + 190, dx:dx + 250]           # B(x, y) = A(x + dx, y + dy)
    out = device([A, B], edge=31)
    kp = out["kp_ptr"]
    at_b = {tuple(p): k for k, p in enumerate(out["xy"][kp[1]:kp[2]].tolist())}
    n = 0
    for k in range(int(kp[1])):
        x, y = out["xy"][k].tolist()
        bx, by = x - dx, y - dy
        if 31 <= bx < 250 - 31 and 31 <= by < 190 - 31:
            assert (bx, by) in at_b, (x, y)
            j = int(kp[1]) + at_b[(bx, by)]
            assert out["score"][j] == out["score"][k] and out["angle_bin"][j] == out["angle_bin"][k]
            assert np.array_equal(out["desc"][j], out["desc"][k])
            n += 1
    assert n >= 30


# ---------------------------------------------------------------------------------------------------------- half turn
def test_half_turn(gpu_ready):
    img = batch()[1]
    turned = np.ascontiguousarray(np.rot90(img, 2))
    out = device([img, turned], edge=16)
    kp = out["kp_ptr"]
    n = int(kp[1])
    assert n >= 50 and int(kp[2]) == 2 * n
    h, w = img.shape
    mirrored = np.stack([w - 1 - out["xy"][n:, 0], h - 1 - out["xy"][n:, 1]], axis=1)[::-1]
    assert np.array_equal(mirrored, out["xy"][:n])
    assert np.array_equal(out["score"][n:][::-1], out["score"][:n])
    sure = ~reference(1, 16)["ambiguous"]
    assert sure.sum() >= n - 1
    assert np.array_equal(out["angle_bin"][n:][::-1][sure], (out["angle_bin"][:n][sure].astype(int) + 15) % 30)
    assert np.array_equal(out["desc"][n:][::-1][sure], out["desc"][:n][sure])
    assert len(np.unique(out["angle_bin"][:n])) >= 10          # the steering is exercised over many bins


# -------------------------------------------------------------------------------------------- the public interface
SHIFTS = [(0, 0), (9, 4), (15, 11)]


@functools.lru_cache(maxsize=None)
def views():
    scene = fr.make_scene(180, 230, seed=21)
    return tuple(frozen(np.ascontiguousarray(scene[dy:dy + 160, dx:dx + 200])) for dx, dy in SHIFTS)


def test_process_images_to_tracks(gpu_ready):
    from sfm_amd.matcher import ImageMatcher
    m = ImageMatcher()
    pairs = [(0, 1), (0, 2), (1, 2)]
    feats, results = m.process_images(list(views()), pairs)
    assert len(feats) == 3 and all(f.xy.dtype == np.float32 and f.descriptors.shape == (len(f.xy), 32) for f in feats)
    assert all(f.response.dtype == np.float32 and f.angle.dtype == np.float32 and (f.angle % 12 == 0).all() for f in feats)
    for (i, j), r in zip(pairs, results):
        assert r is not None and r["F"] is not None
        shift = np.array(SHIFTS[j], np.float32) - np.array(SHIFTS[i], np.float32)
        q, t, d = r["matches"].queryIdx, r["matches"].trainIdx, r["matches"].distance
        exact = {(int(a), int(b)) for a, b, dist in zip(q, t, d)
                 if dist == 0 and np.array_equal(feats[j].xy[b], feats[i].xy[a] - shift)}
        at_j = {tuple(p): k for k, p in enumerate(feats[j].xy.tolist())}
        common = [(a, at_j[tuple((p - shift).tolist())]) for a, p in enumerate(feats[i].xy) if tuple((p - shift).tolist()) in at_j]
        assert len(common) >= 20 and set(common) <= exact, (i, j, len(common), len(exact))
    tracks = m.build_tracks([f.xy for f in feats], pairs, results)
    assert (tracks.lengths() == 3).sum() >= 10
    one_xy, one_desc = m.detect_features(views()[0])
    assert np.array_equal(one_xy, feats[0].xy) and np.array_equal(one_desc, feats[0].descriptors)


def test_an_image_without_keypoints(gpu_ready):
    from sfm_amd import detect_features, detect_and_describe_batched
    from sfm_amd.matcher import match_pairs
    xy, desc = detect_features(np.full((40, 50), 9, np.uint8))
    assert xy.shape == (0, 2) and xy.dtype == np.float32 and desc is None
    xy, desc = detect_features(batch()[0][:20, :20])          # too small for any keypoint
    assert xy.shape == (0, 2) and desc is None
    other = detect_features(batch()[1])[1]
    for res in match_pairs([desc, other], [(0, 1), (1, 0)], metric="hamming"):
        assert [len(a) for a in res] == [0, 0, 0]
    assert detect_and_describe_batched([]) == []


def test_colour_input_and_a_user_pattern(gpu_ready):
    from sfm_amd import detect_features
    rng = np.random.default_rng(8)
    gray = batch()[1]
    base = np.array(default_tables()[0])
    xy, desc = detect_features(gray, edge=16)
    perm = rng.permutation(256)
    xy_p, desc_p = detect_features(gray, edge=16, pattern=base[perm])
    assert np.array_equal(xy, xy_p)
    bits = np.unpackbits(desc, axis=1, bitorder="little")
    assert np.array_equal(np.unpackbits(desc_p, axis=1, bitorder="little"), bits[:, perm]) and not np.array_equal(desc, desc_p)
    assert np.array_equal(detect_features(gray, edge=16)[1], desc)          # the default table is still served from its cache
    bgr = rng.integers(0, 256, gray.shape + (3,), dtype=np.uint8)
    xy_c, desc_c = detect_features(bgr, edge=16)
    xy_g, desc_g = detect_features(fr.bgr_to_gray(bgr), edge=16)
    assert len(xy_c) > 100 and np.array_equal(xy_c, xy_g) and np.array_equal(desc_c, desc_g)
    with pytest.raises(ValueError):
        detect_features(gray, pattern=np.full((256, 4), 14, np.int8))
