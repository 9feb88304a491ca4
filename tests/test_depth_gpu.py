"""The dense-depth stage on the device against tests/depth_reference.py: every output byte - plane, cost, depth bits,
n_consistent, keep, xyz bits - on inputs of tens of pixels a side, then the default scene end to end and the chain from a
`Reconstruction`."""
import os
import re

import numpy as np
import pytest

import depth_reference as dr
from test_depth_reference import default_views, quality, random_case, random_warp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PLAN = open(os.path.join(ROOT, "sfm_amd", "csrc", "depth_plan.h")).read()
TW, TH = (int(re.search(rf"#define {n} (\d+)", _PLAN).group(1)) for n in ("DEPTH_TW", "DEPTH_TH"))


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    b = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()
    b[np.isnan(a)] = 0                                            # the payload of a NaN is not part of the rule
    return b


def device_maps(images, refs, sources, warps, planes, backproj, r):
    from sfm_amd import depth as dm
    src_ptr = np.cumsum([0] + [len(s) for s in sources]).astype(np.int64)
    src_image = np.array([s for src in sources for s in src], dtype=np.int32)
    W = np.concatenate([np.asarray(w).reshape(-1, 12) for w in warps]) if len(src_image) else np.zeros((0, 12))
    plane_ptr = np.cumsum([0] + [len(p) for p in planes]).astype(np.int64)
    return dm.depth_maps_raw([np.ascontiguousarray(a) for a in images], list(refs), src_ptr, src_image, W,
                             np.asarray(backproj, dtype=np.float64).reshape(-1, 12), plane_ptr,
                             np.concatenate([np.asarray(p, dtype=np.float64) for p in planes]), radius=r)


def assert_equal_to_reference(case, r, rel_tol=0.3, max_cost=24.0, min_consistent=1, what=""):
    """Sweep and filter of one case on the device and in NumPy: every byte.  Returns the device's DepthMaps.  The filter's
    settings are loose on purpose: on random geometry a mean cost of 24 is the median and a third of the depth is a common
    disagreement, so that every outcome of n_consistent and keep occurs."""
    images, refs, sources, warps, planes, backproj = case
    maps = device_maps(images, refs, sources, warps, planes, backproj, r)
    want = dr.sweep(images, refs, sources, warps, planes, r)
    for v in range(len(refs)):
        for name, got, ref in (("plane", maps.plane[v], want[v][0]), ("cost", maps.cost[v], want[v][1]), ("depth", maps.depth[v], want[v][2])):
            assert got.dtype == ref.dtype and got.shape == ref.shape, (what, v, name)
            assert np.array_equal(bits(got), bits(ref)), (what, v, name, int((bits(got) != bits(ref)).sum()))
    maps.filter(rel_tol, max_cost, min_consistent)
    limit = None if max_cost is None else maps.cost_limits(max_cost)
    wantf = dr.filter_views(images, refs, sources, warps, backproj, want, rel_tol, limit, min_consistent)
    for v in range(len(refs)):
        for name, got, ref in (("n_consistent", maps.n_consistent[v], wantf[v][0]), ("keep", maps.keep[v], wantf[v][1]),
                               ("xyz", maps.xyz[v], wantf[v][2])):
            assert got.dtype == ref.dtype and got.shape == ref.shape, (what, v, name)
            assert np.array_equal(bits(got), bits(ref)), (what, v, name, int((bits(got) != bits(ref)).sum()))
    return maps


def smooth_images(rng, shapes):
    """Textured images that a sideways shift matches somewhere: a cut of one smoothed random field per image."""
    field = (dr._texture(rng, 128) * 255).astype(np.uint8)
    return [field[3 * k:3 * k + h, 2 * k:2 * k + w].copy() for k, (h, w) in enumerate(shapes)]


@pytest.mark.parametrize("r", [0, 1, 4])
def test_batch_of_sizes_around_the_tile(gpu_ready, r):
    """Widths and heights at tile - 1, tile and tile + 1, more than one tile a side, sources of other sizes than their
    reference, and a last image that is a source but has no depth map of its own."""
    rng = np.random.default_rng(40 + r)
    shapes = ((TH - 1, TW + 1), (TH, TW), (TH + 1, TW - 1), (2 * TH + 1, TW), (TH, 2 * TW + 1), (9, 11))
    case = list(random_case(rng, shapes, 3))
    case[0] = smooth_images(rng, shapes)
    maps = assert_equal_to_reference(case, r, what=f"r={r}")
    assert len(maps.views) == 5
    for name in ("keep", "n_consistent", "plane"):                # the case is not a trivial one
        flat = np.concatenate([a.ravel() for a in getattr(maps, name)])
        assert 0.02 < (flat > 0).mean() < 0.98, name


@pytest.mark.parametrize("n_planes", [1, 2, 3, 33])
def test_plane_counts(gpu_ready, n_planes):
    rng = np.random.default_rng(50 + n_planes)
    shapes = ((13, 20), (14, 19), (12, 21))
    case = list(random_case(rng, shapes, n_planes))
    case[0] = smooth_images(rng, shapes)
    maps = assert_equal_to_reference(case, 2, what=f"D={n_planes}")
    if n_planes == 33:                                            # the sub-plane step is taken and skipped
        moved = np.concatenate([(maps.depth[v] != case[4][v][maps.plane[v]].astype(np.float32)).ravel() for v in range(2)])
        assert 0.05 < moved.mean() < 0.999


def test_zero_one_and_eight_sources(gpu_ready):
    rng = np.random.default_rng(60)
    shapes = [(10, 12)] * 9
    images = smooth_images(rng, shapes)
    refs = [0, 1, 2]
    sources = [[], [0], [0, 1, 3, 4, 5, 6, 7, 8]]
    warps = [np.stack([random_warp(rng, 12) for _ in s]).reshape(-1, 12) if s else np.zeros((0, 12)) for s in sources]
    planes = [np.sort(rng.uniform(1.0, 6.0, 5)) for _ in refs]
    backproj = [rng.normal(size=12) for _ in refs]
    maps = assert_equal_to_reference((images, refs, sources, warps, planes, backproj), 4, what="sources")
    assert (maps.plane[0] == 0).all() and (maps.cost[0] == 0).all()                   # no source: S_k = 0, best = 0
    assert maps.cost[2].max() > 255                                                   # eight sources over 81 pixels


def test_images_smaller_than_the_window(gpu_ready):
    rng = np.random.default_rng(61)
    for shapes in (((2, 3), (3, 2), (1, 1)), ((1, 1), (1, 1)), ((1, 40), (35, 1), (2, 2))):
        for r in (0, 4):
            case = random_case(rng, shapes, 3)
            assert_equal_to_reference(case, r, what=f"{shapes} r={r}")


def test_out_of_view_behind_and_nan_warps(gpu_ready):
    rng = np.random.default_rng(62)
    shapes = ((TH + 2, TW + 3), (12, 17), (15, 15))
    for kinds in (("out",), ("behind",), ("nan",), ("near", "out", "behind", "nan")):
        case = list(random_case(rng, shapes, 4, kinds))
        case[0] = smooth_images(rng, shapes)
        maps = assert_equal_to_reference(case, 1, what=str(kinds))
        if kinds in (("out",), ("behind",)):
            assert all((c == 24 * 2 * 9).all() for c in maps.cost) and all((p == 0).all() for p in maps.plane)
            assert all((n == 0).all() for n in maps.n_consistent)


def test_constant_and_two_level_images(gpu_ready):
    """Ties between planes (the lowest wins) and den <= 0 (no sub-plane step)."""
    rng = np.random.default_rng(63)
    shapes = ((TH + 1, TW + 1),) * 3
    ident = np.array([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])
    shift = lambda b: ident + np.array([0, 0, 0, b, 0, 0, 0, 0, 0, 0, 0, 0.0])
    case = list(random_case(rng, shapes, 5, constant=True))
    case[3] = [np.stack([ident, ident]) for _ in case[1]]                             # every sample valid: every S_k is 0
    maps = assert_equal_to_reference(case, 2, what="constant")
    for v in range(2):
        assert (maps.plane[v] == 0).all() and (maps.cost[v] == 0).all() and (maps.depth[v] == np.float32(case[4][v][0])).all()
    case[3] = [np.stack([shift(2.0), shift(-3.0)]) for _ in case[1]]                  # samples leave the source at the near planes
    maps = assert_equal_to_reference(case, 2, what="constant, shifted")
    assert any((p > 0).any() for p in maps.plane)
    case[0] = [(rng.random(s) < 0.5).astype(np.uint8) * 200 for s in shapes]
    maps = assert_equal_to_reference(case, 1, what="two levels")
    blocks = [np.kron((rng.random((s[0] // 4 + 1, s[1] // 4 + 1)) < 0.5), np.ones((4, 4)))[:s[0], :s[1]].astype(np.uint8) * 90 for s in shapes]
    case[0] = blocks
    maps = assert_equal_to_reference(case, 0, what="two-level blocks")
    flat = np.concatenate([(maps.depth[v] == case[4][v][maps.plane[v]].astype(np.float32)).ravel() for v in range(2)])
    assert flat.mean() > 0.2                                      # flat stretches of S: den <= 0, the plane's own depth


def test_a_view_alone_and_in_a_batch_and_twice(gpu_ready):
    rng = np.random.default_rng(64)
    shapes = ((TH + 3, TW + 5), (20, 31), (17, 40), (11, 13))
    images = smooth_images(rng, shapes)
    _, refs, sources, warps, planes, backproj = random_case(rng, shapes, 6)
    batch = device_maps(images, refs, sources, warps, planes, backproj, 2).filter(0.3, 24.0, 1)
    again = device_maps(images, refs, sources, warps, planes, backproj, 2).filter(0.3, 24.0, 1)
    names = ("plane", "cost", "depth", "n_consistent", "keep", "xyz")
    for name in names:
        for v in range(len(refs)):
            assert getattr(batch, name)[v].tobytes() == getattr(again, name)[v].tobytes(), name
    # view 1 alone, in a call of its own: the sweep's bytes do not depend on the rest of the batch.  The filter's do - the
    # sources lose their depth maps - so the filter is compared where it cannot: with every view present but reordered.
    alone = device_maps(images, [refs[1]], [sources[1]], [warps[1]], [planes[1]], [backproj[1]], 2)
    for name in ("plane", "cost", "depth"):
        assert getattr(alone, name)[0].tobytes() == getattr(batch, name)[1].tobytes(), name
    order = [2, 0, 1]
    pick = lambda a: [a[k] for k in order]
    moved = device_maps(images, pick(refs), pick(sources), pick(warps), pick(planes), pick(backproj), 2).filter(0.3, 24.0, 1)
    for name in names:
        for k, v in enumerate(order):
            assert getattr(moved, name)[k].tobytes() == getattr(batch, name)[v].tobytes(), name


def test_default_scene_end_to_end(gpu_ready):
    """depth_maps -> filter -> point_cloud on the default scene: the restatement's bytes, and the kept points within one
    plane spacing of the true surface for the share tests/test_depth_reference.py states (less the same two points)."""
    from sfm_amd import depth_maps
    s = dr.default_scene()
    refs, sources, warps, backproj, planes = default_views(s)
    maps = depth_maps(s.images, s.K, s.poses, {r: src for r, src in zip(refs, sources)}, {r: planes for r in refs}, radius=2)
    want = dr.sweep(s.images, refs, sources, warps, [planes] * 3, 2)
    for v in range(3):
        for got, ref in zip((maps.plane[v], maps.cost[v], maps.depth[v]), want[v]):
            assert got.dtype == ref.dtype and np.array_equal(bits(got), bits(ref))
    for mc, share in ((1, 0.9985), (2, 0.9995)):
        maps.filter(rel_tol=0.02, max_cost=12.0, min_consistent=mc)
        wantf = dr.filter_views(s.images, refs, sources, warps, backproj, want, 0.02, maps.cost_limits(12.0), mc)
        for v in range(3):
            for got, ref in zip((maps.n_consistent[v], maps.keep[v], maps.xyz[v]), wantf[v]):
                assert got.dtype == ref.dtype and np.array_equal(bits(got), bits(ref))
        pts, index = maps.point_cloud()
        keep = np.concatenate([k.ravel() for k in maps.keep]).astype(bool)
        assert len(pts) == keep.sum() and pts.tobytes() == np.concatenate([x.reshape(-1, 3) for x in maps.xyz])[keep].tobytes()
        assert (np.diff(index[:, 0]) >= 0).all() and np.array_equal(index[index[:, 0] == 1][:, 1:], np.argwhere(maps.keep[1]))
        # the cameras look down +z from z = 0: a point's z is its depth; one plane spacing in inverse depth
        truth = np.stack(s.depth)[index[:, 0], index[:, 1], index[:, 2]]
        spacing = abs(np.diff(1.0 / planes)[0])
        near = np.abs(1.0 / pts[:, 2] - 1.0 / truth) <= spacing
        assert near.mean() >= share - 0.02, (mc, near.mean())
        _, _, col = maps.point_cloud(colors=s.images)
        assert np.array_equal(col, np.stack(s.images)[index[:, 0], index[:, 1], index[:, 2]])
    assert quality()[1] >= 0.9899 - 0.02


def test_dense_from_reconstruction(gpu_ready):
    """The chain from a `Reconstruction`.  The loop scene of the incremental tests is a cloud of points in a cube seen by
    pixel coordinates only - it has no surface to render images of - so the default scene stands in, with a Reconstruction
    built from its true cameras and a sparse set of its surface points."""
    from sfm_amd import Reconstruction, Tracks, dense_from_reconstruction, depth_ranges, select_sources
    s = dr.default_scene()
    ys, xs = np.mgrid[4:72:8, 4:96:8]
    ys, xs = ys.ravel(), xs.ravel()
    z = s.depth[1][ys, xs]
    X = np.stack([(xs - s.K[0, 2]) / s.K[0, 0] * z, (ys - s.K[1, 2]) / s.K[1, 1] * z, z], axis=1)      # camera 1 sits at the origin
    n = len(X)
    kp = []
    for i in range(3):
        q = (X + s.poses[i][1]) @ s.K.T
        kp.append(q[:, :2] / q[:, 2:])
    tracks = Tracks(np.arange(4) * n, np.arange(n + 1) * 3, np.tile(np.arange(3), n), np.repeat(np.arange(n), 3))
    rec = Reconstruction(tracks, np.concatenate(kp), s.K)
    rec.poses, rec.order, rec.unregistered = dict(s.poses), [1, 0, 2], []
    rec.X, rec.has_point = X, np.ones(n, bool)
    assert select_sources(rec, 4) == {0: [1, 2], 1: [0, 2], 2: [0, 1]}
    rng = depth_ranges(rec, 0.2)
    assert all(abs(rng[i][0] - 0.8 * s.z_front) < 1e-9 and abs(rng[i][1] - 1.2 * s.z_back) < 1e-9 for i in range(3))
    pts, index, maps = dense_from_reconstruction(rec, s.images, rel_tol=0.02, max_cost=12.0, min_consistent=1)
    assert len(pts) > int(rec.has_point.sum()) and len(pts) > 0.5 * 3 * 96 * 72
    assert maps.views == [0, 1, 2] and index.shape == (len(pts), 3)
    truth = np.stack(s.depth)[index[:, 0], index[:, 1], index[:, 2]]
    assert (np.abs(pts[:, 2] - truth) < 0.25).mean() > 0.95


def test_entry_points_reject_bad_arguments(gpu_ready):
    """SFM_ERR_ARG (-1) before any device work: the outputs are null pointers throughout, so a call that got as far as a
    launch would not return -1 but fault."""
    import ctypes as C
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    i32, i64 = (lambda *v: np.array(v, dtype=np.int32)), (lambda *v: np.array(v, dtype=np.int64))
    good = dict(off=i64(0, 12, 40), hs=i32(3, 4), ws=i32(4, 7), n_img=2, n_ref=2, refs=i32(0, 1), src_ptr=i64(0, 1, 2), src=i32(1, 0),
                plane_ptr=i64(0, 3, 6), radius=2, ws_bytes=1 << 20)
    bad = [dict(off=i64(0, 12, 11)), dict(off=i64(0, 11, 40)), dict(ws=i32(4, 8)), dict(refs=i32(0, 2)), dict(refs=i32(-1, 1)),
           dict(refs=i32(1, 1)), dict(src=i32(1, 1)), dict(src=i32(1, 2)), dict(src_ptr=i64(0, 9, 9), src=i32(*([1] * 9))),
           dict(radius=5), dict(radius=-1), dict(plane_ptr=i64(0, 0, 3)), dict(plane_ptr=i64(0, 1025, 1026)), dict(ws_bytes=64),
           dict(n_ref=3)]

    def sweep(a):
        return lib.sfm_depth_sweep(h._h, None, hp(a["off"]), hp(a["hs"]), hp(a["ws"]), a["n_img"], a["n_ref"], hp(a["refs"]), hp(a["src_ptr"]),
                                   hp(a["src"]), None, hp(a["plane_ptr"]), None, a["radius"], None, None, None, C.c_void_p(1), a["ws_bytes"])

    def filt(a):
        return lib.sfm_depth_filter(h._h, hp(a["off"]), hp(a["hs"]), hp(a["ws"]), a["n_img"], a["n_ref"], hp(a["refs"]), hp(a["src_ptr"]),
                                    hp(a["src"]), None, None, None, None, None, 0.01, 2, None, None, None, C.c_void_p(1), a["ws_bytes"])

    def census(a):
        return lib.sfm_depth_census(h._h, None, hp(a["off"]), hp(a["hs"]), hp(a["ws"]), a["n_img"], None, C.c_void_p(1), a["ws_bytes"])
    # the good call gets through every check on sizes and indices and is stopped by its null data pointers, also -1 but
    # with another message: the bad ones must each name their own reason
    assert sweep(good) == -1 and b"null pointer" in lib.sfm_last_error(h._h)
    for kw in bad:
        a = dict(good, **kw)
        assert sweep(a) == -1 and b"null pointer" not in lib.sfm_last_error(h._h), kw
        if "radius" not in kw and "plane_ptr" not in kw:
            assert filt(a) == -1 and b"null pointer" not in lib.sfm_last_error(h._h), kw
    for kw in bad[:3] + [dict(ws_bytes=64)]:
        assert census(dict(good, **kw)) == -1 and b"null pointer" not in lib.sfm_last_error(h._h), kw
    assert lib.sfm_depth_filter(h._h, hp(good["off"]), hp(good["hs"]), hp(good["ws"]), 2, 2, hp(good["refs"]), hp(good["src_ptr"]), hp(good["src"]),
                                None, None, None, None, None, float("nan"), 2, None, None, None, C.c_void_p(1), 1 << 20) == -1
