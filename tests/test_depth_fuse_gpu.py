"""The fusion of the depth maps on the device against tests/depth_fuse_reference.py: every output byte - normal maps,
agree_mask, owner, pt_ptr, points, normals, n_views, index - on hand-made maps of a few hundred pixels, then the chain
from the sweep on the default scene and from a `Reconstruction`.

The float32 normals are compared bit for bit like everything else: sqrt and / in float64 are correctly rounded on the
device."""
import numpy as np
import pytest

import depth_fuse_reference as fr
import depth_reference as dr
from test_depth_fuse_reference import all_to_all, assert_same, check_properties, plane_case

pytestmark = pytest.mark.gpu


def device_fuse(case, rel_tol, step, jump):
    """The two device calls on hand-made depth / keep / xyz, uploaded as they are."""
    from sfm_amd import depth_maps_from_arrays
    shapes, refs, sources, warps, backproj, depth, keep, xyz = case
    src_ptr = np.cumsum([0] + [len(s) for s in sources]).astype(np.int64)
    src_image = np.array([s for src in sources for s in src], dtype=np.int32)
    W = np.concatenate([np.asarray(w).reshape(-1, 12) for w in warps]) if len(src_image) else np.zeros((0, 12))
    maps = depth_maps_from_arrays(shapes, refs, src_ptr, src_image, W, np.asarray(backproj, dtype=np.float64).reshape(-1, 12), depth, keep, xyz)
    return maps.fuse(rel_tol=rel_tol, normal_step=step, normal_jump=jump)


def assert_equal_to_reference(case, rel_tol=0.01, step=2, jump=0.05, what=""):
    got = device_fuse(case, rel_tol, step, jump)
    want = fr.fuse(*case, rel_tol, step, jump)
    assert len(got) == len(want.points)
    assert_same(got, want, what)
    return got, want


@pytest.mark.parametrize("step", [1, 4])
def test_sizes_around_the_wavefront_and_the_block(gpu_ready, step):
    """Pixel counts of 1, 63, 64, 65, 255, 256, 257 and 2 x 256 + 1, widths of 1, 2 and twice the step, three images of
    different sizes in every batch, every view a reference with the other two as sources."""
    rng = np.random.default_rng(70 + step)
    batches = ((((1, 1), (7, 9), (8, 8)), None), (((5, 13), (15, 17), (16, 16)), None), (((1, 257), (19, 27), (257, 1)), 30.0),
               (((9, 1), (9, 2), (9, 2 * step)), None), (((16, 16), (16, 16), (2, 128)), 24.0))
    n_normals = n_partners = 0
    for shapes, f in batches:
        refs, sources = all_to_all(3)
        case = plane_case(rng, shapes, refs, sources, ("random", "ones", "checker"), f=f)
        got, want = assert_equal_to_reference(case, step=step, what=f"{shapes} step={step}")
        check_properties(case, got, 0.01)
        n_normals += int(want.normals.any(axis=1).sum())
        n_partners += int((want.n_views > 1).sum())
    assert n_normals > 100 and n_partners > 100                   # the batches are not trivial ones


def test_zero_one_and_eight_sources_and_views_out_of_image_order(gpu_ready):
    """Views listed against the image order (the position decides who owns a point), a view without a source, one with one,
    one with eight of which five have no maps of their own."""
    rng = np.random.default_rng(72)
    shapes = ((10, 12),) * 9
    refs = [4, 0, 2, 1]
    sources = [[], [4], [0, 1, 3, 4, 5, 6, 7, 8], [2, 0, 8]]
    case = plane_case(rng, shapes, refs, sources, f=40.0)
    got, want = assert_equal_to_reference(case, what="sources")
    check_properties(case, got, 0.01)
    assert (want.agree_mask[0] == 0).all() and want.n_views.max() >= 2
    assert (want.agree_mask[2] & 0b11110100 == 0).all() and (want.agree_mask[2] & 0b00001011).any()      # entries 2, 4 .. 7 have no maps
    assert ((case[6][1] != 0) & (want.owner[1] == 0)).any() and ((case[6][2] != 0) & (want.owner[2] == 0)).any()


def test_no_owner_and_every_pixel_an_owner(gpu_ready):
    rng = np.random.default_rng(73)
    shapes = ((17, 16), (16, 17), (9, 30))
    refs, sources = all_to_all(3)
    case = plane_case(rng, shapes, refs, sources, ("zero",))
    got, want = assert_equal_to_reference(case, what="keep all zero")
    assert len(got) == 0 and got.points.shape == (0, 3) and got.pt_ptr.tolist() == [0, 0, 0, 0]
    assert all((m == 0).all() for m in got.agree_mask)
    assert any(nm.any() for nm in got.view_normals)               # keep plays no part in the normal maps
    # kept everywhere, and nothing agrees: a tolerance of zero on perturbed depths
    case = plane_case(rng, shapes, refs, sources, ("ones",), bad=0.0)
    got, want = assert_equal_to_reference(case, rel_tol=0.0, what="every pixel an owner")
    n = sum(h * w for h, w in shapes)
    assert len(got) == n and (got.n_views == 1).all() and got.pt_ptr[-1] == n
    # kept everywhere and the views agree widely: view 0 owns all of its pixels, the others what it does not see
    got, want = assert_equal_to_reference(case, rel_tol=0.5, jump=10.0, what="wide agreement")
    assert got.pt_ptr[1] == 17 * 16 and len(got) < 0.75 * n
    # no view at all, and views without a pixel
    got, want = assert_equal_to_reference(([(3, 3)], [], [], [], [], [], [], []), what="no view")
    assert len(got) == 0 and got.pt_ptr.tolist() == [0]
    case = plane_case(rng, ((0, 5), (4, 4), (3, 0)), [0, 1, 2], [[1], [0, 2], [1]], ("ones",))
    got, want = assert_equal_to_reference(case, what="empty images")
    assert got.pt_ptr.tolist() == [0, 0, 16, 16]


def test_nan_warp_and_source_behind_the_camera(gpu_ready):
    rng = np.random.default_rng(74)
    shapes = ((14, 19), (15, 18), (13, 20))
    refs, sources = all_to_all(3)
    for v, e, kind in ((1, 0, "nan"), (2, 1, "behind"), (0, 1, "nan")):
        case = plane_case(rng, shapes, refs, sources, break_warp=(v, e, kind))
        got, want = assert_equal_to_reference(case, what=f"{kind} warp of view {v}")
        assert ((want.agree_mask[v] >> e) & 1 == 0).all() and ((want.agree_mask[v] >> (1 - e)) & 1).any()


def test_the_same_call_twice_and_a_batch_of_many_blocks(gpu_ready):
    """300 x 300 is 352 blocks a view and 1,053 in the batch: more than one chunk of 1,024 block counts for the two-level
    scan, more than one block per view and blocks whose owners start in the middle of the output."""
    rng = np.random.default_rng(75)
    shapes = ((300, 300), (296, 301), (290, 310))
    assert sum(-(-h * w // 256) for h, w in shapes) > 1024
    refs, sources = all_to_all(3)
    case = plane_case(rng, shapes, refs, sources, ("random", "checker", "ones"))
    a, want = assert_equal_to_reference(case, what="many blocks")
    b = device_fuse(case, 0.01, 2, 0.05)
    for name in ("points", "normals", "n_views", "index"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    for name in ("view_normals", "agree_mask", "owner"):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(getattr(a, name), getattr(b, name))), name
    assert a.pt_ptr.tobytes() == b.pt_ptr.tobytes() and 0.3 * len(want.points) < want.pt_ptr[1] < len(want.points)


def test_default_scene_end_to_end(gpu_ready):
    """depth_maps -> filter -> fuse on the default scene: the restatement's bytes on the device's own maps (which
    tests/test_depth_gpu.py holds against the restatement of the sweep and the filter), the fused share of the table in
    README, colours, and the untouched point_cloud()."""
    from sfm_amd import depth as dm
    from sfm_amd import depth_maps
    s = dr.default_scene()
    refs, sources = all_to_all(3)
    warps = [dm.view_warps(s.K, s.poses, r, src) for r, src in zip(refs, sources)]
    backproj = [dm.view_backprojection(s.K, s.poses, r) for r in refs]
    planes = {r: dm.plane_depths(s.d_min, s.d_max, warps[r], s.size) for r in refs}
    maps = depth_maps(s.images, s.K, s.poses, {r: src for r, src in zip(refs, sources)}, planes, radius=2)
    shapes = [a.shape for a in s.images]
    for mc, share in ((1, 0.385), (2, 0.336)):
        maps.filter(rel_tol=0.02, max_cost=12.0, min_consistent=mc)
        before = maps.point_cloud()
        cloud = maps.fuse()                                       # rel_tol of the filter
        want = fr.fuse(shapes, refs, sources, warps, backproj, maps.depth, maps.keep, maps.xyz, 0.02, 2, 0.05)
        assert_same(cloud, want, f"min_consistent={mc}")
        kept = sum(int(k.sum()) for k in maps.keep)
        assert len(cloud) == len(want.points) and abs(len(cloud) / kept - share) <= 0.02
        assert np.array_equal(cloud.colors(s.images), np.stack(s.images)[want.index[:, 0], want.index[:, 1], want.index[:, 2]])
        after = maps.point_cloud()
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and len(after[0]) == kept
    with pytest.raises(ValueError):
        cloud.colors(s.images[:2])


def test_dense_from_reconstruction_fused(gpu_ready):
    """The chain from a `Reconstruction` with fuse=True, on the scene of tests/test_depth_gpu.py::test_dense_from_reconstruction:
    (FusedCloud, DepthMaps), fewer points than kept pixels, on the surface, with normals that look at the cameras; and with
    fuse=False what it returned before."""
    from sfm_amd import FusedCloud, Reconstruction, Tracks, dense_from_reconstruction
    s = dr.default_scene()
    ys, xs = np.mgrid[4:72:8, 4:96:8]
    ys, xs = ys.ravel(), xs.ravel()
    z = s.depth[1][ys, xs]
    X = np.stack([(xs - s.K[0, 2]) / s.K[0, 0] * z, (ys - s.K[1, 2]) / s.K[1, 1] * z, z], axis=1)
    n = len(X)
    kp = []
    for i in range(3):
        q = (X + s.poses[i][1]) @ s.K.T
        kp.append(q[:, :2] / q[:, 2:])
    tracks = Tracks(np.arange(4) * n, np.arange(n + 1) * 3, np.tile(np.arange(3), n), np.repeat(np.arange(n), 3))
    rec = Reconstruction(tracks, np.concatenate(kp), s.K)
    rec.poses, rec.order, rec.unregistered = dict(s.poses), [1, 0, 2], []
    rec.X, rec.has_point = X, np.ones(n, bool)
    cloud, maps = dense_from_reconstruction(rec, s.images, rel_tol=0.02, max_cost=12.0, min_consistent=1, fuse=True)
    assert isinstance(cloud, FusedCloud) and maps.views == [0, 1, 2]
    kept = sum(int(k.sum()) for k in maps.keep)
    # three views of one surface: duplicates are gone, and no point can stand for many more pixels than there are views
    assert kept / 4 < len(cloud) < kept and cloud.points.shape == (len(cloud), 3) and cloud.index.shape == (len(cloud), 3)
    truth = np.stack(s.depth)[cloud.index[:, 0], cloud.index[:, 1], cloud.index[:, 2]]
    assert (np.abs(cloud.points[:, 2] - truth) < 0.25).mean() > 0.95
    has = cloud.normals.any(axis=1)
    assert has.mean() > 0.9 and (cloud.normals[has][:, 2] < 0).mean() > 0.99 and np.median(cloud.normals[has][:, 2]) < -0.99
    pts, index, maps2 = dense_from_reconstruction(rec, s.images, rel_tol=0.02, max_cost=12.0, min_consistent=1)
    assert len(pts) == kept and index.shape == (kept, 3) and index.dtype == np.int64


def test_entry_points_reject_bad_arguments(gpu_ready):
    """SFM_ERR_ARG (-1) before any device work: the data pointers are null throughout, so a call that got as far as a launch
    would not return -1 but fault."""
    import ctypes as C
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    i32, i64 = (lambda *v: np.array(v, dtype=np.int32)), (lambda *v: np.array(v, dtype=np.int64))
    good = dict(off=i64(0, 12, 40), hs=i32(3, 4), ws=i32(4, 7), n_img=2, n_ref=2, refs=i32(0, 1), src_ptr=i64(0, 1, 2), src=i32(1, 0),
                rel_tol=0.01, step=2, jump=0.05, n_points=5, ws_bytes=1 << 20)
    bad_views = [dict(off=i64(0, 12, 11)), dict(off=i64(0, 11, 40)), dict(ws=i32(4, 8)), dict(refs=i32(0, 2)), dict(refs=i32(-1, 1)),
                 dict(refs=i32(1, 1)), dict(src=i32(1, 1)), dict(src=i32(1, 2)), dict(src_ptr=i64(0, 9, 9), src=i32(*([1] * 9))),
                 dict(ws_bytes=64), dict(n_ref=3)]
    bad_mark = [dict(step=0), dict(step=5), dict(step=-1), dict(jump=-0.01), dict(jump=float("nan")), dict(rel_tol=-0.01),
                dict(rel_tol=float("nan"))]
    bad_gather = [dict(n_points=-1), dict(n_points=41)]

    def mark(a):
        return lib.sfm_depth_fuse_mark(h._h, hp(a["off"]), hp(a["hs"]), hp(a["ws"]), a["n_img"], a["n_ref"], hp(a["refs"]), hp(a["src_ptr"]),
                                       hp(a["src"]), None, None, None, None, None, a["rel_tol"], a["step"], a["jump"], None, None, None,
                                       C.c_void_p(1), C.c_void_p(1), a["ws_bytes"])

    def gather(a):
        return lib.sfm_depth_fuse_gather(h._h, hp(a["off"]), hp(a["hs"]), hp(a["ws"]), a["n_img"], a["n_ref"], hp(a["refs"]), hp(a["src_ptr"]),
                                         hp(a["src"]), None, None, None, None, None, None, None, a["n_points"], None, None, None, None,
                                         C.c_void_p(1), a["ws_bytes"])
    # the good calls get through every check on sizes, indices and parameters and are stopped by their null data pointers, also
    # -1 but with another message: the bad ones must each name their own reason
    assert mark(good) == -1 and b"null pointer" in lib.sfm_last_error(h._h)
    assert gather(good) == -1 and b"null pointer" in lib.sfm_last_error(h._h)
    for kw in bad_views + bad_mark:
        assert mark(dict(good, **kw)) == -1 and b"null pointer" not in lib.sfm_last_error(h._h), kw
    for kw in bad_views + bad_gather:
        assert gather(dict(good, **kw)) == -1 and b"null pointer" not in lib.sfm_last_error(h._h), kw
    assert gather(dict(good, n_points=0)) == 0                    # nothing to gather: returns at once
    need = C.c_int64()
    assert lib.sfm_depth_fuse_workspace_bytes(2, 2, 2, 40, C.byref(need)) == 0 and 0 < need.value < (1 << 20)
