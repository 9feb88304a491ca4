"""sfm_triangulate_tracks on the device against the NumPy restatement (tests/triangulate_reference.py).  The scenes are small:
12 cameras on an arc looking at the unit cube, K as in StructureFromMotion, pixel noise 0.5.

The tolerance on X and max_err is not a constant: a test measures the largest relative deviation of the float64 reference
from its np.longdouble run on the same inputs and allows the device 100 times that (a different but equally valid order
of operations; the 80-bit run stands in for the exact value).  The reference's side of that pair on the parity scene of 2,000
tracks (largest relative deviation, float64 against 80-bit): refine_iters=0: X 2.0e-15, max_err 5.1e-11; refine_iters=5: X 9.1e-15,
max_err 1.8e-11.  Every test prints both sides of its pair.

This is parity with a restatement: a weakness of the algorithm itself passes, because the reference has it too.  The sharper
statement - the device against a 60-digit truth of the problem, on scenes beyond this arc - is tests/test_geometry_truth_gpu.py.
"""
import functools

import numpy as np
import pytest

import triangulate_reference as tr
from test_triangulate_reference import flat, rel_dev_points, rel_dev_scalars, status_cases

pytestmark = pytest.mark.gpu

GATES = dict(min_views=2, max_error=4.0, min_angle_deg=1.0)


def device(args, **opts):
    from sfm_amd import triangulate_tracks_raw
    return triangulate_tracks_raw(*args, **opts)


def take_tracks(g, order):
    """The tracks `order` of (kp_ptr, kp_xy, track_ptr, obs_image, obs_kp), in that order; the keypoints stay."""
    kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = g
    idx = [np.arange(track_ptr[t], track_ptr[t + 1]) for t in order]
    sel = np.concatenate(idx).astype(np.int64) if len(idx) else np.zeros(0, np.int64)
    ptr = np.concatenate([[0], np.cumsum([len(i) for i in idx])]).astype(np.int64)
    return kp_ptr, kp_xy, ptr, obs_image[sel], obs_kp[sel]


def assert_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    for k in ("status", "n_views"):
        assert np.array_equal(a[k][rows_a], b[k][rows_b]), k
    for k in ("X", "max_err"):
        assert np.array_equal(a[k][rows_a].view(np.int64), b[k][rows_b].view(np.int64)), k


def assert_parity(args, what, **opts):
    """status, n_views and counts equal the reference's; X and max_err within 100 x the reference's own float64-vs-80-bit
    deviation on these inputs.  Returns (device output, reference)."""
    ref = tr.triangulate(*args, **opts)
    ld = tr.triangulate(*args, dtype=np.longdouble, **opts)
    out = device(args, **opts)
    assert np.array_equal(ld["status"], ref["status"])
    assert out["status"].dtype == np.int32 and out["n_views"].dtype == np.int32 and out["counts"].dtype == np.int64
    assert np.array_equal(out["status"], ref["status"]), (what, np.flatnonzero(out["status"] != ref["status"])[:5])
    assert np.array_equal(out["n_views"], ref["n_views"]) and np.array_equal(out["counts"], ref["counts"])
    ref_x, ref_e = rel_dev_points(ref["X"], ld["X"]), rel_dev_scalars(ref["max_err"], ld["max_err"])
    dev_x, dev_e = rel_dev_points(out["X"], ref["X"]), rel_dev_scalars(out["max_err"], ref["max_err"])
    print(f"{what}: reference float64 against 80-bit X {ref_x:.3g}, max_err {ref_e:.3g}; "
          f"device against reference X {dev_x:.3g}, max_err {dev_e:.3g}")
    assert dev_x <= 100 * ref_x and dev_e <= 100 * ref_e
    return out, ref


# ------------------------------------------------------------------------------------------------------------ parity
@functools.lru_cache(maxsize=None)
def parity_scene():
    rng = np.random.default_rng(11)
    proj = tr.arc_cameras(12)[0]
    X = rng.uniform(0, 1, (2000, 3))
    lengths = rng.integers(2, 13, 2000)
    return flat(proj, tr.make_tracks(rng, proj, X, lengths, noise=0.5))


@functools.lru_cache(maxsize=None)
def parity_device(iters):
    return device(parity_scene(), refine_iters=iters, **GATES)


@pytest.mark.parametrize("iters", [0, 5])
def test_parity_with_the_reference(gpu_ready, iters):
    args = parity_scene()
    out, ref = assert_parity(args, f"parity scene, refine_iters={iters}", refine_iters=iters, **GATES)
    assert ref["counts"][tr.OK] == 2000 and ref["n_views"].min() == 2 and ref["n_views"].max() == 12
    assert_bits(out, parity_device(iters))                                  # and the same bits from a second call


# ----------------------------------------------------------------------------------------------------------- the gates
@functools.lru_cache(maxsize=None)
def gate_scene():
    """60 tracks per class, every gate quantity far from its threshold (max_error 4 px, min_angle 1 degree):
    ok (errors under 0.8 px, adjacent cameras 10 degrees apart), too few views (one registered image), NaN pixel, behind
    (a point mirrored through the camera ring), low angle (points 6,000 units away, pixel noise 0.01 so that the depth stays clearly signed: 0.1 degrees across the
    whole arc), high error (one view moved by 100 px across the epipolar lines).  Images 12 and 13 are not registered."""
    rng = np.random.default_rng(12)
    proj, _, _, centres = tr.arc_cameras(12)
    target = np.array([0.5, 0.5, 0.5])
    n = 60
    X, cams, noise, kind = [], [], [], []
    for k in range(6 * n):
        c = k % 6
        kind.append(c)
        p = rng.uniform(0, 1, 3)
        m = int(rng.integers(2, 9))
        view = np.sort(rng.choice(12, m, replace=False))
        nz = 0.5
        if c == 1:
            view = np.concatenate([view[:1], [12, 13]])
        elif c == 3:
            mid = centres[int(rng.integers(4, 8))]
            p = target + 2.0 * (mid - target) + rng.uniform(-0.3, 0.3, 3)
            view = np.sort(rng.choice(np.arange(2, 10), min(m, 6), replace=False))
        elif c == 4:
            d = target - centres[int(rng.integers(4, 8))]                   # in front of every camera of the arc
            p, nz = target + 6000.0 * d / np.linalg.norm(d), 0.01
        elif c == 5:
            view = np.sort(rng.choice(12, max(m, 3), replace=False))
        X.append(p); cams.append(view); noise.append(nz)
    proj14 = np.concatenate([proj, proj[:2]])                                 # images 12, 13 project somewhere; they have no camera
    g = tr.make_tracks(rng, proj14, np.asarray(X), None, noise=np.asarray(noise), cams=cams, uniform=True)
    kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = g
    kind = np.asarray(kind)
    for t in np.flatnonzero(kind == 2):                                        # a NaN pixel in some view
        o = track_ptr[t] + int(rng.integers(0, track_ptr[t + 1] - track_ptr[t]))
        kp_xy[kp_ptr[obs_image[o]] + obs_kp[o], int(rng.integers(0, 2))] = np.nan
    for t in np.flatnonzero(kind == 5):                                        # one view moved by 100 px in y
        o = track_ptr[t] + int(rng.integers(0, track_ptr[t + 1] - track_ptr[t]))
        kp_xy[kp_ptr[obs_image[o]] + obs_kp[o], 1] += 100.0
    cam_of_image = np.concatenate([np.arange(12), [-1, -1]]).astype(np.int32)
    return (proj.reshape(-1, 12), cam_of_image) + g, kind


@pytest.mark.parametrize("iters", [0, 5])
def test_gates_on_inputs_far_from_every_threshold(gpu_ready, iters):
    args, kind = gate_scene()
    opts = dict(refine_iters=iters, **GATES)
    ref = tr.triangulate(*args, **opts)
    # the reference's own values first: nothing within 1e-6 relative of a threshold, and the deciding ones far from it
    live = ref["status"] >= tr.BEHIND
    live |= ref["status"] == tr.OK
    err, depth, cos = tr.gate_quantities(*args, np.where(live[:, None], ref["X"], 0.0))
    err, depth, cos = err[live], depth[live], cos[live]
    with np.errstate(invalid="ignore"):
        assert not (np.abs(err - 4.0) <= 4e-6).any() and not (np.abs(depth) <= 1e-6).any()
        cos_min = np.cos(np.deg2rad(1.0))
        assert not (np.abs(cos - cos_min) <= 1e-6 * cos_min).any()
        worst = np.nanmax(err, axis=1)
        assert ((worst < 2.0) | (worst > 20.0)).all(), worst[(worst >= 2.0) & (worst <= 20.0)]
        near, far = np.nanmin(np.abs(depth), axis=1), np.nanmax(np.abs(depth), axis=1)
        assert (near > 0.5).all() and ((np.nanmin(depth, axis=1) > 0) | (np.nanmax(depth, axis=1) < 0)).all(), (near, far)
        widest = np.rad2deg(np.arccos(np.clip(np.nanmin(cos.reshape(len(cos), -1), axis=1), -1, 1)))
        assert ((widest < 0.2) | (widest > 5.0)).all(), widest[(widest >= 0.2) & (widest <= 5.0)]
    want = np.array([tr.OK, tr.TOO_FEW_VIEWS, tr.DEGENERATE, tr.BEHIND, tr.LOW_ANGLE, tr.HIGH_ERROR])[kind]
    assert np.array_equal(ref["status"], want), np.flatnonzero(ref["status"] != want)
    out, _ = assert_parity(args, f"gate scene, refine_iters={iters}", **opts)          # every track, none excluded
    assert out["counts"].tolist() == [60] * 6
    dead = (want == tr.TOO_FEW_VIEWS) | (want == tr.DEGENERATE)
    assert np.isnan(out["X"][dead]).all() and np.isnan(out["max_err"][dead]).all()
    assert np.isfinite(out["X"][~dead]).all() and np.isfinite(out["max_err"][~dead]).all()


def test_status_cases_one_per_code(gpu_ready):
    args, want, views = status_cases()
    out = device(args, refine_iters=5, **GATES)
    assert np.array_equal(out["status"], want) and np.array_equal(out["n_views"], views) and out["counts"].tolist() == [1] * 6
    assert device(args, refine_iters=5, min_angle_deg=0.0)["status"].tolist() == [0, 1, 2, 3, 0, 5]


# -------------------------------------------------------------------------------------------------- two-view contract
def test_two_view_tracks_are_sfm_triangulate2(gpu_ready):
    from sfm_amd import driver
    rng = np.random.default_rng(13)
    proj = tr.arc_cameras(12)[0]
    X = rng.uniform(0, 1, (700, 3))
    g = tr.make_tracks(rng, proj, X, np.full(700, 2), noise=0.5)
    g[1][::7] += 30.0                                                          # some fail the 4 px gate
    args = flat(proj, g)
    out = device(args, refine_iters=0, max_error=4.0, min_angle_deg=0.0)
    kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = g
    node = kp_ptr[obs_image] + obs_kp
    X2, valid, err = driver.triangulate_two_view(proj, obs_image[0::2], obs_image[1::2], kp_xy[node[0::2]], kp_xy[node[1::2]], 4.0)
    assert np.array_equal(out["X"].view(np.int64), X2.view(np.int64))
    assert np.array_equal(out["max_err"].view(np.int64), err.max(axis=1).view(np.int64))
    assert np.array_equal((out["status"] == tr.OK) | (out["status"] == tr.BEHIND), valid) and 0 < valid.sum() < 700
    assert set(out["status"].tolist()) <= {tr.OK, tr.BEHIND, tr.HIGH_ERROR}
    # the two-view tracks of a mixed batch take the same path
    pa = parity_scene()
    two = np.flatnonzero(np.diff(pa[4]) == 2)
    mixed = device(pa, refine_iters=0, max_error=4.0, min_angle_deg=0.0)
    node = pa[2][pa[5]] + pa[6]
    a, b = pa[4][two], pa[4][two] + 1
    X2, valid, err = driver.triangulate_two_view(pa[0].reshape(-1, 3, 4), pa[5][a], pa[5][b], pa[3][node[a]], pa[3][node[b]], 4.0)
    assert len(two) > 100 and np.array_equal(mixed["X"][two].view(np.int64), X2.view(np.int64))
    assert np.array_equal(mixed["max_err"][two].view(np.int64), err.max(axis=1).view(np.int64))


# ------------------------------------------------------------------------------------- shapes where a kernel goes wrong
@pytest.mark.parametrize("n_tracks", [0, 1, 255, 256, 257])
def test_track_counts_around_a_workgroup(gpu_ready, n_tracks):
    """The first n tracks alone give the bits they have inside the batch of 2,000 (which is held to the reference)."""
    args = parity_scene()
    sub = args[:2] + take_tracks(args[2:], np.arange(n_tracks))
    assert sub[4][-1] == len(sub[5])                                          # the last track ends exactly at n_obs
    out = device(sub, refine_iters=5, **GATES)
    assert out["X"].shape == (n_tracks, 3) and out["counts"].tolist() == [n_tracks, 0, 0, 0, 0, 0]
    assert_bits(out, parity_device(5), rows_b=slice(0, n_tracks))


@pytest.mark.parametrize("long_views", [63, 64, 65])
def test_short_tracks_beside_a_long_one(gpu_ready, long_views):
    """Tracks of 2 and 3 views next to one of 63 / 64 / 65 in the same wavefront (it repeats cameras, as a conflicting track
    kept under "keep" does), a track whose observations are all unregistered, an image without keypoints, and 300 tracks in
    all so that a second workgroup runs."""
    rng = np.random.default_rng(long_views)
    proj = tr.arc_cameras(12)[0]
    n = 300
    X = rng.uniform(0, 1, (n, 3))
    cams = [np.sort(rng.choice(12, int(rng.integers(2, 4)), replace=False)) for _ in range(n)]
    cams[5] = rng.integers(0, 12, long_views)
    cams[9] = np.array([3, 3, 3])                                             # three observations, all in image 3
    cams[n - 1] = rng.integers(0, 12, long_views)
    kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = tr.make_tracks(rng, proj, X, None, noise=0.5, cams=cams)
    # image 3 is not registered; image 4 is a new one without keypoints; the images behind it move up by one
    image_of = np.array([0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12])
    kp_ptr = np.concatenate([kp_ptr[:5], kp_ptr[4:]])                          # 13 images, image 4 empty
    obs_image = image_of[obs_image].astype(np.int32)
    cam_of_image = np.array([0, 1, 2, -1, -1, 4, 5, 6, 7, 8, 9, 10, 11], np.int32)
    args = (proj.reshape(-1, 12), cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp)
    assert kp_ptr[5] == kp_ptr[4] and track_ptr[-1] == len(obs_image)
    for iters in (0, 5):
        out, ref = assert_parity(args, f"long track of {long_views}, refine_iters={iters}", refine_iters=iters, **GATES)
        assert out["status"][9] == tr.TOO_FEW_VIEWS and out["n_views"][9] == 0
        assert out["n_views"][5] == long_views - int((cams[5] == 3).sum()) and out["status"][5] == tr.OK
        assert out["n_views"].max() >= 45 and (out["status"] == tr.TOO_FEW_VIEWS).sum() > 1


# ------------------------------------------------------------------------------------------------- batch independence
def test_a_track_does_not_depend_on_its_batch(gpu_ready):
    args = parity_scene()
    base = parity_device(5)
    order = np.random.default_rng(14).permutation(2000)
    out = device(args[:2] + take_tracks(args[2:], order), refine_iters=5, **GATES)
    assert_bits(out, base, rows_b=order)
    for part in (np.arange(0, 777), np.arange(777, 2000)):
        out = device(args[:2] + take_tracks(args[2:], part), refine_iters=5, **GATES)
        assert_bits(out, base, rows_b=part)


# --------------------------------------------------------------------------------------------------- degenerate inputs
def test_degenerate_tracks_fail_alone(gpu_ready):
    """The same camera twice with the same pixel, a NaN pixel, parallel rays (a point at infinity), a keypoint index outside
    its image: none is OK, nothing faults, and the tracks around them keep their bits."""
    rng = np.random.default_rng(15)
    proj = tr.arc_cameras(12)[0]
    P12 = proj[0].copy()
    P12[:, 3] += tr.K_SFM @ [1.0, 0.0, 0.0]                                    # camera 0 moved sideways: same pixel = parallel rays
    proj13 = np.concatenate([proj, P12[None]])
    n = 130
    X = rng.uniform(0, 1, (n, 3))
    cams = [np.sort(rng.choice(12, int(rng.integers(2, 7)), replace=False)) for _ in range(n)]
    bad = {3: "same", 64: "nan", 65: "parallel", 129: "index"}
    cams[3] = np.array([7, 7]); cams[65] = np.array([0, 12])
    kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = tr.make_tracks(rng, proj13, X, None, noise=0.5, cams=cams)
    node = lambda t, k: kp_ptr[obs_image[track_ptr[t] + k]] + obs_kp[track_ptr[t] + k]
    kp_xy[node(3, 1)] = kp_xy[node(3, 0)]
    kp_xy[node(64, 0), 0] = np.nan
    kp_xy[node(65, 1)] = kp_xy[node(65, 0)]
    obs_kp = obs_kp.copy()
    obs_kp[track_ptr[129]] = 10 ** 6
    args = (proj13.reshape(-1, 12), np.arange(13, dtype=np.int32), kp_ptr, kp_xy, track_ptr, obs_image, obs_kp)
    good = np.array([t for t in range(n) if t not in bad])
    for iters in (0, 5):
        out = device(args, refine_iters=iters, **GATES)
        assert (out["status"][list(bad)] != tr.OK).all(), out["status"][list(bad)]
        assert out["status"][64] == tr.DEGENERATE and out["status"][129] == tr.DEGENERATE
        assert (out["status"][good] == tr.OK).all() and out["counts"].sum() == n
        alone = device(args[:2] + take_tracks(args[2:], good), refine_iters=iters, **GATES)
        assert_bits(out, alone, rows_a=good)


def test_bad_options_and_small_workspace_are_rejected(gpu_ready):
    import ctypes as C
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p
    args = parity_scene()
    for bad in (dict(min_views=1), dict(refine_iters=-1), dict(max_error=-1.0), dict(min_angle_deg=-1.0), dict(max_error=np.nan)):
        with pytest.raises(ValueError):
            device(args, **bad)
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    need = C.c_int64()
    assert h.lib.sfm_triangulate_tracks_workspace_bytes(12, C.byref(need)) == 0 and need.value >= 12 * 24
    t = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in zip("pcktoiq", (args[0], args[1], args[2], args[3], args[4], args[5], args[6]))}
    X = torch.zeros((2000, 3), dtype=torch.float64, device=dev)
    st, nv = torch.zeros(2000, dtype=torch.int32, device=dev), torch.zeros(2000, dtype=torch.int32, device=dev)
    me, counts = torch.zeros(2000, dtype=torch.float64, device=dev), torch.full((6,), 7, dtype=torch.int64, device=dev)
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)

    def call(min_views=2, iters=5, ws_bytes=need.value, n_tracks=2000):
        return h.lib.sfm_triangulate_tracks(h._h, _p(t["p"]), 12, _p(t["c"]), 12, _p(t["k"]), _p(t["t"]), len(args[3]), _p(t["o"]),
                                            n_tracks, _p(t["i"]), _p(t["q"]), len(args[5]), min_views, iters, 4.0, 1.0, _p(X), _p(st),
                                            _p(nv), _p(me), _p(counts), _p(ws), ws_bytes)
    assert call(min_views=1) == -1 and b"min_views" in h.lib.sfm_last_error(h._h)
    assert call(iters=-1) == -1
    assert counts.tolist() == [7] * 6                                          # nothing ran
    assert call(ws_bytes=need.value - 1) == -3
    assert call(n_tracks=0) == 0 and counts.tolist() == [0] * 6
    assert call() == 0 and counts.tolist() == [2000, 0, 0, 0, 0, 0]


# ----------------------------------------------------------------------------------------------------- the public call
def test_public_call_validates_and_maps_cameras(gpu_ready):
    from sfm_amd import Tracks, triangulate_tracks
    args = parity_scene()
    proj, _, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = args
    T = Tracks(kp_ptr, track_ptr, obs_image, obs_kp)
    kps = [kp_xy[kp_ptr[i]:kp_ptr[i + 1]] for i in range(12)]
    P = proj.reshape(-1, 3, 4)
    tri = triangulate_tracks(T, kps, P, **GATES)
    base = parity_device(5)
    assert np.array_equal(tri.X.view(np.int64), base["X"].view(np.int64)) and tri.valid.all() and tri.counts[0] == 2000
    # cameras 2..9 only, given in another order: the other images are ignored
    reg = np.array([9, 2, 3, 8, 4, 7, 5, 6])
    part = triangulate_tracks(T, kps, P[reg], registered=reg, **GATES)
    cam_of_image = np.full(12, -1, np.int32)
    cam_of_image[reg] = np.arange(8)
    want = device((proj[reg], cam_of_image) + args[2:], **GATES)
    assert np.array_equal(part.status, want["status"]) and np.array_equal(part.X.view(np.int64), want["X"].view(np.int64))
    assert (part.status == tr.TOO_FEW_VIEWS).any() and part.valid.any()
    pts, cam_idx, pt_idx, uv = part.ba_inputs()
    assert len(pts) == part.valid.sum() and cam_idx.dtype == np.int32 and pt_idx.dtype == np.int32
    assert len(cam_idx) == part.n_views[part.valid].sum() and (np.diff(pt_idx) >= 0).all() and pt_idx.max() == len(pts) - 1
    assert cam_idx.min() >= 0 and cam_idx.max() < 8 and np.isfinite(uv).all() and np.isfinite(pts).all()
    h = P[reg][cam_idx] @ np.concatenate([pts[pt_idx], np.ones((len(pt_idx), 1))], axis=1)[:, :, None]
    assert np.abs(h[:, :2, 0] / h[:, 2:3, 0] - uv).max() < 4.0
    for bad in (lambda: triangulate_tracks(T, kps[:-1], P), lambda: triangulate_tracks(T, kps, P[:5]),
                lambda: triangulate_tracks(T, kps, P[:2], registered=[0, 12]),
                lambda: triangulate_tracks(T, kps, P.reshape(-1, 12)),
                lambda: triangulate_tracks(T, kps[:3] + [kps[3][:-1]] + kps[4:], P),
                lambda: triangulate_tracks(T, kps, {0: (np.eye(3), np.zeros(3))}),
                lambda: triangulate_tracks(T, kps, {99: (np.eye(3), np.zeros(3))}, K=tr.K_SFM),
                lambda: triangulate_tracks(T, kps, P, min_views=1)):
        with pytest.raises(ValueError):
            bad()
    empty = triangulate_tracks(Tracks(kp_ptr, [0], [], []), kps, P)
    assert empty.X.shape == (0, 3) and empty.counts.tolist() == [0] * 6 and len(empty.ba_inputs()[0]) == 0


# ---------------------------------------------------------------------------------------------------------- end to end
def test_matches_to_tracks_to_points_to_bundle_adjustment(gpu_ready):
    """Six cameras, 40 points, noise-free pixels -> synthetic pairwise matches -> build_tracks ->
    StructureFromMotion.triangulate_tracks -> compute_reconstruction_stats; the points feed GpuBA."""
    from sfm_amd import build_tracks
    from sfm_amd.ba import GpuBA
    from sfm_amd.reconstruction import StructureFromMotion, pack_state
    rng = np.random.default_rng(16)
    proj, Rs, ts, _ = tr.arc_cameras(6)
    X = rng.uniform(0, 1, (40, 3))
    px = tr.project_points(proj, X)                                            # [6,40,2], float64
    sees = rng.random((6, 40)) < 0.7
    sees[:3] |= sees.sum(axis=0) < 3                                           # every point in three images or more
    slot = [rng.permutation(40) for _ in range(6)]                            # keypoint index of point p in image i
    keypoints = []
    for i in range(6):
        kp = rng.uniform(0, 1000, (40, 2))                                     # the unseen slots hold keypoints of nothing
        kp[slot[i][sees[i]]] = px[i, sees[i]]
        keypoints.append(kp)
    pairs, matches = [], []
    for i in range(6):
        for j in range(i + 1, 6):
            both = np.flatnonzero(sees[i] & sees[j])
            pairs.append((i, j)); matches.append((slot[i][both], slot[j][both]))
    T = build_tracks([40] * 6, pairs, matches)
    assert len(T) == 40 and T.n_obs == sees.sum()
    sfm = StructureFromMotion(order="aligned")
    assert np.array_equal(sfm.K, tr.K_SFM)
    sfm.poses = {i: (Rs[i], ts[i].reshape(3, 1)) for i in range(6)}
    tri = sfm.triangulate_tracks(T, keypoints, min_angle_deg=1.0)
    assert tri.valid.all() and len(sfm.points3D) == 40 and len(sfm.point_tracks) == 40
    assert sorted(len(d) for d in sfm.point_tracks) == sorted(sees.sum(axis=0).tolist())
    stats = sfm.compute_reconstruction_stats()
    print("end to end:", stats)
    assert stats["num_points"] == 40 and stats["num_cameras"] == 6 and stats["mean_reproj_error"] < 1e-6
    order = np.argsort([np.flatnonzero(slot[T.image[T.track_ptr[t]]] == T.keypoint[T.track_ptr[t]])[0] for t in range(40)])
    assert np.abs(np.asarray(sfm.points3D)[order] - X).max() < 1e-9
    # registered images only: with image 5 unregistered its observations leave the tracks
    del sfm.poses[5]
    tri5 = sfm.triangulate_tracks(T, keypoints)
    assert all(5 not in d for d in sfm.point_tracks) and len(sfm.points3D) == int(tri5.valid.sum())
    assert np.array_equal(tri5.n_views, (sees[:5].sum(axis=0))[np.argsort(order)])
    sfm.poses[5] = (Rs[5], ts[5].reshape(3, 1))
    pts, cam_idx, pt_idx, uv = tri.ba_inputs()
    cams = pack_state(sfm.poses, sfm.points3D, sfm.point_tracks, sfm.K, 10, "aligned")[0]
    be = GpuBA(cams, pts, cam_idx, pt_idx, uv, (1228.0, 1228.0, 512.0, 384.0))
    assert np.isfinite(be.cost())
    be.close()
