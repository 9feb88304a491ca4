"""The device against the multi-precision truth of tests/geometry_truth.py: sfm_triangulate_tracks (plain and robust) at
0, 5 and 30 Gauss-Newton steps with and without the angle gate, the camera centres of k_camera_centres read back from
the workspace, sfm_tracks_evaluate at the truth's points, sfm_triangulate2, the four candidates of sfm_pose_recover, and
tracks at lane and workgroup seams.  Every scene of geometry_truth.scenes() goes in one call per setting; everything is
held to 8 x C_REF and every test prints its worst ratio error / (kappa 2^-53).

Measured on an MI355X: see the table in tests/geometry_truth.py.
"""
import functools

import numpy as np
import pytest

import geometry_truth as gt
import pose_reference as pr
import solver_truth as st
import triangulate_reference as tr
from test_geometry_truth import check_degenerate, five_steps, scene_tracks, show

pytestmark = pytest.mark.gpu
GATES = dict(min_views=2, max_error=4.0)


@functools.lru_cache(maxsize=None)
def device(iters, robust=False, angle=1.0):
    from sfm_amd import triangulate_tracks_raw
    return triangulate_tracks_raw(*gt.flat_args(), refine_iters=iters, min_angle_deg=angle, robust=robust, **GATES)


def judged(out, kind, what, angle=1.0):
    fails, wx, we = gt.judge_tracks(out["X"], out["max_err"], kind, gt.MARGIN, what)
    show(what + f", {kind} X", wx)
    show(what + ", max_err", we)
    f, band = gt.judge_status(out["status"], kind, what, max_error=4.0, min_angle_deg=angle)
    print(f"{what}: worst X {max(wx.values()):.3g} against {gt.MARGIN * gt.C_REF[kind]:g}, worst max_err {max(we.values()):.3g} against "
          f"{gt.MARGIN * gt.C_REF['max_err']:g}; {band:.2%} of the tracks in the status band")
    assert not fails + f, "\n".join((fails + f)[:20])
    assert band <= 0.02
    assert np.array_equal(out["n_views"], gt.n_views())
    check_degenerate(out)


@pytest.mark.parametrize("angle", [0.0, 1.0])
def test_linear_point_and_max_err(gpu_ready, angle):
    judged(device(0, angle=angle), "linear", f"device, 0 steps, min_angle {angle:g}", angle=angle)
    assert np.array_equal(device(0, angle=angle)["X"].view(np.int64), device(0, angle=1.0 - angle)["X"].view(np.int64))


@pytest.mark.parametrize("angle", [0.0, 1.0])
def test_refined_point_and_max_err(gpu_ready, angle):
    judged(device(30, angle=angle), "refined", f"device, 30 steps, min_angle {angle:g}", angle=angle)


def test_five_steps_the_shipped_default(gpu_ready):
    """Judged as the stationary point on the baseline, shifted, far, long, focal, repeated-camera, zero-row, two-view and
    exact scenes; on the narrow and principal-plane scenes the distance to the stationary point is measured in units of
    the bound and printed (worst on the device: 0.076, 0.073 and 0.10; see geometry_truth.py); the cost lies between the stationary
    cost and the linear truth's, each to the bound on the cost."""
    out = device(5)
    five_steps(out["X"], out["max_err"], "device")
    assert np.array_equal(out["X"].view(np.int64), device(5, angle=0.0)["X"].view(np.int64))


def test_camera_centres_in_the_workspace(gpu_ready):
    """k_camera_centres writes the centres first into the workspace (its only region in the plain call)."""
    import torch
    from sfm_amd._track_scene import _Scene
    proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = gt.flat_args()
    sc = _Scene(kp_ptr, kp_xy, np.zeros(0, np.int32), track_ptr, obs_image, obs_kp, 0)
    sc.set_cameras(proj, cam_of_image)
    sc.triangulate(2, 0, 4.0, 1.0)
    at, = st.ws_regions(sc.ws_bytes, (3 * len(proj), 8))
    C = sc.ws[at:at + 24 * len(proj)].view(torch.float64).cpu().numpy().reshape(-1, 3)
    fails, worst = gt.judge_centres(C, gt.MARGIN, "device")
    print(f"device, camera centres: worst error / (kappa 2^-53) {worst:.3g} against {gt.MARGIN * gt.C_REF['centre']:g}")
    assert not fails, "\n".join(fails[:10])


def test_evaluate_at_the_truths_points(gpu_ready):
    """sfm_tracks_evaluate at the stationary points rounded to float64: status by the band rule, max_err and every
    observation's error within the bound of their exact values at that rounded point.  The condition numbers are those
    of this problem (gt.evaluate_case: the point is an input and stays), not the stationary point's: with the latter
    the near view of the principal-plane scene is up to 338 x kappa 2^-53 off, because the stationary point follows a
    perturbation where a given point cannot."""
    from sfm_amd import Tracks
    from sfm_amd.incremental import evaluate_tracks
    proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = gt.flat_args()
    tracks = gt.truth()[0]
    has = np.array([T is not None and T.refined is not None for T in tracks])
    X = np.stack([T.refined.X.astype(np.float64) if h else np.zeros(3) for T, h in zip(tracks, has)])
    kps = [kp_xy[kp_ptr[i]:kp_ptr[i + 1]] for i in range(len(proj))]
    out = evaluate_tracks(Tracks(kp_ptr, track_ptr, obs_image, obs_kp), kps, proj.reshape(-1, 3, 4), X, has, max_error=4.0,
                          min_angle_deg=1.0)
    assert (out["status"][~has] == -1).all()
    fails, band = gt.judge_status(np.where(has, out["status"], 0), "refined", "sfm_tracks_evaluate", max_error=4.0, min_angle_deg=1.0)
    C = gt.MARGIN * gt.C_REF["max_err"]
    scene_of = gt.flat()[7]
    worst = worst_obs = 0.0
    for i in np.flatnonzero(has):
        T, p = tracks[i], tracks[i].refined
        if gt.max_err_left_out(p, gt.scenes()[scene_of[i]].exact):
            continue
        err, k_err, k_max = gt.evaluate_case(T, X[i])
        r = gt._ratio(abs(float(gt.mpf(float(out["max_err"][i])) - max(err))), k_max)
        worst = max(worst, r)
        if not r <= C:
            fails.append(f"track {i}: max_err {r:.3g} x kappa 2^-53 off")
        for k, e in enumerate(err):
            r = gt._ratio(abs(float(gt.mpf(float(out["obs_err"][track_ptr[i] + k])) - e)), k_err[k])
            worst_obs = max(worst_obs, r)
            if not r <= C:
                fails.append(f"track {i}, observation {k}: error {r:.3g} x kappa 2^-53 off")
    print(f"sfm_tracks_evaluate: worst max_err {worst:.3g}, worst observation {worst_obs:.3g} against {C:g}; {band:.2%} in the band")
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("iters", [0, 5, 30])
def test_robust_on_clean_scenes(gpu_ready, iters):
    """Tracks that need no rescue: the robust call satisfies the plain call's bounds (without the angle gate, so that the
    narrow and far scenes are among them; with it the same bits where both keep every view)."""
    plain, rob = device(iters, angle=0.0), device(iters, robust=True, angle=0.0)
    clean = (rob["status"] == tr.OK) & (rob["n_inliers"] == gt.n_views())
    print(f"robust, {iters} steps: {clean.sum()} of {len(clean)} tracks need no rescue")
    assert (clean | (plain["status"] != tr.OK))[np.array([T is not None for T in gt.truth()[0]])].all()
    X, e = np.where(clean[:, None], rob["X"], plain["X"]), np.where(clean, rob["max_err"], plain["max_err"])
    kind = "linear" if iters == 0 else "refined"
    only = None if iters != 5 else [sc.name for sc in gt.scenes() if sc.five == "judge" and not sc.degenerate]
    fails, wx, we = gt.judge_tracks(X, e, kind, gt.MARGIN, f"robust, {iters} steps", only=only)
    show(f"robust, {iters} steps, {kind} X", wx)
    assert not fails, "\n".join(fails[:20])
    check_degenerate(rob)
    r1 = device(iters, robust=True, angle=1.0)
    both = clean & (r1["status"] == tr.OK) & (r1["n_inliers"] == gt.n_views())
    assert both.sum() >= 500 and np.array_equal(rob["X"][both].view(np.int64), r1["X"][both].view(np.int64))


def test_robust_refit_over_the_devices_inliers(gpu_ready):
    """The baseline scene's tracks of 4 views and more with one observation moved by 100 px: the device's obs_inlier is
    taken as given (it must drop the moved observation; the robust tests own the rest of the mask), and the device's X
    lies within the refined bound of the stationary point over exactly those observations."""
    from sfm_amd import triangulate_tracks_raw
    sc = gt.scenes()[0]
    rng = np.random.default_rng(gt.SEED + 70)
    cams, xys, moved = [], [], []
    for c, xy in sc.tracks:
        if len(c) < 4:
            continue
        xy = xy.copy()
        m = int(rng.integers(0, len(c)))
        a = rng.uniform(0, 2 * np.pi)
        xy[m] += 100.0 * np.array([np.cos(a), np.sin(a)])
        cams.append(c); xys.append(xy); moved.append(m)
    args = gt._flat(sc.proj, cams, xys)
    out = triangulate_tracks_raw(*args, refine_iters=30, min_angle_deg=1.0, robust=True, **GATES)
    ptr = args[4]
    worst, fails = 0.0, []
    assert len(cams) >= 30 and (out["status"] == tr.OK).all()
    for t, (c, xy, m) in enumerate(zip(cams, xys, moved)):
        keep = out["obs_inlier"][ptr[t]:ptr[t + 1]] != 0
        assert not keep[m] and keep.sum() == out["n_inliers"][t] >= 3
        T = gt.track_truth({int(q): sc.proj[q] for q in set(c[keep].tolist())}, c[keep].tolist(), xy[keep])
        assert T.refined is not None
        r = gt.ratio_points(out["X"][t], T.refined)
        worst = max(worst, r)
        if not r <= gt.MARGIN * gt.C_REF["refined"]:
            fails.append(f"track {t}: refined X over the inliers is {r:.3g} x kappa 2^-53 off")
    print(f"robust refit: worst error / (kappa 2^-53) {worst:.3g} against {gt.MARGIN * gt.C_REF['refined']:g}")
    assert not fails, "\n".join(fails[:10])


def test_two_view_call(gpu_ready):
    """driver.triangulate_two_view on the two-view scene against the two-view truth; the same bits as the two-view tracks of
    sfm_triangulate_tracks (test_triangulate_gpu.py asserts that contract on its own scenes)."""
    from sfm_amd import driver
    proj, _, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = gt.flat_args()
    idx = scene_tracks("two views")
    a, b = track_ptr[idx], track_ptr[idx] + 1
    node = kp_ptr[obs_image] + obs_kp
    X2, valid, err = driver.triangulate_two_view(proj.reshape(-1, 3, 4), obs_image[a], obs_image[b], kp_xy[node[a]], kp_xy[node[b]], 4.0)
    full = device(0)
    assert np.array_equal(X2.view(np.int64), full["X"][idx].view(np.int64))
    assert np.array_equal(err.max(axis=1).view(np.int64), full["max_err"][idx].view(np.int64))
    X, e = full["X"].copy(), full["max_err"].copy()
    X[idx], e[idx] = X2, err.max(axis=1)
    fails, wx, we = gt.judge_tracks(X, e, "linear", gt.MARGIN, "sfm_triangulate2", only=["two views"])
    show("sfm_triangulate2, linear X", wx)
    show("sfm_triangulate2, max_err", we)
    assert not fails, "\n".join(fails[:10])


def test_pose_candidates(gpu_ready):
    """The four cand_pose of sfm_pose_recover for the 80 matrices of geometry_truth.essentials() match the truth's four as
    a set (pr.match_candidates applied to the truth) within 8 x C_REF."""
    from sfm_amd import pose
    rng = np.random.default_rng(gt.SEED + 80)
    Es = [E for _, E in gt.essentials()]
    p1 = [(rng.uniform(100, 900, (6, 2))).astype(np.float32) for _ in Es]
    p2 = [(rng.uniform(100, 900, (6, 2))).astype(np.float32) for _ in Es]
    _, dbg = pose.recover_pose_batched(Es, p1, p2, pr.K_REF, return_debug=True)
    fails, worst = [], 0.0
    for (name, _), d, T in zip(gt.essentials(), dbg, gt.pose_truths()[0]):
        assert d["status"] == 0, name
        f, r = gt.judge_poses(d["cand_pose"].reshape(4, 12), T, gt.MARGIN * gt.C_REF["pose"])
        fails += [f"{name}: {x}" for x in f]
        worst = max([worst] + r)
    print(f"device, pose candidates: worst error / (kappa 2^-53) {worst:.3g} against {gt.MARGIN * gt.C_REF['pose']:g}")
    assert not fails, "\n".join(fails[:10])


def _take(order):
    proj, cam, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = gt.flat_args()
    idx = [np.arange(track_ptr[t], track_ptr[t + 1]) for t in order]
    sel = np.concatenate(idx)
    ptr = np.concatenate([[0], np.cumsum([len(i) for i in idx])]).astype(np.int64)
    return proj, cam, kp_ptr, kp_xy, ptr, obs_image[sel], obs_kp[sel]


def test_tracks_at_lane_and_workgroup_seams(gpu_ready):
    """A 257-track call with tracks of 64, 65, 300 and 513 views and a two-view track at positions 0, 63, 64, 256 and
    255, alone and preceded by the six 513-view tracks: every track has the bits it has in the call of all scenes,
    where its position and its neighbours are others (the header's guarantee: a track's result is a function of its
    used observations in their order only)."""
    from sfm_amd import triangulate_tracks_raw
    long = scene_tracks("tracks of 64, 65, 300, 513 views")
    rng = np.random.default_rng(gt.SEED + 90)
    order = rng.permutation(len(gt.n_views()))[:257]
    order[[0, 63, 64, 255, 256]] = [long[0], long[6], long[12], scene_tracks("two views")[50], long[18]]
    assert (gt.n_views()[long[18:24]] == 513).all() and gt.n_views()[order[[0, 63, 64, 255, 256]]].tolist() == [64, 65, 300, 2, 513]
    full = device(5)
    for order in (order, np.concatenate([long[18:24], order])):
        out = triangulate_tracks_raw(*_take(order), refine_iters=5, min_angle_deg=1.0, **GATES)
        for k in ("status", "n_views"):
            assert np.array_equal(out[k], full[k][order]), k
        for k in ("X", "max_err"):
            assert np.array_equal(out[k].view(np.int64), full[k][order].view(np.int64)), k
