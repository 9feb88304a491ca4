"""reconstruct_tracks(..., robust_tracks=True): the incremental loop with per-observation inlier flags, on the loop scene
of tests/test_incremental_gpu.py with a tenth of the observations moved (631 observations, 57 moved; 46 of the 120 tracks
hold a moved observation, 37 of those still have at least 3 clean ones).  The plain loop can keep a point only on a clean
track; the robust one drops the moved observation and keeps the point."""
import functools

import numpy as np
import pytest

import triangulate_reference as tr
import triangulate_robust_reference as rr
from test_incremental_gpu import LOOP_GATES, bits, loop_result, loop_scene

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def robust_result():
    from sfm_amd import reconstruct_tracks
    s = loop_scene(21, 0.1)
    return reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, robust_tracks=True)


def flat_args(s, rec):
    T = s.tracks
    return (rec.projections().reshape(-1, 12), rec.cam_of_image(), T.kp_ptr, np.concatenate(s.keypoints), T.track_ptr, T.image,
            T.keypoint)


def assert_classified(s, rec):
    """Every returned point passes the restatement's classify at the returned cameras, with the returned flags; no
    observation lies within 1e-6 px of the gate, so none needs to be excepted.  Returns the restatement's result."""
    T = s.tracks
    ref = rr.classify(*flat_args(s, rec), np.where(rec.has_point[:, None], rec.X, 0.0), rec.has_point, **LOOP_GATES)
    near = np.abs(ref["obs_err"] - LOOP_GATES["max_error"]) <= 1e-6
    assert not near.any() and ref["margin"] > 1e-6
    assert (ref["status"][rec.has_point] == tr.OK).all() and np.array_equal(ref["status"], rec.status)
    assert rec.obs_inlier.dtype == bool and rec.obs_inlier.shape == (T.n_obs,)
    assert np.array_equal(ref["obs_inlier"] != 0, rec.obs_inlier)
    assert np.isnan(rec.X[~rec.has_point]).all() and np.isfinite(rec.X[rec.has_point]).all()
    assert not rec.obs_inlier[~rec.has_point[s.obs_track]].any()
    assert all("observations_rejected" in e for e in rec.log)
    assert rec.log[-1]["observations_rejected"] == int((rec.has_point[s.obs_track] & ~rec.obs_inlier).sum())
    return ref


def test_the_option_off_is_the_plain_loop(gpu_ready):
    from sfm_amd import reconstruct_tracks
    s, a = loop_scene(21, 0.1), loop_result(21, 0.1)
    b = reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, robust_tracks=False)
    assert a.order == b.order and a.unregistered == b.unregistered and b.obs_inlier is None and a.obs_inlier is None
    for k in ("X", "has_point", "status"):
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    assert all("observations_rejected" not in e for e in b.log)


def test_robust_loop_keeps_points_on_tracks_with_a_moved_observation(gpu_ready):
    s, rec, base = loop_scene(21, 0.1), robust_result(), loop_result(21, 0.1)
    T = s.tracks
    print("registration order:", rec.order, "points:", int(rec.has_point.sum()), "plain loop:", int(base.has_point.sum()),
          "rejected per step:", [e.get("observations_rejected") for e in rec.log])
    assert sorted(rec.order) == list(range(8)) and rec.unregistered == []
    args = flat_args(s, rec)
    ref = assert_classified(s, rec)
    # no moved observation of a kept track is an inlier unless it lies within the gate
    kept = s.obs_moved & rec.has_point[s.obs_track] & rec.obs_inlier
    print("moved observations flagged as inliers:", int(kept.sum()), "their errors:", ref["obs_err"][kept])
    assert (ref["obs_err"][kept] <= 4.0).all()
    assert rec.has_point.sum() > base.has_point.sum()
    # the rescue share: of the tracks with a moved observation and at least 3 clean ones, the ones the restatement rescues
    # at the ground-truth cameras; the loop keeps a point on more than 0.9 of them (the share the plain loop's test allows
    # on clean tracks)
    n_moved = np.bincount(s.obs_track, weights=s.obs_moved, minlength=len(T)).astype(int)
    n_clean = T.lengths() - n_moved
    cand = (n_moved > 0) & (n_clean >= 3)
    assert s.obs_moved.sum() == 57 and (n_moved > 0).sum() == 46 and cand.sum() == 37
    truth = rr.triangulate_robust(s.proj.reshape(-1, 12), np.arange(8, dtype=np.int32), *args[2:], refine_iters=5, **LOOP_GATES)
    rescued = cand & (truth["status"] == tr.OK)
    R = int(rescued.sum())
    got = int(rec.has_point[rescued].sum())
    print(f"tracks with a moved observation and at least 3 clean ones: 37; rescued by the restatement at the ground-truth "
          f"cameras R = {R}; the loop keeps a point on {got} of them; on clean tracks {int(rec.has_point[n_moved == 0].sum())} of "
          f"{int((n_moved == 0).sum())}")
    assert R > 0 and got > 0.9 * R


def test_a_bundle_adjustment_inside_the_loop_sees_the_newest_camera(gpu_ready):
    """ba_every = 2, so that bundle adjustments run between registrations.  Until an image is registered its observations
    carry flag 0; they are classified right after the registration, before the adjustment, which therefore sees the new
    camera's inliers on the points that existed already - the ones PnP registered it with - and not only those of the
    tracks adopted in the same step (at most one observation of that camera per adopted track)."""
    from sfm_amd import reconstruct_tracks
    s = loop_scene(21, 0.1)
    rec = reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, robust_tracks=True, ba_every=2)
    inside = [e for e in rec.log if e.get("ba") is not None and not e.get("final")]
    print("registration order:", rec.order, "points:", int(rec.has_point.sum()), "adjustments inside the loop:",
          [(e["chosen"], e["points_added"], e["ba"].get("observations_newest_camera"), e["ba"].get("n_observations"),
            e["ba"]["success"]) for e in inside])
    assert sorted(rec.order) == list(range(8)) and len(inside) == 3
    for e in inside:
        assert e["ba"]["success"] and e["chosen"] is not None
        assert e["ba"]["observations_newest_camera"] > e["points_added"]
        assert e["ba"]["n_observations"] >= e["ba"]["observations_newest_camera"]
    ref = assert_classified(s, rec)
    kept = s.obs_moved & rec.has_point[s.obs_track] & rec.obs_inlier
    assert (ref["obs_err"][kept] <= 4.0).all()


def test_a_dead_end_still_logs_the_rejected_observations(gpu_ready):
    from sfm_amd import reconstruct_tracks
    s = loop_scene(21, 0.0, 2, 200)
    rec = reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, robust_tracks=True)
    assert sorted(rec.order) in ([0, 1, 2, 3], [4, 5, 6, 7]) and rec.log[-2]["candidates"] == [] and rec.log[-2]["chosen"] is None
    assert_classified(s, rec)


def test_ba_inputs_and_state_hold_no_rejected_observation(gpu_ready):
    s, rec = loop_scene(21, 0.1), robust_result()
    T = s.tracks
    keep = rec.has_point[s.obs_track] & rec.obs_inlier
    assert 0 < keep.sum() < rec.has_point[s.obs_track].sum()
    cams, pts, cam_idx, pt_idx, uv = rec.ba_inputs()
    assert len(uv) == keep.sum() and len(pts) == rec.has_point.sum() and cams.shape == (8, 6)
    assert np.array_equal(uv, s.uv[keep]) and np.array_equal(cam_idx, rec.cam_of_image()[T.image[keep]])
    assert np.array_equal(pt_idx, (np.cumsum(rec.has_point) - 1)[s.obs_track[keep]])
    poses, points3D, point_tracks = rec.as_state()
    assert len(points3D) == rec.has_point.sum() and sum(len(d) for d in point_tracks) == keep.sum()
    new_id = np.cumsum(rec.has_point) - 1
    for o in np.flatnonzero(rec.has_point[s.obs_track] & ~rec.obs_inlier):
        assert int(T.image[o]) not in point_tracks[new_id[s.obs_track[o]]]


def test_robust_loop_is_deterministic(gpu_ready):
    from sfm_amd import reconstruct_tracks
    s, a = loop_scene(21, 0.1), robust_result()
    b = reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, robust_tracks=True)
    assert a.order == b.order and a.unregistered == b.unregistered
    for k in ("X", "has_point", "status", "K", "obs_inlier"):
        assert np.array_equal(bits(getattr(a, k)), bits(getattr(b, k))), k
    for i in a.order:
        assert np.array_equal(bits(a.poses[i][0]), bits(b.poses[i][0])) and np.array_equal(bits(a.poses[i][1]), bits(b.poses[i][1]))
