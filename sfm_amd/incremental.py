"""Incremental reconstruction from multi-view tracks, driven through the batched device calls of this package:
`build_tracks` -> `reconstruct_tracks` -> cameras and points.  Two device calls join the existing stages:

  `resection_lists`   sfm_tracks_resection (sfm_amd/csrc/resection.hip): the 2D-3D correspondences of every unregistered
                      image, taken from the tracks by index - what PnP consumes, and their counts rank the next view
  `evaluate_tracks`   sfm_tracks_evaluate (sfm_amd/csrc/triangulate.hip): the triangulation gates at points that are
                      given - what a bundle adjustment leaves behind
  `classify_tracks`   sfm_tracks_classify (sfm_amd/csrc/triangulate.hip): the same gates over the observations
                      that agree with the point, and a flag per observation - the loop's `robust_tracks` mode

For the life of a `reconstruct_tracks` call the CSR arrays, kp_ptr, kp_xy, node_track, X and has_point live in device
tensors uploaded once; per step only the cameras go up and only the correspondence lists, statuses and counts come
down.  PnP (`solve_pnp_ransac_batched`) and the bundle adjustment (`solve_ba`) still go through their host-array entry
points.  No CPU fallback: without the library or a GPU these raise.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._track_scene import _Scene
from .driver import TRIANGULATION_MAX_ERROR, projection_matrix
from .triangulate import _cameras, _check_options, _check_tracks, keypoint_table


def node_track_of(tracks):
    """node_track [n_nodes] int32 rebuilt from the CSR arrays: the track of every node that is an observation, -1 elsewhere."""
    n_nodes = int(tracks.kp_ptr[-1])
    node_track = np.full(n_nodes, -1, dtype=np.int32)
    if tracks.n_obs:
        node = tracks.kp_ptr[tracks.image] + tracks.keypoint
        node_track[node] = np.repeat(np.arange(len(tracks), dtype=np.int32), tracks.lengths())
    return node_track


def resection_lists(tracks, keypoints, X, has_point, cam_of_image, device=0):
    """The 2D-3D correspondences of every unregistered image (cam_of_image[i] < 0), by index: a keypoint is listed when
    its track has a point.  X [n_tracks,3], has_point [n_tracks].  Returns host arrays (seg_ptr [n_img+1] int64,
    corr_track [n] int32, corr_X [n,3] float64, corr_uv [n,2] float32): image i owns entries seg_ptr[i]:seg_ptr[i+1], in
    keypoint order - the first arguments of sfm_pnp_ransac.  `tracks.node_track` is rebuilt from the CSR arrays when None."""
    n_img = _check_tracks(tracks, keypoints)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    has_point = np.asarray(has_point).reshape(-1)
    cam_of_image = np.asarray(cam_of_image).reshape(-1)
    if len(X) != len(tracks) or len(has_point) != len(tracks) or len(cam_of_image) != n_img:
        raise ValueError("X / has_point need one entry per track and cam_of_image one per image")
    kp_xy = keypoint_table(tracks, keypoints)
    if kp_xy.shape[0] == 0 or len(tracks) == 0:
        return (np.zeros(n_img + 1, np.int64), np.zeros(0, np.int32), np.zeros((0, 3), np.float64), np.zeros((0, 2), np.float32))
    node_track = tracks.node_track if tracks.node_track is not None else node_track_of(tracks)
    if len(node_track) != kp_xy.shape[0]:
        raise ValueError("node_track must have one entry per keypoint")
    sc = _Scene(tracks.kp_ptr, kp_xy, node_track, tracks.track_ptr, tracks.image, tracks.keypoint, device)
    sc.set_points(X, has_point)
    sc.set_cameras(np.zeros((0, 12)), cam_of_image)
    seg_ptr, _, corr_track, corr_X, corr_uv = sc.resection()
    return seg_ptr, corr_track, corr_X, corr_uv


def _judge_tracks(robust, tracks, keypoints, proj_or_poses, X, has_point, K, registered, min_views, max_error, min_angle_deg,
                  device):
    """`evaluate_tracks` (robust False) and `classify_tracks` (True): the host checks, one scene, one call, the download."""
    _check_options(min_views, 0, max_error, min_angle_deg)
    _check_tracks(tracks, keypoints)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    has_point = np.asarray(has_point).reshape(-1)
    if len(X) != len(tracks) or len(has_point) != len(tracks):
        raise ValueError("X / has_point need one entry per track")
    proj, cam_of_image = _cameras(tracks, proj_or_poses, K, registered)
    kp_xy = keypoint_table(tracks, keypoints)
    if len(tracks) == 0:
        out = {"status": np.zeros(0, np.int32), "n_views": np.zeros(0, np.int32), "max_err": np.zeros(0),
               "obs_err": np.zeros(0), "counts": np.zeros(6, np.int64)}
        if robust:
            out.update(n_inliers=np.zeros(0, np.int32), obs_inlier=np.zeros(0, bool))
        return out
    sc = _Scene(tracks.kp_ptr, kp_xy, np.zeros(0, np.int32), tracks.track_ptr, tracks.image, tracks.keypoint, device, robust=robust)
    sc.set_points(X, has_point)
    sc.set_cameras(proj, cam_of_image)
    obs_err = (sc.classify if robust else sc.evaluate)(min_views, max_error, min_angle_deg, want_obs_err=True)
    out = {"status": sc.status.cpu().numpy(), "n_views": sc.n_views.cpu().numpy(), "max_err": sc.max_err.cpu().numpy(),
           "obs_err": obs_err.cpu().numpy(), "counts": sc.counts.cpu().numpy()}
    if robust:
        out.update(n_inliers=sc.n_inliers.cpu().numpy(), obs_inlier=sc.obs_inlier[:sc.n_obs].cpu().numpy() != 0)
    return out


def evaluate_tracks(tracks, keypoints, proj_or_poses, X, has_point, K=None, registered=None, min_views=2,
                    max_error=TRIANGULATION_MAX_ERROR, min_angle_deg=0.0, device=0):
    """The gates of `triangulate_tracks` at points that are given (after a bundle adjustment, say).  Cameras as
    `triangulate_tracks` takes them.  Returns {status [n] int32 (sfm_amd._lib.TRI_*, or EVAL_NO_POINT = -1 where has_point
    is 0), n_views [n] int32, max_err [n], obs_err [n_obs] (NaN: image not registered or no point), counts [6] int64 (the
    tracks that have a point, by status)}."""
    return _judge_tracks(False, tracks, keypoints, proj_or_poses, X, has_point, K, registered, min_views, max_error,
                         min_angle_deg, device)


def classify_tracks(tracks, keypoints, proj_or_poses, X, has_point, K=None, registered=None, min_views=2,
                    max_error=TRIANGULATION_MAX_ERROR, min_angle_deg=0.0, device=0):
    """`evaluate_tracks` over the observations that agree with the given points (sfm_tracks_classify): an observation is
    an inlier when it is finite, lies in front of its camera and reprojects within max_error.  Same arguments.  Returns
    {status [n] int32 (0, TRI_TOO_FEW_VIEWS: fewer than min_views inliers, TRI_LOW_ANGLE, or EVAL_NO_POINT = -1 where
    has_point is 0), n_views [n] int32, n_inliers [n] int32, max_err [n] (the largest error of an inlier), obs_inlier
    [n_obs] bool, obs_err [n_obs] (NaN: image not registered or no point), counts [6] int64 (the tracks that have a point,
    by status)}."""
    return _judge_tracks(True, tracks, keypoints, proj_or_poses, X, has_point, K, registered, min_views, max_error,
                         min_angle_deg, device)


# ------------------------------------------------------------------------------------------------------------ the loop
class Reconstruction:
    """What `reconstruct_tracks` returns.  poses {image position: (R [3,3], t [3])}, order (registration order), K (the
    intrinsics the cameras were last evaluated with), X [n_tracks,3] (NaN without a point), has_point [n_tracks] bool,
    status [n_tracks] int32 from the last evaluation (-1 without a point), unregistered (image positions), log (one dict
    per step), obs_inlier ([n_obs] bool from `robust_tracks=True`: the observations a point is kept with - the others are
    left out of `ba_inputs()` and `as_state()`; None otherwise)."""

    def __init__(self, tracks, kp_xy, K):
        self.tracks, self._kp_xy = tracks, kp_xy
        self.K = np.array(K, dtype=np.float64)
        n = len(tracks)
        self.poses, self.order, self.unregistered, self.log = {}, [], list(range(len(tracks.kp_ptr) - 1)), []
        self.X = np.full((n, 3), np.nan)
        self.has_point = np.zeros(n, bool)
        self.status = np.full(n, _lib.EVAL_NO_POINT, np.int32)
        self.obs_inlier = None

    def cam_of_image(self):
        cam = np.full(len(self.tracks.kp_ptr) - 1, -1, dtype=np.int32)
        cam[self.order] = np.arange(len(self.order), dtype=np.int32)
        return cam

    def projections(self):
        """[n_cams,3,4] K[R|t] in registration order."""
        return np.asarray([projection_matrix(self.K, *self.poses[i]) for i in self.order], dtype=np.float64).reshape(-1, 3, 4)

    def _observations(self):
        """(observation indices, point index of each) over the tracks with a point and the registered images; with
        obs_inlier, over the inlier observations only."""
        tr = self.tracks
        new_id = np.cumsum(self.has_point) - 1
        trk = np.repeat(np.arange(len(tr)), tr.lengths())
        sel = np.flatnonzero(self.has_point[trk] & (self.cam_of_image()[tr.image] >= 0)) if tr.n_obs else np.zeros(0, np.int64)
        if self.obs_inlier is not None:
            sel = sel[self.obs_inlier[sel]]
        return sel, new_id[trk[sel]]

    def ba_inputs(self, cam_dim=6):
        """(cams [C,cam_dim], pts [m,3], cam_idx int32, pt_idx int32, uv [k,2]) point-major: what `GpuBA` / `solve_ba` take."""
        from .rotation import log_so3
        tr = self.tracks
        cams = np.zeros((len(self.order), cam_dim))
        for c, i in enumerate(self.order):
            R, t = self.poses[i]
            cams[c, :3], cams[c, 3:6] = log_so3(R), np.asarray(t).reshape(3)
            if cam_dim == 10:
                cams[c, 6:] = (self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2])
        sel, pt = self._observations()
        node = tr.kp_ptr[tr.image[sel]] + tr.keypoint[sel]
        return (cams, self.X[self.has_point].copy(), self.cam_of_image()[tr.image[sel]].astype(np.int32), pt.astype(np.int32),
                self._kp_xy[node].copy())

    def as_state(self, image_ids=None):
        """(poses {image_id: (R, t [3,1])}, points3D, point_tracks) in the reference's shapes: one [x, y, z] and one
        {image_id: [x, y]} (registered images only) per track that has a point."""
        tr = self.tracks
        if image_ids is None:
            image_ids = tr.image_ids if tr.image_ids is not None else range(len(tr.kp_ptr) - 1)
        ids = [int(i) for i in image_ids]
        poses = {ids[i]: (self.poses[i][0].copy(), np.asarray(self.poses[i][1], dtype=np.float64).reshape(3, 1)) for i in self.order}
        sel, pt = self._observations()
        node = tr.kp_ptr[tr.image[sel]] + tr.keypoint[sel]
        point_tracks = [dict() for _ in range(int(self.has_point.sum()))]
        for o, p, uv in zip(sel.tolist(), pt.tolist(), self._kp_xy[node].tolist()):
            point_tracks[p][ids[tr.image[o]]] = uv
        return poses, self.X[self.has_point].tolist(), point_tracks


def _common_track_pairs(tracks, limit):
    """The `limit` image pairs (i < j) with the most common tracks, most first, ties to the lower (i, j).  Counted on the
    host through a dense track x image incidence (float32 products are exact below 2^24 tracks)."""
    n_img = len(tracks.kp_ptr) - 1
    A = np.zeros((len(tracks), n_img), dtype=np.float32)
    A[np.repeat(np.arange(len(tracks)), tracks.lengths()), tracks.image] = 1.0
    common = np.rint(A.T @ A).astype(np.int64)
    i, j = np.triu_indices(n_img, 1)
    c = common[i, j]
    keep = np.flatnonzero(c > 0)
    order = keep[np.lexsort((j[keep], i[keep], -c[keep]))][:limit]
    return [(int(i[k]), int(j[k])) for k in order]


def _pair_pixels(tracks, kp_xy, i, j):
    """(pixels in image i, pixels in image j, tracks) - [m,2] float64 and [m] - of the tracks both images see (the first
    keypoint of an image in a track, should a kept conflicting track hold two), by ascending track."""
    node = tracks.kp_ptr[tracks.image] + tracks.keypoint
    trk = np.repeat(np.arange(len(tracks)), tracks.lengths())

    def first_node(img):
        sel = np.flatnonzero(tracks.image == img)[::-1]
        at = np.full(len(tracks), -1, dtype=np.int64)
        at[trk[sel]] = node[sel]
        return at
    a, b = first_node(i), first_node(j)
    both = np.flatnonzero((a >= 0) & (b >= 0))
    return kp_xy[a[both]], kp_xy[b[both]], both


def _initial_pair(tracks, kp_xy, K, initial_pair, o, device):
    """((i, j), R, t, n_good, good tracks, candidates log) of the start: F - or, with `initial_model` "essential", E by
    five-point RANSAC with the same threshold, hypothesis count and seed - on the common tracks, then the pose, all
    candidates in one batch each; the winner has the most good points (ties: the lower (i, j)).  The good tracks are the
    ones the pose stage counted: inliers of the model that lie in front of both cameras.
    With `max_homography_ratio` = r, one batched homography RANSAC (same threshold, hypothesis count and seed) runs over
    the same pixel lists; a candidate with n_H > r * n_model - the inlier counts of its H and of its F or E - is left
    out of the choice, and every row of the log gains `n_model`, `n_homography` and `degenerate`.  A given
    `initial_pair` is recorded, not left out."""
    from ._lib import SfmError
    from .pose import recover_pose_batched
    from .essential import estimate_essential_batched
    from .homography import estimate_homography_batched
    from .twoview import estimate_fundamental_batched
    pairs = [tuple(initial_pair)] if initial_pair is not None else _common_track_pairs(tracks, o["initial_candidates"])
    if not pairs:
        raise SfmError("no image pair shares a track")
    px = [_pair_pixels(tracks, kp_xy, i, j) for i, j in pairs]
    essential = o["initial_model"] == "essential"
    if essential:
        fund = estimate_essential_batched([p[0] for p in px], [p[1] for p in px], K, threshold=o["fund_threshold"],
                                          n_hypotheses=o["fund_hypotheses"], seed=o["seed"], device=device)
    else:
        fund = estimate_fundamental_batched([p[0] for p in px], [p[1] for p in px], threshold=o["fund_threshold"],
                                            n_hypotheses=o["fund_hypotheses"], seed=o["seed"], device=device)
    live = [k for k, (F, _) in enumerate(fund) if F is not None]
    rows = [{"pair": pairs[k], "common": len(px[k][0]), "n_good": 0} for k in range(len(pairs))]
    ratio = o["max_homography_ratio"]
    if ratio is not None:
        hom = estimate_homography_batched([p[0] for p in px], [p[1] for p in px], threshold=o["fund_threshold"],
                                          n_hypotheses=o["fund_hypotheses"], seed=o["seed"], device=device)
        for k, ((_, fm), (_, hm)) in enumerate(zip(fund, hom)):
            n_model = 0 if fm is None else int(np.count_nonzero(fm))
            n_hom = 0 if hm is None else int(np.count_nonzero(hm))
            rows[k].update(n_model=n_model, n_homography=n_hom, degenerate=bool(float(n_hom) > float(ratio) * float(n_model)))
        if initial_pair is None:
            live = [k for k in live if not rows[k]["degenerate"]]
            if not live:
                raise SfmError(f"every one of the {len(pairs)} candidate pairs is degenerate: a homography explains more than "
                               f"{ratio} of the inliers of its model (max_homography_ratio)")
    best = None
    if live:
        pose = recover_pose_batched([fund[k][0] for k in live], [px[k][0] for k in live], [px[k][1] for k in live], K,
                                    masks=[fund[k][1] for k in live], from_fundamental=not essential, device=device)
        for k, (n_good, R, t, mask) in zip(live, pose):
            rows[k]["n_good"] = int(n_good)
            if R is not None and (best is None or (-n_good, pairs[k]) < (-best[3], best[0])):
                best = (pairs[k], R, np.asarray(t).reshape(3), int(n_good), px[k][2][np.asarray(mask).reshape(-1) != 0])
    if best is None or best[3] < o["min_initial_points"]:
        raise SfmError(f"no initial pair with at least {o['min_initial_points']} good points "
                       f"(best: {None if best is None else (best[0], best[3])})")
    return best + (rows,)


DEFAULTS = dict(initial_candidates=32, min_initial_points=50, min_visible=15, candidates_per_step=8, pnp_threshold=8.0,
                pnp_hypotheses=1024, pnp_min_inliers=15, seed=0, ba_every=7, cam_dim=6, max_error=TRIANGULATION_MAX_ERROR,
                min_angle_deg=1.0, refine_iters=5, min_views=2, fund_threshold=3.0, fund_hypotheses=1024,
                refine_initial_pair=True, image_size=(1024, 768), initial_model="fundamental", max_homography_ratio=None,
                robust_tracks=False)


def reconstruct_tracks(tracks, keypoints, K, initial_pair=None, device=0, **options):
    """Cameras and points from tracks: initial pair (given, or the best of the `initial_candidates` pairs with the most
    common tracks; its pose comes from F, or with `initial_model="essential"` from a five-point E, and is refined by a
    two-camera bundle adjustment unless `refine_initial_pair` is False), then
    per step the resection lists of all unregistered images, one batched PnP over the `candidates_per_step` images that see the most points, registration of the one with the most inliers, triangulation
    of the tracks that have no point yet; a bundle adjustment (`solve_ba`, `cam_dim` 6 = fixed K or 10) every `ba_every`
    registrations and at the end, each followed by `evaluate_tracks` - points that fail a gate are dropped and
    triangulated again.  Every choice is deterministic (ties: more visible points, then the lower image position).
    `max_homography_ratio` (default None: off) guards the initial pair against degenerate geometry: a pair whose
    matches lie on a plane, or whose cameras share a centre, has no defined F, yet F RANSAC still returns a model with
    nearly all matches as inliers, and such pairs tend to have the most matches.  With a value r, a homography RANSAC
    runs beside the F / E stage and a candidate whose homography keeps more than r times the inliers of its model is
    left out (SfmError if that leaves none).  0.8 is the customary value (COLMAP's, recalled).  The NumPy reference
    (tests/test_homography_reference.py: 512 hypotheses at 3 px, 40 and 300 matches, 0 % and 30 % outliers) gives
    n_H / n_F of 0.07 to 0.19 on a general scene and 0.90 to 1.00 on a pure rotation and on a plane.
    `robust_tracks` (default False) drops outlier observations instead of points: tracks are triangulated by
    sfm_triangulate_tracks_robust (a failing track of at least 4 views is searched for a consensus of at least 3), every
    observation carries an inlier flag that sfm_tracks_classify refreshes after every registration and every bundle
    adjustment, the bundle adjustment sees the inlier observations only, a point is dropped when fewer than `min_views`
    observations agree with it or those fail the angle gate, and the log entries gain `observations_rejected` (the result of a bundle
    adjustment in the log also `observations_newest_camera`, what it saw of the camera registered last).  PnP is
    robust by itself and sees every point as before.
    Options and their defaults: `DEFAULTS`.  keypoints: per image position an [n,2] array or cv2.KeyPoints.  Image
    positions are those of `tracks.kp_ptr`.  Validates on the host first (ValueError); raises SfmError when no initial pair
    has `min_initial_points` good points; a data set that falls apart returns the part that registered and lists the
    rest in `unregistered`.  Returns a `Reconstruction`."""
    from ._lib import SfmNumericError
    from .ba import solve_ba
    from .pnp import solve_pnp_ransac_batched
    from .rotation import rodrigues
    unknown = set(options) - set(DEFAULTS)
    if unknown:
        raise TypeError(f"unknown options {sorted(unknown)}")
    o = dict(DEFAULTS, **options)
    _check_options(o["min_views"], o["refine_iters"], o["max_error"], o["min_angle_deg"])
    if o["cam_dim"] not in (6, 10):
        raise ValueError("cam_dim must be 6 or 10")
    if o["initial_model"] not in ("fundamental", "essential"):
        raise ValueError('initial_model must be "fundamental" or "essential"')
    if o["max_homography_ratio"] is not None:
        r = o["max_homography_ratio"]
        if isinstance(r, (bool, str)) or not np.isscalar(r) or not (np.isfinite(r) and r > 0):
            raise ValueError("max_homography_ratio must be None or a finite number above 0")
        o["max_homography_ratio"] = float(r)
    n_img = _check_tracks(tracks, keypoints)
    K = np.asarray(K, dtype=np.float64)
    if K.shape != (3, 3):
        raise ValueError("K must be 3 x 3")
    if initial_pair is not None:
        initial_pair = tuple(int(v) for v in initial_pair)
        if len(initial_pair) != 2 or not all(0 <= v < n_img for v in initial_pair) or initial_pair[0] == initial_pair[1]:
            raise ValueError(f"initial_pair {initial_pair} is not a pair of two of the {n_img} images")
    kp_xy = keypoint_table(tracks, keypoints)
    rec = Reconstruction(tracks, kp_xy, K)
    if tracks.n_obs == 0:
        return rec

    (i0, j0), R, t, n_good, good, rows = _initial_pair(tracks, kp_xy, K, initial_pair, o, device)
    rec.poses = {i0: (np.eye(3), np.zeros(3)), j0: (R, t)}
    rec.order = [i0, j0]
    node_track = tracks.node_track if tracks.node_track is not None else node_track_of(tracks)
    robust = bool(o["robust_tracks"])
    sc = _Scene(tracks.kp_ptr, kp_xy, node_track, tracks.track_ptr, tracks.image, tracks.keypoint, device, robust=robust)
    tri_gates = dict(min_views=o["min_views"], refine_iters=o["refine_iters"], max_error=o["max_error"],
                     min_angle_deg=o["min_angle_deg"])
    eval_gates = dict(min_views=o["min_views"], max_error=o["max_error"], min_angle_deg=o["min_angle_deg"])
    unregistered = [i for i in range(n_img) if i not in rec.poses]

    def cameras_up():
        sc.set_cameras(rec.projections().reshape(-1, 12), rec.cam_of_image())

    def run_ba(cam_dim):
        """(result for the log, cams, pts) of `solve_ba` over rec.X / rec.has_point and the registered cameras."""
        cams, pts, cam_idx, pt_idx, uv = rec.ba_inputs(cam_dim)
        if len(uv) == 0:
            return {"success": False, "reason": "no observations"}, None, None
        K0 = (rec.K[0, 0], rec.K[1, 1], rec.K[0, 2], rec.K[1, 2])
        be = None
        try:
            res, cams, pts, be = solve_ba(cams, pts, cam_idx, pt_idx, uv, K0, float(o["image_size"][0]),
                                          float(o["image_size"][1]), device=device)
        except SfmNumericError as e:
            return {"success": False, "reason": str(e)}, None, None
        finally:
            if be is not None:
                be.close()
        return ({"success": bool(res.success), "cost": float(res.cost), "nfev": int(res.nfev), "status": int(res.status),
                 "n_points": len(pts), "n_observations": len(uv)}, cams, pts)

    def refine_pair():
        """By default the pose of the initial pair comes from E = K^T F K, and F has two more degrees of freedom than E: with noisy
        pixels the essential matrix nearest to it leaves reprojection errors of several pixels, above the `max_error` gate,
        and the first triangulation would adopt nothing.  So the pair gets a bundle adjustment of its own (fixed K) over
        its good tracks, triangulated without the error gate; the result goes back to the gauge [I|0], [R|t] with
        |t| = 1 and no point is kept.  Without success the pose stays as it was.  Returns the result for the log.
        (`initial_model="essential"` removes the cause; the refinement keeps its meaning there.)"""
        sc.triangulate(**dict(tri_gates, max_error=float("inf")))
        seed = np.zeros(len(tracks), dtype=bool)
        seed[good] = True
        seed &= sc.status.cpu().numpy() == _lib.TRI_OK
        rec.X, rec.has_point = np.where(seed[:, None], sc.X_tri.cpu().numpy(), np.nan), seed
        out, cams, _ = run_ba(6)
        rec.X, rec.has_point = np.full((len(tracks), 3), np.nan), np.zeros(len(tracks), dtype=bool)
        if not out["success"]:
            return out
        Ra, Rb = rodrigues(cams[0, :3]), rodrigues(cams[1, :3])
        Rr = Rb @ Ra.T
        t_rel = cams[1, 3:6] - Rr @ cams[0, 3:6]
        if not (np.isfinite(Rr).all() and np.isfinite(t_rel).all() and np.linalg.norm(t_rel) > 0):
            return dict(out, success=False, reason="the refined pose is not finite")
        rec.poses[j0] = (Rr, t_rel / np.linalg.norm(t_rel))
        return out

    def bundle_adjust():
        """The BA result for the log.  On success the cameras and points are adopted, failing points dropped and
        triangulated again; otherwise the state stays as it was."""
        rec.X, rec.has_point = sc.X.cpu().numpy(), sc.has_point.cpu().numpy() != 0
        if robust:
            rec.obs_inlier = sc.obs_inlier[:sc.n_obs].cpu().numpy() != 0
        out, cams, pts = run_ba(o["cam_dim"])
        if robust:
            # what the adjustment saw of the camera registered last: its inliers on old points and on the ones just adopted
            out["observations_newest_camera"] = int((tracks.image[rec._observations()[0]] == rec.order[-1]).sum())
        if not out["success"]:
            return out
        if o["cam_dim"] == 10:
            rec.K = np.mean([np.array([[c[6], 0, c[8]], [0, c[7], c[9]], [0, 0, 1]]) for c in cams], axis=0)
        for c, i in enumerate(rec.order):
            rec.poses[i] = (rodrigues(cams[c, :3]), cams[c, 3:6].copy())
        rec.X[rec.has_point] = pts
        sc.set_points(rec.X, rec.has_point)
        cameras_up()
        out["points_removed"] = sc.drop_failing_points(**eval_gates)
        out["points_added"] = sc.adopt_new_points(**tri_gates)
        return out

    def refresh_flags(entry):
        """Robust mode, after a registration and before anything uses the flags: the new camera's observations are
        classified at the current points (until then they are 0, as those of every unregistered image; nothing is dropped
        here); the entry gets the number of rejected observations."""
        if robust:
            sc.classify(**eval_gates)
            entry["observations_rejected"] = sc.observations_rejected()

    cameras_up()
    refined = refine_pair() if o["refine_initial_pair"] else None
    if refined is not None and refined["success"]:
        cameras_up()
    added = sc.adopt_new_points(**tri_gates)
    rec.log.append({"step": 0, "initial_pair": (i0, j0), "initial_model": o["initial_model"], "n_good": n_good, "candidates": rows, "pair_refinement": refined,
                    "points_added": added})
    refresh_flags(rec.log[-1])
    since_ba = 0
    while unregistered:
        seg_ptr, _, _, corr_X, corr_uv = sc.resection()
        visible = np.diff(seg_ptr)
        cands = sorted((i for i in unregistered if visible[i] >= o["min_visible"]), key=lambda i: (-visible[i], i))
        cands = cands[:o["candidates_per_step"]]
        entry = {"step": len(rec.log), "candidates": cands, "visible": [int(visible[i]) for i in cands], "inliers": [],
                 "chosen": None, "points_added": 0, "points_removed": 0, "ba": None}
        if robust:
            entry["observations_rejected"] = sc.observations_rejected()       # also for an entry that ends the loop below
        rec.log.append(entry)
        if not cands:
            break
        res = solve_pnp_ransac_batched([corr_X[seg_ptr[i]:seg_ptr[i + 1]] for i in cands],
                                       [corr_uv[seg_ptr[i]:seg_ptr[i + 1]] for i in cands], rec.K,
                                       threshold=o["pnp_threshold"], n_hypotheses=o["pnp_hypotheses"], seed=o["seed"],
                                       device=device)
        inl = [len(r[3]) if r[0] else 0 for r in res]
        entry["inliers"] = inl
        k = min(range(len(cands)), key=lambda k: (-inl[k], -visible[cands[k]], cands[k]))
        if inl[k] < o["pnp_min_inliers"]:
            break
        i = cands[k]
        entry["chosen"] = i
        rec.poses[i] = (rodrigues(res[k][1]), np.asarray(res[k][2], dtype=np.float64).reshape(3))
        rec.order.append(i)
        unregistered.remove(i)
        cameras_up()
        entry["points_added"] = sc.adopt_new_points(**tri_gates)
        refresh_flags(entry)                                 # before the adjustment, which sees the inliers only
        since_ba += 1
        if since_ba >= o["ba_every"] and len(rec.order) > 2:
            entry["ba"] = bundle_adjust()
            entry["points_removed"] = entry["ba"].get("points_removed", 0)
            since_ba = 0
            if robust:                                       # the adjustment's own classify and adoption left the flags current
                entry["observations_rejected"] = sc.observations_rejected()
    # the end: a bundle adjustment when cameras were registered since the last one; then the gates once more, so that
    # every point that is returned passes them under the cameras that are returned
    final = {"step": len(rec.log), "final": True, "ba": None, "points_removed": 0, "points_added": 0}
    if since_ba > 0 and len(rec.order) > 2:
        final["ba"] = bundle_adjust()
    final["points_removed"] = sc.drop_failing_points(**eval_gates)
    if final["points_removed"]:
        final["points_added"] = sc.adopt_new_points(**tri_gates)
    if robust:
        sc.classify(**eval_gates)
        final["observations_rejected"] = sc.observations_rejected()
        rec.obs_inlier = sc.obs_inlier[:sc.n_obs].cpu().numpy() != 0
    else:
        sc.evaluate(**eval_gates)
    rec.log.append(final)
    rec.has_point = sc.has_point.cpu().numpy() != 0
    rec.X = np.where(rec.has_point[:, None], sc.X.cpu().numpy(), np.nan)
    rec.status = sc.status.cpu().numpy()
    rec.unregistered = unregistered
    return rec
