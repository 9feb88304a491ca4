"""N-view triangulation of multi-view tracks on the device (`sfm_triangulate_tracks`, sfm_amd/csrc/triangulate.hip): the
join between `build_tracks` and the bundle adjustment.  Every track of a `Tracks` object is triangulated from its
observations in registered images - a linear stage, a fixed number of Gauss-Newton steps, then the gates a reconstruction
needs (views, cheirality, triangulation angle, reprojection error) - in one call, and the result is what `GpuBA` takes.
No CPU fallback: without the library or a GPU these raise.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .driver import TRIANGULATION_MAX_ERROR, projection_matrix


def _check_options(min_views, refine_iters, max_error, min_angle_deg):
    if int(min_views) < 2:
        raise ValueError("min_views must be at least 2")
    if int(refine_iters) < 0:
        raise ValueError("refine_iters must not be negative")
    if not float(max_error) >= 0.0:
        raise ValueError("max_error must not be negative")
    if not 0.0 <= float(min_angle_deg) <= 180.0:
        raise ValueError("min_angle_deg must lie in [0, 180]")


def _check_tracks(tracks, keypoints):
    n_img = len(tracks.kp_ptr) - 1
    if len(keypoints) != n_img:
        raise ValueError(f"{len(keypoints)} keypoint lists for {n_img} images")
    if tracks.n_obs and (tracks.image.min() < 0 or tracks.image.max() >= n_img):
        raise ValueError("an observation names an image out of range")
    return n_img


def triangulate_tracks_raw(proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp, min_views=2, refine_iters=5,
                           max_error=TRIANGULATION_MAX_ERROR, min_angle_deg=0.0, device=0, robust=False):
    """sfm_triangulate_tracks on flat host arrays, nothing validated but the options (the device treats an image or camera
    index out of range as not registered and a keypoint outside its image as a NaN pixel).  proj [n_cams,12] or [n_cams,3,4]
    K[R|t]; cam_of_image [n_img] (-1: not registered); kp_ptr [n_img+1]; kp_xy [n_nodes,2] pixels by node id; track_ptr,
    obs_image, obs_kp: the CSR arrays of the tracks.  Returns {X [n,3], status int32, n_views int32, max_err, counts [6]}.
    robust=True: sfm_triangulate_tracks_robust (an outlier observation is dropped, not the point); the result gains
    n_inliers [n] int32 and obs_inlier [n_obs] uint8."""
    from ._track_scene import _Scene
    _check_options(min_views, refine_iters, max_error, min_angle_deg)
    sc = _Scene(kp_ptr, kp_xy, np.zeros(0, np.int32), track_ptr, obs_image, obs_kp, device, robust=robust)
    sc.set_cameras(proj, cam_of_image)
    (sc.triangulate_robust if robust else sc.triangulate)(min_views, refine_iters, max_error, min_angle_deg)
    out = {"X": sc.X_tri.cpu().numpy(), "status": sc.status.cpu().numpy(), "n_views": sc.n_views.cpu().numpy(),
           "max_err": sc.max_err.cpu().numpy(), "counts": sc.counts.cpu().numpy()}
    if robust:
        out.update(n_inliers=sc.n_inliers.cpu().numpy(), obs_inlier=sc.obs_inlier_tri[:sc.n_obs].cpu().numpy())
    return out


class Triangulation:
    """The points of a `Tracks` object.  X [n,3] (NaN where there is no point), status [n] (sfm_amd._lib.TRI_*), n_views [n]
    observations in registered images, max_err [n] the largest reprojection error in pixels, counts [6] tracks by status,
    valid = status == 0.  From a robust call: obs_inlier [n_obs] bool, the observations the point was kept with, and
    n_inliers [n] their number per track (max_err is then the largest error of an inlier); otherwise obs_inlier is None and
    n_inliers equals n_views on the valid tracks and is 0 elsewhere."""

    def __init__(self, tracks, uv, cam_of_image, out):
        self.tracks = tracks
        self.cam_of_image = cam_of_image
        self.X, self.status, self.n_views = out["X"], out["status"], out["n_views"]
        self.max_err, self.counts = out["max_err"], out["counts"]
        self.obs_inlier = out["obs_inlier"] != 0 if "obs_inlier" in out else None
        self.n_inliers = out["n_inliers"] if "n_inliers" in out else np.where(self.status == _lib.TRI_OK, self.n_views, 0).astype(np.int32)
        self._uv = uv                                     # [n_obs,2] float64 pixels of the observations

    @property
    def valid(self):
        return self.status == _lib.TRI_OK

    def _valid_observations(self):
        """(selected observation indices, point index of each) over the valid tracks and the registered images; after a
        robust call, over the inlier observations only."""
        tr = self.tracks
        new_id = np.cumsum(self.valid) - 1
        trk = np.repeat(np.arange(len(tr)), tr.lengths())
        keep = self.valid[trk] & (self.cam_of_image[tr.image] >= 0)
        if self.obs_inlier is not None:
            keep &= self.obs_inlier
        sel = np.flatnonzero(keep)
        return sel, new_id[trk[sel]]

    def ba_inputs(self):
        """(pts [m,3], cam_idx int32, pt_idx int32, uv [k,2]) of the valid tracks, restricted to registered cameras - and to
        the inlier observations after a robust call - and point-major: what `GpuBA` and `reproj_errors` take beside the
        camera parameters."""
        sel, pt = self._valid_observations()
        return (self.X[self.valid].copy(), self.cam_of_image[self.tracks.image[sel]].astype(np.int32), pt.astype(np.int32),
                self._uv[sel].copy())


def _cameras(tracks, proj_or_poses, K, registered):
    """(proj [n_cams,12], cam_of_image [n_img] int32) from either form of the cameras."""
    n_img = len(tracks.kp_ptr) - 1
    cam_of_image = np.full(n_img, -1, dtype=np.int32)
    if isinstance(proj_or_poses, dict):
        if K is None:
            raise ValueError("poses need K")
        if registered is not None:
            raise ValueError("`registered` goes with projection matrices; poses are keyed by image id")
        K = np.asarray(K, dtype=np.float64)
        if K.shape != (3, 3):
            raise ValueError("K must be 3 x 3")
        ids = tracks.image_ids if tracks.image_ids is not None else list(range(n_img))
        pos = {v: k for k, v in enumerate(ids)}
        proj = []
        for img_id, (R, t) in proj_or_poses.items():
            if img_id not in pos:
                raise ValueError(f"pose of image {img_id!r}, which the tracks do not know")
            R, t = np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
            if R.shape != (3, 3) or t.size != 3:
                raise ValueError(f"pose of image {img_id!r}: R must be 3 x 3 and t have 3 entries")
            cam_of_image[pos[img_id]] = len(proj)
            proj.append(projection_matrix(K, R, t))
        return np.asarray(proj, dtype=np.float64).reshape(-1, 12), cam_of_image
    proj = np.asarray(proj_or_poses, dtype=np.float64)
    if proj.ndim != 3 or proj.shape[1:] != (3, 4):
        raise ValueError("projections must be [n,3,4]")
    if registered is None:
        if proj.shape[0] != n_img:
            raise ValueError(f"{proj.shape[0]} projections for {n_img} images and no `registered` positions")
        registered = np.arange(n_img)
    registered = np.asarray(registered, dtype=np.int64).reshape(-1)
    if len(registered) != proj.shape[0]:
        raise ValueError("`registered` and the projections differ in length")
    if registered.size and (registered.min() < 0 or registered.max() >= n_img):
        raise ValueError("camera index out of range: a registered position is not one of the images")
    if len(np.unique(registered)) != len(registered):
        raise ValueError("an image is registered twice")
    cam_of_image[registered] = np.arange(len(registered), dtype=np.int32)
    return proj.reshape(-1, 12), cam_of_image


def keypoint_table(tracks, keypoints):
    """kp_xy [n_nodes,2] float64: the pixels by node id (node = kp_ptr[image] + keypoint).  ValueError for an image with
    fewer keypoints than the tracks count or an observation that names a keypoint outside its image."""
    from .twoview import keypoints_xy
    n_img = len(tracks.kp_ptr) - 1
    counts = np.diff(tracks.kp_ptr)
    kp_xy = np.zeros((int(tracks.kp_ptr[-1]), 2), dtype=np.float64)
    for i in range(n_img):
        if counts[i] == 0:
            continue
        kp = keypoints[i]
        # an array keeps its precision (float64 pixels stay float64); keypoint objects go through keypoints_xy (float32)
        xy = np.asarray(kp, dtype=np.float64).reshape(-1, 2) if isinstance(kp, np.ndarray) else \
            np.asarray(keypoints_xy(kp), dtype=np.float64)
        if xy.shape[0] < counts[i]:
            raise ValueError(f"image {i} has {xy.shape[0]} keypoints, the tracks count {counts[i]}")
        kp_xy[tracks.kp_ptr[i]:tracks.kp_ptr[i + 1]] = xy[:counts[i]]
    if tracks.n_obs and (tracks.keypoint.min() < 0 or (tracks.keypoint >= counts[tracks.image]).any()):
        raise ValueError("an observation names a keypoint outside its image")
    return kp_xy


def triangulate_tracks(tracks, keypoints, proj_or_poses, K=None, registered=None, min_views=2, refine_iters=5,
                       max_error=TRIANGULATION_MAX_ERROR, min_angle_deg=0.0, device=0, robust=False):
    """Triangulate every track.  keypoints: per image position what `twoview.keypoints_xy` accepts ([n,2] array or
    cv2.KeyPoints); cameras: [n,3,4] projections K[R|t] with `registered` (the image position of each; default: one per
    image, in order) or a {image_id: (R, t)} dict with K, mapped to positions through `tracks.image_ids`.  An observation in
    an image without a camera is ignored.  robust=True drops outlier observations instead of points (a track that fails is
    searched for a consensus of at least 3 views, see sfm_triangulate_tracks_robust in include/sfm_amd.h) and the
    Triangulation carries obs_inlier.  Everything is validated on the host first (ValueError); returns a Triangulation."""
    _check_options(min_views, refine_iters, max_error, min_angle_deg)
    _check_tracks(tracks, keypoints)
    proj, cam_of_image = _cameras(tracks, proj_or_poses, K, registered)
    kp_xy = keypoint_table(tracks, keypoints)
    out = triangulate_tracks_raw(proj, cam_of_image, tracks.kp_ptr, kp_xy, tracks.track_ptr, tracks.image, tracks.keypoint,
                                 min_views, refine_iters, max_error, min_angle_deg, device, robust=bool(robust))
    uv = kp_xy[tracks.kp_ptr[tracks.image] + tracks.keypoint] if tracks.n_obs else np.zeros((0, 2))
    return Triangulation(tracks, uv, cam_of_image, out)
