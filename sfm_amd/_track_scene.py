"""The device-resident arrays of one set of tracks and the calls that walk them against the cameras: the one place
that spells sfm_triangulate_tracks, sfm_triangulate_tracks_robust, sfm_tracks_evaluate, sfm_tracks_classify and
sfm_tracks_resection (sfm_amd/csrc/triangulate.hip, resection.hip).  `triangulate_tracks_raw`, `evaluate_tracks`,
`classify_tracks`, `resection_lists` and the loop of `reconstruct_tracks` all go through a `_Scene`.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .driver import _p


class _Scene:
    """Everything stays on the device between calls; the methods return only what the host loop decides on.  Nothing is
    validated here: the device treats an index out of range as not registered or as a NaN pixel."""

    def __init__(self, kp_ptr, kp_xy, node_track, track_ptr, obs_image, obs_kp, device, robust=False):
        import torch
        self.torch = torch
        self.h = _lib.get_handle(device)
        self.dev = dev = torch.device("cuda", device)
        self.n_img, self.n_nodes = len(kp_ptr) - 1, int(np.asarray(kp_xy).reshape(-1, 2).shape[0])
        self.n_tracks, self.n_obs = len(track_ptr) - 1, len(obs_image)
        self.kp_ptr, self.kp_xy = self._up(kp_ptr, np.int64), self._up(np.asarray(kp_xy).reshape(-1, 2), np.float64)
        self.node_track = self._up(node_track, np.int32)
        self.track_ptr, self.obs_image, self.obs_kp = self._up(track_ptr, np.int64), self._up(obs_image, np.int32), self._up(obs_kp, np.int32)
        T = self.n_tracks
        self.X = torch.full((T, 3), float("nan"), dtype=torch.float64, device=dev)
        self.has_point = torch.zeros(T, dtype=torch.uint8, device=dev)
        self.X_tri = torch.empty((T, 3), dtype=torch.float64, device=dev)
        self.status = torch.empty(T, dtype=torch.int32, device=dev)
        self.n_views = torch.empty(T, dtype=torch.int32, device=dev)
        self.max_err = torch.empty(T, dtype=torch.float64, device=dev)
        self.counts = torch.empty(6, dtype=torch.int64, device=dev)
        self.proj = self.cam_of_image = self.ws = None
        self.n_cams = self.ws_bytes = 0
        self.robust = bool(robust)
        if self.robust:
            # per observation: the flag of the loop's state and the flags of the last robust triangulation
            self.obs_inlier = torch.zeros(max(self.n_obs, 1), dtype=torch.uint8, device=dev)
            self.obs_inlier_tri = torch.zeros(max(self.n_obs, 1), dtype=torch.uint8, device=dev)
            self.n_inliers = torch.empty(T, dtype=torch.int32, device=dev)
        self._obs_track = self.ws_res = None

    def _up(self, a, dtype):
        return self.torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(self.dev)      # a copy: inputs may be read-only

    @property
    def obs_track(self):
        """[max(n_obs, 1)] int64: the track of every observation (built on first use)."""
        if self._obs_track is None:
            torch = self.torch
            self._obs_track = torch.zeros(max(self.n_obs, 1), dtype=torch.int64, device=self.dev)
            self._obs_track[:self.n_obs] = torch.repeat_interleave(torch.arange(self.n_tracks, device=self.dev),
                                                                   self.track_ptr[1:] - self.track_ptr[:-1])
        return self._obs_track

    def set_points(self, X, has_point):
        torch = self.torch
        self.X.copy_(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64).reshape(-1, 3)))
        self.has_point.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(has_point) != 0, dtype=np.uint8)))

    def set_cameras(self, proj, cam_of_image):
        """Per step the only upload: proj [n_cams,12] and cam_of_image [n_img].  One workspace serves the four track
        calls: the robust one's holds the camera centres first, as the others' does, and is the larger."""
        proj = np.asarray(proj, dtype=np.float64).reshape(-1, 12)
        self.n_cams = proj.shape[0]
        self.proj, self.cam_of_image = self._up(proj, np.float64), self._up(cam_of_image, np.int32)
        need = C.c_int64()
        if self.robust:
            self.h.check(self.h.lib.sfm_triangulate_tracks_robust_workspace_bytes(self.n_cams, self.n_tracks, C.byref(need)),
                         "sfm_triangulate_tracks_robust_workspace_bytes")
        else:
            self.h.check(self.h.lib.sfm_triangulate_tracks_workspace_bytes(self.n_cams, C.byref(need)),
                         "sfm_triangulate_tracks_workspace_bytes")
        self.ws, self.ws_bytes = self.torch.empty(need.value, dtype=self.torch.uint8, device=self.dev), need.value

    def source(self):
        """The 12 arguments that describe the cameras and the tracks, which the four track calls share after the handle
        (include/sfm_amd.h).  n_img is the length of cam_of_image."""
        return (_p(self.proj), self.n_cams, _p(self.cam_of_image), self.cam_of_image.numel(), _p(self.kp_ptr), _p(self.kp_xy),
                self.n_nodes, _p(self.track_ptr), self.n_tracks, _p(self.obs_image), _p(self.obs_kp), self.n_obs)

    def resection(self):
        """(seg_ptr [n_img+1] int64, corr_node, corr_track int32, corr_X [n,3] float64, corr_uv [n,2] float32) on the host.
        The workspace and the correspondence buffers are allocated by the first call."""
        torch, dev = self.torch, self.dev
        if self.ws_res is None:
            need = C.c_int64()
            self.h.check(self.h.lib.sfm_resection_workspace_bytes(self.n_nodes, C.byref(need)), "sfm_resection_workspace_bytes")
            self.ws_res, self.ws_res_bytes = torch.empty(need.value, dtype=torch.uint8, device=dev), need.value
            self.seg_ptr = torch.empty(self.n_img + 1, dtype=torch.int64, device=dev)
            self.total = torch.empty(1, dtype=torch.int64, device=dev)
            self._corr(int((self.node_track >= 0).sum().item()))
        while True:
            self.h.call("sfm_tracks_resection", _p(self.kp_ptr), self.n_img, self.n_nodes, _p(self.kp_xy), _p(self.node_track),
                        _p(self.cam_of_image), _p(self.X), _p(self.has_point), self.n_tracks, _p(self.seg_ptr),
                        _p(self.corr_node), _p(self.corr_track), _p(self.corr_X), _p(self.corr_uv), self.cap, _p(self.total),
                        _p(self.ws_res), self.ws_res_bytes)
            n = int(self.total.item())
            if n <= self.cap:
                break
            self._corr(n)                                   # cannot happen with cap = every node of a track; kept as a guard
        return (self.seg_ptr.cpu().numpy(), self.corr_node[:n].cpu().numpy(), self.corr_track[:n].cpu().numpy(),
                self.corr_X[:n].cpu().numpy(), self.corr_uv[:n].cpu().numpy())

    def _corr(self, cap):
        torch, dev = self.torch, self.dev
        self.cap = cap
        self.corr_node = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        self.corr_track = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        self.corr_X = torch.empty((max(cap, 1), 3), dtype=torch.float64, device=dev)
        self.corr_uv = torch.empty((max(cap, 1), 2), dtype=torch.float32, device=dev)

    def triangulate(self, min_views, refine_iters, max_error, min_angle_deg):
        """sfm_triangulate_tracks over all tracks into X_tri / status / n_views / max_err / counts (device)."""
        self.h.call("sfm_triangulate_tracks", *self.source(), int(min_views), int(refine_iters), C.c_double(max_error),
                    C.c_double(min_angle_deg), _p(self.X_tri), _p(self.status), _p(self.n_views), _p(self.max_err),
                    _p(self.counts), _p(self.ws), self.ws_bytes)

    def triangulate_robust(self, min_views, refine_iters, max_error, min_angle_deg):
        """sfm_triangulate_tracks_robust over all tracks into X_tri / status / n_views / n_inliers / max_err / counts and
        obs_inlier_tri (device)."""
        self.h.call("sfm_triangulate_tracks_robust", *self.source(), int(min_views), int(refine_iters), C.c_double(max_error),
                    C.c_double(min_angle_deg), _p(self.X_tri), _p(self.status), _p(self.n_views), _p(self.n_inliers),
                    _p(self.max_err), _p(self.obs_inlier_tri), _p(self.counts), _p(self.ws), self.ws_bytes)

    def _judge(self, name, outputs, min_views, max_error, min_angle_deg, want_obs_err):
        obs_err = self.torch.empty(max(self.n_obs, 1), dtype=self.torch.float64, device=self.dev) if want_obs_err else None
        self.h.call(name, *self.source(), _p(self.X), _p(self.has_point), int(min_views), C.c_double(max_error),
                    C.c_double(min_angle_deg), *(_p(t) for t in outputs), _p(obs_err), _p(self.counts), _p(self.ws), self.ws_bytes)
        return obs_err[:self.n_obs] if want_obs_err else None

    def evaluate(self, min_views, max_error, min_angle_deg, want_obs_err=False):
        """sfm_tracks_evaluate at X / has_point into status / n_views / max_err / counts (device); obs_err or None."""
        return self._judge("sfm_tracks_evaluate", (self.status, self.n_views, self.max_err), min_views, max_error,
                           min_angle_deg, want_obs_err)

    def classify(self, min_views, max_error, min_angle_deg, want_obs_err=False):
        """sfm_tracks_classify at X / has_point into status / n_views / n_inliers / max_err / counts and obs_inlier, the
        flags of the loop's state: those of every track that has a point are refreshed, the others are 0."""
        return self._judge("sfm_tracks_classify", (self.status, self.n_views, self.n_inliers, self.max_err, self.obs_inlier),
                           min_views, max_error, min_angle_deg, want_obs_err)

    def adopt_new_points(self, **gates):
        """Triangulate, then adopt the points of status 0 for tracks without a point; existing points stay.  Returns the
        number adopted (one integer comes down).  In the robust mode the adopted tracks take their flags with them."""
        torch = self.torch
        if self.robust:
            self.triangulate_robust(**gates)
        else:
            self.triangulate(**gates)
        new = (self.has_point == 0) & (self.status == _lib.TRI_OK)
        if self.robust:
            self.obs_inlier = torch.where(new[self.obs_track], self.obs_inlier_tri, self.obs_inlier)
        self.X = torch.where(new[:, None], self.X_tri, self.X)
        self.has_point |= new.to(torch.uint8)
        return int(new.sum().item())

    def observations_rejected(self):
        """The observations in registered images, of tracks that have a point, whose flag is 0 (one integer comes down)."""
        if self.n_obs == 0:
            return 0
        used = self.cam_of_image[self.obs_image.long()] >= 0
        return int((used & (self.has_point[self.obs_track[:self.n_obs]] != 0) & (self.obs_inlier[:self.n_obs] == 0)).sum().item())

    def drop_failing_points(self, **gates):
        """Evaluate - in the robust mode: classify - then every point whose status is not 0 loses has_point (and its
        flags).  Returns the number dropped."""
        if self.robust:
            self.classify(**gates)
        else:
            self.evaluate(**gates)
        bad = (self.has_point != 0) & (self.status != _lib.TRI_OK)
        self.has_point &= ~bad.to(self.torch.uint8) & 1
        if self.robust:
            self.obs_inlier &= ~bad[self.obs_track].to(self.torch.uint8) & 1
        return int(bad.sum().item())
