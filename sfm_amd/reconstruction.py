"""Drop-in for the reference's `StructureFromMotion.bundle_adjust` and
`compute_reconstruction_stats` (/root/reference/utils/sfm_reconstruction.py:401-549, 582-631).

`BundleAdjustMixin` carries the two methods and reads/writes exactly the state the reference's
methods do (`self.poses`, `self.points3D`, `self.point_tracks`, `self.K`, `self.image_width`,
`self.image_height`), so it can be mixed into the reference class
(`class Fast(BundleAdjustMixin, utils.StructureFromMotion)`) or used through the small
stand-alone `StructureFromMotion` below.  The solve runs on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import logging
from pathlib import Path

import numpy as np

from .driver import DriverMixin
from .interchange import ReconstructionIOMixin
from .pnp import PnPMixin
from .pose import InitialPairMixin
from .rotation import rodrigues, log_so3

BUNDLE_ADJUST_FREQUENCY = 7      # sfm_reconstruction.py:19 (used by the reference's driver loop)


def _flatten_tracks(point_tracks, id_to_idx):
    """(lens [P], cam_idx [N], uv [N,2]) of the observation dicts, point-major over `track.items()`.
    The walk over the Python containers runs inside C iterators (itertools / np.fromiter): ~0.3 s per
    million observations instead of several seconds of per-observation interpreter work."""
    from itertools import chain
    lens = np.fromiter(map(len, point_tracks), dtype=np.int64, count=len(point_tracks))
    n = int(lens.sum())
    cam_idx = np.fromiter(map(id_to_idx.__getitem__, chain.from_iterable(point_tracks)), dtype=np.int64, count=n)
    try:
        uv = np.fromiter(chain.from_iterable(chain.from_iterable(map(dict.values, point_tracks))),
                         dtype=np.float64, count=2 * n).reshape(n, 2)
    except (TypeError, ValueError):
        # pixels stored as something other than flat pairs (e.g. [1,2] arrays): element-wise walk
        uv = np.asarray([np.asarray(p2, dtype=np.float64).ravel() for tr in point_tracks for p2 in tr.values()],
                        dtype=np.float64).reshape(-1, 2)
    return lens, cam_idx, uv


def pack_state(poses, points3D, point_tracks, K, cam_dim=10, order="reference"):
    """The packing step of bundle_adjust (sfm_reconstruction.py:409-451), vectorised where the
    reference loops.  Camera index = insertion order of `poses`; observations point-major over
    `track.items()`.  Returns cams [C,d], pts [P,3], cam_idx, pt_idx, uv (the pixel each
    observation is compared with), ids.

    order="reference" reproduces the reference's residual pairing: projections are stacked
    camera-by-camera (:480-485) while `points2D` stays point-major (:486), so the q-th observation
    in stable camera-sorted order is compared with the q-th point-major pixel.
    order="aligned" compares every observation with its own pixel.
    """
    ids = list(poses.keys())
    id_to_idx = {img_id: i for i, img_id in enumerate(ids)}
    cams = np.zeros((len(ids), cam_dim))
    for i, img_id in enumerate(ids):
        R, t = poses[img_id]
        cams[i, :3] = log_so3(R)
        cams[i, 3:6] = np.asarray(t, dtype=np.float64).reshape(3)
        if cam_dim == 10:
            cams[i, 6:] = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    try:
        pts = np.asarray(points3D, dtype=np.float64)
        if pts.size != 3 * len(points3D):
            raise ValueError
        pts = pts.reshape(-1, 3)
    except (TypeError, ValueError):
        pts = np.asarray([np.asarray(p, dtype=np.float64).ravel() for p in points3D], dtype=np.float64).reshape(-1, 3)
    lens, cam_idx, uv = _flatten_tracks(point_tracks, id_to_idx)
    pt_idx = np.repeat(np.arange(len(point_tracks), dtype=np.int64), lens)
    if order == "reference":
        uv = reference_pairing(uv, cam_idx)
    elif order != "aligned":
        raise ValueError(f"unknown order {order!r}")
    return cams, pts, cam_idx, pt_idx, uv, ids


def reference_pairing(uv, cam_idx):
    """The pixel each observation is compared with under the reference's residual pairing (sfm_reconstruction.py:480-486):
    projections are stacked camera by camera, `points2D` stays point-major, so the q-th observation in stable camera-sorted
    order meets the q-th point-major pixel."""
    uv = np.asarray(uv)
    perm = np.argsort(np.asarray(cam_idx), kind="stable")
    eff = np.empty_like(uv)
    eff[perm] = uv
    return eff


class BundleAdjustMixin:
    """bundle_adjust / compute_reconstruction_stats on the GPU, state contract of the reference."""

    ba_order = "reference"     # bug-compatible residual pairing by default; "aligned" opts out
    ba_cam_dim = 10            # 10 = per-camera intrinsics + regulariser (reference); 6 = fixed K
    ba_device = 0
    ba_precision = "fp64"      # "mixed": float32 storage of the Jacobian rows, float64 sums / S / solve
    ba_options = dict(ftol=1e-4, xtol=1e-4, max_nfev=100)     # sfm_reconstruction.py:509-513
    last_ba_result = None
    last_ba_timing = None      # seconds per phase of the last successful bundle_adjust() call

    def bundle_adjust(self):
        """Perform bundle adjustment optimization (sfm_reconstruction.py:401).
        Returns None on success and False on failure, leaving the state untouched on failure.

        The reference's call site (:689-690, unguarded) never sees an exception from a solver failure:
        SciPy reports it through `res.success` (:517-519).  A damped system that is not positive definite,
        a stalled solve or a non-finite step (SfmNumericError) is therefore logged and returned as False.
        What SciPy itself raises is raised here too (non-finite residuals at the start point: ValueError);
        a missing GPU / library still fails loudly (SfmError)."""
        # The reconstruction state is ~1.3 M small containers at 100k points (track dicts, pixel lists, point lists).  Any
        # full garbage collection that fires while this method allocates (the 200 pose tuples, the K matrices, 100k point
        # lists) walks all of them: 50-100 ms each, several per call on an unlucky allocation count - the 3x spread of the
        # write-back between otherwise identical boxes (round 2: 0.045 vs 0.154 s).  Nothing here creates cycles.
        import gc
        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            return self._bundle_adjust()
        finally:
            if gc_was_on:
                gc.enable()

    def _bundle_adjust(self):
        import time
        from ._lib import SfmNumericError
        from .ba import GpuBA
        t_start = time.perf_counter()
        logging.info("Starting bundle adjustment...")
        if len(self.poses) < 2:
            logging.warning("Not enough cameras for bundle adjustment")
            return False
        try:
            if self.ba_order not in ("reference", "aligned"):
                raise ValueError(f"unknown order {self.ba_order!r}")
            # the reference's pairing (order="reference") is applied by the library on the device (SFM_UV_REFERENCE_PAIRING)
            cams, pts, cam_idx, pt_idx, uv, ids = pack_state(
                self.poses, self.points3D, self.point_tracks, self.K, self.ba_cam_dim, "aligned")
            if len(uv) == 0:
                logging.warning("No points for bundle adjustment")
                return False
        except Exception as e:      # same contract as sfm_reconstruction.py:449-451
            logging.error(f"Error preparing bundle adjustment data: {e}")
            return False
        K0 = (self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2])
        t_packed = time.perf_counter()
        be = GpuBA(cams, pts, cam_idx, pt_idx, uv, K0, float(self.image_width), float(self.image_height),
                   device=self.ba_device, precision=self.ba_precision,
                   uv_pairing="reference" if self.ba_order == "reference" else "as_given")
        x0 = be.x.clone()
        t_built = time.perf_counter()
        try:
            res = be.run_trf(**self.ba_options)      # the loop of sfm_ba_run_trf (library side)
        except SfmNumericError as e:
            if "residuals are not finite" in str(e):
                raise ValueError("Residuals are not finite in the initial point.") from e    # scipy least_squares.py
            logging.warning(f"Bundle adjustment failed to converge: {e}")
            return False
        self.last_ba_result = res
        t_solved = time.perf_counter()
        if not res.success:
            logging.warning("Bundle adjustment failed to converge: "
                            "The maximum number of function evaluations is exceeded.")
            return False
        # the reference logs ||objective(x)||_2 (not the Huber cost) before and after (:522-524)
        cost_initial = self._residual_norm(be, x0)
        cost_final = self._residual_norm(be, be.x)
        logging.info(f"Bundle adjustment: cost reduced from {cost_initial:.2f} to {cost_final:.2f}")
        cams_new, pts_new = be.params()
        if self.ba_cam_dim == 10:
            self.K = np.mean([np.array([[c[6], 0, c[8]], [0, c[7], c[9]], [0, 0, 1]]) for c in cams_new], axis=0)   # :532-538
        for idx, img_id in enumerate(ids):
            self.poses[img_id] = (rodrigues(cams_new[idx, :3]), cams_new[idx, 3:6].copy())
        self.points3D = pts_new.tolist()        # 100k three-element lists (0.012 s with the collector off, see bundle_adjust)
        self.last_ba_timing = {"pack_state": t_packed - t_start, "create_problem_and_upload": t_built - t_packed,
                               "solve": t_solved - t_built, "log_norms_and_write_back": time.perf_counter() - t_solved}
        logging.info("Bundle adjustment completed")

    def _residual_norm(self, be, x):
        """||objective(x)||_2 of the reference's closure: reprojection rows + regulariser rows."""
        err2 = be.residual_norm2(x, shared_k=False)          # summed inside the library: no torch kernel on this path
        if self.ba_cam_dim == 10:
            cams = x[:be.n].reshape(be.C, 10).cpu().numpy()
            p = be.desc
            reg = np.stack([(cams[:, 6] - p.fx0) / p.fx0, (cams[:, 7] - cams[:, 6]) / cams[:, 6],
                            (cams[:, 8] - p.cx0) / p.width, (cams[:, 9] - p.cy0) / p.height]) * p.reg_weight
            err2 += float((reg ** 2).sum())
        return float(np.sqrt(err2))

    def compute_reconstruction_stats(self):
        """Reprojection / track statistics (sfm_reconstruction.py:582-631) with one shared K.  Needs nothing but
        the packed arrays: no Schur structure, no workspace (sfm_reproj_errors)."""
        from .ba import reproj_errors
        n_pts, n_cams = len(self.points3D), len(self.poses)
        lens = np.fromiter(map(len, self.point_tracks), dtype=np.int64, count=len(self.point_tracks))
        if n_pts == 0 or lens.sum() == 0:
            return {'mean_reproj_error': 0, 'max_reproj_error': 0, 'mean_track_length': 0,
                    'max_track_length': 0, 'num_points': n_pts, 'num_cameras': n_cams}
        cams, pts, cam_idx, pt_idx, uv, _ = pack_state(self.poses, self.points3D, self.point_tracks,
                                                       self.K, 6, "aligned")
        K0 = (self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2])
        err = reproj_errors(cams, pts, cam_idx, pt_idx, uv, K0, shared_k=True, device=self.ba_device)
        return {'mean_reproj_error': float(err.mean().item()), 'max_reproj_error': float(err.max().item()),
                'mean_track_length': float(np.mean(lens)), 'max_track_length': float(np.max(lens)),
                'num_points': n_pts, 'num_cameras': n_cams}


class StructureFromMotion(BundleAdjustMixin, DriverMixin, PnPMixin, InitialPairMixin, ReconstructionIOMixin):
    """Minimal stand-alone holder of the reconstruction state (sfm_reconstruction.py:40-59) for
    users who only need the hot path, the driver steps either side of it (sfm_amd.driver), the camera
    registration (sfm_amd.pnp) and the choice and set-up of the initial pair (sfm_amd.pose).  The reference's own
    incremental driver loop stays the reference's; `reconstruct_from_tracks` is the track-based loop of this package."""

    def __init__(self, data_dir=None, order="reference", cam_dim=10, device=0, precision="fp64"):
        self.data_dir = Path(data_dir) if data_dir is not None else None
        if self.data_dir is not None:                       # sfm_reconstruction.py:52-54
            self.matches_dir = self.data_dir / 'matches'
            self.fund_dir = self.data_dir / 'fundamental'
            self.corr_dir = self.data_dir / 'correspondences'
        self.image_width = 1024
        self.image_height = 768
        self.constructed = []
        self.K = np.array([[1228, 0, 512], [0, 1228, 384], [0, 0, 1]], dtype=np.float64)
        self.poses = {}
        self.points3D = []
        self.point_tracks = []
        self.ba_order = order
        self.ba_cam_dim = cam_dim
        self.ba_device = device
        self.ba_precision = precision

    def reconstruct_from_tracks(self, tracks, keypoints, **options):
        """The incremental loop on a `Tracks` object (sfm_amd.incremental.reconstruct_tracks) with `self.K`: fills
        `self.poses` ({image_id: (R, t [3,1])}), `self.points3D` and `self.point_tracks` in the reference's shapes, image
        ids through `tracks.image_ids`, and returns the `Reconstruction`."""
        from .incremental import reconstruct_tracks
        options.setdefault("device", self.ba_device)
        options.setdefault("image_size", (self.image_width, self.image_height))
        rec = reconstruct_tracks(tracks, keypoints, self.K, **options)
        self.poses, self.points3D, self.point_tracks = rec.as_state()
        self.K = rec.K.copy()
        ids = tracks.image_ids if tracks.image_ids is not None else list(range(len(tracks.kp_ptr) - 1))
        self.constructed = [f"{ids[i]:04d}.ppm" for i in rec.order]
        logging.info(f"Registered {len(rec.order)} of {len(ids)} images, {len(self.points3D)} points")
        return rec

    def find_image_pairs(self, image_id):
        """Pairs of `image_id` whose other image is already reconstructed (sfm_reconstruction.py:551-580):
        names come from the match files on disk, in directory order."""
        pairs = []
        for path in self.matches_dir.glob('*.npz'):
            pair = path.stem
            if pair.endswith('_matches'):
                pair = pair.replace('_matches', '')
            if not pair.startswith('pair_'):
                continue
            try:
                id1, id2 = map(int, pair.split('_')[1:3])
            except (ValueError, IndexError):
                logging.warning(f"Skipping file with unexpected name: {path}")
                continue
            other = id2 if id1 == image_id else id1 if id2 == image_id else None
            if other is not None and f"{other:04d}.ppm" in self.constructed:
                pairs.append(pair)
        return pairs
