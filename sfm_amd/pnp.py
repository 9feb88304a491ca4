"""GPU drop-in for the `cv2.solvePnPRansac(points3D, points2D, K, None, iterationsCount=1000, reprojectionError=8.0,
flags=cv2.SOLVEPNP_ITERATIVE)` call with which the reference's incremental loop registers a new camera (`pnp_ransac`,
SURVEY section 3.2), batched over every candidate image of a step: one upload, `sfm_pnp_draw_samples`,
`sfm_pnp_ransac`, one download (sfm_amd/csrc/pnp.hip).

OpenCV's structure as recalled (EPnP on samples of 5 in the loop, reprojection error against the threshold, most
inliers, then the ITERATIVE solver on the inliers) with three deviations: minimal samples of 3 solved by closed-form
P3P with all roots scored, every one of `n_hypotheses` runs (no early exit on confidence), and the samples come from
a stateless integer hash - so the result is a function of (points, K, seed) alone and can be replayed in NumPy
(tests/pnp_reference.py).  No CPU fallback: without the library or a GPU these raise.
"""
from __future__ import annotations

import numpy as np

from . import _ransac
from ._ransac import STATUS_NO_MODEL, STATUS_OK, STATUS_TOO_FEW  # noqa: F401
from .rotation import log_so3

MIN_SAMPLE = 3
MIN_POINTS = 4                      # a sample of 3 and at least one point to tell its roots apart
NO_MODEL = (False, None, None, None)


def solve_pnp_ransac_batched(points3D_list, points2D_list, K, threshold=8.0, n_hypotheses=1024, seed=0, refine=True,
                             samples=None, device=0, return_debug=False):
    """One `(success, rvec, tvec, inliers)` per segment as cv2.solvePnPRansac returns them: rvec, tvec [3,1] float64
    and inliers [k,1] int32 (ascending point indices); `(False, None, None, None)` for a segment with fewer than 4
    points or without a model.  No minimum inlier count is applied here.

    K: one 3x3 matrix or one per segment.  samples: optional list of [n_hypotheses, 3] integer arrays (segment-local
    indices, 3 distinct per row) that replace the generator's draw.  return_debug=True returns `(results, debug)` with
    debug = one dict per segment holding `samples` [n_hypotheses,3] int32, `hyp_count` [n_hypotheses] int32,
    `refined` (bool), `status` (0 ok, 1 fewer than 4 points, 2 no model), `n_inliers`, and `R` [3,3], `t` [3] (None
    without a model)."""
    if len(points3D_list) != len(points2D_list):
        raise ValueError("points3D_list / points2D_list differ in length")
    n_hyp, threshold, seed = _ransac.check_options(n_hypotheses, threshold, seed)
    p3 = [np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in points3D_list]
    p2 = [np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in points2D_list]
    for a, b in zip(p3, p2):
        if a.shape[0] != b.shape[0]:
            raise ValueError("points3D / points2D differ in length")
    n_seg = len(p3)
    lengths = [a.shape[0] for a in p3]
    k4 = _ransac.check_K(K, n_seg)
    smp_h = _ransac.check_samples(samples, lengths, n_hyp, MIN_SAMPLE, MIN_POINTS) if samples is not None else None

    ptr_h, Rt_h, mask_h, meta_h, smp_out, cnt_h = _ransac.run(
        "pnp", MIN_SAMPLE, 12, lengths, [p3, p2], [k4], n_hyp, threshold, seed, refine, smp_h, device, return_debug)
    Rt_h = Rt_h.reshape(n_seg, 3, 4)
    res, poses = [], []
    for s in range(n_seg):
        if meta_h[1, s] != STATUS_OK:
            res.append(NO_MODEL)
            poses.append((None, None))
            continue
        R, t = Rt_h[s, :, :3].copy(), Rt_h[s, :, 3].copy()
        inl = np.flatnonzero(mask_h[ptr_h[s]:ptr_h[s + 1]]).astype(np.int32).reshape(-1, 1)
        res.append((True, log_so3(R).reshape(3, 1), t.reshape(3, 1), inl))
        poses.append((R, t))
    if not return_debug:
        return res
    return res, [{"samples": smp_out[s], "hyp_count": cnt_h[s], "refined": bool(meta_h[2, s]), "status": int(meta_h[1, s]),
                  "n_inliers": int(meta_h[0, s]), "R": poses[s][0], "t": poses[s][1]} for s in range(n_seg)]


def solve_pnp_ransac(points3D, points2D, K, **kw):
    """The single-segment form: `(success, rvec, tvec, inliers)`; with return_debug=True `((...), debug)`."""
    return _ransac.single(solve_pnp_ransac_batched, ([points3D], [points2D], K), kw)


class PnPMixin:
    """Camera registration for the incremental loop: `solve_pnp_ransac` stands in for the cv2.solvePnPRansac call of the
    reference's `pnp_ransac`, `pnp_ransac_candidates` scores every candidate image of a step in one call.  State read:
    `self.K`, `find_2d3d_matches` (DriverMixin).  Nothing is written."""
    device = 0
    pnp_threshold = 8.0          # PNP_REPROJECTION_ERROR
    pnp_hypotheses = 1024        # RANSAC_ITERATIONS = 1000, in whole wavefronts
    pnp_seed = 0
    pnp_min_inliers = 15         # PNP_MIN_INLIERS

    def _pnp_device(self):
        return getattr(self, "ba_device", getattr(self, "device", 0))

    def solve_pnp_ransac(self, points3D, points2D):
        """`(success, rvec, tvec, inliers)` as cv2.solvePnPRansac returns them."""
        return solve_pnp_ransac(points3D, points2D, self.K, threshold=self.pnp_threshold,
                                n_hypotheses=self.pnp_hypotheses, seed=self.pnp_seed, device=self._pnp_device())

    def pnp_ransac_candidates(self, image_ids):
        """{image_id: (R [3,3], t [3,1], inliers [k,1] int32) or None} for the ranked candidates of a step
        (`find_next_best_images`): `find_2d3d_matches` per id, then ONE batched PnP call.  None: fewer than 4 matches,
        no model, or fewer than `pnp_min_inliers` inliers.  `self.poses` is left alone."""
        from .rotation import rodrigues
        image_ids = list(image_ids)
        p3, p2 = [], []
        for image_id in image_ids:
            a, b = self.find_2d3d_matches(image_id)
            p3.append(np.asarray(a, dtype=np.float64).reshape(-1, 3))
            p2.append(np.asarray(b, dtype=np.float32).reshape(-1, 2))
        res = solve_pnp_ransac_batched(p3, p2, self.K, threshold=self.pnp_threshold, n_hypotheses=self.pnp_hypotheses,
                                       seed=self.pnp_seed, device=self._pnp_device())
        out = {}
        for image_id, (ok, rvec, tvec, inl) in zip(image_ids, res):
            if not ok or len(inl) < self.pnp_min_inliers:
                out[image_id] = None
            else:
                out[image_id] = (rodrigues(rvec), tvec, inl)
        return out
