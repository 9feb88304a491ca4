"""GPU drop-in for `cv2.findHomography(pts1, pts2, cv2.RANSAC, 3.0)`, batched over image pairs: one upload,
`sfm_hom_draw_samples`, `sfm_hom_ransac`, one download (sfm_amd/csrc/homography.hip).  The fourth batched RANSAC stage
beside F (twoview.py), E (essential.py) and PnP (pnp.py), and what tells a pair without a defined F - matches on a plane,
cameras that share a centre - from a general one: a homography explains nearly all of such a pair's matches
(`max_homography_ratio` of `reconstruct_tracks`).

OpenCV's structure (samples of 4 with a subset check, the DLT on normalised coordinates, the forward transfer error
`<= threshold**2`, most inliers, `H[2][2] = 1`) with three deviations: every one of `n_hypotheses` runs (no early exit on
confidence), the samples come from a stateless integer hash, so the result is a function of (points, seed) alone and can
be replayed in NumPy (tests/homography_reference.py), and the refit is the linear one over the winner's inliers with no
Levenberg-Marquardt step after it.  No CPU fallback: without the library or a GPU these raise.
"""
from __future__ import annotations

import numpy as np

from . import _ransac
from ._ransac import STATUS_NO_MODEL, STATUS_OK, STATUS_TOO_FEW  # noqa: F401

MIN_SAMPLE = 4


def estimate_homography_batched(pts1_list, pts2_list, threshold=3.0, n_hypotheses=1024, seed=0, refine=True,
                                samples=None, device=0, return_debug=False):
    """One `(H, mask)` per pair as cv2.findHomography returns them: H [3,3] float64 with H[2,2] = 1 (x2 ~ H x1) and mask
    [M,1] uint8; `(None, None)` for a pair with fewer than 4 matches or without a model.

    samples: optional list of [n_hypotheses, 4] integer arrays (segment-local indices, 4 distinct per row) that replace
    the generator's draw.  return_debug=True returns `(results, debug)` with debug = one dict per pair holding `samples`
    [n_hypotheses,4] int32, `hyp_count` [n_hypotheses] int32, `refined` (bool), `status` (0 ok, 1 fewer than 4 matches,
    2 no model) and `n_inliers`."""
    if len(pts1_list) != len(pts2_list):
        raise ValueError("pts1_list / pts2_list differ in length")
    n_hyp, threshold, seed = _ransac.check_options(n_hypotheses, threshold, seed)
    p1 = [np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in pts1_list]
    p2 = [np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in pts2_list]
    for a, b in zip(p1, p2):
        if a.shape[0] != b.shape[0]:
            raise ValueError("pts1 / pts2 differ in length")
    n_seg = len(p1)
    lengths = [a.shape[0] for a in p1]
    smp_h = _ransac.check_samples(samples, lengths, n_hyp, MIN_SAMPLE, MIN_SAMPLE) if samples is not None else None

    ptr_h, H_h, mask_h, meta_h, smp_out, cnt_h = _ransac.run(
        "hom", MIN_SAMPLE, 9, lengths, [p1, p2], [], n_hyp, threshold, seed, refine, smp_h, device, return_debug)
    res = []
    for s in range(n_seg):
        if meta_h[1, s] != STATUS_OK:
            res.append((None, None))
        else:
            res.append((H_h[s].reshape(3, 3).copy(), mask_h[ptr_h[s]:ptr_h[s + 1]].reshape(-1, 1).copy()))
    if not return_debug:
        return res
    return res, [{"samples": smp_out[s], "hyp_count": cnt_h[s], "refined": bool(meta_h[2, s]), "status": int(meta_h[1, s]),
                  "n_inliers": int(meta_h[0, s])} for s in range(n_seg)]


def find_homography(pts1, pts2, threshold=3.0, **kw):
    """The single-pair form: `(H, mask)` or `(None, None)`; with return_debug=True `((H, mask), debug)`."""
    return _ransac.single(estimate_homography_batched, ([pts1], [pts2], threshold), kw)


class HomographyMixin:
    """`find_homography_mat`: cv2.findHomography(pts1, pts2, cv2.RANSAC, 3.0) for one pair."""
    device = 0
    hom_threshold = 3.0
    hom_hypotheses = 1024
    hom_seed = 0

    def find_homography_mat(self, pts1, pts2):
        return find_homography(pts1, pts2, self.hom_threshold, n_hypotheses=self.hom_hypotheses, seed=self.hom_seed,
                               device=getattr(self, "device", 0))
