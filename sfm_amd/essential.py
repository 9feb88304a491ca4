"""GPU drop-in for `cv2.findEssentialMat(pts1, pts2, K, cv2.RANSAC, threshold=3.0)`, batched over image pairs: one
upload, `sfm_ess_draw_samples`, `sfm_ess_ransac`, one download (sfm_amd/csrc/essential.hip).  The calibrated
counterpart of `estimate_fundamental_batched` for callers that go on to a pose: `recover_pose_batched(E, ...,
from_fundamental=False)`.

OpenCV's structure (5-point samples solved by Nister's algorithm, most inliers) with three deviations: the error rule
is the fundamental stage's, in pixels on `K^-T E K^-1` (the larger of the two squared point-line distances,
`<= threshold**2`); every one of `n_hypotheses` runs (no early exit on confidence); and the samples come from a
stateless integer hash, so the result is a function of (points, K, seed) alone and can be replayed in NumPy
(tests/essential_reference.py).  No CPU fallback: without the library or a GPU these raise.
"""
from __future__ import annotations

import numpy as np

from . import _ransac
from ._ransac import STATUS_NO_MODEL, STATUS_OK, STATUS_TOO_FEW  # noqa: F401

MIN_SAMPLE = 5


def estimate_essential_batched(pts1_list, pts2_list, K, threshold=3.0, n_hypotheses=1024, seed=0, refine=True,
                               samples=None, device=0, return_debug=False):
    """One `(E, mask)` per pair as cv2.findEssentialMat returns them: E [3,3] float64 in normalised coordinates with
    |E|_F = sqrt(2) and its entry of largest magnitude positive, and mask [M,1] uint8; `(None, None)` for a pair with
    fewer than 5 matches or without a model.  K: one 3x3 matrix, or one per pair; threshold in pixels.

    samples: optional list of [n_hypotheses, 5] integer arrays (segment-local indices, 5 distinct per row) that replace
    the generator's draw.  return_debug=True returns `(results, debug)` with debug = one dict per pair holding `samples`
    [n_hypotheses,5] int32, `hyp_count` [n_hypotheses] int32, `refined` (bool), `status` (0 ok, 1 fewer than 5 matches,
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
    k4 = _ransac.check_K(K, n_seg)
    lengths = [a.shape[0] for a in p1]
    smp_h = _ransac.check_samples(samples, lengths, n_hyp, MIN_SAMPLE, MIN_SAMPLE) if samples is not None else None

    ptr_h, E_h, mask_h, meta_h, smp_out, cnt_h = _ransac.run(
        "ess", MIN_SAMPLE, 9, lengths, [p1, p2], [k4], n_hyp, threshold, seed, refine, smp_h, device, return_debug)
    res = []
    for s in range(n_seg):
        if meta_h[1, s] != STATUS_OK:
            res.append((None, None))
        else:
            res.append((E_h[s].reshape(3, 3).copy(), mask_h[ptr_h[s]:ptr_h[s + 1]].reshape(-1, 1).copy()))
    if not return_debug:
        return res
    return res, [{"samples": smp_out[s], "hyp_count": cnt_h[s], "refined": bool(meta_h[2, s]), "status": int(meta_h[1, s]),
                  "n_inliers": int(meta_h[0, s])} for s in range(n_seg)]


def find_essential(pts1, pts2, K, threshold=3.0, **kw):
    """The single-pair form: `(E, mask)` or `(None, None)`; with return_debug=True `((E, mask), debug)`."""
    return _ransac.single(estimate_essential_batched, ([pts1], [pts2], K, threshold), kw)


class EssentialMixin:
    """`find_essential_mat`: cv2.findEssentialMat(pts1, pts2, K, cv2.RANSAC, threshold) with the object's `K`."""
    device = 0
    ess_threshold = 3.0
    ess_hypotheses = 1024
    ess_seed = 0

    def find_essential_mat(self, pts1, pts2):
        return find_essential(pts1, pts2, self.K, self.ess_threshold, n_hypotheses=self.ess_hypotheses,
                              seed=self.ess_seed, device=getattr(self, "device", 0))
