"""GPU drop-in for the `cv2.findFundamentalMat(pts1, pts2, cv2.FM_RANSAC, 3.0)` call of the reference's pair loop
(/root/reference/utils/find_matches.py:282), batched over every image pair of a driver step:
one upload, `sfm_fund_draw_samples`, `sfm_fund_ransac`, one download (sfm_amd/csrc/twoview.hip).

OpenCV's structure (7-point samples, max of the two squared point-line distances, `<= threshold**2`, most inliers,
`F[2][2] = 1`) with two deviations: every one of `n_hypotheses` runs (no early exit on confidence) and the samples come
from a stateless integer hash, so the result is a function of (points, seed) alone and can be replayed in NumPy
(tests/fundamental_reference.py).  No CPU fallback: without the library or a GPU these raise.
"""
from __future__ import annotations

import numpy as np

from . import _ransac
from ._ransac import STATUS_NO_MODEL, STATUS_OK, STATUS_TOO_FEW  # noqa: F401

MIN_SAMPLE = 7


def estimate_fundamental_batched(pts1_list, pts2_list, threshold=3.0, n_hypotheses=1024, seed=0, refine=True,
                                 samples=None, device=0, return_debug=False):
    """One `(F, mask)` per pair as cv2.findFundamentalMat returns them: F [3,3] float64 with F[2,2] = 1 and mask [M,1]
    uint8; `(None, None)` for a pair with fewer than 7 matches or without a model.

    samples: optional list of [n_hypotheses, 7] integer arrays (segment-local indices, 7 distinct per row) that replace
    the generator's draw.  return_debug=True returns `(results, debug)` with debug = one dict per pair holding `samples`
    [n_hypotheses,7] int32, `hyp_count` [n_hypotheses] int32, `refined` (bool), `status` (0 ok, 1 fewer than 7 matches,
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

    ptr_h, F_h, mask_h, meta_h, smp_out, cnt_h = _ransac.run(
        "fund", MIN_SAMPLE, 9, lengths, [p1, p2], [], n_hyp, threshold, seed, refine, smp_h, device, return_debug)
    res = []
    for s in range(n_seg):
        if meta_h[1, s] != STATUS_OK:
            res.append((None, None))
        else:
            res.append((F_h[s].reshape(3, 3).copy(), mask_h[ptr_h[s]:ptr_h[s + 1]].reshape(-1, 1).copy()))
    if not return_debug:
        return res
    return res, [{"samples": smp_out[s], "hyp_count": cnt_h[s], "refined": bool(meta_h[2, s]), "status": int(meta_h[1, s]),
                  "n_inliers": int(meta_h[0, s])} for s in range(n_seg)]


def find_fundamental(pts1, pts2, threshold=3.0, **kw):
    """The single-pair form: `(F, mask)` or `(None, None)`; with return_debug=True `((F, mask), debug)`."""
    return _ransac.single(estimate_fundamental_batched, ([pts1], [pts2], threshold), kw)


class FundamentalMixin:
    """`find_fundamental_mat`: what the reference's pair loop gets from cv2.findFundamentalMat (find_matches.py:282)."""
    device = 0
    fund_threshold = 3.0
    fund_hypotheses = 1024
    fund_seed = 0

    def find_fundamental_mat(self, pts1, pts2):
        return find_fundamental(pts1, pts2, self.fund_threshold, n_hypotheses=self.fund_hypotheses,
                                seed=self.fund_seed, device=getattr(self, "device", 0))


def keypoints_xy(kp):
    """[n,2] float32 pixel coordinates of one image's keypoints: an array, or objects with `.pt` (cv2.KeyPoint)."""
    if kp is None:
        return np.zeros((0, 2), np.float32)
    if isinstance(kp, np.ndarray):
        return np.asarray(kp, dtype=np.float32).reshape(-1, 2)
    return np.asarray([k.pt if hasattr(k, "pt") else k for k in kp], dtype=np.float32).reshape(-1, 2)
