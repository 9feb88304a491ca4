"""GPU drop-in for the `cv2.findFundamentalMat(pts1, pts2, cv2.FM_RANSAC, 3.0)` call of the reference's pair loop
(/root/reference/utils/find_matches.py:282), batched over every image pair of a driver step:
one upload, `sfm_fund_draw_samples`, `sfm_fund_ransac`, one download (sfm_amd/csrc/twoview.hip).

OpenCV's structure (7-point samples, max of the two squared point-line distances, `<= threshold**2`, most inliers,
`F[2][2] = 1`) with two deviations: every one of `n_hypotheses` runs (no early exit on confidence) and the samples come
from a stateless integer hash, so the result is a function of (points, seed) alone and can be replayed in NumPy
(tests/fundamental_reference.py).  No CPU fallback: without the library or a GPU these raise.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .driver import _dev, _p, _ptr_array

STATUS_OK, STATUS_TOO_FEW, STATUS_NO_MODEL = 0, 1, 2
MIN_SAMPLE = 7


def _check_samples(samples, lengths, n_hyp):
    """Caller-supplied samples -> [n_seg, n_hyp, 7] int32; range and distinctness checked for pairs that will run."""
    if len(samples) != len(lengths):
        raise ValueError("samples: one [n_hypotheses, 7] array per pair")
    out = np.full((len(lengths), n_hyp, MIN_SAMPLE), -1, dtype=np.int32)
    for s, (a, m) in enumerate(zip(samples, lengths)):
        if m < MIN_SAMPLE:
            continue
        a = np.asarray(a)
        if a.shape != (n_hyp, MIN_SAMPLE) or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"samples[{s}] must be an integer array of shape ({n_hyp}, {MIN_SAMPLE}), got {a.dtype} {a.shape}")
        if a.min() < 0 or a.max() >= m:
            raise ValueError(f"samples[{s}] holds an index outside [0, {m})")
        srt = np.sort(a, axis=1)
        if (srt[:, 1:] == srt[:, :-1]).any():
            raise ValueError(f"samples[{s}] repeats an index within a sample")
        out[s] = a
    return out


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
    n_hyp = int(n_hypotheses)
    if n_hyp < 1:
        raise ValueError("n_hypotheses must be at least 1")
    threshold = float(threshold)
    if not (threshold >= 0.0 and np.isfinite(threshold)):
        raise ValueError("threshold must be finite and not negative")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must fit an unsigned 64-bit integer")
    p1 = [np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in pts1_list]
    p2 = [np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in pts2_list]
    for a, b in zip(p1, p2):
        if a.shape[0] != b.shape[0]:
            raise ValueError("pts1 / pts2 differ in length")
    n_seg = len(p1)
    lengths = [a.shape[0] for a in p1]
    n = int(sum(lengths))
    smp_h = _check_samples(samples, lengths, n_hyp) if samples is not None else None

    def debug_row(s, smp, cnt, ref, st, ninl):
        return {"samples": smp, "hyp_count": cnt, "refined": bool(ref), "status": int(st), "n_inliers": int(ninl)}

    if n_seg == 0:
        return ([], []) if return_debug else []
    if n == 0:                                     # nothing to upload: every pair is a short pair
        res = [(None, None)] * n_seg
        dbg = [debug_row(s, np.full((n_hyp, MIN_SAMPLE), -1, np.int32), np.zeros(n_hyp, np.int32), 0, STATUS_TOO_FEW, 0)
               for s in range(n_seg)]
        return (res, dbg) if return_debug else res

    import torch
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    ptr_h, ptr = _ptr_array(lengths, dev)
    d_p1, d_p2 = _dev(np.concatenate(p1), np.float32, dev), _dev(np.concatenate(p2), np.float32, dev)
    if smp_h is None:
        d_smp = torch.empty((n_seg, n_hyp, MIN_SAMPLE), dtype=torch.int32, device=dev)
        h.call("sfm_fund_draw_samples", _p(ptr), n_seg, n_hyp, C.c_uint64(seed), _p(d_smp))
    else:
        d_smp = _dev(smp_h, np.int32, dev)
    need = C.c_int64()
    h.check(h.lib.sfm_fund_workspace_bytes(n, n_seg, n_hyp, C.byref(need)), "sfm_fund_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    F = torch.empty((n_seg, 9), dtype=torch.float64, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    # n_inliers, status, refined in one block: one download for the three
    meta = torch.empty((3, n_seg), dtype=torch.int32, device=dev)
    hyp_count = torch.empty((n_seg, n_hyp), dtype=torch.int32, device=dev) if return_debug else None
    h.call("sfm_fund_ransac", _p(ptr), n_seg, _p(d_p1), _p(d_p2), n, _p(d_smp), n_hyp, C.c_double(threshold),
           1 if refine else 0, _p(F), _p(mask), _p(meta[0]), _p(meta[1]), _p(hyp_count), _p(meta[2]), _p(ws), need.value)
    F_h, mask_h, meta_h = F.cpu().numpy(), mask.cpu().numpy(), meta.cpu().numpy()
    res = []
    for s in range(n_seg):
        if meta_h[1, s] != STATUS_OK:
            res.append((None, None))
        else:
            res.append((F_h[s].reshape(3, 3).copy(), mask_h[ptr_h[s]:ptr_h[s + 1]].reshape(-1, 1).copy()))
    if not return_debug:
        return res
    smp_out = d_smp.cpu().numpy() if smp_h is None else smp_h
    cnt_h = hyp_count.cpu().numpy()
    dbg = [debug_row(s, smp_out[s], cnt_h[s], meta_h[2, s], meta_h[1, s], meta_h[0, s]) for s in range(n_seg)]
    return res, dbg


def find_fundamental(pts1, pts2, threshold=3.0, **kw):
    """The single-pair form: `(F, mask)` or `(None, None)`; with return_debug=True `((F, mask), debug)`."""
    if kw.get("samples") is not None:
        kw["samples"] = [kw["samples"]]
    out = estimate_fundamental_batched([pts1], [pts2], threshold, **kw)
    if kw.get("return_debug"):
        return out[0][0], out[1][0]
    return out[0]


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
