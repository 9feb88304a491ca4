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

import ctypes as C

import numpy as np

from . import _lib
from .driver import _dev, _p, _ptr_array
from .rotation import log_so3

STATUS_OK, STATUS_TOO_FEW, STATUS_NO_MODEL = 0, 1, 2
MIN_SAMPLE = 3
MIN_POINTS = 4                      # a sample of 3 and at least one point to tell its roots apart
NO_MODEL = (False, None, None, None)


def _check_samples(samples, lengths, n_hyp):
    """Caller-supplied samples -> [n_seg, n_hyp, 3] int32; range and distinctness checked for segments that will run."""
    if len(samples) != len(lengths):
        raise ValueError("samples: one [n_hypotheses, 3] array per segment")
    out = np.full((len(lengths), n_hyp, MIN_SAMPLE), -1, dtype=np.int32)
    for s, (a, m) in enumerate(zip(samples, lengths)):
        if m < MIN_POINTS:
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


def _check_K(K, n_seg):
    """One 3x3 matrix, or one per segment -> [n_seg, 4] float64 (fx, fy, cx, cy)."""
    K = np.asarray(K, dtype=np.float64)
    if K.shape == (3, 3):
        K = np.broadcast_to(K, (n_seg, 3, 3))
    if K.shape != (n_seg, 3, 3):
        raise ValueError(f"K must be one 3x3 matrix or one per segment, got {K.shape}")
    k4 = np.stack([K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2]], axis=1)
    if not np.isfinite(k4).all() or (k4[:, :2] == 0).any():
        raise ValueError("K must be finite with non-zero focal lengths")
    return np.ascontiguousarray(k4)


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
    n_hyp = int(n_hypotheses)
    if n_hyp < 1:
        raise ValueError("n_hypotheses must be at least 1")
    threshold = float(threshold)
    if not (threshold >= 0.0 and np.isfinite(threshold)):
        raise ValueError("threshold must be finite and not negative")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must fit an unsigned 64-bit integer")
    p3 = [np.asarray(a, dtype=np.float64).reshape(-1, 3) for a in points3D_list]
    p2 = [np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in points2D_list]
    for a, b in zip(p3, p2):
        if a.shape[0] != b.shape[0]:
            raise ValueError("points3D / points2D differ in length")
    n_seg = len(p3)
    lengths = [a.shape[0] for a in p3]
    n = int(sum(lengths))
    k4 = _check_K(K, n_seg)
    smp_h = _check_samples(samples, lengths, n_hyp) if samples is not None else None

    def debug_row(smp, cnt, ref, st, ninl, R, t):
        return {"samples": smp, "hyp_count": cnt, "refined": bool(ref), "status": int(st), "n_inliers": int(ninl),
                "R": R, "t": t}

    if n_seg == 0:
        return ([], []) if return_debug else []
    if n == 0:                                     # nothing to upload: every segment is a short one
        res = [NO_MODEL] * n_seg
        dbg = [debug_row(np.full((n_hyp, MIN_SAMPLE), -1, np.int32), np.zeros(n_hyp, np.int32), 0, STATUS_TOO_FEW, 0,
                         None, None) for _ in range(n_seg)]
        return (res, dbg) if return_debug else res

    import torch
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    ptr_h, ptr = _ptr_array(lengths, dev)
    d_X, d_uv = _dev(np.concatenate(p3), np.float64, dev), _dev(np.concatenate(p2), np.float32, dev)
    d_K = _dev(k4, np.float64, dev)
    if smp_h is None:
        d_smp = torch.empty((n_seg, n_hyp, MIN_SAMPLE), dtype=torch.int32, device=dev)
        h.call("sfm_pnp_draw_samples", _p(ptr), n_seg, n_hyp, C.c_uint64(seed), _p(d_smp))
    else:
        d_smp = _dev(smp_h, np.int32, dev)
    need = C.c_int64()
    h.check(h.lib.sfm_pnp_workspace_bytes(n, n_seg, n_hyp, C.byref(need)), "sfm_pnp_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    Rt = torch.empty((n_seg, 12), dtype=torch.float64, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    # n_inliers, status, refined in one block: one download for the three
    meta = torch.empty((3, n_seg), dtype=torch.int32, device=dev)
    hyp_count = torch.empty((n_seg, n_hyp), dtype=torch.int32, device=dev) if return_debug else None
    h.call("sfm_pnp_ransac", _p(ptr), n_seg, _p(d_X), _p(d_uv), n, _p(d_K), _p(d_smp), n_hyp, C.c_double(threshold),
           1 if refine else 0, _p(Rt), _p(mask), _p(meta[0]), _p(meta[1]), _p(hyp_count), _p(meta[2]), _p(ws), need.value)
    Rt_h, mask_h, meta_h = Rt.cpu().numpy().reshape(n_seg, 3, 4), mask.cpu().numpy(), meta.cpu().numpy()
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
    smp_out = d_smp.cpu().numpy() if smp_h is None else smp_h
    cnt_h = hyp_count.cpu().numpy()
    dbg = [debug_row(smp_out[s], cnt_h[s], meta_h[2, s], meta_h[1, s], meta_h[0, s], *poses[s]) for s in range(n_seg)]
    return res, dbg


def solve_pnp_ransac(points3D, points2D, K, **kw):
    """The single-segment form: `(success, rvec, tvec, inliers)`; with return_debug=True `((...), debug)`."""
    if kw.get("samples") is not None:
        kw["samples"] = [kw["samples"]]
    out = solve_pnp_ransac_batched([points3D], [points2D], K, **kw)
    if kw.get("return_debug"):
        return out[0][0], out[1][0]
    return out[0]


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
