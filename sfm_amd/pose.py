"""GPU drop-in for the `cv2.recoverPose(E, pts1, pts2, K)` call with which the reference chooses and sets up its
initial pair (`find_best_initial_pair`, `initialize_reconstruction`), batched over every image pair
of a data set: one upload, `sfm_pose_recover`, one download (sfm_amd/csrc/pose.hip).

opencv-python 4.11's `recoverPose` / `decomposeEssentialMat` as RECALLED (cv2 cannot be imported where this project is
built; the reference's own shipped run pins the row, tests/pose_reference.py): points normalised with K, the four
candidates `[R1|t], [R2|t], [R1|-t], [R2|-t]` of E = U S V^T, every point triangulated against `[I|0]` by DLT, good when
in front of both cameras and nearer than `distance_threshold`, the first candidate with the largest count wins.  The
order of the four follows the sign choices of this library's own decomposition, so a TIE between candidates may be
resolved differently from cv2.  No CPU fallback: without the library or a GPU these raise.
"""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np

from . import _lib
from .driver import _dev, _p, _ptr_array
from ._ransac import check_K

STATUS_OK, STATUS_EMPTY, STATUS_NO_MODEL = 0, 1, 2
NO_MODEL = (0, None, None, None)


def recover_pose_batched(E_list, pts1_list, pts2_list, K, masks=None, distance_threshold=50.0, from_fundamental=False,
                         triangulate=False, device=0, return_debug=False):
    """One `(n_good, R, t, mask)` per pair as cv2.recoverPose returns them: R [3,3] and t [3,1] float64, mask [M,1] uint8
    (255 / 0); `(0, None, None, None)` for a pair without points or without a model (E not finite, or of rank < 2).

    E_list: one 3x3 matrix per pair - essential matrices, or with from_fundamental=True fundamental matrices
    (E = K^T F K is formed on the device).  K: one 3x3 matrix or one per pair (skew is taken as 0).  masks: optional list
    of per-point arrays (None entries allowed); a zero entry takes its point out of the count and out of the mask.
    triangulate=True appends a fifth element: the [n_good,3] float64 points of the winner's good correspondences in
    input order, triangulated in pixel coordinates with K [I|0], K [R|t] (None without a model).
    return_debug=True returns `(results, debug)` with debug = one dict per pair holding `cand_count` [4] int32,
    `cand_pose` [4,3,4] float64 (rows [R|t]; NaN without a model), `winner` and `status` (0 ok, 1 no points,
    2 no model)."""
    n_seg = len(E_list)
    if not (len(pts1_list) == n_seg and len(pts2_list) == n_seg):
        raise ValueError("E_list / pts1_list / pts2_list differ in length")
    dist = float(distance_threshold)
    if np.isnan(dist):
        raise ValueError("distance_threshold must not be NaN")
    p1 = [np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in pts1_list]
    p2 = [np.asarray(a, dtype=np.float32).reshape(-1, 2) for a in pts2_list]
    for a, b in zip(p1, p2):
        if a.shape[0] != b.shape[0]:
            raise ValueError("pts1 / pts2 differ in length")
    lengths = [a.shape[0] for a in p1]
    n = int(sum(lengths))
    Es = []
    for s, E in enumerate(E_list):
        E = np.asarray(E, dtype=np.float64)
        if E.shape != (3, 3):
            raise ValueError(f"E_list[{s}] must be a 3x3 matrix, got {E.shape}")
        Es.append(E.reshape(9))
    mask_h = None
    if masks is not None:
        if len(masks) != n_seg:
            raise ValueError("masks: one array per pair (or None)")
        mask_h = np.ones(n, dtype=np.uint8)
        ptr0 = np.concatenate([[0], np.cumsum(lengths)])
        for s, m in enumerate(masks):
            if m is None:
                continue
            m = np.asarray(m).reshape(-1)
            if m.shape[0] != lengths[s]:
                raise ValueError(f"masks[{s}] has {m.shape[0]} entries for {lengths[s]} points")
            mask_h[ptr0[s]:ptr0[s + 1]] = m != 0
    nothing = NO_MODEL + ((None,) if triangulate else ())

    def debug_row(cnt, pose, win, st):
        return {"cand_count": cnt, "cand_pose": pose, "winner": int(win), "status": int(st)}

    if n_seg == 0:
        return ([], []) if return_debug else []
    k4 = check_K(K, n_seg)
    if n == 0:                                     # nothing to upload: every pair is an empty one
        res = [nothing] * n_seg
        dbg = [debug_row(np.zeros(4, np.int32), np.full((4, 3, 4), np.nan), 0, STATUS_EMPTY) for _ in range(n_seg)]
        return (res, dbg) if return_debug else res

    import torch
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    ptr_h, ptr = _ptr_array(lengths, dev)
    d_p1, d_p2 = _dev(np.concatenate(p1), np.float32, dev), _dev(np.concatenate(p2), np.float32, dev)
    d_E, d_K = _dev(np.stack(Es), np.float64, dev), _dev(k4, np.float64, dev)
    d_mask = _dev(mask_h, np.uint8, dev) if mask_h is not None else None
    need = C.c_int64()
    h.check(h.lib.sfm_pose_workspace_bytes(n, n_seg, C.byref(need)), "sfm_pose_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    Rt = torch.empty((n_seg, 12), dtype=torch.float64, device=dev)           # R [n_seg,9] then t [n_seg,3], one download
    R, t = Rt.view(-1)[:9 * n_seg], Rt.view(-1)[9 * n_seg:]
    meta = torch.empty((3, n_seg), dtype=torch.int32, device=dev)            # n_good, status, winner
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    X = torch.empty((n, 3), dtype=torch.float64, device=dev) if triangulate else None
    cnt = torch.empty((n_seg, 4), dtype=torch.int32, device=dev) if return_debug else None
    pose = torch.empty((n_seg, 4, 12), dtype=torch.float64, device=dev) if return_debug else None
    h.call("sfm_pose_recover", _p(ptr), n_seg, _p(d_p1), _p(d_p2), n, _p(d_E), 1 if from_fundamental else 0, _p(d_K),
           _p(d_mask), C.c_double(dist), _p(R), _p(t), _p(meta[0]), _p(meta[1]), _p(mask), _p(X), _p(cnt), _p(pose),
           _p(meta[2]), _p(ws), need.value)
    Rt_h, meta_h, mask_o = Rt.cpu().numpy().reshape(-1), meta.cpu().numpy(), mask.cpu().numpy()
    R_h, t_h = Rt_h[:9 * n_seg].reshape(n_seg, 3, 3), Rt_h[9 * n_seg:].reshape(n_seg, 3, 1)
    X_h = X.cpu().numpy() if triangulate else None
    res = []
    for s in range(n_seg):
        if meta_h[1, s] != STATUS_OK:
            res.append(nothing)
            continue
        m = mask_o[ptr_h[s]:ptr_h[s + 1]]
        row = (int(meta_h[0, s]), R_h[s].copy(), t_h[s].copy(), m.reshape(-1, 1).copy())
        if triangulate:
            row += (X_h[ptr_h[s]:ptr_h[s + 1]][m != 0].copy(),)
        res.append(row)
    if not return_debug:
        return res
    cnt_h, pose_h = cnt.cpu().numpy(), pose.cpu().numpy().reshape(n_seg, 4, 3, 4)
    return res, [debug_row(cnt_h[s], pose_h[s], meta_h[2, s], meta_h[1, s]) for s in range(n_seg)]


def recover_pose(E, pts1, pts2, K, **kw):
    """The single-pair form: `(n_good, R, t, mask)`; with return_debug=True `((...), debug)`."""
    if kw.get("masks") is not None:
        kw["masks"] = [kw["masks"]]
    out = recover_pose_batched([E], [pts1], [pts2], K, **kw)
    if kw.get("return_debug"):
        return out[0][0], out[1][0]
    return out[0]


class InitialPairMixin:
    """The start of the incremental loop: what the reference's `find_best_initial_pair` and
    `initialize_reconstruction` compute, with ONE batched call over all pairs instead of one cv2.recoverPose per pair.
    State read: `self.K`, `self.fund_dir`, `self.corr_dir`; `initialize_from_pair` writes `self.poses`,
    `self.points3D`, `self.point_tracks`, `self.constructed`."""
    device = 0
    pose_distance_threshold = 50.0       # the distanceThresh cv2.recoverPose is called with by default

    def _pose_device(self):
        return getattr(self, "ba_device", getattr(self, "device", 0))

    def _load_pair(self, pair):
        """(F, pts1, pts2) of one pair: F from fundamental/{pair}_F.npz, the inlier correspondences from
        correspondences/{pair}_pts{1,2}.npy (save_pair_data, interchange.py)."""
        with np.load(self.fund_dir / f'{pair}_F.npz', allow_pickle=False) as z:
            F = np.asarray(z['F'], dtype=np.float64)
        pts1 = np.load(self.corr_dir / f'{pair}_pts1.npy', allow_pickle=False)
        pts2 = np.load(self.corr_dir / f'{pair}_pts2.npy', allow_pickle=False)
        if F.shape != (3, 3) or pts1.ndim != 2 or pts1.shape[1] != 2 or pts1.shape != pts2.shape:
            raise ValueError(f"expected a 3x3 F and two [n,2] arrays, got {F.shape} / {pts1.shape} / {pts2.shape}")
        return F, pts1, pts2

    def initial_pair_candidates(self, pairs):
        """[(pair, n_good)] for every readable pair, in the order given: E = K^T F K and recoverPose on the pair's
        inlier correspondences, all pairs in one call.  Unreadable pairs are skipped with a warning."""
        names, Fs, p1, p2 = [], [], [], []
        for pair in pairs:
            try:
                F, a, b = self._load_pair(pair)
            except (FileNotFoundError, ValueError, KeyError, OSError) as e:
                logging.warning(f"Failed to process pair {pair}: {e}")
                continue
            names.append(pair); Fs.append(F); p1.append(a); p2.append(b)
        if not names:
            return []
        res = recover_pose_batched(Fs, p1, p2, self.K, distance_threshold=self.pose_distance_threshold,
                                   from_fundamental=True, device=self._pose_device())
        return [(pair, int(r[0])) for pair, r in zip(names, res)]

    def select_initial_pair(self, pairs):
        """The first pair with the largest count, or None when no pair could be read."""
        best, best_n = None, -1
        for pair, n_good in self.initial_pair_candidates(pairs):
            if n_good > best_n:
                best, best_n = pair, n_good
        return best

    def initialize_from_pair(self, pair):
        """Poses of the two images (the first at the origin), the triangulated good correspondences and their tracks, as
        the reference's initialize_reconstruction leaves them.  Returns True, or False when the pair gives no model."""
        F, pts1, pts2 = self._load_pair(pair)
        id1, id2 = map(int, pair.split('_')[1:3])
        n_good, R, t, mask, X = recover_pose_batched([F], [pts1], [pts2], self.K,
                                                     distance_threshold=self.pose_distance_threshold,
                                                     from_fundamental=True, triangulate=True,
                                                     device=self._pose_device())[0]
        if R is None:
            logging.warning(f"No pose for pair {pair}")
            return False
        keep = np.flatnonzero(mask.ravel())
        self.poses = {id1: (np.eye(3), np.zeros((3, 1))), id2: (R, t)}
        # cv2.triangulatePoints returns its input's type: the shipped run holds float32-rounded points
        self.points3D = list(X.astype(np.float32).astype(np.float64))
        self.point_tracks = [{id1: pts1[k].tolist(), id2: pts2[k].tolist()} for k in keep]
        self.constructed = [f"{id1:04d}.ppm", f"{id2:04d}.ppm"]
        return True
