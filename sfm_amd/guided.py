"""Guided matching: match again under each pair's fundamental matrix, looking only along the epipolar line
(sfm_guided_match of libsfm_amd.so; what COLMAP calls guided matching).  The blind matcher's ratio test compares a
feature with the whole other image and discards every descriptor that repeats there; under F it competes with the few
keypoints near its epipolar line only.  No CPU fallback."""
from __future__ import annotations

import ctypes as C
from numbers import Real

import numpy as np

from . import _lib

HAMMING_DIMS = (16, 32, 64)
L2_DIMS = (32, 64, 128)


def _empty():
    return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)


def check_arguments(keypoints, descs, pairs, Fs, gate=3.0, ratio=0.75, max_distance=None, metric="auto"):
    """Everything about a guided_match_pairs call that can be judged without a device.  Returns (pairs as int tuples,
    per-image [n,2] float32 keypoints or None, per-image descriptor arrays or None, per-pair [9] float64 F or None, metric
    code, dim, whether float32 sets have to be converted).  ValueError says what is wrong."""
    from .twoview import keypoints_xy
    pairs = [(int(i), int(j)) for i, j in pairs]
    if len(keypoints) != len(descs):
        raise ValueError(f"keypoints / descs differ in length ({len(keypoints)} / {len(descs)})")
    if len(Fs) != len(pairs):
        raise ValueError(f"pairs / Fs differ in length ({len(pairs)} / {len(Fs)})")
    if metric not in ("auto", "l2", "hamming"):
        raise ValueError(f"unknown metric {metric!r}")
    if not (isinstance(gate, Real) and gate >= 0):
        raise ValueError("gate must be a number of pixels >= 0")
    if not isinstance(ratio, Real) or ratio != ratio:
        raise ValueError("ratio must be a number")
    if max_distance is not None and not (isinstance(max_distance, Real) and max_distance >= 0):
        raise ValueError("max_distance must be None or a number >= 0")
    n_img = len(descs)
    xy, dd = [None] * n_img, [None] * n_img
    dim = dtype = None
    for k in range(n_img):
        d = descs[k]
        n_d = 0 if d is None else int(np.asarray(d).shape[0])
        p = keypoints_xy(keypoints[k])
        if p.shape[0] != n_d:
            raise ValueError(f"image {k}: {p.shape[0]} keypoints but {n_d} descriptors")
        if n_d == 0:
            continue
        d = np.ascontiguousarray(d)
        if d.ndim != 2:
            raise ValueError(f"image {k}: descriptors must be [n, dim]")
        if d.dtype not in (np.uint8, np.float32):
            raise ValueError(f"image {k}: descriptors must be uint8 or float32, not {d.dtype}")
        if dim is None:
            dim, dtype = int(d.shape[1]), d.dtype
        elif (int(d.shape[1]), d.dtype) != (dim, dtype):
            raise ValueError("descriptor sets must be [n, dim] arrays of one dtype and dim")
        xy[k], dd[k] = np.ascontiguousarray(p), d
    for i, j in pairs:
        if not (0 <= i < n_img and 0 <= j < n_img):
            raise ValueError(f"pair ({i}, {j}) names an image outside 0..{n_img - 1}")
    F9 = []
    for F in Fs:
        if F is None:
            F9.append(None)
            continue
        F = np.asarray(F, dtype=np.float64)
        if F.size != 9:
            raise ValueError("every F must be 3 x 3 (or None)")
        F9.append(F.reshape(9).copy())
    code, convert = None, False
    if dim is not None:
        if metric == "auto":
            metric = "hamming" if dtype == np.uint8 and dim <= 64 else "l2"
        if metric == "hamming":
            if dtype != np.uint8:
                raise ValueError("hamming needs uint8 descriptors")
            if dim not in HAMMING_DIMS:
                raise ValueError(f"guided matching supports Hamming descriptors of {HAMMING_DIMS} bytes, not {dim}")
            code = _lib.METRIC_HAMMING
        else:
            if dim not in L2_DIMS:
                raise ValueError(f"guided matching supports L2 descriptors of dim {L2_DIMS}, not {dim}")
            code = _lib.METRIC_L2_U8
            if dtype == np.float32:
                # the device converts (sfm_match_f32_to_u8); what it would refuse is refused here already, with the reason
                for k, d in enumerate(dd):
                    if d is not None and not bool(((d == np.rint(d)) & (d >= 0) & (d <= 255)).all()):
                        raise ValueError(f"image {k}: guided matching runs on uint8 descriptors; a float32 set is taken only "
                                         "if every value is an integer in [0, 255] (what SIFT emits), and this one is not")
                convert = True
    return pairs, xy, dd, F9, code, dim, convert


def guided_match_pairs(keypoints, descs, pairs, Fs, gate=3.0, ratio=0.75, max_distance=None, cross_check=False, metric="auto",
                       device=0, return_debug=False):
    """Guided matches of MANY image pairs in one call.

    keypoints / descs: per image an [n,2] array of pixels (or objects with `.pt`) and its descriptor array (None = an image
    without keypoints); pairs: (i, j) = image i's keypoints are the queries, image j's the candidates; Fs: per pair the 3 x 3
    fundamental matrix with x_j^T F x_i = 0 (what estimate_fundamental_batched / process_pairs return), or None.
    For a query q the candidates are C(q) = { t : both point-line distances of (q, t) under F are <= gate pixels } (float64,
    sfm_amd/csrc/guided_rule.h).  best / second = the two smallest (distance, t) over C(q); q is kept iff C(q) is not empty,
    d1 <= max_distance (when given), |C(q)| == 1 or d1 < ratio * d2 (as the matcher compares: in double, strictly), and -
    with cross_check - q is in turn the best of { q' : gate(q', best) } by (distance, q').  Without cross_check a train
    keypoint may be matched by several queries.

    Returns one (queryIdx, trainIdx, distance) triple of NumPy arrays (int32, int32, float32; query order) per pair; empty
    arrays for a pair whose F is None or that has an empty side.  One train keypoint is legal: a single candidate needs no
    ratio test.  With return_debug also the number of candidates |C(q)| of every query, per pair (int32 [n_i]).
    uint8 descriptors: Hamming (16 / 32 / 64 bytes) or L2 (dim 32 / 64 / 128); float32 sets are converted if all their
    values are integers in [0, 255] and refused (ValueError) otherwise."""
    csr = guided_match_csr(keypoints, descs, pairs, Fs, gate, ratio, max_distance, cross_check, metric, device, return_debug)
    out = [_empty() for _ in pairs]
    dbg = [np.zeros(n, np.int32) for n in csr["n_queries"]]
    sp, row = csr["seg_ptr"], 0
    for k, s in enumerate(csr["live"]):
        a, b = int(sp[k]), int(sp[k + 1])
        out[s] = (csr["queryIdx"][a:b], csr["trainIdx"][a:b], csr["distance"][a:b])
        if return_debug:
            dbg[s] = csr["n_candidates"][row:row + csr["n_queries"][s]]
            row += csr["n_queries"][s]
    return (out, dbg) if return_debug else out


def guided_match_csr(keypoints, descs, pairs, Fs, gate=3.0, ratio=0.75, max_distance=None, cross_check=False, metric="auto",
                     device=0, with_candidates=True):
    """The arrays of one sfm_guided_match call as the device leaves them (guided_match_pairs cuts them up): a dictionary with
    'live' (the positions in `pairs` of the pairs that have an F: the segments of the call, in order), 'queryIdx' /
    'trainIdx' / 'distance' (all matches back to back), 'seg_ptr' (int64 [len(live) + 1]: segment k's matches are
    [seg_ptr[k], seg_ptr[k+1])), 'n_candidates' (int32, one per query row of the live pairs, or None) and 'n_queries'
    (keypoints of the query image of every pair)."""
    pairs, xy, dd, F9, code, dim, convert = check_arguments(keypoints, descs, pairs, Fs, gate, ratio, max_distance, metric)
    sizes = [0 if d is None else d.shape[0] for d in dd]
    # pairs with an empty side stay in the batch (the device gives them no match): one code path for every size
    live = [s for s in range(len(pairs)) if F9[s] is not None] if dim is not None else []
    res = {"live": live, "n_queries": [sizes[i] for i, _ in pairs], "queryIdx": _empty()[0], "trainIdx": _empty()[1],
           "distance": _empty()[2], "seg_ptr": np.zeros(len(live) + 1, np.int64),
           "n_candidates": np.zeros(0, np.int32) if with_candidates else None}
    if not live:
        return res
    import torch
    from .matcher import _upload_sets
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    used = sorted({img for s in live for img in pairs[s]})
    slot = {img: k for k, img in enumerate(used)}
    none_d, none_p = np.zeros((0, dim), next(d.dtype for d in dd if d is not None)), np.zeros((0, 2), np.float32)
    rows, ptr, _ = _upload_sets([none_d if dd[i] is None else dd[i] for i in used], dev)
    pts, _, _ = _upload_sets([none_p if xy[i] is None else xy[i] for i in used], dev)
    dp = lambda t: C.c_void_p(t.data_ptr())
    hp = lambda a: C.c_void_p(a.ctypes.data)
    if convert:
        flag = torch.ones(1, dtype=torch.int32, device=dev)
        rows8 = torch.empty(rows.shape, dtype=torch.uint8, device=dev)
        h.call("sfm_match_f32_to_u8", dp(rows), rows.numel(), dp(rows8), dp(flag))
        if int(flag.item()) != 1:
            raise ValueError("guided matching runs on uint8 descriptors: a float32 set holds a value that is no integer in [0, 255]")
        rows = rows8
    n_seg = len(live)
    q_beg = np.array([ptr[slot[pairs[s][0]]] for s in live], dtype=np.int64)
    q_end = np.array([ptr[slot[pairs[s][0]] + 1] for s in live], dtype=np.int64)
    t_beg = np.array([ptr[slot[pairs[s][1]]] for s in live], dtype=np.int64)
    t_end = np.array([ptr[slot[pairs[s][1]] + 1] for s in live], dtype=np.int64)
    d_F = torch.from_numpy(np.stack([F9[s] for s in live])).to(dev)
    n_out, need = C.c_int64(), C.c_int64()
    h.check(h.lib.sfm_guided_workspace_bytes(code, n_seg, hp(q_beg), hp(q_end), hp(t_beg), hp(t_end), C.byref(n_out), C.byref(need)),
            "sfm_guided_workspace_bytes")
    n = n_out.value
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    qi = torch.empty(n, dtype=torch.int32, device=dev)
    ti = torch.empty(n, dtype=torch.int32, device=dev)
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    ncand = torch.empty(n, dtype=torch.int32, device=dev) if with_candidates else None
    seg_ptr = torch.empty(n_seg + 1, dtype=torch.int64, device=dev)
    h.call("sfm_guided_match", code, dp(rows), int(rows.shape[0]), dim, dp(pts), n_seg, hp(q_beg), hp(q_end), hp(t_beg), hp(t_end),
           dp(d_F), C.c_double(float(gate)), C.c_double(float(ratio)), C.c_double(-1.0 if max_distance is None else float(max_distance)),
           1 if cross_check else 0, dp(qi), dp(ti), dp(dist), dp(ncand) if with_candidates else None, dp(seg_ptr), dp(ws), need.value)
    sp = seg_ptr.cpu().numpy()
    m = int(sp[-1])
    res.update(queryIdx=qi[:m].cpu().numpy(), trainIdx=ti[:m].cpu().numpy(), distance=dist[:m].cpu().numpy(), seg_ptr=sp)
    if with_candidates:
        res["n_candidates"] = ncand.cpu().numpy()
    return res
