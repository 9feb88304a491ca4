"""Drop-in for the reference's `ImageMatcher.match_features`
(/root/reference/utils/find_matches.py:141-155): brute-force kNN (k=2) + Lowe ratio test on
the GPU through libsfm_amd.so; `geometric_verification` (:157-214) comes from sfm_amd.driver,
`find_fundamental_mat` (the cv2.findFundamentalMat call at :282) from sfm_amd.twoview.
No CPU fallback."""
from __future__ import annotations

import ctypes as C
from collections.abc import Sequence

import numpy as np

from . import _lib
from .driver import VerificationMixin, verify_pairs
from .twoview import FundamentalMixin, estimate_fundamental_batched, keypoints_xy


class DMatch:
    """The attributes of cv2.DMatch the reference reads (find_matches.py:230-232,278-279,323-327)."""
    __slots__ = ("queryIdx", "trainIdx", "distance", "imgIdx")

    def __init__(self, queryIdx, trainIdx, distance, imgIdx=0):
        self.queryIdx = int(queryIdx)
        self.trainIdx = int(trainIdx)
        self.distance = float(distance)
        self.imgIdx = int(imgIdx)

    def __repr__(self):
        return f"DMatch(queryIdx={self.queryIdx}, trainIdx={self.trainIdx}, distance={self.distance})"

    def __eq__(self, other):
        return (isinstance(other, DMatch) and (self.queryIdx, self.trainIdx, self.distance, self.imgIdx) ==
                (other.queryIdx, other.trainIdx, other.distance, other.imgIdx))

    __hash__ = None


def _dmatch(q, t, d):
    """A DMatch from values that already are Python int / float (ndarray.tolist()): no conversions, no __init__ call."""
    m = DMatch.__new__(DMatch)
    m.queryIdx, m.trainIdx, m.distance, m.imgIdx = q, t, d, 0
    return m


class DMatchList(Sequence):
    """What `match_features` returns: the matches of one image pair as a read-only sequence over the three result arrays.

    Everything the reference does with the list works - `len(matches)` (find_matches.py:274,305), iteration in query order with
    `.queryIdx / .trainIdx / .distance` on every element (:230-232, 278-279, 323-327), indexing, slicing, truthiness,
    `list(matches)` - but no object exists until one is asked for: building 30,000 DMatch objects up front cost two orders of
    magnitude more than the kernels that found the matches (50k x 50k: 0.4 ms on the GPU).  Array consumers read
    `.queryIdx`, `.trainIdx`, `.distance` (int32 / int32 / float32 NumPy arrays, query order) and skip the objects altogether:
    `pts1 = kp_xy[matches.queryIdx]` is the vector form of find_matches.py:278."""

    __slots__ = ("queryIdx", "trainIdx", "distance")

    def __init__(self, queryIdx, trainIdx, distance):
        self.queryIdx = np.asarray(queryIdx, dtype=np.int32)
        self.trainIdx = np.asarray(trainIdx, dtype=np.int32)
        self.distance = np.asarray(distance, dtype=np.float32)
        if not (self.queryIdx.ndim == 1 and self.queryIdx.shape == self.trainIdx.shape == self.distance.shape):
            raise ValueError("queryIdx, trainIdx and distance must be 1-D arrays of one length")

    def __len__(self):
        return int(self.queryIdx.shape[0])

    def __getitem__(self, i):
        if isinstance(i, slice):
            return DMatchList(self.queryIdx[i], self.trainIdx[i], self.distance[i])
        i = int(i)
        n = len(self)
        if i < -n or i >= n:
            raise IndexError("DMatchList index out of range")
        return _dmatch(int(self.queryIdx[i]), int(self.trainIdx[i]), float(self.distance[i]))

    def __iter__(self):
        # one tolist() per array, then objects one at a time: nothing of the pair is held beyond the element in hand
        return map(_dmatch, self.queryIdx.tolist(), self.trainIdx.tolist(), self.distance.tolist())

    def __eq__(self, other):
        if isinstance(other, DMatchList):
            return (np.array_equal(self.queryIdx, other.queryIdx) and np.array_equal(self.trainIdx, other.trainIdx) and
                    np.array_equal(self.distance, other.distance))
        if isinstance(other, (list, tuple)):
            return len(other) == len(self) and all(a == b for a, b in zip(self, other))
        return NotImplemented

    __hash__ = None

    def __repr__(self):
        return f"DMatchList({len(self)} matches)"


def _to_device(a, device):
    import torch
    if isinstance(a, torch.Tensor):
        return a.to(device).contiguous()
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a).to(device)


def _resolve_metric(q, t, metric):
    import torch
    if metric == "auto":
        if q.dtype == torch.uint8:
            metric = "hamming" if q.shape[1] <= 64 and q.shape[1] != 128 else "l2"
        else:
            metric = "l2"
    if metric not in ("l2", "hamming"):
        raise ValueError(f"unknown metric {metric!r}")
    return metric


def _metric_code(is_u8, dim, metric):
    """The metric code of a resolved metric ("l2" / "hamming") over uint8 (is_u8) or other rows of `dim` columns - or None:
    float rows at dims 32 / 64 / 128 take the exact uint8 path if their values are integers in [0, 255], which the caller
    finds out its own way (knn2 over the two sets, match_pairs per image)."""
    if metric == "hamming":
        if not is_u8:
            raise ValueError("hamming needs uint8 descriptors")
        return _lib.METRIC_HAMMING
    if dim not in (32, 64, 128):
        return _lib.METRIC_L2_F32
    return _lib.METRIC_L2_U8 if is_u8 else None


def _knn_outputs(n, dev):
    """idx1, idx2, d1, d2 of n output rows"""
    import torch
    return (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
            torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev))


def _ratio_outputs(n, dev):
    """query index, train index, distance of at most n matches"""
    import torch
    return (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
            torch.empty(n, dtype=torch.float32, device=dev))


def _ratio_ws_bytes(n):
    """Scratch of sfm_match_ratio_batched over n rows (include/sfm_amd.h); sfm_match_ratio needs 64 bytes less."""
    return ((n + 255) // 256) * 8 + 64


def knn2(desc1, desc2, metric="auto", device=0):
    """cv2.BFMatcher(norm).knnMatch(desc1, desc2, k=2) -> (idx1, idx2, d1, d2) CUDA tensors.

    metric: "l2" (float32 or uint8 descriptors, SIFT), "hamming" (uint8 bit strings, ORB),
    "auto" = hamming for uint8 of <= 64 bytes, l2 otherwise.  float32 descriptors whose values
    are all integers in [0,255] (what SIFT emits) take the exact integer path on the matrix cores.
    """
    import torch
    dp = _lib.dp
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    q, t = _to_device(desc1, dev), _to_device(desc2, dev)
    if q.dim() != 2 or t.dim() != 2 or q.shape[1] != t.shape[1]:
        raise ValueError("descriptors must be [n, dim] with equal dim")
    if q.dtype != t.dtype:
        raise ValueError("descriptor dtypes differ")
    nq, dim = q.shape
    nt = t.shape[0]
    if nt < 2 or nq < 1:
        raise ValueError("knn2 needs at least 1 query and 2 train descriptors")
    code = _metric_code(q.dtype == torch.uint8, dim, _resolve_metric(q, t, metric))
    if code is None or code == _lib.METRIC_L2_F32:
        q, t = q.float(), t.float()
    if code is None:
        code = _lib.METRIC_L2_F32
        flag = torch.ones(2, dtype=torch.int32, device=dev)
        q8 = torch.empty(q.shape, dtype=torch.uint8, device=dev)
        t8 = torch.empty(t.shape, dtype=torch.uint8, device=dev)
        h.call("sfm_match_f32_to_u8", dp(q), q.numel(), dp(q8), dp(flag[0:1]))
        h.call("sfm_match_f32_to_u8", dp(t), t.numel(), dp(t8), dp(flag[1:2]))
        if bool((flag == 1).all().item()):
            q, t, code = q8, t8, _lib.METRIC_L2_U8
    need = C.c_int64()
    h.check(h.lib.sfm_match_workspace_bytes(code, nq, nt, dim, C.byref(need)), "sfm_match_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    idx1, idx2, d1, d2 = _knn_outputs(nq, dev)
    h.call("sfm_match_knn2", code, dp(q), nq, dp(t), nt, dim, dp(idx1), dp(idx2), dp(d1), dp(d2), dp(ws), need.value)
    return idx1, idx2, d1, d2


def ratio_filter(idx1, d1, d2, ratio=0.75, device=0):
    """`m.distance < ratio * n.distance` (find_matches.py:152) + compaction in query order."""
    import torch
    dp = _lib.dp
    h = _lib.get_handle(device)
    dev = idx1.device
    nq = idx1.shape[0]
    qi, ti, dd = _ratio_outputs(nq, dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws_bytes = _ratio_ws_bytes(nq)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    h.call("sfm_match_ratio", nq, dp(idx1), dp(d1), dp(d2), C.c_double(ratio), dp(qi), dp(ti), dp(dd), dp(cnt), dp(ws), ws_bytes)
    m = int(cnt.item())
    return qi[:m], ti[:m], dd[:m]


def match_arrays(desc1, desc2, ratio=0.75, metric="auto", device=0):
    """(queryIdx, trainIdx, distance) NumPy arrays in query order.

    Degenerate inputs follow the reference: with no query or no train descriptors knnMatch hands back
    an empty list and the ratio loop yields [] (find_matches.py:147-155); with exactly ONE train
    descriptor every knn row holds a single DMatch and `for m, n in matches` (find_matches.py:151)
    raises ValueError, which the per-pair try/except at :344-350 turns into a skipped pair.
    Non-finite float32 distances follow the rule of include/sfm_amd.h: a query none of whose distances can be ranked
    (all NaN) yields no match, one with a single rankable train row keeps it (d1 < ratio * inf)."""
    n1 = int(desc1.shape[0]) if desc1 is not None else 0
    n2 = int(desc2.shape[0]) if desc2 is not None else 0
    if n1 == 0 or n2 == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32)
    if n2 == 1:
        raise ValueError("not enough values to unpack (expected 2, got 1)")
    idx1, _, d1, d2 = knn2(desc1, desc2, metric, device)
    q, t, d = ratio_filter(idx1, d1, d2, ratio, device)
    return q.cpu().numpy(), _ranked(t.cpu().numpy()), d.cpu().numpy()


def _ranked(train_idx):
    """The train indices of a match list, checked: a slot no row could be ranked into (index -1: every distance NaN)
    carries distance +inf, and `d1 < ratio * d2` is false for d1 = +inf, so no match may hold it (include/sfm_amd.h)."""
    if train_idx.size and int(train_idx.min()) < 0:
        raise AssertionError("a match without a train row passed the ratio test")
    return train_idx


_STAGE = {}


def _pinned_stage(n_bytes):
    """A page-locked uint8 buffer of at least n_bytes, kept across calls (grow-only, doubled on growth)."""
    import torch
    buf = _STAGE.get("buf")
    if buf is None or buf.numel() < n_bytes:
        size = max(n_bytes, 2 * (buf.numel() if buf is not None else 0), 1 << 20)
        buf = torch.empty(size, dtype=torch.uint8, pin_memory=True)
        _STAGE["buf"] = buf
    return buf


def _upload_sets(arrs, dev):
    """Descriptor sets of several images -> one device array (rows back to back) and its row offsets."""
    import torch
    dim = arrs[0].shape[1]
    if any(a.ndim != 2 or a.shape[1] != dim or a.dtype != arrs[0].dtype for a in arrs):
        raise ValueError("descriptor sets must be [n, dim] arrays of one dtype and dim")
    ptr = np.zeros(len(arrs) + 1, dtype=np.int64)
    np.cumsum([a.shape[0] for a in arrs], out=ptr[1:])
    # rows back to back straight into a page-locked staging buffer (kept and grown across calls), one asynchronous copy from
    # there: the concatenation into pageable memory plus its staged upload were 0.3 ms of a 0.8 ms call at 18 x 2,000 x 128
    n_bytes = int(ptr[-1]) * dim * arrs[0].dtype.itemsize
    stage = _pinned_stage(max(n_bytes, 1))
    host = stage[:n_bytes].numpy().view(arrs[0].dtype).reshape(int(ptr[-1]), dim)
    if int(ptr[-1]) > 0:
        np.concatenate(arrs, axis=0, out=host)
    allrows = torch.from_numpy(host).to(dev, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()          # the staging buffer is reused by the next call
    return allrows, ptr, dim


def _run_batch(h, dev, rows, ptr, code, dim, seg_pairs, ratio):
    """One sfm_match_knn2_batched + sfm_match_ratio_batched over the image pairs `seg_pairs` (indices into ptr)."""
    import torch
    n_seg = len(seg_pairs)
    q_beg = np.array([ptr[i] for i, _ in seg_pairs], dtype=np.int64)
    q_end = np.array([ptr[i + 1] for i, _ in seg_pairs], dtype=np.int64)
    t_beg = np.array([ptr[j] for _, j in seg_pairs], dtype=np.int64)
    t_end = np.array([ptr[j + 1] for _, j in seg_pairs], dtype=np.int64)
    dp, hp = _lib.dp, _lib.hp
    n_out, need = C.c_int64(), C.c_int64()
    n_rows = int(rows.shape[0])
    h.check(h.lib.sfm_match_batched_workspace_bytes(code, n_seg, hp(q_beg), hp(q_end), hp(t_beg), hp(t_end), n_rows, n_rows,
                                                    C.byref(n_out), C.byref(need)), "sfm_match_batched_workspace_bytes")
    n = n_out.value
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    idx1, idx2, d1, d2 = _knn_outputs(n, dev)
    out_ptr = torch.empty(n_seg + 1, dtype=torch.int64, device=dev)
    h.call("sfm_match_knn2_batched", code, dp(rows), n_rows, dp(rows), n_rows, dim, n_seg, hp(q_beg), hp(q_end), hp(t_beg),
           hp(t_end), dp(idx1), dp(idx2), dp(d1), dp(d2), dp(out_ptr), dp(ws), need.value)
    qi, ti, dd = _ratio_outputs(n, dev)
    seg_ptr = torch.empty(n_seg + 1, dtype=torch.int64, device=dev)
    h.call("sfm_match_ratio_batched", n, n_seg, dp(out_ptr), dp(idx1), dp(d1), dp(d2), C.c_double(ratio), dp(qi), dp(ti),
           dp(dd), dp(seg_ptr), dp(ws), need.value)
    sp = seg_ptr.cpu().numpy()
    m = int(sp[-1])
    qh, th, dh = qi[:m].cpu().numpy(), _ranked(ti[:m].cpu().numpy()), dd[:m].cpu().numpy()
    # disjoint views of the three result arrays (444 copies were 0.25 ms of a 1.2 ms call)
    return [(qh[int(sp[k]):int(sp[k + 1])], th[int(sp[k]):int(sp[k + 1])], dh[int(sp[k]):int(sp[k + 1])]) for k in range(n_seg)]


def match_pairs(descs, pairs, ratio=0.75, metric="auto", device=0):
    """match_features for MANY image pairs in one launch (sfm_match_knn2_batched + sfm_match_ratio_batched).

    descs: list of per-image descriptor arrays (None = an image without keypoints, as cv2 returns it); pairs: list of
    (i, j) = match image i's descriptors (queries) against image j's (train), exactly what the reference does once per
    pair in its serial loop (find_matches.py:329-350, call at :272).  Returns one entry per pair, each what
    match_arrays(descs[i], descs[j]) gives for THAT pair: a (queryIdx, trainIdx, distance) triple of NumPy arrays, bit
    for bit - empty arrays for a pair with an empty side, and the ValueError of the reference's unpacking (:151) AS THE
    ENTRY (not raised) for a pair whose train image has exactly one descriptor: the reference's per-pair try / except
    (:344-350) skips that pair only.  Only images some live pair refers to are uploaded.  The exact uint8 path is decided
    per image: float32 sets whose values are all integers in [0, 255] pair up on the matrix cores, pairs touching any
    other float set run the float32 kernel (one launch per group; on integer-valued rows both kernels give the same bits:
    sums below 2^24 are exact in float32)."""
    import torch
    empty = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    pairs = [(int(i), int(j)) for i, j in pairs]
    sizes = [0 if d is None else int(np.asarray(d).shape[0]) for d in descs]
    out = [empty] * len(pairs)
    live = []
    for s, (i, j) in enumerate(pairs):
        if sizes[i] > 0 and sizes[j] == 1:
            out[s] = ValueError("not enough values to unpack (expected 2, got 1)")
        elif sizes[i] > 0 and sizes[j] >= 2:
            live.append(s)
    if not live:
        return out
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    used = sorted({i for s in live for i in pairs[s]})
    slot = {img: k for k, img in enumerate(used)}
    rows, ptr, dim = _upload_sets([np.ascontiguousarray(descs[i]) for i in used], dev)
    metric = _resolve_metric(rows, rows, metric)
    seg = [(slot[pairs[s][0]], slot[pairs[s][1]]) for s in live]
    everything = list(range(len(live)))
    code = _metric_code(rows.dtype == torch.uint8, dim, metric)
    groups = []                                            # (rows, metric code, positions in `live`)
    if code is None:
        rows = rows.float()
        # per image: every value an integer in [0, 255]?  (what SIFT emits)
        row_ok = ((rows == rows.round()) & (rows >= 0) & (rows <= 255)).all(dim=1)
        csum = torch.zeros(rows.shape[0] + 1, dtype=torch.int64, device=dev)
        torch.cumsum(row_ok.to(torch.int64), 0, out=csum[1:])
        tp = torch.from_numpy(ptr).to(dev)
        img_ok = ((csum[tp[1:]] - csum[tp[:-1]]) == (tp[1:] - tp[:-1])).cpu().numpy()
        exact = [k for k, (a, b) in enumerate(seg) if img_ok[a] and img_ok[b]]
        other = [k for k, (a, b) in enumerate(seg) if not (img_ok[a] and img_ok[b])]
        if exact:
            groups.append((rows.to(torch.uint8), _lib.METRIC_L2_U8, exact))     # rows of other images are never read by this group
        if other:
            groups.append((rows, _lib.METRIC_L2_F32, other))
    elif code == _lib.METRIC_L2_F32:
        groups.append((rows.float(), code, everything))
    else:
        groups.append((rows, code, everything))
    for grows, code, pos in groups:
        for k, res in zip(pos, _run_batch(h, dev, grows, ptr, code, dim, [seg[k] for k in pos], ratio)):
            out[live[k]] = res
    return out


class ImageMatcher(VerificationMixin, FundamentalMixin):
    """`match_features` with the reference's call shape (find_matches.py:141).  The in-tree
    reference matches ORB bit strings with NORM_HAMMING and ratio 0.75; its shipped results come
    from SIFT / L2.  metric="auto" follows the descriptor type."""

    def __init__(self, data_dir=None, ratio=0.75, metric="auto", device=0):
        self.data_dir = data_dir
        self.ratio = float(ratio)
        self.metric = metric
        self.device = device

    def match_features(self, desc1, desc2):
        """Returns a DMatchList: the reference's list of cv2.DMatch as a lazy sequence (see DMatchList)."""
        q, t, d = match_arrays(desc1, desc2, self.ratio, self.metric, self.device)
        return DMatchList(q, t, d)

    def match_features_batched(self, descs, pairs):
        """match_features(descs[i], descs[j]) for every (i, j) of `pairs` in one launch: the list the reference's
        pair loop (find_matches.py:329-350) would have collected call by call.  A pair the reference's per-pair
        try / except (:344-350) would have logged and skipped (one train descriptor) is logged and yields None."""
        import logging
        out = []
        for (i, j), res in zip(pairs, match_pairs(descs, pairs, self.ratio, self.metric, self.device)):
            if isinstance(res, Exception):
                logging.error(f"Error processing pair ({i}, {j}): {res}")
                out.append(None)
                continue
            out.append(DMatchList(*res))
        return out

    def process_pairs(self, keypoints, descs, pairs, min_matches=5, guided=False, homography=False, **guided_options):
        """process_image_pair (find_matches.py:246-310) for every (i, j) of `pairs`, minus the image I/O and the visualisation,
        in three batched device steps: match_pairs (:272) -> the float32 pts1 / pts2 gathers (:278-279), pairs under
        `min_matches` dropped (:274) -> estimate_fundamental_batched (:282) -> verify_pairs (:288).

        keypoints: per image an [n,2] array of pixel coordinates or a list of objects with `.pt` (cv2.KeyPoint).  Returns one
        entry per pair: None where the reference returns None (too few matches, a pair its try / except skips, no model), else
        {'matches': DMatchList, 'pts1', 'pts2' [M,2] float32, 'F' [3,3], 'inlier_mask' [M] bool, 'symmetric_errors',
        'metrics': the dictionary of geometric_verification, 'quality_ok': verify_match_quality of it}.
        guided=True passes the result through `guided_pairs` (with `guided_options`): every pair with a model is matched again
        under its F.
        homography=True runs one more batched call, `estimate_homography_batched` with the threshold, hypothesis count and
        seed of the F stage, over the pairs that have a result: each of those entries gains 'H' ([3,3] with x2 ~ H x1, or
        None) and 'n_homography', the inlier count of H over the entry's matches - set against the inliers of F it tells a
        planar or rotation-only pair from a general one."""
        import logging
        pairs = [(int(i), int(j)) for i, j in pairs]
        if homography:
            return self._with_homographies(self.process_pairs(keypoints, descs, pairs, min_matches, guided=guided, **guided_options))
        if guided:
            return self.guided_pairs(keypoints, descs, pairs, self.process_pairs(keypoints, descs, pairs, min_matches), **guided_options)
        if guided_options:
            raise TypeError(f"options {sorted(guided_options)} need guided=True")
        xy = {}
        out = [None] * len(pairs)
        live, p1, p2, ml = [], [], [], []
        for s, ((i, j), res) in enumerate(zip(pairs, match_pairs(descs, pairs, self.ratio, self.metric, self.device))):
            if isinstance(res, Exception):
                logging.error(f"Error processing pair ({i}, {j}): {res}")
                continue
            q, t, d = res
            if len(q) < min_matches:
                continue
            for img in (i, j):
                if img not in xy:
                    xy[img] = keypoints_xy(keypoints[img])
            live.append(s); ml.append(DMatchList(q, t, d))
            p1.append(xy[i][q]); p2.append(xy[j][t])
        if not live:
            return out
        models = estimate_fundamental_batched(p1, p2, self.fund_threshold, n_hypotheses=self.fund_hypotheses,
                                              seed=self.fund_seed, device=self.device)
        ok = [k for k, (F, _) in enumerate(models) if F is not None]
        if not ok:
            return out
        verified = verify_pairs([(p1[k], p2[k], models[k][0]) for k in ok], 3.0, self.device)
        for k, v in zip(ok, verified):
            out[live[k]] = {"matches": ml[k], "pts1": p1[k], "pts2": p2[k], "F": models[k][0],
                            "inlier_mask": v["inlier_mask"], "symmetric_errors": v["symmetric_errors"],
                            "metrics": v["metrics"], "quality_ok": self.verify_match_quality(v)}
        return out

    def _with_homographies(self, results):
        """`results` of process_pairs with 'H' and 'n_homography' added to every entry that is not None: one batched call."""
        from .homography import estimate_homography_batched
        live = [s for s, r in enumerate(results) if r is not None]
        if live:
            hom = estimate_homography_batched([results[s]["pts1"] for s in live], [results[s]["pts2"] for s in live],
                                              self.fund_threshold, n_hypotheses=self.fund_hypotheses, seed=self.fund_seed,
                                              device=self.device)
            for s, (H, mask) in zip(live, hom):
                results[s]["H"] = H
                results[s]["n_homography"] = 0 if mask is None else int(np.count_nonzero(mask))
        return results

    def guided_pairs(self, keypoints, descs, pairs, results, gate=3.0, ratio=None, max_distance=None, cross_check=False):
        """Guided matching on top of what `process_pairs(keypoints, descs, pairs)` returned: every pair with a result is matched
        again under that result's F (sfm_amd.guided.guided_match_pairs: candidates within `gate` pixels of the epipolar lines,
        ratio test among them; `ratio` defaults to the matcher's).  Returns a list of the same shape in which every non-None
        entry has 'matches' (DMatchList), 'pts1', 'pts2' replaced by the guided set, 'F' unchanged, 'inlier_mask' /
        'symmetric_errors' / 'metrics' / 'quality_ok' recomputed by verify_pairs, and 'n_unguided' = the number of matches the
        entry came with.  An entry whose guided set is empty becomes None.  `build_tracks` consumes the list as it is."""
        from .guided import guided_match_pairs
        pairs = [(int(i), int(j)) for i, j in pairs]
        if len(results) != len(pairs):
            raise ValueError("pairs / results differ in length")
        out = [None] * len(pairs)
        live = [s for s, r in enumerate(results) if r is not None]
        if not live:
            return out
        got = guided_match_pairs(keypoints, descs, [pairs[s] for s in live], [results[s]["F"] for s in live], gate=gate,
                                 ratio=self.ratio if ratio is None else ratio, max_distance=max_distance, cross_check=cross_check,
                                 metric=self.metric, device=self.device)
        xy = {}
        for s in live:
            for img in pairs[s]:
                if img not in xy:
                    xy[img] = keypoints_xy(keypoints[img])
        keep = [(s, g) for s, g in zip(live, got) if len(g[0]) > 0]
        if not keep:
            return out
        p1 = [xy[pairs[s][0]][g[0]] for s, g in keep]
        p2 = [xy[pairs[s][1]][g[1]] for s, g in keep]
        verified = verify_pairs([(a, b, results[s]["F"]) for a, b, (s, _) in zip(p1, p2, keep)], 3.0, self.device)
        for (s, g), a, b, v in zip(keep, p1, p2, verified):
            out[s] = {"matches": DMatchList(*g), "pts1": a, "pts2": b, "F": results[s]["F"],
                      "inlier_mask": v["inlier_mask"], "symmetric_errors": v["symmetric_errors"],
                      "metrics": v["metrics"], "quality_ok": self.verify_match_quality(v),
                      "n_unguided": len(results[s]["matches"])}
        return out

    def detect_features(self, image, mask=None, n_levels=1, scale=(6, 5)):
        """detect_features of the reference (find_matches.py:74-139) for one image on the device: (keypoints [n,2] float32,
        descriptors uint8 [n,32] or None); see sfm_amd.features for the detector, the descriptor and what differs from ORB.
        n_levels > 1: over a pyramid of that many levels at scale = (num, den), keypoints in pixels of the image."""
        from .features import detect_features
        return detect_features(image, mask, device=self.device, n_levels=n_levels, scale=scale)

    def process_images(self, images, pairs, masks=None, min_matches=5, guided=False, homography=False, n_levels=1,
                       scale=(6, 5), **guided_options):
        """From pixel arrays to verified pairs: detect_and_describe_batched over all images, then process_pairs with the
        Hamming metric.  Returns (features, results): one sfm_amd.features.Features per image (PyramidFeatures with
        n_levels > 1: the multi-scale stage, which keeps images matching across a change of distance) and what
        process_pairs([f.xy ...], [f.descriptors ...], pairs) gives; `self.build_tracks([f.xy for f in features], pairs,
        results)` joins them into Tracks.  guided / guided_options / homography: as in process_pairs."""
        from .features import detect_and_describe_batched
        feats = detect_and_describe_batched(images, masks, device=self.device, n_levels=n_levels, scale=scale)
        metric, self.metric = self.metric, "hamming"
        try:
            results = self.process_pairs([f.xy for f in feats], [f.descriptors for f in feats], pairs, min_matches, guided=guided,
                                         homography=homography, **guided_options)
        finally:
            self.metric = metric
        return feats, results

    def build_tracks(self, keypoints, pairs, results, min_length=2, conflicts="drop", verified_only=True):
        """Multi-view tracks (sfm_amd.tracks.Tracks) from what `process_pairs(keypoints, descs, pairs)` returned: the verified
        matches of every pair with a result joined on the device (sfm_tracks_build); pairs whose result is None are skipped.
        verified_only=False joins all matches of those pairs instead of the inliers of the epipolar check."""
        from .tracks import build_tracks
        pairs = [(int(i), int(j)) for i, j in pairs]
        if len(results) != len(pairs):
            raise ValueError("pairs / results differ in length")
        live = [s for s, r in enumerate(results) if r is not None]
        sizes = [0 if k is None else len(keypoints_xy(k)) for k in keypoints]
        return build_tracks(sizes, [pairs[s] for s in live], [results[s]["matches"] for s in live],
                            masks=[results[s]["inlier_mask"] for s in live] if verified_only else None,
                            min_length=min_length, conflicts=conflicts, device=self.device)
