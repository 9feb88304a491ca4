"""Multi-view feature tracks from pairwise matches, built on the device (`sfm_tracks_build`, sfm_amd/csrc/tracks.hip):
the join between the pair loop (`ImageMatcher.process_pairs`) and the reconstruction.  A node is one keypoint of one
image, a verified match is an edge, a track is a connected component; the result is keyed by keypoint index, in CSR form,
and has one byte pattern whatever the order of the pairs and of the matches (tracks by their smallest node, observations
ascending).  No CPU fallback: without the library or a GPU `build_tracks` raises.
"""
from __future__ import annotations

import ctypes as C
import re

import numpy as np

from . import _lib

POLICIES = {"drop": _lib.TRACKS_DROP, "keep": _lib.TRACKS_KEEP}
UNMATCHED, TOO_SHORT, DROPPED = -1, -2, -3          # node_track codes


class Tracks:
    """Tracks in CSR form; a plain container of host arrays.

    kp_ptr [n_img+1] int64 (node id = kp_ptr[image] + keypoint), track_ptr [n_tracks+1] int64, image / keypoint [n_obs]
    int32 (the observations of track t are track_ptr[t]:track_ptr[t+1], ascending by node id), conflict [n_tracks] uint8,
    node_track [n_nodes] int32 (track id, -1 unmatched, -2 shorter than min_length, -3 dropped for a conflict),
    n_conflicting: conflicting components of at least min_length, whatever the policy; n_bad_edges: edges skipped;
    image_ids: the caller's id of each image position (None: the positions themselves)."""

    def __init__(self, kp_ptr, track_ptr, image, keypoint, conflict=None, node_track=None, n_conflicting=0, n_bad_edges=0,
                 image_ids=None):
        self.kp_ptr = np.asarray(kp_ptr, dtype=np.int64)
        self.track_ptr = np.asarray(track_ptr, dtype=np.int64)
        self.image = np.asarray(image, dtype=np.int32)
        self.keypoint = np.asarray(keypoint, dtype=np.int32)
        n = len(self.track_ptr) - 1
        self.conflict = np.zeros(n, np.uint8) if conflict is None else np.asarray(conflict, dtype=np.uint8)
        self.node_track = None if node_track is None else np.asarray(node_track, dtype=np.int32)
        self.n_conflicting = int(n_conflicting)
        self.n_bad_edges = int(n_bad_edges)
        self.image_ids = None if image_ids is None else [int(i) for i in image_ids]
        if n < 0 or self.track_ptr[0] != 0 or self.track_ptr[-1] != len(self.image) or len(self.image) != len(self.keypoint) \
                or len(self.conflict) != n or (np.diff(self.track_ptr) < 0).any():
            raise ValueError("inconsistent CSR arrays")

    def __len__(self):
        return len(self.track_ptr) - 1

    @property
    def n_obs(self):
        return len(self.image)

    def lengths(self):
        return np.diff(self.track_ptr)

    def _uv(self, keypoints):
        """[n_obs,2] float64 pixel positions of the observations; keypoints: per image an [n,2] array or cv2.KeyPoints."""
        from .twoview import keypoints_xy
        uv = np.empty((self.n_obs, 2), dtype=np.float64)
        for img in np.unique(self.image):
            sel = self.image == img
            uv[sel] = np.asarray(keypoints_xy(keypoints[img]), dtype=np.float64)[self.keypoint[sel]]
        return uv

    def observations(self, keypoints):
        """(cam_idx int32, pt_idx int32, uv float64 [n_obs,2]) in point-major order: what GpuBA / pack_state take, with
        camera = image position and point = track."""
        pt_idx = np.repeat(np.arange(len(self), dtype=np.int32), self.lengths())
        return self.image.copy(), pt_idx, self._uv(keypoints)

    def as_point_tracks(self, keypoints, image_ids=None):
        """The reference's `self.point_tracks`: one {image_id: [x, y]} per track.  image_ids maps positions to ids
        (default: self.image_ids, else the positions).  In a conflicting track kept under "keep" the later keypoint of an
        image wins."""
        uv = self._uv(keypoints)
        if image_ids is None:
            image_ids = self.image_ids if self.image_ids is not None else range(len(self.kp_ptr) - 1)
        ids = [int(i) for i in image_ids]
        return [{ids[self.image[o]]: uv[o].tolist() for o in range(self.track_ptr[t], self.track_ptr[t + 1])}
                for t in range(len(self))]


def _pair_arrays(m):
    """(queryIdx, trainIdx) of one pair: a DMatchList, a (q, t[, distance]) tuple or a [M,2] array."""
    if hasattr(m, "queryIdx") and hasattr(m, "trainIdx"):
        q, t = m.queryIdx, m.trainIdx
    elif isinstance(m, np.ndarray) and m.ndim == 2 and m.shape[1] == 2:
        q, t = m[:, 0], m[:, 1]
    else:
        q, t = m[0], m[1]
    q, t = np.asarray(q).reshape(-1), np.asarray(t).reshape(-1)
    if q.shape != t.shape:
        raise ValueError("queryIdx / trainIdx differ in length")
    if q.size and not (np.issubdtype(q.dtype, np.integer) and np.issubdtype(t.dtype, np.integer)):
        raise ValueError("match indices must be integers")
    return q.astype(np.int64), t.astype(np.int64)


def pack_matches(n_keypoints, pairs, matches, masks=None):
    """Validate on the host and flatten: (kp_ptr, seg_ptr, pair_img [n_seg,2] int32, query int32, train int32, mask uint8 or
    None).  ValueError for a pair outside the image list, a pair of an image with itself, an index outside its image or a
    mask of the wrong length."""
    counts = np.asarray(n_keypoints, dtype=np.int64).reshape(-1)
    if (counts < 0).any():
        raise ValueError("negative keypoint count")
    n_img = len(counts)
    kp_ptr = np.zeros(n_img + 1, dtype=np.int64)
    np.cumsum(counts, out=kp_ptr[1:])
    if kp_ptr[-1] >= 2 ** 31:
        raise ValueError("more than 2^31 - 1 keypoints")
    pairs = [(int(i), int(j)) for i, j in pairs]
    if len(matches) != len(pairs) or (masks is not None and len(masks) != len(pairs)):
        raise ValueError("pairs / matches / masks differ in length")
    qs, ts, ms = [], [], []
    for s, ((i, j), m) in enumerate(zip(pairs, matches)):
        if not (0 <= i < n_img and 0 <= j < n_img) or i == j:
            raise ValueError(f"pairs[{s}] = ({i}, {j}) is not a pair of two of the {n_img} images")
        q, t = _pair_arrays(m)
        if q.size and (q.min() < 0 or q.max() >= counts[i] or t.min() < 0 or t.max() >= counts[j]):
            raise ValueError(f"matches[{s}] holds a keypoint index outside image {i} ({counts[i]}) or {j} ({counts[j]})")
        qs.append(q); ts.append(t)
        if masks is not None:
            mk = np.ones(q.size, np.uint8) if masks[s] is None else (np.asarray(masks[s]).reshape(-1) != 0).astype(np.uint8)
            if mk.size != q.size:
                raise ValueError(f"masks[{s}] has {mk.size} entries for {q.size} matches")
            ms.append(mk)
    seg_ptr = np.zeros(len(pairs) + 1, dtype=np.int64)
    np.cumsum([q.size for q in qs], out=seg_ptr[1:])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return (kp_ptr, seg_ptr, np.asarray(pairs, dtype=np.int32).reshape(-1, 2), cat(qs, np.int32), cat(ts, np.int32),
            cat(ms, np.uint8) if masks is not None else None)


def build_tracks_raw(kp_ptr, seg_ptr, pair_img, query_idx, train_idx, mask=None, min_length=2, conflicts="drop", device=0):
    """sfm_tracks_build on flat host arrays, nothing validated but the options: the output arrays cut to their lengths
    {track_ptr, obs_image, obs_kp, track_conflict, node_track, counts [4]}.  Bad edges are counted and skipped by the device."""
    import torch
    from .driver import _p
    if conflicts not in POLICIES:
        raise ValueError(f"conflicts must be one of {sorted(POLICIES)}")
    if int(min_length) < 2:
        raise ValueError("min_length must be at least 2")
    kp_ptr = np.ascontiguousarray(kp_ptr, dtype=np.int64)
    n_img, n_nodes, n_seg, n_edges = len(kp_ptr) - 1, int(kp_ptr[-1]), len(seg_ptr) - 1, len(query_idx)
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    _dev = lambda a, dtype, dev: torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(dev)    # a copy: inputs may be read-only
    cap_t, cap_o = n_nodes // 2, n_nodes
    d_kp, d_seg = _dev(kp_ptr, np.int64, dev), _dev(seg_ptr, np.int64, dev)
    d_pair = _dev(np.asarray(pair_img).reshape(-1, 2), np.int32, dev)
    d_q, d_t = _dev(query_idx, np.int32, dev), _dev(train_idx, np.int32, dev)
    d_mask = _dev(mask, np.uint8, dev) if mask is not None else None
    need = C.c_int64()
    h.check(h.lib.sfm_tracks_workspace_bytes(n_nodes, n_edges, C.byref(need)), "sfm_tracks_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    track_ptr = torch.empty(cap_t + 1, dtype=torch.int64, device=dev)
    obs = torch.empty((2, max(cap_o, 1)), dtype=torch.int32, device=dev)
    conflict = torch.empty(max(cap_t, 1), dtype=torch.uint8, device=dev)
    node_track = torch.empty(max(n_nodes, 1), dtype=torch.int32, device=dev)
    counts = torch.empty(5, dtype=torch.int64, device=dev)
    h.call("sfm_tracks_build", _p(d_kp), n_img, n_nodes, _p(d_seg), n_seg, _p(d_pair), _p(d_q), _p(d_t), _p(d_mask), n_edges,
           int(min_length), POLICIES[conflicts], _p(track_ptr), _p(obs[0]), _p(obs[1]), _p(conflict), _p(node_track),
           _p(counts), cap_t, cap_o, _p(ws), need.value)
    cnt = counts.cpu().numpy()
    n_tracks, n_obs = int(cnt[0]), int(cnt[1])
    obs_h = obs[:, :n_obs].cpu().numpy()
    return {"track_ptr": track_ptr[:n_tracks + 1].cpu().numpy(), "obs_image": obs_h[0].copy(), "obs_kp": obs_h[1].copy(),
            "track_conflict": conflict[:n_tracks].cpu().numpy(), "node_track": node_track[:n_nodes].cpu().numpy(),
            "counts": cnt[:4].copy()}


def build_tracks(n_keypoints, pairs, matches, masks=None, min_length=2, conflicts="drop", device=0):
    """Tracks of a data set.  n_keypoints: keypoints per image; pairs: (i, j) positions in that list; matches: per pair
    (queryIdx, trainIdx) arrays, a [M,2] array or a DMatchList, queryIdx in image i and trainIdx in image j; masks: per pair
    an array whose zero entries drop their match (None entries allowed).  A track is a connected component of at least
    min_length keypoints; one with two keypoints of an image is dropped (conflicts="drop") or kept and flagged ("keep").
    Everything is validated on the host first (ValueError); the join itself runs on the device."""
    if conflicts not in POLICIES:
        raise ValueError(f"conflicts must be one of {sorted(POLICIES)}")
    if int(min_length) < 2:
        raise ValueError("min_length must be at least 2")
    kp_ptr, seg_ptr, pair_img, q, t, mask = pack_matches(n_keypoints, pairs, matches, masks)
    r = build_tracks_raw(kp_ptr, seg_ptr, pair_img, q, t, mask, min_length, conflicts, device)
    return Tracks(kp_ptr, r["track_ptr"], r["obs_image"], r["obs_kp"], r["track_conflict"], r["node_track"],
                  n_conflicting=r["counts"][2], n_bad_edges=r["counts"][3])


def tracks_from_pair_files(data_dir, pair_names, n_keypoints=None, min_length=2, conflicts="drop", device=0):
    """Tracks from what save_pair_data wrote (interchange.load_pair_data: queryIdx, trainIdx, inlier_mask), verified
    matches only.  Image ids come from the pair names ("pair_12_35"): positions are the ids in ascending order, kept in
    `Tracks.image_ids`.  n_keypoints: {image_id: count} or one count for all; default: the largest index seen + 1."""
    from .interchange import load_pair_data
    ids, loaded = set(), []
    for name in pair_names:
        m = re.fullmatch(r"pair_(\d+)_(\d+)", str(name))
        if not m:
            raise ValueError(f"not a pair name: {name!r}")
        a, b = int(m.group(1)), int(m.group(2))
        d = load_pair_data(data_dir, name)
        ids.update((a, b))
        loaded.append((a, b, np.asarray(d["queryIdx"]), np.asarray(d["trainIdx"]), np.asarray(d["inlier_mask"])))
    image_ids = sorted(ids)
    pos = {v: k for k, v in enumerate(image_ids)}
    if n_keypoints is None:
        seen = {v: 0 for v in image_ids}
        for a, b, q, t, _ in loaded:
            if q.size:
                seen[a] = max(seen[a], int(q.max()) + 1)
                seen[b] = max(seen[b], int(t.max()) + 1)
        counts = [seen[v] for v in image_ids]
    elif isinstance(n_keypoints, dict):
        counts = [int(n_keypoints[v]) for v in image_ids]
    else:
        counts = [int(n_keypoints)] * len(image_ids)
    tr = build_tracks(counts, [(pos[a], pos[b]) for a, b, *_ in loaded], [(q, t) for _, _, q, t, _ in loaded],
                      masks=[m for *_, m in loaded], min_length=min_length, conflicts=conflicts, device=device)
    tr.image_ids = image_ids
    return tr
