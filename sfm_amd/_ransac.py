"""What the batched RANSAC wrappers share (twoview.py, pnp.py; `check_K` also serves pose.py): the argument checks and
the one run on the device - upload, `sfm_<stage>_draw_samples` unless the caller brings samples,
`sfm_<stage>_ransac`, one download.  A stage is the prefix of its three library calls (`fund`, `pnp`), its sample
size and the width of its model in doubles; results and debug dictionaries are built by the wrappers."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .driver import _dev, _p, _ptr_array

STATUS_OK, STATUS_TOO_FEW, STATUS_NO_MODEL = 0, 1, 2


def check_options(n_hypotheses, threshold, seed):
    """`(n_hyp, threshold, seed)` as int, float, int, or ValueError."""
    n_hyp = int(n_hypotheses)
    if n_hyp < 1:
        raise ValueError("n_hypotheses must be at least 1")
    threshold = float(threshold)
    if not (threshold >= 0.0 and np.isfinite(threshold)):
        raise ValueError("threshold must be finite and not negative")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must fit an unsigned 64-bit integer")
    return n_hyp, threshold, seed


def check_samples(samples, lengths, n_hyp, size, min_points):
    """Caller-supplied samples -> [n_seg, n_hyp, size] int32; range and distinctness checked for the segments that will
    run (those with at least min_points points)."""
    if len(samples) != len(lengths):
        raise ValueError(f"samples: one [n_hypotheses, {size}] array per segment")
    out = np.full((len(lengths), n_hyp, size), -1, dtype=np.int32)
    for s, (a, m) in enumerate(zip(samples, lengths)):
        if m < min_points:
            continue
        a = np.asarray(a)
        if a.shape != (n_hyp, size) or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"samples[{s}] must be an integer array of shape ({n_hyp}, {size}), got {a.dtype} {a.shape}")
        if a.min() < 0 or a.max() >= m:
            raise ValueError(f"samples[{s}] holds an index outside [0, {m})")
        srt = np.sort(a, axis=1)
        if (srt[:, 1:] == srt[:, :-1]).any():
            raise ValueError(f"samples[{s}] repeats an index within a sample")
        out[s] = a
    return out


def check_K(K, n_seg):
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


def single(batched, args, kw):
    """The single-segment form of a batched call: its one result; with return_debug=True `(result, debug)`."""
    if kw.get("samples") is not None:
        kw["samples"] = [kw["samples"]]
    out = batched(*args, **kw)
    if kw.get("return_debug"):
        return out[0][0], out[1][0]
    return out[0]


def run(stage, size, width, lengths, points, per_segment, n_hyp, threshold, seed, refine, smp_h, device, debug):
    """One call of sfm_<stage>_ransac over all segments.  points: lists of one array per segment, per_segment: arrays of
    n_seg rows, in the order the entry point takes them before and after `n`; each goes up with its own dtype.  smp_h: checked
    samples, or None to draw them on the device.  Returns `(ptr, model [n_seg, width], mask [n], meta [3, n_seg] =
    n_inliers / status / refined, samples, hyp_count)`, the last two None unless debug."""
    n_seg, n = len(lengths), int(sum(lengths))
    if n == 0:                                     # nothing to upload, no handle opened: every segment is a short one
        meta = np.zeros((3, n_seg), np.int32)
        meta[1] = STATUS_TOO_FEW
        return (np.zeros(n_seg + 1, np.int64), np.zeros((n_seg, width)), np.zeros(0, np.uint8), meta,
                np.full((n_seg, n_hyp, size), -1, np.int32), np.zeros((n_seg, n_hyp), np.int32))
    import torch
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    ptr_h, ptr = _ptr_array(lengths, dev)
    d_pts = [_dev(np.concatenate(a), a[0].dtype, dev) for a in points]
    d_seg = [_dev(a, a.dtype, dev) for a in per_segment]
    if smp_h is None:
        d_smp = torch.empty((n_seg, n_hyp, size), dtype=torch.int32, device=dev)
        h.call(f"sfm_{stage}_draw_samples", _p(ptr), n_seg, n_hyp, C.c_uint64(seed), _p(d_smp))
    else:
        d_smp = _dev(smp_h, np.int32, dev)
    need = C.c_int64()
    name = f"sfm_{stage}_workspace_bytes"
    h.check(getattr(h.lib, name)(n, n_seg, n_hyp, C.byref(need)), name)
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    model = torch.empty((n_seg, width), dtype=torch.float64, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    # n_inliers, status, refined in one block: one download for the three
    meta = torch.empty((3, n_seg), dtype=torch.int32, device=dev)
    hyp_count = torch.empty((n_seg, n_hyp), dtype=torch.int32, device=dev) if debug else None
    h.call(f"sfm_{stage}_ransac", _p(ptr), n_seg, *map(_p, d_pts), n, *map(_p, d_seg), _p(d_smp), n_hyp,
           C.c_double(threshold), 1 if refine else 0, _p(model), _p(mask), _p(meta[0]), _p(meta[1]), _p(hyp_count),
           _p(meta[2]), _p(ws), need.value)
    out = ptr_h, model.cpu().numpy(), mask.cpu().numpy(), meta.cpu().numpy()
    if not debug:
        return out + (None, None)
    return out + (d_smp.cpu().numpy() if smp_h is None else smp_h, hyp_count.cpu().numpy())
