"""Feature detection and description on the device (`sfm_features_detect` / `sfm_features_describe`,
sfm_amd/csrc/features.hip): the `detect_features` step of the reference (find_matches.py:74-139 - FAST with threshold 20,
ORB descriptors, the silhouette-mask filter), batched over the images of a data set.  FAST-9/16 is implemented to its
published definition; the descriptor is this library's own steered binary descriptor (include/sfm_amd.h states it
completely) in cv2.ORB's 32-byte layout, because OpenCV and its learned sampling table are not part of this project.
No CPU fallback: without the library or a GPU the calls raise.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib

Features = namedtuple("Features", "xy response angle descriptors")
Features.__doc__ = """xy float32 [n,2] pixels (x, y), response float32 [n] (the FAST score), angle float32 [n] degrees (a
multiple of 12), descriptors uint8 [n,32] - None when n = 0, as cv2 returns it and match_pairs expects it."""


def bgr_to_gray(image):
    """[h,w,3] uint8 in cv2.imread's channel order -> [h,w] uint8 by OpenCV's 8-bit rule
    (R*4899 + G*9617 + B*1868 + 8192) >> 14."""
    a = np.asarray(image)
    b, g, r = (a[..., c].astype(np.int32) for c in range(3))
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def _gray(image):
    a = np.asarray(image)
    if a.dtype != np.uint8:
        raise ValueError("images must be uint8")
    if a.ndim == 3 and a.shape[2] == 3:
        return bgr_to_gray(a)
    if a.ndim != 2:
        raise ValueError("an image must be [h,w] or [h,w,3]")
    return a


def default_pattern():
    """The library's base sampling table, [256,4] int8 (ax, ay, bx, by); host-only, needs no GPU."""
    base = np.zeros((256, 4), dtype=np.int8)
    if _lib.load().sfm_orb_default_pattern(C.c_void_p(base.ctypes.data)) != 0:
        raise _lib.SfmError("sfm_orb_default_pattern failed")
    return base


def rotate_pattern(base):
    """[30,256,4] int8: the base table turned to each of the 30 angle bins; ValueError for a table with an endpoint outside
    radius 13.  Host-only, needs no GPU."""
    base = np.ascontiguousarray(base)
    if base.shape != (256, 4) or base.dtype != np.int8:
        raise ValueError("pattern must be a [256,4] int8 array")
    rot = np.zeros((30, 256, 4), dtype=np.int8)
    if _lib.load().sfm_orb_rotate_pattern(C.c_void_p(base.ctypes.data), C.c_void_p(rot.ctypes.data)) != 0:
        raise ValueError("pattern has an endpoint outside radius 13")
    return rot


_ROT = {}          # (device, bytes of the base table or None) -> the rotated table on that device


def _rot_table(pattern, device):
    import torch
    key = (int(device), None if pattern is None else np.ascontiguousarray(pattern, dtype=np.int8).tobytes())
    t = _ROT.get(key)
    if t is None:
        base = default_pattern() if pattern is None else np.ascontiguousarray(pattern, dtype=np.int8)
        t = _ROT[key] = torch.from_numpy(rotate_pattern(base)).to(torch.device("cuda", device))
    return t


def _upload_images(arrs, dev):
    """Images of several sizes -> one device byte array (back to back, through the matcher's pinned staging buffer, one
    copy) and its offsets."""
    import torch
    from .matcher import _pinned_stage
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    np.cumsum([a.size for a in arrs], out=off[1:])
    n_bytes = int(off[-1])
    host = _pinned_stage(max(n_bytes, 1))[:n_bytes].numpy()
    for a, o in zip(arrs, off):
        host[o:o + a.size] = a.reshape(-1)
    d = torch.from_numpy(host).to(dev, non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()          # the staging buffer is reused by the next call
    return d, off


def detect_and_describe_raw(images, masks=None, threshold=20, max_features=0, edge=31, pattern=None, device=0,
                            want_blurred=False):
    """The two device calls on gray uint8 images, outputs as the ABI gives them: {kp_ptr int64 [n_img+1], xy int32 [n,2],
    score uint8 [n], angle_bin uint8 [n], desc uint8 [n,32], blurred: list of [h,w] uint8 or None}.  masks: None, or one
    entry per image (None = no mask for that image)."""
    import torch
    from .driver import _p
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    imgs = [np.ascontiguousarray(_gray(a)) for a in images]
    n_img = len(imgs)
    if masks is not None:
        if len(masks) != n_img:
            raise ValueError("images / masks differ in length")
        ms = []
        for a, m in zip(imgs, masks):
            m = np.full(a.shape, 255, np.uint8) if m is None else np.asarray(m)
            if m.shape != a.shape:
                raise ValueError("a mask must have the shape of its image")
            ms.append(np.ascontiguousarray((m > 0).astype(np.uint8)))
    heights = np.array([a.shape[0] for a in imgs], dtype=np.int32)
    widths = np.array([a.shape[1] for a in imgs], dtype=np.int32)
    d_img, off = _upload_images(imgs, dev)
    d_mask = _upload_images(ms, dev)[0] if masks is not None else None
    hp = lambda a: C.c_void_p(a.ctypes.data)
    need = C.c_int64()
    h.check(h.lib.sfm_features_workspace_bytes(n_img, hp(off), C.byref(need)), "sfm_features_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    kp_ptr = torch.empty(n_img + 1, dtype=torch.int64, device=dev)
    h.call("sfm_features_detect", _p(d_img), _p(d_mask), hp(off), hp(heights), hp(widths), n_img, int(threshold), int(edge),
           int(max_features or 0), _p(kp_ptr), _p(ws), need.value)
    kp = kp_ptr.cpu().numpy()                              # the one read-back: output sizes are exact
    n = int(kp[-1])
    xy = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev)
    score = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    abin = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    desc = torch.empty((max(n, 1), 32), dtype=torch.uint8, device=dev)
    blurred = torch.empty(max(int(off[-1]), 1), dtype=torch.uint8, device=dev) if want_blurred else None
    rot = _rot_table(pattern, device)
    h.call("sfm_features_describe", _p(d_img), hp(off), hp(heights), hp(widths), n_img, _p(kp_ptr), n, _p(rot), _p(xy),
           _p(score), _p(abin), _p(desc), _p(blurred), _p(ws), need.value)
    out = {"kp_ptr": kp, "xy": xy[:n].cpu().numpy(), "score": score[:n].cpu().numpy(), "angle_bin": abin[:n].cpu().numpy(),
           "desc": desc[:n].cpu().numpy(), "blurred": None}
    if want_blurred:
        b = blurred.cpu().numpy()
        out["blurred"] = [b[off[i]:off[i] + imgs[i].size].reshape(imgs[i].shape) for i in range(n_img)]
    return out


def detect_and_describe_batched(images, masks=None, threshold=20, max_features=None, edge=31, pattern=None, device=0):
    """FAST-9/16 keypoints and 256-bit descriptors of every image in two device calls.  images: [h,w] uint8 arrays, or
    [h,w,3] in cv2.imread's channel order (BGR; converted on the host by OpenCV's integer rule); masks: per image None or an
    [h,w] array, a keypoint is kept only where it is > 0; max_features: keep the strongest per image (None / 0: all; ties at
    the cut go in row-major order); pattern: an optional [256,4] int8 base sampling table (default: the library's own).
    Returns one Features per image, keypoints in row-major order."""
    r = detect_and_describe_raw(images, masks, threshold, max_features or 0, edge, pattern, device)
    kp = r["kp_ptr"]
    out = []
    for i in range(len(kp) - 1):
        a, b = int(kp[i]), int(kp[i + 1])
        out.append(Features(r["xy"][a:b].astype(np.float32), r["score"][a:b].astype(np.float32),
                            r["angle_bin"][a:b].astype(np.float32) * np.float32(12.0), r["desc"][a:b].copy() if b > a else None))
    return out


def detect_features(image, mask=None, threshold=20, max_features=None, edge=31, pattern=None, device=0):
    """The reference's call shape for one image: (keypoints [n,2] float32, descriptors uint8 [n,32] or None)."""
    f = detect_and_describe_batched([image], None if mask is None else [mask], threshold, max_features, edge, pattern, device)[0]
    return f.xy, f.descriptors
