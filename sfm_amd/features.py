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

PyramidFeatures = namedtuple("PyramidFeatures", "xy response angle descriptors level size")
PyramidFeatures.__doc__ = """What n_levels > 1 returns per image.  xy float32 [n,2] in pixels of the image itself (level 0),
response, angle and descriptors as in Features; level uint8 [n], the pyramid level the keypoint was found on; size float32
[n], the side of its 31-pixel patch in pixels of the image: 31 * w0 / w_level.  Keypoints are in (level, row-major) order."""


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


def _check_pyramid(n_levels, scale):
    n_levels = int(n_levels)
    num, den = (int(v) for v in scale)
    if n_levels < 1:
        raise ValueError("n_levels must be at least 1")
    return n_levels, num, den


def _canonical_masks(imgs, masks):
    if len(masks) != len(imgs):
        raise ValueError("images / masks differ in length")
    ms = []
    for a, m in zip(imgs, masks):
        m = np.full(a.shape, 255, np.uint8) if m is None else np.asarray(m)
        if m.shape != a.shape:
            raise ValueError("a mask must have the shape of its image")
        ms.append(np.ascontiguousarray((m > 0).astype(np.uint8)))
    return ms


def _level_batch(h, dev, imgs, ms, n_levels, num, den):
    """Uploads the images and builds the level batch on the device: (lvl_images, lvl_masks or None, lvl_off, lvl_heights,
    lvl_widths) - the tables are host arrays over the n_img * n_levels slots."""
    import torch
    from .driver import _p
    hp = lambda a: C.c_void_p(a.ctypes.data)
    n_img = len(imgs)
    heights = np.array([a.shape[0] for a in imgs], dtype=np.int32)
    widths = np.array([a.shape[1] for a in imgs], dtype=np.int32)
    lvl_off = np.zeros(n_img * n_levels + 1, dtype=np.int64)
    lvl_h = np.zeros(n_img * n_levels, dtype=np.int32)
    lvl_w = np.zeros(n_img * n_levels, dtype=np.int32)
    if h.lib.sfm_features_pyramid_sizes(n_img, hp(heights), hp(widths), n_levels, num, den, hp(lvl_off), hp(lvl_h),
                                        hp(lvl_w)) != 0:
        raise _lib.SfmError("sfm_features_pyramid_sizes: n_levels must be in [2, 16], the scale num/den must satisfy "
                            "den < num <= 2 den, num <= 16 and 8 num >= 9 den, and the level batch must stay within 2^32 pixels")
    d_img, off = _upload_images(imgs, dev)
    d_mask = _upload_images(ms, dev)[0] if ms is not None else None
    need = C.c_int64()
    h.check(h.lib.sfm_features_pyramid_workspace_bytes(n_img, n_levels, C.byref(need)), "sfm_features_pyramid_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    n_px = max(int(lvl_off[-1]), 1)
    lvl_images = torch.empty(n_px, dtype=torch.uint8, device=dev)
    lvl_masks = torch.empty(n_px, dtype=torch.uint8, device=dev) if ms is not None else None
    h.call("sfm_features_pyramid", _p(d_img), _p(d_mask), hp(off), hp(heights), hp(widths), n_img, n_levels, num, den,
           _p(lvl_images), _p(lvl_masks), _p(ws), need.value)
    return lvl_images, lvl_masks, lvl_off, lvl_h, lvl_w


def pyramid_levels(images, masks=None, n_levels=8, scale=(6, 5), device=0):
    """The level batch the multi-scale stage detects on, read back: (levels, level_masks) - levels[i][l] is level l of image
    i as an [h_l, w_l] uint8 array (level 0 is the image); level_masks likewise (0 / 1 from level 1 on), or None without
    masks.  For tests and debugging."""
    import torch
    n_levels, num, den = _check_pyramid(n_levels, scale)
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    imgs = [np.ascontiguousarray(_gray(a)) for a in images]
    ms = _canonical_masks(imgs, masks) if masks is not None else None
    lvl_images, lvl_masks, lvl_off, lvl_h, lvl_w = _level_batch(h, dev, imgs, ms, n_levels, num, den)

    def split(t):
        b = t.cpu().numpy()
        return [[b[lvl_off[s]:lvl_off[s] + int(lvl_h[s]) * int(lvl_w[s])].reshape(lvl_h[s], lvl_w[s]).copy()
                 for s in range(i * n_levels, (i + 1) * n_levels)] for i in range(len(imgs))]
    return split(lvl_images), (split(lvl_masks) if ms is not None else None)


def _pyramid_raw(imgs, ms, threshold, max_features, edge, pattern, device, n_levels, num, den):
    """The multi-scale path: the level batch, detect and describe on it (each level pre-cut to max_features, which changes
    nothing), the merge.  One read-back more than the single-scale path."""
    import torch
    from .driver import _p
    h = _lib.get_handle(device)
    dev = torch.device("cuda", device)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    n_img = len(imgs)
    n_slot = n_img * n_levels
    lvl_images, lvl_masks, lvl_off, lvl_h, lvl_w = _level_batch(h, dev, imgs, ms, n_levels, num, den)
    need = C.c_int64()
    h.check(h.lib.sfm_features_workspace_bytes(n_slot, hp(lvl_off), C.byref(need)), "sfm_features_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    lvl_kp_ptr = torch.empty(n_slot + 1, dtype=torch.int64, device=dev)
    h.call("sfm_features_detect", _p(lvl_images), _p(lvl_masks), hp(lvl_off), hp(lvl_h), hp(lvl_w), n_slot, int(threshold),
           int(edge), int(max_features or 0), _p(lvl_kp_ptr), _p(ws), need.value)
    lvl_kp = lvl_kp_ptr.cpu().numpy()
    n_lvl = int(lvl_kp[-1])
    e = lambda *shape, dt=torch.uint8: torch.empty(shape, dtype=dt, device=dev)
    l_xy, l_score, l_bin, l_desc = e(max(n_lvl, 1), 2, dt=torch.int32), e(max(n_lvl, 1)), e(max(n_lvl, 1)), e(max(n_lvl, 1), 32)
    rot = _rot_table(pattern, device)
    h.call("sfm_features_describe", _p(lvl_images), hp(lvl_off), hp(lvl_h), hp(lvl_w), n_slot, _p(lvl_kp_ptr), n_lvl, _p(rot),
           _p(l_xy), _p(l_score), _p(l_bin), _p(l_desc), None, _p(ws), need.value)
    mneed = C.c_int64()
    h.check(h.lib.sfm_features_merge_workspace_bytes(n_img, n_levels, C.byref(mneed)), "sfm_features_merge_workspace_bytes")
    mws = torch.empty(mneed.value, dtype=torch.uint8, device=dev)
    kp_ptr = torch.empty(n_img + 1, dtype=torch.int64, device=dev)
    h.call("sfm_features_merge_count", _p(lvl_kp_ptr), _p(l_score), n_img, n_levels, int(max_features or 0), _p(kp_ptr),
           _p(mws), mneed.value)
    kp = kp_ptr.cpu().numpy()
    n = int(kp[-1])
    xy, level, score = e(max(n, 1), 2, dt=torch.float32), e(max(n, 1)), e(max(n, 1))
    abin, desc, src = e(max(n, 1)), e(max(n, 1), 32), e(max(n, 1), dt=torch.int32)
    h.call("sfm_features_merge_gather", _p(lvl_kp_ptr), _p(l_xy), _p(l_score), _p(l_bin), _p(l_desc), hp(lvl_h), hp(lvl_w),
           n_img, n_levels, _p(kp_ptr), n, _p(xy), _p(level), _p(score), _p(abin), _p(desc), _p(src), _p(mws), mneed.value)
    return {"kp_ptr": kp, "xy": xy[:n].cpu().numpy(), "score": score[:n].cpu().numpy(), "angle_bin": abin[:n].cpu().numpy(),
            "desc": desc[:n].cpu().numpy(), "blurred": None, "level": level[:n].cpu().numpy(), "src": src[:n].cpu().numpy(),
            "lvl_kp_ptr": lvl_kp, "lvl_off": lvl_off, "lvl_heights": lvl_h, "lvl_widths": lvl_w}


def detect_and_describe_raw(images, masks=None, threshold=20, max_features=0, edge=31, pattern=None, device=0,
                            want_blurred=False, n_levels=1, scale=(6, 5)):
    """The two device calls on gray uint8 images, outputs as the ABI gives them: {kp_ptr int64 [n_img+1], xy int32 [n,2],
    score uint8 [n], angle_bin uint8 [n], desc uint8 [n,32], blurred: list of [h,w] uint8 or None}.  masks: None, or one
    entry per image (None = no mask for that image).
    n_levels > 1: the multi-scale stage over a pyramid of that many levels at scale = (num, den); xy is then float32 in
    pixels of level 0 and the dict adds level uint8 [n], src int32 [n] (the keypoint's index in the level batch's list) and
    the level tables lvl_kp_ptr, lvl_off, lvl_heights, lvl_widths (slot i * n_levels + l); blurred is not available."""
    import torch
    from .driver import _p
    n_levels, num, den = _check_pyramid(n_levels, scale)
    if n_levels > 1:
        if want_blurred:
            raise ValueError("want_blurred needs n_levels = 1")
        imgs = [np.ascontiguousarray(_gray(a)) for a in images]
        ms = _canonical_masks(imgs, masks) if masks is not None else None
        return _pyramid_raw(imgs, ms, threshold, max_features, edge, pattern, device, n_levels, num, den)
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


def detect_and_describe_batched(images, masks=None, threshold=20, max_features=None, edge=31, pattern=None, device=0,
                                n_levels=1, scale=(6, 5)):
    """FAST-9/16 keypoints and 256-bit descriptors of every image in two device calls.  images: [h,w] uint8 arrays, or
    [h,w,3] in cv2.imread's channel order (BGR; converted on the host by OpenCV's integer rule); masks: per image None or an
    [h,w] array, a keypoint is kept only where it is > 0; max_features: keep the strongest per image (None / 0: all; ties at
    the cut go in row-major order); pattern: an optional [256,4] int8 base sampling table (default: the library's own).
    Returns one Features per image, keypoints in row-major order.
    n_levels > 1: every image is detected and described on a pyramid of n_levels levels, each scale = (num, den) times
    smaller than the one before (2 <= n_levels <= 16; den < num <= 2 den, num <= 16, num / den >= 9/8), and max_features is
    one budget over all levels.  Returns one PyramidFeatures per image, keypoints in (level, row-major) order, xy in pixels
    of the image."""
    r = detect_and_describe_raw(images, masks, threshold, max_features or 0, edge, pattern, device, n_levels=n_levels,
                                scale=scale)
    kp = r["kp_ptr"]
    out = []
    for i in range(len(kp) - 1):
        a, b = int(kp[i]), int(kp[i + 1])
        if "level" not in r:
            out.append(Features(r["xy"][a:b].astype(np.float32), r["score"][a:b].astype(np.float32),
                                r["angle_bin"][a:b].astype(np.float32) * np.float32(12.0), r["desc"][a:b].copy() if b > a else None))
            continue
        L = int(n_levels)
        lvl = r["level"][a:b]
        w0, wl = r["lvl_widths"][i * L], r["lvl_widths"][i * L:(i + 1) * L][lvl]
        size = (np.float64(31.0) * np.float64(w0) / wl.astype(np.float64)).astype(np.float32)
        out.append(PyramidFeatures(r["xy"][a:b].copy(), r["score"][a:b].astype(np.float32),
                                   r["angle_bin"][a:b].astype(np.float32) * np.float32(12.0),
                                   r["desc"][a:b].copy() if b > a else None, lvl.copy(), size))
    return out


def detect_features(image, mask=None, threshold=20, max_features=None, edge=31, pattern=None, device=0, n_levels=1,
                    scale=(6, 5)):
    """The reference's call shape for one image: (keypoints [n,2] float32, descriptors uint8 [n,32] or None); with
    n_levels > 1 over a pyramid, keypoints in pixels of the image."""
    f = detect_and_describe_batched([image], None if mask is None else [mask], threshold, max_features, edge, pattern, device,
                                    n_levels=n_levels, scale=scale)[0]
    return f.xy, f.descriptors
