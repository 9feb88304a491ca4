"""The multi-scale feature stage (include/sfm_amd.h, "multi-scale features") restated in NumPy from its text: the chained
level sizes, the 8-bit bilinear resampling, the mask rule, the union of the levels' keypoints with the one cut, and the
coordinate map.  A level itself is detected and described by tests/features_reference.py.  Also the zoom scenes, the
brute-force matcher and the correctness count of the "worth" measurement."""
import numpy as np

import features_reference as fr


# -------------------------------------------------------------------------------------------------------------- sizes
def check_options(n_levels, num, den):
    return 2 <= n_levels <= 16 and den < num <= 2 * den and num <= 16 and 8 * num >= 9 * den


def next_size(n, num, den):
    """A side of the next level; an empty side stays empty."""
    return 0 if n == 0 else max(1, (2 * n * den + num) // (2 * num))


def level_sizes(h, w, n_levels, num=6, den=5):
    """[(h_l, w_l)] for l = 0 .. n_levels - 1."""
    out = [(int(h), int(w))]
    for _ in range(1, n_levels):
        out.append((next_size(out[-1][0], num, den), next_size(out[-1][1], num, den)))
    return out


# --------------------------------------------------------------------------------------------------------- resampling
def taps(nd, ns):
    """(i0, i1, f) int64 [nd] of a destination axis of nd pixels over a source axis of ns."""
    x = np.arange(nd, dtype=np.int64)
    u = (2 * x + 1) * ns - nd
    i0 = u // (2 * nd)
    f = ((u % (2 * nd)) * 256) // (2 * nd)
    return i0, np.minimum(i0 + 1, ns - 1), f


def resample(src, hd, wd):
    src = np.asarray(src)
    if hd == 0 or wd == 0:
        return np.zeros((hd, wd), np.uint8)
    I = src.astype(np.int64)
    y0, y1, fy = taps(hd, I.shape[0])
    x0, x1, fx = taps(wd, I.shape[1])
    fy, gy = fy[:, None], 256 - fy[:, None]
    gx = 256 - fx
    v = gx * gy * I[y0][:, x0] + fx * gy * I[y0][:, x1] + gx * fy * I[y1][:, x0] + fx * fy * I[y1][:, x1]
    return ((v + 32768) >> 16).astype(np.uint8)


def resample_loops(src, hd, wd):
    """The same rule pixel by pixel in Python integers."""
    hs, ws = len(src), len(src[0])
    out = np.zeros((hd, wd), np.uint8)
    for y in range(hd):
        uy = (2 * y + 1) * hs - hd
        y0, fy = uy // (2 * hd), ((uy % (2 * hd)) * 256) // (2 * hd)
        y1 = min(y0 + 1, hs - 1)
        for x in range(wd):
            ux = (2 * x + 1) * ws - wd
            x0, fx = ux // (2 * wd), ((ux % (2 * wd)) * 256) // (2 * wd)
            x1 = min(x0 + 1, ws - 1)
            v = ((256 - fx) * (256 - fy) * int(src[y0][x0]) + fx * (256 - fy) * int(src[y0][x1])
                 + (256 - fx) * fy * int(src[y1][x0]) + fx * fy * int(src[y1][x1]) + 32768) >> 16
            out[y, x] = v
    return out


def resample_mask(mask, hd, wd):
    """1 exactly where all four source mask pixels of the destination pixel are > 0."""
    m = np.asarray(mask) > 0
    if hd == 0 or wd == 0:
        return np.zeros((hd, wd), np.uint8)
    y0, y1, _ = taps(hd, m.shape[0])
    x0, x1, _ = taps(wd, m.shape[1])
    return (m[y0][:, x0] & m[y0][:, x1] & m[y1][:, x0] & m[y1][:, x1]).astype(np.uint8)


def pyramid(img, n_levels, num=6, den=5, mask=None):
    """(levels, masks): level 0 is the image (and the mask as given); masks is None without a mask."""
    sizes = level_sizes(img.shape[0], img.shape[1], n_levels, num, den)
    lv = [np.asarray(img, dtype=np.uint8)]
    mk = None if mask is None else [np.asarray(mask, dtype=np.uint8)]
    for h, w in sizes[1:]:
        if mk is not None:
            mk.append(resample_mask(mk[-1], h, w))
        lv.append(resample(lv[-1], h, w))
    return lv, mk


# ----------------------------------------------------------------------------------------------------- union and cut
def cut_union(score, max_features):
    """Indices (ascending) of the keypoints that stay, and (s, above, ties, quota) of the cut - (0, n, 0, 0) without one."""
    sc = np.asarray(score).astype(np.int64)
    n = len(sc)
    if not max_features or n <= max_features:
        return np.arange(n), (0, n, 0, 0)
    hist = np.bincount(sc, minlength=256)
    above = 0
    for s in range(255, 0, -1):
        if above + hist[s] >= max_features:
            break
        above += hist[s]
    quota = max_features - above
    ties = np.nonzero(sc == s)[0]
    keep = np.sort(np.concatenate([np.nonzero(sc > s)[0], ties[:quota]]))
    return keep, (s, int(above), int(hist[s]), int(quota))


def map_coord(x, n0, nl):
    """float32 level-0 coordinate of pixel x of a level axis of nl pixels over n0: double arithmetic, rounded once."""
    x = np.asarray(x, dtype=np.int64)
    return ((((2 * x + 1).astype(np.float64) * np.float64(n0)) / np.float64(2 * nl)) - np.float64(0.5)).astype(np.float32)


def detect_and_describe(img, rot, mask=None, threshold=20, edge=31, max_features=0, n_levels=8, num=6, den=5,
                        precut=False):
    """dict(xy float32 [n,2], level, score, angle_bin, ambiguous, desc, src, lvl_count [n_levels], cut, levels, masks).  src
    indexes the uncut union unless precut, where every level is first cut to max_features (the device path) and src
    indexes the union of those."""
    lv, mk = pyramid(img, n_levels, num, den, mask)
    per = [fr.detect_and_describe(a, rot, None if mk is None else mk[l], threshold, edge, max_features if precut else 0)
           for l, a in enumerate(lv)]
    cnt = np.array([len(p["score"]) for p in per], dtype=np.int64)
    cat = lambda k, shape, dt: (np.concatenate([p[k] for p in per]) if cnt.sum() else np.zeros(shape, dt))
    xy_l, score = cat("xy", (0, 2), np.int32), cat("score", (0,), np.uint8)
    level = np.repeat(np.arange(n_levels), cnt).astype(np.uint8)
    keep, cut = cut_union(score, max_features)
    h0, w0 = lv[0].shape
    hl = np.array([a.shape[0] for a in lv])[level[keep]]
    wl = np.array([a.shape[1] for a in lv])[level[keep]]
    xy = np.zeros((len(keep), 2), np.float32)
    for k in range(len(keep)):          # per keypoint: the divisor differs
        xy[k, 0] = map_coord(xy_l[keep[k], 0], w0, wl[k])
        xy[k, 1] = map_coord(xy_l[keep[k], 1], h0, hl[k])
    return {"xy": xy, "level": level[keep], "score": score[keep], "angle_bin": cat("angle_bin", (0,), np.uint8)[keep],
            "ambiguous": cat("ambiguous", (0,), bool)[keep], "desc": cat("desc", (0, 32), np.uint8)[keep],
            "src": keep.astype(np.int32), "xy_level": xy_l[keep], "lvl_count": cnt, "cut": cut, "levels": lv, "masks": mk}


def single_scale(img, rot, threshold=20, edge=31):
    r = fr.detect_and_describe(img, rot, None, threshold, edge, 0)
    return {"xy": r["xy"].astype(np.float32), "desc": r["desc"]}


# ------------------------------------------------------------------------------------------------------------- worth
def box_average(img, k):
    """Exact k x k box average, rounded half up."""
    h, w = img.shape
    s = img.astype(np.int64).reshape(h // k, k, w // k, k).sum(axis=(1, 3))
    return ((2 * s + k * k) // (2 * k * k)).astype(np.uint8)


def zoom_pair(zn, zd, seed):
    """(A 240 x 240, B 240 zn / zd square): one fine scene seen at two distances; x_B = (x_A + 0.5) zn / zd - 0.5."""
    fine = fr.make_scene(480 * zn, 480 * zn, seed, noise=0)
    rng = np.random.default_rng(seed + 1000)
    out = []
    for k in (2 * zn, 2 * zd):
        a = box_average(fine, k).astype(np.int64)
        out.append(np.clip(a + rng.integers(-3, 4, size=a.shape), 0, 255).astype(np.uint8))
    return out[0], out[1]


_POP = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def match_ratio(da, db, ratio=0.75):
    """Brute-force Hamming, the nearest two of b for every a (ties: the lower index first), d1 < ratio * d2.
    -> int [m,2] (index in a, index in b)."""
    if len(da) == 0 or len(db) < 2:
        return np.zeros((0, 2), np.int64)
    out = []
    for i in range(len(da)):
        d = _POP[np.bitwise_xor(db, da[i])].sum(axis=1)
        o = np.argsort(d, kind="stable")[:2]
        if d[o[0]] < ratio * d[o[1]]:
            out.append((i, int(o[0])))
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def count_correct(xy_a, xy_b, matches, zn, zd, tol=3.0):
    if len(matches) == 0:
        return 0
    pa = (xy_a[matches[:, 0]].astype(np.float64) + 0.5) * zn / zd - 0.5
    d = np.linalg.norm(pa - xy_b[matches[:, 1]].astype(np.float64), axis=1)
    return int((d <= tol).sum())


def worth_case(zn, zd, seed, rot, n_levels):
    """(keypoints A, keypoints B, matches, correct) at threshold 20, edge 31, no cut."""
    a, b = zoom_pair(zn, zd, seed)
    if n_levels == 1:
        fa, fb = single_scale(a, rot), single_scale(b, rot)
    else:
        fa, fb = detect_and_describe(a, rot, n_levels=n_levels), detect_and_describe(b, rot, n_levels=n_levels)
    m = match_ratio(fa["desc"], fb["desc"])
    return len(fa["xy"]), len(fb["xy"]), len(m), count_correct(fa["xy"], fb["xy"], m, zn, zd)
