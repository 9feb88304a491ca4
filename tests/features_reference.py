"""The feature stage (include/sfm_amd.h, "feature detection and description") restated in NumPy from the definitions:
the FAST score by its arc formula, the suppression by padded-array comparisons, the selection by a stable argsort, the
integer blur, the moments and the descriptor bits.  Everything is integer arithmetic except the atan2 of the orientation,
whose bin decision is reported as ambiguous when it falls on a bin edge.  Also the scene generator of the tests."""
import math

import numpy as np

CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]          # (dx, dy)
BLUR_W = np.array([18, 33, 49, 56, 49, 33, 18], dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------- scenes
def make_scene(h, w, seed, noise=6, levels=None):
    """A constant background, max(8, h*w/400) random filled rectangles of random gray, uniform noise in [-noise, noise],
    clipped; optionally quantised to `levels` gray levels."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), int(rng.integers(60, 200)), dtype=np.int64)
    for _ in range(max(8, h * w // 400)):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        hh, ww = int(rng.integers(2, max(3, h // 3))), int(rng.integers(2, max(3, w // 3)))
        img[y0:y0 + hh, x0:x0 + ww] = int(rng.integers(0, 256))
    if noise:
        img = img + rng.integers(-noise, noise + 1, size=img.shape)
    img = np.clip(img, 0, 255)
    if levels:
        step = 256 // levels
        img = (img // step) * step + step // 2
    return img.astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------- FAST
def fast_b(img):
    """b of the contract for every pixel at least 3 from the border (int array [h, w], -255 elsewhere): the maximum over the
    16 arcs of 9 contiguous circle pixels and both polarities of the smallest +d (or the smallest -d) on the arc."""
    I = img.astype(np.int64)
    h, w = I.shape
    b = np.full((h, w), -255, dtype=np.int64)
    if h < 7 or w < 7:
        return b
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in CIRCLE])
    best = np.full(c.shape, -255, dtype=np.int64)
    for a in range(16):
        arc = d[[(a + j) % 16 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    b[3:h - 3, 3:w - 3] = best
    return b


def fast_score(img, threshold=20):
    """uint8 score map: b - 1 where b > threshold, else 0."""
    b = fast_b(img)
    return np.where(b > threshold, b - 1, 0).astype(np.uint8)


def segment_test(img, y, x, threshold):
    """The published test itself, by brute force: 9 contiguous circle pixels all brighter than I(p) + t or all darker than
    I(p) - t."""
    c = int(img[y, x])
    v = [int(img[y + dy, x + dx]) for dx, dy in CIRCLE]
    for a in range(16):
        arc = [v[(a + j) % 16] for j in range(9)]
        if all(q > c + threshold for q in arc) or all(q < c - threshold for q in arc):
            return True
    return False


def suppress(score):
    """Scores that are strictly greater than all 8 neighbours (outside the image counts as 0); 0 elsewhere."""
    s = score.astype(np.int64)
    h, w = s.shape
    p = np.zeros((h + 2, w + 2), dtype=np.int64)
    p[1:-1, 1:-1] = s
    keep = s > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                keep &= s > p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return np.where(keep, s, 0).astype(np.uint8)


def gate(nms, edge, mask=None):
    h, w = nms.shape
    out = np.zeros_like(nms)
    if h >= 2 * edge + 1 and w >= 2 * edge + 1:
        out[edge:h - edge, edge:w - edge] = nms[edge:h - edge, edge:w - edge]
    if mask is not None:
        out[np.asarray(mask) == 0] = 0
    return out


def select(kept, max_features=0):
    """(xy int32 [n,2] as (x, y), score uint8 [n]) in row-major order after the cut to max_features (0: all)."""
    ys, xs = np.nonzero(kept)                                   # row-major
    sc = kept[ys, xs]
    if max_features and len(sc) > max_features:
        order = np.argsort(-sc.astype(np.int64), kind="stable")          # by score, ties in row-major order
        take = np.sort(order[:max_features])
        ys, xs, sc = ys[take], xs[take], sc[take]
    return np.stack([xs, ys], axis=1).astype(np.int32).reshape(-1, 2), sc.astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- blur
def reflect101(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def blur(img):
    I = img.astype(np.int64)
    h, w = I.shape
    if h == 0 or w == 0:
        return img.copy()
    cols = np.array([[reflect101(x + k - 3, w) for x in range(w)] for k in range(7)])
    rows = np.array([[reflect101(y + k - 3, h) for y in range(h)] for k in range(7)])
    horiz = sum(BLUR_W[k] * I[:, cols[k]] for k in range(7))
    both = sum(BLUR_W[k] * horiz[rows[k], :] for k in range(7))
    return ((both + 32768) >> 16).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------- orientation
_DISC = [(dx, dy) for dy in range(-15, 16) for dx in range(-15, 16) if dx * dx + dy * dy <= 225]
_DX = np.array([p[0] for p in _DISC])
_DY = np.array([p[1] for p in _DISC])


def moments(img, x, y):
    v = img[y + _DY, x + _DX].astype(np.int64)
    return int((_DX * v).sum()), int((_DY * v).sum())


def angle_bin(m10, m01):
    """(bin, ambiguous): ambiguous when a * 15 / pi sits within 1e-9 of a half-integer, or both moments are 0."""
    if m10 == 0 and m01 == 0:
        return 0, True
    t = math.atan2(float(m01), float(m10)) * 15.0 / math.pi
    frac = t - math.floor(t)
    return (int(math.floor(t + 0.5)) % 30 + 30) % 30, abs(frac - 0.5) < 1e-9


# ------------------------------------------------------------------------------------------------------------- pattern
def rotate_pattern(base):
    """[30,256,4] int8: bins 0 .. 14 by rotation in double with rounding half away from zero (libm's cos / sin, as the
    library's host code), bins 15 .. 29 their exact negatives."""
    base = np.asarray(base, dtype=np.int64).reshape(256, 4)
    rot = np.zeros((30, 256, 4), dtype=np.int64)
    away = lambda v: np.sign(v) * np.floor(np.abs(v) + 0.5)
    for b in range(15):
        th = b * (math.pi / 15.0)
        c, s = math.cos(th), math.sin(th)
        for e in (0, 2):
            x, y = base[:, e].astype(np.float64), base[:, e + 1].astype(np.float64)
            if b == 0:
                rot[b, :, e], rot[b, :, e + 1] = base[:, e], base[:, e + 1]
            else:
                rot[b, :, e] = away(x * c - y * s)
                rot[b, :, e + 1] = away(x * s + y * c)
        rot[b + 15] = -rot[b]
    return rot.astype(np.int8)


def describe(img, blurred, xy, rot):
    """(angle_bin uint8 [n], ambiguous bool [n], desc uint8 [n,32])."""
    n = len(xy)
    bins, amb = np.zeros(n, np.uint8), np.zeros(n, bool)
    desc = np.zeros((n, 32), np.uint8)
    B = blurred.astype(np.int64)
    for k, (x, y) in enumerate(np.asarray(xy).tolist()):
        bins[k], amb[k] = angle_bin(*moments(img, x, y))
        t = rot[bins[k]].astype(np.int64)
        bits = B[y + t[:, 1], x + t[:, 0]] < B[y + t[:, 3], x + t[:, 2]]
        desc[k] = np.packbits(bits, bitorder="little")
    return bins, amb, desc


def detect_and_describe(img, rot, mask=None, threshold=20, edge=31, max_features=0):
    """Everything of one image: dict(xy, score, angle_bin, ambiguous, desc, blurred, kept) - kept is the map after
    suppression, gate and mask, before the cut."""
    kept = gate(suppress(fast_score(img, threshold)), edge, mask)
    xy, sc = select(kept, max_features)
    bl = blur(img)
    bins, amb, desc = describe(img, bl, xy, rot)
    return {"xy": xy, "score": sc, "angle_bin": bins, "ambiguous": amb, "desc": desc, "blurred": bl, "kept": kept}


def bgr_to_gray(img):
    """OpenCV's 8-bit rule for COLOR_BGR2GRAY: (R*4899 + G*9617 + B*1868 + 8192) >> 14."""
    a = np.asarray(img).astype(np.int64)
    return ((a[..., 2] * 4899 + a[..., 1] * 9617 + a[..., 0] * 1868 + 8192) >> 14).astype(np.uint8)
