"""NumPy restatement of guided matching (sfm_amd/csrc/guided_rule.h, guided.hip), the fixed synthetic pair the feature was
specified on ("Scene A"), and a second, independent formulation in plain Python loops.

The gate, for a point (x1, y1) of image i, a point (x2, y2) of image j (float32 widened to float64) and the row-major F:
    a  = (f0*x1 + f1*y1) + f2      b  = (f3*x1 + f4*y1) + f5      c = (f6*x1 + f7*y1) + f8
    ta = (f0*x2 + f3*y2) + f6      tb = (f1*x2 + f4*y2) + f7
    s  = (x2*a + y2*b) + c
    den = fmin(a*a + b*b, ta*ta + tb*tb)
    gate = den > 0  and  s*s <= (thr*thr) * den
Every operation rounds on its own (NumPy never fuses), so the device - built without FMA contraction - gives the same
bits.  The match rule: C(q) = { t : gate(q, t) }; best / second = the two smallest (distance, t) over C(q); q is kept iff
|C(q)| >= 1, d1 <= max_distance (when given), |C(q)| == 1 or float(d1) < ratio * float(d2), and - with cross_check - q is
the smallest (distance, q') over { q' : gate(q', best) }."""
import math

import numpy as np

import fundamental_reference as fr

_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the gate
def gate_terms(F, p1, p2, thr):
    """(lhs, rhs, den) of the rule for every (q, t): [n1, n2] float64 arrays."""
    f = np.asarray(F, dtype=np.float64).ravel()
    p1 = np.asarray(p1, dtype=np.float32).reshape(-1, 2)
    p2 = np.asarray(p2, dtype=np.float32).reshape(-1, 2)
    x1, y1 = p1[:, None, 0].astype(np.float64), p1[:, None, 1].astype(np.float64)
    x2, y2 = p2[None, :, 0].astype(np.float64), p2[None, :, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        a = (f[0] * x1 + f[1] * y1) + f[2]
        b = (f[3] * x1 + f[4] * y1) + f[5]
        c = (f[6] * x1 + f[7] * y1) + f[8]
        ta = (f[0] * x2 + f[3] * y2) + f[6]
        tb = (f[1] * x2 + f[4] * y2) + f[7]
        s = (x2 * a + y2 * b) + c
        den = np.fmin(a * a + b * b, ta * ta + tb * tb)
        thr = np.float64(thr)
        lhs, rhs = s * s, (thr * thr) * den
    return lhs, rhs, np.broadcast_to(den, lhs.shape)


def gate(F, p1, p2, thr):
    """bool [n1, n2]: image i's points down, image j's across."""
    lhs, rhs, den = gate_terms(F, p1, p2, thr)
    with np.errstate(invalid="ignore"):
        return (den > 0) & (lhs <= rhs)


def near_threshold(F, p1, p2, thr, rel=1e-9):
    """bool [n1, n2]: combinations within `rel` (relative) of thr^2, where two correct formulations of the rule may differ."""
    lhs, rhs, _ = gate_terms(F, p1, p2, thr)
    with np.errstate(invalid="ignore"):
        return np.abs(lhs - rhs) <= rel * rhs


def cv_gate(F, p1, p2, thr):
    """The rule the project already ships (fundamental_reference.cv_err2 <= thr^2) and its 1e-9 band, [n1, n2] each."""
    p1 = np.asarray(p1, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    p2 = np.asarray(p2, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    n1, n2 = len(p1), len(p2)
    e = fr.cv_err2(np.asarray(F, dtype=np.float64).reshape(3, 3), np.repeat(p1, n2, axis=0), np.tile(p2, (n1, 1))).reshape(n1, n2)
    thr2 = float(thr) * float(thr)
    with np.errstate(invalid="ignore"):
        return e <= thr2, np.abs(e - thr2) <= 1e-9 * thr2


# ------------------------------------------------------------------------------------------------ distances
def distances(d1, d2, metric):
    """float32 [n1, n2]: the matcher's distance - the popcount ("hamming"), or sqrtf of the integer d^2 ("l2")."""
    d1 = np.asarray(d1, dtype=np.uint8); d2 = np.asarray(d2, dtype=np.uint8)
    if metric == "hamming":
        return _POPCOUNT[d1[:, None, :] ^ d2[None, :, :]].sum(-1).astype(np.float32)
    diff = d1[:, None, :].astype(np.int32) - d2[None, :, :].astype(np.int32)          # d^2 <= 128 * 255^2 < 2^31
    return np.sqrt((diff * diff).sum(-1).astype(np.float32))          # d^2 < 2^24: exact in float32; np.sqrt rounds correctly


def _best_of(D_row, cand):
    o = cand[np.lexsort((cand, D_row[cand]))]
    return o


# ------------------------------------------------------------------------------------------------ the match rule
def guided_match(kp1, kp2, desc1, desc2, F, gate_px=3.0, ratio=0.75, max_distance=None, cross_check=False, metric="hamming"):
    """(queryIdx int32, trainIdx int32, distance float32, n_candidates int32 [n1]) of one pair."""
    n1, n2 = len(kp1), len(kp2)
    ncand = np.zeros(n1, np.int32)
    if n1 == 0 or n2 == 0 or F is None:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), ncand
    ok = gate(F, kp1, kp2, gate_px)
    D = distances(desc1, desc2, metric)
    qs, ts, ds = [], [], []
    for q in range(n1):
        cand = np.flatnonzero(ok[q])
        ncand[q] = len(cand)
        if len(cand) == 0:
            continue
        o = _best_of(D[q], cand)
        best, d1 = int(o[0]), D[q, o[0]]
        if max_distance is not None and not float(d1) <= float(max_distance):
            continue
        if len(o) > 1 and not float(d1) < ratio * float(D[q, o[1]]):
            continue
        if cross_check:
            back = np.flatnonzero(ok[:, best])
            if int(back[np.lexsort((back, D[back, best]))][0]) != q:
                continue
        qs.append(q); ts.append(best); ds.append(d1)
    return np.array(qs, np.int32), np.array(ts, np.int32), np.array(ds, np.float32), ncand


def guided_batch(keypoints, descs, pairs, Fs, **kw):
    """guided_match per pair, and the CSR pointer of the batch: ([(q, t, d)], [n_candidates], seg_ptr int64)."""
    out, dbg, ptr = [], [], [0]
    for (i, j), F in zip(pairs, Fs):
        q, t, d, nc = guided_match(keypoints[i], keypoints[j], descs[i], descs[j], F, **kw)
        out.append((q, t, d)); dbg.append(nc); ptr.append(ptr[-1] + len(q))
    return out, dbg, np.array(ptr, np.int64)


# ------------------------------------------------------------------------------------------------ second formulation
def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def gate_scalar(f, x1, y1, x2, y2, thr):
    """The rule on Python floats (IEEE double, one rounding per operation); coordinates are float32 values."""
    x1, y1, x2, y2 = float(np.float32(x1)), float(np.float32(y1)), float(np.float32(x2)), float(np.float32(y2))
    a = (f[0] * x1 + f[1] * y1) + f[2]
    b = (f[3] * x1 + f[4] * y1) + f[5]
    c = (f[6] * x1 + f[7] * y1) + f[8]
    ta = (f[0] * x2 + f[3] * y2) + f[6]
    tb = (f[1] * x2 + f[4] * y2) + f[7]
    s = (x2 * a + y2 * b) + c
    den = _fmin(a * a + b * b, ta * ta + tb * tb)
    return den > 0 and s * s <= (thr * thr) * den


def guided_match_loops(kp1, kp2, desc1, desc2, F, gate_px=3.0, ratio=0.75, max_distance=None, cross_check=False, metric="hamming"):
    """The same rule as guided_match in plain Python: a double loop per query, a running best two, no sorting."""
    n1, n2 = len(kp1), len(kp2)
    ncand = np.zeros(n1, np.int32)
    if n1 == 0 or n2 == 0 or F is None:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), ncand
    f = [float(v) for v in np.asarray(F, dtype=np.float64).ravel()]
    k1 = [(float(p[0]), float(p[1])) for p in np.asarray(kp1, np.float32)]
    k2 = [(float(p[0]), float(p[1])) for p in np.asarray(kp2, np.float32)]
    b1 = [bytes(r) for r in np.asarray(desc1, np.uint8)]
    b2 = [bytes(r) for r in np.asarray(desc2, np.uint8)]

    def dist(q, t):
        if metric == "hamming":
            return np.float32(sum(bin(u ^ v).count("1") for u, v in zip(b1[q], b2[t])))
        return np.float32(math.sqrt(sum((u - v) * (u - v) for u, v in zip(b1[q], b2[t]))))      # the double root rounded once more: 53 >= 2 * 24 + 2 bits, so correctly rounded

    def less(d, i, e, j):
        return d < e or (d == e and i < j)
    qs, ts, ds = [], [], []
    for q in range(n1):
        best = second = None
        for t in range(n2 - 1, -1, -1):                      # backwards: the result must not depend on the order
            if not gate_scalar(f, k1[q][0], k1[q][1], k2[t][0], k2[t][1], gate_px):
                continue
            ncand[q] += 1
            d = dist(q, t)
            if best is None or less(d, t, best[0], best[1]):
                best, second = (d, t), best
            elif second is None or less(d, t, second[0], second[1]):
                second = (d, t)
        if best is None:
            continue
        if max_distance is not None and not float(best[0]) <= float(max_distance):
            continue
        if second is not None and not float(best[0]) < ratio * float(second[0]):
            continue
        if cross_check:
            back = None
            for qq in range(n1):
                if gate_scalar(f, k1[qq][0], k1[qq][1], k2[best[1]][0], k2[best[1]][1], gate_px):
                    d = dist(qq, best[1])
                    if back is None or less(d, qq, back[0], back[1]):
                        back = (d, qq)
            if back[1] != q:
                continue
        qs.append(q); ts.append(best[1]); ds.append(best[0])
    return np.array(qs, np.int32), np.array(ts, np.int32), np.array(ds, np.float32), ncand


# ------------------------------------------------------------------------------------------------ the blind matcher
def blind_match(desc1, desc2, ratio=0.75, metric="hamming"):
    """Global nearest neighbour + Lowe's ratio test (the matcher's rule): (queryIdx, trainIdx, distance)."""
    D = distances(desc1, desc2, metric)
    qs, ts, ds = [], [], []
    allt = np.arange(D.shape[1])
    for q in range(D.shape[0]):
        o = _best_of(D[q], allt)
        if len(o) > 1 and float(D[q, o[0]]) < ratio * float(D[q, o[1]]):
            qs.append(q); ts.append(int(o[0])); ds.append(D[q, o[0]])
    return np.array(qs, np.int32), np.array(ts, np.int32), np.array(ds, np.float32)


# ------------------------------------------------------------------------------------------------ Scene A
def flip_bits(rng, d, k):
    bits = np.unpackbits(d, axis=1)
    for r in range(bits.shape[0]):
        bits[r, rng.choice(bits.shape[1], k, replace=False)] ^= 1
    return np.packbits(bits, axis=1)


def scene(seed=5, n_points=300, group=3, extra=60, poses=None, n_bytes=32, flips=12, sizes=None):
    """A synthetic set of views of one point cloud with repeating descriptors.  The first half of the 3-D points get a random
    descriptor of their own, the other half come in groups of `group` that share one; every observation flips `flips` random
    bits of its base; `extra` partnerless keypoints per image are uniform in 1024 x 768 with random descriptors.  Keypoints
    are float32, 0.5 px Gaussian noise, a fresh permutation per image.  sizes: keep only that many of each image's points
    (after the permutation).  Returns dict(kps, descs, perms, poses, truth(i, j) -> {q: t})."""
    rng = np.random.default_rng(seed)
    N, G = n_points, group
    X = rng.uniform(-1, 1, (N, 3)) + [0, 0, 6.0]
    base = np.concatenate([rng.integers(0, 256, (N // 2, n_bytes), dtype=np.uint8),
                           rng.integers(0, 256, (N // 2 // G, n_bytes), dtype=np.uint8).repeat(G, axis=0)])
    if poses is None:
        yaw = 0.25
        R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        poses = [(np.eye(3), np.zeros(3)), (R, np.array([-1.5, 0.1, 0.3]))]
    kps, descs, perms = [], [], []
    for v, (R, t) in enumerate(poses):
        x = (X @ R.T + t) @ fr.K_REF.T
        x = x[:, :2] / x[:, 2:] + rng.normal(size=(N, 2)) * 0.5
        perm = rng.permutation(N)
        if sizes is not None:
            perm = perm[:sizes[v]]
        perms.append(perm)
        kps.append(np.concatenate([x[perm], rng.uniform(0, 1, (extra, 2)) * [1024, 768]]).astype(np.float32))
        descs.append(np.concatenate([flip_bits(rng, base[perm], flips), rng.integers(0, 256, (extra, n_bytes), dtype=np.uint8)]))

    def truth(i, j):
        inv = {p: k for k, p in enumerate(perms[j])}
        return {q: inv[p] for q, p in enumerate(perms[i]) if p in inv}
    return {"kps": kps, "descs": descs, "perms": perms, "poses": poses, "truth": truth}


def relative_F(pose_i, pose_j):
    """F with x_j^T F x_i = 0 for two world-to-camera poses, scaled to F[2,2] = 1."""
    Ri, ti = pose_i
    Rj, tj = pose_j
    R = Rj @ Ri.T
    t = tj - R @ ti
    F = fr.true_fundamental(R, t)
    return F / F[2, 2]


def scene_a():
    """The fixed pair every figure of the feature is quoted on: 300 points, 60 partnerless keypoints per image, 32-byte
    descriptors, 150 points in 50 groups of 3 sharing a base; F = the true fundamental matrix scaled to F[2,2] = 1."""
    sc = scene()
    sc["F"] = relative_F(sc["poses"][0], sc["poses"][1])
    return sc


def count_correct(q, t, truth):
    return sum(1 for a, b in zip(q.tolist(), t.tolist()) if truth.get(a) == b)
