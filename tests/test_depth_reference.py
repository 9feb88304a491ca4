"""The dense-depth stage without a device: the vectorised restatement of tests/depth_reference.py against a second one in
plain loops, the rule header (sfm_amd/csrc/depth_rule.h) built for the host against NumPy bit for bit, the plan header
under the sanitizers, the quality of the rule on the synthetic scene, the plane choice, and the argument checks."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "depth_check.cpp")
SAMPLE_IN = np.dtype([("W", "<f8", 12), ("x", "<f8"), ("y", "<f8"), ("d", "<f8"), ("ws", "<i4"), ("hs", "<i4")])
SAMPLE_OUT = np.dtype([("valid", "<i4"), ("xi", "<i4"), ("yi", "<i4"), ("pad", "<i4"), ("q2", "<f8")])
REFINE_IN = np.dtype([("best", "<i4"), ("n_planes", "<i4"), ("sm", "<i4"), ("s0", "<i4"), ("sp", "<i4"), ("pad", "<i4"),
                      ("dm", "<f8"), ("d0", "<f8"), ("dp", "<f8")])


# ------------------------------------------------------------------------------------------- the second restatement
def census_loops(img):
    h, w = img.shape
    out = np.zeros((h, w), dtype=np.uint64)
    for y in range(h):
        for x in range(w):
            word = 0
            for k, (dy, dx) in enumerate(dr.OFFSETS):
                yy, xx = min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)
                if int(img[yy, xx]) < int(img[y, x]):
                    word |= 1 << k
            out[y, x] = word
    return out


def sample_one(W, x, y, d, ws, hs):
    """(valid, xi, yi, q2) of one sample in float64 scalars, operation for operation."""
    f = np.float64
    W = [f(v) for v in W]
    x, y, d = f(x), f(y), f(d)
    with np.errstate(all="ignore"):
        a = [(W[4 * i] * x + W[4 * i + 1] * y) + W[4 * i + 2] for i in range(3)]
        q = [d * a[i] + W[4 * i + 3] for i in range(3)]
        u, v = q[0] / q[2], q[1] / q[2]
        valid = bool(q[2] > 0 and u >= -0.5 and u < f(ws) - f(0.5) and v >= -0.5 and v < f(hs) - f(0.5))
        if not valid:
            return False, 0, 0, q[2]
        return True, min(int(np.floor(u + f(0.5))), ws - 1), min(int(np.floor(v + f(0.5))), hs - 1), q[2]


def sweep_loops(images, refs, sources, warps, planes, r):
    cen = [census_loops(a) for a in images]
    out = []
    for v, ref in enumerate(refs):
        h, w = images[ref].shape
        D = len(planes[v])
        c = np.zeros((D, h, w), dtype=np.int64)
        for k in range(D):
            for y in range(h):
                for x in range(w):
                    for s, W in zip(sources[v], warps[v]):
                        hs, ws = images[s].shape
                        ok, xi, yi, _ = sample_one(W, x, y, planes[v][k], ws, hs)
                        c[k, y, x] += bin(int(cen[ref][y, x]) ^ int(cen[s][yi, xi])).count("1") if ok else 24
        plane = np.zeros((h, w), np.int32); cost = np.zeros((h, w), np.uint16); depth = np.zeros((h, w), np.float32)
        for y in range(h):
            for x in range(w):
                S = [sum(int(c[k, min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)])
                         for dy in range(-r, r + 1) for dx in range(-r, r + 1)) for k in range(D)]
                best = min(range(D), key=lambda k: (S[k], k))
                plane[y, x], cost[y, x] = best, S[best]
                dep = np.float32(planes[v][best])
                if 0 < best < D - 1:
                    den = S[best - 1] - 2 * S[best] + S[best + 1]
                    if den > 0:
                        off = np.float64(S[best - 1] - S[best + 1]) / np.float64(2 * den)
                        j = best + 1 if off >= 0 else best - 1
                        w0 = np.float64(1.0) / np.float64(planes[v][best])
                        wv = w0 + abs(off) * (np.float64(1.0) / np.float64(planes[v][j]) - w0)
                        dep = np.float32(np.float64(1.0) / wv)
                depth[y, x] = dep
        out.append((plane, cost, depth))
    return out


def filter_loops(images, refs, sources, warps, backproj, maps, rel_tol, max_cost, min_consistent):
    out = []
    for v, ref in enumerate(refs):
        h, w = images[ref].shape
        n = np.zeros((h, w), np.uint8); keep = np.zeros((h, w), np.uint8); xyz = np.full((h, w, 3), np.nan)
        M = [np.float64(t) for t in np.asarray(backproj[v]).reshape(12)]
        for y in range(h):
            for x in range(w):
                d = np.float64(maps[v][2][y, x])
                if not np.isfinite(d):
                    continue
                cnt = 0
                for s, W in zip(sources[v], warps[v]):
                    if s not in refs:
                        continue
                    hs, ws = images[s].shape
                    ok, xi, yi, q2 = sample_one(W, x, y, d, ws, hs)
                    if not ok:
                        continue
                    ds = np.float64(maps[refs.index(s)][2][yi, xi])
                    with np.errstate(all="ignore"):
                        cnt += bool(np.isfinite(ds) and abs(ds - q2) <= np.float64(rel_tol) * q2)
                n[y, x] = cnt
                keep[y, x] = (max_cost is None or int(maps[v][1][y, x]) <= max_cost[v]) and cnt >= min_consistent
                with np.errstate(all="ignore"):
                    xyz[y, x] = [d * ((M[4 * i] * np.float64(x) + M[4 * i + 1] * np.float64(y)) + M[4 * i + 2]) + M[4 * i + 3] for i in range(3)]
        out.append((n, keep, xyz))
    return out


def random_warp(rng, size, kind="near"):
    """A warp around a sideways translation: about a pixel of motion per 0.1 of inverse depth, a little rotation and scale."""
    W = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    W[:, :3] += rng.normal(0, 0.02, (3, 3)) * [[1, 1, size], [1, 1, size], [1.0 / size, 1.0 / size, 1]]
    W[:, 3] = rng.normal(0, 1.0, 3) * [3.0 * size, 1.0, 0.05]
    if kind == "out":
        W[0, 3] += 1e4
    elif kind == "behind":
        W[2] = [0, 0, -1.0, -0.5]
    elif kind == "nan":
        W[rng.integers(3), rng.integers(4)] = np.nan
    return W.reshape(12)


def same(a, b):
    return all(x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes() for va, vb in zip(a, b) for x, y in zip(va, vb))


def random_case(rng, shapes, n_planes, kinds=("near",), constant=False):
    images = [np.full(s, 77, np.uint8) if constant else rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    n = len(images)
    refs = list(range(n - 1)) if n > 2 else list(range(n))      # the last image of a larger set has no depth map
    sources = [[s for s in range(n) if s != r] for r in refs]
    warps = [np.stack([random_warp(rng, max(shapes[r]), kinds[(r + k) % len(kinds)]) for k in range(len(sources[v]))]).reshape(-1, 12)
             if sources[v] else np.zeros((0, 12)) for v, r in enumerate(refs)]
    planes = [np.sort(rng.uniform(1.0, 6.0, n_planes)) for _ in refs]
    backproj = [rng.normal(size=12) for _ in refs]
    return images, refs, sources, warps, planes, backproj


def test_the_two_formulations_agree():
    rng = np.random.default_rng(5)
    seen_valid = 0
    cases = [(((1, 1), (1, 1)), 1, 0), (((1, 1), (3, 2), (2, 5)), 2, 4), (((7, 7), (5, 6), (6, 4)), 3, 0),
             (((4, 7), (7, 3), (5, 5)), 3, 4), (((6, 5), (5, 6)), 2, 1), (((3, 3),), 3, 2)]
    for shapes, D, r in cases:
        for kinds in (("near",), ("near", "out", "behind"), ("nan", "near")):
            images, refs, sources, warps, planes, backproj = random_case(rng, shapes, D, kinds)
            a = dr.sweep(images, refs, sources, warps, planes, r)
            assert same(a, sweep_loops(images, refs, sources, warps, planes, r)), (shapes, D, r, kinds)
            seen_valid += sum(int((m[1] != 24 * len(sources[v]) * (2 * r + 1) ** 2).sum()) for v, m in enumerate(a))
            limit = [int(12 * len(s) * (2 * r + 1) ** 2) for s in sources]
            for mc, lim in ((0, None), (1, limit), (2, limit)):
                f = dr.filter_views(images, refs, sources, warps, backproj, a, 0.3, lim, mc)
                assert same(f, filter_loops(images, refs, sources, warps, backproj, a, 0.3, lim, mc)), (shapes, D, r, kinds, mc)
    assert seen_valid > 100                                      # the random warps do land inside the sources
    for a in (rng.integers(0, 256, (7, 7), dtype=np.uint8), rng.integers(0, 2, (5, 9), dtype=np.uint8), np.zeros((1, 1), np.uint8)):
        assert np.array_equal(dr.census(a), census_loops(a))


def test_degenerate_inputs():
    rng = np.random.default_rng(6)
    # every sample out of view, behind the camera, or under a NaN warp: every c is 24, every S the same, best = 0, depth d_0
    for kind in ("out", "behind", "nan"):
        images, refs, sources, warps, planes, _ = random_case(rng, ((6, 7), (5, 5)), 3, (kind,))
        for v, (plane, cost, depth) in enumerate(dr.sweep(images, refs, sources, warps, planes, 1)):
            if kind != "nan":                                    # one NaN element leaves the other rows' samples alone
                assert (cost == 24 * 9).all()
            if (cost == 24 * 9).all():
                assert (plane == 0).all() and (depth == np.float32(planes[v][0])).all()
    # constant images: every census word is 0, every S_k is 0 where the samples are valid
    images, refs, sources, warps, planes, backproj = random_case(rng, ((7, 7), (7, 7)), 3, constant=True)
    warps = [np.array([[1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]])] * 2       # the identity: every sample valid
    maps = dr.sweep(images, refs, sources, warps, planes, 4)
    assert same(maps, sweep_loops(images, refs, sources, warps, planes, 4))
    for v, (plane, cost, depth) in enumerate(maps):
        assert (plane == 0).all() and (cost == 0).all() and (depth == np.float32(planes[v][0])).all()
    # a view without a source
    maps = dr.sweep(images, [0], [[]], [np.zeros((0, 12))], planes[:1], 2)
    assert (maps[0][0] == 0).all() and (maps[0][1] == 0).all()
    f = dr.filter_views(images, [0], [[]], [np.zeros((0, 12))], backproj[:1], maps, 0.01, None, 0)
    assert (f[0][0] == 0).all() and (f[0][1] == 1).all() and np.isfinite(f[0][2]).all()


# ------------------------------------------------------------------------------------------- the headers on the host
def build_check(tmp_path, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"), CHECK_SRC, "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return str(exe)


def run_records(exe, tmp_path, mode, rec, out_dtype):
    fin, fout = tmp_path / f"{mode}.in", tmp_path / f"{mode}.out"
    with open(fin, "wb") as f:
        f.write(np.int64(len(rec)).tobytes())
        f.write(rec.tobytes())
    run = subprocess.run([exe, mode, str(fin), str(fout)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    return np.fromfile(fout, dtype=out_dtype)


def sample_records(rng, n):
    rec = np.zeros(n, SAMPLE_IN)
    size = rng.choice([1, 2, 31, 96, 640], n)
    for k in range(n):
        rec["W"][k] = random_warp(rng, size[k], rng.choice(["near", "near", "near", "out", "behind", "nan"]))
    rec["x"], rec["y"] = np.floor(rng.uniform(0, 1, n) * size), np.floor(rng.uniform(0, 1, n) * size)
    rec["d"] = rng.uniform(0.5, 8.0, n)
    rec["ws"], rec["hs"] = size, rng.choice([1, 3, 72, 480], n)
    return rec


def boundary_records(rng):
    """Samples placed on the +-0.5 pixel boundaries: a pure shift W = [I | (b0, b1, 0)] with x, y and b exactly representable
    gives u = x + b0 without rounding, so u sits exactly on -0.5, ws - 0.5 and the halves between, and np.nextafter of the
    shift gives both neighbours."""
    recs = []
    for ws, hs in ((1, 1), (2, 3), (96, 72)):
        for edge_u in (-0.5, 0.5, ws - 1.5, ws - 0.5):
            for edge_v in (-0.5, hs - 0.5, 0.25):
                for nudge in (0, -1, 1):
                    x, y = float(rng.integers(0, 50)), float(rng.integers(0, 50))
                    b0, b1 = edge_u - x, edge_v - y
                    if nudge:
                        b0, b1 = np.nextafter(b0, np.inf * nudge), np.nextafter(b1, np.inf * nudge)
                    r = np.zeros(1, SAMPLE_IN)
                    r["W"] = [1, 0, 0, b0, 0, 1, 0, b1, 0, 0, 1, 0]
                    r["x"], r["y"], r["d"], r["ws"], r["hs"] = x, y, 1.0, ws, hs
                    recs.append(r)
    # the one input whose rounded u + 0.5 reaches the width: u one ulp under 0.5 in a 1-pixel-wide source
    r = np.zeros(1, SAMPLE_IN)
    r["W"] = [1, 0, 0, np.nextafter(0.5, 0.0), 0, 1, 0, np.nextafter(0.5, 0.0), 0, 0, 1, 0]
    r["d"], r["ws"], r["hs"] = 1.0, 1, 1
    recs.append(r)
    return np.concatenate(recs)


def numpy_samples(rec):
    out = np.zeros(len(rec), SAMPLE_OUT)
    for k, r in enumerate(rec):                                   # the warp differs per record
        v, xi, yi, q2 = dr.sample(r["W"], r["x"], r["y"], r["d"], int(r["ws"]), int(r["hs"]))
        out[k] = (int(v), int(xi), int(yi), 0, float(q2))
    return out


def refine_records(rng, n):
    rec = np.zeros(n, REFINE_IN)
    rec["n_planes"] = rng.integers(1, 40, n)
    rec["best"] = rng.integers(0, rec["n_planes"])
    rec["s0"] = rng.integers(0, 31105, n)
    rec["sm"] = rec["s0"] + rng.integers(0, 400, n) * (rng.random(n) < 0.9)
    rec["sp"] = rec["s0"] + rng.integers(0, 400, n) * (rng.random(n) < 0.9)
    w = np.sort(rng.uniform(0.1, 1.0, (n, 3)), axis=1)[:, ::-1]
    rec["dm"], rec["d0"], rec["dp"] = (1.0 / w).T
    return rec


def numpy_refine(rec):
    out = np.zeros(len(rec), np.float32)
    for k, r in enumerate(rec):
        D, b = int(r["n_planes"]), int(r["best"])
        planes = np.ones(D)
        S = np.zeros((D, 1, 1), np.int64)
        for o, (sv, dv) in zip((-1, 0, 1), ((r["sm"], r["dm"]), (r["s0"], r["d0"]), (r["sp"], r["dp"]))):
            if 0 <= b + o < D:
                planes[b + o], S[b + o] = dv, sv
        out[k] = dr.refine(np.full((1, 1), b, np.int64), S, planes)[0, 0]
    return out


def same_samples(got, want):
    q_same = got["q2"].view(np.uint64) == want["q2"].view(np.uint64)
    q_same |= np.isnan(got["q2"]) & np.isnan(want["q2"])          # the payload of a NaN is not part of the rule
    return (got["valid"] == want["valid"]).all() and (got["xi"] == want["xi"]).all() and (got["yi"] == want["yi"]).all() and q_same.all()


def test_rule_header_equals_numpy_bit_for_bit(tmp_path):
    exe = build_check(tmp_path, ["-O2"], "depth_check")
    rng = np.random.default_rng(31)
    rec = sample_records(rng, 20000)
    want = numpy_samples(rec)
    assert 0.1 < want["valid"].mean() < 0.9
    assert same_samples(run_records(exe, tmp_path, "sample", rec, SAMPLE_OUT), want)
    edge = boundary_records(rng)
    want = numpy_samples(edge)
    assert 0.2 < want["valid"].mean() < 0.8
    exact = edge[:-1][0::3]                                       # on the boundary itself: -0.5 is inside, size - 0.5 is outside
    u = exact["x"] + exact["W"][:, 3]
    v = exact["y"] + exact["W"][:, 7]
    inside = (u >= -0.5) & (u < exact["ws"] - 0.5) & (v >= -0.5) & (v < exact["hs"] - 0.5)
    assert (want["valid"][:-1][0::3] == inside).all() and inside.any() and not inside.all()
    assert want[-1]["valid"] == 1 and want[-1]["xi"] == 0 and want[-1]["yi"] == 0      # cut back to the last pixel
    assert same_samples(run_records(exe, tmp_path, "sample", edge, SAMPLE_OUT), want)
    ref = refine_records(rng, 20000)
    want = numpy_refine(ref)
    got = run_records(exe, tmp_path, "refine", ref, np.float32)
    assert got.tobytes() == want.tobytes()
    assert 0.3 < (want != ref["d0"].astype(np.float32)).mean() < 0.95                 # the sub-plane step is taken and skipped
    words = rng.integers(0, 2 ** 48, (5000, 2), dtype=np.uint64)
    assert np.array_equal(run_records(exe, tmp_path, "cost", words, np.int32), dr.popcount(words[:, 0] ^ words[:, 1]))


def test_rule_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """The same program with depth_plan.h, built with -fsanitize=address,undefined and run stand-alone: the thread map of tile
    plus halo (every slot written exactly once, nothing outside the image) for image sizes around the tile constants and
    smaller than a tile and than the window, the tables and the checks; then the rule on random and boundary records."""
    exe = build_check(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                 "-fno-omit-frame-pointer"], "depth_check_san")
    for seed in (1, 2):
        run = subprocess.run([exe, "plan", str(seed)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])
    rng = np.random.default_rng(32)
    rec = np.concatenate([sample_records(rng, 1500), boundary_records(rng)])
    assert same_samples(run_records(exe, tmp_path, "sample", rec, SAMPLE_OUT), numpy_samples(rec))
    assert len(run_records(exe, tmp_path, "sample", rec[:0], SAMPLE_OUT)) == 0
    ref = refine_records(rng, 1500)
    assert run_records(exe, tmp_path, "refine", ref, np.float32).tobytes() == numpy_refine(ref).tobytes()


# ------------------------------------------------------------------------------------------- what the rule is worth
def default_views(s):
    from sfm_amd import depth as dm
    refs = [0, 1, 2]
    sources = [[1, 2], [0, 2], [0, 1]]
    warps = [dm.view_warps(s.K, s.poses, r, src) for r, src in zip(refs, sources)]
    backproj = [dm.view_backprojection(s.K, s.poses, r) for r in refs]
    planes = dm.plane_depths(s.d_min, s.d_max, warps[1], s.size)
    return refs, sources, warps, backproj, planes


def quality(s=None, radius=2):
    """The figures of the default scene with the middle camera as reference: (planes, share within one plane, then per
    min_consistent in (1, 2): share kept, share of the kept within one plane).  rel_tol 0.02, mean cost <= 12 per sample."""
    s = s or dr.default_scene()
    refs, sources, warps, backproj, planes = default_views(s)
    maps = dr.sweep(s.images, refs, sources, warps, [planes] * 3, radius)
    truth = np.argmin(np.abs(1.0 / planes[:, None, None] - 1.0 / s.depth[1][None]), axis=0)
    within = np.abs(maps[1][0] - truth) <= 1
    out = [len(planes), within.mean()]
    limit = [12 * len(src) * (2 * radius + 1) ** 2 for src in sources]
    for mc in (1, 2):
        keep = dr.filter_views(s.images, refs, sources, warps, backproj, maps, 0.02, limit, mc)[1][1].astype(bool)
        out += [keep.mean(), within[keep].mean()]
    return out


def test_quality_on_the_default_scene():
    """Measured on the default scene (seed 0), r = 2, 17 planes: 98.99 % of the pixels within one plane of the truth;
    min_consistent = 1: 86.30 % kept, 99.85 % of them within one plane; min_consistent = 2: 53.20 % kept, 99.95 % of them
    within one plane.  Asserted less two percentage points for a change of texture seed (seeds 1 and 2 give 99.2 / 87.0 /
    99.8 / 53.5 / 99.9 and 99.2 / 86.5 / 99.9 / 53.5 / 100)."""
    n, within, kept1, good1, kept2, good2 = quality()
    print(f"planes {n}  within one plane {within:.4f}  mc=1: kept {kept1:.4f} good {good1:.4f}  mc=2: kept {kept2:.4f} good {good2:.4f}")
    assert abs(n - 17) <= 1
    assert within >= 0.9899 - 0.02
    assert kept1 >= 0.8630 - 0.02 and good1 >= 0.9985 - 0.02
    assert kept2 >= 0.5320 - 0.02 and good2 >= 0.9995 - 0.02
    assert good2 >= good1 >= within and kept1 > kept2             # what the filter is for


def test_plane_depths():
    from sfm_amd import depth as dm
    s = dr.default_scene()
    W = dm.view_warps(s.K, s.poses, 1, [0, 2])
    planes = dm.plane_depths(s.d_min, s.d_max, W, s.size)
    assert abs(len(planes) - 17) <= 1                             # f b (1 / 2.5 - 1 / 5) = 16 px of motion: 17 planes
    assert planes[0] == s.d_min and abs(planes[-1] - s.d_max) < 1e-12 and (np.diff(1.0 / planes) < 0).all()
    assert np.allclose(np.diff(1.0 / planes), np.diff(1.0 / planes)[0])
    # adjacent planes are at most a pixel apart at the corners, and one plane fewer would not be
    step = lambda p: np.nanmax(np.linalg.norm(np.diff(dm._corner_tracks(1.0 / p, W, s.size), axis=1), axis=2))
    assert step(planes) <= 1.0 + 1e-9 and step(1.0 / np.linspace(1 / s.d_min, 1 / s.d_max, len(planes) - 1)) > 1.0
    assert len(dm.plane_depths(s.d_min, s.d_max, W, s.size, max_planes=8)) == 8
    assert len(dm.plane_depths(2.5, 5.0, dm.view_warps(s.K, s.poses, 0, [2]), s.size)) == 33      # twice the baseline
    assert len(dm.plane_depths(3.0, 3.0, W, s.size)) == 1
    assert len(dm.plane_depths(2.5, 5.0, np.zeros((0, 12)), s.size, max_planes=20)) == 20
    for bad in (dict(d_min=0.0), dict(d_min=6.0), dict(d_max=float("inf")), dict(d_min=float("nan")), dict(max_planes=0),
                dict(max_planes=1025), dict(size=(0, 5))):
        with pytest.raises(ValueError):
            dm.plane_depths(**dict(dict(d_min=2.5, d_max=5.0, warps=W, size=s.size), **bad))


def test_warps_and_backprojection_are_consistent():
    """[A | b] and [M | c] against a direct projection: a pixel pushed to depth d and projected into the source."""
    from sfm_amd import depth as dm
    rng = np.random.default_rng(8)
    from sfm_amd.rotation import rodrigues
    K = [np.array([[100.0 + 10 * i, 0, 40 + i], [0, 105.0 + 7 * i, 30 - i], [0, 0, 1]]) for i in range(2)]
    poses = {i: (rodrigues(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, 3)) for i in range(2)}
    W = dm.view_warps(K, poses, 0, [1])[0].reshape(3, 4)
    M = dm.view_backprojection(K, poses, 0).reshape(3, 4)
    for x, y, d in ((3.0, 5.0, 2.0), (70.0, 11.0, 4.5)):
        X = d * (M[:, :3] @ [x, y, 1.0]) + M[:, 3]
        cam = poses[0][0] @ X + poses[0][1]
        assert np.allclose(K[0] @ cam / cam[2], [x, y, 1.0]) and np.isclose(cam[2], d)
        q = K[1] @ (poses[1][0] @ X + poses[1][1])
        assert np.allclose(d * (W[:, :3] @ [x, y, 1.0]) + W[:, 3], q)


# ------------------------------------------------------------------------------------------- argument checks, no device
def test_argument_checks_without_gpu(tmp_path):
    import sfm_amd
    from sfm_amd import depth as dm
    assert sfm_amd.depth_maps is dm.depth_maps and sfm_amd.dense_from_reconstruction is dm.dense_from_reconstruction
    s = dr.default_scene()
    refs, sources, warps, backproj, planes = default_views(s)
    good = dict(images=s.images, K=s.K, poses=s.poses, sources={1: [0, 2]}, planes={1: planes}, radius=2)
    out = dm.check_arguments(**good)
    assert out[1] == [1] and out[2].tolist() == [0, 2] and out[3].tolist() == [0, 2] and out[6].tolist() == [0, len(planes)]
    assert out[4].tobytes() == warps[1].tobytes() and out[5].tobytes() == backproj[1].reshape(1, 12).tobytes()
    bad_calls = [
        dict(good, radius=5), dict(good, radius=-1), dict(good, radius=1.5),
        dict(good, sources={1: [0, 1]}),                                      # a source is its own reference
        dict(good, sources={1: [0, 3]}), dict(good, sources={3: [0]}, planes={3: planes}),
        dict(good, sources={1: [0, 2] * 5}),                                  # more than 8 sources
        dict(good, planes={}), dict(good, planes={1: []}), dict(good, planes={1: np.ones(1025)}),
        dict(good, planes={1: [1.0, 0.0]}), dict(good, planes={1: [1.0, np.nan]}), dict(good, planes={1: [1.0, np.inf]}),
        dict(good, poses={0: s.poses[0], 1: s.poses[1]}),                     # a source without a pose
        dict(good, K=np.eye(4)), dict(good, sources=[(1, [0, 2])]),
        dict(good, images=[a.astype(np.float32) for a in s.images]),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            dm.depth_maps(**kw)
    for kw in (dict(n_sources=0), dict(n_sources=9)):
        with pytest.raises(ValueError):
            dm.select_sources(None, **kw)
    with pytest.raises(ValueError):
        dm.depth_ranges(None, margin=1.0)
    # save_ply_points: binary PLY, header and body sizes
    from sfm_amd.interchange import save_ply_points
    pts = np.arange(12.0).reshape(4, 3)
    for colors, per in ((None, 12), (np.arange(4, dtype=np.uint8), 15), (np.arange(12, dtype=np.uint8).reshape(4, 3), 15)):
        path = tmp_path / "cloud.ply"
        save_ply_points(pts, colors, path)
        raw = open(path, "rb").read()
        head, body = raw.split(b"end_header\n")
        assert head.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 4\n") and len(body) == 4 * per
        assert np.frombuffer(body[:12], "<f4").tolist() == [0.0, 1.0, 2.0]
    assert body[12:15] == bytes([2, 1, 0])                                    # BGR in, red green blue out
    with pytest.raises(ValueError):
        save_ply_points(pts, np.zeros((3, 3), np.uint8), tmp_path / "bad.ply")


def test_c_entry_points_reject_bad_calls_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    need = ctypes.c_int64(-1)
    assert lib.sfm_depth_workspace_bytes(3, 2, 4, ctypes.byref(need)) == 0 and need.value >= 4 * 16 + 3 * 56 + 16 + 12 + 8
    small = need.value
    assert lib.sfm_depth_workspace_bytes(300, 200, 1600, ctypes.byref(need)) == 0 and need.value > small
    assert lib.sfm_depth_workspace_bytes(0, 0, 0, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.sfm_depth_workspace_bytes(3, 2, 4, None) != 0
    assert lib.sfm_depth_workspace_bytes(-1, 0, 0, ctypes.byref(need)) != 0
    assert lib.sfm_depth_workspace_bytes(3, 4, 0, ctypes.byref(need)) != 0           # more views than images
    assert lib.sfm_depth_workspace_bytes(3, 2, 17, ctypes.byref(need)) != 0          # more than 8 sources a view
    assert lib.sfm_depth_census(None, None, None, None, None, 0, None, None, 0) != 0
    assert lib.sfm_depth_sweep(None, None, None, None, None, 0, 0, None, None, None, None, None, None, 2, None, None, None, None, 0) != 0
    assert lib.sfm_depth_filter(None, None, None, None, 0, 0, None, None, None, None, None, None, None, None, 0.01, 2,
                                None, None, None, None, 0) != 0
