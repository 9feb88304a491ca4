"""The fusion of the depth maps without a device: the vectorised restatement of tests/depth_fuse_reference.py against a
second one in plain loops, the new functions of sfm_amd/csrc/depth_rule.h and the scan plan of depth_plan.h built for the
host (bit for bit against NumPy, and under the sanitizers as a stand-alone program), the properties the rule promises, its
worth on the default scene, the argument checks and the PLY writer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import depth_fuse_reference as fr
import depth_reference as dr
from test_depth_reference import run_records, sample_one

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "depth_fuse_check.cpp")
NORMAL_IN = np.dtype([("d", "<f8"), ("X", "<f8", 3), ("dn", "<f8", 4), ("P", "<f8", (4, 3)), ("C", "<f8", 3), ("jump", "<f8")])
NORMAL_OUT = np.dtype([("valid", "<i4"), ("n", "<f4", 3)])
FUSED_IN = np.dtype([("acc", "<f8", 3), ("nacc", "<f8", 3), ("n_views", "<i4"), ("pad", "<i4")])
FUSED_OUT = np.dtype([("X", "<f8", 3), ("n", "<f4", 3), ("pad", "<i4")])


# ------------------------------------------------------------------------------------------- hand-made inputs
def backproject(M, depth):
    """xyz of a depth map as the filter writes it (NaN where the depth is not finite)."""
    h, w = depth.shape
    M = np.asarray(M, dtype=np.float64).reshape(3, 4)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = depth.astype(np.float64)
    with np.errstate(all="ignore"):
        xyz = np.stack([d * ((M[i, 0] * x + M[i, 1] * y) + M[i, 2]) + M[i, 3] for i in range(3)], axis=-1)
    xyz[~np.isfinite(d)] = np.nan
    return xyz


def keep_pattern(rng, shape, kind):
    if kind == "zero":
        return np.zeros(shape, np.uint8)
    if kind == "ones":
        return np.ones(shape, np.uint8)
    if kind == "checker":
        y, x = np.mgrid[0:shape[0], 0:shape[1]]
        return ((x + y) % 2).astype(np.uint8)
    return (rng.random(shape) < 0.7).astype(np.uint8)


def plane_case(rng, shapes, refs, sources, keep_kinds=("random",), noise=0.004, bad=0.05, f=None, break_warp=None):
    """Cameras on a line along x looking down +z at the slanted plane a X + b Y + Z = z0, each image with its own size and
    principal point: the true depth of every reference pixel, perturbed by `noise` (relative, so that at rel_tol 0.01 some
    partners agree and some do not), a share `bad` of NaN, +inf and far-off depths, keep per view after keep_kinds, xyz as
    the filter back-projects it.  break_warp = (view, entry, kind) replaces one warp by a NaN one or one behind the camera.
    Returns (shapes, refs, sources, warps, backproj, depth, keep, xyz)."""
    from sfm_amd import depth as dm
    n = len(shapes)
    f = f or 1.5 * max(max(s) for s in shapes)
    K = [np.array([[f, 0, (w - 1) / 2.0], [0, f, (h - 1) / 2.0], [0, 0, 1.0]]) for h, w in shapes]
    centre = [np.array([0.11 * (i - (n - 1) / 2.0), 0.03 * (i % 2), 0.0]) for i in range(n)]
    poses = {i: (np.eye(3), -centre[i]) for i in range(n)}
    a, b, z0 = 0.15, -0.1, 3.0
    warps = [dm.view_warps(K, poses, r, src) if src else np.zeros((0, 12)) for r, src in zip(refs, sources)]
    if break_warp is not None:
        v, e, kind = break_warp
        warps[v] = warps[v].copy()
        if kind == "nan":
            warps[v][e, 5] = np.nan
        else:
            warps[v][e, 8:12] = [0, 0, -1.0, -0.5]
    backproj = [dm.view_backprojection(K, poses, r) for r in refs]
    depth, keep, xyz = [], [], []
    for v, r in enumerate(refs):
        h, w = shapes[r]
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        rx, ry = (x - K[r][0, 2]) / f, (y - K[r][1, 2]) / f
        d = (z0 - a * centre[r][0] - b * centre[r][1]) / (a * rx + b * ry + 1.0)
        d = d * (1.0 + rng.normal(0, noise, d.shape))
        u = rng.random(d.shape)
        d = np.where(u < bad / 3, np.nan, np.where(u < 2 * bad / 3, np.inf, np.where(u < bad, d * 1.3, d)))
        depth.append(d.astype(np.float32))
        keep.append(keep_pattern(rng, (h, w), keep_kinds[v % len(keep_kinds)]))
        xyz.append(backproject(backproj[v], depth[-1]))
    return list(shapes), list(refs), [list(s) for s in sources], warps, backproj, depth, keep, xyz


def all_to_all(n_img, n_ref=None):
    refs = list(range(n_img if n_ref is None else n_ref))
    return refs, [[s for s in range(n_img) if s != r] for r in refs]


# ------------------------------------------------------------------------------------------- the second restatement
def normal_one(d, X, dn, P, C, jump):
    """(valid, float32 [3]) of one pixel in float64 scalars, operation for operation.  dn / P: the neighbours (x+t, x-t, y+t, y-t)."""
    f = np.float64
    zero = np.zeros(3, np.float32)
    with np.errstate(all="ignore"):
        if not np.isfinite(d):
            return False, zero
        for k in range(4):
            if not (np.isfinite(dn[k]) and abs(f(dn[k]) - f(d)) <= f(jump) * f(d)):
                return False, zero
        a = [f(P[0][i]) - f(P[1][i]) for i in range(3)]
        b = [f(P[2][i]) - f(P[3][i]) for i in range(3)]
        n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
        l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        if not (np.isfinite(l2) and l2 > 0):
            return False, zero
        l = np.sqrt(l2)
        n = [n[i] / l for i in range(3)]
        c = [f(C[i]) - f(X[i]) for i in range(3)]
        if ((n[0] * c[0] + n[1] * c[1]) + n[2] * c[2]) < 0:
            n = [-n[i] for i in range(3)]
        return True, np.array(n, dtype=np.float64).astype(np.float32)


def unit_one(acc):
    f = np.float64
    with np.errstate(all="ignore"):
        l2 = (f(acc[0]) * f(acc[0]) + f(acc[1]) * f(acc[1])) + f(acc[2]) * f(acc[2])
        if not (np.isfinite(l2) and l2 > 0):
            return np.zeros(3, np.float32)
        l = np.sqrt(l2)
        return np.array([f(acc[i]) / l for i in range(3)], dtype=np.float64).astype(np.float32)


def fuse_loops(shapes, refs, sources, warps, backproj, depth, keep, xyz, rel_tol, step, jump):
    out = fr.Fused()
    clamp = lambda v, hi: min(max(v, 0), hi)
    out.view_normals = []
    for v, ref in enumerate(refs):
        h, w = shapes[ref]
        C = np.asarray(backproj[v], dtype=np.float64).reshape(3, 4)[:, 3]
        nm = np.zeros((h, w, 3), np.float32)
        for y in range(h):
            for x in range(w):
                nb = [(y, clamp(x + step, w - 1)), (y, clamp(x - step, w - 1)), (clamp(y + step, h - 1), x), (clamp(y - step, h - 1), x)]
                nm[y, x] = normal_one(np.float64(depth[v][y, x]), xyz[v][y, x], [np.float64(depth[v][q]) for q in nb],
                                      [xyz[v][q] for q in nb], C, jump)[1]
        out.view_normals.append(nm)
    out.agree_mask, out.owner = [], []
    pts, nrm, cnt, idx, pt_ptr = [], [], [], [], [0]
    for v, ref in enumerate(refs):
        h, w = shapes[ref]
        mask, own = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
        for y in range(h):
            for x in range(w):
                if not keep[v][y, x]:
                    continue
                d = np.float64(depth[v][y, x])
                acc = [np.float64(t) for t in xyz[v][y, x]]
                nacc = [np.float64(t) for t in out.view_normals[v][y, x]]
                m, owner, n_views = 0, True, 1
                for e, (s, W) in enumerate(zip(sources[v], warps[v])):
                    if s not in refs:
                        continue
                    hs, ws = shapes[s]
                    ok, xi, yi, q2 = sample_one(W, x, y, d, ws, hs)
                    if not ok:
                        continue
                    rs = refs.index(s)
                    ds = np.float64(depth[rs][yi, xi])
                    with np.errstate(all="ignore"):
                        if not (np.isfinite(ds) and abs(ds - q2) <= np.float64(rel_tol) * q2 and keep[rs][yi, xi]):
                            continue
                        m |= 1 << e
                        n_views += 1
                        owner = owner and not rs < v
                        acc = [acc[i] + np.float64(xyz[rs][yi, xi][i]) for i in range(3)]
                        nacc = [nacc[i] + np.float64(out.view_normals[rs][yi, xi][i]) for i in range(3)]
                mask[y, x], own[y, x] = m, owner
                if owner:
                    with np.errstate(all="ignore"):
                        pts.append([acc[i] / np.float64(n_views) for i in range(3)])
                    nrm.append(unit_one(nacc))
                    cnt.append(n_views)
                    idx.append((v, y, x))
        out.agree_mask.append(mask)
        out.owner.append(own)
        pt_ptr.append(len(pts))
    out.pt_ptr = np.array(pt_ptr, dtype=np.int64)
    out.points = np.array(pts, dtype=np.float64).reshape(-1, 3)
    out.normals = np.array(nrm, dtype=np.float32).reshape(-1, 3)
    out.n_views = np.array(cnt, dtype=np.uint8)
    out.index = np.array(idx, dtype=np.int32).reshape(-1, 3)
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    b = a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()
    b[np.isnan(a)] = 0                                            # the payload of a NaN is not part of the rule
    return b


PER_VIEW, FLAT = ("view_normals", "agree_mask", "owner"), ("pt_ptr", "points", "normals", "n_views", "index")


def assert_same(a, b, what=""):
    for name in PER_VIEW:
        for v, (x, y) in enumerate(zip(getattr(a, name), getattr(b, name))):
            assert x.dtype == y.dtype and x.shape == y.shape, (what, name, v, x.dtype, y.dtype, x.shape, y.shape)
            assert np.array_equal(bits(x), bits(y)), (what, name, v, int((bits(x) != bits(y)).sum()))
    for name in FLAT:
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        assert np.array_equal(bits(x), bits(y)), (what, name, int((bits(x) != bits(y)).any(axis=-1).sum() if x.ndim > 1 else (bits(x) != bits(y)).sum()))


def test_the_two_formulations_agree():
    rng = np.random.default_rng(7)
    seen_partner = seen_dropped = seen_normal = 0
    for shapes, n_ref, step, kinds in ((((5, 6), (6, 5), (4, 7)), 3, 1, ("random",)), (((7, 9), (8, 8)), 2, 2, ("random", "checker")),
                                       (((1, 1), (1, 5), (6, 1)), 3, 1, ("ones",)), (((9, 10), (10, 9), (8, 11)), 2, 4, ("random",)),
                                       (((6, 6), (6, 6), (5, 5)), 3, 2, ("zero", "ones", "random"))):
        refs, sources = all_to_all(len(shapes), n_ref)
        case = plane_case(rng, shapes, refs, sources, kinds)
        for rel_tol, jump in ((0.01, 0.05), (0.0, 0.0), (0.5, 10.0)):
            a = fr.fuse(*case, rel_tol, step, jump)
            assert_same(a, fuse_loops(*case, rel_tol, step, jump), (shapes, step, rel_tol))
            seen_partner += int((a.n_views > 1).sum())
            seen_dropped += sum(int(((k != 0) & (o == 0)).sum()) for k, o in zip(case[6], a.owner))
            seen_normal += int(a.normals.any(axis=1).sum())
    assert seen_partner > 100 and seen_dropped > 100 and seen_normal > 100      # the cases are not trivial ones


# ------------------------------------------------------------------------------------------- the headers on the host
def build_check(tmp_path, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"), CHECK_SRC, "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return str(exe)


def normal_records(rng, n):
    """Neighbourhoods of a slanted surface seen from a camera: most valid, some across a depth jump, some with a NaN or
    infinite depth, some degenerate (a = 0, as at a clamped border), some huge (l2 overflows) or tiny (l2 underflows to 0)."""
    rec = np.zeros(n, NORMAL_IN)
    rec["C"] = rng.normal(0, 1, (n, 3))
    rec["jump"] = rng.choice([0.0, 0.01, 0.05, 0.5], n)
    d = rng.uniform(1.0, 6.0, n)
    rec["d"] = d
    rec["dn"] = d[:, None] * (1.0 + rng.normal(0, 0.02, (n, 4)))
    X = rec["C"] + rng.normal(0, 1, (n, 3)) * [1, 1, 0] + d[:, None] * [0, 0, 1.0]
    rec["X"] = X
    off = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0]]) * 0.05
    rec["P"] = X[:, None, :] + off[None] + rng.normal(0, 0.01, (n, 4, 3))
    kind = rng.integers(0, 12, n)
    rec["dn"][kind == 0, 1] = np.nan
    rec["dn"][kind == 1, 2] = np.inf
    rec["d"][kind == 2] = np.nan
    rec["P"][kind == 3, 0] = rec["P"][kind == 3, 1]                # a = 0
    rec["P"][kind == 4] *= 1e160                                  # l2 = inf
    sel = kind == 5
    rec["P"][sel] = off[None] * 1e-170         # differences so small that l2 underflows to 0
    rec["dn"][kind == 6] = rec["d"][kind == 6, None]              # exactly on the centre depth: passes jump = 0
    rec["P"][kind == 7, 2, 1] = np.nan
    return rec


def numpy_normals(rec):
    """Each record as the centre of a 3 x 3 map at step 1, through the vectorised restatement."""
    out = np.zeros(len(rec), NORMAL_OUT)
    for k, r in enumerate(rec):
        depth = np.full((3, 3), np.nan)
        xyz = np.full((3, 3, 3), np.nan)
        depth[1, 1], xyz[1, 1] = r["d"], r["X"]
        for q, dn, P in zip(((1, 2), (1, 0), (2, 1), (0, 1)), r["dn"], r["P"]):
            depth[q], xyz[q] = dn, P
        nm = fr.view_normals(depth, xyz, r["C"], 1, float(r["jump"]))[1, 1]
        out[k] = (int(nm.any()), nm)
    return out


def fused_records(rng, n):
    rec = np.zeros(n, FUSED_IN)
    rec["n_views"] = rng.integers(1, 10, n)
    rec["acc"] = rng.normal(0, 5, (n, 3)) * rec["n_views"][:, None]
    unit = rng.normal(0, 1, (n, 9, 3))
    unit = (unit / np.linalg.norm(unit, axis=2, keepdims=True)).astype(np.float32).astype(np.float64)
    use = np.arange(9)[None, :] < rec["n_views"][:, None]
    rec["nacc"] = (unit * use[..., None]).sum(axis=1)
    kind = rng.integers(0, 10, n)
    rec["nacc"][kind == 0] = 0.0                                  # no view has a normal
    rec["nacc"][kind == 1] = [1.0, 0.0, 0.0]
    rec["acc"][kind == 2, 1] = np.nan
    rec["nacc"][kind == 3] *= 1e-170                              # l2 underflows to 0
    return rec


def numpy_fused(rec):
    out = np.zeros(len(rec), FUSED_OUT)
    with np.errstate(all="ignore"):
        out["X"] = rec["acc"] / rec["n_views"].astype(np.float64)[:, None]
    out["n"] = fr.unit(rec["nacc"])
    return out


def same_records(got, want, names):
    return all(np.array_equal(bits(got[n]), bits(want[n])) for n in names)


def test_rule_header_equals_numpy_bit_for_bit(tmp_path):
    exe = build_check(tmp_path, ["-O2"], "depth_fuse_check")
    rng = np.random.default_rng(41)
    rec = normal_records(rng, 20000)
    want = numpy_normals(rec)
    assert 0.2 < want["valid"].mean() < 0.8
    flipped = np.einsum("ij,ij->i", want["n"].astype(np.float64), rec["C"] - rec["X"])
    assert (flipped[want["valid"] == 1] >= -1e-6).all()          # every valid normal looks at the camera
    assert same_records(run_records(exe, tmp_path, "normal", rec, NORMAL_OUT), want, ("valid", "n"))
    rec = fused_records(rng, 20000)
    want = numpy_fused(rec)
    assert 0.7 < want["n"].any(axis=1).mean() < 0.9
    assert same_records(run_records(exe, tmp_path, "fused", rec, FUSED_OUT), want, ("X", "n"))


def test_rule_and_scan_plan_under_address_and_ub_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone: the two-level scan as the kernels walk
    it (every count in one thread's hands, the bases equal to a running sum for block counts around the chunk size and for
    more chunks than the top level takes in one tile), pt_ptr from the views of random batches, the layout and the parameter
    checks; then the rule on random records."""
    exe = build_check(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                 "-fno-omit-frame-pointer"], "depth_fuse_check_san")
    for seed in (1, 2):
        run = subprocess.run([exe, "scan", str(seed)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])
    rng = np.random.default_rng(42)
    rec = normal_records(rng, 1500)
    assert same_records(run_records(exe, tmp_path, "normal", rec, NORMAL_OUT), numpy_normals(rec), ("valid", "n"))
    assert len(run_records(exe, tmp_path, "normal", rec[:0], NORMAL_OUT)) == 0
    rec = fused_records(rng, 1500)
    assert same_records(run_records(exe, tmp_path, "fused", rec, FUSED_OUT), numpy_fused(rec), ("X", "n"))


# ------------------------------------------------------------------------------------------- what the rule promises
def check_properties(case, out, rel_tol):
    shapes, refs, sources, warps, backproj, depth, keep, xyz = case
    assert np.array_equal(out.owner[0], (keep[0] != 0).astype(np.uint8))                  # view 0 loses nothing
    counts = [int(o.sum()) for o in out.owner]
    assert np.array_equal(out.pt_ptr, np.cumsum([0] + counts)) and len(out.points) == out.pt_ptr[-1]
    key = (out.index[:, 0].astype(np.int64) << 40) + (out.index[:, 1].astype(np.int64) << 20) + out.index[:, 2]
    assert (np.diff(key) > 0).all()                               # (view, y, x) ascends strictly
    for v in range(len(refs)):
        assert ((out.owner[v] == 0) | (keep[v] != 0)).all() and (out.agree_mask[v][keep[v] == 0] == 0).all()
        assert np.array_equal(out.index[out.index[:, 0] == v][:, 1:], np.argwhere(out.owner[v]))
        # a kept pixel that is not an owner has an agreeing kept partner in an earlier view
        h, w = shapes[refs[v]]
        y, x = np.mgrid[0:h, 0:w]
        earlier = np.zeros((h, w), bool)
        for e, (s, W) in enumerate(zip(sources[v], warps[v])):
            if s not in refs or refs.index(s) >= v or 0 in shapes[s]:
                continue
            rs = refs.index(s)
            valid, xi, yi, q2 = dr.sample(W, x, y, depth[v].astype(np.float64), shapes[s][1], shapes[s][0])
            agree = ((out.agree_mask[v] >> e) & 1).astype(bool)
            assert (valid & (keep[rs][yi, xi] != 0))[agree].all()
            earlier |= agree
        assert np.array_equal((keep[v] != 0) & (out.owner[v] == 0), earlier)
    popcount = lambda m: np.unpackbits(m.reshape(-1, 1), axis=1).sum(axis=1)
    flat_mask = np.concatenate([m[o != 0] for m, o in zip(out.agree_mask, out.owner)]) if len(refs) else np.zeros(0, np.uint8)
    assert np.array_equal(out.n_views, (1 + popcount(flat_mask)).astype(np.uint8))
    length = np.linalg.norm(out.normals.astype(np.float64), axis=1)
    assert (np.abs(length[length > 0] - 1.0) < 1e-6).all()


def test_properties():
    rng = np.random.default_rng(9)
    for shapes, n_ref in ((((12, 14), (13, 12), (11, 15)), 3), (((10, 10),) * 4, 3), (((9, 13), (13, 9)), 2)):
        refs, sources = all_to_all(len(shapes), n_ref)
        case = plane_case(rng, shapes, refs, sources)
        out = fr.fuse(*case, 0.01, 2, 0.05)
        check_properties(case, out, 0.01)
        dropped = sum(int(((k != 0) & (o == 0)).sum()) for k, o in zip(case[6], out.owner))
        assert dropped > 20 and (out.n_views > 1).sum() > 20      # the cases are not trivial ones
    # views listed against the image order: the position decides
    refs, sources = [2, 0, 1], [[0, 1], [1, 2], [2, 0]]
    case = plane_case(rng, ((12, 12),) * 3, refs, sources)
    check_properties(case, fr.fuse(*case, 0.01, 1, 0.05), 0.01)
    # a view without sources, and one whose only source has no maps: every kept pixel an owner, n_views = 1
    case = plane_case(rng, ((8, 9), (9, 8), (7, 7)), [0, 1], [[], [2]], ("ones", "random"))
    out = fr.fuse(*case, 0.5, 2, 0.05)
    check_properties(case, out, 0.5)
    assert all(np.array_equal(o, (k != 0).astype(np.uint8)) for o, k in zip(out.owner, case[6]))
    assert (out.n_views == 1).all() and all((m == 0).all() for m in out.agree_mask)
    # width 1 and height 1: no valid normal, for every step
    for shapes in (((1, 9), (9, 1)), ((1, 1), (1, 2))):
        case = plane_case(rng, shapes, [0, 1], [[1], [0]], ("ones",), bad=0.0)
        for step in (1, 2, 4):
            out = fr.fuse(*case, 0.5, step, 10.0)
            assert not any(nm.any() for nm in out.view_normals) and not out.normals.any()
    # no view at all
    out = fr.fuse([(3, 3)], [], [], [], [], [], [], [], 0.01, 2, 0.05)
    assert out.pt_ptr.tolist() == [0] and out.points.shape == (0, 3) and out.index.shape == (0, 3)


# ------------------------------------------------------------------------------------------- what the rule is worth
_QUALITY = {}


def scene_maps(seed):
    """The default scene with the given texture seed, every view a reference with the other two as sources, planes per view
    from plane_depths with that view's own warps, radius 2: (scene, views, the sweep's maps).  Built once per seed."""
    from sfm_amd import depth as dm
    if seed not in _QUALITY:
        s = dr.default_scene() if seed == 0 else dr.make_scene(seed=seed)
        refs, sources = all_to_all(3)
        warps = [dm.view_warps(s.K, s.poses, r, src) for r, src in zip(refs, sources)]
        backproj = [dm.view_backprojection(s.K, s.poses, r) for r in refs]
        planes = [dm.plane_depths(s.d_min, s.d_max, W, s.size) for W in warps]
        _QUALITY[seed] = (s, (refs, sources, warps, backproj, planes), dr.sweep(s.images, refs, sources, warps, planes, 2))
    return _QUALITY[seed]


def fusion_quality(seed, min_consistent, step=2, jump=0.05):
    """(kept pixels, fused points, median and p95 z error per view, the same fused, share of the fused points with a normal,
    median and p90 angle to the true normal in degrees) at rel_tol 0.02, mean cost <= 12.  The z error is the distance to the
    nearer of the two true planes; the true normal of both looks down -z at the cameras."""
    s, (refs, sources, warps, backproj, planes), maps = scene_maps(seed)
    limit = [12 * len(src) * 25 for src in sources]
    f = dr.filter_views(s.images, refs, sources, warps, backproj, maps, 0.02, limit, min_consistent)
    shapes = [a.shape for a in s.images]
    out = fr.fuse(shapes, refs, sources, warps, backproj, [m[2] for m in maps], [v[1] for v in f], [v[2] for v in f], 0.02, step, jump)
    zerr = lambda z: np.minimum(np.abs(z - s.z_front), np.abs(z - s.z_back))
    per_view = zerr(np.concatenate([v[2][v[1] != 0][:, 2] for v in f]))
    fused = zerr(out.points[:, 2])
    has = out.normals.any(axis=1)
    angle = np.degrees(np.arccos(np.clip(-out.normals[has][:, 2].astype(np.float64), -1, 1)))
    return (len(per_view), len(fused), np.median(per_view), np.percentile(per_view, 95), np.median(fused), np.percentile(fused, 95),
            has.mean(), np.median(angle), np.percentile(angle, 90))


MEASURED = {1: (0.385, 0.969), 2: (0.336, 0.957)}             # seed 0: fused share of the kept pixels, share with a normal


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_quality_on_the_default_scene(seed):
    """Measured with this restatement on the default scene (96 x 72, 3 cameras, every view a reference with the other two
    as sources, planes per view from plane_depths, radius 2, rel_tol 0.02, mean cost <= 12, step 2, jump 0.05), seed 0:
    min_consistent = 1: 15,655 kept pixels -> 6,030 fused points (38.5 %), median / p95 z error 0.0086 / 0.0506 per view ->
    0.0036 / 0.0278 fused, 96.9 % of the fused points with a normal, 1.2 / 8.3 degrees median / p90 to the true normal;
    min_consistent = 2: 11,047 -> 3,711 (33.6 %), 0.0081 / 0.0185 -> 0.0018 / 0.0071, 95.7 %, 0.8 / 4.0 degrees.
    Seeds 1 and 2: see README ("Fusion").  Asserted for all three seeds: the shares less two percentage points, the fused
    share at most 0.45, the fused median z error below the per-view one, a median angle of at most 2 degrees."""
    for mc in (1, 2):
        kept, fused, med_v, p95_v, med_f, p95_f, with_normal, ang_med, ang_p90 = fusion_quality(seed, mc)
        print(f"seed {seed} mc={mc}: kept {kept} fused {fused} ({fused / kept:.4f})  z per view {med_v:.4f} / {p95_v:.4f} -> fused "
              f"{med_f:.4f} / {p95_f:.4f}  with normal {with_normal:.4f}  angle {ang_med:.2f} / {ang_p90:.2f}")
        share, normal_share = MEASURED[mc]
        assert fused / kept <= 0.45 and fused / kept <= share + 0.02
        assert with_normal >= normal_share - 0.02
        assert med_f < med_v
        assert ang_med <= 2.0


# ------------------------------------------------------------------------------------------- argument checks, no device
def test_argument_checks_without_gpu():
    import sfm_amd
    from sfm_amd import depth as dm
    assert sfm_amd.FusedCloud is dm.FusedCloud
    maps = dm.DepthMaps({"refs": [0], "imgs": [np.zeros((2, 2), np.uint8)], "radius": 2, "src_ptr": np.array([0, 0])})
    with pytest.raises(ValueError, match="filter"):
        maps.fuse()
    maps.keep, maps._rel_tol = [np.ones((2, 2), np.uint8)], 0.01          # as after filter(): the checks come before the device
    for kw in (dict(normal_step=0), dict(normal_step=5), dict(normal_step=1.5), dict(normal_jump=-0.1), dict(normal_jump=float("nan")),
               dict(normal_jump="x"), dict(rel_tol=-1.0), dict(rel_tol=float("nan"))):
        with pytest.raises(ValueError):
            maps.fuse(**kw)
    import inspect
    sig = inspect.signature(dm.dense_from_reconstruction)
    assert sig.parameters["fuse"].default is False
    assert [p.default for p in list(inspect.signature(dm.DepthMaps.fuse).parameters.values())[1:]] == [None, 2, 0.05]


def test_c_entry_points_reject_bad_calls_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    need, plain = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.sfm_depth_workspace_bytes(3, 2, 4, ctypes.byref(plain)) == 0
    assert lib.sfm_depth_fuse_workspace_bytes(3, 2, 4, 1000, ctypes.byref(need)) == 0
    assert need.value >= plain.value + (1000 // 256 + 2) * 4 + 8         # the filter's tables, a count per block, a chunk base
    small = need.value
    assert lib.sfm_depth_fuse_workspace_bytes(36, 36, 144, 36 * 1024 * 768, ctypes.byref(need)) == 0 and need.value > small + 110000 * 4
    assert lib.sfm_depth_fuse_workspace_bytes(0, 0, 0, 0, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.sfm_depth_fuse_workspace_bytes(3, 2, 4, 1000, None) != 0
    for bad in ((-1, 0, 0, 0), (3, 4, 0, 10), (3, 2, 17, 10), (3, 2, 4, -1), (3, -1, 0, 10)):
        assert lib.sfm_depth_fuse_workspace_bytes(*bad, ctypes.byref(need)) != 0, bad
    assert lib.sfm_depth_fuse_mark(None, None, None, None, 0, 0, None, None, None, None, None, None, None, None, 0.01, 2, 0.05,
                                   None, None, None, None, None, 0) != 0
    assert lib.sfm_depth_fuse_gather(None, None, None, None, 0, 0, None, None, None, None, None, None, None, None, None, None, 0,
                                     None, None, None, None, None, 0) != 0


def test_ply_with_normals(tmp_path):
    """With normals a vertex is 6 floats (+ 3 bytes of colour); without them the file is what it was: the header and the
    body are written out here as the format had them before normals existed."""
    from sfm_amd.interchange import save_ply_points
    pts = np.arange(12.0).reshape(4, 3)
    nrm = np.array([[0, 0, -1.0], [1, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=np.float32)
    col = np.arange(12, dtype=np.uint8).reshape(4, 3)
    old_head = b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
    path = tmp_path / "cloud.ply"
    save_ply_points(pts, None, path)
    assert open(path, "rb").read() == old_head + b"end_header\n" + pts.astype("<f4").tobytes()
    save_ply_points(pts, col, path)
    body = b"".join(pts[k].astype("<f4").tobytes() + bytes(col[k, ::-1]) for k in range(4))
    assert open(path, "rb").read() == old_head + b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" + body
    save_ply_points(pts, None, path, normals=nrm)
    head, body = open(path, "rb").read().split(b"end_header\n")
    assert head == old_head + b"property float nx\nproperty float ny\nproperty float nz\n"
    assert np.array_equal(np.frombuffer(body, "<f4").reshape(4, 6), np.hstack([pts, nrm]).astype(np.float32))
    save_ply_points(pts, col, path, normals=nrm)
    head, body = open(path, "rb").read().split(b"end_header\n")
    assert head.endswith(b"property float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n") and len(body) == 4 * 27
    assert np.frombuffer(body[:24], "<f4").tolist() == [0, 1, 2, 0, 0, -1] and body[24:27] == bytes([2, 1, 0])
    with pytest.raises(ValueError):
        save_ply_points(pts, None, path, normals=nrm[:3])
