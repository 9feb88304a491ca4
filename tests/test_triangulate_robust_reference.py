"""CPU checks of the robust triangulation: the NumPy restatement (tests/triangulate_robust_reference.py) against a second
one written in plain per-track loops on LAPACK's SVD, tri::pair_of exhaustively, the outlier scene the feature was
measured on, and the host build of sfm_amd/csrc/triangulate_robust.h (address and undefined-behaviour sanitizers on)
against the restatement, bit for bit."""
import functools
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import triangulate_reference as tr
import triangulate_robust_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATES = dict(min_views=2, refine_iters=5, max_error=4.0, min_angle_deg=1.0)
EDGE_OPTIONS = (dict(), dict(min_views=4), dict(min_angle_deg=0.0), dict(refine_iters=0))


@functools.lru_cache(maxsize=None)
def outlier_reference():
    args, moved = rr.outlier_scene()
    return args, moved, rr.triangulate_robust(*args, **GATES), tr.triangulate(*args, **GATES)


@functools.lru_cache(maxsize=None)
def edge_reference(k):
    args, names, moved = rr.edge_scene()
    opts = dict(rr.EDGE_GATES, **EDGE_OPTIONS[k])
    return args, names, moved, opts, rr.triangulate_robust(*args, **opts), tr.triangulate(*args, **opts)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------------------------ a second restatement, in loops
def _errs(P, X, xy):
    h = P.reshape(3, 4) @ np.append(X, 1.0)
    with np.errstate(all="ignore"):
        return h[2], float(np.hypot(h[0] / h[2] - xy[0], h[1] / h[2] - xy[1]))


def _dlt(Ps, xys):
    A = np.concatenate([[x * P[8:12] - P[0:4], y * P[8:12] - P[4:8]] for P, (x, y) in zip(Ps, xys)])
    return np.linalg.svd(A)[2][-1]


def _wide(Cs, X, cos_min):
    d = [X - c for c in Cs]
    return any(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)) <= cos_min for a, b in itertools.combinations(d, 2))


def loops_solve(Ps, Cs, xys, min_views, refine_iters, max_error, min_angle_deg):
    """(status, X) of one track by the plain rule: SVD for the linear stage, Gauss-Newton by np.linalg.solve."""
    if len(Ps) < min_views:
        return tr.TOO_FEW_VIEWS, None
    if not all(np.isfinite(P).all() and np.isfinite(c).all() and np.isfinite(q).all() for P, c, q in zip(Ps, Cs, xys)):
        return tr.DEGENERATE, None
    v = _dlt(Ps, xys)
    if v[3] == 0 or not np.isfinite(v[:3] / v[3]).all():
        return tr.DEGENERATE, None
    Xl = v[:3] / v[3]

    def residual(X):
        h = np.stack([P.reshape(3, 4) @ np.append(X, 1.0) for P in Ps])
        return (h[:, :2] / h[:, 2:3] - np.asarray(xys)).ravel(), h

    X = Xl
    for _ in range(refine_iters):
        r, h = residual(X)
        J = []
        for P, hk in zip(Ps, h):
            M = P.reshape(3, 4)[:, :3]
            J += [(M[0] - hk[0] / hk[2] * M[2]) / hk[2], (M[1] - hk[1] / hk[2] * M[2]) / hk[2]]
        J = np.asarray(J)
        try:
            Xn = X - np.linalg.solve(J.T @ J, J.T @ r)
        except np.linalg.LinAlgError:
            break
        if not np.isfinite(Xn).all():
            break
        X = Xn
    if refine_iters > 0 and (residual(X)[0] ** 2).sum() > (residual(Xl)[0] ** 2).sum():
        X = Xl
    es = [_errs(P, X, q) for P, q in zip(Ps, xys)]
    if any(w <= 0 for w, _ in es):
        return tr.BEHIND, X
    if min_angle_deg > 0 and not _wide(Cs, X, np.cos(np.deg2rad(min_angle_deg))):
        return tr.LOW_ANGLE, X
    return (tr.HIGH_ERROR if any(e > max_error for _, e in es) else tr.OK), X


def loops_robust(proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp, min_views=2, refine_iters=5, max_error=4.0,
                 min_angle_deg=0.0):
    """The integer outputs of the robust rule, track by track."""
    proj = np.asarray(proj, dtype=np.float64).reshape(-1, 12)
    centres = tr.camera_centres(proj)
    T = len(track_ptr) - 1
    out = {"status": np.zeros(T, np.int32), "n_views": np.zeros(T, np.int32), "n_inliers": np.zeros(T, np.int32),
           "obs_inlier": np.zeros(len(obs_image), np.uint8), "scores": np.zeros((T, 64), np.int32), "winner": np.full(T, -1, np.int32)}
    for t in range(T):
        o = [k for k in range(track_ptr[t], track_ptr[t + 1]) if cam_of_image[obs_image[k]] >= 0]
        Ps = [proj[cam_of_image[obs_image[k]]] for k in o]
        Cs = [centres[cam_of_image[obs_image[k]]] for k in o]
        xys = [kp_xy[kp_ptr[obs_image[k]] + obs_kp[k]] for k in o]
        out["n_views"][t] = len(o)
        st, _ = loops_solve(Ps, Cs, xys, min_views, refine_iters, max_error, min_angle_deg)
        out["status"][t] = st
        if st == tr.OK:
            out["obs_inlier"][o] = 1
            out["n_inliers"][t] = len(o)
            continue
        snd = [i for i in range(len(o)) if np.isfinite(Ps[i]).all() and np.isfinite(Cs[i]).all() and np.isfinite(xys[i]).all()]
        if len(snd) < 4:
            continue

        def agreeing(X):
            es = [_errs(Ps[i], X, xys[i]) for i in snd]
            return [i for i, (w, e) in zip(snd, es) if w > 0 and e <= max_error]

        pairs = list(itertools.combinations(snd, 2))
        M = len(pairs)
        if M > 64:
            pairs = [pairs[(h * M) // 64] for h in range(64)]
        best, Xw = 0, None
        for h, (a, b) in enumerate(pairs):
            v = _dlt([Ps[a], Ps[b]], [xys[a], xys[b]])
            with np.errstate(all="ignore"):
                Xh = v[:3] / v[3]
            if v[3] == 0 or not np.isfinite(Xh).all() or _errs(Ps[a], Xh, xys[a])[0] <= 0 or _errs(Ps[b], Xh, xys[b])[0] <= 0:
                continue
            if min_angle_deg > 0 and not _wide([Cs[a], Cs[b]], Xh, np.cos(np.deg2rad(min_angle_deg))):
                continue
            score = len(agreeing(Xh))
            out["scores"][t, h] = score
            if score > best:
                best, Xw, win = score, Xh, h
        if best < max(min_views, 3):
            continue
        S = agreeing(Xw)
        st2, Xr = loops_solve([Ps[i] for i in S], [Cs[i] for i in S], [xys[i] for i in S], max(min_views, 3), refine_iters,
                              max_error, min_angle_deg)
        if st2 != tr.OK:
            continue
        fin = agreeing(Xr)
        out["status"][t], out["winner"][t], out["n_inliers"][t] = tr.OK, win, len(fin)
        out["obs_inlier"][[o[i] for i in fin]] = 1
    out["counts"] = np.bincount(out["status"], minlength=6).astype(np.int64)
    return out


def test_restatement_equals_per_track_loops():
    """Integer outputs equal, on the outlier scene and on every edge case.  The two share no linear algebra (Jacobi and
    Givens against LAPACK); the margins printed are what keeps their decisions the same."""
    args, _, ref, _ = outlier_reference()
    cases = [("outlier scene", args, GATES, ref)]
    for k in range(len(EDGE_OPTIONS)):
        e = edge_reference(k)
        cases.append((f"edge cases {EDGE_OPTIONS[k]}", e[0], e[3], e[4]))
    for what, a, opts, r in cases:
        loops = loops_robust(*a, **opts)
        print(f"{what}: margin {r['margin']:.3g} px, counts {r['counts'].tolist()}, reach the hypotheses {int(r['reached'].sum())}")
        assert r["margin"] > 1e-6
        for k in ("status", "n_views", "n_inliers", "obs_inlier", "counts", "scores", "winner"):
            assert np.array_equal(r[k], loops[k]), (what, k, np.flatnonzero((r[k] != loops[k]).reshape(len(r[k]), -1).any(axis=1))[:5])


def test_pair_of_enumerates_or_strides():
    for s in range(2, 41):
        M = s * (s - 1) // 2
        every = list(itertools.combinations(range(s), 2))
        got = [rr.pair_of(h, s) for h in range(rr.hypotheses(s))]
        assert all((a, b) == every[p] for p, a, b in got)                      # the pair number names the pair
        if M <= 64:
            assert [p for p, _, _ in got] == list(range(M))                    # every pair once
        else:
            numbers = [p for p, _, _ in got]
            assert len(numbers) == 64 and all(x < y for x, y in zip(numbers, numbers[1:])) and numbers[-1] < M
            assert numbers == [(h * M) // 64 for h in range(64)]
    assert rr.hypotheses(11) == 55 and rr.hypotheses(12) == 64 and rr.hypotheses(3) == 3


def test_outlier_scene_is_rescued_with_the_clean_observations():
    args, moved, ref, plain = outlier_reference()
    track_ptr, used = args[4], args[1][args[5]] >= 0
    print("plain rule:", plain["counts"].tolist(), "robust rule:", ref["counts"].tolist(), "margin", ref["margin"])
    assert plain["counts"].tolist() == [201, 6, 0, 0, 0, 193]
    rescued = np.flatnonzero((plain["status"] != tr.OK) & (ref["status"] == tr.OK))
    assert len(rescued) == 164 and (plain["status"][rescued] == tr.HIGH_ERROR).all()
    for t in rescued:
        o = slice(track_ptr[t], track_ptr[t + 1])
        assert np.array_equal(ref["obs_inlier"][o] != 0, used[o] & ~moved[o]), t
        assert ref["n_inliers"][t] == (used[o] & ~moved[o]).sum() and ref["n_views"][t] == used[o].sum()
    still = np.flatnonzero(ref["status"] > tr.TOO_FEW_VIEWS)
    assert len(still) == 29
    for t in still:
        o = slice(track_ptr[t], track_ptr[t + 1])
        assert used[o].sum() < 4 or (used[o] & ~moved[o]).sum() < 3, t
        assert not ref["obs_inlier"][o].any() and ref["n_inliers"][t] == 0
    # a track the plain rule accepts is returned as it is
    ok = plain["status"] == tr.OK
    assert same_bits(ref["X"][ok], plain["X"][ok]) and same_bits(ref["max_err"][ok], plain["max_err"][ok])
    assert np.array_equal(ref["n_inliers"][ok], plain["n_views"][ok])
    assert same_bits(ref["X"][still], plain["X"][still]) and np.array_equal(ref["status"][still], plain["status"][still])
    # the condition under which the integer outputs can be demanded exactly of the device; not a tolerance
    assert ref["margin"] > 1e-6
    # and the 80-bit run takes the same decisions
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        ld = rr.triangulate_robust(*args, dtype=np.longdouble, **GATES)
        for k in ("status", "n_inliers", "obs_inlier", "scores", "winner"):
            assert np.array_equal(ref[k], ld[k]), k


def test_classify_repeats_the_robust_rule():
    """At the X of the robust rule with the same cameras and gates: OK, the same flags, n_inliers and max_err bits."""
    args, _, ref, _ = outlier_reference()
    ok = ref["status"] == tr.OK
    c = rr.classify(*args, np.where(ok[:, None], ref["X"], 0.0), ok, min_views=2, max_error=4.0, min_angle_deg=1.0)
    assert (c["status"][ok] == tr.OK).all() and (c["status"][~ok] == rr.NO_POINT).all() and c["counts"].tolist() == [ok.sum(), 0, 0, 0, 0, 0]
    assert np.array_equal(c["obs_inlier"], ref["obs_inlier"]) and np.array_equal(c["n_inliers"][ok], ref["n_inliers"][ok])
    assert same_bits(c["max_err"][ok], ref["max_err"][ok]) and np.isnan(c["max_err"][~ok]).all()
    bad = rr.classify(*args, np.full((400, 3), np.inf), np.ones(400), min_views=2, max_error=4.0, min_angle_deg=1.0)
    assert (bad["status"] == tr.TOO_FEW_VIEWS).all() and not bad["obs_inlier"].any()      # a non-finite X lands here


# ------------------------------------------------------------------------------------- the header built for the host
@functools.lru_cache(maxsize=None)
def native(tmp):
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(tmp, "triangulate_robust_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "triangulate_robust_check.cpp"), "-o", exe], check=True)

    def run(mode, records):
        np.ascontiguousarray(records, dtype=np.float64).tofile(exe + ".in")
        subprocess.run([exe, mode, exe + ".in", exe + ".out"], check=True)
        return np.fromfile(exe + ".out")
    return run


def records(args, head):
    """The input of the stand-alone program: per track head(t), then 15 numbers per observation."""
    proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = args
    rec = []
    for t in range(len(track_ptr) - 1):
        o = np.arange(track_ptr[t], track_ptr[t + 1])
        rec.append(np.asarray([len(o)] + list(head(t)), dtype=np.float64))
        for k in o:
            cam = cam_of_image[obs_image[k]]
            used = cam >= 0
            rec.append(np.concatenate([[float(used)], proj[cam if used else 0], kp_xy[kp_ptr[obs_image[k]] + obs_kp[k]]]))
    return np.concatenate(rec)


def split(out, track_ptr, width):
    """Per-track records of `width` numbers followed by one flag per observation -> ([T,width], flags [n_obs])."""
    rows, flags, at = [], [], 0
    for n in np.diff(track_ptr):
        rows.append(out[at:at + width]); flags.append(out[at + width:at + width + n])
        at += width + n
    assert at == len(out)
    return np.asarray(rows), np.concatenate(flags).astype(np.uint8)


def native_robust(run, args, min_views=2, refine_iters=5, max_error=4.0, min_angle_deg=0.0):
    head = [min_views, refine_iters, max_error, float(min_angle_deg > 0), np.cos(min_angle_deg * (np.pi / 180.0))]
    rows, flags = split(run("robust", records(args, lambda t: head)), args[4], 7)
    return {"status": rows[:, 0].astype(np.int32), "n_views": rows[:, 1].astype(np.int32), "n_inliers": rows[:, 2].astype(np.int32),
            "X": rows[:, 3:6], "max_err": rows[:, 6], "obs_inlier": flags}


def native_classify(run, args, X, min_views=2, max_error=4.0, min_angle_deg=0.0):
    head = [min_views, 0, max_error, float(min_angle_deg > 0), np.cos(min_angle_deg * (np.pi / 180.0))]
    rows, flags = split(run("classify", records(args, lambda t: head + list(X[t]))), args[4], 3)
    return {"status": rows[:, 0].astype(np.int32), "n_inliers": rows[:, 1].astype(np.int32), "max_err": rows[:, 2], "obs_inlier": flags}


def assert_native_robust(run, args, opts, ref, what):
    out = native_robust(run, args, **opts)
    for k in ("status", "n_views", "n_inliers", "obs_inlier"):
        assert np.array_equal(out[k], ref[k]), (what, k, np.flatnonzero(out[k] != ref[k])[:5])
    assert same_bits(out["X"], ref["X"]), (what, "X")
    assert same_bits(out["max_err"], ref["max_err"]), (what, "max_err")
    return out


def test_host_build_equals_the_restatement_bit_for_bit(tmp_path_factory):
    """tri::solve_robust and tri::classify under the address and undefined-behaviour sanitizers, on the outlier scene and
    on the edge cases under each set of options: every output equals the float64 restatement's, bit for bit."""
    run = native(str(tmp_path_factory.mktemp("native")))
    if run is None:
        pytest.skip("no g++")
    args, _, ref, _ = outlier_reference()
    assert_native_robust(run, args, GATES, ref, "outlier scene")
    cases = [(args, GATES, ref)]
    for k in range(len(EDGE_OPTIONS)):
        e = edge_reference(k)
        out = assert_native_robust(run, e[0], e[3], e[4], f"edge cases {EDGE_OPTIONS[k]}")
        cases.append((e[0], e[3], e[4]))
        if k == 0:
            st = {name: int(out["status"][t]) for t, name in e[1].items()}
            print(st)
            assert st["3 views, one moved"] == tr.HIGH_ERROR and st["4 views, moved two by two"] == tr.HIGH_ERROR
            assert st["all pixels NaN"] == tr.DEGENERATE and sum(v == tr.OK for v in st.values()) == 9
    rng = np.random.default_rng(7)
    for a, opts, r in cases:
        cg = {k: v for k, v in opts.items() if k != "refine_iters"}
        ok = r["status"] == tr.OK
        X = np.where(ok[:, None], r["X"], 0.5)
        for what, Xc in (("the robust rule's points", X), ("perturbed points", X + rng.normal(0, 0.01, X.shape))):
            c = rr.classify(*a, Xc, np.ones(len(X)), **cg)
            out = native_classify(run, a, Xc, **cg)
            assert c["margin"] > 1e-6, (what, c["margin"])
            for k in ("status", "n_inliers", "obs_inlier"):
                assert np.array_equal(out[k], c[k]), (what, k)
            assert same_bits(out["max_err"], c["max_err"]), what
        c = native_classify(run, a, X, **cg)                                   # the contract between the two calls
        assert (c["status"][ok] == tr.OK).all() and np.array_equal(c["n_inliers"][ok], r["n_inliers"][ok])
        trk = np.repeat(np.arange(len(X)), np.diff(a[4]))
        assert np.array_equal(c["obs_inlier"][ok[trk]], r["obs_inlier"][ok[trk]]) and same_bits(c["max_err"][ok], r["max_err"][ok])


def test_host_build_pair_of(tmp_path_factory):
    run = native(str(tmp_path_factory.mktemp("native")))
    if run is None:
        pytest.skip("no g++")
    sizes = list(range(2, 41)) + [1000, 46341]
    out = run("pairs", np.asarray(sizes, dtype=np.float64)).reshape(len(sizes), 1 + 3 * 64)
    for s, row in zip(sizes, out):
        n = rr.hypotheses(s)
        assert row[0] == n
        want = [rr.pair_of(h, s) if h < n else (-1, -1, -1) for h in range(64)]
        assert row[1:].reshape(64, 3).astype(np.int64).tolist() == [list(w) for w in want], s
