"""CPU tests of the geometry after the minimal solvers against the multi-precision truth of tests/geometry_truth.py: the
truth against itself, the caps on what the judge leaves out, the NumPy restatements (triangulate_reference,
pose_reference) at 1 x C_REF with C_REF re-measured, the host builds of triangulate_solve.h, triangulate_robust.h and
pose_solve.h (tests/native/*_check.cpp by g++ -ffp-contract=off and by -ffp-contract=fast -mfma) at 8 x C_REF, and ten
seeded defects that the judge must reject.  No GPU."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import geometry_truth as gt
import pose_reference as pr
import solver_truth as st
import triangulate_reference as tr
from geometry_truth import mpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"off": ("-ffp-contract=off",), "fast": ("-ffp-contract=fast", "-mfma")}
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


def scene_tracks(name):
    return np.flatnonzero(gt.flat()[7] == [sc.name for sc in gt.scenes()].index(name))


def show(what, worst):
    print(f"{what}: worst error / (kappa 2^-53) " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------ the truth against itself
def test_truth_residuals_and_time():
    """The linear stage's eigen residual and the gradient at the stationary point are below 1e-40, the poses' defining
    relations too; all truths with their condition numbers in about a minute of CPU."""
    tracks, centres, secs = gt.truth()
    poses, psecs = gt.pose_truths()
    live = [t for t in tracks if t is not None]
    res = max(float(t.residual) for t in live)
    grad = max(float(t.gradient) for t in live if t.refined is not None)
    pres = max(float(p.residual) for p in poses if not p.none)
    print(f"{len(live)} tracks, {len(centres)} cameras in {secs:.1f} CPU seconds, {len(poses)} essential matrices in {psecs:.1f}; "
          f"eigen residual {res:.1e}, gradient {grad:.1e}, pose relations {pres:.1e}")
    assert res < 1e-40 and grad < 1e-40 and pres < 1e-40
    assert not any(p.none for p in poses)
    assert secs + psecs < 90.0


def test_the_stationary_point_beats_its_neighbours():
    """The cost at 26 neighbours (the directions of a 3 x 3 x 3 cube, 1e-12 of the point's distance to the cameras) is
    larger than at the stationary point, for every fifth track."""
    tracks = gt.truth()[0]
    dirs = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
    n = 0
    for T in tracks[::5]:
        if T is None or T.refined is None:
            continue
        p = T.refined
        h = p.scale_mp * mpf("1e-12")
        for d in dirs:
            assert gt._derivatives(T.obs, [x + h * e for x, e in zip(p.X_mp, d)])[0] > p.cost_mp
        n += 1
    assert n >= 100


def test_exact_cases_reproduce_their_construction():
    """The exact scene's points are integers and its pixels exact floats: the linear and the refined truth are the
    construction to 1e-50 (relative to the distance to the cameras)."""
    tracks = gt.truth()[0]
    sc = next(s for s in gt.scenes() if s.exact)
    worst = mpf(0)
    for i, X in zip(scene_tracks(sc.name), sc.X):
        T = tracks[i]
        assert T.refined is not None
        for p in (T.linear, T.refined):
            worst = max(worst, st._norm([a - mpf(float(b)) for a, b in zip(p.X_mp, X)]) / p.scale_mp)
    print(f"exact scene: the truth lies {float(worst):.1e} from the construction")
    assert worst < mpf("1e-50")


def test_two_view_truth_is_the_n_view_truth_on_two_views():
    """The two-view contract (four rows, the null vector) is the N-view problem with n = 2: the eigenvector of the
    smallest eigenvalue of the 4 x 4 A^T A annihilates A when A is square and singular, and otherwise is the right
    singular vector of its smallest singular value, found here by another route: the null vector of A^T A - lambda I
    with lambda from the characteristic polynomial's smallest root."""
    tracks = gt.truth()[0]
    sc = next(s for s in gt.scenes() if s.name == "two views")
    worst = mpf(0)
    for i in scene_tracks(sc.name)[::6]:
        T = tracks[i]
        G = gt._ata(T.obs)
        lam = min(MPre for MPre in [gt.MP.re(r) for r in gt.MP.polyroots(_charpoly(G), maxsteps=500, extraprec=500)])
        M = [[G[r][c] - (lam if r == c else 0) for c in range(4)] for r in range(4)]
        v = [x[0] for x in gt._solve([M[r][:3] for r in range(3)], [[-M[r][3]] for r in range(3)])]
        worst = max(worst, st._norm([a - b for a, b in zip(v, T.linear.X_mp)]) / T.linear.scale_mp)
    print(f"two views: the two routes differ by {float(worst):.1e}")
    assert worst < mpf("1e-30")


def _charpoly(G):
    """Descending coefficients of det(lambda I - G), 4 x 4, by Faddeev-LeVerrier."""
    n = 4
    I = [[mpf(int(r == c)) for c in range(n)] for r in range(n)]
    M, coef = I, [mpf(1)]
    for k in range(1, n + 1):
        GM = [[gt._dot(G[r], [M[q][c] for q in range(n)]) for c in range(n)] for r in range(n)]
        ck = -sum(GM[r][r] for r in range(n)) / k
        coef.append(ck)
        M = [[GM[r][c] + ck * I[r][c] for c in range(n)] for r in range(n)]
    return coef


def test_left_out_caps():
    """Left out (the bound at 8 x C_REF passes 1e-6) plus undetermined: at most 2 % per scene and quantity outside the
    degenerate scene; centres and poses: none."""
    caps = gt.caps()
    for name, c in caps.items():
        print(f"{name}: " + ", ".join(f"{k} {v:.1%}" for k, v in c.items()))
    bad = [(n, k, v) for n, c in caps.items() for k, v in c.items() if v > 0.02]
    assert not bad, bad
    assert not any(gt.left_out(k, gt.C_REF["centre"]) for _, k in gt.truth()[1])
    assert not any(gt.left_out(k, gt.C_REF["pose"]) for p in gt.pose_truths()[0] for k in p.kappa)


# ------------------------------------------------------------------------------------------- the references
@functools.lru_cache(maxsize=None)
def reference(iters):
    return tr.triangulate(*gt.flat_args(), refine_iters=iters, min_angle_deg=1.0)


def reference_poses():
    out = []
    for _, E in gt.essentials():
        d = pr.decompose(E)
        out.append(np.stack([np.c_[R, t].ravel() for R, t in d]))
    return out


def check_all(X0, e0, X30, e30, centres, poses, mult, what):
    """Every quantity of one implementation under mult x C_REF; returns the worst ratios."""
    fails, worst = [], {}
    f, wx, we0 = gt.judge_tracks(X0, e0, "linear", mult, what)
    fails += f
    worst["linear"] = max(wx.values())
    show(f"{what}, linear X", wx)
    f, wx, we = gt.judge_tracks(X30, e30, "refined", mult, what)
    fails += f
    worst["refined"] = max(wx.values())
    worst["max_err"] = max(list(we.values()) + list(we0.values()))
    show(f"{what}, refined X", wx)
    show(f"{what}, max_err at the linear point", we0)
    show(f"{what}, max_err at the refined point", we)
    if centres is not None:
        f, worst["centre"] = gt.judge_centres(centres, mult, what)
        fails += f
    if poses is not None:
        worst["pose"] = 0.0
        for (name, _), c, T in zip(gt.essentials(), poses, gt.pose_truths()[0]):
            f, r = gt.judge_poses(c, T, mult * gt.C_REF["pose"])
            fails += [f"{what}, {name}: {x}" for x in f]
            worst["pose"] = max([worst["pose"]] + r)
    print(f"{what}: worst ratios " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f"; bounds {mult:g} x "
          + ", ".join(f"{k} {v:g}" for k, v in gt.C_REF.items()))
    assert not fails, "\n".join(fails[:20])
    return worst


def test_references_pass_at_c_ref():
    r0, r30 = reference(0), reference(30)
    check_all(r0["X"], r0["max_err"], r30["X"], r30["max_err"], tr.camera_centres(gt.flat_args()[0]), reference_poses(), 1.0,
              "NumPy reference")


def test_references_define_c():
    """C re-measured per quantity - the worst error / (kappa 2^-53) of the float64 restatements over the cases that C
    leaves in - is not above the stored C_REF and not below half of it."""
    tracks, centres, _ = gt.truth()
    scene_of = gt.flat()[7]
    r0, r30 = reference(0), reference(30)
    pairs = {q: [] for q in gt.QUANTITIES}
    C = tr.camera_centres(gt.flat_args()[0])
    for i, (c, k) in enumerate(centres):
        pairs["centre"].append((k, gt.ratio_points(C[i], _as_point(c, 1.0, float(np.sqrt((c * c).sum())))) * gt.U53))
    for i, T in enumerate(tracks):
        if T is None:
            continue
        exact = gt.scenes()[scene_of[i]].exact
        pairs["linear"].append((T.linear.kappa, gt.ratio_points(r0["X"][i], T.linear) * T.linear.kappa * gt.U53))
        for p, r in ((T.linear, r0), (T.refined, r30)):
            if p is not None:
                unit = 1.0 if exact else p.max_err
                pairs["max_err"].append((p.k_max_err / unit, gt.ratio_max_err(r["max_err"][i], p) * p.k_max_err / unit * gt.U53))
        if T.refined is not None:
            pairs["refined"].append((T.refined.kappa, gt.ratio_points(r30["X"][i], T.refined) * T.refined.kappa * gt.U53))
    for c, T in zip(reference_poses(), gt.pose_truths()[0]):
        d = gt.pose_distances(c, T)
        pairs["pose"] += [(T.kappa[k], d[:, k].min()) for k in range(4)]
    for q in gt.QUANTITIES:
        ok = [(k, e) for k, e in pairs[q] if np.isfinite(e) and k > 0]
        got = gt.measure_c(ok)
        print(f"{q}: C measured {got:.4g} over {len(ok)} cases, stored {gt.C_REF[q]:.4g}")
        assert got <= gt.C_REF[q] <= 2 * got, q


def _as_point(X, kappa, scale):
    p = gt.Point()
    p.X, p.kappa, p.scale = X, kappa, scale
    return p


def test_reference_status_follows_the_band_rule():
    """The references' statuses (max_error 4, min_angle 1 degree) are those the truth's gate quantities give, with at
    most 2 % of the tracks inside the band; the degenerate scene ends in a status and never in a non-finite X with OK."""
    for iters, kind in ((0, "linear"), (30, "refined")):
        r = reference(iters)
        fails, band = gt.judge_status(r["status"], kind, f"reference, refine_iters={iters}", max_error=4.0, min_angle_deg=1.0)
        print(f"refine_iters={iters}: {band:.2%} of the tracks lie in the band; statuses {np.bincount(r['status'], minlength=6).tolist()}")
        assert not fails, "\n".join(fails[:10])
        assert band <= 0.02
        check_degenerate(r)


def check_degenerate(out):
    idx = np.concatenate([scene_tracks(sc.name) for sc in gt.scenes() if sc.degenerate])
    assert np.isin(out["status"][idx], np.arange(6)).all()
    ok = out["status"][idx] == tr.OK
    assert np.isfinite(out["X"][idx][ok]).all()


# ------------------------------------------------------------------------------------------ the host builds
@pytest.fixture(scope="module")
def native_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("geometry_truth_native"))


def build_native(tmp, program, mode):
    exe = os.path.join(tmp, f"{program}_{mode}")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-std=c++17", "-O2", *MODES[mode], "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "native", f"{program}.cpp"), "-o", exe],
                       check=True)
    return exe


def _run(exe, what, data):
    path = f"{exe}.{what}"
    np.ascontiguousarray(data, np.float64).tofile(path + ".in")
    subprocess.run([exe, what.split(".")[0], path + ".in", path + ".out"], check=True)
    return np.fromfile(path + ".out")


def track_records(iters, min_angle_deg=1.0, max_error=4.0):
    """The stdin records of the `solve` and `robust` modes for every track of flat()."""
    proj, _, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = gt.flat_args()
    node = kp_ptr[obs_image] + obs_kp
    obs = np.concatenate([np.ones((len(obs_image), 1)), proj[obs_image], kp_xy[node]], axis=1)
    rec = []
    for t in range(len(track_ptr) - 1):
        rec.append([track_ptr[t + 1] - track_ptr[t], 2, iters, max_error, float(min_angle_deg > 0), np.cos(np.deg2rad(min_angle_deg))])
        rec.append(obs[track_ptr[t]:track_ptr[t + 1]].ravel())
    return np.concatenate([np.asarray(r, np.float64) for r in rec])


@functools.lru_cache(maxsize=None)
def host(tmp, mode):
    """What the three check programs give for flat() and essentials() - computed once per build, never modified."""
    solve, robust, pose = (build_native(tmp, p, mode) for p in ("triangulate_solve_check", "triangulate_robust_check", "pose_solve_check"))
    out = {}
    for iters in (0, 5, 30):
        o = _run(solve, f"solve.{iters}", track_records(iters)).reshape(-1, 6)
        out[iters] = {"status": o[:, 0].astype(np.int32), "n_views": o[:, 1].astype(np.int32), "X": o[:, 2:5], "max_err": o[:, 5]}
    out["centres"] = _run(solve, "centre", gt.flat_args()[0]).reshape(-1, 3)
    o = _run(robust, "robust.30", track_records(30))
    nv = gt.n_views()
    at = np.concatenate([[0], np.cumsum(7 + nv)])[:-1]
    out["robust"] = {"status": o[at].astype(np.int32), "n_inliers": o[at + 2].astype(np.int32), "X": np.stack([o[at + 3], o[at + 4], o[at + 5]], 1),
                     "max_err": o[at + 6]}
    idx = scene_tracks("two views")
    proj, _, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = gt.flat_args()
    a, b = track_ptr[idx], track_ptr[idx] + 1
    node = kp_ptr[obs_image] + obs_kp
    out["dlt2"] = _run(solve, "dlt2", np.concatenate([proj[obs_image[a]], proj[obs_image[b]], kp_xy[node[a]], kp_xy[node[b]]], axis=1)).reshape(-1, 3)
    o = _run(pose, "essential", np.stack([E.ravel() for _, E in gt.essentials()])).reshape(-1, 49)
    assert (o[:, 0] == 1).all()
    out["poses"] = o[:, 1:].reshape(-1, 4, 12)
    return out


@needs_gxx
@pytest.mark.parametrize("mode", list(MODES))
def test_host_builds_of_the_headers(native_dir, mode):
    """tri::solve at 0 and 30 steps, tri::camera_centre, jacobi::dlt2, tri::solve_robust on clean tracks and
    jacobi::decompose_essential, without and with contraction to fma, at 8 x C_REF; statuses by the band rule."""
    h = host(native_dir, mode)
    what = f"host build, -ffp-contract={mode}"
    check_all(h[0]["X"], h[0]["max_err"], h[30]["X"], h[30]["max_err"], h["centres"], h["poses"], gt.MARGIN, what)
    for iters, kind in ((0, "linear"), (30, "refined")):
        fails, _ = gt.judge_status(h[iters]["status"], kind, what, max_error=4.0, min_angle_deg=1.0)
        assert not fails, "\n".join(fails[:10])
        check_degenerate(h[iters])
    # the two-view tracks are jacobi::dlt2, bit for bit, and dlt2 is held to the two-view truth with them
    idx = scene_tracks("two views")
    assert np.array_equal(h["dlt2"], h[0]["X"][idx])
    # the robust entry on tracks that need no rescue: the plain call's bounds
    r = h["robust"]
    clean = (r["status"] == tr.OK) & (r["n_inliers"] == gt.n_views())
    live = np.array([T is not None for T in gt.truth()[0]])
    assert (clean | (h[30]["status"] != tr.OK))[live].all() and clean.sum() >= 500
    X, e = np.where(clean[:, None], r["X"], h[30]["X"]), np.where(clean, r["max_err"], h[30]["max_err"])
    fails, wx, we = gt.judge_tracks(X, e, "refined", gt.MARGIN, what + ", robust")
    show(what + ", robust, refined X", wx)
    assert not fails, "\n".join(fails[:20])


@needs_gxx
@pytest.mark.parametrize("mode", list(MODES))
def test_host_five_steps(native_dir, mode):
    """The shipped default of 5 steps: judged as the refined point where the scene says so, measured elsewhere; its cost
    lies between the stationary cost and the linear truth's, each to the bound on the cost."""
    h = host(native_dir, mode)
    five_steps(h[5]["X"], h[5]["max_err"], f"host build, -ffp-contract={mode}")


def five_steps(X, max_err, what):
    judged = [sc.name for sc in gt.scenes() if sc.five == "judge" and not sc.degenerate]
    fails, wx, we = gt.judge_tracks(X, max_err, "refined", gt.MARGIN, what + ", 5 steps", only=judged)
    show(what + ", 5 steps, refined X", wx)
    measured = [sc.name for sc in gt.scenes() if sc.five == "measure"]
    _, wm, _ = gt.judge_tracks(X, None, "refined", np.inf, what, only=measured)
    print(f"{what}, 5 steps, distance to the stationary point in units of the bound {gt.MARGIN:g} x C_REF: "
          + ", ".join(f"{k} {v / (gt.MARGIN * gt.C_REF['refined']):.3g}" for k, v in wm.items()))
    tracks = gt.truth()[0]
    C = gt.MARGIN * gt.C_COST * gt.C_REF["max_err"]
    worst = 0.0
    for i, T in enumerate(tracks):
        if T is None or T.refined is None:
            continue
        cost = gt.cost_at(T, X[i])
        hi = T.linear.cost_mp + mpf(C * T.linear.k_cost * gt.U53)
        lo = T.refined.cost_mp - mpf(C * T.refined.k_cost * gt.U53)
        if not gt.left_out(T.linear.k_cost, gt.C_COST * gt.C_REF["max_err"], max(T.linear.cost, 1e-300)) and cost > hi:
            fails.append(f"{what}, track {i}: cost: the 5-step point costs {float(cost):.17g}, the linear truth {T.linear.cost:.17g}")
        if cost < lo:
            fails.append(f"{what}, track {i}: cost: the 5-step point costs {float(cost):.17g}, the stationary point {T.refined.cost:.17g}")
        if T.linear.k_cost > 0:
            worst = max(worst, float((cost - T.linear.cost_mp) / mpf(T.linear.k_cost * gt.U53)))
    print(f"{what}, 5 steps: cost above the linear truth's, worst {worst:.3g} x kappa 2^-53 against the bound {C:g}")
    assert not fails, "\n".join(fails[:20])
    return wm


# ------------------------------------------------------------------------------------------ seeded defects
def null4_variant(U, sweeps=30, second_within=None):
    """A copy of the reference's Hestenes iteration on [T,4,4] with two seeded defects: the number of sweeps, and the
    second-smallest column taken when the two smallest squared norms are within `second_within` of the largest."""
    U = U.copy()
    T = len(U)
    V = np.tile(np.eye(4), (T, 1, 1))
    eps = 10 * np.finfo(np.float64).eps
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(3):
                for q in range(p + 1, 4):
                    a, b, g = (U[:, :, p] ** 2).sum(1), (U[:, :, q] ** 2).sum(1), (U[:, :, p] * U[:, :, q]).sum(1)
                    rot = np.abs(g) > eps * np.sqrt(a * b)
                    zeta = (b - a) / (2 * g)
                    tt = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1 + zeta * zeta))
                    c = np.where(rot, 1 / np.sqrt(1 + tt * tt), 1.0)
                    s = np.where(rot, c * tt, 0.0)
                    for M in (U, V):
                        mp_, mq = M[:, :, p].copy(), M[:, :, q].copy()
                        M[:, :, p], M[:, :, q] = c[:, None] * mp_ - s[:, None] * mq, s[:, None] * mp_ + c[:, None] * mq
    nk = (U * U).sum(1)
    order = np.argsort(nk, axis=1, kind="stable")
    best = order[:, 0].copy()
    if second_within is not None:
        close = nk[np.arange(T), order[:, 1]] - nk[np.arange(T), order[:, 0]] <= second_within * nk.max(1)
        best[close] = order[close, 1]
    v = V[np.arange(T), :, best]
    return v[:, :3] / v[:, 3:4]


def two_view_rows(dtype=np.float64, swap=False):
    proj, _, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = gt.flat_args()
    idx = scene_tracks("two views")
    a, b = track_ptr[idx], track_ptr[idx] + 1
    node = kp_ptr[obs_image] + obs_kp
    P = np.stack([proj[obs_image[a]], proj[obs_image[b]]], 1).astype(dtype)
    xy = np.stack([kp_xy[node[b if swap else a]], kp_xy[node[a if swap else b]]], 1).astype(dtype)
    return tr.dlt_rows(P, xy).reshape(len(idx), 4, 4).astype(np.float64)


def test_seeded_defects_are_rejected():
    """Ten defects, each in a copy of the reference or in a device-shaped output; the judge rejects every one and names
    the quantity.  The first five would pass every restatement-parity tolerance of test_triangulate_reference.py
    (test_host_build_equals_the_reference, the centres' 1e-12) and test_triangulate_gpu.py (assert_parity: 100 x the
    float64-vs-80-bit deviation of the same algorithm): those set the header against a restatement written operation for
    operation, which carries the same cofactor sign, sweep count, argmin, row type and step count in float64 and in
    80 bits alike."""
    r0, r30 = reference(0), reference(30)
    idx2 = scene_tracks("two views")
    rejected = {}

    def with_rows(name, X2, quantity="linear X"):
        X = r0["X"].copy()
        X[idx2] = X2
        fails, _, _ = gt.judge_tracks(X, None, "linear", gt.MARGIN, name, only=["two views"])
        rejected[name] = [f for f in fails if quantity in f]

    # the copy is the reference: unchanged it passes
    X = r0["X"].copy()
    X[idx2] = null4_variant(two_view_rows())
    assert not gt.judge_tracks(X, None, "linear", gt.MARGIN, "copy", only=["two views"])[0]

    C = tr.camera_centres(gt.flat_args()[0])
    C[:, 0] *= 1 - 2e-9                                        # a term of relative size 1e-9 with its sign flipped
    rejected["1 centre: a cofactor term of relative size 1e-9 with the wrong sign"] = gt.judge_centres(C, gt.MARGIN, "defect")[0]
    with_rows("2 Jacobi stopped after one sweep", null4_variant(two_view_rows(), sweeps=1))
    with_rows("3 argmin takes the second-smallest column when the two are within 1e-3 of the largest",
              null4_variant(two_view_rows(), second_within=1e-3))
    with_rows("4 DLT rows in float32", null4_variant(two_view_rows(np.float32)))
    narrow = ["arc of 0.04 rad", "arc of 0.01 rad"]
    r1 = tr.triangulate(*gt.flat_args(), refine_iters=1)
    rejected["5 refinement stopped after 1 step on the narrow scenes"] = \
        [f for f in gt.judge_tracks(r1["X"], None, "refined", gt.MARGIN, "defect", only=narrow)[0] if "refined X" in f]
    rejected["6 the fallback to the linear point never taken"] = no_fallback_failures()
    rejected["7 max_err from the linear point"] = \
        [f for f in gt.judge_tracks(r30["X"], r0["max_err"], "refined", gt.MARGIN, "defect", only=["baseline"])[0] if "max_err" in f]
    with_rows("8 dlt2 fed the observations swapped with P unswapped", null4_variant(two_view_rows(swap=True)))
    one_column, t_from_v = [], []
    for (name, E), T in zip(gt.essentials(), gt.pose_truths()[0]):
        U, S, Vt = np.linalg.svd(E)
        if np.linalg.det(U) < 0:
            U[:, 0] = -U[:, 0]                                 # one column where the whole matrix is negated
        if np.linalg.det(Vt) < 0:
            Vt = -Vt
        R1, R2 = U @ pr.W @ Vt, U @ pr.W.T @ Vt
        pack = lambda t: np.stack([np.c_[R, s * t].ravel() for s in (1, -1) for R in (R1, R2)])
        one_column += gt.judge_poses(pack(U[:, 2]), T, gt.MARGIN * gt.C_REF["pose"])[0]
        U2 = -U if np.linalg.det(np.linalg.svd(E)[0]) < 0 else np.linalg.svd(E)[0]
        R1, R2 = U2 @ pr.W @ Vt, U2 @ pr.W.T @ Vt
        t_from_v += gt.judge_poses(pack(Vt[2]), T, gt.MARGIN * gt.C_REF["pose"])[0]
    rejected["9 a U of determinant -1 negated in one column only"] = one_column
    rejected["10 t taken from V"] = t_from_v
    for name, fails in rejected.items():
        print(f"{name}: {fails[0] if fails else 'NOT REJECTED'}")
    assert len(rejected) == 10 and all(rejected.values())


def no_fallback_failures():
    """Tracks of the baseline scene with one observation moved by up to 2000 px: five Gauss-Newton steps from the linear
    point can end above the linear point's cost (about 6 % of such tracks), which the header answers by keeping the
    linear point.  Without that the 5-step point fails the cost bound (cost no more than the linear truth's)."""
    sc = gt.scenes()[0]
    rng = np.random.default_rng(gt.SEED + 60)
    fails = []
    for rep in range(10):
        for k, (c, xy) in enumerate(sc.tracks):
            xy = xy.copy()
            xy[int(rng.integers(0, len(c)))] += rng.uniform(-2000.0, 2000.0, 2)
            args = gt._flat(sc.proj, [c], [xy])
            P, _, uv, mask, nv = tr.gather(*args)
            v = tr.linear_stage(P, uv, mask, nv)
            Xl = v[:, :3] / v[:, 3:4]
            Xr, cost_lin = tr.refine(P, uv, mask, Xl, 5)
            if not tr.evaluate(P, uv, mask, Xr, 4.0)[0][0] > 1.001 * cost_lin[0]:
                continue                                       # the fallback is not taken here: with or without it the same
            assert np.array_equal(tr.triangulate(*args, refine_iters=5)["X"], Xl)
            T = gt.track_truth({int(q): sc.proj[q] for q in set(c.tolist())}, c.tolist(), xy)
            bound = gt.MARGIN * gt.C_COST * gt.C_REF["max_err"] * T.linear.k_cost * gt.U53
            assert gt.cost_at(T, Xl[0]) <= T.linear.cost_mp + mpf(bound)         # with the fallback the bound holds
            if gt.cost_at(T, Xr[0]) > T.linear.cost_mp + mpf(bound):
                fails.append(f"baseline track {k} with a moved observation: cost: without the fallback the 5-step point costs "
                             f"{float(gt.cost_at(T, Xr[0])):.6g}, the linear truth {T.linear.cost:.6g}")
            if len(fails) >= 2:
                return fails
    return fails
