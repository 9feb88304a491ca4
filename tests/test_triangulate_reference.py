"""CPU checks of the N-view triangulation: the NumPy restatement (tests/triangulate_reference.py) against LAPACK's SVD and
SciPy's least squares, and the host build of sfm_amd/csrc/triangulate_solve.h against the restatement."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import triangulate_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_dev_points(X, ref):
    """Largest ||X - ref|| / ||ref|| over the rows where ref is finite; the NaN rows must be the same."""
    X, ref = np.asarray(X, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    dead = np.isnan(ref).any(axis=1)
    assert np.array_equal(np.isnan(X).any(axis=1), dead)
    if dead.all():
        return 0.0
    d = np.sqrt(((X - ref)[~dead] ** 2).sum(axis=1)) / np.sqrt((ref[~dead] ** 2).sum(axis=1))
    return float(d.max())


def rel_dev_scalars(a, ref):
    a, ref = np.asarray(a, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    dead = np.isnan(ref)
    assert np.array_equal(np.isnan(a), dead)
    if dead.all():
        return 0.0
    return float((np.abs(a - ref)[~dead] / np.abs(ref[~dead])).max())


def flat(proj, g, registered=None):
    """The argument list of tr.triangulate from (kp_ptr, kp_xy, track_ptr, obs_image, obs_kp): camera = image."""
    n_img = len(g[0]) - 1
    cam = np.arange(n_img, dtype=np.int32) if registered is None else np.asarray(registered, dtype=np.int32)
    return (np.asarray(proj).reshape(-1, 12), cam) + tuple(g)


@functools.lru_cache(maxsize=None)
def scene(n_tracks=300, n_cams=40, lo=2, hi=40, seed=0):
    """Random tracks of lo..hi views over n_cams cameras on an arc around the unit cube, pixel noise 0.5."""
    rng = np.random.default_rng(seed)
    proj = tr.arc_cameras(n_cams)[0]
    X = rng.uniform(0, 1, (n_tracks, 3))
    lengths = rng.integers(lo, hi + 1, n_tracks)
    lengths[:20] = 2
    return proj, X, tr.make_tracks(rng, proj, X, lengths, noise=0.5)


def test_linear_stage_equals_svd():
    """The Givens factor's null vector is the last right singular vector of the stacked rows.  The rows are in pixels, so
    their condition number is about 1e4 and a null vector is good to about 1e-12; 1e-8 leaves four orders.  (The sharper
    statement is tests/test_geometry_truth.py: the linear point within 99.6 kappa 2^-53 of the eigenvector in mpmath.)"""
    proj, _, g = scene()
    args = flat(proj, g)
    ref = tr.triangulate(*args, refine_iters=0)
    P, C, xy, mask, n_views = tr.gather(*args)
    worst = 0.0
    for t in range(len(n_views)):
        rows = tr.dlt_rows(P[t, :n_views[t]], xy[t, :n_views[t]]).reshape(-1, 4)
        v = np.linalg.svd(rows)[2][-1]
        X = v[:3] / v[3]
        worst = max(worst, np.linalg.norm(ref["linear"][t] - X) / np.linalg.norm(X))
    print("largest relative distance between the Givens / Jacobi linear stage and LAPACK's SVD:", worst)
    assert (ref["status"] == tr.OK).all() and worst < 1e-8


def test_refined_point_equals_least_squares():
    """Five Gauss-Newton steps from the linear point reach the minimiser SciPy finds on the same residual (to 1e-7: SciPy
    differentiates numerically and stops at its own tolerances; tests/test_geometry_truth.py holds the point to
    2.2 kappa 2^-53 of the stationary point in mpmath)."""
    optimize = pytest.importorskip("scipy.optimize")
    proj, _, g = scene()
    args = flat(proj, g)
    ref = tr.triangulate(*args, refine_iters=5)
    P, C, xy, mask, n_views = tr.gather(*args)
    worst = 0.0
    for t in range(0, len(n_views), 5):
        Pt, uv = P[t, :n_views[t]].reshape(-1, 3, 4), xy[t, :n_views[t]]

        def residual(X):
            h = Pt @ np.append(X, 1.0)
            return (h[:, :2] / h[:, 2:3] - uv).ravel()
        sol = optimize.least_squares(residual, ref["linear"][t], method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
        worst = max(worst, np.linalg.norm(ref["X"][t] - sol.x) / np.linalg.norm(sol.x))
        assert 0.5 * (residual(ref["X"][t]) ** 2).sum() <= sol.cost * (1 + 1e-9)
    print("largest relative distance between the refined point and scipy.optimize.least_squares:", worst)
    assert worst < 1e-7


def test_float64_and_80_bit_runs_agree():
    """With the fixed iteration count the float64 run follows the 80-bit one to round-off, for both settings the GPU test uses."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 here")
    proj, _, g = scene()
    for iters in (0, 5):
        a = tr.triangulate(*flat(proj, g), refine_iters=iters)
        b = tr.triangulate(*flat(proj, g), refine_iters=iters, dtype=np.longdouble)
        assert np.array_equal(a["status"], b["status"])
        dx, de = rel_dev_points(a["X"], b["X"]), rel_dev_scalars(a["max_err"], b["max_err"])
        print(f"refine_iters={iters}: float64 against 80-bit, X {dx:.3g}, max_err {de:.3g}")
        assert dx < 1e-9 and de < 1e-9


# ------------------------------------------------------------------------------------------------ constructed statuses
def status_cases():
    """One track per status code, min_views=2, max_error=4, min_angle_deg=1: (proj, cam_of_image, arrays..., expected)."""
    proj, _, _, centres = tr.arc_cameras(12)
    target = np.array([0.5, 0.5, 0.5])
    mid = centres[5:7].mean(axis=0)
    pts = {"ok": target, "few": target, "nan": target, "behind": target + 2.0 * (mid - target),
           "far": target - 2000.0 * (mid - target) / np.linalg.norm(mid - target), "err": target}
    views = {"ok": [0, 5, 11], "few": [0, 12, 13], "nan": [2, 6, 9], "behind": [3, 5, 7, 8], "far": [5, 6], "err": [1, 6, 10]}
    cam_of_image = np.concatenate([np.arange(12), [-1, -1]]).astype(np.int32)
    counts = np.zeros(14, np.int64)
    obs_image, obs_kp, xy = [], [], [[] for _ in range(14)]
    for name in ("ok", "few", "nan", "behind", "far", "err"):
        for k, img in enumerate(views[name]):
            cam = img if img < 12 else 0
            px = tr.project_points(proj[cam:cam + 1], pts[name][None])[0, 0]
            if name == "nan" and k == 1:
                px = np.array([np.nan, px[1]])
            if name == "err" and k == 2:
                px = px + [0.0, 50.0]
            obs_image.append(img); obs_kp.append(len(xy[img])); xy[img].append(px)
    lens = [len(views[n]) for n in ("ok", "few", "nan", "behind", "far", "err")]
    kp_ptr = np.concatenate([[0], np.cumsum([len(x) for x in xy])]).astype(np.int64)
    kp_xy = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1, 2) for x in xy])
    track_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return (proj.reshape(-1, 12), cam_of_image, kp_ptr, kp_xy, track_ptr, np.asarray(obs_image, np.int32),
            np.asarray(obs_kp, np.int32)), np.arange(6, dtype=np.int32), np.array([3, 1, 3, 4, 2, 3], np.int32)


def test_reference_status_codes():
    args, want, views = status_cases()
    for iters in (0, 5):
        r = tr.triangulate(*args, refine_iters=iters, min_angle_deg=1.0)
        assert np.array_equal(r["status"], want) and np.array_equal(r["n_views"], views)
        assert r["counts"].tolist() == [1] * 6
        assert np.isnan(r["X"][[1, 2]]).all() and np.isnan(r["max_err"][[1, 2]]).all()
        assert np.isfinite(r["X"][[0, 3, 4, 5]]).all() and np.isfinite(r["max_err"][[0, 3, 4, 5]]).all()
    # without the angle gate the far point passes
    assert tr.triangulate(*args, min_angle_deg=0.0)["status"].tolist() == [0, 1, 2, 3, 0, 5]


# ------------------------------------------------------------------------------------- the header built for the host
@functools.lru_cache(maxsize=None)
def native(tmp):
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(tmp, "triangulate_solve_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "triangulate_solve_check.cpp"), "-o", exe], check=True)

    def run(mode, records, width):
        np.ascontiguousarray(records, dtype=np.float64).tofile(exe + ".in")
        subprocess.run([exe, mode, exe + ".in", exe + ".out"], check=True)
        return np.fromfile(exe + ".out").reshape(-1, width)
    return run


def native_solve(run, args, min_views=2, refine_iters=5, max_error=4.0, min_angle_deg=0.0):
    proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = args
    cos_min = np.cos(min_angle_deg * (np.pi / 180.0))
    rec = []
    for t in range(len(track_ptr) - 1):
        o = np.arange(track_ptr[t], track_ptr[t + 1])
        rec.append([len(o), min_views, refine_iters, max_error, float(min_angle_deg > 0), cos_min])
        for k in o:
            cam = cam_of_image[obs_image[k]]
            used = cam >= 0
            rec.append(np.concatenate([[float(used)], proj[cam if used else 0], kp_xy[kp_ptr[obs_image[k]] + obs_kp[k]]]))
    out = run("solve", np.concatenate([np.asarray(r, dtype=np.float64).ravel() for r in rec]), 6)
    return {"status": out[:, 0].astype(np.int32), "n_views": out[:, 1].astype(np.int32), "X": out[:, 2:5], "max_err": out[:, 5]}


def test_host_build_equals_the_reference(tmp_path_factory):
    """Random tracks of 2 to 40 views.  The host build runs the reference's operations in the reference's order; it is
    allowed 100 times the distance between the float64 and the 80-bit run of the reference, as the device is."""
    run = native(str(tmp_path_factory.mktemp("native")))
    if run is None:
        pytest.skip("no g++")
    proj, _, g = scene()
    args = flat(proj, g)
    for iters in (0, 5):
        ref = tr.triangulate(*args, refine_iters=iters, min_angle_deg=1.0)
        ld = tr.triangulate(*args, refine_iters=iters, min_angle_deg=1.0, dtype=np.longdouble)
        out = native_solve(run, args, refine_iters=iters, min_angle_deg=1.0)
        assert np.array_equal(out["status"], ref["status"]) and np.array_equal(out["n_views"], ref["n_views"])
        assert sorted(set(ref["n_views"].tolist()))[0] == 2 and ref["n_views"].max() >= 38
        tol_x, tol_e = 100 * rel_dev_points(ref["X"], ld["X"]), 100 * rel_dev_scalars(ref["max_err"], ld["max_err"])
        dx, de = rel_dev_points(out["X"], ref["X"]), rel_dev_scalars(out["max_err"], ref["max_err"])
        print(f"refine_iters={iters}: host build against the reference, X {dx:.3g} (allowed {tol_x:.3g}), "
              f"max_err {de:.3g} (allowed {tol_e:.3g})")
        assert dx <= tol_x and de <= tol_e
    centres = run("centre", args[0], 3)
    assert np.abs(centres - tr.camera_centres(args[0])).max() <= 1e-12 * 6.0
    assert np.abs(centres - tr.arc_cameras(40)[3]).max() < 1e-9


def test_host_build_two_view_tracks_are_dlt2(tmp_path_factory):
    run = native(str(tmp_path_factory.mktemp("native")))
    if run is None:
        pytest.skip("no g++")
    proj, _, g = scene()
    args = flat(proj, g)
    out = native_solve(run, args, refine_iters=0)
    P, C, xy, mask, n_views = tr.gather(*args)
    two = np.flatnonzero(n_views == 2)
    assert len(two) >= 20
    rec = np.concatenate([P[two, 0], P[two, 1], xy[two, 0], xy[two, 1]], axis=1)
    X = run("dlt2", rec, 3)
    assert np.array_equal(out["X"][two], X)
    # an unregistered image between the two used ones changes nothing
    proj12 = tr.arc_cameras(12)[0]
    rng = np.random.default_rng(5)
    g3 = tr.make_tracks(rng, proj12, rng.uniform(0, 1, (30, 3)), np.full(30, 3), noise=0.5)
    reg = np.arange(12, dtype=np.int32)
    a = native_solve(run, flat(proj12, g3), refine_iters=0)
    mid = g3[3][1::3]                                   # the middle image of every track
    for t in range(30):
        reg1 = reg.copy()
        reg1[mid[t]] = -1
        b = native_solve(run, flat(proj12, g3, reg1), refine_iters=0)
        Pt, _, xyt, _, nv = tr.gather(*flat(proj12, g3, reg1))
        assert nv[t] == 2 and a["n_views"][t] == 3
        want = run("dlt2", np.concatenate([Pt[t, 0], Pt[t, 1], xyt[t, 0], xyt[t, 1]])[None], 3)
        assert np.array_equal(b["X"][t], want[0])


def test_host_build_status_codes(tmp_path_factory):
    run = native(str(tmp_path_factory.mktemp("native")))
    if run is None:
        pytest.skip("no g++")
    args, want, views = status_cases()
    for iters in (0, 5):
        out = native_solve(run, args, refine_iters=iters, min_angle_deg=1.0)
        ref = tr.triangulate(*args, refine_iters=iters, min_angle_deg=1.0)
        assert np.array_equal(out["status"], want) and np.array_equal(out["n_views"], views)
        assert np.array_equal(np.isnan(out["X"]), np.isnan(ref["X"])) and np.array_equal(np.isnan(out["max_err"]), np.isnan(ref["max_err"]))
        live = [0, 3, 4, 5]
        assert np.allclose(out["X"][live], ref["X"][live], rtol=1e-6, atol=0)
    # degenerate geometry: the same camera twice with the same pixel, parallel rays; never OK under the angle gate, no fault
    proj = args[0]
    px = tr.project_points(proj[:1].reshape(1, 3, 4), np.array([[0.5, 0.5, 0.5]]))[0, 0]
    P1 = proj[0].reshape(3, 4).copy()
    P1[:, 3] += tr.K_SFM @ [1.0, 0.0, 0.0]                        # same rotation, shifted centre: same pixel = parallel rays
    projd = np.stack([proj[0], P1.ravel()])
    cases = (projd, np.array([0, 0, 0, 1], np.int32), np.array([0, 1, 2, 3, 4], np.int64), np.tile(px, (4, 1)),
             np.array([0, 2, 4], np.int64), np.array([0, 1, 2, 3], np.int32), np.zeros(4, np.int32))
    for iters in (0, 5):
        out = native_solve(run, cases, refine_iters=iters, min_angle_deg=1.0)
        assert (out["status"] != tr.OK).all(), out
