"""CPU tests of the relative-pose reference (tests/pose_reference.py) against the reference's own shipped run, of the
kernel's Jacobi routines built for the host (sfm_amd/csrc/pose_solve.h) against LAPACK, and of the argument checks of
sfm_amd.pose that need no device.  No GPU."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import pose_reference as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = pr.K_REF


@functools.lru_cache(maxsize=None)
def shipped_pairs():
    """[(name, F, pts1, pts2, mask)] of the 148 shipped pairs (all matched points; mask = the verified inliers)."""
    bp = np.load(os.path.join(GOLDEN, "bunny_pairs.npz"), allow_pickle=False)
    off = bp["offsets"]
    return [(str(n), bp["F"][i], bp["pts1"][off[i]:off[i + 1]], bp["pts2"][off[i]:off[i + 1]],
             bp["mask"][off[i]:off[i + 1]]) for i, n in enumerate(bp["names"])]


@functools.lru_cache(maxsize=None)
def shipped_reference():
    """{name: (recover_pose on the inliers only, recover_pose on all points)} - computed once, never modified."""
    out = {}
    for name, F, p1, p2, m in shipped_pairs():
        E = pr.essential_from_fundamental(F, K)
        out[name] = (pr.recover_pose(E, p1[m], p2[m], K), pr.recover_pose(E, p1, p2, K))
    return out


def state():
    return np.load(os.path.join(GOLDEN, "bunny_state.npz"), allow_pickle=False)


# ------------------------------------------------------------------------------------------------ the shipped run
def test_initial_pair_of_the_shipped_run():
    """pair_25_26 on its 229 verified inliers: counts {229,0,0,0}, the winner is camera 26 of the shipped state and the
    pixel-space triangulation gives the first 229 shipped points (float32 values: cv2 returns the input's type)."""
    s = state()
    assert [int(i) for i in s["ids"][:2]] == [25, 26]
    name, F, p1, p2, m = next(p for p in shipped_pairs() if p[0] == "pair_25_26")
    r = shipped_reference()[name][0]
    assert sorted(r["counts"].tolist()) == [0, 0, 0, 229] and r["n_good"] == 229 and r["status"] == 0
    assert (r["mask"] == 255).all() and r["mask"].dtype == np.uint8
    d = pr.pose_distance((r["R"], r["t"]), (s["R"][1], s["t"][1]))
    X = pr.triangulate_pixels(K, r["R"], r["t"], p1[m], p2[m])
    dx = np.abs(X - s["pts"][:229]).max()
    print(f"pose distance to the shipped camera 26: {d:.3g}; points: {dx:.3g}")
    assert d < 1e-12
    assert dx < 1e-6
    assert np.array_equal(s["pts"][:229], s["pts"][:229].astype(np.float32).astype(np.float64))


def test_best_pair_of_the_148_shipped_pairs():
    ref = shipped_reference()
    for which, (best, second) in enumerate([((229, "pair_25_26"), (220, "pair_12_35")),
                                            ((235, "pair_25_26"), (230, "pair_12_35"))]):
        rank = sorted(((r[which]["n_good"], n) for n, r in ref.items()), key=lambda a: -a[0])
        assert rank[0] == best and rank[1] == second, rank[:3]
    margins = [min(np.sort(r[w]["counts"])[-1] - np.sort(r[w]["counts"])[-2] for r in ref.values()) for w in (0, 1)]
    print("smallest best-minus-second margin over the 148 pairs: inliers only", margins[0], ", all points", margins[1])
    assert margins[0] >= 4 and margins[1] >= 1                # no pair has a tie between its candidates


def test_shipped_decisions_are_far_from_the_thresholds():
    """A condition on the inputs of the GPU parity test, which compares every one of the 10,907 x 4 decisions exactly:
    no depth of any candidate lies within 1e-6 (relative) of 0 or of 50."""
    worst = np.inf
    for name, F, p1, p2, m in shipped_pairs():
        poses = shipped_reference()[name][1]["poses"]
        x1, x2 = pr.normalise(p1, K), pr.normalise(p2, K)
        for R, t in poses:
            _, z1, z2 = pr.vote(R, t, x1, x2, 50.0, with_depths=True)
            for z in (z1, z2):
                worst = min(worst, np.abs(z).min(), np.abs(z / 50.0 - 1).min())
    print("closest relative approach of a depth to 0 or 50:", worst)
    assert worst > 1e-6


# ---------------------------------------------------------------------------------------------- synthetic pairs
def test_noise_free_pairs_recover_the_true_pose():
    rng = np.random.default_rng(0)
    worst = 0.0
    for M in (5, 40, 300):
        for _ in range(8):
            E, p1, p2, R, t, _ = pr.synth_pair(rng, M)
            # pixels rounded to float32 would move E's pose by 1e-8: the vote takes them, the pose is E's alone
            r = pr.recover_pose(E, p1, p2, K)
            assert r["status"] == 0 and r["n_good"] == M and (r["mask"] == 255).all()
            assert sorted(r["counts"].tolist())[-2] < M
            worst = max(worst, pr.pose_distance((r["R"], r["t"]), (R, t)))
    print("largest distance of the winner from the true pose:", worst)
    assert worst < 1e-12


def test_thresholds_mask_and_degenerate_input():
    rng = np.random.default_rng(3)
    E, p1, p2, R, t, X = pr.synth_pair(rng, 50, depth=(59.0, 61.0))
    assert pr.recover_pose(E, p1, p2, K, dist=50.0)["n_good"] == 0
    assert pr.recover_pose(E, p1, p2, K, dist=100.0)["n_good"] == 50
    E, p1, p2, R, t, X = pr.synth_pair(rng, 50)
    m = np.ones(50, np.uint8)
    m[::5] = 0
    r = pr.recover_pose(E, p1, p2, K, mask=m)
    assert r["n_good"] == 40 and not r["mask"][::5].any() and (r["mask"][m != 0] == 255).all()
    assert pr.recover_pose(np.zeros((3, 3)), p1, p2, K)["status"] == 2
    assert pr.recover_pose(np.full((3, 3), np.nan), p1, p2, K)["status"] == 2
    # rank 1 with two columns exactly zero, so that the second singular value is exactly 0 (a general rank-1 matrix
    # has one of rounding size, which is > 0 and gets a model, as from cv2)
    assert pr.recover_pose(np.outer([1.0, 2, 2], [2.0, 0, 0]), p1, p2, K)["status"] == 2
    assert pr.recover_pose(E, p1[:0], p2[:0], K)["status"] == 1
    bad = p1.copy()
    bad[3] = [np.nan, 1.0]
    bad[4] = [np.inf, 1.0]
    r = pr.recover_pose(E, bad, p2, K)
    assert r["n_good"] == 48 and not r["mask"][[3, 4]].any()
    assert pr.recover_pose(E, p1, p1, K)["status"] == 0      # no parallax: a model, whatever it counts


# ------------------------------------------------------------------ the kernel's Jacobi routines built for the host
@functools.lru_cache(maxsize=None)
def native(tmp):
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(tmp, "pose_solve_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "pose_solve_check.cpp"), "-o", exe], check=True)

    def run(mode, records, width):
        np.ascontiguousarray(records, dtype=np.float64).tofile(exe + ".in")
        subprocess.run([exe, mode, exe + ".in", exe + ".out"], check=True)
        return np.fromfile(exe + ".out").reshape(-1, width)
    return run


def essential_cases():
    """The 148 shipped K^T F K and 300 random exact essential matrices (S0 = S1) at scales from 1e-3 to 1e3."""
    rng = np.random.default_rng(7)
    Es = [pr.essential_from_fundamental(F, K) for _, F, _, _, _ in shipped_pairs()]
    for k in range(300):
        E = pr.synth_pair(rng, 1)[0]
        Es.append(E * 10.0 ** rng.uniform(-3, 3) * (-1.0) ** k)
    return Es


def test_host_build_of_the_decomposition_equals_lapack(tmp_path_factory):
    run = native(str(tmp_path_factory.mktemp("native")))
    if run is None:
        pytest.skip("no g++")
    Es = essential_cases()
    out = run("essential", np.stack(Es).reshape(-1, 9), 49)
    assert (out[:, 0] == 1.0).all()
    worst = 0.0
    for E, o in zip(Es, out):
        Rt = o[1:].reshape(4, 3, 4)
        poses = [(Rt[c][:, :3], Rt[c][:, 3]) for c in range(4)]
        for R, t in poses:
            assert abs(np.linalg.det(R) - 1) < 1e-12 and abs(np.linalg.norm(t) - 1) < 1e-12
        assert np.array_equal(poses[0][0], poses[2][0]) and np.array_equal(poses[0][1], -poses[2][1])
        _, d = pr.match_candidates(poses, pr.decompose(E))
        worst = max(worst, d)
    print("largest distance between a host-built candidate and LAPACK's nearest:", worst)
    assert worst < 1e-12
    bad = np.stack([np.zeros(9), np.full(9, np.nan), np.outer([1.0, 2, 2], [2.0, 0, 0]).ravel(),
                    np.r_[np.inf, np.ones(8)]])
    assert (run("essential", bad, 49) == 0.0).all()           # no model: the flag is 0 and Rt is left alone


def test_host_build_of_the_dlt_null_vector_equals_lapack(tmp_path_factory):
    run = native(str(tmp_path_factory.mktemp("native")))
    if run is None:
        pytest.skip("no g++")
    A = []
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    for name in ("pair_25_26", "pair_24_25", "pair_12_35"):            # normalised and pixel-space systems
        _, F, p1, p2, m = next(p for p in shipped_pairs() if p[0] == name)
        r = shipped_reference()[name][1]
        for (R, t) in r["poses"]:
            P1 = np.hstack([R, t.reshape(3, 1)])
            for Pa, Pb, a, b in ((P0, P1, pr.normalise(p1, K), pr.normalise(p2, K)),
                                 (K @ P0, K @ P1, p1.astype(np.float64), p2.astype(np.float64))):
                A.append(np.stack([a[:, :1] * Pa[2] - Pa[0], a[:, 1:] * Pa[2] - Pa[1],
                                   b[:, :1] * Pb[2] - Pb[0], b[:, 1:] * Pb[2] - Pb[1]], axis=1))
    A = np.concatenate(A)
    v = run("null4", A.reshape(-1, 16), 4)
    ref = np.linalg.svd(A)[2][:, 3]
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    d = np.minimum(np.abs(v - ref).max(axis=1), np.abs(v + ref).max(axis=1))
    print(f"{len(A)} systems; largest distance of the unit null vector from LAPACK's (up to sign): {d.max():.3g}")
    assert d.max() < 1e-9


# ------------------------------------------------------------------------------ the Python glue without a device
def test_argument_checks_and_empty_batches_need_no_device():
    from sfm_amd import pose
    import sfm_amd
    assert sfm_amd.recover_pose_batched is pose.recover_pose_batched and sfm_amd.recover_pose is pose.recover_pose
    assert pose.recover_pose_batched([], [], [], K) == []
    assert pose.recover_pose_batched([], [], [], K, return_debug=True) == ([], [])
    e = np.zeros((0, 2), np.float32)
    res, dbg = pose.recover_pose_batched([np.eye(3)] * 2, [e, e], [e, e], K, return_debug=True)
    assert res == [(0, None, None, None)] * 2 and [d["status"] for d in dbg] == [1, 1]
    assert pose.recover_pose_batched([np.eye(3)], [e], [e], K, triangulate=True) == [(0, None, None, None, None)]
    p = np.zeros((3, 2), np.float32)
    with pytest.raises(ValueError):
        pose.recover_pose_batched([np.eye(3)], [p], [p[:2]], K)
    with pytest.raises(ValueError):
        pose.recover_pose_batched([np.eye(3)], [p, p], [p, p], K)
    with pytest.raises(ValueError):
        pose.recover_pose_batched([np.eye(2)], [p], [p], K)
    with pytest.raises(ValueError):
        pose.recover_pose_batched([np.eye(3)], [p], [p], K, distance_threshold=float("nan"))
    with pytest.raises(ValueError):
        pose.recover_pose_batched([np.eye(3)], [p], [p], K, masks=[np.ones(2, np.uint8)])
    with pytest.raises(ValueError):
        pose.recover_pose_batched([np.eye(3)], [p], [p], np.eye(3) * 0)
    from sfm_amd.reconstruction import StructureFromMotion
    assert issubclass(StructureFromMotion, pose.InitialPairMixin)
    assert not hasattr(StructureFromMotion, "find_best_initial_pair")
    assert not hasattr(StructureFromMotion, "initialize_reconstruction")


def test_initial_pair_candidates_skips_unreadable_pairs_before_any_device_work(tmp_path, caplog):
    import logging
    from sfm_amd.reconstruction import StructureFromMotion
    s = StructureFromMotion(tmp_path)
    with caplog.at_level(logging.WARNING):
        assert s.initial_pair_candidates(["pair_1_2", "pair_x"]) == []
        assert s.select_initial_pair(["pair_1_2"]) is None
    assert sum("pair_1_2" in r.getMessage() for r in caplog.records) == 2
