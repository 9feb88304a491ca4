"""CPU checks for the incremental reconstruction: the NumPy restatements of tests/incremental_reference.py against naive
loops, the host build of tri::gates / tri::judge (sfm_amd/csrc/triangulate_solve.h) against them, and the planning header
of the resection kernels under the sanitizers."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import incremental_reference as ir
import triangulate_reference as tr
from test_triangulate_reference import flat, rel_dev_scalars, scene, status_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_graph(rng, n_img, n_tracks, max_kp=9):
    """(kp_ptr, kp_xy, node_track, cam_of_image, X, has_point) with empty images, every node_track code and NaN points."""
    counts = rng.integers(0, max_kp + 1, n_img)
    counts[rng.integers(0, n_img)] = 0
    kp_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n_nodes = int(kp_ptr[-1])
    node_track = rng.integers(-3, n_tracks + 2, n_nodes).astype(np.int32)
    cam_of_image = np.where(rng.random(n_img) < 0.4, rng.integers(0, 5, n_img), -1).astype(np.int32)
    X = rng.normal(size=(n_tracks, 3))
    X[rng.random(n_tracks) < 0.1] = np.nan
    has_point = (rng.random(n_tracks) < 0.6).astype(np.uint8) * rng.integers(1, 255, n_tracks).astype(np.uint8)
    return kp_ptr, rng.uniform(0, 1000, (n_nodes, 2)), node_track, cam_of_image, X, has_point


def test_resection_lists_equal_a_naive_double_loop():
    rng = np.random.default_rng(31)
    listed_any = 0
    for _ in range(200):
        n_img, n_tracks = int(rng.integers(1, 8)), int(rng.integers(0, 12))
        kp_ptr, kp_xy, node_track, cam_of_image, X, has_point = random_graph(rng, n_img, n_tracks)
        seg_ptr, node, track = [0], [], []
        for i in range(n_img):
            for n in range(kp_ptr[i], kp_ptr[i + 1]):
                t = node_track[n]
                if cam_of_image[i] < 0 and 0 <= t < n_tracks and has_point[t] != 0:
                    node.append(n); track.append(t)
            seg_ptr.append(len(node))
        r = ir.resection_lists(kp_ptr, kp_xy, node_track, cam_of_image, X, has_point)
        assert r["seg_ptr"].tolist() == seg_ptr and r["total"] == len(node)
        assert r["corr_node"].tolist() == node and r["corr_track"].tolist() == track
        assert np.array_equal(r["corr_X"].view(np.int64), X[track].reshape(-1, 3).view(np.int64))
        assert np.array_equal(r["corr_uv"], kp_xy[node].reshape(-1, 2).astype(np.float32)) and r["corr_uv"].dtype == np.float32
        listed_any += len(node)
    assert listed_any > 100


@functools.lru_cache(maxsize=None)
def native(tmp):
    """The host build of the gates (tests/native/triangulate_gates_check.cpp) under the sanitizers: run(records) -> doubles."""
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(tmp, "triangulate_gates_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "triangulate_gates_check.cpp"), "-o", exe], check=True)

    def run(records):
        np.ascontiguousarray(records, dtype=np.float64).tofile(exe + ".in")
        subprocess.run([exe, exe + ".in", exe + ".out"], check=True)
        return np.fromfile(exe + ".out")
    return run


def native_judge(run, args, X, min_views=2, max_error=4.0, min_angle_deg=0.0):
    """tri::judge of the host build on every track: {status, n_views, max_err, obs_err}."""
    proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = args
    cos_min = np.cos(min_angle_deg * (np.pi / 180.0))
    rec, lens = [], []
    for t in range(len(track_ptr) - 1):
        o = np.arange(track_ptr[t], track_ptr[t + 1])
        lens.append(len(o))
        rec.append(np.concatenate([[len(o), min_views, max_error, float(min_angle_deg > 0), cos_min], X[t]]))
        for k in o:
            cam = cam_of_image[obs_image[k]]
            used = cam >= 0
            rec.append(np.concatenate([[float(used)], proj[cam if used else 0], kp_xy[kp_ptr[obs_image[k]] + obs_kp[k]]]))
    out = run(np.concatenate([np.asarray(r, dtype=np.float64).ravel() for r in rec]))
    at = np.concatenate([[0], np.cumsum(np.asarray(lens) + 3)])
    head = np.stack([out[a:a + 3] for a in at[:-1]])
    return {"status": head[:, 0].astype(np.int32), "n_views": head[:, 1].astype(np.int32), "max_err": head[:, 2],
            "obs_err": np.concatenate([out[a + 3:b] for a, b in zip(at[:-1], at[1:])])}


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def test_host_gates_equal_the_reference_bit_for_bit(tmp_path_factory):
    """Perturbed points on random tracks of 2 to 40 views: the host build of tri::judge runs the operations of the NumPy
    evaluate in its order, so status, n_views, max_err and every observation's error agree in every bit."""
    run = native(str(tmp_path_factory.mktemp("native")))
    if run is None:
        pytest.skip("no g++")
    proj, X, g = scene()
    reg = np.arange(40, dtype=np.int32)
    reg[[7, 19]] = -1
    reg[reg >= 0] = np.arange(38)
    args = (np.delete(np.asarray(proj).reshape(-1, 12), [7, 19], axis=0), reg) + tuple(g)
    rng = np.random.default_rng(32)
    Xp = X + rng.normal(0, 0.02, X.shape)
    Xp[5] = np.nan
    Xp[6] = 0.5 + 40.0 * (Xp[6] - 0.5)
    has = np.ones(len(X), np.uint8)
    ref = ir.evaluate(*args, Xp, has, min_angle_deg=1.0)
    out = native_judge(run, args, Xp, min_angle_deg=1.0)
    assert np.array_equal(out["status"], ref["status"]) and np.array_equal(out["n_views"], ref["n_views"])
    assert same_bits(out["max_err"], ref["max_err"]) and same_bits(out["obs_err"], ref["obs_err"])
    assert ref["status"][5] == tr.DEGENERATE and len(set(ref["status"].tolist())) >= 3 and np.isnan(ref["obs_err"]).any()
    # without a point: NO_POINT, NaN, not counted; n_views stays
    has[::3] = 0
    cut = ir.evaluate(*args, Xp, has, min_angle_deg=1.0)
    assert (cut["status"][::3] == ir.NO_POINT).all() and np.isnan(cut["max_err"][::3]).all()
    assert np.array_equal(cut["n_views"], ref["n_views"]) and cut["counts"].sum() == (has != 0).sum()
    keep = has != 0
    assert np.array_equal(cut["status"][keep], ref["status"][keep]) and same_bits(cut["max_err"][keep], ref["max_err"][keep])


def test_host_gates_repeat_the_status_of_the_triangulation(tmp_path_factory):
    """Fed the reference triangulation's own X, the gates return its status for every track that has an X (0, 3, 4, 5) and
    its max_err bits: solve's last gates() call ran on the same numbers.  The status cases give one track per code."""
    run = native(str(tmp_path_factory.mktemp("native")))
    if run is None:
        pytest.skip("no g++")
    proj, _, g = scene()
    g = list(g)
    g[1] = g[1].copy()
    g[1][::11] += 9.0                                                          # some tracks fail the 4 px gate
    for args in (flat(proj, g), status_cases()[0]):
        for iters in (0, 5):
            ref = tr.triangulate(*args, refine_iters=iters, min_angle_deg=1.0)
            live = np.isin(ref["status"], [tr.OK, tr.BEHIND, tr.LOW_ANGLE, tr.HIGH_ERROR])
            X = np.where(live[:, None], ref["X"], 0.0)
            out = native_judge(run, args, X, min_angle_deg=1.0)
            py = ir.evaluate(*args, X, np.ones(len(X), np.uint8), min_angle_deg=1.0)
            assert np.array_equal(out["status"][live], ref["status"][live]) and np.array_equal(out["n_views"], ref["n_views"])
            assert same_bits(out["max_err"][live], ref["max_err"][live])
            assert np.array_equal(py["status"][live], ref["status"][live]) and same_bits(py["max_err"][live], ref["max_err"][live])
    assert set(ref["status"].tolist()) == set(range(6))


def test_reference_evaluate_follows_its_80_bit_run():
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 here")
    proj, X, g = scene()
    args = flat(proj, g)
    Xp = X + np.random.default_rng(33).normal(0, 0.02, X.shape)
    has = np.ones(len(X), np.uint8)
    a = ir.evaluate(*args, Xp, has, max_error=40.0, min_angle_deg=1.0)
    b = ir.evaluate(*args, Xp, has, max_error=40.0, min_angle_deg=1.0, dtype=np.longdouble)
    assert np.array_equal(a["status"], b["status"])
    d = rel_dev_scalars(a["max_err"], b["max_err"]), rel_dev_scalars(a["obs_err"], b["obs_err"])
    print("evaluate, float64 against 80-bit: max_err %.3g, obs_err %.3g" % d)
    assert max(d) < 1e-9


def test_resection_plan_under_address_and_ub_sanitizers(tmp_path):
    """sfm_amd/csrc/resection_plan.h (workspace layout and size checks) is plain C++: built with g++
    -fsanitize=address,undefined and driven over sizes up to 2^31 - 1, the workgroup edges and the edges of one pass over
    the workgroup sums."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "resection_plan_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "resection_plan_check.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    for seed in (1, 2):
        run = subprocess.run([str(exe), str(seed)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])


def test_alignment_recovers_a_known_similarity():
    rng = np.random.default_rng(34)
    src = rng.normal(size=(30, 3))
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    A *= np.sign(np.linalg.det(A))
    s, t = 2.5, np.array([1.0, -2.0, 3.0])
    dst = s * src @ A.T + t
    s1, R1, t1, out = ir.align_similarity(src, dst)
    assert abs(s1 - s) < 1e-12 and np.abs(R1 - A).max() < 1e-12 and np.abs(t1 - t).max() < 1e-12
    assert np.abs(out - dst).max() < 1e-12
    noisy = dst + rng.normal(0, 0.01, dst.shape)
    assert np.sqrt(((ir.align_similarity(src, noisy)[3] - noisy) ** 2).sum(axis=1).mean()) < 0.03


def test_host_side_helpers_of_the_loop():
    """What reconstruct_tracks computes on the host: node_track from the CSR arrays, the pairs with the most common tracks
    (ties to the lower pair), the pixels of a pair's common tracks, and the input validation - no device involved."""
    from sfm_amd import Tracks, evaluate_tracks, reconstruct_tracks, resection_lists
    from sfm_amd.incremental import _common_track_pairs, _pair_pixels, node_track_of
    # tracks: {0:1, 1:0, 2:2}, {0:2, 2:0}, {1:1, 2:1}
    T = Tracks([0, 3, 5, 8], [0, 3, 5, 7], [0, 1, 2, 0, 2, 1, 2], [1, 0, 2, 2, 0, 1, 1])
    assert node_track_of(T).tolist() == [-1, 0, 1, 0, 2, 1, 2, 0]
    assert _common_track_pairs(T, 32) == [(0, 2), (1, 2), (0, 1)] and _common_track_pairs(T, 1) == [(0, 2)]
    kp_xy = np.arange(16, dtype=np.float64).reshape(8, 2)
    a, b, common = _pair_pixels(T, kp_xy, 0, 2)
    assert a.tolist() == [[2, 3], [4, 5]] and b.tolist() == [[14, 15], [10, 11]] and common.tolist() == [0, 1]
    kps = [kp_xy[0:3], kp_xy[3:5], kp_xy[5:8]]
    K = tr.K_SFM
    for bad in (lambda: reconstruct_tracks(T, kps[:2], K), lambda: reconstruct_tracks(T, kps, K[:2]),
                lambda: reconstruct_tracks(T, kps, K, initial_pair=(0, 3)), lambda: reconstruct_tracks(T, kps, K, initial_pair=(1, 1)),
                lambda: reconstruct_tracks(T, kps, K, cam_dim=7),
                lambda: resection_lists(T, kps, np.zeros((2, 3)), np.ones(3), -np.ones(3)),
                lambda: evaluate_tracks(T, kps, np.zeros((3, 3, 4)), np.zeros((3, 3)), np.ones(2))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        reconstruct_tracks(T, kps, K, no_such_option=1)
    # empty inputs are answered without a device
    E = Tracks([0, 3, 5, 8], [0], [], [])
    rec = reconstruct_tracks(E, kps, K)
    assert rec.poses == {} and rec.order == [] and rec.unregistered == [0, 1, 2] and rec.X.shape == (0, 3) and rec.log == []
    assert rec.as_state() == ({}, [], []) and len(rec.ba_inputs()[1]) == 0
    seg_ptr, corr_track, corr_X, corr_uv = resection_lists(E, kps, np.zeros((0, 3)), np.zeros(0), -np.ones(3))
    assert seg_ptr.tolist() == [0, 0, 0, 0] and corr_X.shape == (0, 3) and corr_uv.dtype == np.float32
    ev = evaluate_tracks(E, kps, np.zeros((3, 3, 4)), np.zeros((0, 3)), np.zeros(0))
    assert ev["counts"].tolist() == [0] * 6 and ev["status"].shape == (0,)
