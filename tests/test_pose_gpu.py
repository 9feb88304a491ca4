"""GPU tests of the batched relative-pose recovery (sfm_amd.pose -> sfm_pose_recover) against the NumPy restatement of
cv2.recoverPose (tests/pose_reference.py) and against the reference's own shipped run.  Counts, n_good and mask bytes
are compared exactly; the four candidates are matched as a set (their order follows the decomposition's sign choices);
poses agree to 1e-12 and the pixel-space points to 1e-9 relative, the bound test_driver_gpu.py holds the same DLT to."""
import functools
import logging

import numpy as np
import pytest

import pose_reference as pr
from test_pose_reference import shipped_pairs, shipped_reference, state

pytestmark = pytest.mark.gpu
K = pr.K_REF


def rel_err(X, ref):
    return float(np.max(np.linalg.norm(X - ref, axis=1) / np.linalg.norm(ref, axis=1))) if len(ref) else 0.0


def check_against_reference(row, dbg, ref, pts1=None, pts2=None, what=""):
    """One segment of a device call (result row + debug dict) against pr.recover_pose's dict: status, the four counts
    through the set matching, n_good, every mask byte, the winner's pose (1e-12) and, when the row carries them, the
    pixel-space points (1e-9 relative).  Returns (pose distance, point distance)."""
    assert dbg["status"] == ref["status"], what
    if ref["status"] != 0:
        assert row[:4] == (0, None, None, None), what
        assert (dbg["cand_count"] == 0).all(), what
        return 0.0, 0.0
    n_good, R, t, mask = row[:4]
    dev_poses = [(dbg["cand_pose"][c][:, :3], dbg["cand_pose"][c][:, 3]) for c in range(4)]
    perm, d_set = pr.match_candidates(dev_poses, ref["poses"])
    assert d_set < 1e-12, (what, d_set)
    assert [int(dbg["cand_count"][perm[k]]) for k in range(4)] == ref["counts"].tolist(), what
    assert n_good == ref["n_good"] and n_good == int(dbg["cand_count"][dbg["winner"]]), what
    assert mask.dtype == np.uint8 and mask.shape == (len(ref["mask"]), 1), what
    assert np.array_equal(mask.ravel(), ref["mask"]), what          # every point: none is left out
    assert R.shape == (3, 3) and t.shape == (3, 1)
    assert np.array_equal(R, dev_poses[dbg["winner"]][0]) and np.array_equal(t.ravel(), dev_poses[dbg["winner"]][1])
    d_pose = pr.pose_distance((R, t), (ref["R"], ref["t"]))
    assert d_pose < 1e-12, (what, d_pose)
    d_x = 0.0
    if len(row) == 5:
        keep = ref["mask"] != 0
        Xr = pr.triangulate_pixels(K, ref["R"], ref["t"], pts1[keep], pts2[keep])
        assert row[4].shape == Xr.shape, what
        d_x = rel_err(row[4], Xr)
        assert d_x < 1e-9, (what, d_x)
    return d_pose, d_x


# ------------------------------------------------------------------------------------------- the shipped pairs
def test_shipped_pairs_equal_the_reference(gpu_ready):
    """All 148 shipped pairs in one call, three ways: the inliers only; all points with the inlier mask as `masks=`;
    all points.  10,907 x 4 decisions, each compared with the reference's."""
    from sfm_amd import pose
    pairs, ref = shipped_pairs(), shipped_reference()
    Es = [pr.essential_from_fundamental(F, K) for _, F, _, _, _ in pairs]
    runs = {"inliers": ([p[2][p[4]] for p in pairs], [p[3][p[4]] for p in pairs], None),
            "masked": ([p[2] for p in pairs], [p[3] for p in pairs], [p[4] for p in pairs]),
            "all": ([p[2] for p in pairs], [p[3] for p in pairs], None)}
    worst = {}
    for label, (p1, p2, masks) in runs.items():
        res, dbg = pose.recover_pose_batched(Es, p1, p2, K, masks=masks, triangulate=True, return_debug=True)
        dp = dx = 0.0
        for s, (name, F, a, b, m) in enumerate(pairs):
            if label == "inliers":
                r = ref[name][0]
            elif label == "all":
                r = ref[name][1]
            else:
                r = pr.recover_pose(Es[s], a, b, K, mask=m)
                assert r["n_good"] == ref[name][0]["n_good"] and not r["mask"][~m].any()
            d = check_against_reference(res[s], dbg[s], r, p1[s], p2[s], f"{label} {name}")
            dp, dx = max(dp, d[0]), max(dx, d[1])
        worst[label] = (dp, dx)
        best = max(range(len(pairs)), key=lambda s: res[s][0])
        assert pairs[best][0] == "pair_25_26" and res[best][0] == (235 if label == "all" else 229)
        if label == "inliers":                    # the device result itself against the reference's shipped run
            st = state()
            n_good, R, t, mask, X = res[best]
            d_ship = pr.pose_distance((R, t), (st["R"][1], st["t"][1]))
            dx_ship = np.abs(X - st["pts"][:229]).max()
            print(f"pair_25_26 against the shipped state: pose {d_ship:.3g}, points {dx_ship:.3g}")
            assert d_ship < 1e-12 and X.shape == (229, 3) and dx_ship < 1e-6
    print("largest distances from the reference (pose, points relative):", worst)


def test_from_fundamental_equals_host_essential(gpu_ready):
    from sfm_amd import pose
    pairs = shipped_pairs()[:40]
    Fs = [p[1] for p in pairs]
    Es = [pr.essential_from_fundamental(F, K) for F in Fs]
    p1, p2 = [p[2] for p in pairs], [p[3] for p in pairs]
    a, da = pose.recover_pose_batched(Es, p1, p2, K, return_debug=True)
    b, db = pose.recover_pose_batched(Fs, p1, p2, K, from_fundamental=True, return_debug=True)
    c, dc = pose.recover_pose_batched(Fs, p1, p2, np.broadcast_to(K, (len(Fs), 3, 3)), from_fundamental=True,
                                      return_debug=True)
    worst = 0.0
    for s in range(len(pairs)):
        dev_a = [(da[s]["cand_pose"][k][:, :3], da[s]["cand_pose"][k][:, 3]) for k in range(4)]
        dev_b = [(db[s]["cand_pose"][k][:, :3], db[s]["cand_pose"][k][:, 3]) for k in range(4)]
        perm, d = pr.match_candidates(dev_b, dev_a)
        worst = max(worst, d, pr.pose_distance(a[s][1:3], b[s][1:3]))
        assert [int(db[s]["cand_count"][perm[k]]) for k in range(4)] == da[s]["cand_count"].tolist()
        assert a[s][0] == b[s][0] and np.array_equal(a[s][3], b[s][3])
        assert all(np.array_equal(x, y) for x, y in zip(b[s], c[s]))                   # per-segment K == shared K
        assert all(np.array_equal(dc[s][k], db[s][k]) for k in ("cand_count", "cand_pose"))
    print("largest pose distance between K^T F K formed on the device and on the host:", worst)
    assert worst < 1e-12


# -------------------------------------------------------------------------------------------- synthetic batches
@functools.lru_cache(maxsize=None)
def edge_batch():
    """Segments of 0, 1, 4, 63, 64, 65, 255, 256, 257 and 1,000 points (0.3 px noise), the last one ending at n, with
    their references."""
    rng = np.random.default_rng(11)
    segs = [pr.synth_pair(rng, M, noise=0.3)[:3] for M in (0, 1, 4, 63, 64, 65, 255, 256, 257, 1000)]
    return segs, [pr.recover_pose(E, a, b, K) for E, a, b in segs]


def test_segment_edges(gpu_ready):
    from sfm_amd import pose
    segs, refs = edge_batch()
    res, dbg = pose.recover_pose_batched([s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs], K,
                                         triangulate=True, return_debug=True)
    assert dbg[0]["status"] == 1 and res[0] == (0, None, None, None, None)
    for s, (E, a, b) in enumerate(segs):
        check_against_reference(res[s], dbg[s], refs[s], a, b, f"segment {s} of {len(a)} points")
        if len(a) >= 4:
            assert res[s][0] >= 0.9 * len(a)
    # n_seg = 1
    E, a, b = segs[5]
    row, d = pose.recover_pose(E, a, b, K, return_debug=True)
    check_against_reference(row, d, refs[5], what="single segment")
    assert all(np.array_equal(x, y) for x, y in zip(row, res[5][:4]))


def test_many_small_segments(gpu_ready):
    """300 segments of one to five points: more than one workgroup of the per-segment kernels, and every wave of the
    per-point kernels straddles segment boundaries."""
    from sfm_amd import pose
    rng = np.random.default_rng(12)
    segs = [pr.synth_pair(rng, int(rng.integers(1, 6)), noise=0.3)[:3] for _ in range(300)]
    res, dbg = pose.recover_pose_batched([s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs], K,
                                         triangulate=True, return_debug=True)
    for s, (E, a, b) in enumerate(segs):
        check_against_reference(res[s], dbg[s], pr.recover_pose(E, a, b, K), a, b, f"segment {s}")


def flat(res, dbg):
    out = []
    for row, d in zip(res, dbg):
        out.append([None if x is None else np.asarray(x).tobytes() for x in row] +
                   [np.asarray(d[k]).tobytes() for k in ("cand_count", "cand_pose", "winner", "status")])
    return out


def test_determinism_and_position_independence(gpu_ready):
    from sfm_amd import pose
    segs, _ = edge_batch()
    order = list(range(len(segs)))

    def run(order):
        r, d = pose.recover_pose_batched([segs[s][0] for s in order], [segs[s][1] for s in order],
                                         [segs[s][2] for s in order], K, triangulate=True, return_debug=True)
        return flat(r, d)
    a, b = run(order), run(order)
    assert a == b
    perm = [9, 3, 0, 7, 1, 8, 2, 6, 4, 5]
    c = run(perm)
    for k, s in enumerate(perm):
        assert c[k] == a[s], (k, s)


def test_every_candidate_slot_wins_somewhere(gpu_ready):
    """32 noise-free scenes: the true pose wins each with every point good and no tie, and over the 32 the winner sits
    in every one of the four candidate slots at least once."""
    from sfm_amd import pose
    rng = np.random.default_rng(5)
    scenes = [pr.synth_pair(rng, 40) for _ in range(32)]
    res, dbg = pose.recover_pose_batched([s[0] for s in scenes], [s[1] for s in scenes], [s[2] for s in scenes], K,
                                         return_debug=True)
    winners = []
    for (E, a, b, R, t, _), row, d in zip(scenes, res, dbg):
        assert row[0] == 40 and (row[3] == 255).all()
        cnt = np.sort(d["cand_count"])
        assert cnt[-1] == 40 and cnt[-2] < 40                       # no tie
        assert pr.pose_distance(row[1:3], (R, t)) < 1e-12
        winners.append(d["winner"])
    print("winning slots:", np.bincount(winners, minlength=4).tolist())
    assert set(winners) == {0, 1, 2, 3}


def test_thresholds_and_mask(gpu_ready):
    from sfm_amd import pose
    rng = np.random.default_rng(3)
    E, p1, p2, R, t, X = pr.synth_pair(rng, 50, depth=(59.0, 61.0))
    assert pose.recover_pose(E, p1, p2, K, distance_threshold=50.0)[0] == 0
    row = pose.recover_pose(E, p1, p2, K, distance_threshold=100.0)
    assert row[0] == 50 and pr.pose_distance(row[1:3], (R, t)) < 1e-12
    # behind the first camera (the last 10 points), and in front of the first but behind the second (10 before them)
    E, p1, p2, R, t = behind_scene()
    row, d = pose.recover_pose(E, p1, p2, K, return_debug=True)
    check_against_reference(row, d, pr.recover_pose(E, p1, p2, K), what="behind")
    assert pr.pose_distance(row[1:3], (R, t)) < 1e-12
    assert row[0] == 60 and (row[3][:60] == 255).all() and not row[3][60:].any()
    m = np.ones(80, np.uint8)
    m[::7] = 0
    row, d = pose.recover_pose(E, p1, p2, K, masks=m, return_debug=True)
    check_against_reference(row, d, pr.recover_pose(E, p1, p2, K, mask=m), what="masked")
    assert not row[3][::7].any() and row[0] == int(m[:60].sum())


def behind_scene():
    """60 points in front of both cameras, 10 in front of the first and behind the second, 10 behind the first; the
    second camera sits at (-0.6, 0, 0.8) looking the same way (R = I, unit baseline)."""
    rng = np.random.default_rng(21)
    R, t = np.eye(3), np.array([0.6, 0.0, -0.8])
    z = np.r_[rng.uniform(4, 12, 60), rng.uniform(0.2, 0.6, 10), rng.uniform(-12, -4, 10)]
    X = np.stack([rng.uniform(-0.3, 0.3, 80) * np.abs(z) + 0.2, rng.uniform(0.05, 0.25, 80) * np.abs(z), z], axis=1)
    Y = X @ R.T + t
    p1 = X[:, :2] / X[:, 2:] * 1228.0 + [512, 384]
    p2 = Y[:, :2] / Y[:, 2:] * 1228.0 + [512, 384]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ R, p1.astype(np.float32), p2.astype(np.float32), R, t


def test_bad_segments_do_not_contaminate_their_neighbours(gpu_ready):
    """E = 0, E with a NaN, a rank-1 E (two zero columns: second singular value exactly 0), a segment of NaN / inf points
    and one without parallax (pts1 == pts2 under a pure translation: every ray pair is parallel) among good segments.
    Nothing here is out of range for the kernels: non-finite values only ever compare false."""
    from sfm_amd import pose
    rng = np.random.default_rng(31)
    good = [pr.synth_pair(rng, M, noise=0.3)[:3] for M in (70, 5, 300, 64)]
    E0, a0, b0 = good[0]
    junk = a0.copy()
    junk[::3] = [np.nan, 1.0]
    junk[1::3] = [np.inf, -np.inf]
    junk[2::3] = [5.0, np.nan]
    tx = np.array([[0, 0.8, 0.0], [-0.8, 0, -0.6], [0.0, 0.6, 0]])                 # [t]x of t = (0.6, 0, -0.8), R = I
    bad = [(np.zeros((3, 3)), a0, b0), (np.where(np.eye(3) > 0, np.nan, E0), a0, b0),
           (np.outer([1.0, 2, 2], [2.0, 0, 0]), a0, b0), (E0, junk, b0), (tx, a0, a0)]
    mixed = [bad[0], good[0], bad[1], bad[2], good[1], good[2], bad[3], bad[4], good[3]]
    is_bad = [True, False, True, True, False, False, True, True, False]
    with np.errstate(all="ignore"):
        res, dbg = pose.recover_pose_batched([s[0] for s in mixed], [s[1] for s in mixed], [s[2] for s in mixed], K,
                                             triangulate=True, return_debug=True)
    clean, dclean = pose.recover_pose_batched([s[0] for s in good], [s[1] for s in good], [s[2] for s in good], K,
                                              triangulate=True, return_debug=True)
    for s, (row, d) in enumerate(zip(res, dbg)):
        if is_bad[s]:
            assert d["status"] == 2 or row[0] == 0, (s, d["status"], row[0])
    assert [d["status"] for d in dbg] == [2, 0, 2, 2, 0, 0, 0, 0, 0]
    assert flat([r for r, bd in zip(res, is_bad) if not bd], [d for d, bd in zip(dbg, is_bad) if not bd]) == \
        flat(clean, dclean)
    for (E, a, b), row, d in zip(good, clean, dclean):
        check_against_reference(row, d, pr.recover_pose(E, a, b, K), a, b)


# --------------------------------------------------------------------------------------------- the mixin chain
def test_initial_pair_mixin_on_the_shipped_files(gpu_ready, tmp_path, caplog):
    from sfm_amd.reconstruction import StructureFromMotion
    s = StructureFromMotion(tmp_path)
    for d in (s.fund_dir, s.corr_dir):
        d.mkdir(parents=True, exist_ok=True)
    pairs = shipped_pairs()
    for name, F, p1, p2, m in pairs:
        np.save(s.corr_dir / f"{name}_pts1.npy", p1[m]); np.save(s.corr_dir / f"{name}_pts2.npy", p2[m])
        np.savez(s.fund_dir / f"{name}_F.npz", F=F, mask=m, pts1=p1, pts2=p2)
    names = [p[0] for p in pairs]
    with caplog.at_level(logging.WARNING):
        cand = s.initial_pair_candidates(names[:5] + ["pair_98_99"] + names[5:])
    assert any("pair_98_99" in r.getMessage() for r in caplog.records)
    assert [c[0] for c in cand] == names
    ref = shipped_reference()
    assert [c[1] for c in cand] == [ref[n][0]["n_good"] for n in names]
    assert s.select_initial_pair(names) == "pair_25_26"
    assert s.initialize_from_pair("pair_25_26") is True
    st = state()
    assert list(s.poses) == [25, 26] and s.constructed == ["0025.ppm", "0026.ppm"]
    assert np.array_equal(s.poses[25][0], np.eye(3)) and np.array_equal(s.poses[25][1], np.zeros((3, 1)))
    assert pr.pose_distance(s.poses[26], (st["R"][1], st["t"][1])) < 1e-12 and s.poses[26][1].shape == (3, 1)
    pts = np.asarray(s.points3D)
    assert isinstance(s.points3D, list) and pts.shape == (229, 3)
    assert np.array_equal(pts, pts.astype(np.float32).astype(np.float64))
    assert np.abs(pts - st["pts"][:229]).max() < 1e-6
    p1, p2 = np.load(s.corr_dir / "pair_25_26_pts1.npy"), np.load(s.corr_dir / "pair_25_26_pts2.npy")
    assert len(s.point_tracks) == 229
    assert all(list(tr) == [25, 26] for tr in s.point_tracks)
    assert np.array_equal(np.asarray([tr[25] for tr in s.point_tracks], dtype=np.float32), p1)
    assert np.array_equal(np.asarray([tr[26] for tr in s.point_tracks], dtype=np.float32), p2)
    assert isinstance(s.point_tracks[0][25], list)
