"""GPU tests of the batched PnP RANSAC (sfm_amd.pnp -> sfm_pnp_draw_samples / sfm_pnp_ransac in libsfm_amd.so) against
the NumPy reference that replays the device's samples (tests/pnp_reference.py), on synthetic views and on the 2D-3D
matches of four cameras of the reconstruction the reference project ships."""
import functools
import os

import numpy as np
import pytest

import pnp_reference as pr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K = pr.K_REF
THR = 8.0


@functools.lru_cache(maxsize=None)
def shipped_batch():
    """8 segments: images 3, 12, 20, 33 as shipped, then the same four with the first half of uv replaced by uniform
    pixels.  Returns X list, uv list, and the shipped (R, t) per segment."""
    d = np.load(os.path.join(GOLDEN, "driver_bunny.npz"), allow_pickle=False)
    s = np.load(os.path.join(GOLDEN, "bunny_state.npz"), allow_pickle=False)
    ids = list(s["ids"])
    X = [d[f"f{im}_points3D"] for im in d["f_images"]]
    uv = [d[f"f{im}_points2D"] for im in d["f_images"]]
    poses = [(s["R"][ids.index(im)], s["t"][ids.index(im)]) for im in d["f_images"]]
    rng = np.random.default_rng(5)
    noisy = []
    for a in uv:
        b = a.copy()
        k = len(b) // 2
        b[:k] = (rng.uniform(0, 1, (k, 2)) * [1024, 768]).astype(np.float32)
        noisy.append(b)
    return X + X, uv + noisy, poses + poses


@functools.lru_cache(maxsize=None)
def run_synth(refine):
    from sfm_amd import pnp
    X, uv, _, _ = pr.synth_batch()
    return pnp.solve_pnp_ransac_batched(X, uv, K, THR, n_hypotheses=512, seed=1, refine=refine, return_debug=True)


@functools.lru_cache(maxsize=None)
def run_shipped(refine):
    from sfm_amd import pnp
    X, uv, _ = shipped_batch()
    return pnp.solve_pnp_ransac_batched(X, uv, K, THR, n_hypotheses=1024, seed=0, refine=refine, return_debug=True)


def check_consistent(X, uv, res, dbg, Ks=None):
    """n_inliers == mask.sum() (== max(hyp_count) without a refit, >= with one); the mask is the error rule applied in
    NumPy to the returned pose except within 1e-9 relative of threshold^2; R orthonormal to 1e-12 with determinant +1;
    rodrigues(rvec) == R to 1e-12; inliers == flatnonzero(mask)."""
    from sfm_amd.rotation import rodrigues
    for s, ((ok, rvec, tvec, inl), d) in enumerate(zip(res, dbg)):
        if d["status"] != 0:
            assert ok is False and rvec is None and tvec is None and inl is None and d["n_inliers"] == 0, s
            continue
        Ks_ = K if Ks is None else Ks[s]
        R, t = d["R"], d["t"]
        assert ok is True and rvec.shape == (3, 1) and tvec.shape == (3, 1) and inl.dtype == np.int32 and inl.shape[1] == 1
        assert d["n_inliers"] == len(inl), s
        if d["refined"]:
            assert d["n_inliers"] >= d["hyp_count"].max(), s
        else:
            assert d["n_inliers"] == d["hyp_count"].max(), s
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12, s
        assert np.abs(rodrigues(rvec) - R).max() < 1e-12 and np.array_equal(tvec.ravel(), t), s
        x, p = X[s], uv[s].astype(np.float64)
        Pm = pr.projection(Ks_, R, t)
        with np.errstate(invalid="ignore", over="ignore"):
            q = x @ Pm[:, :3].T + Pm[:, 3]
            lhs = (q[:, 0] - p[:, 0] * q[:, 2]) ** 2 + (q[:, 1] - p[:, 1] * q[:, 2]) ** 2
            rhs = THR * THR * q[:, 2] ** 2
            near = np.abs(lhs - rhs) <= 1e-9 * rhs
            want = (q[:, 2] > 0) & (lhs <= rhs) & np.isfinite(x).all(1) & np.isfinite(p).all(1)
        mask = np.zeros(len(x), bool)
        mask[inl[:, 0]] = True
        assert np.array_equal(inl[:, 0], np.flatnonzero(mask)), s                # ascending, no repeats
        assert np.array_equal(mask[~near], want[~near]), s


# ------------------------------------------------------------------------------------------- replay parity
def test_replay_parity_on_synthetic_views(gpu_ready):
    """Seed 1, 512 hypotheses, no refit: the device's samples equal the NumPy generator's; hyp_count equals the
    reference's per-hypothesis count on the same samples on at least 99 % of the hypotheses of every segment (the
    project's cap from test_fundamental_gpu.py; the reference alone is 100 % stable on these inputs and a correct kernel
    is expected at 100 % - the share seen is printed); the winner's count equals the reference's; M = 3 has status 1."""
    X, uv, _, _ = pr.synth_batch()
    res, dbg = run_synth(False)
    for s, (M, share) in enumerate(pr.CASES):
        d = dbg[s]
        assert np.array_equal(d["samples"], pr.draw_samples(1, s, M, 512)), s
        if M < 4:
            assert d["status"] == 1 and res[s] == (False, None, None, None) and not d["hyp_count"].any()
            continue
        assert d["status"] == 0, s
        ref = pr.ransac(X[s], uv[s], K, d["samples"], THR)
        agree = float(np.mean(d["hyp_count"] == ref["hyp_count"]))
        print(f"segment {s} (M {M}, outliers {share}): hyp_count equal on {agree:.4%} of 512, "
              f"winner {d['n_inliers']} / reference {ref['n_inliers']}")
        assert agree >= 0.99, s
        assert d["n_inliers"] == ref["n_inliers"], s


def test_replay_parity_on_shipped_matches(gpu_ready):
    """Seed 0, 1,024 hypotheses, no refit, the 4 shipped segments and the 4 with half of the pixels replaced: on the
    hypotheses the reference is `stable` on, hyp_count equals the reference's on at least 99 % per segment; at the
    stable hypothesis of highest reference count the device's count equals it, and the winner has at least that count
    (a bound taken from the reference, without a margin)."""
    X, uv, _ = shipped_batch()
    res, dbg = run_shipped(False)
    for s, d in enumerate(dbg):
        assert d["status"] == 0, s
        assert np.array_equal(d["samples"], pr.draw_samples(0, s, len(X[s]), 1024)), s
        ref = pr.ransac(X[s], uv[s], K, d["samples"], THR)
        st = pr.stable(X[s], uv[s], K, d["samples"], THR)
        eq = d["hyp_count"] == ref["hyp_count"]
        h = int(np.argmax(np.where(st, ref["hyp_count"], -1)))
        print(f"segment {s} ({len(X[s])} matches): left out {1 - st.mean():.4%}; equal on {eq[st].mean():.4%} of the stable "
              f"hypotheses; best stable hypothesis {h}: device {d['hyp_count'][h]} / reference {ref['hyp_count'][h]}; "
              f"winner {d['n_inliers']} / reference {ref['n_inliers']}")
        assert eq[st].mean() >= 0.99, s
        assert d["hyp_count"][h] == ref["hyp_count"][h], s
        assert d["n_inliers"] >= ref["hyp_count"][h], s


def test_shipped_matches_against_the_shipped_poses(gpu_ready):
    """Refit on: every segment registers, with at least 0.9 x the inliers the shipped pose of that camera gets under the
    same rule (the factor of test_shipped_pairs_refined_model_against_the_shipped_one)."""
    X, uv, poses = shipped_batch()
    res, dbg = run_shipped(True)
    for s, ((ok, rvec, tvec, inl), d) in enumerate(zip(res, dbg)):
        ship = int(pr.inliers(K, poses[s][0], poses[s][1], X[s], uv[s].astype(np.float64), THR).sum())
        print(f"segment {s}: {d['n_inliers']} inliers (refined {d['refined']}, best hypothesis {d['hyp_count'].max()}), "
              f"shipped pose {ship}")
        assert ok and d["status"] == 0, s
        assert len(inl) >= 0.9 * ship, s


# ---------------------------------------------------------------------------------------- self-consistency
@pytest.mark.parametrize("refine", [False, True])
def test_self_consistency_synthetic(gpu_ready, refine):
    X, uv, _, _ = pr.synth_batch()
    res, dbg = run_synth(refine)
    check_consistent(X, uv, res, dbg)
    assert [d["status"] for d in dbg] == [1, 0, 0, 0, 0, 0]
    if not refine:
        assert not any(d["refined"] for d in dbg)


@pytest.mark.parametrize("refine", [False, True])
def test_self_consistency_shipped(gpu_ready, refine):
    X, uv, _ = shipped_batch()
    res, dbg = run_shipped(refine)
    check_consistent(X, uv, res, dbg)
    print("refinement kept on", sum(d["refined"] for d in dbg), "of", len(dbg), "segments")


def test_refinement_is_no_worse_than_the_true_pose(gpu_ready):
    """On the synthetic cases the refined pose's summed squared reprojection error over the winner's inlier set is no
    higher than the true pose's and no higher than the winner's own: the inequality test_pnp_reference.py establishes
    for the reference's least-squares fit."""
    X, uv, Rs, ts = pr.synth_batch()
    _, plain = run_synth(False)
    res, dbg = run_synth(True)
    for s, (M, share) in enumerate(pr.CASES):
        if M < 4:
            continue
        x, p = X[s], uv[s].astype(np.float64)
        m = pr.inliers(K, plain[s]["R"], plain[s]["t"], x, p, THR)
        assert m.sum() == plain[s]["n_inliers"]
        cw, ct, cr = (pr.cost(K, R, t, x[m], p[m]) for R, t in ((plain[s]["R"], plain[s]["t"]), (Rs[s], ts[s]),
                                                               (dbg[s]["R"], dbg[s]["t"])))
        print(f"M {M} share {share}: cost over the winner's {m.sum()} inliers: winner {cw:.6g} truth {ct:.6g} "
              f"refined {cr:.6g}; refined kept {dbg[s]['refined']}, inliers {dbg[s]['n_inliers']}")
        assert dbg[s]["refined"], s
        assert cr <= ct and cr <= cw, s


# ----------------------------------------------------------------------------- determinism and independence
def test_two_calls_give_identical_bytes(gpu_ready):
    from sfm_amd import pnp
    X, uv, _, _ = pr.synth_batch()
    a, da = pnp.solve_pnp_ransac_batched(X, uv, K, THR, n_hypotheses=512, seed=1, return_debug=True)
    b, db = run_synth(True)
    for s, (x, y) in enumerate(zip(da, db)):
        assert x["hyp_count"].tobytes() == y["hyp_count"].tobytes() and x["refined"] == y["refined"], s
        if x["status"] == 0:
            assert x["R"].tobytes() == y["R"].tobytes() and x["t"].tobytes() == y["t"].tobytes(), s
            assert a[s][3].tobytes() == b[s][3].tobytes() and a[s][1].tobytes() == b[s][1].tobytes(), s


def test_a_segment_does_not_depend_on_its_position_in_the_batch(gpu_ready):
    """A segment alone and the same segment at positions 0, 3 and 7 of the 8-segment batch, with its samples passed in
    explicitly (the generator keys on the segment index): identical pose, inliers and hyp_count."""
    from sfm_amd import pnp
    X, uv, _ = shipped_batch()
    H = 256
    a, b = X[2], uv[6]
    smp = pr.draw_samples(7, 0, len(a), H)
    r0, d0 = pnp.solve_pnp_ransac(a, b, K, n_hypotheses=H, samples=smp, return_debug=True)
    assert r0[0]
    base = [pr.draw_samples(7, s, len(X[s]), H) for s in range(len(X))]
    for pos in (0, 3, 7):
        qX, quv, sm = list(X), list(uv), list(base)
        qX[pos], quv[pos], sm[pos] = a, b, smp
        res, dbg = pnp.solve_pnp_ransac_batched(qX, quv, K, n_hypotheses=H, samples=sm, return_debug=True)
        assert dbg[pos]["R"].tobytes() == d0["R"].tobytes() and dbg[pos]["t"].tobytes() == d0["t"].tobytes(), pos
        assert res[pos][3].tobytes() == r0[3].tobytes() and dbg[pos]["hyp_count"].tobytes() == d0["hyp_count"].tobytes(), pos


def test_hypothesis_counts_have_the_prefix_property(gpu_ready):
    """1, 63, 64, 65 and 1,024 hypotheses: partial wavefronts and workgroups.  Hypothesis h draws the same sample whatever
    the count, so the counts of a shorter run are a prefix of a longer one's."""
    from sfm_amd import pnp
    X, uv, _, _ = pr.synth_batch()
    full = None
    for H in (1024, 65, 64, 63, 1):
        res, dbg = pnp.solve_pnp_ransac_batched(X[2:5], uv[2:5], K, THR, n_hypotheses=H, seed=3, refine=False,
                                                return_debug=True)
        check_consistent(X[2:5], uv[2:5], res, dbg)
        for s, d in enumerate(dbg):
            assert d["hyp_count"].shape == (H,) and d["samples"].shape == (H, 3)
            if full is not None:
                assert np.array_equal(d["hyp_count"], full[s]["hyp_count"][:H]), (H, s)
        if full is None:
            full = dbg


def test_per_segment_K_equals_a_shared_K(gpu_ready):
    from sfm_amd import pnp
    X, uv, _, _ = pr.synth_batch()
    a, da = pnp.solve_pnp_ransac_batched(X, uv, np.stack([K] * len(X)), THR, n_hypotheses=512, seed=1, return_debug=True)
    b, db = run_synth(True)
    for s, (x, y) in enumerate(zip(da, db)):
        assert x["hyp_count"].tobytes() == y["hyp_count"].tobytes() and x["n_inliers"] == y["n_inliers"], s
        if x["status"] == 0:
            assert x["R"].tobytes() == y["R"].tobytes() and a[s][3].tobytes() == b[s][3].tobytes(), s
    # and a K of its own per segment is used: the second view in pixels of a camera with half the focal length
    K2 = K.copy()
    K2[0, 0] = K2[1, 1] = 614.0
    uv2 = ((uv[3].astype(np.float64) - K[:2, 2]) * 0.5 + K[:2, 2]).astype(np.float32)
    res, dbg = pnp.solve_pnp_ransac_batched([X[3], X[3]], [uv[3], uv2], np.stack([K, K2]), THR, n_hypotheses=256,
                                            return_debug=True)
    check_consistent([X[3], X[3]], [uv[3], uv2], res, dbg, Ks=[K, K2])
    assert min(dbg[0]["n_inliers"], dbg[1]["n_inliers"]) >= 0.9 * 210 and np.abs(dbg[1]["R"] - dbg[0]["R"]).max() < 1e-2


# --------------------------------------------------------------------------------------------------- edges
def test_edges_short_and_long_segments(gpu_ready):
    from sfm_amd import pnp
    assert pnp.solve_pnp_ransac_batched([], [], K) == []
    rng = np.random.default_rng(11)
    bX, buv, _, _ = pr.synth_view(rng, 5000, 0.4)                          # spans several LDS chunks
    fX, fuv, _, _ = pr.synth_view(rng, 4, 0.0)
    X = [bX[:0], bX[:3], fX, bX, fX]
    uv = [buv[:0], buv[:3], fuv, buv, fuv]
    for refine in (False, True):
        res, dbg = pnp.solve_pnp_ransac_batched(X, uv, K, THR, n_hypotheses=128, refine=refine, return_debug=True)
        assert [d["status"] for d in dbg] == [1, 1, 0, 0, 0]
        assert res[0] == (False, None, None, None) and res[1] == (False, None, None, None)
        check_consistent(X, uv, res, dbg)
        # 3,000 of the 5,000 pixels are true projections with 0.5 px noise: the project's 0.9 factor of that count
        assert dbg[2]["n_inliers"] == 4 and dbg[3]["n_inliers"] >= 0.9 * 3000
    res, dbg = pnp.solve_pnp_ransac_batched(X, uv, K, THR, n_hypotheses=128, refine=False, return_debug=True)
    ref = pr.ransac(bX, buv, K, dbg[3]["samples"], THR)
    assert float(np.mean(dbg[3]["hyp_count"] == ref["hyp_count"])) >= 0.99 and dbg[3]["n_inliers"] == ref["n_inliers"]


def test_edges_degenerate_planar_and_non_finite_points(gpu_ready):
    from sfm_amd import pnp
    rng = np.random.default_rng(12)
    aX, auv, _, _ = pr.synth_view(rng, 100, 0.2)
    same = np.tile(aX[:1], (20, 1))                                        # all points identical: no sample has area
    pX = aX.copy()
    pX[:, 2] = 6.0 + 0.1 * pX[:, 0]                                        # a planar scene must still register
    R, t = pr.synth_view(np.random.default_rng(0), 4)[2:]
    q = (pX @ R.T + t) @ K.T
    puv = (q[:, :2] / q[:, 2:] + rng.normal(size=(100, 2)) * 0.5).astype(np.float32)
    nX, nuv = aX.copy(), auv.copy()
    nX[33, 0] = np.nan
    nX[5] = [np.inf, -np.inf, 1.0]
    nuv[77, 1] = np.inf
    nuv[60] = [np.nan, np.nan]
    bad = [33, 5, 77, 60]
    X, uv = [same, pX, nX], [auv[:20], puv, nuv]
    for refine in (False, True):
        res, dbg = pnp.solve_pnp_ransac_batched(X, uv, K, THR, n_hypotheses=256, refine=refine, return_debug=True)
        assert [d["status"] for d in dbg] == [2, 0, 0]
        assert res[0] == (False, None, None, None) and not dbg[0]["hyp_count"].any()
        check_consistent(X, uv, res, dbg)
        # 0.9 x the true projections: all 100 of the planar scene; 80 less the three spoilt ones (5 is an outlier anyway)
        assert dbg[1]["n_inliers"] >= 0.9 * 100
        assert np.isfinite(dbg[2]["R"]).all() and not np.isin(bad, res[2][3][:, 0]).any() and dbg[2]["n_inliers"] >= 0.9 * 77
    res, dbg = pnp.solve_pnp_ransac_batched(X, uv, K, THR, n_hypotheses=256, refine=False, return_debug=True)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = pr.ransac(nX, nuv, K, dbg[2]["samples"], THR)
    assert float(np.mean(dbg[2]["hyp_count"] == ref["hyp_count"])) >= 0.99
    assert dbg[2]["n_inliers"] == ref["n_inliers"]


# ----------------------------------------------------------------------------------------------- the chain
def test_candidates_chain_recovers_a_held_out_camera(gpu_ready, tmp_path):
    """find_2d3d_matches -> solve_pnp_ransac_batched through StructureFromMotion.pnp_ransac_candidates on a synthetic
    state with its pair files under tmp_path: the held-out camera is registered with at least 0.9 x the inliers of its
    true pose; a candidate without pairs yields None; `poses` is not written."""
    from sfm_amd.reconstruction import StructureFromMotion
    rng = np.random.default_rng(21)
    N = 400
    X = rng.uniform(-1, 1, (N, 3)) + [0, 0, 6.0]
    poses, pix = [], []
    for c in range(3):
        yaw = 0.2 * c
        R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        t = np.array([-1.2 * c, 0.1 * c, 0.2 * c])
        x = (X @ R.T + t) @ K.T
        pix.append((x[:, :2] / x[:, 2:] + rng.normal(size=(N, 2)) * 0.5).astype(np.float32))
        poses.append((R, t))
    sfm = StructureFromMotion(data_dir=tmp_path)
    for d in (sfm.matches_dir, sfm.corr_dir):
        d.mkdir(parents=True)
    sfm.constructed = ["0000.ppm", "0001.ppm"]
    sfm.poses = {0: poses[0], 1: poses[1]}
    sfm.points3D = [p for p in X]
    sfm.point_tracks = [{0: pix[0][k].tolist(), 1: pix[1][k].tolist()} for k in range(N)]
    for other in (0, 1):                                                     # image 2 against both, 20 % wrong partners
        sel = rng.permutation(N)[:300]
        p2 = pix[2][sel].copy()
        p2[:60] = (rng.uniform(0, 1, (60, 2)) * [1024, 768]).astype(np.float32)
        np.savez(sfm.matches_dir / f"pair_{other}_2_matches.npz", n=300)
        np.save(sfm.corr_dir / f"pair_{other}_2_pts1.npy", pix[other][sel])
        np.save(sfm.corr_dir / f"pair_{other}_2_pts2.npy", p2)
    before = dict(sfm.poses)
    out = sfm.pnp_ransac_candidates([2, 9])
    assert out[9] is None and list(sfm.poses) == [0, 1] and all(sfm.poses[k] is before[k] for k in before)
    R, t, inl = out[2]
    p3, p2 = sfm.find_2d3d_matches(2)
    truth = int(pr.inliers(K, poses[2][0], poses[2][1], p3, p2.astype(np.float64), THR).sum())
    print(f"held-out camera: {len(p3)} 2D-3D matches, {len(inl)} inliers, true pose {truth}")
    assert len(p3) >= 600 and len(inl) >= 0.9 * truth and truth >= 0.9 * 480       # 2 x 240 true partners among the matches
    assert np.abs(R - poses[2][0]).max() < 1e-2 and np.abs(t.ravel() - poses[2][1]).max() < 5e-2
