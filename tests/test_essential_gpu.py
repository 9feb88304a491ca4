"""GPU tests of the batched essential-matrix RANSAC (sfm_amd.essential -> sfm_ess_draw_samples / sfm_ess_ransac in
libsfm_amd.so) against the NumPy reference that replays the device's samples (tests/essential_reference.py), on
synthetic two-view scenes and on the 148 pairs the reference project ships, and of the loop's `initial_model` option."""
import ctypes as C
import functools

import numpy as np
import pytest

import essential_reference as er
import fundamental_reference as fr
from test_essential_reference import left_out_share, shipped, shipped_replay, synthetic_replay

pytestmark = pytest.mark.gpu

K = fr.K_REF
THR = 3.0


@functools.lru_cache(maxsize=None)
def bunny():
    pairs = er.shipped_pairs()
    return [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs]


@functools.lru_cache(maxsize=None)
def run_synth(refine):
    from sfm_amd import essential
    p1, p2 = er.synth_batch()
    return essential.estimate_essential_batched(p1, p2, K, THR, n_hypotheses=512, seed=1, refine=refine, return_debug=True)


@functools.lru_cache(maxsize=None)
def run_shipped12(refine):
    from sfm_amd import essential
    sh = shipped()
    return essential.estimate_essential_batched([s[1] for s in sh], [s[2] for s in sh], K, THR, n_hypotheses=512, seed=0,
                                                refine=refine, return_debug=True)


@functools.lru_cache(maxsize=None)
def run_bunny(refine=True):
    from sfm_amd import essential
    p1, p2, _ = bunny()
    return essential.estimate_essential_batched(p1, p2, K, THR, n_hypotheses=1024, seed=0, refine=refine, return_debug=True)


def check_replay(name, d, res, st):
    """hyp_count equals the reference's on at least 99 % of the stable hypotheses, of which at most 1 % of the non-voided
    ones are left out; the winner's count equals the reference's best stable count or exceeds it."""
    eq = d["hyp_count"] == res["hyp_count"]
    best = int(res["hyp_count"][st].max())
    print(f"{name}: hyp_count equal on {eq[st].mean():.4%} of the stable hypotheses, {eq.mean():.4%} of all; left out "
          f"{left_out_share(res, st):.2%}; winner {d['n_inliers']} / best stable reference count {best}")
    assert left_out_share(res, st) <= 0.01, name
    assert eq[st].mean() >= 0.99, name
    assert (d["hyp_count"][res["voided"]] == 0).all(), name
    assert d["n_inliers"] >= best, name
    return eq


def check_consistent(p1, p2, res, dbg):
    """n_inliers == mask.sum() (== max(hyp_count) without a refit, >= with one); the mask is the pixel rule applied in NumPy
    to K^-T E K^-1 except within 1e-9 relative of threshold^2; |E|_F = sqrt(2); the sign rule; the singular values of an
    essential matrix.  Returns the largest deviations seen: (s0 - s1) / s0 and s2 / s0."""
    worst = [0.0, 0.0]
    for s, ((E, mask), d) in enumerate(zip(res, dbg)):
        if d["status"] != 0:
            assert E is None and mask is None and d["n_inliers"] == 0, s
            continue
        assert mask.shape == (len(p1[s]), 1) and mask.dtype == np.uint8 and E.shape == (3, 3)
        assert d["n_inliers"] == int(mask.sum()), s
        if d["refined"]:
            assert d["n_inliers"] >= d["hyp_count"].max(), s
        else:
            assert d["n_inliers"] == d["hyp_count"].max(), s
        with np.errstate(invalid="ignore"):
            e = fr.cv_err2(er.to_pixels(E, K), np.asarray(p1[s], np.float64), np.asarray(p2[s], np.float64))
            near = np.abs(e - THR * THR) <= 1e-9 * THR * THR
            want = e <= THR * THR
        assert np.array_equal(mask.ravel().astype(bool)[~near], want[~near]), s
        assert abs(np.linalg.norm(E) - np.sqrt(2.0)) <= 1e-12, s
        assert E.ravel()[np.argmax(np.abs(E))] > 0, s
        sv = np.linalg.svd(E, compute_uv=False)
        worst = [max(worst[0], (sv[0] - sv[1]) / sv[0]), max(worst[1], sv[2] / sv[0])]
        assert sv[0] - sv[1] <= 1e-9 * sv[0] and sv[2] <= 1e-9 * sv[0], (s, sv)
    return worst


# ------------------------------------------------------------------------------------------- replay parity
def test_replay_parity_on_synthetic_pairs(gpu_ready):
    res, dbg = run_synth(False)
    for s, ((M, share), (smp, ref, st)) in enumerate(zip(er.CASES, synthetic_replay())):
        d = dbg[s]
        assert np.array_equal(d["samples"], smp), s
        if M < 5:
            assert d["status"] == 1 and res[s] == (None, None) and (d["hyp_count"] == 0).all()
            continue
        assert d["status"] == 0, s
        check_replay(f"segment {s} (M {M}, outliers {share})", d, ref, st)


def test_replay_parity_on_shipped_pairs(gpu_ready):
    """Pairs 0, 13, ..., 143 in one call, seed 0, 512 hypotheses, no refit; at the stable hypothesis of the highest
    reference count the device's count equals it."""
    res, dbg = run_shipped12(False)
    for s, ((i, _, _, _), (smp, ref, st)) in enumerate(zip(shipped(), shipped_replay())):
        d = dbg[s]
        assert d["status"] == 0 and np.array_equal(d["samples"], smp), i
        check_replay(f"pair {i}", d, ref, st)
        top = int(np.argmax(np.where(st, ref["hyp_count"], -1)))
        assert d["hyp_count"][top] == ref["hyp_count"][top], i


# ---------------------------------------------------------------------------------------- self-consistency
@pytest.mark.parametrize("refine", [False, True])
def test_self_consistency_synthetic(gpu_ready, refine):
    p1, p2 = er.synth_batch()
    res, dbg = run_synth(refine)
    print("synthetic, refit", refine, ": largest (s0 - s1) / s0 %.1e, s2 / s0 %.1e" % tuple(check_consistent(p1, p2, res, dbg)),
          "; refit kept on", sum(d["refined"] for d in dbg), "of", len(dbg))
    assert [d["status"] for d in dbg] == [1, 0, 0, 0, 0, 0, 0]
    if not refine:
        assert not any(d["refined"] for d in dbg)


@pytest.mark.parametrize("refine", [False, True])
def test_self_consistency_shipped_pairs(gpu_ready, refine):
    sh = shipped()
    res, dbg = run_shipped12(refine)
    print("shipped, refit", refine, ": largest (s0 - s1) / s0 %.1e, s2 / s0 %.1e" %
          tuple(check_consistent([s[1] for s in sh], [s[2] for s in sh], res, dbg)), "; refit kept on",
          sum(d["refined"] for d in dbg), "of", len(dbg))
    assert all(d["status"] == 0 for d in dbg)


# ------------------------------------------------------------------------------------------- shipped data
def test_all_shipped_pairs_keep_the_inliers_and_give_a_pose_that_passes_the_gate(gpu_ready):
    """148 pairs in one call, 1,024 hypotheses, refit on: every pair has a model, at least 0.85 x the inliers of the shipped
    F under the same rule, and recover_pose_batched(E, from_fundamental=False, triangulate=True) leaves at least 90 % of
    its good points within 4 px in both views."""
    from sfm_amd.pose import recover_pose_batched
    p1, p2, Fs = bunny()
    res, dbg = run_bunny(True)
    assert all(d["status"] == 0 for d in dbg)
    check_consistent(p1, p2, res, dbg)
    ship = np.array([fr.inliers(F, a.astype(np.float64), b.astype(np.float64), THR).sum() for a, b, F in zip(p1, p2, Fs)])
    mine = np.array([d["n_inliers"] for d in dbg])
    ratio = mine / ship
    print("inliers against the shipped F's: min %.3f (pair %d), median %.3f, not below it in %d of 148; refit kept on %d" %
          (ratio.min(), int(ratio.argmin()), float(np.median(ratio)), int((mine >= ship).sum()), sum(d["refined"] for d in dbg)))
    assert ratio.min() >= 0.85
    pose = recover_pose_batched([E for E, _ in res], p1, p2, K, masks=[m for _, m in res], from_fundamental=False,
                                triangulate=True)
    shares = []
    for s, out in enumerate(pose):
        n_good, R, t, mask, X = out
        good = np.asarray(mask).reshape(-1) != 0
        assert R is not None and n_good == good.sum() > 0, s
        err = er.reprojection_errors(K, R, t, np.asarray(X), p1[s][good].astype(np.float64), p2[s][good].astype(np.float64))
        shares.append(float((err <= 4.0).mean()))
        assert shares[-1] >= 0.9, (s, shares[-1])
    print("share of the good points within 4 px: min %.3f, median %.3f" % (min(shares), float(np.median(shares))))


# ----------------------------------------------------------------------------- determinism and independence
def test_two_calls_give_identical_bytes(gpu_ready):
    from sfm_amd import essential
    p1, p2 = er.synth_batch()
    a, da = essential.estimate_essential_batched(p1, p2, K, THR, n_hypotheses=512, seed=1, return_debug=True)
    b, db = run_synth(True)
    for (Ea, ma), (Eb, mb), x, y in zip(a[1:], b[1:], da[1:], db[1:]):
        assert Ea.tobytes() == Eb.tobytes() and ma.tobytes() == mb.tobytes()
        assert x["hyp_count"].tobytes() == y["hyp_count"].tobytes() and x["refined"] == y["refined"]


def test_a_pair_does_not_depend_on_its_position_in_the_batch(gpu_ready):
    """A pair alone and the same pair at positions 0, 73 and 147 of the 148-pair batch, with its samples passed in
    explicitly (the generator keys on the segment index): identical E, mask and hyp_count."""
    from sfm_amd import essential
    p1, p2, _ = bunny()
    H = 128
    a, b = p1[30], p2[30]
    smp = er.draw_samples(7, 0, len(a), H)
    (E0, m0), d0 = essential.find_essential(a, b, K, THR, n_hypotheses=H, samples=smp, return_debug=True)
    assert E0 is not None
    base = [er.draw_samples(7, s, len(p1[s]), H) for s in range(len(p1))]
    for pos in (0, 73, 147):
        q1, q2, sm = list(p1), list(p2), list(base)
        q1[pos], q2[pos], sm[pos] = a, b, smp
        res, dbg = essential.estimate_essential_batched(q1, q2, K, THR, n_hypotheses=H, samples=sm, return_debug=True)
        E, m = res[pos]
        assert E.tobytes() == E0.tobytes() and m.tobytes() == m0.tobytes(), pos
        assert dbg[pos]["hyp_count"].tobytes() == d0["hyp_count"].tobytes(), pos


# --------------------------------------------------------------------------------------------------- edges
def test_edges_short_and_long_segments(gpu_ready):
    from sfm_amd import essential
    assert essential.estimate_essential_batched([], [], K) == []
    rng = np.random.default_rng(11)
    big1, big2, _ = fr.synth_pair(rng, 1500, 0.4)                          # spans several LDS chunks
    p1 = [big1, big1[:0], big1[:4], big1]
    p2 = [big2, big2[:0], big2[:4], big2]
    for refine in (False, True):
        res, dbg = essential.estimate_essential_batched(p1, p2, K, THR, n_hypotheses=64, refine=refine, return_debug=True)
        assert [d["status"] for d in dbg] == [0, 1, 1, 0] and res[1] == (None, None) and res[2] == (None, None)
        check_consistent(p1, p2, res, dbg)
    res, dbg = essential.estimate_essential_batched(p1, p2, K, THR, n_hypotheses=64, refine=False, return_debug=True)
    ref = er.ransac(big1, big2, K, dbg[3]["samples"], THR)
    assert np.mean(dbg[3]["hyp_count"] == ref["hyp_count"]) >= 0.99


def test_edges_repeated_and_non_finite_points(gpu_ready):
    """One match repeated 40 times voids every sample: status 2.  NaN / inf coordinates are never inliers and void the
    samples that hold them."""
    from sfm_amd import essential
    rng = np.random.default_rng(12)
    same = np.tile(np.float32([[321.5, 123.25]]), (40, 1))
    a1, a2, _ = fr.synth_pair(rng, 100, 0.2)
    a1, a2 = a1.copy(), a2.copy()
    a1[33, 0] = np.nan
    a2[77, 1] = np.inf
    a1[5] = [np.inf, -np.inf]
    p1, p2 = [same, a1], [same + np.float32(2.0), a2]
    for refine in (False, True):
        res, dbg = essential.estimate_essential_batched(p1, p2, K, THR, n_hypotheses=256, refine=refine, return_debug=True)
        assert dbg[0]["status"] == 2 and res[0] == (None, None) and (dbg[0]["hyp_count"] == 0).all()
        assert dbg[1]["status"] == 0
        E, mask = res[1]
        assert np.isfinite(E).all() and mask[33, 0] == 0 and mask[77, 0] == 0 and mask[5, 0] == 0
        check_consistent(p1, p2, res, dbg)
    res, dbg = essential.estimate_essential_batched(p1, p2, K, THR, n_hypotheses=256, refine=False, return_debug=True)
    smp = dbg[1]["samples"]
    holds_bad = np.isin(smp, [33, 77, 5]).any(1)
    assert holds_bad.any() and (dbg[1]["hyp_count"][holds_bad] == 0).all()
    with np.errstate(invalid="ignore", over="ignore"):
        ref = er.ransac(a1, a2, K, smp, THR)
    assert np.array_equal(ref["voided"], holds_bad)
    assert np.mean(dbg[1]["hyp_count"] == ref["hyp_count"]) >= 0.99


def test_edges_hypothesis_counts(gpu_ready):
    """1, 63, 64, 65 and 1,024 hypotheses: partial wavefronts and workgroups.  Hypothesis h draws the same sample whatever
    the count, so the counts of a shorter run are a prefix of a longer one's."""
    from sfm_amd import essential
    p1, p2 = er.synth_batch()
    full = None
    for H in (1024, 65, 64, 63, 1):
        res, dbg = essential.estimate_essential_batched(p1[3:6], p2[3:6], K, THR, n_hypotheses=H, seed=3, refine=False,
                                                        return_debug=True)
        check_consistent(p1[3:6], p2[3:6], res, dbg)
        for s, d in enumerate(dbg):
            assert d["hyp_count"].shape == (H,) and d["samples"].shape == (H, 5)
            if full is not None:
                assert np.array_equal(d["hyp_count"], full[s]["hyp_count"][:H]), (H, s)
        if full is None:
            full = dbg


def test_bad_samples_and_bad_arguments_are_rejected(gpu_ready):
    import torch
    from sfm_amd import _lib, essential
    from sfm_amd.driver import _p
    p1, p2 = er.synth_batch()
    smp = er.draw_samples(0, 0, 40, 8)
    for bad in (np.where(np.arange(40).reshape(8, 5) == 7, 40, smp), np.where(np.arange(40).reshape(8, 5) == 7, -1, smp)):
        with pytest.raises(ValueError):
            essential.find_essential(p1[3], p2[3], K, n_hypotheses=8, samples=bad)
    with pytest.raises(ValueError):
        essential.find_essential(p1[3], p2[3], K, n_hypotheses=8, samples=np.tile(smp[:, :1], (1, 5)))
    with pytest.raises(ValueError):
        essential.find_essential(p1[3], p2[3], np.eye(4))
    with pytest.raises(ValueError):
        essential.find_essential(p1[3], p2[3], np.diag([0.0, 1228.0, 1.0]))
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    n, H = 40, 8
    seg = torch.tensor([0, n], dtype=torch.int64, device=dev)
    a, b = (torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in (p1[3], p2[3]))
    k4 = torch.tensor([[1228.0, 1228.0, 512.0, 384.0]], dtype=torch.float64, device=dev)
    d_smp = torch.from_numpy(smp).to(dev)
    E = torch.full((1, 9), 7.0, dtype=torch.float64, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    meta = torch.empty((3, 1), dtype=torch.int32, device=dev)
    need = C.c_int64()
    assert h.lib.sfm_ess_workspace_bytes(n, 1, H, C.byref(need)) == 0 and need.value > 0
    assert h.lib.sfm_ess_workspace_bytes(n, 1, 0, C.byref(need)) == -1
    assert h.lib.sfm_ess_workspace_bytes(n, 1, H, None) == -1
    assert h.lib.sfm_ess_workspace_bytes(n, 1, H, C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)

    def call(n_seg=1, n_hyp=H, thr=3.0, pts=a, out=E, k=k4, ws_bytes=need.value, handle=h._h):
        return h.lib.sfm_ess_ransac(handle, _p(seg), n_seg, _p(pts), _p(b), n, _p(k), _p(d_smp), n_hyp, C.c_double(thr), 0,
                                    _p(out), _p(mask), _p(meta[0]), _p(meta[1]), None, _p(meta[2]), _p(ws), ws_bytes)
    assert call(handle=None) == -1
    assert call(n_seg=-1) == -1 and call(n_hyp=0) == -1 and call(thr=-1.0) == -1 and call(thr=float("nan")) == -1
    assert call(pts=None) == -1 and call(out=None) == -1 and call(k=None) == -1
    assert b"null pointer" in h.lib.sfm_last_error(h._h)
    assert call(ws_bytes=need.value - 1) == -3
    torch.cuda.synchronize()
    assert (E == 7.0).all()                                               # nothing ran
    assert h.lib.sfm_ess_draw_samples(h._h, _p(seg), 1, 0, C.c_uint64(0), _p(d_smp)) == -1
    assert call() == 0
    torch.cuda.synchronize()
    assert meta[1, 0].item() == 0 and abs(float(E.norm()) - np.sqrt(2.0)) < 1e-12


# ------------------------------------------------------------------------------------------------ the loop
def test_loop_with_the_essential_model_on_a_noisy_scene(gpu_ready):
    """`initial_model="essential"` without the two-camera bundle adjustment: all 8 images register and every returned
    point passes the gates under the returned cameras."""
    from sfm_amd import reconstruct_tracks
    import test_incremental_gpu as ti
    import triangulate_reference as tr
    s = ti.loop_scene()
    rec = reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, initial_model="essential", refine_initial_pair=False)
    print("registration order:", rec.order, "step 0:", {k: rec.log[0][k] for k in ("initial_pair", "initial_model", "n_good", "points_added")})
    assert sorted(rec.order) == list(range(8)) and rec.unregistered == []
    assert rec.log[0]["initial_model"] == "essential" and rec.log[0]["pair_refinement"] is None
    ti.assert_invariant(s, rec)
    assert ti.loop_result().log[0]["initial_model"] == "fundamental"
    with pytest.raises(ValueError):
        reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, initial_model="homography")


def test_loop_step_zero_on_the_shipped_matches(gpu_ready):
    """The shipped matches joined into tracks as test_loop_on_the_shipped_matches does, the initial pair fixed to the one
    the default options choose, no two-camera bundle adjustment: the first triangulation under "essential" adopts at
    least 0.9 x what the NumPy chain (essential_reference -> pose_reference -> the gates of triangulate_reference) adopts
    for that pair, and the same chain fed E = K^T F K of the shipped F adopts fewer than half as many.
    Measured with the NumPy chain alone, pair (24, 25), 216 common tracks: five-point 216, shipped F 0; the F of this
    project's own RANSAC with its 8-point refit over all 216 matches (replayed in NumPy, seed 0) 115 - printed, not
    asserted: the refit's F is a better F than the shipped one, not an essential matrix."""
    import pose_reference as pr
    import triangulate_reference as tr
    from sfm_amd import build_tracks, incremental, reconstruct_tracks
    from sfm_amd.triangulate import keypoint_table
    from test_tracks_reference import shipped as shipped_flat
    Ks = tr.K_SFM
    kp_ptr, seg_ptr, pairs, q, t, mask, pts1, pts2 = shipped_flat()
    cut = lambda a: [a[seg_ptr[k]:seg_ptr[k + 1]] for k in range(len(pairs))]
    T = build_tracks([500] * 35, pairs, list(zip(cut(q), cut(t))), masks=cut(mask))
    xy = np.full((35, 500, 2), np.nan, np.float32)
    seg = np.repeat(np.arange(len(pairs)), np.diff(seg_ptr))
    xy[pairs[seg, 0], q] = pts1
    xy[pairs[seg, 1], t] = pts2
    kps = [np.asarray(a, dtype=np.float64) for a in xy]
    kp_xy = keypoint_table(T, kps)
    (i, j) = incremental._initial_pair(T, kp_xy, Ks, None, dict(incremental.DEFAULTS), 0)[0]
    a, b, _ = incremental._pair_pixels(T, kp_xy, i, j)

    def adopted(E, m):
        rp = pr.recover_pose(E, a, b, Ks, mask=m)
        proj = np.stack([Ks @ np.eye(3, 4), Ks @ np.hstack([rp["R"], np.reshape(rp["t"], (3, 1))])]).reshape(2, 12)
        cam = np.full(35, -1, np.int32)
        cam[i], cam[j] = 0, 1
        out = tr.triangulate(proj, cam, T.kp_ptr, kp_xy, T.track_ptr, T.image, T.keypoint, min_views=2, refine_iters=5,
                             max_error=4.0, min_angle_deg=1.0)
        return int((out["status"] == tr.OK).sum())
    ref = er.ransac(a, b, Ks, er.draw_samples(0, 0, len(a), 1024), THR, refine=True)
    chain = adopted(ref["E"], ref["mask"])
    k = int(np.flatnonzero((pairs == (i, j)).all(1))[0])
    F = er.shipped_pairs()[k][2]
    chain_f = adopted(Ks.T @ F @ Ks, fr.inliers(F, a, b, THR))
    own = fr.ransac(a, b, fr.draw_samples(0, 0, len(a), 1024), THR, refine=True)
    chain_own = adopted(Ks.T @ own["F"] @ Ks, own["mask"])
    rec = reconstruct_tracks(T, kps, Ks, initial_pair=(i, j), initial_model="essential", refine_initial_pair=False,
                             min_visible=10 ** 9)                          # no image qualifies: the loop ends after step 0
    got = rec.log[0]["points_added"]
    print(f"initial pair {(i, j)}, {len(a)} common tracks: step 0 adopts {got}; NumPy chain: five-point {chain}, "
          f"K^T F K of the shipped F {chain_f}, of this project's refitted F {chain_own}")
    assert rec.log[0]["initial_model"] == "essential" and rec.order == [i, j]
    assert chain > 0 and 2 * chain_f < chain
    assert got >= 0.9 * chain
