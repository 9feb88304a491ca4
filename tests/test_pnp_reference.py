"""CPU tests of the PnP RANSAC's NumPy reference (tests/pnp_reference.py), of the 3-slot restatement of the sample
generator, of the kernel's P3P solver built for the host (sfm_amd/csrc/pnp_solve.h) against that reference, and of
the Python glue of sfm_amd.pnp with the library calls stubbed.  No GPU."""
import functools
import os

import numpy as np
import pytest

import pnp_reference as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = pr.K_REF
THR = 8.0


@functools.lru_cache(maxsize=None)
def shipped():
    """[(image id, X [M,3] float64, uv [M,2] float32, shipped R, shipped t)] for images 3, 12, 20, 33."""
    d = np.load(os.path.join(GOLDEN, "driver_bunny.npz"), allow_pickle=False)
    s = np.load(os.path.join(GOLDEN, "bunny_state.npz"), allow_pickle=False)
    ids = list(s["ids"])
    return [(int(im), d[f"f{im}_points3D"], d[f"f{im}_points2D"], s["R"][ids.index(im)], s["t"][ids.index(im)])
            for im in d["f_images"]]


# ------------------------------------------------------------------------------------------- the generator
def test_generator_indices_in_range_and_distinct():
    for M in (4, 5, 40, 5000):
        s = pr.draw_samples(3, 2, M, 1024)
        assert s.shape == (1024, 3) and s.dtype == np.int32
        assert s.min() >= 0 and s.max() < M
        srt = np.sort(s, axis=1)
        assert (srt[:, 1:] != srt[:, :-1]).all()
    assert (pr.draw_samples(3, 2, 3, 16) == -1).all()


def test_generator_is_a_function_of_seed_segment_hypothesis():
    a = pr.draw_samples(5, 3, 40, 256)
    assert np.array_equal(a, pr.draw_samples(5, 3, 40, 256))
    assert np.array_equal(a[:64], pr.draw_samples(5, 3, 40, 64))          # the prefix property in n_hyp
    assert not np.array_equal(a, pr.draw_samples(6, 3, 40, 256))          # the seed matters
    assert not np.array_equal(a, pr.draw_samples(5, 4, 40, 256))          # the segment index matters
    assert not np.array_equal(a, pr.draw_samples(5, 3, 41, 256))          # the point count matters
    batch = [pr.draw_samples(5, s, m, 256) for s, m in enumerate([10, 300, 4, 40])]
    assert np.array_equal(batch[3], a)                                    # other segments do not
    # the first slots are those of the 7-slot generator of the fundamental-matrix RANSAC: one generator, fewer slots
    import fundamental_reference as fr
    assert np.array_equal(a, fr.draw_samples(5, 3, 40, 256)[:, :3])


def test_device_generator_on_the_host_equals_the_numpy_generator(tmp_path):
    """draw_distinct<3> and draw_distinct<7> of ransac_common.h compiled by g++ against the NumPy generator
    (tests/ransac_reference.py), index for index: 64 hypotheses at M = size (where duplicate rejection runs longest), just above it and at 1000, for two
    seeds (one >= 2^63: the wrapping arithmetic) and segments 0 and 147."""
    import shutil
    import subprocess
    import fundamental_reference as fr
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "ransac_common_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "ransac_common_check.cpp"), "-o", exe], check=True)
    cases = [(size, seed, seg, M, 64) for size, Ms in ((3, (4, 5, 1000)), (7, (7, 8, 1000))) for M in Ms
             for seed in (12345, 2 ** 63 + 0x1234567) for seg in (0, 147)]
    np.array(cases, dtype=np.uint64).tofile(exe + ".in")
    subprocess.run([exe, exe + ".in", exe + ".out"], check=True)
    got, at = np.fromfile(exe + ".out", dtype=np.int32), 0
    for size, seed, seg, M, H in cases:
        want = (pr if size == 3 else fr).draw_samples(seed, seg, M, H)
        assert np.array_equal(got[at:at + H * size].reshape(H, size), want), (size, seed, seg, M)
        at += H * size
    assert at == len(got)


# ---------------------------------------------------------------------------------------- the minimal solver
def test_noise_free_view_every_sample_recovers_the_pose():
    """No noise, no outliers (pixels rounded to float32, 3e-5 px): every hypothesis reaches all M points at 0.01 px."""
    X, uv, R, t = pr.synth_view(np.random.default_rng(0), 50, 0.0, noise=0.0)
    r = pr.ransac(X, uv, K, pr.draw_samples(0, 0, 50, 64), threshold=0.01)
    print("noise-free: hypotheses with all 50 inliers:", int((r["hyp_count"] == 50).sum()), "of 64")
    assert r["status"] == 0 and (r["hyp_count"] == 50).all()
    assert np.abs(r["R"] - R).max() < 1e-6 and np.abs(r["t"] - t).max() < 1e-5
    assert abs(np.linalg.det(r["R"]) - 1) < 1e-12


def test_degenerate_samples_give_no_model():
    X, uv, _, _ = pr.synth_view(np.random.default_rng(1), 20, 0.0)
    f = pr.bearings(uv, K)
    assert len(pr.p3p(X[[0, 1, 2]], f[[0, 1, 2]])) >= 1
    assert pr.p3p(X[[0, 1, 0]], f[[0, 1, 2]]) == []                        # bit-identical 3-D points
    line = X[0] + np.outer([0.0, 0.4, 1.0], X[1] - X[0])                   # a collinear triple
    assert pr.p3p(line, f[[0, 1, 2]]) == []
    bad = X[[0, 1, 2]].copy()
    bad[1, 2] = np.nan
    assert pr.p3p(bad, f[[0, 1, 2]]) == []
    same = np.tile(X[:1], (12, 1))                                         # all points identical: status 2
    r = pr.ransac(same, uv[:12], K, pr.draw_samples(0, 0, 12, 32))
    assert r["status"] == 2 and r["R"] is None and r["n_inliers"] == 0 and not r["mask"].any()
    assert pr.ransac(X[:3], uv[:3], K, pr.draw_samples(0, 0, 3, 8))["status"] == 1


def test_non_finite_points_are_never_inliers():
    X, uv, R, t = pr.synth_view(np.random.default_rng(2), 60, 0.2)
    X, uv = X.copy(), uv.copy()
    X[7, 1] = np.nan
    X[9, 2] = np.inf
    uv[11, 0] = np.inf
    uv[13] = [np.nan, -np.inf]
    with np.errstate(invalid="ignore", over="ignore"):
        r = pr.ransac(X, uv, K, pr.draw_samples(0, 0, 60, 128))
    assert r["status"] == 0 and r["n_inliers"] >= 40
    assert not r["mask"][[7, 9, 11, 13]].any()
    assert not pr.inliers(K, R, t, X, uv.astype(np.float64), THR)[[7, 9, 11, 13]].any()


def test_refit_keeps_the_count_and_is_no_worse_than_the_true_pose():
    """ransac(refine=True): the count is not lower than without the refit, and on the five synthetic cases with M >= 4
    the refined pose's summed squared reprojection error over the winner's inlier set is <= the TRUE pose's on the same
    set (a converged least-squares fit cannot be worse than any fixed pose; the unrefined P3P winner is 1.2 - 6 x worse
    than the truth, so the check has teeth)."""
    Xs, uvs, Rs, ts = pr.synth_batch()
    for s, (M, share) in enumerate(pr.CASES):
        if M < 4:
            continue
        X, uv = Xs[s], uvs[s].astype(np.float64)
        smp = pr.draw_samples(1, s, M, 512)
        a = pr.ransac(X, uv, K, smp, THR, refine=False)
        b = pr.ransac(X, uv, K, smp, THR, refine=True)
        assert np.array_equal(a["hyp_count"], b["hyp_count"])
        assert b["refined"] and b["n_inliers"] >= a["n_inliers"] and b["n_inliers"] == b["mask"].sum()
        m = a["mask"]
        cw, ct, cr = (pr.cost(K, R, t, X[m], uv[m]) for R, t in ((a["R"], a["t"]), (Rs[s], ts[s]), (b["R"], b["t"])))
        print(f"M {M} share {share}: winner {a['n_inliers']} refined {b['n_inliers']}; cost over the winner's inliers: "
              f"winner {cw:.4g} truth {ct:.4g} refined {cr:.4g}")
        assert cr <= ct and cr <= cw


def test_share_of_unstable_hypotheses():
    """Share of hypotheses whose count changes under a 1e-13 relative change of X: at most 3 % on every shipped segment
    (seed 0, 1,024 hypotheses) and none on the synthetic cases (seed 1, 512).  A condition on the inputs of the GPU
    replay test, which compares on the stable hypotheses only."""
    for s, (im, X, uv, _, _) in enumerate(shipped()):
        st = pr.stable(X, uv, K, pr.draw_samples(0, s, len(X), 1024), THR)
        print(f"image {im} ({len(X)} matches): unstable share {1 - st.mean():.4%}")
        assert 1 - st.mean() <= 0.03, im
    Xs, uvs, _, _ = pr.synth_batch()
    for s, (M, share) in enumerate(pr.CASES):
        st = pr.stable(Xs[s], uvs[s], K, pr.draw_samples(1, s, M, 512), THR)
        print(f"synthetic M {M} share {share}: unstable share {1 - st.mean():.4%}")
        assert st.all(), (M, share)


# ---------------------------------------------------------------------- the kernel's solver built for the host
@functools.lru_cache(maxsize=None)
def native_solver(tmp):
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        return None
    exe = os.path.join(tmp, "pnp_solve_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "pnp_solve_check.cpp"), "-o", exe], check=True)

    def run(P, f):
        import subprocess
        np.concatenate([P.reshape(-1, 9), f.reshape(-1, 9)], 1).tofile(exe + ".in")
        subprocess.run([exe, exe + ".in", exe + ".out"], check=True)
        o = np.fromfile(exe + ".out").reshape(-1, 49)
        return o[:, 0].astype(int), o[:, 1:].reshape(-1, 4, 3, 4)
    return run


def native_hyp_count(run, X, uv, smp):
    f = pr.bearings(uv, K)
    filled, Rt = run(np.ascontiguousarray(X[smp]), np.ascontiguousarray(f[smp]))
    hc = np.zeros(len(smp), np.int32)
    for h in range(len(smp)):
        for c in range(4):
            if filled[h] >> c & 1:
                R = Rt[h, c, :, :3]
                assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
                hc[h] = max(hc[h], pr.inliers(K, R, Rt[h, c, :, 3], X, uv, THR).sum())
    return hc


def test_kernel_p3p_solver_on_the_host_equals_the_reference(tmp_path_factory):
    """pnp_solve.h compiled by g++: per hypothesis the best count of its candidates equals the reference's on every
    hypothesis of the synthetic cases, and on at least 99 % of the stable hypotheses of every shipped segment - the
    bounds the GPU replay test sets for the kernel, here for its solver alone.  Degenerate samples fill no slot."""
    run = native_solver(str(tmp_path_factory.mktemp("native")))
    if run is None:
        pytest.skip("no g++")
    Xs, uvs, _, _ = pr.synth_batch()
    for s, (M, share) in enumerate(pr.CASES):
        if M < 4:
            continue
        X, uv = Xs[s], uvs[s].astype(np.float64)
        smp = pr.draw_samples(1, s, M, 512)
        agree = float(np.mean(native_hyp_count(run, X, uv, smp) == pr.ransac(X, uv, K, smp, THR)["hyp_count"]))
        print(f"synthetic M {M} share {share}: equal on {agree:.4%}")
        assert agree == 1.0
    for s, (im, X, uv, _, _) in enumerate(shipped()):
        uv = uv.astype(np.float64)
        smp = pr.draw_samples(0, s, len(X), 1024)
        st = pr.stable(X, uv, K, smp, THR)
        eq = native_hyp_count(run, X, uv, smp) == pr.ransac(X, uv, K, smp, THR)["hyp_count"]
        print(f"image {im}: equal on {eq[st].mean():.4%} of the stable hypotheses, {eq.mean():.4%} of all")
        assert eq[st].mean() >= 0.99, im
    X = Xs[3]
    f = pr.bearings(uvs[3], K)
    line = X[0] + np.outer([0.0, 0.4, 1.0], X[1] - X[0])
    nan = X[:3].copy()
    nan[2, 0] = np.nan
    filled, Rt = run(np.stack([X[[0, 1, 0]], line, nan]), np.stack([f[:3]] * 3))
    assert (filled == 0).all() and (Rt == 0).all()


# ----------------------------------------------------------------------------- Python glue, library stubbed
class _StubLib:
    def sfm_pnp_workspace_bytes(self, n, n_seg, n_hyp, out):
        out._obj.value = 256
        return 0


class _StubHandle:
    def __init__(self):
        self.lib = _StubLib()
        self.calls = []

    def check(self, rc, what):
        assert rc == 0

    def call(self, name, *args):
        self.calls.append(name)
        getattr(self, name)(*args)


@pytest.fixture
def stubbed(monkeypatch):
    """solve_pnp_ransac_batched with torch on the CPU and the two library calls answered by the reference."""
    import ctypes
    import torch
    from sfm_amd import _lib, pnp
    h = _StubHandle()

    def as_np(ptr, shape, dtype):
        n = int(np.prod(shape))
        if n == 0 or not ptr.value:
            return np.zeros(shape, dtype)
        buf = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def draw(seg_ptr, n_seg, n_hyp, seed, samples):
        ptr = as_np(seg_ptr, (n_seg + 1,), np.int64)
        out = as_np(samples, (n_seg, n_hyp, 3), np.int32)
        for s in range(n_seg):
            out[s] = pr.draw_samples(seed.value, s, int(ptr[s + 1] - ptr[s]), n_hyp)

    def ransac(seg_ptr, n_seg, X, uv, n, Kseg, samples, n_hyp, thr, refine, Rt, mask, n_inl, status, hyp_count, refined, ws, nb):
        ptr = as_np(seg_ptr, (n_seg + 1,), np.int64)
        pX, puv, k4 = as_np(X, (n, 3), np.float64), as_np(uv, (n, 2), np.float32), as_np(Kseg, (n_seg, 4), np.float64)
        smp = as_np(samples, (n_seg, n_hyp, 3), np.int32)
        oR, om = as_np(Rt, (n_seg, 12), np.float64), as_np(mask, (n,), np.uint8)
        oi, os_, orf = (as_np(x, (n_seg,), np.int32) for x in (n_inl, status, refined))
        oc = as_np(hyp_count, (n_seg, n_hyp), np.int32) if hyp_count.value else None
        for s in range(n_seg):
            b, e = int(ptr[s]), int(ptr[s + 1])
            r = pr.ransac(pX[b:e], puv[b:e], pr.k_matrix(k4[s]), smp[s] if e - b >= 4 else np.zeros((n_hyp, 3), int),
                          thr.value, bool(refine))
            oR[s] = 0.0 if r["R"] is None else np.c_[r["R"], r["t"]].ravel()
            om[b:e] = r["mask"]
            oi[s], os_[s], orf[s] = r["n_inliers"], r["status"], int(r["refined"])
            if oc is not None:
                oc[s] = r["hyp_count"]

    h.sfm_pnp_draw_samples, h.sfm_pnp_ransac = draw, ransac
    monkeypatch.setattr(_lib, "get_handle", lambda device=0: h)
    real_device = torch.device
    monkeypatch.setattr(torch, "device", lambda *a, **k: real_device("cpu"))
    return pnp, h


def test_glue_short_segments_shapes_and_dtypes(stubbed):
    from sfm_amd.rotation import rodrigues
    pnp, h = stubbed
    rng = np.random.default_rng(0)
    X, uv, R, t = pr.synth_view(rng, 60, 0.2)
    Y, vw, _, _ = pr.synth_view(rng, 3, 0.0)
    res, dbg = pnp.solve_pnp_ransac_batched([X, Y, X[:0]], [uv, vw, uv[:0]], K, n_hypotheses=64, return_debug=True)
    assert h.calls == ["sfm_pnp_draw_samples", "sfm_pnp_ransac"]            # one of each for the whole list
    ok, rvec, tvec, inl = res[0]
    assert ok is True and rvec.shape == (3, 1) and tvec.shape == (3, 1) and rvec.dtype == tvec.dtype == np.float64
    assert inl.dtype == np.int32 and inl.shape == (dbg[0]["n_inliers"], 1) and (np.diff(inl[:, 0]) > 0).all()
    assert np.abs(rodrigues(rvec) - dbg[0]["R"]).max() < 1e-12 and np.array_equal(tvec.ravel(), dbg[0]["t"])
    assert np.abs(rodrigues(rvec) - R).max() < 1e-2 and np.abs(tvec.ravel() - t).max() < 5e-2
    assert res[1] == (False, None, None, None) and res[2] == (False, None, None, None)
    assert [d["status"] for d in dbg] == [0, 1, 1] and dbg[1]["R"] is None
    assert dbg[0]["samples"].shape == (64, 3) and dbg[0]["hyp_count"].shape == (64,)
    assert dbg[0]["n_inliers"] >= dbg[0]["hyp_count"].max()
    assert np.array_equal(dbg[0]["samples"], pr.draw_samples(0, 0, 60, 64))
    # explicit samples replace the draw; the single-segment form; K per segment
    smp = pr.draw_samples(9, 0, 60, 64)
    h.calls.clear()
    (ok2, r2, t2, i2), d2 = pnp.solve_pnp_ransac(X, uv, K, n_hypotheses=64, samples=smp, return_debug=True)
    assert h.calls == ["sfm_pnp_ransac"] and ok2 and np.array_equal(d2["samples"], smp)
    per = pnp.solve_pnp_ransac_batched([X, X], [uv, uv], np.stack([K, K]), n_hypotheses=64, samples=[smp, smp])
    assert np.array_equal(per[0][1], r2) and np.array_equal(per[1][3], i2)
    assert pnp.solve_pnp_ransac(Y, vw, K, n_hypotheses=64) == (False, None, None, None)
    assert pnp.solve_pnp_ransac_batched([], [], K) == []
    h.calls.clear()
    assert pnp.solve_pnp_ransac_batched([X[:0]], [uv[:0]], K) == [(False, None, None, None)] and h.calls == []


def test_glue_argument_errors(stubbed):
    pnp, _ = stubbed
    X, uv, _, _ = pr.synth_view(np.random.default_rng(1), 20, 0.0)
    good = pr.draw_samples(0, 0, 20, 8)
    f = pnp.solve_pnp_ransac_batched
    with pytest.raises(ValueError):
        f([X], [uv, uv], K)
    with pytest.raises(ValueError):
        f([X], [uv[:5]], K)
    with pytest.raises(ValueError):
        f([X], [uv], K, n_hypotheses=0)
    with pytest.raises(ValueError):
        f([X], [uv], K, threshold=float("nan"))
    with pytest.raises(ValueError):
        f([X], [uv], K, threshold=-1.0)
    with pytest.raises(ValueError):
        f([X], [uv], K, seed=-1)
    with pytest.raises(ValueError):
        f([X], [uv], K, seed=2 ** 64)
    with pytest.raises(ValueError):
        f([X], [uv], np.stack([K, K]))
    with pytest.raises(ValueError):
        f([X], [uv], K[:2])
    for bad in (good[:4], good.astype(np.float64), np.where(good == good[0, 0], 20, good),
                np.where(good == good[0, 0], -1, good), np.repeat(good[:, :1], 3, axis=1)):
        with pytest.raises(ValueError):
            f([X], [uv], K, n_hypotheses=8, samples=[bad])
    with pytest.raises(ValueError):
        f([X], [uv], K, n_hypotheses=8, samples=[good, good])


def test_pnp_ransac_candidates_applies_min_inliers_and_leaves_the_poses_alone(stubbed, monkeypatch):
    from sfm_amd.reconstruction import StructureFromMotion
    pnp, h = stubbed
    rng = np.random.default_rng(3)
    X, uv, R, t = pr.synth_view(rng, 80, 0.25)
    few = pr.synth_view(rng, 12, 0.0)                                     # registers, but under pnp_min_inliers
    answers = {5: (X, uv), 6: (few[0], few[1]), 7: (np.array([]), np.array([])), 8: (X[:3], uv[:3])}
    sfm = StructureFromMotion()
    sfm.pnp_hypotheses = 64
    assert sfm.pnp_threshold == 8.0 and sfm.pnp_min_inliers == 15 and sfm.pnp_seed == 0 and StructureFromMotion.pnp_hypotheses == 1024
    assert not hasattr(sfm, "pnp_ransac")
    sfm.poses = {0: (np.eye(3), np.zeros(3))}
    monkeypatch.setattr(sfm, "find_2d3d_matches", lambda image_id: answers[image_id])
    out = sfm.pnp_ransac_candidates([5, 6, 7, 8])
    assert h.calls.count("sfm_pnp_ransac") == 1 and list(out) == [5, 6, 7, 8]
    assert out[6] is None and out[7] is None and out[8] is None
    Rg, tg, inl = out[5]
    assert Rg.shape == (3, 3) and tg.shape == (3, 1) and inl.dtype == np.int32 and inl.shape[1] == 1
    assert len(inl) >= 0.9 * pr.inliers(K, R, t, X, uv.astype(np.float64), THR).sum()
    assert np.abs(Rg - R).max() < 1e-2
    assert list(sfm.poses) == [0]
    sfm.pnp_min_inliers = 5
    assert sfm.pnp_ransac_candidates([6])[6] is not None
    ok, rvec, tvec, inl1 = sfm.solve_pnp_ransac(X, uv)                    # the stand-in for the cv2 call
    assert ok and rvec.shape == (3, 1) and np.array_equal(inl1, inl)


def test_without_a_gpu_solve_pnp_ransac_raises():
    import torch
    from sfm_amd import _lib, pnp
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    X, uv, _, _ = pr.synth_view(np.random.default_rng(4), 20, 0.0)
    with pytest.raises(_lib.SfmError):
        pnp.solve_pnp_ransac(X, uv, K)
