"""CPU tests of the fundamental-matrix RANSAC's NumPy reference (tests/fundamental_reference.py), of the restated
sample generator, of the reference on the 148 pairs the reference project ships, of the kernel's solver and error rule
(sfm_amd/csrc/fundamental_solve.h, fundamental_rule.h) compiled for the host against the reference, hypothesis by
hypothesis, and of the Python glue of sfm_amd.twoview / ImageMatcher.process_pairs with the library calls stubbed.
No GPU."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import fundamental_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
THR = 3.0


@functools.lru_cache(maxsize=None)
def bunny_pairs():
    g = np.load(os.path.join(GOLDEN, "bunny_pairs.npz"), allow_pickle=False)
    off = g["offsets"]
    return [(g["pts1"][off[s]:off[s + 1]], g["pts2"][off[s]:off[s + 1]], g["F"][s], g["mask"][off[s]:off[s + 1]])
            for s in range(len(g["F"]))]


@functools.lru_cache(maxsize=None)
def bunny_replay():
    """[(samples, reference result)] of the 148 shipped pairs at seed 0, 1,024 hypotheses, no refit - computed once,
    never modified."""
    out = []
    for s, (p1, p2, _, _) in enumerate(bunny_pairs()):
        smp = fr.draw_samples(0, s, len(p1), 1024)
        out.append((smp, fr.ransac(p1, p2, smp, THR)))
    return out


@functools.lru_cache(maxsize=None)
def synthetic_replay():
    """[(samples, reference result)] of fr.CASES at seed 1, 512 hypotheses - computed once, never modified."""
    p1s, p2s, _ = fr.synth_batch()
    out = []
    for s, (M, _) in enumerate(fr.CASES):
        smp = fr.draw_samples(1, s, M, 512)
        out.append((smp, fr.ransac(p1s[s], p2s[s], smp, THR)))
    return out


# ---------------------------------------------------------------------------------------- noise-free scenes
@pytest.mark.parametrize("M", [40, 300])
def test_noise_free_scene_every_sample_recovers_the_true_model(M):
    """Float64, no noise, no outliers: every sample's best candidate fits all M points at 1e-6 px, and the winner is
    K^-T [t]x R K^-1 scaled to F[2][2] = 1 within 1e-8 of the largest entry."""
    rng = np.random.default_rng(M)
    p1, p2, Ft = fr.synth_pair(rng, M, 0.0, noise=0.0, float32=False)
    smp = fr.draw_samples(1, 0, M, 512)
    r = fr.ransac(p1, p2, smp, threshold=1e-6)
    assert r["status"] == 0
    print("noise-free M", M, "hypotheses with all inliers", int((r["hyp_count"] == M).sum()), "of 512")
    assert (r["hyp_count"] == M).all()
    dev = np.abs(r["F"] - Ft).max() / np.abs(Ft).max()
    print("winner against the true F, relative to the largest entry:", dev)
    assert dev < 1e-8
    assert r["F"][2, 2] == 1.0 and r["n_inliers"] == M


# ------------------------------------------------------------------------------------------- the generator
def test_generator_indices_in_range_and_distinct():
    for M in (7, 8, 40, 5000):
        s = fr.draw_samples(3, 2, M, 1024)
        assert s.shape == (1024, 7) and s.dtype == np.int32
        assert s.min() >= 0 and s.max() < M
        srt = np.sort(s, axis=1)
        assert (srt[:, 1:] != srt[:, :-1]).all()
    assert (fr.draw_samples(3, 2, 6, 16) == -1).all()


def test_generator_is_a_function_of_seed_segment_hypothesis():
    a = fr.draw_samples(5, 3, 40, 256)
    assert np.array_equal(a, fr.draw_samples(5, 3, 40, 256))
    assert np.array_equal(a[:64], fr.draw_samples(5, 3, 40, 64))          # not of the hypothesis count
    assert not np.array_equal(a, fr.draw_samples(6, 3, 40, 256))          # the seed matters
    assert not np.array_equal(a, fr.draw_samples(5, 4, 40, 256))          # the segment index matters
    # a segment's samples do not change when other segments are added: nothing but (seed, segment, n_points) enters
    batch = [fr.draw_samples(5, s, m, 256) for s, m in enumerate([10, 300, 7, 40])]
    assert np.array_equal(batch[3], a)
    assert np.array_equal(fr.mix64(np.array([0, 1], dtype=np.uint64)),
                          np.array([0xE220A8397B1DCDAF, 0x910A2DEC89025CC1], dtype=np.uint64))   # splitmix64's first outputs


def test_generator_is_uniform_over_a_40_point_segment():
    """1,024 hypotheses of a 40-point segment: each index appears in a sample with probability 7/40; the count over the
    hypotheses is binomial, and every index lies within 5 standard deviations of the uniform share."""
    H, M = 1024, 40
    for seed, seg in ((0, 0), (1, 17)):
        s = fr.draw_samples(seed, seg, M, H)
        cnt = np.bincount(s.ravel(), minlength=M)
        mean, sd = H * 7 / M, np.sqrt(H * (7 / M) * (1 - 7 / M))
        z = (cnt - mean) / sd
        print("seed", seed, "segment", seg, "largest deviation in standard deviations:", np.abs(z).max())
        assert np.abs(z).max() < 5.0


# ------------------------------------------------------------------------------------------ shipped pairs
def test_shipped_pairs_winner_is_as_good_as_the_shipped_model():
    """148 shipped pairs, 1,024 hypotheses, seed 0, the restated generator: every pair's winner has at least 0.9 x as
    many inliers under the reference's verification rule (symmetric distance < 3, the shipped mask) as the shipped F.
    Measured: minimum ratio 1.000, median 1.030 (the bound is set by the issue's three-seed survey, minimum 0.953)."""
    ratios = []
    for s, ((p1, p2, Fs, mk), (_, r)) in enumerate(zip(bunny_pairs(), bunny_replay())):
        p1 = p1.astype(np.float64)
        p2 = p2.astype(np.float64)
        assert r["status"] == 0, s
        mine = int((fr.sym_err(r["F"], p1, p2) < 3.0).sum())
        ship = int((fr.sym_err(Fs, p1, p2) < 3.0).sum())
        assert abs(ship - int(mk.sum())) <= 1, (s, ship, int(mk.sum()))          # float64 against the shipped float32 mask
        ratios.append(mine / ship)
    ratios = np.array(ratios)
    print("winner / shipped verification inliers: min %.3f (pair %d) median %.3f" %
          (ratios.min(), int(ratios.argmin()), np.median(ratios)))
    assert ratios.min() >= 0.9


def test_refit_keeps_or_improves_the_count():
    rng = np.random.default_rng(5)
    p1, p2, Ft = fr.synth_pair(rng, 300, 0.3)
    smp = fr.draw_samples(0, 0, 300, 256)
    a = fr.ransac(p1, p2, smp, refine=False)
    b = fr.ransac(p1, p2, smp, refine=True)
    assert np.array_equal(a["hyp_count"], b["hyp_count"])
    assert b["n_inliers"] >= a["n_inliers"] and b["n_inliers"] == b["mask"].sum()
    sv = np.linalg.svd(b["F"], compute_uv=False)
    assert sv[2] < 1e-12 * sv[0] and b["F"][2, 2] == 1.0


# ------------------------------------------------------- the kernel's solver and rule built for the host
def build_native(tmp, extra=()):
    exe = os.path.join(tmp, "fundamental_solve_check" + ("_san" if extra else ""))
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "fundamental_solve_check.cpp"), "-o", exe], check=True)
    return exe


def transforms(p1, p2):
    """The segment's {sc1, cx1, cy1, sc2, cx2, cy2} as the reference forms them: over the finite matches."""
    a, b = np.asarray(p1, np.float64).reshape(-1, 2), np.asarray(p2, np.float64).reshape(-1, 2)
    fin = np.isfinite(a).all(1) & np.isfinite(b).all(1)
    T1, T2 = (fr.hartley(a[fin]), fr.hartley(b[fin])) if fin.any() else (np.eye(3), np.eye(3))
    return [T1[0, 0], -T1[0, 2] / T1[0, 0], -T1[1, 2] / T1[0, 0], T2[0, 0], -T2[0, 2] / T2[0, 0], -T2[1, 2] / T2[0, 0]]


def run_native(exe, p1, p2, smp, t=None):
    """(model [H,3] bool, F [H,3,3,3], count [H,3]) of the host build for samples smp of one pair, under transforms t
    (the reference's for this pair when None)."""
    a = np.asarray(p1, np.float32).astype(np.float64).reshape(-1, 2)
    b = np.asarray(p2, np.float32).astype(np.float64).reshape(-1, 2)
    t = transforms(a, b) if t is None else t
    np.concatenate([[len(a), len(smp), THR], t, np.c_[a, b].ravel(), np.asarray(smp, np.float64).ravel()]).tofile(exe + ".in")
    subprocess.run([exe, exe + ".in", exe + ".out"], check=True)
    o = np.fromfile(exe + ".out").reshape(-1, 33)
    return o[:, :3] != 0, o[:, 3:30].reshape(-1, 3, 3, 3), o[:, 30:].astype(int)


def check_rules(exe, p1, p2):
    """The rule cases on one pair of M >= 7 matches (copies are modified, never p1 / p2)."""
    M = len(p1)
    plain = np.arange(7)[None]
    model, Fs, cnt = run_native(exe, p1, p2, plain)
    assert model[0].any() and cnt[0].max() >= 7                       # a plain sample fits at least its own seven
    # a NaN and an infinity in a sampled match void all three candidates.  Match 0 with a bad y is the case the
    # pivot test alone does not see: row 0 meets no earlier rotation, its pivot xc * xa stays finite, and a rotation
    # that treated a NaN length as zero, (c, s) = (1, 0), would drop the NaN that stands in the row's other entries.
    for row, img, col, bad in [(0, 0, 1, np.nan), (0, 1, 1, np.nan), (0, 1, 1, np.inf), (1, 0, 0, np.nan), (3, 1, 1, np.inf),
                               (5, 0, 1, -np.inf), (6, 1, 0, np.nan), (6, 1, 1, np.inf)]:
        q = [p1.copy(), p2.copy()]
        q[img][row, col] = bad
        model, Fs, cnt = run_native(exe, q[0], q[1], plain)
        assert not model.any() and (cnt == 0).all(), (M, row, img, col, bad)
    # an index of -1 and an index of M void the sample and read nothing
    model, Fs, cnt = run_native(exe, p1, p2, np.array([[0, 1, 2, 3, 4, 5, M], [0, 1, 2, -1, 4, 5, 6]]))
    assert not model.any() and (cnt == 0).all(), M
    # a non-finite match that is not sampled is never counted: the last match made non-finite, against the same
    # samples on the pair without it, under the same transforms (they leave non-finite matches out).  At M = 7 a sample
    # of the other six repeats one of them - neither the kernel nor this program asks for distinct indices.
    smp = fr.draw_samples(2, 0, M - 1, 64) if M > 7 else np.array([[0, 1, 2, 3, 4, 5, 5], [3, 0, 1, 2, 3, 4, 5]])
    for bad in (np.nan, np.inf):
        q1, q2 = p1.copy(), p2.copy()
        q1[M - 1, 1] = bad
        t = transforms(q1, q2)
        with_it, F_with, cnt_with = run_native(exe, q1, q2, smp, t)
        without, F_without, cnt_without = run_native(exe, q1[:M - 1], q2[:M - 1], smp, t)
        assert np.array_equal(cnt_with, cnt_without) and np.array_equal(F_with, F_without), M
        assert (cnt_with <= M - 1).all() and (M == 7 or cnt_with.max() >= 7)


def check_native(exe):
    p1s, p2s, _ = fr.synth_batch()
    for s, ((M, share), (smp, ref)) in enumerate(zip(fr.CASES, synthetic_replay())):
        model, Fs, cnt = run_native(exe, p1s[s], p2s[s], smp)
        hyp = cnt.max(1)
        agree = float(np.mean(hyp == ref["hyp_count"]))
        cand = float(np.mean(np.sort(cnt, 1) == np.sort(ref["cand_count"], 1)))     # the slot order is the basis's
        print(f"segment {s} (M {M}, outliers {share}): hyp_count equal on {agree:.4%} of 512, per candidate {cand:.4%}, "
              f"winner {hyp.max()} / reference {ref['n_inliers']}")
        assert agree >= 0.99, s
        assert hyp.max() == ref["n_inliers"], s
        assert (cnt[~model] == 0).all(), s            # the program's model flag is "F != 0": the empty slot never counts
    check_rules(exe, p1s[2], p2s[2])          # M = 40
    check_rules(exe, p1s[0], p2s[0])          # M = 7
    # the shipped pairs: printed, nothing asserted.  The reference takes its null space from np.linalg.svd and this
    # build rotates columns (with the fmas the solver writes out, nothing else contracted); on the ill-conditioned
    # samples of real matches the two round apart.
    agree, winners = [], 0
    for (p1, p2, _, _), (smp, ref) in zip(bunny_pairs(), bunny_replay()):
        _, _, cnt = run_native(exe, p1, p2, smp)
        agree.append(float(np.mean(cnt.max(1) == ref["hyp_count"])))
        winners += int(cnt.max() == ref["hyp_count"].max())
    print("shipped pairs: per-hypothesis agreement min %.4f median %.4f max %.4f; winner count equal on %d of %d"
          % (min(agree), float(np.median(agree)), max(agree), winners, len(agree)))


def test_kernel_solver_and_rule_on_the_host_equal_the_reference(tmp_path):
    """fundamental_solve.h + fundamental_rule.h compiled by g++ -ffp-contract=off (the fmas the solver writes out stay
    fmas): hyp_count equals the reference's on at
    least 99 % of the 512 hypotheses of every case of the GPU test's batch - the cap the GPU replay test sets for the
    kernels, here for their solver and rule alone - and the winner's count equals the reference's; then the rule cases
    at M = 40 and M = 7.  Measured: 100 % in all six cases, per candidate too.  On the 148 shipped pairs the agreement is
    printed only: between 0.73 and 1.00 per pair (median 0.95), one winner count of 148 differs."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    check_native(build_native(str(tmp_path)))


def test_kernel_solver_and_rule_on_the_host_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run as the stand-alone program it is: every index of
    the 35 rotations and of the rows stays inside its array, and nothing undefined happens on the way."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    check_native(build_native(str(tmp_path), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")))


# ----------------------------------------------------------------------------- Python glue, library stubbed
class _StubLib:
    """Stands in for libsfm_amd.so: records calls and answers sfm_fund_ransac from the NumPy reference."""

    def __init__(self):
        self.calls = []

    def sfm_fund_workspace_bytes(self, n, n_seg, n_hyp, out):
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
    """estimate_fundamental_batched with torch on the CPU and the two library calls answered by the reference."""
    import ctypes
    import torch
    from sfm_amd import _lib, twoview
    h = _StubHandle()

    def as_np(ptr, shape, dtype):
        n = int(np.prod(shape))
        if n == 0 or not ptr.value:
            return np.zeros(shape, dtype)
        buf = (ctypes.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def draw(seg_ptr, n_seg, n_hyp, seed, samples):
        ptr = as_np(seg_ptr, (n_seg + 1,), np.int64)
        out = as_np(samples, (n_seg, n_hyp, 7), np.int32)
        for s in range(n_seg):
            out[s] = fr.draw_samples(seed.value, s, int(ptr[s + 1] - ptr[s]), n_hyp)

    def ransac(seg_ptr, n_seg, pts1, pts2, n, samples, n_hyp, thr, refine, F, mask, n_inl, status, hyp_count, refined, ws, nb):
        ptr = as_np(seg_ptr, (n_seg + 1,), np.int64)
        p1, p2 = as_np(pts1, (n, 2), np.float32), as_np(pts2, (n, 2), np.float32)
        smp = as_np(samples, (n_seg, n_hyp, 7), np.int32)
        oF, om = as_np(F, (n_seg, 9), np.float64), as_np(mask, (n,), np.uint8)
        oi, os_, orf = (as_np(x, (n_seg,), np.int32) for x in (n_inl, status, refined))
        oc = as_np(hyp_count, (n_seg, n_hyp), np.int32) if hyp_count.value else None
        for s in range(n_seg):
            b, e = int(ptr[s]), int(ptr[s + 1])
            r = fr.ransac(p1[b:e], p2[b:e], smp[s] if e - b >= 7 else np.zeros((n_hyp, 7), int), thr.value, bool(refine))
            oF[s] = 0.0 if r["F"] is None else r["F"].ravel()
            om[b:e] = r["mask"]
            oi[s], os_[s], orf[s] = r["n_inliers"], r["status"], int(r["refined"])
            if oc is not None:
                oc[s] = r["hyp_count"]

    h.sfm_fund_draw_samples, h.sfm_fund_ransac = draw, ransac
    monkeypatch.setattr(_lib, "get_handle", lambda device=0: h)
    real_device = torch.device
    monkeypatch.setattr(torch, "device", lambda *a, **k: real_device("cpu"))
    return twoview, h


def test_glue_short_pairs_shapes_and_dtypes(stubbed):
    twoview, h = stubbed
    rng = np.random.default_rng(0)
    a1, a2, _ = fr.synth_pair(rng, 60, 0.2)
    b1, b2, _ = fr.synth_pair(rng, 6, 0.0)
    res, dbg = twoview.estimate_fundamental_batched([a1, b1, a1[:0]], [a2, b2, a2[:0]], n_hypotheses=64, return_debug=True)
    assert h.calls == ["sfm_fund_draw_samples", "sfm_fund_ransac"]          # one of each for the whole list
    F, mask = res[0]
    assert F.shape == (3, 3) and F.dtype == np.float64 and F[2, 2] == 1.0
    assert mask.shape == (60, 1) and mask.dtype == np.uint8 and set(np.unique(mask)) <= {0, 1}
    assert res[1] == (None, None) and res[2] == (None, None)
    assert [d["status"] for d in dbg] == [0, 1, 1]
    assert dbg[0]["samples"].shape == (64, 7) and dbg[0]["hyp_count"].shape == (64,)
    assert dbg[0]["n_inliers"] == int(mask.sum()) >= dbg[0]["hyp_count"].max()
    assert np.array_equal(dbg[0]["samples"], fr.draw_samples(0, 0, 60, 64))
    # explicit samples replace the draw; the single-pair form
    smp = fr.draw_samples(9, 0, 60, 64)
    h.calls.clear()
    (F2, m2), d2 = twoview.find_fundamental(a1, a2, n_hypotheses=64, samples=smp, return_debug=True)
    assert h.calls == ["sfm_fund_ransac"] and np.array_equal(d2["samples"], smp)
    assert twoview.find_fundamental(b1, b2, n_hypotheses=64) == (None, None)
    assert twoview.estimate_fundamental_batched([], []) == []
    h.calls.clear()
    assert twoview.estimate_fundamental_batched([b1[:0]], [b2[:0]]) == [(None, None)] and h.calls == []


def test_glue_argument_errors(stubbed):
    twoview, _ = stubbed
    rng = np.random.default_rng(1)
    a1, a2, _ = fr.synth_pair(rng, 20, 0.0)
    good = fr.draw_samples(0, 0, 20, 8)
    with pytest.raises(ValueError):
        twoview.estimate_fundamental_batched([a1], [a2, a2])
    with pytest.raises(ValueError):
        twoview.estimate_fundamental_batched([a1], [a2[:5]])
    with pytest.raises(ValueError):
        twoview.estimate_fundamental_batched([a1], [a2], n_hypotheses=0)
    with pytest.raises(ValueError):
        twoview.estimate_fundamental_batched([a1], [a2], threshold=float("nan"))
    with pytest.raises(ValueError):
        twoview.estimate_fundamental_batched([a1], [a2], seed=-1)
    for bad in (good[:4], good.astype(np.float64), np.where(good == good[0, 0], 20, good),
                np.where(good == good[0, 0], -1, good), np.repeat(good[:, :1], 7, axis=1)):
        with pytest.raises(ValueError):
            twoview.estimate_fundamental_batched([a1], [a2], n_hypotheses=8, samples=[bad])
    with pytest.raises(ValueError):
        twoview.estimate_fundamental_batched([a1], [a2], n_hypotheses=8, samples=[good, good])


def test_process_pairs_drops_short_pairs_and_pairs_without_a_model(stubbed, monkeypatch):
    """process_pairs with match_pairs and verify_pairs stubbed: pairs under min_matches (find_matches.py:274), pairs the
    reference's try / except skips and pairs without a model yield None; the others the dictionary of the pair loop."""
    from sfm_amd import driver, matcher
    twoview, h = stubbed
    rng = np.random.default_rng(2)
    a1, a2, Ft = fr.synth_pair(rng, 80, 0.25)
    same = np.tile(np.float32([[100.0, 100.0]]), (12, 1))                # all points equal: no model
    kps = [a1, a2, a1[:4], same]
    ident = lambda n: (np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32), np.zeros(n, np.float32))
    answers = {(0, 1): ident(80), (2, 1): ident(4), (3, 3): ident(12), (1, 0): ValueError("not enough values to unpack"),
               (0, 2): ident(0)}
    monkeypatch.setattr(matcher, "match_pairs", lambda descs, pairs, *a, **k: [answers[p] for p in pairs])

    def verify(pairs, threshold=3.0, device=0):
        out = []
        for p1, p2, F in pairs:
            e = fr.sym_err(F, p1.astype(np.float64), p2.astype(np.float64)).astype(np.float32)
            out.append(driver._verification_result(p1, p2, e, e < threshold))
        return out
    monkeypatch.setattr(matcher, "verify_pairs", verify)
    m = matcher.ImageMatcher()
    m.fund_hypotheses = 128
    pairs = [(0, 1), (2, 1), (3, 3), (1, 0), (0, 2)]
    out = m.process_pairs(kps, [None] * 4, pairs)
    assert [o is None for o in out] == [False, True, True, True, True]
    assert h.calls.count("sfm_fund_ransac") == 1
    r = out[0]
    assert set(r) >= {"F", "inlier_mask", "pts1", "pts2", "matches", "metrics"}
    assert r["pts1"].dtype == np.float32 and r["pts1"].shape == (80, 2) and np.array_equal(r["pts2"], a2)
    assert len(r["matches"]) == 80 and r["metrics"]["total_matches"] == 80
    true_in = int((fr.sym_err(Ft, a1.astype(np.float64), a2.astype(np.float64)) < 3.0).sum())
    assert r["metrics"]["inliers"] >= 0.9 * true_in
    # min_matches is the reference's `< min_matches` test: 4 matches pass at min_matches=4 but are under 7 -> no model
    assert m.process_pairs(kps, [None] * 4, [(2, 1)], min_matches=4) == [None]
    # keypoints as objects with .pt
    class KP:
        def __init__(self, pt):
            self.pt = (float(pt[0]), float(pt[1]))
    out2 = m.process_pairs([[KP(p) for p in a1], [KP(p) for p in a2]], [None] * 2, [(0, 1)])
    assert np.array_equal(out2[0]["pts1"], a1) and np.array_equal(out2[0]["F"], r["F"])
