"""CPU tests of the homography RANSAC: the NumPy reference (tests/homography_reference.py) against the true homographies
of a pure rotation and of a plane, the ratio of homography to fundamental-matrix inliers that tells those scenes from a
general one, and the kernel's solver and error rule (sfm_amd/csrc/homography_solve.h, homography_rule.h) compiled for
the host against the reference, hypothesis by hypothesis.  No GPU."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import fundamental_reference as fr
import homography_reference as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 3.0


@functools.lru_cache(maxsize=None)
def shipped():
    """[(pair index, pts1, pts2, shipped F)] of pairs 0, 13, ..., 143 - never modified."""
    pairs = hr.shipped_pairs()
    return [(i,) + pairs[i] for i in hr.SHIPPED]


@functools.lru_cache(maxsize=None)
def shipped_replay():
    """[(samples, reference result, stable)] of the shipped pairs at seed 0, 512 hypotheses, in segment positions 0..11 -
    computed once, never modified."""
    out = []
    for s, (_, p1, p2, _) in enumerate(shipped()):
        smp = hr.draw_samples(0, s, len(p1), 512)
        out.append((smp, hr.ransac(p1, p2, smp, THR), hr.stable(p1, p2, smp, THR)))
    return out


@functools.lru_cache(maxsize=None)
def synthetic_replay():
    """[(samples, reference result, stable)] of hr.CASES at seed 1, 512 hypotheses - computed once, never modified."""
    p1s, p2s = hr.synth_batch()
    out = []
    for s, (_, M, _) in enumerate(hr.CASES):
        smp = hr.draw_samples(1, s, M, 512)
        st = hr.stable(p1s[s], p2s[s], smp, THR) if M >= 4 else np.ones(512, bool)
        out.append((smp, hr.ransac(p1s[s], p2s[s], smp, THR), st))
    return out


def left_out_share(res, st):
    """Share of the non-voided hypotheses that `stable` leaves out."""
    live = ~res["voided"]
    return float((~st[live]).mean()) if live.any() else 0.0


def test_samples_are_the_shared_generator_at_four_slots():
    a = hr.draw_samples(5, 3, 40, 256)
    assert a.shape == (256, 4) and a.dtype == np.int32 and a.min() >= 0 and a.max() < 40
    assert all(len(set(r)) == 4 for r in a.tolist())
    assert np.array_equal(a, fr.draw_samples(5, 3, 40, 256)[:, :4])
    assert (hr.draw_samples(5, 3, 3, 16) == -1).all()
    assert sorted(hr.draw_samples(5, 3, 4, 1)[0].tolist()) == [0, 1, 2, 3]


@pytest.mark.parametrize("kind", ["rotation", "planar"])
def test_winner_against_the_true_homography(kind):
    """512 hypotheses at 3 px on 40 and 300 matches with 0 % and 30 % outliers: the winner's count is at least 0.95 x the
    count of the true homography (K R K^-1, or the plane-induced one) under the same rule; the 5 % cover 0.5 px noise
    against a 3 px gate.  With and without the refit.  Measured: 100 % or above in every case."""
    for M in (40, 300):
        for share in (0.0, 0.3):
            p1, p2, Ht = hr.scene(kind, M, share)
            truth = int(hr.inliers(Ht, p1, p2, THR).sum())
            smp = hr.draw_samples(0, 0, M, 512)
            for refine in (False, True):
                res = hr.ransac(p1, p2, smp, THR, refine=refine)
                print(f"{kind} M {M} share {share} refit {refine}: winner {res['n_inliers']} / true H {truth}, "
                      f"voided {res['voided'].mean():.2%}")
                assert res["status"] == 0 and res["H"][2, 2] == 1.0
                assert res["n_inliers"] >= 0.95 * truth, (M, share, refine)
                assert truth >= 0.9 * (M - int(M * share))        # the truth is the truth: it holds the clean matches


def test_stable_leaves_out_at_most_one_percent():
    """The share of the non-voided hypotheses that `stable` leaves out, per segment.  Measured: 0 % in every synthetic
    case and in every one of the 12 shipped pairs (15 to 54 % of whose samples the sample rule voids)."""
    for (kind, M, share), (smp, res, st) in zip(hr.CASES, synthetic_replay()):
        print(f"{kind} M {M} share {share}: left out {left_out_share(res, st):.2%}, voided {res['voided'].mean():.2%}")
        assert left_out_share(res, st) <= 0.01, (kind, M, share)
    for (i, _, _, _), (smp, res, st) in zip(shipped(), shipped_replay()):
        print(f"pair {i}: left out {left_out_share(res, st):.2%}, voided {res['voided'].mean():.2%}")
        assert left_out_share(res, st) <= 0.01, i


@functools.lru_cache(maxsize=None)
def ratios():
    """{(kind, M, share): (n_H, n_F)} of the winning H and F, 512 hypotheses each at 3 px, no refit."""
    out = {}
    for kind in ("general", "rotation", "planar"):
        for M in (40, 300):
            for share in (0.0, 0.3):
                p1, p2, _ = hr.scene(kind, M, share)
                with np.errstate(all="ignore"):
                    n_f = fr.ransac(p1, p2, fr.draw_samples(0, 0, M, 512), THR)["n_inliers"]
                n_h = hr.ransac(p1, p2, hr.draw_samples(0, 0, M, 512), THR)["n_inliers"]
                out[kind, M, share] = (n_h, n_f)
    return out


def test_the_ratio_separates_the_scene_kinds_at_0_8():
    """n_H / n_F of the winners: at most 0.8 on the general scene, above it on a pure rotation and on a plane - what
    `max_homography_ratio=0.8` of reconstruct_tracks decides on."""
    span = {}
    for (kind, M, share), (n_h, n_f) in ratios().items():
        r = n_h / n_f
        print(f"{kind} M {M} share {share}: n_H {n_h} / n_F {n_f} = {r:.3f}")
        lo, hi = span.get(kind, (np.inf, -np.inf))
        span[kind] = (min(lo, r), max(hi, r))
        assert (r <= 0.8) if kind == "general" else (r > 0.8), (kind, M, share)
    print("ranges:", {k: (round(v[0], 3), round(v[1], 3)) for k, v in span.items()})


# ------------------------------------------------------- the kernel's solver and rule built for the host
def build_native(tmp, extra=()):
    exe = os.path.join(tmp, "homography_solve_check" + ("_san" if extra else ""))
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "homography_solve_check.cpp"), "-o", exe], check=True)
    return exe


def run_native(exe, p1, p2, smp):
    """(ok [H] bool, H [H,3,3], count [H]) of the host build for samples smp of one pair, under the reference's transforms."""
    a = np.asarray(p1, np.float32).astype(np.float64).reshape(-1, 2)
    b = np.asarray(p2, np.float32).astype(np.float64).reshape(-1, 2)
    T1, T2, _ = hr.transforms(a, b)
    t = [T1[0, 0], -T1[0, 2] / T1[0, 0], -T1[1, 2] / T1[0, 0], T2[0, 0], -T2[0, 2] / T2[0, 0], -T2[1, 2] / T2[0, 0]]
    np.concatenate([[len(a), len(smp), THR], t, np.c_[a, b].ravel(), np.asarray(smp, np.float64).ravel()]).tofile(exe + ".in")
    subprocess.run([exe, exe + ".in", exe + ".out"], check=True)
    o = np.fromfile(exe + ".out").reshape(-1, 11)
    return o[:, 0] != 0, o[:, 1:10].reshape(-1, 3, 3), o[:, 10].astype(int)


def check_native(exe):
    p1s, p2s = hr.synth_batch()
    for s, ((kind, M, share), (smp, res, st)) in enumerate(zip(hr.CASES, synthetic_replay())):
        if M < 4:
            continue
        ok, Hs, cnt = run_native(exe, p1s[s], p2s[s], smp)
        eq = cnt == res["hyp_count"]
        print(f"{kind} M {M} share {share}: equal on {eq[st].mean():.4%} of the stable hypotheses, {eq.mean():.4%} of all; "
              f"voided {res['voided'].mean():.2%}")
        assert eq[st].mean() >= 0.99, (kind, M, share)
        assert np.array_equal(~ok, res["voided"]) and (Hs[~ok] == 0).all() and (cnt[~ok] == 0).all()
    for (i, p1, p2, _), (smp, res, st) in zip(shipped(), shipped_replay()):
        ok, Hs, cnt = run_native(exe, p1, p2, smp)
        eq = cnt == res["hyp_count"]
        print(f"pair {i}: equal on {eq[st].mean():.4%} of the stable hypotheses, {eq.mean():.4%} of all")
        assert eq[st].mean() >= 0.99, i
        assert np.array_equal(~ok, res["voided"])
    # by rule: a collinear triple in image 1, one in image 2, a reflected sample, a NaN and an infinity each void their
    # sample; the plain sample does not
    p1, p2, _ = hr.scene("planar", 40, 0.0)
    p1, p2 = p1.copy(), p2.copy()
    p1[2] = p1[0] + np.float32(0.25) * (p1[1] - p1[0])
    p2[7] = p2[4] + np.float32(2.0) * (p2[5] - p2[4])
    p2[8:12] = p1[8:12] * np.float32([-1, 1]) + np.float32([1024, 0])
    p1[13, 0], p2[18, 1] = np.nan, np.inf
    smp = np.arange(24).reshape(6, 4)
    ok, Hs, cnt = run_native(exe, p1, p2, smp)
    assert ok.tolist() == [False, False, False, False, False, True] and cnt[5] >= 4 and (cnt[:5] == 0).all()
    assert hr.voided(p1, p2, smp).tolist() == [True, True, True, True, True, False]
    with np.errstate(all="ignore"):
        assert hr.ransac(p1, p2, smp, THR)["hyp_count"][5] == cnt[5]
    # an index outside the segment voids its sample and reads nothing
    ok, _, cnt = run_native(exe, p1, p2, np.array([[20, 21, 22, 40], [20, 21, -1, 23]]))
    assert not ok.any() and (cnt == 0).all()


def test_kernel_solver_and_rule_on_the_host_equal_the_reference(tmp_path):
    """homography_solve.h + homography_rule.h compiled by g++ -ffp-contract=off: hyp_count equals the reference's on at
    least 99 % of the stable hypotheses of every synthetic case and of the 12 shipped pairs - the bound the GPU replay
    test sets for the kernels, here for their solver and rule alone - and the samples it voids are the reference's.
    Measured: 100 % of the stable hypotheses in every case and pair."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    check_native(build_native(str(tmp_path)))


def test_kernel_solver_and_rule_on_the_host_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run as the stand-alone program it is: every index of
    the 36 rotations and of the rows stays inside its array, and nothing undefined happens on the way."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    check_native(build_native(str(tmp_path), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")))
