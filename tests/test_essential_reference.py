"""CPU tests of the essential-matrix RANSAC: the NumPy reference (tests/essential_reference.py) against the truth and
on the shipped pairs, and the kernel's solver (sfm_amd/csrc/essential_solve.h) compiled for the host against the
reference, sample by sample.  No GPU."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import essential_reference as er
import fundamental_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = fr.K_REF
THR = 3.0


@functools.lru_cache(maxsize=None)
def shipped():
    """[(pair index, pts1, pts2, shipped F)] of pairs 0, 13, ..., 143 - never modified."""
    pairs = er.shipped_pairs()
    return [(i,) + pairs[i] for i in er.SHIPPED]


@functools.lru_cache(maxsize=None)
def shipped_replay():
    """[(samples, reference result, stable)] of the shipped pairs at seed 0, 512 hypotheses, in segment positions 0..11 -
    computed once, never modified."""
    out = []
    for s, (_, p1, p2, _) in enumerate(shipped()):
        smp = er.draw_samples(0, s, len(p1), 512)
        out.append((smp, er.ransac(p1, p2, K, smp, THR), er.stable(p1, p2, K, smp, THR)))
    return out


@functools.lru_cache(maxsize=None)
def synthetic_replay():
    """[(samples, reference result, stable)] of er.CASES at seed 1, 512 hypotheses - computed once, never modified."""
    p1s, p2s = er.synth_batch()
    out = []
    for s, (M, _) in enumerate(er.CASES):
        smp = er.draw_samples(1, s, M, 512)
        out.append((smp, er.ransac(p1s[s], p2s[s], K, smp, THR), er.stable(p1s[s], p2s[s], K, smp, THR) if M >= 5 else np.ones(512, bool)))
    return out


def left_out_share(res, st):
    """Share of the non-voided hypotheses that `stable` leaves out."""
    live = ~res["voided"]
    return float((~st[live]).mean()) if live.any() else 0.0


def test_samples_are_the_shared_generator_at_five_slots():
    a = er.draw_samples(5, 3, 40, 256)
    assert a.shape == (256, 5) and a.dtype == np.int32 and a.min() >= 0 and a.max() < 40
    assert all(len(set(r)) == 5 for r in a.tolist())
    assert np.array_equal(a, fr.draw_samples(5, 3, 40, 256)[:, :5])
    assert (er.draw_samples(5, 3, 4, 16) == -1).all()


def test_reference_against_the_truth():
    """Noise-free synthetic pair, 512 hypotheses.  Measured: nearest candidate to +-E_true within 1e-8 on 100 % of the
    hypotheses (median 1e-14, worst 1e-8); largest epipolar residual at the sample points 6e-16; median residual of
    2 E E^T E - tr(E E^T) E 3e-15."""
    p1, p2, F = fr.synth_pair(np.random.default_rng(5), 300, 0.0, noise=0.0, float32=False)
    Et = K.T @ F @ K
    Et = (Et / np.linalg.norm(Et)).reshape(9)
    smp = er.draw_samples(0, 0, 300, 512).astype(np.int64)
    n1, n2 = er.normalise(p1, K), er.normalise(p2, K)
    E, ok = er.five_point(n1[smp], n2[smp])
    assert ok.any(1).all()
    En = E.reshape(512, 10, 9) / np.sqrt(2.0)
    d = np.minimum(np.abs(En - Et).max(-1), np.abs(En + Et).max(-1))
    near = np.where(ok, d, np.inf).min(1)
    print(f"nearest candidate to the truth: within 1e-8 on {np.mean(near <= 1e-8):.2%}, median {np.median(near):.1e}, worst {near.max():.1e}; "
          f"candidates per sample: mean {ok.sum(1).mean():.2f}, max {ok.sum(1).max()}")
    assert np.mean(near <= 1e-8) >= 0.99
    x1 = np.concatenate([n1[smp], np.ones((512, 5, 1))], -1)
    x2 = np.concatenate([n2[smp], np.ones((512, 5, 1))], -1)
    epi = np.abs(np.einsum("hpi,hkij,hpj->hkp", x2, E, x1))[ok]
    print(f"epipolar residual at the sample points: max {epi.max():.1e}")
    assert epi.max() <= 1e-12
    Ev = E[ok]
    EEt = Ev @ Ev.transpose(0, 2, 1)
    cub = np.abs(2 * EEt @ Ev - np.trace(EEt, axis1=1, axis2=2)[:, None, None] * Ev).max(axis=(1, 2))
    print(f"residual of 2 E E^T E - tr(E E^T) E: median {np.median(cub):.1e}, max {cub.max():.1e}")
    assert np.median(cub) <= 1e-12


def test_five_point_pose_passes_the_gate_where_the_fundamental_route_does_not():
    """The motivation as a regression, on pairs 0, 13, ..., 143: the reference's unrefined winner -> recover_pose -> two-view
    triangulation leaves at least 90 % of the good points within 4 px in every pair; E = K^T F K of the shipped F is printed
    beside it."""
    for (i, p1, p2, F), (smp, res, _) in zip(shipped(), shipped_replay()):
        assert res["status"] == 0
        n_good, share, med = er.pose_quality(res["E"], res["mask"], p1, p2, K)
        fm = fr.inliers(F, p1.astype(np.float64), p2.astype(np.float64), THR)
        f_good, f_share, f_med = er.pose_quality(K.T @ F @ K, fm, p1, p2, K)
        print(f"pair {i}: five-point {res['n_inliers']} inliers, {n_good} good, {share:.1%} within 4 px, median {med:.2f} px | "
              f"K^T F K: {int(fm.sum())} inliers, {f_good} good, {f_share:.1%} within 4 px, median {f_med:.2f} px")
        assert n_good > 0 and share >= 0.9, i


def test_stable_leaves_out_at_most_one_percent():
    """The share of the non-voided hypotheses that `stable` leaves out, per segment.  Measured: 0 % in every
    synthetic case and in every one of the 12 shipped pairs (1 to 10 % of whose samples the repeated-pixel rule voids)."""
    for (M, share), (smp, res, st) in zip(er.CASES, synthetic_replay()):
        print(f"synthetic M {M} share {share}: left out {left_out_share(res, st):.2%}, voided {res['voided'].mean():.2%}")
        assert left_out_share(res, st) <= 0.01, (M, share)
    for (i, _, _, _), (smp, res, st) in zip(shipped(), shipped_replay()):
        print(f"pair {i}: left out {left_out_share(res, st):.2%}, voided {res['voided'].mean():.2%}")
        assert left_out_share(res, st) <= 0.01, i


# ---------------------------------------------------------------------- the kernel's solver built for the host
def build_native(tmp, extra=()):
    exe = os.path.join(tmp, "essential_solve_check" + ("_san" if extra else ""))
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", *extra, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "essential_solve_check.cpp"), "-o", exe], check=True)
    return exe


def run_native(exe, p1, p2, smp):
    """(number of candidates [H], E [H,10,3,3]) of the host build for samples smp of one pair."""
    px = np.concatenate([np.asarray(p1, np.float32)[smp], np.asarray(p2, np.float32)[smp]], 2).reshape(len(smp), 20)
    np.concatenate([px.astype(np.float64), np.tile(er.k4_of(K), (len(smp), 1))], 1).tofile(exe + ".in")
    subprocess.run([exe, exe + ".in", exe + ".out"], check=True)
    o = np.fromfile(exe + ".out").reshape(-1, 91)
    return o[:, 0].astype(int), o[:, 1:].reshape(-1, 10, 3, 3)


def native_hyp_count(exe, p1, p2, smp):
    nc, E = run_native(exe, p1, p2, smp)
    ok = np.arange(10)[None] < nc[:, None]
    assert (E[~ok] == 0).all()
    Ev = E[ok].reshape(-1, 9)
    assert np.abs(np.sqrt((Ev * Ev).sum(1)) - np.sqrt(2.0)).max(initial=0.0) <= 1e-12
    assert (np.take_along_axis(Ev, np.argmax(np.abs(Ev), 1)[:, None], 1) > 0).all()
    cnt = er.counts(E, ok, K, np.asarray(p1, np.float64), np.asarray(p2, np.float64), THR)
    return cnt.max(1), nc


def check_native(exe):
    p1s, p2s = er.synth_batch()
    for s, ((M, share), (smp, res, st)) in enumerate(zip(er.CASES, synthetic_replay())):
        if M < 5:
            continue
        hc, nc = native_hyp_count(exe, p1s[s], p2s[s], smp)
        eq = hc == res["hyp_count"]
        print(f"synthetic M {M} share {share}: equal on {eq[st].mean():.4%} of the stable hypotheses, {eq.mean():.4%} of all; "
              f"candidates per sample: mean {nc.mean():.2f}, max {nc.max()}")
        assert eq[st].mean() >= 0.99, (M, share)
    for (i, p1, p2, _), (smp, res, st) in zip(shipped(), shipped_replay()):
        hc, nc = native_hyp_count(exe, p1, p2, smp)
        eq = hc == res["hyp_count"]
        print(f"pair {i}: equal on {eq[st].mean():.4%} of the stable hypotheses, {eq.mean():.4%} of all")
        assert eq[st].mean() >= 0.99, i
        assert (nc[res["voided"]] == 0).all()            # a voided sample fills no slot
    # by rule: a repeated pixel in image 1, one in image 2, a NaN and an infinity each void their sample; the plain sample does not
    p1, p2 = p1s[4].copy(), p2s[4].copy()
    p1[1], p2[12], p1[20, 0], p2[31, 1] = p1[0], p2[11], np.nan, np.inf
    smp = np.array([[0, 1, 2, 3, 4], [10, 11, 12, 13, 14], [20, 21, 22, 23, 24], [30, 31, 32, 33, 34], [40, 41, 42, 43, 44]])
    nc, _ = run_native(exe, p1, p2, smp)
    assert (nc[:4] == 0).all() and nc[4] > 0
    assert np.array_equal(er.voided(p1, p2, smp), [True, True, True, True, False])


def test_kernel_five_point_solver_on_the_host_equals_the_reference(tmp_path):
    """essential_solve.h compiled by g++ -ffp-contract=off: per hypothesis the best count of its candidates equals the
    reference's on at least 99 % of the stable hypotheses of every synthetic case and of the 12 shipped pairs - the bound
    the GPU replay test sets for the kernels, here for their solver alone.  Measured: 100 % of the stable and of all
    hypotheses in every synthetic case and in every shipped pair."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    check_native(build_native(str(tmp_path)))


def test_kernel_five_point_solver_on_the_host_under_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run as the stand-alone program it is: every index of
    the working storage stays inside its 200 doubles, and nothing undefined happens on the way."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    check_native(build_native(str(tmp_path), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")))
