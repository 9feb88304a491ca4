#!/usr/bin/env python3
"""Device-time measurement of the driver-row kernels with inputs resident in HBM:
association (pair tests/s), two-view triangulation (tracks/s), epipolar verification (matches/s), and the batched
fundamental-matrix RANSAC beside the batched matcher it follows in the pair loop, the batched essential-matrix RANSAC
beside it on the same pairs, the batched homography RANSAC beside it as well, the batched PnP RANSAC of the
camera registration, the batched relative-pose recovery of the initial-pair scan, the track building, the N-view
triangulation of the tracks, the resection lists, the gate evaluation and the incremental loop on top of them, the
feature detection / description stage in front of them all, and the dense-depth stage behind them.  Prints one JSON line per kernel.  bench.py calls measure() and, in its cpu_baseline leg, hands in the NumPy oracle's
functions to time on a bounded sample of the same inputs (this tool itself never imports oracle/).
usage: python tools/bench_driver.py [--reps 20] [--fundamental-only | --essential-only | --homography-only | --pnp-only | --pose-only | --tracks-only | --triangulate-only |
       --incremental-only | --features-only | --pyramid-only | --guided-only | --depth-only | --mesh-only]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn(); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e-3


def measure(reps=20, tracks=100000, corr=20000, cpu_fns=None, emit=None):
    """[assoc, triangulate, epipolar] result dicts; `emit(dict)` is called as each becomes available.
    cpu_fns: optional {"associate", "triangulate_point", "symmetric_epipolar_errors"} callables (the oracle's)
    timed on a bounded sample beside each kernel."""
    import types
    a = types.SimpleNamespace(reps=reps, tracks=tracks, corr=corr)
    results = []

    def out(d):
        results.append(d)
        if emit:
            emit(d)
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p
    cpu = cpu_fns is not None
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    vp = C.c_void_p

    # ---- association: T tracks x M correspondences, ~40 % of tracks have a partner
    T, M = a.tracks, a.corr
    c = (rng.random((M, 2)) * [1024, 768]).astype(np.float32)
    t = (rng.random((T, 2)) * [1024, 768]).astype(np.float32)
    k = int(0.4 * T)
    t[rng.permutation(T)[:k]] = c[rng.integers(0, M, k)] + (rng.normal(size=(k, 2)) * 0.7).astype(np.float32)
    d_t = torch.from_numpy(t.astype(np.float64)).to(dev); d_c = torch.from_numpy(c.astype(np.float64)).to(dev)
    t_ptr = torch.tensor([0, T], dtype=torch.int64, device=dev); m_ptr = torch.tensor([0, M], dtype=torch.int64, device=dev)
    need = C.c_int64(); h.lib.sfm_assoc_workspace_bytes(T, C.byref(need))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    cap = 4 * T
    o_r = torch.empty(cap, dtype=torch.int32, device=dev); o_c = torch.empty(cap, dtype=torch.int32, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)

    def assoc():
        h.call("sfm_assoc_radius", _p(d_t), _p(t_ptr), _p(d_c), _p(m_ptr), 1, T, C.c_double(2.0), _p(o_r), _p(o_c),
               cap, _p(tot), _p(ws), need.value)
    sec = timed(assoc, a.reps)
    ns = min(T, 2000)
    r = {"kernel": "assoc_radius", "tracks": T, "correspondences": M, "hits": int(tot.item()),
         "ms": sec * 1e3, "pair_tests_per_s": T * M / sec,
         "fp64_flop_per_s": 5.0 * 2 * T * M / sec}      # 2 passes (count, fill) x 5 flop per test
    if cpu:
        t0 = time.perf_counter(); cpu_fns["associate"](t[:ns].astype(np.float64), c); sec_cpu = time.perf_counter() - t0
        r.update(cpu_numpy_pair_tests_per_s=ns * M / sec_cpu, cpu_sample=f"{ns} x {M}")
    out(r)

    # ---- triangulation: n two-view tracks over 64 cameras
    n = 1_000_000
    from sfm_amd import synth
    sc = synth.make_scene(64, 20000, obs_per_point=2, seed=3, noise_px=0.5)
    poses, pts, tracks, K = sc.state()
    ids = list(poses)
    proj = np.stack([K @ np.hstack([poses[i][0], np.asarray(poses[i][1]).reshape(3, 1)]) for i in ids])
    ci = sc.cam_idx.reshape(-1, 2); uv = sc.uv.reshape(-1, 2, 2)
    rep = -(-n // len(ci))
    c0 = np.tile(ci[:, 0], rep)[:n].astype(np.int32); c1 = np.tile(ci[:, 1], rep)[:n].astype(np.int32)
    x0 = np.tile(uv[:, 0], (rep, 1))[:n]; x1 = np.tile(uv[:, 1], (rep, 1))[:n]
    d = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (proj.reshape(-1, 12), c0, c1, x0, x1)]
    X = torch.empty((n, 3), dtype=torch.float64, device=dev); valid = torch.empty(n, dtype=torch.int32, device=dev)

    def tri():
        h.call("sfm_triangulate2", _p(d[0]), proj.shape[0], _p(d[1]), _p(d[2]), _p(d[3]), _p(d[4]), n,
               C.c_double(4.0), _p(X), _p(valid), vp(0))
    sec = timed(tri, a.reps)
    ns = 2000
    r = {"kernel": "triangulate2", "tracks": n, "valid_frac": float(valid.float().mean().item()),
         "ms": sec * 1e3, "tracks_per_s": n / sec, "hbm_GBps_algorithmic": n * 68 / sec / 1e9}
    if cpu:
        t0 = time.perf_counter()
        for i in range(ns):
            cpu_fns["triangulate_point"]([proj[c0[i]], proj[c1[i]]], [x0[i], x1[i]])
        sec_cpu = time.perf_counter() - t0
        r.update(cpu_numpy_tracks_per_s=ns / sec_cpu, cpu_sample=f"{ns} tracks")
    out(r)

    # ---- epipolar verification: n matches in 1,000 pairs
    n, n_seg = 10_000_000, 1000
    F = rng.normal(size=(n_seg, 9)) * np.array([1e-6, 1e-6, 1e-3, 1e-6, 1e-6, 1e-3, 1e-3, 1e-3, 1.0])
    p1 = (rng.random((n, 2)) * 1000).astype(np.float32); p2 = (rng.random((n, 2)) * 1000).astype(np.float32)
    seg = torch.from_numpy(np.linspace(0, n, n_seg + 1).astype(np.int64)).to(dev)
    dF, d1, d2 = (torch.from_numpy(v).to(dev) for v in (F, p1, p2))
    err = torch.empty(n, dtype=torch.float32, device=dev); mask = torch.empty(n, dtype=torch.uint8, device=dev)

    def epi():
        h.call("sfm_epipolar_errors", _p(dF), _p(seg), n_seg, _p(d1), _p(d2), n, C.c_float(3.0), _p(err), _p(mask))
    sec = timed(epi, a.reps)
    ns = 1_000_000
    r = {"kernel": "epipolar_errors", "matches": n, "pairs": n_seg, "ms": sec * 1e3,
         "matches_per_s": n / sec, "hbm_GBps_algorithmic": n * 21 / sec / 1e9,
         "hbm_frac_of_8TBps": n * 21 / sec / 8e12}
    if cpu:
        t0 = time.perf_counter(); cpu_fns["symmetric_epipolar_errors"](p1[:ns], p2[:ns], F[0].reshape(3, 3))
        sec_cpu = time.perf_counter() - t0
        r.update(cpu_numpy_matches_per_s=ns / sec_cpu, cpu_sample=f"{ns} matches")
    out(r)
    return results


FUND_FLOP_PER_TEST = 40          # one candidate against one match: two epipolar lines, s, two norms, the comparison


def _synthetic_pairs(rng, n_pairs, M, outlier_share=0.3, noise=0.5):
    """Two-view scenes with the reference's K: points in a box in front of two cameras, float32 pixels."""
    K = np.array([[1228.0, 0, 512], [0, 1228.0, 384], [0, 0, 1]])
    p1, p2 = [], []
    for _ in range(n_pairs):
        X = rng.uniform(-1, 1, (M, 3)) + [0, 0, 6.0]
        yaw = rng.uniform(0.1, 0.4)
        R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        t = np.array([-1.5, 0.1, 0.3]) * rng.uniform(0.5, 1.5)
        x1 = X @ K.T; x1 = x1[:, :2] / x1[:, 2:] + rng.normal(size=(M, 2)) * noise
        x2 = (X @ R.T + t) @ K.T; x2 = x2[:, :2] / x2[:, 2:] + rng.normal(size=(M, 2)) * noise
        k = int(M * outlier_share)
        x2[:k] = rng.uniform(0, 1, (k, 2)) * [1024, 768]
        p1.append(x1.astype(np.float32)); p2.append(x2.astype(np.float32))
    return p1, p2


def measure_fundamental(reps=20, n_hyp=1024, emit=None):
    """sfm_fund_ransac on (a) the 148 shipped pairs and (b) 630 synthetic pairs of 300 matches, inputs resident in HBM:
    the whole call and k_fund_hypotheses alone (the handle's event slot), and, from the same run, the device time of the
    batched matcher's two launches over the same 630 pairs (36 images x 500 descriptors of dimension 128)."""
    import torch
    from sfm_amd import _lib, matcher
    from sfm_amd.driver import _p, _ptr_array
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_pairs.npz"), allow_pickle=False)
    off = g["offsets"]
    shipped = ([g["pts1"][off[s]:off[s + 1]] for s in range(len(off) - 1)], [g["pts2"][off[s]:off[s + 1]] for s in range(len(off) - 1)])
    results = []
    for name, (p1, p2) in (("shipped_148_pairs", shipped), ("synthetic_630_pairs_x_300", _synthetic_pairs(rng, 630, 300))):
        n_seg = len(p1)
        lengths = [len(a) for a in p1]
        n = int(sum(lengths))
        _, ptr = _ptr_array(lengths, dev)
        d1 = torch.from_numpy(np.concatenate(p1).astype(np.float32)).to(dev)
        d2 = torch.from_numpy(np.concatenate(p2).astype(np.float32)).to(dev)
        smp = torch.empty((n_seg, n_hyp, 7), dtype=torch.int32, device=dev)
        h.call("sfm_fund_draw_samples", _p(ptr), n_seg, n_hyp, C.c_uint64(0), _p(smp))
        need = C.c_int64(); h.lib.sfm_fund_workspace_bytes(n, n_seg, n_hyp, C.byref(need))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        F = torch.empty((n_seg, 9), dtype=torch.float64, device=dev)
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        meta = torch.empty((3, n_seg), dtype=torch.int32, device=dev)

        def ransac(refine=1):
            h.call("sfm_fund_ransac", _p(ptr), n_seg, _p(d1), _p(d2), n, _p(smp), n_hyp, C.c_double(3.0), refine, _p(F),
                   _p(mask), _p(meta[0]), _p(meta[1]), C.c_void_p(0), _p(meta[2]), _p(ws), need.value)
        for _ in range(3):
            ransac()
        sec = timed(ransac, reps)
        sec_plain = timed(lambda: ransac(0), reps)
        h.set_profiling(True); h.profile()
        for _ in range(reps):
            ransac()
        ms, launches = h.profile()["fund_hyp"]
        h.set_profiling(False)
        k_sec = ms * 1e-3 / max(launches, 1)
        tests = float(n) * n_hyp * 3                     # pairs x hypotheses x candidates x points, summed over the pairs
        r = {"kernel": "fund_ransac", "case": name, "pairs": n_seg, "matches": n, "hypotheses": n_hyp,
             "ms_call_with_refit": sec * 1e3, "ms_call_without_refit": sec_plain * 1e3, "ms_k_fund_hypotheses": k_sec * 1e3,
             "candidate_point_tests_per_s": tests / k_sec, "flop_per_test": FUND_FLOP_PER_TEST,
             "fp64_flop_per_s_scoring": FUND_FLOP_PER_TEST * tests / k_sec,
             "pairs_with_model": int((meta[1] == 0).sum().item()), "refit_kept": int(meta[2].sum().item())}
        results.append(r)
        if emit:
            emit(r)

    # the step this one follows: the batched matcher over the same 630 pairs, two launches, descriptors resident
    n_img, n_desc, dim = 36, 500, 128
    descs = [rng.integers(0, 256, (n_desc, dim)).astype(np.uint8) for _ in range(n_img)]
    pairs = [(i, j) for i in range(n_img) for j in range(i + 1, n_img)]
    rows, ptr_h, dim = matcher._upload_sets(descs, dev)
    q_beg = np.array([ptr_h[i] for i, _ in pairs], dtype=np.int64); q_end = np.array([ptr_h[i + 1] for i, _ in pairs], dtype=np.int64)
    t_beg = np.array([ptr_h[j] for _, j in pairs], dtype=np.int64); t_end = np.array([ptr_h[j + 1] for _, j in pairs], dtype=np.int64)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    n_out, need = C.c_int64(), C.c_int64()
    n_rows, n_seg, code = int(rows.shape[0]), len(pairs), _lib.METRIC_L2_U8
    h.check(h.lib.sfm_match_batched_workspace_bytes(code, n_seg, hp(q_beg), hp(q_end), hp(t_beg), hp(t_end), n_rows, n_rows,
                                                    C.byref(n_out), C.byref(need)), "sfm_match_batched_workspace_bytes")
    nq = n_out.value
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    i1, i2, qi, ti = (torch.empty(nq, dtype=torch.int32, device=dev) for _ in range(4))
    e1, e2, dd = (torch.empty(nq, dtype=torch.float32, device=dev) for _ in range(3))
    out_ptr = torch.empty(n_seg + 1, dtype=torch.int64, device=dev); seg_ptr = torch.empty(n_seg + 1, dtype=torch.int64, device=dev)

    def match():
        h.call("sfm_match_knn2_batched", code, _p(rows), n_rows, _p(rows), n_rows, dim, n_seg, hp(q_beg), hp(q_end), hp(t_beg),
               hp(t_end), _p(i1), _p(i2), _p(e1), _p(e2), _p(out_ptr), _p(ws), need.value)
        h.call("sfm_match_ratio_batched", nq, n_seg, _p(out_ptr), _p(i1), _p(e1), _p(e2), C.c_double(0.75), _p(qi), _p(ti),
               _p(dd), _p(seg_ptr), _p(ws), need.value)
    for _ in range(3):
        match()
    sec = timed(match, reps)
    r = {"kernel": "match_pairs_device", "pairs": n_seg, "images": n_img, "descriptors_per_image": n_desc, "dim": dim,
         "ms": sec * 1e3, "note": "knn2_batched + ratio_batched, descriptors resident: the step sfm_fund_ransac follows"}
    results.append(r)
    if emit:
        emit(r)
    return results

def measure_essential(reps=20, n_hyp=1024, emit=None):
    """sfm_ess_ransac on the 148 shipped pairs, inputs resident in HBM: the whole call with and without the refit and
    k_ess_solve / k_ess_score alone (the handle's event slots), beside sfm_fund_ransac on the same pairs with the same
    number of hypotheses."""
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p, _ptr_array
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_pairs.npz"), allow_pickle=False)
    off = g["offsets"]
    n_seg, n = len(off) - 1, int(off[-1])
    _, ptr = _ptr_array([int(off[s + 1] - off[s]) for s in range(n_seg)], dev)
    d1 = torch.from_numpy(np.ascontiguousarray(g["pts1"][:n], dtype=np.float32)).to(dev)
    d2 = torch.from_numpy(np.ascontiguousarray(g["pts2"][:n], dtype=np.float32)).to(dev)
    k4 = torch.tensor([[1228.0, 1228.0, 512.0, 384.0]] * n_seg, dtype=torch.float64, device=dev)
    model = torch.empty((n_seg, 9), dtype=torch.float64, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    meta = torch.empty((3, n_seg), dtype=torch.int32, device=dev)
    row = {"kernel": "ess_ransac", "case": "shipped_148_pairs", "pairs": n_seg, "matches": n, "hypotheses": n_hyp}
    for stage, size, extra in (("ess", 5, [k4]), ("fund", 7, [])):
        smp = torch.empty((n_seg, n_hyp, size), dtype=torch.int32, device=dev)
        h.call(f"sfm_{stage}_draw_samples", _p(ptr), n_seg, n_hyp, C.c_uint64(0), _p(smp))
        need = C.c_int64()
        h.check(getattr(h.lib, f"sfm_{stage}_workspace_bytes")(n, n_seg, n_hyp, C.byref(need)), f"sfm_{stage}_workspace_bytes")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)

        def ransac(refine=1):
            h.call(f"sfm_{stage}_ransac", _p(ptr), n_seg, _p(d1), _p(d2), n, *map(_p, extra), _p(smp), n_hyp, C.c_double(3.0),
                   refine, _p(model), _p(mask), _p(meta[0]), _p(meta[1]), C.c_void_p(0), _p(meta[2]), _p(ws), need.value)
        for _ in range(3):
            ransac()
        row[f"ms_{stage}_call_with_refit"] = timed(ransac, reps) * 1e3
        row[f"ms_{stage}_call_without_refit"] = timed(lambda: ransac(0), reps) * 1e3
        row[f"{stage}_workspace_bytes"] = need.value
        h.set_profiling(True); h.profile()
        for _ in range(reps):
            ransac()
        prof = h.profile()
        h.set_profiling(False)
        for slot in (("ess_solve", "ess_score") if stage == "ess" else ("fund_hyp",)):
            ms, launches = prof[slot]
            row[f"ms_k_{slot}"] = ms / max(launches, 1)
        row[f"{stage}_pairs_with_model"] = int((meta[1] == 0).sum().item())
        row[f"{stage}_refit_kept"] = int(meta[2].sum().item())
        row[f"{stage}_inliers"] = int(meta[0].sum().item())
    if emit:
        emit(row)
    return [row]


def measure_homography(reps=20, n_hyp=1024, emit=None):
    """sfm_hom_ransac on the cases of measure_fundamental - the 148 shipped pairs and 630 synthetic pairs of 300 matches -
    inputs resident in HBM: the whole call with and without the refit and k_hom_hypotheses alone (the handle's event
    slot), beside sfm_fund_ransac on the same pairs with the same number of hypotheses in the same run."""
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p, _ptr_array
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_pairs.npz"), allow_pickle=False)
    off = g["offsets"]
    shipped = ([g["pts1"][off[s]:off[s + 1]] for s in range(len(off) - 1)], [g["pts2"][off[s]:off[s + 1]] for s in range(len(off) - 1)])
    results = []
    for name, (p1, p2) in (("shipped_148_pairs", shipped), ("synthetic_630_pairs_x_300", _synthetic_pairs(rng, 630, 300))):
        n_seg = len(p1)
        lengths = [len(a) for a in p1]
        n = int(sum(lengths))
        _, ptr = _ptr_array(lengths, dev)
        d1 = torch.from_numpy(np.concatenate(p1).astype(np.float32)).to(dev)
        d2 = torch.from_numpy(np.concatenate(p2).astype(np.float32)).to(dev)
        model = torch.empty((n_seg, 9), dtype=torch.float64, device=dev)
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        meta = torch.empty((3, n_seg), dtype=torch.int32, device=dev)
        row = {"kernel": "hom_ransac", "case": name, "pairs": n_seg, "matches": n, "hypotheses": n_hyp}
        for stage, size in (("hom", 4), ("fund", 7)):
            smp = torch.empty((n_seg, n_hyp, size), dtype=torch.int32, device=dev)
            h.call(f"sfm_{stage}_draw_samples", _p(ptr), n_seg, n_hyp, C.c_uint64(0), _p(smp))
            need = C.c_int64()
            h.check(getattr(h.lib, f"sfm_{stage}_workspace_bytes")(n, n_seg, n_hyp, C.byref(need)), f"sfm_{stage}_workspace_bytes")
            ws = torch.empty(need.value, dtype=torch.uint8, device=dev)

            def ransac(refine=1):
                h.call(f"sfm_{stage}_ransac", _p(ptr), n_seg, _p(d1), _p(d2), n, _p(smp), n_hyp, C.c_double(3.0), refine,
                       _p(model), _p(mask), _p(meta[0]), _p(meta[1]), C.c_void_p(0), _p(meta[2]), _p(ws), need.value)
            for _ in range(3):
                ransac()
            row[f"ms_{stage}_call_with_refit"] = timed(ransac, reps) * 1e3
            row[f"ms_{stage}_call_without_refit"] = timed(lambda: ransac(0), reps) * 1e3
            h.set_profiling(True); h.profile()
            for _ in range(reps):
                ransac()
            ms, launches = h.profile()[f"{stage}_hyp"]
            h.set_profiling(False)
            row[f"ms_k_{stage}_hypotheses"] = ms / max(launches, 1)
            row[f"{stage}_pairs_with_model"] = int((meta[1] == 0).sum().item())
            row[f"{stage}_refit_kept"] = int(meta[2].sum().item())
            row[f"{stage}_inliers"] = int(meta[0].sum().item())
        results.append(row)
        if emit:
            emit(row)
    return results


PNP_FLOP_PER_TEST = 30       # 9 fma for p = P [X; 1], 2 fma + 1 fma + 1 mul for the error, 2 mul for thr^2 p2^2 (fma = 2)


def measure_pnp(reps=20, n_hyp=1024, emit=None):
    """sfm_pnp_ransac on (a) the 4 shipped 2D-3D match sets (images 3, 12, 20, 33) and (b) 64 synthetic segments of 1,000
    points with 40 % outliers, inputs resident in HBM: the whole call with and without the refinement (HIP events around
    `reps` calls) and k_pnp_hypotheses alone (the handle's event slot)."""
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p, _ptr_array
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "driver_bunny.npz"), allow_pickle=False)
    shipped = ([g[f"f{im}_points3D"] for im in g["f_images"]], [g[f"f{im}_points2D"] for im in g["f_images"]])
    K = np.array([1228.0, 1228.0, 512.0, 384.0])
    X3, x2 = [], []
    for s in range(64):
        yaw = rng.uniform(-0.4, 0.4)
        R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        X = rng.uniform(-1, 1, (1000, 3)) + [0, 0, 6.0]
        p = X @ R.T + rng.uniform(-1, 1, 3) * [1.5, 0.3, 0.3]
        x = p[:, :2] / p[:, 2:] * K[:2] + K[2:] + rng.normal(size=(1000, 2)) * 0.5
        x[:400] = rng.uniform(0, 1, (400, 2)) * [1024, 768]
        X3.append(X); x2.append(x.astype(np.float32))
    results = []
    for name, (p3, p2) in (("shipped_4_images", shipped), ("synthetic_64_segments_x_1000", (X3, x2))):
        n_seg = len(p3)
        lengths = [len(a) for a in p3]
        n = int(sum(lengths))
        _, ptr = _ptr_array(lengths, dev)
        dX = torch.from_numpy(np.concatenate(p3).astype(np.float64)).to(dev)
        duv = torch.from_numpy(np.concatenate(p2).astype(np.float32)).to(dev)
        dK = torch.from_numpy(np.tile(K, (n_seg, 1))).to(dev)
        smp = torch.empty((n_seg, n_hyp, 3), dtype=torch.int32, device=dev)
        h.call("sfm_pnp_draw_samples", _p(ptr), n_seg, n_hyp, C.c_uint64(0), _p(smp))
        need = C.c_int64(); h.lib.sfm_pnp_workspace_bytes(n, n_seg, n_hyp, C.byref(need))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        Rt = torch.empty((n_seg, 12), dtype=torch.float64, device=dev)
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        meta = torch.empty((3, n_seg), dtype=torch.int32, device=dev)

        def ransac(refine=1):
            h.call("sfm_pnp_ransac", _p(ptr), n_seg, _p(dX), _p(duv), n, _p(dK), _p(smp), n_hyp, C.c_double(8.0), refine,
                   _p(Rt), _p(mask), _p(meta[0]), _p(meta[1]), C.c_void_p(0), _p(meta[2]), _p(ws), need.value)
        for _ in range(3):
            ransac()
        sec = timed(ransac, reps)
        sec_plain = timed(lambda: ransac(0), reps)
        ransac()
        h.set_profiling(True); h.profile()
        for _ in range(reps):
            ransac()
        ms, launches = h.profile()["pnp_hyp"]
        h.set_profiling(False)
        k_sec = ms * 1e-3 / max(launches, 1)
        tests = float(n) * n_hyp * 4                     # segments x hypotheses x candidate slots x points
        r = {"kernel": "pnp_ransac", "case": name, "segments": n_seg, "points": n, "hypotheses": n_hyp,
             "ms_call_with_refine": sec * 1e3, "ms_call_without_refine": sec_plain * 1e3, "ms_k_pnp_hypotheses": k_sec * 1e3,
             "candidate_point_tests_per_s": tests / k_sec, "flop_per_test": PNP_FLOP_PER_TEST,
             "fp64_flop_per_s_scoring": PNP_FLOP_PER_TEST * tests / k_sec,
             "segments_with_model": int((meta[1] == 0).sum().item()), "refine_kept": int(meta[2].sum().item()),
             "inliers": [int(v) for v in meta[0].cpu().numpy()[:4]]}
        results.append(r)
        if emit:
            emit(r)
    return results


def _synthetic_pose_pairs(rng, n_pairs, M, noise=0.5):
    """(E [n_pairs,9], pts1, pts2 [n_pairs*M,2] float32): one random two-view geometry per pair with the reference's K,
    points at depths of 4 to 12 baselines, vectorised (4,950 pairs of 2,000 matches are 9.9 M points)."""
    fx, cx, cy = 1228.0, 512.0, 384.0
    w = rng.normal(size=(n_pairs, 3))
    w *= (rng.uniform(0.05, 0.5, n_pairs) / np.linalg.norm(w, axis=1))[:, None]
    th = np.linalg.norm(w, axis=1)[:, None, None]
    Kx = np.zeros((n_pairs, 3, 3))
    Kx[:, 0, 1], Kx[:, 0, 2], Kx[:, 1, 0] = -w[:, 2], w[:, 1], w[:, 2]
    Kx[:, 1, 2], Kx[:, 2, 0], Kx[:, 2, 1] = -w[:, 0], -w[:, 1], w[:, 0]
    Kx /= th
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    t = rng.normal(size=(n_pairs, 3))
    t /= np.linalg.norm(t, axis=1)[:, None]
    tx = np.zeros((n_pairs, 3, 3))
    tx[:, 0, 1], tx[:, 0, 2], tx[:, 1, 0] = -t[:, 2], t[:, 1], t[:, 2]
    tx[:, 1, 2], tx[:, 2, 0], tx[:, 2, 1] = -t[:, 0], -t[:, 1], t[:, 0]
    E = (tx @ R).reshape(n_pairs, 9)
    z = rng.uniform(4.0, 12.0, (n_pairs, M))
    X = np.stack([rng.uniform(-0.35, 0.35, (n_pairs, M)) * z, rng.uniform(-0.25, 0.25, (n_pairs, M)) * z, z], axis=2)
    Y = X @ R.transpose(0, 2, 1) + t[:, None, :]
    p1 = X[..., :2] / X[..., 2:] * fx + [cx, cy] + rng.normal(size=(n_pairs, M, 2)) * noise
    p2 = Y[..., :2] / Y[..., 2:] * fx + [cx, cy] + rng.normal(size=(n_pairs, M, 2)) * noise
    return E, p1.reshape(-1, 2).astype(np.float32), p2.reshape(-1, 2).astype(np.float32)


def measure_pose(reps=20, emit=None):
    """sfm_pose_recover on (a) the 148 shipped pairs (all matched points, E = K^T F K formed on the device) and (b) 4,950
    synthetic pairs - all pairs of 100 images - of 2,000 matches, inputs resident in HBM: the whole call with and without
    the pixel-space triangulation (HIP events around `reps` calls) and k_pose_vote alone (the handle's event slot)."""
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p, _ptr_array
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "bunny_pairs.npz"), allow_pickle=False)
    cases = [("shipped_148_pairs", g["F"].reshape(-1, 9), g["pts1"], g["pts2"], np.diff(g["offsets"]).tolist(), 1)]
    n_pairs, M = 4950, 2000
    E, p1, p2 = _synthetic_pose_pairs(rng, n_pairs, M)
    cases.append(("synthetic_4950_pairs_x_2000", E, p1, p2, [M] * n_pairs, 0))
    results = []
    for name, EF, p1, p2, lengths, is_f in cases:
        n_seg, n = len(lengths), int(sum(lengths))
        _, ptr = _ptr_array(lengths, dev)
        d1 = torch.from_numpy(np.ascontiguousarray(p1, dtype=np.float32)).to(dev)
        d2 = torch.from_numpy(np.ascontiguousarray(p2, dtype=np.float32)).to(dev)
        dE = torch.from_numpy(np.ascontiguousarray(EF, dtype=np.float64)).to(dev)
        dK = torch.from_numpy(np.tile(np.array([1228.0, 1228.0, 512.0, 384.0]), (n_seg, 1))).to(dev)
        need = C.c_int64(); h.lib.sfm_pose_workspace_bytes(n, n_seg, C.byref(need))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        R = torch.empty((n_seg, 9), dtype=torch.float64, device=dev); t = torch.empty((n_seg, 3), dtype=torch.float64, device=dev)
        meta = torch.empty((2, n_seg), dtype=torch.int32, device=dev)
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        X = torch.empty((n, 3), dtype=torch.float64, device=dev)

        def recover(tri=True):
            h.call("sfm_pose_recover", _p(ptr), n_seg, _p(d1), _p(d2), n, _p(dE), is_f, _p(dK), C.c_void_p(0), C.c_double(50.0),
                   _p(R), _p(t), _p(meta[0]), _p(meta[1]), _p(mask), _p(X) if tri else C.c_void_p(0), C.c_void_p(0),
                   C.c_void_p(0), C.c_void_p(0), _p(ws), need.value)
        for _ in range(3):
            recover()
        sec = timed(recover, reps)
        sec_plain = timed(lambda: recover(False), reps)
        h.set_profiling(True); h.profile()
        for _ in range(reps):
            recover()
        ms, launches = h.profile()["pose_vote"]
        h.set_profiling(False)
        k_sec = ms * 1e-3 / max(launches, 1)
        r = {"kernel": "pose_recover", "case": name, "pairs": n_seg, "points": n,
             "ms_call_with_triangulation": sec * 1e3, "ms_call_without_triangulation": sec_plain * 1e3,
             "ms_k_pose_vote": k_sec * 1e3, "candidate_point_triangulations_per_s": 4.0 * n / k_sec,
             "pairs_with_model": int((meta[1] == 0).sum().item()), "good_points": int(meta[0].sum().item()),
             "best_pair_count": int(meta[0].max().item())}
        results.append(r)
        if emit:
            emit(r)
    return results


def measure_tracks(reps=20, emit=None):
    """sfm_tracks_build on (a) the shipped matches (148 pairs, 35 images of 500 keypoints: verified matches only and all
    matches) and (b) a synthetic data set of 100 images x 2,000 keypoints with all 4,950 pairs matched on the points both
    images see (85 % visibility, 2 % of the matches wrong), inputs resident in HBM: device time of the whole call by HIP
    events around `reps` calls after warm-up, edges per second, and beside it the host time of the same join with
    scipy.sparse.csgraph.connected_components (the labelling alone, without the CSR output)."""
    import torch
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from sfm_amd import _lib
    from sfm_amd.driver import _dev, _p
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    gold = os.path.join(ROOT, "tests", "golden")
    bm = np.load(os.path.join(gold, "bunny_matches.npz"), allow_pickle=False)
    bp = np.load(os.path.join(gold, "bunny_pairs.npz"), allow_pickle=False)
    pairs = np.array([[int(x) - 1 for x in str(n).split("_")[1:3]] for n in bp["names"]], dtype=np.int32)
    kp35 = np.arange(36, dtype=np.int64) * 500
    cases = [("shipped_verified", kp35, bm["offsets"], pairs, bm["queryIdx"], bm["trainIdx"], bp["mask"].astype(np.uint8)),
             ("shipped_all_matches", kp35, bm["offsets"], pairs, bm["queryIdx"], bm["trainIdx"], None)]
    n_img, n_kp = 100, 2000
    sees = rng.random((n_img, n_kp)) < 0.85
    slot = np.stack([rng.permutation(n_kp) for _ in range(n_img)])           # keypoint index of point p in image i
    pl, ql, tl = [], [], []
    for i in range(n_img):
        for j in range(i + 1, n_img):
            both = np.flatnonzero(sees[i] & sees[j])
            q, t = slot[i][both], slot[j][both].copy()
            wrong = rng.random(len(both)) < 0.02
            t[wrong] = rng.integers(0, n_kp, int(wrong.sum()))
            pl.append((i, j)); ql.append(q); tl.append(t)
    seg = np.concatenate([[0], np.cumsum([len(q) for q in ql])]).astype(np.int64)
    cases.append((f"synthetic_{n_img}_images_x_{n_kp}_all_{len(pl)}_pairs", np.arange(n_img + 1, dtype=np.int64) * n_kp, seg,
                  np.array(pl, dtype=np.int32), np.concatenate(ql), np.concatenate(tl), None))
    results = []
    for name, kp_ptr, seg_ptr, pair_img, q, t, mask in cases:
        n_nodes, n_edges, n_seg = int(kp_ptr[-1]), len(q), len(pair_img)
        d_kp, d_seg, d_pair = _dev(kp_ptr, np.int64, dev), _dev(seg_ptr, np.int64, dev), _dev(pair_img, np.int32, dev)
        d_q, d_t = _dev(q, np.int32, dev), _dev(t, np.int32, dev)
        d_mask = _dev(mask, np.uint8, dev) if mask is not None else None
        need = C.c_int64(); h.lib.sfm_tracks_workspace_bytes(n_nodes, n_edges, C.byref(need))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        track_ptr = torch.empty(n_nodes // 2 + 1, dtype=torch.int64, device=dev)
        obs = torch.empty((2, n_nodes), dtype=torch.int32, device=dev)
        conflict = torch.empty(n_nodes // 2, dtype=torch.uint8, device=dev)
        node_track = torch.empty(n_nodes, dtype=torch.int32, device=dev)
        counts = torch.empty(5, dtype=torch.int64, device=dev)
        row = {"kernel": "tracks_build", "case": name, "images": len(kp_ptr) - 1, "pairs": n_seg, "nodes": n_nodes,
               "edges": n_edges, "edges_followed": int(n_edges if mask is None else mask.sum())}
        for policy, key in ((0, "drop"), (1, "keep")):
            def build():
                h.call("sfm_tracks_build", _p(d_kp), len(kp_ptr) - 1, n_nodes, _p(d_seg), n_seg, _p(d_pair), _p(d_q), _p(d_t),
                       _p(d_mask), n_edges, 2, policy, _p(track_ptr), _p(obs[0]), _p(obs[1]), _p(conflict), _p(node_track),
                       _p(counts), n_nodes // 2, n_nodes, _p(ws), need.value)
            for _ in range(3):
                build()
            sec = timed(build, reps)
            c = counts.cpu().numpy()
            row.update({f"ms_call_{key}": sec * 1e3, f"edges_per_s_{key}": n_edges / sec, f"tracks_{key}": int(c[0]),
                        f"observations_{key}": int(c[1])})
            row["conflicting"] = int(c[2])
        seg_of = np.repeat(np.arange(n_seg), np.diff(seg_ptr))
        live = np.ones(n_edges, bool) if mask is None else mask != 0
        t0 = time.perf_counter()
        a = kp_ptr[pair_img[seg_of, 0]] + q
        b = kp_ptr[pair_img[seg_of, 1]] + t
        g = coo_matrix((np.ones(int(live.sum()), np.int8), (a[live], b[live])), shape=(n_nodes, n_nodes))
        n_comp, _ = connected_components(g, directed=False)
        row["ms_scipy_connected_components_host"] = (time.perf_counter() - t0) * 1e3
        row["scipy_components_incl_singletons"] = int(n_comp)
        results.append(row)
        if emit:
            emit(row)
    return results


HBM_STREAM_BPS = 6.3e12         # achievable HBM read rate of an MI355X (8 TB/s on paper): what the stream floor divides by


def _triangulate_case(name, proj, cam_idx, uv, lengths, launch_bound):
    """Flat arrays of one workload: every camera an image of its own, every observation a keypoint of its own (numbered
    inside its image in track order), observations point-major."""
    n_cams = len(proj)
    order = np.argsort(cam_idx, kind="stable")
    kp_ptr = np.concatenate([[0], np.cumsum(np.bincount(cam_idx, minlength=n_cams))]).astype(np.int64)
    obs_kp = np.empty(len(cam_idx), np.int32)
    obs_kp[order] = (np.arange(len(cam_idx)) - kp_ptr[cam_idx[order]]).astype(np.int32)
    kp_xy = np.empty((len(cam_idx), 2))
    kp_xy[kp_ptr[cam_idx] + obs_kp] = uv
    track_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return dict(name=name, proj=proj.reshape(-1, 12), cam_of_image=np.arange(n_cams, dtype=np.int32), kp_ptr=kp_ptr, kp_xy=kp_xy,
                track_ptr=track_ptr, obs_image=cam_idx.astype(np.int32), obs_kp=obs_kp, launch_bound=launch_bound)


def _triangulate_cases():
    """The workloads of measure_triangulate and measure_incremental: (a) a set shaped like the shipped tracks (35 images,
    1,641 tracks of 2 to 12 views, 4 on average), (b) 200 cameras / 100,000 points / 10 views each from sfm_amd.synth with
    both visibility patterns of bench.py."""
    from sfm_amd import synth
    from sfm_amd.rotation import rodrigues
    rng = np.random.default_rng(0)

    def projections(sc):
        return np.stack([sc.K @ np.hstack([rodrigues(c[:3]), c[3:6].reshape(3, 1)]) for c in sc.cams_true])
    cases = []
    sc = synth.make_scene(35, 1641, obs_per_point=None, seed=5, noise_px=0.5, visibility="nearest")
    lengths = np.minimum(2 + rng.geometric(0.4, 1641) - 1 + (rng.random(1641) < 0.64), 12).astype(np.int64)    # mean 4, max 12
    first = rng.integers(0, 35 - lengths + 1)
    keep = np.concatenate([p * 35 + first[p] + np.arange(lengths[p]) for p in range(1641)])                     # neighbouring views
    cases.append(_triangulate_case("shipped_shape_35_images_1641_tracks", projections(sc), sc.cam_idx[keep], sc.uv[keep], lengths, True))
    for vis in ("random", "nearest"):
        sc = synth.make_scene(200, 100000, obs_per_point=10, seed=1004, noise_px=0.5, visibility=vis)
        cases.append(_triangulate_case(f"synth_200_cameras_100000_points_{vis}", projections(sc), sc.cam_idx, sc.uv,
                                       np.full(100000, 10, np.int64), False))
    return cases


def _track_source(d, n_cams, n_tracks, n_obs, kp_xy=None):
    """The 12 arguments the four track calls share after the handle (include/sfm_amd.h), from the device tensors of one
    workload of _triangulate_case: every camera an image, every observation a node; kp_xy replaces the workload's pixels."""
    from sfm_amd.driver import _p
    return (_p(d["proj"]), n_cams, _p(d["cam_of_image"]), n_cams, _p(d["kp_ptr"]), _p(d["kp_xy"] if kp_xy is None else kp_xy),
            n_obs, _p(d["track_ptr"]), n_tracks, _p(d["obs_image"]), _p(d["obs_kp"]), n_obs)


def measure_triangulate(reps=20, emit=None):
    """sfm_triangulate_tracks, inputs resident in HBM, device time of the whole call (camera-centre prologue, counter reset
    and the track kernel) by HIP events around `reps` calls after warm-up, on (a) a set shaped like the shipped tracks (35
    images, 1,641 tracks of 2 to 12 views, 4 on average: launch-bound) and (b) 200 cameras / 100,000 points / 10 views
    each from sfm_amd.synth with both visibility patterns of bench.py, for refine_iters 0 and 5.  Per row: ms,
    observations per second and the share of the HBM stream floor (every input array read once and every output written
    once, over HBM_STREAM_BPS); beside it the time of sfm_triangulate2 on as many two-view tracks as an anchor.  Then, per
    case, rows for sfm_triangulate_tracks_robust beside sfm_triangulate_tracks on the same inputs (refine_iters 5), with
    the observations as they are and with 5 % of them moved by 30 to 100 px, and the share of tracks in the second pass."""
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _dev, _p
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    cases = _triangulate_cases()
    results = []
    for c in cases:
        n_cams, n_tracks, n_obs = len(c["proj"]), len(c["track_ptr"]) - 1, len(c["obs_image"])
        d = {k: _dev(c[k], t, dev) for k, t in (("proj", np.float64), ("cam_of_image", np.int32), ("kp_ptr", np.int64),
                                                ("kp_xy", np.float64), ("track_ptr", np.int64), ("obs_image", np.int32),
                                                ("obs_kp", np.int32))}
        src = _track_source(d, n_cams, n_tracks, n_obs)
        need = C.c_int64(); h.lib.sfm_triangulate_tracks_workspace_bytes(n_cams, C.byref(need))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        X = torch.empty((n_tracks, 3), dtype=torch.float64, device=dev); me = torch.empty(n_tracks, dtype=torch.float64, device=dev)
        st = torch.empty(n_tracks, dtype=torch.int32, device=dev); nv = torch.empty(n_tracks, dtype=torch.int32, device=dev)
        counts = torch.empty(6, dtype=torch.int64, device=dev)
        stream_bytes = (sum(c[k].nbytes for k in ("proj", "cam_of_image", "kp_ptr", "kp_xy", "track_ptr", "obs_image", "obs_kp"))
                        + n_tracks * (24 + 8 + 4 + 4) + 48)
        floor_s = stream_bytes / HBM_STREAM_BPS
        row = {"kernel": "triangulate_tracks", "case": c["name"], "cameras": n_cams, "tracks": n_tracks, "observations": n_obs,
               "stream_bytes": int(stream_bytes), "hbm_stream_floor_ms": floor_s * 1e3, "hbm_stream_Bps_assumed": HBM_STREAM_BPS}
        for iters in (0, 5):
            def run():
                h.call("sfm_triangulate_tracks", *src, 2, iters, C.c_double(4.0), C.c_double(1.0), _p(X), _p(st), _p(nv), _p(me),
                       _p(counts), _p(ws), need.value)
            for _ in range(3):
                run()
            sec = timed(run, reps)
            row.update({f"ms_refine{iters}": sec * 1e3, f"observations_per_s_refine{iters}": n_obs / sec,
                        f"share_of_hbm_stream_floor_refine{iters}": floor_s / sec,
                        f"ok_tracks_refine{iters}": int(counts.cpu().numpy()[0])})
        # anchor: sfm_triangulate2 on as many two-view tracks (the first two observations of every track)
        a = c["track_ptr"][:-1]
        node = c["kp_ptr"][c["obs_image"]] + c["obs_kp"]
        t2 = [_dev(v, t, dev) for v, t in ((c["obs_image"][a], np.int32), (c["obs_image"][a + 1], np.int32),
                                           (c["kp_xy"][node[a]], np.float64), (c["kp_xy"][node[a + 1]], np.float64))]
        valid = torch.empty(n_tracks, dtype=torch.int32, device=dev)

        def tri2():
            h.call("sfm_triangulate2", _p(d["proj"]), n_cams, _p(t2[0]), _p(t2[1]), _p(t2[2]), _p(t2[3]), n_tracks,
                   C.c_double(4.0), _p(X), _p(valid), C.c_void_p(0))
        for _ in range(3):
            tri2()
        row["ms_triangulate2_same_number_of_two_view_tracks"] = timed(tri2, reps) * 1e3
        row["note"] = ("launch-bound: two launches and a counter reset over a few microseconds of work; the share of the stream "
                       "floor says nothing at this size") if c["launch_bound"] else \
                      "gather- and latency-bound: the passes re-read the observations from cache; the floor counts every array once"
        results.append(row)
        if emit:
            emit(row)
        # the robust call beside the plain one on the same inputs in the same run (refine_iters 5), once with the
        # observations as they are and once with 5 % of them moved by 30 to 100 px
        need_r = C.c_int64(); h.lib.sfm_triangulate_tracks_robust_workspace_bytes(n_cams, n_tracks, C.byref(need_r))
        ws_r = torch.empty(need_r.value, dtype=torch.uint8, device=dev)
        ni = torch.empty(n_tracks, dtype=torch.int32, device=dev)
        flags = torch.empty(max(n_obs, 1), dtype=torch.uint8, device=dev)              # the call zeroes it
        rng = np.random.default_rng(7)
        moved = rng.random(n_obs) < 0.05
        ang, rad = rng.uniform(0, 2 * np.pi, int(moved.sum())), rng.uniform(30, 100, int(moved.sum()))
        xy_moved = c["kp_xy"].copy()
        xy_moved[node[moved]] += np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
        for what, xy in (("as they are", d["kp_xy"]), ("5 % moved by 30 to 100 px", _dev(xy_moved, np.float64, dev))):
            src_xy = _track_source(d, n_cams, n_tracks, n_obs, kp_xy=xy)

            def run_plain():
                h.call("sfm_triangulate_tracks", *src_xy, 2, 5, C.c_double(4.0), C.c_double(1.0), _p(X), _p(st), _p(nv), _p(me),
                       _p(counts), _p(ws), need.value)

            def run_robust():
                h.call("sfm_triangulate_tracks_robust", *src_xy, 2, 5, C.c_double(4.0), C.c_double(1.0), _p(X), _p(st), _p(nv),
                       _p(ni), _p(me), _p(flags), _p(counts), _p(ws_r), need_r.value)
            for _ in range(3):
                run_plain()
            sec_plain = timed(run_plain, reps)
            ok_plain = int(counts.cpu().numpy()[0])
            for _ in range(3):
                run_robust()
            sec_robust = timed(run_robust, reps)
            # the length of the device work list, which the header documents as the last of the workspace's three arrays
            up256 = lambda v: (v + 255) // 256 * 256
            at = up256(24 * n_cams) + up256(4 * n_tracks)
            second_pass = int(ws_r[at:at + 4].view(torch.int32).item())
            rrow = {"kernel": "triangulate_tracks_robust", "case": c["name"], "observations_are": what, "cameras": n_cams,
                    "tracks": n_tracks, "observations": n_obs, "ms_triangulate_tracks_refine5": sec_plain * 1e3,
                    "ms_robust_refine5": sec_robust * 1e3, "robust_over_plain": sec_robust / sec_plain,
                    "ok_tracks_plain": ok_plain, "ok_tracks_robust": int(counts.cpu().numpy()[0]),
                    "tracks_in_second_pass": second_pass, "share_of_tracks_in_second_pass": second_pass / max(n_tracks, 1),
                    "observations_rejected": int(((flags[:n_obs] == 0) & (st == 0)[torch.repeat_interleave(
                        torch.arange(n_tracks, device=dev), d["track_ptr"][1:] - d["track_ptr"][:-1])]).sum().item())}
            results.append(rrow)
            if emit:
                emit(rrow)
    return results


def _arc_scene(n_cams, n_pts, seed=21, noise=0.5):
    """The scene of the loop tests at any size: cameras on an arc of 2 radians around the unit cube looking at its centre,
    K of StructureFromMotion, points uniform in the cube seen by 3/8 to 8/8 of the cameras, pixel noise 0.5 px.  Returns
    (Tracks, keypoints per image, K)."""
    from sfm_amd import Tracks
    rng = np.random.default_rng(seed)
    K = np.array([[1228.0, 0, 512], [0, 1228.0, 384], [0, 0, 1]])
    target = np.array([0.5, 0.5, 0.5])
    proj = []
    for a in np.linspace(-1.0, 1.0, n_cams):
        c = target + [6.0 * np.sin(a), 1.5, -6.0 * np.cos(a)]
        z = (target - c) / np.linalg.norm(target - c)
        x = np.cross([0.0, 1.0, 0.0], z); x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        proj.append(K @ np.hstack([R, (-R @ c)[:, None]]))
    proj = np.stack(proj)
    X = rng.uniform(0, 1, (n_pts, 3))
    lengths = np.rint(rng.integers(3, 9, n_pts) * (n_cams / 8.0)).astype(np.int64)
    cam_idx = np.concatenate([np.sort(rng.choice(n_cams, int(n), replace=False)) for n in lengths])
    pt = np.repeat(np.arange(n_pts), lengths)
    hm = np.einsum("oij,oj->oi", proj[cam_idx], np.hstack([X[pt], np.ones((len(pt), 1))]))
    uv = hm[:, :2] / hm[:, 2:3] + rng.normal(0, noise, (len(pt), 2))
    c = _triangulate_case("arc", proj, cam_idx, uv, lengths, False)
    T = Tracks(c["kp_ptr"], c["track_ptr"], c["obs_image"], c["obs_kp"])
    return T, [c["kp_xy"][c["kp_ptr"][i]:c["kp_ptr"][i + 1]] for i in range(n_cams)], K


def measure_incremental(reps=20, emit=None):
    """sfm_tracks_resection and sfm_tracks_evaluate, inputs resident in HBM, device time of the whole call by HIP events
    around `reps` calls after warm-up, on the workloads of measure_triangulate (points: those sfm_triangulate_tracks gives;
    for the resection every second image is unregistered), beside the wall time of the NumPy restatement
    (tests/incremental_reference.py) on the same arrays; then the wall time of reconstruct_tracks on the synthetic scene
    of the loop tests at 36 cameras / 2,000 points."""
    import torch
    from sfm_amd import _lib, reconstruct_tracks
    from sfm_amd.driver import _dev, _p
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        import incremental_reference as ir
    except ImportError:
        ir = None
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    results = []
    for c in _triangulate_cases():
        n_cams, n_tracks, n_obs = len(c["proj"]), len(c["track_ptr"]) - 1, len(c["obs_image"])
        d = {k: _dev(c[k], t, dev) for k, t in (("proj", np.float64), ("cam_of_image", np.int32), ("kp_ptr", np.int64),
                                                ("kp_xy", np.float64), ("track_ptr", np.int64), ("obs_image", np.int32),
                                                ("obs_kp", np.int32))}
        src = _track_source(d, n_cams, n_tracks, n_obs)
        need = C.c_int64(); h.lib.sfm_triangulate_tracks_workspace_bytes(n_cams, C.byref(need))
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        X = torch.empty((n_tracks, 3), dtype=torch.float64, device=dev); me = torch.empty(n_tracks, dtype=torch.float64, device=dev)
        st = torch.empty(n_tracks, dtype=torch.int32, device=dev); nv = torch.empty(n_tracks, dtype=torch.int32, device=dev)
        counts = torch.empty(6, dtype=torch.int64, device=dev)
        h.call("sfm_triangulate_tracks", *src, 2, 5, C.c_double(4.0), C.c_double(1.0), _p(X), _p(st), _p(nv), _p(me), _p(counts),
               _p(ws), need.value)
        has = (st == 0).to(torch.uint8)
        X_h, has_h = X.cpu().numpy(), has.cpu().numpy()
        obs_err = torch.empty(n_obs, dtype=torch.float64, device=dev)

        def evaluate():
            h.call("sfm_tracks_evaluate", *src, _p(X), _p(has), 2, C.c_double(4.0), C.c_double(1.0), _p(st), _p(nv), _p(me),
                   _p(obs_err), _p(counts), _p(ws), need.value)
        for _ in range(3):
            evaluate()
        sec = timed(evaluate, reps)
        row = {"kernel": "tracks_evaluate", "case": c["name"], "cameras": n_cams, "tracks": n_tracks, "observations": n_obs,
               "ms": sec * 1e3, "observations_per_s": n_obs / sec, "ok_tracks": int(counts.cpu().numpy()[0])}
        if ir is not None:
            t0 = time.perf_counter()
            ref = ir.evaluate(c["proj"], c["cam_of_image"], c["kp_ptr"], c["kp_xy"], c["track_ptr"], c["obs_image"], c["obs_kp"],
                              np.where(has_h[:, None] != 0, X_h, 0.0), has_h, max_error=4.0, min_angle_deg=1.0)
            row["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            row["status_equal_numpy"] = bool(np.array_equal(ref["status"], st.cpu().numpy()))
        results.append(row)
        if emit:
            emit(row)
        # resection: every second image unregistered
        cam = c["cam_of_image"].copy()
        cam[::2] = -1
        node_track = np.full(n_obs, -1, np.int32)
        node_track[c["kp_ptr"][c["obs_image"]] + c["obs_kp"]] = np.repeat(np.arange(n_tracks), np.diff(c["track_ptr"]))
        d_cam, d_nt = _dev(cam, np.int32, dev), _dev(node_track, np.int32, dev)
        need_r = C.c_int64(); h.lib.sfm_resection_workspace_bytes(n_obs, C.byref(need_r))
        ws_r = torch.empty(need_r.value, dtype=torch.uint8, device=dev)
        seg_ptr = torch.empty(n_cams + 1, dtype=torch.int64, device=dev); total = torch.empty(1, dtype=torch.int64, device=dev)
        cn = torch.empty(n_obs, dtype=torch.int32, device=dev); ct = torch.empty(n_obs, dtype=torch.int32, device=dev)
        cX = torch.empty((n_obs, 3), dtype=torch.float64, device=dev); cuv = torch.empty((n_obs, 2), dtype=torch.float32, device=dev)

        def resection():
            h.call("sfm_tracks_resection", _p(d["kp_ptr"]), n_cams, n_obs, _p(d["kp_xy"]), _p(d_nt), _p(d_cam), _p(X), _p(has),
                   n_tracks, _p(seg_ptr), _p(cn), _p(ct), _p(cX), _p(cuv), n_obs, _p(total), _p(ws_r), need_r.value)
        for _ in range(3):
            resection()
        sec = timed(resection, reps)
        n_listed = int(total.item())
        row = {"kernel": "tracks_resection", "case": c["name"], "images": n_cams, "nodes": n_obs, "listed": n_listed,
               "ms": sec * 1e3, "nodes_per_s": n_obs / sec}
        if ir is not None:
            t0 = time.perf_counter()
            ref = ir.resection_lists(c["kp_ptr"], c["kp_xy"], node_track, cam, X_h, has_h)
            row["numpy_ms"] = (time.perf_counter() - t0) * 1e3
            row["equal_numpy"] = bool(ref["total"] == n_listed and np.array_equal(ref["corr_node"], cn[:n_listed].cpu().numpy()))
        results.append(row)
        if emit:
            emit(row)
    T, keypoints, K = _arc_scene(36, 2000)
    reconstruct_tracks(T, keypoints, K)                                        # warm-up: module loads, allocator
    t0 = time.perf_counter()
    rec = reconstruct_tracks(T, keypoints, K)
    row = {"kernel": "reconstruct_tracks", "case": "arc_36_cameras_2000_points", "observations": int(T.n_obs),
           "wall_s": time.perf_counter() - t0, "registered": len(rec.order), "points": int(rec.has_point.sum()),
           "bundle_adjustments": sum(1 for e in rec.log if e.get("ba"))}
    results.append(row)
    if emit:
        emit(row)
    return results

def measure_features(reps=20, emit=None):
    """sfm_features_detect + sfm_features_describe on a batch of 36 synthetic 1600 x 1200 images (the scene generator of
    tests/features_reference.py, seeds 100 .. 135), threshold 20, max_features 10,000, images
    resident in HBM: device time of each call by HIP events around `reps` calls, the time of each kernel (group) by the
    library's own event brackets (sfm_set_profiling), and the achieved bytes per second of the score and the blur kernel
    against their unique bytes (one read and one write per pixel each)."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from features_reference import make_scene
    from sfm_amd import _lib, features
    from sfm_amd.driver import _p
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    H, W, n_img, threshold, edge, max_features = 1200, 1600, 36, 20, 31, 10000
    imgs = [make_scene(H, W, seed=100 + k) for k in range(n_img)]
    off = np.arange(n_img + 1, dtype=np.int64) * (H * W)
    heights, widths = np.full(n_img, H, np.int32), np.full(n_img, W, np.int32)
    d_img = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    need = C.c_int64()
    h.check(h.lib.sfm_features_workspace_bytes(n_img, hp(off), C.byref(need)), "sfm_features_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    kp_ptr = torch.empty(n_img + 1, dtype=torch.int64, device=dev)
    rot = features._rot_table(None, 0)

    def detect():
        h.call("sfm_features_detect", _p(d_img), None, hp(off), hp(heights), hp(widths), n_img, threshold, edge, max_features,
               _p(kp_ptr), _p(ws), need.value)
    detect()
    kp = kp_ptr.cpu().numpy()
    n = int(kp[-1])
    xy = torch.empty((n, 2), dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.uint8, device=dev)
    abin = torch.empty(n, dtype=torch.uint8, device=dev)
    desc = torch.empty((n, 32), dtype=torch.uint8, device=dev)

    def describe():
        h.call("sfm_features_describe", _p(d_img), hp(off), hp(heights), hp(widths), n_img, _p(kp_ptr), n, _p(rot), _p(xy),
               _p(score), _p(abin), _p(desc), None, _p(ws), need.value)

    def both():
        detect(); describe()
    for _ in range(3):
        both()
    pixels = n_img * H * W
    row = {"kernel": "features", "images": n_img, "height": H, "width": W, "threshold": threshold, "edge": edge,
           "max_features": max_features, "keypoints": n, "keypoints_per_image_min": int(np.diff(kp).min()),
           "keypoints_per_image_max": int(np.diff(kp).max()),
           "ms_detect": timed(detect, reps) * 1e3, "ms_describe": timed(describe, reps) * 1e3}
    row["pixels_per_s_detect_plus_describe"] = pixels / ((row["ms_detect"] + row["ms_describe"]) * 1e-3)
    h.set_profiling(True)
    h.profile()
    for _ in range(reps):
        both()
    prof = h.profile()
    h.set_profiling(False)
    for slot in ("feat_score", "feat_select", "feat_scatter", "feat_blur", "feat_describe"):
        ms, cnt = prof[slot]
        row[f"ms_{slot}"] = ms / max(cnt, 1)
    for slot in ("feat_score", "feat_blur"):
        row[f"unique_bytes_per_s_{slot}"] = 2 * pixels / (row[f"ms_{slot}"] * 1e-3) if row[f"ms_{slot}"] > 0 else None
        row[f"share_of_hbm_stream_{slot}"] = (row[f"unique_bytes_per_s_{slot}"] or 0.0) / HBM_STREAM_BPS
    if emit:
        emit(row)
    return [row]


def measure_features_pyramid(reps=20, emit=None):
    """The multi-scale feature stage beside the single-scale one in the same run: the 36 synthetic 1600 x 1200 images of
    measure_features, 8 levels at 6/5, threshold 20, max_features 10,000, inputs resident in HBM.  Device time by HIP events
    around `reps` calls after 3 warm-up calls, per image: sfm_features_pyramid, detect + describe on the level batch, the
    two merge calls, their sum, and the ratio of that sum to sfm_features_detect + sfm_features_describe on the 36 images
    alone (the yardstick); beside them the pixel ratio of the level batch to the images, which is what detect + describe
    are expected to scale by.  Not part of measure(): only `--pyramid-only` runs it."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from features_reference import make_scene
    from sfm_amd import _lib, features
    from sfm_amd.driver import _p
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    H, W, n_img, threshold, edge, max_features, n_levels, num, den = 1200, 1600, 36, 20, 31, 10000, 8, 6, 5
    imgs = [make_scene(H, W, seed=100 + k) for k in range(n_img)]
    off = np.arange(n_img + 1, dtype=np.int64) * (H * W)
    heights, widths = np.full(n_img, H, np.int32), np.full(n_img, W, np.int32)
    d_img = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    rot = features._rot_table(None, 0)
    e = lambda *shape, dt=torch.uint8: torch.empty(shape, dtype=dt, device=dev)

    def stage(images, offs, hs, ws, n):
        """(detect, describe, kp_ptr, n_kp, outputs) of the single-scale calls on a batch"""
        need = C.c_int64()
        h.check(h.lib.sfm_features_workspace_bytes(n, hp(offs), C.byref(need)), "sfm_features_workspace_bytes")
        wsp, kp_ptr = e(need.value), e(n + 1, dt=torch.int64)

        def detect():
            h.call("sfm_features_detect", _p(images), None, hp(offs), hp(hs), hp(ws), n, threshold, edge, max_features,
                   _p(kp_ptr), _p(wsp), need.value)
        detect()
        n_kp = int(kp_ptr.cpu().numpy()[-1])
        o = (e(n_kp, 2, dt=torch.int32), e(n_kp), e(n_kp), e(n_kp, 32))

        def describe():
            h.call("sfm_features_describe", _p(images), hp(offs), hp(hs), hp(ws), n, _p(kp_ptr), n_kp, _p(rot), _p(o[0]),
                   _p(o[1]), _p(o[2]), _p(o[3]), None, _p(wsp), need.value)
        return detect, describe, kp_ptr, n_kp, o

    n_slot = n_img * n_levels
    lvl_off, lvl_h, lvl_w = np.zeros(n_slot + 1, np.int64), np.zeros(n_slot, np.int32), np.zeros(n_slot, np.int32)
    h.check(h.lib.sfm_features_pyramid_sizes(n_img, hp(heights), hp(widths), n_levels, num, den, hp(lvl_off), hp(lvl_h),
                                             hp(lvl_w)), "sfm_features_pyramid_sizes")
    need = C.c_int64()
    h.check(h.lib.sfm_features_pyramid_workspace_bytes(n_img, n_levels, C.byref(need)), "sfm_features_pyramid_workspace_bytes")
    pws, lvl_images = e(need.value), e(int(lvl_off[-1]))

    def pyramid():
        h.call("sfm_features_pyramid", _p(d_img), None, hp(off), hp(heights), hp(widths), n_img, n_levels, num, den,
               _p(lvl_images), None, _p(pws), need.value)
    pyramid()
    one_detect, one_describe, _, n_one, _ = stage(d_img, off, heights, widths, n_img)
    lvl_detect, lvl_describe, lvl_kp_ptr, n_lvl, lo = stage(lvl_images, lvl_off, lvl_h, lvl_w, n_slot)
    lvl_describe()
    mneed = C.c_int64()
    h.check(h.lib.sfm_features_merge_workspace_bytes(n_img, n_levels, C.byref(mneed)), "sfm_features_merge_workspace_bytes")
    mws, kp_ptr = e(mneed.value), e(n_img + 1, dt=torch.int64)

    def count():
        h.call("sfm_features_merge_count", _p(lvl_kp_ptr), _p(lo[1]), n_img, n_levels, max_features, _p(kp_ptr), _p(mws),
               mneed.value)
    count()
    kp = kp_ptr.cpu().numpy()
    n = int(kp[-1])
    xy, level, score, abin = e(n, 2, dt=torch.float32), e(n), e(n), e(n)
    desc, src = e(n, 32), e(n, dt=torch.int32)

    def merge():
        count()
        h.call("sfm_features_merge_gather", _p(lvl_kp_ptr), _p(lo[0]), _p(lo[1]), _p(lo[2]), _p(lo[3]), hp(lvl_h), hp(lvl_w),
               n_img, n_levels, _p(kp_ptr), n, _p(xy), _p(level), _p(score), _p(abin), _p(desc), _p(src), _p(mws), mneed.value)

    def lvl_both():
        lvl_detect(); lvl_describe()

    def one_both():
        one_detect(); one_describe()
    for _ in range(3):
        pyramid(); lvl_both(); merge(); one_both()
    per = lambda fn: timed(fn, reps) * 1e3 / n_img
    row = {"kernel": "features_pyramid", "images": n_img, "height": H, "width": W, "n_levels": n_levels, "scale": [num, den],
           "threshold": threshold, "edge": edge, "max_features": max_features, "reps": reps,
           "keypoints_single_scale": n_one, "keypoints_level_batch": n_lvl, "keypoints": n,
           "keypoints_per_level": np.bincount(level.cpu().numpy(), minlength=n_levels).tolist(),
           "pixel_ratio_level_batch": float(lvl_off[-1]) / float(off[-1]),
           "ms_per_image_single_scale": per(one_both), "ms_per_image_pyramid": per(pyramid),
           "ms_per_image_detect_describe_levels": per(lvl_both), "ms_per_image_merge": per(merge)}
    row["ms_per_image_single_scale_again"] = per(one_both)          # the yardstick once more, after the others: its spread
    row["ms_per_image_multi_scale"] = (row["ms_per_image_pyramid"] + row["ms_per_image_detect_describe_levels"] +
                                       row["ms_per_image_merge"])
    row["ratio_multi_scale_to_single_scale"] = row["ms_per_image_multi_scale"] / row["ms_per_image_single_scale"]
    row["ratio_detect_describe_levels_to_single_scale"] = (row["ms_per_image_detect_describe_levels"] /
                                                           row["ms_per_image_single_scale"])
    if emit:
        emit(row)
    return [row]


def measure_guided(reps=20, emit=None):
    """sfm_guided_match with and without cross_check beside the blind batched matcher (knn2_batched + ratio_batched) on
    the same batch in the same run, inputs resident in HBM: the sizes of the matcher row of measure_fundamental (36 images
    x 500 keypoints, all 630 pairs) with ORB-sized descriptors (32 bytes, Hamming).  Keypoints are uniform in 1024 x 768 and
    every pair has the F of one synthetic two-view geometry, so a 3 px gate passes about 1 % of the combinations.  A third
    guided figure with a 0 px gate (no candidate, no descriptor distance) is the gate loop alone."""
    import torch
    from sfm_amd import _lib, matcher
    from sfm_amd.driver import _p
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    n_img, n_kp, dim = 36, 500, 32
    descs = [rng.integers(0, 256, (n_kp, dim)).astype(np.uint8) for _ in range(n_img)]
    kps = [(rng.uniform(0, 1, (n_kp, 2)) * [1024, 768]).astype(np.float32) for _ in range(n_img)]
    pairs = [(i, j) for i in range(n_img) for j in range(i + 1, n_img)]
    yaw = 0.25
    R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    t = np.array([-1.5, 0.1, 0.3])
    K = np.array([[1228.0, 0, 512], [0, 1228.0, 384], [0, 0, 1]])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = np.linalg.inv(K).T @ tx @ R @ np.linalg.inv(K)
    F = F / F[2, 2]
    rows, ptr_h, dim = matcher._upload_sets(descs, dev)
    xy, _, _ = matcher._upload_sets(kps, dev)
    q_beg = np.array([ptr_h[i] for i, _ in pairs], dtype=np.int64); q_end = np.array([ptr_h[i + 1] for i, _ in pairs], dtype=np.int64)
    t_beg = np.array([ptr_h[j] for _, j in pairs], dtype=np.int64); t_end = np.array([ptr_h[j + 1] for _, j in pairs], dtype=np.int64)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    n_rows, n_seg, code = int(rows.shape[0]), len(pairs), _lib.METRIC_HAMMING
    d_F = torch.from_numpy(np.tile(F.reshape(1, 9), (n_seg, 1))).to(dev)
    n_out, need = C.c_int64(), C.c_int64()
    h.check(h.lib.sfm_match_batched_workspace_bytes(code, n_seg, hp(q_beg), hp(q_end), hp(t_beg), hp(t_end), n_rows, n_rows,
                                                    C.byref(n_out), C.byref(need)), "sfm_match_batched_workspace_bytes")
    nq = n_out.value
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    i1, i2, qi, ti, nc = (torch.empty(nq, dtype=torch.int32, device=dev) for _ in range(5))
    e1, e2, dd = (torch.empty(nq, dtype=torch.float32, device=dev) for _ in range(3))
    out_ptr = torch.empty(n_seg + 1, dtype=torch.int64, device=dev); seg_ptr = torch.empty(n_seg + 1, dtype=torch.int64, device=dev)

    def blind():
        h.call("sfm_match_knn2_batched", code, _p(rows), n_rows, _p(rows), n_rows, dim, n_seg, hp(q_beg), hp(q_end), hp(t_beg),
               hp(t_end), _p(i1), _p(i2), _p(e1), _p(e2), _p(out_ptr), _p(ws), need.value)
        h.call("sfm_match_ratio_batched", nq, n_seg, _p(out_ptr), _p(i1), _p(e1), _p(e2), C.c_double(0.75), _p(qi), _p(ti),
               _p(dd), _p(seg_ptr), _p(ws), need.value)
    g_out, g_need = C.c_int64(), C.c_int64()
    h.check(h.lib.sfm_guided_workspace_bytes(code, n_seg, hp(q_beg), hp(q_end), hp(t_beg), hp(t_end), C.byref(g_out), C.byref(g_need)),
            "sfm_guided_workspace_bytes")
    assert g_out.value == nq
    g_ws = torch.empty(g_need.value, dtype=torch.uint8, device=dev)

    def guided(cross, gate=3.0):
        h.call("sfm_guided_match", code, _p(rows), n_rows, dim, _p(xy), n_seg, hp(q_beg), hp(q_end), hp(t_beg), hp(t_end), _p(d_F),
               C.c_double(gate), C.c_double(0.75), C.c_double(-1.0), cross, _p(qi), _p(ti), _p(dd), _p(nc), _p(seg_ptr), _p(g_ws),
               g_need.value)
    for _ in range(3):
        blind(); guided(0); guided(1)
    ms_blind = timed(blind, reps) * 1e3
    n_blind = int(seg_ptr[-1].item())
    ms_fwd = timed(lambda: guided(0), reps) * 1e3
    n_fwd, cand = int(seg_ptr[-1].item()), float(nc.sum().item())
    ms_cross = timed(lambda: guided(1), reps) * 1e3
    n_cross = int(seg_ptr[-1].item())
    ms_gate = timed(lambda: guided(0, 0.0), reps) * 1e3
    combos = float(n_seg) * n_kp * n_kp
    r = {"kernel": "guided_match", "pairs": n_seg, "images": n_img, "keypoints_per_image": n_kp, "descriptor_bytes": dim,
         "gate_px": 3.0, "ratio": 0.75, "ms_blind_match_pairs": ms_blind, "ms_guided": ms_fwd, "ms_guided_cross_check": ms_cross,
         "guided_over_blind": ms_fwd / ms_blind, "guided_cross_check_over_blind": ms_cross / ms_blind,
         "ms_guided_gate_0px": ms_gate, "gate_tests_per_s": combos / (ms_gate * 1e-3), "share_of_combinations_passing": cand / combos,
         "matches_blind": n_blind, "matches_guided": n_fwd, "matches_guided_cross_check": n_cross,
         "note": "whole calls by device events, descriptors / keypoints / F resident; random descriptors, so the match counts say nothing"}
    if emit:
        emit(r)
    return [r]


def measure_mesh_clean(h, dev, nv, nt, triangles, vertices, vnormals, reps=20, strips=(1 << 20, 1 << 22)):
    """sfm_mesh_components, sfm_mesh_clean_mark and sfm_mesh_clean_emit (min_triangles 100) on a mesh that is resident on the
    device, whole calls by HIP events around `reps` calls after 3 warm-up calls, and sfm_mesh_components on the strip whose
    triangle i is (i, i + 1, i + 2) at each size of `strips`: the keys of the "mesh" row they belong to."""
    import torch
    from sfm_amd.driver import _p
    need = C.c_int64()

    def components_of(n_vertices, n_triangles, d_triangles):
        h.check(h.lib.sfm_mesh_components_workspace_bytes(n_vertices, C.byref(need)), "sfm_mesh_components_workspace_bytes")
        ws_bytes = need.value
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = [torch.empty(max(n, 1), dtype=torch.int32, device=dev) for n in (n_vertices, n_triangles, n_vertices, n_vertices, n_vertices)]
        counts = torch.empty(3, dtype=torch.int64, device=dev)

        def run():
            h.call("sfm_mesh_components", n_vertices, n_triangles, _p(d_triangles), *[_p(t) for t in out], _p(counts), _p(ws), ws_bytes)
        for _ in range(3):
            run()
        return run, out, counts

    run_components, (vc, tc, c_root, c_vertices, c_triangles), cc_counts = components_of(nv, nt, triangles)
    nc = int(cc_counts.cpu().numpy()[0])
    sizes = np.sort(c_triangles[:nc].cpu().numpy())[::-1]
    h.check(h.lib.sfm_mesh_clean_workspace_bytes(nv, nt, C.byref(need)), "sfm_mesh_clean_workspace_bytes")
    clean_need = need.value
    clean_ws = torch.empty(clean_need, dtype=torch.uint8, device=dev)
    keep = torch.empty(max(nc, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(3, dtype=torch.int64, device=dev)

    def run_clean_mark():
        h.call("sfm_mesh_clean_mark", nv, nt, nc, _p(vc), _p(tc), _p(c_triangles), 100, 0, _p(keep), _p(counts), _p(clean_ws), clean_need)
    for _ in range(3):
        run_clean_mark()
    kept, nv2, nt2 = (int(c) for c in counts.cpu().numpy())
    vmap = torch.empty(max(nv2, 1), dtype=torch.int32, device=dev)
    tmap = torch.empty(max(nt2, 1), dtype=torch.int32, device=dev)
    tri2 = torch.empty((max(nt2, 1), 3), dtype=torch.int32, device=dev)
    v2 = torch.empty((max(nv2, 1), 3), dtype=torch.float64, device=dev)
    n2 = torch.empty((max(nv2, 1), 3), dtype=torch.float32, device=dev)

    def run_clean_emit():
        h.call("sfm_mesh_clean_emit", nv, nt, nc, _p(vc), _p(tc), _p(keep), _p(triangles), _p(vertices), _p(vnormals), nv2, nt2, _p(vmap), _p(tmap),
               _p(tri2), _p(v2), _p(n2), _p(clean_ws), clean_need)
    for _ in range(3):
        run_clean_emit()
    out = {"ms_mesh_components": timed(run_components, reps) * 1e3, "ms_mesh_clean_mark": timed(run_clean_mark, reps) * 1e3,
           "ms_mesh_clean_emit": timed(run_clean_emit, reps) * 1e3, "mesh_components": nc, "mesh_component_triangles_largest": [int(s) for s in sizes[:8]],
           "mesh_components_below_100_triangles": int((sizes < 100).sum()), "clean_min_triangles": 100, "clean_components_kept": kept,
           "clean_vertices": nv2, "clean_triangles": nt2}
    del vc, tc, c_root, c_vertices, c_triangles, clean_ws, vmap, tmap, tri2, v2, n2
    for n in strips:
        i = torch.arange(n - 2, dtype=torch.int32, device=dev)
        strip = torch.stack([i, i + 1, i + 2], dim=1).contiguous()
        run_strip, _, strip_counts = components_of(n, n - 2, strip)
        assert strip_counts.cpu().numpy().tolist() == [1, 0, 0]
        out[f"ms_mesh_components_strip_{n}"] = timed(run_strip, reps) * 1e3
        del strip, run_strip
    if len(strips) == 2:
        out["mesh_components_strip_ratio"] = out[f"ms_mesh_components_strip_{strips[1]}"] / out[f"ms_mesh_components_strip_{strips[0]}"]
    return out


def measure_mesh_fill(h, dev, nv, nt, triangles, vertices, reps=20, fan=1 << 20):
    """sfm_mesh_edges, sfm_mesh_fill_mark and sfm_mesh_fill_emit (max_edges 16) on a mesh that is resident on the device, whole
    calls by HIP events around `reps` calls after 3 warm-up calls, with the counts they report, and sfm_mesh_edges on a fan of
    `fan` triangles (0, 1 + i, 1 + (i + 1) % fan) about one vertex beside the strip (i, i + 1, i + 2) of as many: the keys of
    the "mesh" row they belong to.  The yardsticks are ms_mesh_components and ms_mesh_clean_mark + ms_mesh_clean_emit of
    the same row."""
    import torch
    from sfm_amd.driver import _p
    need = C.c_int64()

    def edges_of(n_vertices, n_triangles, d_triangles):
        h.call("sfm_mesh_edges_workspace_bytes", n_triangles, C.byref(need))
        ws_bytes = need.value
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = [torch.empty(max(n, 1), dtype=torch.int32, device=dev) for n in (3 * n_triangles,) * 4 + (n_triangles,) * 2]
        counts = torch.empty(8, dtype=torch.int64, device=dev)

        def run():
            h.call("sfm_mesh_edges", n_vertices, n_triangles, _p(d_triangles), *[_p(t) for t in out], _p(counts), _p(ws), ws_bytes)
        for _ in range(3):
            run()
        return run, out, counts, ws_bytes

    run_edges, (uses, twin, nxt, loop, leader, length), e_counts, edges_ws_bytes = edges_of(nv, nt, triangles)
    ec = [int(c) for c in e_counts.cpu().numpy()]
    n_loops = ec[4]
    h.check(h.lib.sfm_mesh_fill_workspace_bytes(nt, C.byref(need)), "sfm_mesh_fill_workspace_bytes")
    fill_need = need.value
    fill_ws = torch.empty(fill_need, dtype=torch.uint8, device=dev)
    flags = torch.empty(max(3 * nt, 1), dtype=torch.int32, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)

    def run_fill_mark():
        h.call("sfm_mesh_fill_mark", nv, nt, _p(triangles), _p(nxt), n_loops, _p(leader), 16, _p(flags), _p(counts), _p(fill_ws), fill_need)
    for _ in range(3):
        run_fill_mark()
    filled, n_tri, n_open, status = (int(c) for c in counts.cpu().numpy())
    fv = torch.empty((max(filled, 1), 3), dtype=torch.float64, device=dev)
    fn = torch.empty((max(filled, 1), 3), dtype=torch.float32, device=dev)
    name = torch.empty(max(filled, 1), dtype=torch.int32, device=dev)
    ft = torch.empty((max(n_tri, 1), 3), dtype=torch.int32, device=dev)
    fh = torch.empty(max(n_tri, 1), dtype=torch.int32, device=dev)

    def run_fill_emit():
        h.call("sfm_mesh_fill_emit", nv, nt, _p(triangles), _p(nxt), n_loops, _p(leader), _p(flags), _p(vertices), filled, n_tri, _p(fv), _p(fn), _p(name),
               _p(ft), _p(fh), _p(fill_ws), fill_need)
    for _ in range(3):
        run_fill_emit()
    lengths = np.sort(length[:n_loops].cpu().numpy())
    out = {"ms_mesh_edges": timed(run_edges, reps) * 1e3, "ms_mesh_fill_mark": timed(run_fill_mark, reps) * 1e3,
           "ms_mesh_fill_emit": timed(run_fill_emit, reps) * 1e3, "mesh_edges": ec[0], "mesh_boundary_edges": ec[1], "mesh_inconsistent_edges": ec[2],
           "mesh_nonmanifold_edges": ec[3], "mesh_short_loops": ec[4], "mesh_long_boundary_edges": ec[5], "mesh_edges_status": ec[7],
           "mesh_short_loop_edges": {str(int(k)): int((lengths == k).sum()) for k in np.unique(lengths)}, "mesh_edges_workspace_bytes": edges_ws_bytes,
           "fill_max_edges": 16, "fill_sub_loops": filled, "fill_triangles": n_tri, "fill_left_open": n_open, "fill_status": status}
    del uses, twin, nxt, loop, leader, length, fill_ws, flags, fv, fn, name, ft, fh
    i = torch.arange(fan, dtype=torch.int32, device=dev)
    for shape, tri, n_vertices, want in (("fan", torch.stack([torch.zeros_like(i), 1 + i, 1 + (i + 1) % fan], dim=1).contiguous(), fan + 1, [2 * fan, fan]),
                                         ("strip", torch.stack([i, i + 1, i + 2], dim=1).contiguous(), fan + 2, [2 * fan + 1, fan + 2])):
        run, _, shape_counts, _ = edges_of(n_vertices, fan, tri)
        assert shape_counts.cpu().numpy().tolist()[:2] == want
        out[f"ms_mesh_edges_{shape}_{fan}"] = timed(run, reps) * 1e3
        del tri, run
    out["mesh_edges_fan_over_strip"] = out[f"ms_mesh_edges_fan_{fan}"] / out[f"ms_mesh_edges_strip_{fan}"]
    return out


def measure_mesh_smooth(h, dev, nv, nt, triangles, vertices, iterations=10, reps=20):
    """sfm_mesh_adjacency, sfm_mesh_smooth (`iterations` Taubin iterations at 0.5 | -0.53, boundary pinned) and
    sfm_mesh_vertex_normals on a mesh that is resident on the device: whole calls by HIP events around `reps` calls after 3
    warm-up calls, with the counts they report.  The yardstick is ms_mesh_edges of the same row, one radix sort plus passes on
    half as many keys."""
    import torch
    from sfm_amd.driver import _p
    need = C.c_int64()
    h.call("sfm_mesh_adjacency_workspace_bytes", nv, nt, C.byref(need))
    adj_bytes = need.value
    adj_ws = torch.empty(adj_bytes, dtype=torch.uint8, device=dev)
    ptr = torch.empty(nv + 1, dtype=torch.int32, device=dev)
    index = torch.empty(max(6 * nt, 1), dtype=torch.int32, device=dev)
    flags = torch.empty(max(nv, 1), dtype=torch.uint8, device=dev)
    a_counts, s_counts = torch.empty(4, dtype=torch.int64, device=dev), torch.empty(5, dtype=torch.int64, device=dev)

    def run_adjacency():
        h.call("sfm_mesh_adjacency", nv, nt, _p(triangles), _p(ptr), _p(index), _p(flags), _p(a_counts), _p(adj_ws), adj_bytes)
    for _ in range(3):
        run_adjacency()
    entries, boundary, isolated, unsound = (int(c) for c in a_counts.cpu().numpy())
    h.call("sfm_mesh_smooth_workspace_bytes", nv, C.byref(need))
    smooth_bytes = need.value
    smooth_ws = torch.empty(smooth_bytes, dtype=torch.uint8, device=dev)
    moved = torch.empty((max(nv, 1), 3), dtype=torch.float64, device=dev)
    state = torch.empty(max(nv, 1), dtype=torch.uint8, device=dev)

    def run_smooth(n=iterations):
        h.call("sfm_mesh_smooth", nv, _p(vertices), _p(ptr), _p(index), entries, _p(flags), None, 1, C.c_double(0.5), C.c_double(-0.53), 1, n, _p(moved),
               _p(state), _p(s_counts), _p(smooth_ws), smooth_bytes)
    for _ in range(3):
        run_smooth()
    sc = [int(c) for c in s_counts.cpu().numpy()]
    h.call("sfm_mesh_vertex_normals_workspace_bytes", nv, nt, C.byref(need))
    normals_bytes = need.value
    normals_ws = torch.empty(normals_bytes, dtype=torch.uint8, device=dev)
    normals = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev)

    def run_normals():
        h.call("sfm_mesh_vertex_normals", nv, nt, _p(moved), _p(triangles), _p(normals), _p(normals_ws), normals_bytes)
    for _ in range(3):
        run_normals()
    out = {"smooth_iterations": iterations, "ms_mesh_adjacency": timed(run_adjacency, reps) * 1e3, "ms_mesh_smooth": timed(run_smooth, reps) * 1e3,
           "ms_mesh_smooth_1_iteration": timed(lambda: run_smooth(1), reps) * 1e3, "ms_mesh_vertex_normals": timed(run_normals, reps) * 1e3,
           "adjacency_entries": entries, "adjacency_boundary_vertices": boundary, "adjacency_isolated_vertices": isolated, "adjacency_unsound_triangles": unsound,
           "smooth_pinned_boundary": sc[0], "smooth_unsound_vertices": sc[2], "smooth_isolated": sc[3], "smooth_status": sc[4],
           "mean_vertex_degree": entries / nv if nv else 0.0, "adjacency_workspace_bytes": adj_bytes, "smooth_workspace_bytes": smooth_bytes,
           "vertex_normals_workspace_bytes": normals_bytes}
    out["ms_mesh_smooth_per_step"] = out["ms_mesh_smooth"] / (2 * iterations)
    out["smooth_vertex_steps_per_s"] = nv * 2 * iterations / (out["ms_mesh_smooth"] * 1e-3)
    return out


def measure_mesh_decimate(h, dev, nv, nt, triangles, vertices, vnormals, voxel, view_args, render_args, reps=20):
    """sfm_mesh_decimate_cluster, sfm_mesh_decimate_mark and sfm_mesh_decimate_emit on a mesh that is resident on the device, at
    cells of 2 and 4 voxels from the per-axis minimum of the vertices, with the mean and with the quadric: whole calls by HIP
    events around `reps` calls after 3 warm-up calls, with the counts they report.  The yardstick is ms_mesh_edges of the same
    row, one radix sort of 3 nt keys.  Then what the feature buys: sfm_mesh_texture (texels 8) and sfm_mesh_render of the mesh
    decimated at factor 2 with the quadric, beside ms_mesh_texture and ms_mesh_render of the full mesh in the same row.
    view_args: the arguments of sfm_mesh_texture up to the channel count; render_args: (n_img, heights, widths, d_proj, n_out)."""
    import torch
    from sfm_amd import mesh as mm
    from sfm_amd.driver import _p
    hp = lambda a: C.c_void_p(a.ctypes.data)
    need = C.c_int64()
    h.call("sfm_mesh_decimate_workspace_bytes", nv, nt, C.byref(need))
    ws_bytes = need.value
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    per = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    vc, start, first, size = per(nv), per(nv + 1), per(nv), per(nv)
    keep = torch.empty(max(nt, 1), dtype=torch.uint8, device=dev)
    counts, marks = torch.empty(2, dtype=torch.int64, device=dev), torch.empty(5, dtype=torch.int64, device=dev)
    origin = np.ascontiguousarray(vertices[:nv].amin(0).cpu().numpy(), dtype=np.float64) if nv else np.zeros(3)
    out = {"decimate_workspace_bytes": ws_bytes}
    kept_mesh = None
    for factor in (2, 4):
        cell = float(factor) * voxel

        def run_cluster():
            h.call("sfm_mesh_decimate_cluster", nv, nt, _p(vertices), hp(origin), C.c_double(cell), _p(vc), _p(start), _p(first), _p(size), _p(counts), _p(ws),
                   ws_bytes)
        for _ in range(3):
            run_cluster()
        nc, bad = (int(c) for c in counts.cpu().numpy())

        def run_mark():
            h.call("sfm_mesh_decimate_mark", nv, nt, nc, _p(triangles), _p(vc), _p(keep), _p(marks), _p(ws), ws_bytes)
        for _ in range(3):
            run_mark()
        kept, unsound, degenerate, dropped, status = (int(c) for c in marks.cpu().numpy())
        v2 = torch.empty((max(nc, 1), 3), dtype=torch.float64, device=dev)
        n2 = torch.empty((max(nc, 1), 3), dtype=torch.float32, device=dev)
        placed = torch.empty(max(nc, 1), dtype=torch.uint8, device=dev)
        t2 = torch.empty((max(kept, 1), 3), dtype=torch.int32, device=dev)
        tmap = per(kept)
        key = f"decimate_{factor}"
        out.update({f"ms_{key}_cluster": timed(run_cluster, reps) * 1e3, f"ms_{key}_mark": timed(run_mark, reps) * 1e3, f"{key}_clusters": nc,
                    f"{key}_triangles": kept, f"{key}_degenerate": degenerate, f"{key}_cancelled": dropped, f"{key}_unsound_vertices": bad,
                    f"{key}_unsound_triangles": unsound, f"{key}_status": status})
        for placement, name in ((0, "mean"), (1, "quadric")):
            def run_emit():
                h.call("sfm_mesh_decimate_emit", nv, nt, nc, _p(vertices), _p(vnormals), _p(triangles), _p(vc), _p(start), _p(keep), hp(origin),
                       C.c_double(cell), placement, nc, kept, _p(v2), _p(n2), _p(placed), _p(t2), _p(tmap), _p(ws), ws_bytes)
            for _ in range(3):
                run_emit()
            out[f"ms_{key}_emit_{name}"] = timed(run_emit, reps) * 1e3
        out[f"{key}_placed_by_quadric"] = int(placed[:nc].sum().item())
        out[f"ms_{key}_quadric"] = out[f"ms_{key}_cluster"] + out[f"ms_{key}_mark"] + out[f"ms_{key}_emit_quadric"]
        if factor == 2:
            kept_mesh = (nc, kept, v2, n2, t2)
    # the texture and the render of the mesh decimated at factor 2 (the quadric's vertices are the last ones written)
    nc, kept, v2, n2, t2 = kept_mesh
    texels, cells_per_row, aw, ah = 8, mm.check_texture_layout(kept, 8, None)[0], C.c_int32(), C.c_int32()
    h.check(h.lib.sfm_mesh_texture_size(kept, texels, cells_per_row, C.byref(aw), C.byref(ah)), "sfm_mesh_texture_size")
    aw, ah = aw.value, ah.value
    n_img, heights, widths, d_proj, n_out = render_args
    h.check(h.lib.sfm_mesh_texture_workspace_bytes(n_img, C.byref(need)), "sfm_mesh_texture_workspace_bytes")
    texture_need = need.value
    texture_ws = torch.empty(texture_need, dtype=torch.uint8, device=dev)
    atlas = torch.empty(max(ah * aw * 3, 1), dtype=torch.uint8, device=dev)
    aviews = torch.empty(max(ah * aw, 1), dtype=torch.uint8, device=dev)
    auv = torch.empty(max(kept * 6, 1), dtype=torch.float32, device=dev)

    def run_texture():
        h.call("sfm_mesh_texture", *view_args, nc, _p(v2), _p(n2), kept, _p(t2), texels, cells_per_row, C.c_double(3.0 * voxel), C.c_double(0.35), 0,
               _p(atlas), _p(aviews), _p(auv), _p(texture_ws), texture_need)
    for _ in range(3):
        run_texture()
    h.check(h.lib.sfm_mesh_render_workspace_bytes(n_img, hp(heights), hp(widths), nc, kept, C.byref(need)), "sfm_mesh_render_workspace_bytes")
    render_need = need.value
    render_ws = torch.empty(render_need, dtype=torch.uint8, device=dev)
    r_depth = torch.empty(n_out, dtype=torch.float32, device=dev)
    r_tri = torch.empty(n_out, dtype=torch.int32, device=dev)
    r_bary = torch.empty(n_out * 3, dtype=torch.float32, device=dev)
    r_color = torch.empty(n_out * 3, dtype=torch.uint8, device=dev)

    def run_render():
        h.call("sfm_mesh_render", n_img, hp(heights), hp(widths), _p(d_proj), nc, _p(v2), kept, _p(t2), 2, 3, None, _p(auv), _p(atlas), aw, ah, 0,
               _p(r_depth), _p(r_tri), _p(r_bary), _p(r_color), _p(render_ws), render_need)
    for _ in range(3):
        run_render()
    out.update({"decimate_2_texture_atlas": [aw, ah], "ms_decimate_2_mesh_texture": timed(run_texture, reps) * 1e3,
                "ms_decimate_2_mesh_render": timed(run_render, reps) * 1e3, "decimate_2_render_share_of_pixels_drawn": float((r_tri >= 0).float().mean().item())})
    return out


def measure_depth(reps=20, emit=None, mesh=False):
    """sfm_depth_census, sfm_depth_sweep and sfm_depth_filter on 36 synthetic 1024 x 768 views (the scene generator of
    tests/depth_reference.py: cameras on a line, baseline 0.1, f = 1228), every view a reference with its 4 nearest cameras
    as sources, planes from sfm_amd.depth.plane_depths over 2.5 .. 5, radius 2, inputs resident in HBM: device time of each
    call by HIP events around `reps` calls, per reference view, and the samples (pixels x planes x sources) per second of
    the sweep.  Behind them sfm_depth_fuse_mark and sfm_depth_fuse_gather (rel_tol 0.02, step 2, jump 0.05) on the filter's
    outputs, beside the compaction they replace: torch.nonzero + gather as in DepthMaps.point_cloud().  In the same run
    sfm_features_detect + sfm_features_describe on the same images, as a known quantity.  With mesh=True also the surface
    of the same run: sfm_tsdf_integrate of the 36 filtered maps into 256^3 nodes (a cube around the kept pixels, truncation 3
    voxels), sfm_mesh_mark and sfm_mesh_emit (min_weight 1), then sfm_mesh_colors of that mesh from the 36 views (BGR, tol 3
    voxels, min_cos 0.35) with its vertex-view projections per second, beside it sfm_mesh_exposure_sample and
    sfm_mesh_exposure_gram of the same mesh and views and sfm_images_gain over the 36 images, and sfm_mesh_texture of the same mesh from the same views
    at texels 8 with its texel-view projections per second (the texels of the triangles' patches x views), then sfm_mesh_render
    of that mesh into its 36 views with that atlas (ms per camera, pixels and triangle-camera pairs per second, the length of
    the large-box list), then sfm_render_score of those 36 renders against the 36 images (window 7: once with both maps written and
    the views' depth, once the statistics alone; ms per view and the pooled figures), then the components of that mesh and its cleaning
    at min_triangles 100 (sfm_mesh_components, sfm_mesh_clean_mark, sfm_mesh_clean_emit) and sfm_mesh_components on the ascending strip
    at 2^20 and 2^22 vertices with the ratio of the two times (`measure_mesh_clean`), then the edge table of that mesh and the filling of
    its holes at max_edges 16 (sfm_mesh_edges, sfm_mesh_fill_mark, sfm_mesh_fill_emit) and sfm_mesh_edges on a fan and on a strip of 2^20
    triangles (`measure_mesh_fill`), then its adjacency, ten Taubin iterations and the normals of the moved faces (sfm_mesh_adjacency,
    sfm_mesh_smooth, sfm_mesh_vertex_normals; `measure_mesh_smooth`), then the decimation of that mesh at cells of 2 and 4 voxels with both placements (sfm_mesh_decimate_cluster,
    sfm_mesh_decimate_mark, sfm_mesh_decimate_emit) and sfm_mesh_texture and sfm_mesh_render of the decimated mesh (`measure_mesh_decimate`),
    whole calls by HIP events; the row is then named "mesh"."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from depth_reference import make_scene
    from sfm_amd import _lib, depth as dm, features
    from sfm_amd.driver import _p
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    n_img, W, H, radius, n_src = 36, 1024, 768, 2, 4
    sc = make_scene(n_cams=n_img, width=W, height=H, f=1228.0, baseline=0.1)
    refs = list(range(n_img))
    sources = {r: sorted(sorted((s for s in refs if s != r), key=lambda s: (abs(s - r), s))[:n_src]) for r in refs}
    planes = {r: dm.plane_depths(sc.d_min, sc.d_max, dm.view_warps(sc.K, sc.poses, r, sources[r]), sc.size) for r in refs}
    imgs, refs, src_ptr, src_image, warps, backproj, plane_ptr, depths = dm.check_arguments(sc.images, sc.K, sc.poses, sources, planes, radius)
    off = np.arange(n_img + 1, dtype=np.int64) * (H * W)
    heights, widths = np.full(n_img, H, np.int32), np.full(n_img, W, np.int32)
    ref_image = np.array(refs, dtype=np.int32)
    d_img = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(dev)
    d_warps, d_back, d_planes = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (warps, backproj, depths))
    hp = lambda a: C.c_void_p(a.ctypes.data)
    need = C.c_int64()
    h.check(h.lib.sfm_depth_workspace_bytes(n_img, n_img, len(src_image), C.byref(need)), "sfm_depth_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    n_out = n_img * H * W
    census = torch.empty(n_out, dtype=torch.int64, device=dev)
    plane = torch.empty(n_out, dtype=torch.int32, device=dev)
    cost = torch.empty(n_out, dtype=torch.int16, device=dev)
    depth = torch.empty(n_out, dtype=torch.float32, device=dev)
    ncons = torch.empty(n_out, dtype=torch.uint8, device=dev)
    keep = torch.empty(n_out, dtype=torch.uint8, device=dev)
    xyz = torch.empty((n_out, 3), dtype=torch.float64, device=dev)
    limit = np.array([12 * (src_ptr[v + 1] - src_ptr[v]) * (2 * radius + 1) ** 2 for v in range(n_img)], dtype=np.int32)

    def run_census():
        h.call("sfm_depth_census", _p(d_img), hp(off), hp(heights), hp(widths), n_img, _p(census), _p(ws), need.value)

    def run_sweep():
        h.call("sfm_depth_sweep", _p(census), hp(off), hp(heights), hp(widths), n_img, n_img, hp(ref_image), hp(src_ptr), hp(src_image),
               _p(d_warps), hp(plane_ptr), _p(d_planes), radius, _p(plane), _p(cost), _p(depth), _p(ws), need.value)

    def run_filter():
        h.call("sfm_depth_filter", hp(off), hp(heights), hp(widths), n_img, n_img, hp(ref_image), hp(src_ptr), hp(src_image),
               _p(d_warps), _p(d_back), _p(depth), _p(cost), hp(limit), C.c_double(0.02), 2, _p(ncons), _p(keep), _p(xyz), _p(ws), need.value)
    run_census(); run_sweep(); run_filter()
    samples = int(sum(H * W * (plane_ptr[v + 1] - plane_ptr[v]) * (src_ptr[v + 1] - src_ptr[v]) for v in range(n_img)))
    truth = np.stack(sc.depth)
    z = depth.cpu().numpy().reshape(n_img, H, W)
    kept = keep.cpu().numpy().reshape(n_img, H, W).astype(bool)
    row = {"kernel": "depth", "views": n_img, "height": H, "width": W, "radius": radius, "sources_per_view": n_src,
           "planes_min": int(np.diff(plane_ptr).min()), "planes_max": int(np.diff(plane_ptr).max()), "samples": samples,
           "share_kept": float(kept.mean()), "share_of_kept_within_2_percent_of_truth": float((np.abs(z - truth) <= 0.02 * truth)[kept].mean()),
           "ms_census_per_view": timed(run_census, reps) * 1e3 / n_img, "ms_sweep_per_view": timed(run_sweep, reps) * 1e3 / n_img,
           "ms_filter_per_view": timed(run_filter, reps) * 1e3 / n_img}
    row["samples_per_s_sweep"] = samples / (row["ms_sweep_per_view"] * n_img * 1e-3)
    # the fusion behind the filter; beside it what it replaces: the compaction of point_cloud() (torch.nonzero + gather)
    h.check(h.lib.sfm_depth_fuse_workspace_bytes(n_img, n_img, len(src_image), n_out, C.byref(need)), "sfm_depth_fuse_workspace_bytes")
    fuse_ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    normal_map = torch.empty((n_out, 3), dtype=torch.float32, device=dev)
    agree_mask = torch.empty(n_out, dtype=torch.uint8, device=dev)
    owner = torch.empty(n_out, dtype=torch.uint8, device=dev)
    pt_ptr = torch.empty(n_img + 1, dtype=torch.int64, device=dev)
    views = (hp(off), hp(heights), hp(widths), n_img, n_img, hp(ref_image), hp(src_ptr), hp(src_image), _p(d_warps))

    def run_mark():
        h.call("sfm_depth_fuse_mark", *views, _p(d_back), _p(depth), _p(keep), _p(xyz), C.c_double(0.02), 2, C.c_double(0.05),
               _p(normal_map), _p(agree_mask), _p(owner), _p(pt_ptr), _p(fuse_ws), need.value)
    run_mark()
    m = int(pt_ptr.cpu().numpy()[-1])
    points = torch.empty((max(m, 1), 3), dtype=torch.float64, device=dev)
    normals = torch.empty((max(m, 1), 3), dtype=torch.float32, device=dev)
    n_views = torch.empty(max(m, 1), dtype=torch.uint8, device=dev)
    index = torch.empty((max(m, 1), 3), dtype=torch.int32, device=dev)

    def run_gather():
        h.call("sfm_depth_fuse_gather", *views, _p(depth), _p(xyz), _p(normal_map), _p(agree_mask), _p(owner), _p(pt_ptr), m,
               _p(points), _p(normals), _p(n_views), _p(index), _p(fuse_ws), need.value)

    def run_point_cloud():
        return xyz[torch.nonzero(keep, as_tuple=False).reshape(-1)]
    run_gather()
    z_fused = points[:m, 2].cpu().numpy()
    idx = index[:m].cpu().numpy()
    t_fused = truth[idx[:, 0], idx[:, 1], idx[:, 2]]
    row.update({"fused_points": m, "fused_share_of_kept": m / max(int(kept.sum()), 1),
                "share_of_fused_with_normal": float((normals[:m] != 0).any(dim=1).float().mean().item()) if m else 0.0,
                "share_of_fused_within_2_percent_of_truth": float((np.abs(z_fused - t_fused) <= 0.02 * t_fused).mean()) if m else 0.0,
                "ms_fuse_mark_per_view": timed(run_mark, reps) * 1e3 / n_img, "ms_fuse_gather_per_view": timed(run_gather, reps) * 1e3 / n_img,
                "ms_point_cloud_nonzero_gather_per_view": timed(run_point_cloud, reps) * 1e3 / n_img})
    del normal_map, agree_mask, owner, points, normals, n_views, index, fuse_ws
    if mesh:
        from sfm_amd import mesh as mm
        row["kernel"] = "mesh"
        sub = xyz[torch.nonzero(keep, as_tuple=False).reshape(-1)[::64]].cpu().numpy()
        lo, voxel, box = mm.bounding_grid(sub, 256, 0.05)
        nx = ny = nz = 256                                         # a cube: the shorter sides of the box are centred in it
        origin = np.ascontiguousarray(lo + 0.5 * voxel * (np.array(box) - 1) - 0.5 * voxel * 255, dtype=np.float64)
        d_proj = torch.from_numpy(mm.projections_from_backprojections(backproj)).to(dev)
        h.check(h.lib.sfm_tsdf_workspace_bytes(n_img, C.byref(need)), "sfm_tsdf_workspace_bytes")
        tsdf_need = need.value
        tsdf_ws = torch.empty(tsdf_need, dtype=torch.uint8, device=dev)
        h.check(h.lib.sfm_mesh_workspace_bytes(nx, ny, nz, C.byref(need)), "sfm_mesh_workspace_bytes")
        mesh_need = need.value
        mesh_ws = torch.empty(mesh_need, dtype=torch.uint8, device=dev)
        tsdf = torch.empty(nx * ny * nz, dtype=torch.float32, device=dev)
        weight = torch.empty(nx * ny * nz, dtype=torch.int16, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)

        def run_integrate():
            h.call("sfm_tsdf_integrate", hp(heights), hp(widths), n_img, n_img, hp(ref_image), _p(d_proj), _p(depth), _p(keep), hp(origin),
                   C.c_double(voxel), nx, ny, nz, C.c_double(3.0 * voxel), _p(tsdf), _p(weight), _p(tsdf_ws), tsdf_need)

        def run_mesh_mark():
            h.call("sfm_mesh_mark", _p(tsdf), _p(weight), nx, ny, nz, 1, _p(counts), _p(mesh_ws), mesh_need)
        run_integrate(); run_mesh_mark()
        nv, nt = (int(c) for c in counts.cpu().numpy())
        vertices = torch.empty((max(nv, 1), 3), dtype=torch.float64, device=dev)
        vnormals = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev)
        triangles = torch.empty((max(nt, 1), 3), dtype=torch.int32, device=dev)

        def run_mesh_emit():
            h.call("sfm_mesh_emit", _p(tsdf), nx, ny, nz, hp(origin), C.c_double(voxel), nv, nt, _p(vertices), _p(vnormals), _p(triangles),
                   _p(mesh_ws), mesh_need)
        run_mesh_emit()
        # the colours of the same mesh: BGR images (the gray ones in three channels), the defaults of Mesh.colors
        d_bgr = d_img[:, None].expand(-1, 3).contiguous()
        d_centres = torch.from_numpy(np.ascontiguousarray(np.asarray(backproj).reshape(-1, 3, 4)[:, :, 3])).to(dev)
        h.check(h.lib.sfm_mesh_colors_workspace_bytes(n_img, C.byref(need)), "sfm_mesh_colors_workspace_bytes")
        colors_need = need.value
        colors_ws = torch.empty(colors_need, dtype=torch.uint8, device=dev)
        vcolors = torch.empty((max(nv, 1), 3), dtype=torch.uint8, device=dev)
        vviews = torch.empty(max(nv, 1), dtype=torch.uint8, device=dev)
        vbest = torch.empty(max(nv, 1), dtype=torch.int32, device=dev)

        def run_mesh_colors():
            h.call("sfm_mesh_colors", hp(heights), hp(widths), n_img, n_img, hp(ref_image), _p(d_proj), _p(d_centres), _p(depth), _p(keep),
                   _p(d_bgr), 3, nv, _p(vertices), _p(vnormals), C.c_double(3.0 * voxel), C.c_double(0.35), 0, _p(vcolors), _p(vviews),
                   _p(vbest), _p(colors_ws), colors_need)
        run_mesh_colors()
        # the exposure stage on the same mesh and views, beside the colour call above as its yardstick: the samples, the two
        # tables, and the gains applied to the 36 images (a gain of 0.9 .. 1.1 per image and channel)
        h.check(h.lib.sfm_mesh_exposure_workspace_bytes(n_img, 3, nv, C.byref(need)), "sfm_mesh_exposure_workspace_bytes")
        exposure_need = need.value
        exposure_ws = torch.empty(exposure_need, dtype=torch.uint8, device=dev)
        e_seen = torch.empty(max(n_img * nv, 1), dtype=torch.uint8, device=dev)
        e_samples = torch.empty(max(n_img * 3 * nv, 1), dtype=torch.uint8, device=dev)
        e_overlap = torch.empty(n_img * n_img, dtype=torch.int64, device=dev)
        e_sums = torch.empty(n_img * n_img * 3, dtype=torch.int64, device=dev)
        e_gained = torch.empty_like(d_bgr)
        e_gains = np.ascontiguousarray(np.random.default_rng(0).uniform(0.9, 1.1, (n_img, 3)))

        def run_exposure_sample():
            h.call("sfm_mesh_exposure_sample", hp(heights), hp(widths), n_img, n_img, hp(ref_image), _p(d_proj), _p(d_centres), _p(depth), _p(keep),
                   _p(d_bgr), 3, nv, _p(vertices), _p(vnormals), C.c_double(3.0 * voxel), C.c_double(0.35), _p(e_seen), _p(e_samples),
                   _p(exposure_ws), exposure_need)

        def run_exposure_gram():
            h.call("sfm_mesh_exposure_gram", n_img, 3, nv, _p(e_seen), _p(e_samples), _p(e_overlap), _p(e_sums), _p(exposure_ws), exposure_need)

        def run_images_gain():
            h.call("sfm_images_gain", hp(heights), hp(widths), n_img, 3, hp(e_gains), _p(d_bgr), _p(e_gained))
        for _ in range(3):
            run_exposure_sample(); run_exposure_gram(); run_images_gain()
        e_plan = (C.c_int32 * 4)()
        h.check(h.lib.sfm_mesh_exposure_plan(n_img, 3, nv, e_plan), "sfm_mesh_exposure_plan")
        ov = e_overlap.cpu().numpy().reshape(n_img, n_img)
        row.update({"ms_mesh_exposure_sample": timed(run_exposure_sample, reps) * 1e3, "ms_mesh_exposure_gram": timed(run_exposure_gram, reps) * 1e3,
                    "ms_images_gain": timed(run_images_gain, reps) * 1e3, "ms_mesh_colors_beside_exposure": timed(run_mesh_colors, reps) * 1e3,
                    "exposure_gram_workgroups": int(e_plan[3]), "exposure_gram_multiply_adds": n_img * n_img * nv * 4,
                    "exposure_pairs_with_common_vertices": int((np.triu(ov, 1) > 0).sum()), "exposure_largest_overlap": int(np.triu(ov, 1).max()),
                    "exposure_vertices_seen_per_view": float(np.diag(ov).mean()), "gain_bytes": int(d_bgr.numel())})
        row["gain_bytes_per_s_read_plus_written"] = 2 * row["gain_bytes"] / (row["ms_images_gain"] * 1e-3)
        del exposure_ws, e_seen, e_samples, e_overlap, e_sums, e_gained
        # the texture of the same mesh from the same views: texels 8, the square atlas of Mesh.texture; 20 calls after 3
        texels, cells_per_row, aw, ah = 8, mm.check_texture_layout(nt, 8, None)[0], C.c_int32(), C.c_int32()
        h.check(h.lib.sfm_mesh_texture_size(nt, texels, cells_per_row, C.byref(aw), C.byref(ah)), "sfm_mesh_texture_size")
        aw, ah = aw.value, ah.value
        h.check(h.lib.sfm_mesh_texture_workspace_bytes(n_img, C.byref(need)), "sfm_mesh_texture_workspace_bytes")
        texture_need = need.value
        texture_ws = torch.empty(texture_need, dtype=torch.uint8, device=dev)
        atlas = torch.empty(max(ah * aw * 3, 1), dtype=torch.uint8, device=dev)
        aviews = torch.empty(max(ah * aw, 1), dtype=torch.uint8, device=dev)
        auv = torch.empty(max(nt * 6, 1), dtype=torch.float32, device=dev)

        def run_mesh_texture():
            h.call("sfm_mesh_texture", hp(heights), hp(widths), n_img, n_img, hp(ref_image), _p(d_proj), _p(d_centres), _p(depth), _p(keep),
                   _p(d_bgr), 3, nv, _p(vertices), _p(vnormals), nt, _p(triangles), texels, cells_per_row, C.c_double(3.0 * voxel),
                   C.c_double(0.35), 0, _p(atlas), _p(aviews), _p(auv), _p(texture_ws), texture_need)
        for _ in range(3):
            run_mesh_texture()
        owned = nt * (texels + 2) * (texels + 3) // 2              # the texels that belong to a triangle: its patch with the gutter
        with_view = int((aviews[:ah * aw] != 0).sum().item())      # only those can have a view
        row.update({"texture_texels": texels, "texture_cells_per_row": cells_per_row, "texture_atlas": [aw, ah],
                    "texture_share_of_texels_in_a_triangle": owned / max(aw * ah, 1), "texture_share_of_those_with_a_view": with_view / max(owned, 1),
                    "texture_projections": owned * n_img, "ms_mesh_texture": timed(run_mesh_texture, reps) * 1e3})
        row["texture_projections_per_s"] = row["texture_projections"] / (row["ms_mesh_texture"] * 1e-3)
        # the render of the same mesh into its 36 views with that atlas, beside the texture call above as its yardstick
        h.check(h.lib.sfm_mesh_render_workspace_bytes(n_img, hp(heights), hp(widths), nv, nt, C.byref(need)), "sfm_mesh_render_workspace_bytes")
        render_need = need.value
        render_ws = torch.empty(render_need, dtype=torch.uint8, device=dev)
        r_depth = torch.empty(n_out, dtype=torch.float32, device=dev)
        r_tri = torch.empty(n_out, dtype=torch.int32, device=dev)
        r_bary = torch.empty(n_out * 3, dtype=torch.float32, device=dev)
        r_color = torch.empty(n_out * 3, dtype=torch.uint8, device=dev)

        def run_mesh_render():
            h.call("sfm_mesh_render", n_img, hp(heights), hp(widths), _p(d_proj), nv, _p(vertices), nt, _p(triangles), 2, 3, None, _p(auv), _p(atlas),
                   aw, ah, 0, _p(r_depth), _p(r_tri), _p(r_bary), _p(r_color), _p(render_ws), render_need)
        for _ in range(3):
            run_mesh_render()
        ms_render = timed(run_mesh_render, reps) * 1e3
        drawn = r_tri >= 0
        row.update({"render_cameras": n_img, "ms_mesh_render": ms_render, "ms_mesh_render_per_camera": ms_render / n_img,
                    "render_pixels_per_s": n_out / (ms_render * 1e-3), "render_triangle_camera_pairs": nt * n_img,
                    "render_triangle_camera_pairs_per_s": nt * n_img / (ms_render * 1e-3),
                    "render_large_boxes": int(render_ws[:8].cpu().numpy().view(np.uint64)[0]), "render_workspace_bytes": render_need,
                    "render_share_of_pixels_drawn": float(drawn.float().mean().item())})
        # the score of those 36 renders against their photographs (window 7, rel_tol 0.02): once with both maps written and
        # with the views' depth, once the statistics alone; the render above and the filter pass are its yardsticks
        h.check(h.lib.sfm_render_score_workspace_bytes(n_img, hp(heights), hp(widths), C.byref(need)), "sfm_render_score_workspace_bytes")
        score_need = need.value
        score_ws = torch.empty(score_need, dtype=torch.uint8, device=dev)
        s_stats = torch.empty(n_img * 16, dtype=torch.int64, device=dev)
        s_error = torch.empty(n_out * 3, dtype=torch.uint8, device=dev)
        s_ssim = torch.empty(n_out, dtype=torch.float32, device=dev)

        def run_score_full():
            h.call("sfm_render_score", n_img, hp(heights), hp(widths), 3, _p(r_color), _p(r_tri), _p(r_depth), _p(d_bgr), None, _p(depth), _p(keep), 7,
                   C.c_double(0.02), _p(s_stats), _p(s_error), _p(s_ssim), _p(score_ws), score_need)

        def run_score_stats():
            h.call("sfm_render_score", n_img, hp(heights), hp(widths), 3, _p(r_color), _p(r_tri), _p(r_depth), _p(d_bgr), None, None, None, 7,
                   C.c_double(0.02), _p(s_stats), None, None, _p(score_ws), score_need)
        for _ in range(3):
            run_score_stats(); run_score_full()
        ms_score_stats = timed(run_score_stats, reps) * 1e3
        ms_score = timed(run_score_full, reps) * 1e3
        pooled = mm.score_figures(s_stats.cpu().numpy(), 3)
        row.update({"ms_render_score": ms_score, "ms_render_score_per_view": ms_score / n_img, "ms_render_score_stats_only": ms_score_stats,
                    "ms_render_score_stats_only_per_view": ms_score_stats / n_img, "score_pixels_per_s": n_out / (ms_score * 1e-3),
                    "score_window": 7, "score_mae": float(np.mean(pooled["mae"])), "score_psnr": pooled["psnr"], "score_ssim": pooled["ssim"],
                    "score_windows": pooled["n_ssim"], "score_depth_agree": pooled["depth_agree"], "score_render_only": pooled["render_only"],
                    "score_view_only": pooled["view_only"]})
        del score_ws, s_stats, s_error, s_ssim
        del atlas, aviews, auv, texture_ws, render_ws, r_depth, r_tri, r_bary, r_color, drawn
        # the components of the same mesh and its cleaning at min_triangles 100, whole calls, 20 after 3; sfm_mesh_mark and
        # sfm_mesh_emit of this row are their yardsticks.  Then the labelling alone on the ascending strip at 2^20 and 2^22
        # vertices: linear work gives a time ratio of 4, work bound by the chain 16.
        row.update(measure_mesh_clean(h, dev, nv, nt, triangles, vertices, vnormals, reps))
        # the edge table of the same mesh and the filling of its holes at max_edges 16, whole calls, 20 after 3; the labelling
        # and the cleaning above are their yardsticks.  Then the table alone on a fan of 2^20 triangles about one vertex and
        # on a strip of as many: the sort keeps the fan near the strip.
        row.update(measure_mesh_fill(h, dev, nv, nt, triangles, vertices, reps))
        # the adjacency of the same mesh, ten Taubin iterations over it and the normals of the moved faces, whole calls, 20
        # after 3; the edge table above is the yardstick
        row.update(measure_mesh_smooth(h, dev, nv, nt, triangles, vertices, 10, reps))
        # the decimation of the same mesh at cells of 2 and 4 voxels, both placements, whole calls, 20 after 3; the edge table
        # above is the yardstick.  Then the texture and the render of the decimated mesh beside those of the full one above.
        row.update(measure_mesh_decimate(h, dev, nv, nt, triangles, vertices, vnormals, float(voxel),
                                         (hp(heights), hp(widths), n_img, n_img, hp(ref_image), _p(d_proj), _p(d_centres), _p(depth), _p(keep), _p(d_bgr), 3),
                                         (n_img, heights, widths, d_proj, n_out), reps))
        zv =vertices[:nv, 2].cpu().numpy()
        seen = int((weight != 0).sum().item())
        row.update({"grid_nodes": [nx, ny, nz], "voxel": float(voxel), "nodes_seen": seen, "projections": nx * ny * nz * n_img,
                    "mesh_vertices": nv, "mesh_triangles": nt,
                    "share_of_vertices_within_one_voxel_of_a_plane": float((np.minimum(np.abs(zv - sc.z_front), np.abs(zv - sc.z_back)) <= voxel).mean()) if nv else 0.0,
                    "ms_tsdf_integrate": timed(run_integrate, reps) * 1e3, "ms_mesh_mark": timed(run_mesh_mark, reps) * 1e3,
                    "ms_mesh_emit": timed(run_mesh_emit, reps) * 1e3, "ms_mesh_colors": timed(run_mesh_colors, reps) * 1e3,
                    "color_projections": nv * n_img, "share_of_vertices_with_a_view": float((vviews[:nv] != 0).float().mean().item()) if nv else 0.0,
                    "mean_views_per_vertex": float(vviews[:nv].float().mean().item()) if nv else 0.0})
        row["projections_per_s"] = row["projections"] / (row["ms_tsdf_integrate"] * 1e-3)
        row["color_projections_per_s"] = row["color_projections"] / (row["ms_mesh_colors"] * 1e-3)
        del tsdf, weight, vertices, vnormals, triangles, mesh_ws, d_bgr, vcolors, vviews, vbest, colors_ws
    # the known quantity beside it: the feature stage on the same images
    threshold, edge, max_features = 20, 31, 10000
    h.check(h.lib.sfm_features_workspace_bytes(n_img, hp(off), C.byref(need)), "sfm_features_workspace_bytes")
    fws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    kp_ptr = torch.empty(n_img + 1, dtype=torch.int64, device=dev)
    rot = features._rot_table(None, 0)

    def detect():
        h.call("sfm_features_detect", _p(d_img), None, hp(off), hp(heights), hp(widths), n_img, threshold, edge, max_features,
               _p(kp_ptr), _p(fws), need.value)
    detect()
    n = int(kp_ptr.cpu().numpy()[-1])
    xy = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev)
    score = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    abin = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    desc = torch.empty((max(n, 1), 32), dtype=torch.uint8, device=dev)

    def both():
        detect()
        h.call("sfm_features_describe", _p(d_img), hp(off), hp(heights), hp(widths), n_img, _p(kp_ptr), n, _p(rot), _p(xy),
               _p(score), _p(abin), _p(desc), None, _p(fws), need.value)
    row["keypoints"] = n
    row["ms_features_detect_plus_describe_per_view"] = timed(both, reps) * 1e3 / n_img
    if emit:
        emit(row)
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tracks", type=int, default=100000)
    ap.add_argument("--corr", type=int, default=20000)
    ap.add_argument("--fundamental-only", action="store_true", help="only the fundamental-matrix RANSAC rows")
    ap.add_argument("--essential-only", action="store_true", help="only the essential-matrix RANSAC row")
    ap.add_argument("--homography-only", action="store_true", help="only the homography RANSAC rows (beside the fundamental-matrix RANSAC)")
    ap.add_argument("--pnp-only", action="store_true", help="only the PnP RANSAC rows")
    ap.add_argument("--pose-only", action="store_true", help="only the relative-pose recovery rows")
    ap.add_argument("--tracks-only", action="store_true", help="only the track-building rows")
    ap.add_argument("--triangulate-only", action="store_true", help="only the N-view track triangulation rows")
    ap.add_argument("--incremental-only", action="store_true", help="only the resection / evaluation / incremental-loop rows")
    ap.add_argument("--features-only", action="store_true", help="only the feature detection / description row")
    ap.add_argument("--pyramid-only", action="store_true", help="only the multi-scale feature row (beside the single-scale stage on the same images); no other selection runs it")
    ap.add_argument("--guided-only", action="store_true", help="only the guided-matching row (beside the blind matcher)")
    ap.add_argument("--depth-only", action="store_true", help="only the dense-depth row (beside the feature stage on the same images)")
    ap.add_argument("--mesh-only", action="store_true", help="only the meshing row: TSDF integration, mark and emit beside the sweep and the fusion of the same run, and the stages on that mesh up to its components and cleaning, its edge table, the filling of its holes, its smoothing and its decimation")
    a = ap.parse_args()
    emit = lambda d: print(json.dumps(d), flush=True)
    only = a.fundamental_only or a.essential_only or a.homography_only or a.pnp_only or a.pose_only or a.tracks_only or a.triangulate_only or a.incremental_only or \
        a.features_only or a.guided_only or a.depth_only or a.mesh_only or a.pyramid_only
    if not only:
        measure(a.reps, a.tracks, a.corr, emit=emit)
    if a.fundamental_only or not only:
        measure_fundamental(a.reps, emit=emit)
    if a.essential_only or not only:
        measure_essential(a.reps, emit=emit)
    if a.homography_only or not only:
        measure_homography(a.reps, emit=emit)
    if a.pnp_only or not only:
        measure_pnp(a.reps, emit=emit)
    if a.pose_only or not only:
        measure_pose(a.reps, emit=emit)
    if a.tracks_only or not only:
        measure_tracks(a.reps, emit=emit)
    if a.triangulate_only or not only:
        measure_triangulate(a.reps, emit=emit)
    if a.incremental_only or not only:
        measure_incremental(a.reps, emit=emit)
    if a.features_only or not only:
        measure_features(a.reps, emit=emit)
    if a.pyramid_only:
        measure_features_pyramid(a.reps, emit=emit)
    if a.guided_only or not only:
        measure_guided(a.reps, emit=emit)
    if a.depth_only or not only:
        measure_depth(a.reps, emit=emit)
    if a.mesh_only:
        measure_depth(a.reps, emit=emit, mesh=True)


if __name__ == "__main__":
    main()
