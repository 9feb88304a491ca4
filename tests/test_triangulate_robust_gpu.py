"""sfm_triangulate_tracks_robust and sfm_tracks_classify on the device against the NumPy restatement
(tests/triangulate_robust_reference.py).  The integer outputs - status, n_views, n_inliers, obs_inlier, counts - are
demanded exactly; the condition for that is the restatement's margin (the smallest distance of a compared error from
max_error), asserted first.  X and max_err get the rule of tests/test_triangulate_gpu.py: 100 times the restatement's own
float64-against-80-bit deviation on the same inputs, both sides printed.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import triangulate_reference as tr
import triangulate_robust_reference as rr
from test_triangulate_gpu import GATES as PLAIN_GATES, parity_device, parity_scene, take_tracks
from test_triangulate_reference import flat, rel_dev_points, rel_dev_scalars
from test_triangulate_robust_reference import EDGE_OPTIONS, GATES, edge_reference, outlier_reference
from track_calls import judge_raw

pytestmark = pytest.mark.gpu

CLASSIFY_GATES = dict(min_views=2, max_error=4.0, min_angle_deg=1.0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def device(args, **opts):
    from sfm_amd import triangulate_tracks_raw
    return triangulate_tracks_raw(*args, robust=True, **opts)


def plain(args, **opts):
    from sfm_amd import triangulate_tracks_raw
    return triangulate_tracks_raw(*args, **opts)


def obs_rows(track_ptr, tracks):
    idx = [np.arange(track_ptr[t], track_ptr[t + 1]) for t in tracks]
    return np.concatenate(idx).astype(np.int64) if len(idx) else np.zeros(0, np.int64)


def assert_bits(a, b, rows_a=slice(None), rows_b=slice(None)):
    for k in ("status", "n_views", "n_inliers"):
        assert np.array_equal(a[k][rows_a], b[k][rows_b]), k
    for k in ("X", "max_err"):
        assert np.array_equal(bits(a[k][rows_a]), bits(b[k][rows_b])), k


def assert_parity(args, what, **opts):
    """Integer outputs equal to the restatement's; X and max_err within 100 x its own float64-vs-80-bit deviation."""
    ref = rr.triangulate_robust(*args, **opts)
    assert ref["margin"] > 1e-6, (what, ref["margin"])
    ld = rr.triangulate_robust(*args, dtype=np.longdouble, **opts)
    out = device(args, **opts)
    for k in ("status", "n_inliers", "obs_inlier"):
        assert np.array_equal(ld[k], ref[k]), k
    assert out["status"].dtype == np.int32 and out["n_inliers"].dtype == np.int32 and out["obs_inlier"].dtype == np.uint8
    for k in ("status", "n_views", "n_inliers", "obs_inlier", "counts"):
        assert np.array_equal(out[k], ref[k]), (what, k, np.flatnonzero(out[k] != ref[k])[:5])
    ref_x, ref_e = rel_dev_points(ref["X"], ld["X"]), rel_dev_scalars(ref["max_err"], ld["max_err"])
    dev_x, dev_e = rel_dev_points(out["X"], ref["X"]), rel_dev_scalars(out["max_err"], ref["max_err"])
    print(f"{what}: margin {ref['margin']:.3g} px; reference float64 against 80-bit X {ref_x:.3g}, max_err {ref_e:.3g}; "
          f"device against reference X {dev_x:.3g}, max_err {dev_e:.3g}")
    assert dev_x <= 100 * ref_x and dev_e <= 100 * ref_e
    return out, ref


@functools.lru_cache(maxsize=None)
def outlier_device():
    return device(outlier_reference()[0], **GATES)


# ------------------------------------------------------------------------------------------------------- clean parity
@pytest.mark.parametrize("iters", [0, 5])
def test_clean_tracks_are_the_plain_call_bit_for_bit(gpu_ready, iters):
    args = parity_scene()
    out = device(args, refine_iters=iters, **PLAIN_GATES)
    base = parity_device(iters)
    for k in ("status", "n_views"):
        assert np.array_equal(out[k], base[k]), k
    for k in ("X", "max_err"):
        assert np.array_equal(bits(out[k]), bits(base[k])), k
    assert (out["status"] == tr.OK).all() and np.array_equal(out["n_inliers"], out["n_views"])
    assert out["obs_inlier"].all() and len(out["obs_inlier"]) == len(args[5])       # every observation is used here
    assert np.array_equal(out["counts"], base["counts"])
    # with images 3 and 8 unregistered the flags are the used mask
    cam = np.arange(12, dtype=np.int32)
    cam[[3, 8]] = -1
    sub = (args[0], cam) + tuple(args[2:])
    out, base = device(sub, refine_iters=iters, **PLAIN_GATES), plain(sub, refine_iters=iters, **PLAIN_GATES)
    ok = base["status"] == tr.OK
    trk = np.repeat(np.arange(2000), np.diff(args[4]))
    assert ok.sum() > 1500 and (~ok).sum() > 0
    assert np.array_equal(out["status"][ok], base["status"][ok]) and np.array_equal(bits(out["X"][ok]), bits(base["X"][ok]))
    assert np.array_equal(out["obs_inlier"][ok[trk]] != 0, (cam[args[5]] >= 0)[ok[trk]])
    assert np.array_equal(out["n_inliers"][ok], base["n_views"][ok]) and np.array_equal(out["n_views"], base["n_views"])


# ------------------------------------------------------------------------------------------------------ outlier scene
def test_outlier_scene_equals_the_restatement(gpu_ready):
    args, moved, ref, base = outlier_reference()
    out, ref2 = assert_parity(args, "outlier scene", **GATES)
    assert ref2["counts"].tolist() == [365, 6, 0, 0, 0, 29] and int(ref2["reached"].sum()) == 165
    again = device(args, **GATES)                                              # a second call gives the same bits
    assert_bits(again, out)
    assert np.array_equal(again["obs_inlier"], out["obs_inlier"]) and np.array_equal(again["counts"], out["counts"])
    assert_bits(outlier_device(), out)
    # tracks the plain call accepts, and the ones that stay failing, carry the plain call's bits
    p = plain(args, **GATES)
    same = (p["status"] == tr.OK) | (out["status"] != tr.OK)
    assert same.sum() == 201 + 6 + 29
    for k in ("X", "max_err"):
        assert np.array_equal(bits(out[k][same]), bits(p[k][same])), k
    assert np.array_equal(out["status"][same], p["status"][same]) and np.array_equal(out["n_views"], p["n_views"])


# --------------------------------------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize("k", range(len(EDGE_OPTIONS)))
def test_edge_cases_equal_the_restatement(gpu_ready, k):
    args, names, moved, opts, ref, base = edge_reference(k)
    out, _ = assert_parity(args, f"edge cases {EDGE_OPTIONS[k]}", **opts)
    p = plain(args, **opts)
    st = {name: (int(p["status"][t]), int(out["status"][t]), int(out["n_inliers"][t])) for t, name in names.items()}
    print(st)
    stay = [t for t, name in names.items() if out["status"][t] != tr.OK]
    for key in ("X", "max_err"):                                               # a track that stays failing: the plain call's bits
        assert np.array_equal(bits(out[key][stay]), bits(p[key][stay])), key
    assert np.array_equal(out["status"][stay], p["status"][stay]) and not out["n_inliers"][stay].any()
    if k == 0:
        assert st["3 views, one moved"][:2] == (tr.HIGH_ERROR, tr.HIGH_ERROR)
        assert st["4 views, the first moved"] == (tr.HIGH_ERROR, tr.OK, 3) and st["4 views, the last moved"] == (tr.HIGH_ERROR, tr.OK, 3)
        assert st["4 views, moved two by two"][:2] == (tr.HIGH_ERROR, tr.HIGH_ERROR)
        assert st["6 views, two moved"] == (tr.HIGH_ERROR, tr.OK, 4)
        assert st["5 views, one NaN pixel"] == (tr.DEGENERATE, tr.OK, 4)
        assert st["all pixels NaN"][:2] == (tr.DEGENERATE, tr.DEGENERATE)
        assert st["behind"] == (tr.BEHIND, tr.OK, 3)
        assert st["11 sound views"][1:] == (tr.OK, 10) and st["12 sound views"][1:] == (tr.OK, 11)
        assert st["16 sound views"][1:] == (tr.OK, 14) and st["unregistered images inside"][1:] == (tr.OK, 4)
        # the flags of a rescued track are its clean used observations
        used = args[1][args[5]] >= 0
        for t, name in names.items():
            if out["status"][t] == tr.OK and "NaN" not in name:
                o = slice(args[4][t], args[4][t + 1])
                assert np.array_equal(out["obs_inlier"][o] != 0, used[o] & ~moved[o]), name
    if k == 1:                                                                 # min_views = 4: a consensus of 3 is not enough
        assert st["4 views, the first moved"][1] == tr.HIGH_ERROR and st["6 views, two moved"][1:] == (tr.OK, 4)


# -------------------------------------------------------------------------------------------------------------- sizes
def outlier_kinds():
    ref = outlier_reference()[2]
    rescued = np.flatnonzero(ref["reached"] & (ref["status"] == tr.OK))
    quiet = np.flatnonzero(~ref["reached"])
    return rescued, quiet


@pytest.mark.parametrize("n_tracks", [1, 63, 64, 65, 255, 256, 257])
def test_track_counts_with_a_failing_track_first_and_last(gpu_ready, n_tracks):
    """The batch holds a track that goes through the second pass first and last; every track has the bits it has in the
    batch of 400, which is held to the restatement."""
    args = outlier_reference()[0]
    rescued, _ = outlier_kinds()
    others = np.setdiff1d(np.arange(400), rescued[:2])[:max(n_tracks - 2, 0)]
    order = rescued[:1] if n_tracks == 1 else np.concatenate([rescued[:1], others, rescued[1:2]])
    assert len(order) == n_tracks
    out = device(args[:2] + take_tracks(args[2:], order), **GATES)
    base = outlier_device()
    assert_bits(out, base, rows_b=order)
    assert np.array_equal(out["obs_inlier"], base["obs_inlier"][obs_rows(args[4], order)])
    assert np.array_equal(out["counts"], np.bincount(base["status"][order], minlength=6))
    assert out["status"][0] == tr.OK and out["status"][-1] == tr.OK and out["n_inliers"][0] < out["n_views"][0]


@pytest.mark.parametrize("n_failing", [0, 1, 64, 65])
def test_work_lists_around_a_wavefront(gpu_ready, n_failing):
    args, _, ref, _ = outlier_reference()
    reached = np.flatnonzero(ref["reached"])
    quiet = np.flatnonzero(~ref["reached"])
    order = np.random.default_rng(n_failing).permutation(np.concatenate([reached[:n_failing], quiet[:100]]))
    out = device(args[:2] + take_tracks(args[2:], order), **GATES)
    base = outlier_device()
    assert_bits(out, base, rows_b=order)
    assert np.array_equal(out["obs_inlier"], base["obs_inlier"][obs_rows(args[4], order)])
    assert np.array_equal(out["counts"], np.bincount(base["status"][order], minlength=6))


def test_a_long_failing_track_beside_two_view_ones(gpu_ready):
    rng = np.random.default_rng(31)
    proj = tr.arc_cameras(16)[0]
    n = 70
    X = rng.uniform(0.2, 0.8, (n, 3))
    cams = [np.sort(rng.choice(16, 2, replace=False)) for _ in range(n)]
    cams[33] = np.arange(16)
    g = tr.make_tracks(rng, proj, X, None, noise=0.5, cams=cams, uniform=True)
    lo = g[2][33]
    rr.move(g[0], g[1], g[3], g[4], [lo + 5, lo + 12], [[50.0, 35.0], [-40.0, 60.0]])
    args = flat(proj, g)
    out, ref = assert_parity(args, "a 16-view failing track among two-view ones", **GATES)
    assert out["status"][33] == tr.OK and out["n_views"][33] == 16 and out["n_inliers"][33] == 14 and ref["reached"].sum() >= 1
    want = np.ones(16, np.uint8)
    want[[5, 12]] = 0
    assert np.array_equal(out["obs_inlier"][lo:lo + 16], want)


# ------------------------------------------------------------------------------------------------------- independence
def test_a_track_does_not_depend_on_its_batch(gpu_ready):
    args = outlier_reference()[0]
    base = outlier_device()
    for order in (np.arange(400)[::-1], np.random.default_rng(32).permutation(400), np.arange(0, 133), np.arange(133, 400)):
        out = device(args[:2] + take_tracks(args[2:], order), **GATES)
        assert_bits(out, base, rows_b=order)
        assert np.array_equal(out["obs_inlier"], base["obs_inlier"][obs_rows(args[4], order)])
    rescued, _ = outlier_kinds()
    for t in rescued[:3]:                                                      # a track alone
        out = device(args[:2] + take_tracks(args[2:], [t]), **GATES)
        assert_bits(out, base, rows_b=[t])
        assert np.array_equal(out["obs_inlier"], base["obs_inlier"][obs_rows(args[4], [t])])


# ----------------------------------------------------------------------------------------------------------- classify
device_classify = functools.partial(judge_raw, "sfm_tracks_classify")       # evaluate's keys and {n_inliers, obs_inlier}


def test_classify_at_perturbed_points_equals_the_restatement(gpu_ready):
    args, moved, ref, _ = outlier_reference()
    ok = ref["status"] == tr.OK
    Xp = np.where(ok[:, None], ref["X"], 0.5) + np.random.default_rng(33).normal(0, 0.004, (400, 3))
    has = np.ones(400, np.uint8)
    has[::5] = 0
    r = rr.classify(*args, Xp, has, **CLASSIFY_GATES)
    ld = rr.classify(*args, Xp, has, dtype=np.longdouble, **CLASSIFY_GATES)
    assert r["margin"] > 1e-6 and np.array_equal(r["obs_inlier"], ld["obs_inlier"]) and np.array_equal(r["status"], ld["status"])
    out = device_classify(args, Xp, has, **CLASSIFY_GATES)
    for k in ("status", "n_views", "n_inliers", "obs_inlier", "counts"):
        assert np.array_equal(out[k], r[k]), (k, np.flatnonzero(out[k] != r[k])[:5])
    ref_m, ref_o = rel_dev_scalars(r["max_err"], ld["max_err"]), rel_dev_scalars(r["obs_err"], ld["obs_err"])
    dev_m, dev_o = rel_dev_scalars(out["max_err"], r["max_err"]), rel_dev_scalars(out["obs_err"], r["obs_err"])
    print(f"classify at perturbed points: margin {r['margin']:.3g} px, counts {r['counts'].tolist()}; reference float64 against "
          f"80-bit max_err {ref_m:.3g}, obs_err {ref_o:.3g}; device against reference max_err {dev_m:.3g}, obs_err {dev_o:.3g}")
    assert dev_m <= 100 * ref_m and dev_o <= 100 * ref_o
    assert r["counts"][tr.OK] > 100 and r["counts"][tr.TOO_FEW_VIEWS] > 0 and 0 < r["obs_inlier"].sum() < len(moved)
    # tracks without a point: SFM_EVAL_NO_POINT, views still counted, no flag, NaN, left out of counts
    gone = has == 0
    trk = np.repeat(np.arange(400), np.diff(args[4]))
    assert (out["status"][gone] == rr.NO_POINT).all() and not out["n_inliers"][gone].any() and np.isnan(out["max_err"][gone]).all()
    assert not out["obs_inlier"][gone[trk]].any() and np.isnan(out["obs_err"][gone[trk]]).all() and out["counts"].sum() == 320
    assert np.array_equal(out["n_views"], ref["n_views"])
    none = device_classify(args, Xp, has, want_obs_err=False, **CLASSIFY_GATES)             # obs_err == NULL is accepted
    assert none["obs_err"] is None and np.array_equal(none["obs_inlier"], out["obs_inlier"])
    assert np.array_equal(bits(none["max_err"]), bits(out["max_err"]))
    # a non-finite point: too few views, no inlier
    Xi = Xp.copy()
    Xi[1] = np.inf
    bad = device_classify(args, Xi, np.ones(400, np.uint8), **CLASSIFY_GATES)
    assert bad["status"][1] == tr.TOO_FEW_VIEWS and bad["n_inliers"][1] == 0 and np.isnan(bad["max_err"][1])


def test_classify_repeats_the_robust_call_bit_for_bit(gpu_ready):
    for args, opts in ((outlier_reference()[0], GATES), (edge_reference(0)[0], edge_reference(0)[3])):
        out = device(args, **opts)
        ok = out["status"] == tr.OK
        cg = {k: v for k, v in opts.items() if k != "refine_iters"}
        c = device_classify(args, np.where(ok[:, None], out["X"], 0.0), ok, **cg)
        assert (c["status"][ok] == tr.OK).all() and (c["status"][~ok] == rr.NO_POINT).all()
        assert np.array_equal(c["obs_inlier"], out["obs_inlier"]) and np.array_equal(c["n_inliers"], out["n_inliers"])
        assert np.array_equal(bits(c["max_err"][ok]), bits(out["max_err"][ok])) and np.array_equal(c["n_views"], out["n_views"])
        assert c["counts"].tolist() == [int(ok.sum()), 0, 0, 0, 0, 0]


# -------------------------------------------------------------------------------------------------------------- C ABI
def test_bad_options_and_small_workspace_are_rejected(gpu_ready):
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p
    args = outlier_reference()[0]
    for bad in (dict(min_views=1), dict(refine_iters=-1), dict(max_error=-1.0), dict(min_angle_deg=-1.0), dict(max_error=np.nan)):
        with pytest.raises(ValueError):
            device(args, **bad)
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    n, n_obs = 400, len(args[5])
    need, need_c = C.c_int64(), C.c_int64()
    assert h.lib.sfm_triangulate_tracks_robust_workspace_bytes(12, n, C.byref(need)) == 0 and need.value >= 12 * 24 + 4 * n + 4
    assert h.lib.sfm_triangulate_tracks_robust_workspace_bytes(12, n, None) == -1
    assert h.lib.sfm_triangulate_tracks_robust_workspace_bytes(-1, n, C.byref(need_c)) == -1
    assert h.lib.sfm_triangulate_tracks_workspace_bytes(12, C.byref(need_c)) == 0
    t = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in zip("pcktoiq", args)}
    X = torch.full((n, 3), 7.0, dtype=torch.float64, device=dev)
    st, nv, ni = (torch.full((n,), 7, dtype=torch.int32, device=dev) for _ in range(3))
    me, counts = torch.full((n,), 7.0, dtype=torch.float64, device=dev), torch.full((6,), 7, dtype=torch.int64, device=dev)
    fl = torch.full((n_obs,), 7, dtype=torch.uint8, device=dev)
    has = torch.ones(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)

    def robust(min_views=2, iters=5, max_error=4.0, ws_bytes=need.value, n_tracks=n, X_=X, fl_=fl):
        return h.lib.sfm_triangulate_tracks_robust(h._h, _p(t["p"]), 12, _p(t["c"]), 14, _p(t["k"]), _p(t["t"]), len(args[3]),
                                                   _p(t["o"]), n_tracks, _p(t["i"]), _p(t["q"]), n_obs, min_views, iters,
                                                   C.c_double(max_error), C.c_double(1.0), _p(X_), _p(st), _p(nv), _p(ni), _p(me),
                                                   _p(fl_), _p(counts), _p(ws), ws_bytes)

    def classify(min_views=2, max_error=4.0, ws_bytes=need_c.value, n_tracks=n, has_=has, fl_=fl):
        return h.lib.sfm_tracks_classify(h._h, _p(t["p"]), 12, _p(t["c"]), 14, _p(t["k"]), _p(t["t"]), len(args[3]), _p(t["o"]),
                                         n_tracks, _p(t["i"]), _p(t["q"]), n_obs, _p(X), _p(has_), min_views, C.c_double(max_error),
                                         C.c_double(1.0), _p(st), _p(nv), _p(ni), _p(me), _p(fl_), None, _p(counts), _p(ws), ws_bytes)

    def untouched():
        return (counts.tolist() == [7] * 6 and bool((st == 7).all()) and bool((ni == 7).all()) and bool((fl == 7).all())
                and bool((X == 7.0).all()))
    assert robust(min_views=1) == -1 and b"min_views" in h.lib.sfm_last_error(h._h)
    assert robust(iters=-1) == -1 and robust(max_error=-1.0) == -1 and classify(min_views=1) == -1 and classify(max_error=-1.0) == -1
    assert untouched()                                                         # nothing ran
    assert robust(ws_bytes=need.value - 1) == -3 and classify(ws_bytes=need_c.value - 1) == -3
    assert robust(X_=None) == -1 and robust(fl_=None) == -1 and classify(has_=None) == -1 and classify(fl_=None) == -1
    torch.cuda.synchronize()
    assert bool((st == 7).all()) and bool((fl == 7).all()) and bool((X == 7.0).all())    # only counts were zeroed
    counts.fill_(7)
    assert robust(n_tracks=0) == 0 and counts.tolist() == [0] * 6
    counts.fill_(7)
    assert classify(n_tracks=0) == 0 and counts.tolist() == [0] * 6 and bool((st == 7).all())
    assert robust() == 0 and counts.tolist() == [365, 6, 0, 0, 0, 29]
    X.copy_(torch.where(torch.isnan(X), torch.zeros_like(X), X))
    has.copy_((st == 0).to(torch.uint8))
    assert classify() == 0 and counts.tolist() == [365, 0, 0, 0, 0, 0]


# --------------------------------------------------------------------------------------------------- the public calls
def test_public_calls(gpu_ready):
    from sfm_amd import Tracks, classify_tracks, triangulate_tracks
    from sfm_amd.ba import GpuBA, solve_ba
    from sfm_amd.rotation import log_so3
    args, moved, ref, _ = outlier_reference()
    proj, cam, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = args
    T = Tracks(kp_ptr, track_ptr, obs_image, obs_kp)
    kps = [kp_xy[kp_ptr[i]:kp_ptr[i + 1]] for i in range(14)]
    reg = np.arange(12)
    tri = triangulate_tracks(T, kps, proj.reshape(-1, 3, 4), registered=reg, robust=True, **GATES)
    base = outlier_device()
    assert np.array_equal(bits(tri.X), bits(base["X"])) and np.array_equal(tri.status, base["status"])
    assert tri.obs_inlier.dtype == bool and np.array_equal(tri.obs_inlier, base["obs_inlier"] != 0)
    assert np.array_equal(tri.n_inliers, base["n_inliers"]) and tri.valid.sum() == 365
    off = triangulate_tracks(T, kps, proj.reshape(-1, 3, 4), registered=reg, **GATES)
    assert off.obs_inlier is None and off.valid.sum() == 201 and np.array_equal(off.n_inliers, np.where(off.valid, off.n_views, 0))
    # ba_inputs holds no rejected observation, and the bundle adjustment converges on it
    pts, cam_idx, pt_idx, uv = tri.ba_inputs()
    assert len(pts) == 365 and len(uv) == tri.n_inliers[tri.valid].sum() == tri.obs_inlier.sum() and (np.diff(pt_idx) >= 0).all()
    node_uv = kp_xy[kp_ptr[obs_image] + obs_kp]
    sel = np.flatnonzero(tri.obs_inlier)
    assert np.array_equal(uv, node_uv[sel]) and np.array_equal(cam_idx, cam[obs_image[sel]])
    trk = np.repeat(np.arange(400), np.diff(track_ptr))
    rescued = ref["reached"] & (ref["status"] == tr.OK)                        # their moved observations are the rejected ones
    rejected = moved & (cam[obs_image] >= 0) & rescued[trk]
    assert rejected.sum() > 150 and not tri.obs_inlier[rejected].any() and tri.obs_inlier[rescued[trk] & ~moved & (cam[obs_image] >= 0)].all()
    _, Rs, ts, _ = tr.arc_cameras(14)
    cams0 = np.stack([np.concatenate([log_so3(R), t]) for R, t in zip(Rs[:12], ts[:12])])
    K0 = (1228.0, 1228.0, 512.0, 384.0)
    be0 = GpuBA(cams0, pts, cam_idx, pt_idx, uv, K0)
    cost0 = be0.cost()
    be0.close()
    res, cams, pts2, be = solve_ba(cams0, pts, cam_idx, pt_idx, uv, K0)
    cost1 = be.cost()
    be.close()
    # converged, and a minimiser does not end above its start (the ground-truth cameras and the triangulated points).  No
    # bound on single errors: a two-view track whose observation moved along the epipolar line passes every gate.
    print(f"bundle adjustment over the inlier observations: {len(uv)} observations, cost {cost0:.6g} -> {cost1:.6g}, nfev {res.nfev}")
    assert res.success and np.isfinite(cost1) and cost1 <= cost0
    # classify_tracks: shapes and dtypes
    ok = tri.valid
    c = classify_tracks(T, kps, proj.reshape(-1, 3, 4), np.where(ok[:, None], tri.X, 0.0), ok, registered=reg, **CLASSIFY_GATES)
    assert sorted(c) == ["counts", "max_err", "n_inliers", "n_views", "obs_err", "obs_inlier", "status"]
    assert c["status"].shape == (400,) and c["status"].dtype == np.int32 and c["n_views"].dtype == np.int32
    assert c["n_inliers"].shape == (400,) and c["n_inliers"].dtype == np.int32 and c["max_err"].shape == (400,)
    assert c["obs_inlier"].shape == (len(obs_image),) and c["obs_inlier"].dtype == bool and c["obs_err"].shape == (len(obs_image),)
    assert c["counts"].shape == (6,) and c["counts"].dtype == np.int64 and c["counts"].tolist() == [365, 0, 0, 0, 0, 0]
    assert np.array_equal(c["obs_inlier"], tri.obs_inlier) and np.array_equal(bits(c["max_err"][ok]), bits(tri.max_err[ok]))
    with pytest.raises(ValueError):
        classify_tracks(T, kps, proj.reshape(-1, 3, 4), tri.X, ok, registered=reg, min_views=1)
