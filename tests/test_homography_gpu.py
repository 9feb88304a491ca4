"""GPU tests of the batched homography RANSAC (sfm_amd.homography -> sfm_hom_draw_samples / sfm_hom_ransac in
libsfm_amd.so) against the NumPy reference that replays the device's samples (tests/homography_reference.py), of the
guard it gives the incremental loop's initial pair (`max_homography_ratio`) and of `process_pairs(..., homography=True)`.
512 hypotheses and at most a dozen segments per call."""
import ctypes as C
import functools

import numpy as np
import pytest

import homography_reference as hr
import triangulate_reference as tr
from test_homography_reference import left_out_share, shipped, shipped_replay, synthetic_replay

pytestmark = pytest.mark.gpu

THR = 3.0


@functools.lru_cache(maxsize=None)
def run_synth(refine):
    from sfm_amd import homography
    p1, p2 = hr.synth_batch()
    return homography.estimate_homography_batched(p1, p2, THR, n_hypotheses=512, seed=1, refine=refine, return_debug=True)


@functools.lru_cache(maxsize=None)
def run_shipped12(refine):
    from sfm_amd import homography
    sh = shipped()
    return homography.estimate_homography_batched([s[1] for s in sh], [s[2] for s in sh], THR, n_hypotheses=512, seed=0,
                                                  refine=refine, return_debug=True)


def check_replay(name, d, res, st):
    """hyp_count equals the reference's on at least 99 % of the stable hypotheses, of which at most 1 % of the non-voided
    ones are left out; a voided sample counts nothing; the winner's count is at least the reference's best stable count."""
    eq = d["hyp_count"] == res["hyp_count"]
    best = int(res["hyp_count"][st].max()) if st.any() else 0
    print(f"{name}: hyp_count equal on {eq[st].mean():.4%} of the stable hypotheses, {eq.mean():.4%} of all; left out "
          f"{left_out_share(res, st):.2%}; voided {res['voided'].mean():.2%}; winner {d['n_inliers']} / best stable "
          f"reference count {best}")
    assert left_out_share(res, st) <= 0.01, name
    assert st.any() and eq[st].mean() >= 0.99, name
    assert (d["hyp_count"][res["voided"]] == 0).all(), name
    assert d["n_inliers"] >= best, name


def check_consistent(p1, p2, res, dbg):
    """The mask is the NumPy rule applied to the returned H (except within 1e-9 relative of the gate, where the two sides
    of the comparison round), n_inliers is its sum, H[2,2] == 1 (no scene here has an H whose last element fails), H is
    finite."""
    for s, ((H, mask), d) in enumerate(zip(res, dbg)):
        if d["status"] != 0:
            assert H is None and mask is None and d["n_inliers"] == 0, s
            continue
        assert mask.shape == (len(p1[s]), 1) and mask.dtype == np.uint8 and H.shape == (3, 3) and np.isfinite(H).all()
        assert d["n_inliers"] == int(mask.sum()), s
        e, w2 = hr.residuals(H, p1[s], p2[s])
        with np.errstate(invalid="ignore"):
            near = np.abs(e - THR * THR * w2) <= 1e-9 * THR * THR * w2
        want = hr.inliers(H, p1[s], p2[s], THR)
        assert np.array_equal(mask.ravel().astype(bool)[~near], want[~near]), s
        assert abs(d["n_inliers"] - int(want.sum())) <= int(near.sum()), s
        assert H[2, 2] == 1.0, (s, H[2, 2])


# ------------------------------------------------------------------------------------------- replay parity
def test_replay_parity_on_synthetic_pairs(gpu_ready):
    """All of hr.CASES in one call, seed 1, no refit: the samples are the generator's, and per case check_replay.
    Measured: hyp_count equal on 100 % of all hypotheses in every case, nothing left out."""
    res, dbg = run_synth(False)
    for s, ((kind, M, share), (smp, ref, st)) in enumerate(zip(hr.CASES, synthetic_replay())):
        d = dbg[s]
        assert np.array_equal(d["samples"], smp), s
        if M < 4:
            assert d["status"] == 1 and res[s] == (None, None) and (d["hyp_count"] == 0).all()
            continue
        assert d["status"] == 0, s
        check_replay(f"segment {s} ({kind}, M {M}, outliers {share})", d, ref, st)


def test_replay_parity_on_shipped_pairs(gpu_ready):
    """Pairs 0, 13, ..., 143 in one call, seed 0, no refit.  Measured: hyp_count equal on 100 % of all hypotheses in every
    pair, nothing left out."""
    res, dbg = run_shipped12(False)
    for s, ((i, _, _, _), (smp, ref, st)) in enumerate(zip(shipped(), shipped_replay())):
        d = dbg[s]
        assert d["status"] == 0 and np.array_equal(d["samples"], smp), i
        check_replay(f"pair {i}", d, ref, st)


# ---------------------------------------------------------------------------------------- self-consistency
def test_self_consistency_synthetic(gpu_ready):
    p1, p2 = hr.synth_batch()
    plain, refit = run_synth(False), run_synth(True)
    for res, dbg in (plain, refit):
        check_consistent(p1, p2, res, dbg)
        assert [d["status"] for d in dbg] == [1] + [0] * (len(hr.CASES) - 1)
    assert not any(d["refined"] for d in plain[1])
    for s, (a, b) in enumerate(zip(plain[1], refit[1])):
        assert b["n_inliers"] >= a["n_inliers"] if b["refined"] else b["n_inliers"] == a["n_inliers"], s
        assert np.array_equal(a["hyp_count"], b["hyp_count"]), s
    print("refit kept on", sum(d["refined"] for d in refit[1]), "of", len(hr.CASES), "cases; inliers without / with:",
          [(a["n_inliers"], b["n_inliers"]) for a, b in zip(plain[1], refit[1])])


def test_self_consistency_shipped_pairs(gpu_ready):
    sh = shipped()
    p1, p2 = [s[1] for s in sh], [s[2] for s in sh]
    plain, refit = run_shipped12(False), run_shipped12(True)
    for res, dbg in (plain, refit):
        check_consistent(p1, p2, res, dbg)
        assert all(d["status"] == 0 for d in dbg)
    for s, (a, b) in enumerate(zip(plain[1], refit[1])):
        assert b["n_inliers"] >= a["n_inliers"] if b["refined"] else b["n_inliers"] == a["n_inliers"], s
    print("refit kept on", sum(d["refined"] for d in refit[1]), "of 12 pairs; inliers without / with:",
          [(a["n_inliers"], b["n_inliers"]) for a, b in zip(plain[1], refit[1])])


def test_against_the_true_homography(gpu_ready):
    """On the rotation and planar cases with at least 40 matches the device's refitted winner keeps at least 0.95 x the
    inliers of the true homography, the bound tests/test_homography_reference.py sets for the reference."""
    p1, p2 = hr.synth_batch()
    res, dbg = run_synth(True)
    for s, (kind, M, share) in enumerate(hr.CASES):
        Ht = hr.scene(kind, M, share)[2]
        if Ht is None or M < 40:
            continue
        truth = int(hr.inliers(Ht, p1[s], p2[s], THR).sum())
        print(f"{kind} M {M} share {share}: device {dbg[s]['n_inliers']} / true H {truth}")
        assert dbg[s]["n_inliers"] >= 0.95 * truth, s


# ----------------------------------------------------------------------------- determinism and independence
def test_two_calls_give_identical_bytes(gpu_ready):
    from sfm_amd import homography
    p1, p2 = hr.synth_batch()
    a, da = homography.estimate_homography_batched(p1, p2, THR, n_hypotheses=512, seed=1, return_debug=True)
    b, db = run_synth(True)
    for (Ha, ma), (Hb, mb), x, y in zip(a[1:], b[1:], da[1:], db[1:]):
        assert Ha.tobytes() == Hb.tobytes() and ma.tobytes() == mb.tobytes()
        assert x["hyp_count"].tobytes() == y["hyp_count"].tobytes() and x["refined"] == y["refined"]


def test_a_pair_does_not_depend_on_its_position_in_the_batch(gpu_ready):
    """A pair alone and the same pair at positions 0, 5 and 11 of a 12-pair batch, with its samples passed in explicitly
    (the generator keys on the segment index): identical H, mask and hyp_count."""
    from sfm_amd import homography
    sh = shipped()
    p1, p2 = [s[1] for s in sh], [s[2] for s in sh]
    n = 256
    a, b = hr.scene("planar", 513, 0.3)[:2]
    smp = hr.draw_samples(7, 0, len(a), n)
    (H0, m0), d0 = homography.find_homography(a, b, THR, n_hypotheses=n, samples=smp, return_debug=True)
    assert H0 is not None
    base = [hr.draw_samples(7, s, len(p1[s]), n) for s in range(len(p1))]
    for pos in (0, 5, 11):
        q1, q2, sm = list(p1), list(p2), list(base)
        q1[pos], q2[pos], sm[pos] = a, b, smp
        res, dbg = homography.estimate_homography_batched(q1, q2, THR, n_hypotheses=n, samples=sm, return_debug=True)
        H, m = res[pos]
        assert H.tobytes() == H0.tobytes() and m.tobytes() == m0.tobytes(), pos
        assert dbg[pos]["hyp_count"].tobytes() == d0["hyp_count"].tobytes(), pos


# --------------------------------------------------------------------------------------------------- edges
def test_edges_hypothesis_counts(gpu_ready):
    """1, 255, 256, 257 and 512 hypotheses: partial and whole workgroups.  Hypothesis h draws the same sample whatever the
    count, so the counts of a shorter run are a prefix of a longer one's."""
    from sfm_amd import homography
    p1, p2 = hr.synth_batch()
    sel = slice(5, 9)
    full = None
    for n in (512, 257, 256, 255, 1):
        res, dbg = homography.estimate_homography_batched(p1[sel], p2[sel], THR, n_hypotheses=n, seed=3, refine=False,
                                                          return_debug=True)
        check_consistent(p1[sel], p2[sel], res, dbg)
        for s, d in enumerate(dbg):
            assert d["hyp_count"].shape == (n,) and d["samples"].shape == (n, 4)
            if full is not None:
                assert np.array_equal(d["hyp_count"], full[s]["hyp_count"][:n]), (n, s)
        if full is None:
            full = dbg


def test_edges_empty_and_short_segments(gpu_ready):
    from sfm_amd import homography
    assert homography.estimate_homography_batched([], []) == []
    a, b = hr.scene("planar", 300, 0.3)[:2]
    p1, p2 = [a, a[:0], a[:3], a, a[:1]], [b, b[:0], b[:3], b, b[:1]]
    for refine in (False, True):
        res, dbg = homography.estimate_homography_batched(p1, p2, THR, n_hypotheses=64, refine=refine, return_debug=True)
        assert [d["status"] for d in dbg] == [0, 1, 1, 0, 1]
        assert res[1] == (None, None) and res[2] == (None, None) and res[4] == (None, None)
        assert all((dbg[s]["hyp_count"] == 0).all() and (dbg[s]["samples"] == -1).all() for s in (1, 2, 4))
        check_consistent(p1, p2, res, dbg)
    assert homography.estimate_homography_batched([a[:2]], [b[:2]]) == [(None, None)]
    assert homography.find_homography(a[:0], b[:0]) == (None, None)


def raw_call(p1, p2, n_hyp, samples=None, refine=0):
    """sfm_hom_ransac on one batch through the C ABI: (H [n_seg,9], mask [n], meta [3,n_seg]) as the library left them in
    buffers filled with 7."""
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    lengths = [len(a) for a in p1]
    n, n_seg = sum(lengths), len(p1)
    seg = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=dev)
    a = torch.from_numpy(np.ascontiguousarray(np.concatenate(p1), dtype=np.float32)).to(dev)
    b = torch.from_numpy(np.ascontiguousarray(np.concatenate(p2), dtype=np.float32)).to(dev)
    smp = torch.empty((n_seg, n_hyp, 4), dtype=torch.int32, device=dev)
    if samples is None:
        h.call("sfm_hom_draw_samples", _p(seg), n_seg, n_hyp, C.c_uint64(0), _p(smp))
    else:
        smp = torch.from_numpy(np.ascontiguousarray(samples, dtype=np.int32)).to(dev)
    need = C.c_int64()
    assert h.lib.sfm_hom_workspace_bytes(n, n_seg, n_hyp, C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    H = torch.full((n_seg, 9), 7.0, dtype=torch.float64, device=dev)
    mask = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    meta = torch.full((3, n_seg), 7, dtype=torch.int32, device=dev)
    h.call("sfm_hom_ransac", _p(seg), n_seg, _p(a), _p(b), n, _p(smp), n_hyp, C.c_double(THR), refine, _p(H), _p(mask),
           _p(meta[0]), _p(meta[1]), None, _p(meta[2]), _p(ws), need.value)
    return H.cpu().numpy(), mask.cpu().numpy(), meta.cpu().numpy()


def test_collinear_matches_give_no_model(gpu_ready):
    """A segment whose matches all lie on one line in both images: every sample is voided, status 2, H = 0, a zero mask,
    count 0 - between two segments that have a model, whose results it does not touch."""
    rng = np.random.default_rng(12)
    tt = rng.uniform(0, 1, 30).astype(np.float32)
    line1 = np.stack([100 + 500 * tt, 50 + 300 * tt], 1).astype(np.float32)
    line2 = np.stack([80 + 450 * tt, 90 + 310 * tt], 1).astype(np.float32)
    a, b = hr.scene("planar", 40, 0.0)[:2]
    for refine in (0, 1):
        H, mask, meta = raw_call([a, line1, a, a[:3]], [b, line2, b, b[:3]], 256, refine=refine)
        assert meta[1].tolist() == [0, 2, 0, 1] and meta[0, 1] == 0 and meta[0, 3] == 0 and meta[2, 1] == 0
        assert (H[1] == 0).all() and (H[3] == 0).all() and (mask[40:70] == 0).all() and (mask[110:] == 0).all()
        assert meta[0, 0] == mask[:40].sum() > 0 and meta[0, 2] == mask[70:110].sum() > 0 and set(np.unique(mask)) <= {0, 1}
    from sfm_amd import homography
    res, dbg = homography.estimate_homography_batched([line1], [line2], THR, n_hypotheses=256, return_debug=True)
    assert res == [(None, None)] and dbg[0]["status"] == 2 and (dbg[0]["hyp_count"] == 0).all()


def test_repeated_and_non_finite_points(gpu_ready):
    """One match repeated 40 times voids every sample: status 2.  NaN / inf coordinates are never inliers and void the
    samples that hold them; a repeated match voids the samples that hold it twice."""
    from sfm_amd import homography
    same = np.tile(np.float32([[321.5, 123.25]]), (40, 1))
    a1, a2 = (x.copy() for x in hr.scene("rotation", 40, 0.0)[:2])
    a1[33, 0] = np.nan
    a2[17, 1] = np.inf
    a1[5] = [np.inf, -np.inf]
    a1[21], a2[21] = a1[20], a2[20]
    p1, p2 = [same, a1], [same + np.float32(2.0), a2]
    for refine in (False, True):
        res, dbg = homography.estimate_homography_batched(p1, p2, THR, n_hypotheses=512, refine=refine, return_debug=True)
        assert dbg[0]["status"] == 2 and res[0] == (None, None) and (dbg[0]["hyp_count"] == 0).all()
        assert dbg[1]["status"] == 0
        H, mask = res[1]
        assert np.isfinite(H).all() and mask[33, 0] == 0 and mask[17, 0] == 0 and mask[5, 0] == 0
        check_consistent(p1, p2, res, dbg)
    res, dbg = homography.estimate_homography_batched(p1, p2, THR, n_hypotheses=512, refine=False, return_debug=True)
    smp = dbg[1]["samples"]
    holds_bad = np.isin(smp, [33, 17, 5]).any(1) | (np.isin(smp, [20]).any(1) & np.isin(smp, [21]).any(1))
    assert holds_bad.any() and (dbg[1]["hyp_count"][holds_bad] == 0).all()
    with np.errstate(invalid="ignore", over="ignore"):
        ref = hr.ransac(a1, a2, smp, THR)
    assert ref["voided"][holds_bad].all()
    assert np.mean(dbg[1]["hyp_count"] == ref["hyp_count"]) >= 0.99
    assert (dbg[1]["hyp_count"][ref["voided"]] == 0).all()


def test_bad_samples_and_bad_arguments_are_rejected(gpu_ready):
    import torch
    from sfm_amd import _lib, homography
    from sfm_amd.driver import _p
    a40, b40 = hr.scene("planar", 40, 0.0)[:2]
    smp = hr.draw_samples(0, 0, 40, 8)
    at = np.arange(32).reshape(8, 4) == 7
    for bad in (np.where(at, 40, smp), np.where(at, -1, smp)):
        with pytest.raises(ValueError):
            homography.find_homography(a40, b40, n_hypotheses=8, samples=bad)
    with pytest.raises(ValueError):
        homography.find_homography(a40, b40, n_hypotheses=8, samples=np.tile(smp[:, :1], (1, 4)))
    with pytest.raises(ValueError):
        homography.find_homography(a40, b40, n_hypotheses=8, samples=smp[:, :3])
    with pytest.raises(ValueError):
        homography.find_homography(a40, b40, n_hypotheses=0)
    with pytest.raises(ValueError):
        homography.find_homography(a40, b40, threshold=-1.0)
    with pytest.raises(ValueError):
        homography.find_homography(a40, b40[:39])
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    n, n_hyp = 40, 8
    seg = torch.tensor([0, n], dtype=torch.int64, device=dev)
    a, b = (torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in (a40, b40))
    d_smp = torch.from_numpy(smp).to(dev)
    H = torch.full((1, 9), 7.0, dtype=torch.float64, device=dev)
    mask = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    meta = torch.full((3, 1), 7, dtype=torch.int32, device=dev)
    need = C.c_int64()
    assert h.lib.sfm_hom_workspace_bytes(n, 1, n_hyp, C.byref(need)) == 0 and need.value > 0
    assert h.lib.sfm_hom_workspace_bytes(n, 1, 0, C.byref(need)) == -1
    assert h.lib.sfm_hom_workspace_bytes(-1, 1, n_hyp, C.byref(need)) == -1
    assert h.lib.sfm_hom_workspace_bytes(n, 1, n_hyp, None) == -1
    assert h.lib.sfm_hom_workspace_bytes(n, 1, n_hyp, C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)

    def call(n_seg=1, n_hyp=n_hyp, thr=3.0, pts=a, out=H, n_pts=n, ws_bytes=need.value, handle=h._h, samples=d_smp):
        return h.lib.sfm_hom_ransac(handle, _p(seg), n_seg, _p(pts), _p(b), n_pts, _p(samples), n_hyp, C.c_double(thr), 0,
                                    _p(out), _p(mask), _p(meta[0]), _p(meta[1]), None, _p(meta[2]), _p(ws), ws_bytes)
    assert call(handle=None) == -1
    assert call(n_seg=-1) == -1 and call(n_hyp=0) == -1 and call(n_pts=-1) == -1
    assert call(thr=-1.0) == -1 and call(thr=float("nan")) == -1 and call(thr=float("inf")) == -1
    assert b"bad argument" in h.lib.sfm_last_error(h._h)
    assert call(pts=None) == -1 and call(out=None) == -1 and call(samples=None) == -1
    assert b"null pointer" in h.lib.sfm_last_error(h._h)
    assert call(ws_bytes=need.value - 1) == -3
    torch.cuda.synchronize()
    assert (H == 7.0).all() and (mask == 7).all() and (meta == 7).all()     # nothing ran
    assert h.lib.sfm_hom_draw_samples(h._h, _p(seg), 1, 0, C.c_uint64(0), _p(d_smp)) == -1
    assert h.lib.sfm_hom_draw_samples(h._h, _p(seg), 1, n_hyp, C.c_uint64(0), None) == -1
    assert h.lib.sfm_hom_draw_samples(None, _p(seg), 1, n_hyp, C.c_uint64(0), _p(d_smp)) == -1
    assert call() == 0
    torch.cuda.synchronize()
    ref = hr.ransac(a40, b40, smp, THR)
    assert meta[1, 0].item() == 0 and float(H[0, 8]) == 1.0 and int(mask.sum()) == meta[0, 0].item() == ref["n_inliers"]
    # a sample index outside its segment, passed below the wrapper's check: that hypothesis counts nothing, the rest run
    bad = smp.copy()
    bad[3, 2], bad[5, 0] = 40, -1
    counts = torch.full((1, n_hyp), 7, dtype=torch.int32, device=dev)
    d_bad = torch.from_numpy(bad).to(dev)
    assert h.lib.sfm_hom_ransac(h._h, _p(seg), 1, _p(a), _p(b), n, _p(d_bad), n_hyp, C.c_double(3.0), 0, _p(H), _p(mask),
                                _p(meta[0]), _p(meta[1]), _p(counts), _p(meta[2]), _p(ws), need.value) == 0
    got = counts.cpu().numpy()[0]
    ref = ref["hyp_count"]
    assert got[3] == 0 and got[5] == 0 and np.array_equal(np.delete(got, [3, 5]), np.delete(ref, [3, 5]))


def test_exported_names_and_the_mixin(gpu_ready):
    import sfm_amd
    from sfm_amd import HomographyMixin, estimate_homography_batched, find_homography  # noqa: F401
    assert "hom_hyp" in sfm_amd._lib.PROF_SLOTS and len(sfm_amd._lib.PROF_SLOTS) == 21
    a, b, Ht = hr.scene("planar", 300, 0.3)

    class Finder(HomographyMixin):
        hom_hypotheses = 512
    H, mask = Finder().find_homography_mat(a, b)
    assert H[2, 2] == 1.0 and mask.shape == (300, 1) and int(mask.sum()) >= 0.95 * hr.inliers(Ht, a, b, THR).sum()
    h = sfm_amd._lib.get_handle(0)
    h.set_profiling(True)
    try:
        h.profile()
        find_homography(a, b, n_hypotheses=512)
        ms, launches = h.profile()["hom_hyp"]
    finally:
        h.set_profiling(False)
    print(f"hom_hyp slot: {ms:.3f} ms over {launches} launch")
    assert launches == 1 and ms > 0


# ----------------------------------------------------------------------------------------------- the guard
class GuardScene:
    pass


@functools.lru_cache(maxsize=None)
def guard_scene(planar=False, seed=33, n_pts=120):
    """In the way of test_incremental_gpu.loop_scene: 8 cameras of tr.arc_cameras(8), K = K_SFM, pixel noise 0.5 px, every
    image numbering its keypoints in an order of its own, every pair matched on the points both see.  Camera 1 stands at
    camera 0's centre, turned 0.08 rad about its vertical axis; cameras 0 and 1 see every point and the others 3 to 5
    of the six remaining cameras' worth, so (0, 1) is the pair with the most common tracks.  planar: every point lies
    in one plane instead."""
    from sfm_amd import build_tracks
    rng = np.random.default_rng(seed)
    s = GuardScene()
    proj, Rs, ts, centres = tr.arc_cameras(8)
    c, sn = np.cos(0.08), np.sin(0.08)
    Rs, ts, centres = Rs.copy(), ts.copy(), centres.copy()
    if not planar:
        Rs[1] = np.array([[c, 0, sn], [0, 1, 0], [-sn, 0, c]]) @ Rs[0]
        centres[1] = centres[0]
        ts[1] = -Rs[1] @ centres[1]
    s.Rs, s.ts, s.centres = Rs, ts, centres
    s.proj = np.stack([tr.K_SFM @ np.hstack([R, t[:, None]]) for R, t in zip(Rs, ts)])
    s.X = rng.uniform(0, 1, (n_pts, 3))
    if planar:
        s.X[:, 2] = 0.5 + 0.2 * (s.X[:, 0] - 0.5) - 0.1 * (s.X[:, 1] - 0.5)
    sees = np.zeros((8, n_pts), bool)
    sees[:2] = True
    for p in range(n_pts):
        sees[2 + rng.choice(6, int(rng.integers(3, 6)), replace=False), p] = True
    px = tr.project_points(s.proj, s.X) + rng.normal(0, 0.5, (8, n_pts, 2))
    slot = [rng.permutation(n_pts) for _ in range(8)]
    s.keypoints = []
    for i in range(8):
        kp = rng.uniform(0, 1000, (n_pts, 2))
        kp[slot[i][sees[i]]] = px[i, sees[i]]
        s.keypoints.append(kp)
    pairs, matches = [], []
    for i in range(8):
        for j in range(i + 1, 8):
            both = np.flatnonzero(sees[i] & sees[j])
            pairs.append((i, j)); matches.append((slot[i][both], slot[j][both]))
    s.tracks = build_tracks([n_pts] * 8, pairs, matches)
    assert len(s.tracks) == n_pts and s.tracks.n_obs == sees.sum()
    return s


def test_guard_leaves_out_the_pair_that_shares_a_centre(gpu_ready):
    """Cameras 0 and 1 share a centre and see the most common tracks.  With max_homography_ratio=0.8 the pair is logged
    degenerate and is not the initial pair, all 8 images register and every returned point passes the gates.  What the
    unguarded loop chooses is printed, not asserted."""
    from sfm_amd import reconstruct_tracks
    from sfm_amd._lib import SfmError
    import test_incremental_gpu as ti
    s = guard_scene()
    rec = reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, max_homography_ratio=0.8)
    rows = {r["pair"]: r for r in rec.log[0]["candidates"]}
    print("guarded: initial pair", rec.log[0]["initial_pair"], "order", rec.order, "row of (0, 1):", rows[(0, 1)])
    print("ratios n_H / n_model:", {p: round(r["n_homography"] / max(r["n_model"], 1), 3) for p, r in rows.items()})
    assert all(set(r) == {"pair", "common", "n_good", "n_model", "n_homography", "degenerate"} for r in rows.values())
    assert rows[(0, 1)]["common"] == 120 == max(r["common"] for r in rows.values())
    assert rows[(0, 1)]["degenerate"] is True and rows[(0, 1)]["n_homography"] > 0.8 * rows[(0, 1)]["n_model"]
    assert [p for p, r in rows.items() if r["degenerate"]] == [(0, 1)]
    assert all(r["degenerate"] == (r["n_homography"] > 0.8 * r["n_model"]) for r in rows.values())
    assert rec.log[0]["initial_pair"] != (0, 1) and rows[rec.log[0]["initial_pair"]]["degenerate"] is False
    assert sorted(rec.order) == list(range(8)) and rec.unregistered == []
    ti.assert_invariant(s, rec)
    # a given pair is not left out by the guard: (0, 1) goes on to the pose stage, which finds no point in front of two
    # cameras that share a centre - the loop's own error, not the guard's
    with pytest.raises(SfmError, match="no initial pair with at least"):
        reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, initial_pair=(0, 1), max_homography_ratio=0.8, min_initial_points=1)
    # and it is recorded: the pair the guarded loop chose, given explicitly
    given = rec.log[0]["initial_pair"]
    fixed = reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, initial_pair=given, max_homography_ratio=0.8, min_visible=10 ** 9)
    assert fixed.log[0]["initial_pair"] == given and len(fixed.log[0]["candidates"]) == 1
    assert fixed.log[0]["candidates"][0]["degenerate"] is False and fixed.log[0]["candidates"][0]["n_homography"] > 0
    try:
        plain = reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM)
        print("unguarded: initial pair", plain.log[0]["initial_pair"], "n_good", plain.log[0]["n_good"], "registered",
              len(plain.order), "of 8, points", int(plain.has_point.sum()))
    except SfmError as e:
        print("unguarded: SfmError:", e)


def test_guard_on_an_all_planar_scene_and_its_option(gpu_ready):
    from sfm_amd import reconstruct_tracks
    from sfm_amd._lib import SfmError
    import test_incremental_gpu as ti
    s = guard_scene(planar=True)
    with pytest.raises(SfmError, match="degenerate"):
        reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, max_homography_ratio=0.8)
    # a given pair of the planar scene is degenerate, recorded as such and not left out: either it becomes the initial pair
    # or the pose stage turns it down with the loop's own error
    try:
        fixed = reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, initial_pair=(0, 7), max_homography_ratio=0.8,
                                   min_visible=10 ** 9, min_initial_points=1)
        row = fixed.log[0]["candidates"][0]
        print("planar scene, given pair (0, 7):", row)
        assert fixed.log[0]["initial_pair"] == (0, 7) and row["degenerate"] is True
    except SfmError as e:
        print("planar scene, given pair (0, 7):", e)
        assert "no initial pair with at least" in str(e)
    for bad in (0, -0.5, float("nan"), float("inf"), "0.8", True):
        with pytest.raises(ValueError):
            reconstruct_tracks(s.tracks, s.keypoints, tr.K_SFM, max_homography_ratio=bad)
    # the option absent: the rows carry exactly today's keys
    rec = ti.loop_result()
    assert all(set(r) == {"pair", "common", "n_good"} for r in rec.log[0]["candidates"])
    assert set(rec.log[0]) == {"step", "initial_pair", "initial_model", "n_good", "candidates", "pair_refinement", "points_added"}


# ------------------------------------------------------------------------------------------- process_pairs
def test_process_pairs_with_homographies(gpu_ready):
    """Descriptors whose true correspondences obey a plane-induced homography for pair (0, 1) and a general geometry for
    pair (0, 2): homography=True adds 'H' and 'n_homography' and nothing else; without it the dictionaries are today's."""
    from sfm_amd.matcher import ImageMatcher
    rng = np.random.default_rng(21)
    N = 300
    base = rng.integers(0, 256, (N, 128)).astype(np.float32)
    a, b, Ht = hr.scene("planar", N, 0.0)
    g1, g2, _ = hr.scene("general", N, 0.0)
    kps, descs = [], []
    for x in (a, b, g2):
        perm = rng.permutation(N)
        kps.append(np.asarray(x, np.float32)[perm])
        descs.append(np.clip(base[perm] + rng.integers(-3, 4, (N, 128)), 0, 255).astype(np.float32))
    kps.append(kps[0][:3]); descs.append(descs[0][:3])                       # an image with 3 keypoints: under min_matches
    pairs = [(0, 1), (3, 1), (1, 2)]
    plain = ImageMatcher().process_pairs(kps, descs, pairs)
    out = ImageMatcher().process_pairs(kps, descs, pairs, homography=True)
    assert plain[1] is None and out[1] is None
    for k in (0, 2):
        assert set(plain[k]) == {"matches", "pts1", "pts2", "F", "inlier_mask", "symmetric_errors", "metrics", "quality_ok"}
        assert set(out[k]) == set(plain[k]) | {"H", "n_homography"}
        for key in ("pts1", "pts2", "F", "inlier_mask", "symmetric_errors"):
            assert np.array_equal(np.asarray(out[k][key]), np.asarray(plain[k][key])), (k, key)
        assert out[k]["metrics"] == plain[k]["metrics"] and out[k]["quality_ok"] == plain[k]["quality_ok"]
        assert out[k]["H"].shape == (3, 3) and out[k]["H"][2, 2] == 1.0
        assert out[k]["n_homography"] == int(hr.inliers(out[k]["H"], out[k]["pts1"], out[k]["pts2"], 3.0).sum())
    truth = int(hr.inliers(Ht, out[0]["pts1"], out[0]["pts2"], 3.0).sum())
    print("planar pair: n_homography", out[0]["n_homography"], "true H", truth, "of", len(out[0]["pts1"]), "matches; "
          "other pair: n_homography", out[2]["n_homography"], "of", len(out[2]["pts1"]))
    assert len(out[0]["pts1"]) >= 250 and out[0]["n_homography"] >= 0.95 * truth
    with pytest.raises(TypeError):
        ImageMatcher().process_pairs(kps, descs, pairs, homography=True, gate=3.0)
