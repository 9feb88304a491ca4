"""Guided matching without a device: the two restatements of tests/guided_reference.py against each other, the rule header
(sfm_amd/csrc/guided_rule.h) built for the host against the NumPy gate bit for bit, the plan header under the sanitizers,
the gate against the rule the project already ships, what guided matching buys on Scene A, and the argument checks."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import fundamental_reference as fr
import guided_reference as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "guided_check.cpp")
RECORD = np.dtype([("F", "<f8", 9), ("thr", "<f8"), ("p", "<f4", 4)])      # struct Record of guided_check.cpp


@pytest.fixture(scope="module")
def scene_a():
    return gr.scene_a()


def build_check(tmp_path, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"), CHECK_SRC, "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return str(exe)


def run_gate(exe, tmp_path, rec):
    fin, fout = tmp_path / "gate.in", tmp_path / "gate.out"
    with open(fin, "wb") as f:
        f.write(np.int64(len(rec)).tobytes())
        f.write(rec.tobytes())
    run = subprocess.run([exe, "gate", str(fin), str(fout)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    return np.fromfile(fout, dtype=np.uint8).astype(bool)


def numpy_gate(rec):
    """The NumPy gate of every record (one (F, p, q, thr) each)."""
    out = np.zeros(len(rec), bool)
    for k, r in enumerate(rec):
        out[k] = gr.gate(r["F"], r["p"][None, :2], r["p"][None, 2:], r["thr"])[0, 0]
    return out


def numpy_gate_rows(rec):
    """The same, vectorised over records with a row-wise restatement of gate_terms (kept next to it on purpose)."""
    f = rec["F"].astype(np.float64)
    x1, y1, x2, y2 = (rec["p"][:, k].astype(np.float64) for k in range(4))
    with np.errstate(all="ignore"):
        a = (f[:, 0] * x1 + f[:, 1] * y1) + f[:, 2]
        b = (f[:, 3] * x1 + f[:, 4] * y1) + f[:, 5]
        c = (f[:, 6] * x1 + f[:, 7] * y1) + f[:, 8]
        ta = (f[:, 0] * x2 + f[:, 3] * y2) + f[:, 6]
        tb = (f[:, 1] * x2 + f[:, 4] * y2) + f[:, 7]
        s = (x2 * a + y2 * b) + c
        den = np.fmin(a * a + b * b, ta * ta + tb * tb)
        return (den > 0) & (s * s <= (rec["thr"] * rec["thr"]) * den), s * s, den


def random_records(rng, n):
    """Random (F, p, q, thr): F of random two-view geometries, q near p's epipolar line so that both outcomes occur."""
    rec = np.zeros(n, RECORD)
    k = 0
    while k < n:
        m = min(n - k, 2000)
        yaw = rng.uniform(-0.4, 0.4)
        R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        F = fr.true_fundamental(R, rng.normal(size=3))
        F = F / F[2, 2] if rng.random() < 0.5 and F[2, 2] != 0 else F * 10.0 ** rng.integers(-6, 7)
        p = (rng.uniform(0, 1, (m, 2)) * [1024, 768]).astype(np.float32)
        line = np.c_[p.astype(np.float64), np.ones(m)] @ F.T                      # F x1
        x2 = rng.uniform(0, 1024, m)
        with np.errstate(all="ignore"):
            y2 = -(line[:, 0] * x2 + line[:, 2]) / line[:, 1] + rng.normal(size=m) * rng.choice([0.5, 3.0, 30.0], m)
        y2 = np.where(np.isfinite(y2), y2, rng.uniform(0, 768, m))
        rec["F"][k:k + m] = F.ravel()
        rec["p"][k:k + m, :2] = p
        rec["p"][k:k + m, 2] = x2
        rec["p"][k:k + m, 3] = y2
        rec["thr"][k:k + m] = rng.choice([0.5, 1.0, 3.0, 3.0, 10.0, 60.0], m)
        k += m
    return rec


def threshold_records(rng):
    """Triples that sit at the threshold.  (1) a sideways translation, F = g [[0,0,0],[0,0,-1],[0,1,0]]: the rule reduces to
    g^2 (y1 - y2)^2 <= thr^2 g^2 without a rounding error for small integers and powers of two, so y2 = y1 + thr is exact
    equality; np.nextafter on the float32 coordinate y2 gives the two neighbours.  (2) random triples with thr placed at the
    flip point sqrt(s^2 / den) and up to two ulps either side."""
    recs = []
    for g in (1.0, 0.5, 2.0 ** -20, 2.0 ** 12):
        F = g * np.array([0, 0, 0, 0, 0, -1.0, 0, 1.0, 0])
        for thr in (3.0, 0.5, 2.0, 64.0):
            for y1 in (10.0, 383.5, 700.25):
                for sign in (1.0, -1.0):
                    y2 = np.float32(y1 + sign * thr)
                    for yy in (y2, np.nextafter(y2, np.float32(-np.inf)), np.nextafter(y2, np.float32(np.inf))):
                        r = np.zeros(1, RECORD)
                        r["F"], r["thr"], r["p"] = F, thr, [rng.uniform(0, 1024), y1, rng.uniform(0, 1024), yy]
                        recs.append(r)
    exact = np.concatenate(recs)
    ok, lhs, den = numpy_gate_rows(exact)
    eq = lhs == (exact["thr"] * exact["thr"]) * den
    assert eq[0::3].all() and ok[0::3].all(), "the constructed triples are exact equalities, and equality passes"
    assert (ok[1::3] != ok[2::3]).all(), "one ulp of the coordinate either side: one passes, one fails"
    base = random_records(rng, 3000)
    _, lhs, den = numpy_gate_rows(base)
    good = np.isfinite(lhs) & (den > 0) & (lhs > 0)
    base, lhs, den = base[good], lhs[good], den[good]
    t0 = np.sqrt(lhs / den)
    flips = []
    for step in range(-2, 3):
        r = base.copy()
        t = t0.copy()
        for _ in range(abs(step)):
            t = np.nextafter(t, np.inf if step > 0 else -np.inf)
        r["thr"] = t
        flips.append(r)
    flips = np.concatenate(flips)
    ok = numpy_gate_rows(flips)[0]
    assert 0.2 < ok.mean() < 0.8, "the flip points have both outcomes"
    return np.concatenate([exact, flips])


# ------------------------------------------------------------------------------------------- the two restatements
def random_pair(rng, n1, n2, n_bytes=4):
    """A small pair with many candidates per query: few descriptor bits, so ties in the distance are common."""
    yaw = rng.uniform(-0.3, 0.3)
    R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    F = fr.true_fundamental(R, np.array([-1.5, 0.1, 0.3]) + rng.normal(size=3) * 0.1)
    F = F / F[2, 2]
    k1 = (rng.uniform(0, 1, (n1, 2)) * [1024, 768]).astype(np.float32)
    k2 = (rng.uniform(0, 1, (n2, 2)) * [1024, 768]).astype(np.float32)
    d1 = rng.integers(0, 256, (n1, n_bytes), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n2, n_bytes), dtype=np.uint8)
    return k1, k2, d1, d2, F


def assert_same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def test_the_two_formulations_agree_on_random_input():
    rng = np.random.default_rng(11)
    seen = 0
    for n1, n2 in ((40, 70), (1, 30), (30, 1), (25, 2), (0, 5), (5, 0), (64, 65)):
        k1, k2, d1, d2, F = random_pair(rng, n1, n2)
        for metric in ("hamming", "l2"):
            for cross in (False, True):
                for maxd in (None, 12.0 if metric == "hamming" else 250.0):
                    for ratio in (0.75, 1.0, float("inf")):
                        kw = dict(gate_px=40.0, ratio=ratio, max_distance=maxd, cross_check=cross, metric=metric)
                        a = gr.guided_match(k1, k2, d1, d2, F, **kw)
                        assert_same(a, gr.guided_match_loops(k1, k2, d1, d2, F, **kw))
                        seen += len(a[0])
    assert seen > 500


def test_the_two_formulations_agree_on_degenerate_input():
    rng = np.random.default_rng(12)
    k1, k2, d1, d2, F = random_pair(rng, 30, 40)
    # F = 0, an F with a NaN: no candidate anywhere (an infinite F is not asked about: the formulations only have to agree)
    for bad in (np.zeros((3, 3)), np.where(np.eye(3) > 0, np.nan, F), np.where(np.eye(3) > 0, np.inf, F)):
        a = gr.guided_match(k1, k2, d1, d2, bad, gate_px=60.0)
        assert np.isinf(bad).any() or (len(a[0]) == 0 and a[3].sum() == 0)
        assert_same(a, gr.guided_match_loops(k1, k2, d1, d2, bad, gate_px=60.0))
    # NaN / inf keypoints on either side: no candidate for / at them, the other queries as without them
    clean = gr.guided_match(k1, k2, d1, d2, F, gate_px=60.0, ratio=1.0)
    for side in (0, 1):
        ka, kb = k1.copy(), k2.copy()
        (ka if side == 0 else kb)[[3, 7, 11]] = [[np.nan, 5], [np.inf, 100], [200, -np.inf]]
        a = gr.guided_match(ka, kb, d1, d2, F, gate_px=60.0, ratio=1.0)
        assert_same(a, gr.guided_match_loops(ka, kb, d1, d2, F, gate_px=60.0, ratio=1.0))
        ok = gr.gate(F, ka, kb, 60.0)
        assert not (ok[[3, 7, 11]] if side == 0 else ok[:, [3, 7, 11]]).any()
        if side == 0:
            keep = ~np.isin(clean[0], [3, 7, 11])
            assert_same([x[keep] for x in clean[:3]], a[:3])
    # identical descriptors inside one gate: the lowest index wins, the next one is second, and d1 == ratio * d2 is rejected
    d2[:] = d2[0]
    a = gr.guided_match(k1, k2, d1, d2, F, gate_px=60.0, ratio=1.0)
    assert len(a[0]) == int((a[3] == 1).sum())
    ok = gr.gate(F, k1, k2, 60.0)
    b = gr.guided_match(k1, k2, d1, d2, F, gate_px=60.0, ratio=1.5)
    assert (b[1] == np.array([np.flatnonzero(ok[q])[0] for q in b[0]])).all() and len(b[0]) == int((b[3] >= 1).sum())
    assert_same(b, gr.guided_match_loops(k1, k2, d1, d2, F, gate_px=60.0, ratio=1.5))


# ------------------------------------------------------------------------------------------- the rule header on the host
def test_rule_header_equals_the_numpy_gate_bit_for_bit(tmp_path):
    """guided_rule.h built by g++ -O2 -ffp-contract=off into a stand-alone program: 1e5 random (F, p, q) triples, and triples
    constructed to sit at the threshold (equality, and one ulp either side)."""
    exe = build_check(tmp_path, ["-O2"], "guided_check")
    rng = np.random.default_rng(21)
    rec = random_records(rng, 100000)
    want = numpy_gate_rows(rec)[0]
    assert 0.05 < want.mean() < 0.95
    # the row-wise restatement used for speed is the reference's gate
    some = rng.choice(len(rec), 300, replace=False)
    assert (numpy_gate(rec[some]) == want[some]).all()
    got = run_gate(exe, tmp_path, rec)
    assert (got == want).all(), f"{(got != want).sum()} of {len(rec)} random triples differ"
    edge = threshold_records(rng)
    want = numpy_gate_rows(edge)[0]
    assert (numpy_gate(edge[:200]) == want[:200]).all()
    got = run_gate(exe, tmp_path, edge)
    assert (got == want).all(), f"{(got != want).sum()} of {len(edge)} threshold triples differ"
    # NaN anywhere fails, F = 0 fails
    bad = rec[:64].copy()
    bad["thr"] = 1e9
    assert numpy_gate_rows(bad)[0].all()
    for k in range(9):
        bad["F"][k, k] = np.nan
    for k in range(4):
        bad["p"][16 + k, k] = np.nan
    bad["F"][32:48] = 0.0
    want = numpy_gate_rows(bad)[0]
    assert not want[:9].any() and not want[16:20].any() and not want[32:48].any() and want[48:].all()
    assert (run_gate(exe, tmp_path, bad) == want).all()


def test_rule_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """The same program with guided_plan.h, built with -fsanitize=address,undefined and run stand-alone: degenerate segment
    tables (no pair, empty sides, one keypoint, no output row), random ones, and the gate over threshold triples."""
    exe = build_check(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                 "-fno-omit-frame-pointer"], "guided_check_san")
    for seed in (1, 2):
        run = subprocess.run([exe, "plan", str(seed)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])
    rng = np.random.default_rng(22)
    rec = np.concatenate([random_records(rng, 2000), threshold_records(rng)])
    assert (run_gate(exe, tmp_path, rec) == numpy_gate_rows(rec)[0]).all()
    assert len(run_gate(exe, tmp_path, rec[:0])) == 0


# ------------------------------------------------------------------------------------------- against the shipped rule
def test_gate_agrees_with_the_shipped_rule_outside_the_band(scene_a):
    """fundamental_reference.cv_err2 <= thr^2 is the rule the RANSAC stage counts inliers by; the gate is the same rule
    without its divisions.  They may differ only within 1e-9 relative of thr^2 (the band test_fundamental_gpu uses), and
    the band is a condition: at most 1 % of the combinations may fall in it."""
    k, F = scene_a["kps"], scene_a["F"]
    for thr in (3.0, 1.0, 10.0):
        ours = gr.gate(F, k[0], k[1], thr)
        theirs, band = gr.cv_gate(F, k[0], k[1], thr)
        assert ours.shape == (360, 360)
        assert band.mean() <= 0.01
        assert (ours == theirs)[~band].all()
    assert gr.cv_gate(F, k[0], k[1], 3.0)[1].sum() == 0 and gr.near_threshold(F, k[0], k[1], 3.0).sum() == 0


def test_guided_matching_keeps_more_correct_matches_on_scene_a(scene_a):
    """The value of the feature: under the true F guided matching keeps strictly more correct matches than the blind
    matcher, and at least 1.5 x as many (measured: 296 of 302 against 150 of 150)."""
    k, d, F = scene_a["kps"], scene_a["descs"], scene_a["F"]
    truth = scene_a["truth"](0, 1)
    bq, bt, _ = gr.blind_match(d[0], d[1], 0.75)
    gq, gt, _, nc = gr.guided_match(k[0], k[1], d[0], d[1], F, 3.0, 0.75)
    blind, guided = gr.count_correct(bq, bt, truth), gr.count_correct(gq, gt, truth)
    assert (len(bq), blind, len(gq), guided) == (150, 150, 302, 296)
    assert guided > blind and guided >= 1.5 * blind
    assert abs(nc.mean() - 4.9) < 0.1 and nc.max() == 11
    ok = gr.gate(F, k[0], k[1], 3.0)
    gated_blind = {(q, t) for q, t in zip(bq.tolist(), bt.tolist()) if ok[q, t]}
    assert gated_blind <= set(zip(gq.tolist(), gt.tolist()))


# ------------------------------------------------------------------------------------------- the Python side, no device
def test_argument_checks_without_gpu(scene_a):
    import sfm_amd
    from sfm_amd import guided
    from sfm_amd.matcher import ImageMatcher
    assert sfm_amd.guided_match_pairs is guided.guided_match_pairs
    k, d, F = scene_a["kps"], scene_a["descs"], scene_a["F"]
    good = dict(keypoints=k, descs=d, pairs=[(0, 1)], Fs=[F])
    guided.check_arguments(**good)
    f32 = [x.astype(np.float32) for x in d]
    assert guided.check_arguments(k, f32, [(0, 1)], [F])[6] is True            # integer-valued floats are converted
    bad_calls = [
        dict(good, descs=[x[:, :24] for x in d]),                               # unsupported Hamming size
        dict(good, descs=[x[:, :16] for x in d], metric="l2"),                  # unsupported L2 size
        dict(good, descs=[np.tile(x, (1, 8)) for x in d], metric="l2"),         # dim 256
        dict(good, metric="cosine"),
        dict(good, descs=f32, metric="hamming"),
        dict(good, descs=[f32[0] + 0.5, f32[1]]),                               # a float set that is not integer-valued
        dict(good, descs=[f32[0], f32[1] - 1.0]),                               # ... or leaves [0, 255]
        dict(good, descs=[d[0].astype(np.int16), d[1].astype(np.int16)]),
        dict(good, descs=[d[0], d[1][:, :16]]),                                 # sets of two sizes
        dict(good, descs=[d[0], f32[1]]),                                       # ... of two types
        dict(good, descs=[d[0][:-1], d[1]]),                                    # keypoints / descriptors differ in length
        dict(good, keypoints=k[:1]),
        dict(good, Fs=[]),
        dict(good, Fs=[F[:2]]),
        dict(good, pairs=[(0, 2)]),
        dict(good, pairs=[(-1, 1)]),
        dict(good, gate=-1.0),
        dict(good, gate=float("nan")),
        dict(good, ratio=float("nan")),
        dict(good, max_distance=-2.0),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            guided.guided_match_pairs(**kw)
    with pytest.raises(ValueError, match="integer"):
        guided.guided_match_pairs(**dict(good, descs=[f32[0] + 0.25, f32[1]]))
    # nothing to do needs no device either
    empty = guided.guided_match_pairs(k, d, [(0, 1), (1, 0)], [None, None])
    assert len(empty) == 2 and all(len(a) == 0 for e in empty for a in e)
    out, dbg = guided.guided_match_pairs([None, None], [None, None], [(0, 1)], [F], return_debug=True)
    assert len(out[0][0]) == 0 and dbg[0].shape == (0,)
    assert guided.guided_match_pairs(k, d, [], []) == []
    m = ImageMatcher()
    with pytest.raises(ValueError):
        m.guided_pairs(k, d, [(0, 1)], [])
    assert m.guided_pairs(k, d, [(0, 1), (1, 0)], [None, None]) == [None, None]
    with pytest.raises(TypeError):
        m.process_pairs(k, d, [], gate=2.0)


def test_c_entry_points_reject_bad_calls_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    n_out, need = ctypes.c_int64(-1), ctypes.c_int64(-1)
    arr = lambda *v: np.array(v, dtype=np.int64)
    hp = lambda a: ctypes.c_void_p(a.ctypes.data)
    qb, qe, tb, te = arr(0, 5), arr(5, 5), arr(5, 0), arr(9, 5)
    assert lib.sfm_guided_workspace_bytes(_lib.METRIC_HAMMING, 2, hp(qb), hp(qe), hp(tb), hp(te), ctypes.byref(n_out), ctypes.byref(need)) == 0
    assert n_out.value == 5 and need.value >= 5 * 17 + 9 * 4
    assert lib.sfm_guided_workspace_bytes(_lib.METRIC_L2_U8, 0, None, None, None, None, ctypes.byref(n_out), ctypes.byref(need)) == 0
    assert n_out.value == 0 and need.value > 0
    assert lib.sfm_guided_workspace_bytes(_lib.METRIC_L2_F32, 2, hp(qb), hp(qe), hp(tb), hp(te), ctypes.byref(n_out), ctypes.byref(need)) != 0
    assert lib.sfm_guided_workspace_bytes(_lib.METRIC_HAMMING, 2, hp(qe), hp(qb), hp(tb), hp(te), ctypes.byref(n_out), ctypes.byref(need)) != 0
    assert lib.sfm_guided_workspace_bytes(_lib.METRIC_HAMMING, 2, None, hp(qe), hp(tb), hp(te), ctypes.byref(n_out), ctypes.byref(need)) != 0
    assert lib.sfm_guided_workspace_bytes(_lib.METRIC_HAMMING, -1, hp(qb), hp(qe), hp(tb), hp(te), ctypes.byref(n_out), ctypes.byref(need)) != 0
    assert lib.sfm_guided_workspace_bytes(_lib.METRIC_HAMMING, 2, hp(qb), hp(qe), hp(tb), hp(te), None, ctypes.byref(need)) != 0
    assert lib.sfm_guided_match(None, _lib.METRIC_HAMMING, None, 0, 32, None, 0, None, None, None, None, None, 3.0, 0.75, -1.0, 0,
                                None, None, None, None, None, None, 0) != 0
