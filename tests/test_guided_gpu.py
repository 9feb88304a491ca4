"""Guided matching on the device (sfm_guided_match through sfm_amd.guided) against tests/guided_reference.py, byte for byte:
the rule has no FMA contraction and distances are exact integers before one sqrtf, so no tolerance is needed anywhere."""
import numpy as np
import pytest

import fundamental_reference as fr
import guided_reference as gr

pytestmark = pytest.mark.gpu

# the tile constants of the kernel (sfm_amd/csrc/guided_plan.h)
GUIDED_QW = 8          # queries a wavefront walks
GUIDED_QT = 32         # queries per workgroup
GUIDED_CHUNK = 512     # points of the other image per LDS stage
GUIDED_DRAIN = 64      # queued candidates per drain

SIDEWAYS = np.array([[0, 0, 0], [0, 0, -1.0], [0, 1.0, 0]])     # F of a sideways translation: the rule is |y1 - y2| <= gate, exactly


def test_constants_are_the_headers():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sfm_amd", "csrc", "guided_plan.h")).read()
    val = {m.group(1): m.group(2) for m in re.finditer(r"constexpr int (GUIDED_\w+) = ([^;]+);", src)}
    assert int(val["GUIDED_QW"]) == GUIDED_QW and int(val["GUIDED_CHUNK"]) == GUIDED_CHUNK and int(val["GUIDED_DRAIN"]) == GUIDED_DRAIN
    assert int(val["GUIDED_WAVES"]) * GUIDED_QW == GUIDED_QT


def to_l2(descs, dim, seed=3):
    """uint8 [n, dim] descriptors for the L2 metric out of bit strings: 200 per set bit plus a little noise."""
    rng = np.random.default_rng(seed)
    out = []
    for d in descs:
        bits = np.unpackbits(d, axis=1)
        bits = np.tile(bits, (1, -(-dim // bits.shape[1])))[:, :dim]
        out.append((bits.astype(np.int64) * 200 + rng.integers(0, 40, bits.shape)).astype(np.uint8))
    return out


def check(keypoints, descs, pairs, Fs, metric, **kw):
    """One device call against the reference: queryIdx, trainIdx, distance, seg_ptr and n_candidates, byte for byte.  Returns
    the reference's per-pair results and candidate counts."""
    from sfm_amd import guided
    gate = kw.pop("gate", 3.0)
    csr = guided.guided_match_csr(keypoints, descs, pairs, Fs, gate=gate, metric=metric, **kw)
    live = [s for s, F in enumerate(Fs) if F is not None]
    assert csr["live"] == live
    none = [np.zeros((0, 2), np.float32) if k is None else k for k in keypoints]
    want, want_nc, _ = gr.guided_batch(none, [np.zeros((0, 1), np.uint8) if d is None else d for d in descs], pairs, Fs,
                                       gate_px=gate, metric=metric, **kw)
    ptr = np.cumsum([0] + [len(want[s][0]) for s in live]).astype(np.int64)
    assert csr["seg_ptr"].dtype == np.int64 and csr["seg_ptr"].tobytes() == ptr.tobytes()
    for name, k in (("queryIdx", 0), ("trainIdx", 1), ("distance", 2)):
        ref = np.concatenate([want[s][k] for s in live]) if live else want[0][k][:0]
        assert csr[name].dtype == ref.dtype and csr[name].tobytes() == ref.tobytes(), name
    nc = np.concatenate([want_nc[s] for s in live])
    assert csr["n_candidates"].dtype == np.int32 and csr["n_candidates"].tobytes() == nc.tobytes()
    # the per-pair form cuts the same arrays up
    out, dbg = guided.guided_match_pairs(keypoints, descs, pairs, Fs, gate=gate, metric=metric, return_debug=True, **kw)
    for s in range(len(pairs)):
        for a, b in zip(out[s], want[s][:3]):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        assert dbg[s].tobytes() == (want_nc[s] if Fs[s] is not None else np.zeros(len(none[pairs[s][0]]), np.int32)).tobytes()
    return want, want_nc


# ------------------------------------------------------------------------------------------- Scene A and three images
@pytest.fixture(scope="module")
def scenes():
    a = gr.scene_a()
    yaw = -0.2
    R3 = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    poses = [a["poses"][0], a["poses"][1], (R3, np.array([1.2, -0.2, 0.4]))]
    b = gr.scene(seed=7, poses=poses, sizes=(200, 150, 97))              # 260 / 210 / 157 keypoints
    kps, descs = a["kps"] + b["kps"], a["descs"] + b["descs"]
    pairs = [(0, 1), (2, 3), (3, 4), (4, 2), (3, 2)]
    Fs = [a["F"]] + [gr.relative_F(poses[i - 2], poses[j - 2]) for i, j in pairs[1:]]
    return {"a": a, "kps": kps, "descs": {"hamming": descs, "l2": to_l2(descs, 128)}, "pairs": pairs, "Fs": Fs}


@pytest.mark.parametrize("cut", [False, True], ids=["no_max", "max_distance"])
@pytest.mark.parametrize("cross", [False, True], ids=["forward", "cross_check"])
@pytest.mark.parametrize("metric", ["hamming", "l2"])
def test_scene_a_and_three_images_in_one_batch(gpu_ready, scenes, metric, cross, cut):
    kps, descs, pairs, Fs = scenes["kps"], scenes["descs"][metric], scenes["pairs"], scenes["Fs"]
    maxd = None
    if cut:                                                            # a value that cuts about half of Scene A's matches
        _, _, d, _ = gr.guided_match(kps[0], kps[1], descs[0], descs[1], Fs[0], metric=metric)
        vals = np.unique(d)
        maxd = float(vals[np.argmin([abs((d <= v).mean() - 0.5) for v in vals])])
    want, nc = check(kps, descs, pairs, Fs, metric, ratio=0.75, cross_check=cross, max_distance=maxd)
    if metric == "hamming" and not cross and not cut:
        assert len(want[0][0]) == 302 and abs(nc[0].mean() - 4.9) < 0.1 and nc[0].max() == 11
    if cut:
        full = gr.guided_match(kps[0], kps[1], descs[0], descs[1], Fs[0], metric=metric, cross_check=cross)[0]
        assert 0.3 * len(full) < len(want[0][0]) < 0.7 * len(full)
    assert all(len(w[0]) > 5 for w in want)                  # every pair of the batch has something to compare


# ------------------------------------------------------------------------------------------- kernel edges
EDGE_SIZES = [0, 1, 2, GUIDED_QW - 1, GUIDED_QW, GUIDED_QW + 1, GUIDED_QT - 1, GUIDED_QT, GUIDED_QT + 1, 63, 64, 65,
              GUIDED_CHUNK - 1, GUIDED_CHUNK, GUIDED_CHUNK + 1, 2 * GUIDED_CHUNK + 1]


@pytest.fixture(scope="module")
def edge_images():
    """One image per size of EDGE_SIZES: keypoints uniform in 1024 x 768, 64-byte bit strings that differ in few bits (ties)."""
    rng = np.random.default_rng(31)
    base = rng.integers(0, 256, (8, 64), dtype=np.uint8)
    kps = [(rng.uniform(0, 1, (n, 2)) * [1024, 768]).astype(np.float32) for n in EDGE_SIZES]
    descs = [gr.flip_bits(rng, base[rng.integers(0, 8, n)], 3) for n in EDGE_SIZES]
    F = gr.scene_a()["F"]
    return kps, descs, F


@pytest.mark.parametrize("metric,dim", [("hamming", 16), ("hamming", 64), ("l2", 32), ("l2", 64)])
def test_sizes_around_every_tile_constant(gpu_ready, edge_images, metric, dim):
    """Train and query sizes 0, 1, 2, 63, 64, 65 and one below / at / one above GUIDED_QW (queries per wavefront), GUIDED_QT
    (per workgroup) and GUIDED_CHUNK (points per LDS stage), and two stages plus one; a 60 px gate, so a query has up to ~150
    candidates and the queue drains zero, one and several times.  cross_check runs the same sizes with the roles swapped."""
    kps, descs, F = edge_images
    descs = [d[:, :dim] for d in descs] if metric == "hamming" else to_l2([d[:, :8] for d in descs], dim)
    ref_q, ref_t = EDGE_SIZES.index(GUIDED_QT + 1), EDGE_SIZES.index(65)
    pairs = [(k, ref_t) for k in range(len(EDGE_SIZES))] + [(ref_q, k) for k in range(len(EDGE_SIZES))]
    pairs += [(EDGE_SIZES.index(GUIDED_CHUNK + 1), EDGE_SIZES.index(2 * GUIDED_CHUNK + 1)), (0, 0), (1, 1)]
    pairs = [p for p in pairs if p[0] != p[1] or EDGE_SIZES[p[0]] < 2]
    descs = [d if len(d) else None for d in descs]                      # an image without keypoints, as a detector returns it
    kps = [k if len(k) else None for k in kps]
    for cross in (False, True):
        want, nc = check(kps, descs, pairs, [F] * len(pairs), metric, gate=60.0, ratio=0.9, cross_check=cross)
    assert max(int(c.max()) for c in nc if len(c)) > 2 * GUIDED_DRAIN
    assert sum(len(w[0]) for w in want) > 50


def test_one_pair_of_65537_queries(gpu_ready):
    """65,537 queries against 8 train keypoints: 257 blocks of output rows, so the one workgroup that scans the block counts
    gives two counts to a thread and leaves the last threads without any; about a third of the rows are kept."""
    rng = np.random.default_rng(5)
    nq = 256 * 256 + 1
    kps = [(rng.uniform(0, 1, (n, 2)) * [1024, 768]).astype(np.float32) for n in (nq, 8)]
    descs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in (nq, 8)]
    want, nc = check(kps, descs, [(0, 1)], [gr.scene_a()["F"]], "hamming", gate=60.0, ratio=0.9, cross_check=False)
    assert 0.2 * nq < len(want[0][0]) < 0.5 * nq


def test_candidate_counts_drain_the_queue_zero_one_and_several_times(gpu_ready):
    """Queries with exactly 0, 1, 2, 63, 64, 65, 127, 128, 129 and 200 candidates: under a sideways translation the rule is
    |y1 - y2| <= gate, so the train keypoints of one image row are one query's candidates; they are scattered over two LDS
    stages, so the queue is carried from one stage to the next."""
    rng = np.random.default_rng(41)
    counts = [0, 1, 2, GUIDED_DRAIN - 1, GUIDED_DRAIN, GUIDED_DRAIN + 1, 2 * GUIDED_DRAIN - 1, 2 * GUIDED_DRAIN, 2 * GUIDED_DRAIN + 1, 200]
    rows = 50.0 * np.arange(1, len(counts) + 1)
    k1 = np.c_[rng.uniform(0, 1024, len(counts)), rows].astype(np.float32)
    ty = np.concatenate([np.full(c, y) for c, y in zip(counts, rows)] + [np.full(40, 700.0)])
    ty = ty + rng.uniform(-2.5, 2.5, len(ty))
    perm = rng.permutation(len(ty))
    k2 = np.c_[rng.uniform(0, 1024, len(ty)), ty[perm]].astype(np.float32)
    assert len(k2) > GUIDED_CHUNK
    d1 = rng.integers(0, 256, (len(k1), 32), dtype=np.uint8)
    d2 = gr.flip_bits(rng, d1[rng.integers(0, len(k1), len(k2))], 20)
    for metric, a, b in (("hamming", d1, d2), ("l2", *to_l2([d1, d2], 128))):
        for ratio in (0.75, float("inf")):
            want, nc = check([k1, k2], [a, b], [(0, 1), (1, 0)], [SIDEWAYS, SIDEWAYS.T], metric, gate=3.0, ratio=ratio, cross_check=False)
            assert nc[0].tolist() == counts
        check([k1, k2], [a, b], [(0, 1), (1, 0)], [SIDEWAYS, SIDEWAYS.T], metric, gate=3.0, ratio=float("inf"), cross_check=True)


# ------------------------------------------------------------------------------------------- ties
def test_ties_and_the_strict_comparisons(gpu_ready):
    from sfm_amd.guided import guided_match_pairs
    base = np.zeros(32, np.uint8)

    def desc(bits):
        d = base.copy()
        d[:bits // 8] = 0xFF
        d[bits // 8] = (0xFF << (8 - bits % 8)) & 0xFF
        return d
    # query row y = 100: candidates 1, 3, 4 share one descriptor at distance 12 (index 0 sits on another row);
    # query row y = 200: candidates at distance 12 and 16; query row y = 300: one candidate at distance 12;
    # query row y = 400: no candidate
    k1 = np.array([[10, 100], [20, 200], [30, 300], [40, 400]], np.float32)
    d1 = np.stack([base] * 4)
    k2 = np.array([[5, 600], [50, 100], [60, 200], [70, 101], [80, 99], [90, 201], [95, 300]], np.float32)
    d2 = np.stack([desc(0), desc(12), desc(12), desc(12), desc(12), desc(16), desc(12)])
    run = lambda **kw: guided_match_pairs([k1, k2], [d1, d2], [(0, 1)], [SIDEWAYS], gate=3.0, metric="hamming", return_debug=True, **kw)
    (m,), (nc,) = run(ratio=float("inf"))
    assert nc.tolist() == [3, 2, 1, 0]
    assert m[0].tolist() == [0, 1, 2] and m[1].tolist() == [1, 2, 6] and m[2].tolist() == [12.0, 12.0, 12.0]      # the lowest index wins
    (m,), _ = run(ratio=1.0)                                # ... and the next duplicate is second: d1 == d2 fails d1 < 1.0 * d2
    assert m[0].tolist() == [1, 2]
    (m,), _ = run(ratio=0.75)                               # 12 == 0.75 * 16 is rejected (strict); one candidate needs no ratio test
    assert m[0].tolist() == [2]
    (m,), _ = run(ratio=0.7500001)
    assert m[0].tolist() == [1, 2]
    (m,), _ = run(ratio=float("inf"), max_distance=12.0)    # d1 == max_distance is kept
    assert m[0].tolist() == [0, 1, 2]
    (m,), _ = run(ratio=float("inf"), max_distance=11.999)
    assert m[0].tolist() == []
    (m,), _ = run(ratio=float("inf"), cross_check=True)     # train 1's best query is 0, train 2's is 1, train 6's is 2
    assert m[0].tolist() == [0, 1, 2]
    for kw in (dict(ratio=1.0), dict(ratio=0.75), dict(ratio=float("inf"), max_distance=12.0), dict(ratio=float("inf"), cross_check=True)):
        check([k1, k2], [d1, d2], [(0, 1), (1, 0)], [SIDEWAYS, SIDEWAYS.T], "hamming", gate=3.0, **kw)
    # the same ties in L2: d^2 = 12 * 255^2 three times
    check([k1, k2], [np.tile(d1, (1, 4)), np.tile(d2, (1, 4))], [(0, 1)], [SIDEWAYS], "l2", gate=3.0, ratio=1.0)


# ------------------------------------------------------------------------------------------- degenerate input
def test_degenerate_models_and_keypoints_leave_no_trace(gpu_ready, scenes):
    from sfm_amd.guided import guided_match_pairs
    a = scenes["a"]
    kps, descs, F = a["kps"], a["descs"], a["F"]
    clean = guided_match_pairs(kps, descs, [(0, 1)], [F], ratio=1.0)[0]
    nanF = F.copy(); nanF[1, 2] = np.nan
    # F = 0, an F with a NaN and a pair without a model between live pairs: nothing for them, the live pairs as alone
    pairs, Fs = [(0, 1), (0, 1), (1, 0), (0, 1), (0, 1)], [F, np.zeros((3, 3)), None, nanF, F]
    out, dbg = guided_match_pairs(kps, descs, pairs, Fs, ratio=1.0, return_debug=True)
    check(kps, descs, pairs, Fs, "hamming", ratio=1.0)
    for s in (1, 2, 3):
        assert len(out[s][0]) == 0 and dbg[s].sum() == 0 and len(dbg[s]) == len(kps[pairs[s][0]])
    for s in (0, 4):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(out[s], clean))
    # NaN / inf keypoints on either side give no candidate and the other queries keep their matches
    bad = [[np.nan, 5.0], [np.inf, 100.0], [200.0, -np.inf], [np.nan, np.nan]]
    rows = [3, 64, 200, 359]
    for side in (0, 1):
        k = [kps[0].copy(), kps[1].copy()]
        k[side][rows] = bad
        want, nc = check(k, descs, [(0, 1)], [F], "hamming", ratio=1.0)
        q, t, _ = want[0]
        if side == 0:
            assert nc[0][rows].sum() == 0
            keep = ~np.isin(clean[0], rows)
            assert q.tolist() == clean[0][keep].tolist() and t.tolist() == clean[1][keep].tolist()
        else:
            assert not np.isin(t, rows).any()
            untouched = ~np.isin(np.arange(360), np.flatnonzero(gr.gate(F, kps[0], kps[1], 3.0)[:, rows].any(1)))
            sel = np.isin(clean[0], np.flatnonzero(untouched))
            assert set(zip(clean[0][sel].tolist(), clean[1][sel].tolist())) <= set(zip(q.tolist(), t.tolist()))
        check(k, descs, [(0, 1), (1, 0)], [F, F.T], "hamming", ratio=0.8, cross_check=True)


# ------------------------------------------------------------------------------------------- determinism, position, cross-check
def test_repeatable_position_independent_and_cross_check_is_the_intersection(gpu_ready, scenes):
    from sfm_amd.guided import guided_match_pairs
    kps, descs, pairs, Fs = scenes["kps"], scenes["descs"]["hamming"], scenes["pairs"], scenes["Fs"]
    same = lambda x, y: all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(x, y))
    for cross in (False, True):
        one = guided_match_pairs(kps, descs, pairs, Fs, cross_check=cross)
        two = guided_match_pairs(kps, descs, pairs, Fs, cross_check=cross)
        assert all(same(a, b) for a, b in zip(one, two))
        order = [3, 0, 4, 2, 1]                              # another place in another batch, and alone
        moved = guided_match_pairs(kps, descs, [pairs[s] for s in order] + [(1, 0)], [Fs[s] for s in order] + [Fs[0].T], cross_check=cross)
        assert all(same(moved[k], one[s]) for k, s in enumerate(order))
        for s in (0, 3):
            assert same(guided_match_pairs(kps, descs, [pairs[s]], [Fs[s]], cross_check=cross)[0], one[s])
    # cross-check = the forward result intersected with the forward result of the swapped pair under F^T; ratio = inf takes
    # the ratio test (forward only by the rule) out of both.  F^T associates the sums of the rule differently, so the
    # identity needs the two gates to agree - a condition on the data, checked here: nothing of these scenes is within
    # 1e-9 of the threshold.
    for (i, j), F in zip(pairs, Fs):
        g, gt = gr.gate(F, kps[i], kps[j], 3.0), gr.gate(F.T, kps[j], kps[i], 3.0)
        assert gr.near_threshold(F, kps[i], kps[j], 3.0).sum() == 0 and (g == gt.T).all()
    inf = float("inf")
    fwd = guided_match_pairs(kps, descs, pairs, Fs, ratio=inf)
    swp = guided_match_pairs(kps, descs, [(j, i) for i, j in pairs], [F.T for F in Fs], ratio=inf)
    crs = guided_match_pairs(kps, descs, pairs, Fs, ratio=inf, cross_check=True)
    for f, s, c in zip(fwd, swp, crs):
        back = set(zip(s[1].tolist(), s[0].tolist()))
        keep = np.array([(q, t) in back for q, t in zip(f[0].tolist(), f[1].tolist())])
        assert 0 < keep.sum() < len(keep)
        assert same([x[keep] for x in f], c)


# ------------------------------------------------------------------------------------------- properties and the chain
@pytest.fixture(scope="module")
def chain(gpu_ready, scenes):
    from sfm_amd.matcher import ImageMatcher
    a = scenes["a"]
    m = ImageMatcher()
    pairs = [(0, 1), (1, 0)]
    blind = m.process_pairs(a["kps"], a["descs"], pairs)
    return m, a, pairs, blind


def test_blind_matches_inside_the_gate_survive_and_guided_matches_verify(chain):
    m, a, pairs, blind = chain
    kps, descs = a["kps"], a["descs"]
    assert all(r is not None for r in blind)
    guided = m.guided_pairs(kps, descs, pairs, blind, gate=3.0, ratio=m.ratio, cross_check=False)
    for r, g in zip(blind, guided):
        F = r["F"]
        e = fr.cv_err2(F, r["pts1"].astype(np.float64), r["pts2"].astype(np.float64))
        band = np.abs(e - 9.0) <= 1e-9 * 9.0
        assert band.mean() <= 0.01
        inside = (e <= 9.0) & ~band
        assert inside.sum() >= 100
        have = set(zip(g["matches"].queryIdx.tolist(), g["matches"].trainIdx.tolist()))
        assert {(q, t) for q, t in zip(r["matches"].queryIdx[inside].tolist(), r["matches"].trainIdx[inside].tolist())} <= have
        # every guided match has both point-line distances within the gate, so the mean of the two is below the verifier's 3 px
        e = fr.cv_err2(F, g["pts1"].astype(np.float64), g["pts2"].astype(np.float64))
        band = np.abs(e - 9.0) <= 1e-9 * 9.0
        assert band.mean() <= 0.01 and (e <= 9.0)[~band].all()
        assert g["inlier_mask"][~band].all()
        assert g["F"] is F and g["n_unguided"] == len(r["matches"]) and len(g["matches"]) > len(r["matches"])
        i, j = pairs[0] if g is guided[0] else pairs[1]
        assert g["pts1"].tobytes() == kps[i][g["matches"].queryIdx].tobytes() and g["pts2"].tobytes() == kps[j][g["matches"].trainIdx].tobytes()
        assert set(g) == set(r) | {"n_unguided"} and g["metrics"]["total_matches"] == len(g["matches"])


def test_chain_gives_more_tracks_and_the_default_is_untouched(chain):
    m, a, pairs, blind = chain
    kps, descs = a["kps"], a["descs"]
    off = m.process_pairs(kps, descs, pairs, guided=False)
    assert len(off) == len(blind)
    for x, y in zip(off, blind):                             # guided=False is today's process_pairs, key for key
        assert set(x) == set(y) and "n_unguided" not in x
        assert x["matches"] == y["matches"] and x["quality_ok"] == y["quality_ok"] and x["metrics"] == y["metrics"]
        for key in ("pts1", "pts2", "F", "inlier_mask", "symmetric_errors"):
            assert np.asarray(x[key]).tobytes() == np.asarray(y[key]).tobytes()
    on = m.process_pairs(kps, descs, pairs, guided=True)
    t_off, t_on = m.build_tracks(kps, pairs, off), m.build_tracks(kps, pairs, on)
    n_off, n_on = int((t_off.lengths() >= 2).sum()), int((t_on.lengths() >= 2).sum())
    assert n_on > n_off > 0
    truth = a["truth"](0, 1)
    g = on[0]["matches"]
    assert gr.count_correct(g.queryIdx, g.trainIdx, truth) > gr.count_correct(off[0]["matches"].queryIdx, off[0]["matches"].trainIdx, truth)


def test_float_descriptors_are_converted_or_refused(gpu_ready, scenes):
    from sfm_amd.guided import guided_match_pairs
    kps, pairs, Fs = scenes["kps"], scenes["pairs"][:2], scenes["Fs"][:2]
    d8 = scenes["descs"]["l2"]
    a = guided_match_pairs(kps, d8, pairs, Fs, metric="l2")
    b = guided_match_pairs(kps, [d.astype(np.float32) for d in d8], pairs, Fs)
    assert all(x.tobytes() == y.tobytes() for p, q in zip(a, b) for x, y in zip(p, q)) and len(a[0][0]) > 100
