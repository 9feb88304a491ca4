"""CPU self-tests of tests/stage_reference.py: the float64 transcription of the reference formulas stays inside every stage
bound on every scene (this is where the recorded constants come from), seeded defects break the bounds, and the scenes hold
the edges and the residual regime they were built for.  No GPU."""
import numpy as np
import pytest

import stage_reference as sr

VARIANTS = ["edge", "aligned", "dup", "mixed", "c2", "c5", "tile30", "tile45"]
ALPHA_REL = (1e-9, 1e-3, 10.0)
_cache = {}


def host_inputs(variant, d):
    """The linearisation at the scene's start point by the oracle: the inputs of the damped solve's stages."""
    key = (variant, d)
    if key not in _cache:
        from oracle import ba_oracle as bo
        from sfm_amd.structure import build_structure
        sc = sr.edge_scene(variant)
        prob = bo.BAProblem(sc.C, sc.P, d, sc.cam_idx, sc.pt_idx, sc.uv, np.array(sc.K))
        x0 = np.concatenate([sc.cams0[:, :d].ravel(), sc.pts0.ravel()])
        lin = bo.linearize(x0, prob)
        iu = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        n = sc.C * d
        inp = dict(Jc=lin.Jc, Jp=lin.Jp, B=lin.B, Cp6=np.stack([lin.Cp[:, i, j] for i, j in iu], axis=1), gc=lin.g[:n],
                   gp=lin.g[n:].reshape(-1, 3), cam_idx=sc.cam_idx, pt_idx=sc.pt_idx,
                   hdiag=max(np.max(np.einsum("cii->ci", lin.B)), np.max(np.einsum("pii->pi", lin.Cp))),
                   f=lin.f[:2 * prob.n_obs].reshape(-1, 2))
        _cache[key] = (sc, build_structure(sc.cam_idx, sc.pt_idx, sc.C, sc.P), inp)
    return _cache[key]


# ---------------------------------------------------------------------------------------------- the scenes
@pytest.mark.parametrize("variant", VARIANTS)
def test_scene_holds_its_edges_and_residual_regime(variant):
    sc, st, inp = host_inputs(variant, 10)
    sr.assert_edges(sc, st)
    N, P = sc.cam_idx.shape[0], sc.P
    assert sc.C * 10 <= 600 and N < 8000
    if variant == "aligned":
        assert N % 256 == 0 and P % 256 == 0
    if variant == "edge":
        assert N % 256 and P % 256 and sc.C % 8
    if variant == "dup":
        same = (sc.pt_idx[1:] == sc.pt_idx[:-1]) & (sc.cam_idx[1:] == sc.cam_idx[:-1])
        assert same.any()
        a, b = sr.block_items(st, sc.C, 8, 8)
        assert a > int(np.sum(sc.cam_idx == 8))            # a diagonal block with pairs k != k2
    if variant.startswith("tile"):
        assert sc.C * (10 if variant == "tile30" else 6) >= 257
    # Huber regime on the oracle's f: SciPy scales rows with |f| > 1 by ~sqrt(eps), a scene of outliers cannot see a dropped pair
    linear = float(np.mean(np.any(np.abs(inp["f"]) > 1.0, axis=1)))
    print(variant, "observations with a Huber-linear row:", linear)
    if variant == "mixed":
        assert 0.2 <= linear <= 0.5
    else:
        assert linear <= 0.02
    kap = sr.point_kappa(inp["Cp6"], 1e-3 * inp["hdiag"])
    print(variant, "largest kappa2(A_j) at 1e-3 hdiag:", kap.max(), " at the floor:", sr.point_kappa(inp["Cp6"], 1e-9 * inp["hdiag"]).max())
    assert kap.max() <= 100.0


def test_work_item_and_chunk_counts_of_the_split():
    """build_structure on blocks of 255 / 256 / 257 / 512 / 513 pairs and cameras of 511 / 512 / 513 / 1,025 observations."""
    from sfm_amd.structure import build_structure
    tracks = [(0, 1)] * 255 + [(0, 2)] * 256 + [(1, 2)] * 257 + [(0, 3)] * 512 + [(1, 3)] * 513
    ci = np.array([c for t in tracks for c in t]); pi = np.repeat(np.arange(len(tracks)), 2)
    st = build_structure(ci, pi, 4, len(tracks))
    assert [sr.block_items(st, 4, a, b)[1] for a, b in ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3))] == [1, 1, 2, 2, 3]
    obs = [511, 512, 513, 1025]
    ci = np.repeat(np.arange(4), obs); pi = np.arange(ci.shape[0])
    st = build_structure(ci, pi, 4, ci.shape[0])
    assert list(np.diff(st.cch_ptr)) == [2, 2, 3, 5] and st.n_cchunks == 12


# ---------------------------------------------------------------------------------------------- the transcription inside the bounds
def judge_all(inp, st, C, alpha, got, cg=False, pc=True, floor=False):
    """Every stage of `got` (the chain's results under the workspace's names) against its bound, each from the inputs in `got`
    itself.  Returns {stage: (ratio to the bound, where)}."""
    ci, pi = inp["cam_idx"], inp["pt_idx"]
    d = inp["Jc"].shape[2]
    G = np.asarray(got["G"], dtype=np.float64)
    out = {"G": sr.judge_G(inp["Jc"], inp["Jp"], inp["Cp6"], pi, alpha, G)}
    rS, where, problems = sr.judge_S(G, inp["B"], st, C, got["S"])
    assert not problems, problems
    out["S"] = (rS, where)
    out["r"] = sr.judge_r(G, inp["Cp6"], inp["gp"], inp["gc"], alpha, ci, pi, C, got["r"])
    if pc:
        out["pc"] = sr.judge_pc_cg(got["S"], got["r"], alpha, got["pc"], C, floor) if cg else sr.judge_pc_factor(got["S"], got["r"], alpha, got["pc"])
        out["pp"] = sr.judge_pp(G, inp["Cp6"], inp["gp"], alpha, got["pc"], ci, pi, got["pp"])
        rq, rp, rv, where = sr.judge_q(G, inp["Cp6"], alpha, got["pp"], ci, pi, C, got["redq"])
        out["q"] = (rq, where); out["sum_pp2"] = (rp, ""); out["sum_v2"] = (rv, "")
        r_pn, r_pq, kappa = sr.judge_scalars(got["S"], alpha, got["pc"], got["redq"], got["pnorm2"], got["pq"], cg, floor)
        out["PNORM2"] = (r_pn, ""); out["PQ"] = (r_pq, f"kappa2(S + alpha I) = {kappa:.3g}")
    return out


RAW = {"G": sr.C_G, "pp": sr.C_PP, "pc": sr.C_FACT, "PQ": sr.C_PQ}


# (the tile scenes exist once per camera block size: 30 cameras for d = 10, 45 for d = 6)
SCENE_D = [(v, d) for v in VARIANTS for d in (10, 6) if (v, d) not in (("tile30", 6), ("tile45", 10))]


@pytest.mark.parametrize("variant,d", SCENE_D)
def test_float64_transcription_stays_inside_every_bound(variant, d):
    sc, st, inp = host_inputs(variant, d)
    C = sc.C
    pcs = sr.pc_alphas(lambda a: sr.stage_S(sr.transcription(inp, st, C, a)["G"], inp["B"], st, C)[0], inp["hdiag"])
    for rel in sorted(set(ALPHA_REL) | set(pcs)):
        alpha = rel * inp["hdiag"]
        got = sr.transcription(inp, st, C, alpha)
        res = judge_all(inp, st, C, alpha, got, pc=rel in pcs)
        if "pc" in res:
            e_raw, v_raw = sr.measure_e_v(inp["Cp6"], inp["gp"], alpha, got["e"], got["pp"], got["v"])
            print(f"{variant} d={d} alpha={rel:g}: raw e {e_raw:.3g} v {v_raw:.3g} PQ/C_PQ-scale {res['PQ'][0] * 1:.3g}")
            # the constants are 8 x the ratios recorded from this very loop: a transcription beyond the record means the record is stale
            assert e_raw <= 1.02 * sr.C_E / 8 and v_raw <= 1.02 * sr.C_V / 8
        for k, (ratio, where) in res.items():
            print(f"{variant} d={d} alpha={rel:g} {k}: ratio to bound {ratio:.3g} (raw {ratio * RAW.get(k, 1.0):.3g}) {where}")
            assert ratio <= (1.02 / 8 if k in RAW else 1.0), (k, ratio, where)
    for rel in pcs:                                        # the CG contract, by the float64 CG on the block-scaled system
        alpha = rel * inp["hdiag"]
        got = sr.transcription(inp, st, C, alpha, cg=True)
        ratio, where = sr.judge_pc_cg(got["S"], got["r"], alpha, got["pc"], C, floor=rel < 1e-3)
        print(f"{variant} d={d} alpha={rel:g} CG: ratio {ratio:.3g} (raw {ratio * sr.cg_margin(rel < 1e-3):.3g}) {where}")
        assert ratio <= 1.02 / 8
    if 1e-6 in pcs:
        print(f"{variant} d={d}: the p_c floor case moved up to 1e-6 hdiag")


# ---------------------------------------------------------------------------------------------- seeded defects
def _inlier_obs_of_block(sc, st, inp, a, b, which=-1):
    """(pair index, observation k, observation k2) of a pair of block (a, b) whose two observations are inliers."""
    i = a * sc.C - a * (a - 1) // 2 + (b - a)
    lo, hi = int(st.blk_ptr[i]), int(st.blk_ptr[i + 1])
    inl = np.all(np.abs(inp["f"]) <= 1.0, axis=1)
    idx = [p for p in range(lo, hi) if inl[st.pair_k[p]] and inl[st.pair_k2[p]]]
    p = idx[which]
    return p, int(st.pair_k[p]), int(st.pair_k2[p])


@pytest.mark.parametrize("d", [10, 6])
def test_seeded_defects_break_the_bounds(d):
    sc, st, inp = host_inputs("edge", d)
    C = sc.C
    alpha = 1e-3 * inp["hdiag"]
    good = sr.transcription(inp, st, C, alpha)
    G = good["G"]
    ci, pi = inp["cam_idx"], inp["pt_idx"]
    i03 = 0 * C + 3
    lo, hi = int(st.blk_ptr[i03]), int(st.blk_ptr[i03 + 1])
    assert hi - lo == 257
    inl = np.all(np.abs(inp["f"]) <= 1.0, axis=1)

    # the last pair of the 257-pair block (the one pair of its second work item) dropped
    assert inl[st.pair_k[hi - 1]] and inl[st.pair_k2[hi - 1]]
    mask = np.ones(st.n_pairs, dtype=bool); mask[hi - 1] = False
    bad = sr.stage_S(G, inp["B"], st, C, np.float64, pair_mask=mask)[0]
    ratio, where, _ = sr.judge_S(G, inp["B"], st, C, bad)
    print("dropped pair:", ratio, where)
    assert ratio >= 100 and where.startswith("block (3, 0)")

    # one G block rounded to float32 / one block off by 1e-10 relative (every term it takes part in)
    p, k, k2 = _inlier_obs_of_block(sc, st, inp, 0, 3, which=100)
    for name, fn, need in (("float32 block", lambda g: g.astype(np.float32).astype(np.float64), 100.0),
                           ("1e-10 relative", lambda g: g * (1 + 1e-10), 1.0)):
        Gb = G.copy(); Gb[k] = fn(Gb[k])
        bad = sr.stage_S(Gb, inp["B"], st, C, np.float64)[0]
        ratio, where, _ = sr.judge_S(G, inp["B"], st, C, bad)
        print(name, ratio, where)
        assert ratio > need

    # alpha left off one point's A_j; M[1] and M[3] swapped for one point: seen in that point's G blocks
    j = int(pi[k])
    a_vec = np.full(sc.P, alpha); a_vec[j] = 0.0
    M6 = sr.point_factors(inp["Cp6"], alpha, np.float64)
    for name, M6b in (("alpha left off", sr.point_factors(inp["Cp6"], a_vec, np.float64)), ("M[1] <-> M[3]", M6[:, [0, 3, 2, 1, 4, 5]])):
        Mb = M6.copy(); Mb[j] = M6b[j]
        bad = sr.stage_G(inp["Jc"], inp["Jp"], sr.unpack_M(Mb), pi)
        ratio, where = sr.judge_G(inp["Jc"], inp["Jp"], inp["Cp6"], pi, alpha, bad)
        print(name, ratio, where)
        assert ratio >= 100 and f"(point {j}," in where
        e_bad = sr.stage_e(sr.unpack_M(Mb), inp["gp"])
        pp_bad = sr.stage_pp(G, sr.unpack_M(Mb), e_bad, good["pc"], ci, pi, sc.P)
        ratio, where = sr.judge_pp(G, inp["Cp6"], inp["gp"], alpha, good["pc"], ci, pi, pp_bad)
        print(name, "in p_p:", ratio, where)
        assert ratio >= 100 and where.startswith(f"point {j} ")

    # an off-diagonal block taken from its tile without the transpose (the assembler's element index of a DIAGONAL block)
    bad = good["S"].copy()
    bad[3 * d:4 * d, 0:d] = bad[3 * d:4 * d, 0:d].T.copy()
    ratio, where, _ = sr.judge_S(G, inp["B"], st, C, bad)
    print("transposed block:", ratio, where)
    assert ratio >= 100 and where.startswith("block (3, 0)")

    # one chunk partial of r skipped (the second chunk of camera 3), and a single inlier observation of it
    obs3 = st.cam_obs[st.cam_ptr[3]:st.cam_ptr[4]]
    for name, drop in (("chunk", obs3[256:512]), ("observation", obs3[256:257])):
        assert inl[drop].any()
        keep = np.ones(ci.shape[0], dtype=bool); keep[drop] = False
        bad = sr.cam_reduce(G, good["e"], inp["gc"], ci, pi, C, np.float64, obs_mask=keep)[0]
        ratio, where = sr.judge_r(G, inp["Cp6"], inp["gp"], inp["gc"], alpha, ci, pi, C, bad)
        print("r without one", name, ratio, where)
        assert ratio >= 100 and "(camera 3," in where

    # a float32 slip in one accumulator of q, and a residual of the factorisation route that is off in one row
    redq = good["redq"].copy(); redq[3 * d] = np.float32(redq[3 * d])
    assert sr.judge_q(G, inp["Cp6"], alpha, good["pp"], ci, pi, C, redq)[0] >= 100
    pc = good["pc"].copy(); pc[5] *= 1 + 1e-9
    assert sr.judge_pc_factor(good["S"], good["r"], alpha, pc)[0] >= 100
    assert sr.judge_pc_cg(good["S"], good["r"], alpha, pc, C)[0] > 1
