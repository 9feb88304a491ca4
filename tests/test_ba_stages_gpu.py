"""The damped solve on the GPU, stage by stage, against the 80-bit reference of tests/stage_reference.py: every stage is
referenced from the DEVICE'S OWN inputs to that stage (the public workspace regions of sfm_ba_layout), so its bound is that
of the stage's own arithmetic - G = W L^-T, the item tiles summed into S, the right-hand side r, the camera solve on every
route, the back-substitution, the reduce_q pieces and the scalars.  precision="mixed" is held to the SAME bounds as fp64: its
inputs are the stored float32 rows, everything after them is promised to be float64.  Then the bitwise contracts: repeated
builds, the XCD grouping of the work lists, and call sequences that exercise the cached state of the solve."""
import ctypes as C

import numpy as np
import pytest

import stage_reference as sr

pytestmark = pytest.mark.gpu

ALPHA_REL = (1e-9, 1e-3, 10.0)
MAIN = ["edge", "aligned", "dup", "mixed", "c2", "c5"]
GRID = [(v, d, p) for v in MAIN + ["tile"] for d in (10, 6) for p in ("fp64", "mixed")]
ROUTES = {"cholesky": ("cholesky", {}), "cg": ("cg", {}), "cg_per_launch": ("cg", {"SFM_CGS_PERSIST": "0"}),
          "cg_tiles": ("cg", {"SFM_CGS_PERSIST": "0", "SFM_CGS_BIG_FROM": "257"})}
_scenes, _runs = {}, {}


def scene(variant, d):
    if variant == "tile":                        # n = C d >= 257: 30 cameras of 10 parameters, 45 of 6
        variant = "tile30" if d == 10 else "tile45"
    if variant not in _scenes:
        _scenes[variant] = sr.edge_scene(variant)
    return _scenes[variant]


def backend(sc, d, precision="fp64", camera_solver="cholesky"):
    from sfm_amd.ba import GpuBA
    return GpuBA(np.ascontiguousarray(sc.cams0[:, :d]), sc.pts0, sc.cam_idx, sc.pt_idx, sc.uv, sc.K, precision=precision,
                 camera_solver=camera_solver)


def host(be, off, count, dtype=None):
    return be.view(off, count, dtype).cpu().numpy().astype(np.float64)


def read_inputs(be):
    """The stage inputs as the device holds them: the Jacobian rows (float32 under mixed precision, widened exactly), B, g_c,
    C_p, g_p."""
    L, N, d, Cn, P = be.lay, be.N, be.d, be.C, be.P
    assert L.rec_stride == 2 * d * be.rec_dtype.itemsize
    recB = host(be, L.recB_off, N * 8, be.rec_dtype).reshape(N, 8)
    return dict(Jc=host(be, L.rec_off, N * 2 * d, be.rec_dtype).reshape(N, 2, d), Jp=recB[:, :6].reshape(N, 2, 3),
                B=host(be, L.B_off, Cn * d * d).reshape(Cn, d, d), gc=host(be, L.gc_off, Cn * d),
                Cp6=host(be, L.Cp_off, P * 6).reshape(P, 6), gp=host(be, L.gp_off, P * 3).reshape(P, 3))


def read_G(be):
    """(G [N][3][d], the padding doubles of every block)."""
    gs = 32 if be.d == 10 else 18
    raw = host(be, be.lay.G_off, be.N * gs).reshape(be.N, gs)
    return raw[:, :3 * be.d].reshape(be.N, 3, be.d).copy(), raw[:, 3 * be.d:].copy()


def read_Sr(be):
    n = be.n
    raw = host(be, be.lay.reduce_S_off, n * n + n)
    return raw[:n * n].reshape(n, n).copy(), raw[n * n:].copy()


def build(be, alpha):
    be.h.call("sfm_ba_schur_build", be._pp, C.c_double(alpha))


def solve(be, alpha, want_q=1):
    """sfm_ba_schur_solve + sfm_ba_finish_solve + the scalars (PNORM2, PQ)."""
    from sfm_amd import _lib
    be.h.call("sfm_ba_schur_solve", be._pp, C.c_double(alpha), want_q)
    be.h.call("sfm_ba_finish_solve", be._pp, want_q)
    be._solve_scalars(alpha)
    s = be.scalars()
    return s[_lib.SC_PNORM2], s[_lib.SC_PQ]


def step_of(be):
    return np.concatenate([host(be, be.lay.pc_off, be.n), host(be, be.lay.pp_off, be.P * 3)])


def run(variant, d, precision):
    """One backend per grid point on the factorisation route: every stage result at every alpha, copied to the host."""
    key = (variant, d, precision)
    if key in _runs:
        return _runs[key]
    sc = scene(variant, d)
    be = backend(sc, d, precision)
    _, _, _, hdiag = be.linearize()
    st = be.structure()
    sr.assert_edges(sc, st)
    assert be.n_items == int(st["item_ptr"][-1])
    inp = read_inputs(be)
    inp.update(cam_idx=sc.cam_idx, pt_idx=sc.pt_idx)

    def ref_S_at(alpha):
        build(be, alpha)
        return sr.stage_S(read_G(be)[0], inp["B"], st, sc.C)[0]

    pcs = sr.pc_alphas(ref_S_at, hdiag)
    out = dict(sc=sc, st=st, inp=inp, hdiag=hdiag, pcs=pcs, at={})
    for rel in sorted(set(ALPHA_REL) | set(pcs)):
        alpha = rel * hdiag
        build(be, alpha)
        G, pad = read_G(be)
        S, r = read_Sr(be)                        # BEFORE the solve: the factorisation works in place on S | r
        got = dict(alpha=alpha, G=G, pad=pad, S=S, r=r)
        if rel in pcs:
            pn2, pq = solve(be, alpha)
            got.update(pc=host(be, be.lay.pc_off, be.n), pp=host(be, be.lay.pp_off, be.P * 3).reshape(-1, 3),
                       redq=host(be, be.lay.reduce_q_off, be.n + 2), pnorm2=pn2, pq=pq)
        out["at"][rel] = got
    assert be.solver_stats() == (0, 0)
    be.close()
    _runs[key] = out
    return out


def each_alpha(variant, d, precision, need_pc=False):
    R = run(variant, d, precision)
    for rel, got in R["at"].items():
        if need_pc and "pc" not in got:
            continue
        yield R, rel, got


def check(stage, variant, d, precision, rel, ratio, where):
    print(f"{stage} {variant} d={d} {precision} alpha={rel:g} x hdiag: {ratio:.3g} of its bound at {where}")
    assert ratio <= 1.0, f"{stage}: {ratio:.3g} x its bound at {where} (alpha = {rel:g} x hdiag)"


@pytest.mark.parametrize("variant,d,precision", GRID)
def test_stage_G(gpu_ready, variant, d, precision):
    """G_k = (Jp~ M_j^T)^T Jc~ per observation to C_G u kappa2(A_j) ||Jc~|| ||Jp~|| ||M_j||; the padding doubles exactly 0."""
    for R, rel, got in each_alpha(variant, d, precision):
        inp = R["inp"]
        assert not np.any(got["pad"]), "padding doubles of a G block are not zero"
        ratio, where = sr.judge_G(inp["Jc"], inp["Jp"], inp["Cp6"], inp["pt_idx"], got["alpha"], got["G"])
        check("G", variant, d, precision, rel, ratio, where)


@pytest.mark.parametrize("variant,d,precision", GRID)
def test_stage_S(gpu_ready, variant, d, precision):
    """S from the device's G and B: componentwise inside (3m + 2) u T, exact zeros where the structure has no pair, nothing but
    zeros or exact transposes above the diagonal blocks."""
    for R, rel, got in each_alpha(variant, d, precision):
        ratio, where, problems = sr.judge_S(got["G"], R["inp"]["B"], R["st"], R["sc"].C, got["S"])
        assert not problems, problems
        check("S", variant, d, precision, rel, ratio, where)


@pytest.mark.parametrize("variant,d,precision", GRID)
def test_stage_r(gpu_ready, variant, d, precision):
    for R, rel, got in each_alpha(variant, d, precision):
        inp = R["inp"]
        ratio, where = sr.judge_r(got["G"], inp["Cp6"], inp["gp"], inp["gc"], got["alpha"], inp["cam_idx"], inp["pt_idx"],
                                  R["sc"].C, got["r"])
        check("r", variant, d, precision, rel, ratio, where)


@pytest.mark.parametrize("variant,d,precision", GRID)
def test_stage_pc_by_the_factorisation(gpu_ready, variant, d, precision):
    """rho = r + (S + alpha I) p_c with the device's S, r (read before the solve) and p_c."""
    for R, rel, got in each_alpha(variant, d, precision, need_pc=True):
        ratio, where = sr.judge_pc_factor(got["S"], got["r"], got["alpha"], got["pc"])
        rig = sr.factor_rigorous_ratio(got["S"], got["r"], got["alpha"], got["pc"])
        print(f"  against the rigorous (3n + 1) u |L||L^T||p_c|: {rig:.3g}")
        assert rig <= 1.0
        check("p_c", variant, d, precision, rel, ratio, where)


@pytest.mark.parametrize("variant,d,precision", GRID)
def test_stage_pp(gpu_ready, variant, d, precision):
    for R, rel, got in each_alpha(variant, d, precision, need_pc=True):
        inp = R["inp"]
        ratio, where = sr.judge_pp(got["G"], inp["Cp6"], inp["gp"], got["alpha"], got["pc"], inp["cam_idx"], inp["pt_idx"], got["pp"])
        check("p_p", variant, d, precision, rel, ratio, where)


@pytest.mark.parametrize("variant,d,precision", GRID)
def test_stage_q_pieces_and_scalars(gpu_ready, variant, d, precision):
    """reduce_q = [q_c | sum ||p_p||^2 | sum ||v||^2] from the device's G and p_p; PNORM2 and PQ as k_finish_solve combines them."""
    for R, rel, got in each_alpha(variant, d, precision, need_pc=True):
        inp = R["inp"]
        rq, rp, rv, where = sr.judge_q(got["G"], inp["Cp6"], got["alpha"], got["pp"], inp["cam_idx"], inp["pt_idx"], R["sc"].C, got["redq"])
        check("q_c", variant, d, precision, rel, rq, where)
        check("sum ||p_p||^2", variant, d, precision, rel, rp, "reduce_q[n]")
        check("sum ||v||^2", variant, d, precision, rel, rv, "reduce_q[n + 1]")
        r_pn, r_pq, kappa = sr.judge_scalars(got["S"], got["alpha"], got["pc"], got["redq"], got["pnorm2"], got["pq"], cg=False)
        check("PNORM2", variant, d, precision, rel, r_pn, "the scalar")
        check("PQ", variant, d, precision, rel, r_pq, f"the scalar (kappa2(S + alpha I) = {kappa:.3g})")


# (the tile-streaming route needs n = C d >= 257: it runs on the 30 / 45 camera scene only)
ROUTE_CASES = [(r, v, d) for r in ROUTES for v in ("edge", "tile") for d in (10, 6) if not (r == "cg_tiles" and v == "edge")]


@pytest.mark.parametrize("route,variant,d", ROUTE_CASES)
def test_stage_pc_on_every_route(gpu_ready, monkeypatch, route, variant, d):
    """The camera solve on the factorisation, the persistent CG, the launch-per-iteration CG and the tile-streaming CG (which
    needs n >= 257: the 30 / 45 camera scene), the route passed explicitly.  The CG routes are held to the library's contract:
    relative residual 1e-13 on the block-scaled system, with the reference's own factors of the diagonal blocks.  A system
    that fell back to the factorisation is judged by the factorisation's bound; no fallback at alpha >= 1e-3 hdiag.  On the
    fused tile route the build leaves S~ only: S comes from a second backend under SFM_SCHUR_FUSE_SCALE=0
    (test_scaled_system_straight_from_the_item_tiles pins that both hold the same S bit for bit)."""
    solver, env = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    R = run(variant, d, "fp64")
    sc, hdiag = R["sc"], R["hdiag"]
    be = backend(sc, d, camera_solver=solver)
    be.linearize()
    other = None
    if route == "cg_tiles":
        other = backend(sc, d, camera_solver=solver)
        other.linearize()
    for rel in R["pcs"]:
        alpha = rel * hdiag
        build(be, alpha)
        S, r = read_Sr(be)
        if other is not None:
            monkeypatch.setenv("SFM_SCHUR_FUSE_SCALE", "0")
            build(other, alpha)
            S, r2 = read_Sr(other)
            monkeypatch.delenv("SFM_SCHUR_FUSE_SCALE")
            assert np.array_equal(r, r2)
        assert np.array_equal(r, R["at"][rel]["r"]) and np.array_equal(np.tril(S), np.tril(R["at"][rel]["S"]))
        before = be.solver_stats()
        pn2, pq = solve(be, alpha)
        its, fell = (a - b for a, b in zip(be.solver_stats(), before))
        pc, redq = host(be, be.lay.pc_off, be.n), host(be, be.lay.reduce_q_off, be.n + 2)
        floor = rel < 1e-3
        if solver == "cholesky":
            assert (its, fell) == (0, 0)
        else:
            assert floor or fell == 0, f"the camera CG fell back to the factorisation at alpha = {rel:g} x hdiag"
        by_cg = solver == "cg" and fell == 0
        if by_cg:
            assert its > 0
            ratio, where = sr.judge_pc_cg(S, r, alpha, pc, sc.C, floor)
        else:
            ratio, where = sr.judge_pc_factor(S, r, alpha, pc)
        print(f"route {route}: {its} CG iterations, {fell} fallbacks" + ("" if by_cg else " - judged by the factorisation's bound"))
        check("p_c", variant, d, route, rel, ratio, where)
        r_pn, r_pq, kappa = sr.judge_scalars(S, alpha, pc, redq, pn2, pq, cg=solver == "cg", floor=floor)
        check("PNORM2", variant, d, route, rel, r_pn, "the scalar")
        check("PQ", variant, d, route, rel, r_pq, f"the scalar (kappa2(S + alpha I) = {kappa:.3g})")


# ------------------------------------------------------------------------------------------------ bitwise, no tolerance
@pytest.mark.parametrize("precision", ["fp64", "mixed"])
@pytest.mark.parametrize("d", [10, 6])
def test_two_builds_give_the_same_bits(gpu_ready, d, precision):
    sc = scene("edge", d)
    be = backend(sc, d, precision)
    _, _, _, hdiag = be.linearize()
    seen = []
    for alpha in (1e-3 * hdiag, 10.0 * hdiag, 1e-3 * hdiag):
        build(be, alpha)
        seen.append((read_G(be)[0],) + read_Sr(be))
    for a, b in zip(seen[0], seen[2]):
        assert np.array_equal(a, b)
    assert not np.array_equal(seen[0][0], seen[1][0])


@pytest.mark.parametrize("d", [10, 6])
@pytest.mark.parametrize("variant", ["edge", "tile"])
def test_xcd_grouping_of_the_work_lists_changes_no_sum(gpu_ready, monkeypatch, variant, d):
    """SFM_XCD_GROUP=contig / mod8 (read when the problem is created) deal the work items to other workgroups: who runs an item
    must not change S, r or the step."""
    sc = scene(variant, d)
    got = {}
    for grp in ("contig", "mod8"):
        monkeypatch.setenv("SFM_XCD_GROUP", grp)
        be = backend(sc, d)
        _, _, _, hdiag = be.linearize()
        alpha = 1e-3 * hdiag
        build(be, alpha)
        S, r = read_Sr(be)
        sc_ = solve(be, alpha)
        got[grp] = (be.structure()["xcd_items"], S, r, step_of(be), sc_)
        be.close()
    assert not np.array_equal(got["contig"][0], got["mod8"][0]), "the two groupings deal the items alike: nothing is tested"
    for a, b in zip(got["contig"][1:4], got["mod8"][1:4]):
        assert np.array_equal(a, b)
    assert got["contig"][4] == got["mod8"][4]


@pytest.mark.parametrize("route", ["cholesky", "cg", "cg_tiles"])
def test_no_stale_state_across_call_sequences(gpu_ready, monkeypatch, route):
    """After legal sequences of the stage calls the step, PNORM2 and PQ equal, bit for bit, those of a fresh backend doing
    build(alpha1); solve alone: what the solve caches between calls (S formed or not, the alpha of the scaled system and of the
    diagonal blocks' factors, the cleared CG status words) must never leak from an earlier call.  One exception is the
    library's documented behaviour: sfm_ba_unpack_system stands for an exchange that changed S, so on the fused tile route the
    scaled system is formed again from S afterwards - bit for bit the route under SFM_SCHUR_FUSE_SCALE=0."""
    import torch
    solver, env = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = 10
    sc = scene("tile", d)

    def fresh(unfused=False):
        if unfused:
            monkeypatch.setenv("SFM_SCHUR_FUSE_SCALE", "0")
        be = backend(sc, d, camera_solver=solver)
        _, _, _, hdiag = be.linearize()
        build(be, 1e-3 * hdiag)
        out = (solve(be, 1e-3 * hdiag), step_of(be))
        if unfused:
            monkeypatch.delenv("SFM_SCHUR_FUSE_SCALE")
        be.close()
        return out, hdiag

    want, hdiag = fresh()
    a1, a2 = 1e-3 * hdiag, 3e-6 * hdiag

    def seq_alternate(be):
        build(be, a1); solve(be, a1); build(be, a2); solve(be, a2); build(be, a1)

    def seq_builds_only(be):
        build(be, a1); build(be, a2); build(be, a1)

    def seq_pack(be):
        build(be, a1); be.h.call("sfm_ba_pack_system", be._pp); be.h.call("sfm_ba_unpack_system", be._pp)

    def seq_want_q(be):
        build(be, a1); solve(be, a1, 0); build(be, a1)

    def seq_relinearize(be):
        x2 = be.x + 1e-3 * torch.sin(torch.arange(be.x.numel(), device=be.x.device, dtype=be.x.dtype))
        be.h.call("sfm_ba_linearize", be._pp, C.c_void_p(x2.data_ptr())); be.h.call("sfm_ba_finish_linearize", be._pp)
        build(be, a2); solve(be, a2)
        be.linearize()
        build(be, a1)

    for seq in (seq_alternate, seq_builds_only, seq_pack, seq_want_q, seq_relinearize):
        be = backend(sc, d, camera_solver=solver)
        be.linearize()
        seq(be)
        before = be.solver_stats()                 # (a system at the small alpha2 may have gone to the factorisation: that is legal)
        got = (solve(be, a1), step_of(be))
        stats = tuple(a - b for a, b in zip(be.solver_stats(), before))
        be.close()
        ref = fresh(unfused=True)[0] if (route == "cg_tiles" and seq is seq_pack) else want
        assert got[0] == ref[0], (seq.__name__, got[0], ref[0])
        assert np.array_equal(got[1], ref[1]), seq.__name__
        assert stats[1] == 0 and (stats[0] > 0) == (solver == "cg")
