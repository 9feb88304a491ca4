"""The stages that run once per outer iteration - linearisation and trial step - through the stage API, on scenes laid out
against the 256-observation workgroups of their kernels: a last workgroup that is short, half full (the trial step's second
block of 256 rows is missing) or full, tracks inside one workgroup, tracks across a boundary and one track longer than a
workgroup, and a camera system of 260 cameras (more than one workgroup of per-camera threads).

Tolerances are those of tests/test_ba_gpu.py: 1e-11 of the largest entry for the linearisation's blocks (test_linearize_matches_oracle),
rel 1e-8 / 1e-8 / 1e-9 / 1e-10 for js2, gts, ||s||, ||x_new|| (test_damped_solve_matches_oracle).  In mixed precision the
records are float32: they are held against the oracle's at float32 rounding (2^-24 relative), and the blocks - float64 sums over
what was stored - against the same sums over the records read back, at the float64 tolerance."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SQRT_EPS = 1.4901161193847656e-08
SCENES = ["short", "full", "ragged", "long_track"]
DIMS = [10, 6]
PRECISIONS = ["fp64", "mixed"]


def _track_lengths(n_obs, rng):
    """Track lengths from 2 to 7 that add up to n_obs."""
    out, left = [], n_obs
    while left:
        L = int(rng.integers(2, 8))
        if L > left or left - L == 1:
            L = left if left <= 7 else L - 1 if L > 2 else L + 1
        out.append(L)
        left -= L
    assert all(2 <= L <= 7 for L in out) and sum(out) == n_obs
    return out


@functools.lru_cache(maxsize=None)
def _scene(name, extra_front=False):
    """(n_cams, n_pts, cam_idx, pt_idx, uv, cams0 [C,10], pts0): point-major observations.  extra_front: one more point, seen by
    three cameras, in front of all the others - every other track moves by 3 observations."""
    from sfm_amd import synth
    n_cams, n_obs = {"short": (7, 150), "full": (7, 256), "ragged": (7, 1003), "long_track": (260, 0)}[name]
    rng = np.random.default_rng({"short": 11, "full": 12, "ragged": 13, "long_track": 14}[name])
    if name == "long_track":
        lengths = _track_lengths(254, rng) + [260] + _track_lengths(175, rng)     # observations 254 .. 513: over 256 and over 512
    else:
        lengths = _track_lengths(n_obs, rng)
    if extra_front:
        lengths = [3] + lengths
    P = len(lengths)
    full = synth.make_scene(n_cams, P, obs_per_point=None, seed=21, cam_sigma=0.005)     # every camera sees every point
    rng2 = np.random.default_rng(5)
    keep = np.zeros((P, n_cams), dtype=bool)
    for j, L in enumerate(lengths):
        # (the front point's cameras come from a stream of their own: the other tracks are the same in both scenes)
        r = np.random.default_rng(99) if (extra_front and j == 0) else rng2
        keep[j, r.choice(n_cams, size=L, replace=False)] = True
    keep = keep.ravel()
    pts0, cams0, uv = full.pts0.copy(), full.cams0.copy(), full.uv
    if extra_front:                      # points 1.. of this scene are points 0.. of the plain one, seen from the same cameras
        plain = synth.make_scene(n_cams, P - 1, obs_per_point=None, seed=21, cam_sigma=0.005)
        assert np.array_equal(plain.cams_true, full.cams_true)      # (the front point's pixels come from these)
        cams0 = plain.cams0.copy()
        pts0[1:] = plain.pts0
        uv = full.uv.copy().reshape(P, n_cams, 2)
        uv[1:] = plain.uv.reshape(P - 1, n_cams, 2)
        uv = uv.reshape(-1, 2)
    return n_cams, P, full.cam_idx[keep].copy(), full.pt_idx[keep].copy(), uv[keep].copy(), cams0, pts0


def _problem(name, d, extra_front=False):
    from oracle import ba_oracle as bo
    from sfm_amd import synth
    n_cams, P, ci, pi, uv, cams0, pts0 = _scene(name, extra_front)
    prob = bo.BAProblem(n_cams, P, d, ci, pi, uv, np.array(synth.K_REF))
    x0 = np.concatenate([cams0[:, :d].ravel(), pts0.ravel()])
    return prob, x0


def _backend(prob, x0, precision):
    from sfm_amd.ba import GpuBA
    C_, d = prob.n_cams, prob.d
    return GpuBA(x0[:C_ * d].reshape(C_, d), x0[C_ * d:].reshape(-1, 3), prob.cam_idx, prob.pt_idx, prob.uv, prob.K0,
                 prob.width, prob.height, precision=precision)


@functools.lru_cache(maxsize=None)
def _oracle_lin(name, d):
    from oracle import ba_oracle as bo
    prob, x0 = _problem(name, d)
    return bo.linearize(x0, prob)


def _ws(be, off, shape, dtype=None):
    cnt = int(np.prod(shape))
    return be.view(off, cnt, dtype).cpu().numpy().reshape(shape)


def _records(be, N, d):
    """(Jc~ [N,2,d], Jp~ [N,2,3], f~ [N,2]) as stored, widened to float64."""
    recA = _ws(be, be.lay.rec_off, (N, 2, d), be.rec_dtype).astype(np.float64)
    recB = _ws(be, be.lay.recB_off, (N, 8), be.rec_dtype).astype(np.float64)
    return recA, recB[:, :6].reshape(N, 2, 3), recB[:, 6:8]


def _ftilde(f):
    return np.where(f * f <= 1.0, f, np.sign(f) / SQRT_EPS)


def _linearize_outputs(be, prob):
    """Everything sfm_ba_linearize / sfm_ba_finish_linearize leave, as bytes-comparable arrays."""
    N, C_, d, P, lay = prob.n_obs, prob.n_cams, prob.d, prob.n_pts, be.lay
    sc = np.array(be.linearize())
    return dict(sc=sc, recA=_ws(be, lay.rec_off, (N * 2 * d,), be.rec_dtype), recB=_ws(be, lay.recB_off, (N * 8,), be.rec_dtype),
                B=_ws(be, lay.B_off, (C_, d, d)), gc=_ws(be, lay.gc_off, (C_ * d,)), Cp=_ws(be, lay.Cp_off, (P, 6)),
                gp=_ws(be, lay.gp_off, (P, 3)), red=_ws(be, lay.reduce_lin_off, (lay.reduce_lin_count,)), gmax=_ws(be, lay.gmax_off, (2,)))


IU = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", SCENES)
def test_linearize_matches_oracle(gpu_ready, name, d, precision):
    prob, x0 = _problem(name, d)
    lin = _oracle_lin(name, d)
    N, C_, P = prob.n_obs, prob.n_cams, prob.n_pts
    be = _backend(prob, x0, precision)
    out = _linearize_outputs(be, prob)
    cost, gnorm, ginf, hdiag = out["sc"]
    Jc, Jp, ft = _records(be, N, d)
    scale = lambda a: max(1.0, np.max(np.abs(a)))
    ft_ref = _ftilde(lin.f[:2 * N]).reshape(N, 2)
    if precision == "fp64":
        assert np.max(np.abs(Jc - lin.Jc)) <= 1e-11 * scale(lin.Jc)
        assert np.max(np.abs(Jp - lin.Jp)) <= 1e-11 * scale(lin.Jp)
        assert np.max(np.abs(ft - ft_ref) / np.maximum(1.0, np.abs(ft_ref))) <= 1e-11
        B_ref, g_ref = lin.B, lin.g
        C_ref = np.stack([lin.Cp[:, i, j] for i, j in IU], axis=1)
    else:
        # float32 records: round-to-nearest of values that agree with the oracle's to 1e-11 of the largest entry
        u = 2.0 ** -24
        assert np.all(np.abs(Jc - lin.Jc) <= u * np.abs(lin.Jc) + 1e-11 * scale(lin.Jc))
        assert np.all(np.abs(Jp - lin.Jp) <= u * np.abs(lin.Jp) + 1e-11 * scale(lin.Jp))
        assert np.all(np.abs(ft - ft_ref) <= u * np.abs(ft_ref) + 1e-11 * np.maximum(1.0, np.abs(ft_ref)))
        # the blocks are float64 sums over what was stored
        B_ref = np.zeros((C_, d, d)); g_c = np.zeros((C_, d)); Cp3 = np.zeros((P, 3, 3)); g_p = np.zeros((P, 3))
        np.add.at(B_ref, prob.cam_idx, np.einsum("nri,nrj->nij", Jc, Jc))
        np.add.at(g_c, prob.cam_idx, np.einsum("nr,nrd->nd", ft, Jc))
        np.add.at(Cp3, prob.pt_idx, np.einsum("nri,nrj->nij", Jp, Jp))
        np.add.at(g_p, prob.pt_idx, np.einsum("nr,nrd->nd", ft, Jp))
        if d == 10:
            freg = lin.f[2 * N:].reshape(C_, 4)
            B_ref[:, 6:10, 6:10] += np.einsum("cri,crj->cij", lin.Jreg, lin.Jreg)
            g_c[:, 6:10] += np.einsum("cr,crj->cj", _ftilde(freg), lin.Jreg)
        g_ref = np.concatenate([g_c.ravel(), g_p.ravel()])
        C_ref = np.stack([Cp3[:, i, j] for i, j in IU], axis=1)
    n = C_ * d
    assert np.max(np.abs(out["B"] - B_ref)) <= 1e-11 * scale(B_ref)
    assert np.max(np.abs(out["gc"] - g_ref[:n])) <= 1e-11 * scale(g_ref)
    assert np.max(np.abs(out["Cp"] - C_ref)) <= 1e-11 * scale(C_ref)
    assert np.max(np.abs(out["gp"].ravel() - g_ref[n:])) <= 1e-11 * scale(g_ref)
    assert cost == pytest.approx(lin.cost, rel=1e-12)                      # the cost never passes through float32
    assert gnorm == pytest.approx(np.linalg.norm(g_ref), rel=1e-11)
    assert ginf == pytest.approx(np.max(np.abs(g_ref)), rel=1e-11)
    assert hdiag == pytest.approx(max(np.max(np.einsum('cii->ci', B_ref)), np.max(C_ref[:, [0, 3, 5]])), rel=1e-11)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", SCENES)
def test_point_blocks_do_not_depend_on_where_a_track_lies(gpu_ready, name, d, precision):
    """One 3-observation point in front moves every other track by 3 observations against the multiples of 256: tracks that lay
    inside a workgroup of the observation pass now cross a boundary and the other way round.  The blocks of the common points
    must not notice - whichever kernel forms a track's blocks, and from whichever side of a boundary."""
    prob_a, x_a = _problem(name, d)
    prob_b, x_b = _problem(name, d, extra_front=True)
    assert prob_b.n_obs == prob_a.n_obs + 3 and prob_b.n_pts == prob_a.n_pts + 1
    assert np.array_equal(prob_b.cam_idx[3:], prob_a.cam_idx) and np.array_equal(prob_b.uv[3:], prob_a.uv)
    ptr_a = np.concatenate([[0], np.cumsum(np.bincount(prob_a.pt_idx, minlength=prob_a.n_pts))])
    inside = lambda ptr: (ptr[:-1] // 256) == ((ptr[1:] - 1) // 256)
    moved = inside(ptr_a) != inside(ptr_a + 3)
    if prob_a.n_obs > 256:
        assert moved.any()                       # some track changes sides
    out_a = _linearize_outputs(_backend(prob_a, x_a, precision), prob_a)
    out_b = _linearize_outputs(_backend(prob_b, x_b, precision), prob_b)
    assert np.array_equal(out_b["recB"][24:], out_a["recB"])
    assert np.array_equal(out_b["Cp"][1:], out_a["Cp"])
    assert np.array_equal(out_b["gp"][1:], out_a["gp"])


def _fill_step(be, prob, seed):
    """A step in pc / pp without a damped solve: the trial step only reads it."""
    import torch
    rng = np.random.default_rng(seed)
    n, P = prob.n_cams * prob.d, prob.n_pts
    pc = rng.normal(0.0, 1e-3, size=n)
    pp = rng.normal(0.0, 1e-2, size=3 * P)
    be.view(be.lay.pc_off, n).copy_(torch.from_numpy(pc))
    be.view(be.lay.pp_off, 3 * P).copy_(torch.from_numpy(pp))
    return pc, pp


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", SCENES)
def test_trial_step(gpu_ready, name, d, precision):
    prob, x0 = _problem(name, d)
    lin = _oracle_lin(name, d)
    N, C_ = prob.n_obs, prob.n_cams
    be = _backend(prob, x0, precision)
    be.linearize()
    pc, pp = _fill_step(be, prob, seed=3)
    scale = 0.37
    js2, gts, cost_new, snorm, xnorm = be.step(scale)
    # the fused pass against the unfused one: k_cost_obs at the same x_new, same grouping of the sums
    assert cost_new == be.cost(be.x_new)
    Jc, Jp, ft = _records(be, N, d)
    t = scale * (np.einsum("nrd,nd->nr", Jp, pp.reshape(-1, 3)[prob.pt_idx]) + np.einsum("nrd,nd->nr", Jc, pc.reshape(C_, d)[prob.cam_idx]))
    js2_ref, gts_ref = float(np.sum(t * t)), float(np.sum(ft * t))
    if d == 10:
        tr = scale * np.einsum("crj,cj->cr", lin.Jreg, pc.reshape(C_, d)[:, 6:10])
        js2_ref += float(np.sum(tr * tr))
        gts_ref += float(np.sum(_ftilde(lin.f[2 * N:].reshape(C_, 4)) * tr))
    s = scale * np.concatenate([pc, pp])
    assert js2 == pytest.approx(js2_ref, rel=1e-8)
    assert gts == pytest.approx(gts_ref, rel=1e-8)
    assert snorm == pytest.approx(np.linalg.norm(s), rel=1e-9)
    assert xnorm == pytest.approx(np.linalg.norm(x0 + s), rel=1e-10)
    from oracle import ba_oracle as bo
    assert cost_new == pytest.approx(bo.huber_cost(bo.residuals(x0 + s, prob)), rel=1e-9)
    assert np.max(np.abs(be.x_new.cpu().numpy() - (x0 + s))) <= 1e-15 * max(1.0, np.max(np.abs(x0)))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("name", SCENES)
def test_stages_are_reproducible(gpu_ready, name, d, precision):
    prob, x0 = _problem(name, d)
    be = _backend(prob, x0, precision)

    def run():
        out = _linearize_outputs(be, prob)
        _fill_step(be, prob, seed=4)
        out["step"] = np.array(be.step(0.61))
        out["red_step"] = _ws(be, be.lay.reduce_step_off, (5,))
        out["x_new"] = be.x_new.cpu().numpy()
        out["cost_at_x_new"] = np.array([be.cost(be.x_new)])
        return out

    a, b = run(), run()
    for key in a:
        assert np.array_equal(a[key], b[key]), key


def test_library_loop_leaves_the_iterate_in_the_callers_buffer(gpu_ready):
    """After every outer iteration of the loop inside the library the caller's buffer is the iterate - the cost at it is the
    cost the loop reports - and the whole run is the run of the Python loop, which swaps its two buffers instead of copying."""
    from sfm_amd.trf import trf
    prob, x0 = _problem("ragged", 10)
    be = _backend(prob, x0, "fp64")
    kw = dict(max_nfev=10 ** 6, max_outer=4, check_tolerances=False)       # a fixed schedule: four outer iterations
    st = be.trf_begin(**kw)
    try:
        costs = []
        while st.outer():
            costs.append((st.result().cost, be.cost()))
        res = st.result()
    finally:
        st.close()
    assert len(costs) >= 2 and all(at_x == pytest.approx(c, rel=1e-13) for c, at_x in costs)
    x_lib = be.x.cpu().numpy()
    be2 = _backend(prob, x0, "fp64")
    ref = trf(be2, **kw)
    assert (res.nfev, res.njev, res.status) == (ref.nfev, ref.njev, ref.status)
    assert np.array_equal(x_lib, be2.x.cpu().numpy())
