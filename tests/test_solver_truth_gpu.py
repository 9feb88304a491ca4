"""GPU tests of the MODELS the four batched RANSAC stages compute, against the multi-precision truth of
tests/solver_truth.py.  One call per stage through the C ABI (refine = 0) with a workspace of the test's own, filled with
0xFF beforehand; the models of every hypothesis are then read out of the workspace:

    essential                   cand_E [n_seg H][10][9] float64 at 0, then cand_n [n_seg H] int32
    fundamental, homography     T [n_seg][6] float64, then hyp_model [n_seg H][9]
    pnp                         cand_Rt [n_seg H][4][12] float64 at 0

The segments are the scenes of solver_truth.scenes() in order, then one segment below the minimal size and one whose
match 0 holds a NaN.  H = 65 for the essential stage (workgroups of 64 over the flat (segment, hypothesis) index straddle
the segments and the last one is partial; 25 hypotheses per scoring workgroup) and 257 for the 256-lane kernels.  The
Hartley transforms T are only read here; they, and the refits that follow the models, are judged in
tests/test_refit_truth_gpu.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import homography_reference as hr
import ransac_reference
import solver_truth as st

pytestmark = pytest.mark.gpu

THR = {"fundamental": 3.0, "homography": 3.0, "essential": 3.0, "pnp": 8.0}
ENTRY = {"fundamental": "fund", "homography": "hom", "essential": "ess", "pnp": "pnp"}


def segments(solver):
    """The scenes' data, then a short segment and a NaN segment cut from scene 1: [(arrays, k4)]."""
    sc = st.scenes(solver)
    size, least = st.SAMPLE[solver]
    out = [(s.data, s.k4) for s in sc]
    out.append((tuple(a[:least - 1].copy() for a in sc[1].data), sc[1].k4))
    bad = tuple(a[:least + 1].copy() for a in sc[1].data)
    bad[1][0, 0] = np.nan
    out.append((bad, sc[1].k4))
    return out


@functools.lru_cache(maxsize=None)
def run(solver, call):
    """One sfm_*_ransac call over all segments (`call` only tells two runs apart).  Returns (samples [n_seg, H, size],
    hyp_count [n_seg, H], the workspace's model bytes as the arrays named above) - computed once, never modified."""
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    segs = segments(solver)
    size, least = st.SAMPLE[solver]
    H, n_seg = st.N_HYP[solver], len(segs)
    lens = [len(d[0]) for d, _ in segs]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(ptr[-1])
    smp = np.stack([ransac_reference.draw_samples(st.SEED, s, m, H, size, least) for s, m in enumerate(lens)])
    for s in range(len(st.scenes(solver))):
        assert np.array_equal(smp[s], st.samples(solver, s))
    live = smp[np.array(lens) >= least]
    assert smp.min() >= -1 and all((smp[s] < m).all() for s, m in enumerate(lens)) and live.min() >= 0
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(a).astype(dt))).to(dev)
    first = to([d[0] for d, _ in segs], np.float64 if solver == "pnp" else np.float32)
    second = to([d[1] for d, _ in segs], np.float32)
    k4 = torch.tensor([k for _, k in segs], dtype=torch.float64, device=dev)
    seg, d_smp = torch.from_numpy(ptr).to(dev), torch.from_numpy(smp).to(dev)
    width = 12 if solver == "pnp" else 9
    model = torch.empty((n_seg, width), dtype=torch.float64, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    meta = torch.empty((3, n_seg), dtype=torch.int32, device=dev)
    counts = torch.empty((n_seg, H), dtype=torch.int32, device=dev)
    need = C.c_int64()
    assert getattr(h.lib, f"sfm_{ENTRY[solver]}_workspace_bytes")(n, n_seg, H, C.byref(need)) == 0
    ws = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=dev)
    fn = getattr(h.lib, f"sfm_{ENTRY[solver]}_ransac")
    head = (h._h, _p(seg), n_seg, _p(first), _p(second), n)
    tail = (_p(d_smp), H, C.c_double(THR[solver]), 0, _p(model), _p(mask), _p(meta[0]), _p(meta[1]), _p(counts), _p(meta[2]),
            _p(ws), need.value)
    rc = fn(*head, *tail) if solver in ("fundamental", "homography") else fn(*head, _p(k4), *tail)
    assert rc == 0, h.lib.sfm_last_error(h._h)
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    g = n_seg * H
    if solver == "essential":
        off = st.ws_regions(need.value, (g * 90, 8), (g, 4), (g, 4), (g, 4))
        out = {"cand_E": raw[off[0]:off[0] + g * 720].view(np.float64).reshape(n_seg, H, 10, 9),
               "cand_n": raw[off[1]:off[1] + g * 4].view(np.int32).reshape(n_seg, H)}
    elif solver == "pnp":
        off = st.ws_regions(need.value, (g * 48, 8), (g, 4), (g, 4))
        out = {"cand_Rt": raw[off[0]:off[0] + g * 384].view(np.float64).reshape(n_seg, H, 4, 12)}
    else:
        off = st.ws_regions(need.value, (n_seg * 6, 8), (g * 9, 8), (g, 4))
        out = {"T": raw[off[0]:off[0] + n_seg * 48].view(np.float64).reshape(n_seg, 6),
               "hyp_model": raw[off[1]:off[1] + g * 72].view(np.float64).reshape(n_seg, H, 9)}
    return smp, counts.cpu().numpy(), out


def candidates(solver, out, s, h):
    """The models hypothesis h of segment s left in the workspace, [m, D]."""
    if solver == "essential":
        nc = int(out["cand_n"][s, h])
        assert 0 <= nc <= 10
        return out["cand_E"][s, h, :nc]                                    # slots at or past cand_n: undefined, not read
    if solver == "pnp":
        slots = out["cand_Rt"][s, h]
        assert np.isfinite(slots).all()
        return slots[(slots != 0).any(1)]                                  # the filled slots are the non-zero ones
    m = out["hyp_model"][s, h]
    assert np.isfinite(m).all()
    return m[None][:int((m != 0).any())]


@pytest.mark.parametrize("solver", ["fundamental", "homography", "essential", "pnp"])
def test_device_models_against_the_truth(gpu_ready, solver):
    """Every judged hypothesis passes the judge at 8 x C_REF: all roots once and nothing else for the essential and P3P
    candidates; for the fundamental and homography stages the stored best model matches a root, and the count of that
    root, recomputed in NumPy, equals hyp_count wherever the hypothesis is stable.  In the degenerate scenes a model is a
    root or polishes onto one.  Where the sample rule gives no model, in the short segment and in every hypothesis of the
    NaN segment that drew match 0, the slot holds "no model"."""
    smp, counts, out = run(solver, 0)
    tr, _ = st.truth(solver)
    C_dev = st.MARGIN * st.C_REF[solver]
    scenes = st.scenes(solver)
    fails, worst = [], {}
    for s, sc in enumerate(scenes):
        hyps = st.JUDGED[solver]
        if solver == "homography":
            stable = dict(zip(hyps, hr.stable(sc.data[0], sc.data[1], smp[s][hyps], THR[solver])))
        for h in hyps:
            c, sample, idx = candidates(solver, out, s, h), tr[s, h], smp[s, h]
            if solver in ("essential", "pnp") or st.voided(solver, sc, idx):
                f, ratios = st.sample_failures(solver, c, sample, sc, idx, C_dev)
            elif len(c) == 0:
                f, ratios = ([] if sc.degenerate or sample.undetermined else ["no model stored"]), []
            else:
                ok = stable[h] if solver == "homography" else st.count_is_stable(solver, sample, sc, THR[solver])
                f, ratios = st.best_model_failures(solver, c[0], int(counts[s, h]), sample, sc, C_dev, THR[solver], bool(ok))
            fails += [f"{sc.name}, hypothesis {h}: {x}" for x in f]
            worst[sc.name] = max([worst.get(sc.name, 0.0)] + list(ratios))
    print(f"{solver}, device: worst error / (kappa 2^-53) {max(worst.values()):.3g} against the bound {C_dev:.4g}; per scene "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    short, nan = len(scenes), len(scenes) + 1
    assert (smp[short] == -1).all() and (counts[short] == 0).all()
    drew = (smp[nan] == 0).any(1)
    assert drew.any() and (counts[nan][drew] == 0).all()
    for s, hyps in ((short, range(st.N_HYP[solver])), (nan, np.flatnonzero(drew))):
        for h in hyps:
            if len(candidates(solver, out, s, h)):
                fails.append(f"segment {s}, hypothesis {h}: a model where there is none")
            if solver != "essential":
                key = "cand_Rt" if solver == "pnp" else "hyp_model"
                assert (out[key][s, h] == 0).all(), (s, h)                 # zeros, not just "no non-zero slot"
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("solver", ["fundamental", "homography", "essential", "pnp"])
def test_two_calls_leave_identical_models(gpu_ready, solver):
    """A second call into a second workspace: the judged regions hold the same bytes."""
    _, ca, a = run(solver, 0)
    _, cb, b = run(solver, 1)
    assert ca.tobytes() == cb.tobytes()
    for s in range(len(st.scenes(solver))):
        for h in st.JUDGED[solver]:
            assert candidates(solver, a, s, h).tobytes() == candidates(solver, b, s, h).tobytes(), (s, h)
    if solver != "essential":
        key = "cand_Rt" if solver == "pnp" else "hyp_model"
        assert a[key].tobytes() == b[key].tobytes()
