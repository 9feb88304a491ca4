"""GPU tests of the REFITS of the four batched RANSAC stages and of the Hartley transforms, against the 60-digit truth of
tests/refit_truth.py.  Per stage two calls through the C ABI over the segments of refit_truth.segments(stage), with the
same samples and a workspace filled with 0xFF beforehand: refine = 0, then refine = 1.  Each stage is referenced from the
device's own inputs to it: the refit's truth is computed over the MASK of the refine = 0 call (and, for PnP, seeded from
its pose), with the T read out of the workspace for F and H; T itself is judged against the truth of the pixels."""
import ctypes as C
import functools

import numpy as np
import pytest

import refit_truth as rt
from test_solver_truth_gpu import ENTRY, THR

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def run(stage, refine, only=None):
    """One sfm_*_ransac call over all segments, or over segment `only` alone with the samples it has in the batch.
    Returns a dict of host arrays: model [n_seg, W], mask (list per segment), n_inliers, status, refined, and T [n_seg, 6]
    for F and H - computed once, never modified."""
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    ids = list(range(len(rt.segments(stage)))) if only is None else [only]
    segs = [rt.segments(stage)[s] for s in ids]
    size, least = rt.SAMPLE[stage]
    H, n_seg = rt.N_HYP, len(segs)
    lens = [g.n for g in segs]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(ptr[-1])
    smp = np.stack([rt.samples(stage, s) for s in ids])
    assert smp.min() >= -1 and all((smp[k] < m).all() for k, m in enumerate(lens))
    to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.concatenate(a).astype(dt))).to(dev)
    first = to([g.data[0] for g in segs], np.float64 if stage == "pnp" else np.float32)
    second = to([g.data[1] for g in segs], np.float32)
    k4 = torch.tensor([g.k4 for g in segs], dtype=torch.float64, device=dev)
    seg, d_smp = torch.from_numpy(ptr).to(dev), torch.from_numpy(smp).to(dev)
    width = 12 if stage == "pnp" else 9
    model = torch.empty((n_seg, width), dtype=torch.float64, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    meta = torch.full((3, n_seg), -7, dtype=torch.int32, device=dev)
    counts = torch.empty((n_seg, H), dtype=torch.int32, device=dev)
    need = C.c_int64()
    assert getattr(h.lib, f"sfm_{ENTRY[stage]}_workspace_bytes")(n, n_seg, H, C.byref(need)) == 0
    ws = torch.full((need.value,), 0xFF, dtype=torch.uint8, device=dev)
    fn = getattr(h.lib, f"sfm_{ENTRY[stage]}_ransac")
    head = (h._h, _p(seg), n_seg, _p(first), _p(second), n)
    tail = (_p(d_smp), H, C.c_double(THR[stage]), int(refine), _p(model), _p(mask), _p(meta[0]), _p(meta[1]), _p(counts),
            _p(meta[2]), _p(ws), need.value)
    rc = fn(*head, *tail) if stage in ("fundamental", "homography") else fn(*head, _p(k4), *tail)
    assert rc == 0, h.lib.sfm_last_error(h._h)
    torch.cuda.synchronize()
    m = mask.cpu().numpy()
    meta = meta.cpu().numpy()
    out = {"model": model.cpu().numpy(), "mask": [m[ptr[k]:ptr[k + 1]] for k in range(n_seg)], "n_inliers": meta[0],
           "status": meta[1], "refined": meta[2]}
    if stage in ("fundamental", "homography"):
        g = n_seg * H
        off = rt.ws_regions(need.value, (n_seg * 6, 8), (g * 9, 8), (g, 4))
        out["T"] = ws.cpu().numpy()[off[0]:off[0] + n_seg * 48].view(np.float64).reshape(n_seg, 6).copy()
    return out


def kinds(stage, *which):
    return [s for s, g in enumerate(rt.segments(stage)) if g.kind in which]


@pytest.mark.parametrize("stage", ["fundamental", "homography"])
def test_hartley_transforms_against_the_truth(gpu_ready, stage):
    """T of every segment with two finite matches or more lies within 8 x C_REF["hartley"] of the truth; the edge segments
    are exact; the refine = 1 call leaves the same bytes."""
    T = run(stage, 0)["T"]
    assert T.tobytes() == run(stage, 1)["T"].tobytes()
    bound = rt.MARGIN * rt.C_REF["hartley"]
    worst = 0.0
    for s in kinds(stage, "kept", "dropped", "short", "seven"):
        seg = rt.segments(stage)[s]
        r = rt.hartley_ratio(T[s], rt.truth_hartley(seg))
        worst = max(worst, r)
        assert r <= bound, (seg.name, r, bound)
    print(f"{stage}, hartley: worst error / (kappa 2^-53) {worst:.3g} against the bound {bound:.4g}")
    (s,) = kinds(stage, "nonfinite")
    assert T[s].tolist() == [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    (s,) = kinds(stage, "one")
    a, b = rt.segments(stage)[s].data
    fin = np.flatnonzero(np.isfinite(a).all(1) & np.isfinite(b).all(1))
    assert len(fin) == 1
    k = int(fin[0])
    assert T[s].tolist() == [1.0, float(a[k, 0]), float(a[k, 1]), 1.0, float(b[k, 0]), float(b[k, 1])]


@pytest.mark.parametrize("stage", rt.STAGES)
def test_refits_against_the_truth(gpu_ready, stage):
    """On every kept segment the refit is kept (refined == 1) and its model lies within 8 x C_REF of the truth over the
    refine = 0 call's mask; for E, within the bound of a truth root whose count, recomputed in NumPy, equals n_inliers,
    and no truth root counts more (where no root's count changes between threshold (1 -+ 1e-3)).  n_inliers and the mask
    are the NumPy rule of the returned model outside 1e-9 of threshold^2; F[2][2] = H[2][2] = 1 exactly; F has rank 2."""
    r0, r1 = run(stage, 0), run(stage, 1)
    bound = rt.MARGIN * rt.C_REF[stage]
    fails, worst = [], {}
    for s in kinds(stage, "kept"):
        seg = rt.segments(stage)[s]
        mask0, have = r0["mask"][s].astype(bool), int(r0["n_inliers"][s])
        assert r0["status"][s] == 0 and r0["refined"][s] == 0 and have == mask0.sum() and have >= rt.GATE[stage], seg.name
        assert not rt.band(stage, r0["model"][s], seg, 1e-9).any(), seg.name      # the preconditions, on the device's own mask
        extra = r0["T"][s] if "T" in r0 else (r0["model"][s] if stage == "pnp" else ())
        tr = rt.truth(stage, s, mask0, extra)
        counts = rt.root_counts(stage, tr, seg)
        top = int(np.argmax(counts))
        assert counts[top] >= have and bound * tr.unit[top] <= rt.LEFT_OUT, (seg.name, counts, have, tr.kappa)
        assert not rt.band(stage, tr.roots[top].astype(np.float64), seg, 1e-9).any(), seg.name
        model, got = r1["model"][s], int(r1["n_inliers"][s])
        if r1["status"][s] != 0 or r1["refined"][s] != 1:
            fails.append(f"{seg.name}: status {r1['status'][s]}, refined {r1['refined'][s]}")
            continue
        ratio = rt.ratios(stage, model, tr)
        k = int(np.argmin(ratio))
        worst[seg.name] = float(ratio[k])
        if not ratio[k] <= bound:
            fails.append(f"{seg.name}: {ratio[k]:.4g} x unit from the nearest root (kappa {tr.kappa[k]:.3g}), bound {bound:.4g}")
        if stage == "essential" and (counts == rt.root_counts(stage, tr, seg, 1 - 1e-3)).all() and \
                (counts == rt.root_counts(stage, tr, seg, 1 + 1e-3)).all():
            if counts[k] != got:
                fails.append(f"{seg.name}: n_inliers {got}, but the matched root counts {counts[k]}")
            if counts.max() > got:
                fails.append(f"{seg.name}: n_inliers {got}, but a truth root counts {counts.max()}")
        rule, near = rt.rule_mask(stage, model, seg), rt.band(stage, model, seg, 1e-9)
        m1 = r1["mask"][s].astype(bool)
        assert got == m1.sum() and got >= have, seg.name
        if not (m1 == rule)[~near].all() or not rule[~near].sum() <= got <= rule[~near].sum() + near.sum():
            fails.append(f"{seg.name}: the mask is not the rule of the returned model")
        if stage in ("fundamental", "homography") and model[8] != 1.0:
            fails.append(f"{seg.name}: model[2][2] = {model[8]!r}")
        if stage == "fundamental":
            sv = np.linalg.svd(model.reshape(3, 3), compute_uv=False)
            if not sv[2] <= 1e-12 * sv[0]:
                fails.append(f"{seg.name}: singular values {sv}")
    print(f"{stage}, device refit: worst error / unit {max(worst.values(), default=0.0):.3g} against the bound {bound:.4g}; per segment "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("stage", rt.STAGES)
def test_segments_without_a_refit_keep_the_winner(gpu_ready, stage):
    """The segment whose refit loses, the short one, the edge segments and F's M = 7: refined == 0, and model, mask and
    count are the bytes of the refine = 0 call."""
    r0, r1 = run(stage, 0), run(stage, 1)
    (short,) = kinds(stage, "short")
    assert r1["status"][short] == 1
    for s in kinds(stage, "dropped"):
        assert r1["status"][s] == 0 and r0["n_inliers"][s] >= rt.GATE[stage]
    for s in kinds(stage, "seven"):
        assert r1["status"][s] == 0 and r0["n_inliers"][s] == 7
    for s in kinds(stage, "dropped", "short", "nonfinite", "one", "seven"):
        name = rt.segments(stage)[s].name
        assert r1["refined"][s] == 0 and r0["refined"][s] == 0, name
        assert r1["status"][s] == r0["status"][s] and r1["n_inliers"][s] == r0["n_inliers"][s], name
        assert r1["model"][s].tobytes() == r0["model"][s].tobytes(), name
        assert r1["mask"][s].tobytes() == r0["mask"][s].tobytes(), name


@pytest.mark.parametrize("stage", rt.STAGES)
def test_one_segment_alone_has_the_bytes_of_the_batch(gpu_ready, stage):
    s = next(i for i, g in enumerate(rt.segments(stage)) if g.kind == "kept" and g.n == 257)
    batch, alone = run(stage, 1), run(stage, 1, s)
    assert alone["model"][0].tobytes() == batch["model"][s].tobytes()
    assert alone["mask"][0].tobytes() == batch["mask"][s].tobytes()
    assert (alone["n_inliers"][0], alone["status"][0], alone["refined"][0]) == \
        (batch["n_inliers"][s], batch["status"][s], batch["refined"][s])
    if "T" in batch:
        assert alone["T"][0].tobytes() == batch["T"][s].tobytes()
