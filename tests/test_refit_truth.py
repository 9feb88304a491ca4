"""CPU tests of tests/refit_truth.py: the NumPy references' refits and fr.hartley against the 60-digit truth at C_REF,
the preconditions under which the device is judged (test_refit_truth_gpu.py), and mutation checks of the judge itself.
measure_c() prints the constants that stand in refit_truth.C_REF:  python tests/test_refit_truth.py"""
import functools

import numpy as np
import pytest

import refit_truth as rt

KEPT = {stage: [s for s, g in enumerate(rt.segments(stage)) if g.kind == "kept"] for stage in rt.STAGES}


@functools.lru_cache(maxsize=None)
def case(stage, s):
    """(winner model, mask, count, T6, truth over the winner's mask, the reference's refit, LM steps) of a kept
    segment - computed once, never modified."""
    seg = rt.segments(stage)[s]
    model, mask, count, T6 = rt.reference_winner(stage, s)
    assert model is not None and count >= rt.GATE[stage], (stage, seg.name, count)
    tr = rt.truth(stage, s, mask, model if stage == "pnp" else (T6 if T6 is not None else ()))
    got, steps = rt.reference_refit(stage, seg, mask, T6, model)
    return model, mask, count, T6, tr, got, steps


def hartley_ratios():
    """(stage, segment, ratio) of fr.hartley (rt.hartley6) on every segment of the two 9-model stages with two finite
    matches or more - the segments whose T the device test judges."""
    return [(stage, s, rt.hartley_ratio(rt.hartley6(*g.data), rt.truth_hartley(g)))
            for stage in ("fundamental", "homography") for s, g in enumerate(rt.segments(stage))
            if g.kind in ("kept", "dropped", "short", "seven")]


def test_hartley_reference_holds_c_ref():
    worst = max(h for _, _, h in hartley_ratios())
    print(f"hartley: worst reference ratio {worst:.4g} against C_REF {rt.C_REF['hartley']:.4g}")
    assert worst <= rt.C_REF["hartley"]


def measure_c():
    out = {"hartley": 0.0}
    for stage in rt.STAGES:
        worst, secs = 0.0, 0.0
        for s in KEPT[stage]:
            seg = rt.segments(stage)[s]
            model, mask, count, T6, tr, got, steps = case(stage, s)
            r = rt.ratios(stage, got, tr)
            k = int(np.argmin(r))
            worst, secs = max(worst, r[k]), secs + tr.seconds
            line = f"{stage:12s} {seg.name:24s} have {count:4d} roots {len(r)} kappa {tr.kappa[k]:9.3g} ratio {r[k]:9.3g} s {tr.seconds:5.1f}"
            if steps is not None:
                line += f" LM steps {steps}"
            print(line, flush=True)
        out[stage] = worst
        print(f"{stage}: C_REF {worst:.4g}, bound {rt.MARGIN * worst:.4g}, truth {secs:.1f} CPU s", flush=True)
    for stage, s, h in hartley_ratios():
        out["hartley"] = max(out["hartley"], h)
        print(f"hartley      {stage:12s} {rt.segments(stage)[s].name:30s} ratio {h:9.3g}", flush=True)
    up = lambda v: float(np.ceil(v / 10.0 ** (np.floor(np.log10(v)) - 3)) * 10.0 ** (np.floor(np.log10(v)) - 3))
    print({k: float(f"{up(v):.4g}") for k, v in out.items()})              # rounded up at four digits
    for stage in rt.STAGES:
        print(stage, "dropped seed", rt.find_dropped(stage), flush=True)


@pytest.mark.parametrize("stage", rt.STAGES)
def test_references_hold_c_ref(stage):
    """fr.refit, hr.refit, er.refit and pr.lm_refit lie within 1 x C_REF of the truth on every kept segment; the LM replay
    stops by its step rule, not at its cap."""
    worst, fails = 0.0, []
    for s in KEPT[stage]:
        seg = rt.segments(stage)[s]
        model, mask, count, T6, tr, got, steps = case(stage, s)
        r = float(rt.ratios(stage, got, tr).min())
        worst = max(worst, r)
        if not r <= rt.C_REF[stage]:
            fails.append(f"{seg.name}: ratio {r:.4g}")
        if steps is not None and not steps < rt.pr.LM_ITERS:
            fails.append(f"{seg.name}: the LM replay ran into its cap")
    print(f"{stage}: worst reference ratio {worst:.4g} against C_REF {rt.C_REF[stage]:.4g}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("stage", rt.STAGES)
def test_preconditions(stage):
    """On every kept segment: the truth's refit counts at least the winner's inliers (so a correct device refit is
    kept); no match lies within 1e-9 of threshold^2 for the truth's model or the winner; the device's bound stays under
    LEFT_OUT.  The reference's own refit is kept too.  A scene that fails is replaced in refit_truth.RESEED, not skipped."""
    for s in KEPT[stage]:
        seg = rt.segments(stage)[s]
        model, mask, count, T6, tr, got, steps = case(stage, s)
        counts = rt.root_counts(stage, tr, seg)
        assert counts.max() >= count, (seg.name, counts, count)
        assert int(rt.rule_mask(stage, got, seg).sum()) >= count, seg.name
        assert not rt.band(stage, model, seg, 1e-9).any(), seg.name
        for root in tr.roots[counts >= count]:
            assert not rt.band(stage, root.astype(np.float64), seg, 1e-9).any(), seg.name
        k = int(np.argmax(counts))                                        # E: the root that is judged is the best by count
        assert rt.MARGIN * rt.C_REF[stage] * tr.unit[k] <= rt.LEFT_OUT, (seg.name, tr.kappa[k])
    if rt.DROPPED_SEED[stage] is not None:
        s = next(i for i, g in enumerate(rt.segments(stage)) if g.kind == "dropped")
        seg = rt.segments(stage)[s]
        model, mask, count, T6 = rt.reference_winner(stage, s)
        got, _ = rt.reference_refit(stage, seg, mask, T6, model)
        assert int(rt.rule_mask(stage, got, seg).sum()) < count
        assert not rt.band(stage, got, seg, 1e-6).any() and not rt.band(stage, model, seg, 1e-6).any()


def test_dropped_seeds_are_the_first():
    for stage in rt.STAGES:
        assert rt.find_dropped(stage) == rt.DROPPED_SEED[stage], stage


def rejected(stage, model, tr):
    """True if the device's bound turns the model down against every root."""
    return bool((rt.ratios(stage, model, tr) > rt.MARGIN * rt.C_REF[stage]).all())


@pytest.mark.parametrize("stage", rt.STAGES)
def test_the_judge_rejects_mutated_models(stage):
    """Subtly wrong refits, made on the truth's side, fail the DEVICE's bound on every kept segment: one mask bit flipped;
    T1 and T2 exchanged in the de-normalisation; the second-smallest eigenvector (for E: the fifth eigenvector in place of
    the fourth); no rank-2 step; a PnP pose one LM step from the winner."""
    for s in KEPT[stage]:
        seg = rt.segments(stage)[s]
        model, mask, count, T6, tr, got, steps = case(stage, s)
        flipped = np.array(mask, bool)
        k = int(np.flatnonzero(flipped)[-1])
        flipped[k] = False
        mutants = {}
        if stage in ("fundamental", "homography"):
            solve = lambda m=mask, **kw: [float(x) for x in rt.truth_model9(stage, seg, m, T6, **kw).roots_mp[0]]
            mutants["mask bit"] = solve(m=flipped, pick=0)
            mutants["T1 and T2 exchanged"] = solve(swap=True)
            mutants["second eigenvector"] = solve(pick=1)
            if stage == "fundamental":
                mutants["no rank-2 step"] = solve(rank2=False)
        elif stage == "essential":
            best = tr.roots[int(np.argmax(rt.root_counts(stage, tr, seg)))]
            others = {"mask bit": rt.truth_essential(seg, flipped, condition=False),
                      "fifth eigenvector": rt.truth_essential(seg, mask, shift=1)}
            for name, other in others.items():
                d = rt.distances(stage, best.astype(np.float64), other)
                mutants[name] = other.roots[int(np.argmin(d))].astype(np.float64)
        else:
            Rt = np.asarray(model).reshape(3, 4)
            K = rt.pr.k_matrix(seg.k4)
            a, b = rt._f64(seg.data)
            R1, t1, _ = rt.pr.lm_refit(K, Rt[:, :3], Rt[:, 3], a[mask], b[mask], max_steps=1)
            mutants["one LM step"] = np.c_[R1, t1].ravel()
            R2, t2, _ = rt.pr.lm_refit(K, Rt[:, :3], Rt[:, 3], a[flipped], b[flipped])
            mutants["mask bit"] = np.c_[R2, t2].ravel()
        for name, m in mutants.items():
            assert rejected(stage, m, tr), (seg.name, name, rt.ratios(stage, m, tr))


def test_hartley_edges_of_the_reference():
    seg = {g.kind: g for g in rt.segments("fundamental")}
    assert rt.hartley6(*seg["nonfinite"].data).tolist() == [1, 0, 0, 1, 0, 0]
    T = rt.hartley6(*seg["one"].data)
    a, b = seg["one"].data
    assert T.tolist() == [1.0, float(a[4, 0]), float(a[4, 1]), 1.0, float(b[4, 0]), float(b[4, 1])]


if __name__ == "__main__":
    measure_c()
