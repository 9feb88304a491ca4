"""CPU self-tests of tests/dense_reference.py: the float64 transcription of the dense solver's algebra stays inside every judge
on every case of the grid (this is where the recorded constants come from), the matrix families are what they claim, with_pivot
puts the first non-positive pivot exactly where it is asked to, and seeded defects break the judges.  No GPU."""
import numpy as np
import pytest

import dense_reference as dr
import stage_reference as sr

_cache = {}


def transcribed(fam, n, strips):
    """The bordered system of the case through the float64 transcription: the regions and the four solves on both routes."""
    key = (fam, n, strips)
    if key not in _cache:
        A, r, b = dr.family(fam, n)
        F = dr.factor_f64(A, r, strips)
        x = {(tr, flow): dr.solve_f64(F, b, tr, flow) for tr in (0, 1) for flow in (True, False)}
        _cache[key] = (A, r, b, F, x)
    return _cache[key]


def raw_ratios(fam, n, strips):
    """{judge: (ratio without its constant, where)} of the transcription."""
    A, r, b, F, x = transcribed(fam, n, strips)
    assert F["flag"] == 0
    out = {"factor": dr.judge_factor(A, F["Lm"]), "row": dr.judge_row(F["Lm"], r)}
    assert dr.judge_lmt(F["Lm"], F["LmT"]) == []
    ri, wi, problems = dr.judge_inverses(F["Lm"], F["Dinv"], F["DinvT"])
    assert problems == []
    out["inverses"] = (ri, wi)
    out["solve"] = max((dr.judge_solve(F["Lm"], b, x[tr, flow], tr) + ((tr, flow),) for tr in (0, 1) for flow in (True, False)),
                       key=lambda t: t[0])
    const = {"factor": dr.C_FACTOR, "row": dr.C_ROW, "inverses": dr.C_INV, "solve": dr.C_SOLVE}
    return {k: (v[0] * const[k],) + tuple(v[1:]) for k, v in out.items()}


RECORD = {"factor": dr.M_FACTOR, "row": dr.M_ROW, "inverses": dr.M_INV, "solve": dr.M_SOLVE}


@pytest.mark.parametrize("fam,n,strips", dr.GRID)
def test_float64_transcription_stays_inside_every_judge(fam, n, strips):
    """Every case factors in 80 bits and in the transcription without a non-positive pivot; no judge's ratio exceeds its record by
    more than 2 % (the constants are 8 x these records: a transcription beyond one means the record is stale); the product's
    composition passes stage_reference's own judges of the factorisation route."""
    A, r, b, F, x = transcribed(fam, n, strips)
    assert dr.first_bad_pivot(A) is None
    for k, v in raw_ratios(fam, n, strips).items():
        print(f"{fam} n={n} {'strips' if strips else 'one-level'} {k}: raw ratio {v[0]:.3g} (record {RECORD[k]:.3g}) at {v[1:]}")
        assert v[0] <= 1.02 * RECORD[k], (k, v)
    pc = dr.solve_f64(F, -F["Lm"][n], 1)
    ratio, where, rig = dr.judge_end_to_end(A, r, pc)
    print(f"{fam} n={n} end to end: {ratio:.3g} of C_FACT's bound at {where}, {rig:.3g} of the rigorous bound")
    assert ratio <= 1.0 and rig <= 1.0


@pytest.mark.parametrize("judge,case", [("factor", ("well", 1, False)), ("row", ("floor", 33, False)),
                                        ("inverses", ("well", 193, False)), ("solve", ("well", 1, False))])
def test_recorded_constants_are_attained_by_the_case_they_name(judge, case):
    got = raw_ratios(*case)[judge][0]
    print(judge, case, got)
    assert 0.98 * RECORD[judge] <= got <= 1.02 * RECORD[judge]


# ---------------------------------------------------------------------------------------------- the families
@pytest.mark.parametrize("n", sorted(set(dr.HARD_ONE_LEVEL_N + dr.HARD_STRIP_N)))
def test_floor_family_has_the_condition_number_it_claims(n):
    A, _, _ = dr.family("floor", n)
    w = np.linalg.eigvalsh(A)
    print(n, "kappa2", w[-1] / w[0])
    assert w[0] > 0 and abs(w[-1] / w[0] / dr.floor_kappa(n) - 1) <= 0.01
    assert np.array_equal(A, A.T)


@pytest.mark.parametrize("n", [33, 300])
def test_graded_family_is_an_exact_scaling(n):
    """kappa2 about 1e12, and the scaling by powers of two commutes with every rounding: the transcription's factor of the
    graded matrix is D times that of the matrix under it, bit for bit, so the componentwise judges cannot move."""
    A, r, _ = dr.family("graded", n)
    rng = np.random.default_rng(1000 * dr.FAMILIES.index("graded") + n)
    G = rng.normal(size=(n, n)); rng.normal(size=(2, n))
    D = 2.0 ** -rng.integers(0, 21, size=n).astype(np.float64)
    A0 = G @ G.T + n * np.eye(n); A0 = np.tril(A0) + np.tril(A0, -1).T
    assert np.array_equal(A, D[:, None] * A0 * D[None, :])
    kappa = np.linalg.cond(A)
    print(n, "kappa2", kappa)
    assert 1e10 <= kappa <= 1e14
    F, F0 = dr.factor_f64(A, r), dr.factor_f64(A0, r / D)
    assert np.array_equal(np.tril(F["Lm"][:n]), D[:, None] * np.tril(F0["Lm"][:n]))
    assert dr.judge_factor(A, F["Lm"])[0] == dr.judge_factor(A0, F0["Lm"])[0]


@pytest.mark.parametrize("n,strips", [(130, False), (330, True)])
def test_with_pivot_fails_first_at_exactly_k(n, strips):
    A, r, _ = dr.family("well", n)
    L80 = sr.chol_lower(A)
    for k in [k for (n_, s_, k) in dr.PIVOT_GRID if (n_, s_) == (n, strips)]:
        bad = dr.with_pivot(A, k, -1, L80)
        assert dr.first_bad_pivot(bad) == k and dr.first_bad_pivot(bad, np.float64) == k
        Lb = np.tril(bad.astype(dr.LD))
        piv = Lb[k, k] - np.sum(L80[k, :k] ** 2)
        # the pivot is minus the one it replaces, which is no small part of the diagonal entry: no rounding makes it positive
        assert piv <= -0.99 * L80[k, k] ** 2 and L80[k, k] ** 2 >= 0.1 * A[k, k]
        with np.errstate(all="ignore"):                                          # what follows a substituted pivot is garbage
            assert dr.factor_f64(bad, r, strips)["flag"] == 1
        ok = dr.with_pivot(A, k, 0.5, L80)
        assert dr.first_bad_pivot(ok) is None
        F = dr.factor_f64(ok, r, strips)
        assert F["flag"] == 0 and dr.judge_factor(ok, F["Lm"])[0] <= 1.0 / 8
    for k in (40, 100):                                                          # a zero and a NaN pivot
        for v in (0.0, np.nan):
            E = np.eye(n); E[k, k] = v
            with np.errstate(all="ignore"):
                assert dr.first_bad_pivot(E) == k and dr.factor_f64(E, None, strips)["flag"] == 1


# ---------------------------------------------------------------------------------------------- the judges can see
def test_seeded_defects_break_the_judges():
    """A good transcription result with one defect each: the judge that owns it goes to at least 100 x its bound, or the bitwise
    check breaks."""
    fam, n, strips = "well", 193, False
    A, r, b, F, x = transcribed(fam, n, strips)
    Lm = F["Lm"]

    bad = Lm.copy(); bad[70, 70] *= 1 + 1e-9                       # one factor entry, 1e-9 relative
    ratio, where = dr.judge_factor(A, bad)
    print("factor entry:", ratio, where)
    assert ratio >= 100 and "[70][70]" in where

    k = int(np.argmax(np.abs(Lm[n])))                              # one entry of row n likewise
    bad = Lm.copy(); bad[n, k] *= 1 + 1e-9
    ratio, where = dr.judge_row(bad, r)
    print("bordered row entry:", ratio, where)
    assert ratio >= 100 and dr.judge_row(Lm, r)[0] <= 1.0 / 8

    bad = F["LmT"].copy(); bad[64:128, 128:192] = 1.25             # one 64 x 64 block of LmT left at stale values
    problems = dr.judge_lmt(Lm, bad)
    print("stale LmT block:", problems)
    assert problems and "64-block (2, 1)" in problems[0]
    bad = F["LmT"].copy(); bad[0, 64] = np.nextafter(bad[0, 64], 1.0)     # ... and a single last bit
    assert dr.judge_lmt(Lm, bad)
    bad = F["LmT"].copy(); bad[0, 63] = 0.0; bad[64, 127] = 0.0           # just outside the judged set: never written
    assert dr.judge_lmt(Lm, bad) == []

    inv64 = F["inv64"].copy()                                      # Li21 of one block with the wrong sign
    dr.fix_inv64(Lm, inv64, n, only=1)
    Dinv, DinvT = dr.merge_inverses(Lm, inv64, n)
    ratio, where, problems = dr.judge_inverses(Lm, Dinv, DinvT)
    print("Li21 sign:", ratio, where)
    assert ratio >= 100 and "128-block 0" in where and problems == []

    bad = F["DinvT"].copy(); bad[1, 3, 40] = F["Dinv"][1, 3, 40]   # one entry of DinvT not transposed
    assert F["Dinv"][1, 40, 3] != 0
    ratio, where, problems = dr.judge_inverses(Lm, F["Dinv"], bad)
    print("DinvT entry:", problems)
    assert problems and "DinvT[1][3][40]" in problems[0]

    bad = F["Dinv"].copy(); bad[1, 100, 100] = 2.0                 # beyond n = 193 the block is the identity
    assert any("identity beyond n" in p for p in dr.judge_inverses(Lm, bad, np.transpose(bad, (0, 2, 1)))[2])
    bad = F["Dinv"].copy(); bad[0, 3, 9] = 1e-300
    assert any("above its diagonal" in p for p in dr.judge_inverses(Lm, bad, np.transpose(bad, (0, 2, 1)))[2])

    for tr in (0, 1):                                              # one solved entry changed
        for flow in (True, False):
            xb = x[tr, flow].copy(); xb[n // 2] *= 1 + 1e-9
            ratio, where = dr.judge_solve(Lm, b, xb, tr)
            print("solved entry:", tr, flow, ratio, where)
            assert ratio >= 100

    # a forward solve that reads a stale LmT block is seen by the forward judge of the flow route only
    Fb = dict(F); Fb["LmT"] = F["LmT"].copy(); Fb["LmT"][0:64, 128:192] *= 1 + 1e-9
    assert dr.judge_solve(Lm, b, dr.solve_f64(Fb, b, 0, True), 0)[0] >= 100
    assert np.array_equal(dr.solve_f64(Fb, b, 0, False), x[0, False])
    # the end-to-end judge sees a step that is off in one entry
    pc = dr.solve_f64(F, -Lm[n], 1); pc[5] *= 1 + 1e-9
    assert dr.judge_end_to_end(A, r, pc)[0] >= 100
