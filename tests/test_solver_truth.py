"""CPU tests of the minimal solvers' MODELS against the multi-precision truth of tests/solver_truth.py: the truth against
itself, the share of roots the judge leaves out, the NumPy references at 1 x C_REF, the host builds of the four
*_solve.h headers (tests/native/*_solve_check.cpp, once by g++ -ffp-contract=off as the other host checks are, once by
-ffp-contract=fast -mfma as a stand-in for the device's contraction) at 8 x C_REF, and nine seeded defects that the
judge must reject.  No GPU."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import solver_truth as st
from solver_truth import mpf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVERS = ["fundamental", "homography", "essential", "pnp"]
THR = {"fundamental": 3.0, "homography": 3.0, "essential": 3.0, "pnp": 8.0}
MODES = {"off": ("-ffp-contract=off",), "fast": ("-ffp-contract=fast", "-mfma")}
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


# ------------------------------------------------------------------------------------ the truth against itself
def _exact_scene(planar):
    """Points, R (cos 12/13), t and K as exact rationals; the pixels of both views at 60 digits, nothing rounded to a
    float.  planar: the points lie on n . X = d."""
    rng = np.random.default_rng(3)
    X = rng.uniform(-1, 1, (7, 3)) + [0, 0, 6.0]
    n, d = [mpf("0.25"), mpf("0.125"), mpf(1)], mpf(6)
    Xm = [[mpf(float(v)) for v in p] for p in X]
    if planar:
        Xm = [[p[0], p[1], (d - n[0] * p[0] - n[1] * p[1]) / n[2]] for p in Xm]
    c, s = mpf(12) / 13, mpf(5) / 13
    R = [[c, mpf(0), s], [mpf(0), mpf(1), mpf(0)], [-s, mpf(0), c]]
    t = [mpf("-1.5"), mpf("0.125"), mpf("0.25")]
    fx, fy, cx, cy = (mpf(v) for v in (1228, 1100, 512, 384))
    px = []
    for p in Xm:
        q = [st._dot(R[r], p) + t[r] for r in range(3)]
        px.append([fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy, fx * q[0] / q[2] + cx, fy * q[1] / q[2] + cy])
    tx = [[mpf(0), -t[2], t[1]], [t[2], mpf(0), -t[0]], [-t[1], t[0], mpf(0)]]
    E = [[st._dot(tx[i], [R[k][j] for k in range(3)]) for j in range(3)] for i in range(3)]
    Ki = [[1 / fx, mpf(0), -cx / fx], [mpf(0), 1 / fy, -cy / fy], [mpf(0), mpf(0), mpf(1)]]
    K = [[fx, mpf(0), cx], [mpf(0), fy, cy], [mpf(0), mpf(0), mpf(1)]]
    mul = lambda A, B: [[st._dot(A[i], [B[k][j] for k in range(3)]) for j in range(3)] for i in range(3)]
    T = lambda A: [[A[j][i] for j in range(3)] for i in range(3)]
    F = mul(mul(T(Ki), E), Ki)
    Hm = mul(mul(K, [[R[i][j] + t[i] * n[j] / d for j in range(3)] for i in range(3)]), Ki)
    flat = lambda A: [v for r in A for v in r]
    return Xm, px, (fx, fy, cx, cy), flat(E), flat(F), flat(Hm), [v for r in range(3) for v in R[r] + [t[r]]]


def test_the_true_model_is_among_the_roots_of_a_noise_free_sample():
    """Inputs carried at 60 digits, so the scene is noise-free to 1e-60: the true F, H, E and [R|t] lie within 1e-30 of
    a root of their sample's truth."""
    Xm, px, k4, E, F, _, Rt = _exact_scene(False)
    obj = lambda rows: np.array(rows, dtype=object)
    got = {"fundamental": min(st._sine(r, F) for r in st.truth_fundamental(obj(px[:7])).roots_mp),
           "essential": min(st._sine(r, E) for r in st.truth_essential(obj(px[:5]), k4).roots_mp)}
    s = st.truth_pnp(obj(Xm[:3]), obj([p[2:] for p in px[:3]]), k4)
    got["pnp"] = min(st._rt_distance(r, Rt, mpf(s.extent)) for r in s.roots_mp)
    _, px, _, _, _, Hm, _ = _exact_scene(True)
    got["homography"] = min(st._sine(r, Hm) for r in st.truth_homography(obj(px[:4])).roots_mp)
    for solver, d in got.items():
        print(f"{solver}: the true model lies {float(d):.1e} from a root")
        assert d < mpf("1e-30"), solver


@pytest.mark.parametrize("solver", SOLVERS)
def test_truth_residuals_root_counts_and_left_out_caps(solver):
    """Every root's defining equations hold to 1e-40; at most 3, 1, 10 and 4 roots; under 8 x C_REF at most 2 % of the
    roots of the solver's whole sample set are left out, and at most 10 % in any scene but the degenerate ones."""
    tr, secs = st.truth(solver)
    worst = max(float(s.residual) for s in tr.values())
    most = max(len(s.roots) for s in tr.values())
    total, per = st.left_out_shares(solver, st.MARGIN * st.C_REF[solver])
    n = sum(len(s.roots) for s in tr.values())
    print(f"{solver}: {len(tr)} samples, {n} roots, at most {most} per sample, largest residual {worst:.1e}, truth in {secs:.1f} "
          f"CPU seconds; left out under {st.MARGIN:g} x C_REF: {total:.2%} overall, per scene "
          + ", ".join(f"{k} {v:.1%}" for k, v in per.items()))
    assert worst < 1e-40 and most <= st.ROOT_CAP[solver]
    assert secs < 30.0
    assert total <= 0.02
    for sc in st.scenes(solver):
        assert sc.degenerate or per[sc.name] <= 0.10, sc.name


# ------------------------------------------------------------------------------------------ candidate sets
def judged(solver):
    """[(segment, scene, hypothesis, sample indices)] of the solver's sample set."""
    return [(s, sc, h, st.samples(solver, s)[h]) for s, sc in enumerate(st.scenes(solver)) for h in st.JUDGED[solver]]


@functools.lru_cache(maxsize=None)
def reference_sets(solver):
    return {(s, h): st.reference_candidates(solver, sc, idx) for s, sc, h, idx in judged(solver)}


def check_sets(solver, sets, C, what, degenerate_too=True):
    """sample_failures over the whole sample set; returns the worst ratio error / (kappa 2^-53) per scene."""
    tr, _ = st.truth(solver)
    fails, worst = [], {}
    for s, sc, h, idx in judged(solver):
        if sc.degenerate and not degenerate_too:
            continue
        f, ratios = st.sample_failures(solver, sets[s, h], tr[s, h], sc, idx, C)
        fails += [f"{sc.name}, hypothesis {h}: {x}" for x in f]
        worst[sc.name] = max([worst.get(sc.name, 0.0)] + list(ratios))
    print(f"{solver}, {what}: worst error / (kappa 2^-53) {max(worst.values()):.3g} against the bound {C:.4g}; per scene "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert not fails, "\n".join(fails[:20])
    return worst


@pytest.mark.parametrize("solver", SOLVERS)
def test_numpy_references_define_c(solver):
    """C re-measured - the worst error / (kappa 2^-53) of the NumPy reference over the roots that C leaves in, the
    degenerate scenes aside - has not drifted above the recorded C_REF, and the references pass the judge at 1 x C_REF
    (outside the degenerate scenes, where nothing is asked of them)."""
    tr, _ = st.truth(solver)
    pairs = []
    for s, sc, h, idx in judged(solver):
        if sc.degenerate or st.voided(solver, sc, idx) or tr[s, h].undetermined:
            continue
        d = st.distances(solver, reference_sets(solver)[s, h], tr[s, h])
        pairs += [(tr[s, h].kappa[k], d[:, k].min() if d.shape[0] else np.inf) for k in range(d.shape[1])]
    C = st.measure_c(pairs)
    print(f"{solver}: C measured {C:.4g} over {len(pairs)} roots, recorded {st.C_REF[solver]:.4g}")
    assert C is not None and C <= st.C_REF[solver]
    check_sets(solver, reference_sets(solver), st.C_REF[solver], "NumPy reference", degenerate_too=False)


# ---------------------------------------------------------------------------------------- the host builds
@pytest.fixture(scope="module")
def native_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("solver_truth_native"))


def build_native(tmp, solver, mode):
    exe = os.path.join(tmp, f"{solver}_solve_check_{mode}")
    if not os.path.exists(exe):
        subprocess.run(["g++", "-std=c++17", "-O2", *MODES[mode], "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", f"{solver}_solve_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, tag, data, width):
    path = f"{exe}.{tag}"
    np.asarray(data, np.float64).tofile(path + ".in")
    subprocess.run([exe, path + ".in", path + ".out"], check=True)
    return np.fromfile(path + ".out").reshape(-1, width)


@functools.lru_cache(maxsize=None)
def host_sets(tmp, solver, mode):
    """({(segment, hypothesis): candidates [m, D]}, {(segment, hypothesis): their inlier counts or None}) of the header
    built for the host - computed once per build, never modified."""
    exe = build_native(tmp, solver, mode)
    sets, counts = {}, {}
    for s, sc in enumerate(st.scenes(solver)):
        hyps = st.JUDGED[solver]
        smp = st.samples(solver, s)[hyps]
        if solver in ("fundamental", "homography"):
            p1, p2 = (np.asarray(p, np.float64) for p in sc.data)
            T1, T2 = st.hartley_pair(sc)
            t = [T1[0, 0], -T1[0, 2] / T1[0, 0], -T1[1, 2] / T1[0, 0], T2[0, 0], -T2[0, 2] / T2[0, 0], -T2[1, 2] / T2[0, 0]]
            head = np.concatenate([[len(p1), len(smp), THR[solver]], t, np.c_[p1, p2].ravel(), smp.astype(np.float64).ravel()])
            if solver == "fundamental":
                o = _run(exe, s, head, 33)
                for h, row in zip(hyps, o):
                    keep = row[:3] != 0
                    sets[s, h], counts[s, h] = row[3:30].reshape(3, 9)[keep], row[30:][keep].astype(int)
            else:
                o = _run(exe, s, head, 11)
                for h, row in zip(hyps, o):
                    sets[s, h], counts[s, h] = row[1:10].reshape(1, 9)[:int(row[0] != 0)], row[10:].astype(int)[:int(row[0] != 0)]
        elif solver == "essential":
            px = np.c_[sc.data[0][smp].astype(np.float64), sc.data[1][smp].astype(np.float64)].reshape(len(smp), 20)
            o = _run(exe, s, np.c_[px, np.tile(sc.k4, (len(smp), 1))], 91)
            for h, row in zip(hyps, o):
                sets[s, h], counts[s, h] = row[1:].reshape(10, 9)[:int(row[0])], None
        else:
            fx, fy, cx, cy = sc.k4
            uv = sc.data[1][smp].astype(np.float64)                       # the bearings as k_pnp_hypotheses forms them
            bx, by = (uv[..., 0] - cx) / fx, (uv[..., 1] - cy) / fy
            inv = 1.0 / np.sqrt(bx * bx + by * by + 1.0)
            f = np.stack([bx * inv, by * inv, inv], -1)
            o = _run(exe, s, np.c_[sc.data[0][smp].reshape(len(smp), 9), f.reshape(len(smp), 9)], 49)
            for h, row in zip(hyps, o):
                slots = row[1:].reshape(4, 12)
                filled = np.array([(int(row[0]) >> c) & 1 for c in range(4)], bool)
                assert np.array_equal(filled, (slots != 0).any(1)), (sc.name, h)   # the filled slots are the non-zero ones
                sets[s, h], counts[s, h] = slots[filled], None
    return sets, counts


@needs_gxx
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("solver", SOLVERS)
def test_host_builds_of_the_headers(native_dir, solver, mode):
    """The header built for the host, without and with contraction to fma: every sample passes the judge at 8 x C_REF;
    in the degenerate scenes every model is a root or polishes onto one."""
    sets, _ = host_sets(native_dir, solver, mode)
    check_sets(solver, sets, st.MARGIN * st.C_REF[solver], f"host build, -ffp-contract={mode}")


# ------------------------------------------------------------------------------------------ seeded defects
def _pick(solver, sets, need):
    """The first sample of a scene that is not degenerate whose candidate set passes the judge and meets `need`."""
    tr, _ = st.truth(solver)
    C = st.MARGIN * st.C_REF[solver]
    for s, sc, h, idx in judged(solver):
        smp, c = tr[s, h], sets[s, h]
        if sc.degenerate or smp.undetermined or st.voided(solver, sc, idx) or len(c) == 0:
            continue
        if (C * smp.kappa * st.U53 > 1e-10).any() or st.sample_failures(solver, c, smp, sc, idx, C)[0]:
            continue
        if need(smp, c):
            return s, sc, h, idx, smp, np.array(c)
    raise AssertionError("no sample to seed the defect into")


@needs_gxx
def test_seeded_defects_are_rejected(native_dir):
    """Nine defects written into candidate arrays of the host builds (samples whose every bound is below 1e-10): the
    judge rejects each."""
    rejected = {}

    def seeded(name, solver, cands, pick):
        s, sc, h, idx, smp, _ = pick
        fails, _ = st.sample_failures(solver, cands, smp, sc, idx, st.MARGIN * st.C_REF[solver])
        rejected[name] = fails

    ess, _ = host_sets(native_dir, "essential", "off")
    pick = _pick("essential", ess, lambda smp, c: 2 <= len(c) < 10)
    c = pick[5]
    seeded("one root dropped", "essential", c[1:], pick)
    seeded("one root duplicated into a free slot", "essential", np.r_[c, c[:1]], pick)
    moved = c.copy()
    moved[0] += 1e-9 * np.linalg.norm(c[0]) * np.roll(c[0], 1) / np.linalg.norm(c[0])
    seeded("a candidate moved by 1e-9", "essential", moved, pick)
    seeded("E transposed", "essential", c.reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9), pick)

    # the stored best of the fundamental stage: the three candidates and their counts stand in for the device's slot
    fund, cnt = host_sets(native_dir, "fundamental", "off")
    tr, _ = st.truth("fundamental")
    for s, sc, h, idx in judged("fundamental"):
        c, n = fund[s, h], cnt[s, h]
        if sc.degenerate or len(c) < 2 or n.max() == n.min() or not st.count_is_stable("fundamental", tr[s, h], sc, 3.0):
            continue
        best, other = int(np.argmax(n)), int(np.argmin(n))
        C = st.MARGIN * st.C_REF["fundamental"]
        assert not st.best_model_failures("fundamental", c[best], int(n[best]), tr[s, h], sc, C, 3.0, True)[0]
        rejected["F of the other cubic root stored as the best"] = \
            st.best_model_failures("fundamental", c[other], int(n[best]), tr[s, h], sc, C, 3.0, True)[0]
        break

    pnp, _ = host_sets(native_dir, "pnp", "off")
    pick = _pick("pnp", pnp, lambda smp, c: len(c) < 4)
    c = pick[5]
    neg = c.copy()
    neg[0, 3::4] *= -1.0
    seeded("[R|t] with t negated", "pnp", neg, pick)
    mirror = (np.diag([1.0, 1.0, -1.0]) @ c[0].reshape(3, 4)).reshape(1, 12)
    seeded("a 4th P3P slot filled with a mirror solution", "pnp", np.r_[c, mirror], pick)
    # polish removed: a Newton step squares the error, so one step back from 1e-16 is 1e-8.  The depths of candidate 0
    # are set back by that much (relative, in float64) and the pose is formed from them as the truth forms it.
    P, uv, k4 = st.sample_inputs("pnp", pick[1], pick[3])
    _, _, f = st._p3p_problem(st._mp(P.ravel()), st._mp(uv.ravel()), st._mp(k4))
    depth = [float(st._norm([st._dot(st._mp(c[0][4 * r:4 * r + 3]), st._mp(P[i])) + mpf(float(c[0][4 * r + 3])) for r in range(3)]))
             for i in range(3)]
    back = [mpf(l * (1 + sg * 1e-8)) for l, sg in zip(depth, (1, -1, 1))]
    unpolished = c.copy()
    unpolished[0] = [float(v) for v in st._p3p_pose(st._mp(P.ravel()), f, back)]
    seeded("polish removed (one Newton step back)", "pnp", unpolished, pick)

    hom, _ = host_sets(native_dir, "homography", "off")
    tr, _ = st.truth("homography")
    s, sc, h, idx = next(j for j in judged("homography") if st.voided("homography", j[1], j[3]))
    assert len(hom[s, h]) == 0                                             # the header gives none there
    rejected['a model written into a "no model" slot'] = st.sample_failures(
        "homography", tr[s, h].roots.astype(np.float64), tr[s, h], sc, idx, st.MARGIN * st.C_REF["homography"])[0]

    for name, fails in rejected.items():
        print(f"{name}: {fails[0] if fails else 'NOT REJECTED'}")
    assert len(rejected) == 9 and all(rejected.values())
