"""CPU self-tests of tests/model_reference.py: the scenes hold the edges they were built for, the series rotation checks itself,
the float64 transcription (oracle.ba_oracle) stays inside every bound on every scene - this is where the recorded constants come
from - and seeded defects break the bounds at the right place.  No GPU."""
import numpy as np
import pytest

import model_reference as mr

LD = mr.LD
_cache = {}


def problem(sc, d):
    from oracle import ba_oracle as bo
    return bo.BAProblem(sc.C, sc.P, d, sc.cam_idx, sc.pt_idx, sc.uv, np.array(sc.K), sc.width, sc.height, sc.reg_weight)


def scene(variant):
    if ("scene", variant) not in _cache:
        from sfm_amd.structure import build_structure
        sc = mr.model_scene(variant)
        _cache[("scene", variant)] = (sc, build_structure(sc.cam_idx, sc.pt_idx, sc.C, sc.P))
    return _cache[("scene", variant)]


def transcribe(sc, d, x=None):
    """The oracle at x: unscaled rows and f (jacobian_blocks), the Huber-scaled rows (linearize) with f~ as huber_row states it."""
    from oracle import ba_oracle as bo
    prob = problem(sc, d)
    x = sc.x0(d) if x is None else x
    f, Jc, Jp, _ = bo.jacobian_blocks(x, prob)
    lin = bo.linearize(x, prob)
    N = prob.n_obs
    fo = f[:2 * N].reshape(N, 2)
    ft = np.where(np.abs(fo) <= 1.0, fo, np.sign(fo) * mr.HUBER_FT)
    return dict(x=x, prob=prob, lin=lin, f=fo, Jc=Jc, Jp=Jp, Jcs=lin.Jc, Jps=lin.Jp, ft=ft)


def host(variant, d):
    if (variant, d) not in _cache:
        _cache[(variant, d)] = transcribe(scene(variant)[0], d)
    return _cache[(variant, d)]


def sums_f64(sc, d, x, Jc, Jp, ft, obs_mask=None, fx_of_row1=None, reg_cams=None):
    """The sums in float64 from the given rows (np.add.at: one observation after the other), the regulariser rows in float64."""
    reg = None
    if mr._apply_reg(sc, d):
        _, Jr, fr, _ = mr.reg_rows(mr.split_x(x, sc.C, d)[0], sc, np.float64)
        if fx_of_row1 is not None:
            bad = mr.reg_rows(mr.split_x(x, sc.C, d)[0], sc, np.float64, fx_of_row1=fx_of_row1)[1]
            Jr[reg_cams] = bad[reg_cams]
        reg = (Jr, fr)
    return mr.stage_sums(Jc, Jp, ft, sc.cam_idx, sc.pt_idx, sc.C, sc.P, np.float64, reg=reg, obs_mask=obs_mask)


def seeded_step(sc, d, seed=3):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1e-3, size=sc.C * d), rng.normal(0.0, 1e-3, size=sc.P * 3)


def step_f64(sc, d, T, pc, pp, scale, with_reg=True):
    from oracle import ba_oracle as bo
    x = T["x"]
    x_new = x + scale * np.concatenate([pc, pp])
    t = scale * (np.einsum("nra,na->nr", T["Jcs"], pc.reshape(sc.C, d)[sc.cam_idx]) + np.einsum("nra,na->nr", T["Jps"], pp.reshape(sc.P, 3)[sc.pt_idx]))
    js2, gts = float(np.sum(t * t)), float(np.sum(T["ft"] * t))
    if with_reg and mr._apply_reg(sc, d):
        _, Jr, fr, _ = mr.reg_rows(mr.split_x(x, sc.C, d)[0], sc, np.float64)
        tr = scale * np.einsum("cra,ca->cr", Jr, pc.reshape(sc.C, d)[:, 6:])
        js2 += float(np.sum(tr * tr)); gts += float(np.sum(fr * tr))
    s = scale * np.concatenate([pc, pp])
    return x_new, dict(JS2=js2, GTS=gts, COST_NEW=bo.huber_cost(bo.residuals(x_new, T["prob"])), SNORM2=float(np.sum(s * s)),
                       XNEW_NORM2=float(np.sum(x_new * x_new)))


def reproj_f64(sc, d, x, shared_k):
    from oracle import ba_oracle as bo
    x = np.array(x, dtype=np.float64)
    if d == 10 and shared_k:
        x[:sc.C * d].reshape(sc.C, d)[:, 6:] = sc.K
    f = bo.residuals(x, problem(sc, d))[:2 * sc.cam_idx.shape[0]].reshape(-1, 2)
    err = np.sqrt(f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1])
    return err, float(np.sum(err * err))


# ---------------------------------------------------------------------------------------------- scenes and the reference's self-checks
@pytest.mark.parametrize("variant", mr.VARIANTS)
def test_scene_holds_its_edges(variant):
    sc, st = scene(variant)
    mr.assert_model_edges(sc, st)
    for d in (10, 6):
        ref = mr.model(sc.x0(d), sc, d)
        und = int(np.sum(mr.undecided_rows(ref, sc.exact)))
        print(f"{variant} d={d}: N = {sc.cam_idx.shape[0]}, P = {sc.P}, undecided rows {und}, Huber-linear rows {float(np.mean(np.abs(ref['f']) > 1)):.3f}, "
              f"largest kappa {ref['kappa'].max():.3g}")
        assert und == 0


def test_series_rotation_checks_itself():
    rng = np.random.default_rng(0)
    mags = [0.0, 1e-160, 1e-8, 0.00999, 0.01, 0.01001, 0.09, 0.5, 1.8, np.pi - 1e-3, np.pi + 1e-3, 4.5, 6.2]
    v = rng.normal(size=(len(mags), 3)); v /= np.linalg.norm(v, axis=1)[:, None]
    r = (v * np.array(mags)[:, None]).astype(LD)
    R, dR = mr.rotation_series(r)
    orth = float(np.max(np.abs(np.einsum("cij,ckj->cik", R, R) - np.eye(3, dtype=LD))))
    print("|R R^T - I| <=", orth)
    assert orth <= 6e-18 * 1.5
    # central differences in 80 bits: h = 2^-18 leaves a truncation error of h^2 |R'''| / 6 ~ 2.4e-12 and a rounding error of
    # 1e-17 / h ~ 2.6e-12 (1e-17: the series' own error at |r| = 6.2, measured above): 2e-11 holds both, and no h does much better
    h = LD(2.0) ** -18
    for i in range(3):
        e = np.zeros(3, dtype=LD); e[i] = h
        fd = (mr.rotation_series(r + e)[0] - mr.rotation_series(r - e)[0]) / (2 * h)
        err = float(np.max(np.abs(fd - dR[:, i])))
        print(f"dR/dr_{i} against central differences:", err)
        assert err <= 2e-11
    far = np.array(mags) >= 0.09                      # the closed form's own cancellation is ~ 1e-19 / th2^2 below that
    Rc, dRc = mr.rotation_closed(r[far])
    eR, edR = float(np.max(np.abs(Rc - R[far]))), float(np.max(np.abs(dRc - dR[far])))
    print("against the closed form in 80 bits:", eR, edR)
    assert eR <= 2e-17 and edR <= 2e-15
    assert np.array_equal(R[0], np.eye(3)) and np.array_equal(np.diag(R[1]), np.ones(3))          # rvec = 0 and th2 that underflows


# ---------------------------------------------------------------------------------------------- the transcription inside the bounds
RECORD = {"rotation": mr.C_ROT, "translation": mr.C_TRANS, "intrinsics": mr.C_INTR, "point": mr.C_PT, "f": mr.C_F, "err": mr.C_ERR}


def check(name, ratio, where, limit=1.0):
    print(f"  {name}: {ratio:.3g} of its bound at {where}")
    assert ratio <= limit, (name, ratio, where)


@pytest.mark.parametrize("d", [10, 6])
@pytest.mark.parametrize("variant", mr.VARIANTS)
def test_float64_transcription_stays_inside_every_bound(variant, d):
    sc, st = scene(variant)
    T = host(variant, d)
    x = T["x"]
    # the raw ratios the recorded constants are 8 x of
    raw = mr.measure_rows(x, sc, d, T["Jc"], T["Jp"], T["f"])
    for sk in (True, False):
        err, _ = reproj_f64(sc, d, x, sk)
        ref, b = mr.reproj_reference(x, sc, d, sk)
        ratio = np.abs(err.astype(LD) - ref).astype(np.float64) / (b / mr.C_ERR)
        if ratio.max() >= raw.get("err", (0,))[0]:
            raw["err"] = (float(ratio.max()), int(sc.cam_idx[int(np.argmax(ratio))]), ratio)
    for name, (ratio, cam, per_obs) in raw.items():
        print(f"{variant} d={d} raw {name}: {ratio:.4g} at camera {cam} (|r| = {sc.mags[cam]:.6g}); just above the th2 seam (camera 2): "
              f"{float(np.max(per_obs[sc.cam_idx == 2])):.4g}")
        assert ratio <= 1.02 * RECORD[name] / 8, "the transcription exceeds the recorded ratio: the record is stale"
    for mixed in (False, True):
        cast = (lambda a: a.astype(np.float32).astype(np.float64)) if mixed else (lambda a: a)
        Jc, Jp, ft = cast(T["Jcs"]), cast(T["Jps"]), cast(T["ft"])
        print(f"{variant} d={d} {'mixed' if mixed else 'fp64'}")
        check("rows", *mr.judge_rows(x, sc, d, Jc, Jp, ft, mixed=mixed), limit=1.0 if mixed else 1.02 / 8)      # (mixed: rounding to float32 uses the half ulp up)
        S = sums_f64(sc, d, x, Jc, Jp, ft)
        for name, (ratio, where) in mr.judge_sums(Jc, Jp, ft, x, sc, d, S["B"], S["gc"], S["Cp6"], S["gp"]).items():
            check(name, ratio, where)
        g = np.concatenate([S["gc"].ravel(), S["gp"].ravel()])
        hd = max(np.max(np.einsum("cii->ci", S["B"])), np.max(S["Cp6"][:, [0, 3, 5]]))
        for name, (ratio, where) in mr.judge_lin_scalars(x, sc, d, S["B"], S["gc"], S["Cp6"], S["gp"], T["lin"].cost, float(np.sum(g * g)),
                                                         float(np.max(np.abs(g))), float(hd)).items():
            check(name, ratio, where)
        pc, pp = seeded_step(sc, d)
        for scale in (1.0, -0.37):
            x_new, scal = step_f64(sc, d, dict(T, Jcs=Jc, Jps=Jp, ft=ft), pc, pp, scale)
            for name, (ratio, where) in mr.judge_step(Jc, Jp, ft, x, pc, pp, scale, x_new, scal, sc, d).items():
                check(f"step {scale:g} {name}", ratio, where)
    if True:                                               # the oracle's own B and C_p (linearize) hold the bounds too
        lin = T["lin"]
        Cp6 = np.stack([lin.Cp[:, i, j] for i, j in mr.IU], axis=1)
        res = mr.judge_sums(T["Jcs"], T["Jps"], T["ft"], x, sc, d, lin.B, S["gc"], Cp6, S["gp"])
        check("oracle B", *res["B"]); check("oracle Cp", *res["Cp6"])
    x2 = x + 1e-3 * np.sin(np.arange(x.shape[0]))
    for sk in (True, False):
        err, n2 = reproj_f64(sc, d, x2, sk)
        for name, (ratio, where) in mr.judge_reproj(x2, sc, d, sk, err, n2).items():
            check(f"reproj shared_k={sk} {name}", ratio, where, limit=1.02 / 8 if name == "err" else 1.0)


# ---------------------------------------------------------------------------------------------- seeded defects
def rows_with(sc, d, coeffs, monkeypatch, x=None):
    from oracle import ba_oracle as bo
    with monkeypatch.context() as m:
        m.setattr(bo, "_rod_coeffs", coeffs)
        return transcribe(sc, d, x)


def flagged(ratio, where, *needles):
    print(f"  {ratio:.3g} at {where}")
    assert ratio >= 100 and all(s in where for s in needles), (ratio, where, needles)


@pytest.mark.parametrize("d", [10, 6])
def test_seeded_defects_in_the_rotation_break_the_row_bounds(d, monkeypatch):
    from oracle import ba_oracle as bo
    good = bo._rod_coeffs
    sc, _ = scene("ragged")
    x = sc.x0(d)
    th2 = mr.kernel_th2(sc.cams0[:, :3])

    def b_coefficient(t2):                                 # z / 24 -> z / 25 in the series of b
        a, b, a1, b1 = good(t2)
        return a, np.where(t2 < 1e-4, 0.5 - t2 / 25.0 + t2 * t2 / 720.0, b), a1, b1

    def a1_constant(t2):                                   # a1 = -1/3 -> -0.3333 below the seam only
        a, b, a1, b1 = good(t2)
        return a, b, np.where(t2 < 1e-4, -0.3333 + t2 / 30.0 - t2 * t2 / 840.0, a1), b1

    def long_series(t2):                                   # the series used up to th2 < 1e-2
        z = np.asarray(t2, dtype=np.float64)
        cf = good(np.where(z < 1e-2, 0.0, z))
        sr = (1.0 - z / 6.0 + z * z / 120.0, 0.5 - z / 24.0 + z * z / 720.0, -1.0 / 3.0 + z / 30.0 - z * z / 840.0,
              -1.0 / 12.0 + z / 180.0 - z * z / 6720.0)
        return tuple(np.where(z < 1e-2, s, c) for s, c in zip(sr, cf))

    def no_b1(t2):                                         # dR/dr_i without its b1 term on camera 2, just above the seam
        a, b, a1, b1 = good(t2)
        return a, b, a1, np.where(t2 == th2[2], 0.0, b1)

    for name, fn, cam in (("b coefficient", b_coefficient, 3), ("a1 constant", a1_constant, 3), ("series to 1e-2", long_series, 14),
                          ("dR without b1", no_b1, 2)):
        T = rows_with(sc, d, fn, monkeypatch)
        print(name)
        flagged(*mr.judge_rows(x, sc, d, T["Jcs"], T["Jps"], T["ft"]), f"(camera {cam},")
    T = host("ragged", d)
    from oracle import ba_oracle as bo2
    R = bo2.rotation_and_derivs(sc.cams0[:, :3])[0]
    Pi_s = T["Jcs"][:, :, 3:6]
    print("Jp = Pi R^T")
    flagged(*mr.judge_rows(x, sc, d, T["Jcs"], Pi_s @ np.transpose(R, (0, 2, 1))[sc.cam_idx], T["ft"]), "point (")


@pytest.mark.parametrize("d", [10, 6])
def test_seeded_defects_in_the_huber_rows_break_the_row_bounds(d):
    sc, _ = scene("mixed")
    T = host("mixed", d)
    x = T["x"]
    k = int(np.flatnonzero(np.abs(T["f"][:, 0]) > 1)[5])
    Jp = T["Jps"].copy(); Jp[k, 0] = T["Jp"][k, 0]          # the Huber scale applied to Jc but not to Jp
    print("Jp unscaled")
    flagged(*mr.judge_rows(x, sc, d, T["Jcs"], Jp, T["ft"]), f"observation {k} ", "row 0", "point (")
    k = int(np.flatnonzero((np.abs(T["f"][:, 1]) <= 1) & (np.abs(T["f"][:, 1]) > 0.1))[7])
    ft = T["ft"].copy(); ft[k, 1] = np.float32(ft[k, 1])      # f~ of one inlier row rounded to float32 in fp64 mode
    print("float32 f~")
    flagged(*mr.judge_rows(x, sc, d, T["Jcs"], T["Jps"], ft), f"observation {k} ", "row 1", "f~")
    sc, _ = scene("seam")
    T = host("seam", d)
    k = int(sc.seam_obs[0])
    assert T["f"][k, 1] == 1.0 and T["ft"][k, 1] == 1.0        # the inlier branch takes the exact 1.0
    Jc, Jp, ft = T["Jcs"].copy(), T["Jps"].copy(), T["ft"].copy()
    Jc[k, 1] *= mr.HUBER_SCALE; Jp[k, 1] *= mr.HUBER_SCALE; ft[k, 1] = mr.HUBER_FT        # `<` for `<=` at f = exactly 1
    print("< for <=")
    flagged(*mr.judge_rows(T["x"], sc, d, Jc, Jp, ft), f"observation {k} ", "row 1")
    assert mr.judge_rows(T["x"], sc, d, T["Jcs"], T["Jps"], T["ft"])[0] <= 1


@pytest.mark.parametrize("d", [10, 6])
def test_seeded_defects_in_the_sums_break_their_bounds(d):
    sc, st = scene("reg" if d == 10 else "ragged")
    T = host(sc.variant, d)
    x, Jc, Jp, ft = T["x"], T["Jcs"], T["Jps"], T["ft"]
    inl = np.all(np.abs(T["f"]) <= 1, axis=1)

    def judge(S):
        return mr.judge_sums(Jc, Jp, ft, x, sc, d, S["B"], S["gc"], S["Cp6"], S["gp"])

    def of_camera(c):
        return np.asarray(st.cam_obs[st.cam_ptr[c]:st.cam_ptr[c + 1]])

    for name, c, drop in (("last observation of the 257 camera", 1, of_camera(1)[-1:]), ("9th observation of the 9 camera", 4, of_camera(4)[8:9]),
                          ("one chunk partial of the 513 camera", 0, of_camera(0)[256:512])):
        assert inl[drop].any() and len(of_camera(c)) == {1: 257, 4: 9, 0: 513}[c]
        keep = np.ones(sc.cam_idx.shape[0], dtype=bool); keep[drop] = False
        print(name)
        flagged(*judge(sums_f64(sc, d, x, Jc, Jp, ft, obs_mask=keep))["B"], f"camera {c} (")
    k = int(of_camera(5)[3])
    assert abs(ft[k, 0] - ft[k, 1]) > 1e-3
    sw = ft.copy(); sw[k] = sw[k, ::-1]                    # the two residual rows swapped for one observation in g_c
    S = sums_f64(sc, d, x, Jc, Jp, ft); S["gc"] = sums_f64(sc, d, x, Jc, Jp, sw)["gc"]
    print("rows swapped in g_c")
    flagged(*judge(S)["gc"], "camera 5 (")
    # the mixed contract: the stored rows are float32, B summed from the unrounded float64 rows
    J32, P32, f32 = (a.astype(np.float32).astype(np.float64) for a in (Jc, Jp, ft))
    S64 = sums_f64(sc, d, x, Jc, Jp, ft)
    res = mr.judge_sums(J32, P32, f32, x, sc, d, S64["B"], S64["gc"], S64["Cp6"], S64["gp"])
    print("mixed contract")
    for name in ("B", "gc", "Cp6", "gp"):
        flagged(*res[name])
    if d == 10:                                            # (fy - fx) / fx differentiated with fx0, on camera 3
        print("regulariser row with fx0")
        flagged(*judge(sums_f64(sc, d, x, Jc, Jp, ft, fx_of_row1=sc.K[0], reg_cams=[3]))["B"], "camera 3 (")
        # a camera without observations holds exactly the regulariser block
        good = sums_f64(sc, d, x, Jc, Jp, ft)
        assert not np.any(good["B"][12][:6]) and not np.any(good["B"][12][:, :6]) and np.all(np.diag(good["B"][12])[6:] > 0)
        bad = {k_: v.copy() for k_, v in good.items()}; bad["B"][12, 0, 0] = 1e-300
        assert judge(bad)["B"][0] == mr.INF
    else:
        assert not np.any(S64["B"][12]) and not np.any(S64["gc"][12])
    j = sc.tagged["empty"][0]
    assert not np.any(S64["Cp6"][j]) and not np.any(S64["gp"][j])


def test_seeded_defects_in_step_and_reprojection():
    sc, _ = scene("reg")
    d = 10
    T = host("reg", d)
    x, Jc, Jp, ft = T["x"], T["Jcs"], T["Jps"], T["ft"]
    pc, pp = seeded_step(sc, d)
    x_new, scal = step_f64(sc, d, T, pc, pp, 0.5)
    good = mr.judge_step(Jc, Jp, ft, x, pc, pp, 0.5, x_new, scal, sc, d)
    assert all(r <= 1 for r, _ in good.values()), good
    _, no_reg = step_f64(sc, d, T, pc, pp, 0.5, with_reg=False)        # JS2 / GTS without the regulariser share
    res = mr.judge_step(Jc, Jp, ft, x, pc, pp, 0.5, x_new, dict(scal, JS2=no_reg["JS2"], GTS=no_reg["GTS"]), sc, d)
    flagged(*res["JS2"]); flagged(*res["GTS"])
    i = 3 * d + 7
    bad = x_new.copy(); bad[i] = np.nextafter(np.nextafter(bad[i], np.inf), np.inf)          # x_new off by 2 ulp in one entry
    flagged(*mr.judge_step(Jc, Jp, ft, x, pc, pp, 0.5, bad, scal, sc, d)["x_new"], "camera 3, parameter 7")
    one = x_new.copy(); one[i] = mr.fma_rounded(x[i:i + 1], 0.5, np.concatenate([pc, pp])[i:i + 1])[0]
    assert mr.judge_step(Jc, Jp, ft, x, pc, pp, 0.5, one, scal, sc, d)["x_new"][0] == 0
    err_own, n2 = reproj_f64(sc, d, x, False)              # shared_k ignored in the reprojection error
    res = mr.judge_reproj(x, sc, d, True, err_own, n2)
    flagged(*res["err"]); flagged(*res["norm2"])
