"""Stage-by-stage reference of everything that evaluates the camera model (sfm_amd/csrc/ba_model.hip: the linearisation, the
block sums, the trial step, the cost and the reprojection errors) in 80-bit arithmetic, the error scales each stage is judged
by, and the scene builder that puts the edges of the model and of the chunk contraction on purpose.

NumPy only (a plain helper module like tests/stage_reference.py, imported by tests/test_model_reference.py on the CPU and by
tests/test_ba_model_gpu.py on the GPU; it never imports the GPU backend).  The rotation is INDEPENDENT of the Rodrigues
coefficients the kernels and the float64 oracle share: R = exp([r]x) summed as a power series in np.longdouble, dR/dr_i from the
same series by the product rule - no a, b, a1, b1, no small-angle branch.  The rows are referenced from the x the test supplied;
every sum is referenced FROM THE ROWS THE DEVICE STORED (float32 under precision="mixed", widened exactly), so a sum's bound is
that of its own arithmetic.  The float64 oracle (oracle.ba_oracle.jacobian_blocks / linearize / residuals) is the
"transcription" the CPU tests hold to the bounds and seed defects into; its worst ratios are where the constants below come from.

Formulas (kernel comments of ba_model.hip, ba_device.h: huber_row):
  Y = R X + t,  f = (fx Y_x / Y_z + cx - u, fy Y_y / Y_z + cy - v),  Pi = d f / d Y,  Jc = [Pi dR/dr_i X | Pi | diag(xn, yn) | I],  Jp = Pi R
  Huber per scalar row: |f| <= 1: rho0 = f^2, row scale 1, f~ = f;  else rho0 = 2 |f| - 1, row scale 2^-26, f~ = +-2^26
  B_c = sum Jc~^T Jc~ (+ the regulariser rows, d = 10),  g_c = sum Jc~^T f~,  C_p (packed xx xy xz yy yz zz) and g_p the same of Jp~
  regulariser rows: w ((fx - fx0) / fx0, (fy - fx) / fx, (cx - cx0) / width, (cy - cy0) / height), Huber-scaled like the others
  step: x_new = x + scale p,  t = scale (Jc~ p_c + Jp~ p_p) per row,  JS2 = sum t^2,  GTS = sum f~ t
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the model reference needs an extended-precision np.longdouble (x87 80-bit: 64-bit significand)"
U = 2.0 ** -53                 # unit round-off of the arithmetic under test (float64)
HUBER_SCALE = 2.0 ** -26       # row scale of a Huber-linear row: sqrt(EPS) (huber_row)
HUBER_FT = 2.0 ** 26           # |f~| of such a row
SERIES_TERMS = 60              # |R R^T - I| <= 6e-18 up to |r| = 6.2 (tests/test_model_reference.py measures it)
CHUNK_OBS = 256
INF = float("inf")

# ---- tolerances that cannot be derived.  Each is 8 x the worst ratio of the float64 transcription (oracle.ba_oracle.jacobian_blocks
# for the rows and f, the same formulas for the reprojection error) to the same scale, over every variant of model_scene and
# d in {10, 6} (tests/test_model_reference.py re-measures them and fails if the transcription exceeds a record by more than 2 %).
# A kernel rebuilds R X from cross products and contracts into FMA: other roundings, the same scale.  None was chosen by looking
# at a GPU result.  Row bound: |got - ref| <= C_blk u kappa_k max|ref block|, kappa_k = max(|R||X| + |t|) / |Y_z|.
C_ROT = 8 * 18.4               # rotation block Pi (dR/dr_i) X; measured 18.37 on `ragged` d = 10, camera 2 (|r| = 0.01001, just above the
                               # th2 = 1e-4 seam: the cancellation in the closed form's a1 / b1 costs about 1.5 digits there)
C_TRANS = 8 * 2.13             # translation block Pi; measured 2.127 on `ragged` d = 10, camera 0 (|r| = 6.2)
C_INTR = 8 * 0.762             # intrinsics block (xn, yn, 1); measured 0.7619 on `ragged` d = 10, camera 0
C_PT = 8 * 3.66                # point block Pi R; measured 3.658 on `ragged` d = 10, camera 4 (|r| = pi + 1e-3)
C_F = 8 * 1.33                 # f: <= C_F u (kappa_k max(|fx xn|, |fy yn|) + |c| + |uv|); measured 1.322 on `ragged` d = 10, camera 0
C_ERR = 8 * 0.721              # sqrt(f0^2 + f1^2): <= C_ERR u (scale of f0 + scale of f1); measured 0.7209 on `ragged` d = 10, camera 0
                               # (the cameras are the same in every variant: the other variants repeat these figures or stay below)

# ---- derived.  An inner product of n terms summed in any order, with or without FMA, by chunk partials or on the matrix cores,
# has |error| <= gamma_n sum|a||b|, gamma_n = n u / (1 - n u) <= (n + 1) u for n u < 0.01: every term passes one product rounding
# (none under FMA) and at most n - 1 additions whatever the tree.  Over the m observations of a camera / a track n = 2 m (two
# residual rows each):  (2 m + c) u sum|a||b|  with
C_SUM = 1                      # c without regulariser rows: the second-order part of gamma_n
C_SUM_REG = 1 + 4 + 10         # c of B / g_c when the camera carries regulariser rows (d = 10): 4 more terms, and every one of them is
                               # formed from rows k_cam_reg computes from x itself (the reference takes them from x in 80 bits): an
                               # entry of J_reg takes at most 4 roundings (-w fy / (fx fx)), a residual 3, so a term J J or J f~
                               # carries at most 4 + 4 + 1 = 9 u of its own, 10 u with the second order
C_REG_ROW = 5                  # relative round-off, in u, of one entry of the stored regulariser rows and residuals (4 and 3 above, second order)

ROW_BLOCKS = (("rotation", 0, 3), ("translation", 3, 6), ("intrinsics", 6, 10))
STRUCT_ZEROS = ((0, 4), (1, 3), (0, 7), (0, 9), (1, 6), (1, 8))     # entries of Jc [2][d] that are zero whatever x is


# ------------------------------------------------------------------------------------------------ rotation
def skew(v, dt=LD):
    v = np.asarray(v).astype(dt)
    out = np.zeros(v.shape[:-1] + (3, 3), dtype=dt)
    out[..., 0, 1] = -v[..., 2]; out[..., 0, 2] = v[..., 1]
    out[..., 1, 0] = v[..., 2]; out[..., 1, 2] = -v[..., 0]
    out[..., 2, 0] = -v[..., 1]; out[..., 2, 1] = v[..., 0]
    return out


def rotation_series(rvec, terms=SERIES_TERMS):
    """R = sum_k [r]x^k / k! and dR/dr_i by the product rule on every term, in 80 bits: T_k = T_{k-1} [r]x / k,
    d_i T_k = (d_i T_{k-1} [r]x + T_{k-1} [e_i]x) / k.  rvec [C][3] -> R [C][3][3], dR [C][3(i)][3][3]."""
    r = np.asarray(rvec).astype(LD).reshape(-1, 3)
    S = skew(r)
    E = skew(np.eye(3))
    T = np.broadcast_to(np.eye(3, dtype=LD), (r.shape[0], 3, 3)).copy()
    dT = np.zeros((r.shape[0], 3, 3, 3), dtype=LD)
    R, dR = T.copy(), dT.copy()
    for k in range(1, terms + 1):
        dT = (np.einsum("cipq,cqr->cipr", dT, S) + np.einsum("cpq,iqr->cipr", T, E)) / LD(k)
        T = np.einsum("cpq,cqr->cpr", T, S) / LD(k)
        R += T; dR += dT
    return R, dR


def rotation_closed(rvec):
    """The closed form R = I + a [r]x + b [r]x^2 and its derivative in 80 bits (no series: for |r| away from 0 only)."""
    r = np.asarray(rvec).astype(LD).reshape(-1, 3)
    th2 = np.sum(r * r, axis=1); t = np.sqrt(th2)
    s, c = np.sin(t), np.cos(t)
    a, b = s / t, (1 - c) / th2
    a1, b1 = (t * c - s) / (th2 * t), (t * s - 2 * (1 - c)) / (th2 * th2)
    S = skew(r); S2 = S @ S
    R = np.eye(3, dtype=LD)[None] + a[:, None, None] * S + b[:, None, None] * S2
    E = skew(np.eye(3))
    dR = np.stack([a[:, None, None] * E[i][None] + b[:, None, None] * (E[i][None] @ S + S @ E[i][None])
                   + (a1 * r[:, i])[:, None, None] * S + (b1 * r[:, i])[:, None, None] * S2 for i in range(3)], axis=1)
    return R, dR


def kernel_th2(rvec):
    """th2 as k_campre forms it (an FMA contraction moves it by an ulp at most; the scene's magnitudes keep away from that)."""
    r = np.asarray(rvec, dtype=np.float64).reshape(-1, 3)
    return r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]


# ------------------------------------------------------------------------------------------------ the model in 80 bits
def split_x(x, C, d):
    x = np.asarray(x)
    return x[:C * d].reshape(C, d), x[C * d:].reshape(-1, 3)


def _intrinsics(cams, d, K, shared_k):
    if d == 10 and not shared_k:
        return cams[:, 6], cams[:, 7], cams[:, 8], cams[:, 9]
    return tuple(np.full(cams.shape[0], LD(v), dtype=LD) for v in K)


def model(x, sc, d, shared_k=False):
    """f [N][2], Pi [N][2][3], Jc [N][2][d], Jp [N][2][3] (unscaled), kappa [N], fscale [N][2], Yz [N] at x, in 80 bits."""
    cams, pts = split_x(np.asarray(x, dtype=np.float64).astype(LD), sc.C, d)
    R, dR = rotation_series(cams[:, :3])
    fx, fy, cx, cy = _intrinsics(cams, d, sc.K, shared_k)
    ci, pi = sc.cam_idx, sc.pt_idx
    N = ci.shape[0]
    X = pts[pi]
    Y = np.einsum("nij,nj->ni", R[ci], X) + cams[ci, 3:6]
    iz = 1 / Y[:, 2]
    xn, yn = Y[:, 0] * iz, Y[:, 1] * iz
    uv = np.asarray(sc.uv, dtype=np.float64).astype(LD)
    f = np.stack([fx[ci] * xn + cx[ci] - uv[:, 0], fy[ci] * yn + cy[ci] - uv[:, 1]], axis=1)
    Pi = np.zeros((N, 2, 3), dtype=LD)
    Pi[:, 0, 0] = fx[ci] * iz; Pi[:, 0, 2] = -fx[ci] * xn * iz
    Pi[:, 1, 1] = fy[ci] * iz; Pi[:, 1, 2] = -fy[ci] * yn * iz
    Jc = np.zeros((N, 2, d), dtype=LD)
    Jc[:, :, 0:3] = Pi @ np.einsum("nkij,nj->nik", dR[ci], X)
    Jc[:, :, 3:6] = Pi
    if d == 10:
        Jc[:, 0, 6] = xn; Jc[:, 1, 7] = yn; Jc[:, 0, 8] = 1; Jc[:, 1, 9] = 1
    Jp = Pi @ R[ci]
    reach = np.einsum("nij,nj->ni", np.abs(R[ci]), np.abs(X)) + np.abs(cams[ci, 3:6])
    kappa = (np.max(reach, axis=1) / np.abs(Y[:, 2])).astype(np.float64)
    img = np.maximum(np.abs(fx[ci] * xn), np.abs(fy[ci] * yn)).astype(np.float64)
    fscale = (kappa * img)[:, None] + np.stack([np.abs(cx[ci]), np.abs(cy[ci])], axis=1).astype(np.float64) + np.abs(np.asarray(sc.uv, dtype=np.float64))
    return dict(f=f, Pi=Pi, Jc=Jc, Jp=Jp, kappa=kappa, fscale=fscale, Yz=Y[:, 2].astype(np.float64))


def huber(f):
    """(rho0, row scale, f~) of huber_row's header comment, in the type of f."""
    f = np.asarray(f)
    inl = np.abs(f) <= 1
    one = f.dtype.type(1)
    return (np.where(inl, f * f, 2 * np.abs(f) - 1), np.where(inl, one, f.dtype.type(HUBER_SCALE)),
            np.where(inl, f, np.sign(f) * f.dtype.type(HUBER_FT)))


def reg_rows(cams, sc, dt=LD, fx_of_row1=None):
    """The regulariser rows of the cameras [C][10]: (f [C][4], scaled J [C][4][4] w.r.t. (fx, fy, cx, cy), f~ [C][4], rho0 [C][4]).
    fx_of_row1: the focal length row 1 is differentiated with (seeded defect)."""
    c = np.asarray(cams, dtype=np.float64).astype(dt)
    fx0, cx0, cy0 = (dt(sc.K[0]), dt(sc.K[2]), dt(sc.K[3]))
    w, W, H = dt(sc.reg_weight), dt(sc.width), dt(sc.height)
    fx, fy, cx, cy = c[:, 6], c[:, 7], c[:, 8], c[:, 9]
    f = np.stack([(fx - fx0) / fx0 * w, (fy - fx) / fx * w, (cx - cx0) / W * w, (cy - cy0) / H * w], axis=1)
    J = np.zeros((c.shape[0], 4, 4), dtype=dt)
    fd = fx if fx_of_row1 is None else np.full_like(fx, fx_of_row1)
    J[:, 0, 0] = w / fx0
    J[:, 1, 0] = -w * fy / (fd * fd); J[:, 1, 1] = w / fd
    J[:, 2, 2] = w / W; J[:, 3, 3] = w / H
    rho0, s, ft = huber(f)
    return f, J * s[:, :, None], ft, rho0


def _apply_reg(sc, d):
    return d == 10 and sc.reg_weight is not None


# ------------------------------------------------------------------------------------------------ judges: rows
def _half_ulp32(v):
    return 0.5 * np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _row_ratios(ref, exact, Jc_got, Jp_got, ft_got, mixed):
    """Per (observation, residual row, piece) the ratio to the bound under the inlier branch and under the outlier branch.
    Pieces: the blocks of Jc present, the point block, the structural zeros, f~."""
    d = ref["Jc"].shape[2]
    N = ref["f"].shape[0]
    kap = ref["kappa"]
    pieces = [(n, ref["Jc"][:, :, a:b], np.asarray(Jc_got)[:, :, a:b], c) for (n, a, b), c in zip(ROW_BLOCKS, (C_ROT, C_TRANS, C_INTR)) if b <= d]
    pieces.append(("point", ref["Jp"], np.asarray(Jp_got), C_PT))
    names = [p[0] for p in pieces] + ["zeros", "f~"]
    out = np.zeros((2, N, 2, len(names)))          # [branch: inlier, outlier]
    for q, (_, rblk, gblk, const) in enumerate(pieces):
        blk_max = np.max(np.abs(rblk).reshape(N, -1), axis=1).astype(np.float64)
        b64 = (const * U * kap * blk_max)[:, None, None]
        for br, s in enumerate((1.0, HUBER_SCALE)):
            want = rblk * LD(s)
            bound = s * b64 + (_half_ulp32(np.abs(want).astype(np.float64) + s * b64) if mixed else 0.0)
            err = np.abs(np.asarray(gblk, dtype=np.float64).astype(LD) - want).astype(np.float64)
            ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, INF, 0.0))
            out[br, :, :, q] = np.max(ratio, axis=2)
    zq = len(pieces)
    for r, a in STRUCT_ZEROS:
        if a < d:
            out[:, :, r, zq] = np.maximum(out[:, :, r, zq], np.where(np.asarray(Jc_got)[:, r, a] != 0, INF, 0.0)[None])
    fq = zq + 1
    f = ref["f"]
    got = np.asarray(ft_got, dtype=np.float64)
    fb = C_F * U * ref["fscale"] + (_half_ulp32(np.abs(f).astype(np.float64) + C_F * U * ref["fscale"]) if mixed else 0.0)
    out[0, :, :, fq] = np.abs(got.astype(LD) - f).astype(np.float64) / fb
    if exact is not None:                  # rows whose f the kernel forms without a rounding: f~ of an inlier is f itself
        same = got == (f.astype(np.float32).astype(np.float64) if mixed else f.astype(np.float64))
        out[0, :, :, fq] = np.where(exact, np.where(same, 0.0, INF), out[0, :, :, fq])
    out[1, :, :, fq] = np.where(got == np.sign(f).astype(np.float64) * HUBER_FT, 0.0, INF)
    return out, names


def undecided_rows(ref, exact=None):
    """[N][2]: rows whose | |f| - 1 | is within the bound of f itself: the reference cannot say which Huber branch is right.
    A row the scene builds exactly (exact [N][2]) is never undecided."""
    und = np.abs(np.abs(ref["f"]) - 1).astype(np.float64) <= C_F * U * ref["fscale"]
    return und & ~exact if exact is not None else und


def judge_rows(x, sc, d, Jc_got, Jp_got, ft_got, mixed=False):
    """The stored rows Jc~ [N][2][d], Jp~ [N][2][3] and f~ [N][2] against the 80-bit model at x: per observation, residual row and
    block |got - s ref| <= s C_blk u kappa_k max|ref block| (s the row's Huber scale; plus half a float32 ulp under mixed
    precision), f~ = f inside the bound of f on an inlier row, = +-2^26 exactly on an outlier row, structural zeros exact.  An
    undecided row passes if it matches either branch.  Returns (worst ratio, where)."""
    ref = model(x, sc, d)
    exact = getattr(sc, "exact", None)
    rr, names = _row_ratios(ref, exact, Jc_got, Jp_got, ft_got, mixed)
    inl = (np.abs(ref["f"]) <= 1)
    decided = np.where(inl[:, :, None], rr[0], rr[1])
    und = undecided_rows(ref, exact)
    either = np.where(np.max(rr[0], axis=2) <= np.max(rr[1], axis=2), 0, 1)
    ratio = np.where(und[:, :, None], np.where(either[:, :, None] == 0, rr[0], rr[1]), decided)
    k, r, q = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    c = int(sc.cam_idx[k])
    rn = float(np.sqrt(np.sum(np.asarray(x, dtype=np.float64)[c * d:c * d + 3] ** 2)))
    where = (f"observation {k} (camera {c}, |r| = {rn:.6g}, point {int(sc.pt_idx[k])}), row {r}, {names[q]} "
             f"({'inlier' if inl[k, r] else 'outlier'}{', undecided' if und[k, r] else ''}, kappa {ref['kappa'][k]:.3g})")
    return float(ratio[k, r, q]), where


def measure_rows(x, sc, d, Jc_got, Jp_got, f_got):
    """Raw ratios (no constant) of UNSCALED rows and f to u kappa max|block| / u fscale: where C_ROT ... C_F come from.
    Returns {name: (ratio, camera)}."""
    ref = model(x, sc, d)
    out = {}
    N = ref["f"].shape[0]
    for name, rblk, gblk in [(n, ref["Jc"][:, :, a:b], np.asarray(Jc_got)[:, :, a:b]) for n, a, b in ROW_BLOCKS if b <= d] + [("point", ref["Jp"], np.asarray(Jp_got))]:
        scale = U * ref["kappa"] * np.max(np.abs(rblk).reshape(N, -1), axis=1).astype(np.float64)
        err = np.max(np.abs(np.asarray(gblk, dtype=np.float64).astype(LD) - rblk).astype(np.float64).reshape(N, -1), axis=1)
        ratio = err / scale
        out[name] = (float(ratio.max()), int(sc.cam_idx[int(np.argmax(ratio))]), ratio)
    ratio = np.max(np.abs(np.asarray(f_got, dtype=np.float64).astype(LD) - ref["f"]).astype(np.float64) / (U * ref["fscale"]), axis=1)
    out["f"] = (float(ratio.max()), int(sc.cam_idx[int(np.argmax(ratio))]), ratio)
    return out


# ------------------------------------------------------------------------------------------------ sums of the stored rows
IU = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def stage_sums(Jc, Jp, ft, cam_idx, pt_idx, C, P, dt=LD, reg=None, obs_mask=None):
    """{B [C][d][d], gc [C][d], Cp6 [P][6], gp [P][3]} from the stored rows, each with the sum of absolute values of its terms
    (name + "_abs").  reg: (scaled regulariser rows [C][4][4], f~ [C][4]) added into B / g_c.  obs_mask drops observations from
    the camera side (seeded defect)."""
    Jc, Jp, ft = (np.asarray(a).astype(dt) for a in (Jc, Jp, ft))
    ci, pi = np.asarray(cam_idx), np.asarray(pt_idx)
    d = Jc.shape[2]
    out = {}
    Jcc, ftc, cic = (Jc, ft, ci) if obs_mask is None else (Jc[obs_mask], ft[obs_mask], ci[obs_mask])
    for tag, fn in (("", lambda a: a), ("_abs", np.abs)):
        B = np.zeros((C, d, d), dtype=dt); gc = np.zeros((C, d), dtype=dt)
        Cp = np.zeros((P, 3, 3), dtype=dt); gp = np.zeros((P, 3), dtype=dt)
        np.add.at(B, cic, np.einsum("nri,nrj->nij", fn(Jcc), fn(Jcc)))
        np.add.at(gc, cic, np.einsum("nri,nr->ni", fn(Jcc), fn(ftc)))
        np.add.at(Cp, pi, np.einsum("nri,nrj->nij", fn(Jp), fn(Jp)))
        np.add.at(gp, pi, np.einsum("nri,nr->ni", fn(Jp), fn(ft)))
        if reg is not None:
            Jr, fr = fn(np.asarray(reg[0]).astype(dt)), fn(np.asarray(reg[1]).astype(dt))
            B[:, 6:, 6:] += np.einsum("cri,crj->cij", Jr, Jr)
            gc[:, 6:] += np.einsum("cri,cr->ci", Jr, fr)
        out.update({"B" + tag: B, "gc" + tag: gc, "Cp6" + tag: np.stack([Cp[:, i, j] for i, j in IU], axis=1), "gp" + tag: gp})
    return out


def _ratio(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, INF, 0.0))


def judge_sums(Jc, Jp, ft, x, sc, d, B_got, gc_got, Cp6_got, gp_got):
    """B, g_c, C_p (packed 6), g_p from the rows the device stored (widened exactly; the regulariser rows from x in 80 bits):
    componentwise inside (2 m + c) u sum|a||b| (C_SUM / C_SUM_REG above), m the observations of the camera / the track.  An entry
    whose terms are all zero must be exactly zero: a camera without observations holds exactly the regulariser block (d = 10) or
    zeros (d = 6), an empty track exactly zeros.  Returns {name: (worst ratio, where)}."""
    C, P = sc.C, sc.P
    reg = None
    if _apply_reg(sc, d):
        _, Jr, fr, _ = reg_rows(split_x(x, C, d)[0], sc)
        reg = (Jr, fr)
    ref = stage_sums(Jc, Jp, ft, sc.cam_idx, sc.pt_idx, C, P, reg=reg)
    mc = np.bincount(sc.cam_idx, minlength=C); mp = np.bincount(sc.pt_idx, minlength=P)
    cB = C_SUM + (C_SUM_REG if reg is not None else 0)
    out = {}
    for name, got, m, c, shape in (("B", B_got, mc, cB, (C, d, d)), ("gc", gc_got, mc, cB, (C, d)), ("Cp6", Cp6_got, mp, C_SUM, (P, 6)),
                                   ("gp", gp_got, mp, C_SUM, (P, 3))):
        mm = m.reshape((-1,) + (1,) * (len(shape) - 1))
        ratio = _ratio(np.asarray(got).reshape(shape), ref[name], (2 * mm + c) * U * ref[name + "_abs"].astype(np.float64))
        idx = np.unravel_index(int(np.argmax(ratio)), shape)
        i = int(idx[0])
        who = f"camera {i}" if name in ("B", "gc") else f"point {i}"
        out[name] = (float(ratio[idx]), f"{who} ({int(m[i])} observations, {-(-int(m[i]) // CHUNK_OBS)} chunks), entry {list(map(int, idx[1:]))}")
    return out


def model_cost(x, sc, d):
    """(0.5 sum rho0 over the reprojection and regulariser rows at x in 80 bits, its bound): every rho0 moves by rho0'(f) times the
    bound of its f (C_F u fscale; a regulariser residual C_REG_ROW u |f|), and the sum of M positive terms in any order adds
    (M + 2) u of the total (the 0.5 is exact)."""
    ref = model(x, sc, d)
    f = ref["f"]
    rho0 = huber(f)[0]
    slope = np.where(np.abs(f) <= 1, 2 * np.abs(f), LD(2)).astype(np.float64)
    total = np.sum(rho0); db = float(np.sum(slope * C_F * U * ref["fscale"])); M = f.size
    if _apply_reg(sc, d):
        fr, _, _, rr = reg_rows(split_x(x, sc.C, d)[0], sc)
        total += np.sum(rr)
        db += float(np.sum(np.where(np.abs(fr) <= 1, 2 * np.abs(fr), LD(2)) * C_REG_ROW * U * np.abs(fr)))
        M += fr.size
    return 0.5 * total, 0.5 * (db + (M + 2) * U * float(total))


def judge_lin_scalars(x, sc, d, B_got, gc_got, Cp6_got, gp_got, cost, gnorm2, ginf, hdiag):
    """HDIAG and GINF are maxima over the device's own diagonals / gradient: bit for bit.  GNORM2 = sum g^2 over the device's g:
    n terms, each a rounded square: (n + 2) u of the sum.  COST against model_cost.  Returns {name: (ratio, where)}."""
    B = np.asarray(B_got, dtype=np.float64).reshape(sc.C, d, d)
    Cp = np.asarray(Cp6_got, dtype=np.float64).reshape(-1, 6)
    g = np.concatenate([np.ravel(gc_got), np.ravel(gp_got)]).astype(np.float64)
    hd = max(float(np.max(np.einsum("cii->ci", B))), float(np.max(Cp[:, [0, 3, 5]])))
    gi = float(np.max(np.abs(g)))
    g2 = np.sum(g.astype(LD) ** 2)
    cref, cb = model_cost(x, sc, d)
    return {"HDIAG": (0.0 if hdiag == hd else INF, f"{hdiag!r} against {hd!r}"), "GINF": (0.0 if ginf == gi else INF, f"{ginf!r} against {gi!r}"),
            "GNORM2": (float(abs(LD(gnorm2) - g2)) / float((g.size + 2) * U * g2), "the scalar"),
            "COST": (float(abs(LD(cost) - cref)) / cb, "the scalar")}


# ------------------------------------------------------------------------------------------------ the trial step
def fma_rounded(x, s, p):
    """fl(x + s p) with ONE rounding, entry by entry (exact rationals; float() of a Fraction rounds to nearest even)."""
    fs = Fraction(float(s))
    return np.array([float(Fraction(float(a)) + fs * Fraction(float(b))) for a, b in zip(x, p)], dtype=np.float64)


def judge_step(Jc, Jp, ft, x, pc, pp, scale, x_new_got, scalars, sc, d):
    """sfm_ba_step from the device's own rows, the step (pc, pp) the test wrote and scale.  scalars: dict JS2, GTS, COST_NEW,
    SNORM2, XNEW_NORM2.  Returns {name: (ratio, where)}.
      x_new: fl(x + fl(scale p)) or the single-rounded FMA, nothing else (ratio 0 or inf).
      t = scale (Jc~ pc + Jp~ pp), an inner product of d + 3 terms and one more product: |dt| <= (d + 5) u |scale| sum|a||b| =: e;
      JS2 = sum t^2: sum (2 |t| e + e^2) from the rows, and (M + 2) u sum t^2 for the squares and the sum of M rows in any order;
      GTS = sum f~ t: sum |f~| e + (M + 2) u sum |f~ t|.  The regulariser rows (reference: from x in 80 bits) carry C_REG_ROW u more
      per stored entry.  SNORM2 = sum (scale p)^2: (n + 4) u of the sum (product, square, n terms);  XNEW_NORM2 from the device's
      own x_new: (n + 2) u of the sum;  COST_NEW against model_cost at the device's own x_new."""
    C, P = sc.C, sc.P
    n = C * d
    x = np.asarray(x, dtype=np.float64); got = np.asarray(x_new_got, dtype=np.float64)
    p = np.concatenate([np.ravel(pc), np.ravel(pp)]).astype(np.float64)
    two = x + scale * p
    ok = (got == two) | (got == fma_rounded(x, scale, p))
    out = {}
    if np.all(ok):
        out["x_new"] = (0.0, "every entry")
    else:
        i = int(np.argmin(ok))
        who = f"camera {i // d}, parameter {i % d}" if i < n else f"point {(i - n) // 3}, coordinate {(i - n) % 3}"
        out["x_new"] = (INF, f"entry {i} ({who}): {got[i]!r}, {(got[i] - two[i]) / np.spacing(two[i]):+.0f} ulp off x + scale p = {two[i]!r}")
    ci, pi = sc.cam_idx, sc.pt_idx
    Jcl, Jpl, ftl = (np.asarray(a, dtype=np.float64).astype(LD) for a in (Jc, Jp, ft))
    pcl, ppl = np.asarray(pc, dtype=np.float64).astype(LD).reshape(C, d), np.asarray(pp, dtype=np.float64).astype(LD).reshape(P, 3)
    s = LD(scale)
    t = s * (np.einsum("nra,na->nr", Jcl, pcl[ci]) + np.einsum("nra,na->nr", Jpl, ppl[pi]))
    e = ((d + 5) * U * abs(float(scale)) * (np.einsum("nra,na->nr", np.abs(Jcl), np.abs(pcl[ci])) + np.einsum("nra,na->nr", np.abs(Jpl), np.abs(ppl[pi])))).astype(np.float64)
    ta = np.abs(t).astype(np.float64)
    js2, gts = np.sum(t * t), np.sum(ftl * t)
    b_js2, b_gts = float(np.sum(2 * ta * e + e * e)), float(np.sum(np.abs(ftl).astype(np.float64) * e))
    a_gts = float(np.sum(np.abs(ftl * t)))
    M = t.size
    if _apply_reg(sc, d):
        _, Jr, fr, _ = reg_rows(split_x(x, C, d)[0], sc)
        tr = s * np.einsum("cra,ca->cr", Jr, pcl[:, 6:])
        er = ((4 + 2 + C_REG_ROW) * U * abs(float(scale)) * np.einsum("cra,ca->cr", np.abs(Jr), np.abs(pcl[:, 6:]))).astype(np.float64)
        tra = np.abs(tr).astype(np.float64)
        js2 += np.sum(tr * tr); gts += np.sum(fr * tr)
        b_js2 += float(np.sum(2 * tra * er + er * er))
        b_gts += float(np.sum(np.abs(fr).astype(np.float64) * (er + C_REG_ROW * U * tra)))
        a_gts += float(np.sum(np.abs(fr * tr))); M += tr.size
    b_js2 += (M + 2) * U * float(js2); b_gts += (M + 2) * U * a_gts
    out["JS2"] = (float(abs(LD(scalars["JS2"]) - js2)) / b_js2 if b_js2 > 0 else (0.0 if scalars["JS2"] == 0 else INF), "the scalar")
    out["GTS"] = (float(abs(LD(scalars["GTS"]) - gts)) / b_gts if b_gts > 0 else (0.0 if scalars["GTS"] == 0 else INF), "the scalar")
    sn = np.sum((s * p.astype(LD)) ** 2)
    out["SNORM2"] = (float(abs(LD(scalars["SNORM2"]) - sn)) / float((p.size + 4) * U * sn), "the scalar")
    xn = np.sum(got.astype(LD) ** 2)
    out["XNEW_NORM2"] = (float(abs(LD(scalars["XNEW_NORM2"]) - xn)) / float((p.size + 2) * U * xn), "the scalar")
    cref, cb = model_cost(got, sc, d)
    out["COST_NEW"] = (float(abs(LD(scalars["COST_NEW"]) - cref)) / cb, "the scalar")
    return out


# ------------------------------------------------------------------------------------------------ reprojection errors
def reproj_reference(x, sc, d, shared_k):
    """(err [N] in 80 bits, its bound [N]): err = sqrt(f0^2 + f1^2), |d err| <= C_ERR u (fscale0 + fscale1)."""
    ref = model(x, sc, d, shared_k=shared_k)
    return np.sqrt(np.sum(ref["f"] ** 2, axis=1)), C_ERR * U * np.sum(ref["fscale"], axis=1)


def judge_reproj(x, sc, d, shared_k, err_got, norm2_got=None):
    """The per-observation reprojection error, and residual_norm2 = sum err^2 (bound: sum (2 err b + b^2) with b the bound of err,
    plus (N + 2) u of the sum).  Returns {name: (ratio, where)}."""
    err, b = reproj_reference(x, sc, d, shared_k)
    ratio = _ratio(err_got, err, b)
    k = int(np.argmax(ratio))
    out = {"err": (float(ratio[k]), f"observation {k} (camera {int(sc.cam_idx[k])}, shared_k = {int(bool(shared_k))})")}
    if norm2_got is not None:
        tot = np.sum(err * err)
        bound = float(np.sum(2 * err.astype(np.float64) * b + b * b)) + (err.size + 2) * U * float(tot)
        out["norm2"] = (float(abs(LD(norm2_got) - tot)) / bound, "the scalar")
    return out


# ------------------------------------------------------------------------------------------------ scenes with the edges on purpose
class ModelScene:
    """cams0 [C][10], pts0 [P][3], point-major observations (cam_idx, pt_idx, uv), K, width, height, reg_weight, exact [N][2]
    (rows whose f the kernel forms without a rounding) and what the scene was built to contain."""
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def x0(self, d):
        return np.concatenate([np.ascontiguousarray(self.cams0[:, :d]).ravel(), self.pts0.ravel()])


K_REF = (1228.0, 1228.0, 512.0, 384.0)
VARIANTS = ("ragged", "aligned", "mixed", "plane", "seam", "reg")
# camera c: (observations, |rvec|).  The chunk and wave-split edges sit on the cameras at and around the th2 = 1e-4 seam and on the
# largest rotation; cameras 13 and 14 carry the duplicate track, the single-observation tracks and the padding of `aligned`.
NAMED_CAMS = ((513, 6.2), (257, 0.01), (256, 0.01001), (255, 0.00999), (9, np.pi + 1e-3), (8, np.pi - 1e-3), (7, 0.0), (5, 1e-160),
              (4, 1e-8), (3, 1.8), (2, 0.5), (1, 1.8), (0, 0.5))
EXTRA_CAMS = ((13, 0.3), (10, 0.09))     # 0.09: th2 between 1e-4 and 1e-2, where a series kept too long shows
SEAM_CAM, NEAR_CAM, BEHIND_CAM = 6, 13, 14
SEAM_T = (0.0, -0.25, 5.0)
# (Y_x, Y_y) of the seam camera's first four observations (Y_z = 4: 1 / Y_z and the products by fx = fy = 1228 are exact) and the
# f of their rows
SEAM_ROWS = (((1.0, 0.5), (0.0, 1.0)), ((-1.0, -1.25), (-1.0, float(np.nextafter(1.0, 2.0)))), ((0.5, -0.5), (2.0, 0.0)),
             ((-0.5, 0.75), (1.0, -1.0)))
REG_WEIGHT = 64.0              # `reg`: 1228 / 64 is exact, so fx = fx0 (1 + 1/64) has the regulariser residual exactly 1.0
REG_CAMS = {1: 1.0 + 1.0 / 64, 2: 1.0 + 1.0 / 32}       # camera: fx / fx0


def model_scene(variant="ragged", seed=11, noise_px=0.3):
    """Cameras built directly: t ~ (0, 0, 6) with any rvec keeps the [-1, 1]^3 box of points in front.
    variants:
      ragged   N and P with remainders mod 256
      aligned  N % 256 == 0 and P % 256 == 0 (padding tracks on cameras 13 / 14)
      mixed    a third of the observations 4 px off (Huber-linear rows)
      plane    three points at Y_z ~ 0.05 on camera 13, one point behind camera 14
      seam     camera 6 (rvec = 0) with dyadic t, points and intrinsics K: rows with f exactly 0, 1, -1, nextafter(1, 2), 2
      reg      reg_weight 64: regulariser residuals of exactly 1.0 (camera 1) and 2.0 (camera 2), fy far from fx (camera 3)
    """
    assert variant in VARIANTS
    rng = np.random.default_rng(seed)
    spec = NAMED_CAMS + EXTRA_CAMS
    C = len(spec)
    tracks = [(tuple(c for c in range(C) if spec[c][0] > 0), "all"), ((13, 13, 14), "dup"), ((), "empty")]
    tracks += [((13, 14), "")] * 6 + [((13,), "near")] * 3 + [((13,), "")] + [((14,), "behind")] + [((14,), "")]
    left = np.array([max(n - 1, 0) for n, _ in NAMED_CAMS])
    while np.count_nonzero(left) >= 2:                     # two-camera tracks between the two cameras that still lack the most
        a, b = np.argsort(-left, kind="stable")[:2]
        tracks.append(((int(min(a, b)), int(max(a, b))), "")); left[a] -= 1; left[b] -= 1
    tracks += [((int(c),), "")] * int(left.sum()) if left.sum() else []
    tracks = [tracks[i] for i in rng.permutation(len(tracks))]
    if variant == "aligned":
        while (sum(len(t) for t, _ in tracks) % 256) or (len(tracks) % 256):
            n_obs = sum(len(t) for t, _ in tracks)
            tracks.append(((13,) if n_obs % 2 else (13, 14) if n_obs % 256 else (), "pad"))
    P = len(tracks)
    cam_idx = np.array([c for t, _ in tracks for c in t], dtype=np.int64)
    pt_idx = np.repeat(np.arange(P, dtype=np.int64), [len(t) for t, _ in tracks])
    tagged = {tag: [j for j, (_, g) in enumerate(tracks) if g == tag] for tag in ("all", "dup", "empty", "near", "behind")}

    cams = np.zeros((C, 10))
    for c, (_, mag) in enumerate(spec):
        v = rng.normal(size=3); v /= np.linalg.norm(v)
        if mag == 0.01:
            v = np.array([0.0, 1.0, 0.0])                  # 0.01 * 0.01 == 1e-4 exactly: `<` takes the closed form
        cams[c, :3] = mag * v
        cams[c, 3:6] = np.array([0.0, 0.0, 6.0]) + rng.normal(0.0, 0.1, size=3)
        cams[c, 6:] = np.array(K_REF) + rng.uniform(-1.0, 1.0, size=4) * np.array([1.0, 1.0, 0.25, 0.25])
    pts = rng.uniform(-1.0, 1.0, size=(P, 3))
    reg_weight = 0.1
    if variant == "reg":
        reg_weight = REG_WEIGHT
        for c, ratio in REG_CAMS.items():
            cams[c, 6] = K_REF[0] * ratio
        cams[3, 7] = cams[3, 6] + 7.0
    seam_obs = np.flatnonzero(cam_idx == SEAM_CAM)[:len(SEAM_ROWS)]
    if variant == "seam":
        cams[SEAM_CAM, 3:6] = SEAM_T
        cams[SEAM_CAM, 6:] = K_REF
        for k, ((y0, y1), _) in zip(seam_obs, SEAM_ROWS):
            pts[pt_idx[k]] = (y0 - SEAM_T[0], y1 - SEAM_T[1], 4.0 - SEAM_T[2])
    if variant == "plane":
        R = rotation_series(cams[:, :3])[0].astype(np.float64)
        for i, j in enumerate(tagged["near"]):
            pts[j] = R[NEAR_CAM].T @ (np.array([0.002 * (i + 1), -0.003, 0.05 + 0.001 * i]) - cams[NEAR_CAM, 3:6])
        pts[tagged["behind"][0]] = R[BEHIND_CAM].T @ (np.array([0.3, -0.2, -2.0]) - cams[BEHIND_CAM, 3:6])
    sc = ModelScene(variant=variant, C=C, P=P, cams0=cams, pts0=pts, cam_idx=cam_idx, pt_idx=pt_idx, uv=np.zeros((cam_idx.shape[0], 2)),
                    K=K_REF, width=1024.0, height=768.0, reg_weight=reg_weight, tagged=tagged, seam_obs=seam_obs,
                    exact=np.zeros((cam_idx.shape[0], 2), dtype=bool),
                    named_cams={c: n for c, (n, _) in enumerate(NAMED_CAMS)}, mags=[m for _, m in spec])
    proj = model(sc.x0(10), sc, 10)["f"].astype(np.float64)
    uv = proj + rng.normal(0.0, noise_px, size=(cam_idx.shape[0], 2))
    if variant == "mixed":
        out = rng.random(uv.shape[0]) < 1.0 / 3.0
        uv[out] += rng.normal(0.0, 4.0, size=(int(out.sum()), 2))
    for c, (n, _) in enumerate(NAMED_CAMS):                # the last observation of every named camera is an inlier for d = 10 and d = 6
        if n:                                              # (a quarter of a pixel; the intrinsics of d = 6 are at most 0.55 px away)
            k = np.flatnonzero(cam_idx == c)[-1]
            uv[k] = proj[k] + np.array([0.25, -0.25])
    if variant == "seam":
        for k, ((y0, y1), targets) in zip(seam_obs, SEAM_ROWS):
            for r, (y, tgt) in enumerate(zip((y0, y1), targets)):
                val = Fraction(K_REF[r]) * Fraction(y) / 4 + Fraction(K_REF[2 + r])
                uv[k, r] = float(val - Fraction(tgt))
                assert Fraction(float(uv[k, r])) == val - Fraction(tgt)
            sc.exact[k] = True
    sc.uv = uv
    return sc


def _field(st, name):
    return np.asarray(st[name] if isinstance(st, dict) else getattr(st, name), dtype=np.int64)


def assert_model_edges(sc, st):
    """The edges the scene exists for are really there: the observation and chunk counts of the named cameras in the index
    structure, the rotation magnitudes and the branch k_campre takes for each, the kinds of track, and per variant the sizes, the
    depths, the exact seam rows and the regulariser residuals."""
    C = sc.C
    obs = np.diff(_field(st, "cam_ptr")); chunks = np.diff(_field(st, "cch_ptr"))
    for c, cnt in sc.named_cams.items():
        assert (int(obs[c]), int(chunks[c])) == (cnt, -(-cnt // CHUNK_OBS)), (c, int(obs[c]), int(chunks[c]))
    assert sorted(sc.named_cams.values()) == [0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 513]
    th2 = kernel_th2(sc.cams0[:, :3])
    for c, mag in enumerate(sc.mags):
        rn = float(np.sqrt(np.sum(sc.cams0[c, :3].astype(LD) ** 2)))
        assert abs(rn - mag) <= 4 * U * mag, (c, rn, mag)
        assert bool(th2[c] < 1e-4) == (mag < 0.01), (c, mag, th2[c])          # series below the seam, closed form at and above it
    assert th2[6] == 0.0 and 0.0 < th2[7] < np.finfo(np.float64).tiny     # rvec = 0, and th2 that underflows (1e-320: a denormal)
    assert th2[1] == 1e-4 and 0.01 * 0.01 == 1e-4 and not th2[1] < 1e-4          # the seam itself: the closed form
    assert abs(th2[3] / 1e-4 - 1) < 3e-3 and abs(th2[2] / 1e-4 - 1) < 3e-3 and th2[3] < 1e-4 < th2[2]
    assert max(sc.mags) > 4 and any(abs(m - np.pi) <= 1e-3 and m < np.pi for m in sc.mags) and any(abs(m - np.pi) <= 1e-3 and m > np.pi for m in sc.mags)
    track = np.diff(_field(st, "pt_ptr"))
    assert np.any(track == 0) and np.any(track == 1)
    j = sc.tagged["all"][0]
    assert sorted(sc.cam_idx[sc.pt_idx == j]) == [c for c in range(C) if obs[c] > 0]       # one point seen by every camera that sees anything
    dup = sc.cam_idx[sc.pt_idx == sc.tagged["dup"][0]]
    assert len(dup) == 3 and len(set(dup.tolist())) == 2
    N, P = sc.cam_idx.shape[0], sc.P
    assert N <= 3200
    if sc.variant == "aligned":
        assert N % 256 == 0 and P % 256 == 0
    else:
        assert N % 256 and P % 256 and C % 8
    for d in (10, 6):
        ref = model(sc.x0(d), sc, d)
        assert not np.any(undecided_rows(ref, sc.exact)), "a row the reference cannot assign to a Huber branch"
        linear = float(np.mean(np.abs(ref["f"]) > 1))
        if sc.variant == "mixed":
            assert 0.15 <= linear <= 0.45, linear
        near = np.isin(sc.pt_idx, sc.tagged["near"]); behind = np.isin(sc.pt_idx, sc.tagged["behind"])
        if sc.variant == "plane":
            assert np.all(np.abs(ref["Yz"][near] - 0.05) < 0.005) and near.sum() == 3 and np.all(sc.cam_idx[near] == NEAR_CAM)
            assert np.all(ref["Yz"][behind] < -1) and behind.sum() == 1
            assert np.all(ref["Yz"][~(near | behind)] > 3)
        else:
            assert np.all(ref["Yz"] > 3)
        if sc.variant == "seam":
            # the kernel's own statements with rvec = 0 (a = 1, b = 1/2, r x X = 0): every operation exact, checked in rationals
            cam = sc.cams0[SEAM_CAM]
            assert not np.any(cam[:3]) and tuple(cam[6:]) == K_REF
            fxy, cxy = (K_REF[0], K_REF[1]), (K_REF[2], K_REF[3])
            for k, (_, targets) in zip(sc.seam_obs, SEAM_ROWS):
                X = sc.pts0[sc.pt_idx[k]]
                Y = X + cam[3:6]
                assert all(Fraction(float(Y[i])) == Fraction(float(X[i])) + Fraction(float(cam[3 + i])) for i in range(3)) and Y[2] == 4.0
                iz = 1.0 / Y[2]
                for r in range(2):
                    n_ = Y[r] * iz
                    v1 = fxy[r] * n_; v2 = v1 + cxy[r]; f = v2 - sc.uv[k, r]
                    assert Fraction(float(n_)) == Fraction(float(Y[r])) / 4 and Fraction(float(v1)) == Fraction(fxy[r]) * Fraction(float(n_))
                    assert Fraction(float(v2)) == Fraction(float(v1)) + Fraction(cxy[r]) and Fraction(float(f)) == Fraction(float(v2)) - Fraction(float(sc.uv[k, r]))
                    assert f == targets[r] and float(ref["f"][k, r]) == targets[r] and sc.exact[k, r]
            got = sorted(float(v) for v in np.asarray(ref["f"][sc.seam_obs], dtype=np.float64).ravel())
            assert got == sorted([0.0, 1.0, -1.0, float(np.nextafter(1.0, 2.0)), 2.0, 0.0, 1.0, -1.0])
    if sc.variant == "reg":
        c64 = sc.cams0.astype(np.float64)
        w, fx0 = sc.reg_weight, K_REF[0]
        assert w == 64.0 and (c64[1, 6] - fx0) / fx0 * w == 1.0 and (c64[2, 6] - fx0) / fx0 * w == 2.0       # as k_cam_reg forms them
        fr = reg_rows(sc.cams0, sc)[0]
        assert fr[1, 0] == 1 and fr[2, 0] == 2 and abs(float(fr[3, 1])) > 0.3
        away = np.abs(np.abs(fr) - 1).astype(np.float64)
        away[1, 0] = 1.0
        assert np.all(away > 1e-6), "a regulariser row the reference cannot assign to a Huber branch"
    else:
        assert np.all(np.abs(reg_rows(sc.cams0, sc)[0]) < 0.5)
