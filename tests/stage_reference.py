"""Stage-by-stage reference of the damped solve (sfm_ba_schur_build -> sfm_ba_schur_solve -> sfm_ba_finish_solve) in 80-bit
arithmetic, the error scales each stage is judged by, and the scene builder that puts the edges of the work lists on purpose.

NumPy only (a plain helper module like tests/oracle_backend.py, imported by tests/test_stage_reference.py on the CPU and by
tests/test_ba_stages_gpu.py on the GPU; it never imports the GPU backend).  Every stage is referenced FROM THE INPUTS THAT
STAGE WAS GIVEN - on the GPU the device's own workspace regions - so a stage's bound depends on its own arithmetic and not on
the conditioning of everything before it.  The same formulas run in float64 (dt=np.float64) are the "transcription" the CPU
tests hold to the bounds and seed defects into; its worst ratios are where the non-derivable constants below come from.

Formulas: the kernel comments of sfm_amd/csrc/ba.hip, ba_model.hip, ba_camera_cg.hip and SURVEY.md Appendix D.
  M_j = chol(C_j + alpha I)^-1 (packed m00 m10 m11 m20 m21 m22),  e_j = M_j g_pj
  G_k[m][a] = sum_r Jc~_k[r][a] (Jp~_k M_j^T)[r][m]
  S(c, c2) = [c == c2] B_c - sum_{pairs (k, k2) of the block} G_k^T G_k2      (alpha is NOT in the stored diagonal)
  r_c = g_c - sum_{k of camera c} G_k^T e_j
  p_c = -(S + alpha I)^-1 r
  p_pj = -M_j^T (e_j + sum_{k in track j} G_k p_c[cam k]),  v_j = M_j p_pj
  reduce_q = [q_c | sum ||p_p||^2 | sum ||v||^2],  q_c = -sum_{k of camera c} G_k^T v_j
  PNORM2 = ||p_c||^2 + sum ||p_p||^2,  PQ = sum ||v||^2 + rhs2^T (S + alpha I)^-1 rhs2,  rhs2 = p_c + q_c
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "the stage reference needs an extended-precision np.longdouble (x87 80-bit: 64-bit significand)"
U = 2.0 ** -53                 # unit round-off of the arithmetic under test (float64)
CGS_RTOL = 1e-13               # the library's stated contract of the camera CG: relative residual on the block-scaled system
ITEM_PAIRS = 256               # pairs per Schur work item / observations per camera chunk (sfm_amd/structure.py)
CHUNK_OBS = 256

# ---- tolerances that cannot be derived.  Each is 8 x the worst ratio of the float64 transcription of these formulas to the
# same scale, over every scene / camera block size / alpha of tests/test_stage_reference.py (which re-measures the ratios and
# fails if the transcription exceeds a recorded ratio by more than 2 %): a kernel sums in another order and contracts into FMA / MFMA, which
# changes individual roundings, not the scale.  None was chosen by looking at a GPU result.
C_G = 8 * 1.65                 # G: |G~ - G| <= C_G u kappa2(A_j) ||Jc~_k||_F ||Jp~_k||_F ||M_j||_F; measured ratio 1.65
C_E = 8 * 1.95                 # e_j = M_j g_pj (inside r): |e~ - e| <= C_E u kappa2(A_j) ||M_j||_F ||g_pj||; measured 1.95
C_PP = 8 * 2.13                # p_p: <= C_PP u kappa2(A_j) ||M_j||_F (||M_j||_F ||g_pj|| + sum_k ||G_k||_F ||p_c[cam k]||); measured 2.13
C_V = 8 * 2.03                 # v_j = M_j p_pj (inside q and sum ||v||^2): <= C_V u kappa2(A_j) ||M_j||_F ||p_pj||; measured 2.03
C_FACT = 8 * 0.183             # factorisation route: |rho| <= C_FACT n u (|S + alpha I| |p_c| + |r|); measured 0.183 at n = 12 (2.2 u of
                               # the scale: the factor n overstates small systems), 0.0066 at n = 300 (hand-written column Cholesky
                               # and substitutions in float64)
CG_MARGIN = 8 * 0.875          # CG routes, alpha >= 1e-3 hdiag: ||E^-1 rho|| <= CG_MARGIN 1e-13 ||E^-1 r||; measured 0.875 (float64 CG on
                               # the block-scaled system stopped by its RECURRENCE residual at 1e-13)
CG_MARGIN_FLOOR = 8 * 367      # the same at the small alpha (1e-9 / 1e-6 hdiag, kappa2 up to 1e12): the true residual drifts from the
                               # recurrence by ~ u kappa2(S~) per iteration; measured 367 (3.7e-11) on the scene with a third outliers,
                               # up to 20 on the others.  A contract of 1e-13 on the TRUE residual is not attainable there in float64.
C_PQ = 8 * 0.0945               # PQ: <= C_PQ n u kappa2(S + alpha I) |PQ|; measured 0.0945 (n = 20, kappa2 = 1.1)


def _f(st, name):
    """Field of an index structure given as sfm_amd.structure.BAStructure or as the dict of GpuBA.structure()."""
    return np.asarray(st[name] if isinstance(st, dict) else getattr(st, name), dtype=np.int64)


# ------------------------------------------------------------------------------------------------ point side
def point_factors(Cp6, alpha, dt=LD):
    """M_j = L_j^-1 of L_j L_j^T = C_j + alpha I, packed (m00 m10 m11 m20 m21 m22): the statements of point_factor_vals.
    alpha may be an array [P] (the seeded defect 'alpha left off one point')."""
    c = np.asarray(Cp6).astype(dt)
    a = np.asarray(alpha).astype(dt)
    a00, a10, a20, a11, a21, a22 = c[:, 0] + a, c[:, 1], c[:, 2], c[:, 3] + a, c[:, 4], c[:, 5] + a
    l00 = np.sqrt(a00); l10 = a10 / l00; l20 = a20 / l00
    l11 = np.sqrt(a11 - l10 * l10); l21 = (a21 - l20 * l10) / l11
    l22 = np.sqrt(a22 - l20 * l20 - l21 * l21)
    m00 = 1 / l00; m11 = 1 / l11; m22 = 1 / l22
    m10 = -l10 * m00 * m11; m21 = -l21 * m11 * m22
    m20 = -(l20 * m00 + l21 * m10) * m22
    return np.stack([m00, m10, m11, m20, m21, m22], axis=1)


def unpack_M(M6):
    M = np.zeros((M6.shape[0], 3, 3), dtype=M6.dtype)
    M[:, 0, 0] = M6[:, 0]; M[:, 1, 0] = M6[:, 1]; M[:, 1, 1] = M6[:, 2]
    M[:, 2, 0] = M6[:, 3]; M[:, 2, 1] = M6[:, 4]; M[:, 2, 2] = M6[:, 5]
    return M


def point_kappa(Cp6, alpha):
    """kappa2(C_j + alpha I) per point, from the float64 copy: a scale, not a result."""
    c = np.asarray(Cp6, dtype=np.float64)
    A = np.empty((c.shape[0], 3, 3))
    A[:, 0, 0] = c[:, 0] + alpha; A[:, 1, 1] = c[:, 3] + alpha; A[:, 2, 2] = c[:, 5] + alpha
    A[:, 0, 1] = A[:, 1, 0] = c[:, 1]; A[:, 0, 2] = A[:, 2, 0] = c[:, 2]; A[:, 1, 2] = A[:, 2, 1] = c[:, 4]
    return np.linalg.cond(A)


def _fro(a):
    return np.sqrt(np.sum(np.asarray(a, dtype=np.float64).reshape(a.shape[0], -1) ** 2, axis=1))


def stage_e(M3, gp):
    return np.einsum("pmq,pq->pm", M3, np.asarray(gp).reshape(-1, 3).astype(M3.dtype))


def stage_G(Jc, Jp, M3, pt_idx):
    """G [N][3][d] from the stored Jacobian rows (widened exactly) and the point factors."""
    dt = M3.dtype
    V = np.einsum("nrq,nmq->nrm", np.asarray(Jp).astype(dt), M3[pt_idx])        # V = Jp~ M^T
    return np.einsum("nra,nrm->nma", np.asarray(Jc).astype(dt), V)


# ------------------------------------------------------------------------------------------------ camera side
def stage_S(G, B, st, C, dt=LD, pair_mask=None):
    """(S, T, m): S [n][n] holds every block (c, c2), c2 <= c (the diagonal blocks whole), zero above; T the sum of absolute
    values of the same terms; m [C][C] the pair count of each block.  pair_mask drops pairs (seeded defect)."""
    d = G.shape[2]
    n = C * d
    pk, pk2, bp = _f(st, "pair_k"), _f(st, "pair_k2"), _f(st, "blk_ptr")
    blk = np.repeat(np.arange(bp.shape[0] - 1), np.diff(bp))
    if pair_mask is not None:
        pk, pk2, blk = pk[pair_mask], pk2[pair_mask], blk[pair_mask]
    Gd = np.asarray(G).astype(dt)
    nblk = C * (C + 1) // 2
    tile = np.zeros((nblk, d, d), dtype=dt); tabs = np.zeros((nblk, d, d), dtype=dt)
    step = 4096
    for s in range(0, pk.shape[0], step):              # tile[a][b] = sum_m G_k[m][a] G_k2[m][b], k of camera c <= camera c2 of k2
        a, b = Gd[pk[s:s + step]], Gd[pk2[s:s + step]]
        np.add.at(tile, blk[s:s + step], np.einsum("nma,nmb->nab", a, b))
        np.add.at(tabs, blk[s:s + step], np.einsum("nma,nmb->nab", np.abs(a), np.abs(b)))
    S = np.zeros((n, n), dtype=dt); T = np.zeros((n, n), dtype=dt); m = np.zeros((C, C), dtype=np.int64)
    cnt = np.bincount(blk, minlength=nblk)
    Bd = np.asarray(B).astype(dt)
    for c in range(C):
        for c2 in range(c, C):
            i = c * C - c * (c - 1) // 2 + (c2 - c)
            rs, cs = slice(c2 * d, c2 * d + d), slice(c * d, c * d + d)
            S[rs, cs] = -tile[i].T; T[rs, cs] = tabs[i].T        # row camera c2 >= column camera c: the transpose of the tile
            if c == c2:
                S[rs, cs] += Bd[c]; T[rs, cs] += np.abs(Bd[c])
            m[c2, c] = cnt[i]
    return S, T, m


def cam_reduce(G, vec, base, cam_idx, pt_idx, C, dt=LD, obs_mask=None):
    """out_c = base_c - sum_{k of camera c} G_k^T vec[pt k]  (r with vec = e, base = g_c; q_c with vec = v, base = 0), and the
    sum of absolute values of the terms."""
    d = G.shape[2]
    Gd, vd = np.asarray(G).astype(dt), np.asarray(vec).astype(dt)
    ci, pi = np.asarray(cam_idx), np.asarray(pt_idx)
    if obs_mask is not None:
        Gd, ci, pi = Gd[obs_mask], ci[obs_mask], pi[obs_mask]
    acc = np.zeros((C, d), dtype=dt); aabs = np.zeros((C, d), dtype=dt)
    np.add.at(acc, ci, np.einsum("nma,nm->na", Gd, vd[pi]))
    np.add.at(aabs, ci, np.einsum("nma,nm->na", np.abs(Gd), np.abs(vd[pi])))
    b = np.zeros((C, d), dtype=dt) if base is None else np.asarray(base).reshape(C, d).astype(dt)
    return (b - acc).ravel(), (np.abs(b) + aabs).ravel()


def cam_kappa_term(G, pt_scale, cam_idx, pt_idx, C):
    """K_c[a] = sum_{k of camera c} sum_m |G_k[m][a]| pt_scale[pt k]: what an error of pt_scale per component of vec does to out_c."""
    d = G.shape[2]
    K = np.zeros((C, d))
    np.add.at(K, np.asarray(cam_idx), np.abs(np.asarray(G, dtype=np.float64)).sum(axis=1) * pt_scale[np.asarray(pt_idx)][:, None])
    return K.ravel()


def stage_pp(G, M3, e, pc, cam_idx, pt_idx, P):
    """p_p [P][3] and v = M p_p from the step's camera part."""
    dt = M3.dtype
    d = G.shape[2]
    t = np.einsum("nma,na->nm", np.asarray(G).astype(dt), np.asarray(pc).astype(dt).reshape(-1, d)[cam_idx])
    u = np.array(e, dtype=dt)
    np.add.at(u, np.asarray(pt_idx), t)
    return -np.einsum("pmq,pm->pq", M3, u)


def stage_v(M3, pp):
    return np.einsum("pmq,pq->pm", M3, np.asarray(pp).reshape(-1, 3).astype(M3.dtype))


# ------------------------------------------------------------------------------------------------ n x n camera system
def chol_lower(A, dt=LD):
    """Column-by-column Cholesky of the lower triangle of A; None if a pivot is not positive."""
    L = np.tril(np.asarray(A).astype(dt))
    n = L.shape[0]
    for j in range(n):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        if not L[j, j] > 0:
            return None
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
    return L


def solve_lower(L, b):
    x = np.array(b, dtype=L.dtype)
    for j in range(L.shape[0]):
        x[j] /= L[j, j]
        x[j + 1:] -= L[j + 1:, j] * x[j]
    return x


def solve_upper_t(L, b):
    """x with L^T x = b."""
    x = np.array(b, dtype=L.dtype)
    for j in range(L.shape[0] - 1, -1, -1):
        x[j] /= L[j, j]
        x[:j] -= L[j, :j] * x[j]
    return x


def sym_from_lower(S, alpha, dt=LD):
    """The symmetric S + alpha I from the stored lower part (the diagonal blocks are read from their lower triangle too)."""
    Sl = np.tril(np.asarray(S).astype(dt))
    A = Sl + np.tril(Sl, -1).T
    A[np.diag_indices_from(A)] += np.asarray(alpha).astype(dt)
    return A


def block_factors(A, C, dt=LD):
    """E_c = chol(A_cc) per camera block, as one block-diagonal lower-triangular matrix (None if a block is not positive)."""
    n = A.shape[0]; d = n // C
    E = np.zeros((n, n), dtype=dt)
    for c in range(C):
        s = slice(c * d, c * d + d)
        Lc = chol_lower(A[s, s], dt)
        if Lc is None:
            return None
        E[s, s] = Lc
    return E


def block_solve(E, b, C):
    """E^-1 b, block by block."""
    n = E.shape[0]; d = n // C
    out = np.array(b, dtype=E.dtype)
    for c in range(C):
        s = slice(c * d, c * d + d)
        out[s] = solve_lower(E[s, s], out[s])
    return out


def pc_alphas(ref_S_at, hdiag):
    """The alphas / hdiag at which p_c is judged: the smallest of 1e-9, 1e-6, 1e-3 at which the 80-bit Cholesky of the reference's
    S + alpha I exists with kappa2 <= 1e12 (d = 6 has no regulariser rows and keeps its gauge directions: its floor case may have
    to move up), then 1e-3 and 10.  ref_S_at(alpha) gives the reference's S of that alpha."""
    for rel in (1e-9, 1e-6, 1e-3):
        A = sym_from_lower(ref_S_at(rel * hdiag), rel * hdiag)
        if chol_lower(A) is not None and np.linalg.cond(A.astype(np.float64)) <= 1e12:
            return sorted({rel, 1e-3, 10.0})
    raise AssertionError("no alpha with a usable camera system")


def cg_scaled_f64(A, r, C, rtol=CGS_RTOL, max_iter=2000):
    """float64 transcription of the camera CG's contract: S~ = E^-1 A E^-T, r~ = E^-1 r, plain CG on S~ x~ = r~ until the
    RECURRENCE residual is below rtol ||r~||, p_c = -E^-T x~.  Returns (p_c, iterations)."""
    A = np.asarray(A, dtype=np.float64); n = A.shape[0]
    E = block_factors(A, C, np.float64)
    Ei = np.linalg.inv(E)
    St = Ei @ A @ Ei.T
    rt = Ei @ np.asarray(r, dtype=np.float64)
    x = np.zeros(n); res = rt.copy(); p = res.copy(); rr = res @ res; rr0 = rr
    it = 0
    while rr > rtol * rtol * rr0 and it < max_iter:
        Ap = St @ p
        a = rr / (p @ Ap)
        x += a * p; res -= a * Ap
        rn = res @ res
        p = res + (rn / rr) * p; rr = rn; it += 1
    return -(Ei.T @ x), it


def transcription(inp, st, C, alpha, dt=np.float64, cg=False, M6=None):
    """The whole chain in float64 (every stage from the float64 result of the one before, as on the device).  inp: dict with
    Jc, Jp, Cp6, gp, gc, B, cam_idx, pt_idx.  Returns a dict of the stage results under the workspace's names."""
    ci, pi = np.asarray(inp["cam_idx"]), np.asarray(inp["pt_idx"])
    P = np.asarray(inp["Cp6"]).shape[0]
    M3 = unpack_M(point_factors(inp["Cp6"], alpha, dt) if M6 is None else M6)
    G = stage_G(inp["Jc"], inp["Jp"], M3, pi)
    S, _, _ = stage_S(G, inp["B"], st, C, dt)
    e = stage_e(M3, inp["gp"])
    r, _ = cam_reduce(G, e, inp["gc"], ci, pi, C, dt)
    A = sym_from_lower(S, alpha, dt)
    L = chol_lower(A, dt)
    out = dict(G=G, S=S, r=r, e=e, M3=M3, L=L)
    if L is None:
        return out
    pc = cg_scaled_f64(A, r, C)[0] if cg else -solve_upper_t(L, solve_lower(L, r))
    pp = stage_pp(G, M3, e, pc, ci, pi, P)
    v = stage_v(M3, pp)
    q, _ = cam_reduce(G, v, None, ci, pi, C, dt)
    redq = np.concatenate([q, [np.sum(pp * pp), np.sum(v * v)]])
    y = solve_lower(L, pc + q)
    out.update(pc=pc, pp=pp, v=v, redq=redq, pnorm2=pc @ pc + redq[-2], pq=redq[-1] + y @ y)
    return out


def measure_e_v(Cp6, gp, alpha, e_got, pp, v_got):
    """Raw ratios (no constant) of e_j and v_j to u kappa2(A_j) ||M_j||_F ||input||: where C_E and C_V come from."""
    M3 = unpack_M(point_factors(Cp6, alpha))
    ks = point_kappa(Cp6, alpha) * _fro(M3)
    out = []
    for ref, got, vec in ((stage_e(M3, gp), e_got, gp), (stage_v(M3, pp), v_got, pp)):
        scale = U * ks * _fro(np.asarray(vec).reshape(-1, 3))
        err = np.max(np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64), axis=1)
        assert np.all(err[scale == 0] == 0)
        out.append(float(np.max(np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), 0.0))))
    return out


# ------------------------------------------------------------------------------------------------ judges
# Each returns the worst ratio of |result - reference| to the stage's bound (<= 1 passes) and a description of where.
def judge_G(Jc, Jp, Cp6, pt_idx, alpha, G_got):
    pt_idx = np.asarray(pt_idx)
    M3 = unpack_M(point_factors(Cp6, alpha))
    ref = stage_G(Jc, Jp, M3, pt_idx)
    scale = (point_kappa(Cp6, alpha) * _fro(M3))[pt_idx] * _fro(Jc) * _fro(Jp)
    err = np.max(np.abs(np.asarray(G_got).astype(LD) - ref).astype(np.float64).reshape(ref.shape[0], -1), axis=1)
    zero = scale == 0
    assert np.all(err[zero] == 0), "a G block whose scale is zero must be exactly zero"
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, C_G * U * scale))
    k = int(np.argmax(ratio))
    return float(ratio[k]), f"observation {k} (point {int(pt_idx[k])}, kappa {point_kappa(Cp6, alpha)[pt_idx[k]]:.3g})"


def judge_S(G, B, st, C, S_got, pair_mask=None):
    """Componentwise |S~ - S| <= (3m + 2) u T (derived: an inner product of 3m + 1 terms in any order).  Blocks without pairs
    and everything above the diagonal blocks must be exactly zero or, above the diagonal, the exact transpose."""
    d = G.shape[2]; n = C * d
    S, T, m = stage_S(G, B, st, C)
    got = np.asarray(S_got, dtype=np.float64).reshape(n, n)
    cam = np.arange(n) // d
    low = cam[:, None] >= cam[None, :]
    bound = ((3 * m + 2)[cam[:, None], cam[None, :]] * U * T.astype(np.float64))
    err = np.abs(got.astype(LD) - S).astype(np.float64)
    problems = []
    zero = low & (bound == 0)
    if np.any(got[zero] != 0):
        i, j = np.argwhere(zero & (got != 0))[0]
        problems.append(f"S[{i}][{j}] = {got[i, j]!r} where the structure says exactly 0 (block ({cam[i]}, {cam[j]}))")
    up = ~low
    mirror_ok = (got == 0) | (got == got.T)
    if not np.all(mirror_ok[up]):
        i, j = np.argwhere(up & ~mirror_ok)[0]
        problems.append(f"S[{i}][{j}] above the diagonal is neither absent nor the exact transpose")
    ratio = np.where(low & (bound > 0), err / np.where(bound > 0, bound, 1.0), 0.0)
    i, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    ip = _f(st, "item_ptr")
    c, c2 = int(cam[i]), int(cam[j])
    bi = c2 * C - c2 * (c2 - 1) // 2 + (c - c2)
    where = f"block ({c}, {c2}): {int(m[c, c2])} pairs in {int(ip[bi + 1] - ip[bi])} items, entry [{i % d}][{j % d}]"
    return float(ratio[i, j]), where, problems


def _cam_counts(cam_idx, C, d):
    return np.repeat(np.bincount(np.asarray(cam_idx), minlength=C), d)


def judge_r(G, Cp6, gp, gc, alpha, cam_idx, pt_idx, C, r_got, obs_mask=None):
    """|r~ - r| <= u ((3m + 2) T + C_E K): the derived inner-product bound over the camera's m observations plus what the
    kappa-scaled error of e_j = M_j g_pj does through |G_k|."""
    M3 = unpack_M(point_factors(Cp6, alpha))
    e = stage_e(M3, gp)
    ref, T = cam_reduce(G, e, gc, cam_idx, pt_idx, C)
    e_scale = point_kappa(Cp6, alpha) * _fro(M3) * _fro(np.asarray(gp).reshape(-1, 3))
    K = cam_kappa_term(G, e_scale, cam_idx, pt_idx, C)
    return _judge_vec(ref, T, K, C_E, cam_idx, C, G.shape[2], r_got, "r")


def _judge_vec(ref, T, K, const, cam_idx, C, d, got, what):
    mcount = _cam_counts(cam_idx, C, d)
    bound = U * ((3 * mcount + 2) * T.astype(np.float64) + const * K)
    err = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
    zero = bound == 0
    assert np.all(err[zero] == 0), f"entries of {what} whose scale is zero must be exactly zero"
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, bound))
    i = int(np.argmax(ratio))
    return float(ratio[i]), f"{what}[{i}] (camera {i // d}, {int(mcount[i])} observations, {-(-int(mcount[i]) // CHUNK_OBS)} chunks)"


def judge_pc_factor(S_got, r_got, alpha, pc_got):
    """Factorisation route: |rho| <= C_FACT n u (|S + alpha I| |p_c| + |r|), rho = r + (S + alpha I) p_c in 80 bits."""
    A = sym_from_lower(S_got, alpha)
    n = A.shape[0]
    pc, r = np.asarray(pc_got).astype(LD), np.asarray(r_got).astype(LD)
    rho = np.abs(r + A @ pc).astype(np.float64)
    scale = (np.abs(A) @ np.abs(pc) + np.abs(r)).astype(np.float64)
    zero = scale == 0
    assert np.all(rho[zero] == 0), "entries of the residual whose scale is zero must be exactly zero"
    ratio = np.where(zero, 0.0, rho / np.where(zero, 1.0, C_FACT * n * U * scale))
    i = int(np.argmax(ratio))
    return float(ratio[i]), f"row {i} of the camera system (n = {n})"


def factor_rigorous_ratio(S_got, r_got, alpha, pc_got):
    """The same residual against the rigorous worst case of a Cholesky solve, (3n + 1) u |L| |L^T| |p_c| with the reference's
    factor: above 1 is a bug whatever the operation order."""
    A = sym_from_lower(S_got, alpha)
    n = A.shape[0]
    L = chol_lower(A)
    assert L is not None
    pc, r = np.asarray(pc_got).astype(LD), np.asarray(r_got).astype(LD)
    rho = np.abs(r + A @ pc).astype(np.float64)
    bound = ((3 * n + 1) * U * (np.abs(L) @ (np.abs(L).T @ np.abs(pc)))).astype(np.float64)
    ok = bound > 0
    return float(np.max(rho[ok] / bound[ok])) if np.any(ok) else 0.0


def cg_margin(floor):
    return CG_MARGIN_FLOOR if floor else CG_MARGIN


def judge_pc_cg(S_got, r_got, alpha, pc_got, C, floor=False):
    """CG routes: ||E^-1 rho||_2 <= CG_MARGIN 1e-13 ||E^-1 r||_2 with the reference's own factors E_c = chol(S_cc + alpha I)."""
    A = sym_from_lower(S_got, alpha)
    E = block_factors(A, C)
    assert E is not None, "a diagonal block of S + alpha I is not positive definite"
    pc, r = np.asarray(pc_got).astype(LD), np.asarray(r_got).astype(LD)
    num = np.sqrt(np.sum(block_solve(E, r + A @ pc, C) ** 2))
    den = np.sqrt(np.sum(block_solve(E, r, C) ** 2))
    rel = float(num / den)
    return rel / (cg_margin(floor) * CGS_RTOL), f"relative residual {rel:.3e} on the block-scaled system"


def judge_pp(G, Cp6, gp, alpha, pc, cam_idx, pt_idx, pp_got):
    cam_idx, pt_idx = np.asarray(cam_idx), np.asarray(pt_idx)
    P = np.asarray(Cp6).shape[0]; d = G.shape[2]
    M3 = unpack_M(point_factors(Cp6, alpha))
    ref = stage_pp(G, M3, stage_e(M3, gp), pc, cam_idx, pt_idx, P)
    Mn = _fro(M3)
    inner = Mn * _fro(np.asarray(gp).reshape(-1, 3))
    np.add.at(inner, pt_idx, _fro(G) * _fro(np.asarray(pc, dtype=np.float64).reshape(-1, d))[cam_idx])
    scale = point_kappa(Cp6, alpha) * Mn * inner
    err = np.max(np.abs(np.asarray(pp_got).reshape(-1, 3).astype(LD) - ref).astype(np.float64), axis=1)
    zero = scale == 0
    assert np.all(err[zero] == 0), "a point step whose scale is zero must be exactly zero"
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, C_PP * U * scale))
    j = int(np.argmax(ratio))
    return float(ratio[j]), f"point {j} (track of {int(np.sum(pt_idx == j))}, kappa {point_kappa(Cp6, alpha)[j]:.3g})"


def judge_q(G, Cp6, alpha, pp, cam_idx, pt_idx, C, redq_got):
    """reduce_q = [q_c (n) | sum ||p_p||^2 | sum ||v||^2] from the device's G and p_p.  Returns the three ratios."""
    d = G.shape[2]; n = C * d
    pp3 = np.asarray(pp).reshape(-1, 3)
    P = pp3.shape[0]
    M3 = unpack_M(point_factors(Cp6, alpha))
    v = stage_v(M3, pp3)
    v_scale = point_kappa(Cp6, alpha) * _fro(M3) * _fro(pp3)
    ref, T = cam_reduce(G, v, None, cam_idx, pt_idx, C)
    K = cam_kappa_term(G, v_scale, cam_idx, pt_idx, C)
    got = np.asarray(redq_got, dtype=np.float64)
    rq, where = _judge_vec(ref, T, K, C_V, cam_idx, C, d, got[:n], "q")
    pp2 = np.sum(pp3.astype(LD) ** 2)
    rp = float(abs(LD(got[n]) - pp2)) / max(float((3 * P + 2) * U * pp2), 1e-300)
    v2 = np.sum(v ** 2)
    bound_v = U * ((3 * P + 2) * float(v2) + 2.5 * C_V * float(np.sum(v_scale * np.sum(np.abs(v), axis=1).astype(np.float64))))
    rv = float(abs(LD(got[n + 1]) - v2)) / max(bound_v, 1e-300)
    return rq, rp, rv, where


def judge_scalars(S_got, alpha, pc, redq_got, pnorm2, pq, cg, floor=False):
    """PNORM2 = ||p_c||^2 + sum ||p_p||^2 and PQ = sum ||v||^2 + rhs2^T (S + alpha I)^-1 rhs2 as k_finish_solve combines them,
    from the device's p_c and reduce_q; the second term by an 80-bit solve with the device's S.  Its bound is kappa-scaled
    (C_PQ n u kappa2); on the CG routes the second system is solved to the CG contract too, whose error in the quadratic form
    is at most kappa2(S~) 1e-13 (kappa2(S~) <= kappa2(S + alpha I) up to the block scaling: the same scale is used)."""
    n = np.asarray(pc).shape[0]
    got = np.asarray(redq_got, dtype=np.float64)
    pcl = np.asarray(pc).astype(LD)
    pn_ref = np.sum(pcl ** 2) + LD(got[n])
    r_pn = float(abs(LD(pnorm2) - pn_ref)) / float((n + 3) * U * pn_ref)
    A = sym_from_lower(S_got, alpha)
    L = chol_lower(A)
    assert L is not None
    rhs2 = (np.asarray(pc, dtype=np.float64) + got[:n]).astype(LD)        # k_add_vec: one float64 rounding per entry
    y = solve_lower(L, rhs2)
    quad = np.sum(y ** 2)
    kappa = float(np.linalg.cond(A.astype(np.float64)))
    total = quad + LD(got[n + 1])
    bound = (C_PQ * n * U + (cg_margin(floor) * CGS_RTOL if cg else 0.0)) * kappa * float(total)
    r_pq = float(abs(LD(pq) - total)) / bound
    return r_pn, r_pq, kappa


# ------------------------------------------------------------------------------------------------ scenes with the edges on purpose
class EdgeScene:
    """cams0 [C][10], pts0 [P][3], point-major observations (cam_idx, pt_idx, uv), the named blocks {(a, b): pairs} and cameras
    {c: observations} the scene was built to contain."""
    def __init__(self, **kw):
        self.__dict__.update(kw)


NAMED_BLOCKS = {(0, 1): 1, (0, 2): 255, (1, 2): 256, (0, 3): 257, (1, 3): 512, (2, 3): 513}


def edge_scene(variant="edge", seed=7, noise_px=0.3, pt_sigma=5e-4, cam_sigma=5e-5):
    """Two-camera tracks give block (a, b) exactly the pair count asked for; longer tracks on other cameras pad the scene.
    variants:
      edge     11 cameras (not a multiple of 8): blocks of 1 / 255 / 256 / 257 / 512 / 513 pairs, cameras of 256, 257, 1,024 and
               1,282 observations, camera 7 without any, an empty track, a single-observation track; N and P with remainders
      aligned  the same with N % 256 == 0 and P % 256 == 0
      dup      the same plus tracks that hold camera 8 twice (the has_dup route)
      mixed    the same with a third of the observations 4 px off (Huber-linear rows)
      c2, c5   2 / 5 cameras (C = 5 leaves XCD groups empty)
      tile30, tile45   the named blocks plus filler cameras up to 30 / 45: n = C d >= 257 for the tile-streaming CG route
    """
    from sfm_amd import synth
    rng = np.random.default_rng(seed)
    tracks = []                                      # tuples of cameras, one per point ( () = empty track )
    named_cams = {}
    if variant == "c2":
        C, blocks = 2, {(0, 1): 257}
        tracks += [(0,), ()]
    elif variant == "c5":
        C, blocks = 5, {(0, 1): 1, (0, 2): 255, (1, 2): 256, (0, 3): 257, (1, 3): 513}
        tracks += [(2, 3, 4)] * 40 + [(4,), ()]
    else:
        C = {"tile30": 30, "tile45": 45}.get(variant, 11)
        blocks = dict(NAMED_BLOCKS)
        blocks.update({(4, 5): 100, (4, 6): 156, (5, 6): 157})       # camera 4: 256 observations, camera 5: 257
        named_cams = {0: 513, 1: 769, 2: 1024, 3: 1282, 4: 256, 5: 257, 7: 0}
        tracks += [(6, 8, 9, 10)] * 60 + [(8, 9, 10)] * 50 + [(6, 9, 10)] * 30 + [(8,), ()]
        if variant == "dup":
            tracks += [(8, 8, 9)] * 20 + [(8, 9, 9, 10)] * 5
        for c in range(11, C):                       # filler cameras: three-camera tracks among themselves
            tracks += [tuple(sorted({c, 11 + (c - 11 + 1) % (C - 11), 11 + (c - 11 + 5) % (C - 11)}))] * 12
    for (a, b), cnt in blocks.items():
        tracks += [(a, b)] * cnt
    order = rng.permutation(len(tracks))             # the tracks of a block are spread over the point ids
    tracks = [tracks[i] for i in order]
    if variant == "aligned":
        while (sum(len(t) for t in tracks) % 256) or (len(tracks) % 256):
            n_obs = sum(len(t) for t in tracks)
            tracks.append((9,) if n_obs % 2 else (9, 10) if n_obs % 256 else ())
    P = len(tracks)
    cam_idx = np.array([c for t in tracks for c in t], dtype=np.int64)
    pt_idx = np.repeat(np.arange(P, dtype=np.int64), [len(t) for t in tracks])
    full = synth.make_scene(C, P, obs_per_point=None, seed=seed, noise_px=noise_px, pt_sigma=pt_sigma, cam_sigma=cam_sigma)
    uv = full.uv[pt_idx * C + cam_idx].copy()
    if variant == "mixed":
        out = rng.random(uv.shape[0]) < 1.0 / 3.0
        uv[out] += rng.normal(0.0, 4.0, size=(int(out.sum()), 2))
        uv = uv.astype(np.float32).astype(np.float64)
    if variant in ("c2", "c5"):
        named_cams = {int(c): int(np.sum(cam_idx == c)) for c in range(C)}
    return EdgeScene(variant=variant, C=C, P=P, cams0=full.cams0, pts0=full.pts0, cam_idx=cam_idx, pt_idx=pt_idx, uv=uv,
                     blocks=blocks, named_cams=named_cams, K=synth.K_REF)


def block_items(st, C, a, b):
    """(pairs, work items) of block (a <= b) in an index structure."""
    i = a * C - a * (a - 1) // 2 + (b - a)
    return int(np.diff(_f(st, "blk_ptr"))[i]), int(np.diff(_f(st, "item_ptr"))[i])


def assert_edges(scene, st):
    """The edges the scene exists for are really in the index structure: pair counts and item counts of the named blocks, the
    observation and chunk counts of the named cameras, the total item count, an empty and a single-observation track."""
    C = scene.C
    for (a, b), cnt in scene.blocks.items():
        pairs, items = block_items(st, C, a, b)
        assert (pairs, items) == (cnt, -(-cnt // ITEM_PAIRS)), ((a, b), pairs, items)
    obs = np.diff(_f(st, "cam_ptr")); chunks = np.diff(_f(st, "cch_ptr"))
    for c, cnt in scene.named_cams.items():
        assert (int(obs[c]), int(chunks[c])) == (cnt, -(-cnt // CHUNK_OBS)), (c, int(obs[c]), int(chunks[c]))
    n_items = int(np.sum(-(-np.diff(_f(st, "blk_ptr")) // ITEM_PAIRS)))
    assert int(_f(st, "item_ptr")[-1]) == n_items == _f(st, "item_beg").shape[0]
    track = np.diff(_f(st, "pt_ptr"))
    assert np.any(track == 0) and np.any(track == 1)
    if scene.variant in ("edge", "aligned", "dup", "mixed", "tile30", "tile45"):
        got = sorted(block_items(st, C, a, b)[1] for (a, b) in NAMED_BLOCKS)
        assert got == [1, 1, 1, 2, 2, 3]
        assert sorted(int(chunks[c]) for c in (4, 5, 2, 3, 7)) == [0, 1, 2, 4, 6]
