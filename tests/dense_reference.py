"""Reference side of the dense solver's tests (sfm_amd/csrc/dense.hip): the matrix families, the float64 transcription of the
kernel's algebra and the judges every region the factorisation leaves behind is held to.

NumPy only, no GPU (imported by tests/test_dense_reference.py on the CPU and by tests/test_dense_gpu.py on the GPU).  The
judges are evaluated in np.longdouble ON THE OUTPUTS THEY ARE GIVEN - residuals of the factor, the bordered row, the block
inverses and the solves against componentwise scales - so they need no second factorisation and do not move under a diagonal
scaling by powers of two.  The extended-precision factor itself (stage_reference.chol_lower) is only used to place pivots
(with_pivot) and by the end-to-end judge, which is stage_reference's own.

What dense_cholesky leaves in its workspace (dense.h, dense_plan.h), for L L^T = A:
  Lm   [(n + 1)][n]  the lower triangle of L; row n = L^-1 r when the input carried the bordered row r
  LmT  [n][n]        LmT[c][r] = Lm[r][c] for every r and c < 64 floor(r / 64) (the forward solve reads c < 128 floor(r / 128))
  inv64 per 64-block [Li11 0; Li21 Li22],  Li21 = -Li22 (L21 Li11)
  Dinv / DinvT per 128-block [Ai 0; -Ci (B Ai), Ci] and its transpose; identity beyond n
"""
import numpy as np

import stage_reference as sr

LD = sr.LD
U = sr.U

# ---- constants that cannot be derived: the kernel multiplies by explicit inverses of 32, 64 and 128-blocks, so the textbook
# componentwise bounds of a substitution-based Cholesky do not apply as they stand.  As in stage_reference.py each is 8 x the
# worst ratio of the float64 transcription below to the same scale over every (family, n, scheme) of GRID (bordered systems;
# tests/test_dense_reference.py re-measures the ratios and fails if the transcription exceeds a record by more than 2 %): the
# kernel sums in another order and contracts into FMA / MFMA, which changes individual roundings, not the scale.  None was
# chosen by looking at a GPU result.
M_FACTOR = 0.566  # measured on ("well", 1, one-level): entry [0][0]; the factor n + 1 overstates small systems (0.0062 at n = 1030)
M_ROW = 0.0984    # measured on ("floor", 33, one-level): row 0 of L y - r
M_INV = 0.0481    # measured on ("well", 193, one-level): entry [72][4] of Dinv L - I in 128-block 0
M_SOLVE = 0.817   # measured on ("well", 1, one-level), all four solves alike (one product by a rounded inverse); 0.106 at n = 32
C_FACTOR = 8 * M_FACTOR
C_ROW = 8 * M_ROW
C_INV = 8 * M_INV
C_SOLVE = 8 * M_SOLVE

# ---- the grid: (family, n, strips).  One-level sizes: one 32-block and the two halves of a 64-block, a short last block of 1
# and of 63 columns, exact tile edges, even and odd counts of 64-blocks, one to three 128-blocks.  Strips (forced at these
# sizes by SFM_CHOL_STRIP_MIN_N=1): a last strip of one column (257), of one block (320), a strip that ends at n (512), a last
# strip of one block plus one column (577), four strips (1030).
ONE_LEVEL_N = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 300)
STRIP_N = (257, 320, 512, 513, 577, 1030)
HARD_ONE_LEVEL_N = (33, 65, 129, 193, 257, 300)
HARD_STRIP_N = (257, 320, 577)
FAMILIES = ("well", "graded", "floor")
GRID = ([("well", n, False) for n in ONE_LEVEL_N] + [("well", n, True) for n in STRIP_N] +
        [(f, n, False) for f in ("graded", "floor") for n in HARD_ONE_LEVEL_N] +
        [(f, n, True) for f in ("graded", "floor") for n in HARD_STRIP_N])
# where a pivot is taken: (n, strips, k)
PIVOT_GRID = ([(130, False, k) for k in (0, 31, 32, 63, 64, 95, 96, 127, 128, 129)] + [(330, True, k) for k in (256, 300, 329)])


# ------------------------------------------------------------------------------------------------ matrices
def floor_kappa(n):
    """kappa2 of the `floor` family: the project's own limit for the camera solve (stage_reference.pc_alphas) up to n = 320."""
    return 1e12 if n <= 320 else 1e10


def family(name, n, seed=None):
    """(A, r, b): a seeded SPD float64 matrix of the family, the right-hand side of its bordered row and one for the solves.
      well    G G^T + n I: kappa2 a small constant
      graded  D (G G^T + n I) D, D = random powers of two in [2^-20, 1]: kappa2 about 1e12; the scaling is exact, so Cholesky
              and every componentwise judge are invariant under it.  r, b = D x normal
      floor   Q diag(kappa^(-i / (n - 1))) Q^T with a random orthogonal Q, kappa = floor_kappa(n)"""
    rng = np.random.default_rng(1000 * FAMILIES.index(name) + n if seed is None else seed)
    if name in ("well", "graded"):
        G = rng.normal(size=(n, n))
        A = G @ G.T + n * np.eye(n)
        A = np.tril(A) + np.tril(A, -1).T
        r, b = rng.normal(size=n), rng.normal(size=n)
        if name == "graded":
            D = 2.0 ** -rng.integers(0, 21, size=n).astype(np.float64)
            A = D[:, None] * A * D[None, :]
            r, b = D * r, D * b
        return A, r, b
    assert name == "floor" and n >= 33, "the floor spectrum has too few points to mean anything below n = 33"
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    A = (Q * floor_kappa(n) ** (-np.arange(n) / (n - 1.0))) @ Q.T
    A = np.tril(A) + np.tril(A, -1).T
    return A, rng.normal(size=n), rng.normal(size=n)


def first_bad_pivot(A, dt=LD):
    """Index of the first pivot that is not positive in the column Cholesky of the lower triangle of A, or None."""
    L = np.tril(np.asarray(A).astype(dt))
    for j in range(L.shape[0]):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        if not L[j, j] > 0:
            return j
        L[j, j] = np.sqrt(L[j, j])
        L[j + 1:, j] /= L[j, j]
    return None


def with_pivot(A, k, factor, L80=None):
    """A with A[k][k] lowered by (1 - factor) pivot_k, pivot_k = the squared k-th diagonal entry of the 80-bit factor: the exact
    pivot at k becomes factor x pivot_k and every earlier pivot is unchanged.  factor = -1: indefinite exactly at step k."""
    if L80 is None:
        L80 = sr.chol_lower(A)
    out = np.array(A, dtype=np.float64)
    out[k, k] = float(LD(out[k, k]) - (1 - LD(factor)) * L80[k, k] ** 2)
    return out


# ------------------------------------------------------------------------------------------------ float64 transcription
def _chol32(M, fail):
    """wave_chol32: column by column, each column scaled by 1 / sqrt(pivot); a pivot that is not positive is taken as 1."""
    a = np.tril(M).copy()
    L = np.zeros((32, 32)); rinv = np.zeros(32)
    for j in range(32):
        piv = a[j, j]
        if not piv > 0.0:
            fail[0] = 1
            piv = 1.0
        rinv[j] = 1.0 / np.sqrt(piv)
        L[j:, j] = a[j:, j] * rinv[j]
        a[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return L, rinv


def _inv32(L, rinv):
    """wave_inv32_follow: forward substitution of every unit vector in outer-product order."""
    acc = np.zeros((32, 32)); Li = np.zeros((32, 32)); eye = np.eye(32)
    for j in range(32):
        x = np.where(np.arange(32) <= j, (eye[j] - acc[j]) * rinv[j], 0.0)
        Li[j] = x
        acc[j + 1:] += np.outer(L[j + 1:, j], x)
    return Li


def _crit64(M, fail):
    """crit64_lite on an identity-padded 64x64 tile: (L, step data [Li11 0; L21 Li22])."""
    L11, r1 = _chol32(M[:32, :32], fail)
    Li11 = _inv32(L11, r1)
    L21 = M[32:, :32] @ Li11.T
    L22, r2 = _chol32(M[32:, 32:] - L21 @ L21.T, fail)
    Li22 = _inv32(L22, r2)
    L = np.zeros((64, 64)); D = np.zeros((64, 64))
    L[:32, :32] = L11; L[32:, :32] = L21; L[32:, 32:] = L22
    D[:32, :32] = Li11; D[32:, :32] = L21; D[32:, 32:] = Li22
    return L, D


def _panel(Ap, D):
    """trsm_rows16: the rows Ap [m][nb] of a panel against the step data, in two 32-wide stages."""
    m, nb = Ap.shape
    P = np.zeros((m, 64)); P[:, :nb] = Ap
    X1 = P[:, :32] @ D[:32, :32].T
    X2 = (P[:, 32:] - X1 @ D[32:, :32].T) @ D[32:, 32:].T
    return np.concatenate([X1, X2], axis=1)


def _padded(Lm, n):
    """The rows 0 .. n - 1 of the factor, zero beyond n up to whole 128-blocks (the kernels read rows past n as zero)."""
    N = (n + 127) // 128 * 128
    Lp = np.zeros((N, N))
    Lp[:n, :n] = np.nan_to_num(np.tril(np.asarray(Lm)[:n]))
    return Lp


def merge_inverses(Lm, inv64, n):
    """k_inv_merge: (Dinv, DinvT) [ceil(n / 128)][128][128] from the factor and the 64-block inverses."""
    nb128 = (n + 127) // 128
    Lp = _padded(Lm, n)
    Dinv = np.zeros((nb128, 128, 128))
    for b in range(nb128):
        r0 = b * 128
        Ai, Ci = inv64[2 * b], inv64[2 * b + 1]
        Dinv[b, :64, :64] = Ai; Dinv[b, 64:, 64:] = Ci
        Dinv[b, 64:, :64] = -(Ci @ (Lp[r0 + 64:r0 + 128, r0:r0 + 64] @ Ai))
    return Dinv, np.ascontiguousarray(np.transpose(Dinv, (0, 2, 1)))


def fix_inv64(Lm, inv64, n, sign=-1.0, only=None):
    """k_inv64_fix: Li21 = -Li22 (L21 Li11) of every 64-block (sign / only: the seeded defect of a wrong sign in one block)."""
    Lp = _padded(Lm, n)
    for b in range((n + 63) // 64):
        r0 = b * 64
        s = -sign if only == b else sign
        inv64[b, 32:, :32] = s * (inv64[b, 32:, 32:] @ (Lp[r0 + 32:r0 + 64, r0:r0 + 32] @ inv64[b, :32, :32]))


def factor_f64(A, r=None, strips=False):
    """dense_cholesky in float64 NumPy, launch by launch as for_each_chol_launch schedules it: 64-column panels whose diagonal
    block is factored as two 32-blocks with their explicit inverses, the two-stage panel solve against the step data, the
    trailing update (strips: only inside the 256-column strip, then one rank-256 update of the rest), the block inverses.
    Returns a dict of the workspace regions (Lm with the bordered row when r is given, unwritten entries NaN in Lm / LmT)
    and `flag`."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    nrows = n + (r is not None)
    W = np.zeros((nrows, n)); W[:n] = np.tril(A)
    if r is not None:
        W[n] = r
    Lm = np.full((nrows, n), np.nan); LmT = np.full((n, n), np.nan)
    nb128 = (n + 127) // 128
    inv64 = np.zeros((2 * nb128, 64, 64))
    fail = [0]

    def diag(j):
        nb = min(64, n - j)
        M = np.eye(64); M[:nb, :nb] = np.tril(W[j:j + nb, j:j + nb])
        L, D = _crit64(M, fail)
        Lm[j:j + nb, j:j + nb] = np.where(np.tri(nb, dtype=bool), L[:nb, :nb], np.nan)
        inv64[j // 64, :32, :32] = D[:32, :32]; inv64[j // 64, 32:, 32:] = D[32:, 32:]
        return D

    strip = 256 if strips else n
    for jb in range(0, n, strip):
        je = min(jb + strip, n)
        D = diag(jb)
        for j0 in range(jb, je, 64):
            nb = min(64, n - j0); j1 = j0 + nb
            if nrows - j1 <= 0:
                break
            X = _panel(W[j1:nrows, j0:j1], D)
            Lm[j1:nrows, j0:j1] = X[:, :nb]
            LmT[j0:j1, j1:n] = X[:n - j1, :nb].T
            if je - j1 > 0:
                W[j1:nrows, j1:je] -= X @ X[:je - j1].T
                D = diag(j1)
        if je < n:
            W[je:nrows, je:n] -= Lm[je:nrows, jb:je] @ Lm[je:n, jb:je].T
    fix_inv64(Lm, inv64, n)
    if ((n + 63) // 64) & 1:
        inv64[(n + 63) // 64] = np.eye(64)
    Dinv, DinvT = merge_inverses(Lm, inv64, n)
    return dict(n=n, Lm=Lm, LmT=LmT, inv64=inv64, Dinv=Dinv, DinvT=DinvT, flag=fail[0])


def solve_f64(F, b, transpose, flow=True):
    """dense_trsv in float64 NumPy with the regions of factor_f64: block g's unknowns are Dinv_g(^T) times what is left of
    its right-hand side.  flow: k_trsv_flow (every block sums the other blocks' contributions itself, the forward one from
    LmT); else k_trsv_step (each solved block is subtracted from the rows still open)."""
    n = F["n"]
    L = np.nan_to_num(F["Lm"][:n]); LT = F["LmT"]
    nblk = (n + 127) // 128
    x = np.zeros(n); b = np.array(b, dtype=np.float64)
    order = range(nblk - 1, -1, -1) if transpose else range(nblk)
    for g in order:
        r0 = g * 128; nbg = min(128, n - r0)
        rhs = np.zeros(128); rhs[:nbg] = b[r0:r0 + nbg]
        if flow:
            part = np.zeros(nbg)
            for blk in (range(nblk - 1, g, -1) if transpose else range(g)):
                rb = blk * 128; nbb = min(128, n - rb)
                tile = L[rb:rb + nbb, r0:r0 + nbg].T if transpose else LT[rb:rb + nbb, r0:r0 + nbg].T
                part += tile @ x[rb:rb + nbb]
            rhs[:nbg] -= part
        M = F["Dinv"][g] if transpose else F["DinvT"][g]            # x[r] = sum_c M[c][r] rhs[c]
        xg = (M.T @ rhs)[:nbg]
        x[r0:r0 + nbg] = xg
        if not flow:
            if transpose:
                b[:r0] -= L[r0:r0 + nbg, :r0].T @ xg
            elif r0 + 128 < n:                                       # rows behind a block: the block is full
                b[r0 + 128:] -= L[r0 + 128:, r0:r0 + 128] @ xg
    return x


# ------------------------------------------------------------------------------------------------ judges
# Each returns (worst ratio of error to bound - <= 1 passes -, where).  An entry whose scale is zero must be exact.
def _worst(err, scale, const, what):
    err = np.asarray(err, dtype=np.float64); scale = np.asarray(scale, dtype=np.float64)
    assert np.all(np.isfinite(err)), f"{what}: the result is not finite"
    zero = scale == 0
    assert np.all(err[zero] == 0), f"{what}: an entry whose scale is zero must have no error"
    ratio = np.where(zero, 0.0, err / np.where(zero, 1.0, const * scale))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[i]), i


def lower_of(Lm, n):
    """The factor proper: the lower triangle of rows 0 .. n - 1 of Lm (what lies above it is never written)."""
    return np.where(np.tri(n, dtype=bool), np.asarray(Lm, dtype=np.float64)[:n], 0.0)


def _llt_lower(L):
    """L L^T in 80 bits, block row by block row, the lower part only."""
    n = L.shape[0]
    Ll = L.astype(LD)
    out = np.zeros((n, n), dtype=LD)
    for i0 in range(0, n, 128):
        i1 = min(i0 + 128, n)
        out[i0:i1, :i1] = Ll[i0:i1, :i1] @ Ll[:i1, :i1].T
    return out


def judge_factor(A, Lm):
    """|A - L L^T|_ij <= C_FACTOR (n + 1) u (|L| |L|^T)_ij for i >= j; A the symmetric matrix of the input's lower part."""
    n = A.shape[0]
    L = lower_of(Lm, n)
    low = np.tri(n, dtype=bool)
    err = np.where(low, np.abs(np.tril(A).astype(LD) - _llt_lower(L)).astype(np.float64), 0.0)
    scale = np.where(low, (n + 1) * U * (np.abs(L) @ np.abs(L).T), 0.0)
    ratio, (i, j) = _worst(err, scale, C_FACTOR, "factor")
    return ratio, f"entry [{i}][{j}] of A - L L^T (n = {n})"


def judge_row(Lm, r):
    """The bordered row y = row n of Lm: |L y - r| <= C_ROW n u |L| |y|."""
    n = Lm.shape[1]
    L = lower_of(Lm, n)
    y = np.asarray(Lm, dtype=np.float64)[n]
    err = np.abs(L.astype(LD) @ y.astype(LD) - np.asarray(r).astype(LD))
    ratio, (i,) = _worst(err, n * U * (np.abs(L) @ np.abs(y)), C_ROW, "bordered row")
    return ratio, f"row {i} of L y - r (n = {n})"


def lmt_mask(n):
    """[c][r] of LmT the factorisation writes: every row r of the factor and every column c < 64 floor(r / 64) (the forward
    k_trsv_flow reads the subset c < 128 floor(r / 128))."""
    return np.arange(n)[:, None] < 64 * (np.arange(n)[None, :] // 64)


def judge_lmt(Lm, LmT):
    """The transposed copy, bit for bit.  Returns the list of problems."""
    n = Lm.shape[1]
    m = lmt_mask(n)
    want = np.asarray(Lm, dtype=np.float64)[:n].T
    got = np.asarray(LmT, dtype=np.float64)
    bad = m & (want.view(np.int64) != got.view(np.int64))
    if not bad.any():
        return []
    c, r = np.argwhere(bad)[0]
    return [f"LmT[{c}][{r}] = {got[c, r]!r} is not Lm[{r}][{c}] = {want[c, r]!r} ({int(bad.sum())} entries differ, 64-block ({r // 64}, {c // 64}))"]


def judge_inverses(Lm, Dinv, DinvT):
    """Every 128-block g: |X L_gg - I| <= C_INV 128 u |X| |L_gg| with X = Dinv_g and L_gg identity-padded beyond n; DinvT_g the
    transpose bit for bit, the strict upper triangle zero, identity beyond n.  Returns (ratio, where, problems)."""
    n = Lm.shape[1]
    L = lower_of(Lm, n)
    Dinv = np.asarray(Dinv, dtype=np.float64); DinvT = np.asarray(DinvT, dtype=np.float64)
    worst, where, problems = 0.0, "", []
    for g in range((n + 127) // 128):
        r0 = g * 128; nbg = min(128, n - r0)
        X = Dinv[g]
        Lg = np.eye(128); Lg[:nbg, :nbg] = L[r0:r0 + nbg, r0:r0 + nbg]
        differ = np.ascontiguousarray(X.T).view(np.int64) != np.ascontiguousarray(DinvT[g]).view(np.int64)
        if differ.any():
            c, r_ = np.argwhere(differ)[0]
            problems.append(f"DinvT[{g}][{c}][{r_}] is not Dinv[{g}][{r_}][{c}] bit for bit")
        if np.any(np.triu(X, 1) != 0):
            problems.append(f"Dinv[{g}] has a non-zero above its diagonal")
        pad = np.eye(128); pad[:nbg, :nbg] = X[:nbg, :nbg]
        if not np.array_equal(X, pad):                       # -0.0 == 0.0: k_inv_merge negates an exact zero there
            problems.append(f"Dinv[{g}] is not the identity beyond n (block of {nbg})")
        err = np.abs(X.astype(LD) @ Lg.astype(LD) - np.eye(128, dtype=LD))
        ratio, (i, j) = _worst(err, 128 * U * (np.abs(X) @ np.abs(Lg)), C_INV, "block inverse")
        if ratio >= worst:
            worst, where = ratio, f"entry [{i}][{j}] of Dinv L - I in 128-block {g} of {nbg} rows (n = {n})"
    return worst, where, problems


def judge_solve(Lm, b, x, transpose):
    """Backward: |L^T x - b| <= C_SOLVE n u |L|^T |x|; forward: |L y - b| <= C_SOLVE n u |L| |y|."""
    n = Lm.shape[1]
    L = lower_of(Lm, n)
    T = L.T if transpose else L
    x = np.asarray(x, dtype=np.float64)
    err = np.abs(T.astype(LD) @ x.astype(LD) - np.asarray(b).astype(LD))
    ratio, (i,) = _worst(err, n * U * (np.abs(T) @ np.abs(x)), C_SOLVE, "solve")
    return ratio, f"row {i} of {'L^T x - b' if transpose else 'L y - b'} (n = {n})"


def judge_end_to_end(A, r, pc):
    """The product's composition - p_c = the backward solve of the negated bordered row - by stage_reference's own judges of
    the factorisation route, with the constants they carry: (ratio to C_FACT's bound, where, ratio to the rigorous bound)."""
    ratio, where = sr.judge_pc_factor(np.tril(A), r, 0.0, pc)
    return ratio, where, sr.factor_rigorous_ratio(np.tril(A), r, 0.0, pc)
