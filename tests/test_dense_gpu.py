"""The dense solver on the GPU exactly as the product drives it - dense_cholesky(S | r, n, n + 1) into a workspace that holds
old data, then dense_trsv on what the factorisation left there - with every region of that workspace held to the judges of
tests/dense_reference.py: the factor, the bordered row, the transposed copy, the 128-block inverses in both layouts, both
triangular solves on both routes and the product's composition end to end; at the block and strip seams, on well-conditioned,
graded and kappa2 = 1e12 matrices, and with the failure flag raised at every place a pivot is taken.  The workspace is filled
with finite junk before every call, the strict upper triangle of the input is NaN, guard doubles surround every buffer."""
import ctypes as C

import numpy as np
import pytest

import dense_reference as dr
import stage_reference as sr

pytestmark = pytest.mark.gpu

GUARD = 64                      # doubles before and after the workspace, after the matrix and the vectors
ERR_ARG = -1
REGIONS = ("Ld", "Dinv", "DinvT", "inv64", "flag", "Lm", "LmT", "total")
CASES = [(f, n, s, b) for (f, n, s) in dr.GRID for b in (False, True)]
_families, _factors80 = {}, {}


def fam(name, n):
    if (name, n) not in _families:
        _families[name, n] = dr.family(name, n)
    return _families[name, n]


def layout(n):
    from sfm_amd import _lib
    off = (C.c_int64 * 8)()
    assert _lib.load().sfm_dense_ws_layout(n, off) == 0
    return dict(zip(REGIONS, (int(v) for v in off)))


def junk(count, seed):
    """Finite junk of magnitude up to 1e30 (the product's workspace never holds NaN)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.rand(count, dtype=torch.float64, device="cuda", generator=g) * 2 - 1) * 1e30


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Guarded:
    """A device vector of `count` doubles with GUARD doubles of junk after it (and before it: the workspace)."""
    def __init__(self, count, seed, before=False, fill=None):
        import torch
        self.lo = GUARD if before else 0
        self.count = count
        self.buf = junk(self.lo + count + GUARD, seed)
        if fill is not None:
            self.buf[self.lo:self.lo + count] = torch.from_numpy(np.ascontiguousarray(fill, dtype=np.float64).ravel()).cuda()
        self.before = self.buf[:self.lo].clone()
        self.after = self.buf[self.lo + count:].clone()

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 8 * self.lo)

    def refill(self, seed):
        self.buf[self.lo:self.lo + self.count] = junk(self.count, seed)

    def check(self, what):
        import torch
        assert torch.equal(self.buf[:self.lo].view(torch.int64), self.before.view(torch.int64)), f"{what}: written before its start"
        assert torch.equal(self.buf[self.lo + self.count:].view(torch.int64), self.after.view(torch.int64)), f"{what}: written past its end"

    def host(self):
        return self.buf[self.lo:self.lo + self.count].cpu().numpy()


class Solver:
    """One workspace of the dense solver owned by the test."""
    def __init__(self, n, seed):
        from sfm_amd import _lib
        self.h = _lib.get_handle(0)
        self.n = n
        self.lay = layout(n)
        self.ws = Guarded(self.lay["total"], seed, before=True)

    def flag(self):
        import torch
        at = self.ws.lo + self.lay["flag"]
        return int(self.ws.buf[at:at + 1].view(torch.int32)[0].item())

    def factor(self, A, r=None, junk_seed=None):
        """sfm_dense_factor_ws on the lower triangle of A (NaN above it) and the bordered row r; returns the flag."""
        n = self.n
        nrows = n + (r is not None)
        if junk_seed is not None:
            self.ws.refill(junk_seed)
        a = np.empty((nrows, n))
        a[:n] = np.where(np.tri(n, dtype=bool), A, np.nan)
        if r is not None:
            a[n] = r
        dev = Guarded(nrows * n, 11, fill=a)
        self.h.call("sfm_dense_factor_ws", dev.ptr(), n, nrows, self.ws.ptr())
        dev.check("A"); self.ws.check("workspace")
        self.nrows = nrows
        return self.flag()

    def regions(self):
        """The judged regions on the host: Lm (zero where it is never written), LmT, Dinv, DinvT."""
        n, L = self.n, self.lay
        ws = self.ws.host()
        nb = (n + 127) // 128
        Lm = ws[L["Lm"]:L["Lm"] + self.nrows * n].reshape(self.nrows, n).copy()
        Lm[:n][~np.tri(n, dtype=bool)] = 0.0
        LmT = ws[L["LmT"]:L["LmT"] + n * n].reshape(n, n).copy()
        return dict(Lm=Lm, LmT=LmT, LmT_judged=np.where(dr.lmt_mask(n), LmT, 0.0),
                    Dinv=ws[L["Dinv"]:L["Dinv"] + nb * 128 * 128].reshape(nb, 128, 128).copy(),
                    DinvT=ws[L["DinvT"]:L["DinvT"] + nb * 128 * 128].reshape(nb, 128, 128).copy())

    def solve(self, b, transpose):
        """sfm_dense_trsv_ws; returns (x, flag)."""
        rhs = Guarded(self.n, 12, fill=b)
        x = Guarded(self.n, 13)
        self.h.call("sfm_dense_trsv_ws", self.n, self.ws.ptr(), rhs.ptr(), x.ptr(), transpose)
        rhs.check("b"); x.check("x"); self.ws.check("workspace")
        return x.host(), self.flag()


def set_scheme(monkeypatch, strips):
    if strips:
        monkeypatch.setenv("SFM_CHOL_STRIP_MIN_N", "1")
    else:
        monkeypatch.delenv("SFM_CHOL_STRIP_MIN_N", raising=False)


def set_route(monkeypatch, flow):
    if flow:
        monkeypatch.delenv("SFM_TRSV_FLOW", raising=False)
    else:
        monkeypatch.setenv("SFM_TRSV_FLOW", "0")


def run(monkeypatch, s, A, r, b, junk_seed):
    """Factor and solve as the product composes them; every judged byte."""
    assert s.factor(A, r, junk_seed) == 0, "the failure flag after the factorisation"
    out = s.regions()
    for flow in (True, False):
        set_route(monkeypatch, flow)
        for tr in (0, 1):
            out["x", tr, flow], flag = s.solve(b, tr)
            assert flag == 0, f"the failure flag after the solve (transpose {tr}, flow {flow})"
    set_route(monkeypatch, True)
    if r is not None:
        out["pc"], flag = s.solve(-out["Lm"][s.n], 1)
        assert flag == 0
    return out


BITWISE = ("Lm", "LmT_judged", "Dinv", "DinvT")


def assert_same_bytes(a, b, why):
    for k in a:
        if k in BITWISE or isinstance(k, tuple) or k == "pc":
            assert same_bits(a[k], b[k]), f"{k} differs {why}"


def check(what, case, ratio, where):
    print(f"{what} {case}: {ratio:.3g} of its bound at {where}")
    assert ratio <= 1.0, f"{what}: {ratio:.3g} x its bound at {where} ({case})"


def judge_regions(case, A, r, b, out, solves=True):
    """Judges 1 to 6 on one run's regions; the summary line of the case."""
    n = A.shape[0]
    Lm = out["Lm"]
    assert np.all(np.isfinite(Lm)), "the factor is not finite"
    shown = {}
    shown["factor"] = dr.judge_factor(A, Lm)
    if r is not None:
        shown["row"] = dr.judge_row(Lm, r)
    ri, wi, problems_inv = dr.judge_inverses(Lm, out["Dinv"], out["DinvT"])
    shown["inverses"] = (ri, wi)
    problems_lmt = dr.judge_lmt(Lm, out["LmT"])
    if solves:
        for flow in (True, False):
            for tr in (0, 1):
                shown[f"{'backward' if tr else 'forward'} {'flow' if flow else 'step'}"] = dr.judge_solve(Lm, b, out["x", tr, flow], tr)
    rig = None
    if r is not None and "pc" in out:
        ratio, where, rig = dr.judge_end_to_end(A, r, out["pc"])
        shown["end to end"] = (ratio, where)
    print(f"dense {case}: " + ", ".join(f"{k} {v[0]:.3g}" for k, v in shown.items()) +
          ("" if rig is None else f", rigorous {rig:.3g}") + f"; LmT {'ok' if not problems_lmt else 'BROKEN'}")
    assert problems_lmt == [], problems_lmt
    assert problems_inv == [], problems_inv
    for k, (ratio, where) in shown.items():
        check(k, case, ratio, where)
    if rig is not None:
        assert rig <= 1.0, f"{rig:.3g} x the rigorous (3n + 1) u |L||L^T||p_c| ({case})"


@pytest.mark.parametrize("family,n,strips,bordered", CASES, ids=str)
def test_every_region_against_its_judge(gpu_ready, monkeypatch, family, n, strips, bordered):
    """Judges 1 to 6 on the product path, then the bitwise contracts: other junk in the workspace changes no judged byte, the
    same junk gives the same bytes."""
    A, r, b = fam(family, n)
    if not bordered:
        r = None
    set_scheme(monkeypatch, strips)
    case = f"{family} n={n} {'strips' if strips else 'one-level'} nrows={n + bordered}"
    s = Solver(n, seed=3)
    first = run(monkeypatch, s, A, r, b, junk_seed=4)
    judge_regions(case, A, r, b, first)
    other = run(monkeypatch, s, A, r, b, junk_seed=5)
    assert_same_bytes(first, other, "with other junk in the workspace")
    again = run(monkeypatch, s, A, r, b, junk_seed=4)
    assert_same_bytes(first, again, "between two calls on the same workspace contents")


def factor80(n):
    if n not in _factors80:
        _factors80[n] = sr.chol_lower(fam("well", n)[0])
    return _factors80[n]


@pytest.mark.parametrize("bordered", [False, True], ids=["n", "n+1"])
@pytest.mark.parametrize("n,strips,k", dr.PIVOT_GRID)
def test_failure_flag_wherever_a_pivot_is_taken(gpu_ready, monkeypatch, n, strips, k, bordered):
    """One-level n = 130: k < 64 the two wavefront factors of k_chol_diag, 64 <= k < 128 the look-ahead's, k >= 128 a short last
    block of two columns; strips n = 330: the k_chol_diag of the second strip (after k_syrk_lower), the look-ahead inside it, the
    last column.  The pivot at k is minus what it was: flag 1; half what it was: flag 0 and the factor is good; after a failed
    call the same workspace factors the good matrix."""
    A, r, b = fam("well", n)
    if not bordered:
        r = None
    set_scheme(monkeypatch, strips)
    case = f"well n={n} {'strips' if strips else 'one-level'} nrows={n + bordered} k={k}"
    s = Solver(n, seed=6)
    assert s.factor(dr.with_pivot(A, k, -1, factor80(n)), r, junk_seed=7) == 1
    assert s.factor(A, r) == 0                                   # recovery: what the failed call left is the junk now
    ratio, where = dr.judge_factor(A, s.regions()["Lm"])
    check("factor after a failed call", case, ratio, where)
    half = dr.with_pivot(A, k, 0.5, factor80(n))
    assert s.factor(half, r, junk_seed=8) == 0
    out = s.regions()
    if bordered:
        out["pc"], flag = s.solve(-out["Lm"][n], 1)
        assert flag == 0
    judge_regions(case + " x 0.5", half, r, b, out, solves=False)


@pytest.mark.parametrize("bordered", [False, True], ids=["n", "n+1"])
@pytest.mark.parametrize("value", [0.0, float("nan")], ids=["zero", "nan"])
@pytest.mark.parametrize("n,strips,k", [(130, False, 40), (130, False, 100), (330, True, 40), (330, True, 100)])
def test_failure_flag_on_a_zero_and_a_nan_pivot(gpu_ready, monkeypatch, n, strips, k, value, bordered):
    set_scheme(monkeypatch, strips)
    A, r, _ = fam("well", n)
    E = np.eye(n); E[k, k] = value
    s = Solver(n, seed=9)
    assert s.factor(E, r if bordered else None, junk_seed=10) == 1
    assert s.factor(A, r if bordered else None) == 0
    ratio, where = dr.judge_factor(A, s.regions()["Lm"])
    check("factor after a failed call", f"well n={n} after a {value} pivot at {k}", ratio, where)


def test_argument_checks(gpu_ready):
    import torch
    from sfm_amd import _lib
    lib = _lib.load()
    h = _lib.get_handle(0)._h
    off = (C.c_int64 * 8)()
    assert lib.sfm_dense_ws_layout(0, off) == ERR_ARG and lib.sfm_dense_ws_layout(5, None) == ERR_ARG
    n = 5
    assert layout(n)["total"] == layout(n)["LmT"] + n * n and layout(n)["Ld"] == 0
    t = torch.zeros(layout(n)["total"] + (n + 1) * n + 2 * n, dtype=torch.float64, device="cuda")
    ws = C.c_void_p(t.data_ptr())
    a = C.c_void_p(t.data_ptr() + 8 * layout(n)["total"])
    b = C.c_void_p(a.value + 8 * (n + 1) * n)
    x = C.c_void_p(b.value + 8 * n)
    for args in ((None, a, n, n, ws), (h, None, n, n, ws), (h, a, n, n, None), (h, a, 0, 0, ws), (h, a, 0, 1, ws),
                 (h, a, n, n + 2, ws), (h, a, n, n - 1, ws)):
        assert lib.sfm_dense_factor_ws(*args) == ERR_ARG, args
    for args in ((None, n, ws, b, x, 0), (h, n, None, b, x, 0), (h, n, ws, None, x, 0), (h, n, ws, b, None, 1), (h, 0, ws, b, x, 0)):
        assert lib.sfm_dense_trsv_ws(*args) == ERR_ARG, args
    torch.cuda.synchronize()
    assert not t.any()                                           # a rejected call touches nothing
