"""An exact reference for the matcher's float32 L2 and Hamming paths (k_knn2_valu + k_merge_splits in
sfm_amd/csrc/match.hip), and the judge that holds any (idx1, idx2, d1, d2) to it: tests/test_matcher_truth.py on the
CPU (oracle/matcher_oracle.py is the implementation under test there), tests/test_matcher_truth_gpu.py on the device.
Plain NumPy; it shares no routine with the oracle or the kernel and fixes no summation order.

Exact distances.  L2: the float32 inputs widened to float64, sum_k (a_k - b_k)^2, then sqrt.  A difference of two
float32 values is exact in float64 unless their exponents lie more than 29 apart, and is then rounded once at 2^-53;
the squares and the dim - 1 adds round at 2^-53 each.  E is therefore off by at most (dim + 2) 2^-53 relative:
5e-9 of the tolerance below, which is why it may be called exact.  Hamming: x = a ^ b, np.unpackbits, an integer sum.

Tolerance (derived, not measured; it holds for ANY summation order).  A float32 d^2 carries at most dim + 2 roundings
(the difference, the product, dim - 1 adds of non-negative terms, none of which cancels); the root halves that and adds
one rounding of its own:

    eps(dim) = (dim / 2 + 2) 2^-24          1.07e-6, 2.03e-6 and 3.93e-6 at dim 32, 64 and 128

The bound needs every non-zero squared difference to be a normal float32 and no sum to overflow: exact_l2 asserts both
for every pair of rows it is given, so every scene is checked where it is built.

The judge (judge_l2), per query row, E = that query's exact distances:
    range      idx1 != idx2, both in [0, nt)
    value      |d1 - E[idx1]| <= eps E[idx1], and d2 likewise
    first      E[idx1] (1 - eps) <= min_j E[j] (1 + eps)
    second     E[idx2] (1 - eps) <= min_{j != idx1} E[j] (1 + eps)
    order      d1 <= d2
    duplicate  where d1 == d2 as float32 and E[idx1] == E[idx2] exactly (true duplicates): idx1 < idx2
judge_hamming asks exact equality with the ranking by (bit count, lowest index): integers need no band.

Reported by the judge: `value` = the worst |d - E| / (eps E); `selection` = the worst (E[idx] / min E - 1) over the
band's width (1 + eps) / (1 - eps) - 1, so 1.0 is the edge of the band; `in_band` = the share of queries whose idx1 or
idx2 is not an exact minimum (E[idx1] > min E, or E[idx2] > the least E of the other rows) - those the float32
rounding decided.

Scenes (scene(kind, dim, nq, nt), fixed seeds, one per dim):
    uniform    [0, 1)
    root       the square root of L1-normalised gamma(0.6) rows (RootSIFT-like)
    signed     normal entries times a per-row scale 10^U(-3, 3)
    near_ties  train rows uniform + 3.0 (far), with 48 copies of one base row at shuffled positions among them: copy j
               has component j % dim stepped 1 + j // 8 times by np.nextafter; the queries are uniform
In the first three kinds the first train rows (100 where there is room) are the first queries with 1e-3 relative noise,
and two train rows far apart in index are exact copies of the last query (d1 = d2 = 0, lower index first).

Measured, nq = 257, nt = 1025 (value / selection / in_band as above; oracle = oracle/matcher_oracle.py on the CPU,
device = MI355X through matcher.knn2; off = the share of queries whose idx1 is not the exact arg-min; time = CPU
seconds of exact_l2 and the judge).  The device equals the oracle bit for bit, so its figures are the same numbers:

    kind       dim   oracle: value   selection   in_band   off     device: value   selection   in_band   time
    uniform     32           0.157   0           0         0               0.157   0           0         0.07 s
    uniform     64           0.107   0           0         0               0.107   0           0         0.12 s
    uniform    128           0.076   0           0         0               0.076   0           0         0.22 s
    root        32           0.174   0           0         0               0.174   0           0         0.07 s
    root        64           0.105   0           0         0               0.105   0           0         0.14 s
    root       128           0.080   0           0         0               0.080   0           0         0.18 s
    signed      32           0.209   0           0         0               0.209   0           0         0.06 s
    signed      64           0.111   0           0         0               0.111   0           0         0.11 s
    signed     128           0.076   0           0         0               0.076   0           0         0.24 s
    near_ties   32           0.152   0.0430      0.988     0.926           0.152   0.0430      0.988     0.07 s
    near_ties   64           0.098   0.0096      0.996     0.934           0.098   0.0096      0.996     0.12 s
    near_ties  128           0.063   0.0030      0.992     0.946           0.063   0.0030      0.992     0.20 s

So sequential float32 summation stays within a fifth of the order-free bound.  On near_ties the float32 rule decides
nearly every query (idx1 leaves the exact arg-min on 93 - 95 % of them, d1 == d2 on 90 - 96 %) while the selection stays
under 5 % of the band: the judge has room there, and the bit-for-bit comparison with the oracle is what pins the rule.

What the tests found when they were first run.  No defect in the distances or the ranking of finite rows, at any tile,
workgroup or split edge.  One defect on non-finite distances, read from the code beforehand: with the running top-2
started at 3.0e38f a distance of +inf is never inserted, so a query whose sums all overflow is left without a
neighbour, and an empty slot reports 3e38 where the rule says +inf.  The device confirmed the second on the first case
(a NaN query: d1 = d2 = 3e38); the kernel and the merge now start at +inf
(tests/test_matcher_truth_gpu.py: test_non_finite_distances_follow_the_rule).

Non-finite distances (nonfinite_cases) have their own small truth: by the rule of include/sfm_amd.h a train row whose
distance is NaN is never ranked, so the result must equal that of the train set WITHOUT those rows, indices mapped
back, with (-1, +inf) in the slots left over; +inf ranks last by index.
"""
import functools
import os
import subprocess
import tempfile
import time

import numpy as np

KINDS = ("uniform", "root", "signed", "near_ties")
DIMS = (32, 64, 128)
SEED = {32: 3201, 64: 6401, 128: 12801, 16: 1601}
N_NEAR = 48
F32_TINY = 2.0 ** -126
F32_MAX = float(np.finfo(np.float32).max)
METRIC_L2_U8, METRIC_L2_F32, METRIC_HAMMING = 0, 1, 2          # include/sfm_amd.h


def eps(dim):
    return (dim / 2 + 2) * 2.0 ** -24


# ------------------------------------------------------------------ exact distances
def exact_l2(q, t):
    """float64 [nq, nt]: sqrt(sum_k (q_k - t_k)^2) of float32 rows; asserts what the tolerance needs of the rows."""
    q = np.asarray(q); t = np.asarray(t)
    assert q.dtype == np.float32 and t.dtype == np.float32 and q.shape[1] == t.shape[1]
    a = q.astype(np.float64); b = t.astype(np.float64)
    out = np.empty((a.shape[0], b.shape[0]), np.float64)
    step = max(1, (1 << 22) // max(1, b.shape[0] * b.shape[1]))
    for s in range(0, a.shape[0], step):
        d = a[s:s + step, None, :] - b[None, :, :]
        sq = d * d
        assert not np.any((sq < F32_TINY) & (sq > 0)), "a non-zero squared difference is no normal float32: eps(dim) does not hold"
        out[s:s + step] = sq.sum(-1)
    assert out.size == 0 or out.max() < F32_MAX / 2, "a float32 sum could overflow"
    return np.sqrt(out)


def exact_hamming(q, t):
    """int32 [nq, nt]: differing bits of uint8 rows."""
    q = np.asarray(q); t = np.asarray(t)
    assert q.dtype == np.uint8 and t.dtype == np.uint8 and q.shape[1] == t.shape[1]
    out = np.empty((q.shape[0], t.shape[0]), np.int32)
    step = max(1, (1 << 22) // max(1, t.shape[0] * t.shape[1]))
    for s in range(0, q.shape[0], step):
        out[s:s + step] = np.unpackbits(q[s:s + step, None, :] ^ t[None, :, :], axis=-1).sum(-1, dtype=np.int32)
    return out


def _two_least(E):
    """Per row the lowest index of the least entry, and of the least entry among the rest."""
    rows = np.arange(E.shape[0])
    i1 = np.argmin(E, axis=1)
    rest = E.astype(np.float64, copy=True)
    rest[rows, i1] = np.inf
    return i1, np.argmin(rest, axis=1)


# ------------------------------------------------------------------ the judge
class Verdict:
    """What the judge found: `failures` (check name, query row, detail) and the three figures of the module docstring."""

    def __init__(self):
        self.failures = []
        self.value = self.selection = self.in_band = self.seconds = 0.0

    def fail(self, check, rows, detail=""):
        rows = np.atleast_1d(rows)
        if rows.size:
            self.failures.append((check, int(rows[0]), f"{rows.size} rows {detail}"))

    def checks(self):
        return {f[0] for f in self.failures}

    def assert_ok(self, what=""):
        assert not self.failures, (what, self.failures)
        return self


def judge_l2(q, t, result, E=None):
    """Holds (idx1, idx2, d1, d2) of ANY implementation to the exact distances of float32 rows q, t."""
    t0 = time.perf_counter()
    idx1, idx2, d1, d2 = (np.asarray(x) for x in result)
    nq, nt, dim = q.shape[0], t.shape[0], q.shape[1]
    E = exact_l2(q, t) if E is None else E
    e = eps(dim)
    v = Verdict()
    assert idx1.shape == idx2.shape == d1.shape == d2.shape == (nq,) and d1.dtype == np.float32 and d2.dtype == np.float32
    bad = (idx1 == idx2) | (idx1 < 0) | (idx1 >= nt) | (idx2 < 0) | (idx2 >= nt)
    v.fail("range", np.nonzero(bad)[0])
    if bad.any():
        return v                                               # nothing below can index with these
    rows = np.arange(nq)
    E1, E2 = E[rows, idx1], E[rows, idx2]
    m1i = np.argmin(E, axis=1)
    rest = E.copy(); rest[rows, idx1] = np.inf                 # the second slot competes with every row but idx1
    M1, M2 = E[rows, m1i], rest.min(axis=1)
    for name, d, Ex in (("value d1", d1, E1), ("value d2", d2, E2)):
        err = np.abs(d.astype(np.float64) - Ex)
        v.fail("value", np.nonzero(~(err <= e * Ex))[0], name)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(Ex > 0, err / (e * Ex), np.where(err == 0, 0.0, np.inf))
        v.value = max(v.value, float(ratio.max()))
    band = (1 + e) / (1 - e) - 1
    for name, Ex, M in (("first", E1, M1), ("second", E2, M2)):
        v.fail(name, np.nonzero(~(Ex * (1 - e) <= M * (1 + e)))[0])
        with np.errstate(divide="ignore", invalid="ignore"):
            excess = np.where(M > 0, (Ex / M - 1) / band, np.where(Ex == 0, 0.0, np.inf))
        v.selection = max(v.selection, float(excess.max()))
    v.fail("order", np.nonzero(~(d1 <= d2))[0])
    v.fail("duplicate", np.nonzero((d1 == d2) & (E1 == E2) & ~(idx1 < idx2))[0])
    v.in_band = float(np.mean((E1 > M1) | (E2 > M2)))
    v.seconds = time.perf_counter() - t0
    return v


def judge_hamming(q, t, result, E=None):
    """Exact equality with the ranking by (bit count, lowest train index)."""
    idx1, idx2, d1, d2 = (np.asarray(x) for x in result)
    E = exact_hamming(q, t) if E is None else E
    rows = np.arange(q.shape[0])
    i1, i2 = _two_least(E)
    v = Verdict()
    v.fail("range", np.nonzero((idx1 == idx2) | (idx1 < 0) | (idx1 >= t.shape[0]) | (idx2 < 0) | (idx2 >= t.shape[0]))[0])
    v.fail("first", np.nonzero(idx1 != i1)[0])
    v.fail("second", np.nonzero(idx2 != i2)[0])
    v.fail("value", np.nonzero((d1 != E[rows, i1].astype(np.float32)) | (d2 != E[rows, i2].astype(np.float32)))[0])
    return v


# ------------------------------------------------------------------ scenes
def _rows(rng, kind, n, dim):
    if kind == "uniform":
        return rng.random((n, dim), dtype=np.float32)
    if kind == "root":
        g = rng.gamma(0.6, 1.0, size=(n, dim)) + 1e-12
        return np.sqrt(g / g.sum(axis=1, keepdims=True)).astype(np.float32)
    if kind == "signed":
        return (rng.normal(size=(n, dim)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))).astype(np.float32)
    raise ValueError(kind)


def _noisy(rng, rows):
    return (rows.astype(np.float64) * (1 + 1e-3 * rng.normal(size=rows.shape))).astype(np.float32)


def near_copies(base, n):
    """n copies of one row: copy j has component j % dim stepped 1 + j // 8 times upwards by np.nextafter."""
    out = np.repeat(base[None, :].astype(np.float32), n, axis=0)
    for j in range(n):
        k = j % base.shape[0]
        for _ in range(1 + j // 8):
            out[j, k] = np.nextafter(out[j, k], np.float32(np.inf))
    return out


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def scene(kind, dim, nq, nt):
    """(queries [nq, dim], train [nt, dim], exact distances [nq, nt]), read-only; see the module docstring."""
    rng = np.random.default_rng([SEED[dim], KINDS.index(kind), nq, nt])
    if kind == "near_ties":
        q = rng.random((nq, dim), dtype=np.float32)
        t = rng.random((nt, dim), dtype=np.float32) + np.float32(3.0)
        n = min(N_NEAR, nt)
        base = rng.random(dim, dtype=np.float32) * np.float32(0.5) + np.float32(0.25)
        t[rng.permutation(nt)[:n]] = near_copies(base, n)
    else:
        q, t = _rows(rng, kind, nq, dim), _rows(rng, kind, nt, dim)
        m = min(100, nq, nt // 2)
        t[:m] = _noisy(rng, q[:m])
        lo, hi = m + (nt - m) // 4, nt - 1                     # exact copies of the last query, far apart in index
        if hi > lo:
            t[lo] = q[nq - 1]; t[hi] = q[nq - 1]
    return _freeze(q, t, exact_l2(q, t))                       # exact_l2 asserts the conditions of eps(dim) on every pair


@functools.lru_cache(maxsize=None)
def hamming_scene(nbytes, nq, nt):
    """uint8 bit strings as tests/test_matcher_gpu.py: test_hamming_sizes_and_widths builds them: half the train rows (as
    far as there are queries) are sparse flips of queries, a quarter of those again exact duplicates further down."""
    rng = np.random.default_rng([SEED[nbytes], 7, nq, nt])
    b1 = rng.integers(0, 256, size=(nq, nbytes), dtype=np.uint8)
    b2 = rng.integers(0, 256, size=(nt, nbytes), dtype=np.uint8)
    k = min(nq, nt) // 2
    flips = (rng.integers(0, 256, size=(k, nbytes), dtype=np.uint8) & rng.integers(0, 256, size=(k, nbytes), dtype=np.uint8)
             & rng.integers(0, 256, size=(k, nbytes), dtype=np.uint8))
    b2[:k] = b1[:k] ^ flips
    b2[k: k + k // 4] = b2[:k // 4]
    return _freeze(b1, b2)


# ------------------------------------------------------------------ split seams, from the library's own plan
@functools.lru_cache(maxsize=None)
def _tiling_exe():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(tempfile.mkdtemp(prefix="match_tiling_"), "match_tiling_print")
    cmd = ["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "sfm_amd", "csrc"),
           os.path.join(root, "tests", "native", "match_tiling_print.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


@functools.lru_cache(maxsize=None)
def match_tiling(metric, nq, nt, dim):
    """(queries per workgroup, train splits, train rows per split) of one sfm_match_knn2 call: sfm_amd/csrc/match_plan.h
    itself, compiled on the host (tests/native/match_tiling_print.cpp)."""
    run = subprocess.run([_tiling_exe(), str(metric), str(nq), str(nt), str(dim)], capture_output=True, text=True,
                         env={k: v for k, v in os.environ.items() if not k.startswith("SFM_MATCH_")})
    assert run.returncode == 0, run.stderr
    qpw, nsplit, rps = (int(x) for x in run.stdout.split())
    return qpw, nsplit, rps


def seam_positions(nq, nt, nsplit, rps):
    """Where a seam scene plants its rows.  Query 0: duplicates at the last row of split 0 and the first of split 1; query
    1: the same at the seam into the last split; the other queries: one near row each, counted back from the last train
    row (inside the last, shorter split).  {query: (train rows, ascending)}; without a seam only the last kind."""
    plan = {}
    first_free = 0
    if nsplit > 1:
        plan[0] = (rps - 1, rps)
        first_free = 1
        if nsplit > 2 and nq > 1:
            plan[1] = ((nsplit - 1) * rps - 1, (nsplit - 1) * rps)
            first_free = 2
    last_len = nt - (nsplit - 1) * rps
    for k, qi in enumerate(range(first_free, nq)):
        if k + 1 < last_len - 1:                               # stay clear of the seam row itself
            plan[qi] = (nt - 1 - k,)
    return plan


@functools.lru_cache(maxsize=None)
def seam_scene(nq, nt, dim=128):
    """A `root` scene whose near rows sit at the seams of the float32 kernel's train splits (seam_positions)."""
    _, nsplit, rps = match_tiling(METRIC_L2_F32, nq, nt, dim)
    rng = np.random.default_rng([SEED[dim], 11, nq, nt])
    q, t = _rows(rng, "root", nq, dim), _rows(rng, "root", nt, dim)
    plan = seam_positions(nq, nt, nsplit, rps)
    for qi, pos in plan.items():
        t[list(pos)] = _noisy(rng, q[qi:qi + 1])               # one noisy copy, at every position: exact duplicates
    return _freeze(q, t, exact_l2(q, t)) + (plan,)


@functools.lru_cache(maxsize=None)
def hamming_seam_scene(nq, nt, nbytes=64):
    _, nsplit, rps = match_tiling(METRIC_HAMMING, nq, nt, nbytes)
    b1, b2 = (a.copy() for a in hamming_scene(nbytes, nq, nt))
    rng = np.random.default_rng([SEED[nbytes], 13, nq, nt])
    plan = seam_positions(nq, nt, nsplit, rps)
    for qi, pos in plan.items():
        flip = np.zeros(nbytes, np.uint8); flip[rng.integers(0, nbytes)] = 1 << rng.integers(0, 8)
        b2[list(pos)] = b1[qi] ^ flip                          # one bit away: nearer than every planted flip pattern but 0
    return _freeze(b1, b2) + (plan,)


# ------------------------------------------------------------------ image sets for the batched calls
BATCH_SIZES = (300, 2, 33, 0, 1025, 257, 1)


@functools.lru_cache(maxsize=None)
def image_sets(kind, dim, sizes=BATCH_SIZES):
    """Per-image float32 descriptor sets that share rows.  root: every image is a draw from one pool, with 1e-3 relative
    noise; near_ties: a third of every image are near copies of ONE base row (distinct within an image), a third uniform
    rows, the rest far rows (uniform + 3.0), shuffled."""
    rng = np.random.default_rng([SEED[dim], 17, KINDS.index(kind)])
    sets = []
    if kind == "near_ties":
        base = rng.random(dim, dtype=np.float32) * np.float32(0.5) + np.float32(0.25)
        copies = near_copies(base, N_NEAR)
        for n in sizes:
            k = min(n // 3, N_NEAR)
            u = (n - k) // 2
            rows = np.concatenate([copies[rng.permutation(N_NEAR)[:k]], rng.random((u, dim), dtype=np.float32),
                                   rng.random((n - k - u, dim), dtype=np.float32) + np.float32(3.0)])
            sets.append(rows[rng.permutation(n)])
    else:
        pool = _rows(rng, kind, max(sizes) + 50, dim)
        for n in sizes:
            sets.append(_noisy(rng, pool[rng.permutation(pool.shape[0])[:n]]))
    return _freeze(*sets)


@functools.lru_cache(maxsize=None)
def orb_sets(nbytes=64, sizes=BATCH_SIZES):
    rng = np.random.default_rng([SEED[nbytes], 19])
    pool = rng.integers(0, 256, size=(max(sizes) + 50, nbytes), dtype=np.uint8)
    sets = []
    for n in sizes:
        rows = pool[rng.permutation(pool.shape[0])[:n]]
        sets.append(rows ^ (rng.integers(0, 256, size=rows.shape, dtype=np.uint8) & rng.integers(0, 256, size=rows.shape, dtype=np.uint8)
                            & rng.integers(0, 256, size=rows.shape, dtype=np.uint8) & rng.integers(0, 256, size=rows.shape, dtype=np.uint8)))
    return _freeze(*sets)


def batch_pairs(sizes=BATCH_SIZES):
    """Every ordered pair of different images, and every image that can be a train set against itself."""
    n = len(sizes)
    return [(i, j) for i in range(n) for j in range(n) if i != j] + [(i, i) for i in range(n) if sizes[i] >= 2]


# ------------------------------------------------------------------ non-finite distances
NONFINITE_NQ, NONFINITE_NT, NEAR_ROW = 40, 1025, 700


def nonfinite_cases(dim):
    """[(name, queries, train, expected)] float32; `expected` = (idx1, idx2, d1, d2) where the rule of include/sfm_amd.h
    fixes the whole answer, else None (then expect_without_nan_rows says what must come out)."""
    nq, nt = NONFINITE_NQ, NONFINITE_NT
    q0, t0 = (a.copy() for a in scene("root", dim, nq, nt)[:2])
    inf32 = np.float32(np.inf)
    full = lambda v, dt: np.full(nq, v, dt)
    cases = []
    q = q0.copy(); q[3] = np.nan; q[nq - 1, dim - 1] = np.nan
    cases.append(("nan_query", q, t0.copy(), None))
    t = t0.copy(); t[3] = np.nan
    cases.append(("one_nan_train_row", q0.copy(), t, None))
    t = np.full_like(t0, np.nan); t[NEAR_ROW] = t0[NEAR_ROW]
    cases.append(("all_but_one_nan_train_rows", q0.copy(), t, None))
    t = t0.copy(); t[0, dim // 2] = np.inf                     # row 0 is query 0's nearest row in the finite scene
    cases.append(("inf_in_a_train_row", q0.copy(), t, None))
    big = (np.float32(3e19) * (1 + np.float32(0.01) * np.random.default_rng(SEED[dim]).random((nq, dim), dtype=np.float32))).astype(np.float32)
    t = np.zeros_like(t0)
    cases.append(("overflow_everywhere", big, t, (full(0, np.int32), full(1, np.int32), full(inf32, np.float32), full(inf32, np.float32))))
    t = np.zeros_like(t0); t[NEAR_ROW] = np.float32(3e19)
    d_near = np.sqrt(((big.astype(np.float64) - float(np.float32(3e19))) ** 2).sum(axis=1)).astype(np.float32)
    cases.append(("overflow_but_one_near_row", big, t, (full(NEAR_ROW, np.int32), full(0, np.int32), d_near, full(inf32, np.float32))))
    return cases


def expect_from_finite_rows(q, t, knn2):
    """What the rule asks of (q, t), from `knn2` (any implementation that is right on finite rows) run on the rankable
    rows only.  Query rows holding a NaN get (-1, +inf) twice.  Train rows holding a NaN are never ranked and rows holding
    +inf rank after every finite row, so while two finite train rows remain the answer is that of the finite rows alone,
    indices mapped back; a train set left with one row fills the first slot alone."""
    nq = q.shape[0]
    idx1 = np.full(nq, -1, np.int32); idx2 = np.full(nq, -1, np.int32)
    d1 = np.full(nq, np.inf, np.float32); d2 = np.full(nq, np.inf, np.float32)
    qs = np.nonzero(~np.isnan(q).any(axis=1))[0]
    assert np.isfinite(q[qs]).all()
    ts = np.nonzero(np.isfinite(t).all(axis=1))[0]
    assert len(ts) >= 2 or not np.isinf(t).any(), "rows of +inf would have to be ranked"
    if len(ts) >= 2:
        a, b, c, d = knn2(q[qs], t[ts])
        idx1[qs] = ts[a]; idx2[qs] = ts[b]; d1[qs] = c; d2[qs] = d
    elif len(ts) == 1:
        a, _, c, _ = knn2(q[qs], np.repeat(t[ts], 2, axis=0))      # the one row twice: its distance in the first slot
        assert np.all(a == 0)
        idx1[qs] = ts[0]; d1[qs] = c
    return idx1, idx2, d1, d2
