"""The matcher's exact reference and judge (tests/matcher_truth.py) on the CPU: the NumPy oracle passes the judge on
every scene, the scenes are what they claim to be, the judge rejects doctored results, and the oracle follows the rule
for non-finite distances.  tests/test_matcher_truth_gpu.py holds the device to the same judge."""
import numpy as np
import pytest

import matcher_truth as mt
from oracle import matcher_oracle as mo

NQ, NT = 257, 1025


@pytest.fixture(scope="module")
def oracle_results():
    cache = {}

    def get(kind, dim):
        if (kind, dim) not in cache:
            q, t, E = mt.scene(kind, dim, NQ, NT)
            cache[kind, dim] = (q, t, E, mo.knn2(q, t, "l2"))
        return cache[kind, dim]
    return get


@pytest.mark.parametrize("dim", mt.DIMS)
@pytest.mark.parametrize("kind", mt.KINDS)
def test_oracle_passes_the_judge_and_the_scene_is_what_it_claims(oracle_results, kind, dim):
    q, t, E, res = oracle_results(kind, dim)
    v = mt.judge_l2(q, t, res, E).assert_ok((kind, dim))
    print(f"{kind} {dim}: value {v.value:.3f} eps, selection {v.selection:.4f} band, in band {v.in_band:.3f}, {v.seconds:.2f} s")
    off = float(np.mean(res[0] != np.argmin(E, axis=1)))
    if kind == "near_ties":
        # the float32 rule must decide here, or the scene tests nothing the others do not
        assert off >= 0.25, off
    else:
        # no row is left to the band: the judge's selection checks are as sharp as an index comparison
        assert off == 0.0 and v.in_band == 0.0 and v.selection == 0.0
        last = NQ - 1                                          # the planted exact copies of the last query
        assert res[2][last] == 0.0 and res[3][last] == 0.0 and res[0][last] < res[1][last] and res[1][last] == NT - 1
        assert np.array_equal(res[0][:100], np.arange(100))    # the noisy copies of the first queries


@pytest.mark.parametrize("nbytes", [16, 32, 64])
def test_oracle_hamming_passes_the_judge(nbytes):
    q, t = mt.hamming_scene(nbytes, NQ, NT)
    res = mo.knn2(q, t, "hamming")
    mt.judge_hamming(q, t, res).assert_ok(nbytes)
    assert np.any(res[2] == res[3])                            # ties on the bit count: the index rule decides some rows


def test_judge_rejects_doctored_results(oracle_results):
    q, t, E, res = oracle_results("root", 64)
    e = mt.eps(64)

    def doctored(change):
        r = [a.copy() for a in res]
        change(r)
        return mt.judge_l2(q, t, r, E)

    qi = 150                                                   # an ordinary query: no planted near row
    assert res[3][qi] > 1.02 * res[2][qi]

    def swap_first(r):                                         # idx1 -> the first row at least 1 % farther, with ITS true distance
        j = int(np.argmin(np.where(E[qi] >= 1.01 * E[qi, res[0][qi]], E[qi], np.inf)))
        r[0][qi] = j; r[2][qi] = np.float32(E[qi, j])
        if j == res[1][qi]:                                    # that row is the second neighbour: a true swap
            r[1][qi] = res[0][qi]; r[3][qi] = res[2][qi]
    assert "first" in doctored(swap_first).checks()

    def off_value(r):
        r[2][qi] = np.float32(r[2][qi] * (1 + 4 * e))
    assert doctored(off_value).checks() == {"value"}

    last = NQ - 1

    def wrong_duplicate_order(r):
        r[0][last], r[1][last] = res[1][last], res[0][last]
    assert doctored(wrong_duplicate_order).checks() == {"duplicate"}

    def same_index(r):
        r[1][qi] = r[0][qi]
    assert doctored(same_index).checks() == {"range"}

    def out_of_range(r):
        r[1][qi] = NT
    assert doctored(out_of_range).checks() == {"range"}

    def second_not_nearest(r):                                 # idx2 -> the first row at least 1 % beyond the true second
        j = int(np.argmin(np.where(E[qi] >= 1.01 * E[qi, res[1][qi]], E[qi], np.inf)))
        r[1][qi] = j; r[3][qi] = np.float32(E[qi, j])
    assert doctored(second_not_nearest).checks() == {"second"}
    assert not mt.judge_l2(q, t, res, E).failures

    hq, ht = mt.hamming_scene(64, 40, 200)
    hres = [a.copy() for a in mo.knn2(hq, ht, "hamming")]
    tie = int(np.nonzero(hres[2] == hres[3])[0][0])
    hres[0][tie], hres[1][tie] = hres[1][tie], hres[0][tie]
    assert {"first", "second"} <= mt.judge_hamming(hq, ht, hres).checks()


def test_exact_distances_refuse_rows_the_tolerance_does_not_cover():
    q = np.zeros((1, 32), np.float32); t = np.zeros((2, 32), np.float32)
    t[1, 0] = 1e-30                                            # its square is no normal float32
    with pytest.raises(AssertionError, match="normal float32"):
        mt.exact_l2(q, t)
    t[1, 0] = 3e19
    with pytest.raises(AssertionError, match="overflow"):
        mt.exact_l2(q, t)


def test_seam_scenes_sit_on_the_planned_splits():
    """The split geometry comes from match_plan.h itself, and what the seam sizes rely on is checked, not assumed: with
    two query blocks or fewer, 2 splits from 1,024 train rows on and 8 from 4,096."""
    assert mt.match_tiling(mt.METRIC_L2_F32, 257, 1025, 128) == (256, 2, 513)
    for nt, ns in ((1023, 1), (1024, 2), (1025, 2), (4095, 7), (4096, 8), (4097, 8), (4609, 8)):
        qpw, nsplit, rps = mt.match_tiling(mt.METRIC_L2_F32, 5, nt, 128)
        assert (qpw, nsplit) == (256, ns) and (nsplit - 1) * rps < nt <= nsplit * rps
        q, t, E, plan = mt.seam_scene(5, nt)
        res = mo.knn2(q, t, "l2")
        mt.judge_l2(q, t, res, E).assert_ok(nt)
        assert len(plan) == 5
        for qi, pos in plan.items():
            assert res[0][qi] == pos[0]
            if len(pos) == 1:                                  # the nearest row lies in the last, shorter split
                assert nsplit == 1 or (pos[0] >= (nsplit - 1) * rps and nt - (nsplit - 1) * rps <= rps)
            else:                                              # the duplicates on either side of a seam
                assert pos[0] // rps + 1 == pos[1] // rps and (res[0][qi], res[1][qi]) == pos and res[2][qi] == res[3][qi]


@pytest.mark.parametrize("dim", [32, 128])
def test_oracle_follows_the_rule_for_non_finite_distances(dim):
    for name, q, t, expected in mt.nonfinite_cases(dim):
        res = mo.knn2(q, t, "l2")
        if expected is None:
            expected = mt.expect_from_finite_rows(q, t, lambda a, b: mo.knn2(a, b, "l2"))
            for g, r in zip(res, expected):
                assert np.array_equal(g, r), name
        else:
            assert np.array_equal(res[0], expected[0]) and np.array_equal(res[1], expected[1]), name
            assert np.allclose(res[2], expected[2], rtol=mt.eps(dim), atol=0) and np.array_equal(res[3], expected[3]), name
        assert not np.isnan(res[2]).any() and not np.isnan(res[3]).any(), name
        assert np.all(np.isinf(res[2][res[0] < 0])) and np.all(np.isinf(res[3][res[1] < 0])), name
        # the ratio test never hands out a row without a neighbour, and keeps a query that has exactly one
        qi, ti, _ = mo.ratio_filter(*[res[k] for k in (0, 2, 3)])
        assert np.all(ti >= 0), name
        one = np.nonzero((res[0] >= 0) & np.isfinite(res[2]) & np.isinf(res[3]))[0]
        assert np.all(np.isin(one, qi)), name
    names = [c[0] for c in mt.nonfinite_cases(dim)]
    assert names == ["nan_query", "one_nan_train_row", "all_but_one_nan_train_rows", "inf_in_a_train_row",
                     "overflow_everywhere", "overflow_but_one_near_row"]
