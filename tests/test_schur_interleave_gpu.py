"""k_schur_items walks its work items through descriptors (first, stride, count): the items of a block of >= 3 items are
interleaved.  On the `edge` and `aligned` scenes of tests/stage_reference.py (blocks of 1 ... 513 pairs, diagonal blocks of 3, 4
and 6 items; counts that are no multiple of 64 nor of the batch of 32 / 28 pairs; a diagonal item's fused right-hand side), as
they are and with observations doubled so that a camera appears twice on a track (has_dup: every item on the general path), for
d = 10 and 6: S and r inside the stage bounds, bitwise equal between builds and between problems, and the device's descriptors
equal to the Python mirror's."""
import numpy as np
import pytest

import stage_reference as sr
import test_ba_stages_gpu as ts

pytestmark = pytest.mark.gpu

CASES = [(v, dup, d) for v in ("edge", "aligned") for dup in (False, True) for d in (10, 6)]
_scenes = {}


def scene(variant, dup):
    if (variant, dup) not in _scenes:
        sc = sr.edge_scene(variant)
        if dup:
            # camera 3's observation on five of the (2, 3) tracks once more, right behind itself (the order stays point-major): the
            # diagonal block (3, 3), 6 interleaved items, then holds cross pairs (k_a, k_b) beside its self-pairs
            tr = np.diff(np.concatenate([[0], np.flatnonzero(np.diff(sc.pt_idx)) + 1, [sc.pt_idx.shape[0]]]))
            start = np.cumsum(tr) - tr
            two = [int(s) for s, n in zip(start, tr) if n == 2 and sc.cam_idx[s] == 2 and sc.cam_idx[s + 1] == 3][:5]
            assert len(two) == 5
            at = np.sort(np.array(two) + 1)
            keep = np.sort(np.concatenate([np.arange(sc.pt_idx.shape[0]), at]), kind="stable")
            sc = sr.EdgeScene(**{**sc.__dict__, "cam_idx": sc.cam_idx[keep], "pt_idx": sc.pt_idx[keep], "uv": sc.uv[keep]})
        _scenes[(variant, dup)] = sc
    return _scenes[(variant, dup)]


def built(sc, d):
    be = ts.backend(sc, d)
    _, _, _, hdiag = be.linearize()
    alpha = 1e-3 * hdiag
    ts.build(be, alpha)
    return be, alpha


@pytest.mark.parametrize("variant,dup,d", CASES)
def test_interleaved_items(gpu_ready, variant, dup, d):
    from sfm_amd.structure import build_structure
    sc = scene(variant, dup)
    be, alpha = built(sc, d)
    st = be.structure()
    host = build_structure(sc.cam_idx, sc.pt_idx, sc.C, sc.P)
    # the exported arrays are what they were; the descriptors are the mirror's and hold interleaved diagonal and off-diagonal blocks
    for name in ("blk_ptr", "pair_k", "pair_k2", "item_ptr", "item_beg", "item_end", "xcd_ptr", "xcd_items"):
        assert np.array_equal(st[name], getattr(host, name)), name
    desc = be.item_descriptors()
    for name in ("item_first", "item_stride", "item_cnt"):
        assert np.array_equal(desc[name], getattr(host, name)), name
    n_of_item = np.repeat(np.diff(st["item_ptr"]), np.diff(st["item_ptr"]))
    assert np.array_equal(desc["item_stride"], np.where(n_of_item >= 3, n_of_item, 1))
    diag = st["pair_k"][desc["item_first"]] == st["pair_k2"][desc["item_first"]]
    assert np.any(diag & (n_of_item >= 3)) and np.any(~diag & (n_of_item >= 3)) and np.any(n_of_item == 2)
    batch = 32 if d == 10 else 28
    assert np.any((desc["item_cnt"] % 64 != 0) & (desc["item_cnt"] % batch != 0) & (n_of_item >= 3))
    # S and r inside the stage bounds, from the device's own G
    inp = ts.read_inputs(be)
    G = ts.read_G(be)[0]
    S, r = ts.read_Sr(be)
    ratio, where, problems = sr.judge_S(G, inp["B"], st, sc.C, S)
    print(f"S {variant} dup={dup} d={d}: {ratio:.3g} of its bound at {where}")
    assert not problems, problems
    assert ratio <= 1.0, (ratio, where)
    ratio, where = sr.judge_r(G, inp["Cp6"], inp["gp"], inp["gc"], alpha, sc.cam_idx, sc.pt_idx, sc.C, r)
    print(f"r {variant} dup={dup} d={d}: {ratio:.3g} of its bound at {where}")
    assert ratio <= 1.0, (ratio, where)
    # bitwise: a second build on the same problem, and a problem constructed afresh
    ts.build(be, alpha)
    S2, r2 = ts.read_Sr(be)
    assert np.array_equal(S, S2) and np.array_equal(r, r2)
    be.close()
    other, alpha2 = built(sc, d)
    assert alpha2 == alpha
    S3, r3 = ts.read_Sr(other)
    other.close()
    assert np.array_equal(S, S3) and np.array_equal(r, r3)
