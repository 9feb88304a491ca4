"""The rule by which the Schur kernel walks a work item (sfm_amd.structure.item_descriptors, the mirror of k_item_desc in
sfm_amd/csrc/problem.hip): item i of a block of n >= 3 items takes pairs lo + i + j n, blocks of n <= 2 items keep their
contiguous stretches.  Host only: blocks of 1 / 255 / 256 / 257 / 512 / 513 / 514 / 769 pairs and cameras of 513 / 1,025
observations (diagonal blocks of 3 and 5 items).  The exported arrays (pair lists, item ranges) are pinned to a contiguous
split written out here."""
import numpy as np
import pytest

from sfm_amd.structure import build_structure, item_descriptors, ITEM_PAIRS

C_ = 9
# two-camera tracks: block (a, b) gets exactly this many pairs
BLOCKS = {(0, 1): 1, (0, 2): 255, (1, 2): 256, (3, 4): 257, (3, 5): 512, (4, 5): 513, (6, 7): 514, (6, 8): 769}
SINGLES = {2: 2}                          # single-camera tracks: camera 2 then has 255 + 256 + 2 = 513 observations
CAM_OBS = {0: 256, 1: 257, 2: 513, 3: 769, 4: 770, 5: 1025, 6: 1283, 7: 514, 8: 769}
# pairs -> (items, contiguous sizes, sizes as walked)
FROZEN = {1: (1, [1], [1]), 255: (1, [255], [255]), 256: (1, [256], [256]), 257: (2, [256, 1], [256, 1]),
          512: (2, [256, 256], [256, 256]), 513: (3, [256, 256, 1], [171, 171, 171]),
          514: (3, [256, 256, 2], [172, 171, 171]), 769: (4, [256, 256, 256, 1], [193, 192, 192, 192]),
          770: (4, [256, 256, 256, 2], [193, 193, 192, 192]), 1025: (5, [256] * 4 + [1], [205] * 5),
          1283: (6, [256] * 5 + [3], [214, 214, 214, 214, 214, 213])}


@pytest.fixture(scope="module")
def built():
    tracks = [(a, b) for (a, b), cnt in BLOCKS.items() for _ in range(cnt)] + [(c,) for c, cnt in SINGLES.items() for _ in range(cnt)]
    order = np.random.default_rng(3).permutation(len(tracks))          # a block's tracks are spread over the point ids
    tracks = [tracks[i] for i in order]
    cam_idx = np.array([c for t in tracks for c in t], dtype=np.int64)
    pt_idx = np.repeat(np.arange(len(tracks)), [len(t) for t in tracks])
    return tracks, cam_idx, pt_idx, build_structure(cam_idx, pt_idx, C_, len(tracks))


def blocks_of(st):
    """(a, b, lo, hi, first item, items) of every non-empty block."""
    out = []
    for a in range(C_):
        for b in range(a, C_):
            i = a * C_ - a * (a - 1) // 2 + (b - a)
            if st.blk_ptr[i + 1] > st.blk_ptr[i]:
                out.append((a, b, int(st.blk_ptr[i]), int(st.blk_ptr[i + 1]), int(st.item_ptr[i]), int(st.item_ptr[i + 1] - st.item_ptr[i])))
    return out


def test_the_scene_holds_the_sizes_it_is_for(built):
    _, cam_idx, _, st = built
    assert np.bincount(cam_idx, minlength=C_).tolist() == [CAM_OBS[c] for c in range(C_)]
    sizes = {(a, b): hi - lo for a, b, lo, hi, _, _ in blocks_of(st)}
    want = dict(BLOCKS)
    want.update({(c, c): n for c, n in CAM_OBS.items()})
    assert sizes == want
    assert {513, 1025} <= {sizes[(c, c)] for c in range(C_)}


def test_exported_arrays_are_the_contiguous_split(built):
    """pair_k / pair_k2 / blk_ptr by brute force over the tracks, item_ptr / item_beg / item_end as stretches of 256 - what the
    structure exported before the items were interleaved, and what everything that reads pairs by block range relies on."""
    tracks, cam_idx, pt_idx, st = built
    per_block = {}
    k0 = 0
    for t in tracks:
        for i, c in enumerate(t):
            for j, c2 in enumerate(t):
                if c <= c2:
                    per_block.setdefault((c, c2), []).append((k0 + i, k0 + j))
        k0 += len(t)
    pk, pk2, blk_ptr, item_ptr, beg, end = [], [], [0], [0], [], []
    for a in range(C_):
        for b in range(a, C_):
            pairs = sorted(per_block.get((a, b), []))
            lo = len(pk)
            pk += [p[0] for p in pairs]; pk2 += [p[1] for p in pairs]
            blk_ptr.append(len(pk))
            for s in range(lo, len(pk), 256):
                beg.append(s); end.append(min(s + 256, len(pk)))
            item_ptr.append(len(beg))
    for name, want in (("pair_k", pk), ("pair_k2", pk2), ("blk_ptr", blk_ptr), ("item_ptr", item_ptr), ("item_beg", beg), ("item_end", end)):
        got = getattr(st, name)
        assert got.dtype == np.int32 and np.array_equal(got, np.array(want)), name
    for a, b, lo, hi, o, n in blocks_of(st):
        items, contiguous, _ = FROZEN[hi - lo]
        assert n == items == -(-(hi - lo) // ITEM_PAIRS)
        assert (st.item_end[o:o + n] - st.item_beg[o:o + n]).tolist() == contiguous


def test_every_pair_of_a_block_lies_in_exactly_one_item(built):
    st = built[3]
    assert st.item_first.dtype == st.item_stride.dtype == st.item_cnt.dtype == np.int32
    assert st.item_first.shape == st.item_stride.shape == st.item_cnt.shape == (st.n_items,)
    seen = np.zeros(st.n_pairs, dtype=np.int64)
    for a, b, lo, hi, o, n in blocks_of(st):
        for i in range(o, o + n):
            walked = st.item_first[i] + np.arange(st.item_cnt[i]) * st.item_stride[i]
            assert walked.min() >= lo and walked.max() < hi, (a, b, i)
            seen[walked] += 1
    assert np.all(seen == 1)


def test_counts_and_strides(built):
    st = built[3]
    assert st.item_cnt.min() >= 1 and st.item_cnt.max() <= ITEM_PAIRS
    for a, b, lo, hi, o, n in blocks_of(st):
        cnt, first, stride = st.item_cnt[o:o + n], st.item_first[o:o + n], st.item_stride[o:o + n]
        assert cnt.tolist() == FROZEN[hi - lo][2], (a, b)
        if n <= 2:                       # contiguous, as exported
            assert np.all(stride == 1) and np.array_equal(first, st.item_beg[o:o + n]) and np.array_equal(first + cnt, st.item_end[o:o + n])
        else:                            # item i: lo + i + j n; sizes differ by at most one
            assert np.all(stride == n) and np.array_equal(first, lo + np.arange(n)) and cnt.max() - cnt.min() <= 1


def test_rule_on_bare_ranges():
    """item_descriptors on block ranges alone, every size from 1 to 1,300 pairs: a partition, <= 256 pairs per item, sizes within
    one of each other once interleaved."""
    sizes = np.arange(1, 1301)
    blk_ptr = np.concatenate([[0], np.cumsum(sizes)])
    item_ptr = np.concatenate([[0], np.cumsum(-(-sizes // ITEM_PAIRS))])
    first, stride, cnt = item_descriptors(blk_ptr, item_ptr)
    seen = np.zeros(int(blk_ptr[-1]), dtype=np.int64)
    for b, m in enumerate(sizes):
        o, n = int(item_ptr[b]), int(item_ptr[b + 1] - item_ptr[b])
        assert cnt[o:o + n].sum() == m and cnt[o:o + n].max() <= ITEM_PAIRS and cnt[o:o + n].min() >= 1
        assert np.all(stride[o:o + n] == (n if n >= 3 else 1))
        if n >= 3:
            assert cnt[o:o + n].max() - cnt[o:o + n].min() <= 1
        for i in range(o, o + n):
            seen[first[i] + np.arange(cnt[i]) * stride[i]] += 1
    assert np.all(seen == 1)
