"""sfm_tracks_build on the device against the contract restated in tests/tracks_reference.py: every output array and the
counters must be EQUAL (integers throughout, so there are no tolerances), whatever the order of the edges and pairs."""
import functools

import numpy as np
import pytest

import tracks_reference as tr
from test_tracks_reference import shipped, shipped_reference

pytestmark = pytest.mark.gpu


def device(g, min_len=2, policy="drop"):
    from sfm_amd import tracks
    return tracks.build_tracks_raw(*g, min_length=min_len, conflicts=policy)


def assert_equal(dev, ref, what=""):
    for k in ("counts", "track_ptr", "obs_image", "obs_kp", "track_conflict", "node_track"):
        assert dev[k].dtype == ref[k].dtype and dev[k].shape == ref[k].shape, (what, k, dev[k].shape, ref[k].shape)
        assert np.array_equal(dev[k], ref[k]), (what, k, int(np.flatnonzero(dev[k] != ref[k])[0]))


def check(g, what="", policies=("drop", "keep"), min_lens=(2,)):
    out = None
    for policy in policies:
        for min_len in min_lens:
            out = device(g, min_len, policy)
            assert_equal(out, tr.build(*g, min_len=min_len, policy=policy), (what, policy, min_len))
    return out


def one_keypoint_graph(n, a, b):
    """n images of one keypoint each; edge k joins images a[k] and b[k] and is a pair of its own."""
    m = len(a)
    return (np.arange(n + 1, dtype=np.int64), np.arange(m + 1, dtype=np.int64),
            np.stack([a, b], axis=1).astype(np.int32), np.zeros(m, np.int32), np.zeros(m, np.int32), None)


# ------------------------------------------------------------------------------------------------ the shipped matches
@pytest.mark.parametrize("min_len", [2, 3])
@pytest.mark.parametrize("policy", ["drop", "keep"])
@pytest.mark.parametrize("verified", [True, False])
def test_shipped_matches(gpu_ready, verified, policy, min_len):
    kp_ptr, seg_ptr, pairs, q, t, mask, _, _ = shipped()
    out = device((kp_ptr, seg_ptr, pairs, q, t, mask if verified else None), min_len, policy)
    assert_equal(out, shipped_reference(verified, policy, min_len))
    if min_len == 2:
        assert out["counts"].tolist() == {(True, "drop"): [1641, 6548, 56, 0], (True, "keep"): [1697, 6960, 56, 0],
                                          (False, "drop"): [1685, 6602, 119, 0], (False, "keep"): [1804, 7809, 119, 0]}[(verified, policy)]


def test_public_wrapper_on_the_shipped_matches(gpu_ready):
    """build_tracks with per-pair arrays and masks gives the reference's arrays as a Tracks."""
    from sfm_amd import build_tracks
    kp_ptr, seg_ptr, pairs, q, t, mask, pts1, pts2 = shipped()
    cut = lambda a: [a[seg_ptr[s]:seg_ptr[s + 1]] for s in range(len(pairs))]
    T = build_tracks([500] * 35, pairs, list(zip(cut(q), cut(t))), masks=cut(mask))
    ref = shipped_reference(True, "drop", 2)
    assert len(T) == 1641 and T.n_obs == 6548 and T.n_conflicting == 56 and T.n_bad_edges == 0
    assert np.array_equal(T.track_ptr, ref["track_ptr"]) and np.array_equal(T.image, ref["obs_image"])
    assert np.array_equal(T.keypoint, ref["obs_kp"]) and np.array_equal(T.node_track, ref["node_track"])
    assert T.lengths().max() == 12 and int((T.lengths() >= 3).sum()) == 1049
    # pixel positions by keypoint index: every observation of a track is where its pairs saw it
    xy = np.full((35, 500, 2), np.nan, np.float32)
    seg = np.repeat(np.arange(len(pairs)), np.diff(seg_ptr))
    xy[pairs[seg, 0], q] = pts1
    xy[pairs[seg, 1], t] = pts2
    cam, pt, uv = T.observations(list(xy))
    assert np.isfinite(uv).all() and cam.dtype == np.int32 and pt.dtype == np.int32 and (np.diff(pt) >= 0).all()
    tracks = T.as_point_tracks(list(xy), image_ids=range(1, 36))
    assert len(tracks) == 1641 and sum(len(d) for d in tracks) == 6548 and all(1 <= k <= 35 for d in tracks for k in d)


# ------------------------------------------------------------------------------------------------ a synthetic scene
@functools.lru_cache(maxsize=None)
def synthetic_scene():
    """12 images see random subsets of 300 points, each image numbers its keypoints in an order of its own, plus 7
    keypoints that belong to no point; every pair of images is matched on the points both see.  Returns the graph and the
    point of every node (-1: none)."""
    rng = np.random.default_rng(2)
    n_img, n_pts, extra = 12, 300, 7
    sees = rng.random((n_img, n_pts)) < 0.35
    kp_of, counts, owner = [], [], []
    for i in range(n_img):
        vis = np.flatnonzero(sees[i])
        slots = rng.permutation(len(vis) + extra)
        kp = np.full(n_pts, -1)
        kp[vis] = slots[:len(vis)]
        own = np.full(len(vis) + extra, -1)
        own[kp[vis]] = vis
        kp_of.append(kp); counts.append(len(vis) + extra); owner.append(own)
    pairs, matches = [], []
    for i in range(n_img):
        for j in range(i + 1, n_img):
            both = rng.permutation(np.flatnonzero(sees[i] & sees[j]))
            a, b = (i, j) if (i + j) % 2 else (j, i)                          # both directions occur
            pairs.append((a, b)); matches.append((kp_of[a][both], kp_of[b][both]))
    return tr.pack(counts, pairs, matches), np.concatenate(owner)


def test_synthetic_scene_recovers_the_true_partition(gpu_ready):
    g, owner = synthetic_scene()
    out = check(g, "scene", min_lens=(2, 3))
    out = device(g, 2, "drop")
    assert out["counts"][2] == 0 and out["counts"][3] == 0
    in_track = out["node_track"] >= 0
    n_views = np.bincount(owner[owner >= 0], minlength=300)
    assert np.array_equal(in_track, (owner >= 0) & (n_views[np.maximum(owner, 0)] >= 2))
    # one track per point seen twice or more, and one point per track
    pt, trk = owner[in_track], out["node_track"][in_track]
    assert len(np.unique(pt)) == len(np.unique(trk)) == out["counts"][0] == len(set(zip(pt.tolist(), trk.tolist())))
    assert out["counts"][0] == int((n_views >= 2).sum()) and out["counts"][1] == int(n_views[n_views >= 2].sum())


def test_synthetic_scene_with_edges_removed(gpu_ready):
    (kp_ptr, seg_ptr, pairs, q, t, _), _ = synthetic_scene()
    rng = np.random.default_rng(3)
    mask = (rng.random(len(q)) >= 0.3).astype(np.uint8)
    out = check((kp_ptr, seg_ptr, pairs, q, t, mask), "masked", min_lens=(2, 3))
    # removing the edges instead of masking them is the same graph
    keep = mask != 0
    seg = np.repeat(np.arange(len(pairs)), np.diff(seg_ptr))[keep]
    ptr2 = np.concatenate([[0], np.cumsum(np.bincount(seg, minlength=len(pairs)))]).astype(np.int64)
    assert_equal(device((kp_ptr, ptr2, pairs, q[keep], t[keep], None), 3, "keep"), out, "removed")


def test_order_of_edges_and_pairs_does_not_matter(gpu_ready):
    kp_ptr, seg_ptr, pairs, q, t, mask, _, _ = shipped()
    base = device((kp_ptr, seg_ptr, pairs, q, t, None), 2, "keep")
    assert_equal(device((kp_ptr, seg_ptr, pairs, q, t, None), 2, "keep"), base, "second run")
    rng = np.random.default_rng(4)
    # edges permuted inside every pair
    perm = np.concatenate([seg_ptr[s] + rng.permutation(seg_ptr[s + 1] - seg_ptr[s]) for s in range(len(pairs))])
    assert_equal(device((kp_ptr, seg_ptr, pairs, q[perm], t[perm], None), 2, "keep"), base, "edges permuted")
    # pairs permuted, and every other pair given the other way round
    order = rng.permutation(len(pairs))
    flip = rng.random(len(pairs)) < 0.5
    qs, ts, ps = [], [], []
    for s in order:
        a, b = q[seg_ptr[s]:seg_ptr[s + 1]], t[seg_ptr[s]:seg_ptr[s + 1]]
        qs.append(b if flip[s] else a); ts.append(a if flip[s] else b); ps.append(pairs[s][::-1] if flip[s] else pairs[s])
    g = tr.pack([500] * 35, ps, list(zip(qs, ts)))
    assert_equal(device(g, 2, "keep"), base, "pairs permuted")


# ---------------------------------------------------------------------------------- components across all workgroups
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_path_of_40000_nodes(gpu_ready, order):
    """One keypoint per image and 157 workgroups of nodes: one component that crosses every XCD, as one track of 40,000
    views (sorted in global memory)."""
    n = 40000
    k = np.arange(n - 1)
    if order == "descending":
        k = k[::-1].copy()
    elif order == "shuffled":
        k = np.random.default_rng(6).permutation(n - 1)
    a, b = k, k + 1
    if order == "shuffled":
        a, b = np.where(k % 2 == 0, a, b), np.where(k % 2 == 0, b, a)
    out = device(one_keypoint_graph(n, a, b), 2, "drop")
    assert out["counts"].tolist() == [1, n, 0, 0] and out["track_ptr"].tolist() == [0, n]
    assert np.array_equal(out["obs_image"], np.arange(n)) and not out["obs_kp"].any() and not out["node_track"].any()
    assert out["track_conflict"].tolist() == [0]


def test_star_of_40000_nodes(gpu_ready):
    n, hub = 40000, 23456
    leaves = np.delete(np.arange(n), hub)
    g = one_keypoint_graph(n, np.random.default_rng(7).permutation(leaves), np.full(n - 1, hub))
    out = device(g, 2, "drop")
    assert out["counts"].tolist() == [1, n, 0, 0] and np.array_equal(out["obs_image"], np.arange(n))
    assert not out["node_track"].any()


def test_100000_two_node_components(gpu_ready):
    n = 100000
    rng = np.random.default_rng(8)
    partner = rng.permutation(n)
    g = tr.pack([n, n], [(0, 1)], [(np.arange(n), partner)])
    out = device(g, 2, "drop")
    assert out["counts"].tolist() == [n, 2 * n, 0, 0]
    assert np.array_equal(out["track_ptr"], 2 * np.arange(n + 1))
    assert np.array_equal(out["obs_image"], np.tile([0, 1], n)) and np.array_equal(out["obs_kp"][0::2], np.arange(n))
    assert np.array_equal(out["obs_kp"][1::2], partner)
    assert np.array_equal(out["node_track"][:n], np.arange(n)) and np.array_equal(out["node_track"][n + partner], np.arange(n))
    assert device(g, 3, "drop")["counts"].tolist() == [0, 0, 0, 0] and (device(g, 3, "drop")["node_track"] == -2).all()


@pytest.mark.parametrize("n", [65536, 65537, 131329])
def test_node_blocks_around_the_scan_of_the_block_sums(gpu_ready, n):
    """256, 257 and 514 workgroups of nodes for the one workgroup that scans their sums (a sum per thread, then two with
    the last threads empty, then a ragged last run): two-node components, and one node left over where n is odd."""
    n2 = n // 2
    g = tr.pack([n - n2, n2], [(0, 1)], [(np.arange(n2), np.random.default_rng(n).permutation(n2))])
    out = check(g, n, policies=("drop",))
    assert out["counts"].tolist() == [n2, 2 * n2, 0, 0] and int((out["node_track"] == -1).sum()) == n % 2


@pytest.mark.parametrize("n_edges", [63, 64, 65, 255, 256, 257])
def test_edge_counts_around_wavefronts_and_workgroups(gpu_ready, n_edges):
    rng = np.random.default_rng(n_edges)
    counts = rng.integers(20, 60, 9)
    pairs, matches, left = [], [], n_edges
    while left:
        i, j = rng.choice(9, 2, replace=False)
        m = min(left, int(rng.integers(1, 40)))
        pairs.append((i, j)); matches.append((rng.integers(0, counts[i], m), rng.integers(0, counts[j], m)))
        left -= m
    g = tr.pack(counts, pairs, matches)
    assert len(g[3]) == n_edges
    check(g, n_edges, min_lens=(2, 4))


# ------------------------------------------------------------------------------------------------------ long tracks
def test_long_tracks_of_3000_views(gpu_ready):
    """A conflict-free track of 3,000 views and a conflicting one of 3,000 nodes side by side (the workgroup sort in LDS),
    among short ones; under "keep" the conflicting one stays and is flagged."""
    rng = np.random.default_rng(9)
    n_img = 3000
    counts = np.full(n_img, 3)
    pairs, matches = [], []
    for i in rng.permutation(n_img - 1):
        pairs.append((i, i + 1)); matches.append(([0], [0]))                  # keypoint 0 of every image: one clean track
    for i in rng.permutation(1499):                                           # keypoints 1 and 2 of images 0..1499: conflicting
        pairs.append((i + 1, i)); matches.append(([1, 2], [1, 2]))
    pairs.append((0, 1)); matches.append(([1], [2]))                          # ties the two chains into one component
    for i in range(1500, 2999, 2):                                            # short tracks behind them
        pairs.append((i, i + 1)); matches.append(([1], [2]))
    g = tr.pack(counts, pairs, matches)
    keep = check(g, "long", min_lens=(2, 3))
    assert np.sort(np.diff(keep["track_ptr"]))[-2:].tolist() == [3000, 3000] and keep["track_conflict"].sum() == 1
    assert device(g, 2, "drop")["counts"][:3].tolist() == [1 + 750, 3000 + 1500, 1]


# ------------------------------------------------------------------------------------------------------- small cases
def test_duplicates_masks_and_empty_inputs(gpu_ready):
    from sfm_amd import build_tracks
    q, t = np.array([0, 1, 1, 0, 1]), np.array([2, 0, 0, 2, 0])
    g = tr.pack([2, 3, 2], [(0, 1), (1, 2), (0, 1)], [(q, t), (np.array([0, 0]), np.array([1, 1])), (q[:2], t[:2])])
    out = check(g, "duplicates")
    assert out["counts"].tolist() == [2, 5, 0, 0]
    once = tr.pack([2, 3, 2], [(0, 1), (1, 2)], [(q[:2], t[:2]), (np.array([0]), np.array([1]))])
    assert_equal(device(once, 2, "keep"), out, "without the duplicates")
    masked = g[:5] + (np.zeros(len(g[3]), np.uint8),)
    out = check(masked, "all masked")
    assert out["counts"].tolist() == [0, 0, 0, 0] and (out["node_track"] == -1).all() and out["track_ptr"].tolist() == [0]
    none = tr.pack([2, 3, 2], [], [])
    out = check(none, "no edges")
    assert (out["node_track"] == -1).all() and len(out["node_track"]) == 7 and out["track_ptr"].tolist() == [0]
    out = check(tr.pack([2, 3, 2], [(0, 1)], [(np.zeros(0, int), np.zeros(0, int))]), "an empty pair")
    assert out["counts"].tolist() == [0, 0, 0, 0]
    out = check(tr.pack([2, 3, 2], [(2, 0)], [([1], [0])]), "one edge", min_lens=(2, 3))
    assert device(tr.pack([2, 3, 2], [(2, 0)], [([1], [0])]))["node_track"].tolist() == [0, -1, -1, -1, -1, -1, 0]
    T = build_tracks([], [], [])
    assert len(T) == 0 and T.n_obs == 0 and len(T.node_track) == 0
    T = build_tracks([0, 4, 0], [], [])
    assert len(T) == 0 and T.node_track.tolist() == [-1] * 4


def test_bad_edges_are_counted_and_skipped(gpu_ready):
    """A raw call with edges the wrapper would have refused: an image with itself, images out of range, keypoints outside
    their image (one whose node id would fall into the next image, one past the last node), an edge in no segment.  They
    are counted, never followed, and the good edges give what they give alone."""
    kp_ptr = np.array([0, 4, 4, 9, 12], dtype=np.int64)                       # image 1 has no keypoints
    good = [((0, 2), [0, 1, 3], [4, 0, 2]), ((2, 3), [4, 0], [0, 2]), ((3, 0), [1], [2])]
    bad = [((2, 2), [0, 1], [1, 2]), ((0, 4), [0], [0]), ((-1, 2), [0], [0]), ((0, 2), [4, -1], [0, 0]),
           ((0, 1), [0], [0]), ((2, 3), [1, 2], [3, 7]), ((7, 9), [0], [0])]
    mixed = [good[0], bad[0], bad[1], good[1], bad[2], bad[3], bad[4], good[2], bad[5], bad[6]]
    flat = lambda items: tr.pack(np.diff(kp_ptr), [p for p, _, _ in items], [(q, t) for _, q, t in items])
    g, alone = flat(mixed), flat(good)
    n_bad = sum(len(q) for _, q, _ in bad)
    # one more edge behind the last segment, and one masked bad edge that is not counted
    q = np.concatenate([g[3], [0, 9]]).astype(np.int32)
    t = np.concatenate([g[4], [0, 0]]).astype(np.int32)
    seg_ptr = np.concatenate([g[1][:-1], [g[1][-1] + 1]])                     # the last pair (7, 9) takes the masked one
    mask = np.ones(len(q), np.uint8)
    mask[-2] = 0
    full = (g[0], seg_ptr, g[2], q, t, mask)
    ref = tr.build(*full, policy="keep")
    assert ref["counts"][3] == n_bad + 1
    for policy in ("drop", "keep"):
        out = device(full, 2, policy)
        assert_equal(out, tr.build(*full, policy=policy), policy)
        want = device(alone, 2, policy)
        for k in ("track_ptr", "obs_image", "obs_kp", "track_conflict", "node_track"):
            assert np.array_equal(out[k], want[k]), k
        assert out["counts"][:3].tolist() == want["counts"][:3].tolist() and want["counts"][3] == 0


def test_small_buffers_and_bad_options_are_rejected(gpu_ready):
    import ctypes as C
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    kp = torch.tensor([0, 5, 10], dtype=torch.int64, device=dev)
    seg = torch.tensor([0, 1], dtype=torch.int64, device=dev)            # one pair with one edge: image 0 with itself, bad
    pair, idx = torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    track_ptr, counts = torch.zeros(6, dtype=torch.int64, device=dev), torch.full((5,), 7, dtype=torch.int64, device=dev)
    obs_i, obs_k, node = (torch.zeros(10, dtype=torch.int32, device=dev) for _ in range(3))
    conflict = torch.zeros(5, dtype=torch.uint8, device=dev)
    need = C.c_int64()
    assert h.lib.sfm_tracks_workspace_bytes(10, 1, C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)

    def call(min_len=2, policy=0, cap_t=5, cap_o=10, ws_bytes=need.value):
        return h.lib.sfm_tracks_build(h._h, _p(kp), 2, 10, _p(seg), 1, _p(pair), _p(idx), _p(idx), None, 1, min_len, policy,
                                      _p(track_ptr), _p(obs_i), _p(obs_k), _p(conflict), _p(node), _p(counts), cap_t, cap_o,
                                      _p(ws), ws_bytes)
    assert call(cap_t=4) == -1 and b"cap_tracks" in h.lib.sfm_last_error(h._h)
    assert call(cap_o=9) == -1
    assert call(min_len=1) == -1 and b"min_len" in h.lib.sfm_last_error(h._h)
    assert call(policy=2) == -1
    assert call(ws_bytes=need.value - 1) == -3
    assert counts.tolist() == [7] * 5                                    # nothing ran
    assert call() == 0
    assert counts.tolist() == [0, 0, 0, 1, 0] and node.tolist() == [-1] * 10 and track_ptr[0].item() == 0


# ------------------------------------------------------------------------------------------------------- the chain
def test_process_pairs_then_build_tracks(gpu_ready):
    """match -> F -> verify -> tracks on a small synthetic set: four cameras on 200 points with descriptors of their own.
    The tracks are what the reference makes of the matches and masks process_pairs returned, and nearly every track is
    one true point."""
    from sfm_amd.matcher import ImageMatcher
    import fundamental_reference as fr
    rng = np.random.default_rng(21)
    N, n_cam, extra = 200, 4, 30
    X = rng.uniform(-1, 1, (N, 3)) + [0, 0, 6.0]
    base = rng.integers(0, 256, (N, 128)).astype(np.float32)
    kps, descs, owner = [], [], []
    for c in range(n_cam):
        yaw = 0.15 * c
        R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
        x = (X @ R.T + [-0.9 * c, 0.1 * c, 0.2 * c]) @ fr.K_REF.T
        x = x[:, :2] / x[:, 2:] + rng.normal(size=(N, 2)) * 0.3
        perm = rng.permutation(N)
        kps.append(np.concatenate([x[perm], rng.uniform(0, 1, (extra, 2)) * [1024, 768]]).astype(np.float32))
        d = np.clip(base[perm] + rng.integers(-3, 4, (N, 128)), 0, 255).astype(np.float32)
        descs.append(np.concatenate([d, rng.integers(0, 256, (extra, 128)).astype(np.float32)]))
        owner.append(np.concatenate([perm, np.full(extra, -1)]))
    kps.append(kps[0][:3]); descs.append(descs[0][:3]); owner.append(owner[0][:3])      # under min_matches: no result
    pairs = [(0, 1), (0, 2), (1, 2), (4, 1), (2, 3), (3, 0)]
    m = ImageMatcher()
    results = m.process_pairs(kps, descs, pairs)
    assert results[3] is None and sum(r is not None for r in results) == 5
    T = m.build_tracks(kps, pairs, results, min_length=2)
    live = [s for s, r in enumerate(results) if r is not None]
    g = tr.pack([len(k) for k in kps], [pairs[s] for s in live],
                [(results[s]["matches"].queryIdx, results[s]["matches"].trainIdx) for s in live],
                masks=[results[s]["inlier_mask"] for s in live])
    ref = tr.build(*g)
    assert np.array_equal(T.track_ptr, ref["track_ptr"]) and np.array_equal(T.image, ref["obs_image"])
    assert np.array_equal(T.keypoint, ref["obs_kp"]) and np.array_equal(T.node_track, ref["node_track"])
    assert np.array_equal(T.conflict, ref["track_conflict"]) and T.n_conflicting == ref["counts"][2]
    own = np.concatenate(owner)[T.kp_ptr[T.image] + T.keypoint]
    pure = sum(len(set(own[T.track_ptr[k]:T.track_ptr[k + 1]])) == 1 for k in range(len(T)))
    print(f"{len(T)} tracks, {T.n_obs} observations, {int((T.lengths() >= 3).sum())} of three or more views, {pure} of one point")
    assert len(T) >= 150 and (T.lengths() >= 3).sum() >= 100 and pure >= 0.95 * len(T)
    cam, pt, uv = T.observations(kps)
    assert np.array_equal(uv, np.concatenate(kps).astype(np.float64)[T.kp_ptr[T.image] + T.keypoint])
    allm = m.build_tracks(kps, pairs, results, verified_only=False, conflicts="keep")
    assert allm.n_obs >= T.n_obs
