"""CPU tests of the track-building contract: the two restatements of tests/tracks_reference.py against each other and
against the figures of the shipped matches, the host-side planning header under the sanitizers, and everything of
sfm_amd.tracks that needs no device.  No GPU."""
import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import tracks_reference as tr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def shipped():
    """The 148 shipped pairs as flat arrays: 35 images (ids 1..35 -> positions 0..34) of 500 keypoints each.
    (kp_ptr, seg_ptr, pair_img, queryIdx, trainIdx, verification mask uint8, pts1, pts2) - never modified."""
    bm = np.load(os.path.join(GOLDEN, "bunny_matches.npz"), allow_pickle=False)
    bp = np.load(os.path.join(GOLDEN, "bunny_pairs.npz"), allow_pickle=False)
    assert [n.replace("_matches.npz", "") for n in bm["names"]] == [str(n) for n in bp["names"]]
    assert np.array_equal(bm["offsets"], bp["offsets"])
    pairs = np.array([[int(x) - 1 for x in str(n).split("_")[1:3]] for n in bp["names"]], dtype=np.int32)
    out = (np.arange(36, dtype=np.int64) * 500, bm["offsets"].astype(np.int64), pairs, bm["queryIdx"].astype(np.int32),
           bm["trainIdx"].astype(np.int32), bp["mask"].astype(np.uint8), bp["pts1"], bp["pts2"])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def shipped_reference(verified, policy, min_len):
    kp_ptr, seg_ptr, pairs, q, t, mask, _, _ = shipped()
    return tr.build(kp_ptr, seg_ptr, pairs, q, t, mask if verified else None, min_len=min_len, policy=policy)


def random_graph(rng, n_img, max_kp, n_seg, max_edges, bad=0.0, masked=0.0):
    counts = rng.integers(0, max_kp + 1, n_img)
    kp_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pairs, qs, ts = [], [], []
    for _ in range(n_seg):
        i, j = rng.integers(0, n_img, 2)
        if rng.random() < bad:
            i, j = rng.choice([-1, n_img, i]), rng.choice([j, i])
        m = int(rng.integers(0, max_edges + 1))
        hi_i = counts[i] if 0 <= i < n_img and counts[i] > 0 else 1
        hi_j = counts[j] if 0 <= j < n_img and counts[j] > 0 else 1
        q, t = rng.integers(0, hi_i, m), rng.integers(0, hi_j, m)
        wrong = rng.random(m) < bad
        q = np.where(wrong, rng.choice([-1, hi_i, hi_i + 7], m), q)
        pairs.append((i, j)); qs.append(q); ts.append(t)
    seg_ptr = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int64)
    q = np.concatenate(qs).astype(np.int32) if qs else np.zeros(0, np.int32)
    t = np.concatenate(ts).astype(np.int32) if ts else np.zeros(0, np.int32)
    mask = (rng.random(len(q)) >= masked).astype(np.uint8) if masked else None
    return kp_ptr, seg_ptr, np.array(pairs, dtype=np.int32).reshape(-1, 2), q, t, mask


# ------------------------------------------------------------------------------------- the two restatements agree
@pytest.mark.parametrize("verified", [True, False])
def test_restatements_agree_on_the_shipped_matches(verified):
    kp_ptr, seg_ptr, pairs, q, t, mask, _, _ = shipped()
    for policy in ("drop", "keep"):
        for min_len in (2, 3):
            a = shipped_reference(verified, policy, min_len)
            b = tr.build_union_find(kp_ptr, seg_ptr, pairs, q, t, mask if verified else None, min_len=min_len, policy=policy)
            assert tr.same(a, b), (verified, policy, min_len)


def test_restatements_agree_on_random_graphs():
    rng = np.random.default_rng(11)
    n_tracks = n_conf = n_bad = 0
    for k in range(60):
        g = random_graph(rng, int(rng.integers(2, 9)), int(rng.integers(1, 30)), int(rng.integers(0, 12)), 8,
                         bad=0.15 if k % 3 == 0 else 0.0, masked=0.3 if k % 2 else 0.0)
        for policy in ("drop", "keep"):
            for min_len in (2, 3, 5):
                a = tr.build(*g, min_len=min_len, policy=policy)
                b = tr.build_union_find(*g, min_len=min_len, policy=policy)
                assert tr.same(a, b), (k, policy, min_len)
        a = tr.build(*g, min_len=2, policy="keep")
        n_tracks += a["counts"][0]; n_conf += a["counts"][2]; n_bad += a["counts"][3]
    print("tracks", n_tracks, "conflicting", n_conf, "bad edges", n_bad)
    assert n_tracks > 100 and n_conf > 20 and n_bad > 50          # the cases are not trivial ones


def test_output_invariants_on_random_graphs():
    rng = np.random.default_rng(5)
    for k in range(20):
        g = random_graph(rng, 6, 20, 10, 30, masked=0.2)
        kp_ptr = g[0]
        for policy in ("drop", "keep"):
            r = tr.build(*g, min_len=2, policy=policy)
            n_tracks, n_obs = r["counts"][:2]
            assert n_tracks <= kp_ptr[-1] // 2 and n_obs <= kp_ptr[-1]
            node = kp_ptr[r["obs_image"]] + r["obs_kp"]
            firsts = node[r["track_ptr"][:-1]]
            assert (np.diff(firsts) > 0).all()                               # tracks by their smallest node
            for t in range(n_tracks):
                mem = node[r["track_ptr"][t]:r["track_ptr"][t + 1]]
                assert (np.diff(mem) > 0).all() and (r["node_track"][mem] == t).all()
                img = r["obs_image"][r["track_ptr"][t]:r["track_ptr"][t + 1]]
                assert bool(r["track_conflict"][t]) == (len(set(img)) < len(img))
            assert (r["node_track"] >= 0).sum() == n_obs
            if policy == "drop":
                assert not r["track_conflict"].any()
            else:
                assert (r["node_track"] != tr.DROPPED).all() and r["track_conflict"].sum() == r["counts"][2]


# --------------------------------------------------------------------------------------------- the shipped figures
def test_figures_of_the_shipped_matches():
    kp_ptr, seg_ptr, pairs, q, t, mask, _, _ = shipped()
    assert len(pairs) == 148 and len(kp_ptr) == 36 and q.max() <= 499 and t.max() <= 499 and q.min() >= 0

    def figures(verified):
        a, b, n_bad = tr.valid_edges(kp_ptr, seg_ptr, pairs, q, t, mask if verified else None)
        keep, drop = shipped_reference(verified, "keep", 2), shipped_reference(verified, "drop", 2)
        lk, ld = np.diff(keep["track_ptr"]), np.diff(drop["track_ptr"])
        assert n_bad == 0 and keep["counts"][3] == 0
        return {"edges": len(a), "keypoints": len(np.unique(np.r_[a, b])), "components": int(keep["counts"][0]),
                "three_or_more": int((lk >= 3).sum()), "longest": int(lk.max()), "conflicting": int(keep["counts"][2]),
                "tracks": int(drop["counts"][0]), "observations": int(drop["counts"][1]),
                "tracks_three_or_more": int((ld >= 3).sum()), "longest_track": int(ld.max()), "mean": float(ld.mean())}

    v = figures(True)
    mean = v.pop("mean")
    assert v == {"edges": 9817, "keypoints": 6960, "components": 1697, "three_or_more": 1105, "longest": 19,
                 "conflicting": 56, "tracks": 1641, "observations": 6548, "tracks_three_or_more": 1049, "longest_track": 12}
    assert round(mean, 2) == 3.99
    a = figures(False)
    assert (a["edges"], a["keypoints"], a["components"], a["conflicting"], a["longest"], a["tracks"], a["observations"],
            a["longest_track"]) == (10907, 7809, 1804, 119, 49, 1685, 6602, 13)
    # the state the reference ships: two views per point, whatever the matches hold
    s = np.load(os.path.join(GOLDEN, "bunny_state.npz"), allow_pickle=False)
    assert s["pts"].shape[0] == 2555


def test_keypoint_positions_are_consistent_across_pairs():
    """Every keypoint has one pixel position in every pair it occurs in: tracks keyed by index lose nothing."""
    kp_ptr, seg_ptr, pairs, q, t, _, pts1, pts2 = shipped()
    seg = np.repeat(np.arange(len(pairs)), np.diff(seg_ptr))
    node = np.r_[kp_ptr[pairs[seg, 0]] + q, kp_ptr[pairs[seg, 1]] + t]
    xy = np.r_[pts1, pts2]
    order = np.argsort(node, kind="stable")
    node, xy = node[order], xy[order]
    same_node = node[1:] == node[:-1]
    assert same_node.sum() > 10000
    assert (xy[1:][same_node] == xy[:-1][same_node]).all()


# ------------------------------------------------------------------------------------- the planning header, on a CPU
def test_tracks_plan_under_address_and_ub_sanitizers(tmp_path):
    """sfm_amd/csrc/tracks_plan.h (workspace layout, size checks, lane / LDS / global route, the comparators of the sorting
    network the workgroup kernel runs) is plain C++: built with g++ -fsanitize=address,undefined and driven over sizes up to
    2^31 - 1 and every length from 1 to 300 and around the powers of two."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "tracks_plan_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "sfm_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "tracks_plan_check.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    for seed in (1, 2):
        run = subprocess.run([str(exe), str(seed)], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])


# ------------------------------------------------------------------------------------ the Python side without a device
def hand_made():
    """Two tracks over three images: {(0,1), (1,0), (2,2)} and {(0,2), (2,0)}."""
    from sfm_amd.tracks import Tracks
    kps = [np.array([[0, 0], [10, 11], [20, 21]], np.float32), np.array([[30.5, 31], [40, 41]], np.float32),
           np.array([[50, 51], [60, 61], [70, 71.25]], np.float32)]
    t = Tracks([0, 3, 5, 8], [0, 3, 5], [0, 1, 2, 0, 2], [1, 0, 2, 2, 0], conflict=[0, 0],
               node_track=[-1, 0, 1, 0, -1, 1, -1, 0], n_conflicting=0)
    return t, kps


def test_tracks_container_on_a_hand_made_csr():
    from sfm_amd.tracks import Tracks
    t, kps = hand_made()
    assert len(t) == 2 and t.n_obs == 5 and t.lengths().tolist() == [3, 2]
    cam, pt, uv = t.observations(kps)
    assert cam.dtype == np.int32 and pt.dtype == np.int32 and uv.dtype == np.float64 and uv.shape == (5, 2)
    assert cam.tolist() == [0, 1, 2, 0, 2] and pt.tolist() == [0, 0, 0, 1, 1]
    assert uv.tolist() == [[10, 11], [30.5, 31], [70, 71.25], [20, 21], [50, 51]]
    assert (np.diff(pt) >= 0).all()                                     # point-major, as pack_state sorts
    assert t.as_point_tracks(kps) == [{0: [10.0, 11.0], 1: [30.5, 31.0], 2: [70.0, 71.25]}, {0: [20.0, 21.0], 2: [50.0, 51.0]}]
    assert t.as_point_tracks(kps, image_ids=[7, 8, 12])[1] == {7: [20.0, 21.0], 12: [50.0, 51.0]}
    t.image_ids = [3, 4, 5]
    assert list(t.as_point_tracks(kps)[1]) == [3, 5]
    # the same scene through the reference, and the container takes its arrays as they are
    r = tr.build([0, 3, 5, 8], [0, 1, 3], [[0, 1], [2, 0]], [1, 2, 0], [0, 1, 2])
    u = Tracks([0, 3, 5, 8], r["track_ptr"], r["obs_image"], r["obs_kp"], r["track_conflict"], r["node_track"])
    assert u.track_ptr.tolist() == [0, 3, 5] and u.image.tolist() == [0, 1, 2, 0, 2] and u.keypoint.tolist() == [1, 0, 2, 2, 0]
    assert u.node_track.tolist() == t.node_track.tolist()
    empty = Tracks([0, 3], [0], [], [])
    assert len(empty) == 0 and empty.observations(kps)[2].shape == (0, 2) and empty.as_point_tracks(kps) == []
    with pytest.raises(ValueError):
        Tracks([0, 3], [0, 2], [0], [0])
    with pytest.raises(ValueError):
        Tracks([0, 3], [0, 1], [0], [0, 1])


def test_observations_feed_pack_state_shapes():
    """cam_idx / pt_idx / uv have the dtypes and the point-major order of the BA's packed observations."""
    from sfm_amd import ba
    t, kps = hand_made()
    cam, pt, uv = t.observations(kps)
    assert hasattr(ba, "GpuBA")
    assert cam.shape == pt.shape == (5,) and uv.shape == (5, 2)
    assert cam.max() < len(t.kp_ptr) - 1 and pt.max() == len(t) - 1


def test_argument_checks_need_no_device(tmp_path):
    import sfm_amd
    from sfm_amd import tracks
    from sfm_amd.matcher import DMatchList, ImageMatcher
    assert sfm_amd.build_tracks is tracks.build_tracks and sfm_amd.Tracks is tracks.Tracks
    q, t = np.array([0, 1]), np.array([1, 0])
    bad_calls = [
        dict(n_keypoints=[2, 2], pairs=[(0, 2)], matches=[(q, t)]),                    # image out of range
        dict(n_keypoints=[2, 2], pairs=[(-1, 1)], matches=[(q, t)]),
        dict(n_keypoints=[2, 2], pairs=[(1, 1)], matches=[(q, t)]),                    # an image with itself
        dict(n_keypoints=[2, 2], pairs=[(0, 1)], matches=[(np.array([0, 2]), t)]),     # keypoint out of range
        dict(n_keypoints=[2, 2], pairs=[(0, 1)], matches=[(q, np.array([-1, 0]))]),
        dict(n_keypoints=[2, 2], pairs=[(0, 1)], matches=[(q, t[:1])]),                # lengths differ
        dict(n_keypoints=[2, 2], pairs=[(0, 1)], matches=[(q, t)], masks=[np.ones(3)]),
        dict(n_keypoints=[2, 2], pairs=[(0, 1)], matches=[(q, t)], masks=[]),
        dict(n_keypoints=[2, 2], pairs=[(0, 1), (1, 0)], matches=[(q, t)]),
        dict(n_keypoints=[2, -2], pairs=[(0, 1)], matches=[(q, t)]),
        dict(n_keypoints=[2, 2], pairs=[(0, 1)], matches=[(q.astype(float), t)]),      # indices must be integers
        dict(n_keypoints=[2, 2], pairs=[(0, 1)], matches=[(q, t)], min_length=1),
        dict(n_keypoints=[2, 2], pairs=[(0, 1)], matches=[(q, t)], conflicts="split"),
        dict(n_keypoints=[2, 2], pairs=[(0, 1)], matches=[DMatchList([0, 5], [1, 0], [1.0, 2.0])]),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            tracks.build_tracks(**kw)
    with pytest.raises(ValueError):
        ImageMatcher().build_tracks([np.zeros((2, 2))] * 2, [(0, 1)], [])
    with pytest.raises(ValueError):
        ImageMatcher().build_tracks([np.zeros((2, 2))] * 2, [(0, 1)],
                                    [{"matches": DMatchList([0, 2], [1, 0], [1.0, 2.0]), "inlier_mask": np.ones(2, bool)}])
    with pytest.raises(ValueError):
        tracks.tracks_from_pair_files(tmp_path, ["pair_1"])
    with pytest.raises(FileNotFoundError):
        tracks.tracks_from_pair_files(tmp_path, ["pair_1_2"])
    # what the wrapper hands to the device is what the reference takes
    kp_ptr, seg_ptr, pair_img, qq, tt, mask = tracks.pack_matches([3, 2, 3], [(0, 1), (2, 0)], [(np.array([1, 2]), np.array([0, 1])),
                                                                                              DMatchList([2, 0], [1, 2], [0.5, 0.25])],
                                                                  masks=[None, np.array([True, False])])
    assert kp_ptr.tolist() == [0, 3, 5, 8] and seg_ptr.tolist() == [0, 2, 4] and pair_img.tolist() == [[0, 1], [2, 0]]
    assert qq.dtype == np.int32 and tt.dtype == np.int32 and mask.tolist() == [1, 1, 1, 0]
    r = tr.build(kp_ptr, seg_ptr, pair_img, qq, tt, mask)
    assert r["track_ptr"].tolist() == [0, 3, 5] and r["obs_kp"].tolist() == [1, 0, 2, 2, 1]


def test_c_entry_points_reject_bad_calls_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    assert lib.sfm_tracks_build(None, None, 0, 0, None, 0, None, None, None, None, 0, 2, 0, None, None, None, None, None, None,
                                0, 0, None, 0) != 0
    need = ctypes.c_int64(-1)
    assert lib.sfm_tracks_workspace_bytes(1000, 5000, ctypes.byref(need)) == 0 and need.value >= 5 * 4 * 1000
    assert lib.sfm_tracks_workspace_bytes(0, 0, ctypes.byref(need)) == 0 and need.value > 0
    assert lib.sfm_tracks_workspace_bytes(-1, 0, ctypes.byref(need)) != 0
    assert lib.sfm_tracks_workspace_bytes(2 ** 31, 0, ctypes.byref(need)) != 0
    assert lib.sfm_tracks_workspace_bytes(10, 10, None) != 0
