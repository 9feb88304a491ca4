"""The frame the four track-judging entry points share (sfm_triangulate_tracks, sfm_triangulate_tracks_robust,
sfm_tracks_evaluate, sfm_tracks_classify; track_call_begin of sfm_amd/csrc/triangulate.hip), one entry point at a time:
what each kind of bad call returns and what it leaves untouched, then a valid call against the NumPy restatements.

The scene is the smallest that has a used and an unused observation in one track and more than one track per wavefront:
3 cameras on an arc, 4 images of which image 2 is not registered, 5 tracks of 2 to 3 views, pixel noise 0.5.  Every output
is filled with a sentinel before every call; every bad call is turned down on the host before any launch.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import incremental_reference as ir
import triangulate_reference as tr
import triangulate_robust_reference as rr
from test_triangulate_reference import rel_dev_scalars
from track_calls import judge_raw, upload

pytestmark = pytest.mark.gpu

GATES = dict(min_views=2, max_error=4.0, min_angle_deg=1.0)
REFINE_ITERS = 5
ENTRIES = ("sfm_triangulate_tracks", "sfm_triangulate_tracks_robust", "sfm_tracks_evaluate", "sfm_tracks_classify")
# outputs in the order of include/sfm_amd.h, counts and the workspace aside; obs_err follows them in the judging calls
OUTPUTS = {"sfm_triangulate_tracks": ("X", "status", "n_views", "max_err"),
           "sfm_triangulate_tracks_robust": ("X", "status", "n_views", "n_inliers", "max_err", "obs_inlier"),
           "sfm_tracks_evaluate": ("status", "n_views", "max_err", "obs_err"),
           "sfm_tracks_classify": ("status", "n_views", "n_inliers", "max_err", "obs_inlier", "obs_err")}
SENTINEL = {"X": -7.0, "max_err": -7.0, "obs_err": -7.0, "status": 77, "n_views": 77, "n_inliers": 77, "obs_inlier": 77}


@functools.lru_cache(maxsize=None)
def scene():
    """(args, the reference triangulation of the five tracks, has_point of the judging calls: track 4 has none)."""
    rng = np.random.default_rng(61)
    proj = tr.arc_cameras(4)[0]                                                # image 2 projects somewhere; it has no camera
    X = rng.uniform(0, 1, (5, 3))
    cams = [np.array(c) for c in ([0, 1, 3], [0, 2, 3], [1, 2, 3], [0, 1], [1, 3])]
    g = tr.make_tracks(rng, proj, X, None, noise=0.5, cams=cams)
    args = (np.delete(proj.reshape(-1, 12), 2, axis=0), np.array([0, 1, -1, 2], np.int32)) + tuple(g)
    ref = tr.triangulate(*args, refine_iters=REFINE_ITERS, **GATES)
    return args, ref, np.array([1, 1, 1, 1, 0], np.uint8)


class Call:
    """One entry point on the scene, every output a sentinel-filled device tensor."""

    def __init__(self, entry):
        import torch
        from sfm_amd import _lib
        self.torch, self.entry = torch, entry
        self.h = _lib.get_handle(0)
        dev = torch.device("cuda", 0)
        args, ref, has = scene()
        self.judging = entry in ("sfm_tracks_evaluate", "sfm_tracks_classify")
        self.keep, self.source, self.point = upload(args, ref["X"], has)
        self.n_tracks, self.n_obs = self.source[8], self.source[11]
        need = C.c_int64()
        if entry == "sfm_triangulate_tracks_robust":
            assert self.h.lib.sfm_triangulate_tracks_robust_workspace_bytes(self.source[1], self.n_tracks, C.byref(need)) == 0
        else:
            assert self.h.lib.sfm_triangulate_tracks_workspace_bytes(self.source[1], C.byref(need)) == 0
        self.need = need.value
        self.ws = torch.empty(self.need, dtype=torch.uint8, device=dev)
        shape = {"X": (self.n_tracks, 3), "obs_inlier": (self.n_obs,), "obs_err": (self.n_obs,)}
        dtype = {"X": torch.float64, "max_err": torch.float64, "obs_err": torch.float64, "obs_inlier": torch.uint8}
        self.out = {k: torch.empty(shape.get(k, (self.n_tracks,)), dtype=dtype.get(k, torch.int32), device=dev) for k in OUTPUTS[entry]}
        self.counts = torch.empty(6, dtype=torch.int64, device=dev)
        self.fill()

    def fill(self):
        for k, t in self.out.items():
            t.fill_(SENTINEL[k])
        self.counts.fill_(7)

    def run(self, min_views=2, ws_bytes=None, n_tracks=None, null=()):
        """The return code of the call; `null`: the outputs passed as null pointers."""
        from sfm_amd.driver import _p
        self.fill()
        source = list(self.source)
        if n_tracks is not None:
            source[8] = n_tracks
        outs = [None if k in null else _p(t) for k, t in self.out.items()]
        gates = [C.c_double(GATES["max_error"]), C.c_double(GATES["min_angle_deg"])]
        options = [_p(self.point[0]), _p(self.point[1]), min_views] + gates if self.judging else [min_views, REFINE_ITERS] + gates
        return getattr(self.h.lib, self.entry)(self.h._h, *source, *options, *outs, _p(self.counts), _p(self.ws),
                                               self.need if ws_bytes is None else ws_bytes)

    def error(self):
        return self.h.lib.sfm_last_error(self.h._h)

    def outputs_untouched(self):
        self.torch.cuda.synchronize()
        return all(bool((t == SENTINEL[k]).all()) for k, t in self.out.items())

    def host(self):
        return dict({k: t.cpu().numpy() for k, t in self.out.items()}, counts=self.counts.cpu().numpy())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("entry", ENTRIES)
def test_frame_of_the_track_calls(gpu_ready, entry):
    args, ref, has = scene()
    c = Call(entry)
    # 1. an option out of range: nothing is touched, counts included, and the message names the entry point and the option
    assert c.run(min_views=1) == -1
    assert entry.encode() + b":" in c.error() and b"min_views" in c.error()
    assert c.outputs_untouched() and c.counts.tolist() == [7] * 6
    # 2. the workspace one byte short: counts were zeroed, nothing else
    assert c.run(ws_bytes=c.need - 1) == -3
    assert c.outputs_untouched() and c.counts.tolist() == [0] * 6
    # 3. a required output missing
    assert c.run(null=("status",)) == -1
    assert c.outputs_untouched() and c.counts.tolist() == [0] * 6
    # 4. no tracks
    assert c.run(n_tracks=0) == 0
    assert c.outputs_untouched() and c.counts.tolist() == [0] * 6
    # 5. a valid call
    assert c.run() == 0, c.error()
    out = c.host()
    if not c.judging:
        assert (ref["status"] == tr.OK).all() and ref["n_views"].tolist() == [3, 2, 2, 2, 2]
        assert out["counts"].sum() == 5 and np.array_equal(out["counts"], ref["counts"])
        assert np.array_equal(out["status"], ref["status"]) and np.array_equal(out["n_views"], ref["n_views"])
        assert np.array_equal(bits(out["X"]), bits(ref["X"]))
        ev = judge_raw("sfm_tracks_evaluate", args, out["X"], np.ones(5, np.uint8), **GATES)
        assert np.array_equal(bits(out["max_err"]), bits(ev["max_err"]))
        if entry == "sfm_triangulate_tracks_robust":                           # every track passed the first pass
            assert np.array_equal(out["n_inliers"], ref["n_views"]) and np.array_equal(out["obs_inlier"] != 0, args[1][args[5]] >= 0)
        return
    restate = ir.evaluate if entry == "sfm_tracks_evaluate" else rr.classify
    r, ld = restate(*args, ref["X"], has, **GATES), restate(*args, ref["X"], has, dtype=np.longdouble, **GATES)
    assert out["counts"].sum() == has.sum() == 4 and np.array_equal(out["counts"], r["counts"])
    assert np.array_equal(out["status"], r["status"]) and np.array_equal(out["n_views"], r["n_views"])
    assert r["status"].tolist() == [0, 0, 0, 0, ir.NO_POINT] and r["n_views"].tolist() == [3, 2, 2, 2, 2]
    ref_m, dev_m = rel_dev_scalars(r["max_err"], ld["max_err"]), rel_dev_scalars(out["max_err"], r["max_err"])
    print(f"{entry}: reference float64 against 80-bit max_err {ref_m:.3g}; device against reference max_err {dev_m:.3g}")
    assert dev_m <= 100 * ref_m
