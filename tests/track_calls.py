"""The track-judging entry points on flat host arrays, for the tests that call the C ABI directly: the source arguments
the four share and the two calls at points that are given, every output filled with a sentinel first."""
import ctypes as C

import numpy as np


def upload(args, X=None, has_point=None):
    """args = (proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp).  Returns (the device tensors, which must
    outlive the call; the 12 source arguments of include/sfm_amd.h; the device (X, has_point), or None)."""
    import torch
    from sfm_amd.driver import _p
    up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt, order="C")).to(torch.device("cuda", 0))
    proj, cam, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp = args
    d = [up(np.asarray(proj, dtype=np.float64).reshape(-1, 12), np.float64), up(cam, np.int32), up(kp_ptr, np.int64),
         up(np.asarray(kp_xy).reshape(-1, 2), np.float64), up(track_ptr, np.int64), up(obs_image, np.int32), up(obs_kp, np.int32)]
    source = (_p(d[0]), len(d[0]), _p(d[1]), len(cam), _p(d[2]), _p(d[3]), len(d[3]), _p(d[4]), len(track_ptr) - 1, _p(d[5]),
              _p(d[6]), len(obs_image))
    point = None if X is None else (up(np.asarray(X).reshape(-1, 3), np.float64), up(np.asarray(has_point) != 0, np.uint8))
    return d, source, point


def judge_raw(entry, args, X, has_point, want_obs_err=True, **opts):
    """`entry` = "sfm_tracks_evaluate": {status, n_views, max_err, obs_err, counts}; "sfm_tracks_classify": these and
    {n_inliers, obs_inlier}.  Sentinels: 77 in the int and uint8 outputs, 7 in counts, 0.0 in the doubles."""
    import torch
    from sfm_amd import _lib
    from sfm_amd.driver import _p
    assert entry in ("sfm_tracks_evaluate", "sfm_tracks_classify")
    o = dict(dict(min_views=2, max_error=4.0, min_angle_deg=0.0), **opts)
    h = _lib.get_handle(0)
    keep, source, (dX, dhas) = upload(args, X, has_point)
    n_cams, n_tracks, n_obs = source[1], source[8], source[11]
    need = C.c_int64()
    assert h.lib.sfm_triangulate_tracks_workspace_bytes(n_cams, C.byref(need)) == 0
    fill = lambda n, v, dt: torch.full((n,), v, dtype=dt, device=dX.device)
    ws, counts = fill(need.value, 0, torch.uint8), fill(6, 7, torch.int64)
    out = {"status": fill(n_tracks, 77, torch.int32), "n_views": fill(n_tracks, 77, torch.int32),      # in the order of the header
           "n_inliers": fill(n_tracks, 77, torch.int32), "max_err": fill(n_tracks, 0.0, torch.float64),
           "obs_inlier": fill(max(n_obs, 1), 77, torch.uint8),
           "obs_err": fill(max(n_obs, 1), 0.0, torch.float64) if want_obs_err else None}
    if entry == "sfm_tracks_evaluate":
        del out["n_inliers"], out["obs_inlier"]
    h.call(entry, *source, _p(dX), _p(dhas), int(o["min_views"]), C.c_double(o["max_error"]), C.c_double(o["min_angle_deg"]),
           *(_p(t) for t in out.values()), _p(counts), _p(ws), need.value)
    out = {k: None if t is None else t.cpu().numpy()[:n_obs if k.startswith("obs_") else None] for k, t in out.items()}
    return dict(out, counts=counts.cpu().numpy())
