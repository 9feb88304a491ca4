"""NumPy restatements for the incremental reconstruction (sfm_amd/incremental.py): the resection lists of
sfm_tracks_resection (exact: integers and copies), the gates of sfm_tracks_evaluate on top of
tests/triangulate_reference.py (generic over the dtype, so that np.longdouble stands in for the exact value), and a
similarity alignment of two camera / point sets for the loop tests."""
import numpy as np

import triangulate_reference as tr

NO_POINT = -1


def resection_lists(kp_ptr, kp_xy, node_track, cam_of_image, X, has_point):
    """{seg_ptr [n_img+1] int64, total, corr_node, corr_track int32, corr_X [n,3] float64, corr_uv [n,2] float32}: node n
    of image i is listed when cam_of_image[i] < 0, 0 <= node_track[n] < n_tracks and has_point[node_track[n]] != 0, in
    ascending node id; seg_ptr[i] = listed nodes below kp_ptr[i].  A node in no image is not listed."""
    kp_ptr = np.asarray(kp_ptr, dtype=np.int64)
    node_track = np.asarray(node_track, dtype=np.int64)
    cam_of_image = np.asarray(cam_of_image, dtype=np.int64)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    has_point = np.asarray(has_point)
    n_nodes, n_img, n_tracks = len(node_track), len(kp_ptr) - 1, len(has_point)
    node = np.arange(n_nodes)
    img = np.searchsorted(kp_ptr[:n_img], node, side="right") - 1          # the last image that starts at or below the node
    in_image = (img >= 0) & (kp_ptr[np.clip(img, 0, None)] <= node) & (node < kp_ptr[np.clip(img, 0, None) + 1]) if n_img else \
        np.zeros(n_nodes, bool)
    track_ok = (node_track >= 0) & (node_track < n_tracks)
    trk = np.where(track_ok, node_track, 0)
    flag = in_image & track_ok
    if n_nodes and n_img:
        flag &= cam_of_image[np.clip(img, 0, None)] < 0
    if n_tracks:
        flag &= has_point[trk] != 0
    else:
        flag &= False
    listed = np.flatnonzero(flag)
    below = np.concatenate([[0], np.cumsum(flag)]).astype(np.int64)
    seg_ptr = below[np.clip(kp_ptr, 0, n_nodes)]
    seg_ptr[n_img] = below[n_nodes]
    return {"seg_ptr": seg_ptr, "total": int(below[n_nodes]), "corr_node": listed.astype(np.int32),
            "corr_track": node_track[listed].astype(np.int32),
            "corr_X": X[node_track[listed]] if len(listed) else np.zeros((0, 3)),
            "corr_uv": np.asarray(kp_xy, dtype=np.float64).reshape(-1, 2)[listed].astype(np.float32)}


def evaluate(proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp, X, has_point, min_views=2, max_error=4.0,
             min_angle_deg=0.0, dtype=np.float64):
    """{status, n_views int32, max_err [T], obs_err [n_obs], counts [6] int64} in `dtype`: the gates of tr.triangulate at the
    given X, in its order; a track without a point gets NO_POINT, NaN and no place in counts; obs_err is NaN for an
    observation whose image is not registered or whose track has no point."""
    dtype = np.dtype(dtype)
    P, C, xy, mask, n_views = tr.gather(proj, cam_of_image, kp_ptr, kp_xy, track_ptr, obs_image, obs_kp, dtype)
    has = np.asarray(has_point).reshape(-1) != 0
    X = np.asarray(X).reshape(-1, 3).astype(dtype)
    T = len(n_views)
    status = np.zeros(T, np.int32)

    def fail(cond, code):
        status[(status == tr.OK) & cond] = code

    fail(n_views < min_views, tr.TOO_FEW_VIEWS)
    finite = (np.isfinite(P).all(axis=2) & np.isfinite(C).all(axis=2) & np.isfinite(xy).all(axis=2)) | ~mask
    fail(~finite.all(axis=1) | ~np.isfinite(X).all(axis=1), tr.DEGENERATE)
    _, max_err, behind, high, err = tr.evaluate(P, xy, mask, X, max_error)
    fail(behind, tr.BEHIND)
    if min_angle_deg > 0:
        cos_min = dtype.type(np.cos(np.float64(min_angle_deg) * (np.pi / 180.0)))
        fail(~tr.wide_pair(C, mask, X, cos_min), tr.LOW_ANGLE)
    fail(high, tr.HIGH_ERROR)
    dead = (status == tr.TOO_FEW_VIEWS) | (status == tr.DEGENERATE) | ~has
    status[~has] = NO_POINT
    max_err = np.where(dead, dtype.type(np.nan), max_err)
    # back from (track, rank among the used observations) to the observation
    obs_image = np.asarray(obs_image, dtype=np.int64)
    cam_of_image = np.asarray(cam_of_image, dtype=np.int64)
    n_img, n_cams = len(cam_of_image), len(np.asarray(proj).reshape(-1, 12))
    img_ok = (obs_image >= 0) & (obs_image < n_img)
    cam = cam_of_image[np.where(img_ok, obs_image, 0)] if n_img else np.full(len(obs_image), -1)
    used = img_ok & (cam >= 0) & (cam < n_cams)
    trk = np.repeat(np.arange(T), np.diff(np.asarray(track_ptr, dtype=np.int64)))
    sel = np.flatnonzero(used)
    first = np.concatenate([[0], np.cumsum(n_views)])[:-1]
    pos = np.arange(len(sel)) - first[trk[sel]]
    obs_err = np.full(len(obs_image), np.nan, dtype)
    obs_err[sel] = err[trk[sel], pos]
    obs_err[~has[trk]] = np.nan
    return {"status": status, "n_views": n_views, "max_err": max_err, "obs_err": obs_err,
            "counts": np.bincount(status[has], minlength=6).astype(np.int64)}


def align_similarity(src, dst):
    """Umeyama: (s, R, t, aligned) with aligned = s R src + t the least-squares similarity fit of src [n,3] to dst [n,3]."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    a, b = src - ms, dst - md
    U, S, Vt = np.linalg.svd(b.T @ a / len(src))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ D @ Vt
    s = (S * np.diag(D)).sum() / (a ** 2).sum() * len(src)
    t = md - s * R @ ms
    return s, R, t, (s * (R @ src.T)).T + t
