"""NumPy restatement of the fusion of the depth maps (include/sfm_amd.h, "fusion of the depth maps into one cloud with
normals"): steps 1 to 5, vectorised, every floating-point operation in the order the header states it (float64, no FMA).
The device must equal it bit for bit.  The sample rule is the one of tests/depth_reference.py."""
import numpy as np

from depth_reference import sample


def view_normals(depth, xyz, centre, step, jump):
    """Step 1 for one view: float32 [h,w,3] from depth float32 [h,w], xyz float64 [h,w,3] and the view's centre."""
    h, w = depth.shape
    if h == 0 or w == 0:
        return np.zeros((h, w, 3), np.float32)
    d = depth.astype(np.float64)
    X = np.asarray(xyz, dtype=np.float64)
    C = np.asarray(centre, dtype=np.float64)
    ys, xs = np.arange(h), np.arange(w)
    xp, xm = np.clip(xs + step, 0, w - 1), np.clip(xs - step, 0, w - 1)
    yp, ym = np.clip(ys + step, 0, h - 1), np.clip(ys - step, 0, h - 1)
    with np.errstate(all="ignore"):
        a = X[:, xp] - X[:, xm]
        b = X[yp] - X[ym]
        n = np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                      a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                      a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)
        l2 = (n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]
        valid = np.isfinite(d)
        for dn in (d[:, xp], d[:, xm], d[yp], d[ym]):
            valid &= np.isfinite(dn) & (np.abs(dn - d) <= jump * d)
        valid &= np.isfinite(l2) & (l2 > 0)
        n = n / np.sqrt(l2)[..., None]
        c = C - X
        neg = ((n[..., 0] * c[..., 0] + n[..., 1] * c[..., 1]) + n[..., 2] * c[..., 2]) < 0
        n = np.where(neg[..., None], -n, n)
    return np.where(valid[..., None], n, 0.0).astype(np.float32)


def unit(acc):
    """The normalisation of step 4 on [..., 3] float64 sums: float32, zeros where the sum has no length."""
    with np.errstate(all="ignore"):
        l2 = (acc[..., 0] * acc[..., 0] + acc[..., 1] * acc[..., 1]) + acc[..., 2] * acc[..., 2]
        ok = np.isfinite(l2) & (l2 > 0)
        n = acc / np.sqrt(l2)[..., None]
    return np.where(ok[..., None], n, 0.0).astype(np.float32)


class Fused:
    """view_normals, agree_mask, owner: one array per view; pt_ptr int64 [n_ref+1]; points float64 [m,3], normals float32
    [m,3], n_views uint8 [m], index int32 [m,3] as (view position, y, x)."""


def fuse(shapes, refs, sources, warps, backproj, depth, keep, xyz, rel_tol, step, jump):
    """shapes: (h, w) of every IMAGE; refs, sources, warps, backproj as in depth_reference.filter_views; depth (float32
    [h,w]), keep (uint8 [h,w]) and xyz (float64 [h,w,3]) per view."""
    view_of = {ref: v for v, ref in enumerate(refs)}
    out = Fused()
    out.view_normals = [view_normals(depth[v], xyz[v], np.asarray(backproj[v], dtype=np.float64).reshape(3, 4)[:, 3], step, jump)
                        for v in range(len(refs))]
    out.agree_mask, out.owner = [], []
    pts, nrm, cnt, idx, pt_ptr = [], [], [], [], [0]
    for v, ref in enumerate(refs):
        h, w = shapes[ref]
        y, x = np.mgrid[0:h, 0:w]
        d = depth[v].astype(np.float64)
        kept = keep[v] != 0
        mask = np.zeros((h, w), np.uint8)
        own = kept.copy()
        acc = np.array(xyz[v], dtype=np.float64).reshape(h, w, 3)
        nacc = out.view_normals[v].astype(np.float64)
        for e, (s, W) in enumerate(zip(sources[v], np.asarray(warps[v]).reshape(-1, 12))):
            if s not in view_of:
                continue
            hs, ws = shapes[s]
            if hs == 0 or ws == 0 or h == 0 or w == 0:
                continue
            rs = view_of[s]
            valid, xi, yi, q2 = sample(W, x, y, d, ws, hs)
            ds = depth[rs].astype(np.float64)[yi, xi]
            with np.errstate(all="ignore"):
                agree = kept & valid & np.isfinite(ds) & (np.abs(ds - q2) <= rel_tol * q2) & (keep[rs][yi, xi] != 0)
                mask |= (agree.astype(np.uint8) << np.uint8(e))
                if rs < v:
                    own &= ~agree
                acc = np.where(agree[..., None], acc + np.asarray(xyz[rs], dtype=np.float64)[yi, xi], acc)
                nacc = np.where(agree[..., None], nacc + out.view_normals[rs].astype(np.float64)[yi, xi], nacc)
        out.agree_mask.append(mask)
        out.owner.append(own.astype(np.uint8))
        n_views = 1 + np.unpackbits(mask.reshape(h, w, 1), axis=-1).sum(axis=-1).astype(np.int64)
        with np.errstate(all="ignore"):
            mean = acc / n_views.astype(np.float64)[..., None]
        yy, xx = np.nonzero(own)                                  # row-major
        pts.append(mean[yy, xx])
        nrm.append(unit(nacc)[yy, xx])
        cnt.append(n_views[yy, xx].astype(np.uint8))
        idx.append(np.stack([np.full(len(yy), v), yy, xx], axis=1).astype(np.int32))
        pt_ptr.append(pt_ptr[-1] + len(yy))
    out.pt_ptr = np.array(pt_ptr, dtype=np.int64)
    out.points = np.concatenate(pts).reshape(-1, 3) if pts else np.zeros((0, 3))
    out.normals = np.concatenate(nrm).reshape(-1, 3) if nrm else np.zeros((0, 3), np.float32)
    out.n_views = np.concatenate(cnt) if cnt else np.zeros(0, np.uint8)
    out.index = np.concatenate(idx).reshape(-1, 3) if idx else np.zeros((0, 3), np.int32)
    return out
