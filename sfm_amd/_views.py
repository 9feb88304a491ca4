"""The views of a reconstruction as `sfm_tsdf_integrate`, `sfm_mesh_colors`, `sfm_mesh_texture` and `sfm_mesh_exposure_sample`
take them: the one place that spells `heights, widths, n_img, n_ref, ref_image, proj, [centres,] depth, keep[, pixels,
channels]` (include/sfm_amd.h; `_lib.VIEW_MAPS` and `_lib.VIEW_SOURCE` name the types).  A `ViewSet` is checked on the host
before a device is asked for; `Mesh`, `TsdfVolume` (sfm_amd/mesh.py) and the exposure calls (sfm_amd/exposure.py) hand one to
their device calls.
"""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np

from ._lib import dp, hp


def projections_from_backprojections(backproj):
    """[n,12] [P | p] = [K R | K t] from the [M | c] = [R^T K^-1 | -R^T t] that `view_backprojection` makes: P = M^-1, p = -P c."""
    B = np.asarray(backproj, dtype=np.float64).reshape(-1, 3, 4)
    out = np.zeros((len(B), 12))
    for v, b in enumerate(B):
        P = np.linalg.inv(b[:, :3])
        out[v] = np.c_[P, -P @ b[:, 3]].reshape(12)
    return out


def centres_from_projections(proj):
    """float64 [n,3]: the camera centres C = -M^-1 p of row-major [M | p] = [K R | K t]."""
    P = np.asarray(proj, dtype=np.float64).reshape(-1, 3, 4)
    return np.array([-np.linalg.solve(p[:, :3], p[:, 3]) for p in P]).reshape(-1, 3)


def check_color_images(images, shapes):
    """(the views' pixels back to back as uint8 [n_out * channels + 1], channels) from one uint8 [h,w] or [h,w,3] array per
    VIEW, shaped like shapes; ValueError says what is wrong."""
    arrays = [np.asarray(a) for a in images]
    if len(arrays) != len(shapes):
        raise ValueError("images: one array per view")
    tails = {a.shape[2:] for a in arrays if a.ndim in (2, 3)}
    if any(a.ndim not in (2, 3) for a in arrays) or len(tails) > 1 or (tails and next(iter(tails)) not in ((), (3,))):
        raise ValueError("images must all be [h,w] or all be [h,w,3]")
    if any(a.dtype != np.uint8 for a in arrays):
        raise ValueError("images must be uint8")
    for v, (a, sh) in enumerate(zip(arrays, shapes)):
        if a.shape[:2] != tuple(sh):
            raise ValueError(f"view {v}: the image must have the shape of its maps, {tuple(sh)}")
    channels = 3 if tails and next(iter(tails)) == (3,) else 1
    flat = np.concatenate([a.reshape(-1) for a in arrays] + [np.zeros(1, np.uint8)])          # one element more: a pointer must exist
    return np.ascontiguousarray(flat), channels


def _flat_images(images, n_images, views, shapes, of_a_set):
    """`check_color_images` of the views' images out of one array per IMAGE."""
    if len(images) != n_images:
        raise ValueError("images: one array per image of the set" if of_a_set else "images: one array per view")
    return check_color_images([images[r] for r in views], shapes)


def workspace(h, dev, query, *sizes):
    """(uint8 tensor, its bytes): what the library's `query`(*sizes, &bytes) asks for, on dev."""
    import torch
    need = C.c_int64()
    h.check(getattr(h.lib, query)(*sizes, C.byref(need)), query)
    return torch.empty(need.value, dtype=torch.uint8, device=dev), need.value


class ViewSet:
    """heights / widths int32 per IMAGE and ref_image int32 per view on the host; proj float64 [n,12] (row-major [K R | K t])
    and centres float64 [n,3] (None where only the integration is meant) on the host; depth float32 and keep uint8 (or None:
    every finite depth counts), the maps of the views back to back on the device; after `with_images` pixels uint8 on the
    device, `channels` bytes per pixel.  maps: the `DepthMaps` behind the set, or None."""

    def __init__(self, heights, widths, ref_image, proj, centres, depth, keep, maps=None):
        self.heights, self.widths, self.ref_image = heights, widths, ref_image
        self.proj, self.centres, self.depth, self.keep, self.maps = proj, centres, depth, keep, maps
        self.pixels, self.channels = None, 1
        self._tables = {}                                          # proj and centres on the device, made when first asked for

    n_ref = property(lambda self: len(self.ref_image))
    n_images = property(lambda self: len(self.heights))
    views = property(lambda self: [int(r) for r in self.ref_image])
    shapes = property(lambda self: [(int(self.heights[r]), int(self.widths[r])) for r in self.ref_image])
    offsets = property(lambda self: np.concatenate([[0], np.cumsum([h * w for h, w in self.shapes], dtype=np.int64)]))

    @classmethod
    def from_arrays(cls, proj, centres, depth, keep, max_views, images=None, integration_only=False):
        """From arrays made elsewhere, one view per image, checked and still on the host (`to` uploads them): proj [n,12],
        centres [n,3] (None with integration_only), depth one float32 [h,w] per view, keep one uint8 [h,w] per view or None, images None or one
        uint8 [h,w] or [h,w,3] array per view.  Every array gets one element more: a pointer must exist."""
        import torch
        depth = [np.ascontiguousarray(d, dtype=np.float32) for d in depth]
        n = len(depth)
        if n > max_views:
            raise ValueError(f"at most {max_views} views")
        if any(d.ndim != 2 for d in depth) or np.shape(proj) != (n, 12) or (not integration_only and np.shape(centres) != (n, 3)):
            raise ValueError("depth: one [h,w] map per view; proj: 12 numbers and centres: 3 numbers for each")
        if keep is not None and [np.shape(k) for k in keep] != [d.shape for d in depth]:
            raise ValueError("keep must be None or one [h,w] array per view, shaped like its depth map")
        flat = lambda arrays, dtype: torch.from_numpy(np.concatenate([np.asarray(a, dtype=dtype).reshape(-1) for a in arrays] + [np.zeros(1, dtype)]))
        table = lambda a, k: np.ascontiguousarray(a, dtype=np.float64).reshape(-1, k)
        out = cls(np.array([d.shape[0] for d in depth], dtype=np.int32), np.array([d.shape[1] for d in depth], dtype=np.int32),
                  np.arange(n, dtype=np.int32), table(proj, 12), None if integration_only else table(centres, 3), flat(depth, np.float32),
                  None if keep is None else flat(keep, np.uint8))
        return out if images is None else out.with_images(images)

    def to(self, device):
        """The set with its maps and pixels on the device; asks for the device's handle first, which raises without a GPU."""
        import torch
        from . import _lib
        _lib.get_handle(device)
        dev = torch.device("cuda", device)
        out = copy.copy(self)
        out.depth, out.keep, out.pixels = (None if t is None else t.to(dev) for t in (self.depth, self.keep, self.pixels))
        out._tables = {}
        return out

    @classmethod
    def from_maps(cls, maps, what, images=None):
        """From a filtered `DepthMaps`: the projections through `projections_from_backprojections`, the centres the fourth
        column of the back-projections.  what: the caller's name for the ValueError; images: None or what `with_images`
        takes, checked before anything of the maps is read back from the device."""
        if getattr(maps, "keep", None) is None:
            raise ValueError(f"{what}() needs filter() first")
        s = maps._s
        flat = None if images is None else _flat_images(images, len(s["imgs"]), maps.views, maps.shapes, True)
        backproj = s["backproj"].cpu().numpy()[:len(maps.views)].reshape(-1, 3, 4)
        out = cls(s["heights"], s["widths"], s["ref_image"], projections_from_backprojections(backproj),
                  np.ascontiguousarray(backproj[:, :, 3]), s["depth"], s["keep"], maps)
        return out if flat is None else out._with_pixels(*flat)

    def with_centres(self):
        """The set of a volume integrated from arrays, which has none: with the centres through `centres_from_projections`."""
        if self.centres is not None:
            return self
        out = copy.copy(self)
        out.centres, out._tables = centres_from_projections(self.proj), dict(self._tables)
        return out

    def with_images(self, images):
        """A set with the views' pixels on the device (`check_color_images`, then the upload).  images: one uint8 [h,w] or
        [h,w,3] array per IMAGE, all with the same channel count, each view's shaped like its maps."""
        return self._with_pixels(*_flat_images(images, self.n_images, self.views, self.shapes, self.maps is not None))

    def _with_pixels(self, flat, channels):
        import torch
        out = copy.copy(self)
        out.pixels, out.channels = torch.from_numpy(flat).to(self.depth.device), channels
        return out

    def _table(self, name, k):
        if name not in self._tables:
            import torch
            dev = self.depth.device
            self._tables[name] = (torch.from_numpy(np.ascontiguousarray(getattr(self, name), dtype=np.float64).reshape(-1, k)).to(dev) if self.n_ref
                                  else torch.zeros((1, k), dtype=torch.float64, device=dev))      # a pointer must exist
        return self._tables[name]

    def args(self, maps_only=False):
        """The arguments the per-view calls share after the handle: `_lib.VIEW_SOURCE`, or with maps_only `_lib.VIEW_MAPS`."""
        head = (hp(self.heights), hp(self.widths), self.n_images, self.n_ref, hp(self.ref_image), dp(self._table("proj", 12)))
        if maps_only:
            return head + (dp(self.depth), dp(self.keep))
        return head + (dp(self._table("centres", 3)), dp(self.depth), dp(self.keep), dp(self.pixels), int(self.channels))

    def alive(self):
        """The device tensors a call reads through `args()`: to be kept while it may still run."""
        return tuple(self._tables.values()) + (self.depth, self.keep, self.pixels)
