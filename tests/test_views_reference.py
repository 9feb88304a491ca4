"""`ViewSet` (sfm_amd/_views.py) on hand-made inputs, without a device: three images of 3 x 4, 4 x 7 and 0 x 5, two of them views
in swapped order.  The offsets, the one element more behind every array, the centres of the constructors against -M^-1 p, and
every bad input refused before a device is asked for."""
import numpy as np
import pytest

SHAPES = [(3, 4), (4, 7), (0, 5)]


def cameras(n):
    """(proj [n,12], backproj [n,12], centres [n,3]) of n cameras: [M | p] with M = K R, its [M^-1 | c] and c = -M^-1 p."""
    rng = np.random.default_rng(11)
    proj, backproj, centres = [], [], []
    for _ in range(n):
        R = np.linalg.qr(rng.normal(0, 1, (3, 3)))[0]
        K = np.array([[500.0 + rng.uniform(0, 100), 0.0, 31.5], [0.0, 480.0 + rng.uniform(0, 100), 23.5], [0.0, 0.0, 1.0]])
        M, p = K @ R, K @ rng.normal(0, 3, 3)
        c = -np.linalg.solve(M, p)
        proj.append(np.c_[M, p].reshape(12))
        backproj.append(np.c_[np.linalg.inv(M), c].reshape(12))
        centres.append(c)
    return np.array(proj), np.array(backproj), np.array(centres)


def host_maps(refs, backproj, filtered=True):
    """A `DepthMaps` whose state lives on the host, as `depth_maps` builds it on the device."""
    import torch
    from sfm_amd import depth as dm
    n_out = sum(SHAPES[r][0] * SHAPES[r][1] for r in refs)
    maps = dm.DepthMaps({"refs": list(refs), "imgs": [np.zeros(sh, np.uint8) for sh in SHAPES], "radius": 2, "src_ptr": np.zeros(len(refs) + 1, np.int64),
                         "heights": np.array([sh[0] for sh in SHAPES], np.int32), "widths": np.array([sh[1] for sh in SHAPES], np.int32),
                         "ref_image": np.array(refs, np.int32), "backproj": torch.from_numpy(backproj.copy()),
                         "depth": torch.arange(max(n_out, 1), dtype=torch.float32), "keep": torch.ones(max(n_out, 1), dtype=torch.uint8)})
    if filtered:
        maps.keep = [np.ones(SHAPES[r], np.uint8) for r in refs]
    return maps


@pytest.fixture
def no_device(monkeypatch):
    from sfm_amd import _lib

    def asked(*a, **k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(_lib, "get_handle", asked)


def test_view_set_from_maps_and_from_arrays(no_device):
    from sfm_amd import _lib
    from sfm_amd._views import ViewSet
    proj, backproj, centres = cameras(3)
    rel = lambda got, want: np.abs(got - want).max() / np.abs(want).max()
    images = [np.full(sh + (3,), 10 * (i + 1), np.uint8) for i, sh in enumerate(SHAPES)]

    # from a DepthMaps: views 1 and 0, in that order
    v = ViewSet.from_maps(host_maps([1, 0], backproj[:2]), "colors")
    assert (v.n_images, v.n_ref, v.views, v.shapes) == (3, 2, [1, 0], [(4, 7), (3, 4)]) and v.offsets.tolist() == [0, 28, 40]
    assert v.proj.shape == (2, 12) and rel(v.proj, proj[:2]) < 1e-12 and rel(v.centres, centres[:2]) < 1e-12
    assert np.array_equal(v.centres, backproj[:2].reshape(-1, 3, 4)[:, :, 3])                  # the fourth column, as it is
    assert v.pixels is None and v.maps is not None
    w = v.with_images(images)
    assert w is not v and v.pixels is None and w.channels == 3 and w.pixels.numel() == 40 * 3 + 1
    assert w.pixels[:28 * 3].unique().tolist() == [20] and w.pixels[28 * 3:40 * 3].unique().tolist() == [10] and int(w.pixels[-1]) == 0
    assert ViewSet.from_maps(host_maps([1, 0], backproj[:2]), "colors", [a[..., 0] for a in images]).channels == 1
    full, short = w.args(), w.args(maps_only=True)
    assert len(full) == len(_lib.VIEW_SOURCE) and len(short) == len(_lib.VIEW_MAPS)
    assert full[2:4] == (3, 2) and short[2:4] == (3, 2) and full[-1] == 3 and None not in full and None not in short
    assert len(w.alive()) == 5 and w.alive()[0].shape == (2, 12) and w.alive()[1].shape == (2, 3)
    none = ViewSet.from_maps(host_maps([], backproj[:0]), "colors")
    assert none.n_ref == 0 and none.offsets.tolist() == [0] and none.args()[3] == 0 and none.alive()[0].shape == (1, 12)      # a pointer must exist

    # from arrays: every image a view; one element more behind the maps and the pixels
    depth = [np.zeros(sh, np.float32) for sh in SHAPES]
    a = ViewSet.from_arrays(proj, centres, depth, [np.ones(sh, np.uint8) for sh in SHAPES], 3, images)
    assert (a.n_images, a.n_ref, a.views, a.shapes) == (3, 3, [0, 1, 2], SHAPES) and a.offsets.tolist() == [0, 12, 40, 40]
    assert a.depth.numel() == 41 and a.keep.numel() == 41 and a.pixels.numel() == 40 * 3 + 1 and a.maps is None
    unkept = ViewSet.from_arrays(proj, centres, depth, None, 3)
    assert unkept.keep is None and unkept.args()[8] is None and unkept.args()[9] is None and unkept.args(maps_only=True)[7] is None
    empty = ViewSet.from_arrays(np.zeros((0, 12)), np.zeros((0, 3)), [], None, 3, [])
    assert empty.n_ref == 0 and empty.depth.numel() == 1 and empty.pixels.numel() == 1

    # from a volume integrated from arrays: no centres until they are asked for
    vol = ViewSet.from_arrays(proj, None, depth, None, 3, integration_only=True)
    assert vol.centres is None and len(vol.args(maps_only=True)) == 8
    c = vol.with_centres()
    assert vol.centres is None and rel(c.centres, centres) < 1e-12 and c.with_centres() is c


def test_view_set_refuses_bad_inputs_before_the_device(no_device):
    from sfm_amd._views import ViewSet
    proj, backproj, centres = cameras(3)
    gray = [np.zeros(sh, np.uint8) for sh in SHAPES]
    bgr = [np.zeros(sh + (3,), np.uint8) for sh in SHAPES]
    with pytest.raises(ValueError, match="filter"):
        ViewSet.from_maps(host_maps([1, 0], backproj[:2], filtered=False), "colors")
    v = ViewSet.from_maps(host_maps([1, 0], backproj[:2]), "colors")
    for images, why in ((gray[:2], "one array per image"), (gray + gray[:1], "one array per image"), ([gray[1], gray[0], gray[2]], "shape of its maps"),
                        ([gray[0], bgr[1], gray[2]], "all be"), ([a.astype(np.float32) for a in gray], "uint8"),
                        ([gray[0], np.zeros((4, 7, 4), np.uint8), gray[2]], "all be"), ([gray[0], np.zeros(28, np.uint8), gray[2]], "all be")):
        with pytest.raises(ValueError, match=why):
            v.with_images(images)
        with pytest.raises(ValueError, match=why):
            ViewSet.from_maps(host_maps([1, 0], backproj[:2]), "colors", images)
    v.with_images([gray[0], gray[1], np.zeros((9, 9), np.float32)])        # an image that is no view is not looked at
    depth = [np.zeros(sh, np.float32) for sh in SHAPES]
    good = dict(proj=proj, centres=centres, depth=depth, keep=None, max_views=3, images=gray)
    for bad in (dict(proj=proj[:2]), dict(proj=np.zeros((3, 11))), dict(centres=centres[:2]), dict(centres=None), dict(centres=np.zeros((3, 4))),
                dict(depth=depth[:2]), dict(depth=[depth[0], depth[1], np.zeros(5, np.float32)]), dict(keep=gray[:2]),
                dict(keep=[gray[1], gray[0], gray[2]]), dict(max_views=2), dict(images=gray[:2]), dict(images=[gray[1], gray[0], gray[2]]),
                dict(images=[gray[0], bgr[1], gray[2]]), dict(images=[a.astype(np.int32) for a in gray])):
        with pytest.raises(ValueError):
            ViewSet.from_arrays(**dict(good, **bad))
    with pytest.raises(AssertionError, match="a device was asked for"):       # the upload is the step that asks
        ViewSet.from_arrays(**good).to(0)
