"""The exposure compensation on the device against tests/mesh_exposure_reference.py: every byte of `sfm_mesh_exposure_gram`'s
two tables on hand-made inputs around the tile, the step and the chunk; every byte of `sfm_mesh_exposure_sample` on the hand
cases and the random scenes of the colour tests; every byte of `sfm_images_gain` at every alignment of its vector path; then
the chain on the gained sphere from the device's own mesh to the colours of the corrected images."""
import ctypes as C

import numpy as np
import pytest

import mesh_color_reference as cr
import mesh_exposure_reference as er
import view_calls as vc
from test_mesh_exposure_reference import MEASURED, assert_same, assert_worth, scene_args

pytestmark = pytest.mark.gpu

HAND_SIZES = [(7, 5), (1, 1), (16, 9), (0, 4)]                    # (h, w): three views with pixels and one of height 0


def plan(n_ref=1, channels=1, n_vertices=0):
    from sfm_amd import _lib
    out = (C.c_int32 * 4)()
    assert _lib.load().sfm_mesh_exposure_plan(n_ref, channels, n_vertices, out) == 0
    return list(out)


CHUNK = None


def chunk():
    global CHUNK
    if CHUNK is None:
        CHUNK = plan()[2]
    return CHUNK


# ------------------------------------------------------------------------------------------- the tables alone
def device_gram(seen, samples):
    """sfm_mesh_exposure_gram on host arrays; the outputs hold garbage before the call."""
    import torch
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    n_ref, ch, nv = samples.shape
    up = lambda a: torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1), np.zeros(1, a.dtype)])).to(dev)
    d_seen, d_q = up(seen), up(samples)
    overlap = torch.full((n_ref * n_ref + 1,), -0x0123456789ABCDEF, dtype=torch.int64, device=dev)
    sums = torch.full((n_ref * n_ref * ch + 1,), 0x7EDCBA9876543210, dtype=torch.int64, device=dev)
    need = C.c_int64()
    h.check(h.lib.sfm_mesh_exposure_workspace_bytes(n_ref, ch, nv, C.byref(need)), "sfm_mesh_exposure_workspace_bytes")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    dp = lambda t: C.c_void_p(t.data_ptr())
    h.call("sfm_mesh_exposure_gram", n_ref, ch, nv, dp(d_seen), dp(d_q), dp(overlap), dp(sums), dp(ws), need.value)
    o, s = overlap.cpu().numpy(), sums.cpu().numpy()
    assert o[-1] == -0x0123456789ABCDEF and s[-1] == 0x7EDCBA9876543210            # nothing behind the tables
    return o[:-1].reshape(n_ref, n_ref), s[:-1].reshape(n_ref, n_ref, ch)


def gram_patterns(rng, n_ref, ch, nv):
    """(name, seen, samples): all zeros and all 255 with everything seen (the largest partial sums either way of the offset),
    127 / 128 on either side of it, and random flags - any value that is not 0 is a flag - with samples left standing where
    the view does not see the vertex, which must not count."""
    ones = np.ones((n_ref, nv), np.uint8)
    yield "zeros", ones, np.zeros((n_ref, ch, nv), np.uint8)
    yield "all 255", ones, np.full((n_ref, ch, nv), 255, np.uint8)
    yield "127 / 128", (rng.random((n_ref, nv)) < 0.7).astype(np.uint8), rng.integers(127, 129, (n_ref, ch, nv), dtype=np.uint8)
    flags = rng.integers(0, 256, (n_ref, nv), dtype=np.uint8) * (rng.random((n_ref, nv)) < 0.5)
    yield "random", flags.astype(np.uint8), rng.integers(0, 256, (n_ref, ch, nv), dtype=np.uint8)


def vertex_counts():
    c = chunk()
    return [0, 1, 31, 32, 33, 63, 64, 65, c - 1, c, c + 1, 2 * c + 5]


@pytest.mark.parametrize("which", range(12))
def test_gram_vertex_counts_around_the_step_and_the_chunk(gpu_ready, which):
    """n_vertices 0, 1, 31 .. 65, chunk - 1, chunk, chunk + 1 and 2 chunk + 5, each with 1, 2, 31, 32, 33 and 65 views, one and
    three channels, four patterns: every byte of both tables, which held garbage before the call."""
    nv = vertex_counts()[which]
    rng = np.random.default_rng(1000 + which)
    for n_ref in (1, 2, 31, 32, 33, 65):
        for ch in (1, 3):
            for name, seen, q in gram_patterns(rng, n_ref, ch, nv):
                want = er.tables(seen, q)
                got = device_gram(seen, q)
                assert_same((seen, q) + got, (seen, q) + want, (nv, n_ref, ch, name))
                if name == "all 255":
                    assert (got[0] == nv).all() and (got[1] == 255 * nv).all()


def test_gram_300_views(gpu_ready):
    rng = np.random.default_rng(300)
    nv = chunk() + 77
    seen = (rng.random((300, nv)) < 0.3).astype(np.uint8)
    q = rng.integers(0, 256, (300, 3, nv), dtype=np.uint8)
    got = device_gram(seen, q)
    assert_same((seen, q) + got, (seen, q) + er.tables(seen, q), "300 views")
    assert plan(300, 3, nv)[3] == 100 * 2 and (got[0] > 0).all()


def test_gram_equals_the_counting_restatement(gpu_ready):
    """A small case against the restatement that counts vertex by vertex."""
    rng = np.random.default_rng(9)
    seen = (rng.random((5, 70)) < 0.5).astype(np.uint8)
    q = rng.integers(0, 256, (5, 3, 70), dtype=np.uint8)
    assert_same((seen, q) + device_gram(seen, q), (seen, q) + er.tables_loops(seen, q), "counting")


# ------------------------------------------------------------------------------------------- the sample
def device_tables(s):
    from sfm_amd import mesh_exposure_tables
    return mesh_exposure_tables(*scene_args(s))


def assert_scene_equal(s, what=""):
    seen, q = er.sample(*scene_args(s), channels=s.channels)
    want = (seen, q) + er.tables(seen, q)
    assert_same(device_tables(s), want, what)
    return want


@pytest.mark.parametrize("n_vertices", [0, 1, 64, 255, 256, 257, 1000])
def test_sample_vertex_counts_around_the_wave_and_the_workgroup(gpu_ready, n_vertices):
    """Random vertices (one in twenty with a NaN coordinate) and normals around three views of 7 x 5, 1 x 1 and 16 x 9 pixels
    and one of height 0; gray and three channels, keep given and NULL: every byte of seen and samples, and the tables."""
    n_seen = 0
    for channels in (1, 3):
        for with_keep in (True, False):
            s = cr.random_scene(100 + n_vertices, n_vertices, HAND_SIZES, channels, with_keep)
            want = assert_scene_equal(s, (n_vertices, channels, with_keep))
            assert want[0].shape == (4, n_vertices) and want[1].shape == (4, channels, n_vertices) and want[0][3].sum() == 0
            n_seen += int(want[0].sum())
    assert n_seen > 0 or n_vertices <= 1


@pytest.mark.parametrize("n_views", [1, 3, 4, 5, 9])
def test_sample_view_counts_around_the_batch(gpu_ready, n_views):
    """65 vertices; the thread takes four views at a time."""
    sizes = [[(7, 5), (9, 16), (12, 20)][v % 3] for v in range(n_views)]
    for channels in (1, 3):
        s = cr.random_scene(200 + n_views, 65, sizes, channels, with_keep=bool(n_views % 2))
        want = assert_scene_equal(s, (n_views, channels))
        assert want[0].sum(axis=0).max() >= min(n_views, 2)


def test_sample_no_view_hand_cases_and_300_views(gpu_ready):
    s = cr.random_scene(7, 65, [], 1)
    got = device_tables(s)
    assert got[0].shape == (0, 65) and got[1].shape == (0, 1, 65) and got[2].shape == (0, 0) and got[3].shape == (0, 0, 1)
    for channels in (1, 3):
        s, col, n_views, best = cr.merged_hand_cases(channels)
        want = assert_scene_equal(s, ("hand cases", channels))
        assert np.array_equal(want[0].sum(axis=0), n_views)
    want = assert_scene_equal(cr.many_views(300, 65), "300 views")
    assert want[0].all() and (want[2] == 65).all()


def test_tables_of_a_view_subset_are_the_sub_block(gpu_ready):
    """Batch independence: views 1, 2, 4, 5 and 7 of nine, computed alone, give the rows and columns of the whole."""
    sizes = [[(7, 5), (9, 16), (12, 20)][v % 3] for v in range(9)]
    s = cr.random_scene(77, 500, sizes, 3)
    seen, q, overlap, sums = device_tables(s)
    pick = [1, 2, 4, 5, 7]
    sub = cr.Scene(s.proj[pick], s.centres[pick], [s.depth[v] for v in pick], [s.keep[v] for v in pick], [s.images[v] for v in pick],
                   s.vertices, s.normals, s.tol, s.min_cos, s.fill, 3)
    got = device_tables(sub)
    assert_same(got, (seen[pick], q[pick], overlap[np.ix_(pick, pick)], sums[np.ix_(pick, pick)]), "subset")
    assert (np.triu(got[2], 1) > 0).sum() >= 5


def test_sample_and_gram_reject_bad_arguments(gpu_ready):
    """SFM_ERR_ARG (-1) before any device work: the data pointers are never followed."""
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    hp, one = vc.hp, vc.ONE
    good = dict(vc.GOOD, ch=3, nv=10, tol=0.1, min_cos=0.35, ws_bytes=1 << 20, workspace=one, V=one, N=one, seen=one, samples=one)
    nan, inf = float("nan"), float("inf")

    def call(a):
        return lib.sfm_mesh_exposure_sample(h._h, hp(a["hs"]), hp(a["ws"]), a["n_img"], a["n_ref"], hp(a["refs"]), a["proj"], a["centres"], a["depth"],
                                            a["keep"], a["pixels"], a["ch"], a["nv"], a["V"], a["N"], a["tol"], a["min_cos"], a["seen"], a["samples"],
                                            a["workspace"], a["ws_bytes"])

    for kw in vc.BAD_VIEWS + [dict(n_ref=1025, n_img=1025), dict(ch=0), dict(ch=2), dict(nv=-1), dict(nv=1 << 31), dict(tol=-0.1), dict(tol=nan), dict(tol=inf),
               dict(min_cos=0.0), dict(min_cos=1.01), dict(min_cos=nan), dict(ws_bytes=8), dict(workspace=None)]:
        assert call(dict(good, **kw)) == -1, kw
    for name in vc.VIEW_POINTERS + ("V", "N", "seen", "samples"):
        assert call(dict(good, **{name: None})) == -1 and lib.sfm_last_error(h._h).endswith(b": null pointer"), name
    none = dict(V=None, N=None, seen=None, samples=None)
    assert call(dict(good, nv=0, **none)) == 0
    assert call(dict(good, nv=0, **vc.NO_VIEW, **none)) == 0 and call(dict(good, nv=0, **vc.NO_PIXEL, **none)) == 0
    gram = lambda n_ref=2, ch=3, nv=10, seen=one, q=one, o=one, s=one, ws=one, b=1 << 20: lib.sfm_mesh_exposure_gram(h._h, n_ref, ch, nv, seen, q, o, s, ws, b)
    for kw in (dict(n_ref=-1), dict(n_ref=1025), dict(ch=2), dict(nv=-1), dict(nv=1 << 31), dict(seen=None), dict(q=None), dict(o=None), dict(s=None),
               dict(ws=None), dict(b=8)):
        assert gram(**kw) == -1, kw
    assert gram(n_ref=0, seen=None, q=None, o=None, s=None) == 0


# ------------------------------------------------------------------------------------------- the gain pass
def raw_gain(images, gains, shift_in=0, shift_out=0, in_place=False):
    """sfm_images_gain with the arrays starting shift_in / shift_out bytes behind a 256-byte boundary; the output holds 0xAB
    before the call and is returned whole, 64 bytes on either side of the images included."""
    import torch
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    dev = torch.device("cuda", 0)
    ch = 3 if images[0].ndim == 3 else 1
    flat = np.concatenate([a.reshape(-1) for a in images])
    room = 64
    d_in = torch.zeros(256 + len(flat) + 16, dtype=torch.uint8, device=dev)
    d_in[shift_in:shift_in + len(flat)] = torch.from_numpy(flat).to(dev)
    d_out = d_in if in_place else torch.full((256 + room + len(flat) + room,), 0xAB, dtype=torch.uint8, device=dev)
    assert d_in.data_ptr() % 256 == 0 and d_out.data_ptr() % 256 == 0
    heights = np.array([a.shape[0] for a in images], dtype=np.int32)
    widths = np.array([a.shape[1] for a in images], dtype=np.int32)
    g = np.ascontiguousarray(gains, dtype=np.float64).reshape(len(images), ch)
    start = shift_in if in_place else room + shift_out
    h.call("sfm_images_gain", C.c_void_p(heights.ctypes.data), C.c_void_p(widths.ctypes.data), len(images), ch, C.c_void_p(g.ctypes.data),
           C.c_void_p(d_in.data_ptr() + shift_in), C.c_void_p(d_out.data_ptr() + start))
    out = d_out.cpu().numpy()
    return out, start, len(flat)


GAINS = [0.0, 1.0, 0.5, 1.5, 2.5 / 3.0, 0.7]                      # 0.5 puts every odd value on .5, 2.5 / 3 the value 3


@pytest.mark.parametrize("channels", [1, 3])
def test_gain_every_alignment(gpu_ready, channels):
    """Images 1, 3, 15, 16, 17 and 33 wide with odd heights back to back, so that the images start at every phase of a
    16-byte window; source and destination shifted alike (the vector path at every alignment), shifted differently (bytes
    only) and one array for both: every byte, and nothing written in front of or behind the images."""
    rng = np.random.default_rng(40 + channels)
    shapes = [(3, 1), (1, 3), (5, 15), (3, 16), (7, 17), (3, 33), (1, 1), (9, 33)]
    images = [rng.integers(0, 256, (h, w) if channels == 1 else (h, w, 3), dtype=np.uint8) for h, w in shapes]
    images[2][...] = np.arange(images[2].size, dtype=np.uint8).reshape(images[2].shape) | 1            # odd values under 0.5
    gains = np.array([[GAINS[(i + k) % len(GAINS)] for k in range(channels)] for i in range(len(images))])
    want = np.concatenate([a.reshape(-1) for a in er.apply_gains(images, gains)])
    assert (want == 255).sum() > 10 and (want == 0).sum() >= 4
    for shift_in, shift_out in [(k, k) for k in range(16)] + [(0, 1), (5, 0), (3, 12), (15, 14)]:
        out, start, n = raw_gain(images, gains, shift_in, shift_out)
        assert np.array_equal(out[start:start + n], want), (shift_in, shift_out, np.flatnonzero(out[start:start + n] != want)[:5])
        assert (out[:start] == 0xAB).all() and (out[start + n:] == 0xAB).all(), (shift_in, shift_out)
    out, start, n = raw_gain(images, gains, 7, in_place=True)
    assert np.array_equal(out[start:start + n], want) and (out[:start] == 0).all() and (out[start + n:] == 0).all()


def test_gain_through_the_package_and_more_images_than_a_batch(gpu_ready):
    from sfm_amd import apply_gains
    rng = np.random.default_rng(50)
    for channels in (1, 3):
        images = [rng.integers(0, 256, (1 + i % 4, 1 + i % 7) if channels == 1 else (1 + i % 4, 1 + i % 7, 3), dtype=np.uint8) for i in range(70)]
        images[33] = images[33][:0]                                # an image without a pixel
        gains = rng.uniform(0, 2, (70, channels))
        gains[5], gains[40] = 0.0, 1.0
        got = apply_gains(images, gains)
        for i, (a, b) in enumerate(zip(got, er.apply_gains(images, gains))):
            assert a.shape == b.shape and a.dtype == np.uint8 and np.array_equal(a, b), (channels, i)
        assert np.array_equal(got[40], images[40]) and (got[5] == 0).all()
    big = [rng.integers(0, 256, (301, 517, 3), dtype=np.uint8)]   # many workgroups
    assert np.array_equal(apply_gains(big, [[0.5, 1.0, 1.5]])[0], er.apply_gains(big, [[0.5, 1.0, 1.5]])[0])
    assert apply_gains([], np.zeros((0, 1))) == []


def test_gain_rejects_bad_arguments(gpu_ready):
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    hp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    one = C.c_void_p(1)
    hs, ws, g = np.array([3, 4], np.int32), np.array([4, 7], np.int32), np.ones(6)
    call = lambda hs=hs, ws=ws, n=2, ch=3, g=g, a=one, b=one: lib.sfm_images_gain(h._h, hp(hs), hp(ws), n, ch, hp(g), a, b)
    bad_gain = lambda v: np.array([1, 1, 1, 1, v, 1], np.float64)
    for kw in (dict(n=-1), dict(ch=2), dict(ch=0), dict(hs=None), dict(ws=None), dict(g=None), dict(a=None), dict(b=None), dict(hs=np.array([3, -1], np.int32)),
               dict(ws=np.array([4, 32769], np.int32)), dict(g=bad_gain(-0.5)), dict(g=bad_gain(float("nan"))), dict(g=bad_gain(float("inf"))),
               dict(g=bad_gain(-1e-300))):
        assert call(**kw) == -1, kw
    assert lib.sfm_last_error(h._h).endswith(b"finite and >= 0")
    assert call(n=0, hs=None, ws=None, g=None, a=None, b=None) == 0
    assert call(hs=np.array([0, 4], np.int32), ws=np.array([4, 0], np.int32), a=None, b=None) == 0       # images without a pixel


# ------------------------------------------------------------------------------------------- the chain
def test_gained_sphere_from_the_device_mesh(gpu_ready):
    """tsdf_volume_from_depth_arrays -> mesh() -> exposure(gained images) -> apply() -> colors(corrected images) on the gained
    sphere scene: the tables are the restatement's on the device's own mesh, the gains are `solve_gains` of those tables,
    the corrected images are the restatement's bytes, and the colours of the corrected images hold the worth assertions of
    tests/test_mesh_exposure_reference.py."""
    from sfm_amd import mesh_vertex_colors, solve_gains
    from sfm_amd.exposure import centres_from_projections
    from sfm_amd.mesh import tsdf_volume_from_depth_arrays
    proj, depth, origin, voxel, shape, trunc, centres, images, gained, g_true = er.gained_sphere_scene()
    mesh = tsdf_volume_from_depth_arrays(proj, depth, None, origin, voxel, shape, trunc).mesh()
    own = centres_from_projections(proj)                           # what exposure() takes where there is no DepthMaps
    assert np.abs(own - centres).max() < 1e-9
    V, N = mesh.vertices, mesh.normals
    rows = {}
    for sigma_g in (0.1, 1.0):
        e = mesh.exposure(gained, sigma_g=sigma_g)
        seen, q = er.sample(V, N, proj, own, depth, None, gained, trunc, 0.35)
        assert_same((e.seen, e.samples, e.overlap, e.sums), (seen, q) + er.tables(seen, q), ("gained sphere", sigma_g))
        assert np.array_equal(e.gains, solve_gains(e.overlap, e.sums, 10.0, sigma_g, 1)) and e.gains.shape == (14, 3)
        assert np.abs(e.gains - er.solve_gains(e.overlap, e.sums, 10.0, sigma_g, 1)).max() < 1e-12
        assert np.array_equal(e.spread(), er.spread(seen, q), equal_nan=True)
        fixed = e.apply(gained)
        for a, b in zip(fixed, er.apply_gains(gained, e.gains)):
            assert a.dtype == np.uint8 and a.shape == (64, 64, 3) and np.array_equal(a, b)
        col, n_views, best = mesh_vertex_colors(V, N, proj, centres, depth, None, fixed, trunc)
        prod = e.gains * g_true[:, None]
        rows[sigma_g] = dict(error=er.scaled_error(col, n_views, V, float(prod.mean())), agreement=(prod.max(axis=0) - prod.min(axis=0)) / prod.mean(axis=0),
                             spread=er.spread_summary(*er.sample(V, N, proj, centres, depth, None, fixed, trunc, 0.35)))
    for name, imgs, s in (("as rendered", images, 1.0), ("with the gains", gained, float(g_true.mean()))):
        col, n_views, best = mesh_vertex_colors(V, N, proj, centres, depth, None, imgs, trunc)
        ex = mesh.exposure(imgs)
        rows[name] = dict(error=er.scaled_error(col, n_views, V, s), spread=er.spread_summary(ex.seen, ex.samples))
    assert mesh.n_vertices > 5000 and len(MEASURED) == 4
    assert_worth(rows, "device chain, ")
