"""The component labelling and the cleaning on the device against tests/mesh_clean_reference.py: every output byte of
`sfm_mesh_components`, `sfm_mesh_clean_mark` / `sfm_mesh_clean_emit` and `sfm_mesh_gather_rows`, every call twice, on hand
cases, block and chunk seams, the long chain, the cut with ties, unsound triangles, and the device's own meshes."""
import ctypes as C

import numpy as np
import pytest

import mesh_clean_reference as cr
import mesh_reference as mr

pytestmark = pytest.mark.gpu


def assert_components(got, want, what=""):
    assert (got.n_components, got.n_unsound) == (want.n_components, want.n_unsound), (what, got.n_components, want.n_components, got.n_unsound)
    for mine, theirs in (("vertex_component", "vertex_component"), ("triangle_component", "triangle_component"), ("root", "root"),
                         ("n_vertices", "n_vertices"), ("n_triangles", "n_triangles")):
        x, y = getattr(got, mine), getattr(want, theirs)
        assert x.dtype == np.int32 and x.shape == y.shape, (what, mine, x.dtype, x.shape, y.shape)
        assert x.tobytes() == y.tobytes(), (what, mine, int((x != y).sum()))


def device_components(tri, n_vertices, what=""):
    """The device's labels, checked against the reference and against a second run."""
    from sfm_amd import mesh_components
    tri = np.asarray(tri, np.int32).reshape(-1, 3)
    got, again = mesh_components(tri, n_vertices), mesh_components(tri, n_vertices)
    want = cr.components(tri, n_vertices)
    assert_components(got, want, what)
    assert_components(again, want, (what, "second run"))
    return got, want


def assert_cleaned(mesh, want, what=""):
    assert (mesh.n_vertices, mesh.n_triangles) == (len(want.vertex_map), len(want.triangle_map)), (what, mesh.n_vertices, mesh.n_triangles)
    for name, ref, dtype in (("vertex_map", want.vertex_map, np.int32), ("triangle_map", want.triangle_map, np.int32), ("triangles", want.triangles, np.int32),
                             ("vertices", want.vertices, np.float64), ("normals", want.normals, np.float32)):
        x = getattr(mesh, name)
        assert x.dtype == dtype and x.shape == ref.shape, (what, name, x.dtype, x.shape, ref.shape)
        assert x.tobytes() == np.ascontiguousarray(ref).tobytes(), (what, name)


def rows_of(n_vertices, seed=0):
    """Vertices and normals whose bytes are all different, with NaN, infinities and signed zeros among them."""
    rng = np.random.default_rng(1000 + seed)
    v = rng.normal(size=(n_vertices, 3))
    n = rng.normal(size=(n_vertices, 3)).astype(np.float32)
    if n_vertices:
        v[::7, 0], v[::11, 1], v[::13, 2] = np.nan, -0.0, np.inf
        n[::5, 1], n[::9, 2] = np.nan, -0.0
    return v, n


def device_clean(tri, n_vertices, what="", **kw):
    """clean_mesh against the reference, twice."""
    from sfm_amd import clean_mesh
    tri = np.asarray(tri, np.int32).reshape(-1, 3)
    v, n = rows_of(n_vertices)
    got, again = clean_mesh(v, tri, n, **kw), clean_mesh(v, tri, n, **kw)
    comps = cr.components(tri, n_vertices)
    want = cr.clean(comps, tri, v, n, kw.get("min_triangles", 1), kw.get("keep_largest"))
    assert_cleaned(got, want, what)
    assert_cleaned(again, want, (what, "second run"))
    assert_components(got.components_before, comps, what)
    assert got.atlas is None and got.vertex_colors is None
    return got, want


# ------------------------------------------------------------------------------------------- small cases
def test_empty_inputs(gpu_ready):
    none, _ = device_components(np.zeros((0, 3), np.int32), 0)
    assert none.n_components == 0 and none.vertex_component.shape == (0,) and none.root.shape == (0,)
    loose, _ = device_components(np.zeros((0, 3), np.int32), 5, "five singletons")
    assert loose.n_components == 5 and loose.n_vertices.tolist() == [1] * 5 and loose.n_triangles.tolist() == [0] * 5 and loose.root.tolist() == [0, 1, 2, 3, 4]
    got, _ = device_clean(np.zeros((0, 3), np.int32), 0)
    assert got.vertices.shape == (0, 3) and got.triangles.shape == (0, 3) and got.vertex_map.shape == (0,)
    got, _ = device_clean(np.zeros((0, 3), np.int32), 5, min_triangles=0)
    assert got.n_vertices == 5 and got.n_triangles == 0
    got, _ = device_clean(np.zeros((0, 3), np.int32), 5)          # a loose vertex has no triangle: min_triangles 1 drops it
    assert got.n_vertices == 0


def test_hand_cases(gpu_ready):
    for name, (nv, tri, sets, nt) in cr.hand_cases().items():
        got, _ = device_components(tri, nv, name)
        assert [set(np.flatnonzero(got.vertex_component == k).tolist()) for k in range(got.n_components)] == sets, name
        assert got.n_triangles.tolist() == nt and got.root.tolist() == [min(s) for s in sets], name
        for kw in (dict(), dict(min_triangles=0), dict(min_triangles=2), dict(keep_largest=1), dict(min_triangles=0, keep_largest=2)):
            device_clean(tri, nv, (name, kw), **kw)


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1024, 1025])
def test_seams_of_the_block(gpu_ready, n):
    """n vertices with a soup of any size, and n triangles over any vertices: below, at and above one block and four."""
    for k, (nv, nt) in enumerate(((n, 700), (600, n), (n, n))):
        tri = cr.random_soup(10 * n + k, nv, nt, spread=7)
        got, want = device_components(tri, nv, (nv, nt))
        assert want.n_components > 20
        device_clean(tri, nv, (nv, nt), min_triangles=3)
        device_clean(tri, nv, (nv, nt), min_triangles=2, keep_largest=want.n_components // 8)


def test_the_second_scan_level(gpu_ready):
    """262,145 vertices - 1,024 blocks plus one - as 87,381 disjoint triangles and two loose vertices."""
    nv = 262145
    tri = np.arange(87381 * 3, dtype=np.int32).reshape(-1, 3)
    got, want = device_components(tri, nv, "262,145")
    assert got.n_components == 87383 and got.root[-3:].tolist() == [262140, 262143, 262144] and got.n_triangles[-3:].tolist() == [1, 0, 0]
    v, n = rows_of(nv)
    from sfm_amd import clean_mesh
    out = clean_mesh(v, tri, n)
    assert_cleaned(out, cr.clean(want, tri, v, n), "262,145")
    assert out.n_vertices == 262143 and out.n_triangles == 87381
    half = clean_mesh(v, tri, n, keep_largest=40000)              # every size equal: the first 40,000 in component order
    assert_cleaned(half, cr.clean(want, tri, v, n, keep_largest=40000), "262,145, tie")
    assert half.n_triangles == 40000 and half.triangle_map[-1] == 39999


def test_the_long_chain(gpu_ready):
    """A strip over 70,001 vertices whose numbers ascend - the chain that a union-find without compression walks end to end -
    then the same strip with its vertex numbers permuted and its triangles shuffled."""
    nv = 70001
    strip = cr.strip(nv)
    got, _ = device_components(strip, nv, "strip")
    assert got.n_components == 1 and got.n_triangles.tolist() == [nv - 2] and not got.vertex_component.any()
    rng = np.random.default_rng(70001)
    perm = rng.permutation(nv).astype(np.int32)
    order = rng.permutation(len(strip))
    mixed = perm[strip][order]
    got, _ = device_components(mixed, nv, "permuted strip")
    assert got.n_components == 1 and got.n_vertices.tolist() == [nv]
    # two strips and a gap: the partition is the same after undoing the permutation
    cut = np.concatenate([strip[:30000], strip[30002:]])
    plain, _ = device_components(cut, nv, "two strips")
    mixed, _ = device_components(perm[cut][rng.permutation(len(cut))], nv, "two strips, permuted")
    assert plain.n_components == 2 and sorted(plain.n_vertices.tolist()) == sorted(mixed.n_vertices.tolist()) == [30002, 39999]
    back = mixed.vertex_component[perm]                           # the component of old vertex v
    assert ((back == back[0]) == (plain.vertex_component == plain.vertex_component[0])).all()


def test_nothing_depends_on_the_order(gpu_ready):
    nv = 5000
    tri = cr.random_soup(77, nv, 9000, spread=40)
    rng = np.random.default_rng(5)
    order = rng.permutation(len(tri))
    turned = np.stack([np.roll(t, k) for t, k in zip(tri[order], rng.integers(0, 3, len(tri)))])
    a, _ = device_components(tri, nv, "soup")
    b, _ = device_components(turned, nv, "soup, shuffled")
    for name in ("vertex_component", "root", "n_vertices", "n_triangles"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert np.array_equal(b.triangle_component, a.triangle_component[order]) and 10 < a.n_components < nv


def test_the_cut(gpu_ready):
    """300 components with sizes from {1, 2, 3} plus one of 50."""
    rng = np.random.default_rng(300)
    sizes = rng.integers(1, 4, 301)
    sizes[137] = 50
    tri, base = [], 0
    for s in sizes:                                               # a fan of s triangles over s + 2 vertices
        tri += [(base, base + i + 1, base + i + 2) for i in range(s)]
        base += s + 2
    tri = np.array(tri, np.int32)[rng.permutation(int(sizes.sum()))]
    got, want = device_components(tri, base, "fans")
    assert got.n_triangles.tolist() == sizes.tolist()
    threes = int((sizes == 3).sum())
    assert threes > 40
    for kw in (dict(keep_largest=1), dict(keep_largest=1 + threes // 2), dict(keep_largest=1 + threes), dict(keep_largest=2 + threes),
               dict(keep_largest=300), dict(keep_largest=301), dict(keep_largest=5000), dict(min_triangles=2, keep_largest=1 + threes + 7),
               dict(min_triangles=3, keep_largest=1000), dict(min_triangles=0, keep_largest=299)):
        mesh, ref = device_clean(tri, base, kw, **kw)
        assert int(ref.keep.sum()) == min(kw["keep_largest"], int((sizes >= kw.get("min_triangles", 1)).sum()))
    one, _ = device_clean(tri, base, keep_largest=1)
    assert one.n_triangles == 50 and one.n_vertices == 52
    empty, _ = device_clean(tri, base, min_triangles=51)
    assert (empty.n_vertices, empty.n_triangles) == (0, 0)
    assert empty.vertices.shape == (0, 3) and empty.normals.shape == (0, 3) and empty.triangles.shape == (0, 3) and empty.vertex_map.shape == (0,) and empty.triangle_map.shape == (0,)


def test_unsound_triangles(gpu_ready):
    from sfm_amd import Mesh, _lib, mesh_components
    import torch
    nv = 900
    tri = cr.random_soup(9, nv, 1500, spread=9)
    bad = np.array([[-1, 0, 1], [0, nv, 1], [0, 1, 0x7FFFFFFF], [-0x80000000, -5, nv + 7], [nv, nv, nv]], np.int32)
    at = [0, 255, 256, 700, 1500]
    mixed = np.insert(tri, at, bad, axis=0)
    got, want = device_components(mixed, nv, "unsound")
    assert got.n_unsound == 5 and (got.triangle_component[np.array(at) + np.arange(5)] == -1).all()
    sound, _ = device_components(tri, nv, "sound")
    assert got.vertex_component.tobytes() == sound.vertex_component.tobytes() and got.n_triangles.tobytes() == sound.n_triangles.tobytes()
    mesh, _ = device_clean(mixed, nv, "unsound", min_triangles=2)
    assert mesh.triangles.min() >= 0 and mesh.triangles.max() == mesh.n_vertices - 1 and not np.isin(np.array(at) + np.arange(5), mesh.triangle_map).any()
    # all of them unsound, and no vertex at all
    only, _ = device_components(bad, nv, "only unsound")
    assert only.n_unsound == 5 and only.n_components == nv
    none, _ = device_components(bad, 0, "no vertex")
    assert none.n_unsound == 5 and none.n_components == 0 and (none.triangle_component == -1).all()
    # the raw call returns normally; Mesh.components() raises
    dev = torch.device("cuda", 0)
    h = _lib.get_handle(0)
    d_tri = torch.from_numpy(mixed).to(dev)
    need = C.c_int64()
    assert h.lib.sfm_mesh_components_workspace_bytes(nv, C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    out = [torch.empty(n, dtype=torch.int32, device=dev) for n in (nv, len(mixed), nv, nv, nv)]
    counts = torch.empty(3, dtype=torch.int64, device=dev)
    dp = lambda t: C.c_void_p(t.data_ptr())
    assert h.lib.sfm_mesh_components(h._h, nv, len(mixed), dp(d_tri), *[dp(t) for t in out], dp(counts), dp(ws), need.value) == 0
    assert counts.cpu().numpy().tolist() == [want.n_components, 5, 0]
    v, n = rows_of(nv)
    held = Mesh({"vertices": torch.from_numpy(v).to(dev), "normals": torch.from_numpy(n).to(dev), "triangles": d_tri}, nv, len(mixed))
    with pytest.raises(ValueError, match="5 triangles"):
        held.components()
    with pytest.raises(ValueError, match="5 triangles"):
        held.clean()
    cleaned = held.clean(min_triangles=2, components=mesh_components(mixed, nv))
    assert cleaned.triangles.tobytes() == mesh.triangles.tobytes() and cleaned.vertex_map.tobytes() == mesh.vertex_map.tobytes()


def test_entry_points_reject_bad_arguments(gpu_ready):
    """SFM_ERR_ARG (-1) before any device work: the data pointers are 1 or null throughout, so a call that got as far as a
    launch would not return -1 but fault."""
    from sfm_amd import _lib
    h = _lib.get_handle(0)
    lib = h.lib
    p, big, room = C.c_void_p(1), 1 << 31, 1 << 30
    why = lambda: lib.sfm_last_error(h._h)

    def components(nv=5, nt=2, tri=p, vc=p, tc=p, root=p, cv=p, ct=p, counts=p, ws=p, ws_bytes=room):
        return lib.sfm_mesh_components(h._h, nv, nt, tri, vc, tc, root, cv, ct, counts, ws, ws_bytes)

    def mark(nv=5, nt=2, nc=3, vc=p, tc=p, ct=p, min_triangles=1, keep_largest=0, keep=p, counts=p, ws=p, ws_bytes=room):
        return lib.sfm_mesh_clean_mark(h._h, nv, nt, nc, vc, tc, ct, min_triangles, keep_largest, keep, counts, ws, ws_bytes)

    def emit(nv=5, nt=2, nc=3, vc=p, tc=p, keep=p, tri=p, v=p, n=p, cap_v=5, cap_t=2, vmap=p, tmap=p, tri_out=p, v_out=p, n_out=p, ws=p, ws_bytes=room):
        return lib.sfm_mesh_clean_emit(h._h, nv, nt, nc, vc, tc, keep, tri, v, n, cap_v, cap_t, vmap, tmap, tri_out, v_out, n_out, ws, ws_bytes)

    def gather(src=p, row_bytes=4, map_=p, n=3, dst=p):
        return lib.sfm_mesh_gather_rows(h._h, src, row_bytes, map_, n, dst)

    for call, cases in ((components, [dict(nv=-1), dict(nt=-1), dict(nv=big), dict(nt=big), dict(tri=None), dict(vc=None), dict(tc=None), dict(root=None),
                                      dict(cv=None), dict(ct=None), dict(counts=None), dict(ws=None), dict(ws_bytes=64)]),
                        (mark, [dict(nv=-1), dict(nt=big), dict(nc=-1), dict(nc=6), dict(min_triangles=-1), dict(keep_largest=-1), dict(vc=None), dict(tc=None),
                                dict(ct=None), dict(keep=None), dict(counts=None), dict(ws=None), dict(ws_bytes=64)]),
                        (emit, [dict(nv=big), dict(nt=-1), dict(nc=6), dict(cap_v=-1), dict(cap_t=-1), dict(cap_v=big), dict(cap_t=big), dict(vc=None),
                                dict(tc=None), dict(keep=None), dict(tri=None), dict(v=None), dict(n=None), dict(vmap=None), dict(tmap=None),
                                dict(tri_out=None), dict(v_out=None), dict(n_out=None), dict(ws=None), dict(ws_bytes=64)]),
                        (gather, [dict(row_bytes=0), dict(row_bytes=-4), dict(n=-1), dict(n=big), dict(src=None), dict(map_=None), dict(dst=None)])):
        for kw in cases:
            assert call(**kw) == -1, (call.__name__, kw)
            null = any(v is None for k, v in kw.items() if k != "ws")
            assert why().endswith(b": null pointer") == null, (call.__name__, kw, why())
    # nothing to emit: returns at once, whatever the pointers; nothing to gather likewise
    assert emit(cap_v=0, cap_t=0, v=None, n=None, vmap=None, tmap=None, tri_out=None, v_out=None, n_out=None) == 0
    assert gather(n=0, src=None, map_=None, dst=None) == 0


# ------------------------------------------------------------------------------------------- the rows
@pytest.mark.parametrize("row_bytes", [1, 3, 4, 12, 24])
def test_gather_rows(gpu_ready, row_bytes):
    import torch
    from sfm_amd import _lib
    from sfm_amd.mesh_clean import _gather
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(row_bytes)
    src = {1: rng.integers(0, 256, 3001).astype(np.uint8), 3: rng.integers(0, 256, (3001, 3)).astype(np.uint8),
           4: rng.integers(-9, 9, 3001).astype(np.int32), 12: rng.normal(size=(3001, 3)).astype(np.float32), 24: rng.normal(size=(3001, 3))}[row_bytes]
    assert src[0].nbytes == row_bytes
    d_src = torch.from_numpy(src).to(dev)
    for n in (0, 1, 255, 256, 1025, 7000):
        rows = rng.integers(0, 3001, n).astype(np.int32)
        d_map = torch.from_numpy(np.r_[rows, np.int32(0)]).to(dev)
        got = _gather(dev, d_src, row_bytes, d_map, n).cpu().numpy()[:n]
        assert got.dtype == src.dtype and got.tobytes() == src[rows].tobytes(), (row_bytes, n)
    # a source and a destination that are not aligned to the unit: the bytes all the same
    h = _lib.get_handle(0)
    raw = torch.from_numpy(np.r_[np.zeros(1, np.uint8), src.view(np.uint8).reshape(-1)]).to(dev)
    rows = rng.integers(0, 3001, 500).astype(np.int32)
    d_map = torch.from_numpy(rows).to(dev)
    out = torch.zeros(500 * row_bytes + 2, dtype=torch.uint8, device=dev)
    h.call("sfm_mesh_gather_rows", C.c_void_p(raw.data_ptr() + 1), row_bytes, C.c_void_p(d_map.data_ptr()), 500, C.c_void_p(out.data_ptr() + 1))
    got = out.cpu().numpy()
    assert got[0] == 0 and got[-1] == 0 and got[1:-1].tobytes() == src[rows].tobytes()


# ------------------------------------------------------------------------------------------- the device's own meshes
def test_sphere_is_one_component_and_comes_back_byte_for_byte(gpu_ready):
    from sfm_amd import MeshComponents, tsdf_volume_from_arrays
    from test_mesh_reference import sphere_volume
    (origin, voxel, shape), (tsdf, weight) = sphere_volume()
    nx, ny, nz = shape
    mesh = tsdf_volume_from_arrays(tsdf.reshape(nz, ny, nx), weight.reshape(nz, ny, nx), origin, voxel).mesh()
    comps = mesh.components()
    assert isinstance(comps, MeshComponents) and comps.n_components == 1 and comps.n_unsound == 0
    assert comps.n_triangles.tolist() == [mesh.n_triangles] and comps.n_vertices.tolist() == [mesh.n_vertices] and comps.largest(3) == [0]
    assert_components(comps, cr.components(mesh.triangles, mesh.n_vertices), "sphere")
    before = (mesh.vertices.tobytes(), mesh.normals.tobytes(), mesh.triangles.tobytes())
    out = mesh.clean()
    assert out is not mesh and (out.vertices.tobytes(), out.normals.tobytes(), out.triangles.tobytes()) == before
    assert (mesh.vertices.tobytes(), mesh.normals.tobytes(), mesh.triangles.tobytes()) == before and mesh.vertex_map is None
    assert np.array_equal(out.vertex_map, np.arange(mesh.n_vertices)) and np.array_equal(out.triangle_map, np.arange(mesh.n_triangles))
    assert out.components_before.n_components == 1 and out._volume is mesh._volume
    same = mesh.clean(min_triangles=100, keep_largest=1, components=comps)
    assert same.components_before is comps and same.triangles.tobytes() == before[2]


def test_two_spheres_keep_the_larger_one(gpu_ready):
    from sfm_amd import tsdf_volume_from_arrays
    f, shape = cr.two_sphere_field()
    nx, ny, nz = shape
    mesh = tsdf_volume_from_arrays(f.reshape(nz, ny, nx), np.ones((nz, ny, nx), np.uint16), (0.0, 0.0, 0.0), 1.0).mesh()
    comps = mesh.components()
    want = cr.components(mesh.triangles, mesh.n_vertices)
    assert_components(comps, want, "two spheres")
    assert comps.n_components == 2 and comps.largest(1) == [0] and comps.largest(2) == [0, 1]
    out = mesh.clean(keep_largest=1)
    assert_cleaned(out, cr.clean(want, mesh.triangles, mesh.vertices, mesh.normals, keep_largest=1), "two spheres")
    assert mr.is_closed_and_oriented(out.triangles) and mr.euler_characteristic(out.n_vertices, out.triangles) == 2
    small = mesh.clean(min_triangles=int(comps.n_triangles[1]) + 1)
    assert small.triangles.tobytes() == out.triangles.tobytes() and mesh.clean(min_triangles=int(comps.n_triangles[1])).n_triangles == mesh.n_triangles


def test_default_scene_cleaned_coloured_textured_rendered_and_scored(gpu_ready):
    """depth_maps -> filter -> tsdf -> mesh on the default scene (96 x 72, 3 cameras, resolution 64): the components of the
    README's first row, the mesh without its 10-triangle piece, and every later stage on the result."""
    from test_mesh_texture_gpu import default_scene_maps
    s, maps = default_scene_maps()
    mesh = maps.tsdf(resolution=64).mesh()
    images = list(s.images)
    comps = mesh.components()
    want = cr.components(mesh.triangles, mesh.n_vertices)
    assert_components(comps, want, "default scene")
    assert (mesh.n_vertices, mesh.n_triangles) == (11573, 22112)
    assert sorted(comps.n_triangles.tolist(), reverse=True) == [19296, 2806, 10] and [int(comps.n_triangles[c]) for c in comps.largest(3)] == [19296, 2806, 10]
    colors = mesh.colors(images)
    out = mesh.clean(min_triangles=100, components=comps)
    ref = cr.clean(want, mesh.triangles, mesh.vertices, mesh.normals, min_triangles=100)
    assert_cleaned(out, ref, "default scene")
    assert out.n_triangles == 22102 and out.components().n_components == 2 and out.components_before is comps
    # the per-vertex arrays came along
    assert out.vertex_colors.tobytes() == colors[out.vertex_map].tobytes() and out.n_views.tobytes() == mesh.n_views[out.vertex_map].tobytes()
    assert out.best_view.tobytes() == mesh.best_view[out.vertex_map].tobytes() and out.best_view.dtype == np.int32
    # the stages behind it keep their defaults: the colours of the cleaned mesh are those of its vertices in the old one
    assert out.atlas is None and mesh.clean(min_triangles=100).vertex_colors.tobytes() == out.vertex_colors.tobytes()
    assert out.colors(images).tobytes() == colors[out.vertex_map].tobytes()
    atlas = out.texture(images, texels=2)
    assert atlas is out.atlas and atlas.n_triangles == 22102
    render = out.render_views()
    assert render.sizes == [(96, 72)] * 3 and max(int(t.max()) for t in render.triangle) < 22102
    score = out.score(images)
    assert score.pooled()["n_compared"] > 1000 and 0.0 < score.pooled()["ssim"] <= 1.0
    bgr = [np.stack([a, 255 - a, a // 2 + 17], axis=-1) for a in s.images]
    mesh.colors(bgr)
    assert mesh.clean(keep_largest=1).vertex_colors.shape == (int(comps.n_vertices[comps.largest(1)[0]]), 3)


def test_dense_from_reconstruction_cleans_the_mesh(gpu_ready):
    """min_triangles / keep_largest of `dense_from_reconstruction`: with both None the mesh is the one of before."""
    from sfm_amd import Reconstruction, Tracks, dense_from_reconstruction
    import depth_reference as dr
    s = dr.default_scene()
    ys, xs = np.mgrid[4:72:8, 4:96:8]
    ys, xs = ys.ravel(), xs.ravel()
    z = s.depth[1][ys, xs]
    X = np.stack([(xs - s.K[0, 2]) / s.K[0, 0] * z, (ys - s.K[1, 2]) / s.K[1, 1] * z, z], axis=1)
    n = len(X)
    kp = []
    for i in range(3):
        q = (X + s.poses[i][1]) @ s.K.T
        kp.append(q[:, :2] / q[:, 2:])
    tracks = Tracks(np.arange(4) * n, np.arange(n + 1) * 3, np.tile(np.arange(3), n), np.repeat(np.arange(n), 3))
    rec = Reconstruction(tracks, np.concatenate(kp), s.K)
    rec.poses, rec.order, rec.unregistered = dict(s.poses), [1, 0, 2], []
    rec.X, rec.has_point = X, np.ones(n, bool)
    kw = dict(rel_tol=0.02, max_cost=12.0, min_consistent=1, mesh=True)
    plain = dense_from_reconstruction(rec, s.images, **kw)[-1]
    assert plain.components_before is None and plain.vertex_map is None
    comps = plain.components()
    largest = dense_from_reconstruction(rec, s.images, keep_largest=1, colors=list(s.images), **kw)[-1]
    want = plain.clean(keep_largest=1)
    assert largest.triangles.tobytes() == want.triangles.tobytes() and largest.vertices.tobytes() == want.vertices.tobytes()
    assert largest.n_triangles == int(comps.n_triangles.max()) and largest.vertex_colors.shape == (largest.n_vertices,)
    assert largest.components_before.n_components == comps.n_components
