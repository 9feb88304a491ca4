"""Components and cleaning without a GPU: the two restatements of the labelling (tests/mesh_clean_reference.py) against each
other and on hand cases, the selection and the compaction on meshes whose answer is known - a sphere, two spheres, the four
default-scene rows of the README - the host build of mesh_clean_rule.h and mesh_clean_plan.h plain and under the sanitizers
as a stand-alone program, and the argument checks of the Python layer and of the C entry points."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_clean_reference as cr
import mesh_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "mesh_clean_check.cpp")
SOUPS = [(1, 1, 0), (2, 40, 0), (3, 0, 0), (4, 300, 90), (5, 257, 1025), (6, 2000, 700), (7, 2000, 6000), (8, 50, 400)]


# ------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("seed,n_vertices,n_triangles", SOUPS)
def test_the_two_restatements_agree_on_random_soups(seed, n_vertices, n_triangles):
    tri = cr.random_soup(seed, n_vertices, n_triangles)
    a, b = cr.components(tri, n_vertices), cr.components_loops(tri, n_vertices)
    cr.assert_same_components(a, b, seed)
    assert a.n_unsound == 0 and a.n_vertices.sum() == n_vertices and a.n_triangles.sum() == n_triangles
    assert (np.diff(a.root) > 0).all() and (a.vertex_component[a.root] == np.arange(a.n_components)).all()
    # with unsound triangles mixed in: counted, labelled -1, and the rest as before
    if n_triangles:
        bad = np.array([[-1, 0, 0], [0, n_vertices, 0], [0, 0, 0x7FFFFFFF]], np.int32)
        mixed = np.concatenate([bad[:1], tri, bad[1:]])
        c, d = cr.components(mixed, n_vertices), cr.components_loops(mixed, n_vertices)
        cr.assert_same_components(c, d, seed)
        assert c.n_unsound == 3 and (c.triangle_component[[0, -2, -1]] == -1).all() and np.array_equal(c.triangle_component[1:-2], a.triangle_component)
        assert np.array_equal(c.vertex_component, a.vertex_component) and np.array_equal(c.n_triangles, a.n_triangles)


@pytest.mark.parametrize("fn", [cr.components, cr.components_loops])
def test_hand_cases(fn):
    for name, (nv, tri, sets, nt) in cr.hand_cases().items():
        c = fn(np.array(tri, np.int32), nv)
        assert c.n_components == len(sets) and c.n_unsound == 0, name
        assert [set(np.flatnonzero(c.vertex_component == k).tolist()) for k in range(c.n_components)] == sets, name
        assert c.root.tolist() == [min(s) for s in sets] and c.n_vertices.tolist() == [len(s) for s in sets] and c.n_triangles.tolist() == nt, name
        assert all(c.triangle_component[i] == c.vertex_component[t[0]] for i, t in enumerate(tri)), name
    none = fn(np.zeros((0, 3), np.int32), 0)
    assert none.n_components == 0 and none.vertex_component.shape == (0,) and none.root.shape == (0,)
    loose = fn(np.zeros((0, 3), np.int32), 5)
    assert loose.n_components == 5 and loose.vertex_component.tolist() == [0, 1, 2, 3, 4] and loose.n_vertices.tolist() == [1] * 5 and not loose.n_triangles.any()


def test_nothing_depends_on_the_order():
    nv = 500
    tri = cr.random_soup(21, nv, 900)
    rng = np.random.default_rng(3)
    order = rng.permutation(len(tri))
    turned = np.stack([np.roll(t, k) for t, k in zip(tri[order], rng.integers(0, 3, len(tri)))])
    a, b = cr.components(tri, nv), cr.components(turned, nv)
    assert np.array_equal(a.vertex_component, b.vertex_component) and np.array_equal(a.n_triangles, b.n_triangles) and np.array_equal(a.root, b.root)
    assert np.array_equal(b.triangle_component, a.triangle_component[order])
    # the long chain, ascending and with its vertex numbers permuted
    strip = cr.strip(3001)
    one = cr.components(strip, 3001)
    assert one.n_components == 1 and one.n_triangles.tolist() == [2999]
    perm = rng.permutation(3001).astype(np.int32)
    again = cr.components_loops(perm[strip][rng.permutation(len(strip))], 3001)
    assert again.n_components == 1 and again.n_vertices.tolist() == [3001]


def test_selection_and_compaction():
    sizes = np.array([3, 1, 2, 50, 2, 3, 1, 3, 0], np.int32)
    assert cr.select(sizes).tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 0]
    assert cr.select(sizes, 0).tolist() == [1] * 9 and cr.select(sizes, 51).tolist() == [0] * 9
    assert cr.select(sizes, 1, 1).tolist() == [0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert cr.select(sizes, 1, 3).tolist() == [1, 0, 0, 1, 0, 1, 0, 0, 0]           # inside the tie at 3: the first two of the three
    assert cr.select(sizes, 1, 4).tolist() == [1, 0, 0, 1, 0, 1, 0, 1, 0]
    assert cr.select(sizes, 1, 5).tolist() == [1, 0, 1, 1, 0, 1, 0, 1, 0]
    assert cr.select(sizes, 2, 8).tolist() == [1, 0, 1, 1, 1, 1, 0, 1, 0] and cr.select(sizes, 1, 100).tolist() == cr.select(sizes).tolist()
    # two triangles apart and a loose vertex between them
    tri = np.array([[4, 5, 6], [0, 1, 2], [6, 5, 4]], np.int32)
    v = np.arange(21, dtype=np.float64).reshape(7, 3)
    n = -np.arange(21, dtype=np.float32).reshape(7, 3)
    comps = cr.components(tri, 7)
    assert comps.n_triangles.tolist() == [1, 0, 2]
    out = cr.clean(comps, tri, v, n, min_triangles=2)
    assert out.keep.tolist() == [0, 0, 1] and out.vertex_map.tolist() == [4, 5, 6] and out.triangle_map.tolist() == [0, 2]
    assert out.triangles.tolist() == [[0, 1, 2], [2, 1, 0]] and np.array_equal(out.vertices, v[4:]) and np.array_equal(out.normals, n[4:])
    everything = cr.clean(comps, tri, v, n, min_triangles=0)
    assert np.array_equal(everything.triangles, tri) and np.array_equal(everything.vertices, v) and everything.vertex_map.tolist() == list(range(7))
    nothing = cr.clean(comps, tri, v, n, min_triangles=3)
    assert nothing.triangles.shape == (0, 3) and nothing.vertices.shape == (0, 3) and nothing.vertex_map.shape == (0,) and not nothing.keep.any()
    first = cr.clean(comps, tri, v, n, min_triangles=1, keep_largest=1)
    assert first.keep.tolist() == [0, 0, 1]


# ------------------------------------------------------------------------------------------- meshes whose answer is known
def test_the_sphere_is_one_component_and_cleaning_it_is_the_identity():
    from test_mesh_reference import sphere_volume
    (origin, voxel, shape), (tsdf, weight) = sphere_volume()
    m = mr.mesh(tsdf, weight, origin, voxel, shape, 1)
    comps = cr.components(m.triangles, len(m.vertices))
    assert comps.n_components == 1 and comps.n_triangles.tolist() == [len(m.triangles)] and comps.n_vertices.tolist() == [len(m.vertices)]
    out = cr.clean(comps, m.triangles, m.vertices, m.normals)
    assert out.triangles.tobytes() == m.triangles.tobytes() and out.vertices.tobytes() == m.vertices.tobytes() and out.normals.tobytes() == m.normals.tobytes()
    assert np.array_equal(out.vertex_map, np.arange(len(m.vertices))) and np.array_equal(out.triangle_map, np.arange(len(m.triangles)))


def test_two_spheres_are_two_components_and_the_larger_one_is_closed():
    f, shape = cr.two_sphere_field()
    m = mr.mesh(f, np.ones(len(f), np.uint16), (0.0, 0.0, 0.0), 1.0, shape, 1)
    comps = cr.components(m.triangles, len(m.vertices))
    cr.assert_same_components(comps, cr.components_loops(m.triangles, len(m.vertices)))
    assert comps.n_components == 2 and comps.n_triangles[0] > comps.n_triangles[1] > 500
    out = cr.clean(comps, m.triangles, m.vertices, m.normals, keep_largest=1)
    assert out.keep.tolist() == [1, 0] and len(out.triangles) == comps.n_triangles[0] and len(out.vertices) == comps.n_vertices[0]
    assert mr.is_closed_and_oriented(out.triangles) and mr.euler_characteristic(len(out.vertices), out.triangles) == 2
    assert (out.vertices[:, 0] < 20).all() and np.array_equal(out.vertices, m.vertices[out.vertex_map])
    assert mr.euler_characteristic(len(m.vertices), m.triangles) == 4


# the README's table: (min_consistent, min_weight) -> vertices, triangles, the triangles of the components largest first
DEFAULT_SCENE_ROWS = {(1, 1): (11573, 22112, [19296, 2806, 10]), (1, 2): (11024, 21060, [18998, 1940, 120, 2]),
                      (2, 1): (9521, 17952, [13882, 4038, 22, 6, 4]), (2, 2): (8717, 16402, [13248, 3062, 88, 4])}


@pytest.mark.parametrize("key", sorted(DEFAULT_SCENE_ROWS))
def test_default_scene_rows(key):
    nv, nt, sizes = DEFAULT_SCENE_ROWS[key]
    m = cr.default_scene_mesh(*key)
    comps = cr.components(m.triangles, len(m.vertices))
    assert (len(m.vertices), len(m.triangles), comps.n_components) == (nv, nt, len(sizes))
    assert sorted(comps.n_triangles.tolist(), reverse=True) == sizes
    if key == (1, 1):
        cr.assert_same_components(comps, cr.components_loops(m.triangles, len(m.vertices)))
        out = cr.clean(comps, m.triangles, m.vertices, m.normals, min_triangles=100)
        after = cr.components(out.triangles, len(out.vertices))
        assert len(out.triangles) == 22102 and after.n_components == 2 and int(out.keep.sum()) == 2
        assert sorted(after.n_triangles.tolist()) == [2806, 19296] and out.triangles.max() == len(out.vertices) - 1


# ------------------------------------------------------------------------------------------- the headers on the host
def build_check(tmp_path, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", *flags, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"), CHECK_SRC, "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return str(exe)


def run_check(exe):
    for args, least in ((["cut", "5"], 3000), (["cut", "77"], 3000), (["plan"], 1000)):
        run = subprocess.run([exe, *args], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.startswith("ok "), (args, run.stdout, run.stderr[-2000:])
        assert int(run.stdout.split()[1]) > least


def test_rule_and_plan_on_the_host(tmp_path):
    """The cut against a stable sort on random sizes with many ties, the argument checks branch by branch, the workspace
    layouts and the two-level scan of the packed counts around every block and chunk seam."""
    run_check(build_check(tmp_path, ["-O2"], "mesh_clean_check"))


def test_rule_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone."""
    run_check(build_check(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
                          "mesh_clean_check_san"))


# ------------------------------------------------------------------------------------------- argument checks, no device
def test_argument_checks_without_gpu():
    import sfm_amd
    from sfm_amd import depth as dm
    from sfm_amd import mesh as mm
    from sfm_amd import mesh_clean as mc
    assert sfm_amd.MeshComponents is mc.MeshComponents and sfm_amd.clean_mesh is mc.clean_mesh and sfm_amd.mesh_components is mm.mesh_components
    assert [p.default for p in list(inspect.signature(mm.Mesh.clean).parameters.values())[1:]] == [1, None, None]
    assert [p.default for p in list(inspect.signature(mc.clean_mesh).parameters.values())[2:]] == [None, 1, None, 0]
    assert [p.default for p in list(inspect.signature(mc.mesh_components).parameters.values())[2:]] == [0]
    dense = inspect.signature(dm.dense_from_reconstruction).parameters
    assert dense["min_triangles"].default is None and dense["keep_largest"].default is None and dense["mesh"].default is False
    check = mc.check_clean_arguments
    assert check() == (1, 0, None, None, None, None) and check(0, 7)[:2] == (0, 7) and check(np.int64(3), np.int32(2))[:2] == (3, 2)
    tri = [[0, 1, 2], [2, 1, 3]]
    got = check(1, None, None, tri, np.zeros((4, 3)), np.zeros((4, 3)))
    assert got[2] == 4 and got[3].dtype == np.int32 and got[3].shape == (2, 3) and got[4].dtype == np.float64 and got[5].dtype == np.float32
    assert check(n_vertices=0, triangles=np.zeros((0, 3), np.int64))[3].shape == (0, 3)
    for kw in (dict(min_triangles=-1), dict(min_triangles=1.0), dict(min_triangles=True), dict(min_triangles=None), dict(min_triangles=1 << 31),
               dict(keep_largest=0), dict(keep_largest=-2), dict(keep_largest=2.0), dict(keep_largest=False), dict(keep_largest=1 << 31),
               dict(n_vertices=-1), dict(n_vertices=1 << 31), dict(n_vertices=2.5), dict(triangles=[[0, 1]]), dict(triangles=[0, 1, 2]),
               dict(triangles=[[0.0, 1.0, 2.0]]), dict(triangles=[[0, 1, 1 << 31]]), dict(triangles="abc"), dict(vertices=np.zeros((4, 2))),
               dict(vertices=np.zeros(3)), dict(vertices=np.zeros((4, 3)), n_vertices=5), dict(vertices=np.zeros((4, 3)), normals=np.zeros((3, 3))),
               dict(normals=np.zeros((4, 3)))):
        with pytest.raises(ValueError):
            check(**kw)
    for call in (lambda: mc.clean_mesh(None, tri), lambda: mc.clean_mesh(np.zeros((4, 3)), tri, min_triangles=-1),
                 lambda: mc.clean_mesh(np.zeros((4, 3)), tri, keep_largest=0), lambda: mc.mesh_components(tri, None),
                 lambda: mc.mesh_components(tri, -3), lambda: mc.mesh_components([[0, 1]], 4),
                 lambda: dm.dense_from_reconstruction(None, [], min_triangles=5), lambda: dm.dense_from_reconstruction(None, [], mesh=True, keep_largest=0),
                 lambda: dm.dense_from_reconstruction(None, [], mesh=True, min_triangles=-1)):
        with pytest.raises(ValueError):
            call()

    # a mesh and its components held on the host
    class Held:
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    bare = mm.Mesh({}, 0, 0)
    assert bare.vertex_map is None and bare.triangle_map is None and bare.components_before is None and bare.atlas is None
    for kw in (dict(min_triangles=-1), dict(keep_largest=0), dict(min_triangles="many")):
        with pytest.raises(ValueError):
            bare.clean(**kw)
    want = cr.components(np.array([[0, 4, 2], [3, 3, 1], [1, 3, 3]], np.int32), 6)
    state = {"vertex_component": Held(want.vertex_component), "triangle_component": Held(want.triangle_component), "comp_root": Held(np.r_[want.root, [9, 9, 9]]),
             "comp_vertices": Held(np.r_[want.n_vertices, [9, 9, 9]]), "comp_triangles": Held(np.r_[want.n_triangles, [9, 9, 9]])}
    held = mc.MeshComponents(state, 6, 3, want.n_components, 0)
    assert held.n_components == 3 and held.root.tolist() == [0, 1, 5] and held.n_vertices.tolist() == [3, 2, 1] and held.n_triangles.tolist() == [1, 2, 0]
    assert held.vertex_component.tolist() == [0, 1, 0, 1, 0, 2] and held.triangle_component.tolist() == [0, 1, 1]
    assert held.largest() == [1] and held.largest(2) == [1, 0] and held.largest(9) == [1, 0, 2] and held.largest(0) == []
    with pytest.raises(ValueError):
        held.largest(-1)
    with pytest.raises(ValueError, match="this mesh"):
        mm.Mesh({}, 5, 3).clean(components=held)


def test_c_entry_points_reject_bad_calls_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    need = ctypes.c_int64(-1)
    big = 1 << 31
    assert lib.sfm_mesh_components_workspace_bytes(0, ctypes.byref(need)) == 0 and 0 < need.value <= 4096
    assert lib.sfm_mesh_components_workspace_bytes(100000, ctypes.byref(need)) == 0 and 800000 <= need.value < 900000
    assert lib.sfm_mesh_components_workspace_bytes(big - 1, ctypes.byref(need)) == 0 and need.value > 8 * (big - 1)
    for n in (-1, big):
        assert lib.sfm_mesh_components_workspace_bytes(n, ctypes.byref(need)) == -1
    assert lib.sfm_mesh_components_workspace_bytes(5, None) == -1
    assert lib.sfm_mesh_clean_workspace_bytes(0, 0, ctypes.byref(need)) == 0 and 0 < need.value <= 4096
    assert lib.sfm_mesh_clean_workspace_bytes(100000, 200000, ctypes.byref(need)) == 0 and 400000 <= need.value < 500000
    for nv, nt in ((-1, 0), (0, -1), (big, 0), (0, big)):
        assert lib.sfm_mesh_clean_workspace_bytes(nv, nt, ctypes.byref(need)) == -1
    assert lib.sfm_mesh_clean_workspace_bytes(5, 5, None) == -1
    # a null handle
    one = ctypes.c_void_p(1)
    assert lib.sfm_mesh_components(None, 0, 0, None, None, None, None, None, None, one, one, 4096) == -1
    assert lib.sfm_mesh_clean_mark(None, 0, 0, 0, None, None, None, 1, 0, None, one, one, 4096) == -1
    assert lib.sfm_mesh_clean_emit(None, 0, 0, 0, None, None, None, None, None, None, 0, 0, None, None, None, None, None, one, 4096) == -1
    assert lib.sfm_mesh_gather_rows(None, None, 4, None, 0, None) == -1
