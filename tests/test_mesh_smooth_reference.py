"""Mesh smoothing without a GPU: the two restatements of the adjacency and of the normals (tests/mesh_smooth_reference.py)
against each other on the meshes of the README's table and on the hand cases, the table itself recomputed and asserted to its
printed digits, the properties of the rule that need no device, the host build of mesh_smooth_rule.h and mesh_smooth_plan.h
plain and under the sanitizers as a stand-alone program, its adjacency, states, vertices and normals bit for bit those of the
restatement, and the argument checks of the Python layer and of the C entry points."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_decimate_reference as dr
import mesh_reference as mr
import mesh_smooth_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "mesh_smooth_check.cpp")


def table_mesh(name):
    """(mesh, centre, radius or None, voxel)."""
    if name == "sphere":
        return dr.analytic_sphere(), dr.SPHERE_CENTRE, dr.SPHERE_RADIUS, 1.0
    if name == "torus":
        return dr.torus(), None, None, 1.0
    mesh, voxel = sr.noisy_scene_sphere() if name == "noisy" else dr.scene_sphere()
    return mesh, (0.0, 0.0, 0.0), 1.0, voxel


# (mesh, iterations, mu) -> V, T, rms angle between face normal and radius in degrees (2 decimals), signed volume (4), rms and
# mean radial error in voxels (4).  The rows of `scene` and `noisy` are the README's, and the restatement gives the figures
# of the prototype to every printed digit; the analytic sphere and the torus are the restatement's own.
TABLE = {
    ("scene", 0, -0.53): (7006, 14008, 17.83, 4.2562, 0.1229, 0.0641),
    ("scene", 3, -0.53): (7006, 14008, 13.03, 4.2562, 0.1102, 0.0645),
    ("scene", 10, -0.53): (7006, 14008, 9.60, 4.2586, 0.1024, 0.0670),
    ("scene", 30, -0.53): (7006, 14008, 6.85, 4.2683, 0.1001, 0.0752),
    ("scene", 3, None): (7006, 14008, 7.26, 4.2257, 0.0755, 0.0407),
    ("noisy", 0, -0.53): (7142, 14280, 24.95, 4.2536, 0.1737, None),
    ("noisy", 10, -0.53): (7142, 14280, 14.31, 4.2586, 0.1396, None),
    # an exact distance field: its faces are good already, the first iterations of uniform weights on the irregular
    # connectivity of marching tetrahedra make them worse, and ten bring them back
    ("sphere", 0, -0.53): (1008, 2012, 5.24, 324.0296, 0.0250, -0.0185),
    ("sphere", 1, -0.53): (1008, 2012, 13.68, 324.1689, 0.0239, -0.0193),
    ("sphere", 10, -0.53): (1008, 2012, 4.97, 326.1196, 0.0219, -0.0129),
    ("sphere", 3, None): (1008, 2012, 4.41, 310.2811, 0.0852, -0.0804),
    ("torus", 0, -0.53): (2630, 5260, None, 715.4020, None, None),
    ("torus", 10, -0.53): (2630, 5260, None, 718.1803, None, None),
    ("torus", 3, None): (2630, 5260, None, 691.4505, None, None),
}


def figures(name, iterations, mu):
    m, centre, radius, voxel = table_mesh(name)
    s = sr.smooth(m.vertices, m.triangles, iterations, 0.5, mu)
    volume = round(mr.signed_volume(s.vertices, m.triangles), 4)
    if centre is None:
        return s, (len(m.vertices), len(m.triangles), None, volume, None, None)
    rms, mean = sr.radial_error(s.vertices, m.triangles, centre, radius, voxel)
    return s, (len(m.vertices), len(m.triangles), round(sr.face_angle_rms(s.vertices, m.triangles, centre), 2), volume, round(rms, 4), round(mean, 4))


# ------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("name", ["sphere", "torus", "scene", "noisy"])
def test_the_two_restatements_agree_on_the_table_meshes(name):
    m = table_mesh(name)[0]
    a = sr.adjacency(m.triangles, len(m.vertices))
    sr.assert_same_adjacency(a, sr.adjacency_loops(m.triangles, len(m.vertices)), name)
    assert a.counts[1:] == [0, 0, 0] and (a.vertex_flags == 0).all()             # a closed mesh has no boundary vertex
    assert a.counts[0] == 2 * (len(m.vertices) + len(m.triangles) - (0 if name == "torus" else 2))        # Euler: E = V + F - chi
    assert (np.diff(a.ptr) >= 3).all() and all((np.diff(a.index[a.ptr[v]:a.ptr[v + 1]]) > 0).all() for v in range(0, len(m.vertices), 97))
    moved = sr.smooth(m.vertices, m.triangles, 2).vertices
    n = sr.vertex_normals(moved, m.triangles)
    assert np.array_equal(sr.bits(n), sr.bits(sr.vertex_normals_loops(moved, m.triangles))), name
    assert n.dtype == np.float32 and (np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1) < 1e-6).all()


def test_the_two_restatements_agree_on_the_hand_cases():
    got = {}
    for name, v, t, pinned in sr.hand_cases():
        a = sr.adjacency(t, len(v))
        sr.assert_same_adjacency(a, sr.adjacency_loops(t, len(v)), name)
        with np.errstate(all="ignore"):
            assert np.array_equal(sr.bits(sr.vertex_normals(v, t)), sr.bits(sr.vertex_normals_loops(v, t))), name
        got[name] = (a, sr.smooth(v, t, 2, pinned=pinned, adj=a))
    a, s = got["one triangle"]
    assert a.ptr.tolist() == [0, 2, 4, 6] and a.index.tolist() == [1, 2, 0, 2, 0, 1] and a.vertex_flags.tolist() == [1, 1, 1] and s.counts == [3, 0, 0, 0]
    assert s.vertices.tobytes() == sr.hand_cases()[0][1].tobytes()                # everything pinned, nothing moves
    a, s = got["a tetrahedron"]
    assert a.counts == [12, 0, 0, 0] and s.counts == [0, 0, 0, 0] and (s.vertex_state == 0).all()
    a, s = got["two triangles on one edge"]
    assert a.index.tolist() == [1, 2, 0, 2, 3, 0, 1, 3, 1, 2] and a.vertex_flags.tolist() == [1, 1, 1, 1]
    a, s = got["a doubled triangle"]                                                # uses 4 on the edges of (0, 2, 1): its three vertices pin
    assert a.counts == [12, 3, 0, 0] and a.vertex_flags.tolist() == [1, 1, 1, 0]
    assert got["a doubled triangle, turned"][0].vertex_flags.tolist() == [1, 1, 1, 0]
    a, s = got["a triangle (a, a, b)"]                                              # (1, 1, 2) adds two uses to the edge 1 - 2, (3, 0, 3) two to 0 - 3
    assert a.counts == [12, 4, 0, 0]
    a, s = got["an index out of range"]
    assert a.counts == [12, 0, 0, 3] and got["a tetrahedron"][1].vertices.tobytes() == s.vertices.tobytes()
    a, s = got["an isolated vertex"]
    assert a.vertex_flags.tolist() == [0, 0, 0, 0, 2] and a.counts == [12, 0, 1, 0] and s.vertex_state.tolist() == [0, 0, 0, 0, 8] and s.counts == [0, 0, 0, 1]
    assert got["nv = 0"][0].ptr.tolist() == [0] and got["nv = 0"][1].vertices.shape == (0, 3)
    a, s = got["nt = 0 with vertices"]
    assert a.ptr.tolist() == [0] * 6 and a.counts == [0, 0, 5, 0] and (s.normals == 0).all()
    a, s = got["a fan of 1,000 triangles"]
    assert a.ptr[1] == 1000 and a.vertex_flags[0] == 0 and (a.vertex_flags[1:] == 1).all() and s.vertex_state[0] == 0 and s.counts[0] == 1000


# ------------------------------------------------------------------------------------------- the README's table
@pytest.mark.parametrize("name,iterations,mu", sorted(TABLE, key=str))
def test_the_table(name, iterations, mu):
    s, got = figures(name, iterations, mu)
    print(name, iterations, mu, got)
    want = TABLE[(name, iterations, mu)]
    for g, w in zip(got, want):
        assert w is None or g == w, (got, want)
    assert s.counts == [0, 0, 0, 0] and np.isfinite(s.vertices).all()


def test_taubin_keeps_the_volume_a_laplacian_loses():
    """Ten Taubin iterations halve the angular error of the faces and keep the volume to 0.06 %; three plain Laplacian steps
    lose 0.7 % of it.  On the analytic sphere and the torus the ten iterations change the volume less than the three steps."""
    v0 = figures("scene", 0, -0.53)[1]
    t10, l3 = figures("scene", 10, -0.53)[1], figures("scene", 3, None)[1]
    assert t10[2] < 0.55 * v0[2] and abs(t10[3] / v0[3] - 1) < 0.0007 and 0.006 < 1 - l3[3] / v0[3] < 0.008
    assert abs(t10[5] - v0[5]) < 0.005                                              # the bias of the TSDF stays
    for name in ("sphere", "torus"):
        before, taubin, laplace = figures(name, 0, -0.53)[1], figures(name, 10, -0.53)[1], figures(name, 3, None)[1]
        print(name, before, taubin, laplace)
        assert laplace[3] < before[3] and abs(taubin[3] - before[3]) < before[3] - laplace[3]


# ------------------------------------------------------------------------------------------- properties of the rule
def test_smoothing_does_not_depend_on_the_order_of_the_triangles():
    """The adjacency is a set per vertex, so the vertices' bytes do not depend on the order or the rotation of the triangles.
    The normals sum the faces in ascending half-edge: their bytes are claimed for a fixed triangle order only, their
    direction for any."""
    m = dr.scene_sphere()[0]
    rng = np.random.default_rng(7)
    order = rng.permutation(len(m.triangles))
    turned = np.stack([np.roll(t, k) for t, k in zip(m.triangles[order], rng.integers(0, 3, len(order)))])
    a, b = sr.smooth(m.vertices, m.triangles, 5), sr.smooth(m.vertices, turned, 5)
    sr.assert_same_adjacency(a.adjacency, b.adjacency)
    assert a.vertices.tobytes() == b.vertices.tobytes() and a.vertex_state.tobytes() == b.vertex_state.tobytes()
    assert np.abs(a.normals.astype(np.float64) - b.normals).max() < 1e-6


def test_a_vertex_permutation_maps_through():
    m = dr.analytic_sphere()
    rng = np.random.default_rng(9)
    new_of_old = rng.permutation(len(m.vertices))
    old_of_new = np.argsort(new_of_old)
    a = sr.smooth(m.vertices, m.triangles, 1, mu=None, normals=False)
    b = sr.smooth(m.vertices[old_of_new], new_of_old[m.triangles].astype(np.int32), 1, mu=None, normals=False)
    # the neighbours are summed in ascending NEW index: the same set in another order, so equal up to rounding only
    assert np.abs(a.vertices - b.vertices[new_of_old]).max() < 1e-13
    assert sorted(np.diff(a.adjacency.ptr).tolist()) == sorted(np.diff(b.adjacency.ptr).tolist())
    for v in range(0, len(m.vertices), 53):
        mine = a.adjacency.index[a.adjacency.ptr[v]:a.adjacency.ptr[v + 1]]
        w = new_of_old[v]
        assert sorted(new_of_old[mine].tolist()) == b.adjacency.index[b.adjacency.ptr[w]:b.adjacency.ptr[w + 1]].tolist()


def test_pinned_and_unsound_vertices_keep_their_bytes():
    cases = {name: (v, t, p) for name, v, t, p in sr.hand_cases()}
    v, t, pinned = cases["a caller's pinned"]
    s = sr.smooth(v, t, 10, pinned=pinned)
    assert s.counts == [0, int(pinned.sum()), 0, 0] and s.vertices[pinned != 0].tobytes() == v[pinned != 0].tobytes()
    assert (s.vertices[pinned == 0] != v[pinned == 0]).any(axis=1).all() and (s.vertex_state == 2 * pinned).all()
    v, t, _ = cases["a NaN and an inf vertex"]
    s = sr.smooth(v, t, 10)
    bad = [100, 500, 501]
    assert s.counts == [0, 0, 3, 0] and np.flatnonzero(s.vertex_state).tolist() == bad and sr.bits(s.vertices[bad]).tobytes() == sr.bits(v[bad]).tobytes()
    rest = np.setdiff1d(np.arange(len(v)), bad)
    assert np.isfinite(s.vertices[rest]).all()                                      # one NaN does not spread
    near = s.adjacency.index[s.adjacency.ptr[100]:s.adjacency.ptr[101]]
    assert (s.vertices[near] != v[near]).any(axis=1).all()                          # its neighbours move, over their other neighbours
    v, t, _ = cases["values that overflow"]
    with np.errstate(all="ignore"):
        s = sr.smooth(v, t, 10)
    assert s.counts == [0, 0, 0, 0] and not np.isfinite(s.vertices).all()           # values that overflow during the steps propagate


def test_zero_iterations_is_the_identity():
    m = dr.torus()
    for mu in (-0.53, None):
        s = sr.smooth(m.vertices, m.triangles, 0, mu=mu)
        assert s.vertices.tobytes() == m.vertices.tobytes()
    # and a factor of 1 without mu puts every vertex at the mean of its neighbours
    s = sr.smooth(m.vertices, m.triangles, 1, lam=1.0, mu=None, normals=False)
    a = s.adjacency
    for v in (0, 17, 2629):
        assert np.abs(s.vertices[v] - m.vertices[a.index[a.ptr[v]:a.ptr[v + 1]]].mean(axis=0)).max() < 1e-12


def test_an_open_mesh_pins_its_outline():
    v, t = dr.strip(40)
    v[:, 2] += np.random.default_rng(3).uniform(-0.2, 0.2, len(v))
    a = sr.adjacency(t, len(v))
    assert (a.vertex_flags == 1).all()                              # every vertex of a strip is on its outline
    assert sr.smooth(v, t, 5).vertices.tobytes() == v.tobytes()
    free = sr.smooth(v, t, 5, pin_boundary=False)
    assert (free.vertices != v).any(axis=1).all() and free.counts == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------- the headers on the host
def build_check(tmp_path, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"), "-I" + os.path.join(ROOT, "tests", "native"),
           CHECK_SRC, "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return str(exe)


def rule_cases():
    """(name, vertices, triangles, pinned, iterations, lam, mu, pin_boundary)."""
    out = [(name, v, t, p, 2, 0.5, -0.53, True) for name, v, t, p in sr.hand_cases()]
    s, torus, scene8 = dr.analytic_sphere(), dr.torus(), dr.scene_sphere(8)[0]
    out += [("sphere 1", s.vertices, s.triangles, None, 1, 0.5, -0.53, True), ("sphere 10", s.vertices, s.triangles, None, 10, 0.5, -0.53, True),
            ("sphere, laplacian 3", s.vertices, s.triangles, None, 3, 0.5, None, True), ("sphere 0", s.vertices, s.triangles, None, 0, 0.5, -0.53, True),
            ("torus 2", torus.vertices, torus.triangles, None, 2, 0.63, -0.67, True), ("torus, laplacian 1", torus.vertices, torus.triangles, None, 1, 1.0, None, True),
            ("eight cameras, pinned", scene8.vertices, scene8.triangles, None, 3, 0.5, -0.53, True),
            ("eight cameras, free", scene8.vertices, scene8.triangles, None, 3, 0.5, -0.53, False)]
    v, t = dr.strip(259)
    out.append(("strip 259, free", v, t, None, 2, 0.5, -0.53, False))
    return out


def run_check(exe, tmp_path):
    run = subprocess.run([exe, "plan"], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])
    assert int(run.stdout.split()[1]) > 9000
    hx = lambda a: " ".join(f"{int(x):016x}" for x in np.ascontiguousarray(a, np.float64).view(np.uint64).reshape(-1))
    n_vertices = 0
    for i, (name, v, t, pinned, iterations, lam, mu, pin_boundary) in enumerate(rule_cases()):
        v = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
        path = tmp_path / f"mesh_{i}.txt"
        rows = [f"{len(v)} {len(t)} {iterations} {int(mu is not None)} {int(pin_boundary)} {int(pinned is not None)}", hx([lam]), hx([0.0 if mu is None else mu])]
        rows += [hx(v[j]) + ("" if pinned is None else f" {int(pinned[j])}") for j in range(len(v))]
        rows += [" ".join(str(int(x)) for x in row) for row in t]
        path.write_text("\n".join(rows) + "\n")
        run = subprocess.run([exe, "rule", str(path)], capture_output=True, text=True)
        assert run.returncode == 0, (name, run.stderr[-2000:])
        with np.errstate(all="ignore"):
            want = sr.smooth(v, t, iterations, lam, mu, pin_boundary, pinned)
        adj = want.adjacency
        lines = run.stdout.split("\n")[:-1]
        assert lines[0] == "A " + " ".join(str(x) for x in adj.counts) and lines[1] == "S " + " ".join(str(x) for x in want.counts), (name, lines[:2])
        ne, nv = adj.counts[0], len(v)
        assert [int(x.split()[1]) for x in lines[2:2 + ne]] == adj.index.tolist(), name
        assert lines[2 + ne + nv] == f"p {adj.ptr[nv]}" and len(lines) == 3 + ne + nv, name
        for j, line in enumerate(lines[2 + ne:2 + ne + nv]):
            got = line.split()
            assert [int(x) for x in got[1:4]] == [adj.ptr[j], adj.vertex_flags[j], want.vertex_state[j]], (name, j, line)
            xyz = sr.bits(np.array([int(x, 16) for x in got[4:7]], np.uint64).view(np.float64))
            nrm = sr.bits(np.array([int(x, 16) for x in got[7:10]], np.uint32).view(np.float32))
            assert xyz.tolist() == sr.bits(want.vertices[j]).tolist() and nrm.tolist() == sr.bits(want.normals[j]).tolist(), (name, j, line)
        n_vertices += nv
    assert n_vertices > 15000


def test_rule_and_plan_on_the_host(tmp_path):
    """The adjacency, the states, the steps and the normals of the host build bit for bit against the restatement; the
    argument checks branch by branch and in their firing order, the layouts over a grid of sizes, where the steps write."""
    run_check(build_check(tmp_path, ["-O2"], "mesh_smooth_check"), tmp_path)


def test_rule_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone."""
    run_check(build_check(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
                          "mesh_smooth_check_san"), tmp_path)


# ------------------------------------------------------------------------------------------- argument checks, no device
def test_argument_checks_without_gpu():
    import sfm_amd
    from sfm_amd import depth as dm
    from sfm_amd import mesh as mm
    from sfm_amd import mesh_smooth as ms
    for name in ("smooth_mesh", "mesh_adjacency", "mesh_vertex_normals", "check_smooth_arguments", "MeshAdjacency"):
        assert getattr(sfm_amd, name) is getattr(ms, name) is getattr(mm, name), name
    assert [p.default for p in list(inspect.signature(mm.Mesh.smooth).parameters.values())[1:]] == [10, 0.5, -0.53, True, None, "recompute", None]
    assert [p.default for p in list(inspect.signature(ms.smooth_mesh).parameters.values())[2:]] == [None, 10, 0.5, -0.53, True, None, "recompute", 0]
    assert inspect.signature(dm.dense_from_reconstruction).parameters["smooth"].default is None
    check = ms.check_smooth_arguments
    assert ms.MAX_TRIANGLES == (2 ** 31 - 1) // 6 and ms.MAX_ITERATIONS == 1000
    assert check() == (10, 0.5, -0.53, True, None, "recompute", None, None, None, None)
    assert check(0, 1, -2, False, None, "keep")[:6] == (0, 1.0, -2.0, False, None, "keep") and check(1000, np.float32(0.25), None)[:3] == (1000, 0.25, None)
    tri = [[0, 1, 2], [2, 1, 3]]
    got = check(3, pinned=[True, False, False, True], triangles=tri, vertices=np.zeros((4, 3)), vertex_normals=np.zeros((4, 3)))
    assert got[4].dtype == np.uint8 and got[4].tolist() == [1, 0, 0, 1] and got[6] == 4 and got[7].dtype == np.int32 and got[8].dtype == np.float64 and got[9].dtype == np.float32
    assert check(pinned=np.array([0, 7, 255], np.uint8), n_vertices=3)[4].tolist() == [0, 7, 255]
    for kw in (dict(iterations=-1), dict(iterations=1001), dict(iterations=2.0), dict(iterations=None), dict(iterations=True), dict(lam=0), dict(lam=-0.5),
               dict(lam=1.0001), dict(lam=np.nan), dict(lam=np.inf), dict(lam=None), dict(lam="0.5"), dict(lam=True), dict(mu=-0.5), dict(mu=-0.4), dict(mu=0.53),
               dict(mu=0), dict(mu=-2.0001), dict(mu=np.nan), dict(mu=-np.inf), dict(mu="x"), dict(lam=0.6, mu=-0.53), dict(normals="zero"), dict(normals=None),
               dict(normals=1), dict(pinned=[0, 1, 0], n_vertices=4), dict(pinned=np.zeros(4, np.int32), n_vertices=4), dict(pinned=np.zeros((4, 1), np.uint8), n_vertices=4),
               dict(pinned=np.zeros(4), n_vertices=4), dict(n_vertices=-1), dict(n_vertices=1 << 31), dict(triangles=[[0, 1]]), dict(triangles=[[0.0, 1.0, 2.0]]),
               dict(triangles=[[0, 1, 1 << 31]]), dict(vertices=np.zeros((4, 2))),
               dict(vertices=np.zeros((4, 3)), n_vertices=5), dict(vertices=np.zeros((4, 3)), vertex_normals=np.zeros((3, 3)))):
        with pytest.raises(ValueError):
            check(**kw)
    v = np.zeros((4, 3))
    for call in (lambda: ms.smooth_mesh(None, tri), lambda: ms.smooth_mesh(v, tri, iterations=-1), lambda: ms.smooth_mesh(v, tri, lam=2.0),
                 lambda: ms.smooth_mesh(v, tri, mu=0.1), lambda: ms.smooth_mesh(v, tri, normals_mode="both"), lambda: ms.smooth_mesh(v, tri, pinned=[1, 0]),
                 lambda: ms.smooth_mesh(v, [[0, 1]]), lambda: ms.smooth_mesh(v, tri, normals=np.zeros((3, 3))), lambda: ms.mesh_adjacency(tri, None),
                 lambda: ms.mesh_adjacency(tri, -1), lambda: ms.mesh_adjacency([[0, 1]], 4), lambda: ms.mesh_vertex_normals(None, tri),
                 lambda: ms.mesh_vertex_normals(np.zeros((4, 2)), tri), lambda: dm.dense_from_reconstruction(None, [], smooth=10),
                 lambda: dm.dense_from_reconstruction(None, [], mesh=True, smooth=-1), lambda: dm.dense_from_reconstruction(None, [], mesh=True, smooth=1001),
                 lambda: dm.dense_from_reconstruction(None, [], mesh=True, smooth=2.5), lambda: dm.dense_from_reconstruction(None, [], mesh=True, smooth="10")):
        with pytest.raises(ValueError):
            call()
    bare = mm.Mesh({}, 0, 0)
    assert bare.vertex_state is None and bare.n_pinned_boundary is None and bare.n_pinned_given is None and bare.n_isolated is None and bare.adjacency_before is None
    for kw in (dict(iterations=-1), dict(lam=0.0), dict(mu=-0.1), dict(normals="x"), dict(pinned=[1]), dict(adjacency="no")):
        with pytest.raises(ValueError):
            bare.smooth(**kw)


def test_c_entry_points_reject_a_null_handle_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    need = ctypes.c_int64(-1)
    one, two = ctypes.c_void_p(1), ctypes.c_void_p(2)
    assert lib.sfm_mesh_adjacency_workspace_bytes(None, 5, 2, ctypes.byref(need)) == -1 and need.value == -1
    assert lib.sfm_mesh_smooth_workspace_bytes(None, 5, ctypes.byref(need)) == -1 and need.value == -1
    assert lib.sfm_mesh_vertex_normals_workspace_bytes(None, 5, 2, ctypes.byref(need)) == -1 and need.value == -1
    assert lib.sfm_mesh_adjacency(None, 0, 0, None, one, None, None, one, one, 4096) == -1
    assert lib.sfm_mesh_smooth(None, 0, None, one, None, 0, None, None, 1, 0.5, -0.53, 1, 10, None, None, one, two, 4096) == -1
    assert lib.sfm_mesh_vertex_normals(None, 0, 0, None, None, None, one, 4096) == -1
