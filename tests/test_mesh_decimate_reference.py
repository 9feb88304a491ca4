"""Decimation by vertex clustering without a GPU: the two restatements (tests/mesh_decimate_reference.py) against each other
on the meshes of the README's table and on the hand cases, the table itself recomputed - its integers asserted exactly, the
quadric against the mean and against the loss the restatement measured, the cancel rule against "keep the first" -, the host
build of mesh_decimate_rule.h and mesh_decimate_plan.h plain and under the sanitizers as a stand-alone program, its clusters,
placements and kept triangles bit for bit those of the restatement, and the argument checks of the Python layer and of the C
entry points."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_decimate_reference as dr
import mesh_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "mesh_decimate_check.cpp")


def table_mesh(name):
    """(mesh, the origin of its volume, its voxel)."""
    if name == "sphere":
        return dr.analytic_sphere(), np.zeros(3), 1.0
    if name == "torus":
        return dr.torus(), np.zeros(3), 1.0
    mesh, voxel = dr.scene_sphere()
    return mesh, np.full(3, -1.4), voxel


# (mesh, cell in voxels) -> in V, in T, clusters, kept triangles, degenerate, dropped by the duplicate rule, clusters the
# quadric placed, referenced vertices, Euler characteristic over them, (boundary, non-manifold) edges, the same two and the
# triangle count with "keep the first", the volume in and out (mean, quadric) to 4 decimals, the quadric's relative loss as
# the restatement measured it; the grid starts at the origin of the mesh's volume
TABLE = {
    ("sphere", 1.5): (1008, 2012, 140, 276, 1736, 0, 127, 140, 2, (0, 0), (0, 0), 276, 324.0296, 302.3613, 316.2854, 0.0239),
    ("sphere", 2.0): (1008, 2012, 85, 164, 1844, 4, 80, 84, 2, (0, 0), (2, 2), 166, 324.0296, 286.2521, 310.8483, 0.0407),
    ("sphere", 3.0): (1008, 2012, 44, 84, 1928, 0, 38, 44, 2, (0, 0), (0, 0), 84, 324.0296, 243.1146, 290.9125, 0.1022),
    ("scene", 2.0): (7006, 14008, 592, 1176, 12824, 8, 568, 590, 2, (0, 0), (4, 4), 1180, 4.2562, 4.1786, 4.2350, 0.0050),
    ("scene", 3.0): (7006, 14008, 260, 516, 13492, 0, 244, 260, 2, (0, 0), (0, 0), 516, 4.2562, 4.0766, 4.1903, 0.0155),
    ("torus", 2.0): (2630, 5260, 212, 432, 4816, 12, 193, 211, 0, (0, 5), (3, 12), 438, 715.4020, 634.5488, 678.3100, 0.0518),
}
# the median over the referenced new vertices of the distance to the sphere, in voxels: mean / quadric
RADIAL = {1.5: (0.056, 0.015), 2.0: (0.085, 0.032), 3.0: (0.137, 0.073)}


# ------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("name,factor", sorted(TABLE))
@pytest.mark.parametrize("placement", [0, 1])
def test_the_two_restatements_agree_on_the_table_meshes(name, factor, placement):
    m, origin, voxel = table_mesh(name)
    for o in (origin, None):
        a = dr.decimate(m.vertices, m.triangles, m.normals, factor * voxel, o, placement)
        dr.assert_same(a, dr.decimate_loops(m.vertices, m.triangles, m.normals, factor * voxel, o, placement), (name, factor, placement))
        assert a.counts[1] == 0 and a.marks[1] == 0 and a.marks[4] == 0 and (a.cluster_placed.sum() > 0) == (placement == 1)
        assert a.marks[0] + a.marks[2] + a.marks[3] == len(m.triangles) and a.cluster_size.sum() == len(m.vertices)
        assert (np.diff(a.triangle_map) > 0).all() and (a.vertex_cluster[a.cluster_first] == np.arange(a.counts[0])).all()


@pytest.mark.parametrize("placement", [0, 1])
def test_the_two_restatements_agree_on_the_hand_cases(placement):
    got = {}
    for name, v, t, n, cell, origin in dr.hand_cases():
        a = dr.decimate(v, t, n, cell, origin, placement)
        dr.assert_same(a, dr.decimate_loops(v, t, n, cell, origin, placement), name)
        got[name] = a
    a = got["faces, origin, the ends of the grid, NaN, indices"]
    # on a face a vertex belongs to the cell above; -0.0 is at the origin, the number below it is not; 2^21 is outside
    assert a.vertex_cluster[:5].tolist() == [0, 1, 4, 6, 7] and a.vertex_cluster[[5, 6, 7, 9, 10, 11, 15]].tolist() == [-1] * 7 and a.vertex_cluster[8] >= 0
    assert a.counts == [9, 7] and a.marks == [5, 9, 2, 0, 0]
    a = got["duplicates: equal, two even and one odd, an even-odd pair"]
    # (0,1,2) twice as (0,1,2) and (6,4,5): the first; (0,1,3), (1,3,0) even and (3,1,6) odd: the first even; (0,2,3) and
    # (3,5,0): a pair, none; (2,1,3), (1,3,2), (3,5,4): three odd, the first; (7,1,2), (2,7,4) even and (5,1,7) odd: the first
    # even.  The cells of the vertices 4, 5, 6 are those of 1, 2, 0.
    assert a.vertex_cluster.tolist() == [0, 1, 2, 3, 1, 2, 0, 4] and a.triangle_map.tolist() == [0, 2, 7, 10]
    assert a.marks == [4, 0, 0, 9, 0] and a.triangles.tolist() == [[0, 1, 2], [0, 1, 3], [2, 1, 3], [4, 1, 2]]
    a = got["all in one cell"]
    assert a.counts == [1, 0] and a.marks == [0, 0, 4, 0, 0] and a.triangles.shape == (0, 3) and a.cluster_size.tolist() == [9]
    a = got["zero-area triangles only"]
    assert a.cluster_placed.tolist() == [0, 0, 0] and a.vertices[0].tolist() == [(0.2 + 0.4 + 0.6) / 3.0] * 3
    a, b = got["the solution leaves the box"], got["the same cone with its apex in the box"]
    assert a.cluster_placed.tolist() == [0, placement, placement, placement] and b.cluster_placed.tolist() == [placement] * 4
    if placement == 1:
        assert np.abs(b.vertices[0][:2] - 0.5).max() < 0.02 and 0.5 < b.vertices[0][2] <= 0.95 and a.vertices[0].tolist() == dr.decimate(*dr.hand_cases()[4][1:6], 0).vertices[0].tolist()
    assert got["nv = 0"].counts == [0, 0] and got["nv = 0"].vertices.shape == (0, 3) and got["nt = 0 with vertices"].marks == [0] * 5
    s = dr.analytic_sphere()
    shifted, plain = got["shifted by 1e5"], dr.decimate(s.vertices, s.triangles, s.normals, 2.0, np.zeros(3), placement)
    assert shifted.triangles.tobytes() == plain.triangles.tobytes() and shifted.vertex_cluster.tobytes() == plain.vertex_cluster.tobytes()
    assert np.abs(shifted.vertices - 1e5 - plain.vertices).max() < 1e-8


# ------------------------------------------------------------------------------------------- the README's table
@pytest.mark.parametrize("name,factor", sorted(TABLE))
def test_the_table(name, factor):
    nv, nt, nc, kept, degenerate, dropped, n_placed, used, chi, edges, first_edges, first_kept, vol_in, vol_mean, vol_quadric, loss = TABLE[(name, factor)]
    m, origin, voxel = table_mesh(name)
    assert (len(m.vertices), len(m.triangles)) == (nv, nt)
    mean = dr.decimate(m.vertices, m.triangles, m.normals, factor * voxel, origin, 0)
    quadric = dr.decimate(m.vertices, m.triangles, m.normals, factor * voxel, origin, 1)
    first = dr.decimate(m.vertices, m.triangles, m.normals, factor * voxel, origin, 1, duplicates="first")
    assert quadric.counts == [nc, 0] and quadric.marks == [kept, 0, degenerate, dropped, 0] and int(quadric.cluster_placed.sum()) == n_placed
    assert mean.triangles.tobytes() == quadric.triangles.tobytes() and mean.vertex_cluster.tobytes() == quadric.vertex_cluster.tobytes()
    assert dr.used_vertices(quadric.triangles) == used and mr.euler_characteristic(used, quadric.triangles) == chi
    assert dr.nonmanifold_edges(quadric.triangles) == edges and mr.is_closed_and_oriented(quadric.triangles) == (edges == (0, 0))
    assert len(first.triangles) == first_kept and dr.nonmanifold_edges(first.triangles) == first_edges
    v0, v1, v2 = mr.signed_volume(m.vertices, m.triangles), mr.signed_volume(mean.vertices, mean.triangles), mr.signed_volume(quadric.vertices, quadric.triangles)
    print(name, factor, "volume", v0, "mean", v1, "quadric", v2, "loss", 1 - v1 / v0, 1 - v2 / v0)
    assert (round(v0, 4), round(v1, 4), round(v2, 4)) == (vol_in, vol_mean, vol_quadric)
    if name != "torus":
        assert v2 > v1 and 1 - v2 / v0 <= loss + 0.01                  # the quadric keeps more of the volume than the mean
        assert edges == (0, 0) and chi == 2                          # closed, oriented, a sphere
    if factor == 2.0:
        assert not mr.is_closed_and_oriented(first.triangles)          # why the cancel rule exists
    if name == "sphere":
        got = (round(dr.median_radial_error(mean), 3), round(dr.median_radial_error(quadric), 3))
        print(name, factor, "radial", got)
        assert got == RADIAL[factor] and got[1] < 0.6 * got[0]
    # the new vertices stay in their cells, the normals are unit or zero
    idx = np.floor((m.vertices[quadric.cluster_first] - origin) / (factor * voxel))
    assert ((origin + factor * voxel * idx <= quadric.vertices) & (quadric.vertices <= origin + factor * voxel * (idx + 1))).all()
    length = np.linalg.norm(quadric.normals.astype(np.float64), axis=1)
    assert (np.abs(length[length > 0] - 1) < 1e-6).all()


def test_nothing_depends_on_the_order_of_the_triangles():
    m, origin, voxel = table_mesh("scene")
    rng = np.random.default_rng(7)
    order = rng.permutation(len(m.triangles))
    turned = np.stack([np.roll(t, k) for t, k in zip(m.triangles[order], rng.integers(0, 3, len(order)))])
    a = dr.decimate(m.vertices, m.triangles, m.normals, 2 * voxel, origin, 0)
    b = dr.decimate(m.vertices, turned, m.normals, 2 * voxel, origin, 0)
    assert a.vertices.tobytes() == b.vertices.tobytes() and a.marks == b.marks
    canon = lambda t: sorted(tuple(np.roll(x, -int(np.argmin(x)))) for x in t.tolist())
    assert canon(a.triangles) == canon(b.triangles)
    # a cell smaller than every edge: the mesh comes back with its vertices in key order (the mean of one vertex is the vertex)
    s = dr.analytic_sphere()
    d = dr.decimate(s.vertices, s.triangles, s.normals, 2.0 ** -16, np.zeros(3), 0)
    assert d.counts == [len(s.vertices), 0] and d.marks == [len(s.triangles), 0, 0, 0, 0] and (d.cluster_size == 1).all()
    assert d.triangles.tobytes() == d.vertex_cluster[s.triangles].astype(np.int32).tobytes() and d.vertices[d.vertex_cluster].tobytes() == s.vertices.tobytes()


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
    out = [(name, v, t, n, cell, origin) for name, v, t, n, cell, origin in dr.hand_cases()]
    for name, factor in (("sphere", 1.5), ("sphere", 2.0), ("torus", 2.0), ("scene", 2.0)):
        m, origin, voxel = table_mesh(name)
        out.append((f"{name} {factor}", m.vertices, m.triangles, m.normals, factor * voxel, origin))
    return out


def run_check(exe, tmp_path):
    run = subprocess.run([exe, "plan"], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok "), (run.stdout, run.stderr[-2000:])
    assert int(run.stdout.split()[1]) > 8000
    hx = lambda a, kind: " ".join(f"{int(x):0{16 if kind == np.uint64 else 8}x}" for x in np.ascontiguousarray(a).view(kind).reshape(-1))
    n_clusters = 0
    for i, (name, v, t, n, cell, origin) in enumerate(rule_cases()):
        v = np.ascontiguousarray(v, np.float64).reshape(-1, 3)
        for placement in (0, 1):
            path = tmp_path / f"mesh_{i}_{placement}.txt"
            rows = [f"{len(v)} {len(t)} {placement} {int(n is not None)}", hx(np.asarray(origin, np.float64), np.uint64), hx(np.array([cell], np.float64), np.uint64)]
            rows += [hx(v[j], np.uint64) + ("" if n is None else " " + hx(np.asarray(n[j], np.float32), np.uint32)) for j in range(len(v))]
            rows += [" ".join(str(int(x)) for x in row) for row in t]
            path.write_text("\n".join(rows) + "\n")
            run = subprocess.run([exe, "rule", str(path)], capture_output=True, text=True)
            assert run.returncode == 0, (name, run.stderr[-2000:])
            want = dr.decimate(v, t, n, cell, origin, placement)
            lines = run.stdout.split("\n")[:-1]
            assert lines[0] == f"C {want.counts[0]} {want.counts[1]}" and lines[1] == "M " + " ".join(str(x) for x in want.marks[:4]), (name, lines[:2])
            nv, nc = len(v), want.counts[0]
            assert [int(x.split()[1]) for x in lines[2:2 + nv]] == want.vertex_cluster.tolist(), name
            for c, line in enumerate(lines[2 + nv:2 + nv + nc]):
                got = line.split()
                xyz = dr.bits(np.array([int(x, 16) for x in got[4:7]], np.uint64).view(np.float64))
                nrm = dr.bits(np.array([int(x, 16) for x in got[7:10]], np.uint32).view(np.float32))
                assert [int(x) for x in got[1:4]] == [want.cluster_first[c], want.cluster_size[c], want.cluster_placed[c]], (name, c, line)
                assert xyz.tolist() == dr.bits(want.vertices[c]).tolist() and nrm.tolist() == dr.bits(want.normals[c]).tolist(), (name, placement, c, line)
            tris = [[int(x) for x in line.split()[1:]] for line in lines[2 + nv + nc:]]
            assert [r[0] for r in tris] == want.triangle_map.tolist() and [r[1:] for r in tris] == want.triangles.tolist(), name
            n_clusters += nc
    assert n_clusters > 2000


def test_rule_and_plan_on_the_host(tmp_path):
    """The cells, the placements and the duplicate rule of the host build bit for bit against the restatement; the argument
    checks branch by branch and in their firing order, the layout over a grid of sizes, the keys of the triples."""
    run_check(build_check(tmp_path, ["-O2"], "mesh_decimate_check"), tmp_path)


def test_rule_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone."""
    run_check(build_check(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
                          "mesh_decimate_check_san"), tmp_path)


# ------------------------------------------------------------------------------------------- argument checks, no device
def test_argument_checks_without_gpu():
    import sfm_amd
    from sfm_amd import depth as dm
    from sfm_amd import mesh as mm
    from sfm_amd import mesh_decimate as md
    assert sfm_amd.decimate_mesh is md.decimate_mesh is mm.decimate_mesh and sfm_amd.check_decimate_arguments is md.check_decimate_arguments is mm.check_decimate_arguments
    assert [p.default for p in list(inspect.signature(mm.Mesh.decimate).parameters.values())[1:]] == [None, 2.0, None, "quadric"]
    assert [p.default for p in list(inspect.signature(md.decimate_mesh).parameters.values())[2:]] == [None, None, None, "quadric", 0]
    assert inspect.signature(dm.dense_from_reconstruction).parameters["decimate"].default is None
    check = md.check_decimate_arguments
    assert check() == (1.0, None, 1, None, None, None, None) and check(2, placement="mean")[:3] == (2.0, None, 0) and check(np.float32(0.5))[0] == 0.5
    tri = [[0, 1, 2], [2, 1, 3]]
    got = check(0.25, [1, 2, 3], "quadric", None, tri, np.zeros((4, 3)), np.zeros((4, 3)))
    assert got[1].dtype == np.float64 and got[1].tolist() == [1.0, 2.0, 3.0] and got[3] == 4 and got[4].dtype == np.int32 and got[5].dtype == np.float64
    assert got[6].dtype == np.float32
    for kw in (dict(cell=0), dict(cell=-1.0), dict(cell=np.nan), dict(cell=np.inf), dict(cell=None), dict(cell="1"), dict(cell=True), dict(origin=[0, 0]),
               dict(origin=[0, np.nan, 0]), dict(origin=[0, np.inf, 0]), dict(origin="abc"), dict(placement="median"), dict(placement=1), dict(placement=None),
               dict(n_vertices=-1), dict(n_vertices=1 << 31), dict(triangles=[[0, 1]]), dict(triangles=[[0.0, 1.0, 2.0]]), dict(triangles=[[0, 1, 1 << 31]]),
               dict(vertices=np.zeros((4, 2))), dict(vertices=np.zeros((4, 3)), n_vertices=5), dict(vertices=np.zeros((4, 3)), normals=np.zeros((3, 3)))):
        with pytest.raises(ValueError):
            check(**kw)
    v = np.zeros((4, 3))
    for call in (lambda: md.decimate_mesh(None, tri, cell=1.0), lambda: md.decimate_mesh(v, tri), lambda: md.decimate_mesh(v, tri, cell=0.0),
                 lambda: md.decimate_mesh(v, tri, cell=1.0, placement="best"), lambda: md.decimate_mesh(v, tri, cell=1.0, origin=[0, 0, np.nan]),
                 lambda: md.decimate_mesh(v, [[0, 1]], cell=1.0), lambda: dm.dense_from_reconstruction(None, [], decimate=2.0),
                 lambda: dm.dense_from_reconstruction(None, [], mesh=True, decimate=0), lambda: dm.dense_from_reconstruction(None, [], mesh=True, decimate=np.nan),
                 lambda: dm.dense_from_reconstruction(None, [], mesh=True, decimate="2")):
        with pytest.raises(ValueError):
            call()
    bare = mm.Mesh({}, 0, 0)
    assert bare.vertex_cluster is None and bare.cluster_first is None and bare.cluster_size is None and bare.cluster_placed is None
    assert bare.n_degenerate is None and bare.n_cancelled is None and bare.n_unsound_vertices is None and bare.n_unsound_triangles is None
    assert bare.cell is None and bare.origin is None
    with pytest.raises(ValueError, match="no volume"):
        bare.decimate()
    for kw in (dict(cell=0.0), dict(cell=1.0, placement="x"), dict(cell=1.0, origin=[1, 2]), dict(factor=0.0), dict(factor=np.inf), dict(factor="2")):
        with pytest.raises(ValueError):
            bare.decimate(**kw)


def test_c_entry_points_reject_a_null_handle_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    need = ctypes.c_int64(-1)
    one = ctypes.c_void_p(1)
    origin = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    o = ctypes.cast(origin, ctypes.c_void_p)
    assert lib.sfm_mesh_decimate_workspace_bytes(None, 5, 2, ctypes.byref(need)) == -1 and need.value == -1
    assert lib.sfm_mesh_decimate_cluster(None, 0, 0, None, o, 1.0, None, one, None, None, one, one, 4096) == -1
    assert lib.sfm_mesh_decimate_mark(None, 0, 0, 0, None, None, None, one, one, 4096) == -1
    assert lib.sfm_mesh_decimate_emit(None, 0, 0, 0, None, None, None, None, None, None, o, 1.0, 1, 0, 0, None, None, None, None, None, one, 4096) == -1
