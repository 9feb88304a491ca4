"""The edge table and hole filling without a GPU: the two restatements (tests/mesh_fill_reference.py) against each other and
against the measures of tests/mesh_reference.py, the hand cases, the README's table of the sphere and default-scene meshes
asserted in its integers, the independence of the order, the host build of mesh_fill_rule.h and mesh_fill_plan.h plain and
under the sanitizers as a stand-alone program - its centroids and normals bit for bit those of the restatement - and the
argument checks of the Python layer and of the C entry points."""
import ctypes
import inspect
import os
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

import mesh_clean_reference as cr
import mesh_fill_reference as fr
import mesh_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SRC = os.path.join(ROOT, "tests", "native", "mesh_fill_check.cpp")
SOUPS = [(1, 1, 0), (2, 4, 1), (3, 6, 40), (4, 30, 90), (5, 12, 300), (6, 200, 700), (7, 3, 50), (8, 64, 256)]

_MESHES = {}


def sphere_mesh(n_cams, min_weight):
    key = ("sphere", n_cams, min_weight)
    if key not in _MESHES:
        if ("field", n_cams) not in _MESHES:
            proj, depth, origin, voxel, shape, trunc = mr.sphere_scene(n_cams=n_cams)
            _MESHES[("field", n_cams)] = (mr.integrate(proj, depth, None, origin, voxel, shape, trunc), origin, voxel, shape)
        (tsdf, weight), origin, voxel, shape = _MESHES[("field", n_cams)]
        _MESHES[key] = mr.mesh(tsdf, weight, origin, voxel, shape, min_weight)
    return _MESHES[key]


def used_vertices(tri):
    return len(np.unique(np.asarray(tri)))


# ------------------------------------------------------------------------------------------- the two restatements
@pytest.mark.parametrize("seed,n_vertices,n_triangles", SOUPS)
def test_the_two_tables_agree_on_random_soups(seed, n_vertices, n_triangles):
    tri = fr.random_soup(seed, n_vertices, n_triangles)
    a, b = fr.edges(tri, n_vertices), fr.edges_loops(tri, n_vertices)
    fr.assert_same_edges(a, b, seed)
    n = 3 * n_triangles
    assert a.uses.shape == (n,) and a.counts[7] == 0 and a.counts[4] == len(a.loop_leader)
    assert ((a.twin >= 0) <= (a.uses == 2)).all() and ((a.next >= 0) <= (a.uses == 1)).all() and ((a.loop >= 0) <= (a.next >= 0)).all()
    t = np.flatnonzero(a.twin >= 0)
    assert (a.twin[a.twin[t]] == t).all()
    nx = a.next[a.next >= 0]
    assert len(np.unique(nx)) == len(nx)                           # injective where it is defined
    assert (np.diff(a.loop_leader) > 0).all() and (a.loop[a.loop_leader] == np.arange(len(a.loop_leader))).all()
    assert np.array_equal(np.bincount(a.loop[a.loop >= 0], minlength=len(a.loop_leader)), a.loop_edges) and (a.loop_edges >= 3).all()


@pytest.mark.parametrize("seed", range(8))
def test_the_two_fills_agree_on_random_surfaces(seed):
    v, tri = fr.random_surface(seed, 10 + seed, 0.15 + 0.03 * seed)
    nv = len(v)
    a, b = fr.edges(tri, nv), fr.edges_loops(tri, nv)
    fr.assert_same_edges(a, b, seed)
    for max_edges in (3, 4, 8, 16, 64):
        f, g = fr.fill(a, tri, nv, v, max_edges), fr.fill_loops(b, tri, nv, v, max_edges)
        fr.assert_same_fill(f, g, (seed, max_edges))
        assert f.counts[1] == len(f.triangles) == int((f.halfedge_fill >= 0).sum()) and f.counts[0] == len(f.vertices) == len(f.name)
        assert (np.diff(f.name) > 0).all() and (np.diff(f.triangle_halfedge) > 0).all() and (f.halfedge_fill[f.name] == np.arange(len(f.name))).all()
        sizes = np.bincount(f.halfedge_fill[f.halfedge_fill >= 0], minlength=len(f.name))
        assert ((sizes >= 3) & (sizes <= max_edges)).all()
        # every filled half-edge gets its twin: the boundary shrinks by exactly the fill triangles, and nothing else changes
        vv, nn, tt = fr.filled_mesh(v, np.zeros((nv, 3), np.float32), tri, f)
        after = fr.edges(tt, len(vv))
        assert after.counts[1] == a.counts[1] - f.counts[1] and after.counts[2] == 0 and after.counts[3] == 0
        assert after.counts[0] == a.counts[0] + f.counts[1] and vv[:nv].tobytes() == v.tobytes() and tt[:len(tri)].tobytes() == tri.tobytes()


def test_the_measures_of_the_mesh_reference():
    for v, tri in (fr.cube_less_one_quad(), fr.quad_grid(5, 4, [6, 12]), fr.touching_blocks(1, 1, 1, 1), fr.random_surface(3)):
        e = fr.edges(tri, len(v))
        ec = mr.edge_counts(tri)
        a, b, live, _ = fr._ends(tri, len(v))
        assert live.all()
        assert e.uses.tolist() == [ec[(int(p), int(q))] + ec.get((int(q), int(p)), 0) for p, q in zip(a, b)]
        assert fr.is_closed(e) == mr.is_closed_and_oriented(tri)
        assert fr.euler(tri, len(v), e) == mr.euler_characteristic(used_vertices(tri), tri)
    m = sphere_mesh(14, 1)
    e = fr.edges(m.triangles, len(m.vertices))
    assert fr.is_closed(e) and mr.is_closed_and_oriented(m.triangles)
    assert fr.euler(m.triangles, len(m.vertices), e) == mr.euler_characteristic(len(m.vertices), m.triangles) == 2


# ------------------------------------------------------------------------------------------- hand cases
def table(tri, nv, fn=fr.edges):
    return fn(np.array(tri, np.int32).reshape(-1, 3), nv)


@pytest.mark.parametrize("fn", [fr.edges, fr.edges_loops])
def test_hand_cases_of_the_table(fn):
    none = table([], 0, fn)
    assert none.counts == [0] * 8 and none.uses.shape == (0,) and none.loop_leader.shape == (0,)
    assert table([], 5, fn).counts == [0] * 8
    one = table([(0, 1, 2)], 3, fn)
    assert one.counts == [3, 3, 0, 0, 1, 0, 0, 0] and one.uses.tolist() == [1, 1, 1] and one.twin.tolist() == [-1] * 3
    assert one.next.tolist() == [1, 2, 0] and one.loop.tolist() == [0, 0, 0] and one.loop_leader.tolist() == [0] and one.loop_edges.tolist() == [3]
    tet = table([(0, 2, 1), (0, 1, 3), (1, 2, 3)], 4, fn)          # the face (0, 3, 2) is missing
    assert tet.counts == [6, 3, 0, 0, 1, 0, 0, 0] and tet.loop_edges.tolist() == [3] and sorted(tet.uses.tolist()) == [1, 1, 1, 2, 2, 2, 2, 2, 2]
    bow = table([(0, 1, 2), (2, 3, 4)], 5, fn)                     # they share vertex 2 only: two fans, two loops
    assert bow.counts == [6, 6, 0, 0, 2, 0, 0, 0] and bow.next.tolist() == [1, 2, 0, 4, 5, 3] and bow.loop.tolist() == [0, 0, 0, 1, 1, 1]
    fin = table([(0, 1, 2), (1, 0, 3), (0, 1, 4)], 5, fn)          # three triangles on the edge {0, 1}
    assert fin.counts == [7, 6, 0, 1, 0, 6, 0, 0] and fin.uses[[0, 3, 6]].tolist() == [3, 3, 3] and fin.twin.tolist() == [-1] * 9
    assert fin.next.tolist() == [-1, 2, -1, -1, 5, -1, -1, 8, -1]
    same = table([(0, 1, 2), (0, 1, 3)], 4, fn)                    # the edge 0 -> 1 twice in the same direction
    assert same.counts == [5, 4, 1, 0, 0, 4, 0, 0] and same.uses[[0, 3]].tolist() == [2, 2] and same.twin.tolist() == [-1] * 6
    # a repeated index and unsound ones beside a hole: (2, 1, 1) puts 2 -> 1 and 1 -> 2 on the edge that 1 -> 2 of the first uses
    odd = table([(0, 1, 2), (2, 1, 1), (0, 2, 7), (-1, 0, 1), (3, 3, 3)], 4, fn)
    assert odd.counts == [3, 2, 0, 1, 0, 2, 2, 0] and odd.uses.tolist() == [1, 3, 1, 3, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert odd.twin.tolist() == [-1] * 15 and odd.next.tolist() == [-1, -1, 0] + [-1] * 12
    flat = table([(0, 1, 1)], 2, fn)                               # 1 -> 0 is the twin of 0 -> 1
    assert flat.counts == [1, 0, 0, 0, 0, 0, 0, 0] and flat.uses.tolist() == [2, 0, 2] and flat.twin.tolist() == [2, -1, 0]


def test_hand_cases_of_the_fill():
    v3 = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], np.float64)
    tri = np.array([(0, 1, 2)], np.int32)
    e = fr.edges(tri, 3)
    f = fr.fill(e, tri, 3, v3)
    assert f.counts == [1, 3, 0, 0] and f.triangles.tolist() == [[1, 0, 3], [2, 1, 3], [0, 2, 3]] and f.name.tolist() == [0]
    assert f.vertices.tolist() == [[2 / 3, 2 / 3, 0.0]] and f.normals.tolist() == [[0.0, 0.0, -1.0]] and f.triangle_halfedge.tolist() == [0, 1, 2]
    vv, nn, tt = fr.filled_mesh(v3, np.zeros((3, 3), np.float32), tri, f)
    after = fr.edges(tt, 4)
    assert fr.is_closed(after) and fr.euler(tt, 4, after) == 2
    assert fr.fill(e, tri, 3, v3, 2).counts == [0, 0, 1, 0]
    # a tetrahedron less one face, a cube less one quad: closed with euler 2, and the patch faces outwards
    tet_v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    tet = np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3)], np.int32)
    for v, t in ((tet_v, tet), fr.cube_less_one_quad()):
        e, f, (vv, nn, tt) = fr.fill_mesh(v, np.zeros((len(v), 3), np.float32), t)
        after = fr.edges(tt, len(vv))
        assert f.counts[0] == 1 and fr.is_closed(after) and fr.euler(tt, len(vv), after) == 2 and mr.is_closed_and_oriented(tt)
        assert mr.signed_volume(vv, tt) > mr.signed_volume(v, t) - 1e-12 and mr.signed_volume(vv, tt) > 0
    cube_v, cube_t = fr.cube_less_one_quad()
    assert fr.fill_mesh(cube_v, np.zeros((8, 3), np.float32), cube_t)[1].normals.tolist() == [[0.0, 0.0, 1.0]]
    # two holes that touch at a vertex: one loop, two sub-loops, both filled
    v, t = fr.touching_blocks(1, 1, 1, 1)
    e = fr.edges(t, len(v))
    assert e.counts[4] == 1 and e.loop_edges.tolist() == [8] and fr.boundary_cycles(e) == [8, 72]
    f = fr.fill(e, t, len(v), v)
    assert f.counts == [2, 8, 0, 0] and fr.fill(e, t, len(v), v, 3).counts == [0, 0, 2, 0]
    members = fr.loop_members(e, e.loop_leader[0])
    a, b, _, _ = fr._ends(t, len(v))
    assert sorted(len(s) for s in fr.sub_loops_stack(members, a, b)) == [4, 4]
    assert sorted(map(sorted, fr.sub_loops_stack(members, a, b))) == sorted(map(sorted, fr.sub_loops_cut(members, a, b)))
    # a pinch that splits a 64-loop, and one edge more: no short loop
    v, t = fr.touching_blocks(8, 8, 8, 8)
    e = fr.edges(t, len(v))
    assert e.loop_edges.tolist() == [64] and fr.fill(e, t, len(v), v, 64).counts == [2, 64, 0, 0] and fr.fill(e, t, len(v), v, 31).counts == [0, 0, 2, 0]
    v, t = fr.touching_blocks(8, 8, 8, 9)
    e = fr.edges(t, len(v))
    assert e.counts[4] == 0 and e.counts[5] == e.counts[1] and 66 in fr.boundary_cycles(e)
    # disc fans: the rim is the loop
    for rim, short in ((3, True), (16, True), (17, True), (63, True), (64, True), (65, False)):
        nv, t = fr.disc_fan(rim)
        v = fr.ring_vertices(rim)
        e = fr.edges(t, nv)
        assert e.counts[:6] == [2 * rim, rim, 0, 0, int(short), 0 if short else rim] and (e.loop_edges.tolist() == [rim]) == short
        for max_edges in (16, 64):
            f = fr.fill(e, t, nv, v, max_edges)
            fills = short and rim <= max_edges
            assert f.counts == [int(fills), rim if fills else 0, int(short and not fills), 0]
    # NaN and infinity on a rim propagate to the new vertex; the normal is zeros
    nv, t = fr.disc_fan(5)
    v = fr.ring_vertices(5)
    v[2, 1], v[4, 0] = np.nan, np.inf
    f = fr.fill(fr.edges(t, nv), t, nv, v)
    assert np.isinf(f.vertices[0, 0]) and np.isnan(f.vertices[0, 1]) and f.vertices[0, 2] == 0.0 and f.normals.tolist() == [[0.0, 0.0, 0.0]]
    # a long rotation: 1,000 triangles about vertex 0 with one gap
    nv, t = fr.open_fan(1000)
    e = fr.edges(t, nv)
    assert e.counts[:6] == [2001, 1002, 0, 0, 0, 1002] and e.next[3 * 999 + 2] == 0 and fr.boundary_cycles(e) == [1002]


# ------------------------------------------------------------------------------------------- the README's table
# mesh -> vertices, triangles, edges (None: not in the table), boundary edges, the closed boundary cycles {edges: count}, loops
# that pass a vertex twice, filled sub-loops, fill triangles, boundary edges left
TABLE = {
    "sphere 8 cameras": (6943, 13776, 20763, 198, {4: 19, 6: 3, 16: 5, 24: 1}, 6, 46, 198, 0),
    "sphere 14 cameras, min_weight 2": (6988, 13792, None, 324, {4: 30, 6: 10, 16: 6, 24: 2}, 8, 72, 324, 0),
    "default (1, 1)": (11573, 22112, 33689, 1042, {8: 1, 10: 1, 14: 1, 16: 1, 22: 1, 34: 1, 44: 1, 212: 1, 220: 1, 462: 1}, 0, 4, 48, 994),
    "default (2, 2)": (8717, 16402, None, 1030, {4: 1, 6: 2, 48: 1, 80: 1, 176: 1, 290: 1, 420: 1}, 0, 3, 16, 1014),
}
VOLUMES = {"sphere 8 cameras": (4.2244, 4.2527), "sphere 14 cameras, min_weight 2": (4.2029, 4.2557)}


def table_mesh(name):
    return {"sphere 8 cameras": lambda: sphere_mesh(8, 1), "sphere 14 cameras, min_weight 2": lambda: sphere_mesh(14, 2),
            "default (1, 1)": lambda: cr.default_scene_mesh(1, 1), "default (2, 2)": lambda: cr.default_scene_mesh(2, 2)}[name]()


@pytest.mark.parametrize("name", sorted(TABLE))
def test_the_table(name):
    nv, nt, n_edges, n_boundary, cycles, twice, n_filled, n_fill_triangles, left = TABLE[name]
    m = table_mesh(name)
    assert (len(m.vertices), len(m.triangles)) == (nv, nt)
    e, f, (vv, nn, tt) = fr.fill_mesh(m.vertices, m.normals, m.triangles, 16)
    assert e.counts[1] == n_boundary and e.counts[2] == e.counts[3] == e.counts[6] == e.counts[7] == 0 and (n_edges is None or e.counts[0] == n_edges)
    assert dict(Counter(fr.boundary_cycles(e))) == cycles
    a, b, _, _ = fr._ends(m.triangles, nv)
    assert sum(len(fr.sub_loops_stack(fr.loop_members(e, l), a, b)) > 1 for l in e.loop_leader) == twice
    assert f.counts[:2] == [n_filled, n_fill_triangles] and (len(vv), len(tt)) == (nv + n_filled, nt + n_fill_triangles)
    after = fr.edges(tt, len(vv))
    assert after.counts[1] == left and after.counts[2] == after.counts[3] == 0
    assert vv[:nv].tobytes() == m.vertices.tobytes() and nn[:nv].tobytes() == m.normals.tobytes() and tt[:nt].tobytes() == m.triangles.tobytes()
    if name in VOLUMES:
        assert fr.is_closed(after) and mr.is_closed_and_oriented(tt) and fr.euler(tt, len(vv), after) == 2
        assert mr.euler_characteristic(len(vv), tt) == 2
        before, filled = VOLUMES[name]
        assert round(mr.signed_volume(m.vertices, m.triangles), 4) == before and round(mr.signed_volume(vv, tt), 4) == filled
        # the new normals point outwards like the sphere's
        assert (np.einsum("ij,ij->i", f.normals.astype(np.float64), f.vertices) > 0.9 * np.linalg.norm(f.vertices, axis=1)).all()


def test_the_closed_sphere_has_nothing_to_fill():
    m = sphere_mesh(14, 1)
    e, f, (vv, nn, tt) = fr.fill_mesh(m.vertices, m.normals, m.triangles)
    assert e.counts == [21012, 0, 0, 0, 0, 0, 0, 0] and f.counts == [0, 0, 0, 0] and tt.tobytes() == m.triangles.tobytes()
    assert round(mr.signed_volume(m.vertices, m.triangles), 4) == 4.2562


def test_nothing_depends_on_the_order():
    m = sphere_mesh(8, 1)
    nv = len(m.vertices)
    rng = np.random.default_rng(5)
    order = rng.permutation(len(m.triangles))
    turned = np.stack([np.roll(t, k) for t, k in zip(m.triangles[order], rng.integers(0, 3, len(order)))])
    a, b = fr.edges(m.triangles, nv), fr.edges(turned, nv)
    assert a.counts == b.counts and sorted(a.loop_edges.tolist()) == sorted(b.loop_edges.tolist())
    assert sorted(a.uses.tolist()) == sorted(b.uses.tolist())
    f, g = fr.fill(a, m.triangles, nv, m.vertices), fr.fill(b, turned, nv, m.vertices)
    assert f.counts == g.counts
    vv, nn, tt = fr.filled_mesh(m.vertices, m.normals, turned, g)
    after = fr.edges(tt, len(vv))
    assert fr.is_closed(after) and fr.euler(tt, len(vv), after) == 2


# ------------------------------------------------------------------------------------------- the headers on the host
def build_check(tmp_path, flags, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    cmd = ["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I" + os.path.join(ROOT, "sfm_amd", "csrc"), CHECK_SRC, "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return str(exe)


def patch_cases():
    """Loops of the meshes above that pass a vertex twice, a rim with a NaN, and long rims: (half-edges in next order, a, b, v)."""
    out = []
    for v, t in (fr.touching_blocks(1, 1, 1, 1), fr.touching_blocks(8, 8, 8, 8), fr.touching_blocks(3, 2, 1, 5)):
        e = fr.edges(t, len(v))
        a, b, _, _ = fr._ends(t, len(v))
        out += [(fr.loop_members(e, l), a, b, v) for l in e.loop_leader]
    m = sphere_mesh(8, 1)
    e = fr.edges(m.triangles, len(m.vertices))
    a, b, _, _ = fr._ends(m.triangles, len(m.vertices))
    out += [(fr.loop_members(e, l), a, b, m.vertices) for l in e.loop_leader]
    for rim in (3, 17, 64):
        nv, t = fr.disc_fan(rim)
        v = fr.ring_vertices(rim, 1e-3 * rim, 7.0) + np.random.default_rng(rim).normal(size=(rim + 1, 3))
        if rim == 17:
            v[5, 2] = np.nan
        e = fr.edges(t, nv)
        a, b, _, _ = fr._ends(t, nv)
        out.append((fr.loop_members(e, e.loop_leader[0]), a, b, v))
    return out


def run_check(exe, tmp_path):
    for args, least in ((["walk", "5"], 700), (["walk", "77"], 700), (["plan"], 600)):
        run = subprocess.run([exe, *args], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.startswith("ok "), (args, run.stdout, run.stderr[-2000:])
        assert int(run.stdout.split()[1]) > least
    # the centroids and the normals of the host build against the restatement, bit for bit
    n_sub = 0
    for i, (hs, a, b, v) in enumerate(patch_cases()):
        path = tmp_path / f"loop_{i}.txt"
        rows = [f"{h} {a[h]} " + " ".join(f"{int(x):016x}" for x in np.asarray(v[a[h]], np.float64).view(np.uint64)) for h in hs]
        path.write_text(f"{len(hs)}\n" + "\n".join(rows) + "\n")
        run = subprocess.run([exe, "patch", str(path)], capture_output=True, text=True)
        assert run.returncode == 0, (i, run.stderr[-2000:])
        subs = sorted((fr._from_name(s) for s in fr.sub_loops_stack(hs, a, b)), key=lambda s: s[0])
        lines = run.stdout.split("\n")[:-1]
        assert len(lines) == len(subs), (i, run.stdout)
        with np.errstate(all="ignore"):
            for line, sub in zip(lines, subs):
                c, nrm = fr._patch(sub, a, b, v, np.float64)
                want_c = fr.bits(np.array(c, np.float64))
                want_n = fr.bits(np.array(nrm, np.float64).astype(np.float32))
                got = line.split()
                got_c = fr.bits(np.array([int(x, 16) for x in got[2:5]], np.uint64).view(np.float64))
                got_n = fr.bits(np.array([int(x, 16) for x in got[5:8]], np.uint32).view(np.float32))
                assert [int(got[0]), int(got[1])] == [sub[0], len(sub)] and got_c.tolist() == want_c.tolist() and got_n.tolist() == want_n.tolist(), (i, line)
                n_sub += 1
    assert n_sub > 40


def test_rule_and_plan_on_the_host(tmp_path):
    """The stack against the cutting on random closed walks, the patch, the keys, the argument checks branch by branch, the
    layouts and the two-level scan of the packed counts around every seam; the patches bit for bit."""
    run_check(build_check(tmp_path, ["-O2"], "mesh_fill_check"), tmp_path)


def test_rule_and_plan_under_address_and_ub_sanitizers(tmp_path):
    """The same program built with -fsanitize=address,undefined and run stand-alone."""
    run_check(build_check(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
                          "mesh_fill_check_san"), tmp_path)


# ------------------------------------------------------------------------------------------- argument checks, no device
def test_argument_checks_without_gpu():
    import sfm_amd
    from sfm_amd import depth as dm
    from sfm_amd import mesh as mm
    from sfm_amd import mesh_fill as mf
    assert sfm_amd.MeshEdges is mf.MeshEdges and sfm_amd.fill_mesh_holes is mf.fill_mesh_holes and sfm_amd.mesh_edges is mm.mesh_edges
    assert sfm_amd.check_fill_arguments is mf.check_fill_arguments
    assert [p.default for p in list(inspect.signature(mm.Mesh.fill_holes).parameters.values())[1:]] == [16, None]
    assert [p.default for p in list(inspect.signature(mf.fill_mesh_holes).parameters.values())[2:]] == [None, 16, 0]
    assert [p.default for p in list(inspect.signature(mf.mesh_edges).parameters.values())[2:]] == [0]
    assert inspect.signature(dm.dense_from_reconstruction).parameters["fill_holes"].default is None
    check = mf.check_fill_arguments
    assert check() == (16, None, None, None, None) and check(1)[0] == 1 and check(np.int64(64))[0] == 64
    tri = [[0, 1, 2], [2, 1, 3]]
    got = check(8, None, tri, np.zeros((4, 3)), np.zeros((4, 3)))
    assert got[1] == 4 and got[2].dtype == np.int32 and got[2].shape == (2, 3) and got[3].dtype == np.float64 and got[4].dtype == np.float32
    for kw in (dict(max_edges=0), dict(max_edges=65), dict(max_edges=-1), dict(max_edges=16.0), dict(max_edges=True), dict(max_edges=None),
               dict(n_vertices=-1), dict(n_vertices=1 << 31), dict(triangles=[[0, 1]]), dict(triangles=[[0.0, 1.0, 2.0]]), dict(triangles=[[0, 1, 1 << 31]]),
               dict(vertices=np.zeros((4, 2))), dict(vertices=np.zeros((4, 3)), n_vertices=5), dict(vertices=np.zeros((4, 3)), normals=np.zeros((3, 3)))):
        with pytest.raises(ValueError):
            check(**kw)
    for call in (lambda: mf.fill_mesh_holes(None, tri), lambda: mf.fill_mesh_holes(np.zeros((4, 3)), tri, max_edges=0),
                 lambda: mf.fill_mesh_holes(np.zeros((4, 3)), tri, max_edges=65), lambda: mf.mesh_edges(tri, None), lambda: mf.mesh_edges(tri, -3),
                 lambda: mf.mesh_edges([[0, 1]], 4), lambda: dm.dense_from_reconstruction(None, [], fill_holes=16),
                 lambda: dm.dense_from_reconstruction(None, [], mesh=True, fill_holes=0), lambda: dm.dense_from_reconstruction(None, [], mesh=True, fill_holes=65)):
        with pytest.raises(ValueError):
            call()

    # a mesh and its edge table held on the host
    class Held:
        def __init__(self, a):
            self.a = a

        def cpu(self):
            return self

        def numpy(self):
            return self.a

    bare = mm.Mesh({}, 0, 0)
    assert bare.fill_vertex_start is None and bare.n_filled is None and bare.fill_triangle_halfedge is None and bare.edges_before is None
    for kw in (dict(max_edges=0), dict(max_edges=65), dict(max_edges="many")):
        with pytest.raises(ValueError):
            bare.fill_holes(**kw)
    v, t = fr.touching_blocks(1, 1, 1, 1)
    want = fr.edges(t, len(v))
    pad = lambda x: Held(np.r_[x, [9, 9, 9]].astype(np.int32))
    state = {"halfedge_uses": pad(want.uses), "halfedge_twin": pad(want.twin), "halfedge_next": pad(want.next), "halfedge_loop": pad(want.loop),
             "loop_leader": pad(want.loop_leader), "loop_edges": pad(want.loop_edges)}
    held = mf.MeshEdges(state, len(v), len(t), want.counts, lambda: t)
    assert (held.n_edges, held.n_boundary_edges, held.n_inconsistent_edges, held.n_nonmanifold_edges, held.n_loops, held.n_long_boundary_edges,
            held.n_unsound) == tuple(want.counts[:7])
    assert not held.is_closed and held.euler == fr.euler(t, len(v), want) and held.loop_edges.tolist() == [8] and held.halfedge_next.tobytes() == want.next.tobytes()
    closed = mf.MeshEdges({}, 4, 4, [6, 0, 0, 0, 0, 0, 0, 0], lambda: np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)]))
    assert closed.is_closed and closed.euler == 2
    assert not mf.MeshEdges({}, 4, 4, [6, 0, 0, 0, 0, 0, 1, 0]).is_closed and not mf.MeshEdges({}, 4, 4, [6, 0, 1, 0, 0, 0, 0, 0]).is_closed
    with pytest.raises(ValueError, match="this mesh"):
        mm.Mesh({}, 5, 3).fill_holes(edges=held)


def test_c_entry_points_reject_bad_calls_without_a_device():
    from sfm_amd import _lib
    lib = _lib.load()
    need = ctypes.c_int64(-1)
    big = (1 << 31) // 3
    assert lib.sfm_mesh_fill_workspace_bytes(0, ctypes.byref(need)) == 0 and 0 < need.value <= 4096
    assert lib.sfm_mesh_fill_workspace_bytes(100000, ctypes.byref(need)) == 0 and 2400000 <= need.value < 2500000
    assert lib.sfm_mesh_fill_workspace_bytes(big, ctypes.byref(need)) == 0 and need.value > 24 * big
    for n in (-1, big + 1):
        assert lib.sfm_mesh_fill_workspace_bytes(n, ctypes.byref(need)) == -1
    assert lib.sfm_mesh_fill_workspace_bytes(5, None) == -1
    # a null handle
    one = ctypes.c_void_p(1)
    assert lib.sfm_mesh_edges_workspace_bytes(None, 5, ctypes.byref(need)) == -1
    assert lib.sfm_mesh_edges(None, 0, 0, None, None, None, None, None, None, None, one, one, 4096) == -1
    assert lib.sfm_mesh_fill_mark(None, 0, 0, None, None, 0, None, 16, None, one, one, 4096) == -1
    assert lib.sfm_mesh_fill_emit(None, 0, 0, None, None, 0, None, None, None, 0, 0, None, None, None, None, None, one, 4096) == -1
