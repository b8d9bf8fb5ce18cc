"""Scenes, edits and checks shared by tests/test_mesh_removal_host.py and tests/test_gpu_mesh_removal.py: meshes REMOVED from a live scene (csrc/flat_mesh_set.h,
ctl_builder_remove_mesh, ctl_scene_update_mesh_set / ctl_flat_bvh_update_mesh_set).

Every case starts from node_set_cases.base(...): the floor, soups of 1, 4, 5, 63, 64, 65 and 257 triangles, LONG and DG — in MESH order floor, T1, T4, T5, T63, T64, T65,
T257, LONG, DG (mesh_index()), in NODE order floor, T1, T4, LONG, T5, T63, T64, DG, T65, T257.

    R1  the last mesh (DG) removed: every delta is zero, the arrays only shrink
    R2  the first mesh (the floor) removed: every kept range moves, every rebase is non-zero
    R3  LONG and T64 removed: two holes, three runs, a kept mesh (T65, T257) between the holes
    R4  T5 removed and two meshes appended in the same call: LONG2 (mesh_set_cases.split_mesh: more rows than triangles) with a node, A64 without one
    R5  the old scene holds LONG2, appended without a node, and A5 with one behind it; LONG2 is removed with an identity node map: no entry drops, A5's triangle
        words rebase by a triangle delta that differs from its row delta
    R6  every mesh but T65 removed
    R7  nothing removed: node_set_cases N6's node edit, and mesh_set_cases M2's append
    R8  R3, then the floor removed from the result: offsets compacted twice

long_mesh() has no more rows than triangles (its long triangle gets an object split), so R3 alone does not tell the row delta from the triangle delta; R4 and R5 do, with
split_mesh(): check_case_shapes asserts where the two deltas differ.

A description points into its builder, so every description of a case comes from a builder of its own that replays the case's steps.  A step is (edit, removals): `edit`
changes nodes and appends meshes, `removals` calls RemoveMesh.  chain(case) gives per step (the description before, the description after `edit` alone — every held mesh
still there: what ctl_flat_bvh_update_nodes / _update_meshes, code that knows nothing of removal, can reach —, the description after the removals too)."""
import numpy as np

from cudatracerlib_amd import api
import node_set_cases as ns
from node_set_cases import soup, place, base, NONE, FLOOR, T1, T4, LONG, T5, T63, T64, DG, T65, T257      # noqa: F401
from mesh_set_cases import split_mesh, big, two_sided

CASES = ["R1", "R2", "R3", "R4", "R5", "R6", "R8"]       # (R7 removes nothing: its own tests)
MESH_ORDER = ("floor", "T1", "T4", "T5", "T63", "T64", "T65", "T257", "LONG", "DG")


def delete_nodes(sc, names):
    """DeleteNode of base-scene nodes by name, from the back so that the indices in front stay"""
    for k in sorted((ns.BASE_NODES.index(n) for n in names), reverse=True):
        sc.DeleteNode(k)


def remove_meshes(sc, m, names):
    for i in sorted((m[n] for n in names), reverse=True):
        sc.RemoveMesh(i)


def r4_append(sc, m):
    delete_nodes(sc, ["T5"])
    a = sc.add_mesh(*split_mesh(), materials=two_sided((0.7, 0.6, 0.2)))
    sc.add_mesh(*soup(64, 240), materials=two_sided((0.3, 0.3, 0.8)))
    sc.CreateNode(a, place(21))


def r5_setup(sc, m):
    m["LONG2"] = sc.add_mesh(*split_mesh(), materials=two_sided((0.7, 0.6, 0.2)))
    m["A5"] = sc.add_mesh(*soup(5, 241), materials=two_sided((0.8, 0.3, 0.3)))
    sc.CreateNode(m["A5"], big(17))


ALL_BUT_T65 = [n for n in MESH_ORDER if n != "T65"]
# case -> (setup of the OLD scene on top of base, or None; the steps)
STEPS = {
    "R1": (None, [(lambda sc, m: delete_nodes(sc, ["DG"]), lambda sc, m: remove_meshes(sc, m, ["DG"]))]),
    "R2": (None, [(lambda sc, m: delete_nodes(sc, ["floor"]), lambda sc, m: remove_meshes(sc, m, ["floor"]))]),
    "R3": (None, [(lambda sc, m: delete_nodes(sc, ["LONG", "T64"]), lambda sc, m: remove_meshes(sc, m, ["LONG", "T64"]))]),
    "R4": (None, [(r4_append, lambda sc, m: remove_meshes(sc, m, ["T5"]))]),
    "R5": (r5_setup, [(lambda sc, m: None, lambda sc, m: remove_meshes(sc, m, ["LONG2"]))]),
    "R6": (None, [(lambda sc, m: delete_nodes(sc, ALL_BUT_T65), lambda sc, m: remove_meshes(sc, m, ALL_BUT_T65))]),
    "R8": (None, [(lambda sc, m: delete_nodes(sc, ["LONG", "T64"]), lambda sc, m: remove_meshes(sc, m, ["LONG", "T64"])),
                  (lambda sc, m: sc.DeleteNode(0), lambda sc, m: sc.RemoveMesh(0))]),
}


def replay(case, n_steps, width=32, height=32, last_without_removal=False, then=None):
    """a builder of the case's old scene after the first n_steps steps, every step closed by an UpdateScene(); last_without_removal: the last step's edit alone"""
    setup, steps = STEPS[case]
    sc, m = base("R", width, height)
    m = dict(m)
    if setup:
        setup(sc, m)
    sc.UpdateScene()
    for i, (edit, removals) in enumerate(steps[:n_steps]):
        edit(sc, m)
        if not (last_without_removal and i == n_steps - 1):
            removals(sc, m)
        sc.UpdateScene()
    if then:
        then(sc, m)
    return ns.finish("", sc)


def chain(case, width=32, height=32):
    """[(before, after the edit alone, after the removals too)] per step"""
    n = len(STEPS[case][1])
    return [(replay(case, k, width, height), replay(case, k + 1, width, height, last_without_removal=True), replay(case, k + 1, width, height)) for k in range(n)]


def mesh_map(old, new):
    """the mesh map from the stable ids the two descriptions carry"""
    index = {i: k for k, i in enumerate(old.desc.mesh_ids)}
    return np.array([index.get(i, NONE) for i in new.desc.mesh_ids], np.uint32)


def mesh_table(desc):
    return desc.view("meshes", np.uint32, desc.n_meshes, 5)


def removed_in_front(old_desc, mm):
    """numpy, from the counts alone: per OLD mesh (triangles, rows) of the removed meshes in front of it; per old mesh whether it is kept"""
    counts = np.array(api.mesh_counts(old_desc), np.int64).reshape(-1, 2)
    kept = np.zeros(old_desc.n_meshes, bool); kept[mm[mm != NONE]] = True
    gone = np.where(kept[:, None], 0, counts)
    return np.concatenate([[[0, 0]], np.cumsum(gone, axis=0)[:-1]]), kept


def without_meshes(skip, width=32, height=32):
    """node_set_cases.base restated without the meshes (and their nodes) named in `skip`: the scene that never added them"""
    from cudatracerlib_amd import scenes
    sc = api.DynamicScene()
    m = {}
    if "floor" not in skip:
        P, I, N = scenes._quad([[-9, 0, -9], [-9, 0, 9], [9, 0, 9], [9, 0, -9]], [0, 1, 0])
        m["floor"] = sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.6, 0.6, 0.6))])
    for k, n in enumerate(ns.SIZES):
        if "T%d" % n not in skip:
            m["T%d" % n] = sc.add_mesh(*soup(n, 11 + k), materials=[api.diffuse((0.3 + 0.08 * k, 0.5, 0.7 - 0.06 * k), two_sided=True)])
    if "LONG" not in skip:
        m["LONG"] = sc.add_mesh(*ns.long_mesh(), materials=[api.diffuse((0.7, 0.4, 0.3), two_sided=True)])
    if "DG" not in skip:
        m["DG"] = sc.add_mesh(*ns.dg_mesh(), materials=[api.diffuse((0.4, 0.7, 0.3), two_sided=True)])
    for k, name in enumerate(ns.BASE_NODES):
        if name in m:
            sc.CreateNode(m[name], None if name == "floor" else place(k))
    sc.CreatePointLight((1, 9, -2), (90, 90, 90))
    sc.setCamera((0.5, 5.5, -13.0), (0, 1.2, 0), (0, 1, 0), 55.0, width, height)
    return ns.finish("", sc)


GEOMETRY = (("tri_data", "n_tri_data", 8), ("woop", "n_woop", 12), ("woop_index", "n_woop", 1), ("bvh_nodes", "n_bvh_nodes", 16))


def geometry_arrays(desc):
    return [desc.view(name, np.uint32, getattr(desc, count), words) for name, count, words in GEOMETRY]


def check_case_shapes(case, steps):
    """what the cases promise, asserted on the CPU"""
    old, mid, new = steps[0]
    mm = mesh_map(old, new)
    front, kept = removed_in_front(old.desc, mm)
    n_removed = {"R1": 1, "R2": 1, "R3": 2, "R4": 1, "R5": 1, "R6": 9, "R8": 2}[case]
    assert (~kept).sum() == n_removed and (mm == NONE).sum() == (2 if case == "R4" else 0)
    if case == "R1":
        assert not front[kept].any(), "the last mesh: every delta zero"
    if case == "R2":
        assert front[kept].all(), "the first mesh: every rebase non-zero"
    if case in ("R3", "R8"):
        holes = np.nonzero(~kept)[0]
        assert len(holes) == 2 and holes[1] - holes[0] > 1 and holes[0] > 0 and holes[1] < old.desc.n_meshes - 1, "two holes, three runs, a kept mesh between"
    if case in ("R4", "R5"):
        counts = api.mesh_counts(new.desc if case == "R4" else old.desc)
        long2 = new.desc.n_meshes - 2 if case == "R4" else old.desc.n_meshes - 2
        assert counts[long2][1] > counts[long2][0], "split_mesh: more rows than triangles"
    if case == "R5":
        assert front[-1, 0] != front[-1, 1] and kept[-1], "behind LONG2 the row delta differs from the triangle delta"
        assert np.array_equal(ns.old_of_new(old, new), np.arange(old.desc.n_nodes)), "an identity node map"
    if case == "R6":
        assert new.desc.n_meshes == 1 and new.desc.n_nodes == 1
