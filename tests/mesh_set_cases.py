"""Scenes, edits and checks shared by tests/test_mesh_set_host.py and tests/test_gpu_mesh_set.py: NEW meshes on a live scene (csrc/flat_meshes.h,
ctl_scene_update_meshes / ctl_flat_bvh_update_meshes).

Every case edits node_set_cases.base(...) after its first UpdateScene(): further add_mesh calls append to the builder's arrays, CreateNode / DeleteNode change the node set.

    M1  append a 1-triangle mesh and one node of it
    M2  append meshes of 5, 64, 65 and 257 triangles (the wave and block edges of a one-lane-per-row kernel): T5 instanced twice, T64 never
    M3  append LONG2 — split_mesh(): its SBVH holds more rows than triangles (spatial splits: several rows name one triangle) — and DG2 (a singular Woop matrix: no entry)
    M4  M2's append together with N7's node edits (two old nodes deleted, instances of old meshes added)
    M5  append a mesh with two materials, a conductor and a diffuse; its node carries an area light
    M6  two calls: M1's append, then M3's on top
    M7  no mesh appended: N6's edit through the new entry point

A description points into its builder, so every description of a case comes from a builder of its own that replays the case's steps (descriptions(case)); node ids are
assigned in creation order and agree between them.  all_meshes_old_nodes(case) is the description A' of the independent route: every mesh of the last description, but
only the nodes of the one before it."""
import numpy as np

from cudatracerlib_amd import api
import node_set_cases as ns
from node_set_cases import soup, long_mesh, dg_mesh, place, base, old_of_new, NONE, LONG, T63      # noqa: F401

CASES = ["M%d" % k for k in range(1, 8)]
METAL = dict(eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), two_sided=True)


def big(k, scale=3.0):
    """place(k) enlarged: small meshes must show in a 32 x 32 frame"""
    X = place(k); X[:3, :3] *= scale
    return X


def two_sided(rgb):
    return [api.diffuse(rgb, two_sided=True)]


# ---- the steps: (add the meshes -> {name: mesh index}, add / remove the nodes)

def m1_meshes(sc):
    return {"A1": sc.add_mesh(*soup(1, 201), materials=two_sided((0.8, 0.3, 0.3)))}


def m1_nodes(sc, m, a):
    sc.CreateNode(a["A1"], big(17, 3.0))          # in the camera's view: a dozen of the frame's 1024 pixels see the triangle (counted with the oracle's primary rays)


def m2_meshes(sc):
    return {"A%d" % n: sc.add_mesh(*soup(n, 210 + k), materials=two_sided((0.3 + 0.1 * k, 0.6, 0.8 - 0.1 * k))) for k, n in enumerate((5, 64, 65, 257))}


def m2_nodes(sc, m, a):
    sc.CreateNode(a["A5"], big(17)); sc.CreateNode(a["A5"], big(18))
    sc.CreateNode(a["A65"], place(19)); sc.CreateNode(a["A257"], place(20))       # A64 has no node


def split_mesh():
    """27 small triangles and two long ones that cross the cube diagonally: the mesh's SBVH takes spatial splits, so its leaf stream holds more rows than the mesh has
    triangles (node_set_cases.long_mesh() does not: its long triangle is axis-aligned enough for an object split; check_case_shapes asserts the property)"""
    P, I = soup(27, 93, size=0.15)
    X = np.array([[-0.3, -0.2, -0.3], [2.3, 2.2, 2.3], [2.3, 2.3, 2.1], [-0.3, 2.2, -0.3], [2.3, -0.2, 2.3], [2.3, -0.3, 2.1]], np.float32)
    P = np.concatenate([P, X])
    return P, np.arange(len(P), dtype=np.uint32).reshape(-1, 3)


def m3_meshes(sc):
    return {"LONG2": sc.add_mesh(*split_mesh(), materials=two_sided((0.7, 0.6, 0.2))), "DG2": sc.add_mesh(*dg_mesh(), materials=two_sided((0.2, 0.7, 0.6)))}


def m3_nodes(sc, m, a):
    sc.CreateNode(a["LONG2"], place(21)); sc.CreateNode(a["DG2"], big(22))


def m4_nodes(sc, m, a):
    sc.DeleteNode(LONG); sc.DeleteNode(T63 - 1)              # N7's edit (T63 has moved down by one)
    sc.CreateNode(m["T63"], place(12)); sc.CreateNode(m["T257"], place(14))
    m2_nodes(sc, m, a)


def m5_meshes(sc):
    P, I = soup(12, 231, size=0.45)
    return {"A2M": sc.add_mesh(P, I, tri_material=np.arange(12) % 2, materials=[api.conductor(**METAL), api.diffuse((0.9, 0.9, 0.2), two_sided=True)])}


def m5_nodes(sc, m, a):
    node = sc.CreateNode(a["A2M"], big(17, 2.0))
    sc.CreateLight(node, 1, (30.0, 28.0, 20.0))


STEPS = {"M1": [(m1_meshes, m1_nodes)], "M2": [(m2_meshes, m2_nodes)], "M3": [(m3_meshes, m3_nodes)], "M4": [(m2_meshes, m4_nodes)], "M5": [(m5_meshes, m5_nodes)],
         "M6": [(m1_meshes, m1_nodes), (m3_meshes, m3_nodes)]}


def replay(case, n_steps, width=32, height=32, last_without_nodes=False, then=None, nodes_upto=None):
    """a builder of the base scene after the first n_steps steps of the case, every step closed by an UpdateScene(); nodes_upto: only the first so many steps edit the
    node set, the later ones add their meshes alone (last_without_nodes: n_steps - 1);
    then(sc, base meshes, the last step's meshes): further edits on the builder before the closing UpdateScene()"""
    if nodes_upto is None:
        nodes_upto = n_steps - 1 if last_without_nodes else n_steps
    sc, m = base("M", width, height)
    sc.UpdateScene()
    for i, (meshes, nodes) in enumerate(STEPS[case][:n_steps]):
        a = meshes(sc)
        if i < nodes_upto:
            nodes(sc, m, a)
        sc.UpdateScene()
    if then:
        then(sc, m, a)
    return ns.finish("", sc)


def descriptions(case, width=32, height=32):
    """the DynamicScenes of the case in call order: [old, new] — M6: [old, middle, new]"""
    if case == "M7":
        return [ns.old_scene("N6", width, height), ns.new_scene("N6", width, height)]
    return [replay(case, n, width, height) for n in range(len(STEPS[case]) + 1)]


def all_meshes_old_nodes(case, width=32, height=32):
    """A': the last description's meshes under the nodes of the description before it"""
    return replay(case, len(STEPS[case]), width, height, last_without_nodes=True)


def all_meshes_nodes_of_step(case, k, width=32, height=32):
    """every mesh of the case's last description under the nodes of its k-th description (0: the original nodes)"""
    return replay(case, len(STEPS[case]), width, height, nodes_upto=k)


def appended(old, new):
    """the mesh indices `new` appends to `old`"""
    return list(range(old.desc.n_meshes, new.desc.n_meshes))


def rows_exceed_triangles(desc, mesh):
    n_tri, n_rows = api.mesh_counts(desc)[mesh]
    return n_rows > n_tri


def check_case_shapes(case, seq):
    """what the cases promise about their meshes, asserted on the CPU"""
    old, new = seq[0], seq[-1]
    counts = api.mesh_counts(new.desc)
    sizes = [counts[k][0] for k in appended(old, new)]
    want = {"M1": [1], "M2": [5, 64, 65, 257], "M3": [29, 5], "M4": [5, 64, 65, 257], "M5": [12], "M6": [1, 29, 5], "M7": []}[case]
    assert sizes == want, (case, sizes)
    if case in ("M3", "M6"):
        long2 = new.desc.n_meshes - 2
        assert rows_exceed_triangles(new.desc, long2), "LONG2's row range does not exceed its triangle count: the table rule has no duplicate to order"
    if case in ("M2", "M4"):
        nodes = new.desc.view("nodes", np.uint32, new.desc.n_nodes, 6)
        a = appended(old, new)
        assert (nodes[:, 0] == a[0]).sum() == 2 and (nodes[:, 0] == a[1]).sum() == 0, "T5 twice, T64 never"
