"""Scenes, edits and checks shared by tests/test_node_set_host.py and tests/test_gpu_node_set.py: another SET of nodes on a live scene (csrc/flat_nodes.h,
ctl_scene_update_nodes / ctl_flat_bvh_update_nodes).

The base scene: a floor, a point light, and one node each of meshes of 1, 4, 5, 63, 64, 65 and 257 triangles — the wave and leaf-slot boundaries of the drop, generate
and collapse stages —, of LONG (one long triangle among small ones: creation gives it split references) and of DG (five triangles, one degenerate).  Every builder
holds all meshes, whichever it instances.  No two instances share a transform and no two surfaces coincide (random triangle soups at distinct places), so hit ties cannot
depend on the order of a tree; build() asserts the distinct transforms.

    N1  remove the first node                  N6  add two instances of one mesh with different materials
    N2  remove the last node                   N7  add and remove in one call
    N3  remove LONG's node (middle)            N8  add an instance of DG
    N4  remove all but T1's node               N9  N7 + a kept node moved, a kept material edited, the camera changed
    N5  add one instance to a one-node scene   N10 the identity map

As in scene_update_cases.py a description points into its builder, so the old and the new description of a case come from two builders that build the same base:
old_scene(case) and new_scene(case) (= the base + the case's edit).  Node ids are assigned in creation order, so they agree between the two; the map is computed from
them (old_of_new), never written by hand."""
import ctypes as C

import numpy as np

from cudatracerlib_amd import api, scenes
from scene_update_cases import node_transforms, with_materials

CASES = ["N%d" % k for k in range(1, 11)]
SIZES = (1, 4, 5, 63, 64, 65, 257)
NONE = 0xffffffff
# node order of the base scene
FLOOR, T1, T4, LONG, T5, T63, T64, DG, T65, T257 = range(10)
BASE_NODES = ("floor", "T1", "T4", "LONG", "T5", "T63", "T64", "DG", "T65", "T257")


def soup(n, seed, size=0.35, extent=2.0):
    """n triangles of about `size` at jittered lattice places inside a cube of `extent`: (positions (3 n, 3), indices (n, 3))"""
    rs = np.random.RandomState(seed)
    side = int(np.ceil(n ** (1.0 / 3.0)))
    cells = np.array([(x, y, z) for x in range(side) for y in range(side) for z in range(side)], np.float64)[rs.permutation(side ** 3)[:n]]
    centre = (cells + 0.5 + rs.uniform(-0.2, 0.2, size=(n, 3))) * (extent / side)
    P = centre[:, None, :] + rs.uniform(-size, size, size=(n, 3, 3)) * (extent / side)
    return P.reshape(-1, 3).astype(np.float32), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def long_mesh():
    """eleven small triangles and one that spans the scene"""
    P, I = soup(11, 91)
    P = np.concatenate([P, np.array([[-7.5, 0.9, -0.3], [7.5, 1.1, 0.1], [7.4, 1.3, 0.5]], np.float32)])
    return P, np.arange(len(P), dtype=np.uint32).reshape(-1, 3)


def dg_mesh():
    """five triangles; the third has two equal vertices (a singular Woop matrix: no leaf entry)"""
    P, I = soup(5, 92)
    P[7] = P[6]
    return P, I


def place(k):
    """the transform of the k-th placed instance: distinct translations, a different scale and turn each"""
    a = 0.37 * k
    X = np.eye(4, dtype=np.float64)
    X[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) * (0.8 + 0.05 * k)
    X[:3, 3] = (-5.0 + 2.4 * (k % 5), 0.3 + 0.9 * (k // 5), -3.0 + 2.9 * ((k // 5) % 3) + 0.2 * k)
    return X.astype(np.float32)


def base(case, width=32, height=32, skip=None):
    """the builder of the case's base scene, before UpdateScene(): (DynamicScene, {name: mesh index}); skip: a node of the base scene that is never created"""
    sc = api.DynamicScene()
    P, I, N = scenes._quad([[-9, 0, -9], [-9, 0, 9], [9, 0, 9], [9, 0, -9]], [0, 1, 0])
    m = {"floor": sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.6, 0.6, 0.6))])}
    for k, n in enumerate(SIZES):
        m["T%d" % n] = sc.add_mesh(*soup(n, 11 + k), materials=[api.diffuse((0.3 + 0.08 * k, 0.5, 0.7 - 0.06 * k), two_sided=True)])
    m["LONG"] = sc.add_mesh(*long_mesh(), materials=[api.diffuse((0.7, 0.4, 0.3), two_sided=True)])
    m["DG"] = sc.add_mesh(*dg_mesh(), materials=[api.diffuse((0.4, 0.7, 0.3), two_sided=True)])
    if case == "N5":
        sc.CreateNode(m["T5"], place(1))
    else:
        for k, name in enumerate(BASE_NODES):
            if k == skip:
                continue
            sc.CreateNode(m[name], None if name == "floor" else place(k))
    sc.CreatePointLight((1, 9, -2), (90, 90, 90))
    sc.setCamera((0.5, 5.5, -13.0), (0, 1.2, 0), (0, 1, 0), 55.0, width, height)
    return sc, m


def edit(case, sc, m, width=32, height=32):
    """the case's change of the node set on a builder of base(case)"""
    if case == "N1":
        sc.DeleteNode(FLOOR)
    elif case == "N2":
        sc.DeleteNode(T257)
    elif case == "N3":
        sc.DeleteNode(LONG)
    elif case == "N4":
        for k in (T257, T65, DG, T64, T63, T5, LONG, T4, FLOOR):
            sc.DeleteNode(k)
    elif case == "N5":
        sc.CreateNode(m["T64"], place(12))
    elif case == "N6":
        sc.CreateNode(m["T65"], place(11)); sc.CreateNode(m["T65"], place(13))
    elif case in ("N7", "N9"):
        sc.DeleteNode(LONG); sc.DeleteNode(T63 - 1)            # (T63 has moved down by one)
        sc.CreateNode(m["T63"], place(12)); sc.CreateNode(m["T257"], place(14))
        if case == "N9":
            sc.SetNodeTransform(T4, place(16))
            sc.setCamera((3.0, 6.5, -12.0), (0.5, 1.0, 0.5), (0, 1, 0), 50.0, width, height)
    elif case == "N8":
        X = place(12); X[:3, :3] *= 3.0                        # large enough to show in a 32 x 32 frame
        sc.CreateNode(m["DG"], X)
    elif case != "N10":
        raise ValueError(case)


def finish(case, sc):
    """UpdateScene() and what is edited on the description itself: N6 gives the two added nodes other materials, N9 edits a kept node's material (a metal instead of
    a diffuse: another BSDF model, so the entries' model bits must follow)"""
    d = sc.UpdateScene()
    nodes = d.view("nodes", np.uint32, d.n_nodes, 6)
    if case in ("N6", "N9"):
        targets = [(d.n_nodes - 2, api.conductor(eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), two_sided=True)), (d.n_nodes - 1, api.diffuse((0.9, 0.2, 0.2), two_sided=True))] if case == "N6" else \
                  [(T1, api.conductor(eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), two_sided=True))]
        offsets = [(int(nodes[k, 1]), mat) for k, mat in targets]

        def change(mats):
            for o, mat in offsets:
                mats[o] = mat
        ids = d.node_ids
        d = with_materials(d, change); d.node_ids = ids
        sc.desc = d
    X = node_transforms(sc.desc).reshape(sc.desc.n_nodes, -1)
    assert len(np.unique(X, axis=0)) == sc.desc.n_nodes, "two instances share a transform"
    return sc


def old_scene(case, width=32, height=32):
    sc, _ = base(case, width, height)
    return finish("", sc)


def new_scene(case, width=32, height=32):
    sc, m = base(case, width, height)
    edit(case, sc, m, width, height)
    return finish(case, sc)


def undone_scene(width=32, height=32):
    """N7 and then its undoing on the same builder: the two added nodes removed, LONG's and T63's nodes created again at their places (now the last two nodes; the
    material table has grown twice).  Returns (scene, per node its index in the base scene)"""
    sc, m = base("N7", width, height)
    edit("N7", sc, m, width, height)
    sc.DeleteNode(9); sc.DeleteNode(8)
    sc.CreateNode(m["LONG"], place(LONG)); sc.CreateNode(m["T63"], place(T63))
    return finish("", sc), np.array([0, 1, 2, 4, 6, 7, 8, 9, LONG, T63])


def old_of_new(old, new):
    """the node map from the stable ids the two descriptions carry"""
    index = {i: k for k, i in enumerate(old.desc.node_ids)}
    return np.array([index.get(i, NONE) for i in new.desc.node_ids], np.uint32)


def tri_counts(desc):
    """triangles per mesh"""
    return [n for n, _ in api.mesh_counts(desc)]


def entry_keys(fb):
    """(triangle, node, is a split reference) per entry, sorted"""
    L = fb.leaves(); part, _ = fb.parts()
    rows = np.stack([L[:, 12] >> 1, L[:, 13], (part != NONE).astype(np.uint32)], axis=1)
    return rows[np.lexsort(rows.T[::-1])]
