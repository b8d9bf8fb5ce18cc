"""Scenes, poses and checks shared by tests/test_flat_rebuild_host.py and tests/test_gpu_flat_rebuild.py: the rebuild of the flattened Q4 tree
(csrc/flat_rebuild.h).  On top of S1 / S2 / S3 and M1..M3 of tests/scene_update_cases.py:

M4     every instance node of S1 moved to another instance's place: the worst case of a refitted tree
T1 T4 T5   scenes of 1, 4 and 5 triangles: a root with one leaf slot, and the first split
TW     two instances of one mesh under the SAME transform (every Morton code appears twice) over a floor
S3D3   S3 with its ball collapsed by D3 of tests/scene_deform_cases.py (entries with singular Woop rows: inverted boxes)
BIG    synthetic_sm with 260 instances: just above 2^16 leaf entries, so the sort and the scans leave their single-workgroup paths

As in scene_update_cases.py every description comes from a builder of its own: old_scene(case) is what the tree is built from, new_scene(case, pose) the pose it is
rebuilt for (pose None: the scene as built)."""
import numpy as np

from cudatracerlib_amd import api, scenes
from scene_update_cases import build, motion_of, node_transforms
from scene_deform_cases import deform, build_deformed_and_moved

POSES = {"S1": (None, "M1", "M2", "M3", "M4"), "S2": (None, "M2", "M3"), "S3": (None, "M2", "M3"), "T1": (None, "MV"), "T4": (None, "MV"), "T5": (None, "MV"),
         "TW": (None, "MV"), "S3D3": (None, "M3"), "BIG": (None, "M3")}
CASES = [(c, p) for c, poses in POSES.items() for p in poses]
IDS = ["%s-%s" % (c, p or "built") for c, p in CASES]
N_S1_INSTANCES = 60


def m4(sc):
    X = node_transforms(sc.desc)
    for k in range(N_S1_INSTANCES):
        Y = X[k].copy(); Y[:3, 3] = X[(k + 17) % N_S1_INSTANCES][:3, 3]
        sc.SetNodeTransform(k, Y.astype(np.float32))


def _tiny(n_tri, pose, width, height):
    sc = api.DynamicScene()
    rs = np.random.RandomState(7 + n_tri)
    P = np.concatenate([np.array([[0, 0, 0], [1, 0, 0.2], [0.3, 1, 0]]) + np.array([1.7 * k, 0.4 * (k % 2), 0.9 * k]) + rs.uniform(-0.1, 0.1, size=(3, 3)) for k in range(n_tri)]).astype(np.float32)
    I = np.arange(3 * n_tri, dtype=np.uint32).reshape(-1, 3)
    node = sc.CreateNode(sc.add_mesh(P, I, materials=[api.diffuse((0.6, 0.5, 0.4), two_sided=True)]))
    if pose:
        xf = np.eye(4, dtype=np.float32); xf[:3, 3] = (0.8, -0.5, 2.0); xf[0, 0] = 1.5
        sc.SetNodeTransform(node, xf)
    sc.CreatePointLight((2, 6, -3), (40, 40, 40))
    sc.setCamera((3, 2, -9), (3, 0.5, 2), (0, 1, 0), 50.0, width, height)
    sc.UpdateScene()
    return sc


def _twins(pose, width, height):
    sc = api.DynamicScene()
    P, I, N = scenes._quad([[-6, 0, -6], [-6, 0, 6], [6, 0, 6], [6, 0, -6]], [0, 1, 0])
    sc.CreateNode(sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.6, 0.6, 0.6))]))
    V, F = scenes.icosphere(1)
    ball = sc.add_mesh(V, F, normals=V, materials=[api.diffuse((0.3, 0.5, 0.7))])
    xf = np.eye(4, dtype=np.float32); xf[:3, :3] *= 1.7; xf[:3, 3] = (1.0, 2.0, 0.5)
    a, b = sc.CreateNode(ball, xf), sc.CreateNode(ball, xf)
    if pose:
        xf = xf.copy(); xf[:3, 3] = (-2.5, 3.0, -1.0); xf[1, 1] = 2.4
        sc.SetNodeTransform(a, xf); sc.SetNodeTransform(b, xf)
    sc.CreatePointLight((0, 9, 0), (60, 60, 60))
    sc.setCamera((0, 4, -11.5), (0, 2, 0), (0, 1, 0), 60.0, width, height)
    sc.UpdateScene()
    return sc


def _big(pose, width, height):
    sc = scenes.synthetic_sm(width, height, n_instances=260, subdiv=2)
    if pose:
        for node, xf in motion_of("S1", pose, sc.desc).items():
            sc.SetNodeTransform(node, xf)
        sc.UpdateScene()
    return sc


def new_scene(case, pose=None, width=32, height=32):
    if case in ("S1", "S2", "S3"):
        return build(case, width=width, height=height, edit=m4) if pose == "M4" else build(case, pose, width=width, height=height)
    if case in ("T1", "T4", "T5"):
        return _tiny(int(case[1]), pose, width, height)
    if case == "TW":
        return _twins(pose, width, height)
    if case == "S3D3":
        return build_deformed_and_moved("D3", "S3", pose, width, height) if pose else build("S3", width=width, height=height, edit=deform("D3", "S3"))
    if case == "BIG":
        return _big(pose, width, height)
    raise ValueError(case)


def old_scene(case, width=32, height=32):
    return build("S3", width=width, height=height) if case == "S3D3" else new_scene(case, None, width, height)


def moved_nodes(old, new):
    return [k for k in range(new.n_nodes) if not np.array_equal(node_transforms(new)[k], node_transforms(old)[k])]


def check_topology(fb):
    """What the traversal kernel needs of a REBUILT tree, decoded from the node words alone with the formula of csrc/flatten.h (FlatBvh.implied_links):
    every node and every entry is reached exactly once; walking level by level, node by node, slot by slot meets the nodes 0, 1, 2 .. and the entries 0, 1, 2 .. in
    that order — so inner children are consecutive nodes, the entries of leaf children consecutive entries, and every level an index range; leaves hold 1 to 4
    entries and only their last entry carries the closing bit; no node carries a slab; the depth is max_depth and the level lists say the same.  Returns level_start."""
    N, L = fb.nodes(), fb.leaves()
    n_nodes, n_entries = len(N), len(L)
    assert N.shape[1] == 16 and fb.desc.compact == 1 and fb.desc.root_slab == 0 and fb.desc.n_slab_nodes == 0
    assert (N[:, 12:16] == 0).all(), "a rebuilt node carries something in its last 16 B"
    imp = api.FlatBvh.implied_links(N)
    exist = (N[:, 3] >> 24) & 15; leafm = (N[:, 3] >> 28) & exist
    last = (L[:, 12] & 1) == 1
    level, level_start, next_node, next_entry = [0], [0, 1], 1, 0
    while level:
        nxt = []
        for i in level:
            assert exist[i] != 0 and (exist[i] & (exist[i] + 1)) == 0, "slots are filled from slot 0"
            for c in range(4):
                if not (exist[i] >> c) & 1:
                    continue
                link = int(imp[i, c])
                if (leafm[i] >> c) & 1:
                    e = ~link
                    assert e == next_entry, "node %d slot %d: leaf entries out of order (%d, expected %d)" % (i, c, e, next_entry)
                    k = 1
                    while not last[e + k - 1]:
                        k += 1
                        assert k <= 4 and e + k <= n_entries, "a leaf of more than four entries"
                    next_entry = e + k
                else:
                    assert link >= 0 and link % 4 == 0, "an inner link with a slab flag"
                    assert link // 4 == next_node and next_node < n_nodes, "node %d slot %d: inner children out of order" % (i, c)
                    nxt.append(next_node); next_node += 1
        level = nxt
        level_start.append(next_node)
    level_start.pop()   # the empty level that ended the walk
    assert next_node == n_nodes and next_entry == n_entries, "not every node / entry is reached"
    # (each leaf's closing bit sits on its last entry and nowhere else: the walk above consumed exactly n_entries entries in runs that each end at a closing bit)
    assert last[-1]
    depth = len(level_start) - 2
    assert depth == fb.desc.max_depth, "max_depth %d, the tree has %d" % (fb.desc.max_depth, depth)
    # the explicit links host code sees are the implied ones; a slot without a child leads somewhere harmless (csrc/flatten.cpp patch_empty_slots_q4): to the node's
    # first entry in a node of leaves only (leaf bit without the exists bit), else to its first inner child.  (test_oracle_flat.check_implied_links holds a BUILT
    # tree to the same, and to carrying slabs, which a rebuilt tree does not.)
    ch = fb.child_links()
    innerm = exist & ~leafm
    for c in range(4):
        has = ((exist >> c) & 1) == 1
        assert np.array_equal(imp[has, c], ch[has, c]) and (ch[~has, c] == 0x76543210).all()
        if c:
            all_leaves = ~has & (innerm == 0)
            assert (((N[all_leaves, 3] >> (28 + c)) & 1) == 1).all() and np.array_equal(imp[all_leaves, c], ch[all_leaves, 0])
            some_inner = ~has & (innerm != 0)
            assert (((N[some_inner, 3] >> (28 + c)) & 1) == 0).all() and not some_inner.any()   # a node with an inner child has four slots
    ls, ln = fb.levels()
    assert np.array_equal(ls, np.array(level_start, np.uint32)) and np.array_equal(ln, np.arange(n_nodes, dtype=np.uint32))
    return level_start


def entry_rows(fb):
    """the entries with bit 0 of the index word masked, paired with their part_index, sorted: the multiset a rebuild must keep"""
    L = fb.leaves().copy(); L[:, 12] &= ~np.uint32(1)
    part_index, _ = fb.parts()
    rows = np.concatenate([L, part_index[:, None].astype(np.uint32)], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def node_area(fb):
    """summed surface area of the boxes around the nodes' decoded child boxes (csrc/flat_refit.h refit_node_area)"""
    from scene_update_cases import decode_q4
    lo, hi, exist, _ = decode_q4(fb.nodes())
    has = (((exist[:, None] >> np.arange(4)[None, :]) & 1) == 1)[..., None]
    d = np.where(has, hi, -np.inf).max(axis=1) - np.where(has, lo, np.inf).min(axis=1)
    return float((2.0 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0])).sum())
