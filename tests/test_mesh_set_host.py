"""New meshes on the host (csrc/flat_meshes.h, flat_meshes.cpp): ctl_flat_bvh_update_meshes — the yardstick of ctl_scene_update_meshes —, the host re-statement of
k_append_leaf_rows and the acceptance rules both callers share.  Cases: tests/mesh_set_cases.py.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from cudatracerlib_amd import api
from flat_rebuild_cases import check_topology
from node_set_cases import NONE, entry_keys, tri_counts, old_of_new
from mesh_set_cases import CASES, descriptions, all_meshes_old_nodes, all_meshes_nodes_of_step, appended, check_case_shapes, soup

_cache = {}


def chain(case):
    """(the case's descriptions, the maps between consecutive ones, the handle built from the first and updated through all of them) — made once per case, never changed"""
    if case not in _cache:
        seq = descriptions(case)
        maps = [old_of_new(a, b) for a, b in zip(seq, seq[1:])]
        fb = api.FlatBvh(seq[0].desc)
        for s, m in zip(seq[1:], maps):
            fb.update_meshes(s.desc, m)
        _cache[case] = (seq, maps, fb)
    return _cache[case]


def tree_arrays(fb):
    """what `byte for byte` compares: nodes, leaves, part_index, level lists, depth"""
    start, nodes = fb.levels()
    part, boxes = fb.parts()
    return fb.nodes(), fb.leaves(), part, boxes, np.asarray(start), np.asarray(nodes), np.asarray(fb.desc.max_depth)


def same_trees(a, b, what):
    for k, (x, y) in enumerate(zip(tree_arrays(a), tree_arrays(b))):
        assert np.array_equal(x, y), "%s: array %d differs" % (what, k)


@pytest.mark.parametrize("case", CASES)
def test_case_shapes(case):
    check_case_shapes(case, chain(case)[0])


@pytest.mark.parametrize("case", CASES)
def test_entries_and_topology(case):
    """the updated tree is a valid one; its (triangle, node, split) keys are the kept keys plus every regular triangle of every added node exactly once"""
    seq, maps, upd = chain(case)
    check_topology(upd)
    fb = api.FlatBvh(seq[0].desc)
    for old, new, m in zip(seq, seq[1:], maps):
        was = entry_keys(fb)
        fb.update_meshes(new.desc, m)
        got = entry_keys(fb)
        added = np.nonzero(m == NONE)[0]
        new_of_old = np.full(old.desc.n_nodes, NONE, np.uint32); new_of_old[m[m != NONE]] = np.nonzero(m != NONE)[0]
        kept = was[new_of_old[was[:, 1]] != NONE].copy(); kept[:, 1] = new_of_old[kept[:, 1]]
        kept = kept[np.lexsort(kept.T[::-1])]
        assert np.array_equal(got[~np.isin(got[:, 1], added)], kept), "kept entries"
        nodes = new.desc.view("nodes", np.uint32, new.desc.n_nodes, 6)
        counts, first = tri_counts(new.desc), np.concatenate([[0], np.cumsum(tri_counts(new.desc))])
        M = new.desc.view("meshes", np.uint32, new.desc.n_meshes, 5)
        dg = new.desc.n_meshes - 1 if case in ("M3", "M6") and new is seq[-1] else None       # DG2, appended last
        for k in added:
            mesh = int(nodes[k, 0]); mine = got[got[:, 1] == k]
            t0 = int(M[mesh, 0])
            assert first[mesh] == t0, "meshes are laid out in index order"
            want = np.arange(t0, t0 + counts[mesh])
            if mesh == dg:
                want = np.delete(want, 2)                      # dg_mesh's third triangle has a singular Woop matrix
            assert (mine[:, 2] == 0).all() and np.array_equal(mine[:, 0], want), "node %d: one whole entry per regular triangle" % k
    same_trees(fb, upd, "replayed")


@pytest.mark.parametrize("case", ["M1", "M2", "M3", "M4", "M5"])
def test_independent_route(case):
    """A' holds every mesh of the new description but only the nodes of the old one, so ctl_flat_bvh_update_nodes — code that knows nothing of appended meshes — takes a
    tree freshly flattened from A' to the new description.  A' instances the same geometry under the same global triangle indices as the old description, so its fresh
    flatten is the old description's (asserted), and the two routes must agree byte for byte.  (M6: test_independent_route_two_calls.  M7 appends nothing:
    test_no_mesh_appended_is_update_nodes.)"""
    seq, maps, upd = chain(case)
    A = all_meshes_old_nodes(case)
    route = api.FlatBvh(A.desc)
    same_trees(route, api.FlatBvh(seq[0].desc), "A' flattens as the old description does")
    m = old_of_new(A, seq[1])
    assert np.array_equal(m, maps[0])
    route.update_nodes(seq[1].desc, m)
    same_trees(route, upd, "update_nodes from A' against update_meshes from the old description")


def test_independent_route_two_calls():
    """M6, whose second update_meshes starts from an updated handle with a refreshed basis and refreshed hashes.  The route that knows nothing of appended meshes: A0 holds
    every mesh of the last description under the ORIGINAL nodes — it flattens as the first description does (asserted) —, A1 the same meshes under the middle description's
    nodes; update_nodes takes the tree of A0 to A1 and on to the last description.  The result must equal the two chained update_meshes calls byte for byte"""
    seq, maps, upd = chain("M6")
    A0, A1 = all_meshes_nodes_of_step("M6", 0), all_meshes_nodes_of_step("M6", 1)
    assert A0.desc.n_meshes == A1.desc.n_meshes == seq[2].desc.n_meshes and A0.desc.n_nodes == seq[0].desc.n_nodes and A1.desc.n_nodes == seq[1].desc.n_nodes
    route = api.FlatBvh(A0.desc)
    same_trees(route, api.FlatBvh(seq[0].desc), "A0 flattens as the first description does")
    m01, m12 = old_of_new(A0, A1), old_of_new(A1, seq[2])
    assert np.array_equal(m01, maps[0]) and np.array_equal(m12, maps[1])
    route.update_nodes(A1.desc, m01)
    same_trees(route, api.FlatBvh(seq[0].desc).update_meshes(seq[1].desc, maps[0]), "after the first call")
    route.update_nodes(seq[2].desc, m12)
    same_trees(route, upd, "update_nodes twice from A0 against update_meshes twice from the first description")


@pytest.mark.parametrize("case", ["M2", "M3", "M6"])
def test_table_rule(case):
    """the host re-statement of the kernel's arithmetic over the appended rows: the table equals triangle_woop_rows(new), the rows equal creation's interleave"""
    seq = chain(case)[0]
    table = api.triangle_woop_rows(seq[0].desc)
    for old, new in zip(seq, seq[1:]):
        table, leaf = api.append_leaf_rows_host(new.desc, old.desc, table)
        assert np.array_equal(table, api.triangle_woop_rows(new.desc))
        w0, w1 = old.desc.n_woop, new.desc.n_woop
        woop = new.desc.view("woop", np.uint32, w1, 12)[w0:]; idx = new.desc.view("woop_index", np.uint32, w1, 1)[w0:]
        assert np.array_equal(leaf[:, :12], woop) and np.array_equal(leaf[:, 12], idx[:, 0]) and not leaf[:, 13:].any()
    counts = api.mesh_counts(seq[-1].desc)
    if case != "M2":
        long2 = seq[-1].desc.n_meshes - 2
        t0 = int(seq[-1].desc.view("meshes", np.uint32, seq[-1].desc.n_meshes, 5)[long2, 0])
        rows = table[t0:t0 + counts[long2][0]]
        assert len(np.unique(rows)) == len(rows) and (rows != NONE).all() and counts[long2][1] > len(rows), "several rows name one triangle; the table keeps one each"


def test_no_mesh_appended_is_update_nodes():
    seq, maps, upd = chain("M7")
    same_trees(upd, api.FlatBvh(seq[0].desc).update_nodes(seq[1].desc, maps[0]), "M7")


# ---- refusals

def refused(fb, desc, m, word=None, code=None, call="update_meshes"):
    before = [a.copy() if isinstance(a, np.ndarray) else a for a in tree_arrays(fb)]
    with pytest.raises(api.CtlError) as e:
        getattr(fb, call)(desc, m)
    assert e.value.code == (api.ERR_INVALID if code is None else code), str(e.value)
    if word:
        assert word in str(e.value), str(e.value)
    C_ = api.FlatBvhDesc(); api._check(api.lib.ctl_flat_bvh_arrays(fb._h, C.byref(C_))); fb.desc = C_
    for x, y in zip(tree_arrays(fb), before):
        assert np.array_equal(x, y), "a refusal changed the handle"


def test_refusals_on_the_yardstick():
    seq, maps, _ = chain("M2")
    old, new, m = seq[0], seq[1], maps[0]
    fb = api.FlatBvh(old.desc)
    n_old = old.desc.n_meshes
    copy = lambda: api.ctl_scene_desc.from_buffer_copy(new.desc)
    # a changed prefix mesh record
    d = copy(); M = new.desc.view("meshes", np.uint32, new.desc.n_meshes, 5).copy(); M[1, 4] += 1; d.meshes = M.ctypes.data
    refused(fb, d, m, "another record")
    # an appended mesh whose triangles lie inside the old range
    d = copy(); M = new.desc.view("meshes", np.uint32, new.desc.n_meshes, 5).copy(); M[n_old, 0] = old.desc.n_tri_data - 1; d.meshes = M.ctypes.data
    refused(fb, d, m, "not behind")
    # a gap between the held triangles and the first appended mesh: the elements in it would lengthen the last held mesh's range
    d = copy(); M = new.desc.view("meshes", np.uint32, new.desc.n_meshes, 5).copy(); M[n_old, 0] = old.desc.n_tri_data + 1; d.meshes = M.ctypes.data
    refused(fb, d, m, "belong to no appended mesh")
    # shrunken counts
    d = copy(); d.n_tri_data = old.desc.n_tri_data - 1
    refused(fb, d, m, "shorter")
    d = copy(); d.n_meshes = n_old - 1
    refused(fb, d, m, "not removed")
    # another image count
    d = copy(); d.n_images = new.desc.n_images + 1
    refused(fb, d, m, "images")
    # changed values of an old mesh
    d = copy(); woop = new.desc.view("woop", np.float32, new.desc.n_woop, 12).copy(); woop[0, 3] += 0.25; d.woop = woop.ctypes.data
    refused(fb, d, m, "ctl_scene_update first")
    # changed structure of the old part
    d = copy(); idx = new.desc.view("woop_index", np.uint32, new.desc.n_woop, 1).copy(); idx[0, 0] ^= 2; d.woop_index = idx.ctypes.data
    refused(fb, d, m, "structure")
    # a node that names a missing mesh
    d = copy(); nodes = new.desc.view("nodes", np.uint32, new.desc.n_nodes, 6).copy(); nodes[-1, 0] = new.desc.n_meshes; d.nodes = nodes.ctypes.data
    refused(fb, d, m, "missing mesh")
    # the map, as ctl_flat_bvh_update_nodes judges it
    assert api.lib.ctl_flat_bvh_update_meshes(fb._h, C.byref(new.desc), None, api.u32(len(m))) == api.ERR_INVALID
    refused(fb, new.desc, m[:-1], "elements")
    # Q8: unsupported, as for update_nodes
    refused(api.FlatBvh(old.desc, api.FLAT_Q8), new.desc, m, "Q4", api.ERR_UNSUPPORTED)
    # ctl_flat_bvh_update_nodes keeps its answer to appended meshes, word for word
    seq1, maps1, _ = chain("M1")
    fb1 = api.FlatBvh(seq1[0].desc)
    refused(fb1, seq1[1].desc, maps1[0], "the set of meshes differs: only meshes the scene already holds can be instanced; re-create the scene", call="update_nodes")
    # after all that the handles still take the change
    fb.update_meshes(new.desc, m); check_topology(fb)
    same_trees(fb, chain("M2")[2], "after the refusals")


def test_symbols_and_device_check():
    for name in ("ctl_scene_update_meshes", "ctl_scene_update_meshes_ex", "ctl_flat_bvh_update_meshes", "ctl_flat_bvh_update_meshes_ex"):
        assert hasattr(api.lib, name), name
    m = np.zeros(1, np.uint32)
    rc = api.lib.ctl_scene_update_meshes(None, None, m.ctypes.data, api.u32(1), None)
    assert rc == (api.ERR_NO_DEVICE if api.device_count() == 0 else api.ERR_INVALID)       # the device is checked first
    assert C.sizeof(api.ctl_scene_meshes_stats) == 24 + C.sizeof(api.ctl_scene_nodes_stats)
