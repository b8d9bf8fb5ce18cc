"""Removed meshes on the host (csrc/flat_mesh_set.h, flat_mesh_set.cpp, scene_builder.cpp remove_mesh): ctl_builder_remove_mesh against a builder that never added the
mesh, ctl_flat_bvh_update_mesh_set — the yardstick of ctl_scene_update_mesh_set — against a route that knows nothing of removal, the host re-statement of
k_compact_tri_rows, and the acceptance rules both callers share.  Cases: tests/mesh_removal_cases.py.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from cudatracerlib_amd import api
from flat_rebuild_cases import check_topology
from node_set_cases import NONE, old_of_new, old_scene, new_scene
import mesh_set_cases
from mesh_removal_cases import CASES, MESH_ORDER, chain, mesh_map, mesh_table, removed_in_front, without_meshes, geometry_arrays, check_case_shapes, base, delete_nodes
from test_mesh_set_host import tree_arrays, same_trees

_cache = {}


def steps_of(case):
    if case not in _cache:
        _cache[case] = chain(case)
    return _cache[case]


@pytest.mark.parametrize("case", CASES)
def test_case_shapes(case):
    check_case_shapes(case, steps_of(case))


# ---- the builder

@pytest.mark.parametrize("case,skip", [("R1", ["DG"]), ("R2", ["floor"]), ("R3", ["LONG", "T64"]), ("R6", [n for n in MESH_ORDER if n != "T65"])])
def test_builder_equals_one_that_never_added_the_mesh(case, skip):
    """tri_data, woop, woop_index, bvh_nodes and the mesh records, at every index, byte for byte; std_material_offset — the materials are not compacted — is the one the
    mesh had before the removal, and the materials the kept nodes read through it are the never-added scene's"""
    old, _, new = steps_of(case)[0]
    never = without_meshes(skip)
    for name, got, want in zip(("tri_data", "woop", "woop_index", "bvh_nodes"), geometry_arrays(new.desc), geometry_arrays(never.desc)):
        assert got.shape == want.shape and np.array_equal(got, want), "%s: %s" % (case, name)
    G, Wn, O = mesh_table(new.desc), mesh_table(never.desc), mesh_table(old.desc)
    assert np.array_equal(G[:, :4], Wn[:, :4]), "the mesh records' offsets"
    mm = mesh_map(old, new)
    assert np.array_equal(G[:, 4], O[mm, 4]), "std_material_offset stays what it was"
    assert new.desc.n_nodes == never.desc.n_nodes
    gn, wn = new.desc.view("nodes", np.uint32, new.desc.n_nodes, 6), never.desc.view("nodes", np.uint32, never.desc.n_nodes, 6)
    assert np.array_equal(gn[:, 0], wn[:, 0]), "the nodes' mesh indices"
    gm, wm = material_rows(new.desc), material_rows(never.desc)
    assert new.desc.n_materials == old.desc.n_materials, "the material table is not compacted"
    for k in range(new.desc.n_nodes):
        assert np.array_equal(gm[gn[k, 1]], wm[wn[k, 1]]), "node %d's material" % k
    same_trees(api.FlatBvh(new.desc), api.FlatBvh(never.desc), "the two descriptions flatten alike")


def material_rows(desc):
    size = C.sizeof(api.ctl_material)
    buf = (C.c_char * (desc.n_materials * size)).from_address(C.cast(desc.materials, C.c_void_p).value)
    return np.frombuffer(buf, dtype=np.uint32).reshape(desc.n_materials, size // 4)


def test_removing_an_instanced_mesh_is_refused():
    sc, m = base("R")
    sc.UpdateScene()
    before = [a.copy() for a in geometry_arrays(sc.desc)] + [mesh_table(sc.desc).copy(), sc.desc.view("nodes", np.uint32, sc.desc.n_nodes, 6).copy()]
    ids = sc.mesh_ids()
    for mesh, word in ((m["T64"], "node 6"), (sc.desc.n_meshes, "bad mesh index")):
        with pytest.raises(api.CtlError) as e:
            sc.RemoveMesh(mesh)
        assert e.value.code == api.ERR_INVALID and word in str(e.value), str(e.value)
    sc.UpdateScene()
    after = geometry_arrays(sc.desc) + [mesh_table(sc.desc), sc.desc.view("nodes", np.uint32, sc.desc.n_nodes, 6)]
    assert all(np.array_equal(x, y) for x, y in zip(before, after)) and sc.mesh_ids() == ids, "a refusal changed the builder"
    # the ids: stable across a removal, on the builder and on the description
    delete_nodes(sc, ["T64"]); sc.RemoveMesh(m["T64"])
    assert sc.mesh_ids() == ids[:m["T64"]] + ids[m["T64"] + 1:] and sc.UpdateScene().mesh_ids == sc.mesh_ids()
    assert sc.add_mesh(*mesh_set_cases.soup(3, 5)) == len(ids) - 1 and sc.mesh_ids()[-1] == max(ids) + 1, "ids are never reused"


# ---- the yardstick

def lowered(route, mid, old, mm):
    """the leaves of `route` (a tree over `mid`: every held mesh still there) with word 12 lowered by the triangles removed in front of each entry's mesh — numpy, from
    the counts of the old description alone"""
    front, kept = removed_in_front(old.desc, mm)
    total = int(np.array(api.mesh_counts(old.desc), np.int64).reshape(-1, 2)[~kept, 0].sum())
    L = route.leaves().copy()
    mesh_of_node = mid.desc.view("nodes", np.uint32, mid.desc.n_nodes, 6)[:, 0].astype(np.int64)
    mesh = mesh_of_node[L[:, 13] & 0x7fffffff]
    assert (mesh >= old.desc.n_meshes).any() or kept[mesh].all(), "an entry of a removed mesh survived the node edit"
    delta = np.where(mesh < old.desc.n_meshes, front[np.minimum(mesh, old.desc.n_meshes - 1), 0], total)
    L[:, 12] = (L[:, 12].astype(np.int64) - 2 * delta).astype(np.uint32)
    return L


@pytest.mark.parametrize("case,builder", [(c, "lbvh") for c in CASES] + [("R3", "ploc")])
def test_yardstick_equals_the_removal_blind_route(case, builder):
    """ctl_flat_bvh_update_nodes / _update_meshes (R5, whose node map is an identity: ctl_flat_bvh_rebuild) take the old tree to the description with the new nodes and EVERY held mesh; that tree's leaves with their triangle words
    lowered in numpy are the new handle's, and nodes, part_index, the level lists and max_depth are equal as they stand: entry order and boxes do not depend on triangle
    numbers"""
    steps = steps_of(case)
    fb = api.FlatBvh(steps[0][0].desc)
    for k, (old, mid, new) in enumerate(steps):
        mm, nm = mesh_map(old, new), old_of_new(old, new)
        assert np.array_equal(nm, old_of_new(old, mid))
        route = api.FlatBvh(steps[0][0].desc)
        for o, _, n in steps[:k]:
            route.update_mesh_set(n.desc, mesh_map(o, n), old_of_new(o, n), builder=builder)
        identity = np.array_equal(nm, np.arange(old.desc.n_nodes)) and mid.desc.n_meshes == old.desc.n_meshes
        if identity:
            route.rebuild(mid.desc, builder=builder)     # R5: update_nodes leaves a tree alone under an identity map; ctl_flat_bvh_rebuild is the removal-blind call that rebuilds
        elif mid.desc.n_meshes == old.desc.n_meshes:
            route.update_nodes(mid.desc, nm, builder=builder)
        else:
            route.update_meshes(mid.desc, nm, builder=builder)
        fb.update_mesh_set(new.desc, mm, nm, builder=builder)
        check_topology(fb)
        assert fb.desc.n_leaves == route.desc.n_leaves
        got, want = tree_arrays(fb), tree_arrays(route)
        assert np.array_equal(got[1], lowered(route, mid, old, mm)), "%s: the leaves with word 12 lowered" % case
        for i in (0, 2, 3, 4, 5, 6):
            assert np.array_equal(got[i], want[i]), "%s: tree array %d" % (case, i)


@pytest.mark.parametrize("case", CASES)
def test_compacted_table_is_triangle_woop_rows(case):
    """the host re-statement of k_compact_tri_rows over the old table equals the table of the new description (its kept part: R4 appends behind it)"""
    for old, _, new in steps_of(case):
        mm = mesh_map(old, new)
        front, kept = removed_in_front(old.desc, mm)
        got = api.compact_tri_rows_host(old.desc, mm, api.triangle_woop_rows(old.desc))
        n_kept = int(np.array(api.mesh_counts(old.desc), np.int64).reshape(-1, 2)[kept, 0].sum())
        assert len(got) == n_kept and np.array_equal(got, api.triangle_woop_rows(new.desc)[:n_kept]), case


def test_nothing_removed_is_update_meshes_and_update_nodes():
    """R7: byte-equal to the existing calls on the same input"""
    old, new = old_scene("N6"), new_scene("N6")
    nm = old_of_new(old, new)
    same_trees(api.FlatBvh(old.desc).update_mesh_set(new.desc, np.arange(old.desc.n_meshes), nm), api.FlatBvh(old.desc).update_nodes(new.desc, nm), "N6's node edit")
    seq = mesh_set_cases.descriptions("M2")
    nm = old_of_new(seq[0], seq[1])
    mm = np.concatenate([np.arange(seq[0].desc.n_meshes), np.full(seq[1].desc.n_meshes - seq[0].desc.n_meshes, NONE)]).astype(np.uint32)
    same_trees(api.FlatBvh(seq[0].desc).update_mesh_set(seq[1].desc, mm, nm), api.FlatBvh(seq[0].desc).update_meshes(seq[1].desc, nm), "M2's append")


# ---- refusals

def refused(fb, desc, mm, nm, word=None, code=None):
    before = [a.copy() if isinstance(a, np.ndarray) else a for a in tree_arrays(fb)]
    with pytest.raises(api.CtlError) as e:
        fb.update_mesh_set(desc, mm, nm)
    assert e.value.code == (api.ERR_INVALID if code is None else code), str(e.value)
    if word:
        assert word in str(e.value), str(e.value)
    C_ = api.FlatBvhDesc(); api._check(api.lib.ctl_flat_bvh_arrays(fb._h, C.byref(C_))); fb.desc = C_
    for x, y in zip(tree_arrays(fb), before):
        assert np.array_equal(x, y), "a refusal changed the handle"


def refusal_inputs(old, mid, new, mm, nm):
    """[(name, description, mesh map, node map, a word of the message)]: every rule of the acceptance list broken once; the arrays the descriptions point at are kept alive
    by the list's last column"""
    copy = lambda: api.ctl_scene_desc.from_buffer_copy(new.desc)
    out = []
    swapped = mm.copy(); swapped[[1, 2]] = swapped[[2, 1]]
    out.append(("a reordered map", new.desc, swapped, nm, "not reordered", None))
    gone = int(np.setdiff1d(np.arange(old.desc.n_nodes), nm)[0]); on_removed = nm.copy(); on_removed[gone] = gone      # the new node at a removed node's index "was" that node
    assert (np.diff(on_removed.astype(np.int64)) > 0).all()
    out.append(("a kept node on a removed mesh", new.desc, mm, on_removed, "which the mesh map removes", None))
    last = new.desc.n_meshes - 1
    for what, step in (("one too low", -1), ("one too high", 1)):
        d = copy(); M = mesh_table(new.desc).copy(); M[last, 0] = int(M[last, 0]) + step; d.meshes = M.ctypes.data
        out.append(("a kept record with its triangle offset " + what, d, mm, nm, "another record", M))
    kept0 = int(np.nonzero(mm != NONE)[0][-1])
    row0 = int(mesh_table(new.desc)[kept0, 3])
    d = copy(); woop = new.desc.view("woop", np.float32, new.desc.n_woop, 12).copy(); woop[row0, 3] += 0.25; d.woop = woop.ctypes.data
    out.append(("changed values in a kept mesh", d, mm, nm, "ctl_scene_update first", woop))
    d = copy(); idx = new.desc.view("woop_index", np.uint32, new.desc.n_woop, 1).copy(); idx[row0, 0] ^= 2; d.woop_index = idx.ctypes.data
    out.append(("changed woop_index in a kept mesh", d, mm, nm, "another structure", idx))
    return out


def test_refusals_on_the_yardstick():
    old, mid, new = steps_of("R3")[0]
    mm, nm = mesh_map(old, new), old_of_new(old, new)
    fb = api.FlatBvh(old.desc)
    for name, desc, m1, m2, word, _ in refusal_inputs(old, mid, new, mm, nm):
        refused(fb, desc, m1, m2, word)
    # an appended mesh in front of a kept one (R4's map with its first appended element moved to the front)
    o4, _, n4 = steps_of("R4")[0]
    m4 = mesh_map(o4, n4); bad = np.concatenate([[NONE], m4[:-1]]).astype(np.uint32)
    assert (m4 == NONE).sum() == 2
    refused(api.FlatBvh(o4.desc), n4.desc, bad, old_of_new(o4, n4), "behind an appended one")
    # the maps' sizes
    refused(fb, new.desc, mm[:-1], nm, "mesh map has")
    # Q8: unsupported, as for update_nodes
    refused(api.FlatBvh(old.desc, api.FLAT_Q8), new.desc, mm, nm, "Q4", api.ERR_UNSUPPORTED)
    # the existing calls keep their answers to a removed mesh, word for word
    for call, word in (("update_nodes", "the set of meshes differs: only meshes the scene already holds can be instanced; re-create the scene"),
                       ("update_meshes", "meshes can be appended, not removed; re-create the scene")):
        with pytest.raises(api.CtlError) as e:
            getattr(api.FlatBvh(old.desc), call)(new.desc, nm)
        assert e.value.code == api.ERR_INVALID and word in str(e.value), str(e.value)
    # and the handle, untouched by all of it, still takes the correct call
    fb.update_mesh_set(new.desc, mm, nm)
    same_trees(fb, api.FlatBvh(old.desc).update_mesh_set(new.desc), "after the refusals; the maps from the ids")
