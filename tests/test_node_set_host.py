"""Another set of nodes on the host (csrc/flat_nodes.h, flat_nodes.cpp): ctl_flat_bvh_update_nodes — the yardstick of ctl_scene_update_nodes —, ctl_builder_remove_node
and the argument checks both callers share.  Cases: tests/node_set_cases.py.  CPU only."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from cudatracerlib_amd import api
from flat_rebuild_cases import check_topology
from node_set_cases import CASES, NONE, FLOOR, LONG, T1, old_scene, new_scene, old_of_new, entry_keys, tri_counts, base, undone_scene, place
from scene_update_cases import rays_for_update, with_materials

N_RAYS = 3000
_cache = {}


def pair(case):
    """(old, new, map, the handle built from old and updated to new, the tree built from old, the tree freshly built from new) — made once per case, never changed"""
    if case not in _cache:
        old, new = old_scene(case), new_scene(case)
        m = old_of_new(old, new)
        _cache[case] = (old, new, m, api.FlatBvh(old.desc).update_nodes(new.desc, m), api.FlatBvh(old.desc), api.FlatBvh(new.desc))
    return _cache[case]


@pytest.mark.parametrize("case", CASES)
def test_entry_multiset(case):
    old, new, m, upd, built, fresh = pair(case)
    if case == "N3":
        part = built.parts()[0]
        assert built.desc.n_part_boxes > 0 and (built.leaves()[part != NONE, 13] == LONG).any(), "the removed node owns split references"
    elif case != "N5":
        assert built.desc.n_part_boxes > 0, "creation made no split references"
    got, was, want = entry_keys(upd), entry_keys(built), entry_keys(fresh)
    added = np.nonzero(m == NONE)[0]
    new_of_old = np.full(old.desc.n_nodes, NONE, np.uint32); new_of_old[m[m != NONE]] = np.nonzero(m != NONE)[0]
    # kept nodes: the built-from-old tree's rows, renumbered
    kept = was[new_of_old[was[:, 1]] != NONE].copy(); kept[:, 1] = new_of_old[kept[:, 1]]
    kept = kept[np.lexsort(kept.T[::-1])]
    got_kept = got[~np.isin(got[:, 1], added)]
    assert np.array_equal(got_kept, kept)
    # added nodes: exactly one whole entry per regular triangle — the triangles the freshly built tree has entries for
    nodes = new.desc.view("nodes", np.uint32, new.desc.n_nodes, 6)
    counts = tri_counts(new.desc)
    for k in added:
        mine, theirs = got[got[:, 1] == k], want[want[:, 1] == k]
        assert (mine[:, 2] == 0).all() and len(np.unique(mine[:, 0])) == len(mine), "an added node has a split reference or two entries of one triangle"
        assert np.array_equal(mine[:, 0], np.unique(theirs[:, 0]))
        n_tri = counts[nodes[k, 0]]
        assert len(mine) == (n_tri - 1 if case == "N8" else n_tri)        # DG loses its degenerate triangle, nothing else loses any
        if (theirs[:, 2] == 0).all():
            assert np.array_equal(mine, theirs)
    if not len(added) or all((want[want[:, 1] == k, 2] == 0).all() for k in added):
        assert np.array_equal(got, want), "the multiset differs from the freshly built tree's"
    # what an entry carries besides its keys: the mesh's rows, the new node's inverse transform
    L, F = upd.leaves(), fresh.leaves()
    order = lambda A: A[np.lexsort((A[:, 12] >> 1, A[:, 13]))]
    if np.array_equal(got, want):
        a, b = order(L.copy()), order(F.copy()); a[:, 12] &= ~np.uint32(1); b[:, 12] &= ~np.uint32(1)
        whole = np.ones(len(a), bool) if not (got[:, 2] != 0).any() else None
        if whole is not None:
            assert np.array_equal(a, b), "entries differ from the freshly built tree's"
        else:
            assert np.array_equal(a[:, 16:29], b[:, 16:29]), "inverse transforms"


@pytest.mark.parametrize("case", CASES)
def test_tree_shape(case):
    upd = pair(case)[3]
    if case == "N10":
        return    # the identity map refits the built tree: nothing is rebuilt (test_identity_map)
    check_topology(upd)
    if case == "N4":
        N = upd.nodes()
        assert len(N) == 1 and len(upd.leaves()) == 1 and (N[0, 3] >> 24) & 15 == 1 and upd.desc.max_depth == 0, "one triangle: a root with one leaf slot"


def test_identity_map():
    """nothing changed: the tree stays as built (ctl_scene_update does nothing either); the same map with a node moved: a refit, no rebuild"""
    old, new, m, upd, built, fresh = pair("N10")
    assert np.array_equal(m, np.arange(old.desc.n_nodes))
    assert np.array_equal(upd.nodes(), built.nodes()) and np.array_equal(upd.leaves(), built.leaves()) and np.array_equal(upd.child_links(), built.child_links())
    assert upd.desc.n_slab_nodes == built.desc.n_slab_nodes
    sc, _ = base("N10"); sc.SetNodeTransform(T1, place(17)); sc.UpdateScene()
    moved, ref = api.FlatBvh(old.desc).update_nodes(sc.desc, m), api.FlatBvh(old.desc).refit(sc.desc)
    assert np.array_equal(moved.nodes(), ref.nodes()) and np.array_equal(moved.leaves(), ref.leaves()) and not np.array_equal(moved.leaves(), built.leaves())


@pytest.mark.parametrize("case", CASES)
def test_traversal_equals_two_level(orc, case):
    """the oracle's CPU traversal of the yardstick arrays against its two-level traversal of the new description: (t, u, v, triangle, node) bit for bit"""
    old, new, m, upd, _, _ = pair(case)
    d = new.desc
    rays = rays_for_update(d, N_RAYS, 53, aim_nodes=list(np.nonzero(m == NONE)[0]))
    want, got = orc.intersect(d, rays), orc.intersect(d, rays, flat=upd.desc)
    for k in ("tri_idx", "node_idx"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("dist", "u", "v"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
    assert (want["tri_idx"] >= 0).any()
    assert np.array_equal(orc.intersect(d, rays, any_hit=True, flat=upd.desc)["tri_idx"] >= 0, orc.intersect(d, rays, any_hit=True)["tri_idx"] >= 0)


def test_update_follows_update():
    """a second change undoes the first (node_set_cases.undone_scene): the tree holds the original scene's triangles under the original transforms — LONG's node, removed
    and created again, has whole entries where creation had split references — and everything that worked on the old handle works on the new one"""
    old, new, m, upd, built, _ = pair("N7")
    undone, orig = undone_scene()
    again = api.FlatBvh(old.desc).update_nodes(new.desc, m).update_nodes(undone.desc, old_of_new(new, undone))
    check_topology(again)
    a, b = entry_keys(again), entry_keys(built)
    a[:, 1] = orig[a[:, 1]]
    assert np.array_equal(np.unique(a[:, :2], axis=0), np.unique(b[:, :2], axis=0))
    assert (a[a[:, 1] == LONG, 2] == 0).all() and (b[b[:, 1] == LONG, 2] != 0).any()
    again.refit(undone.desc); again.rebuild(undone.desc); check_topology(again)


# ---- the builder

def builder_bytes(sc):
    d = sc.UpdateScene()
    return (bytes(d.view("nodes", np.uint8, d.n_nodes, 24)), bytes(d.view("node_transforms", np.uint8, d.n_nodes, 64)), bytes(d.view("node_inv_transforms", np.uint8, d.n_nodes, 64)),
            bytes(C.string_at(C.addressof(d.lights.contents), d.n_lights_buf * C.sizeof(api.ctl_light))) if d.n_lights_buf else b"", d.n_materials)


def diffuse_light_nodes(d):
    return [int(d.lights[i].node_idx) for i in range(d.n_lights_buf) if d.lights[i].type == 2]     # CTL_LIGHT_DIFFUSE


def test_builder_remove_node():
    sc, m = base("N1")
    panel = sc.CreateNode(m["T4"], np.array([[1, 0, 0, 3], [0, 1, 0, 4], [0, 0, 1, 1], [0, 0, 0, 1]], np.float32))       # node 10, an area light on it
    sc.CreateLight(panel, 0, (5.0, 5.0, 5.0))
    before = builder_bytes(sc)
    nodes0 = sc.desc.view("nodes", np.uint32, sc.desc.n_nodes, 6).copy()
    assert diffuse_light_nodes(sc.desc) == [panel]
    # refusals leave the builder as it was
    for node, code in ((panel, api.ERR_UNSUPPORTED), (11, api.ERR_INVALID), (NONE, api.ERR_INVALID)):
        with pytest.raises(api.CtlError) as e:
            sc.DeleteNode(node)
        assert e.value.code == code, (node, str(e.value))
        assert builder_bytes(sc) == before and sc.node_ids() == tuple(range(11))
    # a removal: indices shift, the lights' node_idx follows, the materials stay
    sc.DeleteNode(LONG)
    d = sc.UpdateScene()
    nodes1 = d.view("nodes", np.uint32, d.n_nodes, 6)
    assert d.n_nodes == 10 and np.array_equal(nodes1, np.delete(nodes0, LONG, axis=0)) and d.n_materials == before[4]
    assert sc.node_ids() == tuple(k for k in range(11) if k != LONG) and d.node_ids == sc.node_ids()
    assert diffuse_light_nodes(d) == [panel - 1]
    # the last node stays
    one, _ = base("N5")
    with pytest.raises(api.CtlError) as e:
        one.DeleteNode(0)
    assert e.value.code == api.ERR_INVALID


def test_remove_then_add_gives_a_fresh_builders_description():
    """base - LONG + T63 against a builder that never had LONG's node: the same description but for the orphaned material copy and the offsets behind it"""
    xf = np.diag([2, 2, 2, 1]).astype(np.float32)
    a, m = base("N1"); a.DeleteNode(LONG); a.CreateNode(m["T63"], xf); da = a.UpdateScene()
    g, mg = base("N1", skip=LONG); g.CreateNode(mg["T63"], xf); dg = g.UpdateScene()
    assert da.n_nodes == dg.n_nodes == 10
    na, ng = da.view("nodes", np.uint32, da.n_nodes, 6), dg.view("nodes", np.uint32, dg.n_nodes, 6)
    assert np.array_equal(na[:, [0, 2, 3, 4, 5]], ng[:, [0, 2, 3, 4, 5]])
    for name in ("node_transforms", "node_inv_transforms"):
        assert np.array_equal(da.view(name, np.uint32, da.n_nodes, 16), dg.view(name, np.uint32, dg.n_nodes, 16)), name
    assert bytes(da.view("scene_bvh_nodes", np.uint8, da.n_scene_bvh_nodes, 64)) == bytes(dg.view("scene_bvh_nodes", np.uint8, dg.n_scene_bvh_nodes, 64))
    assert list(da.box_min) == list(dg.box_min) and list(da.box_max) == list(dg.box_max)
    for k in range(da.n_nodes):      # the material each node sees is the same record
        assert C.string_at(C.addressof(da.materials[int(na[k, 1])]), 384) == C.string_at(C.addressof(dg.materials[int(ng[k, 1])]), 384)
    assert da.n_materials == dg.n_materials + 1     # LONG's orphaned copy
    assert api.scene_desc_diff(da, dg) & api.DIFF_TOPOLOGY     # (ctl_scene_desc_diff keeps calling it that: the counts differ)


# ---- argument checks

def refused(fb, desc, m, code, word=None):
    before = (fb.nodes().copy(), fb.leaves().copy(), fb.parts()[0].copy() if fb.parts()[0] is not None else None)
    with pytest.raises(api.CtlError) as e:
        fb.update_nodes(desc, m)
    assert e.value.code == code, str(e.value)
    if word:
        assert word in str(e.value), str(e.value)
    C_ = api.FlatBvhDesc(); api._check(api.lib.ctl_flat_bvh_arrays(fb._h, C.byref(C_))); fb.desc = C_
    assert np.array_equal(fb.nodes(), before[0]) and np.array_equal(fb.leaves(), before[1]), "a refusal changed the handle"


def test_refusals_on_the_yardstick():
    old, new, m, _, _, _ = pair("N7")
    fb = api.FlatBvh(old.desc)
    INV, UNS = api.ERR_INVALID, api.ERR_UNSUPPORTED
    # the map
    assert api.lib.ctl_flat_bvh_update_nodes(fb._h, C.byref(new.desc), None, api.u32(len(m))) == INV and b"null" in api.lib.ctl_last_error()
    refused(fb, new.desc, m[:-1], INV, "elements")
    bad = m.copy(); bad[1], bad[2] = m[2], m[1]
    refused(fb, new.desc, bad, INV, "increasing")
    bad = m.copy(); bad[1] = bad[0]
    refused(fb, new.desc, bad, INV, "increasing")
    bad = m.copy(); bad[-3] = old.desc.n_nodes
    refused(fb, new.desc, bad, INV, "names node")
    # a kept node with another mesh (the map is off by one node) / another material assignment
    bad = m.copy(); bad[3] = LONG
    refused(fb, new.desc, bad, INV, "assignment")
    d = api.ctl_scene_desc.from_buffer_copy(new.desc)
    nodes = new.desc.view("nodes", np.uint32, new.desc.n_nodes, 6).copy(); nodes[T1, 1] = nodes[T1 + 1, 1]
    d.nodes = nodes.ctypes.data
    refused(fb, d, m, INV, "assignment")
    # another mesh set, another geometry structure, other geometry values, a shrunken material table
    sc, mm = base("N7"); sc.add_mesh(*__import__("node_set_cases").soup(3, 5)); extra = sc.UpdateScene()
    refused(fb, extra, np.arange(extra.n_nodes, dtype=np.uint32), INV)
    d = api.ctl_scene_desc.from_buffer_copy(new.desc)
    idx = new.desc.view("woop_index", np.uint32, new.desc.n_woop, 1).copy(); idx[0, 0] ^= 2
    d.woop_index = idx.ctypes.data
    refused(fb, d, m, INV, "structure")
    d = api.ctl_scene_desc.from_buffer_copy(new.desc)
    woop = new.desc.view("woop", np.float32, new.desc.n_woop, 12).copy(); woop[0, 3] += 0.25
    d.woop = woop.ctypes.data
    refused(fb, d, m, INV, "ctl_scene_update first")
    d = api.ctl_scene_desc.from_buffer_copy(new.desc); d.n_materials = old.desc.n_materials - 1
    refused(fb, d, m, INV)
    # a description ctl_scene_desc_check refuses (a node transform that is not affine)
    d = api.ctl_scene_desc.from_buffer_copy(new.desc)
    X = new.desc.view("node_transforms", np.float32, new.desc.n_nodes, 16).copy(); X[0, 12] = 0.5
    d.node_transforms = X.ctypes.data
    with pytest.raises(api.CtlError):
        api.scene_desc_check(d)
    refused(fb, d, m, INV)
    # no node left
    d = api.ctl_scene_desc.from_buffer_copy(new.desc); d.n_nodes = 0
    refused(fb, d, m[:0], INV, "no node")
    # Q8
    refused(api.FlatBvh(old.desc, api.FLAT_Q8), new.desc, m, UNS, "Q4")
    # after all that the handle still takes the change
    fb.update_nodes(new.desc, m); check_topology(fb)


EXPLICIT_CODE = r'''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
from cudatracerlib_amd import api
from node_set_cases import old_scene, new_scene, old_of_new
old, new = old_scene("N7"), new_scene("N7")
fb = api.FlatBvh(old.desc)
assert fb.desc.compact == 0
try:
    fb.update_nodes(new.desc, old_of_new(old, new))
except api.CtlError as e:
    assert e.code == api.ERR_UNSUPPORTED and "explicit links" in str(e), str(e)
    print("REFUSED OK")
'''


def test_a_tree_with_explicit_links_is_refused():
    """the rule rebuild_refuse has: built through CTL_FLAT_FORCE_EXPLICIT=1 (knobs build), in a child process"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CTL_FLAT_FORCE_EXPLICIT="1", CTL_AMD_LIB=os.path.join(root, "cudatracerlib_amd", "libctl_knobs.so"))
    r = subprocess.run([sys.executable, "-c", EXPLICIT_CODE % (root, os.path.join(root, "tests"))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "REFUSED OK" in r.stdout, r.stderr[-2000:]


def test_symbols_and_device_check():
    for name in ("ctl_builder_remove_node", "ctl_scene_update_nodes", "ctl_flat_bvh_update_nodes"):
        assert hasattr(api.lib, name), name
    m = np.zeros(1, np.uint32)
    rc = api.lib.ctl_scene_update_nodes(None, None, m.ctypes.data, api.u32(1), None)
    assert rc == (api.ERR_NO_DEVICE if api.device_count() == 0 else api.ERR_INVALID)       # the device is checked first
    assert C.sizeof(api.ctl_scene_nodes_stats) == 24 + C.sizeof(api.ctl_scene_rebuild_stats) + 8
