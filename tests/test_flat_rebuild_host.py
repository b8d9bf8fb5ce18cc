"""The rebuild of the flattened Q4 tree, the host half: ctl_flat_bvh_rebuild (csrc/flat_rebuild.cpp) runs the single-source arithmetic of csrc/flat_rebuild.h that the
device kernels of ctl_scene_rebuild_flat run (tests/test_gpu_flat_rebuild.py holds the two equal byte for byte).  A rebuilt tree is held to the bar of a built one: the
layout the traversal kernel expects, containment, the same set of entries, and the oracle's traversal of it reports the two-level traversal's (t, u, v, triangle, node)
bit for bit.  Cases: tests/flat_rebuild_cases.py.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from cudatracerlib_amd import api
from scene_update_cases import build, rays_for_update, assert_same_hits, check_structure
from scene_deform_cases import check_structure_with_collapsed
from flat_rebuild_cases import CASES, IDS, old_scene, new_scene, moved_nodes, check_topology, entry_rows, node_area

N_RAYS = 4000


def check_containment(fb, new_desc, old_desc, case):
    """scene_update_cases.check_structure with the high-side figure of the inner slots measured, in whole steps, on a freshly built tree of the same pose"""
    if case == "S3D3":   # collapsed triangles have no vertices to contain
        _, _, fresh_needs = check_structure_with_collapsed(api.FlatBvh(new_desc), new_desc, new_desc, np.inf)
        _, collapsed, excess = check_structure_with_collapsed(fb, new_desc, old_desc, float(np.ceil(fresh_needs)))
        assert collapsed > 0                                      # the entries with inverted boxes are still in the tree
        return excess
    _, fresh_needs = check_structure(api.FlatBvh(new_desc), new_desc)
    return check_structure(fb, new_desc, built_from=old_desc, inner_high_steps=float(np.ceil(fresh_needs)))[1]


def check_hits(orc, fb, desc, rays, what):
    want = orc.intersect(desc, rays)
    ties = assert_same_hits(orc.intersect(desc, rays, flat=fb.desc), want, what + " closest hit")
    assert ties <= max(4, len(rays) // 1000)
    assert np.array_equal(orc.intersect(desc, rays, any_hit=True, flat=fb.desc)["tri_idx"] >= 0, orc.intersect(desc, rays, any_hit=True)["tri_idx"] >= 0), what + " any hit"
    return want


@pytest.mark.parametrize("case,pose", CASES, ids=IDS)
def test_rebuilt_tree_is_a_valid_tree_of_the_same_entries(orc, case, pose):
    old, new = old_scene(case), new_scene(case, pose)
    refitted = api.FlatBvh(old.desc).refit(new.desc)
    before = entry_rows(refitted)
    fb = api.FlatBvh(old.desc).rebuild(new.desc)
    N, L = fb.nodes().copy(), fb.leaves().copy()
    # structure: the layout the traversal kernel expects, from the node words alone, and the explicit links against the implied ones
    levels = check_topology(fb)
    assert len(L) == len(refitted.leaves())
    if case in ("T1", "T4"):
        assert len(N) == 1 and (N[0, 3] >> 24) == 0xf1 and len(L) == int(case[1])      # a root with one leaf slot; the empty slots lead to its first entry
    if case == "T5":
        assert len(N) == 1 and ((N[0, 3] >> 24) & 15) == 3 and ((N[0, 3] >> 28) & 3) == 3   # the first split: two leaf slots
    # the entries: the same multiset, whatever their order
    assert np.array_equal(entry_rows(fb), before)
    excess = check_containment(fb, new.desc, old.desc, case)
    a_refit, a_rebuilt, a_fresh = node_area(refitted), node_area(fb), node_area(api.FlatBvh(new.desc))
    print("%s %s: %d nodes over %d entries in %d levels; node area refitted %.6g, rebuilt %.6g, fresh %.6g; inner slots high side %.4f steps"
          % (case, pose, len(N), len(L), len(levels) - 1, a_refit, a_rebuilt, a_fresh, excess))
    if pose == "M4":   # the reference situation: refit alone really degrades here (half again the fresh tree's area or more), and the rebuild repairs some of it
        assert a_refit > 1.5 * a_fresh, "M4 does not degrade the refitted tree: choose another motion"
        assert a_rebuilt < a_refit
    # hits
    rays = rays_for_update(new.desc, N_RAYS, 19, aim_nodes=moved_nodes(old.desc, new.desc))
    want = check_hits(orc, fb, new.desc, rays, "%s %s" % (case, pose))
    assert (want["tri_idx"] >= 0).any()
    # determinism: the same input twice gives the same bytes
    again = api.FlatBvh(old.desc).rebuild(new.desc)
    assert np.array_equal(again.nodes(), N) and np.array_equal(again.leaves(), L) and np.array_equal(again.parts()[0], fb.parts()[0]) and np.array_equal(again.child_links(), fb.child_links())
    # a second rebuild, of the rebuilt tree: again a valid tree of the same entries (equal codes are ordered by the entries' positions, which the first rebuild changed,
    # so the bytes need not be the same)
    fb.rebuild(new.desc)
    check_topology(fb)
    assert np.array_equal(entry_rows(fb), before)


@pytest.mark.parametrize("case,pose,other", [("S1", "M4", "M2"), ("S2", "M3", None), ("S3", "M3", "M1"), ("TW", "MV", None), ("S3D3", None, "M3")], ids=["S1", "S2", "S3", "TW", "S3D3"])
def test_rebuild_then_refit(orc, case, pose, other):
    """everything that worked on the built tree works on the rebuilt one: a refit to another pose keeps containment and hits"""
    old, new, then = old_scene(case), new_scene(case, pose), new_scene(case, other)
    fb = api.FlatBvh(old.desc).rebuild(new.desc)
    N, ch = fb.nodes().copy(), fb.child_links().copy()
    fb.refit(then.desc)
    assert np.array_equal(fb.nodes()[:, 10:12], N[:, 10:12]) and np.array_equal(fb.nodes()[:, 3] >> 24, N[:, 3] >> 24) and np.array_equal(fb.child_links(), ch)
    check_topology(fb)
    check_containment(fb, then.desc, old.desc, case)
    rays = rays_for_update(then.desc, N_RAYS, 23, aim_nodes=moved_nodes(new.desc, then.desc))
    check_hits(orc, fb, then.desc, rays, "%s %s then %s" % (case, pose, other))


def test_rebuild_is_refused_where_it_cannot_work():
    old, new = build("S3"), build("S3", "M1")
    q8 = api.FlatBvh(old.desc, api.FLAT_Q8)
    N = q8.nodes().copy()
    with pytest.raises(api.CtlError) as e:
        q8.rebuild(new.desc)
    assert e.value.code == api.ERR_UNSUPPORTED and np.array_equal(q8.nodes(), N)
    fb = api.FlatBvh(old.desc)
    N, L = fb.nodes().copy(), fb.leaves().copy()
    with pytest.raises(api.CtlError):
        fb.rebuild(build("S1").desc)                              # another scene: refused before anything is written
    assert np.array_equal(fb.nodes(), N) and np.array_equal(fb.leaves(), L)


def test_rebuild_without_a_device():
    """ctl_scene_rebuild_flat asks for the device before it looks at its arguments: CTL_ERR_NO_DEVICE on a machine without one (where no scene can exist), and the
    null scene is what a machine with a device complains about"""
    st = api.ctl_scene_rebuild_stats()
    code = api.lib.ctl_scene_rebuild_flat(None, C.addressof(st))
    if api.device_count() == 0:
        assert code == api.ERR_NO_DEVICE and b"no HIP device" in api.lib.ctl_last_error()
    else:
        assert code == api.ERR_INVALID
