"""The PLOC builder of the rebuild (csrc/flat_ploc.h), the host half: ctl_flat_bvh_rebuild_ex / ctl_flat_bvh_update_nodes_ex with CTL_REBUILD_PLOC run the single-source
arithmetic the device kernels run (tests/test_gpu_flat_ploc.py holds the two equal byte for byte).  Held here: the tree is a valid tree of the same entries; the
clustering, collapse and layout equal an independent numpy restatement (tests/ploc_ref.py) word for word; the node area — the proxy INTEGRATION.md tells hosts to
compare — is strictly below the LBVH's on every scene-sized case; the LBVH through the _ex entry points is the LBVH of the plain ones, byte for byte; refusals.
Cases: tests/flat_ploc_cases.py.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from cudatracerlib_amd import api
from scene_update_cases import build, rays_for_update
from flat_rebuild_cases import check_topology, entry_rows, node_area, moved_nodes
from flat_ploc_cases import CASES, IDS, REF_CASES, QUALITY_CASES, old_scene, new_scene
from test_flat_rebuild_host import check_hits, check_containment
import node_set_cases as nsc
import ploc_ref

N_RAYS = 4000
_trees = {}


def trees(case, pose):
    """(old, new, the tree refitted, rebuilt by the LBVH, rebuilt by PLOC, stages 1 - 4 of the refitted tree): computed once per case and pose, never changed"""
    if (case, pose) not in _trees:
        old, new = old_scene(case), new_scene(case, pose)
        refitted = api.FlatBvh(old.desc).refit(new.desc)
        order = refitted.rebuild_order(new.desc)
        _trees[case, pose] = (old, new, refitted, api.FlatBvh(old.desc).rebuild(new.desc), api.FlatBvh(old.desc).rebuild(new.desc, builder="ploc"), order)
    return _trees[case, pose]


def same_bytes(a, b):
    return (np.array_equal(a.nodes(), b.nodes()) and np.array_equal(a.leaves(), b.leaves()) and np.array_equal(a.parts()[0], b.parts()[0])
            and np.array_equal(a.child_links(), b.child_links()) and all(np.array_equal(x, y) for x, y in zip(a.levels(), b.levels())) and a.desc.max_depth == b.desc.max_depth)


@pytest.mark.parametrize("case,pose", CASES, ids=IDS)
def test_ploc_tree_is_a_valid_tree_of_the_same_entries(orc, case, pose):
    old, new, refitted, lbvh, ploc, _ = trees(case, pose)
    levels = check_topology(ploc)
    assert np.array_equal(entry_rows(ploc), entry_rows(lbvh)) and np.array_equal(entry_rows(ploc), entry_rows(refitted))
    check_containment(ploc, new.desc, old.desc, case)
    rays = rays_for_update(new.desc, N_RAYS, 19, aim_nodes=moved_nodes(old.desc, new.desc))
    check_hits(orc, ploc, new.desc, rays, "%s %s" % (case, pose))
    print("%s %s: %d nodes over %d entries in %d levels (LBVH %d nodes, %d levels)" % (case, pose, len(ploc.nodes()), len(ploc.leaves()), len(levels) - 1, len(lbvh.nodes()), lbvh.desc.max_depth + 1))
    # determinism, then what follows a rebuild: a refit, and a second rebuild by either builder
    again = api.FlatBvh(old.desc).rebuild(new.desc, builder="ploc")
    assert same_bytes(again, ploc)
    N, ch = again.nodes().copy(), again.child_links().copy()
    again.refit(old.desc)
    assert np.array_equal(again.nodes()[:, 10:12], N[:, 10:12]) and np.array_equal(again.child_links(), ch)
    check_topology(again)
    again.rebuild(new.desc, builder="ploc")
    check_topology(again)
    assert np.array_equal(entry_rows(again), entry_rows(refitted))
    again.rebuild(new.desc)
    check_topology(again)
    assert np.array_equal(entry_rows(again), entry_rows(refitted))


@pytest.mark.parametrize("case,pose", REF_CASES, ids=["%s-%s" % (c, p or "built") for c, p in REF_CASES])
def test_host_twin_equals_the_numpy_restatement(case, pose):
    """the algorithm itself, not host = device: the link words, level lists, depth and entry order of the host twin against tests/ploc_ref.py"""
    old, new, refitted, _, ploc, (order, boxes, bounds) = trees(case, pose)
    ref = ploc_ref.build(order, boxes, bounds)
    N, L, L0 = ploc.nodes(), ploc.leaves(), refitted.leaves()
    assert len(N) == len(ref["mask"])
    assert np.array_equal(N[:, 3] >> 24, ref["mask"]) and np.array_equal(N[:, 10], ref["w10"]) and np.array_equal(N[:, 11], ref["w11"])
    assert np.array_equal(ploc.levels()[0], ref["level_start"]) and ploc.desc.max_depth == ref["depth"]
    assert np.array_equal(L[:, 12] & 1, ref["last"].astype(np.uint32))
    src = L0[ref["perm"]]
    assert np.array_equal(L[:, :12], src[:, :12]) and np.array_equal(L[:, 12] >> 1, src[:, 12] >> 1) and np.array_equal(L[:, 13:], src[:, 13:])
    assert np.array_equal(ploc.parts()[0], refitted.parts()[0][ref["perm"]])
    api.FlatBvh(old.desc).rebuild(new.desc, builder="ploc")          # (a description points into its builder: the cached scenes keep theirs alive)
    assert api.lib.ctl_rebuild_last_rounds() == ref["rounds"]
    if case == "SAME":
        assert (np.ptp(boxes[order[-9:]], axis=0) == 0).all(), "the nine boxes are not equal: SAME does not test the tie rule"


@pytest.mark.parametrize("case,pose", QUALITY_CASES, ids=["%s-%s" % (c, p or "built") for c, p in QUALITY_CASES])
def test_ploc_node_area_is_below_the_lbvhs(case, pose):
    """the point of the builder.  Both trees fill their leaves by the same rule, so their node counts are comparable"""
    _, new, refitted, lbvh, ploc, _ = trees(case, pose)
    a_ploc, a_lbvh, a_refit, a_fresh = node_area(ploc), node_area(lbvh), node_area(refitted), node_area(api.FlatBvh(new.desc))
    print("%s %s: node area PLOC %.6g, LBVH %.6g, refitted %.6g, fresh %.6g; PLOC / LBVH %.3f, PLOC / fresh %.3f; nodes %d / %d; depth %d / %d"
          % (case, pose, a_ploc, a_lbvh, a_refit, a_fresh, a_ploc / a_lbvh, a_ploc / a_fresh, len(ploc.nodes()), len(lbvh.nodes()), ploc.desc.max_depth, lbvh.desc.max_depth))
    assert a_ploc < a_lbvh


@pytest.mark.parametrize("case,pose", [("S1", "M4"), ("S2", "M3"), ("TW", "MV")], ids=["S1-M4", "S2-M3", "TW"])
def test_lbvh_through_the_ex_entry_point_is_the_lbvh(case, pose):
    old, new, _, lbvh, _, _ = trees(case, pose)
    fb = api.FlatBvh(old.desc)
    api._check(api.lib.ctl_flat_bvh_rebuild_ex(fb._h, C.byref(new.desc), api.REBUILD_LBVH))
    api._check(api.lib.ctl_flat_bvh_arrays(fb._h, C.byref(fb.desc)))
    assert same_bytes(fb, lbvh)
    assert api.lib.ctl_rebuild_last_rounds() == 0


def test_refusals():
    old, new = build("S3"), build("S3", "M1")
    fb = api.FlatBvh(old.desc)
    N, L, P = fb.nodes().copy(), fb.leaves().copy(), fb.parts()[0].copy()
    for bad in (2, -1, 7):
        with pytest.raises(api.CtlError) as e:
            fb.rebuild(new.desc, builder=bad)
        assert e.value.code == api.ERR_INVALID and "unknown builder" in str(e.value)
        assert np.array_equal(fb.nodes(), N) and np.array_equal(fb.leaves(), L) and np.array_equal(fb.parts()[0], P)
    with pytest.raises(ValueError):
        fb.rebuild(new.desc, builder="sah")
    q8 = api.FlatBvh(old.desc, api.FLAT_Q8)
    N8 = q8.nodes().copy()
    with pytest.raises(api.CtlError) as e:
        q8.rebuild(new.desc, builder="ploc")
    assert e.value.code == api.ERR_UNSUPPORTED and np.array_equal(q8.nodes(), N8)
    with pytest.raises(api.CtlError):
        fb.rebuild(build("S1").desc, builder="ploc")               # another scene: refused before anything is written
    assert np.array_equal(fb.nodes(), N) and np.array_equal(fb.leaves(), L)
    # the device entry points ask for the device first, then for the builder
    st = api.ctl_scene_rebuild_stats()
    code = api.lib.ctl_scene_rebuild_flat_ex(None, api.REBUILD_PLOC, C.addressof(st))
    assert code == (api.ERR_NO_DEVICE if api.device_count() == 0 else api.ERR_INVALID)
    m = np.zeros(1, np.uint32)
    code = api.lib.ctl_scene_update_nodes_ex(None, None, m.ctypes.data, api.u32(1), api.REBUILD_PLOC, None)
    assert code == (api.ERR_NO_DEVICE if api.device_count() == 0 else api.ERR_INVALID)


@pytest.mark.parametrize("case", ["N3", "N6"])
def test_node_sets_with_ploc(orc, case):
    """one removal (N3) and one addition (N6): a valid tree of the entries the LBVH call gives"""
    old, new = nsc.old_scene(case), nsc.new_scene(case)
    m = nsc.old_of_new(old, new)
    lbvh = api.FlatBvh(old.desc).update_nodes(new.desc, m)
    ploc = api.FlatBvh(old.desc).update_nodes(new.desc, m, builder="ploc")
    check_topology(ploc)
    assert np.array_equal(entry_rows(ploc), entry_rows(lbvh)) and np.array_equal(nsc.entry_keys(ploc), nsc.entry_keys(lbvh))
    assert not same_bytes(ploc, lbvh)
    rays = rays_for_update(new.desc, N_RAYS, 43)
    check_hits(orc, ploc, new.desc, rays, case)
    with pytest.raises(api.CtlError) as e:
        api.FlatBvh(old.desc).update_nodes(new.desc, m, builder=5)
    assert e.value.code == api.ERR_INVALID
    print("%s: node area PLOC %.6g, LBVH %.6g, fresh %.6g" % (case, node_area(ploc), node_area(lbvh), node_area(api.FlatBvh(new.desc))))
