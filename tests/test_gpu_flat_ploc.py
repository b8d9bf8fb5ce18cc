"""The PLOC builder of the rebuild on the device (ctl_scene_rebuild_flat_ex / ctl_scene_update_nodes_ex with CTL_REBUILD_PLOC; csrc/flat_rebuild.hip, csrc/flat_ploc.h):
the device tree against the host twin byte for byte — nodes, entries, part_index, clip boxes, links, level lists, depth —, the traversal of the rebuilt scene against
the oracle's two-level hits, tracers initialised before the rebuild, a sequence that alternates the two builders with a refit and a deformation, node-set edits, and
the refusals.  Cases: tests/flat_ploc_cases.py.

Order inside every test, as in tests/test_gpu_flat_rebuild.py: the device tree is read back and validated on the host (check_topology) BEFORE a ray is traced through it."""
import ctypes as C

import numpy as np
import pytest

from cudatracerlib_amd import api
from scene_update_cases import build, rays_for_update
from scene_deform_cases import build_deformed_and_moved
from flat_rebuild_cases import moved_nodes
from flat_ploc_cases import CASES, IDS, old_scene, new_scene
import node_set_cases as nsc
from test_gpu_flat_rebuild import validated, same_rebuilt_tree, check_hits
from test_gpu_scene_deform import same_tree, tracers, render, assert_bit_equal, W, H
import test_gpu_node_set as gns

pytestmark = pytest.mark.gpu
N_RAYS = 4000


@pytest.mark.parametrize("case,pose", CASES, ids=IDS)
def test_device_ploc_equals_the_host_twin(gpu, orc, case, pose):
    old, new = old_scene(case), new_scene(case, pose)
    s = gpu.Scene(old.desc, flatten=True)
    s.update(new.desc)
    st = s.rebuild_flat(builder="ploc")
    dev = validated(s)
    host = api.FlatBvh(old.desc).rebuild(new.desc, builder="ploc")
    host_rounds = int(api.lib.ctl_rebuild_last_rounds())
    same_rebuilt_tree(dev, host)
    assert st["n_nodes"] == len(host.nodes()) and st["n_entries"] == len(host.leaves()) and st["max_depth"] == host.desc.max_depth and st["levels"] == st["max_depth"] + 1
    assert st["rounds"] == host_rounds and (host_rounds > 0) == (len(host.leaves()) > 1)
    assert st["node_area_before"] > 0 and st["node_area_after"] > 0 and st["total_ms"] > 0 and st["topology_ms"] > 0
    print("%s %s: %d nodes, %d entries, depth %d, %d rounds; node area %.6g -> %.6g; sort %.3f ms, topology %.3f ms, boxes %.3f ms, total %.3f ms"
          % (case, pose, st["n_nodes"], st["n_entries"], st["max_depth"], st["rounds"], st["node_area_before"], st["node_area_after"], st["sort_ms"], st["topology_ms"], st["refit_ms"], st["total_ms"]))
    check_hits(gpu, orc, s, new.desc, rays_for_update(new.desc, N_RAYS, 29, aim_nodes=moved_nodes(old.desc, new.desc)))


def test_tracers_initialised_before_a_ploc_rebuild_keep_working(gpu, orc):
    """S3 after update(M3) + a PLOC rebuild: every tracer that rendered the old tree renders the new one, its frame bit-equal to a freshly created scene's of that pose"""
    old, new = build("S3", width=W, height=H), build("S3", "M3", width=W, height=H)
    tables = orc.sequence_tables(2)
    for name, make, n_passes in tracers(gpu):
        s = gpu.Scene(old.desc, flatten=True)
        before, tr = render(gpu, make, s, tables, n_passes)
        s.update(new.desc)
        s.rebuild_flat(builder="ploc")
        validated(s)
        got, _ = render(gpu, make, s, tables, n_passes, tr=tr)
        want, _ = render(gpu, make, gpu.Scene(new.desc, flatten=True), tables, n_passes)
        assert_bit_equal(got, want, "%s after update(M3) + PLOC rebuild" % name)
        assert not np.array_equal(got, before), name


def test_a_sequence_that_alternates_the_builders(gpu, orc):
    """S3: update(M3), PLOC rebuild, update(M1) as a refit of the PLOC tree, LBVH rebuild, deform D1, PLOC rebuild — after each step the device tree equals the host
    handle driven the same way, and the hits are the oracle's"""
    plain, m3, m1, m1d1 = build("S3"), build("S3", "M3"), build("S3", "M1"), build_deformed_and_moved("D1", "S3", "M1")
    s = gpu.Scene(plain.desc, flatten=True)
    host = api.FlatBvh(plain.desc)

    def step(what, desc, rebuilt):
        dev = validated(s) if rebuilt else s.flat_bvh()
        (same_rebuilt_tree if rebuilt else same_tree)(dev, host)
        check_hits(gpu, orc, s, desc, rays_for_update(desc, N_RAYS, 37, aim_nodes=[2, 3]))
        print("sequence: %s ok" % what)
    assert s.update(m3.desc) & api.DIFF_TRANSFORMS; host.refit(m3.desc); step("update(M3)", m3.desc, False)
    s.rebuild_flat(builder="ploc"); host.rebuild(m3.desc, builder="ploc"); step("PLOC rebuild", m3.desc, True)
    assert s.update(m1.desc) & api.DIFF_TRANSFORMS; host.refit(m1.desc); step("update(M1)", m1.desc, True)
    s.rebuild_flat(); host.rebuild(m1.desc); step("LBVH rebuild", m1.desc, True)
    assert s.update(m1d1.desc) & api.DIFF_GEOMETRY; host.refit(m1d1.desc); step("deform D1", m1d1.desc, True)
    s.rebuild_flat(builder="ploc"); host.rebuild(m1d1.desc, builder="ploc"); step("second PLOC rebuild", m1d1.desc, True)


@pytest.mark.parametrize("case", ["N3", "N6"])
def test_node_sets_with_ploc(gpu, orc, case):
    """one removal and one addition: the device tree equals the host twin byte for byte, and the frames of tracers created before the call equal a fresh scene's"""
    old, new, m = gns.pair(case)
    s = gpu.Scene(old.desc, flatten=True)
    st = s.update_nodes(new.desc, builder="ploc")
    host = api.FlatBvh(old.desc).update_nodes(new.desc, m, builder="ploc")
    same_rebuilt_tree(gns.validated(s), host)
    assert st["rebuilt"] == 1 and st["entries_after"] == len(host.leaves()) and st["rebuild"]["n_nodes"] == len(host.nodes()) and st["rebuild"]["rounds"] > 0
    assert not np.array_equal(host.nodes(), api.FlatBvh(old.desc).update_nodes(new.desc, m).nodes())        # (it is another tree than the LBVH's)
    fresh = gpu.Scene(new.desc, flatten=True)
    gns.same_hits_as_fresh(gpu, s, fresh, new.desc, rays_for_update(new.desc, N_RAYS, 61, aim_nodes=list(np.nonzero(m == nsc.NONE)[0])), case)
    tables = orc.sequence_tables(2)
    for name, make, n_passes in tracers(gpu):
        s = gpu.Scene(old.desc, flatten=True)
        before, tr = gns.render(gpu, make, s, tables, n_passes)
        s.update_nodes(new.desc, m, builder="ploc")
        gns.validated(s)
        got, _ = gns.render(gpu, make, s, tables, n_passes, tr=tr)
        want, _ = gns.render(gpu, make, gpu.Scene(new.desc, flatten=True), tables, n_passes)
        assert_bit_equal(got, want, "%s %s" % (case, name))
        assert not np.array_equal(got, before), name


def test_refusals_leave_the_scene_as_it_was(gpu, orc):
    old = build("S3")
    rays = rays_for_update(old.desc, N_RAYS, 41)
    s = gpu.Scene(old.desc, flatten=True)
    a, before = gpu.intersect(s, rays), s.flat_bvh()                # (the arrays are views into the handle: it has to stay alive)
    st = api.ctl_scene_rebuild_stats()
    for bad in (2, -1):
        assert api.lib.ctl_scene_rebuild_flat_ex(s._h, bad, C.addressof(st)) == api.ERR_INVALID and b"unknown builder" in api.lib.ctl_last_error()
        with pytest.raises(api.CtlError) as e:
            s.rebuild_flat(builder=bad)
        assert e.value.code == api.ERR_INVALID
    o, n, m = gns.pair("N3")
    ns = gpu.Scene(o.desc, flatten=True)
    nb = ns.flat_bvh()
    with pytest.raises(api.CtlError) as e:
        ns.update_nodes(n.desc, m, builder=9)
    assert e.value.code == api.ERR_INVALID
    na = ns.flat_bvh()
    assert np.array_equal(na.nodes(), nb.nodes()) and np.array_equal(na.leaves(), nb.leaves())
    after = s.flat_bvh()
    assert np.array_equal(after.nodes(), before.nodes()) and np.array_equal(after.leaves(), before.leaves())
    assert np.array_equal(gpu.intersect(s, rays).view(np.uint8), a.view(np.uint8))
    two_level = gpu.Scene(old.desc)
    a = gpu.intersect(two_level, rays)
    with pytest.raises(api.CtlError) as e:
        two_level.rebuild_flat(builder="ploc")
    assert e.value.code == api.ERR_UNSUPPORTED
    assert np.array_equal(gpu.intersect(two_level, rays).view(np.uint8), a.view(np.uint8))
    q8 = gpu.Scene(old.desc, flatten=True, flat_format="q8")
    a, before = gpu.intersect(q8, rays), q8.flat_bvh()
    with pytest.raises(api.CtlError) as e:
        q8.rebuild_flat(builder="ploc")
    assert e.value.code == api.ERR_UNSUPPORTED
    after = q8.flat_bvh()
    assert np.array_equal(after.nodes(), before.nodes()) and np.array_equal(after.leaves(), before.leaves())
    assert np.array_equal(gpu.intersect(q8, rays).view(np.uint8), a.view(np.uint8))
