"""ctl_scene_rebuild_flat on the device: the rebuilt tree against the host rebuild (ctl_flat_bvh_rebuild) byte for byte — nodes, entries, part_index, level lists,
depth —, the traversal of the rebuilt scene against the oracle's two-level hits, tracers that were initialised before the rebuild, a sequence of updates, deformations,
rebuilds and a skin pose, and the refusals.  Cases: tests/flat_rebuild_cases.py.

Order inside every test: the device tree is read back and validated on the host (flat_rebuild_cases.check_topology: every link the traversal kernel would derive stays
inside the arrays) BEFORE any ray is traced through it; a malformed tree is a failed assertion, not a traversal through bad links."""
import numpy as np
import pytest

from cudatracerlib_amd import api
from scene_update_cases import build, rays_for_update
from scene_deform_cases import build_deformed_and_moved
from flat_rebuild_cases import CASES, IDS, old_scene, new_scene, moved_nodes, check_topology
from skin_cases import make_case, yardstick, host_updated, bind, animate
from test_gpu_skin import same_tree
from test_gpu_scene_deform import tracers, render, assert_bit_equal, W, H

pytestmark = pytest.mark.gpu
N_RAYS = 4000


def validated(scene):
    """the device tree read back and checked before anything is traced through it"""
    dev = scene.flat_bvh()
    check_topology(dev)
    return dev


def same_rebuilt_tree(dev, host):
    same_tree(dev, host)                                          # nodes, entries, part_index and clip boxes
    assert np.array_equal(dev.child_links(), host.child_links())
    assert dev.desc.max_depth == host.desc.max_depth and dev.desc.root_slab == 0 and dev.desc.n_slab_nodes == 0
    for a, b in zip(dev.levels(), host.levels()):
        assert np.array_equal(a, b), "level lists"


def check_hits(gpu, orc, scene, desc, rays):
    """ctl_intersect against the oracle's restatement of the reference's TWO-LEVEL traversal, bit for bit, verified ties only; any-hit: occlusion agrees"""
    got, want = gpu.intersect(scene, rays), orc.intersect(desc, rays)
    for k in ("tri_idx", "node_idx"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert all(got["dist"][i] == want["dist"][i] and got["tri_idx"][i] >= 0 and want["tri_idx"][i] >= 0 for i in bad), (k, bad[:10])
        assert len(bad) <= max(4, len(rays) // 1000)
    same = got["tri_idx"] == want["tri_idx"]
    for k in ("dist", "u", "v"):
        assert np.array_equal(got[k][same].view(np.uint32), want[k][same].view(np.uint32)), k
    assert (want["tri_idx"] >= 0).any()
    assert np.array_equal(gpu.intersect(scene, rays, any_hit=True)["tri_idx"] >= 0, orc.intersect(desc, rays, any_hit=True)["tri_idx"] >= 0)


@pytest.mark.parametrize("case,pose", CASES, ids=IDS)
def test_device_rebuild_equals_the_host_rebuild(gpu, orc, case, pose):
    old, new = old_scene(case), new_scene(case, pose)
    s = gpu.Scene(old.desc, flatten=True)
    s.update(new.desc)
    st = s.rebuild_flat()
    dev = validated(s)
    host = api.FlatBvh(old.desc).rebuild(new.desc)
    same_rebuilt_tree(dev, host)
    assert st["n_nodes"] == len(host.nodes()) and st["n_entries"] == len(host.leaves()) and st["max_depth"] == host.desc.max_depth and st["levels"] == st["max_depth"] + 1
    assert st["node_area_before"] > 0 and st["node_area_after"] > 0 and st["total_ms"] > 0
    print("%s %s: %d nodes, %d entries, depth %d; node area %.6g -> %.6g; sort %.3f ms, topology %.3f ms, boxes %.3f ms, total %.3f ms"
          % (case, pose, st["n_nodes"], st["n_entries"], st["max_depth"], st["node_area_before"], st["node_area_after"], st["sort_ms"], st["topology_ms"], st["refit_ms"], st["total_ms"]))
    check_hits(gpu, orc, s, new.desc, rays_for_update(new.desc, N_RAYS, 29, aim_nodes=moved_nodes(old.desc, new.desc)))


def test_tracers_initialised_before_the_rebuild_keep_working(gpu, orc):
    """S3 after update(M3) + rebuild: every tracer that rendered the old tree renders the new one, and its frame is the frame of a freshly created scene of that pose,
    bit for bit — the tree only culls, and the traversal reports the closest hit whatever the topology (S3 under M3 has no two triangles at the same distance along a
    camera path, which is what the refit tests of the same scene rely on too)"""
    old, new = build("S3", width=W, height=H), build("S3", "M3", width=W, height=H)
    tables = orc.sequence_tables(2)
    for name, make, n_passes in tracers(gpu):
        s = gpu.Scene(old.desc, flatten=True)
        before, tr = render(gpu, make, s, tables, n_passes)
        s.update(new.desc)
        s.rebuild_flat()
        validated(s)
        got, _ = render(gpu, make, s, tables, n_passes, tr=tr)
        want, _ = render(gpu, make, gpu.Scene(new.desc, flatten=True), tables, n_passes)
        assert_bit_equal(got, want, "%s after update(M3) + rebuild" % name)
        assert not np.array_equal(got, before), name


def test_a_sequence_of_updates_rebuilds_and_a_pose(gpu, orc):
    """update(M3) -> rebuild -> update(M1) -> deform D1 -> rebuild -> a skin pose, on S3: after each step the device tree equals the host handle driven the same way,
    and the hits are the oracle's"""
    K = make_case("K3-0.37")                                       # S3, the ball mesh (nodes 2 and 3) under two bones
    Y = yardstick(K)
    plain, m3, m1 = K["plain"], build("S3", "M3"), build("S3", "M1")
    m1d1 = build_deformed_and_moved("D1", "S3", "M1")
    from scene_update_cases import motion_of

    def move_m1(sc):
        for node, xf in motion_of("S3", "M1", sc.desc).items():
            sc.SetNodeTransform(node, xf)
    posed = host_updated(K, Y, edit=move_m1)                      # the pose on top of M1's transforms
    s = gpu.Scene(plain.desc, flatten=True)
    host = api.FlatBvh(plain.desc)

    def step(what, desc, rebuilt):
        dev = validated(s) if rebuilt else s.flat_bvh()
        if rebuilt:
            same_rebuilt_tree(dev, host)
        else:
            same_tree(dev, host)
        check_hits(gpu, orc, s, desc, rays_for_update(desc, N_RAYS, 37, aim_nodes=[2, 3]))
        print("sequence: %s ok" % what)
    assert s.update(m3.desc) & api.DIFF_TRANSFORMS; host.refit(m3.desc); step("update(M3)", m3.desc, False)
    s.rebuild_flat(); host.rebuild(m3.desc); step("rebuild", m3.desc, True)
    assert s.update(m1.desc) & api.DIFF_TRANSFORMS; host.refit(m1.desc); step("update(M1)", m1.desc, True)
    assert s.update(m1d1.desc) & api.DIFF_GEOMETRY; host.refit(m1d1.desc); step("deform D1", m1d1.desc, True)
    s.rebuild_flat(); host.rebuild(m1d1.desc); step("second rebuild", m1d1.desc, True)
    bind(s, K); animate(s, K); host.refit(posed.desc); step("skin pose", posed.desc, True)


def test_refusals_leave_the_scene_as_it_was(gpu, orc):
    old = build("S3")
    rays = rays_for_update(old.desc, N_RAYS, 41)
    two_level = gpu.Scene(old.desc)
    a = gpu.intersect(two_level, rays)
    with pytest.raises(api.CtlError) as e:
        two_level.rebuild_flat()
    assert e.value.code == api.ERR_UNSUPPORTED
    assert np.array_equal(gpu.intersect(two_level, rays).view(np.uint8), a.view(np.uint8))
    q8 = gpu.Scene(old.desc, flatten=True, flat_format="q8")
    a, before = gpu.intersect(q8, rays), q8.flat_bvh()            # (the arrays are views into the handle: it has to stay alive)
    with pytest.raises(api.CtlError) as e:
        q8.rebuild_flat()
    assert e.value.code == api.ERR_UNSUPPORTED
    after = q8.flat_bvh()
    assert np.array_equal(after.nodes(), before.nodes()) and np.array_equal(after.leaves(), before.leaves())
    assert np.array_equal(gpu.intersect(q8, rays).view(np.uint8), a.view(np.uint8))
