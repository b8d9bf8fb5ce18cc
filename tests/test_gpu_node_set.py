"""ctl_scene_update_nodes on the device: the tree after a change of the node set against the host yardstick (ctl_flat_bvh_update_nodes) byte for byte — nodes,
entries, part_index, level lists, depth —, hits and frames against a scene freshly created from the new description, the two-level path, follow-up updates, a bound
mesh, tracers that were initialised before the call, and the refusals.  Cases: tests/node_set_cases.py.

Order inside every test (as in test_gpu_flat_rebuild.py): the device tree is read back and validated on the host (flat_rebuild_cases.check_topology: every link the
traversal kernel would derive stays inside the arrays) BEFORE any ray is traced through it."""
import numpy as np
import pytest

from cudatracerlib_amd import api
from flat_rebuild_cases import check_topology
from node_set_cases import CASES, NONE, LONG, T4, old_scene, new_scene, old_of_new, undone_scene
from scene_update_cases import build, rays_for_update, assert_same_hits
from scene_deform_cases import mesh_arrays, nodes_of
from skin_cases import make_case, bind, animate, same_bits
from test_gpu_flat_rebuild import same_rebuilt_tree
from test_gpu_scene_deform import same_tree, tracers, assert_bit_equal

pytestmark = pytest.mark.gpu
N_RAYS = 4000
W = H = 32
_cache = {}


def pair(case):
    if case not in _cache:
        old, new = old_scene(case, W, H), new_scene(case, W, H)
        _cache[case] = (old, new, old_of_new(old, new))
    return _cache[case]


def render(gpu, make, scene, tables, n_passes, tr=None, max_len=5):
    """test_gpu_scene_deform.render at this file's frame size"""
    if tr is None:
        tr = make()
        tr.getParameters().setValue("MaxPathLength", max_len)
        tr.Resize(W, H); tr.InitializeScene(scene)
    img = gpu.Image(W, H)
    for k in range(n_passes):
        tr.setSamplerTables(*tables[k])
        tr.DoPass(img, new_trace=(k == 0))
    return img.getPixelData(), tr


def validated(scene, rebuilt=True):
    dev = scene.flat_bvh()
    if rebuilt:
        check_topology(dev)
    return dev


def same_hits_as_fresh(gpu, s, fresh, desc, rays, what):
    """closest hits bit for bit (no two surfaces of these scenes coincide: the helper's tie allowance must stay unused), occlusion flags"""
    got, want = gpu.intersect(s, rays), gpu.intersect(fresh, rays)
    assert assert_same_hits(got, want, what) == 0, what + ": a hit tie"
    assert (want["tri_idx"] >= 0).any()
    assert np.array_equal(gpu.intersect(s, rays, any_hit=True)["tri_idx"] >= 0, gpu.intersect(fresh, rays, any_hit=True)["tri_idx"] >= 0), what


@pytest.mark.parametrize("case", CASES)
def test_device_tree_equals_the_yardstick(gpu, case):
    old, new, m = pair(case)
    s = gpu.Scene(old.desc, flatten=True)
    host = api.FlatBvh(old.desc)
    st = s.update_nodes(new.desc)                      # the map from the descriptions' node ids
    host.update_nodes(new.desc, m)                     # (N10: nothing differs, so neither side touches its tree)
    dev = validated(s, rebuilt=case != "N10")
    if case == "N10":
        same_tree(dev, host); assert st["rebuilt"] == 0 and st["entries_after"] == st["entries_before"] == len(host.leaves())
    else:
        same_rebuilt_tree(dev, host)
        assert st["rebuilt"] == 1 and st["entries_after"] == len(host.leaves()) and st["entries_before"] == api.FlatBvh(old.desc).desc.n_leaves
        assert st["entries_after"] == st["entries_before"] - st["entries_dropped"] + st["entries_generated"]
        assert st["degenerate_skipped"] == (1 if case == "N8" else 0)
        assert st["rebuild"]["n_nodes"] == len(host.nodes()) and st["rebuild"]["max_depth"] == host.desc.max_depth and st["total_ms"] >= st["edit_ms"] > 0
    print("%s: %d -> %d entries (-%d +%d, %d degenerate); edit %.3f ms, rebuild %.3f ms, total %.3f ms" % (case, st["entries_before"], st["entries_after"], st["entries_dropped"],
          st["entries_generated"], st["degenerate_skipped"], st["edit_ms"], st["rebuild"]["total_ms"], st["total_ms"]))
    fresh = gpu.Scene(new.desc, flatten=True)
    same_hits_as_fresh(gpu, s, fresh, new.desc, rays_for_update(new.desc, N_RAYS, 61, aim_nodes=list(np.nonzero(m == NONE)[0])), case)


@pytest.mark.parametrize("case", CASES)
def test_frames_equal_a_fresh_scene(gpu, orc, case):
    """every tracer, created and used BEFORE the call, renders the new scene after it (new_trace), every pixel bit-equal to a freshly created scene's, same sampler tables"""
    old, new, m = pair(case)
    tables = orc.sequence_tables(2)
    for name, make, n_passes in tracers(gpu):
        s = gpu.Scene(old.desc, flatten=True)
        before, tr = render(gpu, make, s, tables, n_passes)
        s.update_nodes(new.desc, m)
        validated(s, rebuilt=case != "N10")
        got, _ = render(gpu, make, s, tables, n_passes, tr=tr)
        want, _ = render(gpu, make, gpu.Scene(new.desc, flatten=True), tables, n_passes)
        assert_bit_equal(got, want, "%s %s" % (case, name))
        if case != "N10":
            assert not np.array_equal(got, before), name


@pytest.mark.parametrize("case", ["N3", "N6", "N7"])
def test_two_level_scene(gpu, orc, case):
    """host work only: top level, instances, node info and materials in buffers of the new size; hits and the WavefrontPathTracer's frame (the tracer that takes a
    two-level scene) equal a fresh scene's"""
    old, new, m = pair(case)
    s = gpu.Scene(old.desc)
    tables = orc.sequence_tables(2)
    before, tr = render(gpu, gpu.WavefrontPathTracer, s, tables, 2)
    st = s.update_nodes(new.desc, m)
    assert st["rebuilt"] == 0
    fresh = gpu.Scene(new.desc)
    same_hits_as_fresh(gpu, s, fresh, new.desc, rays_for_update(new.desc, N_RAYS, 67, aim_nodes=list(np.nonzero(m == NONE)[0])), case + " two-level")
    got, _ = render(gpu, gpu.WavefrontPathTracer, s, tables, 2, tr=tr)
    want, _ = render(gpu, gpu.WavefrontPathTracer, fresh, tables, 2)
    assert_bit_equal(got, want, case + " two-level")
    assert not np.array_equal(got, before)


def test_follow_ups_on_the_updated_scene(gpu, orc):
    """after N7: a transform update (the refit against ctl_flat_bvh_refit), a rebuild, and a second node-set change that undoes the first (hits equal to the original
    scene's, the two re-created nodes being the last ones now)"""
    old, new, m = pair("N7")
    moved = new_scene("N9", W, H)                        # N7's node set with node T4 moved, a material edited and another camera
    s = gpu.Scene(old.desc, flatten=True); host = api.FlatBvh(old.desc)
    s.update_nodes(new.desc, m); host.update_nodes(new.desc, m)
    mask = s.update(moved.desc); host.refit(moved.desc)
    assert mask & api.DIFF_TRANSFORMS and not mask & api.DIFF_TOPOLOGY
    same_rebuilt_tree(validated(s), host)
    same_hits_as_fresh(gpu, s, gpu.Scene(moved.desc, flatten=True), moved.desc, rays_for_update(moved.desc, N_RAYS, 71, aim_nodes=[T4]), "update after update_nodes")
    s.rebuild_flat(); host.rebuild(moved.desc)
    same_rebuilt_tree(validated(s), host)
    undone, orig = undone_scene(W, H)
    m2 = old_of_new(moved, undone)
    s.update_nodes(undone.desc, m2); host.update_nodes(undone.desc, m2)
    same_rebuilt_tree(validated(s), host)
    rays = rays_for_update(old.desc, N_RAYS, 73, aim_nodes=[LONG])
    got, want = gpu.intersect(s, rays), gpu.intersect(gpu.Scene(old.desc, flatten=True), rays)
    hit = got["node_idx"] >= 0
    got["node_idx"][hit] = orig[got["node_idx"][hit]]
    assert assert_same_hits(got, want, "undone") == 0


def test_bound_mesh(gpu):
    """bind, pose, add an instance of the bound mesh, pose again: the new instance takes the pose in HBM, the binding survives, the next pose moves all instances"""
    K = make_case("K3-0.37")
    plain, mesh = K["plain"], K["mesh"]
    xf = np.array([[45, 0, 0, 250.0], [0, 45, 0, 420.0], [0, 0, 45, 200.0], [0, 0, 0, 1]], np.float32)
    more = build(K["scene"], width=K["width"], height=K["height"], edit=lambda sc: sc.CreateNode(mesh, xf))
    added = more.desc.n_nodes - 1
    s = gpu.Scene(plain.desc, flatten=True)
    bind(s, K); animate(s, K)
    Y1 = api.skin_mesh_host(plain.desc, mesh, K["P"], K["I"], K["BI"], K["BW"], K["n_bones"], K["B0"], K["B1"], K["lerp"], rest_normals=K["N"], n_rows=K["n_rows"])
    st = s.update_nodes(more.desc)
    assert st["entries_generated"] == K["n_tri"] and st["degenerate_skipped"] == 0
    A = mesh_arrays(plain.desc, mesh)
    first_row = {}
    for w in range(len(A["widx"]) - 1, -1, -1):
        first_row[int(A["widx"][w] >> 1)] = w
    t0 = A["tri_range"][0]

    def check(Y, nodes, what):
        dev = validated(s)
        L = dev.leaves()
        for k in nodes:
            mine = L[L[:, 13] == k]
            assert len(mine) == K["n_tri"], what
            rows = np.array([first_row[int(t) - t0] for t in mine[:, 12] >> 1])
            assert same_bits(mine[:, :12], Y["woop"][rows]), "%s: node %d's entries are not the yardstick's rows" % (what, k)
    check(Y1, [added], "the added instance")
    st2 = s.animate_mesh(mesh, K["B0"], K["B1"], 0.8)
    Y2 = api.skin_mesh_host(plain.desc, mesh, K["P"], K["I"], K["BI"], K["BW"], K["n_bones"], K["B0"], K["B1"], 0.8, rest_normals=K["N"], n_rows=K["n_rows"])
    assert st2["refit_levels"] >= 1 and not same_bits(Y1["woop"], Y2["woop"])
    check(Y2, nodes_of(more.desc, mesh), "the second pose")
    assert added in nodes_of(more.desc, mesh) and len(nodes_of(more.desc, mesh)) == 3


def tree_bytes(scene):
    fb = scene.flat_bvh()
    return fb.nodes().copy(), fb.leaves().copy(), fb.parts()[0].copy()


def test_refusals_leave_the_scene_as_it_was(gpu):
    old, new, m = pair("N7")
    rays = rays_for_update(old.desc, N_RAYS, 79)
    s = gpu.Scene(old.desc, flatten=True)
    before, hits = tree_bytes(s), gpu.intersect(s, rays)
    bad_map = m.copy(); bad_map[1], bad_map[2] = m[2], m[1]
    other_mesh = m.copy(); other_mesh[3] = LONG
    d = api.ctl_scene_desc.from_buffer_copy(new.desc)
    woop = new.desc.view("woop", np.float32, new.desc.n_woop, 12).copy(); woop[0, 3] += 0.25
    d.woop = woop.ctypes.data; d.node_ids = new.desc.node_ids
    for desc, mm, code in ((new.desc, m[:-1], api.ERR_INVALID), (new.desc, bad_map, api.ERR_INVALID), (new.desc, other_mesh, api.ERR_INVALID), (d, m, api.ERR_INVALID)):
        with pytest.raises(api.CtlError) as e:
            s.update_nodes(desc, mm)
        assert e.value.code == code, str(e.value)
        after = tree_bytes(s)
        assert all(np.array_equal(a, b) for a, b in zip(after, before)), "a refusal changed the tree"
        assert np.array_equal(gpu.intersect(s, rays).view(np.uint8), hits.view(np.uint8))
    q8 = gpu.Scene(old.desc, flatten=True, flat_format="q8")
    fb = q8.flat_bvh(); nodes, leaves = fb.nodes().copy(), fb.leaves().copy(); hits8 = gpu.intersect(q8, rays)
    with pytest.raises(api.CtlError) as e:
        q8.update_nodes(new.desc, m)
    assert e.value.code == api.ERR_UNSUPPORTED
    fb = q8.flat_bvh()
    assert np.array_equal(fb.nodes(), nodes) and np.array_equal(fb.leaves(), leaves) and np.array_equal(gpu.intersect(q8, rays).view(np.uint8), hits8.view(np.uint8))
    # ctl_scene_update keeps refusing the same description
    with pytest.raises(api.CtlError) as e:
        s.update(new.desc)
    assert e.value.code == api.ERR_INVALID and s.last_mask & api.DIFF_TOPOLOGY
    # ... and after all that the scene takes the change
    s.update_nodes(new.desc, m)
    same_rebuilt_tree(validated(s), api.FlatBvh(old.desc).update_nodes(new.desc, m))


def test_a_refused_update_nodes_leaves_nothing_behind(gpu):
    """a refused update_nodes keeps no state for a later call: rebuild_flat() on the same thread right after it REBUILDS — rebuild stats over the entries the scene had,
    the tree of the host rebuild of the same description — and the next update_nodes is still its yardstick's (N7: the case and the refused map of the test above)"""
    old, new, m = pair("N7")
    s = gpu.Scene(old.desc, flatten=True); host = api.FlatBvh(old.desc)
    n_before = len(host.leaves())
    other_mesh = m.copy(); other_mesh[3] = LONG          # a node of a mesh the scene does not hold at that place
    with pytest.raises(api.CtlError) as e:
        s.update_nodes(new.desc, other_mesh)
    assert e.value.code == api.ERR_INVALID, str(e.value)
    st = s.rebuild_flat(); host.rebuild(old.desc)
    assert set(st) >= {"n_nodes", "n_entries", "max_depth", "levels", "sort_ms", "topology_ms"} and "entries_after" not in st
    assert st["n_entries"] == n_before == len(host.leaves()) and st["n_nodes"] == len(host.nodes())
    same_rebuilt_tree(validated(s), host)
    st2 = s.update_nodes(new.desc, m); host.update_nodes(new.desc, m)
    assert st2["rebuilt"] == 1 and st2["entries_before"] == n_before and st2["entries_after"] == len(host.leaves())
    same_rebuilt_tree(validated(s), host)
