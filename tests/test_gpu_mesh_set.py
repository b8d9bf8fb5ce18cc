"""ctl_scene_update_meshes on the device: the tree after meshes were appended against the host yardstick (ctl_flat_bvh_update_meshes) byte for byte, hits and frames
against a scene freshly created from the new description, the two-level path, follow-up updates that run through the appended ranges of the geometry arrays and of the
triangle -> row table, bound meshes, tracers that were initialised before the call, and the refusals.  Cases: tests/mesh_set_cases.py.

Order inside every test (as in test_gpu_node_set.py): the device tree is read back and validated on the host (flat_rebuild_cases.check_topology) BEFORE any ray is traced
through it."""
import numpy as np
import pytest

from cudatracerlib_amd import api
from flat_rebuild_cases import check_topology
from node_set_cases import NONE, old_of_new, soup
from mesh_set_cases import CASES, descriptions, replay, place, big, split_mesh
from scene_update_cases import rays_for_update, assert_same_hits
from skin_cases import same_bits
from test_gpu_flat_rebuild import same_rebuilt_tree
from test_gpu_scene_deform import tracers, assert_bit_equal
from test_gpu_node_set import render, validated, same_hits_as_fresh, tree_bytes

pytestmark = pytest.mark.gpu
N_RAYS = 4000
W = H = 32
_cache = {}


def chain(case):
    if case not in _cache:
        seq = descriptions(case, W, H)
        _cache[case] = (seq, [old_of_new(a, b) for a, b in zip(seq, seq[1:])])
    return _cache[case]


def updated(gpu, case, builder="lbvh", flatten=True):
    """(the scene created from the case's first description and updated through the others, the yardstick handle, the stats of every call)"""
    seq, maps = chain(case)
    s = gpu.Scene(seq[0].desc, flatten=flatten)
    host = api.FlatBvh(seq[0].desc) if flatten else None
    stats = []
    for new, m in zip(seq[1:], maps):
        stats.append(s.update_meshes(new.desc, builder=builder) if builder == "lbvh" else s.update_meshes(new.desc, m, builder=builder))      # the map from the node ids / given
        if host is not None:
            host.update_meshes(new.desc, m, builder=builder)
    return s, host, stats


@pytest.mark.parametrize("case,builder", [(c, "lbvh") for c in CASES] + [("M2", "ploc")])
def test_device_tree_equals_the_yardstick(gpu, case, builder):
    seq, maps = chain(case)
    s, host, stats = updated(gpu, case, builder)
    same_rebuilt_tree(validated(s), host)
    for old, new, st in zip(seq, seq[1:], stats):
        n = st["nodes"]
        assert st["meshes_added"] == new.desc.n_meshes - old.desc.n_meshes and st["triangles_added"] == new.desc.n_tri_data - old.desc.n_tri_data
        assert st["rows_added"] == new.desc.n_woop - old.desc.n_woop and st["bvh_nodes_added"] == new.desc.n_bvh_nodes - old.desc.n_bvh_nodes
        assert n["rebuilt"] == 1 and n["entries_after"] == n["entries_before"] - n["entries_dropped"] + n["entries_generated"]
        assert (st["append_ms"] > 0 and st["hash_ms"] > 0) if case != "M7" else (st["append_ms"] == 0 and st["meshes_added"] == 0)
        assert n["degenerate_skipped"] == (1 if case in ("M3", "M6") and new is seq[-1] else 0)
        print("%s %s: +%d meshes, +%d triangles, +%d rows; append %.3f ms, hash %.3f ms, node-set stages %.3f ms" % (case, builder, st["meshes_added"], st["triangles_added"], st["rows_added"],
              st["append_ms"], st["hash_ms"], n["total_ms"]))
    assert stats[-1]["nodes"]["entries_after"] == len(host.leaves())
    new, m = seq[-1], maps[-1]
    fresh = gpu.Scene(new.desc, flatten=True)
    same_hits_as_fresh(gpu, s, fresh, new.desc, rays_for_update(new.desc, N_RAYS, 61, aim_nodes=list(np.nonzero(m == NONE)[0])), case)


@pytest.mark.parametrize("case", CASES)
def test_frames_equal_a_fresh_scene(gpu, orc, case):
    """every tracer, created and used BEFORE the call, renders the new scene after it (new_trace), every pixel bit-equal to a freshly created scene's, same sampler
    tables — M5: the new mesh's conductor and its area light included"""
    seq, maps = chain(case)
    tables = orc.sequence_tables(2)
    for name, make, n_passes in tracers(gpu):
        s = gpu.Scene(seq[0].desc, flatten=True)
        before, tr = render(gpu, make, s, tables, n_passes)
        for new, m in zip(seq[1:], maps):
            s.update_meshes(new.desc, m)
        validated(s)
        got, _ = render(gpu, make, s, tables, n_passes, tr=tr)
        want, _ = render(gpu, make, gpu.Scene(seq[-1].desc, flatten=True), tables, n_passes)
        assert_bit_equal(got, want, "%s %s" % (case, name))
        assert not np.array_equal(got, before), name
    if case == "M5":
        assert seq[-1].desc.n_lights_buf == seq[0].desc.n_lights_buf + 1, "the new node's area light"


@pytest.mark.parametrize("case", CASES)
def test_two_level_scene(gpu, orc, case):
    """no tree to rebuild: the grown two-level arrays and the host-side tables; hits and the WavefrontPathTracer's frame equal a fresh scene's"""
    seq, maps = chain(case)
    s = gpu.Scene(seq[0].desc)
    tables = orc.sequence_tables(2)
    before, tr = render(gpu, gpu.WavefrontPathTracer, s, tables, 2)
    old = seq[0]
    for new, m in zip(seq[1:], maps):
        st = s.update_meshes(new.desc, m)
        assert st["nodes"]["rebuilt"] == 0 and st["meshes_added"] == (0 if case == "M7" else new.desc.n_meshes - old.desc.n_meshes) and (case == "M7" or st["meshes_added"] > 0)
        old = new
    new, m = seq[-1], maps[-1]
    fresh = gpu.Scene(new.desc)
    same_hits_as_fresh(gpu, s, fresh, new.desc, rays_for_update(new.desc, N_RAYS, 67, aim_nodes=list(np.nonzero(m == NONE)[0])), case + " two-level")
    got, _ = render(gpu, gpu.WavefrontPathTracer, s, tables, 2, tr=tr)
    want, _ = render(gpu, gpu.WavefrontPathTracer, fresh, tables, 2)
    assert_bit_equal(got, want, case + " two-level")
    assert not np.array_equal(got, before)


@pytest.mark.parametrize("case", ["M3", "M6"])
def test_follow_ups_on_the_updated_scene(gpu, case):
    """after the append: a node of an appended mesh moved (the refit against ctl_flat_bvh_refit); the appended mesh with duplicate rows deformed (k_deform_entries through
    the appended range of the triangle -> row table — M6's table was extended on the device by its second call —, against the host refit); a rebuild; then an
    update_nodes that removes the new nodes again: hits equal the original scene's"""
    seq, maps = chain(case)
    n_steps = len(seq) - 1
    s, host, _ = updated(gpu, case)
    long2 = seq[-1].desc.n_meshes - 2
    node_long2 = seq[-1].desc.n_nodes - 2
    assert int(seq[-1].desc.view("nodes", np.uint32, seq[-1].desc.n_nodes, 6)[node_long2, 0]) == long2

    def move(sc, m, a):
        sc.SetNodeTransform(node_long2, place(23))
    moved = replay(case, n_steps, W, H, then=move)
    mask = s.update(moved.desc); host.refit(moved.desc)
    assert mask & api.DIFF_TRANSFORMS and not mask & (api.DIFF_TOPOLOGY | api.DIFF_GEOMETRY)
    same_rebuilt_tree(validated(s), host)
    same_hits_as_fresh(gpu, s, gpu.Scene(moved.desc, flatten=True), moved.desc, rays_for_update(moved.desc, N_RAYS, 71, aim_nodes=[node_long2]), "an appended mesh's node moved")

    def bend(sc, m, a):
        move(sc, m, a)
        P, I = split_mesh()
        P = P.copy(); P[:, 1] += 0.25 * np.sin(2.0 * P[:, 0]); P[:, 2] *= 1.1
        sc.UpdateMesh(a["LONG2"], P, I)
    bent = replay(case, n_steps, W, H, then=bend)
    mask = s.update(bent.desc); host.refit(bent.desc)
    assert mask & api.DIFF_GEOMETRY and not mask & api.DIFF_TOPOLOGY
    same_rebuilt_tree(validated(s), host)
    same_hits_as_fresh(gpu, s, gpu.Scene(bent.desc, flatten=True), bent.desc, rays_for_update(bent.desc, N_RAYS, 73, aim_nodes=[node_long2]), "an appended mesh deformed")
    s.rebuild_flat(); host.rebuild(bent.desc)
    same_rebuilt_tree(validated(s), host)

    n_new = seq[-1].desc.n_nodes - seq[0].desc.n_nodes

    def remove(sc, m, a):
        bend(sc, m, a)
        for k in range(seq[-1].desc.n_nodes - 1, seq[0].desc.n_nodes - 1, -1):
            sc.DeleteNode(k)
    removed = replay(case, n_steps, W, H, then=remove)
    assert removed.desc.n_nodes == seq[0].desc.n_nodes and removed.desc.n_meshes == seq[-1].desc.n_meshes and n_new >= 2
    m2 = old_of_new(bent, removed)
    s.update_nodes(removed.desc, m2); host.update_nodes(removed.desc, m2)
    same_rebuilt_tree(validated(s), host)
    rays = rays_for_update(seq[0].desc, N_RAYS, 79)
    got, want = gpu.intersect(s, rays), gpu.intersect(gpu.Scene(seq[0].desc, flatten=True), rays)
    assert assert_same_hits(got, want, "the new nodes removed again") == 0


@pytest.mark.parametrize("case", ["M2", "M3", "M3-bound", "M6"])
def test_device_table_is_triangle_woop_rows(gpu, case):
    """the triangle -> row table in HBM after the call equals triangle_woop_rows(new) on both routes: made on the host where the scene had none (M2, M3, M6's first
    call), extended by k_append_leaf_rows where it had one — M6's second call, and M3 on a scene whose table a skin binding made first.  M3 / M6 append the mesh
    with several rows per triangle: whichever lane arrives first, the first row in stream order stays"""
    name = case.split("-")[0]
    seq, maps = chain(name)
    s = gpu.Scene(seq[0].desc, flatten=True)
    assert s.triangle_rows() is None
    if case == "M3-bound":
        P, I = soup(65, 11 + 5); BI, BW = one_bone_skin(P)
        s.bind_skin(6, P, I, BI, BW, 2)                      # T65: the binding makes the table from the index words in HBM
        assert np.array_equal(s.triangle_rows(), api.triangle_woop_rows(seq[0].desc))
    for new, m in zip(seq[1:], maps):
        s.update_meshes(new.desc, m)
        validated(s)
        assert np.array_equal(s.triangle_rows(), api.triangle_woop_rows(new.desc)), case
    if name != "M2":
        long2 = seq[-1].desc.n_meshes - 2
        n_tri, n_rows = api.mesh_counts(seq[-1].desc)[long2]
        assert n_rows > n_tri


def one_bone_skin(P, n_bones=2):
    """every vertex follows bone 0 or bone 1 by its height: uint8 (n_vert, 8) indices and weights"""
    BI = np.zeros((len(P), 8), np.uint8); BW = np.zeros((len(P), 8), np.uint8)
    BI[:, 0] = (P[:, 1] > np.median(P[:, 1])).astype(np.uint8); BW[:, 0] = 255
    return BI, BW


def pose(angle, shift):
    c, s = np.cos(angle), np.sin(angle)
    A = np.array([[c, 0, s, shift], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], np.float32)
    B = np.array([[1, 0, 0, 0], [0, 1, 0, 0.5 * shift], [0, 0, 1, -shift], [0, 0, 0, 1]], np.float32)
    return np.stack([A, B])


def test_bound_meshes(gpu):
    """a mesh bound and posed before the call keeps its posed bytes through the growth copy, and its next pose still moves it; an APPENDED mesh can be bound and posed"""
    seq, maps = chain("M2")
    old, new, m = seq[0], seq[1], maps[0]
    t65 = 6                                                   # node_set_cases.base: floor, then SIZES in order: T65 is mesh 6
    P, I = soup(65, 11 + 5)
    assert api.mesh_counts(old.desc)[t65][0] == 65
    BI, BW = one_bone_skin(P)
    s = gpu.Scene(old.desc, flatten=True)
    s.bind_skin(t65, P, I, BI, BW, 2)
    s.animate_mesh(t65, pose(0.2, 0.1))
    held = s.read_mesh_geometry(t65, vertices=True)
    s.update_meshes(new.desc, m)
    validated(s)
    after = s.read_mesh_geometry(t65, vertices=True)
    for k in ("tri", "woop", "positions", "normals"):
        assert np.array_equal(held[k].view(np.uint32), after[k].view(np.uint32)), "the posed mesh's %s changed in the growth copy" % k
    s.animate_mesh(t65, pose(-0.3, 0.2))
    Y = api.skin_mesh_host(new.desc, t65, P, I, BI, BW, 2, pose(-0.3, 0.2))
    G = s.read_mesh_geometry(t65)
    assert same_bits(G["woop"], Y["woop"]) and same_bits(G["tri"], Y["tri"]) and not same_bits(G["woop"], held["woop"]), "the next pose"
    # an appended mesh: A65, the third of the four
    a65 = old.desc.n_meshes + 2
    P2, I2 = soup(65, 212)
    assert api.mesh_counts(new.desc)[a65][0] == 65
    BI2, BW2 = one_bone_skin(P2)
    s.bind_skin(a65, P2, I2, BI2, BW2, 2)
    s.animate_mesh(a65, pose(0.25, -0.1))
    Y2 = api.skin_mesh_host(new.desc, a65, P2, I2, BI2, BW2, 2, pose(0.25, -0.1))
    G2 = s.read_mesh_geometry(a65)
    assert same_bits(G2["woop"], Y2["woop"]) and same_bits(G2["tri"], Y2["tri"]), "an appended mesh posed"
    validated(s, rebuilt=False)


def test_refusals_leave_the_scene_as_it_was(gpu):
    seq, maps = chain("M2")
    old, new, m = seq[0], seq[1], maps[0]
    rays = rays_for_update(old.desc, N_RAYS, 83)
    s = gpu.Scene(old.desc, flatten=True); host = api.FlatBvh(old.desc)
    before, hits = tree_bytes(s), gpu.intersect(s, rays)
    n_old = old.desc.n_meshes
    copy = lambda: api.ctl_scene_desc.from_buffer_copy(new.desc)
    M = lambda: new.desc.view("meshes", np.uint32, new.desc.n_meshes, 5).copy()
    keep = []
    d1 = copy(); a = M(); a[1, 4] += 1; d1.meshes = a.ctypes.data; keep.append(a)                               # a changed prefix mesh record
    d2 = copy(); a = M(); a[n_old, 0] = old.desc.n_tri_data - 1; d2.meshes = a.ctypes.data; keep.append(a)      # an appended mesh inside the old range
    d3 = copy(); d3.n_tri_data = old.desc.n_tri_data - 1                                                         # shrunken counts
    d4 = copy(); d4.n_images = new.desc.n_images + 1                                                             # another image count
    d5 = copy(); a = new.desc.view("woop", np.float32, new.desc.n_woop, 12).copy(); a[0, 3] += 0.25; d5.woop = a.ctypes.data; keep.append(a)      # changed values of an old mesh
    d6 = copy(); a = new.desc.view("nodes", np.uint32, new.desc.n_nodes, 6).copy(); a[-1, 0] = new.desc.n_meshes; d6.nodes = a.ctypes.data; keep.append(a)   # a missing mesh
    for k, desc in enumerate((d1, d2, d3, d4, d5, d6)):
        with pytest.raises(api.CtlError) as e:
            s.update_meshes(desc, m)
        assert e.value.code == api.ERR_INVALID, (k, str(e.value))
        assert all(np.array_equal(x, y) for x, y in zip(tree_bytes(s), before)), "refusal %d changed the tree" % k
        assert np.array_equal(gpu.intersect(s, rays).view(np.uint8), hits.view(np.uint8)), k
    q8 = gpu.Scene(old.desc, flatten=True, flat_format="q8")
    fb = q8.flat_bvh(); nodes, leaves = fb.nodes().copy(), fb.leaves().copy(); hits8 = gpu.intersect(q8, rays)
    with pytest.raises(api.CtlError) as e:
        q8.update_meshes(new.desc, m)
    assert e.value.code == api.ERR_UNSUPPORTED
    fb = q8.flat_bvh()
    assert np.array_equal(fb.nodes(), nodes) and np.array_equal(fb.leaves(), leaves) and np.array_equal(gpu.intersect(q8, rays).view(np.uint8), hits8.view(np.uint8))
    # the existing calls keep their answers to appended meshes
    seq1, maps1 = chain("M1")
    with pytest.raises(api.CtlError) as e:
        s.update_nodes(seq1[1].desc, maps1[0])
    assert e.value.code == api.ERR_INVALID and "the set of meshes differs: only meshes the scene already holds can be instanced; re-create the scene" in str(e.value)
    with pytest.raises(api.CtlError) as e:
        s.update(seq1[1].desc)
    assert e.value.code == api.ERR_INVALID and s.last_mask & api.DIFF_TOPOLOGY
    # a refused call leaves nothing behind: rebuild_flat() right after it rebuilds the entries the scene had, and the next update_meshes is still its yardstick's
    with pytest.raises(api.CtlError):
        s.update_meshes(d2, m)
    st = s.rebuild_flat(); host.rebuild(old.desc)
    assert "entries_after" not in st and st["n_entries"] == len(host.leaves())
    same_rebuilt_tree(validated(s), host)
    st2 = s.update_meshes(new.desc, m); host.update_meshes(new.desc, m)
    assert st2["nodes"]["rebuilt"] == 1 and st2["meshes_added"] == 4
    same_rebuilt_tree(validated(s), host)
