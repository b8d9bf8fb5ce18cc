"""Deforming meshes, the host half: DynamicScene.UpdateMesh (ctl_builder_update_mesh), the CTL_DIFF_GEOMETRY class of ctl_scene_desc_diff and the refit of the
flattened Q4 tree to new vertex values as ctl_flat_bvh_refit runs it on the host — the steps and the arithmetic ctl_scene_update runs on the device
(tests/test_gpu_scene_deform.py holds the two equal byte for byte).  Cases D1..D4: tests/scene_deform_cases.py.  No GPU."""
import numpy as np
import pytest

from cudatracerlib_amd import api, scenes
from scene_update_cases import build, rays_for_update, assert_same_hits, check_structure, node_transforms
from scene_deform_cases import CASES, IDS, NO_PART, build_pair, deform, mesh_arrays, mesh_of, nodes_of, entries_of, check_structure_with_collapsed
from test_oracle_flat import check_implied_links


def fresh_mesh(info, scene_desc, mesh):
    """a builder that holds nothing but a fresh add_mesh of the deformed arrays, with the mesh's own per-triangle material indices"""
    tri = mesh_arrays(scene_desc, mesh)["tri"]
    tm = ((tri[:, 1] >> 16) & 0xff).astype(np.uint8)
    sc = api.DynamicScene()
    m = sc.add_mesh(info["positions"], info["indices"], normals=info["normals"], uvs=info["uvs"], tri_material=tm, materials=[api.diffuse()] * (int(tm.max()) + 1))
    sc.CreateNode(m)
    sc.setCamera((0, 0, -5), (0, 0, 0), (0, 1, 0), 40.0, 8, 8)
    sc.UpdateScene()
    return sc, m


def vertices_of(info, tris):
    I = info["indices"] if info["indices"] is not None else np.arange(len(info["positions"])).reshape(-1, 3)
    return info["positions"][I[tris]]


@pytest.mark.parametrize("case,scene", CASES, ids=IDS)
def test_update_mesh_rewrites_the_mesh_like_a_fresh_add_mesh(case, scene):
    info = {}
    old, new = build(scene), build(scene, edit=deform(case, scene, info))
    mesh = info["mesh"]
    a, b = mesh_arrays(old.desc, mesh), mesh_arrays(new.desc, mesh)
    fresh_sc, fm = fresh_mesh(info, old.desc, mesh)
    f = mesh_arrays(fresh_sc.desc, fm)
    assert np.array_equal(b["tri"], f["tri"]) and not np.array_equal(b["tri"], a["tri"])          # the bytes of a fresh add_mesh
    # every Woop row is the fresh builder's row of the same triangle
    row_of = {}
    for j, w in enumerate(f["widx"]):
        row_of.setdefault(int(w >> 1), j)
    tris = b["widx"] >> 1
    known = np.array([int(t) in row_of for t in tris])      # (a fresh spatial-split build may reference a zero-area triangle from no leaf at all)
    V = vertices_of(info, tris[~known]).astype(np.float64)
    assert known.all() or (case == "D3" and (np.linalg.norm(np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]), axis=1) == 0).all())
    rows = np.array([row_of[int(t)] for t in tris[known]])
    assert known.mean() > 0.5 and np.array_equal(b["woop"][known], f["woop"][rows]) and not np.array_equal(b["woop"], a["woop"])
    # the structure stays: leaf references, node links
    assert np.array_equal(b["widx"], a["widx"]) and np.array_equal(b["nodes"][:, 12:], a["nodes"][:, 12:]) and not np.array_equal(b["nodes"][:, :12], a["nodes"][:, :12])
    for other in range(old.desc.n_meshes):
        if other != mesh:
            x, y = mesh_arrays(old.desc, other), mesh_arrays(new.desc, other)
            assert all(np.array_equal(x[k], y[k]) for k in ("tri", "woop", "widx", "nodes")), other
    # the mesh BVH's boxes contain what lies under them: a leaf child's box is the union of its references' WHOLE triangles
    nodes = b["nodes"]; fl = nodes.view(np.float32)
    for i in range(len(nodes)):
        for c, cols in ((0, (0, 1, 2, 3, 8, 9)), (1, (4, 5, 6, 7, 10, 11))):
            link = int(nodes[i, 12 + c:13 + c].view(np.int32)[0])
            if link >= 0:
                continue
            e = ~link; tris = []
            while True:
                tris.append(int(b["widx"][e] >> 1))
                if b["widx"][e] & 1:
                    break
                e += 1
            V = vertices_of(info, np.array(tris)).reshape(-1, 3)
            lo, hi = fl[i, [cols[0], cols[2], cols[4]]], fl[i, [cols[1], cols[3], cols[5]]]
            assert np.array_equal(lo, V.min(axis=0)) and np.array_equal(hi, V.max(axis=0)), (i, c)


@pytest.mark.parametrize("case,scene", CASES, ids=IDS)
def test_the_updated_description_traverses_like_a_fresh_one(orc, case, scene):
    """the refitted mesh BVH against a rebuilt one: the oracle's two-level traversal of the updated description reports the hits of a description built from
    scratch with the deformed arrays in the mesh's place (same nodes, same order, hence the same triangle and node numbers)"""
    info = {}
    new = build(scene, edit=deform(case, scene, info))
    mesh = info["mesh"]
    # a builder that adds the deformed arrays where the scene adds the mesh: the scene functions add their meshes through DynamicScene.add_mesh
    real_add = api.DynamicScene.add_mesh
    count = {"n": 0}

    def add_mesh(self, positions, indices=None, normals=None, uvs=None, tri_material=None, materials=None):
        k = count["n"]; count["n"] += 1
        if k == mesh:
            positions = info["positions"]
        return real_add(self, positions, indices, normals=normals, uvs=uvs, tri_material=tri_material, materials=materials)
    api.DynamicScene.add_mesh = add_mesh
    try:
        fresh = build(scene)
    finally:
        api.DynamicScene.add_mesh = real_add
    assert np.array_equal(mesh_arrays(fresh.desc, mesh)["tri"], mesh_arrays(new.desc, mesh)["tri"])
    assert np.array_equal(node_transforms(fresh.desc), node_transforms(new.desc))
    aim = nodes_of(new.desc, mesh)
    rays = rays_for_update(new.desc, 30000, 31, aim_nodes=aim)
    want = orc.intersect(fresh.desc, rays)
    assert_same_hits(orc.intersect(new.desc, rays), want, "%s %s closest hit" % (case, scene))
    assert (want["tri_idx"] >= 0).mean() > 0.2 and np.isin(want["node_idx"], aim).sum() > 20
    assert np.array_equal(orc.intersect(new.desc, rays, any_hit=True)["tri_idx"] >= 0, orc.intersect(fresh.desc, rays, any_hit=True)["tri_idx"] >= 0)


def test_diff_tells_geometry_from_topology():
    for case, scene in CASES:
        old, new, _ = build_pair(case, scene)
        mask = api.scene_desc_diff(old.desc, new.desc)
        assert mask & api.DIFF_GEOMETRY and not mask & api.DIFF_TOPOLOGY, (case, scene, mask)
        assert api.scene_desc_diff(new.desc, old.desc) == mask
    # the emissive panel: its shape set and CDF ride along
    old, new, _ = build_pair("D4", "S3")
    assert api.scene_desc_diff(old.desc, new.desc) & api.DIFF_LIGHTS
    assert api.DIFF_GEOMETRY == 32

    def one_more_mesh(sc):
        V, F = scenes.icosphere(1)
        sc.CreateNode(sc.add_mesh(V, F, normals=V, materials=[api.diffuse((0.5, 0.5, 0.5))]))
    assert api.scene_desc_diff(old.desc, build("S3", edit=one_more_mesh).desc) & api.DIFF_TOPOLOGY
    # a deformed mesh AND one more mesh: topology, as any grown description
    def both(sc):
        deform("D1", "S3")(sc); one_more_mesh(sc)
    assert api.scene_desc_diff(old.desc, build("S3", edit=both).desc) & api.DIFF_TOPOLOGY


def test_update_mesh_refuses_another_triangle_count():
    sc = build("S3")
    mesh = mesh_of("D1", "S3", sc.desc)
    before = {m: mesh_arrays(sc.desc, m) for m in range(sc.desc.n_meshes)}
    V, F = scenes.icosphere(1)
    for args in ((mesh, V, F), (99, V, F), (mesh, sc.mesh_inputs[mesh]["positions"][:10], sc.mesh_inputs[mesh]["indices"])):
        with pytest.raises(api.CtlError) as e:
            sc.UpdateMesh(*args)
        assert e.value.code == api.ERR_INVALID
    d = sc.UpdateScene()
    for m, want in before.items():
        got = mesh_arrays(d, m)
        assert all(np.array_equal(got[k], want[k]) for k in ("tri", "woop", "widx", "nodes")), m
    assert api.scene_desc_diff(d, build("S3").desc) == 0


@pytest.mark.parametrize("case,scene", CASES, ids=IDS)
def test_refit_to_new_vertices(orc, case, scene):
    old, new, mesh = build_pair(case, scene)
    fb = api.FlatBvh(old.desc)
    N0, L0, ch0 = fb.nodes().copy(), fb.leaves().copy(), fb.child_links().copy()
    part0 = fb.parts()[0].copy()
    ours = entries_of(fb, old.desc, mesh)
    assert ours.any() and not ours.all()
    fb.refit(new.desc)
    N1, L1 = fb.nodes(), fb.leaves()
    part1 = fb.parts()[0]
    assert np.array_equal(N1[:, 10:12], N0[:, 10:12]) and np.array_equal(N1[:, 3] >> 24, N0[:, 3] >> 24) and np.array_equal(fb.child_links(), ch0)   # links, masks
    assert np.array_equal(L1[:, 12:16], L0[:, 12:16]) and np.array_equal(L1[~ours, :12], L0[~ours, :12])   # entry order; the other meshes' rows
    assert (L1[ours, :12] != L0[ours, :12]).any()
    # the entries of the deformed mesh hold the new rows of their triangle and stand for the whole triangle; the others keep their clip boxes
    b = mesh_arrays(new.desc, mesh)
    row_of = {}
    for j, w in enumerate(b["widx"]):
        row_of.setdefault(int(w >> 1), j)
    t0 = b["tri_range"][0]
    rows = np.array([row_of[int(t) - t0] for t in (L1[ours, 12] >> 1)])
    assert np.array_equal(L1[ours, :12], b["woop"][rows])
    assert (part1[ours] == NO_PART).all() and np.array_equal(part1[~ours], part0[~ours])
    if case == "D2":
        assert (part0[ours] != NO_PART).sum() > 0 and (part1[~ours] != NO_PART).sum() == (part0[~ours] != NO_PART).sum()
    check_implied_links(fb)
    _, fresh_needs = check_structure(api.FlatBvh(new.desc), new.desc)
    n_after, collapsed, refit_needs = check_structure_with_collapsed(fb, new.desc, old.desc, float(np.ceil(fresh_needs)))
    print("%s %s: inner slots, high side: fresh tree %.4f, refitted tree %.4f; %d split references stay, %d collapsed entries" % (case, scene, fresh_needs, refit_needs, n_after, collapsed))
    assert (collapsed > 20) == (case == "D3")
    assert n_after == (part0[~ours] != NO_PART).sum()
    # twice gives the same bytes
    N1, L1, P1 = N1.copy(), L1.copy(), part1.copy()
    fb.refit(new.desc)
    assert np.array_equal(fb.nodes(), N1) and np.array_equal(fb.leaves(), L1) and np.array_equal(fb.parts()[0], P1)
    # the oracle traversing the refitted arrays against the two-level traversal of the new description
    aim = nodes_of(new.desc, mesh)
    rays = rays_for_update(new.desc, 30000, 37, aim_nodes=aim)
    want = orc.intersect(new.desc, rays)
    assert_same_hits(orc.intersect(new.desc, rays, flat=fb.desc), want, "%s %s closest hit" % (case, scene))
    assert (want["tri_idx"] >= 0).mean() > 0.2 and np.isin(want["node_idx"], aim).sum() > 20
    assert np.array_equal(orc.intersect(new.desc, rays, any_hit=True, flat=fb.desc)["tri_idx"] >= 0, orc.intersect(new.desc, rays, any_hit=True)["tri_idx"] >= 0)


def test_refit_cannot_bring_back_a_triangle_the_tree_never_held():
    """D3 in reverse: the tree is built from the collapsed ball, whose zero-area triangles gather_references dropped; the round ball has no entries to go into"""
    old, new, mesh = build_pair("D3", "S3", reverse=True)
    assert api.scene_desc_diff(old.desc, new.desc) & api.DIFF_GEOMETRY and not api.scene_desc_diff(old.desc, new.desc) & api.DIFF_TOPOLOGY
    fb = api.FlatBvh(old.desc)
    fwd = api.FlatBvh(new.desc)
    assert len(fb.leaves()) < len(fwd.leaves())
    N0, L0 = fb.nodes().copy(), fb.leaves().copy()
    with pytest.raises(api.CtlError) as e:
        fb.refit(new.desc)
    assert e.value.code == api.ERR_INVALID and "mesh %d" % mesh in str(e.value)
    assert np.array_equal(fb.nodes(), N0) and np.array_equal(fb.leaves(), L0)


def test_a_transform_refit_after_a_geometry_refit_keeps_the_entries_whole(orc):
    from scene_deform_cases import build_deformed_and_moved
    old, new, mesh = build_pair("D2", "S2")
    moved = build_deformed_and_moved("D2", "S2", "M2")
    fb = api.FlatBvh(old.desc).refit(new.desc)
    ours = entries_of(fb, new.desc, mesh)
    fb.refit(moved.desc)
    assert (fb.parts()[0][ours] == NO_PART).all()
    rays = rays_for_update(moved.desc, 30000, 41, aim_nodes=nodes_of(moved.desc, mesh))
    assert_same_hits(orc.intersect(moved.desc, rays, flat=fb.desc), orc.intersect(moved.desc, rays), "D2 then M2")
    # one refit to both at once gives the same tree
    once = api.FlatBvh(old.desc).refit(moved.desc)
    assert np.array_equal(once.nodes(), fb.nodes()) and np.array_equal(once.leaves(), fb.leaves()) and np.array_equal(once.parts()[0], fb.parts()[0])
