"""In-place scene updates, the host half: ctl_scene_desc_diff, DynamicScene.SetNodeTransform and the refit of the flattened Q4 tree (csrc/flat_refit.h) as
ctl_flat_bvh_refit runs it on the host — the same arithmetic the device kernels of ctl_scene_update run (tests/test_gpu_scene_update.py holds the two equal
byte for byte).  The flattened tree only culls, so a refitted tree is held to the bar of a built one: the oracle's traversal of it reports the two-level
traversal's (t, u, v, triangle, node) bit for bit.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from cudatracerlib_amd import api, scenes
from scene_update_cases import SCENES, MOTIONS, build, with_materials, rays_for_update, assert_same_hits, check_structure, node_transforms
from test_oracle_flat import check_implied_links

CASES = [(s, m) for s in SCENES for m in MOTIONS]


def test_diff_names_exactly_what_changed():
    a = build("S3")
    assert api.scene_desc_diff(a.desc, build("S3").desc) == 0
    first = api.ctl_scene_desc.from_buffer_copy(a.desc)
    assert api.scene_desc_diff(first, a.UpdateScene()) == 0                                    # two finalizes of the same builder
    cam = build("S3", edit=lambda sc: sc.setCamera((250, 300, -760), (278, 273, 0), (0, 1, 0), 39.3077, 32, 32))
    assert api.scene_desc_diff(a.desc, cam.desc) == api.DIFF_CAMERA

    def recolour(mats):
        mats[1].tex[0].value[0] = 0.25
    assert api.scene_desc_diff(a.desc, with_materials(a.desc, recolour)) == api.DIFF_MATERIALS
    # a material changed through the builder, bsdf_type included: the same scene with a metal on the ball mesh
    mirror = build("S3", ball_material=api.conductor(eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14)))
    assert api.scene_desc_diff(a.desc, mirror.desc) == api.DIFF_MATERIALS
    light = build("S3", edit=lambda sc: sc.CreatePointLight((278.0, 400.0, 200.0), (5e4, 5e4, 5e4)))
    assert api.scene_desc_diff(a.desc, light.desc) == api.DIFF_LIGHTS
    # a transform-only change: a node without an area light (S1 has lights on nodes of their own)
    s1 = build("S1")
    assert api.scene_desc_diff(s1.desc, build("S1", "M1").desc) == api.DIFF_TRANSFORMS
    assert api.scene_desc_diff(s1.desc, build("S1", "M3").desc) == api.DIFF_TRANSFORMS
    # the emissive panel of S3 moves in M2: its shape set and CDF move with it
    assert api.scene_desc_diff(a.desc, build("S3", "M2").desc) == api.DIFF_TRANSFORMS | api.DIFF_LIGHTS

    def one_more_mesh(sc):
        V, F = scenes.icosphere(1)
        sc.CreateNode(sc.add_mesh(V, F, normals=V, materials=[api.diffuse((0.5, 0.5, 0.5))]))
    assert api.scene_desc_diff(a.desc, build("S3", edit=one_more_mesh).desc) & api.DIFF_TOPOLOGY


def test_set_node_transform_moves_the_area_light_with_its_node():
    a, b = build("S3"), build("S3", "M2")
    node = 4
    la = [a.desc.lights[i] for i in range(a.desc.n_lights_buf) if a.desc.lights[i].type == 2 and a.desc.lights[i].node_idx == node][0]
    lb = [b.desc.lights[i] for i in range(b.desc.n_lights_buf) if b.desc.lights[i].type == 2 and b.desc.lights[i].node_idx == node][0]
    assert la.count == lb.count == 2 and la.triangles_index == lb.triangles_index
    tri = lambda d, l: np.frombuffer(C.string_at(d.anim + l.triangles_index, 64 * l.count), np.float32).reshape(l.count, 16)
    ta, tb = tri(a.desc, la), tri(b.desc, lb)
    Xa, Xb = node_transforms(a.desc)[node], node_transforms(b.desc)[node]
    obj = (ta[:, :9].reshape(-1, 3).astype(np.float64) - Xa[:3, 3]) @ np.linalg.inv(Xa[:3, :3]).T
    want = obj @ Xb[:3, :3].T + Xb[:3, 3]
    assert np.allclose(tb[:, :9].reshape(-1, 3), want, rtol=1e-5, atol=1e-3) and not np.allclose(ta[:, :9], tb[:, :9])
    assert abs(lb.sum_area - tb[:, 12].sum()) <= 1e-4 * lb.sum_area and lb.sum_area != la.sum_area
    # the scene box, the ray epsilon and the top-level BVH follow the new transforms too
    c = build("S1"); d = build("S1", "M3")
    assert not np.array_equal(c.desc.view("scene_bvh_nodes", np.uint32, c.desc.n_scene_bvh_nodes, 16), d.desc.view("scene_bvh_nodes", np.uint32, d.desc.n_scene_bvh_nodes, 16))


@pytest.mark.parametrize("scene,motion", CASES)
def test_refit_keeps_the_structure_and_contains_the_moved_geometry(scene, motion):
    old, new = build(scene), build(scene, motion)
    fb = api.FlatBvh(old.desc)
    N0, L0, ch0 = fb.nodes().copy(), fb.leaves().copy(), fb.child_links().copy()
    n_split, _ = check_structure(fb, old.desc)                    # the bar itself, on the tree as built
    assert n_split > 0 or scene != "S2"                           # S2 carries split references (S1's floor has a few too)
    fb.refit(new.desc)
    N1, L1 = fb.nodes(), fb.leaves()
    assert N1.shape == N0.shape and L1.shape == L0.shape
    assert np.array_equal(N1[:, 10:12], N0[:, 10:12]) and np.array_equal(N1[:, 3] >> 24, N0[:, 3] >> 24) and np.array_equal(fb.child_links(), ch0)   # links, masks
    assert np.array_equal(L1[:, :16], L0[:, :16])                 # entry order, Woop rows, index and node words
    inv = new.desc.view("node_inv_transforms", np.uint32, new.desc.n_nodes, 16)
    assert np.array_equal(L1[:, 16:28], inv[L1[:, 13], :12]) and np.array_equal(L1[:, 28], inv[L1[:, 13], 15])
    assert (N1 != N0).any()
    check_implied_links(fb)
    # What a freshly built tree of the new pose needs on the high side of its inner slots is what the refitted tree gets.  The excess is the remainder of a
    # rounding to the child's grid — anywhere in [0, 1) of a step, another value in every node — so the need is taken in WHOLE steps of the child's grid
    _, fresh_needs = check_structure(api.FlatBvh(new.desc), new.desc)
    n_after, refit_needs = check_structure(fb, new.desc, built_from=old.desc, inner_high_steps=float(np.ceil(fresh_needs)))
    print("%s %s: inner slots, high side, in steps of the child's grid: fresh tree %.4f, refitted tree %.4f; %d split references" % (scene, motion, fresh_needs, refit_needs, n_after))
    assert n_after == n_split
    # empty slots keep their inverted boxes
    exist = (N1[:, 3] >> 24) & 15
    for c in range(4):
        gone = ((exist >> c) & 1) == 0
        for lo_w, hi_w in ((4, 5), (6, 7), (8, 9)):
            assert (((N1[gone, lo_w] >> (8 * c)) & 255) == 255).all() and (((N1[gone, hi_w] >> (8 * c)) & 255) == 0).all()


@pytest.mark.parametrize("scene,motion", CASES)
def test_refitted_tree_reports_the_two_level_hits_bit_for_bit(orc, scene, motion):
    old, new = build(scene), build(scene, motion)
    fb = api.FlatBvh(old.desc).refit(new.desc)
    d = new.desc
    moved = [k for k in range(d.n_nodes) if not np.array_equal(node_transforms(d)[k], node_transforms(old.desc)[k])]
    rays = rays_for_update(d, 30000, 19, aim_nodes=moved)
    want = orc.intersect(d, rays)
    ties = assert_same_hits(orc.intersect(d, rays, flat=fb.desc), want, "%s %s closest hit" % (scene, motion))
    assert (want["tri_idx"] >= 0).mean() > 0.2 and ties <= 30
    assert np.isin(want["node_idx"], moved).sum() > 20            # the moved nodes are hit
    occ = orc.intersect(d, rays, any_hit=True, flat=fb.desc)["tri_idx"] >= 0
    assert np.array_equal(occ, orc.intersect(d, rays, any_hit=True)["tri_idx"] >= 0)


@pytest.mark.parametrize("scene", SCENES)
def test_refit_is_idempotent_and_goes_back(orc, scene):
    old, new = build(scene), build(scene, "M2")
    fb = api.FlatBvh(old.desc).refit(new.desc)
    N1, L1 = fb.nodes().copy(), fb.leaves().copy()
    fb.refit(new.desc)
    assert np.array_equal(fb.nodes(), N1) and np.array_equal(fb.leaves(), L1)
    fb.refit(old.desc)                                            # and back: a valid tree of the old pose (it need not be the built one)
    check_implied_links(fb)
    _, fresh_needs = check_structure(api.FlatBvh(old.desc), old.desc)
    check_structure(fb, old.desc, built_from=old.desc, inner_high_steps=float(np.ceil(fresh_needs)))
    rays = rays_for_update(old.desc, 30000, 23)
    assert_same_hits(orc.intersect(old.desc, rays, flat=fb.desc), orc.intersect(old.desc, rays), scene + " back")
    assert np.array_equal(orc.intersect(old.desc, rays, any_hit=True, flat=fb.desc)["tri_idx"] >= 0, orc.intersect(old.desc, rays, any_hit=True)["tri_idx"] >= 0)
    # a refit never reads what an earlier one wrote: there and back and there again is the first result
    fb.refit(new.desc)
    assert np.array_equal(fb.nodes(), N1) and np.array_equal(fb.leaves(), L1)


def test_refit_is_refused_where_it_cannot_work():
    old, new = build("S3"), build("S3", "M1")
    with pytest.raises(api.CtlError) as e:
        api.FlatBvh(old.desc, api.FLAT_Q8).refit(new.desc)
    assert e.value.code == api.ERR_UNSUPPORTED
    with pytest.raises(api.CtlError):
        api.FlatBvh(old.desc).refit(build("S1").desc)             # another scene


def test_update_without_a_device():
    """ctl_scene_update asks for the device before it looks at its arguments: CTL_ERR_NO_DEVICE on a machine without one (where no scene can exist), and the
    null scene is what a machine with a device complains about"""
    d = build("S3").desc
    mask = api.u32(77)
    code = api.lib.ctl_scene_update(None, C.byref(d), C.byref(mask))
    if api.device_count() == 0:
        assert code == api.ERR_NO_DEVICE and b"no HIP device" in api.lib.ctl_last_error()
    else:
        assert code == api.ERR_INVALID
