"""The image set edited in place, the host half: ctl_builder_remove_image / _replace_image / _get_material / _set_material against a builder that made the final state from the
start, byte for byte; the acceptance rules, the pool layout and the run table of ctl_scene_update_image_set through ctl_image_set_plan_host against numpy restatements; the
kernel's arithmetic through ctl_move_texels_host; the refusals; the exported symbols; the no-device answer.  Edits and scenes: tests/image_set_cases.py.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from cudatracerlib_amd import api
import image_update_cases as K
import image_set_cases as S

NEW = ("ctl_builder_remove_image", "ctl_builder_replace_image", "ctl_builder_image_count", "ctl_builder_get_material", "ctl_builder_set_material",
       "ctl_scene_update_image_set", "ctl_image_set_plan_host", "ctl_move_texels_host")


def test_the_new_symbols_are_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctl_amd.h")).read()
    for name in NEW:
        assert getattr(api.lib, name) is not None
        assert "int %s(" % name in header
    assert C.sizeof(api.ctl_scene_image_set_stats) == 40 + 16 + C.sizeof(api.ctl_scene_update_stats) and "} ctl_scene_image_set_stats;" in header
    for method in ("remove_image", "replace_image", "get_material", "set_material", "image_ids"):
        assert hasattr(api.DynamicScene, method)
    assert hasattr(api.Scene, "update_image_set")


# ------------------------------------------------------------------------------------------------ the builder
@pytest.mark.parametrize("name", S.EDIT_NAMES)
def test_edited_builder_equals_a_builder_that_never_held_the_other_images(name):
    start, _ = S.EDITS[name]
    final, kept_from = S.final_specs(name)
    A = S.base_scene(start)
    ids0 = A.desc.image_ids
    assert len(ids0) == len(start) == A.desc.n_images
    d = S.apply_edit(A, name)
    B = S.base_scene(final)
    got, want = S.builder_state(d), S.builder_state(B.desc)
    assert d.n_images == len(final) and A._image_count() == len(final)
    assert S.same_state(got, want), [k for k in want if k not in got or got[k].tobytes() != want[k].tobytes()]
    assert api.scene_desc_diff(d, B.desc) == 0
    # the stable ids give the map the edit implies
    index = {i: k for k, i in enumerate(ids0)}
    assert [index.get(i, S.NONE) for i in d.image_ids] == kept_from


def _refused(call, state_of, needle):
    before = state_of()
    with pytest.raises(api.CtlError) as e:
        call()
    assert e.value.code == api.ERR_INVALID and needle in str(e.value), str(e.value)
    assert S.same_state(before, state_of()), needle


def test_builder_refusals_leave_the_builder_as_it_was():
    tex, env = K.bright_rgbcol(8, 8, 1), K.bright_rgbe(16, 8, 2)
    A = K.floor_scene("floor_env", tex, env)
    spare = A.add_image(K.rgbcol_texels(5, 3, 3)); A.UpdateScene()
    state = lambda: S.builder_state(A.UpdateScene())
    floor = S.material_offset(A.desc, 0)
    _refused(lambda: A.remove_image(A.images["tex"]), state, "material %d (tex[0]) still references image %d" % (floor, A.images["tex"]))
    _refused(lambda: A.remove_image(A.images["env"]), state, "(the environment map) still references image %d" % A.images["env"])
    _refused(lambda: A.remove_image(3), state, "bad image index 3 of 3")
    _refused(lambda: A.remove_image(S.NONE), state, "bad image index")
    _refused(lambda: A.replace_image(A.images["env"], K.bright_rgbe(8, 4, 4)), state, "is the environment map of light")
    _refused(lambda: A.replace_image(7, K.bright_rgbe(8, 4, 4)), state, "bad image index 7 of 3")
    assert api.lib.ctl_builder_replace_image(A._h, api.u32(spare), None, api.u32(4), api.u32(4)) == api.ERR_INVALID
    assert api.lib.ctl_builder_remove_image(None, api.u32(0)) == api.ERR_INVALID
    assert A.image_ids() == (0, 1, 2)
    # a light's radiance texture
    L = S.base_scene([S.spec(S.S42, api.TEXEL_RGBCOL, 1), S.spec(S.S53, api.TEXEL_RGBCOL, 2)])
    L.CreateLight(1, 0, (5.0, 5.0, 5.0), rad_texture=api.image_texture(1)); L.UpdateScene()
    _refused(lambda: L.remove_image(1), lambda: S.builder_state(L.UpdateScene()), "the radiance texture of light 0 still references image 1")
    L.remove_image(0); d = L.UpdateScene()
    assert d.n_images == 1 and d.lights[0].rad_texture.image == 0                         # the texture followed the shift
    # a row orphaned by RemoveMesh: the material table is not compacted, so the row still counts
    O = K.floor_scene("floor_env", tex, env)
    quad = O.mesh_inputs[0]
    other = O.add_image(K.rgbcol_texels(4, 2, 9))
    m = api.diffuse((1, 1, 1)); m.tex[0] = api.image_texture(other)
    node = O.CreateNode(O.add_mesh(quad["positions"] + np.float32(1.0), quad["indices"], normals=quad["normals"], uvs=quad["uvs"], materials=[m]))
    O.UpdateScene()
    row = S.material_offset(O.desc, node)
    O.DeleteNode(node); O.RemoveMesh(2); O.UpdateScene()
    _refused(lambda: O.remove_image(other), lambda: S.builder_state(O.UpdateScene()), "material %d (tex[0]) still references image %d" % (row, other))
    m = O.get_material(row); m.tex[0] = api._const_tex((0.5, 0.5, 0.5)); O.set_material(row, m)      # the host repoints the orphan, then the image goes
    O.remove_image(other)
    assert O.UpdateScene().n_images == 2


def test_replace_image_with_the_same_size_is_update_image():
    X, Y = K.bright_rgbcol(8, 8, 1), K.bright_rgbcol(8, 8, 2)
    A, B = K.floor_scene("plastic", X), K.floor_scene("plastic", X)
    A.replace_image(0, Y); B.update_image(0, Y)
    assert S.same_state(S.builder_state(A.UpdateScene()), S.builder_state(B.UpdateScene()))
    assert A.image_ids() == (0,)                                                           # the same image to a live scene: Scene.update_image carries its texels
    A.replace_image(0, K.bright_rgbcol(4, 8, 3))
    assert A.image_ids() == (1,) and S.image_records(A.UpdateScene())[0][:2] == (4, 8)


def test_set_material_equals_a_builder_that_added_the_mesh_with_it():
    tex, env = K.bright_rgbcol(8, 8, 1), K.bright_rgbe(16, 8, 2)

    def scene(floor_material):
        sc = K.floor_scene("floor_env", tex, env)
        extra = sc.add_image(K.bright_rgbcol(5, 3, 4))
        if floor_material is not None:
            sc.set_material(S.material_offset(sc.desc, 0), floor_material(extra))
        return sc, extra
    phong = lambda image: api.phong(api.image_texture(image), specular_reflectance=(0.3, 0.2, 0.1), exponent=12.0)
    A, extra = scene(phong)
    got = A.get_material(S.material_offset(A.desc, 0))
    assert bytes(got) == bytes(phong(extra))                                               # get returns what set stored
    # builder B registers the same images and adds the floor with that material from the start
    B = api.DynamicScene()
    B.add_image(tex, api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_ANISOTROPIC); B.add_image(env, api.TEXEL_RGBE, api.WRAP_REPEAT, api.FILTER_BILINEAR)
    q, l = A.mesh_inputs[0], A.mesh_inputs[1]
    B.CreateNode(B.add_mesh(q["positions"], q["indices"], normals=q["normals"], uvs=q["uvs"], materials=[phong(2)]))
    ln = B.CreateNode(B.add_mesh(l["positions"], l["indices"], normals=l["normals"], materials=[api.diffuse((0.5, 0.5, 0.5))]))
    B.CreateLight(ln, 0, (30.0, 30.0, 30.0)); B.setEnvironementMap(1, (1.0, 0.9, 0.8))
    B.setCamera((0, 1.5, -30), (0, 0.5, 0), (0, 1, 0), 50.0, K.W, K.H)
    B.add_image(K.bright_rgbcol(5, 3, 4))
    got, want = S.builder_state(A.UpdateScene()), S.builder_state(B.UpdateScene())
    assert S.same_state(got, want), [k for k in want if got[k].tobytes() != want[k].tobytes()]
    stored = A.get_material(S.material_offset(A.desc, 0))
    assert stored.f[0] != phong(extra).f[0]                                               # finalize made the sampling weight from the image's average
    assert api.scene_desc_diff(A.desc, B.desc) == 0


def test_set_material_refusals():
    A = K.floor_scene("roughcoating", K.bright_rgbcol(8, 8, 1))
    floor = S.material_offset(A.desc, 0)
    coat = A.get_material(floor)
    inner = int(coat.u[2])
    state = lambda: S.builder_state(A.UpdateScene())
    nested = A.get_material(inner)
    bad = A.get_material(floor); bad.u[2] = A.add_material(api.diffuse((0.3, 0.3, 0.3)))    # a coating (over a further simple row) where the floor's coating nests: BSDFFirst
    _refused(lambda: A.set_material(inner, bad), state, "must stay a simple BSDF (BSDFFirst)")
    bad = A.get_material(floor); bad.u[2] = floor
    _refused(lambda: A.set_material(floor, bad), state, "names no simple BSDF (BSDFFirst)")
    bad = A.get_material(floor); bad.u[2] = A.desc.n_materials
    _refused(lambda: A.set_material(floor, bad), state, "out of range")
    bad = A.get_material(inner); bad.tex[0] = api.image_texture(5)
    _refused(lambda: A.set_material(inner, bad), state, "tex[0] references image 5 of 1")
    bad = A.get_material(inner); bad.bsdf_type = 99
    _refused(lambda: A.set_material(inner, bad), state, "BSDF type 99")
    _refused(lambda: A.set_material(A.desc.n_materials, nested), state, "bad material index")
    with pytest.raises(api.CtlError):
        A.get_material(A.desc.n_materials)
    A.set_material(inner, api.diffuse((0.1, 0.2, 0.3)))                                    # another simple BSDF under the coating is fine
    assert bytes(A.get_material(inner)) == bytes(api.diffuse((0.1, 0.2, 0.3)))


# ------------------------------------------------------------------------------------------------ the plan
def _edit(name):
    """(description before, description after, the map, the specs before and after)"""
    start, _ = S.EDITS[name]
    final, kept_from = S.final_specs(name)
    A = S.base_scene(start)
    d0 = A.desc
    held = S.base_scene(start)               # a second builder keeps the description the scene would hold alive and unchanged
    d1 = S.apply_edit(A, name)
    assert S.id_map(d0, d1) == kept_from
    return held, A, kept_from, start, final


@pytest.mark.parametrize("name", S.EDIT_NAMES)
def test_layout_runs_and_texel_move(name):
    held, A, image_map, start, final = _edit(name)
    old, new = S.pyramids(start), S.pyramids(final)
    plan = api.image_set_plan_host(held.desc, A.desc, image_map)
    # the layout: what ctl_mip_pyramid_host implies image by image
    sizes = [len(api.mip_pyramid_host(S.texels_of(s), s[1])["texels"]) for s in final]
    assert sizes == [len(p["texels"]) for p in new]
    assert plan["offsets"].tolist() == np.concatenate([[0], np.cumsum(sizes)])[:-1].astype(np.uint64).tolist() and plan["total"] == sum(sizes)
    # the runs
    want = S.numpy_runs([len(p["texels"]) for p in old], sizes, image_map)
    assert plan["n_runs"] == len(want) - 1 and np.array_equal(plan["runs"], want), (plan["runs"].tolist(), want.tolist())
    if name == "remove every second of seven":
        assert plan["n_runs"] == 4
    if name == "remove the first of three":
        assert plan["n_runs"] == 1 and plan["runs"][0].tolist() == [0, 1, 17 + 85, 0]     # everything behind the one-texel image moves down by one texel
    # the move: the kept pyramids at the planned offsets, the words of fresh slots untouched
    old_pool = np.concatenate([p["texels"] for p in old]) if old else np.zeros(0, np.uint32)
    MARK = np.uint32(0xdeadbeef)
    pool = np.full(plan["total"], MARK, np.uint32)
    api.move_texels_host(old_pool, plan["runs"], pool)
    expect = np.full(plan["total"], MARK, np.uint32)
    for j, o in enumerate(image_map):
        if o != S.NONE:
            expect[int(plan["offsets"][j]):int(plan["offsets"][j]) + sizes[j]] = old[o]["texels"]
            assert old[o]["texels"].tobytes() == new[j]["texels"].tobytes()
    assert pool.tobytes() == expect.tobytes()
    # a table whose sizes lie: nothing is read or written outside the pools
    short = np.full(max(0, plan["total"] - 1), MARK, np.uint32)
    api.move_texels_host(old_pool[:max(0, len(old_pool) - 1)], plan["runs"], short)
    assert np.isin(short, np.concatenate([old_pool, [MARK]])).all()


def _plan_refused(held, new_desc, image_map, needle):
    with pytest.raises(api.CtlError) as e:
        api.image_set_plan_host(held.desc, new_desc, image_map)
    assert e.value.code == api.ERR_INVALID and needle in str(e.value), str(e.value)
    return str(e.value)


def test_plan_refusals_each_with_its_own_message():
    specs = [S.spec(S.S42, api.TEXEL_RGBCOL, 1), S.spec(S.S53, api.TEXEL_RGBE, 2), S.spec(S.S88, api.TEXEL_RGBCOL, 3)]
    held = S.base_scene(specs)
    same = S.base_scene(specs)
    assert api.image_set_plan_host(held.desc, same.desc, [0, 1, 2])["n_runs"] == 1       # the identity is a valid map
    seen = set()
    seen.add(_plan_refused(held, same.desc, [0, 1], "the image map has 2 elements, the new description 3 images"))
    seen.add(_plan_refused(held, same.desc, [0, 2, 1], "not strictly increasing at element 2"))
    seen.add(_plan_refused(held, same.desc, [0, 1, 1], "not strictly increasing at element 2"))
    seen.add(_plan_refused(held, same.desc, [0, 1, 3], "names image 3 of 3"))
    # a kept image with another size, type, wrap or filter
    resized = S.base_scene(specs); resized.replace_image(1, K.rgbe_texels(4, 2, 9)); resized.UpdateScene()
    seen.add(_plan_refused(held, resized.desc, [0, 1, 2], "kept image 1 (was 1) has another size, texel type, wrap or filter mode"))
    assert api.image_set_plan_host(held.desc, resized.desc, [0, S.NONE, 2])["n_runs"] == 2
    retyped = S.base_scene([specs[0], S.spec(S.S53, api.TEXEL_RGBCOL, 2), specs[2]])
    _plan_refused(held, retyped.desc, [0, 1, 2], "kept image 1 (was 1) has another size, texel type, wrap or filter mode")
    for wrap, filt in ((api.WRAP_CLAMP, api.FILTER_TRILINEAR), (api.WRAP_REPEAT, api.FILTER_BILINEAR)):
        other = api.DynamicScene()
        for s in specs:
            other.add_image(S.texels_of(s), s[1], wrap, filt)
        q, l = held.mesh_inputs[0], held.mesh_inputs[1]
        other.CreateNode(other.add_mesh(q["positions"], q["indices"], normals=q["normals"], uvs=q["uvs"], materials=[api.diffuse((0.6, 0.6, 0.6))]))
        ln = other.CreateNode(other.add_mesh(l["positions"], l["indices"], normals=l["normals"], materials=[api.diffuse((0.5, 0.5, 0.5))]))
        other.CreateLight(ln, 0, (30.0, 30.0, 30.0)); other.setCamera((0, 1.5, -30), (0, 0.5, 0), (0, 1, 0), 50.0, K.W, K.H); other.UpdateScene()
        _plan_refused(held, other.desc, [0, 1, 2], "kept image 0 (was 0) has another size, texel type, wrap or filter mode")
    # a kept image with another digest
    repainted = S.base_scene(specs); repainted.update_image(2, K.rgbcol_texels(8, 8, 99)); repainted.UpdateScene()
    seen.add(_plan_refused(held, repainted.desc, [0, 1, 2], "kept image 2 (was 2) has another digest"))
    assert api.image_set_plan_host(held.desc, repainted.desc, [0, 1, S.NONE])["n_runs"] == 1
    # another mesh set, another node set: their own calls
    q = held.mesh_inputs[0]
    meshes = S.base_scene(specs); meshes.add_mesh(q["positions"], q["indices"], normals=q["normals"], uvs=q["uvs"]); meshes.UpdateScene()
    seen.add(_plan_refused(held, meshes.desc, [0, 1, 2], "the set of meshes differs"))
    nodes = S.base_scene(specs); nodes.CreateNode(0, np.array([[1, 0, 0, 3], [0, 1, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)); nodes.UpdateScene()
    seen.add(_plan_refused(held, nodes.desc, [0, 1, 2], "the set of nodes differs"))
    assert len(seen) == 7                                                                  # seven rules, seven messages (the two non-increasing maps share theirs)


def test_everything_ctl_scene_update_applies_is_accepted_beside_the_edit():
    """camera, materials (a grown table too), lights: the plan takes them; the first environment map arrives this way"""
    specs = [S.spec(S.S42, api.TEXEL_RGBCOL, 1)]
    held = S.base_scene(specs)
    A = S.base_scene(specs)
    env = A.add_image(K.bright_rgbe(16, 8, 5), api.TEXEL_RGBE, api.WRAP_REPEAT, api.FILTER_BILINEAR)
    A.setEnvironementMap(env, (1.0, 0.9, 0.8))
    m = A.get_material(S.material_offset(A.desc, 0)); m.tex[0] = api.image_texture(0); A.set_material(S.material_offset(A.desc, 0), m)
    A.add_material(api.diffuse((0.2, 0.2, 0.2)))
    A.setCamera((3, 2.5, -28), (0, 0.5, 0), (0, 1, 0), 45.0, K.W, K.H)
    d = A.UpdateScene()
    assert d.n_materials == held.desc.n_materials + 1 and d.n_lights_buf == held.desc.n_lights_buf + 1
    plan = api.image_set_plan_host(held.desc, d, S.id_map(held.desc, d))
    assert plan["n_runs"] == 1 and plan["total"] == 8 + 2 + 128 + 32 + 8 + 2


def test_the_device_call_answers_no_device_first():
    """without a device the call reports CTL_ERR_NO_DEVICE before it looks at its arguments; with one, a null scene is invalid"""
    want = api.ERR_NO_DEVICE if api.device_count() < 1 else api.ERR_INVALID
    assert api.lib.ctl_scene_update_image_set(None, None, None, 0, None) == want
    m = np.zeros(3, np.uint32)
    assert api.lib.ctl_scene_update_image_set(None, None, m.ctypes.data, 3, None) == want
