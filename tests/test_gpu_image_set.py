"""ctl_scene_update_image_set on the device: images removed from, added to and replaced in a live scene — the kept pyramids moved into a new texel pool by k_move_texels
(csrc/scene_image_set.hip), fresh ones uploaded and built there, then the stages of ctl_scene_update.  The yardstick is a scene created from the new description: the pool
word for word, the light tables, the frames of every plugin bit for bit.  Edits: tests/image_set_cases.py; frames 64 x 64, 2 passes, depth 3."""
import ctypes as C

import numpy as np
import pytest

from cudatracerlib_amd import api
import image_update_cases as K
import image_set_cases as S
from test_gpu_image_update import tracers, render, assert_bit_equal

pytestmark = pytest.mark.gpu
TEX, ENV = (64, 64), (32, 16)


def assert_pool_equals_fresh(scene, fresh, desc, what=""):
    for j in range(desc.n_images):
        got, want = scene.read_image(j), fresh.read_image(j)
        assert got["levels"] == want["levels"] and np.array_equal(got["offsets"], want["offsets"]), (what, j)
        bad = np.nonzero(got["texels"] != want["texels"])[0]
        assert got["texels"].tobytes() == want["texels"].tobytes(), (what, j, len(bad), bad[:8].tolist())
    with pytest.raises(api.CtlError):
        scene.read_image(desc.n_images)


@pytest.mark.parametrize("flatten", [False, True])
@pytest.mark.parametrize("name", S.EDIT_NAMES)
def test_pool_read_back(gpu, name, flatten):
    """after the call ctl_scene_read_image of every image equals a fresh scene's from new_desc, word for word, and numpy_pyramid for the fresh images"""
    start, _ = S.EDITS[name]
    final, kept_from = S.final_specs(name)
    A = S.base_scene(start)
    scene = gpu.Scene(A.desc, flatten=flatten)
    d = S.apply_edit(A, name)
    st = scene.update_image_set(A)
    fresh = gpu.Scene(d, flatten=flatten)
    assert_pool_equals_fresh(scene, fresh, d, name)
    want = S.pyramids(final)
    for j, o in enumerate(kept_from):
        if o == S.NONE:
            assert scene.read_image(j)["texels"].tobytes() == want[j]["texels"].tobytes(), (name, j)
    n_old = len(start)
    kept = sum(1 for o in kept_from if o != S.NONE)
    assert (st["images_kept"], st["images_fresh"], st["images_removed"]) == (kept, len(final) - kept, n_old - kept)
    assert st["texels_moved"] == sum(len(want[j]["texels"]) for j, o in enumerate(kept_from) if o != S.NONE)
    assert st["texels_uploaded"] == sum(final[j][0][0] * final[j][0][1] for j, o in enumerate(kept_from) if o == S.NONE)
    assert st["runs"] == len(S.numpy_runs([len(p["texels"]) for p in S.pyramids(start)], [len(p["texels"]) for p in want], kept_from)) - 1
    assert scene.update(d) == 0 and scene.last_mask == 0                                   # the scene's own copy of the description is the new one
    print("%s (%s): move %.3f ms, fresh %.3f ms, hash %.3f ms, total %.3f ms" % (name, "flat" if flatten else "two-level", st["move_ms"], st["pyramid_ms"], st["hash_ms"], st["total_ms"]))


def test_kept_texels_survive(gpu):
    """kept images that ctl_scene_update_image changed earlier — mirrored in the builder, as the header asks — keep those texels through the move"""
    name = "remove every second of seven"
    start, _ = S.EDITS[name]
    final, kept_from = S.final_specs(name)
    A = S.base_scene(start)
    scene = gpu.Scene(A.desc)
    painted = {}
    for i in (2, 6):
        (w, h), texel_type, seed = start[i]
        painted[i] = S.texels_of(((w, h), texel_type, seed + 1000))
        scene.update_image(i, painted[i]); A.update_image(i, painted[i])
    d = S.apply_edit(A, name)
    scene.update_image_set(A)
    for j, o in enumerate(kept_from):
        want = K.numpy_pyramid(painted[o], start[o][1]) if o in painted else S.pyramids([start[o]])[0]
        assert scene.read_image(j)["texels"].tobytes() == want["texels"].tobytes(), (j, o)
    # texels the host did NOT mirror: the digest tells, the call refuses, the scene stays
    scene.update_image(0, S.texels_of((start[0][0], start[0][1], 77)))
    A.add_image(K.rgbcol_texels(2, 2, 5)); A.UpdateScene()
    before = scene.read_image(0)["texels"]
    with pytest.raises(gpu.CtlError) as e:
        scene.update_image_set(A)
    assert e.value.code == api.ERR_INVALID and "another digest" in str(e.value)
    assert np.array_equal(scene.read_image(0)["texels"], before)


def two_quads(tex, env, second):
    """floor_scene("floor_env") extended with a second textured quad (a diffuse panel over image `second`, standing behind the light), finalized"""
    sc = K.floor_scene("floor_env", tex, env)
    sc.images["panel"] = sc.add_image(second, api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_TRILINEAR)
    m = api.diffuse((1, 1, 1)); m.tex[0] = api.image_texture(sc.images["panel"])
    P = np.array([[-12, 0, 14], [12, 0, 14], [12, 14, 14], [-12, 14, 14]], np.float32)
    uv = np.array([[0, 0], [3, 0], [3, 3], [0, 3]], np.float32)
    sc.panel = sc.CreateNode(sc.add_mesh(P, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=np.tile(np.array([0, 0, -1], np.float32), (4, 1)), uvs=uv, materials=[m]))
    sc.UpdateScene()
    return sc


@pytest.mark.parametrize("flatten", [True, False])
def test_frames_equal_a_fresh_scene(gpu, orc, flatten):
    """a new image arrives and the floor is repointed to it (set_material) in one call; the old image leaves in a second call: after each, every plugin renders the frame of
    a scene created from the new description, bit for bit"""
    tex, env, panel = K.bright_rgbcol(*TEX, 1), K.bright_rgbe(*ENV, 2), K.bright_rgbcol(16, 16, 3)
    A = two_quads(tex, env, panel)
    scene = gpu.Scene(A.desc, flatten=flatten)
    tables = orc.sequence_tables(2)
    first = {name: render(gpu, make, scene, tables, n) for name, make, n in tracers(gpu, flatten)}

    def same_as_fresh(what):
        fresh = gpu.Scene(A.desc, flatten=flatten)
        assert_pool_equals_fresh(scene, fresh, A.desc, what)
        frames = {}
        for name, make, n in tracers(gpu, flatten):
            got, want = render(gpu, make, scene, tables, n), render(gpu, make, fresh, tables, n)
            assert want[..., :3].any()
            assert_bit_equal(got, want, what + ": " + name)
            frames[name] = got
        return frames
    # 1. add an image (of another size than the one it will stand in for) and repoint the floor
    newer = A.add_image(K.bright_rgbcol(37, 23, 11) & np.uint32(0xff3f7fff), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_ANISOTROPIC)
    floor = S.material_offset(A.desc, 0)
    m = A.get_material(floor); m.tex[0].image = newer; A.set_material(floor, m)
    A.UpdateScene()
    st = scene.update_image_set(A)
    assert st["images_fresh"] == 1 and st["images_kept"] == 3 and st["runs"] == 1 and st["update"]["mask"] & api.DIFF_MATERIALS
    second = same_as_fresh("image added, floor repointed")
    assert not np.array_equal(second["WavefrontPathTracer"], first["WavefrontPathTracer"])                      # the floor does show the new image
    assert not np.array_equal(second["WavefrontPathTracer"], second["WavefrontPathTracer TextureFiltering"])    # and its pyramid is read
    # 2. the old floor texture leaves: the first image of the pool, so everything behind it moves
    A.remove_image(A.images["tex"]); A.UpdateScene()
    st = scene.update_image_set(A)
    assert st["images_removed"] == 1 and st["images_kept"] == 3 and st["runs"] == 1 and st["bytes_freed"] == 4 * len(K.numpy_pyramid(tex, api.TEXEL_RGBCOL)["texels"])
    third = same_as_fresh("old image removed")
    for name in third:
        assert_bit_equal(third[name], second[name], "removing an unread image changes no pixel: " + name)


def test_first_environment_map(gpu, orc):
    """a scene gains its first environment map: the light table and the anim blob grow; read_lights equals the builder's tables, frames equal a fresh scene's"""
    A = K.floor_scene("plastic", K.bright_rgbcol(*TEX, 1))
    scene = gpu.Scene(A.desc, flatten=True)
    env = A.add_image(K.bright_rgbe(*ENV, 2), api.TEXEL_RGBE, api.WRAP_REPEAT, api.FILTER_BILINEAR)
    A.setEnvironementMap(env, (1.0, 0.9, 0.8)); A.UpdateScene()
    st = scene.update_image_set(A)
    assert st["images_fresh"] == 1 and st["update"]["mask"] & api.DIFF_LIGHTS
    got, want = scene.read_lights(), K.light_tables(A.desc)
    assert len(want["lights"]) == 2 and np.array_equal(got["lights"], want["lights"]) and got["anim"].tobytes() == want["anim"].tobytes()
    fresh = gpu.Scene(A.desc, flatten=True)
    tables = orc.sequence_tables(2)
    for name, make, n in tracers(gpu):
        assert_bit_equal(render(gpu, make, scene, tables, n), render(gpu, make, fresh, tables, n), name)


def test_workflow_continues(gpu, orc):
    """after an image-set edit: ctl_scene_update finds nothing; ctl_scene_update_image on a kept and on a fresh image matches its own yardstick; ctl_scene_update_mesh_set
    adds a mesh whose material reads the fresh image, and the frame equals a fresh scene's"""
    tex, env = K.bright_rgbcol(*TEX, 1), K.bright_rgbe(*ENV, 2)
    A = K.floor_scene("floor_env", tex, env)
    scene = gpu.Scene(A.desc, flatten=True)
    fresh_image = A.add_image(K.bright_rgbcol(16, 8, 3), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_TRILINEAR)
    A.UpdateScene()
    scene.update_image_set(A)
    assert scene.update(A.desc) == 0 and scene.last_mask == 0
    for image, Y in ((A.images["tex"], K.bright_rgbcol(*TEX, 21) & np.uint32(0xff3f7fff)), (fresh_image, K.bright_rgbcol(16, 8, 22)), (A.images["env"], K.bright_rgbe(*ENV, 23))):
        scene.update_image(image, Y); A.update_image(image, Y)
        assert scene.read_image(image)["texels"].tobytes() == api.mip_pyramid_host(Y, api.TEXEL_RGBE if image == A.images["env"] else api.TEXEL_RGBCOL)["texels"].tobytes()
    A.UpdateScene()
    assert scene.update(A.desc) == 0
    got, want = scene.read_lights(), K.light_tables(A.desc)
    assert np.array_equal(got["lights"], want["lights"]) and got["anim"].tobytes() == want["anim"].tobytes()
    # a mesh whose material reads the fresh image: its own call, on its own description
    m = api.diffuse((1, 1, 1)); m.tex[0] = api.image_texture(fresh_image)
    P = np.array([[-12, 0, 14], [12, 0, 14], [12, 14, 14], [-12, 14, 14]], np.float32)
    uv = np.array([[0, 0], [3, 0], [3, 3], [0, 3]], np.float32)
    A.CreateNode(A.add_mesh(P, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=np.tile(np.array([0, 0, -1], np.float32), (4, 1)), uvs=uv, materials=[m]))
    A.UpdateScene()
    st = scene.update_mesh_set(A)
    assert st["meshes"]["meshes_added"] == 1
    tables = orc.sequence_tables(2)
    fresh = gpu.Scene(A.desc, flatten=True)
    for name, make, n in tracers(gpu)[1:3]:
        assert_bit_equal(render(gpu, make, scene, tables, n), render(gpu, make, fresh, tables, n), "a mesh over the fresh image: " + name)
    # and the way back: drop the mesh, repoint nothing (its row is orphaned: set_material first), drop its texture
    node = A.desc.n_nodes - 1
    row = S.material_offset(A.desc, node)
    A.DeleteNode(node); A.RemoveMesh(A.desc.n_meshes - 1); A.UpdateScene()
    scene.update_mesh_set(A)
    orphan = A.get_material(row); orphan.tex[0] = api._const_tex((0.5, 0.5, 0.5)); A.set_material(row, orphan)
    A.remove_image(fresh_image); A.UpdateScene()
    st = scene.update_image_set(A)
    assert st["images_removed"] == 1 and st["images_kept"] == 2
    fresh = gpu.Scene(A.desc, flatten=True)
    assert_pool_equals_fresh(scene, fresh, A.desc, "mesh and texture dropped")
    name, make, n = tracers(gpu)[1]
    assert_bit_equal(render(gpu, make, scene, tables, n), render(gpu, make, fresh, tables, n), "mesh and texture dropped")


def test_identity_map_is_ctl_scene_update(gpu):
    A = K.floor_scene("floor_env", K.bright_rgbcol(*TEX, 1), K.bright_rgbe(*ENV, 2))
    scene = gpu.Scene(A.desc, flatten=True)
    A.setCamera((3, 2.5, -28), (0, 0.5, 0), (0, 1, 0), 45.0, K.W, K.H); A.UpdateScene()
    st = scene.update_image_set(A, image_map=[0, 1])
    assert st["update"]["mask"] == api.DIFF_CAMERA and st["texels_moved"] == 0 and st["runs"] == 0 and st["images_kept"] == 2
    assert scene.update(A.desc) == 0


def test_refusals_leave_the_scene_as_it_was(gpu, orc):
    specs = [S.spec(S.S42, api.TEXEL_RGBCOL, 1), S.spec(S.S53, api.TEXEL_RGBE, 2), S.spec(S.S88, api.TEXEL_RGBCOL, 3)]
    held = S.base_scene(specs)
    scene = gpu.Scene(held.desc, flatten=True)
    tables = orc.sequence_tables(2)
    name, make, n = tracers(gpu)[1]
    before = render(gpu, make, scene, tables, n)
    pool = [scene.read_image(j)["texels"] for j in range(3)]

    def edited(edit):
        sc = S.base_scene(specs); edit(sc); sc.UpdateScene()
        return sc
    q = held.mesh_inputs[0]
    cases = [("a short map", held, [0, 1], "the image map has 2 elements"),
             ("a non-increasing map", held, [0, 2, 1], "not strictly increasing"),
             ("an out-of-range map", held, [0, 1, 3], "names image 3 of 3"),
             ("a kept image of another size", edited(lambda sc: sc.replace_image(1, K.rgbe_texels(4, 2, 9))), [0, 1, 2], "has another size, texel type, wrap or filter mode"),
             ("a kept image of another type", S.base_scene([specs[0], S.spec(S.S53, api.TEXEL_RGBCOL, 2), specs[2]]), [0, 1, 2], "has another size, texel type, wrap or filter mode"),
             ("a kept image with other texels", edited(lambda sc: sc.update_image(2, K.rgbcol_texels(8, 8, 99))), [0, 1, 2], "another digest"),
             ("another mesh set", edited(lambda sc: sc.add_mesh(q["positions"], q["indices"], normals=q["normals"], uvs=q["uvs"])), [0, 1, 2], "the set of meshes differs"),
             ("another node set", edited(lambda sc: sc.CreateNode(0, np.array([[1, 0, 0, 3], [0, 1, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32))), [0, 1, 2], "the set of nodes differs")]
    for what, sc, image_map, needle in cases:
        with pytest.raises(gpu.CtlError) as e:
            scene.update_image_set(sc.desc, image_map=image_map)
        assert e.value.code == api.ERR_INVALID and needle in str(e.value), (what, str(e.value))
        for j in range(3):
            assert np.array_equal(scene.read_image(j)["texels"], pool[j]), (what, j)
        assert_bit_equal(render(gpu, make, scene, tables, n), before, what)
    st = api.ctl_scene_image_set_stats()
    assert api.lib.ctl_scene_update_image_set(scene._h, C.byref(held.desc), None, api.u32(3), C.addressof(st)) == api.ERR_INVALID      # a null map
    assert api.lib.ctl_scene_update_image_set(None, C.byref(held.desc), None, api.u32(0), None) == api.ERR_INVALID
    assert scene.update(held.desc) == 0
    # the other calls keep their refusals: another image set is still topology to ctl_scene_update and to the node-set call
    grown = edited(lambda sc: sc.add_image(K.rgbcol_texels(2, 2, 5)))
    with pytest.raises(gpu.CtlError):
        scene.update(grown.desc)
    assert scene.last_mask & api.DIFF_TOPOLOGY
    with pytest.raises(gpu.CtlError) as e:
        scene.update_nodes(grown.desc, old_of_new=[0, 1])
    assert "the images or transmittance tables differ" in str(e.value)
    assert_bit_equal(render(gpu, make, scene, tables, n), before, "after the other calls' refusals")
