"""ctl_scene_update_image on the device: the level-0 texels of an image of a live scene replaced in place, and the pyramid, the material sampling weights and the environment
light's tables rebuilt by the kernels of csrc/scene_images.hip.  The yardstick is the host builder: ctl_mip_pyramid_host for the pool, a builder B that registered the new
image from the start (equal, byte for byte, to a builder taken through ctl_builder_update_image: tests/test_image_update_host.py) for the tables, the frames and the
workflow.  Scenes and texel sets: tests/image_update_cases.py — 64 x 64 frames of a textured floor under an environment map."""
import ctypes as C

import numpy as np
import pytest

from cudatracerlib_amd import api
import image_update_cases as K

pytestmark = pytest.mark.gpu
DEPTH = 3
TEX, ENV = (64, 64), (32, 16)                   # (width, height) of the frame scenes' floor texture and environment map


def update(scene, image, texels, source):
    if source == "host":
        return scene.update_image(image, texels)
    dev = K.DeviceTexels(texels)
    return scene.update_image(image, dev.ptr.value, width=dev.width, height=dev.height, device=True)


@pytest.mark.parametrize("texel_type", [api.TEXEL_RGBE, api.TEXEL_RGBCOL])
@pytest.mark.parametrize("size", K.PYRAMID_SIZES + [(256, 256)])
def test_pyramid_read_back(gpu, size, texel_type):
    """the pool after the update equals the host builder's pyramid, from a host array and from a device pointer; RGBE texels include zero exponents and both ends"""
    w, h = size
    make = (lambda seed: K.rgbe_texels(w, h, seed)) if texel_type == api.TEXEL_RGBE else (lambda seed: K.rgbcol_texels(w, h, seed))
    sc = K.floor_scene("textured", make(1), tex_type=texel_type, filter_mode=api.FILTER_TRILINEAR)
    scene = gpu.Scene(sc.desc)
    first = scene.read_image(0)
    assert first["texels"].tobytes() == api.mip_pyramid_host(make(1), texel_type)["texels"].tobytes()      # creation uploads the same pyramid
    for seed, source in ((2, "host"), (3, "device")):
        Y = make(seed)
        st = update(scene, 0, Y, source)
        want = api.mip_pyramid_host(Y, texel_type)
        got = scene.read_image(0)
        assert got["levels"] == want["levels"] == st["levels"] and np.array_equal(got["offsets"], want["offsets"])
        bad = np.nonzero(got["texels"] != want["texels"])[0]
        assert got["texels"].tobytes() == want["texels"].tobytes(), (source, len(bad), bad[:8].tolist())
        assert st["texels_written"] == len(want["texels"]) and st["env_tables"] == 0 and st["materials_patched"] == 0
        print("%dx%d type %d %s: upload %.3f pyramid %.3f hash %.3f total %.3f ms" % (w, h, texel_type, source, st["upload_ms"], st["pyramid_ms"], st["hash_ms"], st["total_ms"]))


@pytest.mark.parametrize("env_type", [api.TEXEL_RGBE, api.TEXEL_RGBCOL])
@pytest.mark.parametrize("size", K.ENV_SIZES)
def test_environment_tables(gpu, size, env_type):
    """cdfCols, cdfRows and normalization in HBM against builder B's, byte for byte; every row of the maps has positive luminance (a row without gives the reference's
    0 * inf, whose NaN payload is the one thing host and device may differ in: documented in include/ctl_amd.h, not compared)"""
    w, h = size
    make = (lambda seed: K.bright_rgbe(w, h, seed)) if env_type == api.TEXEL_RGBE else (lambda seed: K.bright_rgbcol(w, h, seed))
    A = K.floor_scene("env", env=make(1), env_type=env_type)
    scene = gpu.Scene(A.desc)
    for seed, source in ((2, "host"), (3, "device")):
        B = K.floor_scene("env", env=make(seed), env_type=env_type)
        st = update(scene, A.images["env"], make(seed), source)
        assert st["env_tables"] == 1 and st["materials_patched"] == 0
        got, want = scene.read_lights(), K.light_tables(B.desc)
        assert not np.isnan(want["anim"].view(np.float32)).any()
        assert np.array_equal(got["lights"], want["lights"]), (source, np.argwhere(got["lights"] != want["lights"])[:4].tolist())
        bad = np.nonzero(got["anim"].view(np.uint32) != want["anim"].view(np.uint32))[0]
        assert got["anim"].tobytes() == want["anim"].tobytes(), (source, len(bad), bad[:8].tolist())
        assert scene.update(B.desc) == 0                                                  # and the scene's own copy of the description agrees


def tracers(gpu, flatten=True):
    """(name, constructor, passes); the PathTracer and the PrimTracer need a flattened scene"""
    def prim():
        t = gpu.PrimTracer(); t.getParameters().setValue("DrawingMode", "first_f_direct"); return t

    def filtered():
        t = gpu.WavefrontPathTracer(); t.getParameters().setValue("TextureFiltering", True); return t
    wave = (("WavefrontPathTracer", gpu.WavefrontPathTracer, 2), ("WavefrontPathTracer TextureFiltering", filtered, 2))
    return wave + ((("PathTracer", gpu.PathTracer, 2), ("PrimTracer", prim, 1)) if flatten else ())


def render(gpu, make, scene, tables, n_passes):
    tr = make()
    tr.getParameters().setValue("MaxPathLength", DEPTH)
    tr.Resize(K.W, K.H); tr.InitializeScene(scene)
    img = gpu.Image(K.W, K.H)
    for k in range(n_passes):
        tr.setSamplerTables(*tables[k])
        tr.DoPass(img, new_trace=(k == 0))
    return img.getPixelData()


def assert_bit_equal(a, b, what):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: %d of %d pixels differ" % (what, (a.view(np.uint32) != b.view(np.uint32)).any(axis=2).sum(), a.shape[0] * a.shape[1])


def frame_pair(seed_x=1, seed_y=11):
    """builder A over the images X, builder B over the images Y, and Y"""
    X = dict(tex=K.bright_rgbcol(*TEX, seed_x), env=K.bright_rgbe(*ENV, seed_x + 1))
    Y = dict(tex=K.bright_rgbcol(*TEX, seed_y) & np.uint32(0xff3f7fff), env=K.bright_rgbe(*ENV, seed_y + 1))
    return K.floor_scene("floor_env", X["tex"], X["env"]), K.floor_scene("floor_env", Y["tex"], Y["env"]), Y


def mip_queries(image):
    """filtered lookups (KernelMIPMap::eval rows of ctl_shading_eval: image, uv, the two footprint axes) from level 0 up to the coarsest level"""
    foot = [((0, 0), (0, 0)), ((0.02, 0), (0, 0.02)), ((0.06, 0.01), (-0.01, 0.07)), ((0.2, 0), (0, 0.2)), ((0.5, 0.1), (0.1, 0.5)), ((0.9, 0), (0, 0.9)), ((0.3, 0), (0, 0.005))]
    uvs = np.array([(0, 0), (0.5, 0.5), (0.3, 0.7), (-0.25, 1.75), (0.96875, 0.03125)], np.float32)
    rows = []
    for d0, d1 in foot:
        q = np.zeros((len(uvs), 7), np.float32); q[:, 0] = np.asarray(image, np.uint32).view(np.float32); q[:, 1:3] = uvs; q[:, 3:5] = d0; q[:, 5:7] = d1
        rows.append(q)
    return np.concatenate(rows)


@pytest.mark.parametrize("flatten", [True, False])
def test_frames_equal_a_fresh_scene(gpu, orc, flatten):
    """after the update every plugin renders the frame of a scene created from builder B's description, in every pixel, bit for bit — the filtered plugins among them,
    which read the rebuilt pyramid: a scene in which only level 0 had been replaced would render other filtered frames (the pyramid does change, and the filtered frame is
    not the unfiltered one).  The filtered-lookup rows of ctl_shading_eval agree likewise."""
    A, B, Y = frame_pair()
    scene, fresh = gpu.Scene(A.desc, flatten=flatten), gpu.Scene(B.desc, flatten=flatten)
    stale = scene.read_image(A.images["tex"])["texels"]
    st_tex = scene.update_image(A.images["tex"], Y["tex"])
    st_env = update(scene, A.images["env"], Y["env"], "device")
    assert st_tex["materials_patched"] == 1 and st_tex["env_tables"] == 0 and st_env["env_tables"] == 1 and st_env["materials_patched"] == 0
    now = scene.read_image(A.images["tex"])["texels"]
    n0 = TEX[0] * TEX[1]
    assert (now[n0:] != stale[n0:]).mean() > 0.9                                          # the levels behind level 0 were rebuilt
    tables = orc.sequence_tables(2)
    frames = {}
    for name, make, n_passes in tracers(gpu, flatten):
        got, want = render(gpu, make, scene, tables, n_passes), render(gpu, make, fresh, tables, n_passes)
        assert want[..., :3].any()
        assert_bit_equal(got, want, name)
        frames[name] = got
    assert not np.array_equal(frames["WavefrontPathTracer"], frames["WavefrontPathTracer TextureFiltering"])      # the pyramid is read
    q = mip_queries(A.images["tex"])
    got, want = api.shading_eval(scene, api.EVAL_BUILD_PARTIALS, api.EVAL_MIP, q), api.shading_eval(fresh, api.EVAL_BUILD_PARTIALS, api.EVAL_MIP, q)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and len(np.unique(want.view(np.uint32), axis=0)) > 10
    # the old images again: the scene is back where it started
    X = K.desc_bytes(A.desc)
    scene.update_image(A.images["tex"], X["texels%d" % A.images["tex"]].view(np.uint32).reshape(TEX[1], TEX[0]))
    scene.update_image(A.images["env"], X["texels%d" % A.images["env"]].view(np.uint32).reshape(ENV[1], ENV[0]))
    assert scene.update(A.desc) == 0
    name, make, n_passes = tracers(gpu)[1]
    assert_bit_equal(render(gpu, make, scene, tables, n_passes), render(gpu, make, gpu.Scene(A.desc, flatten=flatten), tables, n_passes), "back to the first images")


def test_one_image_as_texture_and_environment_map(gpu, orc):
    """one call patches the material AND rebuilds the light's tables"""
    X, Y = K.bright_rgbe(*ENV, 5), K.bright_rgbe(*ENV, 15)
    A, B = K.floor_scene("both", X, tex_type=api.TEXEL_RGBE), K.floor_scene("both", Y, tex_type=api.TEXEL_RGBE)
    scene = gpu.Scene(A.desc, flatten=True)
    st = scene.update_image(A.images["tex"], Y)
    assert st["materials_patched"] == 1 and st["env_tables"] == 1
    assert scene.update(B.desc) == 0
    tables = orc.sequence_tables(2)
    for name, make, n_passes in tracers(gpu)[1:3]:
        assert_bit_equal(render(gpu, make, scene, tables, n_passes), render(gpu, make, gpu.Scene(B.desc, flatten=True), tables, n_passes), name)


def test_workflow_continues(gpu, orc):
    """the scene's own copy of the description is B's afterwards: ctl_scene_update finds nothing; a camera move on B applies and renders like a fresh scene; another texel in
    a description is still topology; ctl_scene_update_nodes and a skin pose still work"""
    A, B, Y = frame_pair()
    scene = gpu.Scene(A.desc, flatten=True)
    scene.update_image(A.images["tex"], Y["tex"]); scene.update_image(A.images["env"], Y["env"])
    B.update_image(B.images["tex"], Y["tex"]); B.update_image(B.images["env"], Y["env"]); B.UpdateScene()      # the host keeps using its builder: the same call there
    assert scene.update(B.desc) == 0 and scene.last_mask == 0
    tables = orc.sequence_tables(2)
    name, make, n_passes = tracers(gpu)[1]

    def same_as_fresh(what, pose=None):
        fresh = gpu.Scene(B.desc, flatten=True)
        if pose is not None:
            pose(fresh)
        assert_bit_equal(render(gpu, make, scene, tables, n_passes), render(gpu, make, fresh, tables, n_passes), what)
    B.setCamera((3, 2.5, -28), (0, 0.5, 0), (0, 1, 0), 45.0, K.W, K.H); B.UpdateScene()
    assert scene.update(B.desc) == api.DIFF_CAMERA
    same_as_fresh("camera move")
    other = K.floor_scene("floor_env", K.bright_rgbcol(*TEX, 21), Y["env"])
    with pytest.raises(gpu.CtlError) as e:
        scene.update(other.desc)
    assert e.value.code == api.ERR_INVALID and scene.last_mask & api.DIFF_TOPOLOGY
    same_as_fresh("after the refused update")
    lift = np.eye(4, dtype=np.float32); lift[0, 3], lift[1, 3], lift[0, 0], lift[2, 2] = 10.0, 4.0, 0.1, 0.1
    B.CreateNode(0, lift); B.UpdateScene()
    st = scene.update_nodes(B)
    assert st["entries_generated"] >= 2
    same_as_fresh("another node")
    P, I = B.mesh_inputs[0]["positions"], B.mesh_inputs[0]["indices"]
    bi = np.zeros((len(P), 8), np.uint8); bw = np.zeros((len(P), 8), np.uint8); bw[:, 0] = 255
    bone = np.eye(4, dtype=np.float32); bone[1, 3] = 0.75

    def pose(s):
        s.bind_skin(0, P, I, bi, bw, 1, rest_normals=B.mesh_inputs[0]["normals"]); s.animate_mesh(0, bone[None])
    pose(scene)
    same_as_fresh("a skin pose", pose)
    # and a further image update on the posed scene
    Z = K.bright_rgbcol(*TEX, 31)
    scene.update_image(A.images["tex"], Z); B.update_image(B.images["tex"], Z); B.UpdateScene()
    same_as_fresh("an image update under the pose", pose)


def test_refusals_leave_the_scene_as_it_was(gpu, orc):
    A, _, Y = frame_pair()
    scene = gpu.Scene(A.desc, flatten=True)
    tables = orc.sequence_tables(2)
    name, make, n_passes = tracers(gpu)[1]
    before = render(gpu, make, scene, tables, n_passes)
    pool, lights = scene.read_image(A.images["tex"])["texels"], scene.read_lights()
    t = np.ascontiguousarray(Y["tex"], np.uint32); h, w = t.shape
    st = api.ctl_scene_image_stats()
    calls = [("a null scene", None, 0, t.ctypes.data, w, h, 0), ("a bad index", scene._h, A.desc.n_images, t.ctypes.data, w, h, 0), ("null texels", scene._h, 0, None, w, h, 0),
             ("another width", scene._h, 0, t.ctypes.data, w // 2, h, 0), ("another height", scene._h, 0, t.ctypes.data, w, h + 1, 0), ("w and h swapped on the map", scene._h, A.images["env"], t.ctypes.data, ENV[1], ENV[0], 0),
             ("an unknown flag bit", scene._h, 0, t.ctypes.data, w, h, 2), ("an unknown flag bit beside a known one", scene._h, 0, t.ctypes.data, w, h, 0x80000001)]
    for what, s, i, p, ww, hh, flags in calls:
        assert api.lib.ctl_scene_update_image(s, api.u32(i), p, api.u32(ww), api.u32(hh), api.u32(flags), C.addressof(st)) == api.ERR_INVALID, what
        assert api.lib.ctl_last_error(), what
        assert_bit_equal(render(gpu, make, scene, tables, n_passes), before, what)
    assert np.array_equal(scene.read_image(A.images["tex"])["texels"], pool)
    after = scene.read_lights()
    assert np.array_equal(after["lights"], lights["lights"]) and np.array_equal(after["anim"], lights["anim"])
    assert scene.update(A.desc) == 0
    out = np.zeros(4, np.uint32)
    assert api.lib.ctl_scene_read_image(scene._h, api.u32(0), out.ctypes.data, C.c_size_t(4), None, None) == api.ERR_INVALID and not out.any()      # a capacity below the pyramid
    assert api.lib.ctl_scene_read_image(scene._h, api.u32(9), None, C.c_size_t(0), None, None) == api.ERR_INVALID
