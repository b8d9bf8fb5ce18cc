"""Scenes of the first-hit texture filtering tests (tests/test_gpu_texture_filtering.py on the device, tests/test_oracle_texture_filtering.py for the oracle alone):
the noise-textured ground plane of tests/test_gpu_render.py::test_first_hit_ray_differentials_and_filtered_textures — 80 x 80 units, uv x 12, a 64 x 64 image whose every
other texel is darkened, one area light above — seen at a grazing angle by each of the five sensor kinds."""
import numpy as np

W, H = 96, 64                                   # the frames of every test but the block-sampler one
BW, BH = 128, 128                               # 2 x 2 blocks of 64 x 64
SENSORS = ("spherical", "perspective", "thinlens", "orthographic", "telecentric")
SENSOR_TYPE = {"spherical": 1, "perspective": 2, "thinlens": 3, "orthographic": 4, "telecentric": 5}


def ground_scene(filter_mode="anisotropic", sensor="perspective", w=W, h=H):
    """the DynamicScene (its description: .desc after this call).  sensor: one of SENSORS, set through DynamicScene.setSensor (ctl_builder_set_camera) from the look-at
    camera's own record — same position and orientation, another projection"""
    from cudatracerlib_amd import api
    sc = api.DynamicScene()
    rs = np.random.RandomState(4)
    tex = rs.uniform(0.05, 0.95, size=(64, 64, 3)).astype(np.float32)
    tex[::2, ::2] *= 0.2                                                  # high-frequency content: minification changes the mean seen through a pixel
    fm = api.FILTER_ANISOTROPIC if filter_mode == "anisotropic" else api.FILTER_TRILINEAR
    img = sc.add_image(api.float3_to_rgbcol(tex), api.TEXEL_RGBCOL, api.WRAP_REPEAT, fm)
    P = np.array([[-40, 0, -40], [-40, 0, 40], [40, 0, 40], [40, 0, -40]], np.float32)
    uv = np.array([[0, 0], [0, 12], [12, 12], [12, 0]], np.float32)
    ground = api.diffuse((1, 1, 1)); ground.tex[0] = api.image_texture(img)
    sc.CreateNode(sc.add_mesh(P, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=np.tile(np.array([0, 1, 0], np.float32), (4, 1)), uvs=uv, materials=[ground]))
    L = np.array([[-6, 12, -6], [6, 12, -6], [6, 12, 6], [-6, 12, 6]], np.float32)
    ln = sc.CreateNode(sc.add_mesh(L, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=np.tile(np.array([0, -1, 0], np.float32), (4, 1)), materials=[api.diffuse((0.5, 0.5, 0.5))]))
    sc.CreateLight(ln, 0, (30.0, 30.0, 30.0))
    sc.setCamera((0, 1.5, -30), (0, 0.5, 0), (0, 1, 0), 50.0, w, h)
    sc.UpdateScene()
    if sensor != "perspective":
        s = api.ctl_sensor.from_buffer_copy(sc.desc.camera)
        s.type = SENSOR_TYPE[sensor]
        # thin lens: a wide aperture focused in front of the far ground; telecentric: a small one.  The two orthographic kinds see [-screen_scale, screen_scale] camera units:
        # 12 units across, so that a pixel's footprint on the grazing ground spans several texels (one texel = 80 / (12 * 64) units)
        s.aperture_radius, s.focus_distance = (0.25, 20.0) if sensor == "thinlens" else (0.05, 20.0)
        s.screen_scale[:] = [6.0, 6.0]
        if sensor in ("orthographic", "telecentric"):
            s.near_depth, s.far_depth = 1e-5, 1e5
        sc.setSensor(s); sc.UpdateScene()
        assert sc.desc.camera.type == s.type
    return sc
