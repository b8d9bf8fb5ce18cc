"""Scenes and texel sets of the image-update tests (tests/test_image_update_host.py on the host, tests/test_gpu_image_update.py on the device): a floor under a light, seen at a
grazing angle as in tests/filtering_scenes.py, whose material and / or environment map read registered images; and a numpy restatement of the mip pyramid
(MIPMap::CompileToBinary, Engine/MIPMap.cpp:41-95) that the library's ctl_mip_pyramid_host is held to."""
import ctypes as C

import numpy as np

from cudatracerlib_amd import api

W = H = 64                                      # the frames
PYRAMID_SIZES = [(1, 1), (2, 2), (4, 2), (5, 3), (8, 8), (64, 32)]            # (width, height)
ENV_SIZES = [(1, 2), (4, 2), (67, 33), (64, 63), (64, 64), (64, 65)]          # (width, height): row counts on both sides of a wave, a one-column map


# ------------------------------------------------------------------------------------------------ texels
def rgbcol_texels(w, h, seed):
    rs = np.random.RandomState(seed)
    t = rs.randint(0, 256, size=(h, w, 4)).astype(np.uint32)
    return t[..., 0] | (t[..., 1] << 8) | (t[..., 2] << 16) | (t[..., 3] << 24)


def rgbe_texels(w, h, seed, extremes=True):
    """RGBE words with every mantissa byte; extremes: a share of texels with exponent byte 0 (which decodes to black whatever the mantissa), exponent bytes 1 .. 3 (2^-135 ..:
    denormal factors, far below the encoder's 1e-32 cut) and exponent bytes 253 .. 255 (2^117 .. 2^119).  The mantissas of the latter stay below 128, so that the sum of a
    2 x 2 block stays below 2^128: past it the average is infinite, and the reference's conversion of the resulting NaN to a byte is undefined"""
    rs = np.random.RandomState(seed)
    m = rs.randint(0, 256, size=(h, w, 3)).astype(np.uint32)
    e = rs.randint(110, 140, size=(h, w)).astype(np.uint32)
    if extremes:
        kind = rs.randint(0, 8, size=(h, w))
        e = np.where(kind == 0, 0, e); e = np.where(kind == 1, rs.randint(1, 4, size=(h, w)), e)
        hi = kind == 2
        e = np.where(hi, rs.randint(253, 256, size=(h, w)), e).astype(np.uint32)
        m = np.where(hi[..., None], m & 127, m)
    return (m[..., 0] | (m[..., 1] << 8) | (m[..., 2] << 16) | (e << 24)).astype(np.uint32)


def bright_rgbe(w, h, seed):
    """an environment map whose every texel, and so every row, has positive luminance"""
    rs = np.random.RandomState(seed)
    return api.float3_to_rgbe(rs.uniform(0.05, 4.0, size=(h, w, 3)).astype(np.float32) * (1.0 + 8.0 * (rs.uniform(size=(h, w, 1)) > 0.9)).astype(np.float32))


def bright_rgbcol(w, h, seed):
    rs = np.random.RandomState(seed)
    c = rs.uniform(0.05, 0.95, size=(h, w, 3)).astype(np.float32)
    c[::2, ::2] *= 0.2                          # high-frequency content: the pyramid's levels differ from level 0's mean seen through a pixel
    return api.float3_to_rgbcol(c)


# ------------------------------------------------------------------------------------------------ the pyramid, restated
def _decode(t, texel_type):
    f32 = np.float32
    x, y, z, w = (t & 0xff).astype(f32), ((t >> 8) & 0xff).astype(f32), ((t >> 16) & 0xff).astype(f32), (t >> 24).astype(np.int32)
    if texel_type == api.TEXEL_RGBE:
        e = np.ldexp(f32(1.0), w - 136).astype(f32)
        c = np.stack([x * e, y * e, z * e], -1).astype(f32)
        c[w == 0] = 0
        return c
    return np.stack([x / f32(255.0), y / f32(255.0), z / f32(255.0)], -1).astype(f32)


def _encode(c, texel_type):
    f32 = np.float32
    if texel_type == api.TEXEL_RGBE:
        mx = np.maximum(c[..., 0], np.maximum(c[..., 1], c[..., 2]))
        m, e = np.frexp(mx.astype(np.float64))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):      # texels below the cut: their factor is not used
            k = ((m.astype(f32) * f32(256.0)) / mx).astype(f32)
        ok = mx.astype(np.float64) >= 1e-32
        q = np.zeros(c.shape, np.uint32)
        q[ok] = (c[ok] * k[ok][:, None]).astype(f32).astype(np.uint32) & 0xff
        out = q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | (((e + 128).astype(np.uint32) & 0xff) << 24)
        return np.where(ok, out, 0).astype(np.uint32)
    q = (np.clip(c, f32(0.0), f32(1.0)) * f32(255.0)).astype(f32).astype(np.uint32) & 0xff
    return (q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | np.uint32(255 << 24)).astype(np.uint32)


def numpy_pyramid(texels, texel_type):
    """dict(texels, levels, offsets) as api.mip_pyramid_host returns them: nLevels = 1 + floor(log2(min(w, h))), level l = the 2 x 2 box average of level l - 1 — decoded,
    summed ((a + b) + c) + e in fp32, times 0.25, re-encoded; an odd width or height drops the last column or row"""
    t = np.ascontiguousarray(texels, np.uint32)
    h, w = t.shape
    levels = 1 + int(np.floor(np.log2(min(w, h))))
    out = [t.reshape(-1)]; offsets = np.zeros(15, np.uint32); o = w * h
    for l in range(1, levels):
        j, k = t.shape[1] // 2, t.shape[0] // 2
        a, b, c, e = (_decode(t[dy:2 * k:2, dx:2 * j:2], texel_type) for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)))
        s = (((a + b).astype(np.float32) + c).astype(np.float32) + e).astype(np.float32)
        t = _encode((np.float32(0.25) * s).astype(np.float32), texel_type)
        offsets[l - 1] = o; o += j * k
        out.append(t.reshape(-1))
    return dict(texels=np.concatenate(out), levels=levels, offsets=offsets)


# ------------------------------------------------------------------------------------------------ scenes
def floor_scene(kind, tex=None, env=None, tex_type=api.TEXEL_RGBCOL, env_type=api.TEXEL_RGBE, wrap=api.WRAP_REPEAT, filter_mode=api.FILTER_ANISOTROPIC, w=W, h=H):
    """The DynamicScene (.desc after this call; .images = {"tex": index, "env": index}).  kind:
         "textured"      a diffuse floor whose reflectance is image `tex`, under an area light: no material reads the image's average
         "plastic"       a plastic floor whose diffuse reflectance is image `tex`, under an area light
         "roughcoating"  a rough coating over a diffuse floor whose sigmaA is image `tex`, under an area light (host only: no transmittance table)
         "env"           a diffuse floor under the environment map `env`
         "both"          ONE image, `tex`, as the plastic floor's diffuse reflectance and as the environment map
         "floor_env"     the plastic floor over `tex` under the environment map `env` and the area light: the scene of the device tests"""
    sc = api.DynamicScene()
    sc.images = {}
    if kind != "env":
        sc.images["tex"] = sc.add_image(tex, tex_type, wrap, filter_mode)
    if kind in ("env", "floor_env"):
        sc.images["env"] = sc.add_image(env, env_type, api.WRAP_REPEAT, api.FILTER_BILINEAR)
    if kind == "both":
        sc.images["env"] = sc.images["tex"]
    P = np.array([[-40, 0, -40], [-40, 0, 40], [40, 0, 40], [40, 0, -40]], np.float32)
    uv = np.array([[0, 0], [0, 12], [12, 12], [12, 0]], np.float32)
    if kind == "env":
        floor = api.diffuse((0.6, 0.6, 0.6))
    elif kind == "textured":
        floor = api.diffuse((1, 1, 1)); floor.tex[0] = api.image_texture(sc.images["tex"])
    elif kind == "roughcoating":
        inner = api.diffuse((0.5, 0.5, 0.5)); ii = sc.add_material(inner)
        floor = api.roughcoating(ii, inner, alpha=0.1, thickness=1.3, sigma_a=api.image_texture(sc.images["tex"], scale=(0.9, 0.8, 0.7)))
    else:
        floor = api.plastic(api.image_texture(sc.images["tex"]), specular_reflectance=0.6)
    sc.CreateNode(sc.add_mesh(P, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=np.tile(np.array([0, 1, 0], np.float32), (4, 1)), uvs=uv, materials=[floor]))
    if kind != "env":
        L = np.array([[-6, 12, -6], [6, 12, -6], [6, 12, 6], [-6, 12, 6]], np.float32)
        ln = sc.CreateNode(sc.add_mesh(L, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=np.tile(np.array([0, -1, 0], np.float32), (4, 1)), materials=[api.diffuse((0.5, 0.5, 0.5))]))
        sc.CreateLight(ln, 0, (30.0, 30.0, 30.0))
    if "env" in sc.images:
        sc.setEnvironementMap(sc.images["env"], (1.0, 0.9, 0.8))
    sc.setCamera((0, 1.5, -30), (0, 0.5, 0), (0, 1, 0), 50.0, w, h)
    sc.UpdateScene()
    return sc


def desc_bytes(d):
    """the parts of a description an image update may touch, as bytes: materials, lights, anim blob, and the level-0 texels of every image"""
    out = dict(materials=np.frombuffer(C.string_at(d.materials, d.n_materials * C.sizeof(api.ctl_material)), np.uint8) if d.n_materials else np.zeros(0, np.uint8),
               lights=np.frombuffer(C.string_at(d.lights, d.n_lights_buf * C.sizeof(api.ctl_light)), np.uint8) if d.n_lights_buf else np.zeros(0, np.uint8),
               anim=np.frombuffer(C.string_at(d.anim, d.n_anim_bytes), np.uint8) if d.n_anim_bytes else np.zeros(0, np.uint8))
    for i in range(d.n_images):
        im = d.images[i]
        out["texels%d" % i] = np.frombuffer(C.string_at(im.texels, im.width * im.height * 4), np.uint8)
    return out


def light_tables(d):
    """dict(lights, anim) of a description in the layout of Scene.read_lights"""
    L = np.frombuffer(C.string_at(d.lights, d.n_lights_buf * C.sizeof(api.ctl_light)), np.uint32).reshape(d.n_lights_buf, -1).copy()
    A = np.frombuffer(C.string_at(d.anim, d.n_anim_bytes), np.uint8).copy()
    return dict(lights=L, anim=A)


class DeviceTexels:
    """an (h, w) uint32 array copied into device memory of the library's allocator (ctl_device_malloc), as a host that decodes or paints on the device holds it"""

    def __init__(self, texels):
        t = np.ascontiguousarray(texels, np.uint32)
        self.width, self.height = t.shape[1], t.shape[0]
        self.ptr = C.c_void_p()
        api._check(api.lib.ctl_device_malloc(C.c_size_t(t.nbytes), C.byref(self.ptr)))
        api._check(api.lib.ctl_memcpy_h2d(self.ptr, t.ctypes.data_as(C.c_void_p), C.c_size_t(t.nbytes)))

    def __del__(self):
        if getattr(self, "ptr", None):
            api.lib.ctl_device_free(self.ptr); self.ptr = None
