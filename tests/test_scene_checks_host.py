"""ctl_scene_desc_check: what ctl_scene_create and ctl_scene_update refuse a description for, and which shade-kernel build they select for it, without a device
(csrc/scene_checks.cpp, the classifiers of csrc/device_scene.h).  The malformed descriptions and the messages they are refused with: tests/scene_check_cases.py;
tests/test_gpu_scene_update.py holds the scene itself to the same answers."""
import pytest

from cudatracerlib_amd import api
import scene_check_cases as K

ALL_PARTS = (api.DIFF_CAMERA, api.DIFF_MATERIALS, api.DIFF_LIGHTS, api.DIFF_TRANSFORMS, api.DIFF_TOPOLOGY)
# the kShade* bits (csrc/device_scene.h)
MORE_BSDFS, ROUGH_BSDFS, IMAGE_TEXTURES, MORE_LIGHTS, NESTING, SURFACE_MAPS, MORE_MICROFACET = 1, 2, 4, 8, 16, 32, 64
BECKMANN, GGX, PHONG = 0, 1, 2


@pytest.mark.parametrize("which", ["cornell", "textured"])
def test_valid_descriptions_pass(which):
    d = K.base(which).desc
    api.scene_desc_check(d)
    for part in ALL_PARTS:
        api.scene_desc_check(d, part)
    with pytest.raises(api.CtlError):
        api.scene_desc_check(d, 32)                               # no such part


@pytest.mark.parametrize("name", K.CASE_NAMES)
def test_refusals(name):
    d, parts, message = K.make(name)
    if message is None:
        api.scene_desc_check(d, parts)
        return
    with pytest.raises(api.CtlError) as e:
        api.scene_desc_check(d, parts)
    assert e.value.code == api.ERR_INVALID and str(e.value).endswith(message) and api.lib.ctl_last_error().decode() == message, (str(e.value), message)


def test_the_prefix_names_the_caller():
    d, _, message = K.make("unknown BSDF type")
    for parts, who in ((0, K.CREATE), (api.DIFF_MATERIALS, K.UPDATE)):
        with pytest.raises(api.CtlError) as e:
            api.scene_desc_check(d, parts)
        assert api.lib.ctl_last_error().decode() == who + message[len(K.CREATE):]


def test_only_the_parts_asked_for_are_checked():
    d, _, _ = K.make("unknown light type")
    api.scene_desc_check(d, api.DIFF_CAMERA)
    api.scene_desc_check(d, api.DIFF_CAMERA | api.DIFF_MATERIALS | api.DIFF_TRANSFORMS)
    with pytest.raises(api.CtlError):
        api.scene_desc_check(d, api.DIFF_LIGHTS)
    d, _, _ = K.make("unknown BSDF type")
    api.scene_desc_check(d, api.DIFF_LIGHTS | api.DIFF_CAMERA)
    d, _, _ = K.make("forward transform not affine")
    api.scene_desc_check(d, api.DIFF_MATERIALS | api.DIFF_LIGHTS | api.DIFF_CAMERA)
    d, _, _ = K.make("bad sensor type")
    api.scene_desc_check(d, api.DIFF_MATERIALS | api.DIFF_LIGHTS | api.DIFF_TRANSFORMS)


# ---- the classifier.  Every material of the description is the one under test (nesting models: material 0 is the diffuse they nest), so the state is that material's.
def state_of_material(which, model, edit=None, parts=0):
    d = K.copy_of(K.base(which).desc)
    mats = K.materials(d)
    proto = api.ctl_material.from_buffer_copy(mats[0])
    proto.bsdf_type = K.BSDF[model]
    proto.map_kind = 0; proto.alpha_state = 0; proto.u[0] = proto.u[1] = proto.u[2] = proto.u[3] = 0
    for k in range(4):
        proto.tex[k].type = K.TEX_CONSTANT
    if edit:
        edit(proto)
    plain = api.ctl_material.from_buffer_copy(proto); plain.bsdf_type = K.BSDF["diffuse"]; plain.map_kind = plain.alpha_state = 0
    for k in range(4):
        plain.tex[k].type = K.TEX_CONSTANT
    for i in range(d.n_materials):
        mats[i] = proto
    nesting = model in ("coating", "roughcoating", "blend")
    if nesting:
        mats[0] = plain
    lights = K.lights(d)                                          # lights that need nothing: the state is the material's alone
    for i in range(d.n_lights_buf):
        lights[i].type = K.LIGHT["point"]
    d.env_map_index = 0xffffffff
    s = api.scene_desc_check(d, parts)
    assert s["models"] == (1 << K.BSDF[model]) | ((1 << K.BSDF["diffuse"]) if nesting else 0), (model, s)
    return s["features"], s["alpha_maps"]


MODEL_BITS = dict(diffuse=0, dielectric=0, conductor=0, roughconductor=0,
                  thindielectric=MORE_BSDFS, roughdielectric=MORE_BSDFS, plastic=MORE_BSDFS, phong=MORE_BSDFS,
                  roughdiffuse=ROUGH_BSDFS, ward=ROUGH_BSDFS, roughplastic=ROUGH_BSDFS,
                  coating=NESTING | MORE_BSDFS | ROUGH_BSDFS, roughcoating=NESTING | MORE_BSDFS | ROUGH_BSDFS, blend=NESTING | MORE_BSDFS | ROUGH_BSDFS)
# the word that holds the microfacet distribution, for the models that have one
DISTRIBUTION_WORD = dict(roughconductor=0, roughdielectric=0, roughcoating=0, roughplastic=2)


@pytest.mark.parametrize("model", sorted(MODEL_BITS))
def test_material_features(model):
    assert len(MODEL_BITS) == 14
    # GGX needs no more than the model does; transmittance tables exist in slots 0 and 1 of the textured scene, so these descriptions are valid ones (parts = 0)
    ggx = (lambda M: M.u.__setitem__(DISTRIBUTION_WORD[model], GGX)) if model in DISTRIBUTION_WORD else None
    assert state_of_material("textured", model, ggx) == (MODEL_BITS[model], 0)

    def image(M): M.tex[2].type = K.TEX_IMAGE; M.tex[2].image = 0; ggx and ggx(M)
    def checker(M): M.tex[1].type = K.TEX_CHECKER; ggx and ggx(M)
    def normal_map(M): M.map_kind = 1; M.map_tex.type = K.TEX_CONSTANT; ggx and ggx(M)
    def height_map(M): M.map_kind = 2; M.map_tex.type = K.TEX_IMAGE; M.map_tex.image = 0; ggx and ggx(M)
    def alpha(M): M.alpha_state = 5; M.alpha_tex.type = K.TEX_CONSTANT; ggx and ggx(M)
    def idle_map_image(M): M.map_kind = 0; M.map_tex.type = K.TEX_IMAGE; M.map_tex.image = 0; ggx and ggx(M)
    assert state_of_material("textured", model, image) == (MODEL_BITS[model] | IMAGE_TEXTURES, 0)
    assert state_of_material("textured", model, checker) == (MODEL_BITS[model], 0)
    assert state_of_material("textured", model, normal_map) == (MODEL_BITS[model] | SURFACE_MAPS | IMAGE_TEXTURES, 0)
    assert state_of_material("textured", model, height_map) == (MODEL_BITS[model] | SURFACE_MAPS | IMAGE_TEXTURES, 0)
    assert state_of_material("textured", model, alpha) == (MODEL_BITS[model], 1)
    assert state_of_material("textured", model, idle_map_image) == (MODEL_BITS[model], 0)


@pytest.mark.parametrize("model", sorted(MODEL_BITS))
@pytest.mark.parametrize("distribution,visible,more", [(BECKMANN, 0, False), (BECKMANN, 1, True), (GGX, 0, False), (GGX, 1, False), (PHONG, 0, True), (PHONG, 1, True)])
def test_microfacet_features(model, distribution, visible, more):
    """the Phong distribution and Beckmann with visible-normal sampling need the full build — for the four microfacet models, in the word that holds their distribution;
    the same words mean something else to every other model (a blend's u[2] is a material index) and set nothing there"""
    nesting = model in ("coating", "roughcoating", "blend")

    def edit(M):
        M.u[1] = visible
        if model in DISTRIBUTION_WORD:
            M.u[DISTRIBUTION_WORD[model]] = distribution
        elif not nesting:
            M.u[0] = M.u[2] = distribution
    # (no table in the Phong slot: checked as a camera-only update would, which leaves the materials alone — the state is derived all the same)
    parts = api.DIFF_CAMERA if (distribution == PHONG and model in ("roughplastic", "roughcoating")) else 0
    want = MODEL_BITS[model] | (MORE_MICROFACET if more and model in DISTRIBUTION_WORD else 0)
    assert state_of_material("textured", model, edit, parts) == (want, 0)


LIGHT_CASES = {
    "point": (lambda L: setattr(L, "type", 1), 0),
    "plain area light": (lambda L: (setattr(L, "type", 2), setattr(L, "orthogonal", 0), setattr(L.rad_texture, "type", 0)), 0),
    "area light, constant texture": (lambda L: (setattr(L, "type", 2), setattr(L, "orthogonal", 0), setattr(L.rad_texture, "type", K.TEX_CONSTANT)), 0),
    "orthogonal area light": (lambda L: (setattr(L, "type", 2), setattr(L, "orthogonal", 1), setattr(L.rad_texture, "type", 0)), MORE_LIGHTS),
    "checker area light": (lambda L: (setattr(L, "type", 2), setattr(L, "orthogonal", 0), setattr(L.rad_texture, "type", K.TEX_CHECKER)), MORE_LIGHTS),
    "image area light": (lambda L: (setattr(L, "type", 2), setattr(L, "orthogonal", 0), setattr(L.rad_texture, "type", K.TEX_IMAGE), setattr(L.rad_texture, "image", 0)), MORE_LIGHTS | IMAGE_TEXTURES),
    "distant": (lambda L: setattr(L, "type", 3), MORE_LIGHTS),
    "spot": (lambda L: setattr(L, "type", 4), MORE_LIGHTS),
    "infinite": (lambda L: (setattr(L, "type", 5), setattr(L, "env_image", 0)), MORE_LIGHTS),
}


@pytest.mark.parametrize("kind", sorted(LIGHT_CASES))
def test_light_features(kind):
    """the Cornell box has diffuse materials only (no bit of their own) and one light record: the state is that light's"""
    edit, want = LIGHT_CASES[kind]
    d = K.copy_of(K.base("cornell").desc)
    assert d.n_lights_buf == 1 and api.scene_desc_check(d) == {"features": 0, "models": 1 << K.BSDF["diffuse"], "alpha_maps": 0}
    edit(K.lights(d)[0])
    # (the Cornell box has no image for an image light to name: lights unchecked, state derived)
    s = api.scene_desc_check(d, 0 if kind not in ("image area light", "infinite") else api.DIFF_CAMERA)
    assert s == {"features": want, "models": 1 << K.BSDF["diffuse"], "alpha_maps": 0}, (kind, s)
