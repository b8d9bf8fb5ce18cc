"""Malformed scene descriptions and the message each is refused with, shared by tests/test_scene_checks_host.py (ctl_scene_desc_check, no device) and
tests/test_gpu_scene_update.py (the same descriptions through ctl_scene_create_ex / ctl_scene_update).

A case is (name, base, patch, parts, message): `patch` edits a ctypes copy of the base description (private copies of the arrays it touches), `parts` is what
ctl_scene_desc_check is asked (0: as creation checks, else DIFF_* bits: as an update that found them checks) and `message` the text behind the "ctl_scene_create: " /
"ctl_scene_update: " prefix.  The messages are those the library gave before the checks were gathered in csrc/scene_checks.cpp (written out here, not derived).

Bases: "cornell" = scenes.cornell_box(64, 64): diffuse materials, one plain area light, no image, no transmittance table.
       "textured" = a miniature scenes.synthetic_bathroom: image textures, a height map, rough plastics / conductors / dielectrics, a coating, transmittance tables in
       slots 0 and 1 (none for the Phong distribution, slot 2), an area light and an InfiniteLight."""
import ctypes as C
import functools

import numpy as np

from cudatracerlib_amd import api, scenes

CREATE, UPDATE = "ctl_scene_create: ", "ctl_scene_update: "
STACK = 96                                                    # kStackSize (csrc/device_scene.h)
BSDF = dict(diffuse=1, roughdiffuse=2, dielectric=3, thindielectric=4, roughdielectric=5, conductor=6, roughconductor=7, plastic=8, roughplastic=9, phong=10, ward=11, hk=12,
            coating=13, roughcoating=14, blend=15)            # CTL_BSDF_*
LIGHT = dict(point=1, diffuse=2, distant=3, spot=4, infinite=5)   # CTL_LIGHT_*
TEX_CONSTANT, TEX_CHECKER, TEX_IMAGE = 2, 3, 4


class ctl_node(C.Structure):
    _fields_ = [("mesh_index", api.u32), ("material_offset", api.u32), ("instanciated_material", api.u32), ("lights", api.u32 * 2), ("n_lights", api.u32)]


@functools.lru_cache(maxsize=None)
def base(name):
    """the builders are kept (a description points into its builder) and never edited: every case works on a copy"""
    if name == "cornell":
        return scenes.cornell_box(64, 64)
    return scenes.synthetic_bathroom(32, 32, n_instances=12, subdiv=1)


def copy_of(desc):
    d = api.ctl_scene_desc.from_buffer_copy(desc)
    d._keep = [desc]
    return d


def own(d, field, ctype, count):
    """give the copy `d` a private copy of one of its arrays and return it (a ctypes array of `ctype`)"""
    arr = (ctype * max(1, count))()
    src = getattr(d, field)
    if count:
        C.memmove(arr, src, C.sizeof(ctype) * count)
    setattr(d, field, C.cast(arr, type(src)) if not isinstance(src, (int, type(None))) else C.addressof(arr))
    d._keep.append(arr)
    return arr


def materials(d):
    return own(d, "materials", api.ctl_material, d.n_materials)


def lights(d):
    return own(d, "lights", api.ctl_light, d.n_lights_buf)


def first_material(d, model):
    return [i for i in range(d.n_materials) if d.materials[i].bsdf_type == BSDF[model]][0]


def first_light(d, kind):
    return [i for i in range(d.n_lights_buf) if d.lights[i].type == LIGHT[kind]][0]


def with_top_level(desc, nodes, start):
    """a copy of `desc` with another scene BVH: nodes (n, 16) uint32 in the reference's BVHNodeData layout (child links in words 12 and 13)"""
    d = copy_of(desc)
    buf = np.ascontiguousarray(nodes, np.uint32)
    d.scene_bvh_nodes = buf.ctypes.data; d.n_scene_bvh_nodes = len(buf); d.scene_start_node = start
    d._keep.append(buf)
    return d


def chain(desc, n, last_link, leaf=0):
    """n nodes, each with scene node `leaf` as its first child (a leaf) and the next chain node as its second; both child boxes = the scene box"""
    lo, hi = np.array(desc.box_min[:], np.float32), np.array(desc.box_max[:], np.float32)
    nodes = np.zeros((n, 16), np.uint32); f = nodes.view(np.float32)
    f[:, 0:4] = f[:, 4:8] = (lo[0], hi[0], lo[1], hi[1]); f[:, 8:12] = (lo[2], hi[2], lo[2], hi[2])
    nodes[:, 12] = np.uint32(~leaf & 0xffffffff)
    nodes[:, 13] = (np.arange(1, n + 1) * 4).astype(np.uint32); nodes[-1, 13] = np.uint32(last_link & 0xffffffff)
    return nodes


def mesh_bvh_depth(desc):
    """the deepest mesh BVH, walked here in numpy: inner links are float4 indices relative to the mesh's first node"""
    N = desc.view("bvh_nodes", np.int32, desc.n_bvh_nodes, 16)
    M = desc.view("meshes", np.uint32, desc.n_meshes, 5)
    best = 0
    for m in range(desc.n_meshes):
        first = int(M[m, 1]) // 4
        todo = [(0, 1)]
        while todo:
            i, depth = todo.pop()
            best = max(best, depth)
            todo += [(int(c) // 4, depth + 1) for c in N[first + i, 12:14] if c >= 0 and c != 0x76543210]
    return best


# ---- the patches: each takes the copy and edits it in place
def _transform(field, word, value):
    def patch(d):
        a = own(d, field, api.ctl_float4x4, d.n_nodes); a[d.n_nodes - 1].m[word] = value
    return patch


def _missing_mesh(d):
    own(d, "nodes", ctl_node, d.n_nodes)[0].mesh_index = d.n_meshes


def _no_nodes(d):
    d.n_nodes = 0


def _sensor(d):
    d.camera.type = 9


def _env_names_area_light(d):
    d.env_map_index = first_light(d, "diffuse")


def _light(kind, edit):
    def patch(d):
        edit(d, lights(d)[first_light(d, kind)])
    return patch


def _light_type(d, L): L.type = 9
def _light_image(d, L): L.rad_texture.type = TEX_IMAGE; L.rad_texture.image = d.n_images
def _env_image(d, L): L.env_image = d.n_images


def _material(model, edit):
    def patch(d):
        i = first_material(d, model)
        edit(d, materials(d)[i], i)
    return patch


def _tex_type(d, M, i): M.tex[0].type = 7
def _tex_image(d, M, i): M.tex[1].type = TEX_IMAGE; M.tex[1].image = d.n_images
def _map_image_off(d, M, i): M.map_kind = 0; M.map_tex.type = TEX_IMAGE; M.map_tex.image = d.n_images
def _map_image_on(d, M, i): M.map_kind = 1; M.map_tex.type = TEX_IMAGE; M.map_tex.image = d.n_images
def _alpha_image_off(d, M, i): M.alpha_state = 0; M.alpha_tex.type = TEX_IMAGE; M.alpha_tex.image = d.n_images
def _alpha_image_on(d, M, i): M.alpha_state = 1; M.alpha_tex.type = TEX_IMAGE; M.alpha_tex.image = d.n_images
def _map_kind(d, M, i): M.map_kind = 3
def _alpha_four(d, M, i): M.alpha_state = 4
def _alpha_eight(d, M, i): M.alpha_state = 8
def _bsdf_hk(d, M, i): M.bsdf_type = BSDF["hk"]
def _nested_range(d, M, i): M.u[2] = d.n_materials
def _nested_nesting(d, M, i): M.u[2] = i
def _roughcoating_phong(d, M, i): M.bsdf_type = BSDF["roughcoating"]; M.u[0] = 2                       # a Phong roughcoating: this scene has no table in slot 2
def _slot(word, value):
    def edit(d, M, i): M.u[word] = value
    return edit


NOT_REFUSED = None
TRANSFORMS = api.DIFF_TRANSFORMS


def _deep_message(desc, hint):
    return "scene BVH depth 120 + mesh BVH depth %d does not fit the traversal stack of %d entries" % (mesh_bvh_depth(desc), STACK) + \
        (" (rebuild the meshes with CTL_BVH_BINNED, whose depth is bounded)" if hint else "")


def _top(make, start=0):
    """a case whose patch replaces the scene BVH: returns a new description instead of editing the copy"""
    def patch(d):
        return with_top_level(d, make(d), start)
    return patch


CASES = [
    ("forward transform not affine", "cornell", _transform("node_transforms", 13, 0.25), 0, "node transforms must be affine"),
    ("inverse transform not affine", "cornell", _transform("node_inv_transforms", 14, 1.0), 0, "node transforms must be affine"),
    ("node names a missing mesh", "cornell", _missing_mesh, 0, "node references a missing mesh"),
    ("no nodes", "cornell", _no_nodes, 0, "scene has no nodes"),
    ("bad sensor type", "cornell", _sensor, 0, "unknown sensor type 9"),
    ("bad sensor type, as an update", "cornell", _sensor, api.DIFF_CAMERA, "unknown sensor type"),
    ("env_map_index names an area light", "textured", _env_names_area_light, 0, "env_map_index does not name an InfiniteLight"),
    ("unknown light type", "cornell", _light("diffuse", _light_type), 0, "unknown light type 9"),
    ("light texture image out of range", "cornell", _light("diffuse", _light_image), 0, "light texture references a missing image"),
    ("env_image out of range", "textured", _light("infinite", _env_image), 0, "InfiniteLight references a missing image"),
    ("unknown texture type", "cornell", _material("diffuse", _tex_type), 0, "texture type 7 has no HIP implementation yet"),
    ("tex[k] image out of range", "textured", _material("roughconductor", _tex_image), 0, "texture references a missing image"),
    ("map image out of range, map disabled", "cornell", _material("diffuse", _map_image_off), 0, NOT_REFUSED),
    ("map image out of range, map enabled", "cornell", _material("diffuse", _map_image_on), 0, "texture references a missing image"),
    ("alpha image out of range, alpha disabled", "cornell", _material("diffuse", _alpha_image_off), 0, NOT_REFUSED),
    ("alpha image out of range, alpha enabled", "cornell", _material("diffuse", _alpha_image_on), 0, "texture references a missing image"),
    ("map_kind beyond HEIGHT", "cornell", _material("diffuse", _map_kind), 0, "unknown surface map kind"),
    ("alpha_state 4", "cornell", _material("diffuse", _alpha_four), 0, "unknown alpha blend state"),
    ("alpha_state beyond the maximum", "cornell", _material("diffuse", _alpha_eight), 0, "unknown alpha blend state"),
    ("unknown BSDF type", "cornell", _material("diffuse", _bsdf_hk), 0, "BSDF type 12 has no HIP implementation yet"),
    ("nested index out of range", "textured", _material("coating", _nested_range), 0, "nested BSDF index out of range or not a simple BSDF (BSDFFirst)"),
    ("nested material is a nesting model", "textured", _material("coating", _nested_nesting), 0, "nested BSDF index out of range or not a simple BSDF (BSDFFirst)"),
    ("roughcoating without its table", "textured", _material("coating", _roughcoating_phong), 0, "roughcoating needs the rough-transmittance table of its distribution"),
    ("roughplastic without its table", "textured", _material("roughplastic", _slot(2, 2)), 0,
     "roughplastic needs the rough-transmittance table of its distribution (ctl_builder_set_rough_transmittance)"),
    ("roughplastic slot above Phong", "textured", _material("roughplastic", _slot(2, 3)), 0, "unknown microfacet distribution"),
    ("roughconductor distribution above Phong", "textured", _material("roughconductor", _slot(0, 3)), 0, "unknown microfacet distribution"),
    ("roughdielectric distribution above Phong", "textured", _material("roughdielectric", _slot(0, 3)), 0, "unknown microfacet distribution"),
    ("scene BVH too deep", "cornell", _top(lambda d: chain(d, 120, ~0)), 0, lambda d: _deep_message(d, True)),
    ("scene BVH too deep, as an update", "cornell", _top(lambda d: chain(d, 120, ~0)), TRANSFORMS, lambda d: _deep_message(d, False)),
    ("scene BVH with a cycle", "cornell", _top(lambda d: chain(d, 8, 0)), 0, "BVH child links form a cycle"),
    ("scene BVH with a cycle, as an update", "cornell", _top(lambda d: chain(d, 8, 0)), TRANSFORMS, "BVH child links form a cycle"),
    ("link outside the array, as an update", "cornell", _top(lambda d: chain(d, 8, 4 * 4000)), TRANSFORMS, "scene BVH child link outside the array"),
    ("start node outside the array, as an update", "cornell", _top(lambda d: chain(d, 8, ~0), start=4 * 4000), TRANSFORMS, "scene BVH start node outside the array"),
    ("leaf names a missing node, as an update", "cornell", _top(lambda d: chain(d, 8, ~0, leaf=d.n_nodes)), TRANSFORMS, "scene BVH leaf names a missing node"),
    # creation walks past a link outside the array (it always has; an update does not): the asymmetry csrc/scene_checks.h records
    ("link outside the array, at creation", "cornell", _top(lambda d: chain(d, 8, 4 * 4000)), 0, NOT_REFUSED),
]
CASE_NAMES = [c[0] for c in CASES]


def make(name):
    """(description, parts, full message or None) of the case `name`"""
    _, which, patch, parts, message = CASES[CASE_NAMES.index(name)]
    d = copy_of(base(which).desc)
    d = patch(d) or d
    if callable(message):
        message = message(d)
    return d, parts, None if message is None else (UPDATE if parts else CREATE) + message
