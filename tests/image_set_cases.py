"""The edits of the image-set tests (tests/test_image_set_host.py on the host, tests/test_gpu_image_set.py on the device): scenes whose image set changes — images added,
removed and replaced by ones of another size — and, for each edit, a builder that made the final image set from the start.  Sizes from image_update_cases.PYRAMID_SIZES,
the smallest at which a boundary can be wrong: 1 x 1 (a one-texel pyramid: a run can be one texel long), 2 x 2, 4 x 2, 5 x 3 (odd, 17 texels: no multiple of 16 B), 8 x 8
and 64 x 32; both texel types."""
import ctypes as C

import numpy as np

from cudatracerlib_amd import api
import image_update_cases as K

NONE = 0xffffffff
S11, S22, S42, S53, S88, S6432 = K.PYRAMID_SIZES


def spec(size, texel_type, seed):
    """an image of the cases: (width, height), texel type, seed of its texels"""
    return (tuple(size), texel_type, seed)


def texels_of(s):
    (w, h), texel_type, seed = s
    return K.rgbe_texels(w, h, seed) if texel_type == api.TEXEL_RGBE else K.rgbcol_texels(w, h, seed)


def _mixed(n, first_seed, sizes=K.PYRAMID_SIZES):
    return [spec(sizes[i % len(sizes)], api.TEXEL_RGBE if i % 2 else api.TEXEL_RGBCOL, first_seed + i) for i in range(n)]


def _forty():
    rs = np.random.RandomState(40)
    removed = sorted(rs.choice(40, 13, replace=False).tolist(), reverse=True)
    return _mixed(40, 400, K.PYRAMID_SIZES[:5]), [("remove", i) for i in removed]


# name -> (the images the scene starts with, the operations in the order the host calls them).  ("remove", index), ("replace", index, spec), ("add", spec): indices as
# they stand when the operation runs
EDITS = {
    "add the first image": ([], [("add", spec(S42, api.TEXEL_RGBCOL, 1))]),
    "remove the only image": ([spec(S53, api.TEXEL_RGBE, 2)], [("remove", 0)]),
    "remove the first of three": ([spec(S11, api.TEXEL_RGBCOL, 3), spec(S53, api.TEXEL_RGBE, 4), spec(S88, api.TEXEL_RGBCOL, 5)], [("remove", 0)]),
    "remove the middle of three": ([spec(S11, api.TEXEL_RGBCOL, 3), spec(S53, api.TEXEL_RGBE, 4), spec(S88, api.TEXEL_RGBCOL, 5)], [("remove", 1)]),
    "remove the last of three": ([spec(S11, api.TEXEL_RGBCOL, 3), spec(S53, api.TEXEL_RGBE, 4), spec(S88, api.TEXEL_RGBCOL, 5)], [("remove", 2)]),
    "remove every second of seven": (_mixed(7, 10), [("remove", 5), ("remove", 3), ("remove", 1)]),
    "replace the middle image, 4x2 by 5x3": ([spec(S22, api.TEXEL_RGBE, 20), spec(S42, api.TEXEL_RGBCOL, 21), spec(S88, api.TEXEL_RGBE, 22)], [("replace", 1, spec(S53, api.TEXEL_RGBCOL, 23))]),
    "replace the middle image, 8x8 by 2x2": ([spec(S53, api.TEXEL_RGBCOL, 24), spec(S88, api.TEXEL_RGBE, 25), spec(S11, api.TEXEL_RGBE, 26)], [("replace", 1, spec(S22, api.TEXEL_RGBE, 27))]),
    "append two": ([spec(S42, api.TEXEL_RGBE, 30), spec(S53, api.TEXEL_RGBCOL, 31)], [("add", spec(S6432, api.TEXEL_RGBCOL, 32)), ("add", spec(S11, api.TEXEL_RGBE, 33))]),
    "remove, replace and append in one edit": (_mixed(5, 50, K.PYRAMID_SIZES[:5]),
                                               [("remove", 1), ("replace", 2, spec(S6432, api.TEXEL_RGBE, 56)),      # (a replaced image keeps its texel type)
                                                ("add",spec(S22, api.TEXEL_RGBE, 57)), ("add", spec(S53, api.TEXEL_RGBCOL, 58))]),
    "forty small images, thirteen removed": _forty(),
}
EDIT_NAMES = list(EDITS)


def final_specs(name):
    """the image set after the edit, as a builder would register it from the start, and per final image the index it had before the edit (NONE: fresh)"""
    start, ops = EDITS[name]
    now = [(s, i) for i, s in enumerate(start)]
    for op in ops:
        if op[0] == "remove":
            del now[op[1]]
        elif op[0] == "replace":
            now[op[1]] = (op[2], NONE)
        else:
            now.append((op[1], NONE))
    return [s for s, _ in now], [o for _, o in now]


def base_scene(specs, w=K.W, h=K.H):
    """a grey floor under an area light with the images `specs` registered (no material reads them: every one of them can be removed).  .desc after this call"""
    sc = api.DynamicScene()
    for s in specs:
        sc.add_image(texels_of(s), s[1], api.WRAP_REPEAT, api.FILTER_TRILINEAR)
    P = np.array([[-40, 0, -40], [-40, 0, 40], [40, 0, 40], [40, 0, -40]], np.float32)
    uv = np.array([[0, 0], [0, 12], [12, 12], [12, 0]], np.float32)
    sc.CreateNode(sc.add_mesh(P, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=np.tile(np.array([0, 1, 0], np.float32), (4, 1)), uvs=uv, materials=[api.diffuse((0.6, 0.6, 0.6))]))
    L = np.array([[-6, 12, -6], [6, 12, -6], [6, 12, 6], [-6, 12, 6]], np.float32)
    ln = sc.CreateNode(sc.add_mesh(L, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=np.tile(np.array([0, -1, 0], np.float32), (4, 1)), materials=[api.diffuse((0.5, 0.5, 0.5))]))
    sc.CreateLight(ln, 0, (30.0, 30.0, 30.0))
    sc.setCamera((0, 1.5, -30), (0, 0.5, 0), (0, 1, 0), 50.0, w, h)
    sc.UpdateScene()
    return sc


def apply_edit(sc, name):
    """the operations of the edit on a builder made by base_scene(EDITS[name][0]); finalizes"""
    for op in EDITS[name][1]:
        if op[0] == "remove":
            sc.remove_image(op[1])
        elif op[0] == "replace":
            sc.replace_image(op[1], texels_of(op[2]))
        else:
            sc.add_image(texels_of(op[1]), op[1][1], api.WRAP_REPEAT, api.FILTER_TRILINEAR)
    return sc.UpdateScene()


def id_map(old_desc, new_desc):
    """old_image_of_new from the stable image ids of two descriptions of one builder: what Scene.update_image_set computes"""
    index = {i: k for k, i in enumerate(old_desc.image_ids)}
    return [index.get(i, NONE) for i in new_desc.image_ids]


def image_records(d):
    """(width, height, texel type, wrap, filter) of every image of a description"""
    return [(int(m.width), int(m.height), int(m.texel_type), int(m.wrap_mode), int(m.filter_mode)) for m in (d.images[i] for i in range(d.n_images))]


def builder_state(d):
    """everything of a finalized description an edit of the image set or the material table may touch, as bytes and counts"""
    out = K.desc_bytes(d)
    out["image_records"] = np.array(image_records(d), np.uint32).reshape(-1, 5)
    out["counts"] = np.array([d.n_images, d.n_materials, d.n_lights_buf, d.n_anim_bytes, d.n_nodes, d.n_meshes, d.env_map_index], np.uint32)
    return out


def same_state(a, b):
    return sorted(a) == sorted(b) and all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


def pyramids(specs):
    """per image the pyramid a scene keeps of it (image_update_cases.numpy_pyramid: texels, levels, offsets)"""
    return [K.numpy_pyramid(texels_of(s), s[1]) for s in specs]


def numpy_runs(old_sizes, new_sizes, image_map):
    """the run table restated: rows of (first destination texel, first source texel, length, kept texels in front), then the sentinel — a run is a maximal group of kept
    images that are consecutive in the old pool and in the new one"""
    old_off = np.concatenate([[0], np.cumsum(old_sizes)]).astype(np.uint64); new_off = np.concatenate([[0], np.cumsum(new_sizes)]).astype(np.uint64)
    runs, moved, prev = [], 0, None
    for j, o in enumerate(image_map):
        if o == NONE:
            prev = None
            continue
        if prev is None or o != prev + 1:
            runs.append([int(new_off[j]), int(old_off[o]), 0, moved])
        runs[-1][2] += int(new_sizes[j]); moved += int(new_sizes[j]); prev = o
    runs.append([int(new_off[-1]), int(old_off[-1]), 0, moved])
    return np.array(runs, np.uint64).reshape(-1, 4)


def material_offset(d, node):
    """ctl_node::material_offset of a node of a description"""
    return int(d.view("nodes", np.uint32, d.n_nodes, 6)[node, 1])
