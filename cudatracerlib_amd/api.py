"""ctypes binding of include/ctl_amd.h with the reference's class/method names.

Every call goes through the C-ABI of libctl_amd.so; nothing here computes radiance, traverses a BVH
or falls back to a CPU path.  Errors of the C layer are raised as ``CtlError`` carrying ``ctl_last_error()``
(the text the reference would have thrown as std::runtime_error, Defines.cpp:15-29).
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# $CTL_AMD_LIB names another build of the same library (tools/build_variant.sh: kernel A/B runs on the GPU box); never a fallback
_LIB_PATH = os.environ.get("CTL_AMD_LIB") or os.path.join(_HERE, "libctl_amd.so")
if not os.path.exists(_LIB_PATH):
    raise ImportError(
        "cudatracerlib_amd: %s is missing — build it with `python -m cudatracerlib_amd.build` "
        "(hipcc --offload-arch=gfx950). There is no CPU fallback." % _LIB_PATH)
lib = C.CDLL(_LIB_PATH)

f32, u32, i32, u8, u64 = C.c_float, C.c_uint32, C.c_int32, C.c_uint8, C.c_uint64
MAX_NUM_LIGHTS = 16
SAMPLER_N1 = 4096 * 30


class CtlError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ctl error %d: %s" % (code, msg))
        self.code = code


# ---------------------------------------------------------------- structs (include/ctl_amd.h)
class ctl_texture(C.Structure):
    _fields_ = [("type", u32), ("value", f32 * 3), ("value1", f32 * 3), ("uv_scale", f32 * 2), ("uv_offset", f32 * 2), ("image", u32)]


class ctl_material(C.Structure):
    _fields_ = [("bsdf_type", u32), ("combined_type", u32), ("two_sided", u32), ("node_light_index", u32),
                ("tex", ctl_texture * 4), ("f", f32 * 8), ("u", u32 * 4),
                ("map_kind", u32), ("alpha_state", u32), ("alpha_test_scalar", f32), ("alpha_test_color", f32 * 3), ("reserved_", u32 * 2),
                ("map_tex", ctl_texture), ("alpha_tex", ctl_texture)]


class ctl_light(C.Structure):
    _fields_ = [("type", u32), ("radiance", f32 * 3), ("area_dist_index", u32), ("triangles_index", u32), ("sum_area", f32), ("count", u32),
                ("orthogonal", u32), ("node_idx", u32), ("position", f32 * 3), ("direction", f32 * 3),
                ("cutoff_angle", f32), ("beam_width", f32), ("cos_cutoff_angle", f32), ("cos_beam_width", f32), ("inv_transition_width", f32),
                ("to_world", f32 * 16), ("env_image", u32), ("env_scale", f32 * 3), ("bsphere_center", f32 * 3), ("bsphere_radius", f32),
                ("cdf_rows_index", u32), ("cdf_cols_index", u32), ("row_weights_index", u32), ("normalization", f32), ("rad_texture", ctl_texture)]


class ctl_mipmap(C.Structure):
    _fields_ = [("texels", C.c_void_p), ("width", u32), ("height", u32), ("texel_type", u32), ("wrap_mode", u32), ("filter_mode", u32)]


class ctl_rough_transmittance(C.Structure):
    _fields_ = [("trans", C.c_void_p), ("diff_trans", C.c_void_p), ("eta_samples", u32), ("alpha_samples", u32), ("theta_samples", u32),
                ("eta_min", f32), ("eta_max", f32), ("alpha_min", f32), ("alpha_max", f32)]


class ctl_sensor(C.Structure):
    _fields_ = [("type", u32), ("to_world", f32 * 16), ("fov", f32), ("near_depth", f32), ("far_depth", f32), ("resolution", f32 * 2),
                ("aperture_radius", f32), ("focus_distance", f32), ("screen_scale", f32 * 2)]


class ctl_float4x4(C.Structure):
    _fields_ = [("m", f32 * 16)]


class ctl_ray(C.Structure):
    _fields_ = [("a", f32 * 4), ("b", f32 * 4)]


class ctl_hit(C.Structure):
    _fields_ = [("dist", f32), ("node_idx", i32), ("tri_idx", i32), ("u", f32), ("v", f32)]


class ctl_pixel_data(C.Structure):
    _fields_ = [("rgb", f32 * 3), ("rgb_splat", f32 * 3), ("weight_sum", f32)]


class ctl_traversal_counts(C.Structure):
    _fields_ = [("n_inner", u64), ("n_tri", u64), ("n_inst", u64), ("wave_inner_iters", u64), ("wave_tri_iters", u64)]


class ctl_tracer_stats(C.Structure):
    _fields_ = [("rays_last_pass", u64), ("rays_total", u64), ("seconds_last_pass", C.c_double), ("seconds_total", C.c_double), ("passes_done", u32),
                ("ms_intersect", C.c_double), ("ms_shade", C.c_double), ("ms_raygen", C.c_double), ("ms_intersect_any", C.c_double),
                ("intersect_rays", u64), ("intersect_launches", u64), ("shadow_rays", u64), ("shadow_launches", u64),
                ("closest_counts", ctl_traversal_counts), ("any_counts", ctl_traversal_counts), ("fused_launches", u64), ("fused_shadow_rays", u64), ("fused_closest_rays", u64), ("ms_fused", C.c_double)]


PHASE_HG, PHASE_ISOTROPIC, PHASE_KAJIYA_KAY, PHASE_RAYLEIGH = 1, 2, 3, 4   # CTL_PHASE_*
VOLUME_HOMOGENEOUS, VOLUME_GRID = 1, 2
MAX_GRID_CELLS = 1 << 22   # CTL_MAX_GRID_CELLS
PARSE_EXTERIOR_MEDIA, PARSE_INTERIOR_MEDIA = 1, 2   # CTL_PARSE_*
MAX_VOL_COUNT = 16


class ctl_phase_function(C.Structure):
    _fields_ = [("type", u32), ("g", f32), ("ks", f32), ("kd", f32), ("exponent", f32), ("normalization", f32)]


class ctl_volume(C.Structure):
    _fields_ = [("type", u32), ("phase", ctl_phase_function), ("volume_to_world", ctl_float4x4), ("world_to_volume", ctl_float4x4),
                ("sig_a", f32 * 3), ("sig_s", f32 * 3), ("le", f32 * 3)]


class ctl_volume_grid(C.Structure):
    _fields_ = [("volume", u32), ("single_grid", u32), ("dim", u32 * 3), ("dim_a", u32 * 3), ("dim_s", u32 * 3),
                ("sig_a_min", f32 * 3), ("sig_a_max", f32 * 3), ("sig_s_min", f32 * 3), ("sig_s_max", f32 * 3), ("le_min", f32 * 3), ("le_max", f32 * 3),
                ("data", C.POINTER(f32)), ("data_a", C.POINTER(f32)), ("data_s", C.POINTER(f32))]


class ctl_scene_desc(C.Structure):
    _fields_ = [("tri_data", C.c_void_p), ("n_tri_data", u32), ("woop", C.c_void_p), ("n_woop", u32), ("woop_index", C.c_void_p),
                ("bvh_nodes", C.c_void_p), ("n_bvh_nodes", u32), ("meshes", C.c_void_p), ("n_meshes", u32), ("nodes", C.c_void_p), ("n_nodes", u32),
                ("materials", C.POINTER(ctl_material)), ("n_materials", u32), ("lights", C.POINTER(ctl_light)), ("n_lights_buf", u32),
                ("anim", C.c_void_p), ("n_anim_bytes", u32), ("scene_start_node", i32), ("scene_bvh_nodes", C.c_void_p), ("n_scene_bvh_nodes", u32),
                ("node_transforms", C.c_void_p), ("node_inv_transforms", C.c_void_p), ("env_map_index", u32),
                ("box_min", f32 * 3), ("box_max", f32 * 3), ("camera", ctl_sensor), ("num_lights", u32),
                ("light_indices", u32 * MAX_NUM_LIGHTS), ("light_cdf", f32 * MAX_NUM_LIGHTS), ("ray_trace_eps", f32),
                ("images", C.POINTER(ctl_mipmap)), ("n_images", u32), ("rough_transmittance", C.POINTER(ctl_rough_transmittance)),
                ("volumes", C.POINTER(ctl_volume)), ("n_volumes", u32), ("volume_grids", C.POINTER(ctl_volume_grid)), ("n_volume_grids", u32)]

    # numpy views of the reference-layout arrays (host memory owned by the builder)
    def view(self, name, dtype, count, width):
        ptr = getattr(self, name)
        if not ptr or not count:
            return np.zeros((0, width), dtype)
        buf = (C.c_char * (count * width * np.dtype(dtype).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype).reshape(count, width)


assert C.sizeof(ctl_volume) == 192 and C.sizeof(ctl_phase_function) == 24 and C.sizeof(ctl_volume_grid) == 144
assert C.sizeof(ctl_texture) == 48 and C.sizeof(ctl_material) == 384 and C.sizeof(ctl_pixel_data) == 28 and C.sizeof(ctl_hit) == 20

lib.ctl_last_error.restype = C.c_char_p
lib.ctl_version.restype = C.c_char_p
lib.ctl_image_device_ptr.restype = C.c_void_p
lib.ctl_image_device_ptr.argtypes = [C.c_void_p]
for _n in ("ctl_builder_destroy", "ctl_scene_destroy", "ctl_image_destroy", "ctl_tracer_destroy", "ctl_sequence_generator_destroy", "ctl_comm_destroy", "ctl_flat_bvh_destroy"):
    getattr(lib, _n).restype = None
    getattr(lib, _n).argtypes = [C.c_void_p]
lib.ctl_builder_update_mesh.argtypes = [C.c_void_p, u32, C.c_void_p, u32, C.c_void_p, u32, C.c_void_p, C.c_void_p]
lib.ctl_scene_bind_skin.argtypes = [C.c_void_p, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, C.c_void_p, C.c_void_p, u32]
lib.ctl_scene_animate_mesh.argtypes = [C.c_void_p, u32, C.c_void_p, C.c_void_p, f32, C.c_void_p]
lib.ctl_scene_get_skin_ms.argtypes = [C.c_void_p, C.POINTER(f32)]
lib.ctl_scene_read_mesh_geometry.argtypes = [C.c_void_p, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.ctl_scene_unbind_skin.argtypes = [C.c_void_p, u32]
lib.ctl_skin_mesh_host.argtypes = [C.c_void_p, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, f32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.ctl_device_malloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
lib.ctl_device_free.argtypes = [C.c_void_p]
lib.ctl_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.ctl_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.ctl_memcpy_d2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.ctl_intersect_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(f32)]
lib.ctl_image_resolve_rgb.argtypes = [C.c_void_p, f32, C.c_void_p]
lib.ctl_image_apply_pipeline_nlm.argtypes = [C.c_void_p, f32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.ctl_image_read_filtered.argtypes = [C.c_void_p, C.c_void_p]
lib.ctl_image_last_filter_ms.argtypes = [C.c_void_p, C.POINTER(f32)]
lib.ctl_image_luminance_info.argtypes = [C.c_void_p, C.c_void_p]
lib.ctl_tracer_set_pixel_variance.argtypes = [C.c_void_p, C.c_int]
lib.ctl_tracer_read_pixel_variance.argtypes = [C.c_void_p, C.c_void_p]
lib.ctl_tracer_set_param_float.argtypes = [C.c_void_p, C.c_char_p, f32]
lib.ctl_builder_add_spot_light.argtypes = [C.c_void_p, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), f32, f32]
lib.ctl_builder_add_distant_light.argtypes = [C.c_void_p, C.POINTER(f32), C.POINTER(f32), f32]
lib.ctl_builder_add_image.argtypes = [C.c_void_p, C.c_void_p, u32, u32, u32, u32, u32, C.POINTER(u32)]
lib.ctl_builder_set_environment_map.argtypes = [C.c_void_p, u32, C.POINTER(f32), C.c_void_p]
lib.ctl_builder_set_camera_lookat.argtypes = [C.c_void_p, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32), f32, u32, u32]
lib.ctl_volume_update.argtypes = [C.POINTER(ctl_volume)]
lib.ctl_builder_create_volume.argtypes = [C.c_void_p, C.POINTER(ctl_volume), C.POINTER(u32)]
lib.ctl_builder_set_volume.argtypes = [C.c_void_p, u32, C.POINTER(ctl_volume)]
lib.ctl_builder_create_volume_grid.argtypes = [C.c_void_p, C.POINTER(u32), u32, C.POINTER(ctl_float4x4), C.POINTER(ctl_phase_function), C.POINTER(u32)]
lib.ctl_builder_set_volume_grid_data.argtypes = [C.c_void_p, u32, u32, C.c_void_p, u32]
lib.ctl_builder_set_volume_grid_coefficients.argtypes = [C.c_void_p, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.ctl_volume_eval.argtypes = [C.c_void_p, i32, C.c_void_p, u32, C.c_void_p, i32]


def _check(code):
    if code != 0:
        raise CtlError(code, lib.ctl_last_error().decode("utf-8", "replace"))


def device_count():
    return int(lib.ctl_device_count())


class ctl_reconstruction_filter(C.Structure):
    _fields_ = [("type", u32), ("x_width", f32), ("y_width", f32), ("p0", f32), ("p1", f32)]


class ctl_tonemap(C.Structure):
    _fields_ = [("key", f32), ("burn", f32)]


def box_filter(xw=1.0, yw=1.0):
    """BoxFilter (SceneTypes/Filter.h:21-37)"""
    return ctl_reconstruction_filter(1, xw, yw, 0.0, 0.0)


def gaussian_filter(xw=2.0, yw=2.0, alpha=-2.0):
    """GaussianFilter (SceneTypes/Filter.h:39-69); the default alpha = -2 is the reference's"""
    return ctl_reconstruction_filter(2, xw, yw, alpha, 0.0)


def mitchell_filter(B=1.0 / 3.0, Cc=1.0 / 3.0, xw=2.0, yw=2.0):
    """MitchellFilter (SceneTypes/Filter.h:71-100)"""
    return ctl_reconstruction_filter(3, xw, yw, B, Cc)


def lanczos_filter(xw=6.0, yw=6.0, tau=3.0):
    """LanczosSincFilter (SceneTypes/Filter.h:102-131)"""
    return ctl_reconstruction_filter(4, xw, yw, tau, 0.0)


def triangle_filter(xw=2.0, yw=2.0):
    """TriangleFilter (SceneTypes/Filter.h:133-150)"""
    return ctl_reconstruction_filter(5, xw, yw, 0.0, 0.0)


class ctl_nlm_filter(C.Structure):
    _fields_ = [("k", f32), ("sigma2_scale", f32)]


def nlm_filter(k=0.45, sigma2_scale=0.005):
    """NonLocalMeansFilter (Kernel/ImagePipeline/Filter/NonLocalMeansFilter.h:103-113): the reference's defaults.  Needs the per-pixel variance: pass
    tracer= (after tracer.setPixelVariance(True)) or variance= to Image.applyImagePipeline"""
    return ctl_nlm_filter(k, sigma2_scale)


def tonemap(key=0.18, burn=0.0):
    """ToneMapPostProcess (Kernel/ImagePipeline/PostProcess/ToneMapPostProcess.h:8-24)"""
    return ctl_tonemap(key, burn)


def set_cache_dir(directory):
    """Directory of the compiled-geometry cache (the reference's .xmsh role); None disables.  Default: $CTL_CACHE_DIR."""
    _check(lib.ctl_set_cache_dir(None if directory is None else str(directory).encode()))


FLAT_Q4, FLAT_Q8 = 0, 3                                    # CTL_FLAT_* node formats of the flattened BVH
FLAT_F4, FLAT_F2 = 1, 2                                    # retired numbers, kept as names only: the library answers them with CTL_ERR_UNSUPPORTED and FLAT_FORMATS does not offer them
FLAT_FORMATS = {"q4": FLAT_Q4, "q8": FLAT_Q8}
DEFAULT_FLAT_FORMAT = "q4"                                 # what Scene(desc, flatten=True) builds when no format is named (csrc/flatten.cpp default_flat_format)


def flatten_probe(desc, format=FLAT_Q4):
    """Host half of Scene(desc, flatten=True): dict(nodes, leaves, depth, hash) of the flattened BVH (built or loaded from the cache)."""
    out = (u64 * 4)()
    _check(lib.ctl_flatten_probe(C.byref(desc), u32(format), out))
    return dict(nodes=out[0], leaves=out[1], depth=out[2], hash=out[3])


class FlatBvhDesc(C.Structure):
    _fields_ = [("format", u32), ("max_depth", u32), ("nodes", C.c_void_p), ("n_nodes", u64), ("node_bytes", u32),
                ("leaves", C.c_void_p), ("n_leaves", u64), ("child_links", C.c_void_p), ("compact", u32), ("root_slab", u32), ("n_slab_nodes", u64),
                ("part_index", C.c_void_p), ("part_boxes", C.c_void_p), ("n_part_boxes", u64)]


class FlatBvh:
    """The flattened BVH as host arrays (ctl_flat_bvh_build): what Scene(desc, flatten=True) uploads.  .desc is a ctl_flat_bvh_desc."""

    def __init__(self, desc, format=FLAT_Q4):
        self._h = C.c_void_p()
        self._keepalive = desc
        _check(lib.ctl_flat_bvh_build(C.byref(desc), u32(format), C.byref(self._h)))
        self.desc = FlatBvhDesc()
        _check(lib.ctl_flat_bvh_arrays(self._h, C.byref(self.desc)))

    @classmethod
    def _from_handle(cls, handle, keepalive=None):
        self = cls.__new__(cls)
        self._h, self._keepalive = handle, keepalive
        self.desc = FlatBvhDesc()
        _check(lib.ctl_flat_bvh_arrays(self._h, C.byref(self.desc)))
        return self

    def refit(self, desc):
        """ctl_flat_bvh_refit: the tree refitted in place to the node transforms of `desc` (the description it was built from, moved) with the arithmetic
        of Scene.update (csrc/flat_refit.h), on the host.  Q4 only.  Returns self."""
        _check(lib.ctl_flat_bvh_refit(self._h, C.byref(desc)))
        _check(lib.ctl_flat_bvh_arrays(self._h, C.byref(self.desc)))
        return self

    def rebuild(self, desc, builder="lbvh"):
        """ctl_flat_bvh_rebuild[_ex]: the tree refitted to `desc` and then REBUILT over the same leaf entries (csrc/flat_rebuild.h: Morton codes, sort, Karras's hierarchy
        collapsed 4-wide, breadth-first layout) on the host — the yardstick of Scene.update(desc) + Scene.rebuild_flat().  builder: "lbvh" or "ploc" (csrc/flat_ploc.h:
        the binary tree by locally-ordered clustering instead).  Q4 trees with implied links only.  Returns self."""
        b = rebuild_builder(builder)
        _check(lib.ctl_flat_bvh_rebuild(self._h, C.byref(desc)) if b == REBUILD_LBVH else lib.ctl_flat_bvh_rebuild_ex(self._h, C.byref(desc), b))
        _check(lib.ctl_flat_bvh_arrays(self._h, C.byref(self.desc)))
        return self

    def rebuild_order(self, desc):
        """ctl_flat_bvh_rebuild_order: what the rebuild's stages 1 - 4 hand to its builder for this tree (refitted to `desc`), nothing written:
        (sorted_entry (n,) uint32, entry_boxes (n, 6) float32 by entry index, bounds (6,) float32)"""
        n = len(self.leaves())
        order, boxes, bounds = np.zeros(n, np.uint32), np.zeros((n, 6), np.float32), np.zeros(6, np.float32)
        _check(lib.ctl_flat_bvh_rebuild_order(self._h, C.byref(desc), order.ctypes.data, boxes.ctypes.data, bounds.ctypes.data))
        return order, boxes, bounds

    def update_nodes(self, desc, old_of_new, builder="lbvh"):
        """ctl_flat_bvh_update_nodes[_ex] (builder: "lbvh" or "ploc", as FlatBvh.rebuild takes it): the tree after a change of the node set (old_of_new as Scene.update_nodes takes it), on the host with the device's single-source
        functions (csrc/flat_nodes.h) — the yardstick of Scene.update_nodes.  A refusal leaves the handle as it was.  Returns self."""
        M = np.ascontiguousarray(old_of_new, dtype=np.uint32)
        b = rebuild_builder(builder)
        _check(lib.ctl_flat_bvh_update_nodes(self._h, C.byref(desc), M.ctypes.data, u32(len(M))) if b == REBUILD_LBVH else
               lib.ctl_flat_bvh_update_nodes_ex(self._h, C.byref(desc), M.ctypes.data, u32(len(M)), b))
        self._keepalive = desc
        _check(lib.ctl_flat_bvh_arrays(self._h, C.byref(self.desc)))
        return self

    def update_meshes(self, desc, old_of_new, builder="lbvh"):
        """ctl_flat_bvh_update_meshes[_ex]: as update_nodes, for a description that also APPENDS meshes (csrc/flat_meshes.h) — the yardstick of Scene.update_meshes.
        A refusal leaves the handle as it was.  Returns self."""
        M = np.ascontiguousarray(old_of_new, dtype=np.uint32)
        b = rebuild_builder(builder)
        _check(lib.ctl_flat_bvh_update_meshes(self._h, C.byref(desc), M.ctypes.data, u32(len(M))) if b == REBUILD_LBVH else
               lib.ctl_flat_bvh_update_meshes_ex(self._h, C.byref(desc), M.ctypes.data, u32(len(M)), b))
        self._keepalive = desc
        _check(lib.ctl_flat_bvh_arrays(self._h, C.byref(self.desc)))
        return self

    def update_mesh_set(self, desc, mesh_map=None, node_map=None, builder="lbvh"):
        """ctl_flat_bvh_update_mesh_set: as update_meshes, for a description that also REMOVES meshes (csrc/flat_mesh_set.h) — the yardstick of Scene.update_mesh_set.
        mesh_map / node_map None: from the mesh / node ids of `desc` and of the description the handle was last given.  A refusal leaves the handle as it was.  Returns self."""
        held = getattr(self, "_keepalive", None)
        mesh_map, node_map = _maps_from_ids("update_mesh_set", desc, getattr(held, "mesh_ids", None), getattr(held, "node_ids", None), mesh_map, node_map)
        MM = np.ascontiguousarray(mesh_map, dtype=np.uint32); M = np.ascontiguousarray(node_map, dtype=np.uint32)
        _check(lib.ctl_flat_bvh_update_mesh_set(self._h, C.byref(desc), MM.ctypes.data, u32(len(MM)), M.ctypes.data, u32(len(M)), rebuild_builder(builder)))
        self._keepalive = desc
        _check(lib.ctl_flat_bvh_arrays(self._h, C.byref(self.desc)))
        return self

    def levels(self):
        """ctl_flat_bvh_levels: (level_start (n_levels + 1,), level_nodes (n_nodes,)) uint32 copies — the nodes by depth as a refit walks them"""
        ls, ln = C.POINTER(u32)(), C.POINTER(u32)(); nl, nn = u32(), u64()
        _check(lib.ctl_flat_bvh_levels(self._h, C.byref(ls), C.byref(nl), C.byref(ln), C.byref(nn)))
        if nn.value == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        return np.ctypeslib.as_array(ls, shape=(nl.value + 1,)).copy(), np.ctypeslib.as_array(ln, shape=(nn.value,)).copy()

    def nodes(self):
        n = self.desc.n_nodes * self.desc.node_bytes // 4
        return np.ctypeslib.as_array(C.cast(self.desc.nodes, C.POINTER(C.c_uint32)), shape=(n,)).reshape(self.desc.n_nodes, -1)

    def child_links(self):
        """the explicit links: Q4 (n_nodes, 4) int32, Q8 (n_nodes, 8) in slot order"""
        w = 8 if self.desc.format == FLAT_Q8 else 4
        return np.ctypeslib.as_array(C.cast(self.desc.child_links, C.POINTER(C.c_int32)), shape=(self.desc.n_nodes * w,)).reshape(-1, w)

    def parts(self):
        """the refit side data of a built Q4 tree: (part_index (n_leaves,) uint32 — 0xffffffff or the entry's clip box, part_boxes (n, 6) float32 {lo, hi} at creation)"""
        if not self.desc.part_index:
            return None, None
        idx = np.ctypeslib.as_array(C.cast(self.desc.part_index, C.POINTER(C.c_uint32)), shape=(self.desc.n_leaves,))
        n = self.desc.n_part_boxes
        boxes = np.ctypeslib.as_array(C.cast(self.desc.part_boxes, C.POINTER(C.c_float)), shape=(n * 6,)).reshape(-1, 6) if n else np.zeros((0, 6), np.float32)
        return idx, boxes

    def leaves(self):
        return np.ctypeslib.as_array(C.cast(self.desc.leaves, C.POINTER(C.c_uint32)), shape=(self.desc.n_leaves * 32,)).reshape(-1, 32)

    @staticmethod
    def implied_links(N):
        """Q4 nodes (n, 16) uint32 -> (n, 4) int32: the links a traversal step derives from the first 48 B (csrc/flatten.h: link = base + nibble);
        an inner link carries the child's slab flag in bit 0.  Slots without a child decode to anything."""
        w0, w1, leafm = N[:, 10].astype(np.uint32), N[:, 11].astype(np.uint32), N[:, 3] >> 28
        ib4, nlb15 = w0 & np.uint32(0x03fffffc), (w1 >> 6) | np.uint32(0xfc000000)
        t = [None, (w0 >> 26) & 15, (w1 >> 2) & 15, (w0 >> 30) | ((w1 & 3) << 2)]
        out = np.empty((len(N), 4), np.uint32)
        out[:, 0] = np.where((leafm & 1) == 1, nlb15 + np.uint32(15), w0 & np.uint32(0x03ffffff))
        for k in (1, 2, 3):
            out[:, k] = np.where(((leafm >> k) & 1) == 1, nlb15, ib4) + t[k].astype(np.uint32)
        return out.view(np.int32)

    @staticmethod
    def clear_slab_flags(N):
        """in place: no inner link hands a slab flag down any more"""
        inner = ((N[:, 3] >> 24) & 15) & ~(N[:, 3] >> 28)      # existing children without a leaf bit; bit 0 of a slot's nibble is the flag only for an inner child (a leaf child's nibble is 15 - entries before it)
        for k, (word, bit) in enumerate(((10, 0), (10, 26), (11, 2), (10, 30))):
            N[:, word] &= ~(((inner >> k) & 1).astype(np.uint32) << np.uint32(bit))
        return N

    def __del__(self):
        if getattr(self, "_h", None):
            lib.ctl_flat_bvh_destroy(self._h)
            self._h = None


def _fp(a):
    return a.ctypes.data_as(C.POINTER(f32))


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        a = a.reshape(shape)
    return a


# ---------------------------------------------------------------- material helpers (Mitsuba plugin defaults, ObjectParser.h:754-966)
E = dict(Null=0x1, DiffuseReflection=0x2, DiffuseTransmission=0x4, GlossyReflection=0x8, GlossyTransmission=0x10, DeltaReflection=0x20, DeltaTransmission=0x40)
TEXEL_RGBE, TEXEL_RGBCOL = 0, 1
WRAP_REPEAT, WRAP_CLAMP, WRAP_MIRROR, WRAP_BLACK = 0, 1, 2, 3
FILTER_POINT, FILTER_BILINEAR, FILTER_ANISOTROPIC, FILTER_TRILINEAR = 0, 1, 2, 3
TEX_CONSTANT, BSDF_DIFFUSE, BSDF_DIELECTRIC, BSDF_CONDUCTOR, BSDF_ROUGHCONDUCTOR = 2, 1, 3, 6, 7


def _const_tex(rgb):
    t = ctl_texture()
    t.type = TEX_CONSTANT
    rgb = (rgb, rgb, rgb) if np.isscalar(rgb) else rgb
    t.value[:] = [float(x) for x in rgb]
    t.uv_scale[:] = [1.0, 1.0]
    return t


def image_texture(image, scale=1.0, uv_scale=(1.0, 1.0), uv_offset=(0.0, 0.0)):
    """ImageTexture(mapping, file, scale) (SceneTypes/Texture.h:159-183) over a registered image."""
    t = _const_tex(scale)
    t.type = 4
    t.uv_scale[:] = [float(x) for x in uv_scale]; t.uv_offset[:] = [float(x) for x in uv_offset]
    t.image = image
    return t


def checker_texture(color0, color1, uv_scale=(1.0, 1.0), uv_offset=(0.0, 0.0)):
    """CheckerboardTexture (SceneTypes/Texture.h:127-157)."""
    t = _const_tex(color0)
    t.type = 3
    c1 = (color1, color1, color1) if np.isscalar(color1) else color1
    t.value1[:] = [float(x) for x in c1]
    t.uv_scale[:] = [float(x) for x in uv_scale]; t.uv_offset[:] = [float(x) for x in uv_offset]
    return t


def _as_tex(v):
    return v if isinstance(v, ctl_texture) else _const_tex(v)


def float3_to_rgbe(rgb):
    """SpectrumConverter::Float3ToRGBE (Math/Spectrum.h:534-555) over an (h, w, 3) float array -> (h, w) uint32 texels."""
    c = np.asarray(rgb, np.float32)
    mx = c.max(axis=-1)
    m, e = np.frexp(mx.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        k = (m.astype(np.float32) * np.float32(256.0) / mx).astype(np.float32)
    out = np.zeros(c.shape[:-1], np.uint32)
    ok = mx >= 1e-32
    q = np.zeros(c.shape, np.uint32)
    q[ok] = (c[ok] * k[ok][:, None]).astype(np.uint8)   # (unsigned char)(c * max_)
    out[ok] = q[ok][:, 0] | (q[ok][:, 1] << 8) | (q[ok][:, 2] << 16) | (((e[ok] + 128).astype(np.uint32) & 0xff) << 24)
    return out


def float3_to_rgbcol(rgb):
    """SpectrumConverter::Float3ToCOLORREF (Math/Spectrum.h:521-526)."""
    c = (np.clip(np.asarray(rgb, np.float32), 0.0, 1.0) * np.float32(255.0)).astype(np.uint8).astype(np.uint32)
    return c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16) | np.uint32(255 << 24)


def _material(bsdf_type, combined, two_sided=False):
    m = ctl_material()
    m.bsdf_type, m.combined_type, m.two_sided, m.node_light_index = bsdf_type, combined, 1 if two_sided else 0, 0xFFFFFFFF
    for i in range(4):
        m.tex[i] = _const_tex(0.0)
    return m


def diffuse(reflectance=(0.5, 0.5, 0.5), two_sided=False):
    """diffuse(reflectance) — BSDF_Simple.h:6-24."""
    m = _material(BSDF_DIFFUSE, E["DiffuseReflection"], two_sided)
    m.tex[0] = _as_tex(reflectance)
    return m


def dielectric(int_ior=1.5046, ext_ior=1.000277, specular_transmittance=1.0, specular_reflectance=1.0):
    """dielectric(eta = intIOR / extIOR) — BSDF_Simple.h:62-94, defaults bk7 / air (Utils.h:280-307)."""
    m = _material(BSDF_DIELECTRIC, E["DeltaReflection"] | E["DeltaTransmission"])
    m.tex[0], m.tex[1] = _const_tex(specular_transmittance), _const_tex(specular_reflectance)
    m.f[0] = np.float32(np.float32(int_ior) / np.float32(ext_ior))
    m.f[1] = 0.0
    return m


def conductor(eta=(0.0, 0.0, 0.0), k=(1.0, 1.0, 1.0), specular_reflectance=1.0, two_sided=False):
    """conductor(eta, k) — BSDF_Simple.h:165-193."""
    m = _material(BSDF_CONDUCTOR, E["DeltaReflection"], two_sided)
    m.tex[0] = _const_tex(specular_reflectance)
    m.f[0:3] = [float(x) for x in eta]
    m.f[3:6] = [float(x) for x in k]
    return m


def roughconductor(alpha=0.1, eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), distribution=1, sample_visible=True, specular_reflectance=1.0, alpha_v=None, two_sided=False):
    """roughconductor(type, eta, k, alphaU, alphaV) — BSDF_Simple.h:195-232 (distribution: 0 Beckmann, 1 GGX)."""
    m = _material(BSDF_ROUGHCONDUCTOR, E["GlossyReflection"], two_sided)
    m.tex[0], m.tex[1], m.tex[2] = _const_tex(specular_reflectance), _const_tex(alpha), _const_tex(alpha if alpha_v is None else alpha_v)
    m.f[0:3] = [float(x) for x in eta]
    m.f[3:6] = [float(x) for x in k]
    m.u[0], m.u[1] = distribution, 1 if sample_visible else 0
    return m


def thindielectric(int_ior=1.5046, ext_ior=1.000277, specular_transmittance=1.0, specular_reflectance=1.0):
    """thindielectric(eta) — BSDF_Simple.h:96-125."""
    m = _material(4, E["DeltaReflection"] | E["DeltaTransmission"])   # the reference's constructor (BSDF_Simple.h:102-118); sample() still reports ENull for the transmitted lobe
    m.tex[0], m.tex[1] = _const_tex(specular_transmittance), _const_tex(specular_reflectance)
    m.f[0] = np.float32(np.float32(int_ior) / np.float32(ext_ior))
    return m


def roughdielectric(alpha=0.1, int_ior=1.5046, ext_ior=1.000277, distribution=1, sample_visible=True, specular_transmittance=1.0, specular_reflectance=1.0, alpha_v=None):
    """roughdielectric(type, eta, alphaU, alphaV) — BSDF_Simple.h:127-163 (distribution: 0 Beckmann, 1 GGX)."""
    m = _material(5, E["GlossyReflection"] | E["GlossyTransmission"])
    m.tex[0], m.tex[1] = _const_tex(specular_transmittance), _const_tex(specular_reflectance)
    m.tex[2], m.tex[3] = _const_tex(alpha), _const_tex(alpha if alpha_v is None else alpha_v)
    eta = np.float32(np.float32(int_ior) / np.float32(ext_ior))
    m.f[0], m.f[1] = eta, np.float32(1.0) / eta
    m.u[0], m.u[1] = distribution, 1 if sample_visible else 0
    return m


def fresnel_diffuse_reflectance(eta):
    """FresnelHelper::fresnelDiffuseReflectance(eta, false) (Math/FresnelHelper.cu:57-60): the library's restatement of the reference's adaptive Gauss-Lobatto
    quadrature (csrc/material_factory.h), bit-equal to the reference's value"""
    lib.ctl_fresnel_diffuse_reflectance.restype = C.c_float; lib.ctl_fresnel_diffuse_reflectance.argtypes = [C.c_float]
    return float(lib.ctl_fresnel_diffuse_reflectance(float(np.float32(eta))))


def material_update(m):
    """BSDF::Update(): the derived fields (fdrInt / fdrExt, invEta2, sampling weights) from the primary ones, by the library (ctl_material_update).  A weight that comes
    from the average of an IMAGE texture is final only after DynamicScene.UpdateScene (ctl_builder_finalize), when the bitmap is there — as in the reference, whose
    UpdateMaterialsPhase2 runs Update() after the textures are loaded (Engine/DynamicScene.cpp:74-89)."""
    _check(lib.ctl_material_update(C.byref(m)))
    return m


def plastic(diffuse_reflectance=(0.5, 0.5, 0.5), int_ior=1.49, ext_ior=1.000277, specular_reflectance=1.0, nonlinear=False):
    """plastic(eta, diffuse, specular) — BSDF_Simple.h:234-270 incl. Update(): fdrInt/fdrExt, invEta2, specularSamplingWeight."""
    m = _material(8, E["DeltaReflection"] | E["DiffuseReflection"])
    m.tex[0], m.tex[1] = _as_tex(diffuse_reflectance), _as_tex(specular_reflectance)
    m.f[2] = float(np.float32(np.float32(int_ior) / np.float32(ext_ior)))
    m.u[0] = 1 if nonlinear else 0
    return material_update(m)


def phong(diffuse_reflectance=(0.5, 0.5, 0.5), specular_reflectance=(0.2, 0.2, 0.2), exponent=30.0):
    """phong(diffuse, specular, exponent) — BSDF_Simple.h:313-340; specularSamplingWeight = sAvg / (dAvg + sAvg)."""
    m = _material(10, E["GlossyReflection"] | E["DiffuseReflection"])
    m.tex[0], m.tex[1], m.tex[2] = _as_tex(diffuse_reflectance), _as_tex(specular_reflectance), _as_tex(exponent)
    return material_update(m)


def roughdiffuse(reflectance=(0.5, 0.5, 0.5), alpha=0.2, use_fast_approx=False):
    """roughdiffuse(reflectance, alpha) — BSDF_Simple.h:26-60 (Oren-Nayar)."""
    m = _material(2, E["DiffuseReflection"])
    m.tex[0], m.tex[1] = _as_tex(reflectance), _as_tex(alpha)
    m.u[0] = 1 if use_fast_approx else 0
    return m


def ward(diffuse_reflectance=(0.5, 0.5, 0.5), specular_reflectance=(0.2, 0.2, 0.2), alpha_u=0.1, alpha_v=0.1, variant=2):
    """ward(variant, diffuse, specular, alphaU, alphaV) — BSDF_Simple.h:342-381; variant 0 Ward, 1 Ward-Duer, 2 balanced."""
    m = _material(11, E["GlossyReflection"] | E["DiffuseReflection"])
    m.tex[0], m.tex[1], m.tex[2], m.tex[3] = _as_tex(diffuse_reflectance), _as_tex(specular_reflectance), _as_tex(alpha_u), _as_tex(alpha_v)
    m.u[0] = variant
    return material_update(m)


def roughplastic(diffuse_reflectance=(0.5, 0.5, 0.5), alpha=0.1, int_ior=1.49, ext_ior=1.000277, distribution=0, specular_reflectance=1.0, nonlinear=False, sample_visible=True):
    """roughplastic(type, eta, alpha, diffuse, specular) — BSDF_Simple.h:272-312; needs the rough-transmittance table of slot `distribution`."""
    m = _material(9, E["GlossyReflection"] | E["DiffuseReflection"])
    m.tex[0], m.tex[1], m.tex[2] = _as_tex(diffuse_reflectance), _as_tex(specular_reflectance), _as_tex(alpha)
    m.f[0] = float(np.float32(np.float32(int_ior) / np.float32(ext_ior)))
    m.u[0], m.u[1], m.u[2] = 1 if nonlinear else 0, 0 if distribution == 2 else (1 if sample_visible else 0), distribution   # getSampleVisible(type, true)
    return material_update(m)


def coating(nested_index, nested, int_ior=1.5046, ext_ior=1.000277, thickness=1.0, sigma_a=0.0, specular_reflectance=1.0):
    """coating(nested, eta, thickness, sigmaA, specular) — BSDF_Complex.h:9-75.  `nested_index` = DynamicScene.add_material(nested)."""
    m = _material(13, E["DeltaReflection"] | nested.combined_type)
    m.tex[0], m.tex[1] = _as_tex(sigma_a), _as_tex(specular_reflectance)
    eta = float(np.float32(np.float32(int_ior) / np.float32(ext_ior)))
    m.f[0], m.f[2] = eta, thickness
    m.u[2] = nested_index
    return material_update(m)


def roughcoating(nested_index, nested, alpha=0.1, int_ior=1.5046, ext_ior=1.000277, thickness=1.0, sigma_a=0.0, distribution=0, specular_reflectance=1.0):
    """roughcoating(type, nested, eta, thickness, sigmaA, alpha, specular) — BSDF_Complex.h:77-147; needs the rough-transmittance table."""
    m = _material(14, E["GlossyReflection"] | nested.combined_type)
    m.tex[0], m.tex[1], m.tex[2] = _as_tex(sigma_a), _as_tex(specular_reflectance), _as_tex(alpha)
    eta = float(np.float32(np.float32(int_ior) / np.float32(ext_ior)))
    m.f[0], m.f[2] = eta, thickness
    m.u[0], m.u[1], m.u[2] = distribution, 0 if distribution == 2 else 1, nested_index
    return material_update(m)


MAP_NONE, MAP_NORMAL, MAP_HEIGHT = 0, 1, 2
ALPHA_DISABLED, ALPHA_MAP_LUMINANCE, ALPHA_MAP_ALPHA, ALPHA_MAP_COLOR = 0, 1, 2, 3
ALPHA_REFLECTANCE_LUMINANCE, ALPHA_REFLECTANCE_ALPHA, ALPHA_REFLECTANCE_COLOR = 5, 6, 7


def set_normal_map(material, texture):
    """Material::SetNormalMap (Engine/Material.h:93-99); excludes a height map."""
    if material.map_kind == MAP_HEIGHT:
        raise CtlError(-1, "Cannot set both height and normal map!")
    material.map_kind = MAP_NORMAL; material.map_tex = _as_tex(texture)
    return material


def set_height_map(material, texture):
    """Material::SetHeightMap (Engine/Material.h:100-106); only image textures perturb the frame (Material.cu:109)."""
    if material.map_kind == MAP_NORMAL:
        raise CtlError(-1, "Cannot set both height and normal map!")
    material.map_kind = MAP_HEIGHT; material.map_tex = _as_tex(texture)
    return material


def set_alpha_map(material, texture, state=ALPHA_MAP_LUMINANCE, test_scalar=1.0, test_color=(0.0, 0.0, 0.0)):
    """Material::SetAlphaMap + AlphaBlendData::test_val_* (Engine/Material.h:24-36,107-111)."""
    material.alpha_state = state; material.alpha_tex = _as_tex(texture)
    material.alpha_test_scalar = float(test_scalar); material.alpha_test_color[:] = [float(x) for x in test_color]
    return material


def blend(index0, nested0, index1, nested1, weight=0.5):
    """blend(nested1, nested2, weight) — BSDF_Complex.h:149-181 (blendbsdf / mixturebsdf of the loader)."""
    m = _material(15, nested0.combined_type | nested1.combined_type)
    m.tex[0] = _as_tex(weight)
    m.u[2], m.u[3] = index0, index1
    return m


# ---------------------------------------------------------------- DynamicScene (Engine/DynamicScene.h:70-187, loader-facing subset)
def phase_isotropic():
    p = ctl_phase_function(); p.type = PHASE_ISOTROPIC
    return p


def phase_hg(g):
    """HGPhaseFunction(g), |g| < 1"""
    p = ctl_phase_function(); p.type = PHASE_HG; p.g = float(g)
    return p


def phase_rayleigh():
    p = ctl_phase_function(); p.type = PHASE_RAYLEIGH
    return p


def phase_kajiya_kay(ks=0.4, kd=0.2, exponent=4.0):
    """KajiyaKayPhaseFunction(ks, kd, e); the normalisation is derived by volume_update / CreateVolume"""
    p = ctl_phase_function(); p.type = PHASE_KAJIYA_KAY; p.ks, p.kd, p.exponent = float(ks), float(kd), float(exponent)
    return p


def _rgb3(v):
    a = np.broadcast_to(np.asarray(v, np.float32), (3,))
    return (f32 * 3)(*[float(x) for x in a])


def homogeneous_volume(volume_to_world, sigma_a, sigma_s, phase=None, le=0.0):
    """HomogeneousVolumeDensity(func, ToWorld, sa, ss, e): the unit cube under volume_to_world (4x4, row-major), with its derived fields (volume_update)"""
    v = ctl_volume(); v.type = VOLUME_HOMOGENEOUS
    v.phase = phase if phase is not None else phase_isotropic()
    v.volume_to_world.m[:] = [float(x) for x in np.asarray(volume_to_world, np.float32).reshape(16)]
    v.sig_a, v.sig_s, v.le = _rgb3(sigma_a), _rgb3(sigma_s), _rgb3(le)
    return volume_update(v)


class GridVolume:
    """a VolumeGrid region for a description: .volume (ctl_volume, type VOLUME_GRID, coefficients 0) and .grid (ctl_volume_grid without its volume index, which
    volumes_desc sets); the float arrays the record points at are kept alive by this object"""

    def __init__(self, volume, grid, arrays):
        self.volume, self.grid, self._arrays = volume, grid, arrays


def grid_volume(volume_to_world, density=None, density_a=None, density_s=None, sig_a=(0.0, 1.0), sig_s=(0.0, 1.0), phase=None):
    """VolumeGrid(func, ToWorld, buffer, dim[, dimS, dimL]) with its data: `density` (an array of shape dim = (dim[0], dim[1], dim[2])) is the single-grid form,
    density_a / density_s the three-grid form (gridL is not carried).  An array's shape is the grid's dim (x, y, z) and its flattened floats are the grid's floats in
    the reference's linear order (DenseVolGrid::idx, include/ctl_amd.h).  sig_a / sig_s: (min, max), each a scalar or rgb; a coefficient at a point is
    min + (max - min) * density.  Returns a GridVolume."""
    v = ctl_volume(); v.type = VOLUME_GRID
    v.phase = phase if phase is not None else phase_isotropic()
    v.volume_to_world.m[:] = [float(x) for x in np.asarray(volume_to_world, np.float32).reshape(16)]
    volume_update(v)
    g = ctl_volume_grid(); arrays = []

    def put(a, dim_field, ptr_field):
        a = np.asarray(a, np.float32)
        if a.ndim != 3:
            raise ValueError("grid_volume: a density grid is a 3-D array")
        flat = np.ascontiguousarray(a.reshape(-1)); arrays.append(flat)
        getattr(g, dim_field)[:] = [int(x) for x in a.shape]
        setattr(g, ptr_field, flat.ctypes.data_as(C.POINTER(f32)))
    if density is not None:
        if density_a is not None or density_s is not None:
            raise ValueError("grid_volume: density, or density_a and density_s")
        g.single_grid = 1; put(density, "dim", "data")
    else:
        if density_a is None or density_s is None:
            raise ValueError("grid_volume: density, or density_a and density_s")
        g.single_grid = 0; put(density_a, "dim_a", "data_a"); put(density_s, "dim_s", "data_s")
    g.sig_a_min, g.sig_a_max, g.sig_s_min, g.sig_s_max = _rgb3(sig_a[0]), _rgb3(sig_a[1]), _rgb3(sig_s[0]), _rgb3(sig_s[1])
    return GridVolume(v, g, arrays)


def volume_update(v):
    """ctl_volume_update: world_to_volume and the Kajiya-Kay normalisation from the primary fields (host only); returns v"""
    _check(lib.ctl_volume_update(C.byref(v)))
    return v


def box_to_volume_matrix(box_min, box_max):
    """the volume_to_world that maps the unit cube onto an axis-aligned box: Translate(min) % Scale(max - min), as the Mitsuba loader builds it"""
    lo, hi = np.asarray(box_min, np.float32), np.asarray(box_max, np.float32)
    m = np.zeros((4, 4), np.float32)
    m[0, 0], m[1, 1], m[2, 2] = (hi - lo)
    m[:3, 3] = lo
    m[3, 3] = 1
    return m


VEVAL_QUERY_FLOATS, VEVAL_RESULT_FLOATS = 10, 17
(VEVAL_REGION_INTERSECT, VEVAL_INTERSECT, VEVAL_REGION_TAU, VEVAL_TAU, VEVAL_REGION_SAMPLE_DISTANCE, VEVAL_SAMPLE_DISTANCE, VEVAL_SAMPLE_VOLUME, VEVAL_PHASE_EVAL,
 VEVAL_PHASE_SAMPLE, VEVAL_P, VEVAL_SAMPLE, VEVAL_TRANSMITTANCE, VEVAL_EVAL_TRANSMITTANCE, VEVAL_GRID_VALUE, VEVAL_REGION_SIGMA, VEVAL_GRID_MARCH) = range(16)   # CTL_VEVAL_*


def set_desc_volumes(d, volumes, grids=None):
    """point the description `d` at `volumes` — a list of ctl_volume and / or GridVolume (api.grid_volume), whose grid records follow in the volumes' order — and at
    `grids`, further ctl_volume_grid records with their `volume` index set.  The arrays are kept alive by `d`; returns d"""
    vols, recs, keep = [], [], []
    for i, v in enumerate(volumes):
        if isinstance(v, GridVolume):
            g = ctl_volume_grid(); C.memmove(C.addressof(g), C.addressof(v.grid), C.sizeof(g)); g.volume = i
            vols.append(v.volume); recs.append(g); keep.append(v)
        else:
            vols.append(v)
    recs += list(grids or ())
    arr = (ctl_volume * max(1, len(vols)))(*vols)
    garr = (ctl_volume_grid * max(1, len(recs)))(*recs)
    d.volumes = C.cast(arr, C.POINTER(ctl_volume)) if vols else None; d.n_volumes = len(vols)
    d.volume_grids = C.cast(garr, C.POINTER(ctl_volume_grid)) if recs else None; d.n_volume_grids = len(recs)
    d._keep = (arr, garr, keep, grids)
    return d


def volumes_desc(volumes, grids=None):
    """a description that holds nothing but `volumes` (a list of ctl_volume and / or GridVolume) and their grid records: what volume_eval reads (set_desc_volumes).
    The arrays are kept alive by the returned object"""
    return set_desc_volumes(ctl_scene_desc(), volumes, grids)


def volume_eval(desc, what, queries, on_device=False):
    """ctl_volume_eval: the participating-media functions (csrc/volume.h) one call per query row ((n, 10) float32; a [volume] index as the bits of its float) ->
    (n, 17) float32.  on_device=False runs on the host and needs no GPU (the yardstick); True runs one small kernel.  Layouts: include/ctl_amd.h CTL_VEVAL_*."""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, VEVAL_QUERY_FLOATS)
    out = np.zeros((len(q), VEVAL_RESULT_FLOATS), np.float32)
    _check(lib.ctl_volume_eval(C.addressof(desc), i32(what), q.ctypes.data, u32(len(q)), out.ctypes.data, i32(1 if on_device else 0)))
    return out


def decode_image_file(path):
    """ctl_decode_image_file: (H, W, 3) float32 for HDR / PFM / EXR files, (H, W, 4) uint8 otherwise; rows top-down"""
    w, h, fl = u32(0), u32(0), i32(0)
    _check(lib.ctl_decode_image_file(path.encode(), C.byref(w), C.byref(h), C.byref(fl), None, None))
    if fl.value:
        out = np.zeros((h.value, w.value, 3), np.float32)
        _check(lib.ctl_decode_image_file(path.encode(), C.byref(w), C.byref(h), C.byref(fl), out.ctypes.data_as(C.POINTER(C.c_float)), None))
    else:
        out = np.zeros((h.value, w.value, 4), np.uint8)
        _check(lib.ctl_decode_image_file(path.encode(), C.byref(w), C.byref(h), C.byref(fl), None, out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out


class DynamicScene:
    def __init__(self):
        self._h = C.c_void_p()
        _check(lib.ctl_builder_create(C.byref(self._h)))
        self.desc = None
        self.mesh_inputs = {}   # mesh index -> dict(positions, indices, normals, uvs) as add_mesh / UpdateMesh last took them: what a caller deforms
        self._node_ids = []     # per node, in index order: its id — assigned at CreateNode, never reused, kept by DeleteNode's shift (node_ids, Scene.update_nodes)
        self._next_node_id = 0
        self._mesh_ids = []     # per mesh, in index order: its id — assigned at add_mesh, never reused, kept by RemoveMesh's shift (mesh_ids, Scene.update_mesh_set)
        self._next_mesh_id = 0
        self._image_ids = []    # per image, in index order: its id — assigned at add_image, never reused, kept by remove_image's shift; replace_image gives the index a new one
        self._next_image_id = 0
        self._image_sizes = {}  # image id -> (width, height) as add_image / replace_image took them

    def __del__(self):
        if getattr(self, "_h", None):
            lib.ctl_builder_destroy(self._h)
            self._h = None

    def add_mesh(self, positions, indices=None, normals=None, uvs=None, tri_material=None, materials=None):
        """Mesh::CompileMesh (Engine/Mesh.cpp:199-290) -> mesh index.  After a first UpdateScene() the call appends to the builder's arrays: the next UpdateScene()
        gives the description that Scene.update_meshes applies to a scene made from the earlier one."""
        P = _f32(positions, (-1, 3))
        I = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        n_tri = len(P) // 3 if I is None else len(I)
        N = None if normals is None else _f32(normals, (-1, 3))
        UV = None if uvs is None else _f32(uvs, (-1, 2))
        TM = None if tri_material is None else np.ascontiguousarray(tri_material, dtype=np.uint8)
        mats = materials if materials is not None else [diffuse()]
        arr = (ctl_material * len(mats))(*mats)
        out = u32()
        _check(lib.ctl_builder_add_mesh(self._h, _fp(P), u32(len(P)), None if I is None else I.ctypes.data_as(C.c_void_p), u32(n_tri),
                                        None if N is None else _fp(N), None if UV is None else _fp(UV),
                                        None if TM is None else TM.ctypes.data_as(C.c_void_p), arr, u32(len(mats)), C.byref(out)))
        self.mesh_inputs[out.value] = dict(positions=P, indices=I, normals=N, uvs=UV)
        self._sync_mesh_ids(out.value)
        self._mesh_ids.append(self._next_mesh_id); self._next_mesh_id += 1
        return out.value

    def _sync_mesh_ids(self, n):
        """meshes the builder made without add_mesh (ParseMitsubaScene) get their ids now"""
        while len(self._mesh_ids) < n:
            self._mesh_ids.append(self._next_mesh_id); self._next_mesh_id += 1

    def RemoveMesh(self, mesh):
        """ctl_builder_remove_mesh — what DynamicScene::UpdateScene does to a mesh without users (DynamicScene.cpp:483-507, Mesh::Free): the mesh's ranges leave the geometry
        arrays, the meshes behind it move down by one index (their ids stay: mesh_ids()) and by the erased sizes; its standard materials stay in the builder, unreferenced.
        CtlError(ERR_INVALID), the builder unchanged, for a bad index or a mesh a node still instances (DeleteNode first).  UpdateScene() then gives the new description,
        which Scene.update_mesh_set applies in place."""
        n = u32()
        _check(lib.ctl_builder_mesh_count(self._h, C.byref(n)))
        self._sync_mesh_ids(n.value)       # meshes a loader made get their ids BEFORE the shift, so that the ids a live Scene holds keep naming the same meshes
        _check(lib.ctl_builder_remove_mesh(self._h, u32(mesh)))
        if mesh < len(self._mesh_ids):
            del self._mesh_ids[mesh]
        self.mesh_inputs = {(k if k < mesh else k - 1): v for k, v in self.mesh_inputs.items() if k != mesh}

    def mesh_ids(self):
        """the stable id of every mesh, in index order (also on the description UpdateScene returns, as desc.mesh_ids)"""
        return tuple(self._mesh_ids)

    def UpdateMesh(self, mesh, positions, indices=None, normals=None, uvs=None):
        """ctl_builder_update_mesh — DynamicScene::AnimateMesh (DynamicScene.cpp:450-456) for a caller that supplies the positions: new vertex arrays for `mesh`, same
        triangle count, arguments as add_mesh.  The mesh's triangle data, Woop rows, BVH boxes and box and the area lights on its nodes follow; UpdateScene() then
        gives the deformed description, which Scene.update applies in place (DIFF_GEOMETRY)."""
        P = _f32(positions, (-1, 3))
        I = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        n_tri = len(P) // 3 if I is None else len(I)
        N = None if normals is None else _f32(normals, (-1, 3))
        UV = None if uvs is None else _f32(uvs, (-1, 2))
        _check(lib.ctl_builder_update_mesh(self._h, u32(mesh), _fp(P), u32(len(P)), None if I is None else I.ctypes.data_as(C.c_void_p), u32(n_tri),
                                           None if N is None else _fp(N), None if UV is None else _fp(UV)))
        self.mesh_inputs[mesh] = dict(positions=P, indices=I, normals=N, uvs=UV)

    def CreateNode(self, mesh_index, to_world=None):
        """DynamicScene::CreateNode + SetNodeTransform (DynamicScene.cpp:269-346)."""
        out = u32()
        m = None
        if to_world is not None:
            m = ctl_float4x4()
            m.m[:] = [float(x) for x in np.asarray(to_world, dtype=np.float32).reshape(16)]
        _check(lib.ctl_builder_add_node(self._h, u32(mesh_index), None if m is None else C.byref(m), C.byref(out)))
        self._sync_node_ids(out.value)
        self._node_ids.append(self._next_node_id); self._next_node_id += 1
        return out.value

    def _sync_node_ids(self, n):
        """nodes the builder made without CreateNode (ParseMitsubaScene) get their ids now"""
        while len(self._node_ids) < n:
            self._node_ids.append(self._next_node_id); self._next_node_id += 1

    def DeleteNode(self, node):
        """DynamicScene::DeleteNode (DynamicScene.cpp:380-384) — ctl_builder_remove_node: the nodes behind `node` move down by one index (their ids stay: node_ids());
        the node's material copies stay in the table.  CtlError(ERR_UNSUPPORTED) for a node with area lights, CtlError(ERR_INVALID) for a bad index or the last node;
        UpdateScene() then gives the new description, which Scene.update_nodes applies in place."""
        _check(lib.ctl_builder_remove_node(self._h, u32(node)))
        if node < len(self._node_ids):
            del self._node_ids[node]

    def node_ids(self):
        """the stable id of every node, in index order (also on the description UpdateScene returns, as desc.node_ids)"""
        return tuple(self._node_ids)

    def SetNodeTransform(self, node, to_world):
        """DynamicScene::SetNodeTransform (DynamicScene.cpp:338-346): the node's area lights follow; UpdateScene() then gives the moved description."""
        m = ctl_float4x4()
        m.m[:] = [float(x) for x in np.asarray(to_world, dtype=np.float32).reshape(16)]
        _check(lib.ctl_builder_set_node_transform(self._h, u32(node), C.byref(m)))

    def CreateLight(self, node, local_material, radiance, rad_texture=None, orthogonal=False):
        """DynamicScene::CreateLight(node, materialName, L) (DynamicScene.cpp:689-711); materials are addressed by local index.
        rad_texture / orthogonal: DiffuseLight::m_rad_texture (a checker or image ctl_texture) and m_bOrthogonal (Light.h:100-101)."""
        L = (f32 * 3)(*[float(x) for x in radiance])
        if rad_texture is None and not orthogonal:
            _check(lib.ctl_builder_add_area_light(self._h, u32(node), u32(local_material), L))
        else:
            _check(lib.ctl_builder_add_area_light_ex(self._h, u32(node), u32(local_material), L, C.byref(rad_texture) if rad_texture is not None else None, i32(1 if orthogonal else 0)))

    def CreatePointLight(self, position, intensity):
        _check(lib.ctl_builder_add_point_light(self._h, (f32 * 3)(*map(float, position)), (f32 * 3)(*map(float, intensity))))

    def setCamera(self, pos, target, up, fov_degrees, width, height):
        _check(lib.ctl_builder_set_camera_lookat(self._h, (f32 * 3)(*map(float, pos)), (f32 * 3)(*map(float, target)), (f32 * 3)(*map(float, up)),
                                                 f32(fov_degrees), u32(width), u32(height)))

    def CreateSpotLight(self, position, target, intensity, cutoff_angle=20.0, beam_width=None):
        """SpotLight(p, t, L, cutoffAngle, beamWidth) in degrees; Mitsuba default beamWidth = 3/4 cutoffAngle (ObjectParser.h spot)."""
        bw = cutoff_angle * 0.75 if beam_width is None else beam_width
        _check(lib.ctl_builder_add_spot_light(self._h, (f32 * 3)(*position), (f32 * 3)(*target), (f32 * 3)(*intensity), f32(cutoff_angle), f32(bw)))

    def CreateDistantLight(self, direction, irradiance, scene_radius=1.0):
        _check(lib.ctl_builder_add_distant_light(self._h, (f32 * 3)(*direction), (f32 * 3)(*irradiance), f32(scene_radius)))

    def add_image(self, texels, texel_type=TEXEL_RGBCOL, wrap=WRAP_REPEAT, filter=FILTER_BILINEAR):
        """Register level 0 of a KernelMIPMap: texels (h, w) uint32, byte 0 = r ... byte 3 = e / alpha.  Returns the image index."""
        t = np.ascontiguousarray(texels, dtype=np.uint32)
        idx = u32()
        _check(lib.ctl_builder_add_image(self._h, t.ctypes.data_as(C.c_void_p), u32(t.shape[1]), u32(t.shape[0]), u32(texel_type), u32(wrap), u32(filter), C.byref(idx)))
        self._sync_image_ids(idx.value)
        self._image_ids.append(self._next_image_id); self._next_image_id += 1
        self._image_sizes[self._image_ids[-1]] = (t.shape[1], t.shape[0])
        return idx.value

    def _sync_image_ids(self, n):
        """images the builder made without add_image (ParseMitsubaScene) get their ids now"""
        while len(self._image_ids) < n:
            self._image_ids.append(self._next_image_id); self._next_image_id += 1

    def _image_count(self):
        n = u32()
        _check(lib.ctl_builder_image_count(self._h, C.byref(n)))
        return n.value

    def image_ids(self):
        """the stable id of every image, in index order (also on the description UpdateScene returns, as desc.image_ids): what Scene.update_image_set computes its map
        from.  An image replaced by another size carries a new id: to the scene it is a fresh image"""
        return tuple(self._image_ids)

    def remove_image(self, image):
        """ctl_builder_remove_image: an image that no material row and no light references leaves the builder; the images behind it move down by one index (their ids stay:
        image_ids()) and every texture that names one of them follows.  CtlError(ERR_INVALID), the builder unchanged, for a bad index or an image still referenced — the
        message names the first referrer; rows orphaned by DeleteNode / RemoveMesh count (set_material repoints them).  UpdateScene() then gives the new description, which
        Scene.update_image_set applies in place."""
        self._sync_image_ids(self._image_count())      # images a loader made get their ids BEFORE the shift
        _check(lib.ctl_builder_remove_image(self._h, u32(image)))
        if image < len(self._image_ids):
            del self._image_ids[image]

    def replace_image(self, image, texels):
        """ctl_builder_replace_image: new level-0 texels (h, w) uint32 of ANOTHER size at the same index; texel type, wrap and filter stay.  With the image's own size it is
        update_image (and the id stays).  CtlError(ERR_INVALID) for a bad index and for the environment map's image: the builder is untouched."""
        t = np.ascontiguousarray(texels, dtype=np.uint32)
        if t.ndim != 2:
            raise ValueError("replace_image: texels (h, w) uint32")
        self._sync_image_ids(self._image_count())
        _check(lib.ctl_builder_replace_image(self._h, u32(image), t.ctypes.data_as(C.c_void_p), u32(t.shape[1]), u32(t.shape[0])))
        if self._image_sizes.get(self._image_ids[image]) != (t.shape[1], t.shape[0]):      # (a size this object never saw — a loader's image — counts as another)
            self._image_ids[image] = self._next_image_id; self._next_image_id += 1
        self._image_sizes[self._image_ids[image]] = (t.shape[1], t.shape[0])

    def get_material(self, index):
        """ctl_builder_get_material: a copy of row `index` of the material table — absolute, as desc.nodes[k].material_offset + local index or what add_material returned"""
        m = ctl_material()
        _check(lib.ctl_builder_get_material(self._h, u32(index), C.byref(m)))
        return m

    def set_material(self, index, material):
        """ctl_builder_set_material — DynamicScene::getMaterials + Invalidate: replaces row `index` of the material table (absolute index) after the checks a new record
        gets; a nested-material index that breaks the BSDFFirst rule is refused.  UpdateScene() then makes the derived sampling weights; Scene.update applies the result."""
        _check(lib.ctl_builder_set_material(self._h, u32(index), C.byref(material)))

    def update_image(self, image, texels):
        """ctl_builder_update_image — DynamicScene::ReloadTextures for a caller that supplies the bitmap: new level-0 texels (h, w) uint32 for a registered image, same size.
        The environment light's CDFs and normalization follow if the image is its map; UpdateScene() then makes the sampling weights of the materials that read the
        image's average.  The host yardstick of Scene.update_image, and what a host that keeps its builder calls beside it.  CtlError(ERR_INVALID) for a bad index or another
        size: the builder is untouched."""
        t = np.ascontiguousarray(texels, dtype=np.uint32)
        if t.ndim != 2:
            raise ValueError("update_image: texels (h, w) uint32")
        _check(lib.ctl_builder_update_image(self._h, u32(image), t.ctypes.data_as(C.c_void_p), u32(t.shape[1]), u32(t.shape[0])))

    def set_bvh_mode(self, mode):
        """mesh BVH builder for the following add_mesh calls: "auto" (default), "sbvh" (the reference's SplitBVHBuilder restated) or "binned"."""
        _check(lib.ctl_builder_set_bvh_mode(self._h, u32({"auto": 0, "sbvh": 1, "binned": 2}[mode])))

    def add_material(self, material):
        """register the nested BSDF of a coating / roughcoating / blend; returns its absolute material index"""
        idx = u32()
        _check(lib.ctl_builder_add_material(self._h, C.byref(material), C.byref(idx)))
        return idx.value

    def setRoughTransmittance(self, slot, trans, diff_trans, eta_range, alpha_range):
        """RoughTransmittanceManager slot (0 beckmann.dat, 1 phong.dat, 2 ggx.dat — indexed by the distribution TYPE at run time,
        RoughTransmittance.cu:124-157).  trans: (2*eta, alpha, theta) float32, diff_trans: (2*eta, alpha)."""
        t = np.ascontiguousarray(trans, np.float32); dt = np.ascontiguousarray(diff_trans, np.float32)
        r = ctl_rough_transmittance()
        r.trans, r.diff_trans = t.ctypes.data, dt.ctypes.data
        r.eta_samples, r.alpha_samples, r.theta_samples = t.shape[0] // 2, t.shape[1], t.shape[2]
        r.eta_min, r.eta_max, r.alpha_min, r.alpha_max = eta_range[0], eta_range[1], alpha_range[0], alpha_range[1]
        _check(lib.ctl_builder_set_rough_transmittance(self._h, u32(slot), C.byref(r)))

    def loadRoughTransmittance(self, slot, path):
        _check(lib.ctl_builder_load_rough_transmittance(self._h, u32(slot), path.encode()))

    def setEnvironementMap(self, image, scale=(1.0, 1.0, 1.0), to_world=None):
        """DynamicScene::setEnvironementMap (DynamicScene.cpp:846-859) for an already decoded lat-long image."""
        m = None
        if to_world is not None:
            m = ctl_float4x4(); m.m[:] = [float(x) for x in np.asarray(to_world, np.float32).reshape(16)]
        _check(lib.ctl_builder_set_environment_map(self._h, u32(image), (f32 * 3)(*scale), C.byref(m) if m is not None else None))

    def CreateVolume(self, volume, *dims, volume_to_world=None, phase=None):
        """DynamicScene::CreateVolume(VolumeRegion) (DynamicScene.cpp:787-792): a ctl_volume (homogeneous_volume(...)), at most MAX_VOL_COUNT; returns its index.
        UpdateScene() then hands the media out in desc.volumes; only the PathTracer plugin renders them.
        CreateVolume(w, h, d, volume_to_world=, phase=) and the nine-int form are DynamicScene::CreateVolume's grid overloads (:794-812, CreateVolumeGrid below);
        CreateVolume(GridVolume) creates a grid with its data (CreateGridVolume)."""
        if dims:
            return self.CreateVolumeGrid(volume, *dims, volume_to_world=volume_to_world, phase=phase)
        if isinstance(volume, GridVolume):
            return self.CreateGridVolume(volume)
        idx = u32()
        _check(lib.ctl_builder_create_volume(self._h, C.byref(volume), C.byref(idx)))
        return idx.value

    def CreateVolumeGrid(self, *dims, volume_to_world=None, phase=None):
        """DynamicScene::CreateVolume(w, h, d, toWorld, phase) / (wA, hA, dA, wS, hS, dS, wL, hL, dL, toWorld, phase) (DynamicScene.cpp:794-812): a VolumeGrid whose
        grids and coefficients are 0 until SetVolumeGridData / SetVolumeGridCoefficients; the L dims are accepted and ignored.  Returns the volume's index."""
        if len(dims) not in (3, 9):
            raise ValueError("CreateVolumeGrid: 3 or 9 dims")
        m = ctl_float4x4(); m.m[:] = [float(x) for x in np.asarray(np.eye(4) if volume_to_world is None else volume_to_world, np.float32).reshape(16)]
        p = phase if phase is not None else phase_isotropic()
        idx = u32(0)
        _check(lib.ctl_builder_create_volume_grid(self._h, (u32 * len(dims))(*[int(x) for x in dims]), u32(len(dims)), C.byref(m), C.byref(p), C.byref(idx)))
        return idx.value

    def SetVolumeGridData(self, index, data, which=0):
        """copy `data` (dim[0] * dim[1] * dim[2] floats, the reference's linear order) into grid `which` of VolumeGrid `index`: 0 = grid / gridA, 1 = gridS"""
        a = np.ascontiguousarray(np.asarray(data, np.float32).reshape(-1))
        _check(lib.ctl_builder_set_volume_grid_data(self._h, u32(index), u32(which), a.ctypes.data, u32(len(a))))

    def SetVolumeGridCoefficients(self, index, sig_a=(0.0, 1.0), sig_s=(0.0, 1.0)):
        """sigAMin / sigAMax and sigSMin / sigSMax of VolumeGrid `index`: (min, max), each a scalar or rgb"""
        a0, a1, s0, s1 = _rgb3(sig_a[0]), _rgb3(sig_a[1]), _rgb3(sig_s[0]), _rgb3(sig_s[1])
        _check(lib.ctl_builder_set_volume_grid_coefficients(self._h, u32(index), a0, a1, s0, s1))

    def CreateGridVolume(self, gv):
        """a GridVolume (api.grid_volume) through CreateVolumeGrid and the two setters; returns the volume's index"""
        g = gv.grid
        dims = list(g.dim) if g.single_grid else list(g.dim_a) + list(g.dim_s) + [1, 1, 1]
        i = self.CreateVolumeGrid(*dims, volume_to_world=np.array(list(gv.volume.volume_to_world.m), np.float32).reshape(4, 4), phase=gv.volume.phase)
        for which, a in enumerate(gv._arrays):
            self.SetVolumeGridData(i, a, which)
        self.SetVolumeGridCoefficients(i, (np.array(list(g.sig_a_min)), np.array(list(g.sig_a_max))), (np.array(list(g.sig_s_min)), np.array(list(g.sig_s_max))))
        return i

    def SetVolume(self, index, volume):
        """replace volume `index` (the host edits the region CreateVolume returned); Scene.update applies the next description in place (DIFF_VOLUMES)"""
        _check(lib.ctl_builder_set_volume(self._h, u32(index), C.byref(volume)))

    def setSensor(self, sensor):
        """the camera as a ctl_sensor struct (ctl_builder_set_camera), e.g. another scene's desc.camera"""
        _check(lib.ctl_builder_set_camera(self._h, C.byref(sensor)))

    def ParseMitsubaScene(self, path, width=-1, height=-1, exterior_media=False, interior_media=False):
        """ParseMitsubaScene (Engine/SceneLoader/Mitsuba/MitsubaLoader.h:13).  exterior_media / interior_media: its create_exterior_bssrdf / create_interior_bssrdf
        (ctl_parse_mitsuba_scene_ex): a shape without a BSDF whose exterior / interior is a homogeneous medium becomes a volume and is removed."""
        w, h = i32(width), i32(height)
        flags = (PARSE_EXTERIOR_MEDIA if exterior_media else 0) | (PARSE_INTERIOR_MEDIA if interior_media else 0)
        if flags:
            _check(lib.ctl_parse_mitsuba_scene_ex(self._h, path.encode(), C.byref(w), C.byref(h), u32(flags)))
        else:
            _check(lib.ctl_parse_mitsuba_scene(self._h, path.encode(), C.byref(w), C.byref(h)))
        return w.value, h.value

    def UpdateScene(self):
        """DynamicScene::UpdateScene + getKernelSceneData(false) (DynamicScene.cpp:480-589): host-side KernelDynamicScene."""
        self.desc = ctl_scene_desc()
        _check(lib.ctl_builder_finalize(self._h, C.byref(self.desc)))
        self._sync_node_ids(self.desc.n_nodes)
        self.desc.node_ids = self.node_ids()   # (a Python attribute next to the C fields) what Scene.update_nodes computes its map from
        self._sync_mesh_ids(self.desc.n_meshes)
        self.desc.mesh_ids = self.mesh_ids()   # likewise, for Scene.update_mesh_set
        self._sync_image_ids(self.desc.n_images)
        self.desc.image_ids = self.image_ids() # likewise, for Scene.update_image_set
        return self.desc

    def getKernelSceneData(self):
        return self.desc if self.desc is not None else self.UpdateScene()


class Scene:
    """The scene resident in HBM (UpdateKernel, Kernel/TraceHelper.cu:182-217)."""

    def __init__(self, desc, flatten=False, flat_format=None, reduced_rough_transmittance=False):
        """flat_format: None = the library default (Q4, or $CTL_FLAT_FORMAT), else FLAT_Q4 / FLAT_Q8 or one of the strings q4 / q8.
        reduced_rough_transmittance: CTL_SCENE_REDUCED_ROUGH_TRANSMITTANCE (faster rough plastic, equal to the reference's lookup up to rounding only)"""
        self._h = C.c_void_p()
        self._keepalive = desc
        flags = (1 if flatten else 0) | (2 if reduced_rough_transmittance else 0)
        if flat_format is not None:
            flags |= (FLAT_FORMATS.get(flat_format, flat_format) + 1) << 8
        _check(lib.ctl_scene_create_ex(C.byref(desc), u32(flags), C.byref(self._h)))
        # (triangles, Woop rows) per mesh, taken while the description is certainly alive: the sizes read_mesh_geometry's buffers must have (an update keeps them)
        self._mesh_counts = mesh_counts(desc)
        self._skins = {}   # mesh -> dict(n_vert, n_bones) of the bound meshes
        self._light_counts = (int(desc.n_lights_buf), int(desc.n_anim_bytes))   # the sizes read_lights' buffers must have
        self._node_ids = getattr(desc, "node_ids", None)   # of the description the scene holds (DynamicScene.UpdateScene), or None
        self._mesh_ids = getattr(desc, "mesh_ids", None)   # likewise
        self._image_ids = getattr(desc, "image_ids", None) # likewise
        self._image_dims = [(int(desc.images[i].width), int(desc.images[i].height)) for i in range(desc.n_images)]   # an update keeps them (read_image)

    def update(self, desc):
        """ctl_scene_update: applies what differs between the description the scene holds and `desc` — camera, materials, lights, node transforms, the vertex
        values of deformed meshes (DynamicScene.UpdateMesh; the flattened Q4 tree is refitted on the device) — in place and returns the DIFF_* mask.  Raises
        CtlError(ERR_INVALID) when the topology differs (the scene is untouched; .last_mask says what was found) and CtlError(ERR_UNSUPPORTED) for a transform or
        geometry change on a Q8 scene.  Start the next pass with new_trace."""
        mask = u32()
        code = lib.ctl_scene_update(self._h, C.byref(desc), C.byref(mask))
        self.last_mask = mask.value
        _check(code)
        self._keepalive = desc
        self._node_ids = getattr(desc, "node_ids", self._node_ids)
        self._light_counts = (int(desc.n_lights_buf), int(desc.n_anim_bytes))
        return mask.value

    def update_nodes(self, sc_or_desc, old_of_new=None, builder="lbvh"):
        """ctl_scene_update_nodes: another SET of nodes in place — after DynamicScene.DeleteNode and / or CreateNode of further instances of meshes the scene already
        holds, and UpdateScene() — with everything else Scene.update applies.  On a flattened Q4 scene the entries of removed nodes are dropped, those of added nodes made
        from the mesh arrays as they stand in HBM, and the tree rebuilt, all on the device (csrc/flat_nodes.hip).  sc_or_desc: the DynamicScene or its description.
        old_of_new: per new node its index in the description the scene holds or 0xffffffff (added); None: computed from the stable node ids of the two descriptions.
        builder: "lbvh" or "ploc", the builder of the rebuild stage (Scene.rebuild_flat).
        Returns the stats dict (entries_before / _after / _dropped / _generated, degenerate_skipped, rebuilt, edit_ms, total_ms, rebuild = the rebuild_flat dict).
        CtlError(ERR_INVALID / ERR_UNSUPPORTED) leaves the scene as it was.  Start the next pass with new_trace."""
        desc = sc_or_desc.getKernelSceneData() if isinstance(sc_or_desc, DynamicScene) else sc_or_desc
        if old_of_new is None:
            new_ids = getattr(desc, "node_ids", None)
            if new_ids is None or self._node_ids is None:
                raise ValueError("update_nodes: no node ids on the descriptions (DynamicScene.UpdateScene sets them): pass old_of_new")
            index = {i: k for k, i in enumerate(self._node_ids)}
            old_of_new = [index.get(i, 0xffffffff) for i in new_ids]
        M = np.ascontiguousarray(old_of_new, dtype=np.uint32)
        st = ctl_scene_nodes_stats()
        b = rebuild_builder(builder)
        _check(lib.ctl_scene_update_nodes(self._h, C.byref(desc), M.ctypes.data, u32(len(M)), C.addressof(st)) if b == REBUILD_LBVH else
               lib.ctl_scene_update_nodes_ex(self._h, C.byref(desc), M.ctypes.data, u32(len(M)), b, C.addressof(st)))
        self._keepalive = desc
        self._node_ids = getattr(desc, "node_ids", None)
        self._light_counts = (int(desc.n_lights_buf), int(desc.n_anim_bytes))
        out = {k: getattr(st, k) for k, _ in st._fields_ if k != "rebuild"}
        out["rebuild"] = {k: getattr(st.rebuild, k) for k, _ in st.rebuild._fields_}
        out["rebuild"]["rounds"] = _last_rounds() if st.rebuilt else 0
        return out

    def triangle_rows(self):
        """ctl_scene_read_triangle_rows (test hook): the triangle -> row table as HBM holds it, uint32 per triangle, or None while the scene has none"""
        n = C.c_size_t(0)
        _check(lib.ctl_scene_read_triangle_rows(self._h, None, 0, C.byref(n)))
        if not n.value:
            return None
        rows = np.zeros(n.value, np.uint32)
        _check(lib.ctl_scene_read_triangle_rows(self._h, rows.ctypes.data, n.value, C.byref(n)))
        return rows

    def update_meshes(self, sc_or_desc, old_of_new=None, builder="lbvh"):
        """ctl_scene_update_meshes: NEW meshes in place — after DynamicScene.add_mesh on a builder whose description the scene holds, any CreateNode / DeleteNode, and
        UpdateScene().  The geometry arrays grow on the device (csrc/flat_meshes.hip: the old contents are copied there, so deformed and posed meshes keep their shape),
        then the stages of update_nodes run; with nothing appended the call is update_nodes.  Arguments as update_nodes takes them.
        Returns the stats dict: meshes_added, triangles_added, rows_added, bvh_nodes_added, append_ms, hash_ms, nodes = the update_nodes dict.
        CtlError(ERR_INVALID / ERR_UNSUPPORTED) leaves the scene as it was.  Start the next pass with new_trace."""
        desc = sc_or_desc.getKernelSceneData() if isinstance(sc_or_desc, DynamicScene) else sc_or_desc
        if old_of_new is None:
            new_ids = getattr(desc, "node_ids", None)
            if new_ids is None or self._node_ids is None:
                raise ValueError("update_meshes: no node ids on the descriptions (DynamicScene.UpdateScene sets them): pass old_of_new")
            index = {i: k for k, i in enumerate(self._node_ids)}
            old_of_new = [index.get(i, 0xffffffff) for i in new_ids]
        M = np.ascontiguousarray(old_of_new, dtype=np.uint32)
        st = ctl_scene_meshes_stats()
        b = rebuild_builder(builder)
        _check(lib.ctl_scene_update_meshes(self._h, C.byref(desc), M.ctypes.data, u32(len(M)), C.addressof(st)) if b == REBUILD_LBVH else
               lib.ctl_scene_update_meshes_ex(self._h, C.byref(desc), M.ctypes.data, u32(len(M)), b, C.addressof(st)))
        self._keepalive = desc
        self._node_ids = getattr(desc, "node_ids", None)
        self._light_counts = (int(desc.n_lights_buf), int(desc.n_anim_bytes))
        self._mesh_counts = mesh_counts(desc)
        self._mesh_ids = getattr(desc, "mesh_ids", None)
        out = {k: getattr(st, k) for k, _ in st._fields_ if k != "nodes"}
        out["nodes"] = {k: getattr(st.nodes, k) for k, _ in st.nodes._fields_ if k != "rebuild"}
        out["nodes"]["rebuild"] = {k: getattr(st.nodes.rebuild, k) for k, _ in st.nodes.rebuild._fields_}
        out["nodes"]["rebuild"]["rounds"] = _last_rounds() if st.nodes.rebuilt else 0
        return out

    def update_mesh_set(self, sc_or_desc, mesh_map=None, node_map=None, builder="lbvh"):
        """ctl_scene_update_mesh_set: meshes REMOVED in place — after DynamicScene.RemoveMesh (and any add_mesh, CreateNode, DeleteNode) on a builder whose description the
        scene holds, and UpdateScene().  The kept meshes' ranges of the geometry arrays are compacted on the device into new, smaller buffers (csrc/flat_mesh_set.hip:
        deformed and posed meshes keep their shape), appended tails follow, then the stages of update_nodes run with the kept entries' triangle words lowered; any removal
        rebuilds the tree.  With nothing removed the call is update_meshes.
        mesh_map: per new mesh its index in the description the scene holds or 0xffffffff (appended); node_map: as update_nodes' old_of_new.  None: computed from the stable
        mesh / node ids of the two descriptions (DynamicScene.UpdateScene sets them).
        Returns the stats dict: meshes_removed, triangles_removed, rows_removed, bvh_nodes_removed, runs, bytes_moved, bytes_freed, compact_ms, hash_ms, meshes = the
        update_meshes dict.  CtlError(ERR_INVALID / ERR_UNSUPPORTED) leaves the scene as it was.  Bound meshes stay bound under their new indices.  Start the next pass
        with new_trace."""
        desc = sc_or_desc.getKernelSceneData() if isinstance(sc_or_desc, DynamicScene) else sc_or_desc
        mesh_map, node_map = _maps_from_ids("update_mesh_set", desc, self._mesh_ids, self._node_ids, mesh_map, node_map)
        MM = np.ascontiguousarray(mesh_map, dtype=np.uint32); M = np.ascontiguousarray(node_map, dtype=np.uint32)
        st = ctl_scene_mesh_set_stats()
        _check(lib.ctl_scene_update_mesh_set(self._h, C.byref(desc), MM.ctypes.data, u32(len(MM)), M.ctypes.data, u32(len(M)), rebuild_builder(builder), C.addressof(st)))
        self._keepalive = desc
        self._node_ids = getattr(desc, "node_ids", None); self._mesh_ids = getattr(desc, "mesh_ids", None)
        self._light_counts = (int(desc.n_lights_buf), int(desc.n_anim_bytes))
        self._mesh_counts = mesh_counts(desc)
        new_of_old = {int(o): m for m, o in enumerate(MM) if o != 0xffffffff}
        self._skins = {new_of_old[m]: v for m, v in self._skins.items() if m in new_of_old}
        out = {k: getattr(st, k) for k, _ in st._fields_ if k not in ("meshes", "reserved")}
        ms = st.meshes
        out["meshes"] = {k: getattr(ms, k) for k, _ in ms._fields_ if k != "nodes"}
        out["meshes"]["nodes"] = {k: getattr(ms.nodes, k) for k, _ in ms.nodes._fields_ if k != "rebuild"}
        out["meshes"]["nodes"]["rebuild"] = {k: getattr(ms.nodes.rebuild, k) for k, _ in ms.nodes.rebuild._fields_}
        out["meshes"]["nodes"]["rebuild"]["rounds"] = _last_rounds() if ms.nodes.rebuilt else 0
        return out

    def update_stats(self):
        """ctl_scene_get_update_stats of the last update: dict(node_area_before, node_area_after, refit_ms, refit_levels, mask, restamped)"""
        st = ctl_scene_update_stats()
        _check(lib.ctl_scene_get_update_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def rebuild_flat(self, builder="lbvh"):
        """ctl_scene_rebuild_flat[_ex]: a new flattened Q4 tree over the leaf entries the scene holds, made on the device in place (csrc/flat_rebuild.hip) — for a tree that
        refits have degraded.  builder: "lbvh" (Karras's radix tree over the Morton codes) or "ploc" (csrc/flat_ploc.h: locally-ordered clustering from the same sorted
        order — a smaller node area for more launches; INTEGRATION.md "Updating a scene" has the measured trade).
        Returns the stats dict (n_nodes, n_entries, max_depth, levels, node_area_before / _after, sort_ms, topology_ms, refit_ms, total_ms, rounds = clustering rounds).
        CtlError(ERR_UNSUPPORTED) for a scene that is not a flattened Q4 scene with refit data and implied links, or when the new tree would be too deep (the scene keeps
        its tree).  Start the next pass with new_trace."""
        st = ctl_scene_rebuild_stats()
        b = rebuild_builder(builder)
        _check(lib.ctl_scene_rebuild_flat(self._h, C.addressof(st)) if b == REBUILD_LBVH else lib.ctl_scene_rebuild_flat_ex(self._h, b, C.addressof(st)))
        out = {k: getattr(st, k) for k, _ in st._fields_}
        out["rounds"] = _last_rounds()
        return out

    def bind_skin(self, mesh, rest_positions, indices, bone_indices, bone_weights, n_bones, rest_normals=None, area_lights=False, flags=None):
        """ctl_scene_bind_skin: binds `mesh` to a rest pose (arrays as DynamicScene.add_mesh takes them; indices None: a soup; rest_normals None: computed once) and to
        its bone bytes, uint8 (n_vert, 8) each.  The mesh is device-owned until unbind_skin.  area_lights=True (ctl_scene_bind_skin_ex with SKIN_AREA_LIGHTS): the mesh's
        nodes may carry area lights; their shape sets are recomputed on the device after every pose and after every update that uploads the light tables or the
        transforms, and are device-owned like the mesh.  flags: the CTL_SKIN_* word itself, through ctl_scene_bind_skin_ex (overrides area_lights)."""
        a = _skin_arrays(rest_positions, rest_normals, indices, bone_indices, bone_weights)
        args = (self._h, u32(mesh), a["P"].ctypes.data, _ptr(a["N"]), u32(len(a["P"])), _ptr(a["I"]), u32(a["n_tri"]), a["BI"].ctypes.data, a["BW"].ctypes.data, u32(n_bones))
        if flags is None and not area_lights:
            _check(lib.ctl_scene_bind_skin(*args))
        else:
            _check(lib.ctl_scene_bind_skin_ex(*(args + (u32(SKIN_AREA_LIGHTS if flags is None else flags),))))
        self._skins[mesh] = dict(n_vert=len(a["P"]), n_bones=n_bones)

    def animate_mesh(self, mesh, bones0, bones1=None, lerp=0.0):
        """ctl_scene_animate_mesh: poses a bound mesh from (n_bones, 4, 4) row-major bone matrices; bones1 None: bones0.  Returns the update-stats dict plus skin_ms, the
        HIP-event time of the three pose kernels, and shape_set_ms, that of the shape-set kernels (0 unless the mesh was bound with area_lights=True).  Start the next
        pass with new_trace."""
        B0 = np.ascontiguousarray(bones0, np.float32).reshape(-1, 16)
        B1 = None if bones1 is None else np.ascontiguousarray(bones1, np.float32).reshape(-1, 16)
        n = self._skins.get(mesh, {}).get("n_bones")
        if n is not None and (len(B0) != n or (B1 is not None and len(B1) != n)):
            raise ValueError("animate_mesh: %d bone matrices for a skin of %d bones" % (len(B0), n))
        st = ctl_scene_update_stats()
        _check(lib.ctl_scene_animate_mesh(self._h, u32(mesh), B0.ctypes.data, _ptr(B1), f32(lerp), C.addressof(st)))
        out = {k: getattr(st, k) for k, _ in st._fields_}
        ms = f32(); _check(lib.ctl_scene_get_skin_ms(self._h, C.byref(ms))); out["skin_ms"] = ms.value
        out["shape_set_ms"] = self.shape_set_ms()
        return out

    def shape_set_ms(self):
        """ctl_scene_get_shape_set_ms: the HIP-event time of the shape-set kernels in the last call that ran them (animate_mesh, update, update_nodes)"""
        if not hasattr(lib, "ctl_scene_get_shape_set_ms"):
            return 0.0
        ms = f32(); _check(lib.ctl_scene_get_shape_set_ms(self._h, C.byref(ms)))
        return ms.value

    def read_lights(self):
        """ctl_scene_read_lights: dict(lights (n_lights_buf, sizeof(ctl_light) / 4) uint32, anim (n_anim_bytes,) uint8) as HBM holds them, for any scene"""
        n_lights, n_anim = self._light_counts
        L = np.zeros((n_lights, C.sizeof(ctl_light) // 4), np.uint32); A = np.zeros(n_anim, np.uint8)
        _check(lib.ctl_scene_read_lights(self._h, L.ctypes.data, u32(n_lights), A.ctypes.data, C.c_size_t(n_anim)))
        return dict(lights=L, anim=A)

    def update_image(self, image, texels, width=None, height=None, device=False):
        """ctl_scene_update_image: new level-0 texels for image `image` of the live scene, same size, and everything derived from texels rebuilt on the device in place — the
        pyramid, the sampling weights of the materials that read the image's average, the environment light's CDFs and normalization (csrc/scene_images.hip).  texels: an
        (h, w) uint32 array; or, with device=True, the address of width x height uint32 texels in device memory (ctl_device_malloc, tensor.data_ptr()) — or a torch tensor,
        whose data_ptr() and shape are taken.  Returns the stats dict (levels, texels_written, materials_patched, env_tables, upload_ms, pyramid_ms, env_ms, hash_ms,
        total_ms).  CtlError(ERR_INVALID) leaves the scene as it was.  Start the next pass with new_trace; a host that keeps its DynamicScene calls its update_image too."""
        st = ctl_scene_image_stats()
        if device or hasattr(texels, "data_ptr"):
            if hasattr(texels, "data_ptr"):
                if width is None:
                    height, width = int(texels.shape[0]), int(texels.shape[1])
                keep, ptr = texels, int(texels.data_ptr())
            else:
                keep, ptr = None, int(texels)
            if width is None or height is None:
                raise ValueError("update_image: a device pointer needs width and height")
            _check(lib.ctl_scene_update_image(self._h, u32(image), C.c_void_p(ptr), u32(width), u32(height), u32(IMAGE_TEXELS_DEVICE), C.addressof(st)))
            del keep
        else:
            t = np.ascontiguousarray(texels, dtype=np.uint32)
            if t.ndim != 2:
                raise ValueError("update_image: texels (h, w) uint32")
            _check(lib.ctl_scene_update_image(self._h, u32(image), t.ctypes.data_as(C.c_void_p), u32(t.shape[1]), u32(t.shape[0]), u32(0), C.addressof(st)))
        return {k: getattr(st, k) for k, _ in st._fields_}

    def read_image(self, image):
        """ctl_scene_read_image: dict(texels (n,) uint32 — level 0 and the pyramid behind it as the pool holds them —, levels, offsets (15,) uint32: offsets[l - 1] = the
        texel offset of level l >= 1), the layout of mip_pyramid_host"""
        levels = u32(); off = (u32 * 15)()
        _check(lib.ctl_scene_read_image(self._h, u32(image), None, C.c_size_t(0), C.byref(levels), off))
        w, h = self._image_dims[image]   # (the call above refused a bad index)
        n = _pyramid_texels(w, h, levels.value, off)
        T = np.zeros(n, np.uint32)
        _check(lib.ctl_scene_read_image(self._h, u32(image), T.ctypes.data, C.c_size_t(n), C.byref(levels), off))
        return dict(texels=T, levels=levels.value, offsets=np.array(off[:], np.uint32))

    def update_image_set(self, sc_or_desc, image_map=None):
        """ctl_scene_update_image_set: another SET of images in place — after DynamicScene.add_image, remove_image and replace_image (and whatever set_material and the light
        calls changed beside them) on a builder whose description the scene holds, and UpdateScene().  The pyramids of the kept images move on the device into a new texel
        pool laid out as a fresh scene's (csrc/scene_image_set.hip: texels written by update_image survive), fresh images are uploaded and their pyramids built there, then
        the stages of update run over the rest of the description.  Another mesh or node set is refused: those go through their own calls.
        image_map: per new image its index in the description the scene holds or 0xffffffff (fresh: added or replaced); None: computed from the stable image ids of the two
        descriptions (DynamicScene.UpdateScene sets them).
        Returns the stats dict: images_kept, images_fresh, images_removed, runs, texels_moved, texels_uploaded, bytes_freed, move_ms, pyramid_ms, hash_ms, total_ms, update =
        the update_stats dict.  CtlError(ERR_INVALID / ERR_UNSUPPORTED) leaves the scene as it was.  Start the next pass with new_trace."""
        desc = sc_or_desc.getKernelSceneData() if isinstance(sc_or_desc, DynamicScene) else sc_or_desc
        if image_map is None:
            new_ids = getattr(desc, "image_ids", None)
            if new_ids is None or self._image_ids is None:
                raise ValueError("update_image_set: no image ids on the descriptions (DynamicScene.UpdateScene sets them): pass image_map")
            index = {i: k for k, i in enumerate(self._image_ids)}
            image_map = [index.get(i, 0xffffffff) for i in new_ids]
        M = np.ascontiguousarray(image_map, dtype=np.uint32)
        st = ctl_scene_image_set_stats()
        _check(lib.ctl_scene_update_image_set(self._h, C.byref(desc), M.ctypes.data if len(M) else None, u32(len(M)), C.addressof(st)))
        self._keepalive = desc
        self._image_ids = getattr(desc, "image_ids", None)
        self._node_ids = getattr(desc, "node_ids", self._node_ids)
        self._light_counts = (int(desc.n_lights_buf), int(desc.n_anim_bytes))
        self._image_dims = [(int(desc.images[i].width), int(desc.images[i].height)) for i in range(desc.n_images)]
        self.last_mask = st.update.mask
        out = {k: getattr(st, k) for k, _ in st._fields_ if k != "update"}
        out["update"] = {k: getattr(st.update, k) for k, _ in st.update._fields_}
        return out

    def read_mesh_geometry(self, mesh, vertices=False):
        """ctl_scene_read_mesh_geometry: dict(tri (n_tri, 8) uint32, woop (n_rows, 12) uint32) as HBM holds them — any mesh of any scene — and, with vertices=True
        (a bound, posed mesh), positions and normals (n_vert, 3) float32 of the last pose"""
        if not 0 <= mesh < len(self._mesh_counts):
            raise CtlError(ERR_INVALID, "read_mesh_geometry: bad mesh index")
        n_tri, n_rows = self._mesh_counts[mesh]
        tri = np.zeros((n_tri, 8), np.uint32); woop = np.zeros((n_rows, 12), np.uint32)
        P = N = None
        if vertices:
            if mesh not in self._skins:
                raise CtlError(ERR_INVALID, "read_mesh_geometry: mesh %d is not bound" % mesh)
            n_vert = self._skins[mesh]["n_vert"]
            P = np.zeros((n_vert, 3), np.float32); N = np.zeros((n_vert, 3), np.float32)
        _check(lib.ctl_scene_read_mesh_geometry(self._h, u32(mesh), _ptr(P), _ptr(N), tri.ctypes.data, woop.ctypes.data))
        return dict(positions=P, normals=N, tri=tri, woop=woop)

    def unbind_skin(self, mesh):
        """ctl_scene_unbind_skin: the next update(desc) sees the mesh as changed (DIFF_GEOMETRY) and restores the description's values"""
        _check(lib.ctl_scene_unbind_skin(self._h, u32(mesh)))
        self._skins.pop(mesh, None)

    def flat_bvh(self):
        """ctl_scene_read_flat_bvh: the device tree copied back as a FlatBvh, without the model / alpha bits stamped into the device copy"""
        h = C.c_void_p()
        _check(lib.ctl_scene_read_flat_bvh(self._h, C.byref(h)))
        return FlatBvh._from_handle(h)

    def __del__(self):
        if getattr(self, "_h", None):
            lib.ctl_scene_destroy(self._h)
            self._h = None


DIFF_CAMERA, DIFF_MATERIALS, DIFF_LIGHTS, DIFF_TRANSFORMS, DIFF_TOPOLOGY, DIFF_GEOMETRY, DIFF_VOLUMES = 1, 2, 4, 8, 16, 32, 64   # CTL_DIFF_*
ERR_INVALID, ERR_NO_DEVICE, ERR_UNSUPPORTED, ERR_INTERNAL = -1, -2, -5, -7


class ctl_scene_update_stats(C.Structure):
    _fields_ = [("node_area_before", C.c_double), ("node_area_after", C.c_double), ("refit_ms", f32), ("refit_levels", u32), ("mask", u32), ("restamped", u32)]


class ctl_scene_image_stats(C.Structure):
    _fields_ = [("levels", u32), ("texels_written", u32), ("materials_patched", u32), ("env_tables", u32),
                ("upload_ms", f32), ("pyramid_ms", f32), ("env_ms", f32), ("hash_ms", f32), ("total_ms", f32)]


class ctl_scene_image_set_stats(C.Structure):
    _fields_ = [("images_kept", u32), ("images_fresh", u32), ("images_removed", u32), ("runs", u32), ("texels_moved", u64), ("texels_uploaded", u64), ("bytes_freed", u64),
                ("move_ms", f32), ("pyramid_ms", f32), ("hash_ms", f32), ("total_ms", f32), ("update", ctl_scene_update_stats)]


class ctl_scene_rebuild_stats(C.Structure):
    _fields_ = [("n_nodes", u32), ("n_entries", u32), ("max_depth", u32), ("levels", u32), ("node_area_before", C.c_double), ("node_area_after", C.c_double),
                ("sort_ms", f32), ("topology_ms", f32), ("refit_ms", f32), ("total_ms", f32)]


class ctl_scene_nodes_stats(C.Structure):
    _fields_ = [("entries_before", u32), ("entries_after", u32), ("entries_dropped", u32), ("entries_generated", u32), ("degenerate_skipped", u32), ("rebuilt", u32),
                ("rebuild", ctl_scene_rebuild_stats), ("edit_ms", f32), ("total_ms", f32)]


class ctl_scene_meshes_stats(C.Structure):
    _fields_ = [("meshes_added", u32), ("triangles_added", u32), ("rows_added", u32), ("bvh_nodes_added", u32), ("append_ms", f32), ("hash_ms", f32), ("nodes", ctl_scene_nodes_stats)]


class ctl_scene_mesh_set_stats(C.Structure):
    _fields_ = [("meshes_removed", u32), ("triangles_removed", u32), ("rows_removed", u32), ("bvh_nodes_removed", u32), ("runs", u32), ("reserved", u32),
                ("bytes_moved", u64), ("bytes_freed", u64), ("compact_ms", f32), ("hash_ms", f32), ("meshes", ctl_scene_meshes_stats)]


def _maps_from_ids(who, desc, held_mesh_ids, held_node_ids, mesh_map, node_map):
    """the mesh and node maps of update_mesh_set where the caller gave none: from the stable ids on the two descriptions"""
    if mesh_map is None:
        new_ids = getattr(desc, "mesh_ids", None)
        if new_ids is None or held_mesh_ids is None:
            raise ValueError(who + ": no mesh ids on the descriptions (DynamicScene.UpdateScene sets them): pass mesh_map")
        index = {i: k for k, i in enumerate(held_mesh_ids)}
        mesh_map = [index.get(i, 0xffffffff) for i in new_ids]
    if node_map is None:
        new_ids = getattr(desc, "node_ids", None)
        if new_ids is None or held_node_ids is None:
            raise ValueError(who + ": no node ids on the descriptions (DynamicScene.UpdateScene sets them): pass node_map")
        index = {i: k for k, i in enumerate(held_node_ids)}
        node_map = [index.get(i, 0xffffffff) for i in new_ids]
    return mesh_map, node_map


# (declared only where the library has them: tools/ab_bench.py loads the parent commit's library through $CTL_AMD_LIB for a same-box A/B of bench.py, which calls none
# of them; calling one on such a library raises AttributeError)
for _n, _a in (("ctl_scene_rebuild_flat", [C.c_void_p, C.c_void_p]), ("ctl_flat_bvh_rebuild", [C.c_void_p, C.c_void_p]), ("ctl_flat_bvh_levels", [C.c_void_p] * 5),
               ("ctl_builder_remove_node", [C.c_void_p, u32]), ("ctl_scene_update_nodes", [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_void_p]),
               ("ctl_flat_bvh_update_nodes", [C.c_void_p, C.c_void_p, C.c_void_p, u32]),
               ("ctl_scene_rebuild_flat_ex", [C.c_void_p, C.c_int, C.c_void_p]), ("ctl_flat_bvh_rebuild_ex", [C.c_void_p, C.c_void_p, C.c_int]),
               ("ctl_scene_update_nodes_ex", [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_int, C.c_void_p]),
               ("ctl_flat_bvh_update_nodes_ex", [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_int]), ("ctl_rebuild_last_rounds", []),
               ("ctl_flat_bvh_rebuild_order", [C.c_void_p] * 5),
               ("ctl_scene_bind_skin_ex", [C.c_void_p, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, C.c_void_p, C.c_void_p, u32, u32]),
               ("ctl_scene_get_shape_set_ms", [C.c_void_p, C.POINTER(f32)]), ("ctl_scene_read_lights", [C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_size_t]),
               ("ctl_shape_sets_host", [C.c_void_p, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
               ("ctl_builder_update_image", [C.c_void_p, u32, C.c_void_p, u32, u32]), ("ctl_mip_pyramid_host", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
               ("ctl_scene_update_image", [C.c_void_p, u32, C.c_void_p, u32, u32, u32, C.c_void_p]),
               ("ctl_scene_read_image", [C.c_void_p, u32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
               ("ctl_scene_update_meshes", [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_void_p]), ("ctl_scene_update_meshes_ex", [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_int, C.c_void_p]),
               ("ctl_flat_bvh_update_meshes", [C.c_void_p, C.c_void_p, C.c_void_p, u32]), ("ctl_flat_bvh_update_meshes_ex", [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_int]),
               ("ctl_builder_remove_mesh", [C.c_void_p, u32]), ("ctl_builder_mesh_count", [C.c_void_p, C.c_void_p]),
               ("ctl_scene_update_mesh_set", [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, C.c_int, C.c_void_p]),
               ("ctl_flat_bvh_update_mesh_set", [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32, C.c_int]),
               ("ctl_compact_tri_rows_host", [C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, C.c_void_p]),
               ("ctl_builder_image_count", [C.c_void_p, C.c_void_p]), ("ctl_builder_remove_image", [C.c_void_p, u32]), ("ctl_builder_replace_image", [C.c_void_p, u32, C.c_void_p, u32, u32]),
               ("ctl_builder_get_material", [C.c_void_p, u32, C.c_void_p]), ("ctl_builder_set_material", [C.c_void_p, u32, C.c_void_p]),
               ("ctl_scene_update_image_set", [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_void_p]),
               ("ctl_image_set_plan_host", [C.c_void_p, C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
               ("ctl_move_texels_host", [C.c_void_p, u64, C.c_void_p, u32, C.c_void_p, u64]),
               ("ctl_triangle_woop_rows", [C.c_void_p, C.c_void_p]), ("ctl_scene_read_triangle_rows", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]), ("ctl_append_leaf_rows_host", [C.c_void_p, u32, u32, u32, u32, C.c_void_p, C.c_void_p])):
    if hasattr(lib, _n):
        getattr(lib, _n).argtypes = _a
if hasattr(lib, "ctl_rebuild_last_rounds"):
    lib.ctl_rebuild_last_rounds.restype = u32

REBUILD_LBVH, REBUILD_PLOC = 0, 1   # CTL_REBUILD_LBVH, CTL_REBUILD_PLOC
SKIN_AREA_LIGHTS = 1                # CTL_SKIN_AREA_LIGHTS
IMAGE_TEXELS_DEVICE = 1             # CTL_IMAGE_TEXELS_DEVICE


def rebuild_builder(builder):
    """the builder constant of the _ex entry points: "lbvh" / "ploc"; an int goes through as it is (the library refuses an unknown one with ERR_INVALID)"""
    if isinstance(builder, str):
        try:
            return {"lbvh": REBUILD_LBVH, "ploc": REBUILD_PLOC}[builder]
        except KeyError:
            raise ValueError("builder: 'lbvh' or 'ploc', not %r" % (builder,))
    return int(builder)


def _last_rounds():
    return int(lib.ctl_rebuild_last_rounds()) if hasattr(lib, "ctl_rebuild_last_rounds") else 0


def _ptr(a):
    return None if a is None else a.ctypes.data


def _skin_arrays(rest_positions, rest_normals, indices, bone_indices, bone_weights):
    P = _f32(rest_positions, (-1, 3))
    N = None if rest_normals is None else _f32(rest_normals, (-1, 3))
    I = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
    BI = np.ascontiguousarray(bone_indices, dtype=np.uint8).reshape(-1, 8); BW = np.ascontiguousarray(bone_weights, dtype=np.uint8).reshape(-1, 8)
    if len(BI) != len(P) or len(BW) != len(P) or (N is not None and len(N) != len(P)):
        raise ValueError("skin arrays: one row per vertex")
    return dict(P=P, N=N, I=I, BI=BI, BW=BW, n_tri=len(P) // 3 if I is None else len(I))


def skin_mesh_host(desc, mesh, rest_positions, indices, bone_indices, bone_weights, n_bones, bones0, bones1=None, lerp=0.0, rest_normals=None, n_rows=None):
    """ctl_skin_mesh_host (host only): the yardstick of Scene.animate_mesh + read_mesh_geometry — dict(positions, normals (n_vert, 3) float32, tri (n_tri, 8) uint32,
    woop (n_rows, 12) uint32); n_rows: the mesh's rows of the Woop stream (default: counted from the description's mesh offsets)"""
    a = _skin_arrays(rest_positions, rest_normals, indices, bone_indices, bone_weights)
    B0 = np.ascontiguousarray(bones0, np.float32).reshape(-1, 16)
    B1 = None if bones1 is None else np.ascontiguousarray(bones1, np.float32).reshape(-1, 16)
    if len(B0) != n_bones or (B1 is not None and len(B1) != n_bones):
        raise ValueError("skin_mesh_host: %d bone matrices for %d bones" % (len(B0), n_bones))
    if n_rows is None:
        n_rows = mesh_counts(desc)[mesh][1] if 0 <= mesh < desc.n_meshes else 0
    P = np.zeros((len(a["P"]), 3), np.float32); N = np.zeros_like(P); tri = np.zeros((a["n_tri"], 8), np.uint32); woop = np.zeros((n_rows, 12), np.uint32)
    _check(lib.ctl_skin_mesh_host(C.addressof(desc), u32(mesh), a["P"].ctypes.data, _ptr(a["N"]), u32(len(a["P"])), _ptr(a["I"]), u32(a["n_tri"]), a["BI"].ctypes.data, a["BW"].ctypes.data,
                                  u32(n_bones), B0.ctypes.data, _ptr(B1), f32(lerp), P.ctypes.data, N.ctypes.data, tri.ctypes.data, woop.ctypes.data))
    return dict(positions=P, normals=N, tri=tri, woop=woop)


def shape_sets_host(desc, mesh, tri, woop):
    """ctl_shape_sets_host (host only): the yardstick of Scene.read_lights after a pose — desc's light table and anim blob with the shape sets of the lights on nodes that
    instance `mesh` recalculated from tri (n_tri, 8) / woop (n_rows, 12) uint32, the mesh's posed ranges as skin_mesh_host returns them.  dict(lights, anim) as read_lights"""
    T = np.ascontiguousarray(tri, np.uint32).reshape(-1, 8); Wp = np.ascontiguousarray(woop, np.uint32).reshape(-1, 12)
    if 0 <= mesh < desc.n_meshes and (len(T), len(Wp)) != tuple(mesh_counts(desc)[mesh]):
        raise ValueError("shape_sets_host: %d triangles and %d rows for a mesh of %s" % (len(T), len(Wp), mesh_counts(desc)[mesh]))
    L = np.zeros((desc.n_lights_buf, C.sizeof(ctl_light) // 4), np.uint32); A = np.zeros(desc.n_anim_bytes, np.uint8)
    _check(lib.ctl_shape_sets_host(C.addressof(desc), u32(mesh), T.ctypes.data, Wp.ctypes.data, L.ctypes.data, A.ctypes.data))
    return dict(lights=L, anim=A)


def _pyramid_texels(width, height, levels, offsets):
    """the texel count of a pyramid from its level table: the last level's offset plus its size"""
    last = levels - 1
    return (int(offsets[last - 1]) if last else 0) + (width >> last) * (height >> last)


def mip_pyramid_host(texels, texel_type=TEXEL_RGBCOL):
    """ctl_mip_pyramid_host (host only): the pyramid a scene keeps of an (h, w) uint32 image — dict(texels (n,) uint32: level 0, then levels 1 .., levels, offsets (15,)
    uint32: offsets[l - 1] = the texel offset of level l >= 1; level l is (w >> l) x (h >> l)).  What Scene.read_image reads back."""
    t = np.ascontiguousarray(texels, dtype=np.uint32)
    if t.ndim != 2:
        raise ValueError("mip_pyramid_host: texels (h, w) uint32")
    m = ctl_mipmap(); m.texels = t.ctypes.data; m.width, m.height, m.texel_type = t.shape[1], t.shape[0], texel_type
    levels = u32(); off = (u32 * 15)()
    _check(lib.ctl_mip_pyramid_host(C.addressof(m), None, C.c_size_t(0), C.byref(levels), off))
    n = _pyramid_texels(m.width, m.height, levels.value, off)
    T = np.zeros(n, np.uint32)
    _check(lib.ctl_mip_pyramid_host(C.addressof(m), T.ctypes.data, C.c_size_t(n), C.byref(levels), off))
    return dict(texels=T, levels=levels.value, offsets=np.array(off[:], np.uint32))


def image_set_plan_host(old_desc, new_desc, image_map):
    """ctl_image_set_plan_host (no GPU): the acceptance check of Scene.update_image_set for a scene made from old_desc, and its plan — dict(offsets (n,) uint64: the texel
    offset of every image's level 0 in the new pool; total: the pool's texels; runs (n_runs + 1, 4) uint64: per run first destination texel, first source texel, length,
    kept texels in front of it, then the sentinel; n_runs).  CtlError(ERR_INVALID) names the rule broken."""
    M = np.ascontiguousarray(image_map, dtype=np.uint32)
    off = np.zeros(len(M), np.uint64); runs = np.zeros((len(M) + 1, 4), np.uint64); total = u64(); n_runs = u32()
    _check(lib.ctl_image_set_plan_host(C.byref(old_desc), C.byref(new_desc), M.ctypes.data if len(M) else None, u32(len(M)), off.ctypes.data if len(M) else None,
                                       C.addressof(total), runs.ctypes.data, C.addressof(n_runs)))
    return dict(offsets=off, total=int(total.value), runs=runs[:n_runs.value + 1].copy(), n_runs=int(n_runs.value))


def move_texels_host(old_pool, runs, new_pool):
    """ctl_move_texels_host (no GPU): k_move_texels' arithmetic on the host — the kept texels of old_pool into new_pool (uint32, written in place) through the run table of
    image_set_plan_host; words no run covers are untouched"""
    O = np.ascontiguousarray(old_pool, np.uint32); R = np.ascontiguousarray(runs, np.uint64).reshape(-1, 4)
    if new_pool.dtype != np.uint32 or not new_pool.flags.c_contiguous:
        raise ValueError("move_texels_host: new_pool must be a contiguous uint32 array")
    _check(lib.ctl_move_texels_host(O.ctypes.data if len(O) else None, u64(len(O)), R.ctypes.data, u32(len(R) - 1), new_pool.ctypes.data if len(new_pool) else None, u64(len(new_pool))))
    return new_pool


def triangle_woop_rows(desc):
    """ctl_triangle_woop_rows: per triangle the first row of the two-level leaf stream that names it (0xffffffff: none)"""
    rows = np.zeros(desc.n_tri_data, np.uint32)
    _check(lib.ctl_triangle_woop_rows(C.byref(desc), rows.ctypes.data))
    return rows


def append_leaf_rows_host(new_desc, old_desc, old_rows):
    """ctl_append_leaf_rows_host: the arithmetic of k_append_leaf_rows (csrc/flat_meshes.h) on the host for what new_desc appends to old_desc; old_rows: the table of
    old_desc.  Returns (the table of new_desc.n_tri_data words, the appended 64-B leaf-stream rows as (rows, 16) uint32)"""
    table = np.zeros(new_desc.n_tri_data, np.uint32); table[:old_desc.n_tri_data] = old_rows
    leaf = np.zeros((new_desc.n_woop - old_desc.n_woop, 16), np.uint32)
    _check(lib.ctl_append_leaf_rows_host(C.byref(new_desc), u32(old_desc.n_meshes), u32(old_desc.n_tri_data), u32(old_desc.n_woop), u32(old_desc.n_bvh_nodes), table.ctypes.data, leaf.ctypes.data))
    return table, leaf


def compact_tri_rows_host(old_desc, mesh_map, old_rows):
    """ctl_compact_tri_rows_host: the arithmetic of k_compact_tri_rows (csrc/flat_mesh_set.h) on the host — the triangle -> row table of the meshes that mesh_map (per new
    mesh its index in old_desc, 0xffffffff = appended) keeps, from old_desc's table"""
    MM = np.ascontiguousarray(mesh_map, dtype=np.uint32); R = np.ascontiguousarray(old_rows, dtype=np.uint32)
    out = np.zeros(max(1, old_desc.n_tri_data), np.uint32); n = u32()
    _check(lib.ctl_compact_tri_rows_host(C.byref(old_desc), MM.ctypes.data, u32(len(MM)), R.ctypes.data, out.ctypes.data, C.byref(n)))
    return out[:n.value].copy()


def mesh_counts(desc):
    """[(triangles, rows of the Woop stream)] per mesh of a description: a mesh's range ends where the next one (by offset) starts, the last one's at the array's end
    (csrc/geometry_hash.h mesh_ranges).  One sort per array."""
    if not desc.n_meshes:
        return []
    M = desc.view("meshes", np.uint32, desc.n_meshes, 5).astype(np.int64)

    def lengths(start, total):
        start = np.minimum(start, total); order = np.argsort(start, kind="stable")
        end = np.empty_like(start); end[order] = np.append(start[order][1:], total)
        return end - start
    return list(zip(lengths(M[:, 0], desc.n_tri_data).tolist(), lengths(M[:, 2] // 3, desc.n_woop).tolist()))


def scene_desc_diff(a, b):
    """ctl_scene_desc_diff: the DIFF_* bits of what differs between two descriptions (host only)"""
    mask = u32()
    _check(lib.ctl_scene_desc_diff(C.byref(a), C.byref(b), C.byref(mask)))
    return mask.value


def scene_desc_check(desc, parts=0):
    """ctl_scene_desc_check (host only): raises CtlError(ERR_INVALID) with the message ctl_scene_create (parts == 0) or ctl_scene_update (parts = the DIFF_* bits it would
    find) refuses `desc` with; returns dict(features, models, alpha_maps), the shade-kernel selection of the description"""
    state = (u32 * 3)()
    _check(lib.ctl_scene_desc_check(C.byref(desc), u32(parts), state))
    return {"features": state[0], "models": state[1], "alpha_maps": state[2]}


# ---- ctl_shading_eval (TEST INFRASTRUCTURE): the device BSDF / emitter / texture functions one call per query (include/ctl_amd.h CTL_EVAL_*)
EVAL_BUILD_BASIC, EVAL_BUILD_FULL, EVAL_BUILD_PARTIALS = 0, 1, 2
(EVAL_BSDF_SAMPLE, EVAL_BSDF_EVAL, EVAL_BSDF_SAMPLE_EVAL, EVAL_LIGHT_SAMPLE, EVAL_EMITTER_SAMPLE, EVAL_LIGHT_PDF, EVAL_LIGHT_EVAL, EVAL_ENV_EVAL, EVAL_TEXTURE, EVAL_MIP,
 EVAL_NORMAL_MAP, EVAL_ALPHA_TEST) = range(12)
EVAL_QUERY_FLOATS = (8, 10, 11, 9, 8, 14, 10, 3, 4, 7, 21, 3)
EVAL_RESULT_FLOATS = (9, 4, 13, 15, 19, 1, 3, 3, 3, 3, 9, 1)
lib.ctl_shading_eval.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, u32, u32, C.c_void_p, u32, C.c_void_p, u32]


def shading_eval(scene, build, what, queries, materials=None):
    """ctl_shading_eval: `queries` is an (n, EVAL_QUERY_FLOATS[what]) float32 array whose index columns hold the BITS of a uint32 (np.uint32(i).view(np.float32));
    materials: None or a ctypes array of ctl_material that replaces the scene's for this call.  Returns the (n, EVAL_RESULT_FLOATS[what]) float32 result rows.
    Raises CtlError with the library's code when the call is refused (nothing is launched then)."""
    import numpy as np
    q = np.ascontiguousarray(queries, np.float32)
    if q.ndim != 2:
        q = q.reshape(-1, EVAL_QUERY_FLOATS[what] if 0 <= what < len(EVAL_QUERY_FLOATS) else 1)
    ow = EVAL_RESULT_FLOATS[what] if 0 <= what < len(EVAL_RESULT_FLOATS) else 1
    out = np.zeros((len(q), ow), np.float32)
    n_m = len(materials) if materials is not None else 0
    _check(lib.ctl_shading_eval(scene._h, build, what, C.addressof(materials) if materials is not None else None, n_m, len(q), q.ctypes.data, q.shape[1], out.ctypes.data, ow))
    return out


def _rays_struct(rays):
    r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
    return r, r.ctypes.data_as(C.c_void_p)


def intersect(scene, rays, any_hit=False):
    """__internal__IntersectBuffers (Kernel/TraceHelper.cu:736-746). rays: (n, 8) = ox oy oz tmin dx dy dz tmax.
    Returns a structured array with dist, node_idx, tri_idx, u, v."""
    r, rp = _rays_struct(rays)
    hits = np.zeros(len(r), dtype=[("dist", "f4"), ("node_idx", "i4"), ("tri_idx", "i4"), ("u", "f4"), ("v", "f4")])
    _check(lib.ctl_intersect(scene._h, rp, u32(len(r)), hits.ctypes.data_as(C.c_void_p), 1 if any_hit else 0))
    return hits


def trace_single_ray(scene, origin, direction, tmin=0.0, tmax=3.402823466e+38):
    """TracerBase::TraceSingleRay (Kernel/Tracer.cu:74-78) -> the record of the closest hit (dist, node_idx, tri_idx, u, v)"""
    rays = np.zeros((1, 8), np.float32); rays[0, :3] = origin; rays[0, 3] = tmin; rays[0, 4:7] = direction; rays[0, 7] = tmax
    r, rp = _rays_struct(rays)
    hit = np.zeros(1, dtype=[("dist", "f4"), ("node_idx", "i4"), ("tri_idx", "i4"), ("u", "f4"), ("v", "f4")])
    _check(lib.ctl_trace_single_ray(scene._h, rp, hit.ctypes.data_as(C.c_void_p)))
    return hit[0]


ISECT_ANY_HIT, ISECT_ALPHA, ISECT_SINGLE = 1, 2, 4   # CTL_ISECT_*
_HIT_DTYPE = [("dist", "f4"), ("node_idx", "i4"), ("tri_idx", "i4"), ("u", "f4"), ("v", "f4")]
lib.ctl_intersect_ex.argtypes = [C.c_void_p, C.c_void_p, u32, C.c_void_p, u32]
lib.ctl_intersect_pair.argtypes = [C.c_void_p, C.c_void_p, u32, C.c_void_p, C.c_void_p, u32, C.c_void_p, u32]
lib.ctl_traversal_stack_histogram.argtypes = [C.c_void_p, u32, C.c_int]
lib.ctl_traversal_lds_rows.argtypes = [C.c_void_p]


def intersect_ex(scene, rays, any_hit=False, alpha=False, single=False, flags=None):
    """ctl_intersect_ex (TEST INFRASTRUCTURE): intersect() with a choice of kernel variant — alpha: the alpha-testing kernels (when the scene has alpha maps); single: the
    single-ray traversal of the PathTracer / PrimTracer plugins (flattened scenes only; it alpha-tests whenever the scene has alpha maps).  flags: the raw CTL_ISECT_* word
    instead of the three booleans.  A slot no kernel wrote comes back with tri_idx = node_idx = -2."""
    r, rp = _rays_struct(rays)
    hits = np.zeros(len(r), dtype=_HIT_DTYPE)
    if flags is None:
        flags = (ISECT_ANY_HIT if any_hit else 0) | (ISECT_ALPHA if alpha else 0) | (ISECT_SINGLE if single else 0)
    _check(lib.ctl_intersect_ex(scene._h, rp, u32(len(r)), hits.ctypes.data_as(C.c_void_p), u32(flags)))
    return hits


def intersect_pair(scene, rays, shadow_rays, alpha=False, flags=None):
    """ctl_intersect_pair (TEST INFRASTRUCTURE): the tracer's fused launch — closest hits of `rays`, then occlusion of `shadow_rays`, in one persistent launch.
    Returns (hits, occ): the record array of intersect() and a uint32 array (1 occluded, 0 free; 0xffffffff: the slot was never written)."""
    r, rp = _rays_struct(rays)
    s, sp = _rays_struct(shadow_rays)
    hits = np.zeros(len(r), dtype=_HIT_DTYPE); occ = np.zeros(len(s), np.uint32)
    if flags is None:
        flags = ISECT_ALPHA if alpha else 0
    _check(lib.ctl_intersect_pair(scene._h, rp, u32(len(r)), hits.ctypes.data_as(C.c_void_p), sp, u32(len(s)), occ.ctypes.data_as(C.c_void_p), u32(flags)))
    return hits, occ


def traversal_stack_histogram(reset=False, n_bins=96):
    """ctl_traversal_stack_histogram: rays of the counting traversals of flattened scenes so far (intersect_count, setCounting) by the deepest stack entry they used,
    as a uint64 array of n_bins (the last bin collects everything deeper); reset clears the counters after reading them"""
    h = np.zeros(n_bins, np.uint64)
    _check(lib.ctl_traversal_stack_histogram(h.ctypes.data_as(C.c_void_p), u32(n_bins), 1 if reset else 0))
    return h


def traversal_lds_rows():
    """ctl_traversal_lds_rows: stack entries a lane keeps in LDS, by kernel family (deeper entries live in scratch)"""
    r = (u32 * 5)()
    _check(lib.ctl_traversal_lds_rows(r))
    return dict(zip(("two_level", "q4", "q8", "single_q4", "single_q8"), (int(x) for x in r)))


def intersect_count(scene, rays, any_hit=False):
    r, rp = _rays_struct(rays)
    c = ctl_traversal_counts()
    _check(lib.ctl_intersect_count(scene._h, rp, u32(len(r)), 1 if any_hit else 0, C.byref(c)))
    return dict(n_inner=c.n_inner, n_tri=c.n_tri, n_inst=c.n_inst, wave_inner_iters=c.wave_inner_iters, wave_tri_iters=c.wave_tri_iters)


class Comm:
    """The framebuffer reduce of a multi-GPU render (ctl_comm_*, comm.cpp): one rank per process and GPU, RCCL over xGMI.
    Comm.unique_id() on one rank -> the 128 bytes to every rank -> Comm(id, rank, world) on every rank (collective) -> reduce(image, root)."""

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        _check(lib.ctl_comm_get_unique_id(buf))
        return bytes(buf)

    def __init__(self, unique_id, rank, world, timeout_ms=0):
        """timeout_ms: give ncclCommInitRank up after this long (0: $CTL_COMM_TIMEOUT_MS, else 120 s) — a rank that never arrives raises instead of hanging the job"""
        self._h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        _check(lib.ctl_comm_create_timeout(buf, C.c_int32(rank), C.c_int32(world), C.c_int32(timeout_ms), C.byref(self._h)))

    def reduce(self, image, root=0):
        """sum of all ranks' PixelData frames into `root`'s image, in place, one ncclReduce; returns when it is complete.  ONE call per frame: a second one on an
        image that already holds a reduced frame is refused (use reduce_to for a per-pass gather)"""
        _check(lib.ctl_image_reduce(image._h, self._h, C.c_int32(root)))

    def reduce_to(self, src, dst, root=0):
        """out of place (the per-pass gather of a progressive display): `dst` on the root = sum over the ranks of `src`; every rank's src stays its own cumulative frame.
        dst may be None on the other ranks"""
        _check(lib.ctl_image_reduce_to(src._h, dst._h if dst is not None else None, self._h, C.c_int32(root)))

    def gather(self, image, root=0):
        """north_star's exchange: every rank's own tiles + halo (ceil(tiles / world) x 65 x 65 x 28 B) to `root`'s image, in place, one ncclGather; ONE call per render"""
        _check(lib.ctl_image_gather(image._h, self._h, C.c_int32(root)))

    def gather_to(self, src, dst, root=0):
        """out of place (repeatable: the per-pass progressive gather): `dst` on the root = every rank's own tiles of its `src`; dst may be None on the other ranks"""
        _check(lib.ctl_image_gather_to(src._h, dst._h if dst is not None else None, self._h, C.c_int32(root)))

    def __del__(self):
        if getattr(self, "_h", None):
            lib.ctl_comm_destroy(self._h)
            self._h = None


class Image:
    """Engine/Image.h:31-91 — PixelData accumulator in HBM."""

    def __init__(self, width, height):
        self._h = C.c_void_p()
        self.width, self.height = width, height
        _check(lib.ctl_image_create(u32(width), u32(height), C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            lib.ctl_image_destroy(self._h)
            self._h = None

    def packedTileBytes(self, world):
        """bytes of one rank's packed tiles (ctl_image_packed_tile_bytes)"""
        n = C.c_uint64()
        _check(lib.ctl_image_packed_tile_bytes(u32(self.width), u32(self.height), u32(world), C.byref(n)))
        return n.value

    def packTiles(self, rank, world):
        """the tiles t % world == rank of this image with their one-pixel halo as (slots, 65 * 65, 7) float32 — what ctl_image_gather sends (ctl_image_pack_tiles)"""
        out = np.empty(self.packedTileBytes(world) // 4, np.float32)
        _check(lib.ctl_image_pack_tiles(self._h, u32(rank), u32(world), out.ctypes.data_as(C.c_void_p)))
        return out.reshape(-1, 65 * 65, 7)

    def unpackTiles(self, world, packed_all_ranks):
        """write the packed tiles of ALL ranks (rank-major) into this image: tiles copied, then halos added (ctl_image_unpack_tiles)"""
        a = np.ascontiguousarray(packed_all_ranks, np.float32)
        if a.nbytes != self.packedTileBytes(world) * world:
            raise ValueError("unpackTiles: %d bytes, expected %d" % (a.nbytes, self.packedTileBytes(world) * world))
        _check(lib.ctl_image_unpack_tiles(self._h, u32(world), a.ctypes.data_as(C.c_void_p)))

    def Clear(self):
        _check(lib.ctl_image_clear(self._h))

    def getPixelData(self):
        """(h, w, 7) float32: rgb[3], rgbSplat[3], weightSum."""
        a = np.zeros((self.height, self.width, 7), np.float32)
        _check(lib.ctl_image_read_pixels(self._h, a.ctypes.data_as(C.c_void_p)))
        return a

    def addSamples(self, samples):
        """Image::AddSample (Engine/Image.cu:22-44) for samples (n, 5) = sx, sy, r, g, b"""
        a = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1, 5)
        _check(lib.ctl_image_add_samples(self._h, u32(len(a)), a.ctypes.data_as(C.c_void_p)))

    def setPixelData(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(self.height, self.width, 7)
        _check(lib.ctl_image_write_pixels(self._h, a.ctypes.data_as(C.c_void_p)))

    def device_ptr(self):
        return lib.ctl_image_device_ptr(self._h)

    def applyImagePipeline(self, splat_scale=0.0, filter=None, process=None, tracer=None, variance=None):
        """applyImagePipeline(tracer, img, filter, process) (Kernel/ImagePipeline/ImagePipeline.cu:54-84): (h, w, 4) uint8 display image.
        filter = ctl_reconstruction_filter (see box_filter ... triangle_filter), ctl_nlm_filter (see nlm_filter) or None; process = ctl_tonemap (see tonemap) or None.
        The NonLocalMeans filter takes the per-pixel variance from exactly one of tracer= (its PixelVarianceBuffer) and variance= ((h, w) float32)."""
        a = np.zeros((self.height, self.width), np.uint32)
        if isinstance(filter, ctl_nlm_filter):
            v = None
            if variance is not None:
                v = np.ascontiguousarray(variance, dtype=np.float32)
                if v.size != self.width * self.height:
                    raise ValueError("applyImagePipeline: variance has %d values, the image %d pixels" % (v.size, self.width * self.height))
            _check(lib.ctl_image_apply_pipeline_nlm(self._h, f32(splat_scale), C.byref(filter), None if tracer is None else tracer._h, None if v is None else v.ctypes.data_as(C.c_void_p),
                                                    None if process is None else C.byref(process), a.ctypes.data_as(C.c_void_p)))
        elif tracer is not None or variance is not None:
            raise ValueError("applyImagePipeline: tracer= / variance= belong to the NonLocalMeans filter")
        elif filter is None and process is None:
            _check(lib.ctl_image_apply_pipeline(self._h, f32(splat_scale), a.ctypes.data_as(C.c_void_p)))
        else:
            _check(lib.ctl_image_apply_pipeline_ex(self._h, f32(splat_scale), None if filter is None else C.byref(filter),
                                                   None if process is None else C.byref(process), a.ctypes.data_as(C.c_void_p)))
        return a.view(np.uint8).reshape(self.height, self.width, 4)

    def getFilteredData(self):
        """Image::getFilteredData: (h, w) uint32 RGBE (r | g << 8 | b << 16 | e << 24), the plane the last pipeline call with a filter or a post-process left"""
        a = np.zeros((self.height, self.width), np.uint32)
        _check(lib.ctl_image_read_filtered(self._h, a.ctypes.data_as(C.c_void_p)))
        return a

    def getLuminanceInfo(self):
        """Image::ComputeLuminanceInfo, read-only: (min, max, avg, logAvg) float32 of the filtered plane's luminance as the last pipeline call with a post-process
        computed and used them (stored by that call, not recomputed here)"""
        a = np.zeros(4, np.float32)
        _check(lib.ctl_image_luminance_info(self._h, a.ctypes.data_as(C.c_void_p)))
        return a

    def lastFilterMs(self):
        """HIP-event time (ms) of the NonLocalMeans kernel of the last applyImagePipeline with nlm_filter (measurement)"""
        v = f32()
        _check(lib.ctl_image_last_filter_ms(self._h, C.byref(v)))
        return v.value

    def WriteDisplayImage(self, path, splat_scale=0.0):
        """Image::WriteDisplayImage: .png (display image), .hdr / .pfm (linear)."""
        _check(lib.ctl_image_write_file(self._h, f32(splat_scale), path.encode()))

    def getRGB(self, splat_scale=0.0):
        """copySamplesToOutput (Kernel/ImagePipeline/ImagePipeline.cu:14-30) up to linear RGB."""
        a = np.zeros((self.height, self.width, 3), np.float32)
        _check(lib.ctl_image_resolve_rgb(self._h, f32(splat_scale), a.ctypes.data_as(C.c_void_p)))
        return a

class _Parameters:
    def __init__(self, tracer):
        self._t = tracer

    def setValue(self, key, value):
        """bool, int (also the index of an enum value), float, or the name of an enum value (TracerParameterCollection::setValue, Kernel/TracerSettings.h:277)"""
        if isinstance(value, bool):
            _check(lib.ctl_tracer_set_param_bool(self._t._h, key.encode(), 1 if value else 0))
        elif isinstance(value, str):
            _check(lib.ctl_tracer_set_param_enum(self._t._h, key.encode(), value.encode()))
        elif isinstance(value, float):
            _check(lib.ctl_tracer_set_param_float(self._t._h, key.encode(), f32(value)))
        else:
            _check(lib.ctl_tracer_set_param_int(self._t._h, key.encode(), int(value)))

    def getFloat(self, key):
        v = f32()
        _check(lib.ctl_tracer_get_param_float(self._t._h, key.encode(), C.byref(v)))
        return v.value

    def getValue(self, key):
        v = C.c_int()
        _check(lib.ctl_tracer_get_param_int(self._t._h, key.encode(), C.byref(v)))
        return v.value


class WavefrontPathTracer:
    """Integrators/PseudoRealtime/WavefrontPathTracer.h:24-67 behind Tracer<true> (Kernel/Tracer.h:193-294).
    Build-specific parameters, through getParameters().setValue like the reference's own: PassBatch, AlphaTest, ShadeByModelClass, FuseTraversal, PathSemantics,
    U16Barycentrics, OrderedAccumulation(MaxMB), and ParticipatingMedia (bool, default False: a scene with participating media is refused; True: it is rendered under
    PathTrace's rules, the volume table read at every pass — refused together with PathSemantics = "Wavefront")."""

    PLUGIN = b"WavefrontPathTracer"

    def __init__(self):
        self._h = C.c_void_p()
        _check(lib.ctl_tracer_create(self.PLUGIN, C.byref(self._h)))
        self._scene = None

    def __del__(self):
        if getattr(self, "_h", None):
            lib.ctl_tracer_destroy(self._h)
            self._h = None
        self._free_depth()

    def _free_depth(self):
        d = getattr(self, "_depth", None)
        if d is not None:
            lib.ctl_device_free(d[0]); self._depth = None

    def getParameters(self):
        return _Parameters(self)

    def Resize(self, w, h):
        _check(lib.ctl_tracer_resize(self._h, u32(w), u32(h)))
        self._size = (w, h)

    def InitializeScene(self, scene):
        self._scene = scene
        _check(lib.ctl_tracer_initialize_scene(self._h, scene._h))

    def reservePasses(self, n):
        """size the ray queues for a DoPasses(n) to come (they would otherwise grow inside that call)"""
        _check(lib.ctl_tracer_reserve_passes(self._h, u32(n)))

    def setBlockWeight(self, block_x, block_y, weight):
        """IUserPreferenceSampler::setWeight of the tracer's block sampler (parameter BlockSamplerType); after Resize"""
        _check(lib.ctl_tracer_set_block_weight(self._h, u32(block_x), u32(block_y), f32(weight)))

    def getBlockCounts(self, width, height):
        """samples per 64x64 block of the last rendered pass: (blocks_y, blocks_x) uint8"""
        by, bx = (height + 63) // 64, (width + 63) // 64
        a = np.zeros((by, bx), np.uint8)
        _check(lib.ctl_tracer_get_block_counts(self._h, a.ctypes.data_as(C.c_void_p), u32(bx * by)))
        return a

    def setTileShard(self, rank, world):
        _check(lib.ctl_tracer_set_tile_shard(self._h, u32(rank), u32(world)))

    def setSamplerTables(self, t1, t2):
        t1, t2 = _f32(t1), _f32(t2)
        assert t1.size == SAMPLER_N1 and t2.size == 2 * SAMPLER_N1
        _check(lib.ctl_tracer_set_sampler_tables(self._h, _fp(t1), _fp(t2)))

    def DoPass(self, image, new_trace=False):
        _check(lib.ctl_tracer_do_pass(self._h, image._h, 1 if new_trace else 0))

    def DoPasses(self, image, n, new_trace=False):
        _check(lib.ctl_tracer_do_passes(self._h, image._h, 1 if new_trace else 0, u32(n)))

    def Debug(self, image, x, y):
        """TracerBase::Debug(Image*, Vec2i) (Kernel/Tracer.h:119-123): draws the next set of sampling tables from the tracer's generator, follows one path for the pixel
        (PathTracer plugin) and returns its radiance as 3 floats"""
        out = (f32 * 3)()
        _check(lib.ctl_tracer_debug_pixel(self._h, image._h, u32(x), u32(y), out))
        return np.array(out[:], np.float32)

    def setDepthBuffer(self, width, height):
        """IDepthTracer::setDepthBuffer: allocates width*height floats on the device and hands them to the tracer; read them back with getDepthBuffer()"""
        lib.ctl_tracer_set_depth_buffer.argtypes = [C.c_void_p, C.c_void_p, u32, u32]
        if getattr(self, "_depth", None) is not None:      # a buffer set before: the tracer lets go of it first, then it is freed
            lib.ctl_tracer_set_depth_buffer(self._h, None, u32(0), u32(0)); self._free_depth()
        p = C.c_void_p()
        _check(lib.ctl_device_malloc(C.c_size_t(4 * width * height), C.byref(p)))
        try:
            _check(lib.ctl_tracer_set_depth_buffer(self._h, p, u32(width), u32(height)))
        except Exception:
            lib.ctl_device_free(p)                          # the tracer refused (the PathTracer plugin is no IDepthTracer): nothing keeps the allocation
            raise
        self._depth = (p, width, height)

    def getDepthBuffer(self):
        p, w, h = self._depth
        out = np.zeros((h, w), np.float32)
        _check(lib.ctl_device_synchronize())
        _check(lib.ctl_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, C.c_size_t(out.nbytes)))
        return out

    def setPixelVariance(self, on):
        """keep the reference's PixelVarianceBuffer up to date after every pass (what nlm_filter is guided by).  Off by default; the frame does not change"""
        _check(lib.ctl_tracer_set_pixel_variance(self._h, 1 if on else 0))

    def getPixelVariance(self):
        """PixelVarianceInfo::computeVariance() per pixel: (height, width) float32, NaN before the first pass"""
        if getattr(self, "_size", None) is None:
            raise CtlError(-1, "getPixelVariance: Resize was not called")
        a = np.zeros((self._size[1], self._size[0]), np.float32)
        _check(lib.ctl_tracer_read_pixel_variance(self._h, a.ctypes.data_as(C.c_void_p)))
        return a

    def setCounting(self, on):
        """count N_inner / N_tri / N_inst in the intersect kernels (measurement mode)"""
        _check(lib.ctl_tracer_set_counting(self._h, 1 if on else 0))

    def stats(self):
        s = ctl_tracer_stats()
        _check(lib.ctl_tracer_get_stats(self._h, C.byref(s)))
        return s

    def getRaysInLastPass(self):
        return self.stats().rays_last_pass

    def getLastTimeSpentRenderingSec(self):
        return self.stats().seconds_last_pass

    def getNumPassesDone(self):
        return self.stats().passes_done


class PathTracer(WavefrontPathTracer):
    """Integrators/PathTracer.h:7-31 — the megakernel integrator (one kernel per pass) behind the same plugin API; needs a
    flattened scene.  For A/B against the wavefront tracer."""
    PLUGIN = b"PathTracer"


# PathTrace_DrawMode (Integrators/PrimTracer.h:7), in PTDM order: the values of the PrimTracer's DrawingMode parameter
PathTrace_DrawMode = ("linear_depth", "D3D_depth", "v_absdot_n_geo", "v_dot_n_geo", "v_dot_n_shade", "n_geo_colored", "n_shade_colored", "uv", "bary_coords",
                      "first_Le", "first_f", "first_f_direct", "first_non_delta_Le", "first_non_delta_f", "first_non_delta_f_direct")


class PrimTracer(WavefrontPathTracer):
    """Integrators/PrimTracer.h:10-27 — PrimTracer : Tracer<false>, IDepthTracer ("direct" in the reference's example program): one sample per pixel at the
    pixel's own position, the quantity DrawingMode names (PathTrace_DrawMode; default first_f), MaxPathLength (default 7) for the delta chains of the
    first_non_delta_* modes.  Non-progressive: every pass clears the image, getNumPassesDone() is 1 after any call.  Needs a flattened scene."""
    PLUGIN = b"PrimTracer"


class SequenceGenerator:
    """SamplingSequenceGeneratorHost<IndependantSamplingSequenceGenerator> (Kernel/Sampler.h:36-85)."""

    def __init__(self):
        self._h = C.c_void_p()
        _check(lib.ctl_sequence_generator_create(C.byref(self._h)))

    def __del__(self):
        if getattr(self, "_h", None):
            lib.ctl_sequence_generator_destroy(self._h)
            self._h = None

    def compute(self):
        t1 = np.zeros(SAMPLER_N1, np.float32)
        t2 = np.zeros(2 * SAMPLER_N1, np.float32)
        _check(lib.ctl_sequence_generator_compute(self._h, _fp(t1), _fp(t2)))
        return t1, t2

    def compute_many(self, n, threads=8):
        """tables of the next n passes, (n, 30*4096) and (n, 2*30*4096), generated in parallel through XORWOW skip-ahead"""
        t1 = np.zeros((n, SAMPLER_N1), np.float32)
        t2 = np.zeros((n, 2 * SAMPLER_N1), np.float32)
        _check(lib.ctl_sequence_generator_compute_many(self._h, u32(n), _fp(t1), _fp(t2), u32(threads)))
        return t1, t2

    def compute_many_device(self, n):
        """the same tables written in HBM by the tracers' k_sequence_fill and copied back (needs a HIP device)"""
        t1 = np.zeros((n, SAMPLER_N1), np.float32)
        t2 = np.zeros((n, 2 * SAMPLER_N1), np.float32)
        _check(lib.ctl_sequence_generator_compute_many_device(self._h, u32(n), _fp(t1), _fp(t2)))
        return t1, t2
