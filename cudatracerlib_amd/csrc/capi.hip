// capi.hip — the extern "C" surface declared in include/ctl_amd.h.  Exceptions of the C++ layer (the reference's
// error convention, Defines.cpp:15-29) are mapped to ctl_status codes + ctl_last_error().
#include "../../include/ctl_amd.h"
#include "tracer.h"
#include "prim_tracer.h"
#include "kernels.h"
#include "scene_builder.h"
#include "scene_checks.h"
#include "mitsuba_loader.h"
#include "flatten.h"
#include "flat_rebuild.h"
#include "flat_nodes.h"
#include "flat_meshes.h"
#include "flat_mesh_set.h"
#include "flat_device.h"
#include "scene_image_set.h"
#include "mesh_skin.h"
#include "shape_set.h"
#include "material_factory.h"
#include "material_textures.h"
#include "image_io.h"
#include <memory>
#include "scene_cache.h"
#include "shading_eval.h"
#include "traversal_probe.h"
#include "volume_eval.h"
#include <cstdlib>
#include <cstring>
#include <string>
#include <new>

using namespace ctl;

struct ctl_builder { scene_builder b; };
struct ctl_scene {
    Scene s; uint32_t n_materials, n_images;   // the sizes of the description's material and image arrays (ctl_shading_eval checks a query's indices against them)
    node_set_basis basis;   // the small arrays of the description the scene holds, as ctl_scene_update_nodes checks a new node set against them (flat_nodes.h)
    ctl_scene(const ctl_scene_desc& d, bool flatten, int fmt = -1, bool reduced_rt = false) : s(d, flatten, fmt, reduced_rt), n_materials(d.n_materials), n_images(d.n_images) { basis.fill(d); }
};
// basis: of the description the tree stands for; extra_missing: triangles an added node got no entry for (flat_nodes.h), on top of what the entries themselves show
struct ctl_flat_bvh { flat_scene f; node_set_basis basis; std::vector<uint32_t> extra_missing; };
struct ctl_image { Image img; ctl_image(uint32_t w, uint32_t h) : img(w, h) {} };
// wavefront / scene: the WavefrontPathTracer judges what it refuses of participating media (WavefrontPathTracer::check_media: a scene that has media while its
// ParticipatingMedia is off, PathSemantics = Wavefront while it is on) here, when the scene is handed over and — in front of every other complaint — when a pass starts;
// the PathTracer and the PrimTracer judge theirs themselves.  `scene` is the pointer InitializeScene got, the one DoPass reads the scene through
struct ctl_tracer {
    std::unique_ptr<TracerBase> t; bool wavefront = false; const Scene* scene = nullptr;
    void refuse_media() const {   // (and, at the same two places, what it refuses of TextureFiltering: check_texture_filtering)
        if (!wavefront || !scene) return;
        const WavefrontPathTracer* w = static_cast<const WavefrontPathTracer*>(t.get());
        w->check_media(scene); w->check_texture_filtering();
    }
};
struct ctl_sequence_generator { sequence_generator g; };

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define CTL_TRY try {
#define CTL_CATCH                                                                    \
    } catch (const hip_error& e) { return fail(device_count() > 0 ? CTL_ERR_HIP : CTL_ERR_NO_DEVICE, e.what()); } \
    catch (const io_error& e) { return fail(CTL_ERR_IO, e.what()); }             \
    catch (const unsupported_error& e) { return fail(CTL_ERR_UNSUPPORTED, e.what()); } \
    catch (const internal_error& e) { return fail(CTL_ERR_INTERNAL, e.what()); } \
    catch (const std::bad_alloc&) { return fail(CTL_ERR_INVALID, "out of host memory"); } \
    catch (const std::exception& e) { return fail(CTL_ERR_INVALID, e.what()); }      \
    return CTL_OK;
#define CTL_REQUIRE(c, msg) if (!(c)) return fail(CTL_ERR_INVALID, msg)

extern "C" {

const char* ctl_last_error(void) { return g_err.c_str(); }
const char* ctl_version(void) { return "cudatracerlib_amd 0.1 (gfx950)"; }
int ctl_device_count(void) { return device_count(); }

// ---- builder
int ctl_builder_create(ctl_builder** out) { CTL_REQUIRE(out, "null out"); CTL_TRY *out = new ctl_builder(); CTL_CATCH }
void ctl_builder_destroy(ctl_builder* b) { delete b; }
int ctl_builder_add_mesh(ctl_builder* b, const float* positions, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri, const float* normals, const float* uvs,
                         const uint8_t* tri_material, const ctl_material* materials, uint32_t n_mat, uint32_t* mesh_index_out) {
    CTL_REQUIRE(b, "null builder");
    CTL_TRY uint32_t i = b->b.add_mesh(positions, n_vert, indices, n_tri, normals, uvs, tri_material, materials, n_mat); if (mesh_index_out) *mesh_index_out = i; CTL_CATCH
}
int ctl_builder_update_mesh(ctl_builder* b, uint32_t mesh_index, const float* positions, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri, const float* normals, const float* uvs) {
    CTL_REQUIRE(b, "null builder");
    CTL_TRY b->b.update_mesh(mesh_index, positions, n_vert, indices, n_tri, normals, uvs); CTL_CATCH
}
int ctl_builder_update_image(ctl_builder* b, uint32_t image_index, const uint32_t* texels, uint32_t width, uint32_t height) {
    CTL_REQUIRE(b, "null builder");
    CTL_TRY b->b.update_image(image_index, texels, width, height); CTL_CATCH
}
int ctl_mip_pyramid_host(const ctl_mipmap* image, uint32_t* texels_out, size_t capacity, uint32_t* levels_out, uint32_t level_offsets_out[15]) {
    CTL_REQUIRE(image && image->texels && image->width && image->height, "ctl_mip_pyramid_host: null or empty image");
    CTL_REQUIRE(image->texel_type <= CTL_TEXEL_RGBCOL, "ctl_mip_pyramid_host: unknown texel type");
    CTL_TRY
        std::vector<uint32_t> pool; mip_level_table L;
        mip_pyramid_append(*image, pool, L);
        if (levels_out) *levels_out = L.levels;
        if (level_offsets_out) for (int k = 0; k < 15; k++) level_offsets_out[k] = L.offsets[k];
        if (texels_out) {
            if (capacity < pool.size()) throw std::runtime_error("ctl_mip_pyramid_host: the pyramid holds " + std::to_string(pool.size()) + " texels in " + std::to_string(L.levels) + " levels");
            std::memcpy(texels_out, pool.data(), pool.size() * 4);
        }
    CTL_CATCH
}
int ctl_builder_set_bvh_mode(ctl_builder* b, uint32_t mode) { CTL_REQUIRE(b && mode <= CTL_BVH_BINNED, "null builder or unknown mode"); b->b.bvh_mode = mode; return CTL_OK; }
int ctl_builder_add_node(ctl_builder* b, uint32_t mesh_index, const ctl_float4x4* to_world, uint32_t* node_index_out) {
    CTL_REQUIRE(b, "null builder");
    CTL_TRY uint32_t i = b->b.add_node(mesh_index, to_world); if (node_index_out) *node_index_out = i; CTL_CATCH
}
int ctl_builder_remove_node(ctl_builder* b, uint32_t node_index) {
    CTL_REQUIRE(b, "null builder");
    CTL_REQUIRE(node_index < b->b.nodes.size(), "ctl_builder_remove_node: bad node index");
    CTL_REQUIRE(b->b.nodes.size() > 1, "ctl_builder_remove_node: the last node of the builder stays (a scene has at least one node)");
    if (b->b.nodes[node_index].n_lights) return fail(CTL_ERR_UNSUPPORTED, "ctl_builder_remove_node: node " + std::to_string(node_index) + " carries area lights");
    CTL_TRY b->b.remove_node(node_index); CTL_CATCH
}
int ctl_builder_add_area_light(ctl_builder* b, uint32_t node_index, uint32_t local_material, const float radiance[3]) {
    CTL_REQUIRE(b && radiance, "null argument");
    CTL_TRY b->b.add_area_light(node_index, local_material, radiance); CTL_CATCH
}
int ctl_builder_add_area_light_ex(ctl_builder* b, uint32_t node_index, uint32_t local_material, const float radiance[3], const ctl_texture* rad_texture, int32_t orthogonal) {
    CTL_REQUIRE(b && radiance, "null argument");
    CTL_TRY b->b.add_area_light(node_index, local_material, radiance, rad_texture, orthogonal != 0); CTL_CATCH
}
int ctl_builder_add_point_light(ctl_builder* b, const float position[3], const float intensity[3]) {
    CTL_REQUIRE(b && position && intensity, "null argument");
    CTL_TRY b->b.add_point_light(position, intensity); CTL_CATCH
}
int ctl_builder_add_spot_light(ctl_builder* b, const float position[3], const float target[3], const float intensity[3], float cutoff_angle_degrees, float beam_width_degrees) {
    CTL_REQUIRE(b && position && target && intensity, "null argument");
    CTL_TRY b->b.add_spot_light(position, target, intensity, cutoff_angle_degrees, beam_width_degrees); CTL_CATCH
}
int ctl_builder_add_distant_light(ctl_builder* b, const float direction[3], const float irradiance[3], float scene_radius) {
    CTL_REQUIRE(b && direction && irradiance, "null argument");
    CTL_TRY b->b.add_distant_light(direction, irradiance, scene_radius); CTL_CATCH
}
int ctl_builder_add_image(ctl_builder* b, const uint32_t* texels, uint32_t width, uint32_t height, uint32_t texel_type, uint32_t wrap_mode, uint32_t filter_mode, uint32_t* image_index_out) {
    CTL_REQUIRE(b && texels, "null argument");
    CTL_TRY uint32_t i = b->b.add_image(texels, width, height, texel_type, wrap_mode, filter_mode); if (image_index_out) *image_index_out = i; CTL_CATCH
}
int ctl_builder_set_environment_map(ctl_builder* b, uint32_t image_index, const float scale[3], const ctl_float4x4* to_world) {
    CTL_REQUIRE(b && scale, "null argument");
    CTL_TRY b->b.set_environment_map(image_index, scale, to_world); CTL_CATCH
}
int ctl_builder_add_material(ctl_builder* b, const ctl_material* material, uint32_t* index_out) {
    CTL_REQUIRE(b && material, "null argument");
    CTL_TRY uint32_t i = b->b.add_aux_material(*material); if (index_out) *index_out = i; CTL_CATCH
}
int ctl_builder_set_rough_transmittance(ctl_builder* b, uint32_t slot, const ctl_rough_transmittance* table) {
    CTL_REQUIRE(b && table, "null argument");
    CTL_TRY b->b.set_rough_transmittance(slot, *table); CTL_CATCH
}
int ctl_builder_load_rough_transmittance(ctl_builder* b, uint32_t slot, const char* dat_path) {
    CTL_REQUIRE(b && dat_path, "null argument");
    CTL_TRY b->b.load_rough_transmittance(slot, dat_path); CTL_CATCH
}
int ctl_builder_set_camera_lookat(ctl_builder* b, const float pos[3], const float target[3], const float up[3], float fov_degrees, uint32_t width, uint32_t height) {
    CTL_REQUIRE(b && pos && target && up && width && height, "bad argument");
    CTL_TRY b->b.set_camera_lookat(pos, target, up, fov_degrees, width, height); CTL_CATCH
}
int ctl_builder_set_camera(ctl_builder* b, const ctl_sensor* sensor) { CTL_REQUIRE(b && sensor, "null argument"); CTL_TRY b->b.set_camera(*sensor); CTL_CATCH }
int ctl_builder_set_node_transform(ctl_builder* b, uint32_t node_index, const ctl_float4x4* to_world) { CTL_REQUIRE(b && to_world, "null argument"); CTL_TRY b->b.set_node_transform(node_index, *to_world, true); CTL_CATCH }
int ctl_builder_create_volume(ctl_builder* b, const ctl_volume* volume, uint32_t* index_out) {
    CTL_REQUIRE(b && volume, "null argument");
    CTL_TRY uint32_t i = b->b.create_volume(*volume); if (index_out) *index_out = i; CTL_CATCH
}
int ctl_builder_set_volume(ctl_builder* b, uint32_t index, const ctl_volume* volume) { CTL_REQUIRE(b && volume, "null argument"); CTL_TRY b->b.set_volume(index, *volume); CTL_CATCH }
int ctl_builder_finalize(ctl_builder* b, ctl_scene_desc* out) { CTL_REQUIRE(b && out, "null argument"); CTL_TRY b->b.finalize(*out); CTL_CATCH }

int ctl_material_update(ctl_material* m) {   // (a weight from an IMAGE texture's average is final after ctl_builder_finalize, material_textures.h)
    CTL_REQUIRE(m, "null argument"); CTL_REQUIRE(material_update(*m), "unknown bsdf_type"); material_update_textures(*m, image_set()); return CTL_OK;
}
int ctl_builder_create_volume_grid(ctl_builder* b, const uint32_t* dims, uint32_t n_dims, const ctl_float4x4* volume_to_world, const ctl_phase_function* phase, uint32_t* index_out) {
    CTL_REQUIRE(b && dims && volume_to_world && phase, "null argument");
    CTL_TRY uint32_t i = b->b.create_volume_grid(dims, n_dims, *volume_to_world, *phase); if (index_out) *index_out = i; CTL_CATCH
}
int ctl_builder_set_volume_grid_data(ctl_builder* b, uint32_t index, uint32_t which, const float* data, uint32_t n) { CTL_REQUIRE(b && data, "null argument"); CTL_TRY b->b.set_volume_grid_data(index, which, data, n); CTL_CATCH }
int ctl_builder_set_volume_grid_coefficients(ctl_builder* b, uint32_t index, const float* sig_a_min, const float* sig_a_max, const float* sig_s_min, const float* sig_s_max) {
    CTL_REQUIRE(b && sig_a_min && sig_a_max && sig_s_min && sig_s_max, "null argument");
    CTL_TRY b->b.set_volume_grid_coefficients(index, sig_a_min, sig_a_max, sig_s_min, sig_s_max); CTL_CATCH
}
int ctl_volume_update(ctl_volume* v) { CTL_REQUIRE(v, "null argument"); CTL_TRY volume_update(*v); CTL_CATCH }
// ---- the participating-media functions (volume.h) one call per query, on the host or by a kernel (volume_eval.hip)
int ctl_volume_eval(const ctl_scene_desc* desc, int32_t what, const float* queries, uint32_t n, float* out, int32_t on_device) {
    CTL_REQUIRE(desc && (n == 0 || (queries && out)), "null argument");
    CTL_TRY volume_eval(*desc, what, queries, n, out, on_device != 0); CTL_CATCH
}
float ctl_fresnel_diffuse_reflectance(float eta) { return fresnel_diffuse_reflectance(eta); }
// ---- the shared transcendental functions (ctl_fmath.h), evaluated on the host or by a kernel: the parity tests hold the two bit-identical
__global__ void k_shared_math(int which, int n, const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= n) return;
    switch (which) {
    case 0: out[i] = fm::sin(x[i]); break; case 1: out[i] = fm::cos(x[i]); break; case 2: out[i] = fm::tan(x[i]); break; case 3: out[i] = fm::acos(x[i]); break;
    case 4: out[i] = fm::atan(x[i]); break; case 5: out[i] = fm::atan2(x[i], y[i]); break; case 6: out[i] = fm::exp(x[i]); break; case 7: out[i] = fm::log(x[i]); break;
    case 8: out[i] = fm::log2(x[i]); break; default: out[i] = fm::pow(x[i], y[i]); break;
    }
}
int ctl_shared_math_eval(int32_t which, uint32_t n, const float* x, const float* y, float* out, int32_t on_device) {
    CTL_REQUIRE(x && y && out && which >= 0 && which <= 9, "null argument or unknown function");
    CTL_TRY
        if (!on_device) {
            for (uint32_t i = 0; i < n; i++) {
                switch (which) {
                case 0: out[i] = fm::sin(x[i]); break; case 1: out[i] = fm::cos(x[i]); break; case 2: out[i] = fm::tan(x[i]); break; case 3: out[i] = fm::acos(x[i]); break;
                case 4: out[i] = fm::atan(x[i]); break; case 5: out[i] = fm::atan2(x[i], y[i]); break; case 6: out[i] = fm::exp(x[i]); break; case 7: out[i] = fm::log(x[i]); break;
                case 8: out[i] = fm::log2(x[i]); break; default: out[i] = fm::pow(x[i], y[i]); break;
                }
            }
        } else {
            require_device();
            dbuf<float> dx, dy, dout; dx.alloc(n); dy.alloc(n); dout.alloc(n);
            CTL_HIP(hipMemcpy(dx.p, x, (size_t)n * 4, hipMemcpyHostToDevice)); CTL_HIP(hipMemcpy(dy.p, y, (size_t)n * 4, hipMemcpyHostToDevice));
            hipLaunchKernelGGL(k_shared_math, dim3((n + 255) / 256), dim3(256), 0, 0, (int)which, (int)n, (const float*)dx.p, (const float*)dy.p, dout.p);
            CTL_HIP(hipMemcpy(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost));
        }
    CTL_CATCH
}
// ---- ctl_shading_eval (TEST INFRASTRUCTURE): the device shading functions one call per query (shading_eval.h).  Everything a query can name is checked here, on the
// host, against host copies of the scene's materials and emitters: a kernel is launched only for queries it can answer.
namespace {
struct eval_check {
    int build; bool override_mats; std::vector<ctl_material> mats; std::vector<ctl_light> lights; uint32_t n_images; bool tables[3]; bool have_reduced;
    int code = CTL_OK; std::string why;
    bool refuse(int c, const std::string& w) { code = c; why = "ctl_shading_eval: " + w; return false; }
    bool texture(const ctl_texture& t, bool any_build = false) {   // any_build: the caller's function reads image textures in every build (the alpha test, mipmap.h)
        if (t.type != 0 && t.type != CTL_TEX_CONSTANT && t.type != CTL_TEX_CHECKER && t.type != CTL_TEX_IMAGE) return refuse(CTL_ERR_INVALID, "unknown texture type " + std::to_string(t.type));
        if (t.type == CTL_TEX_IMAGE) {
            if (t.image != 0xffffffffu && t.image >= n_images) return refuse(CTL_ERR_INVALID, "image index " + std::to_string(t.image) + " of " + std::to_string(n_images));
            if (build == 0 && !any_build) return refuse(CTL_ERR_UNSUPPORTED, "the basic build carries no image textures");
        }
        return true;
    }
    bool material(uint32_t mi, bool nested) {
        if (mi >= mats.size()) return refuse(CTL_ERR_INVALID, std::string(nested ? "nested " : "") + "material index " + std::to_string(mi) + " of " + std::to_string(mats.size()));
        const ctl_material& M = mats[mi]; const uint32_t t = M.bsdf_type;
        if (!is_simple_bsdf(t) && !is_nesting_bsdf(t)) return refuse(CTL_ERR_INVALID, "unknown bsdf_type " + std::to_string(t));
        if (nested && is_nesting_bsdf(t)) return refuse(CTL_ERR_INVALID, "a nested material is itself a nesting model");
        if (build == 0) {   // what the scene's shade kernel would need the full build for (device_scene.h).  A BSDF query does not read the surface map: kEvalNormalMap judges it
            const uint32_t f = bsdf_shade_features(M);
            if (f & (kShadeMoreBsdfs | kShadeRoughBsdfs | kShadeNestingBsdfs)) return refuse(CTL_ERR_UNSUPPORTED, "the basic build does not carry bsdf_type " + std::to_string(t));
            if (f & kShadeMoreMicrofacet) return refuse(CTL_ERR_UNSUPPORTED, "the basic build carries neither the Phong distribution nor Beckmann visible-normal sampling");
        }
        if (const uint32_t* dist = bsdf_distribution(M)) {
            if (*dist > CTL_MF_PHONG) return refuse(CTL_ERR_INVALID, "unknown microfacet distribution");
            if (bsdf_reads_rough_transmittance(t)) {
                if (!tables[*dist]) return refuse(CTL_ERR_INVALID, "a rough BSDF without its transmittance table (slot " + std::to_string(*dist) + ")");
                if (M.reserved_[0] && (override_mats || !have_reduced)) return refuse(CTL_ERR_INVALID, "a material that names a reduced transmittance table the call does not have");
            }
        }
        for (int k = 0; k < 4; k++) if (!texture(M.tex[k])) return false;
        for (int k = 0; k < nested_bsdf_count(t); k++) if (!material(M.u[2 + k], true)) return false;
        return true;
    }
    bool light(uint32_t li) {
        if (li >= lights.size()) return refuse(CTL_ERR_INVALID, "light index " + std::to_string(li) + " of " + std::to_string(lights.size()));
        const ctl_light& L = lights[li];
        if (L.type < CTL_LIGHT_POINT || L.type > CTL_LIGHT_INFINITE) return refuse(CTL_ERR_INVALID, "unknown light type");
        if (build == 0 && (light_shade_features(L) & kShadeMoreLights)) return refuse(CTL_ERR_UNSUPPORTED, "the basic build carries point lights and plain area lights only");
        if (L.type == CTL_LIGHT_INFINITE && L.env_image >= n_images) return refuse(CTL_ERR_INVALID, "environment image index out of range");
        if (L.type == CTL_LIGHT_DIFFUSE && L.rad_texture.type == CTL_TEX_IMAGE && L.rad_texture.image != 0xffffffffu && L.rad_texture.image >= n_images) return refuse(CTL_ERR_INVALID, "image index of a light texture out of range");
        return true;
    }
};
uint32_t eval_word(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
}
int ctl_shading_eval(const ctl_scene* scene, int32_t build, int32_t what, const ctl_material* materials, uint32_t n_materials, uint32_t n, const float* queries, uint32_t query_stride,
                     float* out, uint32_t out_stride) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, "no HIP device: the MI355X path tracer has no CPU fallback");
    CTL_REQUIRE(scene && (n == 0 || (queries && out)), "null argument");
    CTL_REQUIRE(build >= 0 && build <= 2, "ctl_shading_eval: unknown build");
    CTL_REQUIRE(what >= 0 && what < kEvalCount, "ctl_shading_eval: unknown function");
    CTL_REQUIRE(query_stride >= kEvalQueryFloats[what] && out_stride >= kEvalResultFloats[what], "ctl_shading_eval: a row is shorter than the function's query / result");
    CTL_REQUIRE(!materials || n_materials, "ctl_shading_eval: an empty material array");
    if (what == kEvalMip && build != 2) return fail(CTL_ERR_UNSUPPORTED, "ctl_shading_eval: filtered texture lookups live in the partials build");
    if (what == kEvalNormalMap && build == 0) return fail(CTL_ERR_UNSUPPORTED, "ctl_shading_eval: the basic build carries no surface maps");
    CTL_TRY
        require_device();
        dev_scene S = scene->s.S;   // this call's copy: a material override replaces its mats pointer only
        eval_check K; K.build = build; K.override_mats = materials != nullptr; K.n_images = scene->n_images; K.have_reduced = S.rt_reduced != nullptr;
        if (materials) K.mats.assign(materials, materials + n_materials);
        else { K.mats.resize(scene->n_materials); if (scene->n_materials) CTL_HIP(hipMemcpy(K.mats.data(), S.mats, sizeof(ctl_material) * scene->n_materials, hipMemcpyDeviceToHost)); }
        K.lights.resize(S.n_lights_buf); if (S.n_lights_buf) CTL_HIP(hipMemcpy(K.lights.data(), S.lights, sizeof(ctl_light) * S.n_lights_buf, hipMemcpyDeviceToHost));
        K.tables[0] = K.tables[1] = K.tables[2] = false;
        if (S.rough_transmittance) { ctl_rough_transmittance t3[3]; CTL_HIP(hipMemcpy(t3, S.rough_transmittance, sizeof(t3), hipMemcpyDeviceToHost)); for (int k = 0; k < 3; k++) K.tables[k] = t3[k].trans && t3[k].diff_trans; }
        bool ok = true;
        if (what == kEvalEnvEval && n) {
            if (S.env_map_index == 0xffffffffu) ok = K.refuse(CTL_ERR_INVALID, "the scene has no environment emitter"); else ok = K.light(S.env_map_index);
        }
        if (what == kEvalEmitterSample && n) {
            if (S.num_lights > CTL_MAX_NUM_LIGHTS) ok = K.refuse(CTL_ERR_INVALID, "more lights than CTL_MAX_NUM_LIGHTS");
            for (uint32_t k = 0; ok && k < S.num_lights; k++) ok = K.light(S.light_indices[k]);
        }
        // the distinct (index, ...) keys of a batch are few: remember what passed
        std::vector<uint8_t> mat_ok(K.mats.size(), 0), light_ok(K.lights.size(), 0);
        for (uint32_t i = 0; ok && i < n; i++) {
            const float* a = queries + (size_t)i * query_stride;
            switch (what) {
            case kEvalBsdfSample: case kEvalBsdfEval: case kEvalBsdfSampleEval: case kEvalNormalMap: {
                const uint32_t mi = eval_word(a[0]);
                if (mi < mat_ok.size() && mat_ok[mi]) break;
                ok = K.material(mi, false);
                if (ok && what == kEvalNormalMap) {
                    const ctl_material& M = K.mats[mi];
                    if (M.map_kind > CTL_MAP_HEIGHT) ok = K.refuse(CTL_ERR_INVALID, "unknown surface map kind");
                    else if (M.map_kind != CTL_MAP_NONE) ok = K.texture(M.map_tex);
                }
                if (ok) mat_ok[mi] = 1;
                break; }
            case kEvalLightSample: case kEvalLightPdf: case kEvalLightEval: {
                const uint32_t li = eval_word(a[0]);
                if (li < light_ok.size() && light_ok[li]) break;
                ok = K.light(li); if (ok) light_ok[li] = 1;
                break; }
            case kEvalTexture: {
                const uint32_t kind = eval_word(a[0]), idx = eval_word(a[1]);
                if (kind > 6) { ok = K.refuse(CTL_ERR_INVALID, "unknown texture slot"); break; }
                if (kind == 6) { if (idx >= K.lights.size()) ok = K.refuse(CTL_ERR_INVALID, "light index out of range"); else ok = K.texture(K.lights[idx].rad_texture); break; }
                if (idx >= K.mats.size()) { ok = K.refuse(CTL_ERR_INVALID, "material index out of range"); break; }
                ok = K.texture(kind == 5 ? K.mats[idx].alpha_tex : (kind == 4 ? K.mats[idx].map_tex : K.mats[idx].tex[kind]));
                break; }
            case kEvalAlphaTest: {
                const uint32_t mi = eval_word(a[0]);
                if (mi >= K.mats.size()) { ok = K.refuse(CTL_ERR_INVALID, "material index " + std::to_string(mi) + " of " + std::to_string(K.mats.size())); break; }
                const ctl_material& M = K.mats[mi];
                if (M.alpha_state > CTL_ALPHA_REFLECTANCE_COLOR || M.alpha_state == 4) { ok = K.refuse(CTL_ERR_INVALID, "unknown alpha blend state"); break; }
                if (M.alpha_state != CTL_ALPHA_DISABLED) ok = K.texture((M.alpha_state & 4) ? M.tex[0] : M.alpha_tex, true);
                // the device function takes its uv from a triangle's half-precision vertex coordinates: only such a uv can be asked
                if (ok && !(half_to_float(float_to_half(a[1])) == a[1] && half_to_float(float_to_half(a[2])) == a[2])) ok = K.refuse(CTL_ERR_INVALID, "the uv of an alpha-test query must be representable in half precision");
                break; }
            case kEvalMip: {
                const uint32_t im = eval_word(a[0]);
                if (im >= K.n_images) ok = K.refuse(CTL_ERR_INVALID, "image index " + std::to_string(im) + " of " + std::to_string(K.n_images));
                break; }
            default: break;
            }
        }
        if (!ok) return fail(K.code, K.why);
        dbuf<ctl_material> dmats; dbuf<float> dq, dout; dbuf<uint4> dtri, dnode;
        if (what == kEvalAlphaTest && n) {   // one synthetic triangle and node per query: node_info[i].x = the material, the three vertices at the query's uv (u in the HIGH half of a word, as getUVSetData reads it)
            std::vector<uint4> tri((size_t)n * 2), node(n);
            for (uint32_t i = 0; i < n; i++) {
                const float* a = queries + (size_t)i * query_stride;
                const uint32_t w = ((uint32_t)float_to_half(a[1]) << 16) | float_to_half(a[2]);
                tri[2 * (size_t)i] = make_uint4(0, 0, 0, 0); tri[2 * (size_t)i + 1] = make_uint4(0, w, w, w); node[i] = make_uint4(eval_word(a[0]), 0, 0, 0);
            }
            dtri.alloc(tri.size()); dnode.alloc(node.size());
            CTL_HIP(hipMemcpy(dtri.p, tri.data(), tri.size() * sizeof(uint4), hipMemcpyHostToDevice)); CTL_HIP(hipMemcpy(dnode.p, node.data(), node.size() * sizeof(uint4), hipMemcpyHostToDevice));
            S.tri_data = dtri.p; S.node_info = dnode.p;
        }
        if (materials) { dmats.alloc(n_materials); CTL_HIP(hipMemcpy(dmats.p, materials, sizeof(ctl_material) * n_materials, hipMemcpyHostToDevice)); S.mats = dmats.p; S.rt_reduced = nullptr; }
        if (n) {
            dq.alloc((size_t)n * query_stride); dout.alloc((size_t)n * out_stride);
            CTL_HIP(hipMemcpy(dq.p, queries, (size_t)n * query_stride * 4, hipMemcpyHostToDevice));
            CTL_HIP(hipMemset(dout.p, 0, (size_t)n * out_stride * 4));
            const bool launched = build == 0 ? launch_shading_eval_basic(S, what, n, dq.p, query_stride, dout.p, out_stride)
                                : build == 1 ? launch_shading_eval_full(S, what, n, dq.p, query_stride, dout.p, out_stride)
                                             : launch_shading_eval_partials(S, what, n, dq.p, query_stride, dout.p, out_stride);
            if (!launched) throw unsupported_error("ctl_shading_eval: this build does not carry the function");
            CTL_HIP(hipGetLastError());
            CTL_HIP(hipMemcpy(out, dout.p, (size_t)n * out_stride * 4, hipMemcpyDeviceToHost));
        }
    CTL_CATCH
}
int ctl_traversal_stack_histogram(uint64_t* out, uint32_t n_bins, int reset) {
    CTL_REQUIRE(out && n_bins >= 1, "null argument");
    CTL_TRY
        require_device();
        unsigned long long h[kStackSize];
        read_stack_histogram(h, reset != 0);
        for (uint32_t i = 0; i < n_bins; i++) out[i] = 0;
        for (int i = 0; i < kStackSize; i++) out[(uint32_t)i < n_bins ? (uint32_t)i : n_bins - 1] += h[i];
    CTL_CATCH
}
// ---- scene
int ctl_scene_create(const ctl_scene_desc* desc, ctl_scene** out) { CTL_REQUIRE(desc && out, "null argument"); CTL_TRY *out = new ctl_scene(*desc, false); CTL_CATCH }
int ctl_scene_create_ex(const ctl_scene_desc* desc, uint32_t flags, ctl_scene** out) { CTL_REQUIRE(desc && out, "null argument"); CTL_TRY
    const uint32_t fmt = (flags >> 8) & 7u;   // 0: default, else CTL_FLAT_* + 1
    *out = new ctl_scene(*desc, (flags & CTL_SCENE_FLATTEN) != 0, (int)fmt - 1, (flags & CTL_SCENE_REDUCED_ROUGH_TRANSMITTANCE) != 0);
CTL_CATCH }
void ctl_scene_destroy(ctl_scene* s) { delete s; }
// ---- in-place updates (scene_update.hip)
int ctl_scene_desc_diff(const ctl_scene_desc* a, const ctl_scene_desc* b, uint32_t* mask_out) { CTL_REQUIRE(a && b && mask_out, "null argument"); CTL_TRY *mask_out = scene_desc_diff(*a, *b); CTL_CATCH }
int ctl_scene_desc_check(const ctl_scene_desc* desc, uint32_t parts, uint32_t state_out[3]) {
    CTL_REQUIRE(desc, "null argument");
    CTL_REQUIRE(!(parts & ~kCheckAllParts), "ctl_scene_desc_check: unknown CTL_DIFF_* bits");
    CTL_TRY
        if (!parts) parts = kCheckAllParts;
        check_scene_desc(*desc, parts, (parts & CTL_DIFF_TOPOLOGY) ? "ctl_scene_create" : "ctl_scene_update");
        if (state_out) { const shading_state s = derive_shading_state(*desc); state_out[0] = s.features; state_out[1] = s.models; state_out[2] = s.alpha_maps; }
    CTL_CATCH
}
int ctl_scene_update(ctl_scene* scene, const ctl_scene_desc* new_desc, uint32_t* mask_out) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, "no HIP device: the MI355X path tracer has no CPU fallback");
    CTL_REQUIRE(scene && new_desc, "null argument");
    const int rc = [&]() -> int { CTL_TRY scene->s.update(*new_desc, nullptr); CTL_CATCH }();
    if (mask_out) *mask_out = scene->s.last_mask();   // also when the update is refused: the caller sees why
    if (rc == CTL_OK) { scene->n_materials = new_desc->n_materials; scene->n_images = new_desc->n_images; scene->basis.fill(*new_desc); }
    return rc;
}
int ctl_scene_get_update_stats(ctl_scene* scene, ctl_scene_update_stats* out) { CTL_REQUIRE(scene && out, "null argument"); *out = scene->s.last_update(); return CTL_OK; }
// ---- skinned meshes (mesh_skin.hip)
static const char* kNoDevice = "no HIP device: the MI355X path tracer has no CPU fallback";
int ctl_scene_bind_skin(ctl_scene* scene, uint32_t mesh_index, const float* rest_positions, const float* rest_normals, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                        const uint8_t* bone_indices, const uint8_t* bone_weights, uint32_t n_bones) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene, "null scene");
    CTL_TRY scene->s.bind_skin(mesh_index, rest_positions, rest_normals, n_vert, indices, n_tri, bone_indices, bone_weights, n_bones); CTL_CATCH
}
int ctl_scene_bind_skin_ex(ctl_scene* scene, uint32_t mesh_index, const float* rest_positions, const float* rest_normals, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                           const uint8_t* bone_indices, const uint8_t* bone_weights, uint32_t n_bones, uint32_t flags) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene, "null scene");
    CTL_REQUIRE(!(flags & ~(uint32_t)CTL_SKIN_AREA_LIGHTS), "ctl_scene_bind_skin_ex: unknown CTL_SKIN_* bits");
    CTL_TRY scene->s.bind_skin(mesh_index, rest_positions, rest_normals, n_vert, indices, n_tri, bone_indices, bone_weights, n_bones, flags); CTL_CATCH
}
int ctl_scene_animate_mesh(ctl_scene* scene, uint32_t mesh_index, const ctl_float4x4* bones0, const ctl_float4x4* bones1, float lerp, ctl_scene_update_stats* stats_out) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene && bones0, "null argument");
    CTL_TRY scene->s.animate_mesh(mesh_index, bones0, bones1, lerp, stats_out); CTL_CATCH
}
int ctl_scene_get_skin_ms(ctl_scene* scene, float* ms_out) { CTL_REQUIRE(scene && ms_out, "null argument"); *ms_out = scene->s.last_skin_ms(); return CTL_OK; }
int ctl_scene_get_shape_set_ms(ctl_scene* scene, float* ms_out) { CTL_REQUIRE(scene && ms_out, "null argument"); *ms_out = scene->s.last_shape_set_ms(); return CTL_OK; }
int ctl_scene_read_lights(ctl_scene* scene, ctl_light* lights_out, uint32_t n_lights, uint8_t* anim_out, size_t n_anim_bytes) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene, "null scene");
    CTL_TRY scene->s.read_lights(lights_out, n_lights, anim_out, n_anim_bytes); CTL_CATCH
}
// ---- images in place (scene_images.hip)
int ctl_scene_update_image(ctl_scene* scene, uint32_t image_index, const uint32_t* texels, uint32_t width, uint32_t height, uint32_t flags, ctl_scene_image_stats* stats_out) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene, "null scene");
    CTL_TRY scene->s.update_image(image_index, texels, width, height, flags, stats_out); CTL_CATCH
}
int ctl_scene_read_image(ctl_scene* scene, uint32_t image_index, uint32_t* texels_out, size_t capacity, uint32_t* levels_out, uint32_t level_offsets_out[15]) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene, "null scene");
    CTL_TRY scene->s.read_image(image_index, texels_out, capacity, levels_out, level_offsets_out); CTL_CATCH
}
// ---- another set of images (scene_image_set.hip, scene_image_set.cpp)
int ctl_builder_image_count(const ctl_builder* b, uint32_t* count_out) { CTL_REQUIRE(b && count_out, "null argument"); *count_out = (uint32_t)b->b.images.size(); return CTL_OK; }
int ctl_builder_remove_image(ctl_builder* b, uint32_t image_index) { CTL_REQUIRE(b, "null argument"); CTL_TRY b->b.remove_image(image_index); CTL_CATCH }
int ctl_builder_replace_image(ctl_builder* b, uint32_t image_index, const uint32_t* texels, uint32_t width, uint32_t height) {
    CTL_REQUIRE(b, "null argument");
    CTL_TRY b->b.replace_image(image_index, texels, width, height); CTL_CATCH
}
int ctl_builder_get_material(const ctl_builder* b, uint32_t absolute_index, ctl_material* out) { CTL_REQUIRE(b && out, "null argument"); CTL_TRY *out = b->b.material(absolute_index); CTL_CATCH }
int ctl_builder_set_material(ctl_builder* b, uint32_t absolute_index, const ctl_material* material) { CTL_REQUIRE(b && material, "null argument"); CTL_TRY b->b.set_material(absolute_index, *material); CTL_CATCH }
int ctl_scene_update_image_set(ctl_scene* scene, const ctl_scene_desc* new_desc, const uint32_t* old_image_of_new, uint32_t n_new_images, ctl_scene_image_set_stats* stats_out) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene && new_desc, "null argument");
    CTL_REQUIRE(old_image_of_new || !n_new_images, "ctl_scene_update_image_set: null image map");
    const int rc = [&]() -> int { CTL_TRY flat_rebuilder::update_image_set(scene->s, *new_desc, old_image_of_new, n_new_images, scene->basis, stats_out); CTL_CATCH }();
    if (rc == CTL_OK) { scene->n_materials = new_desc->n_materials; scene->n_images = new_desc->n_images; scene->basis.fill(*new_desc); }
    return rc;
}
static_assert(sizeof(image_run) == 4 * sizeof(uint64_t), "a run is four words of the table ctl_image_set_plan_host hands out");
int ctl_image_set_plan_host(const ctl_scene_desc* old_desc, const ctl_scene_desc* new_desc, const uint32_t* old_image_of_new, uint32_t n_new_images,
                            uint64_t* offsets_out, uint64_t* total_out, uint64_t* run_table_out, uint32_t* n_runs_out) {
    CTL_REQUIRE(old_desc && new_desc, "null argument");
    CTL_TRY
        node_set_basis basis; basis.fill(*old_desc);
        geometry_hashes held; hash_geometry(*old_desc, held);
        image_set_plan plan; plan_image_set(basis, held, *new_desc, old_image_of_new, n_new_images, nullptr, plan, "ctl_image_set_plan_host");
        if (offsets_out && !plan.offsets.empty()) std::memcpy(offsets_out, plan.offsets.data(), plan.offsets.size() * 8);
        if (total_out) *total_out = plan.total;
        if (run_table_out) std::memcpy(run_table_out, plan.runs.data(), plan.runs.size() * sizeof(image_run));
        if (n_runs_out) *n_runs_out = plan.n_runs();
    CTL_CATCH
}
int ctl_move_texels_host(const uint32_t* old_pool, uint64_t n_old_texels, const uint64_t* run_table, uint32_t n_runs, uint32_t* new_pool, uint64_t n_new_texels) {
    CTL_REQUIRE(run_table && (old_pool || !n_old_texels) && (new_pool || !n_new_texels), "null argument");
    CTL_TRY move_texels_host(old_pool, n_old_texels, reinterpret_cast<const image_run*>(run_table), n_runs, new_pool, n_new_texels); CTL_CATCH
}
int ctl_shape_sets_host(const ctl_scene_desc* desc, uint32_t mesh_index, const ctl_triangle_data* tri_data, const ctl_woop_tri* woop, ctl_light* lights_out, uint8_t* anim_out) {
    CTL_REQUIRE(desc, "null description");
    CTL_TRY shape_sets_host(*desc, mesh_index, tri_data, woop, lights_out, anim_out); CTL_CATCH
}
int ctl_scene_read_mesh_geometry(ctl_scene* scene, uint32_t mesh_index, float* positions_out, float* normals_out, ctl_triangle_data* tri_data_out, ctl_woop_tri* woop_out) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene, "null scene");
    CTL_TRY scene->s.read_mesh_geometry(mesh_index, positions_out, normals_out, tri_data_out, woop_out); CTL_CATCH
}
int ctl_scene_unbind_skin(ctl_scene* scene, uint32_t mesh_index) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene, "null scene");
    CTL_TRY scene->s.unbind_skin(mesh_index); CTL_CATCH
}
int ctl_skin_mesh_host(const ctl_scene_desc* desc, uint32_t mesh_index, const float* rest_positions, const float* rest_normals, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                       const uint8_t* bone_indices, const uint8_t* bone_weights, uint32_t n_bones, const ctl_float4x4* bones0, const ctl_float4x4* bones1, float lerp,
                       float* positions_out, float* normals_out, ctl_triangle_data* tri_data_out, ctl_woop_tri* woop_out) {
    CTL_REQUIRE(desc, "null description");
    CTL_TRY skin_mesh_host(*desc, mesh_index, rest_positions, rest_normals, n_vert, indices, n_tri, bone_indices, bone_weights, n_bones, bones0, bones1, lerp, positions_out, normals_out, tri_data_out, woop_out); CTL_CATCH
}
// a triangle an added node got no entry for (ctl_flat_bvh_update_nodes) and that a changed mesh of `d` makes regular: refused as the device refuses it
static void refuse_gained_triangles(const ctl_flat_bvh& h, const ctl_scene_desc& d, const char* who) {
    if (h.extra_missing.empty() || h.f.refit.geom.empty()) return;
    geometry_hashes g; hash_geometry(d, g);
    if (!g.same_structure(h.f.refit.geom)) return;   // (the refit refuses it)
    std::vector<uint8_t> changed(d.n_meshes, 0);
    for (uint32_t m = 0; m < d.n_meshes; m++) changed[m] = g.same_values(h.f.refit.geom, m) ? 0 : 1;
    std::vector<uint32_t> rows; triangle_woop_rows(d, rows);
    const int m = mesh_gaining_a_triangle(d, h.extra_missing, rows, changed);
    if (m >= 0) throw std::runtime_error(std::string(who) + ": mesh " + std::to_string(m) + " has a triangle that was degenerate when a node was added and no longer is: the tree has no leaf entry for it");
}
int ctl_flat_bvh_refit(ctl_flat_bvh* h, const ctl_scene_desc* new_desc) { CTL_REQUIRE(h && new_desc, "null argument"); CTL_TRY refuse_gained_triangles(*h, *new_desc, "refit"); refit_flat_scene(h->f, *new_desc, nullptr); h->basis.fill(*new_desc); CTL_CATCH }
// ---- rebuild of the flattened tree (flat_rebuild.hip, flat_rebuild.cpp)
static bool known_builder(int b) { return b == CTL_REBUILD_LBVH || b == CTL_REBUILD_PLOC; }
int ctl_scene_rebuild_flat_ex(ctl_scene* scene, int builder, ctl_scene_rebuild_stats* stats_out) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene, "null scene");
    CTL_REQUIRE(known_builder(builder), "ctl_scene_rebuild_flat_ex: unknown builder");
    CTL_TRY rebuild_builder_scope use(builder); scene->s.rebuild_flat(stats_out); CTL_CATCH
}
int ctl_scene_rebuild_flat(ctl_scene* scene, ctl_scene_rebuild_stats* stats_out) { return ctl_scene_rebuild_flat_ex(scene, CTL_REBUILD_LBVH, stats_out); }
int ctl_flat_bvh_rebuild_ex(ctl_flat_bvh* h, const ctl_scene_desc* new_desc, int builder) {
    CTL_REQUIRE(h && new_desc, "null argument");
    CTL_REQUIRE(known_builder(builder), "ctl_flat_bvh_rebuild_ex: unknown builder");
    CTL_TRY refuse_gained_triangles(*h, *new_desc, "rebuild"); rebuild_flat_scene(h->f, *new_desc, nullptr, builder); h->basis.fill(*new_desc); CTL_CATCH
}
int ctl_flat_bvh_rebuild(ctl_flat_bvh* h, const ctl_scene_desc* new_desc) { return ctl_flat_bvh_rebuild_ex(h, new_desc, CTL_REBUILD_LBVH); }
uint32_t ctl_rebuild_last_rounds(void) { return rebuild_last_rounds(); }
int ctl_flat_bvh_rebuild_order(const ctl_flat_bvh* h, const ctl_scene_desc* desc, uint32_t* sorted_entry, float* entry_boxes, float* bounds) {
    CTL_REQUIRE(h && desc && sorted_entry && entry_boxes && bounds, "null argument");
    CTL_TRY
    refuse_gained_triangles(*h, *desc, "ctl_flat_bvh_rebuild_order");
    rebuild_refuse(h->f.format, h->f.refit.ready() && h->f.refit.part_index.size() == h->f.leaves.size(), h->f.compact_links, h->f.leaves.size(), "ctl_flat_bvh_rebuild_order");
    if (desc->n_nodes != h->f.refit.xf0.size() || !desc->node_transforms) throw std::runtime_error("ctl_flat_bvh_rebuild_order: the description has another number of nodes than the tree was built from");
    std::vector<refit_box> ebox; refit_box B; std::vector<std::pair<uint64_t, uint32_t>> order;
    rebuild_sorted_entries(h->f, *desc, ebox, B, order);
    for (size_t i = 0; i < order.size(); i++) { sorted_entry[i] = order[i].second; std::memcpy(entry_boxes + 6 * i, &ebox[i], 24); }
    std::memcpy(bounds, &B, 24);
    CTL_CATCH
}
// ---- another set of nodes (flat_nodes.hip, flat_nodes.cpp)
int ctl_scene_update_nodes_ex(ctl_scene* scene, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes, int builder, ctl_scene_nodes_stats* stats_out) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene && new_desc, "null argument");
    CTL_REQUIRE(old_of_new, "ctl_scene_update_nodes: null node map");
    CTL_REQUIRE(known_builder(builder), "ctl_scene_update_nodes_ex: unknown builder");
    const int rc = [&]() -> int { CTL_TRY rebuild_builder_scope use(builder); scene->s.update_nodes(*new_desc, old_of_new, n_new_nodes, scene->basis, stats_out); CTL_CATCH }();
    if (rc == CTL_OK) { scene->n_materials = new_desc->n_materials; scene->n_images = new_desc->n_images; scene->basis.fill(*new_desc); }
    return rc;
}
int ctl_scene_update_nodes(ctl_scene* scene, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes, ctl_scene_nodes_stats* stats_out) {
    return ctl_scene_update_nodes_ex(scene, new_desc, old_of_new, n_new_nodes, CTL_REBUILD_LBVH, stats_out);
}
int ctl_flat_bvh_update_nodes_ex(ctl_flat_bvh* h, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes, int builder) {
    CTL_REQUIRE(h && new_desc, "null argument");
    CTL_REQUIRE(known_builder(builder), "ctl_flat_bvh_update_nodes_ex: unknown builder");
    CTL_TRY update_nodes_flat_scene(h->f, h->basis, *new_desc, old_of_new, n_new_nodes, h->extra_missing, builder); h->basis.fill(*new_desc); CTL_CATCH
}
int ctl_flat_bvh_update_nodes(ctl_flat_bvh* h, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes) {
    return ctl_flat_bvh_update_nodes_ex(h, new_desc, old_of_new, n_new_nodes, CTL_REBUILD_LBVH);
}
// ---- new meshes (flat_meshes.hip, flat_meshes.cpp)
int ctl_scene_update_meshes_ex(ctl_scene* scene, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes, int builder, ctl_scene_meshes_stats* stats_out) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene && new_desc, "null argument");
    CTL_REQUIRE(old_of_new, "ctl_scene_update_meshes: null node map");
    CTL_REQUIRE(known_builder(builder), "ctl_scene_update_meshes_ex: unknown builder");
    const int rc = [&]() -> int { CTL_TRY rebuild_builder_scope use(builder); flat_rebuilder::update_meshes(scene->s, *new_desc, old_of_new, n_new_nodes, scene->basis, stats_out); CTL_CATCH }();
    if (rc == CTL_OK) { scene->n_materials = new_desc->n_materials; scene->n_images = new_desc->n_images; scene->basis.fill(*new_desc); }
    return rc;
}
int ctl_scene_update_meshes(ctl_scene* scene, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes, ctl_scene_meshes_stats* stats_out) {
    return ctl_scene_update_meshes_ex(scene, new_desc, old_of_new, n_new_nodes, CTL_REBUILD_LBVH, stats_out);
}
int ctl_flat_bvh_update_meshes_ex(ctl_flat_bvh* h, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes, int builder) {
    CTL_REQUIRE(h && new_desc, "null argument");
    CTL_REQUIRE(known_builder(builder), "ctl_flat_bvh_update_meshes_ex: unknown builder");
    CTL_TRY update_meshes_flat_scene(h->f, h->basis, *new_desc, old_of_new, n_new_nodes, h->extra_missing, builder); h->basis.fill(*new_desc); CTL_CATCH
}
int ctl_flat_bvh_update_meshes(ctl_flat_bvh* h, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes) {
    return ctl_flat_bvh_update_meshes_ex(h, new_desc, old_of_new, n_new_nodes, CTL_REBUILD_LBVH);
}
int ctl_scene_read_triangle_rows(ctl_scene* scene, uint32_t* rows_out, size_t capacity, size_t* count_out) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene && count_out, "null argument");
    CTL_TRY *count_out = flat_rebuilder::read_tri_rows(scene->s, rows_out, capacity); CTL_CATCH
}
int ctl_triangle_woop_rows(const ctl_scene_desc* desc, uint32_t* rows_out) {
    CTL_REQUIRE(desc && rows_out, "null argument");
    CTL_TRY std::vector<uint32_t> rows; triangle_woop_rows(*desc, rows); if (!rows.empty()) std::memcpy(rows_out, rows.data(), rows.size() * 4); CTL_CATCH
}
int ctl_append_leaf_rows_host(const ctl_scene_desc* new_desc, uint32_t old_n_meshes, uint32_t old_n_tri_data, uint32_t old_n_woop, uint32_t old_n_bvh_nodes, uint32_t* tri_row, uint32_t* leaf_rows_out) {
    CTL_REQUIRE(new_desc && tri_row, "null argument");
    CTL_TRY mesh_set_plan P; plan_mesh_growth(old_n_meshes, old_n_tri_data, old_n_woop, old_n_bvh_nodes, *new_desc, "ctl_append_leaf_rows_host: ", P); append_leaf_rows_host(*new_desc, P, leaf_rows_out, tri_row); CTL_CATCH
}
// ---- removed meshes (flat_mesh_set.hip, flat_mesh_set.cpp)
int ctl_builder_mesh_count(const ctl_builder* b, uint32_t* count_out) { CTL_REQUIRE(b && count_out, "null argument"); *count_out = (uint32_t)b->b.meshes.size(); return CTL_OK; }
int ctl_builder_remove_mesh(ctl_builder* b, uint32_t mesh_index) { CTL_REQUIRE(b, "null argument"); CTL_TRY b->b.remove_mesh(mesh_index); CTL_CATCH }
int ctl_scene_update_mesh_set(ctl_scene* scene, const ctl_scene_desc* new_desc, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes, const uint32_t* old_of_new, uint32_t n_new_nodes,
                              int builder, ctl_scene_mesh_set_stats* stats_out) {
    if (device_count() <= 0) return fail(CTL_ERR_NO_DEVICE, kNoDevice);
    CTL_REQUIRE(scene && new_desc, "null argument");
    CTL_REQUIRE(old_of_new, "ctl_scene_update_mesh_set: null node map");
    CTL_REQUIRE(old_mesh_of_new || !n_new_meshes, "ctl_scene_update_mesh_set: null mesh map");
    CTL_REQUIRE(known_builder(builder), "ctl_scene_update_mesh_set: unknown builder");
    const int rc = [&]() -> int { CTL_TRY rebuild_builder_scope use(builder); flat_rebuilder::update_mesh_set(scene->s, *new_desc, old_mesh_of_new, n_new_meshes, old_of_new, n_new_nodes, scene->basis, stats_out); CTL_CATCH }();
    if (rc == CTL_OK) { scene->n_materials = new_desc->n_materials; scene->n_images = new_desc->n_images; scene->basis.fill(*new_desc); }
    return rc;
}
int ctl_flat_bvh_update_mesh_set(ctl_flat_bvh* h, const ctl_scene_desc* new_desc, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes, const uint32_t* old_of_new, uint32_t n_new_nodes, int builder) {
    CTL_REQUIRE(h && new_desc, "null argument");
    CTL_REQUIRE(known_builder(builder), "ctl_flat_bvh_update_mesh_set: unknown builder");
    CTL_TRY update_mesh_set_flat_scene(h->f, h->basis, *new_desc, old_mesh_of_new, n_new_meshes, old_of_new, n_new_nodes, h->extra_missing, builder); h->basis.fill(*new_desc); CTL_CATCH
}
int ctl_compact_tri_rows_host(const ctl_scene_desc* old_desc, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes, const uint32_t* held_rows, uint32_t* rows_out, uint32_t* count_out) {
    CTL_REQUIRE(old_desc && held_rows && rows_out && count_out, "null argument");
    CTL_TRY node_set_basis basis; basis.fill(*old_desc); mesh_compaction cut; plan_mesh_compaction(basis, old_mesh_of_new, n_new_meshes, "ctl_compact_tri_rows_host: ", cut);
    if (cut.removes()) compact_tri_rows_host(cut, held_rows, old_desc->n_tri_data, rows_out); else if (old_desc->n_tri_data) std::memcpy(rows_out, held_rows, (size_t)old_desc->n_tri_data * 4);
    *count_out = cut.kept_tris; CTL_CATCH
}
int ctl_flat_bvh_levels(const ctl_flat_bvh* h, const uint32_t** level_start, uint32_t* n_levels, const uint32_t** level_nodes, uint64_t* n_level_nodes) {
    CTL_REQUIRE(h && level_start && n_levels && level_nodes && n_level_nodes, "null argument");
    const auto& R = h->f.refit;
    *level_start = R.level_start.data(); *n_levels = R.level_start.empty() ? 0u : (uint32_t)R.level_start.size() - 1u;
    *level_nodes = R.level_nodes.data(); *n_level_nodes = R.level_nodes.size();
    return CTL_OK;
}
int ctl_scene_read_flat_bvh(ctl_scene* scene, ctl_flat_bvh** out) {
    CTL_REQUIRE(scene && out, "null argument");
    CTL_TRY std::unique_ptr<ctl_flat_bvh> h(new ctl_flat_bvh()); scene->s.read_flat_bvh(h->f); h->basis = scene->basis; *out = h.release(); CTL_CATCH
}
int ctl_set_cache_dir(const char* dir) { CTL_TRY set_cache_dir(dir); CTL_CATCH }
// the node formats 1 and 2 (F4 / F2) lost to Q4 and are retired; a format above CTL_FLAT_Q8 never existed
#define CTL_REFUSE_RETIRED_FORMAT(format) if ((format) == 1u || (format) == 2u) return fail(CTL_ERR_UNSUPPORTED, "flat node formats 1 and 2 (F4 / F2) are retired: no kernel reads them (EXPERIMENTS.md has the measurements and where the builder code is in git)")
int ctl_flatten_probe(const ctl_scene_desc* desc, uint32_t format, uint64_t* out4) {
    CTL_REQUIRE(desc && out4 && format <= CTL_FLAT_Q8, "null argument or bad format");
    CTL_REFUSE_RETIRED_FORMAT(format);
    CTL_TRY
        flat_scene F;
        if (!flatten_scene(*desc, F, (size_t)1 << 30, (int)format)) throw std::runtime_error("ctl_flatten_probe: nothing to flatten");
        content_hash H; H.add_vector(F.nodes); H.add_vector(F.child_links); H.add_vector(F.leaves); if (!F.nodes_q8.empty()) H.add_vector(F.nodes_q8);
        out4[0] = F.nodes.size() + F.nodes_q8.size(); out4[1] = F.leaves.size(); out4[2] = (uint64_t)F.max_depth;
        out4[3] = std::strtoull(H.hex().substr(16).c_str(), nullptr, 16);
    CTL_CATCH
}
int ctl_flat_bvh_build(const ctl_scene_desc* desc, uint32_t format, ctl_flat_bvh** out) {
    CTL_REQUIRE(desc && out && format <= CTL_FLAT_Q8, "null argument or bad format");
    CTL_REFUSE_RETIRED_FORMAT(format);
    CTL_TRY
        std::unique_ptr<ctl_flat_bvh> h(new ctl_flat_bvh());
        if (!flatten_scene(*desc, h->f, (size_t)1 << 30, (int)format)) throw std::runtime_error("ctl_flat_bvh_build: nothing to flatten");
        if (h->f.format == kFlatQ4 && h->f.refit.ready()) hash_geometry(*desc, h->f.refit.geom);   // what ctl_flat_bvh_refit tells deformed meshes by
        h->basis.fill(*desc);
        *out = h.release();
    CTL_CATCH
}
int ctl_flat_bvh_arrays(const ctl_flat_bvh* h, ctl_flat_bvh_desc* out) {
    CTL_REQUIRE(h && out, "null argument");
    const flat_scene& F = h->f;
    out->format = (uint32_t)F.format; out->max_depth = (uint32_t)F.max_depth;
    if (F.format == kFlatQ4) { out->nodes = F.nodes.data(); out->n_nodes = F.nodes.size(); out->node_bytes = 64; }
    else { out->nodes = F.nodes_q8.data(); out->n_nodes = F.nodes_q8.size(); out->node_bytes = 128; }
    out->leaves = F.leaves.data(); out->n_leaves = F.leaves.size();
    out->child_links = F.child_links.data(); out->compact = (F.compact_links || F.format == kFlatQ8) ? 1u : 0u;
    out->root_slab = F.root_slab ? 1u : 0u; out->n_slab_nodes = F.slab_nodes;
    const bool side = F.format == kFlatQ4 && F.refit.part_index.size() == F.leaves.size();
    out->part_index = side ? F.refit.part_index.data() : nullptr; out->n_part_boxes = side ? F.refit.part_boxes.size() : 0;
    out->part_boxes = (side && !F.refit.part_boxes.empty()) ? F.refit.part_boxes[0].lo : nullptr;
    return CTL_OK;
}
void ctl_flat_bvh_destroy(ctl_flat_bvh* h) { delete h; }
int ctl_parse_mitsuba_scene(ctl_builder* b, const char* xml_path, int32_t* width_inout, int32_t* height_inout) {
    CTL_REQUIRE(b && xml_path, "null argument");
    CTL_TRY parse_mitsuba_scene(b->b, xml_path, width_inout, height_inout); CTL_CATCH
}
int ctl_parse_mitsuba_scene_ex(ctl_builder* b, const char* xml_path, int32_t* width_inout, int32_t* height_inout, uint32_t flags) {
    CTL_REQUIRE(b && xml_path, "null argument");
    CTL_TRY parse_mitsuba_scene(b->b, xml_path, width_inout, height_inout, flags); CTL_CATCH
}
int ctl_decode_image_file(const char* path, uint32_t* width, uint32_t* height, int32_t* is_float, float* rgb, uint8_t* rgba8) {
    CTL_REQUIRE(path && width && height && is_float, "null argument");
    CTL_TRY
        const decoded_image img = load_image_file(path);
        *width = img.width; *height = img.height; *is_float = img.is_float ? 1 : 0;
        if (img.is_float && rgb) std::memcpy(rgb, img.rgb.data(), img.rgb.size() * sizeof(float));
        if (!img.is_float && rgba8) std::memcpy(rgba8, img.rgba8.data(), img.rgba8.size());
    CTL_CATCH
}

// ---- sampler
int ctl_sequence_generator_create(ctl_sequence_generator** out) { CTL_REQUIRE(out, "null out"); CTL_TRY *out = new ctl_sequence_generator(); CTL_CATCH }
void ctl_sequence_generator_destroy(ctl_sequence_generator* g) { delete g; }
int ctl_sequence_generator_compute(ctl_sequence_generator* g, float* tables_1d, float* tables_2d) { CTL_REQUIRE(g && tables_1d && tables_2d, "null argument"); CTL_TRY g->g.compute(tables_1d, tables_2d); CTL_CATCH }

int ctl_sequence_generator_compute_many(ctl_sequence_generator* g, uint32_t n_passes, float* tables_1d, float* tables_2d, uint32_t threads) {
    CTL_REQUIRE(g && tables_1d && tables_2d, "null argument");
    const size_t n1 = (size_t)CTL_SAMPLER_NUM_SEQUENCES * CTL_SAMPLER_SEQUENCE_LENGTH;
    CTL_TRY g->g.compute_many(tables_1d, tables_2d, n_passes, n1, 2 * n1, threads); CTL_CATCH
}
int ctl_sequence_generator_compute_many_device(ctl_sequence_generator* g, uint32_t n_passes, float* tables_1d, float* tables_2d) {
    CTL_REQUIRE(g && tables_1d && tables_2d, "null argument");
    const size_t n1 = (size_t)CTL_SAMPLER_NUM_SEQUENCES * CTL_SAMPLER_SEQUENCE_LENGTH;
    CTL_TRY
        require_device();
        if (n_passes == 0) return CTL_OK;
        std::vector<sequence_generator::pass_start> starts(n_passes);
        g->g.take_pass_starts(n_passes, starts.data());
        const std::vector<uint32_t>& J = sequence_generator::chunk_jump_matrices();
        dbuf<uint32_t> dj, ds; dbuf<float> d1, d2;
        dj.alloc(J.size()); ds.alloc(starts.size() * sizeof(sequence_generator::pass_start) / 4); d1.alloc(n1 * n_passes); d2.alloc(2 * n1 * n_passes);
        CTL_HIP(hipMemcpy(dj.p, J.data(), J.size() * 4, hipMemcpyHostToDevice));
        CTL_HIP(hipMemcpy(ds.p, starts.data(), starts.size() * sizeof(sequence_generator::pass_start), hipMemcpyHostToDevice));
        launch_sequence_fill(nullptr, dj.p, ds.p, n_passes, d1.p, d2.p);
        CTL_HIP(hipDeviceSynchronize());
        CTL_HIP(hipMemcpy(tables_1d, d1.p, n1 * n_passes * 4, hipMemcpyDeviceToHost));
        CTL_HIP(hipMemcpy(tables_2d, d2.p, 2 * n1 * n_passes * 4, hipMemcpyDeviceToHost));
    CTL_CATCH
}

// ---- image
int ctl_image_create(uint32_t width, uint32_t height, ctl_image** out) { CTL_REQUIRE(out && width && height, "bad argument"); CTL_TRY *out = new ctl_image(width, height); CTL_CATCH }
void ctl_image_destroy(ctl_image* img) { delete img; }
int ctl_image_clear(ctl_image* img) { CTL_REQUIRE(img, "null image"); CTL_TRY img->img.Clear(); CTL_CATCH }
int ctl_image_read_pixels(ctl_image* img, ctl_pixel_data* host_out) { CTL_REQUIRE(img && host_out, "null argument"); CTL_TRY img->img.read(host_out); CTL_CATCH }
int ctl_image_write_pixels(ctl_image* img, const ctl_pixel_data* host_in) { CTL_REQUIRE(img && host_in, "null argument"); CTL_TRY img->img.write(host_in); CTL_CATCH }
int ctl_image_add_samples(ctl_image* img, uint32_t n, const float* host_samples5) { CTL_REQUIRE(img && (host_samples5 || !n), "null argument"); CTL_TRY img->img.add_samples(n, host_samples5); CTL_CATCH }
// ---- multi-GPU: the one collective (comm.cpp)
struct ctl_comm { Comm* c; };
int ctl_comm_get_unique_id(uint8_t out128[128]) { CTL_REQUIRE(out128, "null argument"); CTL_TRY comm_unique_id(out128); CTL_CATCH }
int ctl_comm_create(const uint8_t id128[128], int32_t rank, int32_t world, ctl_comm** out) {
    CTL_REQUIRE(id128 && out, "null argument");
    CTL_TRY *out = new ctl_comm{ comm_create(id128, rank, world) }; CTL_CATCH
}
void ctl_comm_destroy(ctl_comm* c) { if (c) { comm_destroy(c->c); delete c; } }
int ctl_comm_create_timeout(const uint8_t id128[128], int32_t rank, int32_t world, int32_t timeout_ms, ctl_comm** out) {
    CTL_REQUIRE(id128 && out, "null argument");
    CTL_TRY *out = new ctl_comm{ comm_create(id128, rank, world, timeout_ms) }; CTL_CATCH
}
int ctl_image_reduce(ctl_image* img, ctl_comm* comm, int32_t root) { CTL_REQUIRE(img && comm, "null argument"); CTL_TRY comm_reduce_image(comm->c, &img->img, &img->img, root); CTL_CATCH }
int ctl_image_reduce_to(ctl_image* src, ctl_image* dst, ctl_comm* comm, int32_t root) {
    CTL_REQUIRE(src && comm, "null argument");
    CTL_REQUIRE(dst != src, "ctl_image_reduce_to: source and destination must differ (ctl_image_reduce is the in-place form)");
    CTL_TRY comm_reduce_image(comm->c, &src->img, dst ? &dst->img : nullptr, root); CTL_CATCH
}
int ctl_image_gather(ctl_image* img, ctl_comm* comm, int32_t root) { CTL_REQUIRE(img && comm, "null argument"); CTL_TRY comm_gather_image(comm->c, &img->img, &img->img, root); CTL_CATCH }
int ctl_image_gather_to(ctl_image* src, ctl_image* dst, ctl_comm* comm, int32_t root) {
    CTL_REQUIRE(src && comm, "null argument");
    CTL_REQUIRE(dst != src, "ctl_image_gather_to: source and destination must differ (ctl_image_gather is the in-place form)");
    CTL_TRY comm_gather_image(comm->c, &src->img, dst ? &dst->img : nullptr, root); CTL_CATCH
}
int ctl_image_packed_tile_bytes(uint32_t width, uint32_t height, uint32_t world, uint64_t* out_bytes) {
    CTL_REQUIRE(out_bytes && width && height, "bad argument"); CTL_TRY *out_bytes = image_packed_tile_bytes(width, height, world); CTL_CATCH
}
int ctl_image_pack_tiles(ctl_image* img, uint32_t rank, uint32_t world, void* host_out) { CTL_REQUIRE(img && host_out, "null argument"); CTL_TRY image_pack_tiles(&img->img, rank, world, host_out); CTL_CATCH }
int ctl_image_unpack_tiles(ctl_image* img, uint32_t world, const void* host_in_all_ranks) { CTL_REQUIRE(img && host_in_all_ranks, "null argument"); CTL_TRY image_unpack_tiles(&img->img, world, host_in_all_ranks); CTL_CATCH }
void* ctl_image_device_ptr(ctl_image* img) { return img ? (void*)img->img.device() : nullptr; }
int ctl_image_resolve_rgb(ctl_image* img, float splat_scale, float* host_rgb_out) { CTL_REQUIRE(img && host_rgb_out, "null argument"); CTL_TRY img->img.resolve_rgb(splat_scale, host_rgb_out); CTL_CATCH }

int ctl_image_apply_pipeline_ex(ctl_image* img, float splat_scale, const ctl_reconstruction_filter* filter, const ctl_tonemap* process, uint32_t* host_rgbcol_out) {
    CTL_REQUIRE(img && host_rgbcol_out, "null argument"); CTL_TRY img->img.apply_pipeline_ex(splat_scale, filter, process, host_rgbcol_out); CTL_CATCH
}
int ctl_image_apply_pipeline_nlm(ctl_image* img, float splat_scale, const ctl_nlm_filter* nlm, ctl_tracer* tracer, const float* host_variance, const ctl_tonemap* process,
                                 uint32_t* host_rgbcol_out) {
    // what can be judged from the arguments alone comes first (also without a device), then the device, then the state of the handles
    CTL_REQUIRE(img && nlm && host_rgbcol_out, "null argument");
    CTL_REQUIRE((tracer != nullptr) != (host_variance != nullptr), "applyImagePipeline: the NonLocalMeans filter takes its variance from exactly one of a tracer and a host array");
    CTL_REQUIRE(nlm->k >= 0.0f && nlm->sigma2_scale >= 0.0f, "applyImagePipeline: the NonLocalMeans settings k and sigma2_scale must not be negative or NaN");
    CTL_TRY
        require_device();
        const PixelVarianceBuffer* vb = nullptr;
        if (tracer) {
            TracerBase& T = *tracer->t;
            if (T.getWidth() != img->img.getWidth() || T.getHeight() != img->img.getHeight()) throw std::runtime_error("applyImagePipeline: the tracer's size differs from the image's");
            if (!T.pixelVarianceOn()) throw std::runtime_error("applyImagePipeline: the tracer keeps no pixel variance (ctl_tracer_set_pixel_variance)");
            vb = T.getPixelVarianceBuffer();
        }
        img->img.apply_pipeline_nlm(splat_scale, *nlm, vb, tracer ? tracer->t->getStream() : nullptr, host_variance, process, host_rgbcol_out);
    CTL_CATCH
}
int ctl_image_read_filtered(ctl_image* img, uint32_t* host_rgbe_out) { CTL_REQUIRE(img && host_rgbe_out, "null argument"); CTL_TRY img->img.read_filtered(host_rgbe_out); CTL_CATCH }
int ctl_image_luminance_info(ctl_image* img, float* out4) {
    CTL_REQUIRE(img && out4, "null argument");
    CTL_REQUIRE(img->img.luminance_info(out4), "getLuminanceInfo: no pipeline call with a post-process has computed the luminance info yet");
    return CTL_OK;
}
int ctl_image_last_filter_ms(ctl_image* img, float* ms_out) { CTL_REQUIRE(img && ms_out, "null argument"); *ms_out = img->img.last_filter_ms(); return CTL_OK; }
int ctl_image_apply_pipeline(ctl_image* img, float splat_scale, uint32_t* host_rgbcol_out) { CTL_REQUIRE(img && host_rgbcol_out, "null argument"); CTL_TRY img->img.apply_pipeline(splat_scale, host_rgbcol_out); CTL_CATCH }
int ctl_image_write_file(ctl_image* img, float splat_scale, const char* path) { CTL_REQUIRE(img && path, "null argument"); CTL_TRY img->img.write_file(splat_scale, path); CTL_CATCH }

// ---- tracer
int ctl_tracer_create(const char* plugin, ctl_tracer** out) {
    CTL_REQUIRE(plugin && out, "null argument");
    const bool wave = !std::strcmp(plugin, "WavefrontPathTracer") || !std::strcmp(plugin, "PT_Wave"), mega = !std::strcmp(plugin, "PathTracer") || !std::strcmp(plugin, "PT");   // main.cpp:91-96
    const bool prim = !std::strcmp(plugin, "PrimTracer") || !std::strcmp(plugin, "direct");
    if (!wave && !mega && !prim) return fail(CTL_ERR_UNSUPPORTED, std::string("unknown tracer plugin: ") + plugin);
    CTL_TRY ctl_tracer* t = new ctl_tracer(); try { t->wavefront = wave; if (wave) t->t.reset(new WavefrontPathTracer()); else if (mega) t->t.reset(new PathTracer()); else t->t.reset(new PrimTracer()); } catch (...) { delete t; throw; } *out = t; CTL_CATCH
}
void ctl_tracer_destroy(ctl_tracer* t) { delete t; }
int ctl_tracer_set_param_bool(ctl_tracer* t, const char* key, int value) { CTL_REQUIRE(t && key, "null argument"); CTL_TRY t->t->getParameters().setValue(key, value ? 1 : 0, TracerParameter::Bool); CTL_CATCH }
int ctl_tracer_set_param_int(ctl_tracer* t, const char* key, int value) { CTL_REQUIRE(t && key, "null argument"); CTL_TRY
    auto& P = t->t->getParameters();
    P.setValue(key, value, P.kindOf(key) == TracerParameter::Enum ? TracerParameter::Enum : TracerParameter::Int);   // an enum may be set by its index
CTL_CATCH }
int ctl_tracer_set_param_float(ctl_tracer* t, const char* key, float value) { CTL_REQUIRE(t && key, "null argument"); CTL_TRY t->t->getParameters().setFloat(key, value); CTL_CATCH }
int ctl_tracer_get_param_float(ctl_tracer* t, const char* key, float* value_out) { CTL_REQUIRE(t && key && value_out, "null argument"); CTL_TRY *value_out = t->t->getParameters().getFloat(key); CTL_CATCH }
int ctl_tracer_set_param_enum(ctl_tracer* t, const char* key, const char* value_name) { CTL_REQUIRE(t && key && value_name, "null argument"); CTL_TRY t->t->getParameters().setEnumByName(key, value_name); CTL_CATCH }
int ctl_tracer_get_param_int(ctl_tracer* t, const char* key, int* value_out) { CTL_REQUIRE(t && key && value_out, "null argument"); CTL_TRY *value_out = t->t->getParameters().getValue(key); CTL_CATCH }
int ctl_tracer_resize(ctl_tracer* t, uint32_t width, uint32_t height) { CTL_REQUIRE(t && width && height, "bad argument"); CTL_TRY t->t->Resize(width, height); CTL_CATCH }
int ctl_tracer_initialize_scene(ctl_tracer* t, ctl_scene* s) { CTL_REQUIRE(t && s, "null argument"); CTL_TRY t->t->InitializeScene(&s->s); t->scene = &s->s; CTL_CATCH }
int ctl_tracer_set_tile_shard(ctl_tracer* t, uint32_t rank, uint32_t world) { CTL_REQUIRE(t, "null tracer"); CTL_TRY t->t->setTileShard(rank, world); CTL_CATCH }
int ctl_tracer_set_sampler_tables(ctl_tracer* t, const float* tables_1d, const float* tables_2d) { CTL_REQUIRE(t && tables_1d && tables_2d, "null argument"); CTL_TRY t->t->setSamplerTables(tables_1d, tables_2d); CTL_CATCH }
int ctl_tracer_do_pass(ctl_tracer* t, ctl_image* img, int new_trace) { CTL_REQUIRE(t && img, "null argument"); CTL_TRY t->refuse_media(); t->t->DoPass(&img->img, new_trace != 0); CTL_CATCH }
int ctl_tracer_do_passes(ctl_tracer* t, ctl_image* img, int new_trace, uint32_t n_passes) { CTL_REQUIRE(t && img, "null argument"); CTL_TRY t->refuse_media(); t->t->DoPasses(&img->img, new_trace != 0, n_passes); CTL_CATCH }
int ctl_tracer_reserve_passes(ctl_tracer* t, uint32_t n) { CTL_REQUIRE(t, "null tracer"); CTL_TRY t->t->reservePasses(n); CTL_CATCH }
int ctl_tracer_set_block_weight(ctl_tracer* t, uint32_t bx, uint32_t by, float w) { CTL_REQUIRE(t, "null tracer"); CTL_TRY t->t->setBlockWeight(bx, by, w); CTL_CATCH }
int ctl_tracer_get_block_counts(ctl_tracer* t, uint8_t* out, uint32_t n) {
    CTL_REQUIRE(t && out, "null argument");
    CTL_TRY
        BlockSampler* bs = t->t->getBlockSampler();
        if (n != bs->n_blocks()) throw std::runtime_error("ctl_tracer_get_block_counts: the film has " + std::to_string(bs->n_blocks()) + " blocks");
        const auto& c = bs->last_counts();
        for (uint32_t i = 0; i < n; i++) out[i] = c.size() == n ? c[i] : 1;
    CTL_CATCH
}
int ctl_tracer_get_stats(ctl_tracer* t, ctl_tracer_stats* out) { CTL_REQUIRE(t && out, "null argument"); CTL_TRY t->t->getKernelStats(*out); CTL_CATCH }
int ctl_tracer_debug_pixel(ctl_tracer* t, ctl_image* img, uint32_t x, uint32_t y, float* rgb_out) { CTL_REQUIRE(t && img, "null argument"); CTL_TRY t->t->Debug(&img->img, x, y, rgb_out); CTL_CATCH }
int ctl_tracer_set_depth_buffer(ctl_tracer* t, float* device_depth, uint32_t width, uint32_t height) { CTL_REQUIRE(t, "null tracer"); CTL_REQUIRE(device_depth || (width == 0 && height == 0), "null buffer"); CTL_TRY t->t->setDepthBuffer(device_depth, width, height); CTL_CATCH }
int ctl_tracer_set_pixel_variance(ctl_tracer* t, int on) { CTL_REQUIRE(t, "null tracer"); CTL_TRY t->t->setPixelVariance(on != 0); CTL_CATCH }
int ctl_tracer_read_pixel_variance(ctl_tracer* t, float* host_out) { CTL_REQUIRE(t && host_out, "null argument"); CTL_TRY t->t->readPixelVariance(host_out); CTL_CATCH }
int ctl_tracer_set_counting(ctl_tracer* t, int on) { CTL_REQUIRE(t, "null tracer"); CTL_TRY t->t->setCounting(on != 0); CTL_CATCH }

// ---- intersect (row a7 on its own)
// alpha: the kernels alpha-test candidate hits, under the tracer's rule (the scene has alpha maps); single: the single-ray traversal (traversal_probe.h) instead of the wavefront kernel
static void run_intersect(Scene& sc, const float4* d_ro, const float4* d_rd, uint32_t n, float4* d_hit, int* d_node, uint32_t* d_occ, int any_hit, unsigned long long* d_counts, float* ms_out,
                          bool alpha = false, bool single = false) {
    dbuf<uint32_t> ctl; ctl.alloc(2);
    uint32_t h[2] = { n, 0 };
    CTL_HIP(hipMemcpy(ctl.p, h, sizeof(h), hipMemcpyHostToDevice));
    int dev = 0; hipDeviceProp_t prop; CTL_HIP(hipGetDevice(&dev)); CTL_HIP(hipGetDeviceProperties(&prop, dev));
    launch_ctx lc{ nullptr, prop.multiProcessorCount * 8, alpha && sc.S.alpha_maps != 0 };
    hipEvent_t a, b; CTL_HIP(hipEventCreate(&a)); CTL_HIP(hipEventCreate(&b));
    CTL_HIP(hipEventRecord(a, nullptr));
    if (single) launch_trace_single_probe(lc, sc.S, d_ro, d_rd, n, d_hit, d_node, any_hit);
    else if (d_counts) launch_intersect_count(lc, sc.S, d_ro, d_rd, ctl.p, ctl.p + 1, d_hit, d_node, nullptr, any_hit, d_counts);
    else if (any_hit) launch_intersect_any(lc, sc.S, d_ro, d_rd, ctl.p, ctl.p + 1, d_occ, d_hit, d_node);
    else launch_intersect_closest(lc, sc.S, d_ro, d_rd, ctl.p, ctl.p + 1, d_hit, d_node);
    CTL_HIP(hipEventRecord(b, nullptr));
    CTL_HIP(hipEventSynchronize(b));
    CTL_HIP(hipGetLastError());
    float ms = 0; CTL_HIP(hipEventElapsedTime(&ms, a, b));
    if (ms_out) *ms_out = ms;
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
}
// the entry points that exist for the tests fill their device outputs with values no kernel writes, so that a ray that was never traced shows in the result
constexpr int kPoisonIndex = -2; constexpr uint32_t kPoisonOcc = 0xffffffffu;
static void upload_rays(const ctl_ray* rays, uint32_t n, dbuf<float4>& d_ro, dbuf<float4>& d_rd) {
    std::vector<float4> ro(n), rd(n);
    for (uint32_t i = 0; i < n; i++) { ro[i] = make_float4(rays[i].a[0], rays[i].a[1], rays[i].a[2], rays[i].a[3]); rd[i] = make_float4(rays[i].b[0], rays[i].b[1], rays[i].b[2], rays[i].b[3]); }
    d_ro.upload(ro.data(), n); d_rd.upload(rd.data(), n);
    CTL_HIP(hipStreamSynchronize(nullptr));   // the staging vectors end here
}
static void poison_hits(uint32_t n, dbuf<float4>& d_hit, dbuf<int>& d_node) {
    const std::vector<float4> hh(n, make_float4(0.0f, 0.0f, 0.0f, __builtin_bit_cast(float, kPoisonIndex))); const std::vector<int> hn(n, kPoisonIndex);
    d_hit.upload(hh.data(), n); d_node.upload(hn.data(), n);
    CTL_HIP(hipStreamSynchronize(nullptr));
}
static void download_hits(uint32_t n, const dbuf<float4>& d_hit, const dbuf<int>& d_node, ctl_hit* hits) {
    std::vector<float4> hh(n); std::vector<int> hn(n);
    CTL_HIP(hipMemcpy(hh.data(), d_hit.p, (size_t)n * 16, hipMemcpyDeviceToHost)); CTL_HIP(hipMemcpy(hn.data(), d_node.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; i++) { hits[i].dist = hh[i].x; hits[i].u = hh[i].y; hits[i].v = hh[i].z; hits[i].tri_idx = __builtin_bit_cast(int, hh[i].w); hits[i].node_idx = hn[i]; }
}
static void intersect_host(Scene& sc, const ctl_ray* rays, uint32_t n, ctl_hit* hits, int any_hit, ctl_traversal_counts* counts, bool alpha = false, bool single = false, bool poison = false) {
    dbuf<float4> d_ro, d_rd, d_hit; dbuf<int> d_node; dbuf<unsigned long long> d_cnt;
    upload_rays(rays, n, d_ro, d_rd);
    if (poison) poison_hits(n, d_hit, d_node); else { d_hit.alloc(n); d_node.alloc(n); }
    if (counts) { d_cnt.alloc(5); CTL_HIP(hipMemset(d_cnt.p, 0, 40)); }
    CTL_HIP(hipDeviceSynchronize());
    run_intersect(sc, d_ro.p, d_rd.p, n, d_hit.p, d_node.p, nullptr, any_hit, counts ? d_cnt.p : nullptr, nullptr, alpha, single);
    if (hits) download_hits(n, d_hit, d_node, hits);
    if (counts) { unsigned long long c[5]; CTL_HIP(hipMemcpy(c, d_cnt.p, 40, hipMemcpyDeviceToHost)); *counts = ctl_traversal_counts{ c[0], c[1], c[2], c[3], c[4] }; }
}
int ctl_trace_single_ray(ctl_scene* s, const ctl_ray* ray, ctl_hit* hit_out) { CTL_REQUIRE(s && ray && hit_out, "null argument"); return ctl_intersect(s, ray, 1, hit_out, 0); }
int ctl_intersect(ctl_scene* s, const ctl_ray* rays, uint32_t n, ctl_hit* hits, int any_hit) {
    CTL_REQUIRE(s && (rays || !n) && (hits || !n), "null argument");
    if (!n) return CTL_OK;
    CTL_TRY intersect_host(s->s, rays, n, hits, any_hit, nullptr); CTL_CATCH
}
int ctl_intersect_count(ctl_scene* s, const ctl_ray* rays, uint32_t n, int any_hit, ctl_traversal_counts* out) {
    CTL_REQUIRE(s && rays && out, "null argument");
    CTL_TRY intersect_host(s->s, rays, n, nullptr, any_hit, out); CTL_CATCH
}
int ctl_intersect_ex(ctl_scene* s, const ctl_ray* rays, uint32_t n, ctl_hit* hits, uint32_t flags) {
    CTL_REQUIRE(s && (rays || !n) && (hits || !n), "null argument");
    CTL_REQUIRE(!(flags & ~(uint32_t)(CTL_ISECT_ANY_HIT | CTL_ISECT_ALPHA | CTL_ISECT_SINGLE)), "ctl_intersect_ex: unknown flag bits");
    // (the PathTracer's own refusal, megakernel.hip InitializeScene: its traversal walks the flattened tree only)
    if ((flags & CTL_ISECT_SINGLE) && !s->s.S.flat_nodes) return fail(CTL_ERR_UNSUPPORTED, "ctl_intersect_ex: CTL_ISECT_SINGLE needs a scene created with CTL_SCENE_FLATTEN");
    if (!n) return CTL_OK;
    CTL_TRY intersect_host(s->s, rays, n, hits, (flags & CTL_ISECT_ANY_HIT) ? 1 : 0, nullptr, (flags & CTL_ISECT_ALPHA) != 0, (flags & CTL_ISECT_SINGLE) != 0, true); CTL_CATCH
}
int ctl_intersect_pair(ctl_scene* s, const ctl_ray* rays, uint32_t n, ctl_hit* hits, const ctl_ray* shadow_rays, uint32_t sn, uint32_t* occ_out, uint32_t flags) {
    CTL_REQUIRE(s && (rays || !n) && (hits || !n) && (shadow_rays || !sn) && (occ_out || !sn), "null argument");
    CTL_REQUIRE(!(flags & ~(uint32_t)CTL_ISECT_ALPHA), "ctl_intersect_pair: only CTL_ISECT_ALPHA is accepted");
    if (!n && !sn) return CTL_OK;
    CTL_TRY
        Scene& sc = s->s;
        dbuf<float4> d_ro, d_rd, d_sro, d_srd, d_hit; dbuf<int> d_node; dbuf<uint32_t> d_occ, ctl;
        upload_rays(rays, n, d_ro, d_rd); upload_rays(shadow_rays, sn, d_sro, d_srd);
        poison_hits(n, d_hit, d_node);
        const std::vector<uint32_t> po(sn, kPoisonOcc); d_occ.upload(po.data(), sn);
        const uint32_t h[4] = { n, sn, 0u, 0u };   // the two queue lengths, then one ray cursor per queue, as tracer.hip hands them to the fused launch
        ctl.upload(h, 4);
        int dev = 0; hipDeviceProp_t prop; CTL_HIP(hipGetDevice(&dev)); CTL_HIP(hipGetDeviceProperties(&prop, dev));
        const launch_ctx lc{ nullptr, prop.multiProcessorCount * 8, (flags & CTL_ISECT_ALPHA) != 0 && sc.S.alpha_maps != 0 };
        CTL_HIP(hipDeviceSynchronize());
        launch_intersect_pair(lc, sc.S, d_ro.p, d_rd.p, ctl.p, ctl.p + 2, d_hit.p, d_node.p, d_sro.p, d_srd.p, ctl.p + 1, ctl.p + 3, d_occ.p);
        CTL_HIP(hipDeviceSynchronize());
        CTL_HIP(hipGetLastError());
        if (n) download_hits(n, d_hit, d_node, hits);
        if (sn) CTL_HIP(hipMemcpy(occ_out, d_occ.p, (size_t)sn * 4, hipMemcpyDeviceToHost));
    CTL_CATCH
}
int ctl_traversal_lds_rows(uint32_t out5[5]) { CTL_REQUIRE(out5, "null argument"); traversal_lds_rows(out5); return CTL_OK; }
int ctl_intersect_device(ctl_scene* s, const void* d_ray_o, const void* d_ray_d, uint32_t n, void* d_hit4, void* d_hit_node, int any_hit, float* ms_out) {
    CTL_REQUIRE(s && d_ray_o && d_ray_d && d_hit4 && d_hit_node, "null argument");
    CTL_TRY run_intersect(s->s, (const float4*)d_ray_o, (const float4*)d_ray_d, n, (float4*)d_hit4, (int*)d_hit_node, nullptr, any_hit, nullptr, ms_out); CTL_CATCH
}

// ---- device memory helpers
int ctl_device_malloc(size_t bytes, void** out) { CTL_REQUIRE(out, "null out"); CTL_TRY require_device(); CTL_HIP(hipMalloc(out, bytes)); CTL_CATCH }
int ctl_device_free(void* p) { CTL_TRY CTL_HIP(hipFree(p)); CTL_CATCH }
int ctl_memcpy_h2d(void* dst, const void* src, size_t bytes) { CTL_TRY CTL_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); CTL_CATCH }
int ctl_memcpy_d2h(void* dst, const void* src, size_t bytes) { CTL_TRY CTL_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); CTL_CATCH }
int ctl_memcpy_d2d(void* dst, const void* src, size_t bytes) { CTL_TRY CTL_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice)); CTL_CATCH }
int ctl_device_synchronize(void) { CTL_TRY require_device(); CTL_HIP(hipDeviceSynchronize()); CTL_CATCH }
int ctl_set_device(int ordinal) { CTL_TRY require_device(); CTL_HIP(hipSetDevice(ordinal)); CTL_CATCH }

} // extern "C"
