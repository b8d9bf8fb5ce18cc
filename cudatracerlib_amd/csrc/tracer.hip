// tracer.hip — host side of the plugin: scene upload / re-layout, Image, the Tracer<PROGRESSIVE> pass loop and the
// WavefrontPathTracer bounce loop (Integrators/PseudoRealtime/WavefrontPathTracer.cu:166-191 re-designed:
// no host synchronisation inside a pass — queue lengths stay on the device).
#include "tracer.h"
#include "scene_builder.h"
#include "scene_checks.h"
#include "scene_volumes.h"
#include "flatten.h"
#include "image_io.h"
#include "mitsuba_loader.h"   // unsupported_error
#include "spline.h"
#include "mip_pyramid.h"
#include "ctl_fmath.h"
#include "knobs.h"
#include <algorithm>
#include <thread>
#include <cctype>
#include <cstring>
#include <cstdlib>
#include <string>

namespace ctl {

void throw_hip(hipError_t e, const char* file, int line) {   // ThrowCudaErrors (Defines.cpp:15-29)
    throw hip_error(std::string("In file ") + file + ", line " + std::to_string(line) + " : " + hipGetErrorString(e));
}
int device_count() { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
void require_device() { if (device_count() <= 0) throw hip_error("no HIP device: the MI355X path tracer has no CPU fallback"); apply_tuning_from_env(); }
int persistent_grid_blocks() { int dev = 0; hipDeviceProp_t prop; CTL_HIP(hipGetDevice(&dev)); CTL_HIP(hipGetDeviceProperties(&prop, dev)); return prop.multiProcessorCount * 8; }

// ------------------------------------------------------------------------------------------------ Scene
// The blocks of the upload that Scene::update repeats for the part of a description that changed (scene_update.hip); the constructor runs them all, in the order it always did.
void Scene::upload_top_level(const ctl_scene_desc& d) {
    // the scene BVH keeps the reference's 64-B node (one aligned 64-B fetch group per visit)
    std::vector<float4> tmp(std::max<size_t>(4, (size_t)d.n_scene_bvh_nodes * 4), make_float4(0, 0, 0, 0));
    if (d.n_scene_bvh_nodes) std::memcpy(tmp.data(), d.scene_bvh_nodes, (size_t)d.n_scene_bvh_nodes * 64);
    top_nodes_.upload(tmp.data(), tmp.size());
}
void Scene::pack_instances(const ctl_scene_desc& d, std::vector<float4>& inst, std::vector<float4>& fwd, std::vector<uint4>& ninfo) {
    // instances: inverse transform rows + the mesh offsets the reference fetches from Node / KernelMesh (TraceHelper.cu:530,557-560)
    inst.resize((size_t)d.n_nodes * 4); fwd.resize((size_t)d.n_nodes * 3); ninfo.resize(d.n_nodes);
    for (uint32_t k = 0; k < d.n_nodes; k++) {
        const float* im = d.node_inv_transforms[k].m; const float* fm = d.node_transforms[k].m;
        const ctl_node& N = d.nodes[k];   // (affine transforms, an existing mesh: check_scene_desc)
        const ctl_kernel_mesh& km = d.meshes[N.mesh_index];
        for (int r = 0; r < 3; r++) { inst[k * 4 + r] = make_float4(im[r * 4], im[r * 4 + 1], im[r * 4 + 2], im[r * 4 + 3]); fwd[k * 3 + r] = make_float4(fm[r * 4], fm[r * 4 + 1], fm[r * 4 + 2], fm[r * 4 + 3]); }
        inst[k * 4 + 3] = make_float4(im[15], __builtin_bit_cast(float, km.bvh_node_offset), __builtin_bit_cast(float, km.bvh_tri_offset / 3), __builtin_bit_cast(float, km.tri_offset));
        ninfo[k] = make_uint4(N.material_offset, N.lights[0], N.lights[1], N.n_lights);
    }
}
void Scene::upload_instances(const ctl_scene_desc& d) {
    std::vector<float4> inst, fwd; std::vector<uint4> ninfo;
    pack_instances(d, inst, fwd, ninfo);
    inst_.upload(inst.data(), inst.size()); inst_fwd_.upload(fwd.data(), fwd.size()); node_info_.upload(ninfo.data(), ninfo.size());
}
void Scene::upload_lights(const ctl_scene_desc& d) {
    if (d.n_lights_buf) lights_.upload(d.lights, d.n_lights_buf); else if (!lights_.p) lights_.alloc(1);
    if (d.n_anim_bytes) anim_.upload(d.anim, d.n_anim_bytes); else if (!anim_.p) anim_.alloc(16);
}

void Scene::upload_materials(const ctl_scene_desc& d) {
    std::vector<ctl_material> dmats(d.materials, d.materials + d.n_materials);   // uploaded below, once the reduced transmittance tables are attached
    for (auto& m : dmats) m.reserved_[0] = m.reserved_[1] = 0;
    // Rough plastics with a CONSTANT roughness texture look RoughTransmittanceManager's table up at a fixed (alpha, eta) (RoughTransmittance.cu:55-88 -> Math/Spline.cu:376-453).
    // What depends on those two alone is made here, once per material (bsdf_rough.h roughplastic_T):
    //  * default — the sixteen rows the 3-D interpolation reads for this (alpha, eta) and the sixteen products wy * wz of its weights; the device runs the reference's own sum
    //    over them: the same value to the bit, without the warp's two pow(), two sets of spline weights, the strided addressing and the per-tap branch of every lookup;
    //  * CTL_SCENE_REDUCED_ROUGH_TRANSMITTANCE (opt-in) — the rows summed over alpha / eta beforehand (a 1-D table, 4 taps instead of 64): equal up to fp32 rounding, which is NOT
    //    equal: the last bits move the rescaled lobe sample, and a texture boundary under the next hit turns that into another colour (profiles/r05_fuzz.log: up to 0.13 % of a
    //    textured scene's pixels beyond the tolerance, 5 % of the bathroom miniature's pixels equal to the bit against 100 %).
    // The arithmetic is the device's: ctl_fmath.h's pow (the kernels' m_pow), fp32, no contraction.
    const bool reduced_rough_transmittance = reduced_rough_transmittance_;
    S.rt_reduced = nullptr;
    if (d.rough_transmittance) {
        std::vector<float> pool;
        for (auto& m : dmats) {
            if (m.bsdf_type != CTL_BSDF_ROUGHPLASTIC || m.tex[2].type != CTL_TEX_CONSTANT || m.u[2] > CTL_MF_PHONG) continue;
            const ctl_rough_transmittance& T = d.rough_transmittance[m.u[2]];
            if (!T.trans || !T.diff_trans || T.theta_samples < 2 || T.alpha_samples < 2 || T.eta_samples < 2) continue;
            float r = m.tex[2].value[0]; r += m.tex[2].value[1]; r += m.tex[2].value[2];
            const float avg = r * (1.0f / 3), alpha = avg > 1e-4f ? avg : 1e-4f;   // avg3 (shading.h) + the MicrofacetDistribution constructor's max(alpha, 1e-4f)
            float eta = m.f[0];
            const float* data = T.trans; const float* ddata = T.diff_trans;
            if (eta < 1) { data += (size_t)T.eta_samples * T.alpha_samples * T.theta_samples; ddata += (size_t)T.eta_samples * T.alpha_samples; eta = 1.0f / eta; }
            if (eta < T.eta_min) eta = T.eta_min;
            const float wa = fm::pow((alpha - T.alpha_min) / (T.alpha_max - T.alpha_min), 0.25f), we = fm::pow((eta - T.eta_min) / (T.eta_max - T.eta_min), 0.25f);
            const float dv = spline_eval_2d(wa, we, ddata, T.alpha_samples, T.eta_samples);
            const float diffuse = std::min(1.0f, std::max(0.0f, dv));   // RoughTransmittanceManager::EvaluateDiffuse clamps
            const uint32_t sx = T.theta_samples;
            if (reduced_rough_transmittance) {
                m.reserved_[0] = (uint32_t)pool.size() + 1; m.reserved_[1] = sx;
                pool.resize(pool.size() + sx);
                spline_reduce_3d_to_1d(wa, we, data, sx, T.alpha_samples, T.eta_samples, pool.data() + pool.size() - sx);
                pool.push_back(diffuse);
                continue;
            }
            if (const char* e = knob_env("CTL_RT_ROWS")) { if (std::atoi(e) == 0) continue; }   // measurement build only (knobs.h): every lookup through the generic 3-D function (profiles/r05_fuzz.log)
            float wy[4], wz[4]; uint32_t ky, kz;
            if (!spline_weights(wa, T.alpha_samples, wy, ky) || !spline_weights(we, T.eta_samples, wz, kz)) continue;   // outside the table: the device's generic lookup returns its 0
            m.reserved_[0] = (uint32_t)pool.size() + 1; m.reserved_[1] = sx | 0x80000000u;   // kRtRows (bsdf_rough.h)
            const size_t base = pool.size();
            pool.resize(base + 16 + (size_t)16 * sx + 1, 0.0f);
            for (int z = -1, zy = 0; z <= 2; ++z) for (int y = -1; y <= 2; ++y, ++zy) {
                const float wyz = wy[y + 1] * wz[z + 1];      // spline_eval_3d's own product
                pool[base + zy] = wyz;
                // a row whose weight is zero is never read (spline_eval_3d skips a zero product); at the table's border it would lie outside
                if (wyz != 0) std::memcpy(&pool[base + 16 + (size_t)zy * sx], data + ((size_t)(kz + z) * T.alpha_samples + (ky + y)) * sx, sizeof(float) * sx);
            }
            pool[base + 16 + (size_t)16 * sx] = diffuse;
            // the device adds every tap where spline_eval_3d skips a zero weight: the same value only over FINITE entries (0 x inf is NaN) — a table that holds anything else
            // keeps the generic lookup
            bool finite = true;
            for (size_t q = base; q < pool.size(); q++) finite = finite && std::isfinite(pool[q]);
            if (!finite) { pool.resize(base); m.reserved_[0] = m.reserved_[1] = 0; }
        }
        if (!pool.empty()) { rt_reduced_.upload(pool.data(), pool.size()); S.rt_reduced = rt_reduced_.p; }
        else for (auto& m : dmats) m.reserved_[0] = 0;
    }
    mats_.upload(dmats.data(), dmats.size());
}
void Scene::bind(const ctl_scene_desc& d) {
    for (int k = 0; k < 3; k++) { box_min[k] = d.box_min[k]; box_max[k] = d.box_max[k]; }
    S.top_nodes = top_nodes_.p; S.bot_nodes = bot_nodes_.p; S.leaf_tris = leaf_tris_.p; S.inst = inst_.p; S.inst_fwd = inst_fwd_.p; S.normal_lut = normal_lut_.p;
    S.tri_data = tri_data_.p; S.node_info = node_info_.p; S.mats = mats_.p; S.lights = lights_.p; S.anim = anim_.p; S.n_lights_buf = d.n_lights_buf; S.n_anim_bytes = (uint32_t)d.n_anim_bytes; S.n_materials_probe = std::max(1u, d.n_materials);
    S.start_node = d.scene_start_node; S.n_nodes = d.n_nodes; S.num_lights = d.num_lights; S.env_map_index = d.env_map_index; S.eps = d.ray_trace_eps;
    for (int i = 0; i < CTL_MAX_NUM_LIGHTS; i++) { S.light_indices[i] = d.light_indices[i]; S.light_cdf[i] = d.light_cdf[i]; }
}
void Scene::set_camera(const ctl_scene_desc& d) {
    near_depth = d.camera.near_depth; far_depth = d.camera.far_depth;
    // PerspectiveSensor / ThinLensSensor / OrthographicSensor / TelecentricSensor ::Update (SceneTypes/Sensor.cu:76-96, :226-246, :408-427, :515-535)
    const ctl_sensor& c = d.camera;
    const bool ortho = c.type == CTL_SENSOR_ORTHOGRAPHIC || c.type == CTL_SENSOR_TELECENTRIC;
    const float aspect = c.resolution[0] / c.resolution[1];
    const float recip = 1.0f / (c.far_depth - c.near_depth), cot = 1.0f / tanf(c.fov / 2.0f);
    float persp[16] = { cot, 0, 0, 0, 0, cot, 0, 0, 0, 0, c.far_depth * recip, -c.near_depth * c.far_depth * recip, 0, 0, 1, 0 };
    if (ortho) {   // float4x4::orthographic (float4x4.h:625-628) = Scale(1, 1, 1 / (far - near)) % Translate(0, 0, -near)
        const float so[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1.0f / (c.far_depth - c.near_depth), 0, 0, 0, 0, 1 };
        const float to[16] = { 1, 0, 0, 0.0f, 0, 1, 0, 0.0f, 0, 0, 1, -c.near_depth, 0, 0, 0, 1 };
        mat_mul(so, to, persp);
    }
    S.cam.type = c.type; S.cam.aperture_radius = c.aperture_radius; S.cam.focus_distance = c.focus_distance; S.cam.screen_scale_x = c.screen_scale[0] != 0.0f ? c.screen_scale[0] : 1.0f;
    const float sc[16] = { -0.5f, 0, 0, 0, 0, -0.5f * aspect, 0, 0, 0, 0, 1.0f, 0, 0, 0, 0, 1 };
    const float tr[16] = { 1, 0, 0, -1.0f, 0, 1, 0, -1.0f / aspect, 0, 0, 1, 0.0f, 0, 0, 0, 1 };
    float a[16], c2s[16];
    mat_mul(sc, tr, a); mat_mul(a, persp, c2s);
    mat_inverse(c2s, S.cam.s2c);
    std::memcpy(S.cam.to_world, c.to_world, 48);
    S.cam.inv_res[0] = 1.0f / c.resolution[0]; S.cam.inv_res[1] = 1.0f / c.resolution[1];
    {   // m_dx, m_dy (Sensor.cu:86-89): sampleToCamera(1/w, 0, 0) - sampleToCamera(0), projective TransformPoint
        auto tp = [&](float x, float y, float out[3]) {
            float r[4];
            for (int i = 0; i < 4; i++) { float s2 = 0.0f; s2 += S.cam.s2c[i * 4] * x; s2 += S.cam.s2c[i * 4 + 1] * y; s2 += S.cam.s2c[i * 4 + 2] * 0.0f; s2 += S.cam.s2c[i * 4 + 3] * 1.0f; r[i] = s2; }
            out[0] = r[0] / r[3]; out[1] = r[1] / r[3]; out[2] = r[2] / r[3];
        };
        float p0[3], px[3], py[3]; tp(0, 0, p0); tp(S.cam.inv_res[0], 0, px); tp(0, S.cam.inv_res[1], py);
        for (int k = 0; k < 3; k++) { S.cam.dx[k] = px[k] - p0[k]; S.cam.dy[k] = py[k] - p0[k]; }
    }
}

Scene::Scene(const ctl_scene_desc& d, bool flatten, int flat_format, bool reduced_rough_transmittance) : reduced_rough_transmittance_(reduced_rough_transmittance) {
    require_device();
    check_scene_desc(d, kCheckAllParts, "ctl_scene_create");   // everything that can be judged from the description alone, before the first upload
    n_nodes = d.n_nodes;
    std::vector<float4> tmp;
    upload_top_level(d);
    // the mesh BVHs keep the reference's 64-B node too
    tmp.assign(std::max<size_t>(4, (size_t)d.n_bvh_nodes * 4), make_float4(0, 0, 0, 0));
    if (d.n_bvh_nodes) std::memcpy(tmp.data(), d.bvh_nodes, (size_t)d.n_bvh_nodes * 64);
    bot_nodes_.upload(tmp.data(), tmp.size());
    // leaf entries: Woop rows + index word interleaved to a 64-B stride so a leaf streams as whole 64-B groups
    // (the reference reads 3 float4 from t_tris and 1 uint from t_triIndices, Kernel/TraceHelper.cu:641-644)
    std::vector<std::pair<uint32_t, uint32_t>> ranges;   // (first woop entry, mesh)
    for (uint32_t m = 0; m < d.n_meshes; m++) ranges.emplace_back(d.meshes[m].bvh_tri_offset / 3, m);
    std::sort(ranges.begin(), ranges.end());
    tmp.assign(std::max<size_t>(4, (size_t)d.n_woop * 4), make_float4(0, 0, 0, 0));
    for (size_t r = 0; r < ranges.size(); r++) {
        const uint32_t first = ranges[r].first, last = (r + 1 < ranges.size()) ? ranges[r + 1].first : d.n_woop;
        const ctl_kernel_mesh& km = d.meshes[ranges[r].second];
        for (uint32_t w = first; w < last; w++) {
            const ctl_woop_tri& t = d.woop[w];
            tmp[w * 4 + 0] = make_float4(t.a[0], t.a[1], t.a[2], t.a[3]);
            tmp[w * 4 + 1] = make_float4(t.b[0], t.b[1], t.b[2], t.b[3]);
            tmp[w * 4 + 2] = make_float4(t.c[0], t.c[1], t.c[2], t.c[3]);
            const uint32_t idx = d.woop_index[km.bvh_index_offset + (w - first)].index;
            tmp[w * 4 + 3] = make_float4(__builtin_bit_cast(float, idx), 0, 0, 0);
        }
    }
    leaf_tris_.upload(tmp.data(), tmp.size());
    upload_instances(d);
    { std::vector<float> lut(1024); normal_codec_lut(lut.data()); normal_lut_.upload((const float2*)lut.data(), 512); }
    static_assert(sizeof(ctl_triangle_data) == 32, "TriangleData is 32 B");
    static_assert(sizeof(ctl_material) == 384 && sizeof(ctl_texture) == 48, "material descriptor layout (include/ctl_amd.h)");
    tri_data_.upload((const uint4*)d.tri_data, (size_t)d.n_tri_data * 2);
    upload_lights(d);
    // KernelMIPMap of every image: one texel pool (level 0, then the pyramid MIPMap::CompileToBinary builds, Engine/MIPMap.cpp:41-95: nLevels = 1 + log2(min(w, h)),
    // level i = the 2x2 box average of level i-1, decoded, averaged and re-encoded) + a table of level-0 descriptors with device pointers + the level offsets
    {
        std::vector<uint32_t> pool;
        std::vector<size_t> off(d.n_images);
        std::vector<dev_mip_levels> lv(std::max<uint32_t>(1, d.n_images));
        static_assert(sizeof(mip_level_table) == sizeof(dev_mip_levels), "one layout");
        for (uint32_t i = 0; i < d.n_images; i++) {
            const ctl_mipmap& m = d.images[i];
            if (!m.texels || !m.width || !m.height) throw std::runtime_error("ctl_scene_create: empty image");
            mip_level_table L; off[i] = mip_pyramid_append(m, pool, L);   // mip_pyramid.h
            std::memcpy(&lv[i], &L, sizeof(L));
        }
        if (!pool.empty()) texels_.upload(pool.data(), pool.size()); else texels_.alloc(4);
        image_off_ = off; image_levels_.assign(lv.begin(), lv.begin() + d.n_images); image_avg_.assign((size_t)d.n_images * 4, 0.0f);   // what ctl_scene_update_image starts from (scene_images.hip)
        for (uint32_t i = 0; i < d.n_images; i++) {
            mip_level_table L; std::memcpy(&L, &lv[i], sizeof(L));
            mip_texel_decode(pool[off[i] + mip_average_texel_offset(d.images[i], L)], d.images[i].texel_type, &image_avg_[(size_t)i * 4]); image_avg_[(size_t)i * 4 + 3] = 1.0f;
        }
        std::vector<ctl_mipmap> tab(d.n_images);
        for (uint32_t i = 0; i < d.n_images; i++) { tab[i] = d.images[i]; tab[i].texels = texels_.p + off[i]; }
        if (d.n_images) images_.upload(tab.data(), tab.size()); else images_.alloc(1);
        mip_levels_.upload(lv.data(), lv.size());
        float lut[64];   // MIPMap.cpp:87-92
        for (int i = 0; i < 64; i++) { const float r2 = (float)i / (float)(64 - 1); lut[i] = std::exp(-2.0f * r2) - std::exp(-2.0f); }
        mip_lut_.upload(lut, 64);
        S.images = images_.p; S.mip_levels = mip_levels_.p; S.mip_weight_lut = mip_lut_.p;
    }
    // RoughTransmittanceManager's tables (roughplastic): one float pool + 3 descriptors with device pointers
    S.rough_transmittance = nullptr;
    if (d.rough_transmittance) {
        std::vector<float> pool; size_t off_t[3] = {}, off_d[3] = {};
        for (int i = 0; i < 3; i++) {
            const ctl_rough_transmittance& t = d.rough_transmittance[i];
            if (!t.trans || !t.diff_trans) continue;
            const size_t nt = (size_t)2 * t.eta_samples * t.alpha_samples * t.theta_samples, nd = (size_t)2 * t.eta_samples * t.alpha_samples;
            off_t[i] = pool.size(); pool.insert(pool.end(), t.trans, t.trans + nt);
            off_d[i] = pool.size(); pool.insert(pool.end(), t.diff_trans, t.diff_trans + nd);
        }
        if (!pool.empty()) {
            rt_data_.upload(pool.data(), pool.size());
            ctl_rough_transmittance tab[3];
            for (int i = 0; i < 3; i++) { tab[i] = d.rough_transmittance[i]; const bool ok = tab[i].trans && tab[i].diff_trans; tab[i].trans = ok ? rt_data_.p + off_t[i] : nullptr; tab[i].diff_trans = ok ? rt_data_.p + off_d[i] : nullptr; }
            rt_.upload(tab, 3);
            S.rough_transmittance = rt_.p;
        }
    }
    upload_materials(d);
    set_shading_state(derive_shading_state(d));
    S.hit_key_out = nullptr; S.flat_leaf_keys = 0;
    S.flat_nodes = nullptr; S.flat_leaves = nullptr; S.flat_root = 0; S.flat_format = 0; S.flat_compact = 0; S.inst_w_one = 0; S.flat_top_cached = 0;
    if (flatten) {
        // node format: Q4 (64-B 4-wide nodes with 8-bit child boxes) unless the caller or $CTL_FLAT_FORMAT asks for Q8; the retired formats 1 and 2 (F4 / F2) are refused (EXPERIMENTS.md has the measurements)
        if (flat_format == 1 || flat_format == 2) throw unsupported_error("ctl_scene_create: flat node formats 1 and 2 (F4 / F2) are retired: no traversal kernel reads them (EXPERIMENTS.md)");
        flat_scene F;
        if (flatten_scene(d, F, (size_t)1 << 30, flat_format < 0 ? default_flat_format() : flat_format)) {   // up to 2^30 instanced triangles (64 GiB of leaf entries)
            if (F.stack_need() + 2 > (F.format == kFlatQ8 ? kFlat8StackGroups : kStackSize)) throw std::runtime_error("ctl_scene_create: flattened BVH too deep for the traversal stack");
            if (F.format == kFlatQ4) flat_nodes_.upload((const float4*)F.nodes.data(), F.nodes.size() * 4);
            else flat_nodes_.upload((const float4*)F.nodes_q8.data(), F.nodes_q8.size() * 8);
            for (const flat_leaf& L : F.leaves) if (L.node >= d.n_nodes) throw std::runtime_error("ctl_scene_create: flattened leaf entry out of range");
            S.flat_leaf_keys = 0;
            if (F.format == kFlatQ4 && F.refit.ready()) flat_missing_triangles(F.leaves, 0xffffffffu, d, flat_missing_tris_);   // what a geometry update cannot bring back (scene_update.hip); before the bits below are stamped
            // The DEVICE copy of the entries carries the BSDF model of each entry's material in bits 28..31 of its index word (the host arrays, the cache and the oracle's view stay
            // as flatten.cpp made them): a closest-hit traversal leaves it per ray (dev_scene::hit_key_out) and the shade kernel regroups its lanes by it without the
            // hit -> node -> triangle -> material chain of dependent loads that made the regrouping cost more than it won.
            if (d.n_tri_data < (1u << 27) && d.n_materials) {
                for (flat_leaf& L : F.leaves) {
                    const uint32_t tri = L.index >> 1, mi = d.nodes[L.node].material_offset + ((d.tri_data[tri].nor_mat_extra[1] >> 16) & 0xffu);   // TriangleData::getMatIndex (TriangleData.h:40-44)
                    // key 0 is the miss key: a hit whose material does not exist would be partitioned as a hit and shaded from a record outside the scene's materials
                    if (mi >= d.n_materials) throw std::runtime_error("ctl_scene_create: triangle " + std::to_string(tri) + " of node " + std::to_string(L.node) + " names material " + std::to_string(mi) + " of " + std::to_string(d.n_materials));
                    L.index |= (d.materials[mi].bsdf_type & 15u) << 28;
                }
                S.flat_leaf_keys = 1;
            }
            // ... and, in a scene with alpha maps, bit 31 of the node word says that THIS entry's material has one: the alpha-testing traversal kernels (AlphaTest) test those
            // entries only, and the wavefront kernel collects their candidates for a phase of its own (flat_woop_test, intersect_flat)
            if (S.alpha_maps && d.n_materials)
                for (flat_leaf& L : F.leaves) {
                    const uint32_t tri = (S.flat_leaf_keys ? (L.index & 0x0fffffffu) : L.index) >> 1, mi = d.nodes[L.node].material_offset + ((d.tri_data[tri].nor_mat_extra[1] >> 16) & 0xffu);
                    if (mi >= d.n_materials || d.materials[mi].alpha_state != CTL_ALPHA_DISABLED) L.node |= 0x80000000u;
                }
            F.leaves.emplace_back(); std::memset(&F.leaves.back(), 0, sizeof(flat_leaf)); F.leaves.back().index = 1;   // one spare (closing) entry behind the last leaf
            flat_leaves_.upload((const float4*)F.leaves.data(), F.leaves.size() * 8);
            S.inst_w_one = inverse_transforms_have_w_one(d);
            CTL_HIP(hipDeviceSynchronize());
            S.flat_nodes = flat_nodes_.p; S.flat_leaves = flat_leaves_.p; S.flat_format = F.format; S.flat_compact = (F.format == kFlatQ4 && F.compact_links) ? 1 : 0;
            S.flat_root = ((S.flat_compact || F.format == kFlatQ8) && F.root_slab) ? 1 : 0;   // bit 0 of an inner link: the node carries an oriented slab (flat_slab.h); Q8 links are node index << 1 | that bit
            S.flat_top_cached = S.flat_compact ? (int)std::min<size_t>(F.nodes.size(), (size_t)flat_top_cache_nodes()) : 0;
            // what ctl_scene_update needs to refit this tree in place (flat_refit.h; Q4 only): the side arrays go to HBM now, the scratch boxes with the first transform update
            flat_n_nodes_ = F.format == kFlatQ4 ? F.nodes.size() : F.nodes_q8.size(); flat_n_entries_ = F.leaves.size() - 1; flat_max_depth_ = F.max_depth; flat_root_slab_ = F.root_slab; flat_slab_nodes_ = F.slab_nodes;
            if (F.format == kFlatQ4 && F.refit.ready()) {
                refit_part_index_.upload(F.refit.part_index.data(), F.refit.part_index.size());
                if (!F.refit.part_boxes.empty()) refit_part_boxes_.upload(F.refit.part_boxes.data(), F.refit.part_boxes.size());
                refit_level_nodes_.upload(F.refit.level_nodes.data(), F.refit.level_nodes.size());
                if (!S.flat_compact) flat_child_links_ = F.child_links;   // host view of a tree with explicit links (read_flat_bvh); a compact tree's links are derived
                refit_ = std::move(F.refit); refit_.part_index.clear(); refit_.part_index.shrink_to_fit(); refit_.level_nodes.clear(); refit_.level_nodes.shrink_to_fit();
                CTL_HIP(hipDeviceSynchronize());
            }
        }
    }
    CTL_HIP(hipDeviceSynchronize());
    bind(d);
    set_camera(d);
    snapshot(d);
}
Scene::~Scene() {}   // out of line: scene_volumes is complete here

// ------------------------------------------------------------------------------------------------ Image
Image::Image(uint32_t w, uint32_t h) : w_(w), h_(h) { require_device(); px_.alloc((size_t)w * h); Clear(); }
void Image::Clear() { CTL_HIP(hipMemset(px_.p, 0, px_.n * sizeof(ctl_pixel_data))); reduced_ = false; }
void Image::read(ctl_pixel_data* host) { CTL_HIP(hipDeviceSynchronize()); CTL_HIP(hipMemcpy(host, px_.p, px_.n * sizeof(ctl_pixel_data), hipMemcpyDeviceToHost)); }
void Image::write(const ctl_pixel_data* host) { CTL_HIP(hipMemcpy(px_.p, host, px_.n * sizeof(ctl_pixel_data), hipMemcpyHostToDevice)); reduced_ = false; }
void Image::add_samples(uint32_t n, const float* host_samples5) {
    if (!n) return;
    dbuf<float> tmp; tmp.alloc((size_t)n * 5);
    CTL_HIP(hipDeviceSynchronize());   // the frame is complete (a tracer renders on its own stream)
    CTL_HIP(hipMemcpy(tmp.p, host_samples5, (size_t)n * 5 * sizeof(float), hipMemcpyHostToDevice));
    launch_ctx lc{ nullptr, 1024 };
    launch_add_samples(lc, px_.p, w_, h_, n, tmp.p);
    CTL_HIP(hipDeviceSynchronize());
}
void Image::resolve_rgb(float splat_scale, float* host_rgb) {
    if (!rgb_.p) rgb_.alloc(px_.n * 3);
    CTL_HIP(hipDeviceSynchronize());
    launch_ctx lc{ nullptr, 1024 };
    launch_resolve_rgb(lc, px_.p, (uint32_t)px_.n, splat_scale, rgb_.p);
    CTL_HIP(hipDeviceSynchronize());
    CTL_HIP(hipMemcpy(host_rgb, rgb_.p, px_.n * 3 * sizeof(float), hipMemcpyDeviceToHost));
}

void Image::apply_pipeline(float splat_scale, uint32_t* host_rgbcol) {
    if (!out_.p) out_.alloc(px_.n);
    CTL_HIP(hipDeviceSynchronize());
    launch_ctx lc{ nullptr, 1024 };
    launch_apply_pipeline(lc, px_.p, (uint32_t)px_.n, splat_scale, out_.p);
    CTL_HIP(hipDeviceSynchronize());
    CTL_HIP(hipMemcpy(host_rgbcol, out_.p, px_.n * sizeof(uint32_t), hipMemcpyDeviceToHost));
}
void Image::write_file(float splat_scale, const char* path) {
    const std::string p(path); const size_t dot = p.find_last_of('.');
    std::string ext = dot == std::string::npos ? "" : p.substr(dot + 1);
    for (auto& c : ext) c = (char)std::tolower((unsigned char)c);
    if (ext == "hdr" || ext == "pfm") {   // toFreeImage(true): linear float data
        std::vector<float> rgb(px_.n * 3); resolve_rgb(splat_scale, rgb.data());
        if (ext == "hdr") write_hdr(p, rgb.data(), w_, h_); else write_pfm(p, rgb.data(), w_, h_);
    } else if (ext == "png") {            // toFreeImage(false): the processed (gamma-corrected, 8-bit) data
        std::vector<uint32_t> col(px_.n); apply_pipeline(splat_scale, col.data());
        std::vector<float> rgb(px_.n * 3);
        for (size_t i = 0; i < px_.n; i++) for (int c = 0; c < 3; c++) rgb[i * 3 + c] = (float)((col[i] >> (8 * c)) & 0xff) / 255.0f;
        write_png(p, rgb.data(), w_, h_, false);
    } else throw unsupported_error("Failed saving Screenshot! (only .png, .hdr and .pfm writers are built in)");
}

// ------------------------------------------------------------------------------------------------ timing
event_timer::~event_timer() { for (auto& r : used_) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); } for (auto e : free_) (void)hipEventDestroy(e); }
hipEvent_t event_timer::get() { if (!free_.empty()) { hipEvent_t e = free_.back(); free_.pop_back(); return e; } hipEvent_t e; CTL_HIP(hipEventCreate(&e)); return e; }
void event_timer::begin(hipStream_t s, int cls) { rec r{ get(), get(), cls }; CTL_HIP(hipEventRecord(r.a, s)); used_.push_back(r); }
void event_timer::end(hipStream_t s) { CTL_HIP(hipEventRecord(used_.back().b, s)); }
void event_timer::collect(double ms_out[5]) {
    for (auto& r : used_) { float ms = 0; CTL_HIP(hipEventElapsedTime(&ms, r.a, r.b)); ms_out[r.cls] += ms; free_.push_back(r.a); free_.push_back(r.b); }
    used_.clear();
}

// ------------------------------------------------------------------------------------------------ TracerBase / Tracer<PROGRESSIVE>
TracerBase::TracerBase() {
    require_device();
    m_sParameters.addEnum("BlockSamplerType", 0, { "Uniform", "Variance", "Difference", "Select" });   // Tracer.cpp:19 (BlockSamplerTypes::Uniform), an enum parameter as there
    m_sParameters.addInterval("FractionDeterministic", 2, 1, INT_MAX);   // IBlockSampler.h:157-163 (the sampler's own parameter collection there)
    m_sParameters.addInterval("FractionWeighted", 4, 1, INT_MAX);
    CTL_HIP(hipEventCreate(&start)); CTL_HIP(hipEventCreate(&stop));
    CTL_HIP(hipStreamCreate(&stream));
}
TracerBase::~TracerBase() {
    if (start) (void)hipEventDestroy(start);
    if (stop) (void)hipEventDestroy(stop);
    if (stream) (void)hipStreamDestroy(stream);
}
BlockSampler* TracerBase::getBlockSampler() {   // setCorrectBlockSampler (Tracer.cpp:89-101)
    if (w == 0xffffffffu) throw std::runtime_error("the block sampler exists once Resize was called");
    const auto type = (BlockSampler::Type)m_sParameters.getValue("BlockSamplerType");
    if (!block_sampler_ || block_sampler_->type() != type || block_sampler_->width() != w || block_sampler_->height() != h) {
        block_sampler_.reset(new BlockSampler(type, w, h));
        // an adaptive sampler starts from empty statistics, as when it owned them; a Uniform one (also created by the readers and setters outside a render) reads none
        if (var_buffer_ && type != BlockSampler::Uniform) var_buffer_->clear(stream);
    }
    block_sampler_->fraction_deterministic = m_sParameters.getValue("FractionDeterministic");
    block_sampler_->fraction_weighted = m_sParameters.getValue("FractionWeighted");
    return block_sampler_.get();
}
PixelVarianceBuffer* TracerBase::ensureVarianceBuffer() {
    if (w == 0xffffffffu) return nullptr;
    if (!var_buffer_ || var_buffer_->width() != w || var_buffer_->height() != h) var_buffer_.reset(new PixelVarianceBuffer(w, h));
    return var_buffer_.get();
}
void TracerBase::setPixelVariance(bool on) {
    if (!isMultiPass()) throw unsupported_error("setPixelVariance: a Tracer<false> takes one sample per pixel and keeps no PixelVarianceBuffer");
    if (on && shard_world > 1) throw std::runtime_error("setPixelVariance: the pixel variance needs the whole frame on one rank");
    pixel_variance_on_ = on;
    if (!on && !block_sampler_) var_buffer_.reset();
}
const PixelVarianceBuffer* TracerBase::getPixelVarianceBuffer() { return (pixel_variance_on_ || block_sampler_ || var_buffer_) ? ensureVarianceBuffer() : nullptr; }
void TracerBase::readPixelVariance(float* host_out) {
    const PixelVarianceBuffer* vb = getPixelVarianceBuffer();
    if (!vb) throw std::runtime_error("readPixelVariance: the tracer keeps no pixel variance (setPixelVariance is off, or Resize was not called)");
    dbuf<float> tmp; tmp.alloc((size_t)w * h);
    vb->compute_variance(tmp.p, stream);
    CTL_HIP(hipMemcpyAsync(host_out, tmp.p, (size_t)w * h * sizeof(float), hipMemcpyDeviceToHost, stream));
    CTL_HIP(hipStreamSynchronize(stream));
}
void TracerBase::setSamplerTables(const float* t1, const float* t2) {
    const size_t n1 = (size_t)CTL_SAMPLER_NUM_SEQUENCES * CTL_SAMPLER_SEQUENCE_LENGTH;
    user_t1.assign(t1, t1 + n1); user_t2.assign(t2, t2 + 2 * n1); have_user_tables = true;
}
void TracerBase::getKernelStats(ctl_tracer_stats& s) const {
    std::memset(&s, 0, sizeof(s));
    s.rays_last_pass = m_uLastNumRaysTraced; s.rays_total = m_uAccNumRaysTraced; s.seconds_last_pass = m_fLastRuntime; s.seconds_total = m_fAccRuntime;
    s.passes_done = m_uPassesDone; s.ms_raygen = kernel_ms[0]; s.ms_intersect = kernel_ms[1]; s.ms_shade = kernel_ms[2]; s.ms_intersect_any = kernel_ms[3]; s.ms_fused = kernel_ms[4];
    s.intersect_rays = intersect_rays; s.intersect_launches = intersect_launches; s.shadow_rays = shadow_rays; s.shadow_launches = shadow_launches; s.fused_launches = fused_launches; s.fused_shadow_rays = fused_shadow_rays; s.fused_closest_rays = fused_closest_rays;
    s.closest_counts = closest_counts; s.any_counts = any_counts;
}

// Tracer<true>::DoPass (Kernel/Tracer.h:209-248), generalised to n passes per call.  As in the reference the host
// regenerates the sampling tables once per pass (UpdateKernel -> SamplingSequenceGeneratorHost::Compute); here the
// generation of pass k+1 overlaps the GPU work of pass k because nothing in a pass synchronises with the host.
template <bool PROGRESSIVE> void Tracer<PROGRESSIVE>::ensureTableRing(unsigned int B) {
    const size_t n1 = (size_t)CTL_SAMPLER_NUM_SEQUENCES * CTL_SAMPLER_SEQUENCE_LENGTH, n2 = n1 * 2;
    const unsigned int ring = kTableRing;
    if (d_t1.n < n1 * ring * B) { d_t1.alloc(n1 * ring * B); d_t2.alloc(n2 * ring * B); }
    if (h_cap < n1 * ring) {   // pinned staging for the one pass per batch whose tables the caller may hand in (setSamplerTables)
        if (h_t1) { (void)hipHostFree(h_t1); (void)hipHostFree(h_t2); h_t1 = h_t2 = nullptr; }
        CTL_HIP(hipHostMalloc((void**)&h_t1, n1 * ring * sizeof(float))); CTL_HIP(hipHostMalloc((void**)&h_t2, n2 * ring * sizeof(float)));
        h_cap = n1 * ring;
    }
    if (slot_done.empty()) { slot_done.resize(ring); for (auto& e : slot_done) CTL_HIP(hipEventCreate(&e)); }
    if (starts_cap < (size_t)ring * B) {
        if (h_starts) { (void)hipHostFree(h_starts); h_starts = nullptr; }
        CTL_HIP(hipHostMalloc((void**)&h_starts, (size_t)ring * B * sizeof(sequence_generator::pass_start)));
        d_starts.alloc((size_t)ring * B * sizeof(sequence_generator::pass_start) / sizeof(uint32_t));
        starts_cap = (size_t)ring * B;
    }
    if (!d_jumps.p) {
        const std::vector<uint32_t>& J = sequence_generator::chunk_jump_matrices();
        d_jumps.alloc(J.size()); CTL_HIP(hipMemcpy(d_jumps.p, J.data(), J.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
}
void TracerBase::setDepthBuffer(float*, unsigned int, unsigned int) { throw unsupported_error("setDepthBuffer: this tracer is not an IDepthTracer (only the WavefrontPathTracer is, WavefrontPathTracer.h:24)"); }
// The sampler tables of the nb passes of ring slot `slot` (batches of B passes): the caller's tables (setSamplerTables) serve the first of them, the tracer's XORWOW
// stream the rest (UpdateKernel -> GenerateNewRandomSequences, Kernel/TraceHelper.cu:182-185).  One stream as in the reference (Kernel/Sampler.h:57-85): the host only
// advances it (one GF(2) jump per pass); the tables are written in HBM by k_sequence_fill — 256 lanes per pass, each two jumps and 1440 draws from the pass's start
// state — in the time the host threads needed for one pass, and without the 1.5 MB-per-pass upload (measured: 1.9 ms at the head of every 20-pass call -> 0.1 ms).
// The slot's staging must be idle: the batch that last used it has finished.
template <bool PROGRESSIVE> void Tracer<PROGRESSIVE>::stageTables(unsigned int slot, unsigned int B, unsigned int nb) {
    const size_t n1 = (size_t)CTL_SAMPLER_NUM_SEQUENCES * CTL_SAMPLER_SEQUENCE_LENGTH, n2 = n1 * 2;
    float* dst1 = d_t1.p + (size_t)slot * B * n1; float* dst2 = d_t2.p + (size_t)slot * B * n2;
    unsigned int j0 = 0;
    if (have_user_tables) {
        float* a = h_t1 + (size_t)slot * n1; float* b = h_t2 + (size_t)slot * n2;
        std::memcpy(a, user_t1.data(), n1 * 4); std::memcpy(b, user_t2.data(), n2 * 4); have_user_tables = false; j0 = 1;
        CTL_HIP(hipMemcpyAsync(dst1, a, n1 * 4, hipMemcpyHostToDevice, stream));
        CTL_HIP(hipMemcpyAsync(dst2, b, n2 * 4, hipMemcpyHostToDevice, stream));
    }
    if (nb > j0) {
        sequence_generator::pass_start* hs = h_starts + (size_t)slot * B;
        uint32_t* ds = d_starts.p + (size_t)slot * B * (sizeof(sequence_generator::pass_start) / sizeof(uint32_t));
        m_SamplingSequenceGenerator.take_pass_starts(nb - j0, hs);
        CTL_HIP(hipMemcpyAsync(ds, hs, (size_t)(nb - j0) * sizeof(sequence_generator::pass_start), hipMemcpyHostToDevice, stream));
        launch_sequence_fill(stream, d_jumps.p, ds, nb - j0, dst1 + (size_t)j0 * n1, dst2 + (size_t)j0 * n2);
    }
}
template <bool PROGRESSIVE> void Tracer<PROGRESSIVE>::Debug(Image* I, unsigned int x, unsigned int y, float rgb[3]) {
    if (!m_pScene) throw std::runtime_error("Debug: InitializeScene was not called");
    if (w == 0xffffffffu) throw std::runtime_error("Debug: Resize was not called");
    if (x >= w || y >= h) throw std::runtime_error("Debug: pixel outside the film");
    // UpdateKernel(scene, generator): one more set of tables is drawn, into slot 0 of the ring
    ensureTableRing(std::max(1u, passBatch()));
    for (auto e : slot_done) CTL_HIP(hipEventSynchronize(e));
    stageTables(0, 1, 1);
    float out[3] = { 0, 0, 0 };
    DebugInternal(I, x, y, d_t1.p, d_t2.p, out);
    CTL_HIP(hipStreamSynchronize(stream));
    if (rgb) { rgb[0] = out[0]; rgb[1] = out[1]; rgb[2] = out[2]; }
}
template <bool PROGRESSIVE> void Tracer<PROGRESSIVE>::DoPasses(Image* I, bool a_NewTrace, unsigned int n) {
    if (!m_pScene) throw std::runtime_error("DoPass: InitializeScene was not called");
    if (w == 0xffffffffu) throw std::runtime_error("DoPass: Resize was not called");
    if (I->getWidth() != w || I->getHeight() != h) throw std::runtime_error("DoPass: image size differs from the tracer size");
    if (n == 0) return;
    if (a_NewTrace || !PROGRESSIVE) { m_uPassesDone = 0; m_uAccNumRaysTraced = 0; m_fAccRuntime = 0; if (PROGRESSIVE) I->Clear(); }   // Tracer<false> clears before every pass
    // a block sampler that does not simply take every block once decides pass by pass, from the frame so far (Tracer.h:209-248).  Tracer<false> has none:
    // BlockSamplerType is accepted there and changes nothing, as in the reference
    BlockSampler* bs = PROGRESSIVE && (m_sParameters.getValue("BlockSamplerType") != 0 || block_sampler_) ? getBlockSampler() : nullptr;
    const bool adaptive = bs && !bs->every_block_once();
    if (adaptive && shard_world > 1) throw std::runtime_error("block samplers other than Uniform need the whole frame on one rank");
    // the PixelVarianceBuffer is updated after every pass (Tracer.h:233-237) where an adaptive sampler reads it or setPixelVariance asked for it
    const bool per_pass = adaptive || (PROGRESSIVE && pixel_variance_on_);
    if (per_pass && shard_world > 1) throw std::runtime_error("the pixel variance needs the whole frame on one rank");
    PixelVarianceBuffer* vb = (bs || per_pass) ? ensureVarianceBuffer() : nullptr;
    if (a_NewTrace) { if (bs) bs->start_new_rendering(); if (vb) vb->clear(stream); }
    const size_t n1 = (size_t)CTL_SAMPLER_NUM_SEQUENCES * CTL_SAMPLER_SEQUENCE_LENGTH, n2 = n1 * 2;
    // passes are rendered in batches of `B` (one wavefront carries the paths of B passes; each path uses its own pass's
    // tables), B chosen so that a launch holds enough paths to fill 256 CUs even when a rank owns 1/8 of the tiles
    // a tracer that can update the variance between the passes of a batch keeps its batches (the adaptive samplers decide pass by pass in any case)
    const bool var_in_batch = per_pass && !adaptive && updatesVarianceInBatch(std::min(passBatch(), n));
    const unsigned int B = (per_pass && !var_in_batch) ? 1u : std::min(passBatch(), n);
    const unsigned int ring = kTableRing;   // batches in flight; slot reuse is guarded by an event per slot
    ensureTableRing(B);
    for (int i = 0; i < 5; i++) kernel_ms[i] = 0;
    intersect_rays = intersect_launches = shadow_rays = shadow_launches = fused_launches = fused_shadow_rays = fused_closest_rays = 0;
    CTL_HIP(hipEventRecord(start, stream));
    unsigned int batch_idx = 0;
    for (unsigned int k = 0; k < n; batch_idx++) {
        const unsigned int nb = std::min(B, n - k), slot = batch_idx % ring;
        if (batch_idx >= ring) CTL_HIP(hipEventSynchronize(slot_done[slot]));   // the batch that last used this slot has finished
        if (!PROGRESSIVE) { m_uPassesDone = 0; I->Clear(); }   // every pass of a non-progressive tracer is a new trace (B = 1); the previous pass ended with a synchronisation
        stageTables(slot, B, nb);
        m_uPassesDone += nb;
        std::vector<unsigned char> block_counts;
        pass_block_counts_ = nullptr; pass_max_block_count_ = 1;
        if (adaptive) {
            bs->counts(block_counts);
            pass_block_counts_ = bs->upload_counts(block_counts, stream);
            pass_max_block_count_ = 0; pass_paths_ = 0;
            for (unsigned char c : block_counts) { pass_max_block_count_ = std::max<uint32_t>(pass_max_block_count_, c); pass_paths_ += (uint64_t)c * 4096u; }
        }
        batch_variance_ = var_in_batch ? vb->device() : nullptr; batch_first_pass_ = m_uPassesDone - nb;
        DoRender(I, d_t1.p + (size_t)slot * B * n1, d_t2.p + (size_t)slot * B * n2, nb);
        if (per_pass && !var_in_batch) vb->add_pass(I->device(), getSplatScale(), pass_block_counts_, stream);   // PixelVarianceBuffer::AddPass: the sampled blocks (no counts: every block once)
        if (adaptive) bs->add_pass(*vb, block_counts, stream);                                  // IBlockSampler::AddPass; synchronises
        CTL_HIP(hipEventRecord(slot_done[slot], stream));
        k += nb;
    }
    CTL_HIP(hipEventRecord(stop, stream));
    CTL_HIP(hipEventSynchronize(stop));
    CTL_HIP(hipGetLastError());
    float ms = 0; CTL_HIP(hipEventElapsedTime(&ms, start, stop));
    timer.collect(kernel_ms);
    m_fLastRuntime = ms / 1000.0f;
    takeRayCounts(intersect_rays, shadow_rays);
    m_uLastNumRaysTraced = intersect_rays + shadow_rays;
    m_fAccRuntime += m_fLastRuntime; m_uAccNumRaysTraced += m_uLastNumRaysTraced;
}
template class Tracer<true>;
template class Tracer<false>;

// ------------------------------------------------------------------------------------------------ WavefrontPathTracer
WavefrontPathTracer::WavefrontPathTracer() {
    // WavefrontPathTracer.h:29-39
    m_sParameters.addBool("Direct", true);
    m_sParameters.addInterval("MaxPathLength", 50, 1, INT_MAX);
    m_sParameters.addInterval("RRStartDepth", 5, 1, INT_MAX);
    // build-specific: passes rendered together in one wavefront; 0 = choose so that a launch carries ~64 M paths (passBatch())
    m_sParameters.addInterval("PassBatch", 0, 0, 128);
    // build-specific: run Material::AlphaTest on candidate hits.  Off = the reference's wavefront tracer (its intersectKernel has no
    // alpha test, only the single-ray traceRay of the megakernel integrators does, TraceHelper.cu:135-153)
    m_sParameters.addBool("AlphaTest", false);
    // build-specific: a scene that needs the full feature set is shaded by one launch per MODEL CLASS present in it (shade_class_a/b/p/c.hip: basic models + misses / the other single-layer
    // models / rough plastic / the nesting models), each register-allocated for its own models, instead of the one kernel that carries all fifteen (k_shade_full: 104 spilled registers).  Needs the
    // BSDF model per hit from the closest-hit traversal (flattened BVH).  false = k_shade_full.
    // Not an experiment arm: k_shade_full runs by itself whenever the traversal leaves no key (two-level scene, counting batch, >= 2^27 triangles); the parameter lets a test hold both paths to one frame on one scene
    m_sParameters.addBool("ShadeByModelClass", true);
    // build-specific: trace a bounce's path rays and the previous bounce's shadow rays in one persistent launch (k_intersect_pair).  Every traversal launch
    // pays ~0.4 ms of ramp and drain whatever its size (tools/shard_time_probe.py: 4 % of the time at 20 passes per launch on one GPU, a quarter on one rank
    // of eight); the fused launch fills the drain of the first set with the second: +2 % on the whole frame, +7 % on a rank of eight.  false = two launches.
    // Not an experiment arm: the unfused launches run by themselves when counting or with Direct = false; the parameter lets a test hold both paths to one frame on one scene
    m_sParameters.addBool("FuseTraversal", true);
    // build-specific: whose per-path rules the shading stage follows.  PathTrace (default): the reference's deterministic megakernel PathTrace<DIRECT> (PathTracer.cu:10-113),
    // what the oracle pins and the PathTracer plugin renders.  Wavefront: pathIterateKernel's own rules (WavefrontPathTracer.cu:51-164) — Russian roulette before sampling at
    // pathDepth >= RRStartDepth, no sampling / next-event estimation at the last bounce, sampleEmitterDirect with one 2-D sample, 16-bit previous normal, the
    // t >= dDist (1 - eps) shadow rule: what the reference's PT_Wave converges to (darker than PT by the last bounce's direct term, and fewer rays)
    m_sParameters.addEnum("PathSemantics", 0, { "PathTrace", "Wavefront" });
    // build-specific: hit barycentrics through the 16-bit pair of the reference's traversal result (Kernel/TraceHelper.cu:722-731); off = full floats (single-ray traceRay)
    m_sParameters.addBool("U16Barycentrics", false);
    m_sParameters.addInterval("OrderedAccumulationMaxMB", 4096, 0, 1 << 20);   // build-specific: largest stage of the ordered accumulation (MB of HBM); a batch that needs more accumulates with atomics
    // build-specific: render participating media.  false (default): the plugin has no medium code in its launches and refuses a scene that has media; true: k_medium_stage
    // (medium_stage.hip) runs the medium half of PathTrace (PathTracer.cu:17-58) in front of every depth's shade launch and the media build of the shade kernel
    // (shade_full_media*.hip) attenuates the surface NEE — for a scene whose volume table is empty the pass launches exactly the kernels it launches with false.
    // PathTrace rules only: refused together with PathSemantics = Wavefront
    m_sParameters.addBool("ParticipatingMedia", false);
    // build-specific: ray differentials at the first hit and filtered image textures there, as PathTrace has them (PathTracer.cu:60-61, Texture.cu:15-29, MIPMap.cu:193-278).
    // false (default): every lookup reads level 0 and the pass launches what it always launched; true: the vertices of depth 1 are shaded by k_shade_full_partials
    // (shade_full_partials.hip) — for a scene without image textures the pass launches exactly the kernels it launches with false.
    // PathTrace rules only: refused together with PathSemantics = Wavefront, and together with ParticipatingMedia
    m_sParameters.addBool("TextureFiltering", false);
    m_sParameters.addBool("OrderedAccumulation", true);  // build-specific: finished paths are staged per (pass, pixel) and added to the frame in pass order (kernels.h pass_params::stage); false = four float atomics per path as Image::AddSample does
    grid_blocks = persistent_grid_blocks();
}
void WavefrontPathTracer::check_media(const Scene* s) const {
    if (m_sParameters.getValue("ParticipatingMedia") == 0) { if (s) s->refuse_volumes("WavefrontPathTracer"); return; }
    if (m_sParameters.getValue("PathSemantics") == 1)
        throw unsupported_error("WavefrontPathTracer: ParticipatingMedia = true with PathSemantics = Wavefront is not supported: pathIterateKernel has no medium rules; participating media are rendered under PathSemantics = PathTrace");
}
void WavefrontPathTracer::check_texture_filtering() const {
    if (m_sParameters.getValue("TextureFiltering") == 0) return;
    if (m_sParameters.getValue("PathSemantics") == 1)
        throw unsupported_error("WavefrontPathTracer: TextureFiltering = true with PathSemantics = Wavefront is not supported: pathIterateKernel has no ray differentials; first-hit texture filtering is rendered under PathSemantics = PathTrace");
    if (m_sParameters.getValue("ParticipatingMedia") != 0)
        throw unsupported_error("WavefrontPathTracer: TextureFiltering = true with ParticipatingMedia = true is not supported: the media build of the shade kernel has no ray differentials; the PathTracer plugin renders participating media with filtered textures");
}
float4* WavefrontPathTracer::new_f4(size_t n) { f4_.emplace_back(new dbuf<float4>()); f4_.back()->alloc(n); return f4_.back()->p; }

// a ray's slot number travels in 31 bits (bit 31 of the traversal kernels' ray word is the "hit found" flag, traverse_flat.h) and the batch position of a path in 8.
// Checked BEFORE any state changes (Resize, DoRender, reservePasses): a refused size or batch leaves the tracer as it was.
static void check_batch(uint64_t n_local, unsigned int batch, const char* who) {
    if (n_local * std::max(1u, batch) >= (1ull << 31) || batch > 255u)
        throw std::runtime_error(std::string("WavefrontPathTracer::") + who + ": " + std::to_string(n_local) + " pixels x " + std::to_string(batch) + " passes per wavefront exceed the 2^31 ray slots (or 255 passes) of a batch: lower PassBatch");
}
// the stage of the ordered accumulation for a batch of b passes, or nullptr (parameter off, over OrderedAccumulationMaxMB, allocation failed).  Also called by reservePasses:
// the allocation (663 MB for 20 passes of a 1080p frame) then happens before the render, not inside its first call.
float4* WavefrontPathTracer::ensureStage(unsigned int b) {
    if (m_sParameters.getValue("OrderedAccumulation") == 0 || n_local_pixels == 0) return nullptr;
    const size_t need = (size_t)n_local_pixels * b;
    if (need * sizeof(float4) > (size_t)m_sParameters.getValue("OrderedAccumulationMaxMB") << 20) return nullptr;
    if (stage_.n < need) {
        try { stage_.alloc(need); CTL_HIP(hipMemsetAsync(stage_.p, 0, need * sizeof(float4), stream)); }
        catch (const std::exception&) { stage_.free(); (void)hipGetLastError(); }
    }
    return stage_.n >= need ? stage_.p : nullptr;
}
bool WavefrontPathTracer::updatesVarianceInBatch(unsigned int b) {
    if (w == 0xffffffffu) return false;
    growBatch(b, "DoPasses");
    if (!ensureStage(b)) return false;
    // the second stage of such a batch (kernels.h pass_params::stray_stage); both within OrderedAccumulationMaxMB, or the passes are rendered one per launch
    const size_t need = (size_t)n_local_pixels * b;
    if (2 * need * sizeof(float4) > (size_t)m_sParameters.getValue("OrderedAccumulationMaxMB") << 20) return false;
    if (stray_stage_.n < need) {
        try { stray_stage_.alloc(need); CTL_HIP(hipMemsetAsync(stray_stage_.p, 0, need * sizeof(float4), stream)); }
        catch (const std::exception&) { stray_stage_.free(); (void)hipGetLastError(); return false; }
    }
    return true;
}
void WavefrontPathTracer::growBatch(unsigned int b, const char* who) {
    if (w == 0xffffffffu || (uint64_t)n_local_pixels * b <= capacity) return;
    check_batch(n_local_pixels, b, who);
    alloc_batch_ = b; Resize(w, h);
}
void WavefrontPathTracer::Resize(unsigned int _w, unsigned int _h) {
    const uint64_t new_local = shard_pixel_count(_w, _h, shard_rank, shard_world);
    check_batch(new_local, 1, "Resize");
    if (new_local * alloc_batch_ >= (1ull << 31)) alloc_batch_ = 1;   // a batch reserved for a smaller frame / shard: the queues grow again with the next render's batch
    Tracer<true>::Resize(_w, _h);
    // DoubleRayBuffer(w*h, w*h) (WavefrontPathTracer.h:59) — here per rank: its tile shard's pixels
    n_local_pixels = shard_pixel_count(_w, _h, shard_rank, shard_world);
    capacity = n_local_pixels * std::max(1u, alloc_batch_);   // grown by DoRender when a larger batch arrives
    f4_.clear();
    for (int b = 0; b < 2; b++) {
        path_soa& p = Q.path[b];
        p.ray_o = new_f4(capacity); p.ray_d = new_f4(capacity); p.thr = new_f4(capacity); p.rad = new_f4(capacity); p.nor = new_f4(capacity); p.pend = new_f4(capacity);
        px_[b].alloc(capacity); p.px = px_[b].p;
        Q.sh_o[b] = new_f4(capacity); Q.sh_d[b] = new_f4(capacity); occ_[b].alloc(capacity); Q.sh_occ[b] = occ_[b].p;
    }
    Q.hit = new_f4(capacity); hit_node_.alloc(capacity); Q.hit_node = hit_node_.p;
    Q.fin.rad = new_f4(capacity); Q.fin.dir = new_f4(capacity); Q.fin.px = new_f4(capacity);
    stats_.alloc(14); Q.stats = stats_.p; CTL_HIP(hipMemset(stats_.p, 0, 14 * sizeof(unsigned long long)));
    Q.capacity = capacity;
    class_order_.free(); for (int c = 0; c < 5; c++) Q.class_order[c] = nullptr;   // the model-class lists (20 B per slot) are allocated by the first render that shades by class
    mat_key_.alloc(capacity); Q.mat_key = mat_key_.p;
    counts_.free(); work_.free(); class_counts_.free(); stage_.free(); stray_stage_.free();
    for (int b = 0; b < 2; b++) { mrec_[b].free(); Q.path[b].mrec = nullptr; }   // allocated by the first render with participating media (DoRender)
}

// stats: [0] path rays, [1] shadow rays, [2..6] closest-hit traversal counts, [7..11] any-hit traversal counts
void WavefrontPathTracer::takeRayCounts(uint64_t& path_rays, uint64_t& shadow_rays_) {
    unsigned long long r[14];   // [12]: shadow rays of the last bounce, [13]: path rays of the first (never part of a fused launch)
    CTL_HIP(hipMemcpy(r, stats_.p, sizeof(r), hipMemcpyDeviceToHost));
    CTL_HIP(hipMemset(stats_.p, 0, sizeof(r)));
    path_rays = r[0]; shadow_rays_ = r[1];
    fused_shadow_rays = fused_launches ? r[1] - r[12] : 0; fused_closest_rays = fused_launches ? r[0] - r[13] : 0;
    closest_counts = ctl_traversal_counts{ r[2], r[3], r[4], r[5], r[6] };
    any_counts = ctl_traversal_counts{ r[7], r[8], r[9], r[10], r[11] };
}

// WavefrontPathTracer::DoRender (Integrators/PseudoRealtime/WavefrontPathTracer.cu:166-191): ray generation, then per
// bounce {intersect path rays, intersect the previous bounce's shadow rays, shade}.  Queue lengths stay in HBM, so
// the whole pass is enqueued without any host round trip (the reference synchronises 3x per bounce).
unsigned int WavefrontPathTracer::passBatch() const {
    const int v = m_sParameters.getValue("PassBatch");
    if (v > 0) return (unsigned int)v;
    if (w == 0xffffffffu) return 1;
    const uint64_t per_pass = shard_pixel_count(w, h, shard_rank, shard_world);
    if (per_pass == 0) return 1;   // more ranks than 64x64 tiles: this rank owns nothing and its passes are empty launches
    // Paths per launch.  Measured on MI355X (tools/passbatch_probe.py, synthetic-SM 1080p): 2 M paths per launch 1.04 Grays/s, 4 M 1.50, 8 M 1.88,
    // 33 M 2.33, 67 M 2.45, 134 M 2.51 — the persistent traversal kernels keep 524 k rays in flight and every launch pays a ramp and a
    // tail of a few hundred us, so small launches are mostly ramp and tail.  ~350 B of queue state per path: 64 M paths = 22 GB of the 288 GB.
    const uint64_t target = 64u << 20;
    return (unsigned int)std::min<uint64_t>(128, std::max<uint64_t>(1, (target + per_pass - 1) / per_pass));
}

void WavefrontPathTracer::DoRender(Image* I, const float* d_t1p, const float* d_t2p, unsigned int n_batch) {
    check_media(m_pScene); check_texture_filtering();
    growBatch(n_batch, "DoRender");   // the queues grow to the largest batch asked for
    // participating media: the table is read per pass — ctl_scene_update may have changed the media since InitializeScene.  An empty table: the launches of a scene without media
    const bool media_on = m_sParameters.getValue("ParticipatingMedia") != 0;
    const vol::table V = media_on ? m_pScene->volume_table() : vol::table{};
    const bool media = V.n != 0;
    for (int b = 0; b < 2; b++) {   // path_soa::mrec exists only while the parameter is on; never cleared: k_medium_stage starts every camera path from the zero record
        if (!media_on) mrec_[b].free(); else if (media && mrec_[b].n < capacity) mrec_[b].alloc(capacity);
        Q.path[b].mrec = mrec_[b].p;
    }
    const int maxPathLength = m_sParameters.getValue("MaxPathLength"), rrStart = m_sParameters.getValue("RRStartDepth");
    const bool direct = m_sParameters.getValue("Direct") != 0;
    const size_t n_counts = (size_t)(maxPathLength + 2) * 4, n_work = (size_t)2 * (maxPathLength + 2);
    const size_t n_class = (size_t)(maxPathLength + 2) * 8;
    if (counts_.n < n_counts) { counts_.alloc(n_counts); work_.alloc(n_work); class_counts_.alloc(n_class); }
    Q.counts = counts_.p; Q.work = work_.p; Q.class_counts = class_counts_.p;
    const dev_scene& S = m_pScene->S;
    const launch_ctx lc{ stream, grid_blocks, m_sParameters.getValue("AlphaTest") != 0 && S.alpha_maps != 0 };
    pass_params P{};
    P.t1 = d_t1p; P.t2 = (const float2*)d_t2p;
    P.batch = n_batch;
    P.width = w; P.height = h; P.tile_rank = shard_rank; P.tile_world = shard_world; P.n_local_pixels = n_local_pixels;
    P.direct = direct ? 1 : 0; P.max_path_length = maxPathLength; P.rr_start_depth = rrStart;
    P.block_counts = pass_block_counts_; P.max_block_count = pass_max_block_count_;
    P.wavefront_rules = m_sParameters.getValue("PathSemantics") == 1 ? 1 : 0; P.u16_bary = m_sParameters.getValue("U16Barycentrics") != 0 ? 1 : 0;
    // first-hit texture filtering: only an image texture can see the partials (material textures, normal maps, textured area lights: all behind kShadeImageTextures), so a scene
    // without one keeps its usual depth-1 launches — the frame is the default one by construction
    P.tex_partials = (m_sParameters.getValue("TextureFiltering") != 0 && (S.shade_features & kShadeImageTextures)) ? 1 : 0;
    P.depth_buffer = depth_buffer_; P.depth_w = depth_w_; P.depth_h = depth_h_; P.depth_near = m_pScene->near_depth; P.depth_far = m_pScene->far_depth;
    // ordered accumulation (kernels.h pass_params::stage): one staged sample per (pass of the batch, pixel), added to the frame in pass order after the last bounce
    // The stage covers THIS RANK'S tiles only (n_local_pixels slots per pass of the batch, 16 B each: 663 MB for 20 passes of a whole 1080p frame, an eighth of that on a rank
    // of eight).  It is an optimisation, not a requirement: past OrderedAccumulationMaxMB (default 4096) or when the allocation fails the paths fall back to Image::AddSample's
    // four float atomics — same sums, hardware order.
    P.stage = nullptr; P.stage_stride = (size_t)n_local_pixels;
    if (!pass_block_counts_) P.stage = ensureStage(n_batch);
    P.stray_stage = (batch_variance_ && P.stage) ? stray_stage_.p : nullptr;
    if (pass_block_counts_ && pass_paths_ > capacity) throw std::runtime_error("ray queue overflow: the block sampler asks for more samples in one pass than the queues hold (DoubleRayBuffer.h:86-89)");
    CTL_HIP(hipMemsetAsync(class_counts_.p, 0, n_class * sizeof(uint32_t), stream));
    CTL_HIP(hipMemsetAsync(counts_.p, 0, n_counts * sizeof(uint32_t), stream));
    CTL_HIP(hipMemsetAsync(work_.p, 0, n_work * sizeof(uint32_t), stream));
    timer.begin(stream, 0); launch_raygen(lc, S, Q, P); timer.end(stream);
    auto shadow_pass = [&](int d) {   // any-hit intersection of the shadow rays emitted at depth d
        timer.begin(stream, 3);
        if (counting) launch_intersect_count(lc, S, Q.sh_o[d & 1], Q.sh_d[d & 1], &Q.counts[d * 4 + 1], &Q.work[2 * d + 3], nullptr, nullptr, Q.sh_occ[d & 1], 1, Q.stats + 7);
        else launch_intersect_any(lc, S, Q.sh_o[d & 1], Q.sh_d[d & 1], &Q.counts[d * 4 + 1], &Q.work[2 * d + 3], Q.sh_occ[d & 1]);
        timer.end(stream);
        shadow_launches++;
    };
    const bool fuse = !counting && direct && m_sParameters.getValue("FuseTraversal") != 0;
    // closest-hit traversals of a flattened scene leave the BSDF model of every hit in Q.mat_key (device_scene.h hit_key_out) for the shade kernel's regrouping and the model-class lists;
    // the counting kernels do without
    // (with media the one media build of the full kernel shades every vertex: no model classes, and its regrouping keys itself)
    P.model_classes = (!media && S.shade_features != 0 && m_sParameters.getValue("ShadeByModelClass") != 0) ? 1 : 0;
    dev_scene Sk = S; Sk.hit_key_out = (!media && S.flat_leaf_keys && (S.shade_features == 0 || P.model_classes) && !counting) ? Q.mat_key : nullptr;   // (k_shade_full keys its regrouping by model AND material index)
    P.key_from_traversal = Sk.hit_key_out ? 1 : 0;
    if (!P.key_from_traversal) P.model_classes = 0;
    if (P.model_classes && !class_order_.p) { class_order_.alloc((size_t)capacity * 5); for (int c = 0; c < 5; c++) Q.class_order[c] = class_order_.p + (size_t)c * capacity; }
    for (int depth = 1; depth <= maxPathLength; depth++) {
        const int cur = (depth - 1) & 1;
        if (fuse && depth > 1) {   // path rays of this bounce + shadow rays of the previous one in one launch
            const int d = depth - 1;
            timer.begin(stream, 4);
            launch_intersect_pair(lc, Sk, Q.path[cur].ray_o, Q.path[cur].ray_d, &Q.counts[(depth - 1) * 4 + 0], &Q.work[2 * depth], Q.hit, Q.hit_node,
                                  Q.sh_o[d & 1], Q.sh_d[d & 1], &Q.counts[d * 4 + 1], &Q.work[2 * d + 3], Q.sh_occ[d & 1]);
            timer.end(stream);
            fused_launches++;
            timer.begin(stream, 2);
            launch_finalize(lc, Q, P, depth - 1, I->device());
            if (media) launch_medium_stage(lc, S, Q, P, V, depth, I->device());
            launch_shade(lc, S, Q, P, depth, I->device(), media ? &V : nullptr);
            timer.end(stream);
            continue;
        }
        timer.begin(stream, 1);
        if (counting) launch_intersect_count(lc, S, Q.path[cur].ray_o, Q.path[cur].ray_d, &Q.counts[(depth - 1) * 4 + 0], &Q.work[2 * depth], Q.hit, Q.hit_node, nullptr, 0, Q.stats + 2);
        else launch_intersect_closest(lc, Sk, Q.path[cur].ray_o, Q.path[cur].ray_d, &Q.counts[(depth - 1) * 4 + 0], &Q.work[2 * depth], Q.hit, Q.hit_node);
        timer.end(stream);
        intersect_launches++;
        if (depth > 1 && direct) shadow_pass(depth - 1);
        timer.begin(stream, 2);
        if (depth > 1 && direct) launch_finalize(lc, Q, P, depth - 1, I->device());
        if (media) launch_medium_stage(lc, S, Q, P, V, depth, I->device());   // the medium half of PathTrace for this depth's vertices: Q.hit is written, the previous depth's shadow rays are resolved
        launch_shade(lc, S, Q, P, depth, I->device(), media ? &V : nullptr);
        timer.end(stream);
    }
    if (direct) {
        shadow_pass(maxPathLength);
        timer.begin(stream, 2); launch_finalize(lc, Q, P, maxPathLength, I->device()); timer.end(stream);
    }
    if (batch_variance_ && !P.stage) throw std::runtime_error("WavefrontPathTracer::DoRender: the batch's variance update needs the stage of the ordered accumulation");
    if (P.stage) { timer.begin(stream, 2); launch_resolve_stage(lc, P.stage, P.stage_stride, n_batch, I->device(), w, h, shard_rank, shard_world, batch_variance_, P.stray_stage, batch_first_pass_); timer.end(stream); }
    launch_accumulate_stats(lc, Q, maxPathLength);
}

} // namespace ctl
