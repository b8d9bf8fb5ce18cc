// scene_update.hip — ctl_scene_desc_diff and ctl_scene_update: what UpdateKernel(m_pScene) does in the reference for a host that moved the camera, edited a
// material or called DynamicScene::SetNodeTransform (Kernel/Tracer.h:121,229).  The scene keeps a host copy of the description it was made from — the small
// arrays whole, the geometry arrays (triangles, Woop rows, mesh BVHs, texels, transmittance tables) as a 128-bit hash — and an update applies the blocks of the
// upload (tracer.hip) whose part of the description differs.  A transform change refits the flattened Q4 tree on the device (flat_refit.hip).
#include "tracer.h"
#include "flatten.h"
#include "flat_refit.h"
#include "scene_checks.h"
#include "scene_cache.h"
#include "mitsuba_loader.h"   // unsupported_error
#include <cstring>

namespace ctl {

void scene_geometry_hash(const ctl_scene_desc& d, uint64_t out[2]) {
    content_hash H;
    H.add_value(d.n_tri_data); if (d.n_tri_data) H.add(d.tri_data, (size_t)d.n_tri_data * sizeof(ctl_triangle_data));
    H.add_value(d.n_woop); if (d.n_woop) { H.add(d.woop, (size_t)d.n_woop * sizeof(ctl_woop_tri)); H.add(d.woop_index, (size_t)d.n_woop * sizeof(ctl_woop_index)); }
    H.add_value(d.n_bvh_nodes); if (d.n_bvh_nodes) H.add(d.bvh_nodes, (size_t)d.n_bvh_nodes * sizeof(ctl_bvh_node));
    for (uint32_t i = 0; i < d.n_images; i++) if (d.images[i].texels) H.add(d.images[i].texels, (size_t)d.images[i].width * d.images[i].height * 4);
    const int have_rt = d.rough_transmittance ? 1 : 0; H.add_value(have_rt);
    if (d.rough_transmittance) for (int i = 0; i < 3; i++) {
        const ctl_rough_transmittance& t = d.rough_transmittance[i];
        H.add_value(t.eta_samples); H.add_value(t.alpha_samples); H.add_value(t.theta_samples); H.add_value(t.eta_min); H.add_value(t.eta_max); H.add_value(t.alpha_min); H.add_value(t.alpha_max);
        const int have = (t.trans && t.diff_trans) ? 1 : 0; H.add_value(have);
        if (have) { H.add(t.trans, (size_t)2 * t.eta_samples * t.alpha_samples * t.theta_samples * 4); H.add(t.diff_trans, (size_t)2 * t.eta_samples * t.alpha_samples * 4); }
    }
    H.digest(out);
}

uint32_t scene_desc_diff(const ctl_scene_desc& a, const ctl_scene_desc& b, const uint64_t* a_geometry_hash) {
    auto same = [](const void* x, const void* y, size_t bytes) { return bytes == 0 || (x && y && std::memcmp(x, y, bytes) == 0); };
    uint32_t mask = 0;
    // topology first: the counts decide whether the arrays can be compared at all
    if (a.n_tri_data != b.n_tri_data || a.n_woop != b.n_woop || a.n_bvh_nodes != b.n_bvh_nodes || a.n_meshes != b.n_meshes || a.n_nodes != b.n_nodes || a.n_materials != b.n_materials ||
        a.n_images != b.n_images || (a.rough_transmittance != nullptr) != (b.rough_transmittance != nullptr))
        return CTL_DIFF_TOPOLOGY | ((std::memcmp(&a.camera, &b.camera, sizeof(ctl_sensor)) != 0) ? CTL_DIFF_CAMERA : 0u);
    if (!same(a.meshes, b.meshes, (size_t)a.n_meshes * sizeof(ctl_kernel_mesh))) mask |= CTL_DIFF_TOPOLOGY;
    for (uint32_t k = 0; k < a.n_nodes; k++) {
        const ctl_node &x = a.nodes[k], &y = b.nodes[k];
        if (x.mesh_index != y.mesh_index || x.material_offset != y.material_offset || x.instanciated_material != y.instanciated_material) mask |= CTL_DIFF_TOPOLOGY;
        if (x.lights[0] != y.lights[0] || x.lights[1] != y.lights[1] || x.n_lights != y.n_lights) mask |= CTL_DIFF_LIGHTS;
    }
    for (uint32_t i = 0; i < a.n_images; i++) {
        const ctl_mipmap &x = a.images[i], &y = b.images[i];
        if (x.width != y.width || x.height != y.height || x.texel_type != y.texel_type || x.wrap_mode != y.wrap_mode || x.filter_mode != y.filter_mode) mask |= CTL_DIFF_TOPOLOGY;
    }
    if (a_geometry_hash) {
        uint64_t hb[2]; scene_geometry_hash(b, hb);
        if (hb[0] != a_geometry_hash[0] || hb[1] != a_geometry_hash[1]) mask |= CTL_DIFF_TOPOLOGY;
    } else if (!(mask & CTL_DIFF_TOPOLOGY)) {
        uint64_t ha[2], hb[2];
        if (!same(a.tri_data, b.tri_data, (size_t)a.n_tri_data * sizeof(ctl_triangle_data)) || !same(a.woop, b.woop, (size_t)a.n_woop * sizeof(ctl_woop_tri)) ||
            !same(a.woop_index, b.woop_index, (size_t)a.n_woop * sizeof(ctl_woop_index)) || !same(a.bvh_nodes, b.bvh_nodes, (size_t)a.n_bvh_nodes * sizeof(ctl_bvh_node))) mask |= CTL_DIFF_TOPOLOGY;
        else { scene_geometry_hash(a, ha); scene_geometry_hash(b, hb); if (ha[0] != hb[0] || ha[1] != hb[1]) mask |= CTL_DIFF_TOPOLOGY; }   // texels and transmittance tables
    }
    if (std::memcmp(&a.camera, &b.camera, sizeof(ctl_sensor)) != 0) mask |= CTL_DIFF_CAMERA;
    if (!same(a.materials, b.materials, (size_t)a.n_materials * sizeof(ctl_material))) mask |= CTL_DIFF_MATERIALS;
    if (a.n_lights_buf != b.n_lights_buf || !same(a.lights, b.lights, (size_t)a.n_lights_buf * sizeof(ctl_light)) || a.n_anim_bytes != b.n_anim_bytes || !same(a.anim, b.anim, a.n_anim_bytes) ||
        a.num_lights != b.num_lights || a.env_map_index != b.env_map_index || std::memcmp(a.light_indices, b.light_indices, sizeof(a.light_indices)) != 0 ||
        std::memcmp(a.light_cdf, b.light_cdf, sizeof(a.light_cdf)) != 0) mask |= CTL_DIFF_LIGHTS;
    if (!same(a.node_transforms, b.node_transforms, (size_t)a.n_nodes * sizeof(ctl_float4x4)) || !same(a.node_inv_transforms, b.node_inv_transforms, (size_t)a.n_nodes * sizeof(ctl_float4x4)) ||
        a.scene_start_node != b.scene_start_node || a.n_scene_bvh_nodes != b.n_scene_bvh_nodes || !same(a.scene_bvh_nodes, b.scene_bvh_nodes, (size_t)a.n_scene_bvh_nodes * sizeof(ctl_bvh_node)) ||
        std::memcmp(a.box_min, b.box_min, 12) != 0 || std::memcmp(a.box_max, b.box_max, 12) != 0 || std::memcmp(&a.ray_trace_eps, &b.ray_trace_eps, 4) != 0) mask |= CTL_DIFF_TRANSFORMS;
    return mask;
}

Scene::~Scene() {}

void Scene::snapshot(const ctl_scene_desc& d) {
    std::unique_ptr<desc_snapshot> s(new desc_snapshot());
    s->meshes.assign(d.meshes, d.meshes + d.n_meshes); s->nodes.assign(d.nodes, d.nodes + d.n_nodes); s->materials.assign(d.materials, d.materials + d.n_materials);
    s->lights.assign(d.lights, d.lights + d.n_lights_buf); s->anim.assign(d.anim, d.anim + d.n_anim_bytes); s->top.assign(d.scene_bvh_nodes, d.scene_bvh_nodes + d.n_scene_bvh_nodes);
    s->xf.assign(d.node_transforms, d.node_transforms + d.n_nodes); s->ixf.assign(d.node_inv_transforms, d.node_inv_transforms + d.n_nodes);
    s->images.assign(d.images, d.images + d.n_images); for (auto& m : s->images) m.texels = nullptr;
    if (snap_) { s->geometry_hash[0] = snap_->geometry_hash[0]; s->geometry_hash[1] = snap_->geometry_hash[1]; }   // after an update: the geometry is the one already hashed
    else scene_geometry_hash(d, s->geometry_hash);
    s->d = d;
    s->d.tri_data = nullptr; s->d.woop = nullptr; s->d.woop_index = nullptr; s->d.bvh_nodes = nullptr;
    s->d.meshes = s->meshes.data(); s->d.nodes = s->nodes.data(); s->d.materials = s->materials.data(); s->d.lights = s->lights.data(); s->d.anim = s->anim.data();
    s->d.scene_bvh_nodes = s->top.data(); s->d.node_transforms = s->xf.data(); s->d.node_inv_transforms = s->ixf.data(); s->d.images = s->images.data();
    // none of the caller's pointers is kept: the diff only asks whether the tables are present (their contents are part of the hash), so a present table is marked by
    // a pointer to the snapshot itself, which is never dereferenced
    s->d.rough_transmittance = d.rough_transmittance ? reinterpret_cast<const ctl_rough_transmittance*>(s.get()) : nullptr;
    snap_ = std::move(s);
}

// The refit (and / or the re-stamp of the entries' material bits) of the device tree; the null stream, between two synchronisations: ordered after every trace that
// was launched and before the next
void Scene::refit_flat(const ctl_scene_desc& d, bool boxes, bool restamp, ctl_scene_update_stats* st) {
    refit_device R{};
    R.nodes = flat_nodes_.p; R.leaves = flat_leaves_.p; R.n_nodes = (uint32_t)flat_n_nodes_; R.n_entries = (uint32_t)flat_n_entries_; R.compact = S.flat_compact;
    R.part_index = refit_part_index_.p; R.part_boxes = refit_part_boxes_.p; R.inst = inst_.p; R.inst_fwd = inst_fwd_.p;
    R.restamp = restamp ? (int)snap_->materials.size() : 0; R.leaf_keys = S.flat_leaf_keys; R.alpha_maps = (int)S.alpha_maps; R.tri_data = tri_data_.p; R.node_info = node_info_.p; R.mats = mats_.p;
    if (!boxes) { launch_refit_entries(nullptr, R, false); CTL_HIP(hipDeviceSynchronize()); return; }
    std::vector<double> P((size_t)d.n_nodes * 12);
    for (uint32_t k = 0; k < d.n_nodes; k++)
        if (!refit_carry_matrix(d.node_transforms[k].m, refit_.xf0[k].m, &P[(size_t)k * 12])) throw std::runtime_error("ctl_scene_update: singular node transform");
    refit_carry_.upload(P.data(), P.size());
    if (refit_ebox_.n < flat_n_entries_) refit_ebox_.alloc(flat_n_entries_);
    if (refit_nbox_.n < flat_n_nodes_) refit_nbox_.alloc(flat_n_nodes_);
    if (!refit_area_.p) refit_area_.alloc(2);
    R.carry = refit_carry_.p; R.ebox = refit_ebox_.p; R.nbox = refit_nbox_.p;
    CTL_HIP(hipMemsetAsync(refit_area_.p, 0, 16, nullptr));
    launch_refit_area(nullptr, flat_nodes_.p, R.n_nodes, refit_area_.p);
    struct event_pair { hipEvent_t a = nullptr, b = nullptr; ~event_pair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev;   // destroyed also when a call below throws
    CTL_HIP(hipEventCreate(&ev.a)); CTL_HIP(hipEventCreate(&ev.b));
    hipEvent_t a = ev.a, b = ev.b;
    CTL_HIP(hipEventRecord(a, nullptr));
    launch_refit_entries(nullptr, R, true);
    const size_t n_levels = refit_.level_start.size() - 1;
    for (size_t l = n_levels; l-- > 0;) launch_refit_level(nullptr, R, refit_level_nodes_.p + refit_.level_start[l], refit_.level_start[l + 1] - refit_.level_start[l]);
    CTL_HIP(hipEventRecord(b, nullptr));
    launch_refit_area(nullptr, flat_nodes_.p, R.n_nodes, refit_area_.p + 1);
    double area[2] = { 0, 0 };
    CTL_HIP(hipMemcpy(area, refit_area_.p, 16, hipMemcpyDeviceToHost));
    CTL_HIP(hipDeviceSynchronize());
    float ms = 0; CTL_HIP(hipEventElapsedTime(&ms, a, b));
    st->node_area_before = area[0]; st->node_area_after = area[1]; st->refit_ms = ms; st->refit_levels = (uint32_t)n_levels;
}

uint32_t Scene::update(const ctl_scene_desc& d, ctl_scene_update_stats* stats) {
    require_device();
    if (!snap_) throw std::runtime_error("ctl_scene_update: the scene holds no description");
    const uint32_t mask = scene_desc_diff(snap_->d, d, snap_->geometry_hash);
    last_mask_ = mask;
    if (mask == 0) { last_update_ = ctl_scene_update_stats{}; if (stats) *stats = last_update_; return 0; }   // nothing differs: no synchronisation, no tracer is stalled
    if (mask & CTL_DIFF_TOPOLOGY) throw std::runtime_error("ctl_scene_update: the topology of the scene differs (geometry arrays, counts, node -> mesh / material assignment, images or transmittance tables): re-create the scene");
    const bool refit = (mask & CTL_DIFF_TRANSFORMS) && flattened();
    if (refit && S.flat_format != kFlatQ4) throw unsupported_error("ctl_scene_update: the Q8 node format is not refitted; a transform change needs a scene in the default format (or a new scene)");
    if (refit && refit_.level_start.size() < 2) throw unsupported_error("ctl_scene_update: the flattened tree carries no refit data");
    // Everything that can refuse the new description runs before anything is written, and before a tracer is stalled.  A transform change brings a new scene BVH: its
    // links must stay inside the array (creation is more lenient there, scene_checks.h) and its depth fit next to the mesh BVHs of creation (the geometry hash matched)
    check_scene_desc(d, mask, "ctl_scene_update");
    ctl_scene_update_stats st{}; st.mask = mask;
    CTL_HIP(hipDeviceSynchronize());   // no trace reads the arrays any more
    const uint32_t had_alpha_maps = S.alpha_maps;
    if (mask & (CTL_DIFF_MATERIALS | CTL_DIFF_LIGHTS)) set_shading_state(derive_shading_state(d));
    bool restamp = false;
    if (mask & CTL_DIFF_MATERIALS) {
        upload_materials(d);
        // the entries of a flattened scene carry their material's BSDF model and "has an alpha map": re-stamped on the device where either changed
        if (flattened() && d.n_materials) {
            for (uint32_t i = 0; i < d.n_materials; i++) if (d.materials[i].bsdf_type != snap_->materials[i].bsdf_type || d.materials[i].alpha_state != snap_->materials[i].alpha_state) restamp = true;
            if (had_alpha_maps != S.alpha_maps) restamp = true;
        }
    }
    if (mask & CTL_DIFF_LIGHTS) { upload_lights(d); if (!(mask & CTL_DIFF_TRANSFORMS)) upload_instances(d); }   // node_info carries the nodes' light slots
    if (mask & CTL_DIFF_TRANSFORMS) {
        upload_top_level(d); upload_instances(d);
        if (flattened()) S.inst_w_one = inverse_transforms_have_w_one(d);
    }
    CTL_HIP(hipDeviceSynchronize());
    bind(d);
    if (mask & CTL_DIFF_CAMERA) set_camera(d);
    if (refit || restamp) { refit_flat(d, refit, restamp, &st); st.restamped = restamp ? 1u : 0u; }
    last_update_ = st;
    snapshot(d);
    if (stats) *stats = st;
    return mask;
}

void Scene::read_flat_bvh(flat_scene& F) {
    if (!flattened()) throw std::runtime_error("ctl_scene_read_flat_bvh: the scene was not created with CTL_SCENE_FLATTEN");
    CTL_HIP(hipDeviceSynchronize());
    F = flat_scene(); F.format = S.flat_format; F.max_depth = flat_max_depth_; F.compact_links = S.flat_compact != 0; F.root_slab = flat_root_slab_; F.slab_nodes = flat_slab_nodes_;
    F.leaves.resize(flat_n_entries_);
    CTL_HIP(hipMemcpy(F.leaves.data(), flat_leaves_.p, flat_n_entries_ * sizeof(flat_leaf), hipMemcpyDeviceToHost));
    for (flat_leaf& L : F.leaves) { if (S.flat_leaf_keys) L.index &= 0x0fffffffu; L.node &= 0x7fffffffu; }
    if (S.flat_format == kFlatQ8) {
        F.nodes_q8.resize(flat_n_nodes_);
        CTL_HIP(hipMemcpy(F.nodes_q8.data(), flat_nodes_.p, flat_n_nodes_ * sizeof(flat8_node), hipMemcpyDeviceToHost));
        F.child_links.assign(flat_n_nodes_ * 8, (int32_t)kFlat8None);
        for (size_t i = 0; i < flat_n_nodes_; i++) {   // the links the kernels derive (flat8.h)
            const flat8_node& n = F.nodes_q8[i];
            const uint32_t q0w = (uint32_t)n.e[0] | ((uint32_t)n.e[1] << 8) | ((uint32_t)n.e[2] << 16) | ((uint32_t)n.imask << 24);
            const uint32_t im = flat8_inner_mask(q0w), lm = flat8_leaf_mask(q0w, n.base_b);
            for (uint32_t s = 0; s < 8; s++) {
                if ((im >> s) & 1u) F.child_links[i * 8 + s] = (int32_t)flat8_child_node(n.base_b, im, s);
                else if ((lm >> s) & 1u) F.child_links[i * 8 + s] = ~(int32_t)flat8_leaf_entry(n.leaf_base, lm, s);
            }
        }
        return;
    }
    F.nodes.resize(flat_n_nodes_);
    CTL_HIP(hipMemcpy(F.nodes.data(), flat_nodes_.p, flat_n_nodes_ * sizeof(flat4_node), hipMemcpyDeviceToHost));
    F.child_links.assign(flat_n_nodes_ * 4, 0x76543210);
    for (size_t i = 0; i < flat_n_nodes_; i++) {
        const flat4_node& n = F.nodes[i];
        int32_t c[4]; if (F.compact_links) flat4_implied_links(n, c); else std::memcpy(c, &flat_child_links_[i * 4], 16);
        for (int k = 0; k < 4; k++) if ((n.mask >> k) & 1) F.child_links[i * 4 + k] = (F.compact_links && c[k] >= 0) ? (c[k] & ~3) : c[k];
    }
}

}  // namespace ctl
