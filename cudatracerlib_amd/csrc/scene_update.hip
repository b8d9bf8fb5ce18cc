// scene_update.hip — ctl_scene_desc_diff and ctl_scene_update: what UpdateKernel(m_pScene) does in the reference for a host that moved the camera, edited a
// material or called DynamicScene::SetNodeTransform (Kernel/Tracer.h:121,229).  The scene keeps a host copy of the description it was made from — the small
// arrays whole, the geometry arrays (triangles, Woop rows, mesh BVHs, texels, transmittance tables) as a 128-bit hash — and an update applies the blocks of the
// upload (tracer.hip) whose part of the description differs.  A transform change refits the flattened Q4 tree on the device (flat_refit.hip).
#include "tracer.h"
#include "flatten.h"
#include "flat_refit.h"
#include "scene_checks.h"
#include "geometry_hash.h"
#include "scene_cache.h"
#include "mitsuba_loader.h"   // unsupported_error
#include "scene_volumes.h"
#include "scene_image_set.h"
#include "flat_device.h"
#include <cstring>

namespace ctl {

// the grid records of two descriptions and the floats they point at (CTL_DIFF_VOLUMES): a record is compared field by field, its pointers by what they hold
static bool volume_grids_same(const ctl_scene_desc& a, const ctl_scene_desc& b) {
    if (a.n_volume_grids != b.n_volume_grids) return false;
    if (a.n_volume_grids && (!a.volume_grids || !b.volume_grids)) return false;
    auto cells_same = [](const uint32_t* da, const float* x, const uint32_t* db, const float* y) {
        if (std::memcmp(da, db, 12) != 0) return false;
        const size_t n = (size_t)da[0] * da[1] * da[2];
        return n == 0 || (x && y && std::memcmp(x, y, n * 4) == 0);
    };
    for (uint32_t k = 0; k < a.n_volume_grids; k++) {
        const ctl_volume_grid &x = a.volume_grids[k], &y = b.volume_grids[k];
        if (x.volume != y.volume || (x.single_grid != 0) != (y.single_grid != 0) || std::memcmp(x.sig_a_min, y.sig_a_min, 18 * sizeof(float)) != 0) return false;
        if (x.single_grid ? !cells_same(x.dim, x.data, y.dim, y.data) : !(cells_same(x.dim_a, x.data_a, y.dim_a, y.data_a) && cells_same(x.dim_s, x.data_s, y.dim_s, y.data_s))) return false;
    }
    return true;
}

// what ctl_scene_update applies, judged without the geometry arrays and the images (scene_image_set.h): the tail of scene_desc_diff, and the whole diff of
// ctl_scene_update_image_set, whose plan has compared the rest through the hashes.  b may hold more materials than a (the table grows, it is never compacted)
uint32_t scene_desc_diff_small(const ctl_scene_desc& a, const ctl_scene_desc& b) {
    auto same = [](const void* x, const void* y, size_t bytes) { return bytes == 0 || (x && y && std::memcmp(x, y, bytes) == 0); };
    uint32_t mask = 0;
    for (uint32_t k = 0; k < a.n_nodes && k < b.n_nodes; k++) {
        const ctl_node &x = a.nodes[k], &y = b.nodes[k];
        if (x.lights[0] != y.lights[0] || x.lights[1] != y.lights[1] || x.n_lights != y.n_lights) mask |= CTL_DIFF_LIGHTS;
    }
    if (std::memcmp(&a.camera, &b.camera, sizeof(ctl_sensor)) != 0) mask |= CTL_DIFF_CAMERA;
    if (a.n_materials != b.n_materials || !same(a.materials, b.materials, (size_t)a.n_materials * sizeof(ctl_material))) mask |= CTL_DIFF_MATERIALS;
    if (a.n_lights_buf != b.n_lights_buf || !same(a.lights, b.lights, (size_t)a.n_lights_buf * sizeof(ctl_light)) || a.n_anim_bytes != b.n_anim_bytes || !same(a.anim, b.anim, a.n_anim_bytes) ||
        a.num_lights != b.num_lights || a.env_map_index != b.env_map_index || std::memcmp(a.light_indices, b.light_indices, sizeof(a.light_indices)) != 0 ||
        std::memcmp(a.light_cdf, b.light_cdf, sizeof(a.light_cdf)) != 0) mask |= CTL_DIFF_LIGHTS;
    if (!same(a.node_transforms, b.node_transforms, (size_t)a.n_nodes * sizeof(ctl_float4x4)) || !same(a.node_inv_transforms, b.node_inv_transforms, (size_t)a.n_nodes * sizeof(ctl_float4x4)) ||
        a.scene_start_node != b.scene_start_node || a.n_scene_bvh_nodes != b.n_scene_bvh_nodes || !same(a.scene_bvh_nodes, b.scene_bvh_nodes, (size_t)a.n_scene_bvh_nodes * sizeof(ctl_bvh_node)) ||
        std::memcmp(a.box_min, b.box_min, 12) != 0 || std::memcmp(a.box_max, b.box_max, 12) != 0 || std::memcmp(&a.ray_trace_eps, &b.ray_trace_eps, 4) != 0) mask |= CTL_DIFF_TRANSFORMS;
    if (a.n_volumes != b.n_volumes || !same(a.volumes, b.volumes, (size_t)a.n_volumes * sizeof(ctl_volume)) || !volume_grids_same(a, b)) mask |= CTL_DIFF_VOLUMES;
    return mask;
}

uint32_t scene_desc_diff(const ctl_scene_desc& a, const ctl_scene_desc& b, const geometry_hashes* a_geometry, geometry_hashes* b_geometry, const std::vector<uint8_t>* ignore_values) {
    auto same = [](const void* x, const void* y, size_t bytes) { return bytes == 0 || (x && y && std::memcmp(x, y, bytes) == 0); };
    uint32_t mask = 0;
    // topology first: the counts decide whether the arrays can be compared at all
    if (a.n_tri_data != b.n_tri_data || a.n_woop != b.n_woop || a.n_bvh_nodes != b.n_bvh_nodes || a.n_meshes != b.n_meshes || a.n_nodes != b.n_nodes || a.n_materials != b.n_materials ||
        a.n_images != b.n_images || (a.rough_transmittance != nullptr) != (b.rough_transmittance != nullptr))
        return CTL_DIFF_TOPOLOGY | ((std::memcmp(&a.camera, &b.camera, sizeof(ctl_sensor)) != 0) ? CTL_DIFF_CAMERA : 0u) |
               ((a.n_volumes != b.n_volumes || !same(a.volumes, b.volumes, (size_t)a.n_volumes * sizeof(ctl_volume)) || !volume_grids_same(a, b)) ? (uint32_t)CTL_DIFF_VOLUMES : 0u);
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
    // the geometry arrays, one pass over each description's: another structure (woop_index, the mesh BVHs' links, texels, transmittance tables) is topology, other
    // VALUES in some mesh (triangle data, Woop rows, the mesh BVHs' boxes) are CTL_DIFF_GEOMETRY
    {
        geometry_hashes ha, hb_local; geometry_hashes& hb = b_geometry ? *b_geometry : hb_local;
        if (!a_geometry) hash_geometry(a, ha);
        const geometry_hashes& ga = a_geometry ? *a_geometry : ha;
        if (ignore_values && ignore_values->size() != b.n_meshes) ignore_values = nullptr;
        hash_geometry(b, hb, ignore_values);   // the ranges of an ignored mesh are not read
        if (ignore_values && hb.values.size() == ga.values.size()) for (uint32_t m = 0; m < b.n_meshes; m++) if ((*ignore_values)[m]) { hb.values[2 * m] = ga.values[2 * m]; hb.values[2 * m + 1] = ga.values[2 * m + 1]; }
        if (!hb.same_structure(ga)) mask |= CTL_DIFF_TOPOLOGY;
        else for (uint32_t m = 0; m < b.n_meshes; m++) if (!hb.same_values(ga, m)) { mask |= CTL_DIFF_GEOMETRY; break; }
    }
    mask |= scene_desc_diff_small(a, b);
    return mask;
}

// ---- the scene's volume tables (scene_volumes.h): device table, host copy (what the snapshot's `volumes` points at) and the kernel argument
scene_volumes::scene_volumes() {
    dev.alloc(CTL_MAX_VOL_COUNT); CTL_HIP(hipMemset(dev.p, 0, CTL_MAX_VOL_COUNT * sizeof(ctl_volume)));
    dev_grids.alloc(CTL_MAX_VOL_COUNT); CTL_HIP(hipMemset(dev_grids.p, 0, CTL_MAX_VOL_COUNT * sizeof(vol::grid_rec)));
    pack.recs.assign(CTL_MAX_VOL_COUNT, vol::grid_rec{});   // what dev_grids holds now
}
const ctl_volume* scene_volumes::store(const ctl_scene_desc& d, const ctl_volume_grid** grids_out) {
    vol::grid_pack now; vol::pack_grids(d, now);
    if (!now.same(pack)) {   // the records whole (16 slots), the floats into the buffer they had unless it must grow
        CTL_HIP(hipMemcpy(dev_grids.p, now.recs.data(), CTL_MAX_VOL_COUNT * sizeof(vol::grid_rec), hipMemcpyHostToDevice));
        if (now.cells.size() > dev_cells.n) dev_cells.alloc(now.cells.size());
        if (!now.cells.empty()) CTL_HIP(hipMemcpy(dev_cells.p, now.cells.data(), now.cells.size() * 4, hipMemcpyHostToDevice));
        pack = std::move(now);
    }
    // the snapshot's records: the caller's, with the data pointers turned to the scene's own copy of the floats
    grids.assign(d.volume_grids, d.volume_grids + d.n_volume_grids);
    for (ctl_volume_grid& G : grids) {
        const vol::grid_rec& R = pack.recs[G.volume];
        G.data = G.single_grid ? pack.cells.data() + R.off : nullptr; G.data_a = G.single_grid ? nullptr : pack.cells.data() + R.off_a; G.data_s = G.single_grid ? nullptr : pack.cells.data() + R.off_s;
    }
    *grids_out = grids.empty() ? nullptr : grids.data();
    const size_t n = d.n_volumes;   // (<= CTL_MAX_VOL_COUNT: check_scene_desc)
    if (n != host.size() || (n && std::memcmp(host.data(), d.volumes, n * sizeof(ctl_volume)) != 0)) {
        host.assign(d.volumes, d.volumes + n);
        if (n) CTL_HIP(hipMemcpy(dev.p, host.data(), n * sizeof(ctl_volume), hipMemcpyHostToDevice));
    }
    T = vol::make_table(dev.p, (uint32_t)n, pack.any ? dev_grids.p : nullptr, pack.any ? dev_cells.p : nullptr);
    return host.empty() ? nullptr : host.data();
}
vol::table Scene::volume_table() const { return volumes_ ? volumes_->T : vol::table{}; }
void Scene::refuse_volumes(const char* who) const {
    const uint32_t n = volume_table().n;
    if (n) throw unsupported_error(std::string(who) + ": the scene has participating media (" + std::to_string(n) + " volumes), which only the PathTracer plugin with Regularization = false renders");
}

void Scene::snapshot(const ctl_scene_desc& d, const geometry_hashes* geom) {
    std::unique_ptr<desc_snapshot> s(new desc_snapshot());
    s->meshes.assign(d.meshes, d.meshes + d.n_meshes); s->nodes.assign(d.nodes, d.nodes + d.n_nodes); s->materials.assign(d.materials, d.materials + d.n_materials);
    s->lights.assign(d.lights, d.lights + d.n_lights_buf); s->anim.assign(d.anim, d.anim + d.n_anim_bytes); s->top.assign(d.scene_bvh_nodes, d.scene_bvh_nodes + d.n_scene_bvh_nodes);
    s->xf.assign(d.node_transforms, d.node_transforms + d.n_nodes); s->ixf.assign(d.node_inv_transforms, d.node_inv_transforms + d.n_nodes);
    s->images.assign(d.images, d.images + d.n_images); for (auto& m : s->images) m.texels = nullptr;
    // the media: creation and every update end here, after the device has been synchronised — the table is written in place (no re-creation, no refit)
    const ctl_volume_grid* grids = nullptr;
    if (!volumes_) volumes_.reset(new scene_volumes());
    const ctl_volume* volumes = volumes_->store(d, &grids);
    if (geom) s->geom = *geom;                    // after an update: the pass that found the difference made them
    else if (snap_) s->geom = snap_->geom;
    else hash_geometry(d, s->geom);
    s->d = d;
    s->d.volumes = volumes; s->d.volume_grids = grids;
    s->d.tri_data = nullptr; s->d.woop = nullptr; s->d.woop_index = nullptr; s->d.bvh_nodes = nullptr;
    s->d.meshes = s->meshes.data(); s->d.nodes = s->nodes.data(); s->d.materials = s->materials.data(); s->d.lights = s->lights.data(); s->d.anim = s->anim.data();
    s->d.scene_bvh_nodes = s->top.data(); s->d.node_transforms = s->xf.data(); s->d.node_inv_transforms = s->ixf.data(); s->d.images = s->images.data();
    // none of the caller's pointers is kept: the diff only asks whether the tables are present (their contents are part of the hash), so a present table is marked by
    // a pointer to the snapshot itself, which is never dereferenced
    s->d.rough_transmittance = d.rough_transmittance ? reinterpret_cast<const ctl_rough_transmittance*>(s.get()) : nullptr;
    snap_ = std::move(s);
}

std::vector<double> Scene::carry_matrices(const ctl_scene_desc& d, const std::vector<ctl_float4x4>& xf0, const char* who) {
    std::vector<double> P((size_t)d.n_nodes * 12);
    for (uint32_t k = 0; k < d.n_nodes; k++)
        if (!refit_carry_matrix(d.node_transforms[k].m, xf0[k].m, &P[(size_t)k * 12])) throw std::runtime_error(std::string(who) + ": singular node transform");
    return P;
}
std::vector<uint8_t> Scene::device_owned_meshes() const {
    std::vector<uint8_t> owned;
    if (!skins_.empty()) { owned.assign(snap_->d.n_meshes, 0); for (const auto& kv : skins_) if (kv.first < owned.size()) owned[kv.first] = 1; }
    return owned;
}

// The refit (and / or the re-stamp of the entries' material bits) of the device tree; the null stream, between two synchronisations: ordered after every trace that
// was launched and before the next
void Scene::refit_flat(const ctl_scene_desc& d, bool boxes, bool restamp, const std::vector<uint8_t>* mesh_changed, ctl_scene_update_stats* st) {
    refit_device R{};
    R.nodes = flat_nodes_.p; R.leaves = flat_leaves_.p; R.n_nodes = (uint32_t)flat_n_nodes_; R.n_entries = (uint32_t)flat_n_entries_; R.compact = S.flat_compact;
    R.part_index = refit_part_index_.p; R.part_boxes = refit_part_boxes_.p; R.inst = inst_.p; R.inst_fwd = inst_fwd_.p;
    R.restamp = restamp ? (int)snap_->materials.size() : 0; R.leaf_keys = S.flat_leaf_keys; R.alpha_maps = (int)S.alpha_maps; R.tri_data = tri_data_.p; R.node_info = node_info_.p; R.mats = mats_.p;
    if (!boxes) { launch_refit_entries(nullptr, R, false); CTL_HIP(hipDeviceSynchronize()); return; }
    const std::vector<double> P = carry_matrices(d, refit_.xf0, "ctl_scene_update");
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
    if (mesh_changed) {   // the entries of the deformed meshes take their new Woop rows and become whole, then every entry is refitted as after a transform change
        std::vector<uint32_t> rows, changed(d.n_nodes);
        if (!refit_tri_row_.p) { triangle_woop_rows(d, rows); refit_tri_row_.upload(rows.data(), rows.size()); }   // woop_index is structure: the table holds for every later update
        for (uint32_t k = 0; k < d.n_nodes; k++) changed[k] = (*mesh_changed)[d.nodes[k].mesh_index];
        refit_node_changed_.upload(changed.data(), changed.size());
        CTL_HIP(hipStreamSynchronize(nullptr));   // `changed` and `rows` are pageable: the copies have left them
        const deform_device D{ refit_node_changed_.p, d.n_nodes, refit_tri_row_.p, d.n_tri_data, leaf_tris_.p, d.n_woop };
        launch_deform_entries(nullptr, R, D);
    }
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

// One mesh's ranges of the two-level arrays, laid out as the constructor lays them out (tracer.hip), into the SAME allocations: tracers keep their pointers.  Synchronous
// copies from pageable memory.
void Scene::upload_mesh_geometry(const ctl_scene_desc& d, const mesh_ranges& R, uint32_t m) {
    const ctl_kernel_mesh& km = d.meshes[m];
    if (R.tri1[m] > R.tri0[m]) CTL_HIP(hipMemcpy(tri_data_.p + (size_t)R.tri0[m] * 2, d.tri_data + R.tri0[m], (size_t)(R.tri1[m] - R.tri0[m]) * sizeof(ctl_triangle_data), hipMemcpyHostToDevice));
    if (R.node1[m] > R.node0[m]) CTL_HIP(hipMemcpy(bot_nodes_.p + (size_t)R.node0[m] * 4, d.bvh_nodes + R.node0[m], (size_t)(R.node1[m] - R.node0[m]) * sizeof(ctl_bvh_node), hipMemcpyHostToDevice));
    const uint32_t first = R.woop0[m], last = R.woop1[m];
    if (last <= first) return;
    std::vector<float4> tmp((size_t)(last - first) * 4);
    for (uint32_t w = first; w < last; w++) {
        const ctl_woop_tri& t = d.woop[w];
        const size_t o = (size_t)(w - first) * 4, at = (size_t)km.bvh_index_offset + (w - first);
        tmp[o + 0] = make_float4(t.a[0], t.a[1], t.a[2], t.a[3]);
        tmp[o + 1] = make_float4(t.b[0], t.b[1], t.b[2], t.b[3]);
        tmp[o + 2] = make_float4(t.c[0], t.c[1], t.c[2], t.c[3]);
        const uint32_t idx = at < d.n_woop ? d.woop_index[at].index : 1u;
        tmp[o + 3] = make_float4(__builtin_bit_cast(float, idx), 0, 0, 0);
    }
    CTL_HIP(hipMemcpy(leaf_tris_.p + (size_t)first * 4, tmp.data(), tmp.size() * sizeof(float4), hipMemcpyHostToDevice));
}

uint32_t Scene::update(const ctl_scene_desc& d, ctl_scene_update_stats* stats) {
    require_device();
    if (!snap_) throw std::runtime_error("ctl_scene_update: the scene holds no description");
    geometry_hashes geom;
    const std::vector<uint8_t> device_owned = device_owned_meshes();
    // lights_stale_: an emissive skin was unbound (shape_set.hip) and HBM holds its last pose's shape sets — the light tables are uploaded whatever the descriptions say
    const uint32_t mask = scene_desc_diff(snap_->d, d, &snap_->geom, &geom, device_owned.empty() ? nullptr : &device_owned) | (lights_stale_ ? (uint32_t)CTL_DIFF_LIGHTS : 0u);
    return flat_rebuilder::apply_update(*this, d, mask, geom, stats);
}

// ctl_scene_update behind its diff: `mask` = what differs between the description the scene holds and d, geom = d's hashes.  ctl_scene_update_image_set (scene_image_set.hip)
// comes here too, with the mask of scene_desc_diff_small — there d may hold more materials than the snapshot
uint32_t flat_rebuilder::apply_update(Scene& A, const ctl_scene_desc& d, uint32_t mask, const geometry_hashes& geom, ctl_scene_update_stats* stats) {
    A.last_mask_ = mask;
    if (mask == 0) { A.last_update_ = ctl_scene_update_stats{}; if (stats) *stats = A.last_update_; return 0; }   // nothing differs: no synchronisation, no tracer is stalled
    if (mask & CTL_DIFF_TOPOLOGY) throw std::runtime_error("ctl_scene_update: the topology of the scene differs (geometry arrays, counts, node -> mesh / material assignment, images or transmittance tables): re-create the scene");
    const bool refit = (mask & (CTL_DIFF_TRANSFORMS | CTL_DIFF_GEOMETRY)) && A.flattened();
    if (refit && A.S.flat_format != kFlatQ4) throw unsupported_error("ctl_scene_update: the Q8 node format is not refitted; a transform or geometry change needs a scene in the default format (or a new scene)");
    if (refit && A.refit_.level_start.size() < 2) throw unsupported_error("ctl_scene_update: the flattened tree carries no refit data");
    // Everything that can refuse the new description runs before anything is written, and before a tracer is stalled.  A transform change brings a new scene BVH: its
    // links must stay inside the array (creation is more lenient there, scene_checks.h) and its depth fit next to the mesh BVHs of creation (the geometry hash matched)
    check_scene_desc(d, mask, "ctl_scene_update");
    std::vector<uint8_t> mesh_changed;   // CTL_DIFF_GEOMETRY: the meshes whose value hash differs
    const mesh_ranges ranges(d);
    if (mask & CTL_DIFF_GEOMETRY) {
        mesh_changed.assign(d.n_meshes, 0);
        for (uint32_t m = 0; m < d.n_meshes; m++) mesh_changed[m] = geom.same_values(A.snap_->geom, m) ? 0 : 1;
        // the arrays were sized by creation and the counts agree; a range the re-upload writes must still lie inside them
        for (uint32_t m = 0; m < d.n_meshes; m++) if (mesh_changed[m] && ((size_t)ranges.tri1[m] * 2 > A.tri_data_.n || (size_t)ranges.woop1[m] * 4 > A.leaf_tris_.n || (size_t)ranges.node1[m] * 4 > A.bot_nodes_.n))
            throw std::runtime_error("ctl_scene_update: mesh " + std::to_string(m) + " reaches outside the scene's geometry arrays");
        if (A.flattened() && !A.flat_missing_tris_.empty()) {
            // a triangle that gather_references dropped at creation (singular Woop matrix) and that is regular now: the tree has no leaf entry to put it in
            std::vector<uint32_t> rows; triangle_woop_rows(d, rows);
            const int m = mesh_gaining_a_triangle(d, A.flat_missing_tris_, rows, mesh_changed);
            if (m >= 0) {
                A.last_mask_ |= CTL_DIFF_TOPOLOGY;
                throw std::runtime_error("ctl_scene_update: mesh " + std::to_string(m) + " has a triangle that was degenerate when the scene was flattened and no longer is: the flattened tree has no leaf entry for it; re-create the scene");
            }
        }
    }
    ctl_scene_update_stats st{}; st.mask = mask;
    CTL_HIP(hipDeviceSynchronize());   // no trace reads the arrays any more
    const uint32_t had_alpha_maps = A.S.alpha_maps;
    if (mask & (CTL_DIFF_MATERIALS | CTL_DIFF_LIGHTS)) A.set_shading_state(derive_shading_state(d));
    bool restamp = false;
    if (mask & CTL_DIFF_MATERIALS) {
        A.upload_materials(d);
        // the entries of a flattened scene carry their material's BSDF model and "has an alpha map": re-stamped on the device where either changed
        if (A.flattened() && d.n_materials) {
            const std::vector<ctl_material>& held = A.snap_->materials;   // (a material behind the held table is no entry's yet)
            for (uint32_t i = 0; i < d.n_materials && i < held.size(); i++) if (d.materials[i].bsdf_type != held[i].bsdf_type || d.materials[i].alpha_state != held[i].alpha_state) restamp = true;
            if (had_alpha_maps != A.S.alpha_maps) restamp = true;
        }
    }
    if (mask & CTL_DIFF_LIGHTS) { A.upload_lights(d); A.lights_stale_ = false; if (!(mask & CTL_DIFF_TRANSFORMS)) A.upload_instances(d); }   // node_info carries the nodes' light slots
    if (mask & CTL_DIFF_TRANSFORMS) {
        A.upload_top_level(d); A.upload_instances(d);
        if (A.flattened()) A.S.inst_w_one = inverse_transforms_have_w_one(d);
    }
    if (mask & CTL_DIFF_GEOMETRY) {
        for (uint32_t m = 0; m < d.n_meshes; m++) if (mesh_changed[m]) A.upload_mesh_geometry(d, ranges, m);
        if (A.flattened()) restamp = true;   // the entries' model / alpha bits come from tri_data: re-stamped from the new one
    }
    // the shape sets of the lights on emissive skins are the device's: d's own were made from rest-pose rows (and have just been uploaded, or its transforms have moved the node)
    if (mask & (CTL_DIFF_LIGHTS | CTL_DIFF_TRANSFORMS | CTL_DIFF_GEOMETRY)) A.run_shape_sets(d);
    CTL_HIP(hipDeviceSynchronize());
    A.bind(d);
    if (mask & CTL_DIFF_CAMERA) A.set_camera(d);
    if (refit || restamp) { A.refit_flat(d, refit, restamp, (mask & CTL_DIFF_GEOMETRY) ? &mesh_changed : nullptr, &st); st.restamped = restamp ? 1u : 0u; }
    A.last_update_ = st;
    A.snapshot(d, &geom);
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
    if (refit_part_index_.p && refit_part_index_.n == flat_n_entries_) {   // the refit side data as the device holds it: a geometry update turns split references into whole entries
        F.refit.part_index.resize(flat_n_entries_);
        CTL_HIP(hipMemcpy(F.refit.part_index.data(), refit_part_index_.p, flat_n_entries_ * 4, hipMemcpyDeviceToHost));
        F.refit.part_boxes = refit_.part_boxes; F.refit.xf0 = refit_.xf0; F.refit.level_start = refit_.level_start;
        F.refit.level_nodes.resize(refit_level_nodes_.n);
        if (refit_level_nodes_.n) CTL_HIP(hipMemcpy(F.refit.level_nodes.data(), refit_level_nodes_.p, refit_level_nodes_.n * 4, hipMemcpyDeviceToHost));
        F.refit.geom = snap_->geom;
    }
    F.child_links.assign(flat_n_nodes_ * 4, 0x76543210);
    for (size_t i = 0; i < flat_n_nodes_; i++) {
        const flat4_node& n = F.nodes[i];
        int32_t c[4]; if (F.compact_links) flat4_implied_links(n, c); else std::memcpy(c, &flat_child_links_[i * 4], 16);
        for (int k = 0; k < 4; k++) if ((n.mask >> k) & 1) F.child_links[i * 4 + k] = (F.compact_links && c[k] >= 0) ? (c[k] & ~3) : c[k];
    }
}

}  // namespace ctl
