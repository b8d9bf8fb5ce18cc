// scene_checks.cpp — check_scene_desc / check_traversal_stack (scene_checks.h): host arithmetic over a description, nothing else.
#include "scene_checks.h"
#include "device_scene.h"   // kStackSize and the BSDF model classifiers
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace ctl {
namespace {

[[noreturn]] void refuse(const char* who, const std::string& what) { throw std::runtime_error(std::string(who) + ": " + what); }

// depth of a BVH in the reference's node layout (child >= 0: float4 index of an inner node)
int depth_of(const ctl_bvh_node* nodes, size_t n_nodes, int root, bool strict, const char* who) {
    int best = 0; std::vector<std::pair<int, int>> st;
    auto inside = [&](int link) { return (size_t)(link / 4) < n_nodes && !(strict && (link & 3)); };
    if (root >= 0) { if (inside(root)) st.emplace_back(root / 4, 1); else if (strict) refuse(who, "scene BVH start node outside the array"); }
    while (!st.empty()) {
        const auto [i, dpt] = st.back(); st.pop_back();
        best = std::max(best, dpt);
        if (dpt > 4 * kStackSize) refuse(who, "BVH child links form a cycle");
        for (int c : { nodes[i].child0, nodes[i].child1 }) {
            if (c < 0 || c == 0x76543210) continue;
            if (inside(c)) st.emplace_back(c / 4, dpt + 1);
            else if (strict) refuse(who, "scene BVH child link outside the array");
        }
    }
    return best;
}

void check_nodes(const ctl_scene_desc& d, uint32_t parts, const char* who) {
    for (uint32_t k = 0; k < d.n_nodes; k++) {
        if (parts & CTL_DIFF_TRANSFORMS) {
            const float* im = d.node_inv_transforms[k].m; const float* fm = d.node_transforms[k].m;
            if (im[12] != 0.0f || im[13] != 0.0f || im[14] != 0.0f || fm[12] != 0.0f || fm[13] != 0.0f || fm[14] != 0.0f) refuse(who, "node transforms must be affine");
        }
        if ((parts & CTL_DIFF_TOPOLOGY) && d.nodes[k].mesh_index >= d.n_meshes) refuse(who, "node references a missing mesh");
    }
}

void check_lights(const ctl_scene_desc& d, const char* who) {
    for (uint32_t i = 0; i < d.n_lights_buf; i++) {
        const ctl_light& L = d.lights[i];
        if (L.type < CTL_LIGHT_POINT || L.type > CTL_LIGHT_INFINITE) refuse(who, "unknown light type " + std::to_string(L.type));
        if (L.type == CTL_LIGHT_DIFFUSE && L.rad_texture.type == CTL_TEX_IMAGE && L.rad_texture.image != 0xffffffffu && L.rad_texture.image >= d.n_images) refuse(who, "light texture references a missing image");
        if (L.type == CTL_LIGHT_INFINITE && L.env_image >= d.n_images) refuse(who, "InfiniteLight references a missing image");
    }
}

void check_materials(const ctl_scene_desc& d, const char* who) {
    auto table = [&](uint32_t slot) -> const ctl_rough_transmittance* { return d.rough_transmittance ? &d.rough_transmittance[slot] : nullptr; };
    for (uint32_t i = 0; i < d.n_materials; i++) {
        const ctl_material& mi = d.materials[i];
        if (mi.map_kind > CTL_MAP_HEIGHT) refuse(who, "unknown surface map kind");
        if (mi.alpha_state > CTL_ALPHA_REFLECTANCE_COLOR || mi.alpha_state == 4) refuse(who, "unknown alpha blend state");
        for (int k = 0; k < 6; k++) {   // the map and the alpha texture count only where they are read
            if (k == 4 && mi.map_kind == CTL_MAP_NONE) continue;
            if (k == 5 && mi.alpha_state == CTL_ALPHA_DISABLED) continue;
            const ctl_texture& t = k < 4 ? mi.tex[k] : (k == 4 ? mi.map_tex : mi.alpha_tex);
            if (t.type == CTL_TEX_IMAGE && t.image != 0xffffffffu && t.image >= d.n_images) refuse(who, "texture references a missing image");
            if (t.type != CTL_TEX_CONSTANT && t.type != CTL_TEX_CHECKER && t.type != CTL_TEX_IMAGE && t.type != 0) refuse(who, "texture type " + std::to_string(t.type) + " has no HIP implementation yet");
        }
        const uint32_t t = mi.bsdf_type;
        for (int k = 0; k < nested_bsdf_count(t); k++) {
            const uint32_t ni = mi.u[2 + k];
            if (ni >= d.n_materials || d.materials[ni].bsdf_type >= CTL_BSDF_HK) refuse(who, "nested BSDF index out of range or not a simple BSDF (BSDFFirst)");
        }
        if (const uint32_t* dist = bsdf_distribution(mi)) {
            const ctl_rough_transmittance* T = *dist <= CTL_MF_PHONG ? table(*dist) : nullptr;
            if (t == CTL_BSDF_ROUGHCOATING) {
                if (!T || !T->trans) refuse(who, "roughcoating needs the rough-transmittance table of its distribution");
            } else {
                if (*dist > CTL_MF_PHONG) refuse(who, "unknown microfacet distribution");
                if (t == CTL_BSDF_ROUGHPLASTIC && (!T || !T->trans || !T->diff_trans)) refuse(who, "roughplastic needs the rough-transmittance table of its distribution (ctl_builder_set_rough_transmittance)");
            }
        }
        if (!is_simple_bsdf(t) && !is_nesting_bsdf(t)) refuse(who, "BSDF type " + std::to_string(t) + " has no HIP implementation yet");
    }
}

// participating media (CTL_DIFF_VOLUMES): what csrc/volume.h takes for granted
void check_volumes(const ctl_scene_desc& d, const char* who) {
    if (d.n_volumes > CTL_MAX_VOL_COUNT) refuse(who, std::to_string(d.n_volumes) + " volumes; the aggregate holds at most " + std::to_string(CTL_MAX_VOL_COUNT) + " (KernelAggregateVolume::MAX_VOL_COUNT)");
    if (d.n_volumes && !d.volumes) refuse(who, "n_volumes without a volumes array");
    for (uint32_t i = 0; i < d.n_volumes; i++) {
        const ctl_volume& V = d.volumes[i]; const std::string vi = "volume " + std::to_string(i) + ": ";
        if (V.type != CTL_VOLUME_HOMOGENEOUS && V.type != CTL_VOLUME_GRID) refuse(who, vi + "volume type " + std::to_string(V.type) + " has no HIP implementation (homogeneous media only)");
        for (int k = 0; k < 9; k++) {
            const float c = k < 3 ? V.sig_a[k] : (k < 6 ? V.sig_s[k - 3] : V.le[k - 6]);
            if (!std::isfinite(c) || c < 0.0f) refuse(who, vi + "sig_a, sig_s and le must be finite and non-negative");
            if (V.type == CTL_VOLUME_GRID && c != 0.0f) refuse(who, vi + "a VolumeGrid's sig_a, sig_s and le must be 0 (its coefficients are its grid record's)");
        }
        uint32_t records = 0;
        for (uint32_t g = 0; g < d.n_volume_grids && d.volume_grids; g++) if (d.volume_grids[g].volume == i) records++;
        if (V.type == CTL_VOLUME_GRID && records != 1) refuse(who, vi + "a VolumeGrid needs exactly one grid record, the description has " + std::to_string(records));
        if (V.type != CTL_VOLUME_GRID && records != 0) refuse(who, vi + "a grid record names a volume that is no VolumeGrid");
        for (int k = 0; k < 16; k++) if (!std::isfinite(V.volume_to_world.m[k])) refuse(who, vi + "volume_to_world is not finite");
        for (int k = 0; k < 16; k++) if (!std::isfinite(V.world_to_volume.m[k])) refuse(who, vi + "volume_to_world is not invertible (world_to_volume is not finite; ctl_volume_update derives it)");
        const ctl_phase_function& F = V.phase;
        if (F.type < CTL_PHASE_HG || F.type > CTL_PHASE_RAYLEIGH) refuse(who, vi + "unknown phase function type " + std::to_string(F.type));
        if (F.type == CTL_PHASE_HG && !(std::fabs(F.g) < 1.0f)) refuse(who, vi + "the Henyey-Greenstein g must lie in (-1, 1)");
        if (F.type == CTL_PHASE_KAJIYA_KAY && !(std::isfinite(F.ks) && std::isfinite(F.kd) && std::isfinite(F.exponent) && std::isfinite(F.normalization)))
            refuse(who, vi + "the Kajiya-Kay ks, kd, exponent and normalization must be finite");
    }
    // the grid records (ctl_volume_grid): what csrc/volume_grid.h takes for granted
    if (d.n_volume_grids && !d.volume_grids) refuse(who, "n_volume_grids without a volume_grids array");
    if (d.n_volume_grids > CTL_MAX_VOL_COUNT) refuse(who, std::to_string(d.n_volume_grids) + " grid records; a table holds at most " + std::to_string(CTL_MAX_VOL_COUNT));
    for (uint32_t g = 0; g < d.n_volume_grids; g++) {
        const ctl_volume_grid& G = d.volume_grids[g]; const std::string gi = "volume grid " + std::to_string(g) + ": ";
        if (G.volume >= d.n_volumes) refuse(who, gi + "names volume " + std::to_string(G.volume) + " of " + std::to_string(d.n_volumes));
        auto grid = [&](const uint32_t* dim, const float* data, const char* name) {
            if (!dim[0] || !dim[1] || !dim[2]) refuse(who, gi + name + " has a zero dimension");
            // (each factor is checked first, so that the product cannot overflow 64 bits)
            if (dim[0] > CTL_MAX_GRID_CELLS || dim[1] > CTL_MAX_GRID_CELLS || dim[2] > CTL_MAX_GRID_CELLS || (uint64_t)dim[0] * dim[1] > CTL_MAX_GRID_CELLS || (uint64_t)dim[0] * dim[1] * dim[2] > CTL_MAX_GRID_CELLS)
                refuse(who, gi + name + " has more than " + std::to_string(CTL_MAX_GRID_CELLS) + " cells (CTL_MAX_GRID_CELLS)");
            if (!data) refuse(who, gi + name + " has no data");
            const size_t n = (size_t)dim[0] * dim[1] * dim[2];
            for (size_t k = 0; k < n; k++) if (!std::isfinite(data[k]) || data[k] < 0.0f) refuse(who, gi + name + " values must be finite and non-negative");
        };
        if (G.single_grid) grid(G.dim, G.data, "grid");
        else { grid(G.dim_a, G.data_a, "gridA"); grid(G.dim_s, G.data_s, "gridS"); }
        const float* lo[3] = { G.sig_a_min, G.sig_s_min, G.le_min }; const float* hi[3] = { G.sig_a_max, G.sig_s_max, G.le_max };
        for (int c = 0; c < 3; c++) for (int k = 0; k < 3; k++) {
            if (!std::isfinite(lo[c][k]) || lo[c][k] < 0.0f || !std::isfinite(hi[c][k]) || hi[c][k] < 0.0f) refuse(who, gi + "sigAMin ... leMax must be finite and non-negative");
            if (hi[c][k] < lo[c][k]) refuse(who, gi + "a maximum lies below its minimum (sigAMin ... leMax)");
        }
    }
}

}  // namespace

void check_traversal_stack(const ctl_scene_desc& d, bool strict_top_level, const char* who) {
    if (strict_top_level) {
        if (d.scene_start_node < 0 && (uint32_t)~d.scene_start_node >= d.n_nodes) refuse(who, "scene BVH start node names a missing node");
        for (uint32_t i = 0; i < d.n_scene_bvh_nodes; i++)
            for (int c : { d.scene_bvh_nodes[i].child0, d.scene_bvh_nodes[i].child1 }) if (c < 0 && (uint32_t)~c >= d.n_nodes) refuse(who, "scene BVH leaf names a missing node");
    }
    const int top = d.scene_start_node >= 0 ? depth_of(d.scene_bvh_nodes, d.n_scene_bvh_nodes, d.scene_start_node, strict_top_level, who) : 0;
    int bottom = 0;
    for (uint32_t m = 0; m < d.n_meshes; m++) {
        const uint32_t first = d.meshes[m].bvh_node_offset / 4;
        if (first < d.n_bvh_nodes) bottom = std::max(bottom, depth_of(d.bvh_nodes + first, d.n_bvh_nodes - first, 0, false, who));
    }
    if (top + bottom + 3 > kStackSize)
        refuse(who, "scene BVH depth " + std::to_string(top) + " + mesh BVH depth " + std::to_string(bottom) + " does not fit the traversal stack of " + std::to_string(kStackSize) + " entries" +
                    (strict_top_level ? "" : " (rebuild the meshes with CTL_BVH_BINNED, whose depth is bounded)"));   // (a hint for whoever builds the meshes: an update cannot)
}

void check_scene_desc(const ctl_scene_desc& d, uint32_t parts, const char* who) {
    const bool creating = (parts & CTL_DIFF_TOPOLOGY) != 0;
    if (creating && !d.n_nodes) refuse(who, "scene has no nodes");
    if ((parts & CTL_DIFF_LIGHTS) && d.env_map_index != 0xffffffffu && (d.env_map_index >= d.n_lights_buf || d.lights[d.env_map_index].type != CTL_LIGHT_INFINITE))
        refuse(who, "env_map_index does not name an InfiniteLight");
    if (parts & (CTL_DIFF_TRANSFORMS | CTL_DIFF_TOPOLOGY)) check_nodes(d, parts, who);
    if (parts & CTL_DIFF_LIGHTS) check_lights(d, who);
    if (parts & CTL_DIFF_MATERIALS) check_materials(d, who);
    if (parts & (CTL_DIFF_TRANSFORMS | CTL_DIFF_TOPOLOGY | CTL_DIFF_GEOMETRY)) check_traversal_stack(d, !creating, who);   // (a geometry update brings the mesh BVHs anew: what creation checks of them)
    if (parts & (CTL_DIFF_VOLUMES | CTL_DIFF_TOPOLOGY)) check_volumes(d, who);
    if ((parts & CTL_DIFF_CAMERA) && (d.camera.type < CTL_SENSOR_SPHERICAL || d.camera.type > CTL_SENSOR_TELECENTRIC))
        refuse(who, creating ? "unknown sensor type " + std::to_string(d.camera.type) : std::string("unknown sensor type"));   // (creation has always named the value, an update never has)
}

}  // namespace ctl
