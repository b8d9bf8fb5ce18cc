// flat_nodes.cpp — the checks both callers of a node-set change share (plan_node_set) and the host yardstick of the kernels in flat_nodes.hip
// (update_nodes_flat_scene, what ctl_flat_bvh_update_nodes runs): the functions of flat_nodes.h and flat_rebuild.h in the device's order, so the device tree equals this
// one byte for byte (tests/test_gpu_node_set.py).
#include "flat_nodes.h"
#include "flat_meshes.h"
#include "flat_mesh_set.h"
#include "flatten.h"
#include "flat_rebuild.h"
#include "scene_checks.h"
#include "mitsuba_loader.h"   // unsupported_error
#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>

namespace ctl {

void node_set_basis::fill(const ctl_scene_desc& d) {
    meshes.assign(d.meshes, d.meshes + (d.meshes ? d.n_meshes : 0)); nodes.assign(d.nodes, d.nodes + (d.nodes ? d.n_nodes : 0));
    images.assign(d.images, d.images + (d.images ? d.n_images : 0)); for (auto& m : images) m.texels = nullptr;
    n_materials = d.n_materials; n_tri_data = d.n_tri_data; n_woop = d.n_woop; n_bvh_nodes = d.n_bvh_nodes; rough_transmittance = d.rough_transmittance != nullptr; filled = true;
}

void plan_node_set(const node_set_basis& old, const geometry_hashes& old_geom, const ctl_scene_desc& nd, const uint32_t* old_of_new, uint32_t n_new_nodes,
                   const std::vector<uint8_t>* device_owned, node_set_plan& out, const char* who_, mesh_set_plan* grow) {
    const std::string who = std::string(who_) + ": ";
    if (!old.filled) throw std::runtime_error(who + "the description the tree was made from is not known");
    // the map
    if (!old_of_new) throw std::runtime_error(who + "null node map");
    if (nd.n_nodes == 0 || n_new_nodes == 0) throw std::runtime_error(who + "no node left");
    if (n_new_nodes != nd.n_nodes) throw std::runtime_error(who + "the node map has " + std::to_string(n_new_nodes) + " elements, the new description " + std::to_string(nd.n_nodes) + " nodes");
    if (!nd.nodes || !nd.meshes || !nd.node_transforms || !nd.node_inv_transforms) throw std::runtime_error(who + "the new description lacks its node or mesh arrays");
    const uint32_t n_old = (uint32_t)old.nodes.size();
    out = node_set_plan();
    out.new_of_old.assign(n_old, kNodesNone);
    uint32_t last = kNodesNone;
    for (uint32_t k = 0; k < n_new_nodes; k++) {
        const uint32_t o = old_of_new[k];
        if (o == kNodesNone) { out.added.push_back(k); continue; }
        if (o >= n_old) throw std::runtime_error(who + "node map element " + std::to_string(k) + " names node " + std::to_string(o) + " of " + std::to_string(n_old));
        if (last != kNodesNone && o <= last) throw std::runtime_error(who + "the kept nodes of the map are not strictly increasing at element " + std::to_string(k));
        last = o; out.new_of_old[o] = k;
    }
    out.identity = n_new_nodes == n_old && out.added.empty();
    // the geometry side must be the tree's own — or, where the caller takes appended meshes, the tree's own plus tails (flat_meshes.cpp)
    if (grow) {
        plan_mesh_growth((uint32_t)old.meshes.size(), old.n_tri_data, old.n_woop, old.n_bvh_nodes, nd, who, *grow);   // (n_meshes is at least the held count from here on)
        if (!old.meshes.empty() && std::memcmp(nd.meshes, old.meshes.data(), old.meshes.size() * sizeof(ctl_kernel_mesh)) != 0)
            throw std::runtime_error(who + "a mesh the scene holds has another record: meshes can be appended, not changed; re-create the scene");
        out.identity = out.identity && !grow->grown();
    } else if (nd.n_meshes != old.meshes.size() || (nd.n_meshes && std::memcmp(nd.meshes, old.meshes.data(), (size_t)nd.n_meshes * sizeof(ctl_kernel_mesh)) != 0))
        throw std::runtime_error(who + "the set of meshes differs: only meshes the scene already holds can be instanced; re-create the scene");
    if (!grow && (nd.n_tri_data != old.n_tri_data || nd.n_woop != old.n_woop || nd.n_bvh_nodes != old.n_bvh_nodes)) throw std::runtime_error(who + "the geometry arrays have other sizes; re-create the scene");
    if (nd.n_images != old.images.size() || (nd.rough_transmittance != nullptr) != old.rough_transmittance) throw std::runtime_error(who + "the images or transmittance tables differ; re-create the scene");
    for (uint32_t i = 0; i < nd.n_images; i++) {
        const ctl_mipmap &x = old.images[i], &y = nd.images[i];
        if (x.width != y.width || x.height != y.height || x.texel_type != y.texel_type || x.wrap_mode != y.wrap_mode || x.filter_mode != y.filter_mode) throw std::runtime_error(who + "image " + std::to_string(i) + " differs; re-create the scene");
    }
    if (nd.n_materials < old.n_materials) throw std::runtime_error(who + "the material table shrank (" + std::to_string(nd.n_materials) + " of " + std::to_string(old.n_materials) + "): it is not compacted");
    for (uint32_t k = 0; k < n_new_nodes; k++) {
        const ctl_node& y = nd.nodes[k];
        if (y.mesh_index >= nd.n_meshes) throw std::runtime_error(who + "node " + std::to_string(k) + " references a missing mesh");
        if (old_of_new[k] == kNodesNone) continue;
        const ctl_node& x = old.nodes[old_of_new[k]];
        if (x.mesh_index != y.mesh_index || x.material_offset != y.material_offset || x.instanciated_material != y.instanciated_material)
            throw std::runtime_error(who + "kept node " + std::to_string(k) + " (was " + std::to_string(old_of_new[k]) + ") has another mesh or material assignment");
    }
    check_scene_desc(nd, kCheckAllParts, who_);   // what ctl_scene_desc_check refuses
    if (!old_geom.empty() && grow && grow->grown()) {
        // the held part: the same pointers under the old counts must hash to what the tree holds; then the whole description's hashes, which the tree holds from now on
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t n_held = (uint32_t)old.meshes.size();
        if (device_owned && device_owned->size() != n_held) device_owned = nullptr;
        ctl_scene_desc held = nd; held.n_meshes = n_held; held.n_tri_data = old.n_tri_data; held.n_woop = old.n_woop; held.n_bvh_nodes = old.n_bvh_nodes;
        geometry_hashes hg; hash_geometry(held, hg, device_owned);
        std::vector<uint8_t> owned_all; if (device_owned) { owned_all = *device_owned; owned_all.resize(nd.n_meshes, 0); }
        hash_geometry(nd, out.geom, device_owned ? &owned_all : nullptr);
        if (device_owned && hg.values.size() == old_geom.values.size())
            for (uint32_t m = 0; m < n_held; m++) if ((*device_owned)[m]) { hg.values[2 * m] = out.geom.values[2 * m] = old_geom.values[2 * m]; hg.values[2 * m + 1] = out.geom.values[2 * m + 1] = old_geom.values[2 * m + 1]; }
        grow->hash_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (!hg.same_structure(old_geom)) throw std::runtime_error(who + "the structure of the geometry arrays the scene holds (woop_index, mesh BVH links, texels, transmittance tables) differs; re-create the scene");
        for (uint32_t m = 0; m < n_held; m++) if (!hg.same_values(old_geom, m))
            throw std::runtime_error(who + "mesh " + std::to_string(m) + " has other vertex values than the scene holds: apply them with ctl_scene_update first");
    } else if (!old_geom.empty()) {
        if (device_owned && device_owned->size() != nd.n_meshes) device_owned = nullptr;
        hash_geometry(nd, out.geom, device_owned);
        if (device_owned && out.geom.values.size() == old_geom.values.size())
            for (uint32_t m = 0; m < nd.n_meshes; m++) if ((*device_owned)[m]) { out.geom.values[2 * m] = old_geom.values[2 * m]; out.geom.values[2 * m + 1] = old_geom.values[2 * m + 1]; }
        if (!out.geom.same_structure(old_geom)) throw std::runtime_error(who + "the structure of the geometry arrays (woop_index, mesh BVH links, texels, transmittance tables) differs; re-create the scene");
        for (uint32_t m = 0; m < nd.n_meshes; m++) if (!out.geom.same_values(old_geom, m))
            throw std::runtime_error(who + "mesh " + std::to_string(m) + " has other vertex values than the scene holds: apply them with ctl_scene_update first");
    }
    // the candidates of the generate stage
    const mesh_ranges R(nd);
    out.added_base.assign(1, 0u);
    for (uint32_t k : out.added) {
        const uint32_t m = nd.nodes[k].mesh_index;
        out.added_tri0.push_back(R.tri0[m]);
        const uint64_t next = (uint64_t)out.added_base.back() + (R.tri1[m] - R.tri0[m]);
        if (next >= (1ull << 31)) throw std::runtime_error(who + "the added nodes have too many triangles");
        out.added_base.push_back((uint32_t)next);
    }
}

void update_nodes_flat_scene(flat_scene& F, const node_set_basis& old, const ctl_scene_desc& nd, const uint32_t* old_of_new, uint32_t n_new_nodes, std::vector<uint32_t>& extra_missing, int builder) {
    const char* who = "ctl_flat_bvh_update_nodes";
    rebuild_last_rounds() = 0u;
    rebuild_refuse(F.format, F.refit.ready() && F.refit.part_index.size() == F.leaves.size(), F.compact_links, F.leaves.size(), who);
    node_set_plan plan;
    plan_node_set(old, F.refit.geom, nd, old_of_new, n_new_nodes, nullptr, plan, who);
    apply_node_set_flat(F, old, nd, old_of_new, n_new_nodes, plan, extra_missing, builder, who);
}

void apply_node_set_flat(flat_scene& F, const node_set_basis& old, const ctl_scene_desc& nd, const uint32_t* old_of_new, uint32_t n_new_nodes, const node_set_plan& plan,
                         std::vector<uint32_t>& extra_missing, int builder, const char* who) {
    if (old.nodes.size() != F.refit.xf0.size()) throw std::runtime_error(std::string(who) + ": the handle's description has another number of nodes than its tree");
    if (plan.identity) {   // as ctl_scene_update: a refit where a node has moved, else nothing (the geometry values are the tree's own: plan_node_set)
        bool moved = false;
        for (const flat_leaf& L : F.leaves) if (L.node >= nd.n_nodes || std::memcmp(L.inv, nd.node_inv_transforms[L.node].m, 48) != 0 || std::memcmp(&L.w33, &nd.node_inv_transforms[L.node].m[15], 4) != 0) { moved = true; break; }
        if (moved) refit_flat_scene(F, nd, nullptr);
        return;
    }
    const uint32_t n_old_nodes = (uint32_t)old.nodes.size(), n_old = (uint32_t)F.leaves.size();
    // the new tree in a scene of its own: a refusal below leaves F as it was
    flat_scene T; T.format = F.format; T.compact_links = F.compact_links; T.split_refs = F.split_refs;
    T.refit.part_boxes = F.refit.part_boxes; T.refit.geom = plan.geom.empty() ? F.refit.geom : plan.geom;
    // 1. drop and renumber (stable)
    for (uint32_t i = 0; i < n_old; i++) {
        const uint32_t k = nodes_new_of(F.leaves[i].node, plan.new_of_old.data(), n_old_nodes);
        if (k == kNodesNone) continue;
        T.leaves.push_back(F.leaves[i]); T.leaves.back().node = nodes_renumber(F.leaves[i].node, k);
        if (!plan.node_tri_delta.empty()) T.leaves.back().index = mesh_set_entry_index(F.leaves[i].index, plan.node_tri_delta[F.leaves[i].node & ~kNodesStampBit]);
        T.refit.part_index.push_back(F.refit.part_index[i]);
    }
    // 2. generate
    std::vector<uint32_t> tri_row, skipped;
    if (!plan.added.empty()) triangle_woop_rows(nd, tri_row);
    for (size_t j = 0; j < plan.added.size(); j++) {
        const uint32_t k = plan.added[j], count = plan.added_base[j + 1] - plan.added_base[j];
        const float* inv = nd.node_inv_transforms[k].m;
        for (uint32_t t = 0; t < count; t++) {
            const uint32_t tri = plan.added_tri0[j] + t, row = tri_row[tri];
            if (row >= nd.n_woop) { skipped.push_back(tri); continue; }
            const ctl_woop_tri& w = nd.woop[row];
            if (!nodes_rows_regular(w.a, w.b, w.c)) { skipped.push_back(tri); continue; }
            uint32_t words[32]; nodes_entry_words(w.a, w.b, w.c, tri, k, inv, inv[15], words);
            T.leaves.emplace_back(); std::memcpy(&T.leaves.back(), words, sizeof(flat_leaf));
            T.refit.part_index.push_back(kRefitNoPart);
        }
    }
    rebuild_refuse(T.format, true, T.compact_links, T.leaves.size(), who);
    // 3. carry data
    T.refit.xf0.resize(n_new_nodes);
    for (uint32_t k = 0; k < n_new_nodes; k++) T.refit.xf0[k] = old_of_new[k] == kNodesNone ? nd.node_transforms[k] : F.refit.xf0[old_of_new[k]];
    // the inverse transforms of the new description into every entry (k_refit_entries does it on the device), then 4. the rebuild
    for (flat_leaf& L : T.leaves) { std::memcpy(L.inv, nd.node_inv_transforms[L.node].m, 48); L.w33 = nd.node_inv_transforms[L.node].m[15]; }
    rebuild_flat_entries(T, nd, builder);
    F = std::move(T);
    if (plan.cut) mesh_set_rebase_triangles(extra_missing, *plan.cut);
    extra_missing.insert(extra_missing.end(), skipped.begin(), skipped.end());
    std::sort(extra_missing.begin(), extra_missing.end()); extra_missing.erase(std::unique(extra_missing.begin(), extra_missing.end()), extra_missing.end());
}

}  // namespace ctl
