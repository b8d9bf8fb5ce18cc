// flat_mesh_set.cpp — the host side of removing meshes from a live scene (flat_mesh_set.h): the checks both callers share (plan_mesh_set), the host re-statement of
// k_compact_tri_rows, and the host yardstick of ctl_scene_update_mesh_set (update_mesh_set_flat_scene).
#include "flat_mesh_set.h"
#include "flatten.h"
#include "flat_rebuild.h"
#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>

namespace ctl {

void compact_tri_rows_host(const mesh_compaction& cut, const uint32_t* held_rows, uint32_t n_held, uint32_t* out) {
    for (uint32_t i = 0; i < cut.kept_tris; i++) {   // the kernel's lane i
        const uint32_t j = nodes_find_added(cut.tri_dst.data(), cut.runs(), i), src = cut.tri_src[j] + (i - cut.tri_dst[j]);
        out[i] = src < n_held ? mesh_set_row_word(held_rows[src], cut.row_src[j] - cut.row_dst[j]) : kNodesNone;
    }
}

void plan_mesh_compaction(const node_set_basis& old, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes, const std::string& who, mesh_compaction& cut) {
    cut = mesh_compaction();
    const uint32_t n_old = (uint32_t)old.meshes.size();
    if (n_new_meshes && !old_mesh_of_new) throw std::runtime_error(who + "null mesh map");
    cut.new_of_old.assign(n_old, kNodesNone);
    uint32_t last = kNodesNone; bool appended = false;
    for (uint32_t m = 0; m < n_new_meshes; m++) {
        const uint32_t o = old_mesh_of_new[m];
        if (o == kNodesNone) { appended = true; continue; }
        if (o >= n_old) throw std::runtime_error(who + "mesh map element " + std::to_string(m) + " names mesh " + std::to_string(o) + " of " + std::to_string(n_old));
        if (appended) throw std::runtime_error(who + "mesh map element " + std::to_string(m) + " keeps a mesh behind an appended one: appended meshes stand behind the kept ones, as the builder appends");
        if (last != kNodesNone && o <= last) throw std::runtime_error(who + "the kept meshes of the map are not strictly increasing at element " + std::to_string(m) + ": meshes are not reordered");
        last = o; cut.new_of_old[o] = cut.kept_meshes++;
    }
    cut.removed_meshes = n_old - cut.kept_meshes;
    if (!cut.removes()) { cut.kept_tris = old.n_tri_data; cut.kept_rows = old.n_woop; cut.kept_nodes = old.n_bvh_nodes; return; }
    // the held layout must be the builder's: every array in mesh order from element 0, the index words beside the rows
    std::vector<uint32_t> t0(n_old + 1), r0(n_old + 1), b0(n_old + 1);
    for (uint32_t m = 0; m < n_old; m++) {
        const ctl_kernel_mesh& k = old.meshes[m];
        t0[m] = k.tri_offset; r0[m] = k.bvh_tri_offset / 3; b0[m] = k.bvh_node_offset / 4;
        if (k.bvh_tri_offset % 3 || k.bvh_node_offset % 4 || k.bvh_index_offset != r0[m] || (m == 0 && (t0[0] || r0[0] || b0[0])) || (m && (t0[m] < t0[m - 1] || r0[m] < r0[m - 1] || b0[m] < b0[m - 1])))
            throw std::runtime_error(who + "the meshes the scene holds are not laid out in mesh order as the builder lays them out (mesh " + std::to_string(m) + "): re-create the scene");
    }
    t0[n_old] = old.n_tri_data; r0[n_old] = old.n_woop; b0[n_old] = old.n_bvh_nodes;
    if (t0[n_old] < t0[n_old - 1] || r0[n_old] < r0[n_old - 1] || b0[n_old] < b0[n_old - 1]) throw std::runtime_error(who + "the last mesh the scene holds starts behind the end of an array");
    cut.mesh_tri_delta.assign(n_old, 0u); cut.mesh_row_delta.assign(n_old, 0u); cut.mesh_node_delta.assign(n_old, 0u);
    bool open = false;
    for (uint32_t m = 0; m < n_old; m++) {
        cut.mesh_tri_delta[m] = cut.removed_tris; cut.mesh_row_delta[m] = cut.removed_rows; cut.mesh_node_delta[m] = cut.removed_nodes;
        if (cut.new_of_old[m] == kNodesNone) { cut.removed_tris += t0[m + 1] - t0[m]; cut.removed_rows += r0[m + 1] - r0[m]; cut.removed_nodes += b0[m + 1] - b0[m]; open = false; continue; }
        if (!open) {
            cut.tri_src.push_back(t0[m]); cut.tri_dst.push_back(t0[m] - cut.removed_tris); cut.row_src.push_back(r0[m]); cut.row_dst.push_back(r0[m] - cut.removed_rows);
            cut.node_src.push_back(b0[m]); cut.node_dst.push_back(b0[m] - cut.removed_nodes); open = true;
        }
    }
    cut.kept_tris = old.n_tri_data - cut.removed_tris; cut.kept_rows = old.n_woop - cut.removed_rows; cut.kept_nodes = old.n_bvh_nodes - cut.removed_nodes;
}

void plan_mesh_set(const node_set_basis& old, const geometry_hashes& old_geom, const ctl_scene_desc& nd, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes,
                   const uint32_t* old_of_new, uint32_t n_new_nodes, const std::vector<uint8_t>* device_owned, node_set_plan& plan, mesh_set_change& out, const char* who_) {
    const std::string who = std::string(who_) + ": ";
    if (!old.filled) throw std::runtime_error(who + "the description the tree was made from is not known");
    if (n_new_meshes != nd.n_meshes) throw std::runtime_error(who + "the mesh map has " + std::to_string(n_new_meshes) + " elements, the new description " + std::to_string(nd.n_meshes) + " meshes");
    out = mesh_set_change();
    plan_mesh_compaction(old, old_mesh_of_new, n_new_meshes, who, out.cut);
    const mesh_compaction& cut = out.cut;
    if (!cut.removes()) {   // nothing removed: ctl_scene_update_meshes' checks (with nothing appended either, ctl_scene_update_nodes')
        plan_node_set(old, old_geom, nd, old_of_new, n_new_nodes, device_owned, plan, who_, &out.grow);
        out.hash_ms = out.grow.hash_ms;
        return;
    }
    const uint32_t n_old = (uint32_t)old.meshes.size(), n_old_nodes = (uint32_t)old.nodes.size();
    if (device_owned && device_owned->size() != n_old) device_owned = nullptr;
    if (device_owned) for (uint32_t m = 0; m < n_old; m++) if ((*device_owned)[m] && cut.new_of_old[m] == kNodesNone)
        throw std::runtime_error(who + "mesh " + std::to_string(m) + " is bound to a skin and cannot be removed: ctl_scene_unbind_skin first");
    if (!old_of_new) throw std::runtime_error(who + "null node map");
    for (uint32_t k = 0; k < n_new_nodes; k++) {
        const uint32_t o = old_of_new[k];
        if (o == kNodesNone || o >= n_old_nodes) continue;   // (an element outside the old nodes: plan_node_set's refusal)
        const uint32_t m = old.nodes[o].mesh_index;
        if (m < n_old && cut.new_of_old[m] == kNodesNone) throw std::runtime_error(who + "kept node " + std::to_string(k) + " (was " + std::to_string(o) + ") instances mesh " + std::to_string(m) + ", which the mesh map removes");
    }
    if (nd.n_meshes && !nd.meshes) throw std::runtime_error(who + "the new description lacks its mesh array");
    // the scene as it would be had the removed meshes never been added: what the new description must equal in its kept part, and append to
    node_set_basis cb = old;
    cb.meshes.clear();
    for (uint32_t m = 0; m < n_old; m++) {
        if (cut.new_of_old[m] == kNodesNone) continue;
        ctl_kernel_mesh k = old.meshes[m];
        k.tri_offset -= cut.mesh_tri_delta[m]; k.bvh_tri_offset -= cut.mesh_row_delta[m] * 3; k.bvh_index_offset -= cut.mesh_row_delta[m]; k.bvh_node_offset -= cut.mesh_node_delta[m] * 4;
        const uint32_t at = (uint32_t)cb.meshes.size();
        if (std::memcmp(&nd.meshes[at], &k, sizeof(k)) != 0)
            throw std::runtime_error(who + "kept mesh " + std::to_string(at) + " (was " + std::to_string(m) + ") has another record than the held one with its offsets lowered by what was removed in front of it (" +
                                     std::to_string(cut.mesh_tri_delta[m]) + " triangles, " + std::to_string(cut.mesh_row_delta[m]) + " rows, " + std::to_string(cut.mesh_node_delta[m]) + " BVH nodes)");
        cb.meshes.push_back(k);
    }
    for (ctl_node& n : cb.nodes) n.mesh_index = n.mesh_index < n_old ? cut.new_of_old[n.mesh_index] : kNodesNone;
    cb.n_tri_data = cut.kept_tris; cb.n_woop = cut.kept_rows; cb.n_bvh_nodes = cut.kept_nodes;
    plan_node_set(cb, geometry_hashes(), nd, old_of_new, n_new_nodes, nullptr, plan, who_, &out.grow);   // (without hashes: they are compared mesh by mesh below)
    if (!old_geom.empty()) {
        if (old_geom.mesh_structure.size() != (size_t)n_old * 2 || old_geom.values.size() != (size_t)n_old * 2) throw std::runtime_error(who + "the hashes the scene holds carry no per-mesh structure words");
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<uint8_t> owned_new;
        if (device_owned) { owned_new.assign(nd.n_meshes, 0); for (uint32_t m = 0; m < n_old; m++) if ((*device_owned)[m]) owned_new[cut.new_of_old[m]] = 1; }
        hash_geometry(nd, plan.geom, device_owned ? &owned_new : nullptr);
        out.hash_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (plan.geom.images != old_geom.images || plan.geom.tables[0] != old_geom.tables[0] || plan.geom.tables[1] != old_geom.tables[1])
            throw std::runtime_error(who + "the texels or transmittance tables differ; re-create the scene");
        for (uint32_t m = 0; m < n_old; m++) {
            const uint32_t k = cut.new_of_old[m];
            if (k == kNodesNone) continue;
            if (!plan.geom.same_mesh_structure(k, old_geom, m)) throw std::runtime_error(who + "kept mesh " + std::to_string(k) + " (was " + std::to_string(m) + ") has another structure (woop_index, mesh BVH links) than the scene holds; re-create the scene");
            if (device_owned && (*device_owned)[m]) { plan.geom.values[2 * (size_t)k] = old_geom.values[2 * (size_t)m]; plan.geom.values[2 * (size_t)k + 1] = old_geom.values[2 * (size_t)m + 1]; continue; }
            if (plan.geom.values[2 * (size_t)k] != old_geom.values[2 * (size_t)m] || plan.geom.values[2 * (size_t)k + 1] != old_geom.values[2 * (size_t)m + 1])
                throw std::runtime_error(who + "kept mesh " + std::to_string(k) + " (was " + std::to_string(m) + ") has other vertex values than the scene holds: apply them with ctl_scene_update first");
        }
    }
    plan.identity = false;   // any removal rebuilds, as any growth does
    plan.node_tri_delta.assign(n_old_nodes, 0u);
    for (uint32_t o = 0; o < n_old_nodes; o++) if (old.nodes[o].mesh_index < n_old) plan.node_tri_delta[o] = cut.mesh_tri_delta[old.nodes[o].mesh_index];
    plan.cut = &out.cut;
}

void update_mesh_set_flat_scene(flat_scene& F, const node_set_basis& old, const ctl_scene_desc& nd, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes,
                                const uint32_t* old_of_new, uint32_t n_new_nodes, std::vector<uint32_t>& extra_missing, int builder) {
    const char* who = "ctl_flat_bvh_update_mesh_set";
    rebuild_last_rounds() = 0u;
    rebuild_refuse(F.format, F.refit.ready() && F.refit.part_index.size() == F.leaves.size(), F.compact_links, F.leaves.size(), who);
    node_set_plan plan; mesh_set_change change;
    plan_mesh_set(old, F.refit.geom, nd, old_mesh_of_new, n_new_meshes, old_of_new, n_new_nodes, nullptr, plan, change, who);
    apply_node_set_flat(F, old, nd, old_of_new, n_new_nodes, plan, extra_missing, builder, who);
}

}  // namespace ctl
