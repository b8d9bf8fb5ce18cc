// flat_meshes.cpp — the host side of appending meshes to a live scene (flat_meshes.h): what an accepted description appends (plan_mesh_growth, the block plan_node_set
// runs for a caller that takes appended meshes), the host re-statement of k_append_leaf_rows (append_leaf_rows_host) and the host yardstick of ctl_scene_update_meshes
// (update_meshes_flat_scene: the acceptance check, then the node-set stages of flat_nodes.cpp, which take their Woop rows from the new description).
#include "flat_meshes.h"
#include "flatten.h"
#include "flat_rebuild.h"
#include <algorithm>
#include <stdexcept>
#include <utility>

namespace ctl {

void plan_mesh_growth(uint32_t old_meshes, uint32_t old_tri_data, uint32_t old_woop, uint32_t old_bvh_nodes, const ctl_scene_desc& nd, const std::string& who, mesh_set_plan& out) {
    out = mesh_set_plan();
    out.old_meshes = old_meshes; out.old_tri_data = old_tri_data; out.old_woop = old_woop; out.old_bvh_nodes = old_bvh_nodes;
    if (nd.n_meshes < old_meshes) throw std::runtime_error(who + "the description has " + std::to_string(nd.n_meshes) + " meshes, the scene holds " + std::to_string(old_meshes) + ": meshes can be appended, not removed; re-create the scene");
    if (nd.n_tri_data < old_tri_data || nd.n_woop < old_woop || nd.n_bvh_nodes < old_bvh_nodes) throw std::runtime_error(who + "a geometry array is shorter than the one the scene holds: meshes can be appended, not removed; re-create the scene");
    if ((nd.n_tri_data && !nd.tri_data) || (nd.n_woop && (!nd.woop || !nd.woop_index)) || (nd.n_bvh_nodes && !nd.bvh_nodes)) throw std::runtime_error(who + "the new description lacks its geometry arrays");
    out.meshes_added = nd.n_meshes - old_meshes; out.triangles_added = nd.n_tri_data - old_tri_data; out.rows_added = nd.n_woop - old_woop; out.bvh_nodes_added = nd.n_bvh_nodes - old_bvh_nodes;
    if (nd.n_meshes && !nd.meshes) throw std::runtime_error(who + "the new description lacks its mesh array");
    std::vector<std::pair<uint32_t, uint32_t>> order;   // (first row, mesh)
    uint32_t first_tri = nd.n_tri_data, first_node = nd.n_bvh_nodes;
    for (uint32_t m = old_meshes; m < nd.n_meshes; m++) {
        const ctl_kernel_mesh& k = nd.meshes[m];
        const std::string mesh = "appended mesh " + std::to_string(m);
        if (k.tri_offset < old_tri_data || k.tri_offset > nd.n_tri_data) throw std::runtime_error(who + mesh + " has its triangles at " + std::to_string(k.tri_offset) + ", not behind the " + std::to_string(old_tri_data) + " the scene holds and inside the new array");
        if (k.bvh_tri_offset / 3 < old_woop || k.bvh_tri_offset / 3 > nd.n_woop || k.bvh_index_offset < old_woop || k.bvh_index_offset > nd.n_woop)
            throw std::runtime_error(who + mesh + " has its leaf rows or index words not behind the " + std::to_string(old_woop) + " the scene holds and inside the new arrays");
        if (k.bvh_node_offset / 4 < old_bvh_nodes || k.bvh_node_offset / 4 > nd.n_bvh_nodes) throw std::runtime_error(who + mesh + " has its BVH nodes not behind the " + std::to_string(old_bvh_nodes) + " the scene holds and inside the new array");
        order.emplace_back(k.bvh_tri_offset / 3, m); first_tri = std::min(first_tri, k.tri_offset); first_node = std::min(first_node, k.bvh_node_offset / 4);
    }
    std::sort(order.begin(), order.end());
    // an element belongs to the mesh whose range it lies in, and a mesh's range ends where the next one starts (mesh_ranges): appended elements in front of the first
    // appended mesh would lengthen the last held mesh's range — its value hash in the snapshot would no longer be the one that was checked, and its appended rows would
    // have their index words outside the appended ones.  So in all three arrays the first appended mesh starts exactly where the held elements end
    if (out.rows_added && (order.empty() || order.front().first != old_woop)) throw std::runtime_error(who + "the leaf rows from " + std::to_string(old_woop) + " on belong to no appended mesh: the first appended mesh must start where the held rows end");
    if (out.triangles_added && (order.empty() || first_tri != old_tri_data)) throw std::runtime_error(who + "the triangles from " + std::to_string(old_tri_data) + " on belong to no appended mesh: the first appended mesh must start where the held triangles end");
    if (out.bvh_nodes_added && (order.empty() || first_node != old_bvh_nodes)) throw std::runtime_error(who + "the BVH nodes from " + std::to_string(old_bvh_nodes) + " on belong to no appended mesh: the first appended mesh must start where the held nodes end");
    for (const auto& o : order) { out.first.push_back(o.first); out.index_offset.push_back(nd.meshes[o.second].bvh_index_offset); out.tri_offset.push_back(nd.meshes[o.second].tri_offset); }
}

void append_leaf_rows_host(const ctl_scene_desc& d, const mesh_set_plan& P, uint32_t* leaf_rows_out, uint32_t* tri_row) {
    for (uint32_t t = P.old_tri_data; t < d.n_tri_data; t++) tri_row[t] = kNodesNone;
    const uint32_t n_meshes = (uint32_t)P.first.size();
    for (uint32_t w = P.old_woop; w < d.n_woop; w++) {   // the kernel's lane w
        const uint32_t j = nodes_find_added(P.first.data(), n_meshes, w);
        const uint32_t at = meshes_index_slot(P.index_offset[j], P.first[j], w, P.old_woop, d.n_woop);
        const uint32_t index_word = at != kNodesNone ? d.woop_index[at].index : kMeshesFillerIndex;
        if (leaf_rows_out) meshes_row_words(reinterpret_cast<const float*>(&d.woop[w]), index_word, leaf_rows_out + (size_t)(w - P.old_woop) * 16);
        if (at == kNodesNone) continue;
        const uint32_t tri = meshes_row_triangle(P.tri_offset[j], index_word, d.n_tri_data);
        if (tri != kNodesNone) tri_row[tri] = meshes_table_rule(tri_row[tri], w);
    }
}

void update_meshes_flat_scene(flat_scene& F, const node_set_basis& old, const ctl_scene_desc& nd, const uint32_t* old_of_new, uint32_t n_new_nodes, std::vector<uint32_t>& extra_missing, int builder) {
    const char* who = "ctl_flat_bvh_update_meshes";
    rebuild_last_rounds() = 0u;
    rebuild_refuse(F.format, F.refit.ready() && F.refit.part_index.size() == F.leaves.size(), F.compact_links, F.leaves.size(), who);
    node_set_plan plan; mesh_set_plan grow;
    plan_node_set(old, F.refit.geom, nd, old_of_new, n_new_nodes, nullptr, plan, who, &grow);
    apply_node_set_flat(F, old, nd, old_of_new, n_new_nodes, plan, extra_missing, builder, who);   // the node-set stages for every accepted plan; with nothing appended the plan, and so the call, is ctl_flat_bvh_update_nodes'
}

}  // namespace ctl
