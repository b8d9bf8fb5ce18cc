// flat_meshes.h — NEW MESHES for a live scene (ctl_scene_update_meshes, ctl_flat_bvh_update_meshes): the step in front of flat_nodes.h's node-set stages.  A description
// made after further add_mesh calls is the held description plus tails of tri_data, woop, woop_index, bvh_nodes and meshes (scene_builder.cpp only ever appends), so the
// geometry arrays in HBM grow by their tails — the old contents are copied on the device: deformed and posed values live nowhere else — and the rows of the appended
// range are laid out as creation lays them out (tracer.hip):
//   row w of the two-level leaf stream   64 B: Woop rows a, b, c, then { index word, 0, 0, 0 } (meshes_row_words)
//   triangle -> row table                tri_row[mesh.tri_offset + (index >> 1)] = the FIRST row in stream order that names the triangle (triangle_woop_rows, flatten.h):
//                                        a minimum over the rows (meshes_table_rule), so the order in which rows arrive does not matter; the device takes it with atomicMin
// The arithmetic is single source for the kernel (flat_meshes.hip k_append_leaf_rows) and the host re-statement (flat_meshes.cpp append_leaf_rows_host).
#pragma once
#include "flat_nodes.h"
#include <string>

namespace ctl {

constexpr uint32_t kMeshesFillerIndex = 1u;   // the index word of a row without a woop_index slot, as Scene::upload_mesh_geometry writes it; the table skips such a row

// the 16 words of row w of the leaf stream from the raw ctl_woop_tri (12 floats) and its index word
CTL_REFIT_HD void meshes_row_words(const float raw[12], uint32_t index_word, uint32_t out[16]) {
    for (int k = 0; k < 12; k++) out[k] = refit_f2u(raw[k]);
    out[12] = index_word; out[13] = 0u; out[14] = 0u; out[15] = 0u;
}
// the slot of woop_index that holds row w's index word — w is the (w - first_row)-th row of its mesh —, or kNodesNone: no slot inside [row0, n_rows)
CTL_REFIT_HD uint32_t meshes_index_slot(uint32_t index_offset, uint32_t first_row, uint32_t w, uint32_t row0, uint32_t n_rows) {
    const uint64_t at = (uint64_t)index_offset + (w - first_row);
    return at >= row0 && at < n_rows ? (uint32_t)at : kNodesNone;
}
// the triangle (global index) a row's index word names, or kNodesNone: outside the triangle array
CTL_REFIT_HD uint32_t meshes_row_triangle(uint32_t tri_offset, uint32_t index_word, uint32_t n_tris) {
    const uint64_t tri = (uint64_t)tri_offset + (index_word >> 1);
    return tri < n_tris ? (uint32_t)tri : kNodesNone;
}
// the table's rule: the first reference in stream order stays (kNodesNone, "no row", is the largest value)
CTL_REFIT_HD uint32_t meshes_table_rule(uint32_t held, uint32_t row) { return row < held ? row : held; }

// ---- host side
// what an accepted description appends (plan_node_set with a mesh_set_plan, flat_nodes.h)
struct mesh_set_plan {
    uint32_t old_meshes = 0, old_tri_data = 0, old_woop = 0, old_bvh_nodes = 0;            // the held counts
    uint32_t meshes_added = 0, triangles_added = 0, rows_added = 0, bvh_nodes_added = 0;
    bool grown() const { return meshes_added || triangles_added || rows_added || bvh_nodes_added; }
    // the appended meshes in the order of their first rows (ascending; first[0] == old_woop when rows were appended): what k_append_leaf_rows searches
    std::vector<uint32_t> first, index_offset, tri_offset;
    float hash_ms = 0;   // host time of the two hashing passes over the new description
};
// the appended rows [P.old_woop, d.n_woop) on the host with the kernel's functions: leaf_rows_out (may be null) 16 words per appended row; tri_row: d.n_tri_data words whose
// first P.old_tri_data hold the old table — the rest is set to kNodesNone first, as the device sets it
void append_leaf_rows_host(const ctl_scene_desc& d, const mesh_set_plan& P, uint32_t* leaf_rows_out, uint32_t* tri_row);
// ctl_flat_bvh_update_meshes: the acceptance check, then update_nodes_flat_scene's stages (flat_nodes.cpp apply_node_set_flat)
void update_meshes_flat_scene(flat_scene& F, const node_set_basis& old, const ctl_scene_desc& nd, const uint32_t* old_of_new, uint32_t n_new_nodes, std::vector<uint32_t>& extra_missing, int builder = 0);
// the mesh_set_plan of a description against held counts alone (the test hook ctl_append_leaf_rows_host): offsets are checked as plan_node_set checks them
void plan_mesh_growth(uint32_t old_meshes, uint32_t old_tri_data, uint32_t old_woop, uint32_t old_bvh_nodes, const ctl_scene_desc& nd, const std::string& who, mesh_set_plan& out);

}  // namespace ctl
