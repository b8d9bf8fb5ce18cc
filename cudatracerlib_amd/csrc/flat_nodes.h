// flat_nodes.h — another SET OF NODES for a live scene (ctl_scene_update_nodes, ctl_flat_bvh_update_nodes): the arithmetic, single source for the host yardstick
// (flat_nodes.cpp update_nodes_flat_scene) and the device (flat_nodes.hip), as flat_rebuild.h is for the rebuild that follows.
//
// A node's leaf entries are a pure function of the mesh's Woop rows, the node's inverse transform and the material bits, so the entries of a flattened Q4 tree follow a
// change of the node set without the scene being made again:
//   1. drop and renumber   per entry: its node word (bit 31 is the alpha stamp) through new_of_old[] (kNodesNone = the node was removed) -> kept or dropped; an exclusive
//                          scan over the flags hands out the positions; the 128 B of every kept entry and its part_index word move there, the node word renumbered with
//                          its stamp bit kept (and, where meshes were removed, the triangle word lowered: flat_mesh_set.h).  Stable, no atomic decides a position.  part_boxes stay as they are: a box no entry refers to is harmless
//   2. generate            for every added node in index order, for every triangle of its mesh in mesh order: the triangle's Woop rows (through the triangle -> row table of
//                          triangle_woop_rows, flatten.h); a triangle whose Woop matrix is singular (nodes_rows_regular — the rule gather_references applies at creation) or
//                          that no row stands for gets NO entry; a scan over the regular flags gives the positions behind the kept entries; the entry in flat_leaf's layout:
//                          rows a, b, c; { globalTri << 1, node, 0, 0 }; rows 0..2 of the node's inverse transform; w33.  part_index = kRefitNoPart: an added instance gets
//                          WHOLE-triangle entries — no early split clipping —, so it culls less well on long triangles, never wrongly.  The BSDF-model bits and the alpha bit
//                          are the re-stamp's work (flat_refit.hip k_refit_entries), which runs over every entry next
//   3. carry data          xf0[] — the pose clip boxes are carried from — is remapped for kept nodes and is the node's own new transform for added ones
//   4. rebuild             the stages of flat_rebuild.h over the new entry count, into buffers of their own
// The triangles skipped in 2 join the scene's list of triangles without an entry: a later geometry update that makes one regular is refused for the new node too.
#pragma once
#include "flat_refit.h"
#include "geometry_hash.h"
#include "../../include/ctl_amd.h"
#include <vector>

namespace ctl {

constexpr uint32_t kNodesNone = 0xffffffffu;        // old_of_new: an added node; new_of_old: a removed one
constexpr uint32_t kNodesStampBit = 0x80000000u;    // bit 31 of an entry's node word: "its material has an alpha map" (tracer.hip)

// the new number of the node an entry names, or kNodesNone: the entry is dropped (also an entry whose node word names no node of the old description)
CTL_REFIT_HD uint32_t nodes_new_of(uint32_t node_word, const uint32_t* new_of_old, uint32_t n_old_nodes) {
    const uint32_t node = node_word & ~kNodesStampBit;
    return node < n_old_nodes ? new_of_old[node] : kNodesNone;
}
CTL_REFIT_HD uint32_t nodes_renumber(uint32_t node_word, uint32_t new_node) { return (node_word & kNodesStampBit) | new_node; }
// does the triangle with these Woop rows get an entry?  The matrix refit_entry_box inverts, with its verdict
CTL_REFIT_HD bool nodes_rows_regular(const float wa[4], const float wb[4], const float wc[4]) {
    const double wm[16] = { (double)wb[0], (double)wb[1], (double)wb[2], (double)wb[3], (double)wc[0], (double)wc[1], (double)wc[2], (double)wc[3],
                            (double)wa[0], (double)wa[1], (double)wa[2], -(double)wa[3], 0.0, 0.0, 0.0, 1.0 };
    double inv[16];
    return refit_inv4(wm, inv);
}
// candidate g of the generate stage (the g-th triangle of the added nodes, in node order then mesh order) belongs to added node j: base[j] <= g < base[j + 1]
CTL_REFIT_HD uint32_t nodes_find_added(const uint32_t* base, uint32_t n_added, uint32_t g) {
    uint32_t lo = 0u, hi = n_added;   // base[lo] <= g < base[hi]
    while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (base[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}
// the 32 words of a generated entry (flat_leaf, flatten.h); inv: rows 0..2 of the node's inverse transform, w33: its element (3, 3)
CTL_REFIT_HD void nodes_entry_words(const float wa[4], const float wb[4], const float wc[4], uint32_t tri, uint32_t node, const float inv[12], float w33, uint32_t out[32]) {
    for (int k = 0; k < 4; k++) { out[k] = refit_f2u(wa[k]); out[4 + k] = refit_f2u(wb[k]); out[8 + k] = refit_f2u(wc[k]); }
    out[12] = tri << 1; out[13] = node; out[14] = 0u; out[15] = 0u;
    for (int k = 0; k < 12; k++) out[16 + k] = refit_f2u(inv[k]);
    out[28] = refit_f2u(w33); out[29] = 0u; out[30] = 0u; out[31] = 0u;
}

// ---- host side, shared by both callers
// what the checks need of the description a tree was made from, besides its geometry hashes: the small arrays whole, the geometry arrays as counts
struct node_set_basis {
    std::vector<ctl_kernel_mesh> meshes; std::vector<ctl_node> nodes; std::vector<ctl_mipmap> images;   // (texels null)
    uint32_t n_materials = 0, n_tri_data = 0, n_woop = 0, n_bvh_nodes = 0; bool rough_transmittance = false, filled = false;
    void fill(const ctl_scene_desc& d);
};
struct mesh_compaction;   // flat_mesh_set.h
// a checked change of the node set
struct node_set_plan {
    bool identity = false;                 // same count, old_of_new[k] == k: nothing of this file runs
    std::vector<uint32_t> new_of_old;      // per old node: its new index or kNodesNone
    std::vector<uint32_t> added;           // the added nodes' new indices, ascending
    std::vector<uint32_t> added_tri0;      // per added node: the first triangle of its mesh (global index) ...
    std::vector<uint32_t> added_base;      // ... and the candidates in front of it; one more element: the number of candidates
    geometry_hashes geom;                  // of the new description (values of device-owned meshes carried over)
    // a plan that also REMOVES meshes (flat_mesh_set.h plan_mesh_set; empty / null on every other call, whose stages and bytes are unchanged): per old node the triangles
    // removed in front of its mesh — step 1 lowers the triangle word of the node's kept entries by it —, and the compaction the lists of triangles follow
    std::vector<uint32_t> node_tri_delta;
    const mesh_compaction* cut = nullptr;
};
// Everything both callers refuse before anything is written (std::runtime_error -> CTL_ERR_INVALID): the map, the kept nodes' mesh / material assignment, the mesh set,
// counts, images and tables, the geometry structure and — outside device-owned meshes — values, check_scene_desc of the new description.
// grow (null: the rules above, unchanged): the description may APPEND meshes (flat_meshes.h; ctl_scene_update_meshes) — n_meshes and the three geometry counts at least the
// held ones, the held mesh records a byte-equal prefix, every appended mesh wholly behind the old ends of the arrays, the hashes of the description restricted to the old
// counts equal to the held ones; `*grow` receives what is appended.  `identity` then also needs nothing appended.  device_owned holds one byte per HELD mesh.
struct mesh_set_plan;
void plan_node_set(const node_set_basis& old, const geometry_hashes& old_geom, const ctl_scene_desc& nd, const uint32_t* old_of_new, uint32_t n_new_nodes,
                   const std::vector<uint8_t>* device_owned, node_set_plan& out, const char* who, mesh_set_plan* grow = nullptr);
// the host yardstick (ctl_flat_bvh_update_nodes): steps 1 - 4 on a host handle, the Woop rows from `nd`.  extra_missing: the triangles step 2 skipped are merged in
// (ascending, unique).  Refusals leave F as it was; an identity map is refit_flat_scene(F, nd) where a node has moved, else nothing.
struct flat_scene;
void update_nodes_flat_scene(flat_scene& F, const node_set_basis& old, const ctl_scene_desc& nd, const uint32_t* old_of_new, uint32_t n_new_nodes, std::vector<uint32_t>& extra_missing, int builder = 0);   // builder: CTL_REBUILD_LBVH (0) or CTL_REBUILD_PLOC
// the same after the checks: `plan` is plan_node_set's answer for these arguments (update_meshes_flat_scene, flat_meshes.cpp, comes here with a plan that appends meshes)
void apply_node_set_flat(flat_scene& F, const node_set_basis& old, const ctl_scene_desc& nd, const uint32_t* old_of_new, uint32_t n_new_nodes, const node_set_plan& plan,
                         std::vector<uint32_t>& extra_missing, int builder, const char* who);

}  // namespace ctl
