// flat_mesh_set.h — another SET OF MESHES for a live scene (ctl_scene_update_mesh_set, ctl_flat_bvh_update_mesh_set): meshes REMOVED, on top of what flat_meshes.h appends
// and flat_nodes.h does to the node set.  The geometry arrays are dense and every offset the kernels read assumes so; there is no free list.  Removal is COMPACTION: the
// kept meshes' ranges move down over the holes, on the device, and everything that names a global triangle or row follows.
//
// The builder lays the meshes out in mesh order in tri_data, the Woop stream (with woop_index beside it) and bvh_nodes, so the kept meshes form the same RUNS in all three
// arrays: maximal groups of kept meshes that are consecutive.  A run has, per array, a source start, a destination start and a length; a removal in a scene of ten thousand
// meshes gives a handful of runs.  What moves:
//   tri_data, mesh BVH nodes, leaf stream   element i of the compacted array is element src[j] + (i - dst[j]) of the held one, j = the run i lies in (mesh_set_source: the binary
//                                           search nodes_find_added is, over dst[]).  The contents are mesh-relative (index words, node links) and move unchanged
//   triangle -> row table                   the word of the source triangle minus the run's ROW delta; "no row" stays (mesh_set_row_word)
//   leaf entries of the flattened tree      word 12 is globalTri << 1: minus the TRIANGLE delta of the entry's mesh while the entry moves (mesh_set_entry_index; flat_nodes.hip
//                                           k_nodes_move, flat_nodes.cpp step 1)
// The arithmetic is single source for the kernels (flat_mesh_set.hip) and the host re-statement (flat_mesh_set.cpp).
#pragma once
#include "flat_meshes.h"
#include <algorithm>

namespace ctl {

// the element of the held array that element i of the compacted one is a copy of; dst[0] == 0 <= i
CTL_REFIT_HD uint32_t mesh_set_source(const uint32_t* dst, const uint32_t* src, uint32_t n_runs, uint32_t i) {
    const uint32_t j = nodes_find_added(dst, n_runs, i);
    return src[j] + (i - dst[j]);
}
CTL_REFIT_HD uint32_t mesh_set_row_word(uint32_t held, uint32_t row_delta) { return held == kNodesNone || held < row_delta ? kNodesNone : held - row_delta; }
CTL_REFIT_HD uint32_t mesh_set_entry_index(uint32_t index_word, uint32_t tri_delta) { return index_word - (tri_delta << 1); }

// ---- host side
// the removal half of an accepted mesh map: counts are elements of the description's arrays (triangles, rows of the Woop stream, BVH nodes)
struct mesh_compaction {
    std::vector<uint32_t> new_of_old;                  // per held mesh: its new index, or kNodesNone = removed
    std::vector<uint32_t> mesh_tri_delta, mesh_row_delta, mesh_node_delta;   // per held mesh: what was removed in front of it
    uint32_t kept_meshes = 0, kept_tris = 0, kept_rows = 0, kept_nodes = 0;  // the compacted counts: what an appended mesh must follow
    uint32_t removed_meshes = 0, removed_tris = 0, removed_rows = 0, removed_nodes = 0;
    std::vector<uint32_t> tri_dst, tri_src, row_dst, row_src, node_dst, node_src;   // the runs, ascending; the same number in every array
    bool removes() const { return removed_meshes != 0; }
    uint32_t runs() const { return (uint32_t)tri_dst.size(); }
    uint32_t new_triangle(uint32_t old_tri) const {    // the new global index of a held triangle, or kNodesNone: its mesh was removed
        const auto it = std::upper_bound(tri_src.begin(), tri_src.end(), old_tri);
        if (it == tri_src.begin()) return kNodesNone;
        const size_t j = (size_t)(it - tri_src.begin()) - 1;
        const uint32_t len = (j + 1 < tri_dst.size() ? tri_dst[j + 1] : kept_tris) - tri_dst[j];
        return old_tri - tri_src[j] < len ? tri_dst[j] + (old_tri - tri_src[j]) : kNodesNone;
    }
};
// what ctl_scene_update_mesh_set's checks hand to the stages: the removal, then the append measured from the compacted counts
struct mesh_set_change { mesh_compaction cut; mesh_set_plan grow; float hash_ms = 0; };

// Everything both callers refuse before anything is written (std::runtime_error -> CTL_ERR_INVALID).  The mesh map: old_mesh_of_new[m] = the held mesh that new mesh m was,
// or UINT32_MAX for an appended one; kept meshes strictly increasing (no reordering), appended ones all behind them.  With nothing removed the rest is
// plan_node_set(..., &grow), unchanged.  With a removal: no removed mesh is device-owned (bound to a skin); no kept node names a removed mesh; every kept mesh's record is the
// held one with its offsets lowered by the sizes removed in front of it; then plan_node_set's rules against the COMPACTED basis (node map, appended meshes behind the
// compacted ends, images, materials, kept nodes' mesh through the map, check_scene_desc); then ONE hash pass over `nd`: per kept mesh the structure words
// (geometry_hash.h mesh_structure) and — outside device-owned meshes, whose words are carried — the value words equal the held ones through the map, images and
// transmittance tables equal.  `plan` then never is an identity, carries the per-old-node triangle deltas and points at out.cut, which must outlive it.
void plan_mesh_set(const node_set_basis& old, const geometry_hashes& old_geom, const ctl_scene_desc& nd, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes,
                   const uint32_t* old_of_new, uint32_t n_new_nodes, const std::vector<uint8_t>* device_owned, node_set_plan& plan, mesh_set_change& out, const char* who);
// the mesh map alone against the held records (the first step of plan_mesh_set, and the test hook ctl_compact_tri_rows_host): `cut` whole.  Refuses a map that reorders,
// keeps a mesh behind an appended one or names a mesh the scene does not hold, and — for a removal — held records that are not in the builder's layout
void plan_mesh_compaction(const node_set_basis& old, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes, const std::string& who, mesh_compaction& cut);
// a list of held triangles (ascending) in the new numbering, those of removed meshes dropped.  (Inline, like new_triangle: the node-set stages call it, and link without
// flat_mesh_set.cpp where they are built alone)
inline void mesh_set_rebase_triangles(std::vector<uint32_t>& tris, const mesh_compaction& cut) {
    size_t n = 0;
    for (uint32_t t : tris) { const uint32_t k = cut.new_triangle(t); if (k != kNodesNone) tris[n++] = k; }
    tris.resize(n);
}
// the host re-statement of k_compact_tri_rows: the compacted table (cut.kept_tris words) from the held one
void compact_tri_rows_host(const mesh_compaction& cut, const uint32_t* held_rows, uint32_t n_held, uint32_t* out);
// ctl_flat_bvh_update_mesh_set: the checks, then update_nodes_flat_scene's stages (flat_nodes.cpp apply_node_set_flat), which rebase the kept entries' triangle words
struct flat_scene;
void update_mesh_set_flat_scene(flat_scene& F, const node_set_basis& old, const ctl_scene_desc& nd, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes,
                                const uint32_t* old_of_new, uint32_t n_new_nodes, std::vector<uint32_t>& extra_missing, int builder = 0);

}  // namespace ctl
