// geometry_hash.h — what a scene keeps of the geometry arrays of the description it was made from (scene_update.hip), and what ctl_scene_desc_diff tells
// CTL_DIFF_GEOMETRY from CTL_DIFF_TOPOLOGY by: one 128-bit hash of the STRUCTURE and one per mesh of the VALUES, made in a single pass over the arrays.
//   structure   the counts, woop_index, the links of the mesh BVH nodes (child0, child1, parent, pad), transmittance tables — and whatever part of the
//               triangle / Woop / node arrays lies in front of the first mesh's range
//   images[i]   image i's size and level-0 texels.  Another texel is a difference of STRUCTURE as it always was (same_structure compares these words too); they are kept
//               per image so that ctl_scene_update_image (scene_images.hip), which replaces one image's texels in place, can replace that image's words
//   values[m]   mesh m's ranges of tri_data and woop, and the float boxes (the first 48 B) of its bvh_nodes
//   mesh_structure[m]  mesh m's own share of the structure, from the same pass: its woop_index words and the links of its BVH nodes.  Both are MESH-RELATIVE (an index word
//               names a triangle of the mesh, a link a node or a leaf row of the mesh; the offsets are added per instance, tracer.hip pack_instances), so the words
//               survive a move of the mesh's ranges: what ctl_scene_update_mesh_set (flat_mesh_set.h) compares mesh by mesh, where the whole-array hash changes with any
//               removal.  tables: the transmittance tables' share alone, for the same caller.  same_structure reads neither
// A description whose structure hash (and counts, meshes, node -> mesh / material assignment) equals the scene's differs from it in geometry VALUES at most, and
// the per-mesh hashes say in which meshes: the ones an update re-uploads and whose leaf entries it rewrites.
#pragma once
#include "../../include/ctl_amd.h"
#include <cstdint>
#include <vector>

namespace ctl {

// [first, last) of every mesh in the three geometry arrays: a mesh's range ends where the next one (by offset) starts, the last one's at the array's end;
// offsets beyond an array are held to its end, so that a range never reaches outside
struct mesh_ranges {
    std::vector<uint32_t> tri0, tri1, woop0, woop1, node0, node1;
    explicit mesh_ranges(const ctl_scene_desc& d);
};

struct geometry_hashes {
    uint64_t structure[2] = { 0, 0 };
    std::vector<uint64_t> values;   // two words per mesh
    std::vector<uint64_t> images;   // two words per image
    std::vector<uint64_t> mesh_structure;   // two words per mesh
    uint64_t tables[2] = { 0, 0 };
    bool same_mesh_structure(size_t m, const geometry_hashes& o, size_t om) const { return mesh_structure.size() > 2 * m + 1 && o.mesh_structure.size() > 2 * om + 1 && mesh_structure[2 * m] == o.mesh_structure[2 * om] && mesh_structure[2 * m + 1] == o.mesh_structure[2 * om + 1]; }
    bool same_structure(const geometry_hashes& o) const { return structure[0] == o.structure[0] && structure[1] == o.structure[1] && values.size() == o.values.size() && images == o.images; }
    bool same_values(const geometry_hashes& o, size_t m) const { return values[2 * m] == o.values[2 * m] && values[2 * m + 1] == o.values[2 * m + 1]; }
    // a mesh whose values in HBM are no description's any more (ctl_scene_unbind_skin): the two words no digest is expected to give, so that every later comparison
    // finds the mesh changed; hash_geometry writes the same words for a mesh it was told to skip, and a diff that ignores a mesh carries them forward.  Idempotent.
    void invalidate_values(size_t m) { if (values.size() > 2 * m + 1) values[2 * m] = values[2 * m + 1] = 0; }
    bool empty() const { return values.empty() && !structure[0] && !structure[1]; }
};
// the two words of one image: width, height and, where `texels` is given, the width * height level-0 texels
void hash_image(uint32_t width, uint32_t height, const uint32_t* texels, uint64_t out[2]);
// skip_values (may be null, else one byte per mesh): the value ranges of a marked mesh are not read and its two words are 0
void hash_geometry(const ctl_scene_desc& d, geometry_hashes& out, const std::vector<uint8_t>* skip_values = nullptr);

}  // namespace ctl
