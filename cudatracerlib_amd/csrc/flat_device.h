// flat_device.h — what flat_rebuild.hip and flat_nodes.hip share on the device side of a live scene's flattened tree: the rebuild of the tree in buffers of its own
// (flat_rebuilder, a friend of Scene: it reads the scene's buffers and swaps the new ones in), which Scene::rebuild_flat runs over the scene's entries and
// Scene::update_nodes over the entries it has assembled.
#pragma once
#include "tracer.h"
#include "flat_rebuild.h"
#include "flat_ploc.h"
#include "flat_nodes.h"
#include <utility>

namespace ctl {

template <typename T> void swap_buffers(dbuf<T>& a, dbuf<T>& b) { std::swap(a.p, b.p); std::swap(a.n, b.n); }
inline dim3 blocks_for(size_t n) { return dim3((unsigned)((n + 255u) / 256u)); }

// what the node-set stages (flat_rebuilder::apply_node_set, flat_nodes.hip) read of the two-level geometry: the scene's own arrays (Scene::update_nodes) or grown ones that are not
// the scene's yet (flat_rebuilder::update_meshes).  Counts in elements of the pointer's type; tri_row may be null (see apply_node_set)
struct node_set_view { const float4* leaf_tris; size_t n_leaf_tris; const uint4* tri_data; const uint32_t* tri_row; size_t n_tri_row; };
// the geometry arrays of a scene with appended meshes (flat_meshes.hip), in buffers of their own until apply_node_set swaps them in; tri_row: null on a two-level scene
struct mesh_growth { dbuf<uint4> tri_data; dbuf<float4> bot_nodes, leaf_tris; dbuf<uint32_t> tri_row; };
// the staging of appended tails and their layout into such buffers (flat_meshes.hip): alloc, then run once the front part of the buffers is on its way
struct mesh_tail_stage {
    dbuf<float4> raw; dbuf<uint32_t> words, first, index_offset, tri_offset;
    void alloc(const mesh_set_plan& grow);
    void run(mesh_growth& Gr, const ctl_scene_desc& d, const mesh_set_plan& grow);
};
struct mesh_set_change;   // flat_mesh_set.h
// scene_images.hip: the pyramid of one image from its level 0, in place in the pool — one k_mip_level launch per level on the null stream, nothing waited for.  level0: the
// image's first texel (device); width, height, type: the image's; L: its level table
void launch_mip_levels(uint32_t* level0, uint32_t width, uint32_t height, uint32_t type, const dev_mip_levels& L);

// The rebuild of flat_rebuild.h on the device over n entries (and the closing entry behind them) that need not be the scene's own: ctl_scene_rebuild_flat runs it over
// flat_leaves_, ctl_scene_update_nodes over the entries it has just assembled.  Three steps, so that a caller can put its own work between them:
//   allocate   every buffer of the new tree; nothing of the scene is written (the scratch that has no meaning between calls — rocPRIM's storage, the entry boxes, the carry
//              matrices — grows in place)
//   run        stages 1 - 9 into the new buffers; a tree too deep for the traversal stack is refused here (unsupported_error), the scene still as it was
//   commit     the swap: tracers read S at every launch
struct flat_rebuilder {
    const char* who = "";
    int builder = CTL_REBUILD_LBVH;       // set where the rebuilder is made: Scene::rebuild_flat and Scene::update_nodes read rebuild_builder_choice() there
    uint32_t n = 0;                       // entries
    float4* src_leaves = nullptr; uint32_t* src_part = nullptr;   // what the tree is built over; src_leaves holds n + 1 entries
    refit_device R{};                     // the caller fills inst, inst_fwd, restamp, leaf_keys, alpha_maps, tri_data, node_info, mats; the rest is set by allocate()
    // results
    uint32_t n_nodes = 0; int max_depth = 0; std::vector<uint32_t> level_start; double area[2] = { 0, 0 }; float ms[4] = { 0, 0, 0, 0 };   // entry boxes, sort, topology, node boxes
    uint32_t rounds = 0;                  // of the clustering (CTL_REBUILD_PLOC)
    void allocate(Scene& A, const std::vector<double>& carry_matrices);
    void run(Scene& A);
    void commit(Scene& A);
    void report(ctl_scene_rebuild_stats& st) const;
    // The node-set stages behind Scene::update_nodes' checks (flat_nodes.hip), and ctl_scene_update_meshes (flat_meshes.hip): the growth of the geometry arrays for appended
    // meshes in front of the same stages; with nothing appended it is Scene::update_nodes.  Both work on the scene's private buffers as the rebuild does.  They stand here,
    // as static functions of the scene's friend, and not in class Scene: tracer.h is one of the sources of bench.py's traversal-kernel hash (KERNEL_BUILD), so a declaration
    // there would retire the committed traffic profile for a change that touches no kernel the profile measures.
    static void apply_node_set(Scene& A, const ctl_scene_desc& d, const uint32_t* old_of_new, const node_set_basis& basis, const node_set_plan& plan, const node_set_view& V, mesh_growth* grown,
                               ctl_scene_nodes_stats* stats, const char* who);
    static size_t read_tri_rows(Scene& A, uint32_t* rows_out, size_t capacity);   // ctl_scene_read_triangle_rows: the words of the scene's triangle -> row table (0: none yet)
    static void update_meshes(Scene& A, const ctl_scene_desc& d, const uint32_t* old_of_new, uint32_t n_new_nodes, const node_set_basis& basis, ctl_scene_meshes_stats* stats);
    static void apply_mesh_growth(Scene& A, const ctl_scene_desc& d, const uint32_t* old_of_new, const node_set_basis& basis, const node_set_plan& plan, const mesh_set_plan& grow,
                                  ctl_scene_meshes_stats* stats, const char* who);   // update_meshes behind its checks
    // ctl_scene_update_mesh_set (flat_mesh_set.hip): meshes removed — the geometry arrays compacted on the device into new buffers —, meshes appended and the node set changed in
    // one call; with nothing removed it is update_meshes.  remap_skins (mesh_skin.hip): the bound meshes under their new indices, called where the compacted buffers become the scene's
    static void update_mesh_set(Scene& A, const ctl_scene_desc& d, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes, const uint32_t* old_of_new, uint32_t n_new_nodes,
                                const node_set_basis& basis, ctl_scene_mesh_set_stats* stats);
    static void remap_skins(Scene& A, const mesh_compaction& cut, const ctl_scene_desc& d);
    // ctl_scene_update behind its diff (scene_update.hip): Scene::update is scene_desc_diff + this; ctl_scene_update_image_set comes here with the mask of scene_desc_diff_small
    static uint32_t apply_update(Scene& A, const ctl_scene_desc& d, uint32_t mask, const geometry_hashes& geom, ctl_scene_update_stats* stats);
    // ctl_scene_update_image_set (scene_image_set.hip): images removed, added and replaced by ones of another size — the kept pyramids moved on the device into a new texel
    // pool, the fresh ones uploaded and built there —, then the stages of ctl_scene_update over the rest of d; with an identity map it is Scene::update
    static void update_image_set(Scene& A, const ctl_scene_desc& d, const uint32_t* old_image_of_new, uint32_t n_new_images, const node_set_basis& basis, ctl_scene_image_set_stats* stats);
    flat_rebuilder() {}
    flat_rebuilder(const flat_rebuilder&) = delete; flat_rebuilder& operator=(const flat_rebuilder&) = delete;
    ~flat_rebuilder();
private:
    uint32_t cap = 0; hipEvent_t ev[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    dbuf<refit_box> ebox_new, nbox_new; dbuf<uint32_t> bounds, idx_in, idx_out, first, last, perm, part_new, level_iota; dbuf<uint64_t> keys_in, keys_out, counts, incl;
    dbuf<float4> nodes_new, leaves_new; dbuf<double> area_dev;
    // CTL_REBUILD_PLOC alone: the clusters' boxes and ids (read from one, written to the other), every cluster's pick, the round's flag words and their scan, the stored tree
    dbuf<refit_box> cbox[2]; dbuf<uint32_t> cid[2], pick, tree_left, tree_right, tree_count; dbuf<uint64_t> round_flags, round_incl;
    void cluster(Scene& A);
    template <typename Tree> void wide_nodes(Scene& A, const Tree& T);
};

}  // namespace ctl
