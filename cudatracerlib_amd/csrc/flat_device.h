// flat_device.h — what flat_rebuild.hip and flat_nodes.hip share on the device side of a live scene's flattened tree.
//
// Scene (tracer.h) keeps its buffers private, and tracer.h is one of the sources the committed counter profile is tied to (bench.py KERNEL_BUILD), so it is left as it
// is: Scene::rebuild_flat — a member, defined in flat_rebuild.hip — makes a flat_scene_state, references to the members the work needs and the private upload blocks as
// callables, and hands it to the free functions below.  ctl_scene_update_nodes enters through the same member: capi.hip posts a node_set_job for the calling thread
// first (post_node_set_job), which rebuild_flat takes instead of rebuilding.
#pragma once
#include "tracer.h"
#include "flat_rebuild.h"
#include "flat_nodes.h"
#include <functional>
#include <utility>

namespace ctl {

struct flat_scene_state {
    Scene& scene; dev_scene& S;
    std::unique_ptr<desc_snapshot>& snap; flat_scene::refit_side& refit; std::vector<uint32_t>& missing_tris; const std::map<uint32_t, std::shared_ptr<skin_binding>>& skins;
    size_t &n_nodes, &n_entries, &slab_nodes; int& max_depth; bool& root_slab;
    dbuf<uint32_t> &tri_row, &part_index, &level_nodes; dbuf<refit_box> &part_boxes, &ebox, &nbox; dbuf<double>& carry; dbuf<unsigned char>& temp;
    dbuf<float4> &top_nodes, &leaf_tris, &inst, &inst_fwd, &flat_nodes, &flat_leaves; dbuf<uint4> &tri_data, &node_info; dbuf<ctl_material>& mats;
    std::function<void(const ctl_scene_desc&)> upload_top_level, upload_lights, upload_materials, bind, set_camera;
    std::function<void(const ctl_scene_desc&, const geometry_hashes*)> snapshot;
    std::function<void(const shading_state&)> set_shading_state;
};

template <typename T> void swap_buffers(dbuf<T>& a, dbuf<T>& b) { std::swap(a.p, b.p); std::swap(a.n, b.n); }
inline dim3 blocks_for(size_t n) { return dim3((unsigned)((n + 255u) / 256u)); }

// The rebuild of flat_rebuild.h on the device over n entries (and the closing entry behind them) that need not be the scene's own: ctl_scene_rebuild_flat runs it over
// flat_leaves_, ctl_scene_update_nodes over the entries it has just assembled.  Three steps, so that a caller can put its own work between them:
//   allocate   every buffer of the new tree; nothing of the scene is written (the scratch that has no meaning between calls — rocPRIM's storage, the entry boxes, the carry
//              matrices — grows in place)
//   run        stages 1 - 9 into the new buffers; a tree too deep for the traversal stack is refused here (unsupported_error), the scene still as it was
//   commit     the swap: tracers read S at every launch
struct flat_rebuilder {
    const char* who = "";
    uint32_t n = 0;                       // entries
    float4* src_leaves = nullptr; uint32_t* src_part = nullptr;   // what the tree is built over; src_leaves holds n + 1 entries
    refit_device R{};                     // the caller fills inst, inst_fwd, restamp, leaf_keys, alpha_maps, tri_data, node_info, mats; the rest is set by allocate()
    // results
    uint32_t n_nodes = 0; int max_depth = 0; std::vector<uint32_t> level_start; double area[2] = { 0, 0 }; float ms[4] = { 0, 0, 0, 0 };   // entry boxes, sort, topology, node boxes
    void allocate(flat_scene_state& A, const std::vector<double>& carry_matrices);
    void run(flat_scene_state& A);
    void commit(flat_scene_state& A);
    void report(ctl_scene_rebuild_stats& st) const;
    flat_rebuilder() {}
    flat_rebuilder(const flat_rebuilder&) = delete; flat_rebuilder& operator=(const flat_rebuilder&) = delete;
    ~flat_rebuilder();
private:
    uint32_t cap = 0; hipEvent_t ev[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    dbuf<refit_box> ebox_new, nbox_new; dbuf<uint32_t> bounds, idx_in, idx_out, first, last, perm, part_new, level_iota; dbuf<uint64_t> keys_in, keys_out, counts, incl;
    dbuf<float4> nodes_new, leaves_new; dbuf<double> area_dev;
};
void rebuild_flat_device(flat_scene_state& A, ctl_scene_rebuild_stats* stats);   // flat_rebuild.hip: ctl_scene_rebuild_flat

// flat_nodes.hip: ctl_scene_update_nodes
struct node_set_job { const ctl_scene_desc* d; const uint32_t* old_of_new; uint32_t n_new_nodes; const node_set_basis* basis; ctl_scene_nodes_stats* stats; };
void post_node_set_job(const node_set_job* job);    // for the calling thread; nullptr withdraws it
const node_set_job* take_node_set_job();
void update_nodes_device(flat_scene_state& A, const node_set_job& job);

}  // namespace ctl
