// flat_mesh_set.hip — meshes removed from a live scene on the device (ctl_scene_update_mesh_set): the compaction of the two-level geometry arrays in front of the append of
// flat_meshes.hip and the node-set stages of flat_nodes.hip.  The functions of flat_mesh_set.h, which the host re-statement (flat_mesh_set.cpp) runs too.
//
//   k_compact_quads     one lane per 16-B quad of the DESTINATION, consecutive lanes consecutive quads: element = quad >> shift (tri_data: 2 quads per triangle, the mesh BVH nodes
//                       and the leaf stream: 4 per node / row), its run by the binary search over the run table in global memory (a handful of words, read by every lane of
//                       a wave at the same addresses except around a run boundary), one uint4 load from the held array, one uint4 store.  Mesh-relative contents move unchanged;
//                       the source is whatever stands in HBM: deformed and posed values survive
//   k_compact_tri_rows  one lane per destination triangle: the source triangle's word of the triangle -> row table minus the run's ROW delta, "no row" kept
//   mesh_tail_stage     (flat_meshes.hip) the appended tails behind the compacted ends, k_append_leaf_rows extending the table
//   apply_node_set      (flat_nodes.hip) the node-set stages over the new buffers: k_nodes_move lowers the triangle word of every kept entry by its mesh's TRIANGLE delta;
//                       the buffers become the scene's where the new tree is committed
// Nothing moves in place: source and destination overlap, and until the commit the scene's own arrays are what a refusal leaves behind.  During the call HBM holds the old
// arrays and the compacted ones.  Plain launches on the null stream between two synchronisations; no workgroup waits for another, no atomic decides a position, no LDS;
// every index is checked against the size of the array it goes into.
#include "flat_device.h"
#include "flat_mesh_set.h"
#include "mitsuba_loader.h"   // unsupported_error
#include <algorithm>
#include <cstring>

namespace ctl {

namespace {

struct compact_quads { const uint4* src; uint4* dst; const uint32_t* run_dst; const uint32_t* run_src; uint32_t n_runs, shift; uint64_t n_dst_quads, n_src_quads; };

__global__ void __launch_bounds__(256) k_compact_quads(compact_quads K) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= K.n_dst_quads) return;
    const uint32_t element = (uint32_t)(i >> K.shift), q = (uint32_t)i & ((1u << K.shift) - 1u);
    const uint64_t s = ((uint64_t)mesh_set_source(K.run_dst, K.run_src, K.n_runs, element) << K.shift) | q;
    if (s >= K.n_src_quads) return;   // cannot happen: the runs lie inside the held array (plan_compaction); never read outside it
    K.dst[i] = K.src[s];
}

struct compact_rows { const uint32_t* src; uint32_t* dst; const uint32_t* tri_dst; const uint32_t* tri_src; const uint32_t* row_delta; uint32_t n_runs, n_dst, n_src; };

__global__ void __launch_bounds__(256) k_compact_tri_rows(compact_rows K) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= K.n_dst) return;
    const uint32_t j = nodes_find_added(K.tri_dst, K.n_runs, i), s = K.tri_src[j] + (i - K.tri_dst[j]);
    K.dst[i] = s < K.n_src ? mesh_set_row_word(K.src[s], K.row_delta[j]) : kNodesNone;
}

struct event_trio { hipEvent_t e[3] = { nullptr, nullptr, nullptr }; ~event_trio() { for (auto x : e) if (x) (void)hipEventDestroy(x); } };   // destroyed also when a call throws

void launch_compact(const void* src, size_t src_quads, void* dst, size_t dst_quads_allocated, const uint32_t* run_dst, const uint32_t* run_src, uint32_t n_runs, uint32_t shift, uint32_t kept_elements) {
    const uint64_t n = (uint64_t)kept_elements << shift;
    if (!n || !n_runs) return;
    if (n > dst_quads_allocated) throw std::runtime_error("ctl_scene_update_mesh_set: a compacted array is larger than its buffer");
    const compact_quads K{ static_cast<const uint4*>(src), static_cast<uint4*>(dst), run_dst, run_src, n_runs, shift, n, (uint64_t)src_quads };
    hipLaunchKernelGGL(k_compact_quads, blocks_for((size_t)n), dim3(256), 0, nullptr, K);
    CTL_HIP(hipGetLastError());
}

}  // namespace

void flat_rebuilder::update_mesh_set(Scene& A, const ctl_scene_desc& d, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes, const uint32_t* old_of_new, uint32_t n_new_nodes,
                                     const node_set_basis& basis, ctl_scene_mesh_set_stats* stats) {
    require_device();
    const char* who = "ctl_scene_update_mesh_set";
    if (!A.snap_) throw std::runtime_error(std::string(who) + ": the scene holds no description");
    const bool flat = A.flattened();
    if (flat) rebuild_refuse(A.S.flat_format, A.refit_.level_start.size() >= 2 && A.refit_part_index_.p && A.refit_part_index_.n == A.flat_n_entries_, A.S.flat_compact != 0, A.flat_n_entries_, who);
    const std::vector<uint8_t> device_owned = A.device_owned_meshes();
    node_set_plan plan; mesh_set_change change;
    plan_mesh_set(basis, A.snap_->geom, d, old_mesh_of_new, n_new_meshes, old_of_new, n_new_nodes, device_owned.empty() ? nullptr : &device_owned, plan, change, who);
    const mesh_compaction& cut = change.cut; const mesh_set_plan& grow = change.grow;
    ctl_scene_mesh_set_stats st{}; st.hash_ms = change.hash_ms;
    if (!cut.removes()) {   // nothing removed: ctl_scene_update_meshes (with nothing appended either, ctl_scene_update_nodes)
        apply_mesh_growth(A, d, old_of_new, basis, plan, grow, &st.meshes, who);
        if (stats) *stats = st;
        return;
    }
    // the arrays the scene holds must be the held description's (they are: creation sized them, and every later call kept the counts)
    if (A.tri_data_.n != (size_t)basis.n_tri_data * 2 || A.bot_nodes_.n != std::max<size_t>(4, (size_t)basis.n_bvh_nodes * 4) || A.leaf_tris_.n != std::max<size_t>(4, (size_t)basis.n_woop * 4) ||
        (A.refit_tri_row_.p && A.refit_tri_row_.n != basis.n_tri_data))
        throw std::runtime_error(std::string(who) + ": the scene's geometry arrays have other sizes than the description it holds");
    const bool table = flat && A.refit_tri_row_.p;
    const uint32_t n_runs = cut.runs();
    CTL_HIP(hipDeviceSynchronize());   // no trace reads the arrays any more; a pose or a deformation has finished (those calls are synchronous)
    // every allocation before the first launch
    mesh_growth Gr; mesh_tail_stage tails; dbuf<uint32_t> runs;
    Gr.tri_data.alloc((size_t)d.n_tri_data * 2); Gr.bot_nodes.alloc(std::max<size_t>(4, (size_t)d.n_bvh_nodes * 4)); Gr.leaf_tris.alloc(std::max<size_t>(4, (size_t)d.n_woop * 4));
    if (table) Gr.tri_row.alloc(d.n_tri_data);
    runs.alloc((size_t)std::max(1u, n_runs) * 7); tails.alloc(grow);
    event_trio ev; for (auto& x : ev.e) CTL_HIP(hipEventCreate(&x));
    {   // the run table: tri_dst, tri_src, row_dst, row_src, node_dst, node_src, row delta — n_runs words each
        std::vector<uint32_t> h((size_t)std::max(1u, n_runs) * 7, 0u);
        const std::vector<uint32_t>* parts[6] = { &cut.tri_dst, &cut.tri_src, &cut.row_dst, &cut.row_src, &cut.node_dst, &cut.node_src };
        for (int k = 0; k < 6; k++) std::copy(parts[k]->begin(), parts[k]->end(), h.begin() + (size_t)k * n_runs);
        for (uint32_t j = 0; j < n_runs; j++) h[(size_t)6 * n_runs + j] = cut.row_src[j] - cut.row_dst[j];
        CTL_HIP(hipMemcpy(runs.p, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    }
    const uint32_t* T = runs.p;
    CTL_HIP(hipEventRecord(ev.e[0], nullptr));
    // ---- compact: the kept ranges from the scene's arrays into the new ones (an array shorter than its four-quad minimum keeps the constructor's zero padding)
    if ((size_t)d.n_bvh_nodes * 4 < Gr.bot_nodes.n) CTL_HIP(hipMemsetAsync(Gr.bot_nodes.p, 0, Gr.bot_nodes.n * 16, nullptr));
    if ((size_t)d.n_woop * 4 < Gr.leaf_tris.n) CTL_HIP(hipMemsetAsync(Gr.leaf_tris.p, 0, Gr.leaf_tris.n * 16, nullptr));
    launch_compact(A.tri_data_.p, A.tri_data_.n, Gr.tri_data.p, Gr.tri_data.n, T, T + n_runs, n_runs, 1u, cut.kept_tris);
    launch_compact(A.leaf_tris_.p, A.leaf_tris_.n, Gr.leaf_tris.p, Gr.leaf_tris.n, T + 2 * (size_t)n_runs, T + 3 * (size_t)n_runs, n_runs, 2u, cut.kept_rows);
    launch_compact(A.bot_nodes_.p, A.bot_nodes_.n, Gr.bot_nodes.p, Gr.bot_nodes.n, T + 4 * (size_t)n_runs, T + 5 * (size_t)n_runs, n_runs, 2u, cut.kept_nodes);
    if (table && cut.kept_tris && n_runs) {
        const compact_rows K{ A.refit_tri_row_.p, Gr.tri_row.p, T, T + n_runs, T + 6 * (size_t)n_runs, n_runs, cut.kept_tris, (uint32_t)A.refit_tri_row_.n };
        hipLaunchKernelGGL(k_compact_tri_rows, blocks_for(cut.kept_tris), dim3(256), 0, nullptr, K);
        CTL_HIP(hipGetLastError());
    }
    CTL_HIP(hipEventRecord(ev.e[1], nullptr));
    // ---- append: the tails of the description behind the compacted ends, as ctl_scene_update_meshes lays them out
    tails.run(Gr, d, grow);
    if (flat && !table) {   // no table yet: made as ctl_scene_update_nodes makes it, on the host from the whole new description
        std::vector<uint32_t> rows; triangle_woop_rows(d, rows);
        Gr.tri_row.upload(rows.data(), rows.size()); CTL_HIP(hipStreamSynchronize(nullptr));
    }
    CTL_HIP(hipEventRecord(ev.e[2], nullptr));
    // ---- the node-set stages over the new buffers; they are swapped in where the new tree is committed, the old ones freed with Gr
    const node_set_view V{ Gr.leaf_tris.p, Gr.leaf_tris.n, Gr.tri_data.p, Gr.tri_row.p, Gr.tri_row.n };
    apply_node_set(A, d, old_of_new, basis, plan, V, &Gr, &st.meshes.nodes, who);   // (synchronises)
    CTL_HIP(hipEventElapsedTime(&st.compact_ms, ev.e[0], ev.e[1])); CTL_HIP(hipEventElapsedTime(&st.meshes.append_ms, ev.e[1], ev.e[2]));
    st.meshes_removed = cut.removed_meshes; st.triangles_removed = cut.removed_tris; st.rows_removed = cut.removed_rows; st.bvh_nodes_removed = cut.removed_nodes; st.runs = n_runs;
    const uint64_t per_tri = 32u + (table ? 4u : 0u);
    st.bytes_moved = (uint64_t)cut.kept_tris * per_tri + ((uint64_t)cut.kept_rows + cut.kept_nodes) * 64u;
    st.bytes_freed = (uint64_t)cut.removed_tris * per_tri + ((uint64_t)cut.removed_rows + cut.removed_nodes) * 64u;
    st.meshes.hash_ms = change.hash_ms; st.meshes.meshes_added = grow.meshes_added; st.meshes.triangles_added = grow.triangles_added; st.meshes.rows_added = grow.rows_added; st.meshes.bvh_nodes_added = grow.bvh_nodes_added;
    if (stats) *stats = st;
}

}  // namespace ctl
