// flat_meshes.hip — new meshes for a live scene on the device (ctl_scene_update_meshes): the growth of the two-level geometry arrays in front of the node-set stages of
// flat_nodes.hip.  The functions of flat_meshes.h, which the host re-statement (flat_meshes.cpp append_leaf_rows_host) runs too.
//
//   grow               tri_data, the mesh BVH nodes, the leaf stream and the triangle -> row table at the new sizes, in buffers of their own; the old contents device to
//                      device (the host does not have deformed or posed values), the table's appended range 0xffffffff, the appended tri_data and BVH nodes uploaded as the
//                      constructor lays them out (tracer.hip)
//   k_append_leaf_rows one lane per appended row w in [old n_woop, new n_woop) over the staged raw ctl_woop_tri rows and woop_index words: the row's mesh by a binary search
//                      over the appended meshes' first rows, the 64-B row { a, b, c, { index word, 0, 0, 0 } } as four 16-B stores, and the table by
//                      atomicMin(&tri_row[mesh.tri_offset + (index >> 1)], w): the first reference in stream order stays, whatever order the lanes arrive in (a plain vector
//                      atomic on global memory; meshes_table_rule is the same minimum)
//   apply_node_set     (flat_nodes.hip) the node-set stages over the grown buffers; they become the scene's where the new tree is committed
// The null stream between two synchronisations, like the node-set stages.  Every index is checked against the size of the array it goes into.  A refusal or a failed
// allocation frees the grown buffers: the scene as it was.
#include "flat_device.h"
#include "flat_meshes.h"
#include "mitsuba_loader.h"   // unsupported_error
#include <algorithm>
#include <cstring>

namespace ctl {

namespace {

struct append_rows {
    const float4* raw; const uint32_t* index_words;   // staged: 3 float4 and one word per appended row, row0 first
    uint32_t row0, n_rows;                            // the appended rows are [row0, n_rows)
    const uint32_t* first; const uint32_t* index_offset; const uint32_t* tri_offset; uint32_t n_meshes;   // the appended meshes by first row (mesh_set_plan)
    float4* leaf_tris; uint32_t leaf_rows;            // the grown leaf stream and the rows it holds
    uint32_t* tri_row; uint32_t n_tris;               // the grown table (null: the scene has none)
};

__global__ void __launch_bounds__(256) k_append_leaf_rows(append_rows A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n_rows - A.row0) return;
    const uint32_t w = A.row0 + i;
    if (w >= A.leaf_rows) return;   // cannot happen: the stream was allocated for n_rows rows; never write outside the arrays
    const uint32_t j = nodes_find_added(A.first, A.n_meshes, w);   // first[0] == row0 <= w (plan_mesh_growth)
    const uint32_t at = meshes_index_slot(A.index_offset[j], A.first[j], w, A.row0, A.n_rows);
    const uint32_t index_word = at != kNodesNone ? A.index_words[at - A.row0] : kMeshesFillerIndex;
    const float4 a = A.raw[(size_t)i * 3], b = A.raw[(size_t)i * 3 + 1], c = A.raw[(size_t)i * 3 + 2];
    const float raw[12] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w };
    uint32_t words[16]; meshes_row_words(raw, index_word, words);
    float4* __restrict__ R = A.leaf_tris + (size_t)w * 4;
    for (int q = 0; q < 4; q++) R[q] = make_float4(__uint_as_float(words[4 * q]), __uint_as_float(words[4 * q + 1]), __uint_as_float(words[4 * q + 2]), __uint_as_float(words[4 * q + 3]));
    if (!A.tri_row || at == kNodesNone) return;
    const uint32_t tri = meshes_row_triangle(A.tri_offset[j], index_word, A.n_tris);
    if (tri != kNodesNone) atomicMin(&A.tri_row[tri], w);
}

struct event_pair { hipEvent_t a = nullptr, b = nullptr; ~event_pair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } };   // destroyed also when a call throws

// a buffer of `total` elements with the old buffer's contents in front.  total >= src.n (the counts only grow), and the tail behind the old VALID elements is written
// by the caller: the constructor's zero padding (an array of fewer than four float4) is either copied whole or overwritten from its start
template <typename T> void grow_copy(dbuf<T>& dst, size_t total, const dbuf<T>& src) {
    dst.alloc(total);
    if (src.n && total) CTL_HIP(hipMemcpyAsync(dst.p, src.p, std::min(src.n, total) * sizeof(T), hipMemcpyDeviceToDevice, nullptr));
}

}  // namespace

size_t flat_rebuilder::read_tri_rows(Scene& A, uint32_t* rows_out, size_t capacity) {
    require_device();
    const size_t n = A.refit_tri_row_.p ? A.refit_tri_row_.n : 0;
    CTL_HIP(hipDeviceSynchronize());
    if (rows_out && n && capacity >= n) CTL_HIP(hipMemcpy(rows_out, A.refit_tri_row_.p, n * 4, hipMemcpyDeviceToHost));
    return n;
}

// the appended tails of `d` into grown buffers whose front part already stands (device to device copies or compaction, both on the null stream): tri_data and the mesh BVH
// nodes uploaded, the appended range of the table "no row", then k_append_leaf_rows.  alloc() first: every allocation before the first copy
void mesh_tail_stage::alloc(const mesh_set_plan& grow) {
    const uint32_t n_appended = (uint32_t)grow.first.size();
    raw.alloc((size_t)grow.rows_added * 3); words.alloc(grow.rows_added);
    first.alloc(std::max(1u, n_appended)); index_offset.alloc(std::max(1u, n_appended)); tri_offset.alloc(std::max(1u, n_appended));
}
void mesh_tail_stage::run(mesh_growth& Gr, const ctl_scene_desc& d, const mesh_set_plan& grow) {
    static_assert(sizeof(ctl_woop_tri) == 48 && sizeof(ctl_woop_index) == 4 && sizeof(ctl_bvh_node) == 64 && sizeof(ctl_triangle_data) == 32, "the staged layouts");
    const uint32_t n_appended = (uint32_t)grow.first.size();
    if ((size_t)d.n_tri_data * 2 > Gr.tri_data.n || (size_t)d.n_bvh_nodes * 4 > Gr.bot_nodes.n || (size_t)d.n_woop * 4 > Gr.leaf_tris.n || (Gr.tri_row.p && Gr.tri_row.n < d.n_tri_data))
        throw std::runtime_error("the grown geometry arrays are smaller than the new description");
    if (grow.triangles_added) CTL_HIP(hipMemcpy(Gr.tri_data.p + (size_t)grow.old_tri_data * 2, d.tri_data + grow.old_tri_data, (size_t)grow.triangles_added * sizeof(ctl_triangle_data), hipMemcpyHostToDevice));
    if (grow.bvh_nodes_added) CTL_HIP(hipMemcpy(Gr.bot_nodes.p + (size_t)grow.old_bvh_nodes * 4, d.bvh_nodes + grow.old_bvh_nodes, (size_t)grow.bvh_nodes_added * sizeof(ctl_bvh_node), hipMemcpyHostToDevice));
    if (Gr.tri_row.p && grow.triangles_added) CTL_HIP(hipMemsetAsync(Gr.tri_row.p + grow.old_tri_data, 0xff, (size_t)grow.triangles_added * 4, nullptr));
    if (grow.rows_added) {
        CTL_HIP(hipMemcpy(raw.p, d.woop + grow.old_woop, (size_t)grow.rows_added * sizeof(ctl_woop_tri), hipMemcpyHostToDevice));
        CTL_HIP(hipMemcpy(words.p, d.woop_index + grow.old_woop, (size_t)grow.rows_added * sizeof(ctl_woop_index), hipMemcpyHostToDevice));
        CTL_HIP(hipMemcpy(first.p, grow.first.data(), (size_t)n_appended * 4, hipMemcpyHostToDevice)); CTL_HIP(hipMemcpy(index_offset.p, grow.index_offset.data(), (size_t)n_appended * 4, hipMemcpyHostToDevice));
        CTL_HIP(hipMemcpy(tri_offset.p, grow.tri_offset.data(), (size_t)n_appended * 4, hipMemcpyHostToDevice));
        const append_rows K{ raw.p, words.p, grow.old_woop, d.n_woop, first.p, index_offset.p, tri_offset.p, n_appended, Gr.leaf_tris.p, (uint32_t)(Gr.leaf_tris.n / 4), Gr.tri_row.p, d.n_tri_data };
        hipLaunchKernelGGL(k_append_leaf_rows, blocks_for(grow.rows_added), dim3(256), 0, nullptr, K);
        CTL_HIP(hipGetLastError());
    }
}

void flat_rebuilder::update_meshes(Scene& A, const ctl_scene_desc& d, const uint32_t* old_of_new, uint32_t n_new_nodes, const node_set_basis& basis, ctl_scene_meshes_stats* stats) {
    require_device();
    const char* who = "ctl_scene_update_meshes";
    if (!A.snap_) throw std::runtime_error(std::string(who) + ": the scene holds no description");
    const bool flat = A.flattened();
    if (flat) rebuild_refuse(A.S.flat_format, A.refit_.level_start.size() >= 2 && A.refit_part_index_.p && A.refit_part_index_.n == A.flat_n_entries_, A.S.flat_compact != 0, A.flat_n_entries_, who);
    const std::vector<uint8_t> device_owned = A.device_owned_meshes();
    node_set_plan plan; mesh_set_plan grow;
    plan_node_set(basis, A.snap_->geom, d, old_of_new, n_new_nodes, device_owned.empty() ? nullptr : &device_owned, plan, who, &grow);
    apply_mesh_growth(A, d, old_of_new, basis, plan, grow, stats, who);
}

// behind the checks (ctl_scene_update_mesh_set comes here too when its map removes nothing: flat_mesh_set.hip)
void flat_rebuilder::apply_mesh_growth(Scene& A, const ctl_scene_desc& d, const uint32_t* old_of_new, const node_set_basis& basis, const node_set_plan& plan, const mesh_set_plan& grow,
                                       ctl_scene_meshes_stats* stats, const char* who) {
    const bool flat = A.flattened();
    ctl_scene_meshes_stats st{}; st.hash_ms = grow.hash_ms;
    if (!grow.grown()) {   // nothing appended: ctl_scene_update_nodes
        const node_set_view V{ A.leaf_tris_.p, A.leaf_tris_.n, A.tri_data_.p, A.refit_tri_row_.p, A.refit_tri_row_.n };
        apply_node_set(A, d, old_of_new, basis, plan, V, nullptr, &st.nodes, who);
        if (stats) *stats = st;
        return;
    }
    // the arrays the scene holds must be the held description's (they are: creation sized them, and every later call kept the counts)
    const size_t old_tri = (size_t)grow.old_tri_data * 2, old_bot = std::max<size_t>(4, (size_t)grow.old_bvh_nodes * 4), old_leaf = std::max<size_t>(4, (size_t)grow.old_woop * 4);
    if (A.tri_data_.n != old_tri || A.bot_nodes_.n != old_bot || A.leaf_tris_.n != old_leaf || (A.refit_tri_row_.p && A.refit_tri_row_.n != grow.old_tri_data))
        throw std::runtime_error(std::string(who) + ": the scene's geometry arrays have other sizes than the description it holds");
    CTL_HIP(hipDeviceSynchronize());   // no trace reads the arrays any more; a pose or a deformation has finished (those calls are synchronous)
    // every allocation before the first copy
    mesh_growth Gr; mesh_tail_stage tails; tails.alloc(grow);
    event_pair ev; CTL_HIP(hipEventCreate(&ev.a)); CTL_HIP(hipEventCreate(&ev.b));
    CTL_HIP(hipEventRecord(ev.a, nullptr));
    // ---- grow: old contents device to device, the tails from the description
    grow_copy(Gr.tri_data, (size_t)d.n_tri_data * 2, A.tri_data_);
    grow_copy(Gr.bot_nodes, std::max<size_t>(4, (size_t)d.n_bvh_nodes * 4), A.bot_nodes_);
    grow_copy(Gr.leaf_tris, std::max<size_t>(4, (size_t)d.n_woop * 4), A.leaf_tris_);
    if (flat && A.refit_tri_row_.p) {   // the device extension of the table
        Gr.tri_row.alloc(d.n_tri_data);
        if (grow.old_tri_data) CTL_HIP(hipMemcpyAsync(Gr.tri_row.p, A.refit_tri_row_.p, (size_t)grow.old_tri_data * 4, hipMemcpyDeviceToDevice, nullptr));
    }
    tails.run(Gr, d, grow);
    if (flat && !Gr.tri_row.p) {   // no table yet: made as ctl_scene_update_nodes makes it, on the host from the whole new description (the same table: tests/test_mesh_set_host.py)
        std::vector<uint32_t> rows; triangle_woop_rows(d, rows);
        Gr.tri_row.upload(rows.data(), rows.size()); CTL_HIP(hipStreamSynchronize(nullptr));
    }
    CTL_HIP(hipEventRecord(ev.b, nullptr));
    // ---- the node-set stages over the grown buffers; they are swapped in where the new tree is committed
    const node_set_view V{ Gr.leaf_tris.p, Gr.leaf_tris.n, Gr.tri_data.p, Gr.tri_row.p, Gr.tri_row.n };
    apply_node_set(A, d, old_of_new, basis, plan, V, &Gr, &st.nodes, who);   // (synchronises)
    CTL_HIP(hipEventElapsedTime(&st.append_ms, ev.a, ev.b));
    st.meshes_added = grow.meshes_added; st.triangles_added = grow.triangles_added; st.rows_added = grow.rows_added; st.bvh_nodes_added = grow.bvh_nodes_added;
    if (stats) *stats = st;
}

}  // namespace ctl
