// flat_nodes.hip — another set of nodes for a live scene on the device (ctl_scene_update_nodes): the kernels around the functions of flat_nodes.h, which the host
// yardstick (flat_nodes.cpp update_nodes_flat_scene) runs too — same functions, same order, so the device tree equals the host's byte for byte
// (tests/test_gpu_node_set.py) — and the host work of the call.
//
//   k_nodes_flag       one lane per entry: the node word through new_of_old[] -> 1 (kept) or 0 (dropped)
//   rocPRIM            exclusive_scan over the flags: the kept entries' positions; its last element is their number
//   k_nodes_candidates one lane per triangle of the added nodes (node order, then mesh order): 1 when a row of the two-level leaf stream stands for the triangle and its Woop
//                      matrix is regular (the rows as they stand in HBM: deformed and posed values are what the new instance gets), else 0
//   rocPRIM            exclusive_scan over those flags: the generated entries' positions behind the kept ones
//   k_nodes_move       eight lanes per entry, each one 16-B load and one 16-B store (a wave moves eight whole 128-B lines): a kept entry to its position, the node word
//                      renumbered with its stamp bit kept; its part_index word with it
//   k_nodes_generate   one lane per regular candidate: the three rows from the leaf stream, the entry in flat_leaf's layout (nodes_entry_words) as eight 16-B stores
//   flat_rebuilder     (flat_rebuild.hip) the re-stamp of the model / alpha bits and the entry boxes (k_refit_entries), then the rebuild, over the new set in buffers of its own
// Everything runs on the null stream between two synchronisations, like the refit.  Plain launches, plain stores; no atomic decides a position; every index is checked
// against the size of the array it goes into.  The scene's own buffers are written only after the new tree stands: a refusal or a failed allocation leaves the scene as it was.
#include "flat_device.h"
#include "flat_mesh_set.h"
#include "scene_checks.h"
#include "mitsuba_loader.h"   // unsupported_error
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <cstring>

namespace ctl {

namespace {

__global__ void __launch_bounds__(256) k_nodes_flag(const float4* __restrict__ leaves, uint32_t n_entries, const uint32_t* __restrict__ new_of_old, uint32_t n_old_nodes, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n_entries) return;
    if (i == n_entries) { flags[i] = 0u; return; }   // one more element: the exclusive scan leaves the total there
    const uint32_t node_word = __float_as_uint(leaves[(size_t)i * 8 + 3].y);
    flags[i] = nodes_new_of(node_word, new_of_old, n_old_nodes) != kNodesNone ? 1u : 0u;
}

struct nodes_added { const uint32_t* base; const uint32_t* tri0; const uint32_t* node; uint32_t n_added, n_candidates; const uint32_t* tri_row; uint32_t n_tris; const float4* leaf_tris; uint32_t n_rows; };

__global__ void __launch_bounds__(256) k_nodes_candidates(nodes_added D, uint32_t* __restrict__ flags) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g > D.n_candidates) return;
    if (g == D.n_candidates) { flags[g] = 0u; return; }
    const uint32_t j = nodes_find_added(D.base, D.n_added, g), tri = D.tri0[j] + (g - D.base[j]);
    uint32_t regular = 0u;
    if (tri < D.n_tris) {
        const uint32_t row = D.tri_row[tri];
        if (row < D.n_rows) {
            const float4 a = D.leaf_tris[(size_t)row * 4], b = D.leaf_tris[(size_t)row * 4 + 1], c = D.leaf_tris[(size_t)row * 4 + 2];
            const float wa[4] = { a.x, a.y, a.z, a.w }, wb[4] = { b.x, b.y, b.z, b.w }, wc[4] = { c.x, c.y, c.z, c.w };
            regular = nodes_rows_regular(wa, wb, wc) ? 1u : 0u;
        }
    }
    flags[g] = regular;
}

// tri_delta: null, or per old node the triangles removed in front of its mesh (flat_mesh_set.h): the entry's triangle word is lowered while it moves
struct nodes_move { const float4* old_leaves; const uint32_t* old_part; const uint32_t* flags; const uint32_t* pos; const uint32_t* new_of_old; uint32_t n_old_nodes, n_old, n_new; float4* new_leaves; uint32_t* new_part; const uint32_t* tri_delta; };

__global__ void __launch_bounds__(256) k_nodes_move(nodes_move M) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, i = t >> 3, q = t & 7u;
    if (i >= M.n_old || !M.flags[i]) return;
    const uint32_t p = M.pos[i];
    if (p >= M.n_new) return;   // cannot happen: the positions are the scan of the flags and n_new is at least their sum; never write outside the arrays
    float4 v = M.old_leaves[(size_t)i * 8 + q];
    if (q == 3u) {
        const uint32_t w = __float_as_uint(v.y); v.y = __uint_as_float(nodes_renumber(w, nodes_new_of(w, M.new_of_old, M.n_old_nodes)));
        if (M.tri_delta && (w & ~kNodesStampBit) < M.n_old_nodes) v.x = __uint_as_float(mesh_set_entry_index(__float_as_uint(v.x), M.tri_delta[w & ~kNodesStampBit]));   // (a kept entry's node is always one of the old ones)
    }
    M.new_leaves[(size_t)p * 8 + q] = v;
    if (q == 0u) M.new_part[p] = M.old_part[i];
}

__global__ void __launch_bounds__(256) k_nodes_generate(nodes_added D, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ pos, const float4* __restrict__ inst, uint32_t n_scene_nodes,
                                                        uint32_t first, uint32_t n_new, float4* __restrict__ new_leaves, uint32_t* __restrict__ new_part) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= D.n_candidates || !flags[g]) return;
    const uint32_t j = nodes_find_added(D.base, D.n_added, g), tri = D.tri0[j] + (g - D.base[j]), node = D.node[j], p = first + pos[g];
    if (p >= n_new || node >= n_scene_nodes || tri >= D.n_tris) return;   // cannot happen (see k_nodes_move)
    const uint32_t row = D.tri_row[tri];
    if (row >= D.n_rows) return;
    const float4 a = D.leaf_tris[(size_t)row * 4], b = D.leaf_tris[(size_t)row * 4 + 1], c = D.leaf_tris[(size_t)row * 4 + 2];
    const float4 i0 = inst[(size_t)node * 4], i1 = inst[(size_t)node * 4 + 1], i2 = inst[(size_t)node * 4 + 2], i3 = inst[(size_t)node * 4 + 3];
    const float wa[4] = { a.x, a.y, a.z, a.w }, wb[4] = { b.x, b.y, b.z, b.w }, wc[4] = { c.x, c.y, c.z, c.w };
    const float inv[12] = { i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w, i2.x, i2.y, i2.z, i2.w };
    uint32_t w[32]; nodes_entry_words(wa, wb, wc, tri, node, inv, i3.x, w);
    float4* __restrict__ E = new_leaves + (size_t)p * 8;
    for (int q = 0; q < 8; q++) E[q] = make_float4(__uint_as_float(w[4 * q]), __uint_as_float(w[4 * q + 1]), __uint_as_float(w[4 * q + 2]), __uint_as_float(w[4 * q + 3]));
    new_part[p] = kRefitNoPart;
}

struct event_set {
    hipEvent_t e[3] = { nullptr, nullptr, nullptr };
    event_set() { for (auto& x : e) CTL_HIP(hipEventCreate(&x)); }
    ~event_set() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

void exclusive_scan_u32(dbuf<unsigned char>& temp, uint32_t* in, uint32_t* out, size_t count, const char* who) {
    size_t need = 0;
    CTL_HIP(rocprim::exclusive_scan(nullptr, need, in, out, 0u, count, rocprim::plus<uint32_t>(), (hipStream_t) nullptr));
    if (need > temp.n) throw std::runtime_error(std::string(who) + ": scan storage");
    size_t bytes = temp.n;
    CTL_HIP(rocprim::exclusive_scan(temp.p, bytes, in, out, 0u, count, rocprim::plus<uint32_t>(), (hipStream_t) nullptr));
}

}  // namespace

void Scene::update_nodes(const ctl_scene_desc& d, const uint32_t* old_of_new, uint32_t n_new_nodes, const node_set_basis& basis, ctl_scene_nodes_stats* stats) {
    require_device();
    const char* who = "ctl_scene_update_nodes";
    if (!snap_) throw std::runtime_error(std::string(who) + ": the scene holds no description");
    const bool flat = flattened();
    if (flat) rebuild_refuse(S.flat_format, refit_.level_start.size() >= 2 && refit_part_index_.p && refit_part_index_.n == flat_n_entries_, S.flat_compact != 0, flat_n_entries_, who);
    const std::vector<uint8_t> device_owned = device_owned_meshes();
    node_set_plan plan;
    plan_node_set(basis, snap_->geom, d, old_of_new, n_new_nodes, device_owned.empty() ? nullptr : &device_owned, plan, who);
    const node_set_view V{ leaf_tris_.p, leaf_tris_.n, tri_data_.p, refit_tri_row_.p, refit_tri_row_.n };
    flat_rebuilder::apply_node_set(*this, d, old_of_new, basis, plan, V, nullptr, stats, who);
}

// the stages behind the checks.  V: the two-level arrays the stages read — the scene's own, or grown ones (`grown`, flat_meshes.hip) that become the scene's where the new tree
// is committed; V.tri_row null on a flattened scene: the scene has no triangle -> row table yet and gets one from `d` here
void flat_rebuilder::apply_node_set(Scene& A, const ctl_scene_desc& d, const uint32_t* old_of_new, const node_set_basis& basis, const node_set_plan& plan, const node_set_view& V, mesh_growth* grown,
                           ctl_scene_nodes_stats* stats, const char* who) {
    const bool flat = A.flattened();
    const uint32_t n_old_nodes = A.snap_->d.n_nodes;
    if (basis.nodes.size() != n_old_nodes || (flat && A.refit_.xf0.size() != n_old_nodes)) throw std::runtime_error(std::string(who) + ": the scene's description has another number of nodes than its tree");
    ctl_scene_nodes_stats st{}; st.entries_before = st.entries_after = flat ? (uint32_t)A.flat_n_entries_ : 0u;
    if (plan.identity) {   // nothing of the node set changes: ctl_scene_update, no rebuild
        A.update(d, nullptr);
        if (stats) *stats = st;
        return;
    }
    // host work before the device is touched: the instance records, the creation poses, the carry matrices
    const shading_state shade = derive_shading_state(d);
    std::vector<float4> inst, fwd; std::vector<uint4> ninfo;
    Scene::pack_instances(d, inst, fwd, ninfo);
    std::vector<ctl_float4x4> xf0(d.n_nodes); std::vector<double> P;
    if (flat) {
        for (uint32_t k = 0; k < d.n_nodes; k++) xf0[k] = old_of_new[k] == kNodesNone ? d.node_transforms[k] : A.refit_.xf0[old_of_new[k]];
        P = Scene::carry_matrices(d, xf0, who);
    }
    CTL_HIP(hipDeviceSynchronize());   // no trace reads the arrays any more
    dbuf<float4> inst_new, fwd_new; dbuf<uint4> ninfo_new;
    inst_new.alloc(inst.size()); fwd_new.alloc(fwd.size()); ninfo_new.alloc(ninfo.size());
    CTL_HIP(hipMemcpy(inst_new.p, inst.data(), inst.size() * sizeof(float4), hipMemcpyHostToDevice)); CTL_HIP(hipMemcpy(fwd_new.p, fwd.data(), fwd.size() * sizeof(float4), hipMemcpyHostToDevice));
    CTL_HIP(hipMemcpy(ninfo_new.p, ninfo.data(), ninfo.size() * sizeof(uint4), hipMemcpyHostToDevice));
    std::vector<uint32_t> skipped;
    rebuild_last_rounds() = 0u;
    flat_rebuilder B; B.builder = rebuild_builder_choice();   // what the C entry point asked for (rebuild_builder_scope, flat_rebuild.h)
    if (flat) {
        const uint32_t n_old = (uint32_t)A.flat_n_entries_, n_added = (uint32_t)plan.added.size(), G = plan.added_base.back();
        // ---- scratch of this call; the scene's tri_row table and rocPRIM storage are caches without a meaning of their own
        dbuf<uint32_t> map_dev, flags, pos, base_dev, tri0_dev, added_dev, gflags, gpos, part_mid, delta_dev; dbuf<float4> leaves_mid; dbuf<ctl_material> mats_tmp; dbuf<unsigned char> temp;
        map_dev.alloc(n_old_nodes); flags.alloc((size_t)n_old + 1); pos.alloc((size_t)n_old + 1); gflags.alloc((size_t)G + 1); gpos.alloc((size_t)G + 1);
        base_dev.alloc(plan.added_base.size()); tri0_dev.alloc(std::max<size_t>(1, n_added)); added_dev.alloc(std::max<size_t>(1, n_added));
        CTL_HIP(hipMemcpy(map_dev.p, plan.new_of_old.data(), (size_t)n_old_nodes * 4, hipMemcpyHostToDevice));
        if (plan.node_tri_delta.size() == n_old_nodes) { delta_dev.alloc(n_old_nodes); CTL_HIP(hipMemcpy(delta_dev.p, plan.node_tri_delta.data(), (size_t)n_old_nodes * 4, hipMemcpyHostToDevice)); }
        CTL_HIP(hipMemcpy(base_dev.p, plan.added_base.data(), plan.added_base.size() * 4, hipMemcpyHostToDevice));
        if (n_added) { CTL_HIP(hipMemcpy(tri0_dev.p, plan.added_tri0.data(), (size_t)n_added * 4, hipMemcpyHostToDevice)); CTL_HIP(hipMemcpy(added_dev.p, plan.added.data(), (size_t)n_added * 4, hipMemcpyHostToDevice)); }
        const uint32_t* tri_row = V.tri_row; size_t n_tri_row = V.n_tri_row;
        if (!tri_row) {   // triangle -> row of the leaf stream; woop_index is structure (the hashes matched): the table holds for every later update
            std::vector<uint32_t> rows; triangle_woop_rows(d, rows);
            A.refit_tri_row_.upload(rows.data(), rows.size()); CTL_HIP(hipStreamSynchronize(nullptr));
            tri_row = A.refit_tri_row_.p; n_tri_row = A.refit_tri_row_.n;
        }
        size_t scan_bytes = 0;
        CTL_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, flags.p, pos.p, 0u, (size_t)std::max(n_old, G) + 1, rocprim::plus<uint32_t>(), (hipStream_t) nullptr));
        if (A.rebuild_temp_.n < std::max<size_t>(scan_bytes, 16)) { temp.alloc(std::max<size_t>(scan_bytes, 16)); swap_buffers(A.rebuild_temp_, temp); temp.free(); }
        event_set ev;
        CTL_HIP(hipEventRecord(ev.e[0], nullptr));
        // 1. which entries stay, 2. which triangles of the added nodes get an entry; the two scans
        hipLaunchKernelGGL(k_nodes_flag, blocks_for((size_t)n_old + 1), dim3(256), 0, nullptr, A.flat_leaves_.p, n_old, map_dev.p, n_old_nodes, flags.p);
        const nodes_added D{ base_dev.p, tri0_dev.p, added_dev.p, n_added, G, tri_row, (uint32_t)n_tri_row, V.leaf_tris, (uint32_t)(V.n_leaf_tris / 4) };
        hipLaunchKernelGGL(k_nodes_candidates, blocks_for((size_t)G + 1), dim3(256), 0, nullptr, D, gflags.p);
        CTL_HIP(hipGetLastError());
        exclusive_scan_u32(A.rebuild_temp_, flags.p, pos.p, (size_t)n_old + 1, who);
        exclusive_scan_u32(A.rebuild_temp_, gflags.p, gpos.p, (size_t)G + 1, who);
        uint32_t n_kept = 0, n_gen = 0;
        CTL_HIP(hipMemcpy(&n_kept, pos.p + n_old, 4, hipMemcpyDeviceToHost)); CTL_HIP(hipMemcpy(&n_gen, gpos.p + G, 4, hipMemcpyDeviceToHost));
        if (n_kept > n_old || n_gen > G) throw std::runtime_error(std::string(who) + ": the positions handed out exceed the entry count");
        const uint64_t n_new64 = (uint64_t)n_kept + n_gen;
        rebuild_refuse(A.S.flat_format, true, true, (size_t)n_new64, who);
        const uint32_t n_new = (uint32_t)n_new64;
        if (n_gen < G) {   // the triangles without an entry join the scene's list (flat_missing_triangles)
            std::vector<uint32_t> f(G);
            CTL_HIP(hipMemcpy(f.data(), gflags.p, (size_t)G * 4, hipMemcpyDeviceToHost));
            for (uint32_t j = 0; j < n_added; j++) for (uint32_t g = plan.added_base[j]; g < plan.added_base[j + 1]; g++) if (!f[g]) skipped.push_back(plan.added_tri0[j] + (g - plan.added_base[j]));
        }
        // every allocation before the first entry is written
        leaves_mid.alloc(((size_t)n_new + 1) * 8); part_mid.alloc(n_new); mats_tmp.alloc(std::max<uint32_t>(1u, d.n_materials));
        B.who = who; B.n = n_new; B.src_leaves = leaves_mid.p; B.src_part = part_mid.p;
        B.allocate(A, P);
        if (d.n_materials) CTL_HIP(hipMemcpy(mats_tmp.p, d.materials, (size_t)d.n_materials * sizeof(ctl_material), hipMemcpyHostToDevice));
        const nodes_move M{ A.flat_leaves_.p, A.refit_part_index_.p, flags.p, pos.p, map_dev.p, n_old_nodes, n_old, n_new, leaves_mid.p, part_mid.p, delta_dev.p };
        hipLaunchKernelGGL(k_nodes_move, blocks_for((size_t)n_old * 8), dim3(256), 0, nullptr, M);
        if (G) hipLaunchKernelGGL(k_nodes_generate, blocks_for(G), dim3(256), 0, nullptr, D, gflags.p, gpos.p, inst_new.p, d.n_nodes, n_kept, n_new, leaves_mid.p, part_mid.p);
        CTL_HIP(hipGetLastError());
        CTL_HIP(hipMemcpyAsync(leaves_mid.p + (size_t)n_new * 8, A.flat_leaves_.p + (size_t)n_old * 8, 128, hipMemcpyDeviceToDevice, nullptr));   // the closing entry
        CTL_HIP(hipEventRecord(ev.e[1], nullptr));
        // the re-stamp, the entry boxes and 4. the rebuild, with the NEW instance records and materials (the scene still holds the old ones)
        B.R.inst = inst_new.p; B.R.inst_fwd = fwd_new.p; B.R.restamp = (int)d.n_materials; B.R.leaf_keys = A.S.flat_leaf_keys; B.R.alpha_maps = (int)shade.alpha_maps;
        B.R.tri_data = V.tri_data; B.R.node_info = ninfo_new.p; B.R.mats = mats_tmp.p;
        B.run(A);   // (synchronises) a tree too deep is refused here: the scene as it was
        CTL_HIP(hipEventRecord(ev.e[2], nullptr)); CTL_HIP(hipEventSynchronize(ev.e[2]));
        CTL_HIP(hipEventElapsedTime(&st.edit_ms, ev.e[0], ev.e[1])); CTL_HIP(hipEventElapsedTime(&st.total_ms, ev.e[0], ev.e[2]));
        st.entries_after = n_new; st.entries_dropped = n_old - n_kept; st.entries_generated = n_gen; st.degenerate_skipped = G - n_gen; st.rebuilt = 1u;
        B.report(st.rebuild);
        // ---- from here on the scene is written
        B.commit(A);
        A.refit_.xf0 = xf0;
        if (plan.cut) mesh_set_rebase_triangles(A.flat_missing_tris_, *plan.cut);   // removed meshes: the held list in the new numbering, before the new triangles join it
        if (!skipped.empty()) {
            A.flat_missing_tris_.insert(A.flat_missing_tris_.end(), skipped.begin(), skipped.end());
            std::sort(A.flat_missing_tris_.begin(), A.flat_missing_tris_.end()); A.flat_missing_tris_.erase(std::unique(A.flat_missing_tris_.begin(), A.flat_missing_tris_.end()), A.flat_missing_tris_.end());
        }
    }
    // appended meshes (flat_meshes.hip): the grown geometry arrays become the scene's — A.bind() below hands their addresses to the tracers, a bound skin reads them at its next pose
    if (grown) {
        swap_buffers(A.tri_data_, grown->tri_data); swap_buffers(A.bot_nodes_, grown->bot_nodes); swap_buffers(A.leaf_tris_, grown->leaf_tris);
        if (grown->tri_row.p) swap_buffers(A.refit_tri_row_, grown->tri_row);
    }
    if (plan.cut) remap_skins(A, *plan.cut, d);   // removed meshes (flat_mesh_set.hip): the bindings under their new mesh indices, before the shape sets of emissive skins run
    // the rest of the description, block by block as ctl_scene_update applies it; the instance records go in by a swap of buffers
    swap_buffers(A.inst_, inst_new); swap_buffers(A.inst_fwd_, fwd_new); swap_buffers(A.node_info_, ninfo_new);
    A.set_shading_state(shade);
    A.upload_materials(d); A.upload_lights(d); A.upload_top_level(d);
    A.lights_stale_ = false; A.run_shape_sets(d);   // the lights of emissive skins: node indices by the new description, the pose stays (shape_set.hip)
    if (flat) A.S.inst_w_one = inverse_transforms_have_w_one(d);
    CTL_HIP(hipDeviceSynchronize());
    A.bind(d); A.n_nodes = d.n_nodes; A.set_camera(d);
    A.snapshot(d, plan.geom.empty() ? nullptr : &plan.geom);
    if (stats) *stats = st;
}

}  // namespace ctl
