// flat_rebuild.hip — the rebuild of the flattened Q4 tree on the device (ctl_scene_rebuild_flat): the kernels around the functions of flat_rebuild.h, which the host
// rebuild (flat_rebuild.cpp rebuild_flat_scene) runs too — same functions, same order, so the device tree equals the host's byte for byte (tests/test_gpu_flat_rebuild.py).
//
//   k_refit_entries    (flat_refit.hip, as it is) every entry's world box for the current transforms
//   k_rebuild_bounds   min / max of the valid boxes as ordered integers: a wave reduction, then one integer atomic min / max per wave and axis — exact, whatever the order
//   k_rebuild_keys     one lane per entry: its Morton code and its index
//   rocPRIM            radix_sort_pairs over (code, index): stable, so equal codes keep index order
//   per level, from the root (the host reads the level's totals back — 8 B — and checks them against the buffers before anything is written with them):
//     k_rebuild_count  one lane per node of the level: its slots (rebuild_node_slots), inner children << 32 | entries of leaf children
//     rocPRIM          inclusive_scan over the level
//     k_rebuild_emit   one lane per node: the slots again, the node's 64 B, the ranges of its inner children at their node numbers, the permutation words of its leaf
//                      children's entries at their positions
//   k_rebuild_gather   eight lanes per entry: the 128 B of entry perm[p] to position p of the second entry buffer, bit 0 of the index word rewritten; part_index and the
//                      entry's box with it; the closing entry stays at the end
//   k_refit_level      (flat_refit.hip, as it is) deepest level first, on the new arrays
// Plain launches on the null stream; no kernel waits for another workgroup; no atomic decides a position.
// The host side is flat_rebuilder (flat_device.h: allocate / run / commit), which ctl_scene_update_nodes (flat_nodes.hip) runs too, over the entries it has assembled.
#include "flat_device.h"
#include "flat_refit.h"
#include "mitsuba_loader.h"   // unsupported_error
#include <rocprim/rocprim.hpp>
#include <algorithm>
#include <utility>

namespace ctl {

namespace {

__global__ void __launch_bounds__(256) k_rebuild_bounds(const refit_box* __restrict__ ebox, uint32_t n, uint32_t* __restrict__ bounds) {
    uint32_t lo[3] = { 0xffffffffu, 0xffffffffu, 0xffffffffu }, hi[3] = { 0u, 0u, 0u };
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const refit_box b = ebox[i];
        if (!rebuild_box_valid(b)) continue;
        for (int k = 0; k < 3; k++) { const uint32_t l = rebuild_ord(b.lo[k]), h = rebuild_ord(b.hi[k]); if (l < lo[k]) lo[k] = l; if (h > hi[k]) hi[k] = h; }
    }
    for (int k = 0; k < 3; k++) {
        for (int o = 32; o > 0; o >>= 1) { const uint32_t l = (uint32_t)__shfl_down((int)lo[k], o, 64), h = (uint32_t)__shfl_down((int)hi[k], o, 64); if (l < lo[k]) lo[k] = l; if (h > hi[k]) hi[k] = h; }
        if ((threadIdx.x & 63u) == 0u) { atomicMin(&bounds[k], lo[k]); atomicMax(&bounds[3 + k], hi[k]); }
    }
}

__global__ void __launch_bounds__(256) k_rebuild_keys(const refit_box* __restrict__ ebox, uint32_t n, const uint32_t* __restrict__ bounds, uint64_t* __restrict__ keys, uint32_t* __restrict__ index) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    refit_box B;
    for (int k = 0; k < 3; k++) { B.lo[k] = rebuild_unord(bounds[k]); B.hi[k] = rebuild_unord(bounds[3 + k]); }
    keys[i] = rebuild_key(ebox[i], B);
    index[i] = i;
}

struct rebuild_level { const uint64_t* keys; uint32_t* first; uint32_t* last; uint32_t begin, count; };

__global__ void __launch_bounds__(256) k_rebuild_count(rebuild_level L, uint64_t* __restrict__ counts) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= L.count) return;
    rebuild_slots S; rebuild_node_slots(L.keys, L.first[L.begin + j], L.last[L.begin + j], S);
    counts[j] = rebuild_slot_counts(S);
}

// child_base / entry_base: the first node of the next level / the first entry position of this level; cap_nodes / n_entries: the sizes of the arrays written (the host has
// checked the level's totals against them; never write outside the arrays)
__global__ void __launch_bounds__(256) k_rebuild_emit(rebuild_level L, const uint64_t* __restrict__ incl, const uint32_t* __restrict__ sorted_index, uint32_t child_base, uint32_t entry_base,
                                                      uint32_t cap_nodes, uint32_t n_entries, float4* __restrict__ nodes, uint32_t* __restrict__ perm) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= L.count) return;
    const uint32_t i = L.begin + j;
    rebuild_slots S; rebuild_node_slots(L.keys, L.first[i], L.last[i], S);
    const uint64_t before = incl[j] - rebuild_slot_counts(S);
    uint32_t child = child_base + (uint32_t)(before >> 32), entry = entry_base + (uint32_t)before;
    uint32_t w[16]; rebuild_encode_node(S, child, entry, w);
    float4* __restrict__ N = nodes + (size_t)i * 4;
    for (int q = 0; q < 4; q++) N[q] = make_float4(__uint_as_float(w[4 * q]), __uint_as_float(w[4 * q + 1]), __uint_as_float(w[4 * q + 2]), __uint_as_float(w[4 * q + 3]));
    for (uint32_t k = 0; k < S.n; k++) {
        if (S.leaf(k)) {
            for (uint32_t s = S.first[k]; s <= S.last[k]; s++, entry++) if (entry < n_entries) perm[entry] = sorted_index[s] | (s == S.last[k] ? kRebuildLastBit : 0u);
        } else { if (child < cap_nodes) { L.first[child] = S.first[k]; L.last[child] = S.last[k]; } child++; }
    }
}

struct rebuild_gather { const float4* old_leaves; float4* new_leaves; const uint32_t* perm; uint32_t n; const uint32_t* old_part; uint32_t* new_part; const refit_box* old_box; refit_box* new_box; };

__global__ void __launch_bounds__(256) k_rebuild_gather(rebuild_gather G) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, p = t >> 3, q = t & 7u;
    if (p > G.n) return;
    if (p == G.n) { G.new_leaves[(size_t)p * 8 + q] = G.old_leaves[(size_t)p * 8 + q]; return; }   // the closing entry
    const uint32_t word = G.perm[p], src = word & ~kRebuildLastBit;
    if (src >= G.n) return;   // cannot happen: the positions handed out sum to n and every one was written; never read outside the arrays
    float4 v = G.old_leaves[(size_t)src * 8 + q];
    if (q == 3u) v.x = __uint_as_float((__float_as_uint(v.x) & ~1u) | ((word & kRebuildLastBit) ? 1u : 0u));
    G.new_leaves[(size_t)p * 8 + q] = v;
    if (q == 0u) { G.new_part[p] = G.old_part[src]; G.new_box[p] = G.old_box[src]; }
}

__global__ void __launch_bounds__(256) k_rebuild_iota(uint32_t* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = i;
}

}  // namespace

flat_rebuilder::~flat_rebuilder() { for (auto x : ev) if (x) (void)hipEventDestroy(x); }

void flat_rebuilder::allocate(Scene& A, const std::vector<double>& P) {
    // a wide node that is not the root has more than kRebuildLeafMax entries under it, and one with an inner child has four slots: fewer than n / 3 + 1 nodes with leaves of up
    // to four entries (the per-level check in run() holds whatever the bound)
    cap = (kRebuildLeafMax >= 4u ? n / 2u : n) + 2u;
    // every allocation before the first write: a failed one leaves the scene as it was (the buffers free themselves)
    dbuf<refit_box> ebox_cur; dbuf<double> carry; dbuf<unsigned char> temp;
    if (A.refit_ebox_.n < n) ebox_cur.alloc(n);
    ebox_new.alloc(n); nbox_new.alloc(cap); bounds.alloc(6); idx_in.alloc(n); idx_out.alloc(n); first.alloc(cap); last.alloc(cap); perm.alloc(n); part_new.alloc(n);
    keys_in.alloc(n); keys_out.alloc(n); counts.alloc(cap); incl.alloc(cap); nodes_new.alloc((size_t)cap * 4); leaves_new.alloc(((size_t)n + 1) * 8); carry.alloc(P.size()); area_dev.alloc(2);
    size_t sort_bytes = 0, scan_bytes = 0;
    CTL_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys_in.p, keys_out.p, idx_in.p, idx_out.p, (size_t)n, 0u, 64u, (hipStream_t) nullptr));
    CTL_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, counts.p, incl.p, (size_t)cap, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
    const size_t temp_need = std::max<size_t>(std::max(sort_bytes, scan_bytes), 16);
    if (A.rebuild_temp_.n < temp_need) { temp.alloc(temp_need); swap_buffers(A.rebuild_temp_, temp); temp.free(); }   // (scratch of no meaning between calls: kept)
    for (auto& x : ev) CTL_HIP(hipEventCreate(&x));
    if (ebox_cur.p) swap_buffers(A.refit_ebox_, ebox_cur);
    swap_buffers(A.refit_carry_, carry);
    CTL_HIP(hipMemcpy(A.refit_carry_.p, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice));
    R.nodes = A.flat_nodes_.p; R.leaves = src_leaves; R.n_nodes = (uint32_t)A.flat_n_nodes_; R.n_entries = n; R.compact = 1;
    R.part_index = src_part; R.part_boxes = A.refit_part_boxes_.p; R.carry = A.refit_carry_.p; R.ebox = A.refit_ebox_.p; R.nbox = A.refit_nbox_.p;
}

void flat_rebuilder::run(Scene& A) {
    CTL_HIP(hipMemsetAsync(area_dev.p, 0, 16, nullptr));
    launch_refit_area(nullptr, A.flat_nodes_.p, R.n_nodes, area_dev.p);
    // 1. entry boxes
    CTL_HIP(hipEventRecord(ev[0], nullptr));
    launch_refit_entries(nullptr, R, true);
    CTL_HIP(hipEventRecord(ev[1], nullptr));
    // 2. - 4. bounds, keys, sort
    CTL_HIP(hipMemsetAsync(bounds.p, 0xff, 12, nullptr)); CTL_HIP(hipMemsetAsync(bounds.p + 3, 0, 12, nullptr));
    hipLaunchKernelGGL(k_rebuild_bounds, dim3(std::min<unsigned>(blocks_for(n).x, 1024u)), dim3(256), 0, nullptr, A.refit_ebox_.p, n, bounds.p);
    hipLaunchKernelGGL(k_rebuild_keys, blocks_for(n), dim3(256), 0, nullptr, A.refit_ebox_.p, n, bounds.p, keys_in.p, idx_in.p);
    CTL_HIP(hipGetLastError());
    size_t bytes = A.rebuild_temp_.n;
    CTL_HIP(rocprim::radix_sort_pairs(A.rebuild_temp_.p, bytes, keys_in.p, keys_out.p, idx_in.p, idx_out.p, (size_t)n, 0u, 64u, (hipStream_t) nullptr));
    CTL_HIP(hipEventRecord(ev[2], nullptr));
    // 5. - 8. the wide nodes, level by level
    const uint32_t root_range[2] = { 0u, n - 1u };
    CTL_HIP(hipMemcpy(first.p, &root_range[0], 4, hipMemcpyHostToDevice)); CTL_HIP(hipMemcpy(last.p, &root_range[1], 4, hipMemcpyHostToDevice));
    level_start.assign(1, 0u);
    uint32_t begin = 0, count = 1, entry_base = 0;
    const int depth_limit = (kStackSize - 4) / 3;   // stack_need() + 2 <= kStackSize, as at creation
    while (count) {
        if ((int)level_start.size() - 1 > depth_limit)
            throw unsupported_error(std::string(who) + ": the rebuilt tree is deeper than " + std::to_string(depth_limit) + " levels below the root, too deep for the traversal stack; the scene keeps its tree");
        const rebuild_level L{ keys_out.p, first.p, last.p, begin, count };
        hipLaunchKernelGGL(k_rebuild_count, blocks_for(count), dim3(256), 0, nullptr, L, counts.p);
        CTL_HIP(hipGetLastError());
        size_t need = 0;
        CTL_HIP(rocprim::inclusive_scan(nullptr, need, counts.p, incl.p, (size_t)count, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
        if (need > A.rebuild_temp_.n) throw std::runtime_error(std::string(who) + ": scan storage");
        bytes = A.rebuild_temp_.n;
        CTL_HIP(rocprim::inclusive_scan(A.rebuild_temp_.p, bytes, counts.p, incl.p, (size_t)count, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
        uint64_t total = 0;
        CTL_HIP(hipMemcpy(&total, incl.p + (count - 1u), 8, hipMemcpyDeviceToHost));
        const uint64_t n_inner = total >> 32, n_leaf_entries = total & 0xffffffffull;
        if ((uint64_t)begin + count + n_inner > cap || (uint64_t)begin + count + n_inner >= (1u << 24)) throw std::runtime_error(std::string(who) + ": the node count does not fit its buffer");
        if ((uint64_t)entry_base + n_leaf_entries > n) throw std::runtime_error(std::string(who) + ": the entry positions handed out exceed the entry count");
        hipLaunchKernelGGL(k_rebuild_emit, blocks_for(count), dim3(256), 0, nullptr, L, incl.p, idx_out.p, begin + count, entry_base, cap, n, nodes_new.p, perm.p);
        CTL_HIP(hipGetLastError());
        entry_base += (uint32_t)n_leaf_entries; begin += count; count = (uint32_t)n_inner;
        level_start.push_back(begin);
    }
    n_nodes = begin; max_depth = (int)level_start.size() - 2;
    if (entry_base != n) throw std::runtime_error(std::string(who) + ": the entry positions handed out do not sum to the entry count");
    level_iota.alloc(n_nodes);
    // 9. the entries in their final order
    const rebuild_gather G{ src_leaves, leaves_new.p, perm.p, n, src_part, part_new.p, A.refit_ebox_.p, ebox_new.p };
    hipLaunchKernelGGL(k_rebuild_gather, blocks_for(((size_t)n + 1) * 8), dim3(256), 0, nullptr, G);
    hipLaunchKernelGGL(k_rebuild_iota, blocks_for(n_nodes), dim3(256), 0, nullptr, level_iota.p, n_nodes);
    CTL_HIP(hipGetLastError());
    CTL_HIP(hipEventRecord(ev[3], nullptr));
    // 10. boxes, deepest level first, on the new arrays
    refit_device R2 = R;
    R2.nodes = nodes_new.p; R2.leaves = leaves_new.p; R2.n_nodes = n_nodes; R2.part_index = part_new.p; R2.ebox = ebox_new.p; R2.nbox = nbox_new.p;
    for (size_t l = level_start.size() - 1; l-- > 0;) launch_refit_level(nullptr, R2, level_iota.p + level_start[l], level_start[l + 1] - level_start[l]);
    CTL_HIP(hipEventRecord(ev[4], nullptr));
    launch_refit_area(nullptr, nodes_new.p, n_nodes, area_dev.p + 1);
    CTL_HIP(hipMemcpy(area, area_dev.p, 16, hipMemcpyDeviceToHost));
    CTL_HIP(hipDeviceSynchronize());
    for (int k = 0; k < 4; k++) CTL_HIP(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
}

void flat_rebuilder::commit(Scene& A) {
    // the swap: tracers read S at every launch
    swap_buffers(A.flat_nodes_, nodes_new); swap_buffers(A.flat_leaves_, leaves_new); swap_buffers(A.refit_part_index_, part_new); swap_buffers(A.refit_level_nodes_, level_iota);
    swap_buffers(A.refit_ebox_, ebox_new); swap_buffers(A.refit_nbox_, nbox_new);
    A.S.flat_nodes = A.flat_nodes_.p; A.S.flat_leaves = A.flat_leaves_.p; A.S.flat_root = 0; A.S.flat_top_cached = (int)std::min<size_t>(n_nodes, (size_t)flat_top_cache_nodes());
    A.flat_n_nodes_ = n_nodes; A.flat_n_entries_ = n; A.flat_max_depth_ = max_depth; A.flat_root_slab_ = false; A.flat_slab_nodes_ = 0;
    A.refit_.level_start = level_start;
}

void flat_rebuilder::report(ctl_scene_rebuild_stats& st) const {
    st.n_nodes = n_nodes; st.n_entries = n; st.max_depth = (uint32_t)max_depth; st.levels = (uint32_t)level_start.size() - 1u;
    st.node_area_before = area[0]; st.node_area_after = area[1];
    st.sort_ms = ms[1]; st.topology_ms = ms[2]; st.refit_ms = ms[0] + ms[3]; st.total_ms = ms[0] + ms[1] + ms[2] + ms[3];
}

void Scene::rebuild_flat(ctl_scene_rebuild_stats* stats) {
    require_device();
    const char* who = "ctl_scene_rebuild_flat";
    if (!flattened()) throw unsupported_error(std::string(who) + ": the scene was not created with CTL_SCENE_FLATTEN");
    rebuild_refuse(S.flat_format, refit_.level_start.size() >= 2 && refit_part_index_.p && refit_part_index_.n == flat_n_entries_, S.flat_compact != 0, flat_n_entries_, who);
    if (!snap_) throw std::runtime_error(std::string(who) + ": the scene holds no description");
    const ctl_scene_desc& d = snap_->d;
    if (d.n_nodes != refit_.xf0.size()) throw std::runtime_error(std::string(who) + ": the description has another number of nodes than the tree was built from");
    const std::vector<double> P = carry_matrices(d, refit_.xf0, who);
    CTL_HIP(hipDeviceSynchronize());   // no trace reads the arrays any more
    flat_rebuilder B; B.who = who; B.n = (uint32_t)flat_n_entries_; B.src_leaves = flat_leaves_.p; B.src_part = refit_part_index_.p;
    B.R.inst = inst_.p; B.R.inst_fwd = inst_fwd_.p; B.R.restamp = 0; B.R.leaf_keys = S.flat_leaf_keys; B.R.alpha_maps = (int)S.alpha_maps; B.R.tri_data = tri_data_.p; B.R.node_info = node_info_.p; B.R.mats = mats_.p;
    B.allocate(*this, P);
    B.run(*this);
    B.commit(*this);
    if (stats) B.report(*stats);
}

}  // namespace ctl
