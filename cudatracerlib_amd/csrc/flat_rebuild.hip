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
#include "tracer.h"
#include "flat_refit.h"
#include "flat_rebuild.h"
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

template <typename T> void swap_buffers(dbuf<T>& a, dbuf<T>& b) { std::swap(a.p, b.p); std::swap(a.n, b.n); }
inline dim3 blocks_for(size_t n) { return dim3((unsigned)((n + 255u) / 256u)); }
struct rebuild_events {
    hipEvent_t e[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    rebuild_events() { for (auto& x : e) CTL_HIP(hipEventCreate(&x)); }
    ~rebuild_events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

}  // namespace

void Scene::rebuild_flat(ctl_scene_rebuild_stats* stats) {
    require_device();
    const char* who = "ctl_scene_rebuild_flat";
    if (!flattened()) throw unsupported_error(std::string(who) + ": the scene was not created with CTL_SCENE_FLATTEN");
    rebuild_refuse(S.flat_format, refit_.level_start.size() >= 2 && refit_part_index_.p && refit_part_index_.n == flat_n_entries_, S.flat_compact != 0, flat_n_entries_, who);
    if (!snap_) throw std::runtime_error(std::string(who) + ": the scene holds no description");
    const ctl_scene_desc& d = snap_->d;
    if (d.n_nodes != refit_.xf0.size()) throw std::runtime_error(std::string(who) + ": the description has another number of nodes than the tree was built from");
    std::vector<double> P((size_t)d.n_nodes * 12);
    for (uint32_t k = 0; k < d.n_nodes; k++)
        if (!refit_carry_matrix(d.node_transforms[k].m, refit_.xf0[k].m, &P[(size_t)k * 12])) throw std::runtime_error(std::string(who) + ": singular node transform");
    // a wide node that is not the root has more than kRebuildLeafMax entries under it, and one with an inner child has four slots: fewer than n / 3 + 1 nodes with leaves of up
    // to four entries (the per-level check below holds whatever the bound)
    const uint32_t n = (uint32_t)flat_n_entries_, cap = (kRebuildLeafMax >= 4u ? n / 2u : n) + 2u;
    CTL_HIP(hipDeviceSynchronize());   // no trace reads the arrays any more
    // every allocation before the first write: a failed one leaves the scene as it was (the buffers below free themselves)
    dbuf<refit_box> ebox_cur, ebox_new, nbox_new; dbuf<uint32_t> bounds, idx_in, idx_out, first, last, perm, part_new, level_iota; dbuf<uint64_t> keys_in, keys_out, counts, incl;
    dbuf<float4> nodes_new, leaves_new; dbuf<double> carry, area; dbuf<unsigned char> temp;
    if (refit_ebox_.n < n) ebox_cur.alloc(n);
    ebox_new.alloc(n); nbox_new.alloc(cap); bounds.alloc(6); idx_in.alloc(n); idx_out.alloc(n); first.alloc(cap); last.alloc(cap); perm.alloc(n); part_new.alloc(n);
    keys_in.alloc(n); keys_out.alloc(n); counts.alloc(cap); incl.alloc(cap); nodes_new.alloc((size_t)cap * 4); leaves_new.alloc(((size_t)n + 1) * 8); carry.alloc(P.size()); area.alloc(2);
    size_t sort_bytes = 0, scan_bytes = 0;
    CTL_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys_in.p, keys_out.p, idx_in.p, idx_out.p, (size_t)n, 0u, 64u, (hipStream_t) nullptr));
    CTL_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, counts.p, incl.p, (size_t)cap, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
    const size_t temp_need = std::max<size_t>(std::max(sort_bytes, scan_bytes), 16);
    if (rebuild_temp_.n < temp_need) { temp.alloc(temp_need); swap_buffers(rebuild_temp_, temp); temp.free(); }   // (scratch of no meaning between calls: kept)
    rebuild_events ev;
    if (ebox_cur.p) swap_buffers(refit_ebox_, ebox_cur);
    swap_buffers(refit_carry_, carry);
    CTL_HIP(hipMemcpy(refit_carry_.p, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice));

    refit_device R{};
    R.nodes = flat_nodes_.p; R.leaves = flat_leaves_.p; R.n_nodes = (uint32_t)flat_n_nodes_; R.n_entries = n; R.compact = 1;
    R.part_index = refit_part_index_.p; R.part_boxes = refit_part_boxes_.p; R.inst = inst_.p; R.inst_fwd = inst_fwd_.p; R.carry = refit_carry_.p; R.ebox = refit_ebox_.p; R.nbox = refit_nbox_.p;
    R.restamp = 0; R.leaf_keys = S.flat_leaf_keys; R.alpha_maps = (int)S.alpha_maps; R.tri_data = tri_data_.p; R.node_info = node_info_.p; R.mats = mats_.p;
    CTL_HIP(hipMemsetAsync(area.p, 0, 16, nullptr));
    launch_refit_area(nullptr, flat_nodes_.p, R.n_nodes, area.p);
    // 1. entry boxes
    CTL_HIP(hipEventRecord(ev.e[0], nullptr));
    launch_refit_entries(nullptr, R, true);
    CTL_HIP(hipEventRecord(ev.e[1], nullptr));
    // 2. - 4. bounds, keys, sort
    CTL_HIP(hipMemsetAsync(bounds.p, 0xff, 12, nullptr)); CTL_HIP(hipMemsetAsync(bounds.p + 3, 0, 12, nullptr));
    hipLaunchKernelGGL(k_rebuild_bounds, dim3(std::min<unsigned>(blocks_for(n).x, 1024u)), dim3(256), 0, nullptr, refit_ebox_.p, n, bounds.p);
    hipLaunchKernelGGL(k_rebuild_keys, blocks_for(n), dim3(256), 0, nullptr, refit_ebox_.p, n, bounds.p, keys_in.p, idx_in.p);
    CTL_HIP(hipGetLastError());
    size_t bytes = rebuild_temp_.n;
    CTL_HIP(rocprim::radix_sort_pairs(rebuild_temp_.p, bytes, keys_in.p, keys_out.p, idx_in.p, idx_out.p, (size_t)n, 0u, 64u, (hipStream_t) nullptr));
    CTL_HIP(hipEventRecord(ev.e[2], nullptr));
    // 5. - 8. the wide nodes, level by level
    const uint32_t root_range[2] = { 0u, n - 1u };
    CTL_HIP(hipMemcpy(first.p, &root_range[0], 4, hipMemcpyHostToDevice)); CTL_HIP(hipMemcpy(last.p, &root_range[1], 4, hipMemcpyHostToDevice));
    std::vector<uint32_t> level_start{ 0u };
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
        if (need > rebuild_temp_.n) throw std::runtime_error(std::string(who) + ": scan storage");
        bytes = rebuild_temp_.n;
        CTL_HIP(rocprim::inclusive_scan(rebuild_temp_.p, bytes, counts.p, incl.p, (size_t)count, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
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
    const uint32_t n_nodes = begin; const int max_depth = (int)level_start.size() - 2;
    if (entry_base != n) throw std::runtime_error(std::string(who) + ": the entry positions handed out do not sum to the entry count");
    level_iota.alloc(n_nodes);
    // 9. the entries in their final order
    const rebuild_gather G{ flat_leaves_.p, leaves_new.p, perm.p, n, refit_part_index_.p, part_new.p, refit_ebox_.p, ebox_new.p };
    hipLaunchKernelGGL(k_rebuild_gather, blocks_for(((size_t)n + 1) * 8), dim3(256), 0, nullptr, G);
    hipLaunchKernelGGL(k_rebuild_iota, blocks_for(n_nodes), dim3(256), 0, nullptr, level_iota.p, n_nodes);
    CTL_HIP(hipGetLastError());
    CTL_HIP(hipEventRecord(ev.e[3], nullptr));
    // 10. boxes, deepest level first, on the new arrays
    refit_device R2 = R;
    R2.nodes = nodes_new.p; R2.leaves = leaves_new.p; R2.n_nodes = n_nodes; R2.part_index = part_new.p; R2.ebox = ebox_new.p; R2.nbox = nbox_new.p;
    for (size_t l = level_start.size() - 1; l-- > 0;) launch_refit_level(nullptr, R2, level_iota.p + level_start[l], level_start[l + 1] - level_start[l]);
    CTL_HIP(hipEventRecord(ev.e[4], nullptr));
    launch_refit_area(nullptr, nodes_new.p, n_nodes, area.p + 1);
    double a[2] = { 0, 0 };
    CTL_HIP(hipMemcpy(a, area.p, 16, hipMemcpyDeviceToHost));
    CTL_HIP(hipDeviceSynchronize());
    // the swap: tracers read S at every launch
    swap_buffers(flat_nodes_, nodes_new); swap_buffers(flat_leaves_, leaves_new); swap_buffers(refit_part_index_, part_new); swap_buffers(refit_level_nodes_, level_iota);
    swap_buffers(refit_ebox_, ebox_new); swap_buffers(refit_nbox_, nbox_new);
    S.flat_nodes = flat_nodes_.p; S.flat_leaves = flat_leaves_.p; S.flat_root = 0; S.flat_top_cached = (int)std::min<size_t>(n_nodes, (size_t)flat_top_cache_nodes());
    flat_n_nodes_ = n_nodes; flat_max_depth_ = max_depth; flat_root_slab_ = false; flat_slab_nodes_ = 0;
    refit_.level_start = level_start;
    if (stats) {
        float t01 = 0, t12 = 0, t23 = 0, t34 = 0;
        CTL_HIP(hipEventElapsedTime(&t01, ev.e[0], ev.e[1])); CTL_HIP(hipEventElapsedTime(&t12, ev.e[1], ev.e[2])); CTL_HIP(hipEventElapsedTime(&t23, ev.e[2], ev.e[3])); CTL_HIP(hipEventElapsedTime(&t34, ev.e[3], ev.e[4]));
        stats->n_nodes = n_nodes; stats->n_entries = n; stats->max_depth = (uint32_t)max_depth; stats->levels = (uint32_t)level_start.size() - 1u;
        stats->node_area_before = a[0]; stats->node_area_after = a[1];
        stats->sort_ms = t12; stats->topology_ms = t23; stats->refit_ms = t01 + t34; stats->total_ms = t01 + t12 + t23 + t34;
    }
}

}  // namespace ctl
