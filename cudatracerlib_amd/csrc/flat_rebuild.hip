// flat_rebuild.hip — the rebuild of the flattened Q4 tree on the device (ctl_scene_rebuild_flat): the kernels around the functions of flat_rebuild.h, which the host
// rebuild (flat_rebuild.cpp rebuild_flat_scene) runs too — same functions, same order, so the device tree equals the host's byte for byte (tests/test_gpu_flat_rebuild.py).
//
//   k_refit_entries    (flat_refit.hip, as it is) every entry's world box for the current transforms
//   k_rebuild_bounds   min / max of the valid boxes as ordered integers: a wave reduction, then one integer atomic min / max per wave and axis — exact, whatever the order
//   k_rebuild_keys     one lane per entry: its Morton code and its index
//   rocPRIM            radix_sort_pairs over (code, index): stable, so equal codes keep index order
//   CTL_REBUILD_PLOC only (flat_ploc.h), per round until one cluster is left (the host reads the round's totals back — 8 B — and checks them before the merge writes):
//     k_ploc_nearest   one lane per cluster: the boxes of the workgroup's clusters and of kPlocRadius to either side staged in LDS, the search from LDS
//     k_ploc_flags     merge flag << 32 | survivor flag per cluster
//     rocPRIM          inclusive_scan over the round's flags
//     k_ploc_merge     survivors to their new positions, merged pairs with their new binary node (children, entry count, union box)
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

// ---- CTL_REBUILD_PLOC: the clustering rounds (flat_ploc.h)

// the clusters of round 0: the sorted entries
__global__ void __launch_bounds__(256) k_ploc_init(const refit_box* __restrict__ ebox, const uint32_t* __restrict__ sorted_index, uint32_t n, const uint32_t* __restrict__ bounds,
                                                   refit_box* __restrict__ cbox, uint32_t* __restrict__ cid) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    refit_box B;
    for (int k = 0; k < 3; k++) { B.lo[k] = rebuild_unord(bounds[k]); B.hi[k] = rebuild_unord(bounds[3 + k]); }
    const uint32_t src = sorted_index[i];
    if (src >= n) return;   // cannot happen: the sort permutes 0 .. n - 1; never read outside the array
    cbox[i] = ploc_cluster_box(ebox[src], B);
    cid[i] = i;
}

// The hot kernel of a round: one lane per cluster.  The workgroup stages the boxes of its 256 clusters and of kPlocRadius clusters to either side in LDS, one array per
// box component, so that the 64 lanes of a wave read 64 consecutive words at every step of the search (no bank is asked twice), and every box is fetched from memory once
// per workgroup instead of 2 kPlocRadius + 1 times.  6 (256 + 2 kPlocRadius) words = 6.4 KB of LDS at radius 8.
constexpr uint32_t kPlocTile = 256u + 2u * kPlocRadius;
struct ploc_lds_boxes {
    const float (*c)[kPlocTile]; uint32_t origin;   // position `origin` (which may be "negative": kPlocRadius before the workgroup's first) is tile slot 0
    __device__ refit_box operator()(uint32_t j) const {
        const uint32_t s = j - origin;
        refit_box b;
        for (int k = 0; k < 3; k++) { b.lo[k] = c[k][s]; b.hi[k] = c[3 + k][s]; }
        return b;
    }
};
__global__ void __launch_bounds__(256) k_ploc_nearest(const refit_box* __restrict__ cbox, uint32_t m, uint32_t* __restrict__ pick) {
    __shared__ float tile[6][kPlocTile];
    const uint32_t base = blockIdx.x * 256u, origin = base - kPlocRadius;   // (wraps in the first workgroup; position - origin does not)
    for (uint32_t s = threadIdx.x; s < kPlocTile; s += 256u) {
        const uint32_t g = origin + s;
        if (g < m) {   // (a wrapped g is >= m: m < 2^26)
            const refit_box b = cbox[g];
            for (int k = 0; k < 3; k++) { tile[k][s] = b.lo[k]; tile[3 + k][s] = b.hi[k]; }
        }
    }
    __syncthreads();
    const uint32_t i = base + threadIdx.x;
    if (i >= m) return;
    pick[i] = ploc_nearest(ploc_lds_boxes{ tile, origin }, m, i);   // reads the slots of positions max(i - r, 0) .. min(i + r, m - 1): all staged
}

__global__ void __launch_bounds__(256) k_ploc_flags(const uint32_t* __restrict__ pick, uint32_t m, uint64_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < m) flags[i] = ploc_round_flags(pick, m, i);
}

// the survivors to their new positions, the merged ones with their new node: n + made + rank.  The host has checked the round's totals (survivors = m - merges,
// made + merges <= n - 1) before this launch; never write outside the arrays all the same
struct ploc_round { const refit_box* box_in; const uint32_t* id_in; const uint32_t* pick; const uint64_t* incl; uint32_t m, made, n; refit_box* box_out; uint32_t* id_out; uint32_t *left, *right, *count; };
__global__ void __launch_bounds__(256) k_ploc_merge(ploc_round P) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P.m) return;
    const uint64_t f = ploc_round_flags(P.pick, P.m, i);
    if (!(f & 1ull)) return;
    const uint64_t before = P.incl[i] - f;
    const uint32_t pos = (uint32_t)before, rank = (uint32_t)(before >> 32);
    if (pos >= P.m) return;
    if (f >> 32) {
        const uint32_t p = P.pick[i], j = P.made + rank;
        if (j + 1u >= P.n) return;
        const ploc_tree T{ P.n, P.left, P.right, P.count };
        const uint32_t a = P.id_in[i], b = P.id_in[p];
        const uint32_t entries = T.entries(a) + T.entries(b);   // (inner nodes of earlier rounds: written by earlier launches)
        P.left[j] = a; P.right[j] = b; P.count[j] = entries;
        P.id_out[pos] = P.n + j; P.box_out[pos] = ploc_union(P.box_in[i], P.box_in[p]);
    } else { P.id_out[pos] = P.id_in[i]; P.box_out[pos] = P.box_in[i]; }
}

// ---- the wide nodes, over either binary tree (Tree: rebuild_lbvh_tree, ploc_tree)
struct rebuild_level { uint32_t* first; uint32_t* last; uint32_t begin, count; };

template <typename Tree> __global__ void __launch_bounds__(256) k_rebuild_count(Tree T, rebuild_level L, uint64_t* __restrict__ counts) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= L.count) return;
    rebuild_slots S; rebuild_node_slots(T, L.first[L.begin + j], L.last[L.begin + j], S);
    counts[j] = rebuild_slot_counts(S);
}

// child_base / entry_base: the first node of the next level / the first entry position of this level; cap_nodes / n_entries: the sizes of the arrays written (the host has
// checked the level's totals against them; never write outside the arrays)
template <typename Tree> __global__ void __launch_bounds__(256) k_rebuild_emit(Tree T, rebuild_level L, const uint64_t* __restrict__ incl, const uint32_t* __restrict__ sorted_index, uint32_t child_base, uint32_t entry_base,
                                                      uint32_t cap_nodes, uint32_t n_entries, float4* __restrict__ nodes, uint32_t* __restrict__ perm) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= L.count) return;
    const uint32_t i = L.begin + j;
    rebuild_slots S; rebuild_node_slots(T, L.first[i], L.last[i], S);
    const uint64_t before = incl[j] - rebuild_slot_counts(S);
    uint32_t child = child_base + (uint32_t)(before >> 32), entry = entry_base + (uint32_t)before;
    uint32_t w[16]; rebuild_encode_node(S, child, entry, w);
    float4* __restrict__ N = nodes + (size_t)i * 4;
    for (int q = 0; q < 4; q++) N[q] = make_float4(__uint_as_float(w[4 * q]), __uint_as_float(w[4 * q + 1]), __uint_as_float(w[4 * q + 2]), __uint_as_float(w[4 * q + 3]));
    for (uint32_t k = 0; k < S.n; k++) {
        if (S.leaf(k)) {
            for (uint32_t e = 0, c = S.count(k); e < c; e++, entry++) {
                const uint32_t s = T.entry(S.first[k], S.last[k], e);
                if (entry < n_entries && s < n_entries) perm[entry] = sorted_index[s] | (e + 1u == c ? kRebuildLastBit : 0u);
            }
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
    if (builder == CTL_REBUILD_PLOC) {
        for (int k = 0; k < 2; k++) { cbox[k].alloc(n); cid[k].alloc(n); }
        pick.alloc(n); tree_left.alloc(n); tree_right.alloc(n); tree_count.alloc(n); round_flags.alloc(n); round_incl.alloc(n);
    }
    size_t sort_bytes = 0, scan_bytes = 0, round_bytes = 0;
    CTL_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys_in.p, keys_out.p, idx_in.p, idx_out.p, (size_t)n, 0u, 64u, (hipStream_t) nullptr));
    CTL_HIP(rocprim::inclusive_scan(nullptr, scan_bytes, counts.p, incl.p, (size_t)cap, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
    if (builder == CTL_REBUILD_PLOC) CTL_HIP(rocprim::inclusive_scan(nullptr, round_bytes, round_flags.p, round_incl.p, (size_t)n, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
    const size_t temp_need = std::max<size_t>(std::max(std::max(sort_bytes, scan_bytes), round_bytes), 16);
    if (A.rebuild_temp_.n < temp_need) { temp.alloc(temp_need); swap_buffers(A.rebuild_temp_, temp); temp.free(); }   // (scratch of no meaning between calls: kept)
    for (auto& x : ev) CTL_HIP(hipEventCreate(&x));
    if (ebox_cur.p) swap_buffers(A.refit_ebox_, ebox_cur);
    swap_buffers(A.refit_carry_, carry);
    CTL_HIP(hipMemcpy(A.refit_carry_.p, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice));
    R.nodes = A.flat_nodes_.p; R.leaves = src_leaves; R.n_nodes = (uint32_t)A.flat_n_nodes_; R.n_entries = n; R.compact = 1;
    R.part_index = src_part; R.part_boxes = A.refit_part_boxes_.p; R.carry = A.refit_carry_.p; R.ebox = A.refit_ebox_.p; R.nbox = A.refit_nbox_.p;
}

// 5. the clustering rounds.  Per round the host reads the round's totals back (8 B) and checks them before anything is written with them; the loop ends by its own checks
// (flat_ploc.h "Progress"), never by looping on
void flat_rebuilder::cluster(Scene& A) {
    hipLaunchKernelGGL(k_ploc_init, blocks_for(n), dim3(256), 0, nullptr, A.refit_ebox_.p, idx_out.p, n, bounds.p, cbox[0].p, cid[0].p);
    CTL_HIP(hipGetLastError());
    const uint32_t cap_rounds = ploc_round_cap(n);
    uint32_t m = n, made = 0u; int cur = 0;
    while (m > 1u) {
        if (rounds == cap_rounds) throw unsupported_error(std::string(who) + ": the clustering needs more than " + std::to_string(cap_rounds) + " rounds; the scene keeps its tree");
        rounds++;
        hipLaunchKernelGGL(k_ploc_nearest, blocks_for(m), dim3(256), 0, nullptr, cbox[cur].p, m, pick.p);
        hipLaunchKernelGGL(k_ploc_flags, blocks_for(m), dim3(256), 0, nullptr, pick.p, m, round_flags.p);
        CTL_HIP(hipGetLastError());
        size_t need = 0;
        CTL_HIP(rocprim::inclusive_scan(nullptr, need, round_flags.p, round_incl.p, (size_t)m, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
        if (need > A.rebuild_temp_.n) throw std::runtime_error(std::string(who) + ": scan storage");
        size_t bytes = A.rebuild_temp_.n;
        CTL_HIP(rocprim::inclusive_scan(A.rebuild_temp_.p, bytes, round_flags.p, round_incl.p, (size_t)m, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
        uint64_t total = 0;
        CTL_HIP(hipMemcpy(&total, round_incl.p + (m - 1u), 8, hipMemcpyDeviceToHost));
        const uint64_t merges = total >> 32, survivors = total & 0xffffffffull;
        if (merges == 0u) throw internal_error(std::string(who) + ": a clustering round merged nothing");
        if (survivors + merges != m || (uint64_t)made + merges > (uint64_t)n - 1u) throw std::runtime_error(std::string(who) + ": the clustering round's totals do not fit the cluster count");
        const ploc_round P{ cbox[cur].p, cid[cur].p, pick.p, round_incl.p, m, made, n, cbox[cur ^ 1].p, cid[cur ^ 1].p, tree_left.p, tree_right.p, tree_count.p };
        hipLaunchKernelGGL(k_ploc_merge, blocks_for(m), dim3(256), 0, nullptr, P);
        CTL_HIP(hipGetLastError());
        made += (uint32_t)merges; m = (uint32_t)survivors; cur ^= 1;
    }
    if (made != n - 1u) throw std::runtime_error(std::string(who) + ": the clustering did not end in one tree");
}

// 6. - 8. the wide nodes, level by level
template <typename Tree> void flat_rebuilder::wide_nodes(Scene& A, const Tree& T) {
    const uint32_t root_range[2] = { T.root_first(n), T.root_first(n) + n - 1u };
    CTL_HIP(hipMemcpy(first.p, &root_range[0], 4, hipMemcpyHostToDevice)); CTL_HIP(hipMemcpy(last.p, &root_range[1], 4, hipMemcpyHostToDevice));
    level_start.assign(1, 0u);
    uint32_t begin = 0, count = 1, entry_base = 0;
    const int depth_limit = (kStackSize - 4) / 3;   // stack_need() + 2 <= kStackSize, as at creation
    while (count) {
        if ((int)level_start.size() - 1 > depth_limit)
            throw unsupported_error(std::string(who) + ": the rebuilt tree is deeper than " + std::to_string(depth_limit) + " levels below the root, too deep for the traversal stack; the scene keeps its tree");
        const rebuild_level L{ first.p, last.p, begin, count };
        hipLaunchKernelGGL(k_rebuild_count<Tree>, blocks_for(count), dim3(256), 0, nullptr, T, L, counts.p);
        CTL_HIP(hipGetLastError());
        size_t need = 0;
        CTL_HIP(rocprim::inclusive_scan(nullptr, need, counts.p, incl.p, (size_t)count, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
        if (need > A.rebuild_temp_.n) throw std::runtime_error(std::string(who) + ": scan storage");
        size_t bytes = A.rebuild_temp_.n;
        CTL_HIP(rocprim::inclusive_scan(A.rebuild_temp_.p, bytes, counts.p, incl.p, (size_t)count, rocprim::plus<uint64_t>(), (hipStream_t) nullptr));
        uint64_t total = 0;
        CTL_HIP(hipMemcpy(&total, incl.p + (count - 1u), 8, hipMemcpyDeviceToHost));
        const uint64_t n_inner = total >> 32, n_leaf_entries = total & 0xffffffffull;
        if ((uint64_t)begin + count + n_inner > cap || (uint64_t)begin + count + n_inner >= (1u << 24)) throw std::runtime_error(std::string(who) + ": the node count does not fit its buffer");
        if ((uint64_t)entry_base + n_leaf_entries > n) throw std::runtime_error(std::string(who) + ": the entry positions handed out exceed the entry count");
        hipLaunchKernelGGL(k_rebuild_emit<Tree>, blocks_for(count), dim3(256), 0, nullptr, T, L, incl.p, idx_out.p, begin + count, entry_base, cap, n, nodes_new.p, perm.p);
        CTL_HIP(hipGetLastError());
        entry_base += (uint32_t)n_leaf_entries; begin += count; count = (uint32_t)n_inner;
        level_start.push_back(begin);
    }
    n_nodes = begin; max_depth = (int)level_start.size() - 2;
    if (entry_base != n) throw std::runtime_error(std::string(who) + ": the entry positions handed out do not sum to the entry count");
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
    // 5. - 8. the binary tree and the wide nodes over it
    rounds = 0u;
    if (builder == CTL_REBUILD_PLOC) { cluster(A); wide_nodes(A, ploc_tree{ n, tree_left.p, tree_right.p, tree_count.p }); }
    else wide_nodes(A, rebuild_lbvh_tree{ keys_out.p });
    rebuild_last_rounds() = rounds;
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
    rebuild_last_rounds() = 0u;
    flat_rebuilder B; B.builder = rebuild_builder_choice(); B.who = who; B.n = (uint32_t)flat_n_entries_; B.src_leaves = flat_leaves_.p; B.src_part = refit_part_index_.p;
    B.R.inst = inst_.p; B.R.inst_fwd = inst_fwd_.p; B.R.restamp = 0; B.R.leaf_keys = S.flat_leaf_keys; B.R.alpha_maps = (int)S.alpha_maps; B.R.tri_data = tri_data_.p; B.R.node_info = node_info_.p; B.R.mats = mats_.p;
    B.allocate(*this, P);
    B.run(*this);
    B.commit(*this);
    if (stats) B.report(*stats);
}

}  // namespace ctl
