// flat_rebuild.cpp — the host rebuild of the flattened Q4 tree (ctl_flat_bvh_rebuild): the yardstick of the kernels in flat_rebuild.hip, which run the same functions of
// flat_rebuild.h and flat_refit.h in the same order, so the device tree equals this one byte for byte (tests/test_gpu_flat_rebuild.py).
#include "flatten.h"
#include "flat_rebuild.h"
#include "flat_ploc.h"
#include "device_scene.h"     // kStackSize
#include "mitsuba_loader.h"   // unsupported_error
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>

namespace ctl {

namespace {
template <typename F> void in_threads(size_t n, F f) {
    const size_t nt = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(std::thread::hardware_concurrency(), 16), n / 4096));
    if (nt <= 1) { f((size_t)0, n); return; }
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; t++) th.emplace_back([&, t]() { f(n * t / nt, n * (t + 1) / nt); });
    for (auto& x : th) x.join();
}
}  // namespace

void rebuild_refuse(int format, bool refit_ready, bool compact, size_t n_entries, const char* who) {
    if (format != kFlatQ4) throw unsupported_error(std::string(who) + ": only the Q4 node format can be rebuilt");
    if (!refit_ready) throw unsupported_error(std::string(who) + ": the flattened tree carries no refit data");
    if (!compact) throw unsupported_error(std::string(who) + ": a tree with explicit links is not rebuilt (the rebuilt layout spells implied links)");
    if (n_entries == 0 || n_entries + 15u >= (1u << 26)) throw unsupported_error(std::string(who) + ": the entry count does not fit the implied links");
}

int& rebuild_builder_choice() { static thread_local int b = CTL_REBUILD_LBVH; return b; }
uint32_t& rebuild_last_rounds() { static thread_local uint32_t r = 0u; return r; }

void rebuild_flat_scene(flat_scene& F, const ctl_scene_desc& d, double* area_before_after, int builder) {
    rebuild_last_rounds() = 0u;
    rebuild_refuse(F.format, F.refit.ready() && F.refit.part_index.size() == F.leaves.size(), F.compact_links, F.leaves.size(), "rebuild");
    double refit_area[2] = { 0, 0 };
    refit_flat_scene(F, d, refit_area);   // the pose (and the vertex values) of `d`: what ctl_scene_update does before ctl_scene_rebuild_flat; throws before it writes
    rebuild_flat_entries(F, d, builder);
    if (area_before_after) { area_before_after[0] = refit_area[1]; area_before_after[1] = flat_scene_node_area(F); }
}

namespace {
// 5. PLOC's clustering (flat_ploc.h), the rounds one after the other: cbox = the boxes of the sorted entries.  Fills the stored tree; returns the rounds
uint32_t ploc_cluster(std::vector<refit_box> cbox, std::vector<uint32_t>& left, std::vector<uint32_t>& right, std::vector<uint32_t>& count) {
    const uint32_t n = (uint32_t)cbox.size(), cap = ploc_round_cap(n);
    left.assign(n, 0u); right.assign(n, 0u); count.assign(n, 0u);
    const ploc_tree T{ n, left.data(), right.data(), count.data() };
    std::vector<uint32_t> id(n), nn(n), nid; std::vector<refit_box> nbox;
    for (uint32_t i = 0; i < n; i++) id[i] = i;
    uint32_t m = n, made = 0u, rounds = 0u;
    while (m > 1u) {
        if (rounds == cap) throw unsupported_error("rebuild: the clustering needs more than " + std::to_string(cap) + " rounds; the tree is left as it was");
        rounds++;
        const refit_box* B = cbox.data();
        for (uint32_t i = 0; i < m; i++) nn[i] = ploc_nearest([B](uint32_t j) { return B[j]; }, m, i);
        nid.clear(); nbox.clear();
        uint32_t merges = 0u;
        for (uint32_t i = 0; i < m; i++) {
            const uint64_t f = ploc_round_flags(nn.data(), m, i);
            if (!(f & 1ull)) continue;
            if (f >> 32) {
                const uint32_t p = nn[i], j = made + merges;
                left[j] = id[i]; right[j] = id[p]; count[j] = T.entries(id[i]) + T.entries(id[p]);
                nid.push_back(n + j); nbox.push_back(ploc_union(cbox[i], cbox[p])); merges++;
            } else { nid.push_back(id[i]); nbox.push_back(cbox[i]); }
        }
        if (merges == 0u) throw internal_error("rebuild: a clustering round merged nothing");
        made += merges; m -= merges;
        id.swap(nid); cbox.swap(nbox);
    }
    return rounds;
}

struct wide_levels { std::vector<uint32_t> level_start, perm; std::vector<flat4_node> nodes; std::vector<int32_t> links; uint32_t entries = 0; };
// 6. - 8. the wide nodes, level by level, over either binary tree
template <typename Tree> void wide_nodes(const Tree& T, uint32_t n, const std::vector<std::pair<uint64_t, uint32_t>>& order, wide_levels& W) {
    std::vector<uint32_t> first{ T.root_first(n) }, last{ T.root_first(n) + n - 1u };
    std::vector<uint32_t>& level_start = W.level_start; std::vector<uint32_t>& perm = W.perm; std::vector<flat4_node>& nodes = W.nodes; std::vector<int32_t>& links = W.links;
    level_start.assign(1, 0u); perm.assign(n, 0u);
    uint32_t entry_base = 0;
    for (uint32_t l = 0; level_start[l] < first.size(); l++) {
        const uint32_t begin = level_start[l], end = (uint32_t)first.size();
        uint32_t child = end, entry = entry_base;
        nodes.resize(end); links.resize((size_t)end * 4, 0x76543210);
        for (uint32_t i = begin; i < end; i++) {
            rebuild_slots S; rebuild_node_slots(T, first[i], last[i], S);
            uint32_t w[16]; rebuild_encode_node(S, child, entry, w);
            std::memcpy(&nodes[i], w, 64);
            for (uint32_t k = 0; k < S.n; k++) {
                if (S.leaf(k)) {
                    links[(size_t)i * 4 + k] = ~(int32_t)entry;
                    for (uint32_t e = 0, c = S.count(k); e < c; e++) perm[entry++] = order[T.entry(S.first[k], S.last[k], e)].second | (e + 1u == c ? kRebuildLastBit : 0u);
                } else { links[(size_t)i * 4 + k] = (int32_t)(child * 4u); first.push_back(S.first[k]); last.push_back(S.last[k]); child++; }
            }
        }
        entry_base = entry;
        level_start.push_back(end);
    }
    W.entries = entry_base;
}
}  // namespace

void rebuild_sorted_entries(const flat_scene& F, const ctl_scene_desc& d, std::vector<refit_box>& ebox, refit_box& bounds, std::vector<std::pair<uint64_t, uint32_t>>& order) {
    const uint32_t n = (uint32_t)F.leaves.size();
    // 1. entry boxes
    std::vector<double> P((size_t)d.n_nodes * 12);
    for (uint32_t k = 0; k < d.n_nodes; k++)
        if (!refit_carry_matrix(d.node_transforms[k].m, F.refit.xf0[k].m, &P[(size_t)k * 12])) throw std::runtime_error("rebuild: singular node transform");
    ebox.resize(n);
    in_threads(n, [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            const flat_leaf& L = F.leaves[i];
            const uint32_t pi = F.refit.part_index[i];
            refit_entry_box(L.a, L.b, L.c, d.node_transforms[L.node].m, pi == kRefitNoPart ? nullptr : &F.refit.part_boxes[pi], &P[(size_t)L.node * 12], ebox[i]);
        }
    });
    // 2. bounds  3. keys  4. sort
    uint32_t lo[3] = { 0xffffffffu, 0xffffffffu, 0xffffffffu }, hi[3] = { 0u, 0u, 0u };
    for (uint32_t i = 0; i < n; i++) if (rebuild_box_valid(ebox[i])) for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], rebuild_ord(ebox[i].lo[k])); hi[k] = std::max(hi[k], rebuild_ord(ebox[i].hi[k])); }
    for (int k = 0; k < 3; k++) { bounds.lo[k] = rebuild_unord(lo[k]); bounds.hi[k] = rebuild_unord(hi[k]); }
    order.resize(n);
    for (uint32_t i = 0; i < n; i++) order[i] = { rebuild_key(ebox[i], bounds), i };
    std::sort(order.begin(), order.end());
}

void rebuild_flat_entries(flat_scene& F, const ctl_scene_desc& d, int builder) {
    const uint32_t n = (uint32_t)F.leaves.size();
    std::vector<refit_box> ebox; refit_box bounds; std::vector<std::pair<uint64_t, uint32_t>> order;
    rebuild_sorted_entries(F, d, ebox, bounds, order);
    std::vector<uint64_t> keys(n);
    for (uint32_t i = 0; i < n; i++) keys[i] = order[i].first;
    // 5. - 8. the binary tree and the wide nodes over it
    wide_levels W;
    uint32_t rounds = 0u;
    if (builder == CTL_REBUILD_PLOC) {
        std::vector<refit_box> cbox(n);
        for (uint32_t i = 0; i < n; i++) cbox[i] = ploc_cluster_box(ebox[order[i].second], bounds);
        std::vector<uint32_t> left, right, count;
        rounds = ploc_cluster(std::move(cbox), left, right, count);
        wide_nodes(ploc_tree{ n, left.data(), right.data(), count.data() }, n, order, W);
    } else wide_nodes(rebuild_lbvh_tree{ keys.data() }, n, order, W);
    rebuild_last_rounds() = rounds;
    std::vector<uint32_t>& level_start = W.level_start; std::vector<uint32_t>& perm = W.perm; std::vector<flat4_node>& nodes = W.nodes; std::vector<int32_t>& links = W.links;
    const uint32_t entry_base = W.entries;
    const int max_depth = (int)level_start.size() - 2;
    if (entry_base != n) throw std::runtime_error("rebuild: the entry positions handed out do not sum to the entry count");
    if (nodes.size() >= (1u << 24)) throw unsupported_error("rebuild: the node count does not fit the implied links");
    if (3 * max_depth + 2 + 2 > kStackSize) throw unsupported_error("rebuild: the rebuilt tree (depth " + std::to_string(max_depth) + ") is too deep for the traversal stack; the tree is left refitted");
    // 9. the entries in their final order
    std::vector<flat_leaf> leaves(n); std::vector<uint32_t> part_index(n); std::vector<refit_box> nebox(n);
    for (uint32_t p = 0; p < n; p++) {
        const uint32_t src = perm[p] & ~kRebuildLastBit;
        leaves[p] = F.leaves[src]; leaves[p].index = (leaves[p].index & ~1u) | ((perm[p] & kRebuildLastBit) ? 1u : 0u);
        part_index[p] = F.refit.part_index[src]; nebox[p] = ebox[src];
    }
    F.nodes.swap(nodes); F.leaves.swap(leaves); F.child_links.swap(links); F.refit.part_index.swap(part_index);
    F.max_depth = max_depth; F.root_slab = false; F.slab_nodes = 0;
    F.refit.level_start = level_start;
    F.refit.level_nodes.resize(F.nodes.size());
    for (size_t i = 0; i < F.nodes.size(); i++) F.refit.level_nodes[i] = (uint32_t)i;
    // 10. boxes, deepest level first (the loop of refit_flat_scene)
    std::vector<refit_box> nbox(F.nodes.size());
    for (size_t l = level_start.size() - 1; l-- > 0;)
        for (uint32_t i = level_start[l]; i < level_start[l + 1]; i++) {
            flat4_node& nd = F.nodes[i];
            const uint32_t exist = nd.mask & 15u;
            refit_box cb[4];
            for (int c = 0; c < 4; c++) {
                if (!((exist >> c) & 1u)) continue;
                const int32_t k = F.child_links[(size_t)i * 4 + c];
                if (k >= 0) { cb[c] = nbox[(size_t)k / 4]; continue; }
                for (int r = 0; r < 3; r++) { cb[c].lo[r] = kRefitBig; cb[c].hi[r] = -kRefitBig; }
                for (uint32_t e = (uint32_t)~k;; e++) {
                    for (int r = 0; r < 3; r++) { cb[c].lo[r] = refit_min(cb[c].lo[r], nebox[e].lo[r]); cb[c].hi[r] = refit_max(cb[c].hi[r], nebox[e].hi[r]); }
                    if (F.leaves[e].index & 1u) break;
                }
            }
            uint32_t w[10]; std::memcpy(w, &nd, 40);
            refit_node_boxes(w, exist, cb, nbox[i]);
            std::memcpy(&nd, w, 40);
        }
}

}  // namespace ctl
