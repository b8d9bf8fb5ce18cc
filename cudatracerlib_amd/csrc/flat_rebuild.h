// flat_rebuild.h — NEW TOPOLOGY for the flattened Q4 tree (flatten.h) of a live scene: the arithmetic, single source for the host (flat_rebuild.cpp
// rebuild_flat_scene, what ctl_flat_bvh_rebuild runs) and the device (flat_rebuild.hip, what ctl_scene_rebuild_flat runs).
//
// A refit (flat_refit.h) keeps the tree correct, not good: after a large motion the boxes overlap and the rays/s fall.  A rebuild keeps the SET of leaf entries — their
// 128 B move untouched but for the "last entry of its leaf" bit — and makes a new order of them and a new tree above them:
//   1. entry boxes     refit_entry_box for the current transforms (split references keep their clip box, carried from the creation pose as in a refit)
//   2. bounds          min / max over the boxes that are not inverted, compared as ordered integers (rebuild_ord): exact, so any reduction order gives the same bits
//   3. keys            63-bit Morton code of lo + hi (twice the centre) against the bounds, 21 bits per axis; an inverted box (singular Woop matrix, collapsed triangle)
//                      gets the largest code: the entry stays in the tree, a later geometry update may give it rows again
//   4. sort            by (code, entry index): a stable sort of (code, index) pairs
//   5. hierarchy       Karras's binary radix tree over the sorted keys, the position in the sorted order breaking ties between equal codes.  The tree is never stored: the
//                      collapse walks it from the root and asks for the split of a range where it needs one (rebuild_find_split — the split Karras's construction gives the
//                      node with that range; one lane per wide node, no lane waits for another)
//   6. collapse        rebuild_node_slots: a wide node takes the grandchildren of its binary node; a binary subtree of at most four entries is ONE leaf slot; a slot that is
//                      left free goes to the inner slot with the most entries under it (the lower slot on a tie), which is replaced by its two binary children; slots stay in
//                      key order.  Every inner slot lies at least two binary levels below its node, so the depth is about half the binary depth.  Counts and ranges only — no
//                      floating point — so host and device cannot disagree
//   7. layout          level by level from the root; per level an exclusive scan over the level's nodes hands out the node numbers of the inner children and the entry
//                      positions of the leaf children, so that the inner children of a node are consecutive nodes, the entries of its leaf children consecutive entries, both
//                      in slot order (what flat4_node::links spells), and level l is an index range.  No atomic decides a position
//   8. nodes           rebuild_encode_node: mask and link words as flat4_encode_links (flatten.h) and patch_empty_slots_q4 (flatten.cpp) make them; no node carries an
//                      oriented slab: the last 16 B are zero, every slab flag is 0
//   9. boxes           refit_node_boxes, deepest level first
// Stage 5 is the LBVH builder (CTL_REBUILD_LBVH).  The PLOC builder (CTL_REBUILD_PLOC, flat_ploc.h) replaces it by a stored binary tree made bottom-up from the boxes in the
// same sorted order; stages 6 and 7 are written over "a binary tree" (rebuild_lbvh_tree here, ploc_tree there) and do not know which one they walk.
#pragma once
#include "flat_refit.h"
#include "../../include/ctl_amd.h"
#include <cstddef>
#include <stdexcept>
#include <utility>
#include <vector>

namespace ctl {

constexpr uint64_t kRebuildMaxCode = 0x7fffffffffffffffull;
#ifndef CTL_REBUILD_LEAF_MAX
#define CTL_REBUILD_LEAF_MAX 4   // a variant build may set 1 .. 4 (EXPERIMENTS.md); a leaf slot of the Q4 format holds at most four entries
#endif
constexpr uint32_t kRebuildLeafMax = CTL_REBUILD_LEAF_MAX;   // a binary subtree of at most this many entries becomes one leaf slot
static_assert(kRebuildLeafMax >= 1 && kRebuildLeafMax <= 4, "a Q4 leaf slot holds 1 .. 4 entries");
constexpr uint32_t kRebuildLastBit = 0x80000000u;   // in the permutation word of a new entry position: the entry closes its leaf

// floats as integers in the floats' order (-0 below +0): min / max over them are exact and the same whatever the order of the reduction
CTL_REFIT_HD uint32_t rebuild_ord(float f) { const uint32_t b = refit_f2u(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
CTL_REFIT_HD float rebuild_unord(uint32_t o) { return refit_u2f((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }
CTL_REFIT_HD bool rebuild_box_valid(const refit_box& b) { return b.lo[0] <= b.hi[0] && b.lo[1] <= b.hi[1] && b.lo[2] <= b.hi[2]; }

CTL_REFIT_HD uint64_t rebuild_spread21(uint32_t v) {   // bit i -> bit 3 i
    uint64_t x = v & 0x1fffffu;
    x = (x | (x << 32)) & 0x001f00000000ffffull;
    x = (x | (x << 16)) & 0x001f0000ff0000ffull;
    x = (x | (x << 8)) & 0x100f00f00f00f00full;
    x = (x | (x << 4)) & 0x10c30c30c30c30c3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}
// bounds: lo = the smallest low corner, hi = the largest high corner of the valid boxes
CTL_REFIT_HD uint64_t rebuild_key(const refit_box& b, const refit_box& bounds) {
    if (!rebuild_box_valid(b)) return kRebuildMaxCode;
    uint64_t code = 0;
    for (int k = 0; k < 3; k++) {
        const double c = (double)b.lo[k] + (double)b.hi[k], o = 2.0 * (double)bounds.lo[k], ext = 2.0 * ((double)bounds.hi[k] - (double)bounds.lo[k]);
        uint32_t q = 0u;
        if (ext > 0.0) {
            const double t = (c - o) / ext * 2097152.0;
            if (t >= 2097151.0) q = 2097151u; else if (t >= 0.0) q = (uint32_t)t;   // (a NaN gives 0)
        }
        code |= rebuild_spread21(q) << (2 - k);
    }
    return code;
}

CTL_REFIT_HD int rebuild_clz64(uint64_t x) {
    if (!x) return 64;
    int n = 0;
    if (!(x >> 32)) { n += 32; x <<= 32; }
    if (!(x >> 48)) { n += 16; x <<= 16; }
    if (!(x >> 56)) { n += 8; x <<= 8; }
    if (!(x >> 60)) { n += 4; x <<= 4; }
    if (!(x >> 62)) { n += 2; x <<= 2; }
    if (!(x >> 63)) n += 1;
    return n;
}
// length of the common prefix of (key, position) at the sorted positions i and j
CTL_REFIT_HD int rebuild_delta(const uint64_t* keys, uint32_t i, uint32_t j) {
    const uint64_t a = keys[i], b = keys[j];
    return a != b ? rebuild_clz64(a ^ b) : 64 + rebuild_clz64((uint64_t)(i ^ j));
}
// the binary node over the sorted positions first .. last (first < last) has the children first .. split and split + 1 .. last
CTL_REFIT_HD uint32_t rebuild_find_split(const uint64_t* keys, uint32_t first, uint32_t last) {
    const int common = rebuild_delta(keys, first, last);
    uint32_t split = first, step = last - first;
    do {
        step = (step + 1u) >> 1;
        const uint32_t s = split + step;
        if (s < last && rebuild_delta(keys, first, s) > common) split = s;
    } while (step > 1u);
    return split;
}

// the binary tree the collapse walks, as the LBVH supplies it: a binary node is its range first .. last of sorted positions, its split comes from rebuild_find_split, its
// entries are the positions themselves.  (flat_ploc.h has the stored tree of the PLOC builder behind the same three functions.)
struct rebuild_lbvh_tree {
    const uint64_t* keys;
    CTL_REFIT_HD void split(uint32_t first, uint32_t last, uint32_t& lf, uint32_t& ll, uint32_t& rf, uint32_t& rl) const { const uint32_t s = rebuild_find_split(keys, first, last); lf = first; ll = s; rf = s + 1u; rl = last; }
    CTL_REFIT_HD uint32_t entry(uint32_t first, uint32_t last, uint32_t e) const { (void)last; return first + e; }   // the sorted position of the e-th entry under the node
    CTL_REFIT_HD uint32_t root_first(uint32_t n) const { (void)n; return 0u; }
};

// the slots of a wide node: binary nodes in left-before-right order, each with its entry count (last - first + 1; what `first` names is the tree's business: a sorted
// position for the LBVH, a node id for a stored tree); a binary node of at most four (kRebuildLeafMax) entries is a leaf slot, any other an inner child
struct rebuild_slots {
    uint32_t n, first[4], last[4];
    CTL_REFIT_HD uint32_t count(uint32_t k) const { return last[k] - first[k] + 1u; }
    CTL_REFIT_HD bool leaf(uint32_t k) const { return count(k) <= kRebuildLeafMax; }
};
template <typename Tree> CTL_REFIT_HD void rebuild_split_slot(const Tree& T, rebuild_slots& S, uint32_t k) {
    for (uint32_t j = S.n; j > k + 1u; j--) { S.first[j] = S.first[j - 1u]; S.last[j] = S.last[j - 1u]; }
    uint32_t lf, ll, rf, rl; T.split(S.first[k], S.last[k], lf, ll, rf, rl);
    S.first[k + 1u] = rf; S.last[k + 1u] = rl; S.first[k] = lf; S.last[k] = ll; S.n++;
}
template <typename Tree> CTL_REFIT_HD void rebuild_node_slots(const Tree& T, uint32_t a, uint32_t b, rebuild_slots& S) {
    S.n = 1u; S.first[0] = a; S.last[0] = b;
    for (int k = 1; k < 4; k++) { S.first[k] = 0u; S.last[k] = 0u; }
    if (S.leaf(0)) return;   // only the root of a tree of at most four entries: one leaf slot
    rebuild_split_slot(T, S, 0u);                      // the binary node's children ...
    if (!S.leaf(1)) rebuild_split_slot(T, S, 1u);      // ... and its grandchildren
    if (!S.leaf(0)) rebuild_split_slot(T, S, 0u);
    while (S.n < 4u) {   // a free slot goes to the inner slot with the most entries, the lower one on a tie
        uint32_t best = 4u, most = kRebuildLeafMax;
        for (uint32_t k = 0; k < S.n; k++) if (S.count(k) > most) { most = S.count(k); best = k; }
        if (best == 4u) break;
        rebuild_split_slot(T, S, best);
    }
}
// inner children and entries of leaf children of a node, packed for ONE scan per level: inner children << 32 | entries
CTL_REFIT_HD uint64_t rebuild_slot_counts(const rebuild_slots& S) {
    uint64_t c = 0;
    for (uint32_t k = 0; k < S.n; k++) c += S.leaf(k) ? (uint64_t)S.count(k) : (1ull << 32);
    return c;
}
// the 16 words of the node: its inner children are the nodes first_child .., the entries of its leaf children the entries first_entry .., both in slot order.  Boxes
// (words 0..2, the exponents, words 4..9) are left to refit_node_boxes, which keeps the mask byte
CTL_REFIT_HD void rebuild_encode_node(const rebuild_slots& S, uint32_t first_child, uint32_t first_entry, uint32_t words[16]) {
    for (int i = 0; i < 16; i++) words[i] = 0u;
    uint32_t mask = 0u, t[4] = { 0u, 0u, 0u, 0u }, ni = 0u, nl = 0u;
    for (uint32_t k = 0; k < S.n; k++) {
        mask |= 1u << k;
        if (S.leaf(k)) { mask |= 16u << k; t[k] = 15u - nl; nl += S.count(k); }
        else { t[k] = ni << 2; ni++; }
    }
    if (ni == 0u) for (uint32_t k = S.n; k < 4u; k++) { mask |= 16u << k; t[k] = 15u; }   // empty slots of a node without inner children lead to its first entry (patch_empty_slots_q4)
    const uint32_t inner_base4 = ni ? first_child * 4u : 0u, leaf_base = nl ? first_entry : 0u;
    words[3] = mask << 24;
    words[10] = inner_base4 | (t[1] << 26) | ((t[3] & 3u) << 30);
    words[11] = (t[3] >> 2) | (t[2] << 2) | ((~(leaf_base + 15u)) << 6);
}

// flat_rebuild.cpp.  rebuild_refuse: what both sides refuse before anything is written (unsupported_error).  rebuild_flat_scene: refit_flat_scene to `d`, then the rebuild;
// a rebuilt tree that is too deep for the traversal stack is refused with the tree left refitted.  area_before_after (may be null): the refitted and the rebuilt tree's.
// builder: CTL_REBUILD_LBVH or CTL_REBUILD_PLOC (flat_ploc.h); the callers have refused any other value
struct flat_scene;
void rebuild_refuse(int format, bool refit_ready, bool compact, size_t n_entries, const char* who);
void rebuild_flat_scene(flat_scene& F, const ctl_scene_desc& d, double* area_before_after, int builder = CTL_REBUILD_LBVH);
// stages 1 - 9 alone, over the entries F holds (leaves, refit.part_index / part_boxes / xf0) for the transforms of `d`: what rebuild_flat_scene runs after its refit, and
// update_nodes_flat_scene (flat_nodes.cpp) over another set of entries.  Too deep a tree: unsupported_error before F is written
void rebuild_flat_entries(flat_scene& F, const ctl_scene_desc& d, int builder = CTL_REBUILD_LBVH);
// stages 1 - 4 alone, nothing written: the entries' boxes for the transforms of `d`, their bounds, and (code, entry) in sorted order (ctl_flat_bvh_rebuild_order)
void rebuild_sorted_entries(const flat_scene& F, const ctl_scene_desc& d, std::vector<refit_box>& ebox, refit_box& bounds, std::vector<std::pair<uint64_t, uint32_t>>& order);
// a state of the rebuild that its own arithmetic rules out (a clustering round without a merge): CTL_ERR_INTERNAL
struct internal_error : std::runtime_error { using std::runtime_error::runtime_error; };
// The builder of the device calls, per thread: CTL_REBUILD_LBVH unless the C entry point holds a rebuild_builder_scope around the call.  It is read in exactly two
// places, on the thread of the C call: where Scene::rebuild_flat and Scene::update_nodes make their flat_rebuilder (B.builder = rebuild_builder_choice()) — the members
// keep their signatures, flat_rebuilder itself takes the builder as a plain field.  rebuild_last_rounds: the clustering rounds of this thread's last rebuild call, host
// or device; every call sets it to 0 when it starts, so a refused call and the LBVH leave 0
int& rebuild_builder_choice();
uint32_t& rebuild_last_rounds();
struct rebuild_builder_scope {
    int prev;
    explicit rebuild_builder_scope(int b) : prev(rebuild_builder_choice()) { rebuild_builder_choice() = b; }
    ~rebuild_builder_scope() { rebuild_builder_choice() = prev; }
    rebuild_builder_scope(const rebuild_builder_scope&) = delete; rebuild_builder_scope& operator=(const rebuild_builder_scope&) = delete;
};

}  // namespace ctl
