// flat_ploc.h — the second builder of the rebuild (flat_rebuild.h): PLOC, parallel locally-ordered clustering (Meister & Bittner 2018), single source for the host
// (flat_rebuild.cpp) and the device (flat_rebuild.hip).  The LBVH takes its binary tree from the Morton codes alone; PLOC keeps the sorted ORDER of stages 1 - 4 and
// builds the binary tree bottom-up from the boxes, so that what is merged is what is close, not what shares a code prefix.  Stages 5 - 7 of flat_rebuild.h become:
//   5. clustering   the clusters start as the sorted entries: binary node id = sorted position, box = the entry's box (an inverted box — the largest code, sorted last —
//                   clusters as the point bounds.hi; the node boxes come from the refit kernels as ever, so nothing else changes for it).  One round:
//                     nearest   cluster i looks at the clusters up to kPlocRadius positions to either side and picks the one whose union box with its own has the smallest
//                               surface area (ploc_union_area: fp32, one expression order, no contraction); on equal areas the partner with the smaller
//                               i XOR j wins (see Progress)
//                     merge     clusters that picked each other merge; the pair's lower position keeps the merged cluster, the higher one is removed
//                     compact   an exclusive scan over (merge flag << 32 | survivor flag) hands out the rank of a merge among the round's merges and the new position of a
//                               survivor (order kept): the new inner node is n + merges of earlier rounds + rank.  No atomic decides an id or a position
//                   per inner node: left child (the cluster that had the lower position), right child, entry count.  n - 1 merges make the tree; its root is 2 n - 2.
//                   Progress: a cluster picks the candidate with the smallest (area, i XOR j).  Both parts are symmetric in the pair, and for one i the XOR differs
//                   from candidate to candidate, so a pair that is smallest by (area, XOR) among ALL pairs of the round is the single smallest among the candidates of
//                   both its ends: they pick each other, and every round merges at least one pair.  Why XOR and not simply the lower position: a run of k EQUAL boxes
//                   (instances under one transform; the entries without a box, which all cluster as one point) ties everywhere, "the lower position" then makes every
//                   cluster of the run point down the run, only its first two pick each other, and the run takes k - 1 rounds — past the round cap for a few hundred
//                   collapsed triangles.  With the XOR the neighbours 2 j, 2 j + 1 pick each other all along the run: it halves every round.
//                   The loop nevertheless stops by two checks of its host side: a round without a merge is internal_error (areas that are no numbers — overflowed extents — can do it: a first candidate with such an area is kept), more
//                   than ploc_round_cap(n) rounds unsupported_error (a chain of one merge per round must not become minutes of launches); the tree that was there stays
//   6. collapse     rebuild_node_slots over ploc_tree: a slot is a binary node with its entry count, its split its two stored children.  The same rules, integers only
//   7. layout       as for the LBVH; the entries of a leaf slot are its subtree's entries from left to right (ploc_tree::entry: at most four, at most three levels down)
#pragma once
#include "flat_rebuild.h"

namespace ctl {

#ifndef CTL_PLOC_RADIUS
#define CTL_PLOC_RADIUS 8   // a variant build may set another search radius (EXPERIMENTS.md)
#endif
constexpr uint32_t kPlocRadius = CTL_PLOC_RADIUS;
static_assert(kPlocRadius >= 1 && kPlocRadius <= 64, "the search window is staged in LDS");

// the box an entry clusters with
CTL_REFIT_HD refit_box ploc_cluster_box(const refit_box& b, const refit_box& bounds) {
    if (rebuild_box_valid(b)) return b;
    refit_box p;
    for (int k = 0; k < 3; k++) { p.lo[k] = bounds.hi[k]; p.hi[k] = bounds.hi[k]; }
    return p;
}
CTL_REFIT_HD refit_box ploc_union(const refit_box& a, const refit_box& b) {
    refit_box u;
    for (int k = 0; k < 3; k++) { u.lo[k] = refit_min(a.lo[k], b.lo[k]); u.hi[k] = refit_max(a.hi[k], b.hi[k]); }
    return u;
}
// half the surface area of the union box: the distance of two clusters.  Symmetric in value; (dx dy + dy dz) + dz dx, each operation rounded on its own
CTL_REFIT_HD float ploc_union_area(const refit_box& a, const refit_box& b) {
    const float dx = refit_max(a.hi[0], b.hi[0]) - refit_min(a.lo[0], b.lo[0]);
    const float dy = refit_max(a.hi[1], b.hi[1]) - refit_min(a.lo[1], b.lo[1]);
    const float dz = refit_max(a.hi[2], b.hi[2]) - refit_min(a.lo[2], b.lo[2]);
    const float xy = dx * dy, yz = dy * dz, zx = dz * dx;
    const float s = xy + yz;
    return s + zx;
}
// the position cluster i of m picks (i itself only when m == 1).  box(j): the box of the cluster at position j, 0 <= j < m.  The first candidate is taken whatever its
// area, a later one when strictly smaller, or equal with the smaller i XOR j.  An area that is no number never wins as a LATER candidate and, as the first one, stays
// (no comparison with it holds): deterministic on both sides, outside the progress argument, and what the host-side stop is for
template <typename Box> CTL_REFIT_HD uint32_t ploc_nearest(const Box& box, uint32_t m, uint32_t i) {
    const refit_box a = box(i);
    const uint32_t j0 = i > kPlocRadius ? i - kPlocRadius : 0u, j1 = (m - 1u - i > kPlocRadius) ? i + kPlocRadius : m - 1u;
    uint32_t best = i; float best_area = 0.0f;
    for (uint32_t j = j0; j <= j1; j++) {
        if (j == i) continue;
        const float s = ploc_union_area(a, box(j));
        if (best == i || s < best_area || (s == best_area && (i ^ j) < (i ^ best))) { best = j; best_area = s; }
    }
    return best;
}
// what the round does to cluster i: merge flag << 32 | survivor flag (the word the round's scan sums)
CTL_REFIT_HD uint64_t ploc_round_flags(const uint32_t* nn, uint32_t m, uint32_t i) {
    const uint32_t p = nn[i];
    if (p == i || p >= m || nn[p] != i) return 1ull;   // not in a pair: survives as it is
    return i < p ? ((1ull << 32) | 1ull) : 0ull;       // the lower position keeps the merged cluster, the higher one is removed
}
// rounds after which the clustering is refused: 8 ceil(log2 n) + 16 (about 2.5 log2 n are needed on scenes)
CTL_REFIT_HD uint32_t ploc_round_cap(uint32_t n) {
    uint32_t bits = 0u;
    while (bits < 32u && (1ull << bits) < (uint64_t)n) bits++;
    return 8u * bits + 16u;
}

// the stored binary tree over n entries: ids 0 .. n - 1 are the sorted positions, n + j is the j-th inner node made.  As a slot of rebuild_slots a binary node is
// first = its id, last = id + entry count - 1
struct ploc_tree {
    uint32_t n; const uint32_t *left, *right, *count;   // per inner node j = id - n
    CTL_REFIT_HD uint32_t entries(uint32_t id) const { return id < n ? 1u : count[id - n]; }
    CTL_REFIT_HD void split(uint32_t first, uint32_t last, uint32_t& lf, uint32_t& ll, uint32_t& rf, uint32_t& rl) const {
        (void)last;
        lf = left[first - n]; ll = lf + entries(lf) - 1u; rf = right[first - n]; rl = rf + entries(rf) - 1u;
    }
    CTL_REFIT_HD uint32_t entry(uint32_t first, uint32_t last, uint32_t e) const {   // the sorted position of the e-th entry under the node, from the left
        (void)last;
        uint32_t id = first;
        while (id >= n) {
            const uint32_t l = left[id - n], c = entries(l);
            if (e < c) id = l; else { e -= c; id = right[id - n]; }
        }
        return id;
    }
    CTL_REFIT_HD uint32_t root_first(uint32_t n_) const { return n_ > 1u ? 2u * n_ - 2u : 0u; }
};

}  // namespace ctl
