// flatten.cpp — optional re-layout at scene upload: ONE world-space BVH over all instanced triangles ("flattening
// static instances into one BVH is allowed by the API and likely necessary").  The MI355X has 288 GB of HBM: 128 B per instanced
// triangle buys a traversal that never restarts at a mesh root per instance and has two instead of four kinds of work per wave.
// The tree only culls: a leaf entry keeps the mesh's own object-space Woop rows, its node id and the node's inverse transform, and the
// kernel evaluates it with the reference's instance-transform + Woop arithmetic, so (t, u, v, triangle, node) equal the two-level traversal bit for bit
// (flatten.h).  World-space vertices are recovered from the Woop rows in double only to compute the boxes, which are padded.
#include "flatten.h"
#include "knobs.h"
#include "flat_slab.h"
#include "bvh_builder.h"
#include "scene_cache.h"
#include "mitsuba_loader.h"   // unsupported_error
#include <cmath>
#include <cstring>
#include <algorithm>
#include <stdexcept>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

namespace ctl {

namespace {

// builder settings of the world-space BVH; the environment overrides are measurement knobs (tools/flat_build_probe.sh).  SAH node cost 0.5:
// a 4-wide node covers two levels of the binary tree in one fetch + one loop iteration, a leaf entry costs one of each per triangle.
// Measured on synthetic-SM: node cost 1 -> 34.0 nodes + 8.45 triangles per ray, 0.5 -> 35.3 + 6.28 and +1 % rays/s; leaf size 2 / 4 / 8: no difference
int flat_max_leaf() { static const int v = [] { const char* e = knob_env("CTL_FLAT_MAX_LEAF"); const int x = e ? atoi(e) : 0; return x >= 1 && x <= 16 ? x : 4; }(); return v; }
// collapse of the binary tree into 4-wide nodes: 1 = SAH-optimal dynamic programme (bvh_builder.h), 0 = greedy; its node cost is in leaf-entry tests:
// k_intersect spends ~277 lane-slots on a node step and ~365 on a leaf-entry step at its measured lane utilisation
int flat_collapse_mode() { static const int v = [] { const char* e = knob_env("CTL_FLAT_COLLAPSE"); return e ? atoi(e) : 0; }(); return v; }
float flat_collapse_node_cost() { static const float v = [] { const char* e = knob_env("CTL_FLAT_COLLAPSE_NODE_COST"); const float x = e ? (float)atof(e) : 0.0f; return x > 0.0f ? x : 0.75f; }(); return v; }
// early split clipping (flatten_scene): longest side a triangle reference may have, in medians of the scene's triangle boxes (0 = off); $CTL_FLAT_SPLIT
float flat_split_ratio() { static const float v = [] { const char* e = knob_env("CTL_FLAT_SPLIT"); const float x = e ? (float)atof(e) : -1.0f; return x >= 0.0f ? x : 4.0f; }(); return v; }   // with the gain rule below, on the GPU (profiles/r04_split_clipping.log): 4: synthetic-sm-hard 3381 Mrays/s (no clipping: 1383), 8: 3316, 16: 3203; synthetic-SM and -bathroom unchanged
// ... and a split is kept only where the two parts' boxes have less than this fraction of the part's box surface (1 = always); $CTL_FLAT_SPLIT_GAIN
float flat_split_gain() { static const float v = [] { const char* e = knob_env("CTL_FLAT_SPLIT_GAIN"); const float x = e ? (float)atof(e) : -1.0f; return x > 0.0f ? x : 0.65f; }(); return v; }   // 0.6 .. 0.7 equal; 0.8 .. 1.0 also split axis-aligned floors and walls: synthetic-SM - 7 %, synthetic-sm-hard 2800 .. 2960
// insertion-based re-optimisation of the BVH2 before the collapse (bvh_builder.cpp reinserter): passes, and the share of the nodes (largest first) a pass visits
int flat_reinsert_passes() { static const int v = [] { const char* e = knob_env("CTL_FLAT_REINSERT"); const int x = e ? atoi(e) : -1; return x >= 0 && x <= 64 ? x : 16; }(); return v; }
float flat_reinsert_fraction() { static const float v = [] { const char* e = knob_env("CTL_FLAT_REINSERT_FRACTION"); const float x = e ? (float)atof(e) : 0.0f; return x > 0.0f && x <= 1.0f ? x : 0.03f; }(); return v; }
int flat_slot_order() { static const int v = [] { const char* e = knob_env("CTL_FLAT_SLOT_ORDER"); const int x = e ? atoi(e) : -1; return x >= 0 && x <= 2 ? x : 0; }(); return v; }
float flat_node_cost() { static const float v = [] { const char* e = knob_env("CTL_FLAT_NODE_COST"); const float x = e ? (float)atof(e) : 0.0f; return x > 0.0f ? x : 0.5f; }(); return v; }

// 4x4 inverse in double (cofactor expansion)
bool inv4(const double m[16], double out[16]) {
    double inv[16];
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    if (det == 0.0 || !std::isfinite(det)) return false;
    const double id = 1.0 / det;
    for (int i = 0; i < 16; i++) out[i] = inv[i] * id;
    return true;
}

// vertices of a Woop triangle (TriIntersectorData::getData, Engine/TriIntersectorData.cu:20-32) in double
bool woop_vertices(const ctl_woop_tri& w, double v[3][3]) {
    const double m[16] = { w.b[0], w.b[1], w.b[2], w.b[3], w.c[0], w.c[1], w.c[2], w.c[3], w.a[0], w.a[1], w.a[2], -(double)w.a[3], 0, 0, 0, 1 };
    double inv[16];
    if (!inv4(m, inv)) return false;
    for (int k = 0; k < 3; k++) { v[2][k] = inv[k * 4 + 3]; v[0][k] = v[2][k] + inv[k * 4 + 0]; v[1][k] = v[2][k] + inv[k * 4 + 1]; }
    return true;
}
// world-space length that one unit of object-space round-off of this triangle can reach: its largest object-space coordinate times the
// largest row sum of the instance's linear part
double woop_slack(const double v[3][3], const float* M) {
    double m = 0; for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) m = std::max(m, std::fabs(v[j][k]));
    double rs = 0; for (int r = 0; r < 3; r++) rs = std::max(rs, std::fabs((double)M[r * 4]) + std::fabs((double)M[r * 4 + 1]) + std::fabs((double)M[r * 4 + 2]));
    return m * rs;
}
// phase timing on stderr when CTL_VERBOSE is set
struct phase_timer {
    const bool on = std::getenv("CTL_VERBOSE") != nullptr; std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char* what) { if (!on) return; const auto n = std::chrono::steady_clock::now(); std::fprintf(stderr, "[ctl flatten] %-18s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count()); t = n; }
};
// static split of [0, n) over the host threads
template <typename F> void parallel_for(size_t n, const F& f, size_t min_chunk = 4096) {
    const size_t nt = std::min<size_t>(std::min(64u, std::max(1u, std::thread::hardware_concurrency())), std::max<size_t>(1, n / min_chunk));
    if (nt <= 1) { f(0, n); return; }
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; t++) th.emplace_back([&, t]() { f(n * t / nt, n * (t + 1) / nt); });
    for (auto& x : th) x.join();
}
// knobs that are part of the cache key as the environment spells them (flat_cache_key) and clamped where they are used
long flat_bfs_top() { static const long v = [] { const char* e = knob_env("CTL_FLAT_BFS_TOP"); return e ? atol(e) : 65536L; }(); return v; }
int flat_slab_subtree() { static const int v = [] { const char* e = knob_env("CTL_FLAT_SLAB_SUBTREE"); return e ? atoi(e) : kSlabSubtreeDefault; }(); return v; }
double flat_slab_useful() { static const double v = [] { const char* e = knob_env("CTL_FLAT_SLAB_USEFUL"); return e ? atof(e) : 0.6; }(); return v; }
int flat_force_explicit() { static const int v = [] { const char* e = knob_env("CTL_FLAT_FORCE_EXPLICIT"); return e ? atoi(e) : 0; }(); return v; }

// child links and leaf ranges of a tree read back from the cache: every link must land inside the arrays before they reach the GPU
bool flat_links_valid(const flat_scene& F) {
    const size_t nl = F.leaves.size();
    auto ok = [&](int32_t c, size_t n_nodes, int unit) {
        if (c == 0x76543210) return true;
        if (c >= 0) return c % unit == 0 && (size_t)(c / unit) < n_nodes;
        return (size_t)(~c) < nl;
    };
    if (F.format == kFlatQ4) {
        if (F.child_links.size() != F.nodes.size() * 4) return false;
        for (size_t i = 0; i < F.nodes.size(); i++) {
            const flat4_node& n = F.nodes[i];
            int32_t imp[4]; if (F.compact_links) flat4_implied_links(n, imp);
            for (int c = 0; c < 4; c++) {
                const int32_t k = F.child_links[i * 4 + c];
                if (((n.mask >> c) & 1) && !ok(k, F.nodes.size(), 4)) return false;
                // the kernels follow the IMPLIED links (and the slab flag they carry) when the tree is compact: they must be the explicit ones
                if (F.compact_links && ((n.mask >> c) & 1) && (imp[c] & ~(k >= 0 ? 1 : 0)) != k) return false;
                if (!F.compact_links && ((n.mask >> c) & 1) && n.child[c] != k) return false;
                // a slot without a child repeats the link of one that exists (patch_empty_slots_q4): a link the kernels may follow, so it is checked like the others
                if (!((n.mask >> c) & 1)) {
                    const int32_t mine = F.compact_links ? imp[c] : n.child[c]; bool found = false;
                    for (int e = 0; e < 4; e++) if ((n.mask >> e) & 1) { const int32_t theirs = F.compact_links ? imp[e] : n.child[e]; if (mine == theirs || (mine >= 0 && theirs >= 0 && (mine & ~3) == (theirs & ~3))) found = true; }
                    if (!found && (n.mask & 15)) return false;
                }
            }
        }
    }
    else if (F.format == kFlatQ8) {
        // every link the kernels derive (flat8.h) must land inside the arrays, and must be the explicit one host code sees
        if (F.child_links.size() != F.nodes_q8.size() * 8 || F.nodes_q8.size() >= kFlat8MaxNodes) return false;
        for (size_t i = 0; i < F.nodes_q8.size(); i++) {
            const flat8_node& n = F.nodes_q8[i];
            const uint32_t q0w = (uint32_t)n.e[0] | ((uint32_t)n.e[1] << 8) | ((uint32_t)n.e[2] << 16) | ((uint32_t)n.imask << 24);
            const uint32_t im = flat8_inner_mask(q0w), lm = flat8_leaf_mask(q0w, n.base_b);
            for (uint32_t s = 0; s < 8; s++) {
                const int32_t k = F.child_links[i * 8 + s];
                if ((im >> s) & 1u) { const uint32_t c = flat8_child_node(n.base_b, im, s); if (c >= F.nodes_q8.size() || k != (int32_t)c) return false; }
                else if ((lm >> s) & 1u) { const uint32_t e = flat8_leaf_entry(n.leaf_base, lm, s); if (e >= nl || k != ~(int32_t)e || !(F.leaves[e].index & 1u)) return false; }
                else if (k != (int32_t)kFlat8None) return false;
            }
            // an empty slot that round-off lets through is read as entry leaf_base + rank: one past the node's own entries at most, which must exist (the upload appends a closing entry)
            if ((size_t)n.leaf_base + flat8_popc(lm) > nl) return false;
        }
    }
    else return false;
    if (F.node_bytes() == 0) return false;
    return nl > 0 && (F.leaves[nl - 1].index & 1u);   // the last entry closes its leaf
}
struct slab_ctri { double w[3][3]; double slack; int c; };   // a triangle under child c of the node whose slab is being chosen
float round_down(double x) { float f = (float)x; return ((double)f > x) ? std::nextafterf(f, -INFINITY) : f; }
float round_up(double x) { float f = (float)x; return ((double)f < x) ? std::nextafterf(f, INFINITY) : f; }
// the part of the refit side data (flat_refit.h) that the tree and the description give: the nodes by depth and the transforms the tree was built for
void finish_refit_side(flat_scene& F, const ctl_scene_desc& d) {
    F.refit.level_start.clear(); F.refit.level_nodes.clear(); F.refit.xf0.clear();
    if (F.format != kFlatQ4 || F.nodes.empty()) return;
    F.refit.xf0.assign(d.node_transforms, d.node_transforms + d.n_nodes);
    std::vector<uint32_t> depth(F.nodes.size(), 0u), count;
    for (size_t i = 0; i < F.nodes.size(); i++) {   // children come later in memory than their parent
        if (depth[i] >= count.size()) count.resize(depth[i] + 1, 0u);
        count[depth[i]]++;
        for (int c = 0; c < 4; c++) { const int32_t k = F.child_links[i * 4 + c]; if (((F.nodes[i].mask >> c) & 1) && k >= 0 && k != 0x76543210) depth[(size_t)k / 4] = depth[i] + 1; }
    }
    F.refit.level_start.assign(count.size() + 1, 0u);
    for (size_t l = 0; l < count.size(); l++) F.refit.level_start[l + 1] = F.refit.level_start[l] + count[l];
    F.refit.level_nodes.resize(F.nodes.size());
    std::vector<uint32_t> fill(F.refit.level_start.begin(), F.refit.level_start.end() - 1);
    for (size_t i = 0; i < F.nodes.size(); i++) F.refit.level_nodes[fill[depth[i]]++] = (uint32_t)i;
}

// ---- the stages of flatten_scene, in the order it runs them ----

// object -> world of a triangle's vertices in double (M: the instancing node's row-major 4 x 4)
void world_vertices(const float* M, const double v[3][3], double w[3][3]) {
    for (int j = 0; j < 3; j++) for (int r = 0; r < 3; r++) w[j][r] = (double)M[r * 4] * v[j][0] + (double)M[r * 4 + 1] * v[j][1] + (double)M[r * 4 + 2] * v[j][2] + (double)M[r * 4 + 3];
}
// The kernel decides a hit with the fp32 object-space Woop test, whose accepted region differs from the exact triangle by round-off: a reference's box is padded on axis r
// by 8 ulp of the largest coordinate (and of the extent) of the WHOLE triangle's box b — and of `off`, the triangle's OBJECT-space magnitude carried through the instance
// transform (woop_slack: a mesh far from its own origin, a strongly scaled instance: the round-off of the object-space test scales with those, not with the world box)
float woop_pad(const aabb& b, int r, float off) {
    const float mag = std::max(std::max(std::max(std::fabs(b.lo[r]), std::fabs(b.hi[r])), b.hi[r] - b.lo[r]), off);
    return mag * 9.5367431640625e-7f + 1e-30f;   // 8 ulp
}

// per mesh its unique triangles as (mesh-local triangle id, entry of the shared woop stream), sorted by id
typedef std::vector<std::vector<std::pair<uint32_t, uint32_t>>> mesh_triangles;
// the triangles of every instanced mesh (spatial splits reference a triangle from several leaves of the mesh's own BVH: each is taken once) -> the number of instanced triangles
size_t unique_mesh_triangles(const ctl_scene_desc& d, mesh_triangles& mesh_tris) {
    // leaf-entry range of every mesh (the woop stream is shared; a mesh ends where the next one starts)
    std::vector<std::pair<uint32_t, uint32_t>> starts;
    for (uint32_t m = 0; m < d.n_meshes; m++) starts.emplace_back(d.meshes[m].bvh_tri_offset / 3, m);
    std::sort(starts.begin(), starts.end());
    std::vector<uint32_t> mesh_first(d.n_meshes), mesh_last(d.n_meshes);
    for (size_t r = 0; r < starts.size(); r++) { mesh_first[starts[r].second] = starts[r].first; mesh_last[starts[r].second] = (r + 1 < starts.size()) ? starts[r + 1].first : d.n_woop; }
    mesh_tris.assign(d.n_meshes, {});
    size_t total = 0;
    for (uint32_t k = 0; k < d.n_nodes; k++) {
        const uint32_t m = d.nodes[k].mesh_index;
        if (mesh_tris[m].empty()) {
            auto& v = mesh_tris[m];
            for (uint32_t w = mesh_first[m]; w < mesh_last[m]; w++) v.emplace_back(d.woop_index[d.meshes[m].bvh_index_offset + (w - mesh_first[m])].index >> 1, w);
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first == b.first; }), v.end());
        }
        total += mesh_tris[m].size();
    }
    return total;
}

// what the BVH is built over: one reference per instanced triangle, more for a triangle that early split clipping entered in parts
struct ltri { double v[3][3]; uint32_t tri, woop; };   // a mesh's triangle: object-space vertices, mesh-local id, entry of the woop stream
struct wtri { uint32_t tri, node, woop, local; };      // local: index into mesh_local[mesh of node] (the references of a split triangle share it)
struct references {
    std::vector<std::vector<ltri>> mesh_local;
    std::vector<wtri> tris; std::vector<aabb> boxes;   // per reference: its triangle and its padded world box
    std::vector<uint8_t> is_part;                      // references whose box is the clip box of a part (the refit side data keeps it); empty without split clipping
    size_t split_refs = 0;                             // references added by split clipping
    // world-space vertices of reference g's triangle in double, and the world-space reach of its object-space round-off
    void world(const ctl_scene_desc& d, size_t g, double w[3][3], double& slack) const {
        const wtri& t = tris[g]; const ltri& l = mesh_local[d.nodes[t.node].mesh_index][t.local]; const float* M = d.node_transforms[t.node].m;
        world_vertices(M, l.v, w); slack = woop_slack(l.v, M);
    }
};

// mesh-local vertices in double once per mesh (degenerate triangles can never be hit and are dropped), then the padded world box of every instanced triangle, per node in parallel
bool gather_references(const ctl_scene_desc& d, const mesh_triangles& mesh_tris, references& refs) {
    refs.mesh_local.assign(d.n_meshes, {});
    for (uint32_t m = 0; m < d.n_meshes; m++) {
        refs.mesh_local[m].reserve(mesh_tris[m].size());
        for (auto& e : mesh_tris[m]) { ltri l; l.tri = e.first; l.woop = e.second; if (woop_vertices(d.woop[e.second], l.v)) refs.mesh_local[m].push_back(l); }
    }
    std::vector<size_t> node_first(d.n_nodes + 1, 0);
    for (uint32_t k = 0; k < d.n_nodes; k++) node_first[k + 1] = node_first[k] + refs.mesh_local[d.nodes[k].mesh_index].size();
    refs.tris.resize(node_first[d.n_nodes]); refs.boxes.resize(node_first[d.n_nodes]);
    if (refs.tris.empty()) return false;
    parallel_for(d.n_nodes, [&](size_t k0, size_t k1) {
        for (size_t k = k0; k < k1; k++) {
            const ctl_node& N = d.nodes[k]; const ctl_kernel_mesh& km = d.meshes[N.mesh_index];
            const float* M = d.node_transforms[k].m;
            size_t o = node_first[k];
            for (const ltri& l : refs.mesh_local[N.mesh_index]) {
                wtri& t = refs.tris[o]; t.tri = km.tri_offset + l.tri; t.node = (uint32_t)k; t.woop = l.woop; t.local = (uint32_t)(o - node_first[k]);
                aabb& b = refs.boxes[o]; b.reset(); o++;
                double w[3][3]; world_vertices(M, l.v, w);
                for (int j = 0; j < 3; j++) for (int r = 0; r < 3; r++) { const float lo = round_down(w[j][r]), hi = round_up(w[j][r]); if (lo < b.lo[r]) b.lo[r] = lo; if (hi > b.hi[r]) b.hi[r] = hi; }
                const float off = (float)woop_slack(l.v, M);
                for (int r = 0; r < 3; r++) { const float e = woop_pad(b, r, off); b.lo[r] -= e; b.hi[r] += e; }
            }
        }
    }, 1);
    return true;
}

// a convex polygon (a triangle clipped by axis planes) and its box
struct poly { double p[9][3]; int n; double lo[3], hi[3]; };
// the parts of triangle w inside the cells of a recursive spatial-median subdivision of its box, until no part is longer than lmax (exact polygon clipping in double)
void clip_to_parts(const double w[3][3], double lmax, std::vector<poly>& done) {
    std::vector<poly> todo(1); done.clear();
    poly& P0 = todo[0]; P0.n = 3;
    for (int j = 0; j < 3; j++) for (int r = 0; r < 3; r++) P0.p[j][r] = w[j][r];
    for (int r = 0; r < 3; r++) { P0.lo[r] = std::min(std::min(w[0][r], w[1][r]), w[2][r]); P0.hi[r] = std::max(std::max(w[0][r], w[1][r]), w[2][r]); }
    while (!todo.empty()) {
        poly P = todo.back(); todo.pop_back();
        int ax = 0; for (int r = 1; r < 3; r++) if (P.hi[r] - P.lo[r] > P.hi[ax] - P.lo[ax]) ax = r;
        if (P.hi[ax] - P.lo[ax] <= lmax || P.n > 7 || done.size() + todo.size() >= 16384) { done.push_back(P); continue; }
        const double mid = 0.5 * (P.lo[ax] + P.hi[ax]);
        const size_t todo_before = todo.size();
        for (int side_k = 0; side_k < 2; side_k++) {   // Sutherland-Hodgman against x[ax] <= mid / >= mid
            poly Q; Q.n = 0;
            for (int i = 0; i < P.n; i++) {
                const double* a = P.p[i]; const double* c = P.p[(i + 1) % P.n];
                const bool ia = side_k ? a[ax] >= mid : a[ax] <= mid, ic = side_k ? c[ax] >= mid : c[ax] <= mid;
                if (ia) { for (int r = 0; r < 3; r++) Q.p[Q.n][r] = a[r]; Q.n++; }
                if (ia != ic) { const double u = (mid - a[ax]) / (c[ax] - a[ax]); for (int r = 0; r < 3; r++) Q.p[Q.n][r] = r == ax ? mid : a[r] + u * (c[r] - a[r]); Q.n++; }
            }
            if (Q.n < 3) continue;
            for (int r = 0; r < 3; r++) { Q.lo[r] = Q.hi[r] = Q.p[0][r]; for (int i = 1; i < Q.n; i++) { Q.lo[r] = std::min(Q.lo[r], Q.p[i][r]); Q.hi[r] = std::max(Q.hi[r], Q.p[i][r]); } }
            // the interpolated corners carry round-off of the order of the triangle's size: keep a part's box inside the parent part's box, and widen it by that round-off
            for (int r = 0; r < 3; r++) { const double e = 4e-16 * (std::fabs(P.lo[r]) + std::fabs(P.hi[r]) + (P.hi[r] - P.lo[r])); Q.lo[r] = std::max(P.lo[r], Q.lo[r] - e); Q.hi[r] = std::min(P.hi[r], Q.hi[r] + e); }
            todo.push_back(Q);
        }
        // keep the split only where it removes empty space: the two parts' boxes together must have less than flat_split_gain() x the surface of the part's box.  Halving a
        // beam that crosses its box diagonally quarters each box (sum 0.5); halving an axis-aligned rectangle of a floor removes nothing (sum 1.0) and only adds references
        if (todo.size() == todo_before + 2) {
            auto half_area = [](const poly& B) { const double x = B.hi[0] - B.lo[0], y = B.hi[1] - B.lo[1], z = B.hi[2] - B.lo[2]; return x * y + y * z + z * x; };
            if (half_area(todo[todo_before]) + half_area(todo[todo_before + 1]) >= flat_split_gain() * half_area(P)) { todo.resize(todo_before); done.push_back(P); }
        } else if (todo.size() == todo_before + 1) { todo.resize(todo_before); done.push_back(P); }   // everything on one side of the plane (a sliver): no split
        else if (todo.size() == todo_before) done.push_back(P);
    }
}

// Early split clipping: a triangle much larger than its neighbours (a floor under two thousand instances, a beam across a hall of small triangles) would otherwise sit in a leaf
// near the root whose box every ray crosses.  Such a triangle is entered as several REFERENCES — the same entry, each with the box of one of its parts (clip_to_parts, rounded
// outwards, padded like the whole triangle) — until no reference is longer than flat_split_ratio() x the MEDIAN length of the scene's triangle boxes: the scene's own scale, so
// a beam through fine geometry ends up in finer pieces than a floor under coarse one.  The total is held to + 30 % references by doubling that length.  The traversal tests the
// whole triangle wherever a reference leads it (same hit, same bits; a second encounter of the closest hit does not pass t < t_hit).  Measured with the oracle's counting
// traversal (tools/bvh_quality_probe.py): DESIGN.md §3.
void split_large_references(const ctl_scene_desc& d, references& refs) {
    std::vector<aabb>& boxes = refs.boxes;
    const size_t n0 = boxes.size(), budget = n0 * 3 / 10 + 64;
    auto longest = [](const aabb& b) { return std::max(std::max(b.hi[0] - b.lo[0], b.hi[1] - b.lo[1]), b.hi[2] - b.lo[2]); };
    std::vector<float> ext(n0);
    for (size_t g = 0; g < n0; g++) ext[g] = longest(boxes[g]);
    std::nth_element(ext.begin(), ext.begin() + n0 / 2, ext.end());
    const double median = ext[n0 / 2];
    struct piece { aabb box; uint32_t src; };
    std::vector<piece> extra; std::vector<aabb> first;   // first[i]: the box that replaces boxes[big[i]]
    std::vector<uint32_t> big;
    std::vector<poly> done;
    double side = 0.0;   // longest side of the scene: references are never made shorter than 1 / 4096 of it (a scene whose median triangle is a point)
    { aabb sb; sb.reset(); for (const aabb& b : boxes) for (int r = 0; r < 3; r++) { sb.lo[r] = std::min(sb.lo[r], b.lo[r]); sb.hi[r] = std::max(sb.hi[r], b.hi[r]); } side = longest(sb); }
    for (double lmax = std::max(std::max(median * flat_split_ratio(), side / 4096.0), 1e-30);; lmax *= 2.0) {
        extra.clear(); first.clear(); big.clear();
        bool over = false;
        for (size_t g = 0; g < n0 && !over; g++) {
            const aabb& b = boxes[g];
            if (longest(b) <= lmax) continue;
            double w[3][3], slack; refs.world(d, g, w, slack);
            const float off = (float)slack;
            clip_to_parts(w, lmax, done);
            if (done.size() < 2) continue;
            big.push_back((uint32_t)g);
            for (size_t i = 0; i < done.size(); i++) {
                aabb pb;
                for (int r = 0; r < 3; r++) {
                    pb.lo[r] = round_down(done[i].lo[r]); pb.hi[r] = round_up(done[i].hi[r]);
                    const float e = woop_pad(b, r, off);   // the WHOLE triangle's padding: the test that accepts a hit is the whole triangle's
                    pb.lo[r] = std::max(b.lo[r], pb.lo[r] - e); pb.hi[r] = std::min(b.hi[r], pb.hi[r] + e);
                }
                if (i == 0) first.push_back(pb); else extra.push_back(piece{ pb, (uint32_t)g });
            }
            if (extra.size() > budget) over = true;
        }
        if (!over) break;
    }
    for (size_t i = 0; i < big.size(); i++) boxes[big[i]] = first[i];
    refs.tris.reserve(n0 + extra.size()); boxes.reserve(n0 + extra.size());
    for (const piece& e : extra) { refs.tris.push_back(refs.tris[e.src]); boxes.push_back(e.box); }
    refs.is_part.assign(boxes.size(), 0);
    for (uint32_t g : big) refs.is_part[g] = 1;
    for (size_t g = n0; g < boxes.size(); g++) refs.is_part[g] = 1;
    refs.split_refs = extra.size();
}

inline bool is_inner(int child) { return child >= 0 && child != 0x76543210; }   // a wide node's child: index of a wide node (else ~first leaf entry, or 0x76543210 for none)

// Memory order of the wide nodes: the inner children of a node sit next to each other in slot order, subtrees stay clustered — a ray that enters a node usually enters one or two
// of its children next, and neighbouring lines share DRAM pages / L2 sets.  The first bfs_top nodes (65 536 = 4 MiB of 4-wide nodes, one XCD's L2) breadth-first — the top
// of the tree, which every ray walks, as one contiguous block — and depth-first clusters below that frontier.  Measured on synthetic-SM against the all-depth-first order
// (2164 / 2159 Mrays/s): 4096 nodes 2183, 32 768: 2173, 262 144: 2179, everything breadth-first 2176 (profiles/r02r_node_order_ab.log).
template <typename Node> void memory_order(std::vector<Node>& W, size_t bfs_top) {
    constexpr int width = (int)(sizeof(Node::child) / sizeof(int));   // unused slots of a 4-wide node hold 0x76543210 too (bvh_builder.cpp)
    std::vector<int> new_id(W.size(), -1), order; order.reserve(W.size());
    std::vector<int> stack; new_id[0] = 0; order.push_back(0);
    std::vector<int> frontier; frontier.push_back(0);
    for (size_t head = 0; head < frontier.size() && order.size() < bfs_top; head++) {
        const int me = frontier[head]; frontier[head] = -1;
        for (int c = 0; c < width; c++) if (is_inner(W[me].child[c])) { const int k = W[me].child[c]; new_id[k] = (int)order.size(); order.push_back(k); frontier.push_back(k); }
    }
    for (size_t i = frontier.size(); i-- > 0;) if (frontier[i] >= 0) stack.push_back(frontier[i]);   // not yet expanded, first one on top
    while (!stack.empty()) {
        const int me = stack.back(); stack.pop_back();
        int kids[width], nk = 0;
        for (int c = 0; c < width; c++) if (is_inner(W[me].child[c])) kids[nk++] = W[me].child[c];
        for (int c = 0; c < nk; c++) { new_id[kids[c]] = (int)order.size(); order.push_back(kids[c]); }
        for (int c = nk - 1; c >= 0; c--) stack.push_back(kids[c]);
    }
    std::vector<Node> W2(W.size());
    for (size_t i = 0; i < order.size(); i++) { W2[i] = W[order[i]]; for (int c = 0; c < width; c++) if (is_inner(W2[i].child[c])) W2[i].child[c] = new_id[W2[i].child[c]]; }
    W.swap(W2);
}

// Slot order of the 4-wide nodes.  The closest-hit traversal orders the entered children by distance; the any-hit traversal (shadow rays) takes them in SLOT order, so the slot
// order is its visiting order: 1 = largest box first (the child a random ray most likely meets), 2 = smallest first (measurement), 0 = as the collapse left them
void order_slots(std::vector<wide4_node>& W, int so) {
    if (!so) return;
    for (wide4_node& w : W) {
        int idx[4] = { 0, 1, 2, 3 };
        std::stable_sort(idx, idx + w.n, [&](int a, int b) { const float x = w.cbox[a].area(), y = w.cbox[b].area(); return so == 1 ? x > y : x < y; });
        wide4_node t = w;
        for (int k = 0; k < w.n; k++) { w.cbox[k] = t.cbox[idx[k]]; w.child[k] = t.child[idx[k]]; }
    }
}

// The child boxes of a wide node as 8-bit codes against the node's own box:  lo = origin[k] + 2^(e[k]-127) * lo[k][c],  hi likewise — one exponent per axis, codes rounded
// outwards and conservative under the device's fp32 evaluation origin + step * code (one rounding) too.  A slot without a child (bit c of `exist` clear) gets an INVERTED
// box, lo = 255 / hi = 0 on every axis: whatever the ray, its entry plane lies behind its exit plane (|step / dir| is a normal float >= 2^-126, so 255 steps always differ from
// 0 steps), and the kernels need no "child exists" test per slot.
struct child_codes { float origin[3]; uint8_t e[3]; uint8_t lo[3][8], hi[3][8]; };
void quantise_child_boxes(const aabb& box, const aabb* cbox, int width, uint32_t exist, child_codes& Q) {
    for (int k = 0; k < 3; k++) {
        Q.origin[k] = box.lo[k];
        const double ext = (double)box.hi[k] - (double)box.lo[k];
        int e = 1;   // smallest normal exponent
        if (ext > 0) { int ex; std::frexp(ext / 255.0, &ex); e = ex + 127; /* 2^ex >= ext/255 */ if (e < 1) e = 1; if (e > 254) e = 254; }
        Q.e[k] = (uint8_t)e;
        const double step = std::ldexp(1.0, e - 127);
        for (int c = 0; c < width; c++) {
            long lo = 255, hi = 0;
            if ((exist >> c) & 1u) {
                lo = (long)std::floor(((double)cbox[c].lo[k] - (double)Q.origin[k]) / step);
                hi = (long)std::ceil(((double)cbox[c].hi[k] - (double)Q.origin[k]) / step);
                while (lo > 0 && (float)((double)Q.origin[k] + step * (double)lo) > cbox[c].lo[k]) lo--;
                while (hi < 255 && (float)((double)Q.origin[k] + step * (double)hi) < cbox[c].hi[k]) hi++;
                lo = std::min(255L, std::max(0L, lo)); hi = std::min(255L, std::max(0L, hi));
            }
            Q.lo[k][c] = (uint8_t)lo; Q.hi[k][c] = (uint8_t)hi;
        }
    }
}
inline uint32_t pack4(const uint8_t* b) { return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24); }   // byte c = child c
inline void unpack4(uint32_t w, uint8_t* b) { for (int c = 0; c < 4; c++) b[c] = (uint8_t)(w >> (8 * c)); }

// The Q4 nodes (flatten.h) of the 4-wide tree W, which is in memory order, and the order of the leaf entries: in node order, the leaf children of a node one after the other in
// slot order (flat4_node's implied links).  entry_src: new entry -> position in R.leaf_prims.  Leaves out.child_links as the explicit links of every node.
void encode_q4(const std::vector<wide4_node>& W, const bvh_result& R, flat_scene& out, std::vector<uint32_t>& entry_src) {
    out.nodes.resize(W.size());
    parallel_for(W.size(), [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            const wide4_node& w = W[i]; flat4_node& f = out.nodes[i];
            std::memset(&f, 0, sizeof(f));
            child_codes Q; quantise_child_boxes(w.box, w.cbox, 4, (1u << w.n) - 1u, Q);
            std::memcpy(f.origin, Q.origin, 12); std::memcpy(f.e, Q.e, 3);
            f.qlo_x = pack4(Q.lo[0]); f.qhi_x = pack4(Q.hi[0]); f.qlo_y = pack4(Q.lo[1]); f.qhi_y = pack4(Q.hi[1]); f.qlo_z = pack4(Q.lo[2]); f.qhi_z = pack4(Q.hi[2]);
            for (int c = 0; c < 4; c++) {
                if (c < w.n) { f.mask |= (uint8_t)(1u << c); f.child[c] = w.child[c] >= 0 ? w.child[c] * 4 : w.child[c]; }
                else f.child[c] = 0x76543210;
            }
        }
    });
    entry_src.clear(); entry_src.reserve(R.leaf_prims.size());
    for (flat4_node& n : out.nodes) {
        // leaf children: entries appended in slot order, link = ~first new entry.  Inner children are consecutive nodes already (memory_order); flat4_encode_links refuses a
        // node whose links the layout does not imply
        uint32_t counts[4];
        for (int c = 0; c < 4; c++) {
            counts[c] = 0;
            if (n.child[c] == 0x76543210 || n.child[c] >= 0) continue;
            const uint32_t first = (uint32_t)entry_src.size();
            for (uint32_t e = (uint32_t)~n.child[c];; e++) { entry_src.push_back(e); counts[c]++; if (R.leaf_last[e]) break; }
            n.child[c] = ~(int32_t)first;
            n.mask |= (uint8_t)(16u << c);
        }
        if (!flat4_encode_links(n.child, counts, 0u, n.links) || out.nodes.size() >= (1u << 24)) out.compact_links = false;   // slab flags: assign_slabs_q4
    }
    // The explicit-link form of the tree (no implied links, no slabs) is what a scene beyond 2^24 nodes or 2^26 entries gets; CTL_FLAT_FORCE_EXPLICIT=1 (knobs build only) builds it
    // for any scene so that the tests can walk that path
    if (flat_force_explicit() != 0) out.compact_links = false;
    out.child_links.resize(out.nodes.size() * 4);
    for (size_t i = 0; i < out.nodes.size(); i++) std::memcpy(&out.child_links[i * 4], out.nodes[i].child, 16);
}

// The Q8 nodes (flat8.h) of the 8-wide tree W, which is in memory order, the explicit links and the order of the leaf entries (as encode_q4; every leaf slot is ONE entry).
// false: a leaf holds several entries.  The BVH2 was built with one primitive per leaf, but coincident boxes (duplicate triangles, split references with identical boxes) can
// still share a leaf once the builder's depth limit is reached: such a scene takes the 4-wide format, whose leaves hold any number of entries
bool encode_q8(const std::vector<wide8_node>& W, const bvh_result& R, flat_scene& out, std::vector<uint32_t>& entry_src) {
    out.nodes_q8.resize(W.size()); out.child_links.assign(W.size() * 8, (int32_t)kFlat8None);
    parallel_for(W.size(), [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            const wide8_node& w = W[i]; flat8_node& f = out.nodes_q8[i];
            std::memset(&f, 0, sizeof(f));
            uint32_t first_inner = 0, exist = 0; bool have_inner = false, consecutive = true; uint32_t ni = 0;
            for (int c = 0; c < 8; c++) {
                const int k = w.child[c];
                if (k == 0x76543210) continue;
                exist |= 1u << c;
                out.child_links[i * 8 + c] = k;   // leaf links are rewritten below (entries in node order)
                if (k >= 0) { if (!have_inner) { first_inner = (uint32_t)k; have_inner = true; } if ((uint32_t)k != first_inner + ni) consecutive = false; ni++; f.imask |= (uint8_t)(1u << c); }
                else f.base_b |= 1u << (24 + c);   // B of a non-inner slot: a leaf
            }
            if (!consecutive) f.base_b = 0xffffffffu;   // cannot happen (memory_order); flat_links_valid refuses the tree
            else f.base_b |= first_inner;
            child_codes Q; quantise_child_boxes(w.box, w.cbox, 8, exist, Q);
            std::memcpy(f.origin, Q.origin, 12); std::memcpy(f.e, Q.e, 3);
            for (int h = 0; h < 2; h++) {
                f.qlo_x[h] = pack4(Q.lo[0] + 4 * h); f.qhi_x[h] = pack4(Q.hi[0] + 4 * h); f.qlo_y[h] = pack4(Q.lo[1] + 4 * h); f.qhi_y[h] = pack4(Q.hi[1] + 4 * h);
                f.qlo_z[h] = pack4(Q.lo[2] + 4 * h); f.qhi_z[h] = pack4(Q.hi[2] + 4 * h);
            }
            f.slab_lo[0] = f.slab_lo[1] = 0u; f.slab_hi[0] = f.slab_hi[1] = 0xffffffffu;
        }
    });
    entry_src.clear(); entry_src.reserve(R.leaf_prims.size());
    for (size_t i = 0; i < out.nodes_q8.size(); i++) {
        out.nodes_q8[i].leaf_base = (uint32_t)entry_src.size();
        for (int c = 0; c < 8; c++) {
            int32_t& k = out.child_links[i * 8 + c];
            if (k >= 0) continue;   // inner child, or kFlat8None (positive)
            const uint32_t e = (uint32_t)~k;
            if (!R.leaf_last[e]) return false;
            k = ~(int32_t)entry_src.size(); entry_src.push_back(e);
        }
    }
    return true;
}

// the BVH2 over the references and its collapse into the 8-wide tree of `out`.  false when the scene does not fit the format: node indices are 24 bits, and encode_q8
bool build_q8(const references& refs, bvh_result& R, flat_scene& out, std::vector<uint32_t>& entry_src, phase_timer& pt) {
    build_bvh(refs.boxes, 1, true, 60, R, flat_node_cost(), flat_reinsert_passes(), flat_reinsert_fraction());   // every leaf slot is ONE entry (flat8.h)
    pt.lap("build BVH2");
    std::vector<wide8_node> W;
    collapse_bvh8(R, W, out.max_depth);   // octant-ordered slots (bvh_builder.h)
    if (W.size() >= kFlat8MaxNodes) return false;
    memory_order(W, (size_t)flat_bfs_top());
    const bool fits = encode_q8(W, R, out, entry_src);
    pt.lap("node layout");
    return fits;
}
// ... and into the 4-wide tree, which holds any scene (its links turn explicit past the limits of the implied ones)
void build_q4(const references& refs, bvh_result& R, flat_scene& out, std::vector<uint32_t>& entry_src, phase_timer& pt) {
    build_bvh(refs.boxes, flat_max_leaf(), true, 60, R, flat_node_cost(), flat_reinsert_passes(), flat_reinsert_fraction());
    pt.lap("build BVH2");
    std::vector<wide4_node> W;
    collapse_bvh4(R, W, out.max_depth, flat_collapse_mode(), flat_collapse_node_cost(), std::min(flat_max_leaf(), 4));
    order_slots(W, flat_slot_order());
    memory_order(W, (size_t)flat_bfs_top());
    encode_q4(W, R, out, entry_src);
    pt.lap("node layout");
}

// the leaf entries in their final order, and (Q4) the refit side's clip boxes of the split references among them (flat_refit.h)
void emit_leaf_entries(const ctl_scene_desc& d, const references& refs, const bvh_result& R, const std::vector<uint32_t>& entry_src, flat_scene& out) {
    out.leaves.resize(entry_src.size());
    parallel_for(entry_src.size(), [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            const uint32_t src = entry_src[i];
            const wtri& t = refs.tris[R.leaf_prims[src]];
            flat_leaf& L = out.leaves[i];
            std::memset(&L, 0, sizeof(L));
            const ctl_woop_tri& w = d.woop[t.woop];   // the mesh's own rows: the kernel applies the instance transform to the ray
            std::memcpy(L.a, w.a, 16); std::memcpy(L.b, w.b, 16); std::memcpy(L.c, w.c, 16);
            std::memcpy(L.inv, d.node_inv_transforms[t.node].m, 48); L.w33 = d.node_inv_transforms[t.node].m[15];
            L.index = (t.tri << 1) | (R.leaf_last[src] ? 1u : 0u); L.node = t.node;
        }
    });
    if (out.format != kFlatQ4) return;
    out.refit.part_index.assign(entry_src.size(), kRefitNoPart);
    for (size_t i = 0; i < entry_src.size(); i++) {
        const size_t g = R.leaf_prims[entry_src[i]];
        if (g >= refs.is_part.size() || !refs.is_part[g]) continue;
        out.refit.part_index[i] = (uint32_t)out.refit.part_boxes.size();
        refit_box pb; for (int r = 0; r < 3; r++) { pb.lo[r] = refs.boxes[g].lo[r]; pb.hi[r] = refs.boxes[g].hi[r]; }
        out.refit.part_boxes.push_back(pb);
    }
}

// what make_slab sees of a finished tree, either wide format: the explicit links, the leaf entries and the world-space triangle behind each
struct slab_context {
    const ctl_scene_desc& d; const references& refs; const bvh_result& R; const std::vector<uint32_t>& entry_src;
    int W;                                  // children per node: 4 (an inner link is node index * 4) or 8 (an inner link is the node index)
    const std::vector<int32_t>& links;      // W explicit links per node
    const std::vector<flat_leaf>& leaves;   // a leaf = the entries from its first one up to the next `last` flag
    std::vector<uint8_t> sub_tris;          // triangles under every node, saturated at 255
    size_t node_of(int32_t k) const { return W == 8 ? (size_t)k : (size_t)k / 4; }
    void world_tri(uint32_t entry, double w[3][3], double& slack) const { refs.world(d, R.leaf_prims[entry_src[entry]], w, slack); }

    slab_context(const ctl_scene_desc& d_, const references& refs_, const bvh_result& R_, const std::vector<uint32_t>& entry_src_, const flat_scene& F)
        : d(d_), refs(refs_), R(R_), entry_src(entry_src_), W(F.format == kFlatQ8 ? 8 : 4), links(F.child_links), leaves(F.leaves), sub_tris(F.child_links.size() / (size_t)W, 0) {
        for (size_t i = sub_tris.size(); i-- > 0;) {   // children follow their parent in memory, so one backwards sweep does it
            uint32_t n = 0;
            for (int c = 0; c < W; c++) {
                const int32_t k = links[i * W + c];
                if (k == 0x76543210) continue;
                if (k >= 0) n += sub_tris[node_of(k)];
                else for (uint32_t e = (uint32_t)~k;; e++) { n++; if (leaves[e].index & 1u) break; }
            }
            sub_tris[i] = (uint8_t)std::min(n, 255u);
        }
    }
};
struct slab_codes { uint32_t slab_n; float base; uint8_t lo[8], hi[8]; };
// The oriented slab (flat_slab.h) of one node that has leaf children: origin / ex / ql / qh = its child boxes as stored (child_codes), exist / leafm = per-slot masks, ch = its
// W explicit links.  An INNER child whose whole subtree holds at most $CTL_FLAT_SLAB_SUBTREE triangles (a bottom node: the patch of surface under it is as flat as its
// triangles) gets a real interval too: a ray that crosses the patch's box but not the patch itself is turned away one level higher and never fetches the bottom node.
// false: the node carries no slab.
bool make_slab(const slab_context& C, const float* origin, const uint8_t* ex, uint32_t exist, uint32_t leafm, const uint8_t ql[3][8], const uint8_t qh[3][8], const int32_t* ch, slab_codes& S) {
    const int W = C.W;
    const int sub_cap = std::min(std::max(flat_slab_subtree(), 0), kSlabSubtreeMax);
    const double useful_below = flat_slab_useful();
    if (useful_below <= 0.0) return false;
    // triangles of the leaf children and of the inner children with small subtrees; `tight` = the children that get an interval of their own
    constexpr int kT = 8 * kSlabSubtreeMax; static thread_local std::vector<slab_ctri> T; if (T.size() < (size_t)kT) T.resize(kT);
    int nt = 0; uint32_t tight = 0;
    const int kTw = W * kSlabSubtreeMax;   // the 4-wide tree's own cap (its arrays held 4 x the subtree limit)
    for (int c = 0; c < W; c++) {
        if (!((exist >> c) & 1)) continue;
        if ((leafm >> c) & 1) { tight |= 1u << c; for (uint32_t e = (uint32_t)~ch[c];; e++) { T[nt].c = c; C.world_tri(e, T[nt].w, T[nt].slack); nt++; if ((C.leaves[e].index & 1u) || nt == kTw) break; } continue; }
        if (sub_cap <= 0 || C.sub_tris[C.node_of(ch[c])] > sub_cap) continue;
        const int nt_before = nt; bool complete = true;
        int32_t stack[128]; int sp = 0; stack[sp++] = ch[c];
        while (sp && complete) {
            const int32_t k = stack[--sp];
            if (k >= 0) { for (int q = 0; q < W; q++) { const int32_t kk = C.links[C.node_of(k) * W + q]; if (kk == 0x76543210) continue; if (sp < (W == 4 ? 64 : 128)) stack[sp++] = kk; else complete = false; } }
            else for (uint32_t e = (uint32_t)~k;; e++) { if (nt < kTw) { T[nt].c = c; C.world_tri(e, T[nt].w, T[nt].slack); nt++; } else complete = false; if (C.leaves[e].index & 1u) break; }
        }
        if (complete) tight |= 1u << c; else nt = nt_before;   // an interval must cover EVERY triangle under the child, or the child keeps the whole node
    }
    if (!tight || nt == 0) return false;
    double stepk[3], ext1 = 0, mag = 0;
    for (int k = 0; k < 3; k++) { stepk[k] = std::ldexp(1.0, (int)ex[k] - 127); ext1 += 255.0 * stepk[k]; mag = std::max(mag, std::fabs((double)origin[k]) + 255.0 * stepk[k]); }
    int best_n[3] = { 0, 0, 0 }; double best_cost = 1e300; double best_lo[8], best_hi[8];
    // candidate directions: the triangles' own normals (at most 24 of them, evenly picked) and — for patches — the area-weighted mean normal of every child and of all
    double mean_n[9][3] = {};
    for (int t = 0; t < nt; t++) {
        const double (*w)[3] = T[t].w;
        const double a[3] = { w[1][0] - w[0][0], w[1][1] - w[0][1], w[1][2] - w[0][2] }, b[3] = { w[2][0] - w[0][0], w[2][1] - w[0][1], w[2][2] - w[0][2] };
        const double n[3] = { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0] };
        for (int k = 0; k < 3; k++) { mean_n[T[t].c][k] += n[k]; mean_n[W][k] += n[k]; }
    }
    const int cand_step = std::max(1, nt / 24), n_tri_cand = (nt + cand_step - 1) / cand_step;
    for (int ci = 0; ci < n_tri_cand + (nt > 4 ? W + 1 : 0); ci++) {
        double n[3];
        if (ci < n_tri_cand) {
            const double (*w)[3] = T[ci * cand_step].w;
            const double a[3] = { w[1][0] - w[0][0], w[1][1] - w[0][1], w[1][2] - w[0][2] }, b[3] = { w[2][0] - w[0][0], w[2][1] - w[0][1], w[2][2] - w[0][2] };
            n[0] = a[1] * b[2] - a[2] * b[1]; n[1] = a[2] * b[0] - a[0] * b[2]; n[2] = a[0] * b[1] - a[1] * b[0];
        } else for (int k = 0; k < 3; k++) n[k] = mean_n[ci - n_tri_cand][k];
        const double m = std::max(std::max(std::fabs(n[0]), std::fabs(n[1])), std::fabs(n[2]));
        if (!(m > 0) || !std::isfinite(m)) continue;
        int nq[3]; for (int k = 0; k < 3; k++) nq[k] = (int)std::lround(n[k] / m * (double)kSlabNMax);
        if (nq[0] == best_n[0] && nq[1] == best_n[1] && nq[2] == best_n[2]) continue;   // the direction that leads already
        double lo[8], hi[8]; for (int c = 0; c < 8; c++) { lo[c] = 1e300; hi[c] = -1e300; }
        for (int t = 0; t < nt; t++) for (int j = 0; j < 3; j++) {
            const double D = nq[0] * (T[t].w[j][0] - (double)origin[0]) + nq[1] * (T[t].w[j][1] - (double)origin[1]) + nq[2] * (T[t].w[j][2] - (double)origin[2]);
            lo[T[t].c] = std::min(lo[T[t].c], D); hi[T[t].c] = std::max(hi[T[t].c], D);
        }
        double cost = 0; int nl = 0;
        for (int c = 0; c < W; c++) if ((tight >> c) & 1) {
            double range = 0; for (int k = 0; k < 3; k++) range += std::fabs((double)nq[k]) * stepk[k] * (double)((int)qh[k][c] - (int)ql[k][c]);
            cost += range > 0 ? std::min(1.0, (hi[c] - lo[c]) / range) : 1.0; nl++;
        }
        cost /= nl;
        if (cost < best_cost) { best_cost = cost; for (int k = 0; k < 3; k++) best_n[k] = nq[k]; for (int c = 0; c < W; c++) { best_lo[c] = lo[c]; best_hi[c] = hi[c]; } }
    }
    if (!(best_cost < useful_below)) return false;
    // static pad per child: round-off reach of the object-space test (2^-20 of the magnitudes involved) + the node-extent share of the kernel's evaluation error
    const double n1 = std::fabs((double)best_n[0]) + std::fabs((double)best_n[1]) + std::fabs((double)best_n[2]);
    double pad[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    for (int t = 0; t < nt; t++) pad[T[t].c] = std::max(pad[T[t].c], n1 * 9.5367431640625e-7 * (T[t].slack + mag) + (double)kSlabRayPad * ext1);   // 2^-20 of the magnitudes: ~8 x the fp32 round-off of the object-space test
    // D range the codes span: the leaf children's padded intervals — and, when the node has inner children too, the whole node (its
    // quantisation grid's box), which their code 0 .. 255 must cover
    double nlo = 1e300, nhi = -1e300;
    for (int c = 0; c < W; c++) if ((tight >> c) & 1) { nlo = std::min(nlo, best_lo[c] - pad[c]); nhi = std::max(nhi, best_hi[c] + pad[c]); }
    if (exist != tight) {   // a child without an interval of its own spans the whole node
        double pmax = 0; for (int c = 0; c < W; c++) pmax = std::max(pmax, pad[c]);
        double blo = 0, bhi = 0; for (int k = 0; k < 3; k++) { const double x = best_n[k] * 255.0 * stepk[k]; if (x < 0) blo += x; else bhi += x; }
        nlo = std::min(nlo, blo - pmax); nhi = std::max(nhi, bhi + pmax);
    }
    const float base = round_down(nlo);
    // step: a float with 5 mantissa bits (the top 14 bits of its pattern share a word with the normal), rounded up; 254 steps span the range
    float stepf = round_up((nhi - (double)base) / 254.0);
    if (!(stepf > 0.0f) || !std::isfinite(stepf)) stepf = 1.17549435e-38f;
    { uint32_t bits; std::memcpy(&bits, &stepf, 4); bits = (bits + 0x3ffffu) & 0xfffc0000u; std::memcpy(&stepf, &bits, 4); }
    if (!std::isfinite(stepf) || stepf < 1.17549435e-38f) return false;
    const double step = (double)stepf;
    bool ok = true;
    for (int c = 0; c < W; c++) {
        long lo, hi;
        if (!((exist >> c) & 1)) { lo = 255; hi = 0; }
        else if (!((tight >> c) & 1)) { lo = 0; hi = 255; }
        else {
            lo = (long)std::floor((best_lo[c] - pad[c] - (double)base) / step);
            hi = (long)std::ceil((best_hi[c] + pad[c] - (double)base) / step);
            // conservative under the fp32 evaluation base + step * code as well
            while (lo > 0 && (double)(float)((double)base + step * (double)lo) > best_lo[c] - pad[c]) lo--;
            while (hi < 255 && (double)(float)((double)base + step * (double)hi) < best_hi[c] + pad[c]) hi++;
            if (lo < 0 || hi > 255 || (double)base + step * (double)lo > best_lo[c] - pad[c] || (double)base + step * (double)hi < best_hi[c] + pad[c]) ok = false;
        }
        S.lo[c] = (uint8_t)(lo & 255); S.hi[c] = (uint8_t)(hi & 255);
    }
    if (!ok || (double)base + 255.0 * step < nhi) return false;
    uint32_t sb; std::memcpy(&sb, &stepf, 4);
    S.slab_n = ((uint32_t)best_n[0] & 63u) | (((uint32_t)best_n[1] & 63u) << 6) | (((uint32_t)best_n[2] & 63u) << 12) | sb;
    S.base = base;
    return true;
}

// slabs of a compact Q4 tree: they take the last 16 B of a node, and the slab flag of an inner child goes into its parent's link (flatten.h)
void assign_slabs_q4(const slab_context& C, flat_scene& out) {
    std::vector<uint8_t> has_slab(out.nodes.size(), 0);
    parallel_for(out.nodes.size(), [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            flat4_node& f = out.nodes[i];
            f.slab_n = 0; f.slab_base = 0.0f; f.slab_lo = 0; f.slab_hi = 0xffffffffu;
            uint8_t ql[3][8] = {}, qh[3][8] = {};
            unpack4(f.qlo_x, ql[0]); unpack4(f.qlo_y, ql[1]); unpack4(f.qlo_z, ql[2]); unpack4(f.qhi_x, qh[0]); unpack4(f.qhi_y, qh[1]); unpack4(f.qhi_z, qh[2]);
            slab_codes S;
            if (!make_slab(C, f.origin, f.e, f.mask & 15u, (uint32_t)(f.mask >> 4) & (f.mask & 15u), ql, qh, &out.child_links[i * 4], S)) continue;
            f.slab_n = S.slab_n; f.slab_base = S.base; f.slab_lo = pack4(S.lo); f.slab_hi = pack4(S.hi);
            has_slab[i] = 1;
        }
    });
    for (size_t i = 0; i < out.nodes.size(); i++) {
        out.slab_nodes += has_slab[i];
        // slab flag of an inner child = bit 0 of its link: bit 0 of links[0] for slot 0, bit 0 of the slot's nibble otherwise (flatten.h)
        for (int c = 0; c < 4; c++) {
            const int32_t k = out.child_links[i * 4 + c];
            if (k < 0 || k == 0x76543210 || !has_slab[(size_t)k / 4]) continue;
            if (c == 0) out.nodes[i].links[0] |= 1u; else if (c == 1) out.nodes[i].links[0] |= 1u << 26; else if (c == 2) out.nodes[i].links[1] |= 1u << 2; else out.nodes[i].links[0] |= 1u << 30;
        }
    }
    out.root_slab = has_slab[0] != 0;
}
// slabs of a Q8 tree, and B of an inner slot: the child node has leaf slots or a slab — a step on it loads q5 too, and a lane that holds a parked leaf group waits before it (flat8.h)
void assign_slabs_q8(const slab_context& C, flat_scene& out) {
    std::vector<uint8_t> has_slab(out.nodes_q8.size(), 0);
    parallel_for(out.nodes_q8.size(), [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            flat8_node& f = out.nodes_q8[i];
            uint8_t ql[3][8], qh[3][8];
            for (int h = 0; h < 2; h++) {
                unpack4(f.qlo_x[h], ql[0] + 4 * h); unpack4(f.qlo_y[h], ql[1] + 4 * h); unpack4(f.qlo_z[h], ql[2] + 4 * h);
                unpack4(f.qhi_x[h], qh[0] + 4 * h); unpack4(f.qhi_y[h], qh[1] + 4 * h); unpack4(f.qhi_z[h], qh[2] + 4 * h);
            }
            const uint32_t leafm = (f.base_b >> 24) & ~(uint32_t)f.imask, exist = leafm | f.imask;
            slab_codes S;
            if (!make_slab(C, f.origin, f.e, exist, leafm, ql, qh, &out.child_links[i * 8], S)) continue;
            f.slab_n = S.slab_n; f.slab_base = S.base;
            for (int h = 0; h < 2; h++) { f.slab_lo[h] = pack4(S.lo + 4 * h); f.slab_hi[h] = pack4(S.hi + 4 * h); }
            has_slab[i] = 1;
        }
    });
    auto heavy = [&](size_t k) { const flat8_node& c = out.nodes_q8[k]; return has_slab[k] || ((c.base_b >> 24) & ~(uint32_t)c.imask) != 0u; };
    for (size_t i = 0; i < out.nodes_q8.size(); i++) {
        out.slab_nodes += has_slab[i];
        for (int c = 0; c < 8; c++) { const int32_t k = out.child_links[i * 8 + c]; if (k >= 0 && k != 0x76543210 && heavy((size_t)k)) out.nodes_q8[i].base_b |= 1u << (24 + c); }
    }
    out.root_slab = heavy(0);
}

// Slots without a child.  Their box is inverted, which the slab test rejects — unless the ray origin is so far from a small node (~2^16 node extents) that
// entry and exit plane round to the same distance on every axis; then the kernel follows the slot's link.  It must lead somewhere harmless: the link of a
// slot that exists (a second visit of a sibling finds nothing new).  Implied links: an empty slot's nibble is 0, which is the node's first inner child; a node
// without inner children gets the empty slot's LEAF bit set and nibble 15 = its first leaf entry (only the kernels and flat4_implied_links read a leaf bit
// without its exists bit; host code asks for both).  Explicit links: the slot's word repeats the first child's.
void patch_empty_slots_q4(flat_scene& out) {
    for (flat4_node& f : out.nodes) {
        const uint32_t exist = f.mask & 15u, leafm = (uint32_t)(f.mask >> 4) & exist;
        if (exist == 15u || exist == 0u) continue;
        if (out.compact_links) {
            if ((exist & ~leafm) != 0u) continue;   // nibble 0 -> first inner child
            for (int c = 1; c < 4; c++) if (!((exist >> c) & 1u)) {
                f.mask |= (uint8_t)(16u << c);
                if (c == 1) f.links[0] |= 15u << 26; else if (c == 2) f.links[1] |= 15u << 2; else { f.links[0] |= 3u << 30; f.links[1] |= 3u; }
            }
        } else for (int c = 1; c < 4; c++) if (!((exist >> c) & 1u)) f.child[c] = f.child[0];
    }
}

// Flattened-BVH cache (scene_cache.h).  The key: everything the result depends on — the builder's version and knobs, the node format, the leaf streams and the instance list
std::string flat_cache_key(const ctl_scene_desc& d, int format) {
    if (cache_dir().empty()) return std::string();
    content_hash H; const uint32_t version = 18;
    H.add_value(version); H.add_value(flat_slab_subtree()); H.add_value(flat_force_explicit()); H.add_value(flat_collapse_mode()); H.add_value(flat_slab_useful()); H.add_value(flat_collapse_node_cost());
    H.add_value(flat_bfs_top()); H.add_value((int)sizeof(flat_leaf)); H.add_value(flat_max_leaf()); H.add_value(flat_node_cost()); H.add_value(flat_split_ratio()); H.add_value(flat_split_gain());
    H.add_value(flat_reinsert_passes()); H.add_value(flat_reinsert_fraction()); H.add_value(flat_slot_order()); H.add_value(format); H.add_value(d.n_meshes); H.add_value(d.n_nodes); H.add_value(d.n_woop);
    H.add(d.woop, (size_t)d.n_woop * sizeof(ctl_woop_tri)); H.add(d.woop_index, (size_t)d.n_woop * sizeof(ctl_woop_index));
    H.add(d.meshes, (size_t)d.n_meshes * sizeof(ctl_kernel_mesh));
    for (uint32_t k = 0; k < d.n_nodes; k++) { H.add_value(d.nodes[k].mesh_index); H.add(d.node_transforms[k].m, 64); }
    return H.hex();
}
// The sections of a flat_<key> file in file order, for the reader and the writer alike (IO: cache_reader, or section_writer below; Tree: flat_scene, const for the writer).
// The refit side's part_index / part_boxes (flat_refit.h) close the file of a Q4 tree
struct cached_scalars { int format = -1, depth = 0, compact = 0, root_slab = 0; uint64_t slab_nodes = 0, split_refs = 0; };
template <typename IO, typename Tree> bool cache_sections(IO& io, cached_scalars& s, Tree& F) {
    return io.value(s.format) && io.value(s.depth) && io.value(s.compact) && io.vector(F.nodes) && io.vector(F.nodes_q8) && io.vector(F.leaves) && io.vector(F.child_links) &&
           io.value(s.root_slab) && io.value(s.slab_nodes) && io.value(s.split_refs) && (s.format != kFlatQ4 || (io.vector(F.refit.part_index) && io.vector(F.refit.part_boxes)));
}
struct section_writer {
    cache_writer& w;
    template <typename T> bool value(const T& v) { w.value(v); return true; }
    template <typename T> bool vector(const std::vector<T>& v) { w.vector(v); return true; }
};
void reset_tree(flat_scene& F, int format) { F = flat_scene(); F.format = format; }
// the tree of `key` from the cache into `out`, checked before it can reach the GPU; false (and `out` as it was reset) when there is none that holds.  A Q4 file without the
// refit sections is refused: every file of cache version 18 has them (older versions wrote files without, and are never found under this key)
bool load_cached(const std::string& key, const ctl_scene_desc& d, flat_scene& out) {
    if (key.empty()) return false;
    const int format = out.format;
    cache_reader rd("flat", key);
    cached_scalars s;
    bool ok = rd.found() && cache_sections(rd, s, out) && rd.verify() && s.format == format && ((out.compact_links = s.compact != 0), flat_links_valid(out));
    if (ok && format == kFlatQ4) {
        ok = out.refit.part_index.size() == out.leaves.size();
        for (uint32_t p : out.refit.part_index) if (p != kRefitNoPart && p >= out.refit.part_boxes.size()) ok = false;
    }
    if (!ok) { reset_tree(out, format); return false; }
    out.max_depth = s.depth; out.root_slab = s.root_slab != 0; out.slab_nodes = (size_t)s.slab_nodes; out.split_refs = (size_t)s.split_refs;
    finish_refit_side(out, d);
    return true;
}
void store_cached(const std::string& key, const flat_scene& F) {
    cache_writer wr("flat", key);
    if (!wr.active()) return;
    cached_scalars s; s.format = F.format; s.depth = F.max_depth; s.compact = F.compact_links ? 1 : 0; s.root_slab = F.root_slab ? 1 : 0; s.slab_nodes = F.slab_nodes; s.split_refs = F.split_refs;
    section_writer io{ wr };
    cache_sections(io, s, F);
    wr.commit();
}

}  // namespace

int default_flat_format() {
    static const int v = [] {
        const char* e = knob_env("CTL_FLAT_FORMAT");
        return (e && (!std::strcmp(e, "q8") || !std::strcmp(e, "Q8"))) ? (int)kFlatQ8 : (int)kFlatQ4;
    }();
    return v;
}

bool flatten_scene(const ctl_scene_desc& d, flat_scene& out, size_t max_triangles, int format) {
    reset_tree(out, format == kFlatQ8 ? kFlatQ8 : kFlatQ4);
    phase_timer pt;
    mesh_triangles mesh_tris;
    const size_t total = unique_mesh_triangles(d, mesh_tris);
    if (total == 0 || total > max_triangles) return false;
    std::string key = flat_cache_key(d, out.format);
    if (load_cached(key, d, out)) { pt.lap("cache hit"); return true; }

    references refs;
    if (!gather_references(d, mesh_tris, refs)) return false;
    pt.lap("world triangles");
    if (flat_split_ratio() > 0.0f) { split_large_references(d, refs); pt.lap("split large triangles"); }

    bvh_result R; std::vector<uint32_t> entry_src;   // the BVH2 over the references; leaf entry -> position in R.leaf_prims
    if (out.format == kFlatQ8 && !build_q8(refs, R, out, entry_src, pt)) {
        // a scene that does not fit the 8-wide format becomes what a request for the 4-wide one builds and caches: same references, the BVH2 rebuilt with its leaf size
        reset_tree(out, kFlatQ4);
        key = flat_cache_key(d, kFlatQ4);
        if (load_cached(key, d, out)) { pt.lap("cache hit"); return true; }
    }
    if (out.format == kFlatQ4) build_q4(refs, R, out, entry_src, pt);
    out.split_refs = refs.split_refs;
    emit_leaf_entries(d, refs, R, entry_src, out);
    pt.lap("leaf entries");
    if (out.format == kFlatQ8 || out.compact_links) {   // a tree with explicit links has no room for slabs
        const slab_context C(d, refs, R, entry_src, out);
        if (out.format == kFlatQ8) assign_slabs_q8(C, out); else assign_slabs_q4(C, out);
        pt.lap("slabs");
    }
    if (out.format == kFlatQ4) patch_empty_slots_q4(out);
    if (!key.empty()) { store_cached(key, out); pt.lap("cache write"); }
    finish_refit_side(out, d);
    return true;
}

double flat_scene_node_area(const flat_scene& F) {
    double a = 0.0;
    for (const flat4_node& n : F.nodes) { uint32_t w[10]; std::memcpy(w, &n, 40); a += refit_node_area(w); }
    return a;
}

void triangle_woop_rows(const ctl_scene_desc& d, std::vector<uint32_t>& tri_row) {
    const mesh_ranges R(d);
    tri_row.assign(d.n_tri_data, 0xffffffffu);
    for (uint32_t m = 0; m < d.n_meshes; m++)
        for (uint32_t w = R.woop1[m]; w-- > R.woop0[m];) {   // backwards: the first reference in stream order stays
            const size_t at = (size_t)d.meshes[m].bvh_index_offset + (w - R.woop0[m]);
            if (at >= d.n_woop) continue;
            const uint64_t tri = (uint64_t)d.meshes[m].tri_offset + (d.woop_index[at].index >> 1);
            if (tri < d.n_tri_data) tri_row[tri] = w;
        }
}

void flat_missing_triangles(const std::vector<flat_leaf>& leaves, uint32_t index_mask, const ctl_scene_desc& d, std::vector<uint32_t>& missing) {
    std::vector<uint8_t> has(d.n_tri_data, 0), instanced(d.n_meshes, 0);
    for (const flat_leaf& L : leaves) { const uint32_t tri = (L.index & index_mask) >> 1; if (tri < d.n_tri_data) has[tri] = 1; }
    for (uint32_t k = 0; k < d.n_nodes; k++) if (d.nodes[k].mesh_index < d.n_meshes) instanced[d.nodes[k].mesh_index] = 1;
    const mesh_ranges R(d);
    missing.clear();
    for (uint32_t m = 0; m < d.n_meshes; m++) if (instanced[m]) for (uint32_t t = R.tri0[m]; t < R.tri1[m]; t++) if (!has[t]) missing.push_back(t);
    std::sort(missing.begin(), missing.end());
}

int mesh_gaining_a_triangle(const ctl_scene_desc& d, const std::vector<uint32_t>& missing, const std::vector<uint32_t>& tri_row, const std::vector<uint8_t>& mesh_changed) {
    if (missing.empty()) return -1;
    const mesh_ranges R(d);
    for (uint32_t m = 0; m < d.n_meshes; m++) {
        if (!mesh_changed[m]) continue;
        for (auto it = std::lower_bound(missing.begin(), missing.end(), R.tri0[m]); it != missing.end() && *it < R.tri1[m]; ++it) {
            const uint32_t row = *it < tri_row.size() ? tri_row[*it] : 0xffffffffu;
            double v[3][3];
            if (row < d.n_woop && woop_vertices(d.woop[row], v)) return (int)m;
        }
    }
    return -1;
}

// The host refit: the yardstick of the kernels in flat_refit.hip, which run the same functions of flat_refit.h in the same order.
void refit_flat_scene(flat_scene& F, const ctl_scene_desc& d, double* area_before_after) {
    if (F.format != kFlatQ4) throw unsupported_error("refit: only the Q4 node format can be refitted");
    if (!F.refit.ready() || F.refit.part_index.size() != F.leaves.size()) throw std::runtime_error("refit: the tree carries no refit data");
    if (d.n_nodes != F.refit.xf0.size()) throw std::runtime_error("refit: the description has another number of nodes than the tree was built from");
    std::vector<double> P((size_t)d.n_nodes * 12);
    for (uint32_t k = 0; k < d.n_nodes; k++)
        if (!refit_carry_matrix(d.node_transforms[k].m, F.refit.xf0[k].m, &P[(size_t)k * 12])) throw std::runtime_error("refit: singular node transform");
    for (const flat_leaf& L : F.leaves) if (L.node >= d.n_nodes) throw std::runtime_error("refit: leaf entry out of range");
    // deformed meshes (ctl_scene_update's CTL_DIFF_GEOMETRY): found by their value hashes; everything that can refuse runs before the first byte is written
    std::vector<uint8_t> mesh_changed; std::vector<uint32_t> tri_row; geometry_hashes geom; bool deformed = false;
    if (!F.refit.geom.empty()) {
        hash_geometry(d, geom);
        if (!geom.same_structure(F.refit.geom)) throw std::runtime_error("refit: the topology of the description differs from the one the tree was built from");
        mesh_changed.assign(d.n_meshes, 0);
        for (uint32_t m = 0; m < d.n_meshes; m++) if (!geom.same_values(F.refit.geom, m)) { mesh_changed[m] = 1; deformed = true; }
    }
    if (deformed) {
        for (uint32_t k = 0; k < d.n_nodes; k++) if (d.nodes[k].mesh_index >= d.n_meshes) throw std::runtime_error("refit: node references a missing mesh");
        triangle_woop_rows(d, tri_row);
        std::vector<uint32_t> missing; flat_missing_triangles(F.leaves, 0xffffffffu, d, missing);
        const int m = mesh_gaining_a_triangle(d, missing, tri_row, mesh_changed);
        if (m >= 0) throw std::runtime_error("refit: mesh " + std::to_string(m) + " has a triangle that was degenerate when the tree was built and no longer is: the tree has no leaf entry for it");
        for (const flat_leaf& L : F.leaves) if (mesh_changed[d.nodes[L.node].mesh_index] && ((L.index >> 1) >= d.n_tri_data || tri_row[L.index >> 1] >= d.n_woop)) throw std::runtime_error("refit: leaf entry without a Woop row");
    }
    if (area_before_after) area_before_after[0] = flat_scene_node_area(F);
    if (deformed) {
        parallel_for(F.leaves.size(), [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; i++) {
                flat_leaf& L = F.leaves[i];
                if (!mesh_changed[d.nodes[L.node].mesh_index]) continue;
                const ctl_woop_tri& w = d.woop[tri_row[L.index >> 1]];
                std::memcpy(L.a, w.a, 16); std::memcpy(L.b, w.b, 16); std::memcpy(L.c, w.c, 16);
                F.refit.part_index[i] = kRefitNoPart;   // the clip box was cut from the triangle as it was: the entry stands for the whole triangle from now on
            }
        });
    }
    if (!F.refit.geom.empty()) F.refit.geom = geom;
    std::vector<refit_box> ebox(F.leaves.size()), nbox(F.nodes.size());
    parallel_for(F.leaves.size(), [&](size_t i0, size_t i1) {
        for (size_t i = i0; i < i1; i++) {
            flat_leaf& L = F.leaves[i];
            std::memcpy(L.inv, d.node_inv_transforms[L.node].m, 48); L.w33 = d.node_inv_transforms[L.node].m[15];
            const uint32_t pi = F.refit.part_index[i];
            refit_entry_box(L.a, L.b, L.c, d.node_transforms[L.node].m, pi == kRefitNoPart ? nullptr : &F.refit.part_boxes[pi], &P[(size_t)L.node * 12], ebox[i]);
        }
    });
    const auto& R = F.refit;
    for (size_t l = R.level_start.size() - 1; l-- > 0;) {
        parallel_for(R.level_start[l + 1] - R.level_start[l], [&](size_t j0, size_t j1) {
            for (size_t j = j0; j < j1; j++) {
                const uint32_t i = R.level_nodes[R.level_start[l] + j];
                flat4_node& n = F.nodes[i];
                const uint32_t exist = n.mask & 15u;
                refit_box cb[4];
                for (int c = 0; c < 4; c++) {
                    if (!((exist >> c) & 1u)) continue;
                    const int32_t k = F.child_links[(size_t)i * 4 + c];
                    if (k >= 0) { cb[c] = nbox[(size_t)k / 4]; continue; }
                    for (int r = 0; r < 3; r++) { cb[c].lo[r] = kRefitBig; cb[c].hi[r] = -kRefitBig; }
                    for (uint32_t e = (uint32_t)~k;; e++) {
                        for (int r = 0; r < 3; r++) { cb[c].lo[r] = std::min(cb[c].lo[r], ebox[e].lo[r]); cb[c].hi[r] = std::max(cb[c].hi[r], ebox[e].hi[r]); }
                        if (F.leaves[e].index & 1u) break;
                    }
                }
                uint32_t w[10]; std::memcpy(w, &n, 40);
                refit_node_boxes(w, exist, cb, nbox[i]);
                std::memcpy(&n, w, 40);
                if (F.compact_links && n.slab_n != 0u) { n.slab_n = kRefitNeutralSlabN; std::memcpy(&n.slab_base, &kRefitNeutralSlabBase, 4); uint32_t lo = 0, hi = 0; for (int c = 0; c < 4; c++) { if ((exist >> c) & 1u) hi |= 255u << (8 * c); else lo |= 255u << (8 * c); } n.slab_lo = lo; n.slab_hi = hi; }
            }
        }, 1024);
    }
    if (area_before_after) area_before_after[1] = flat_scene_node_area(F);
}

}  // namespace ctl
