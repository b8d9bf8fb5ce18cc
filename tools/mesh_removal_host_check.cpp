// mesh_removal_host_check.cpp — a stand-alone run of the host side of ctl_scene_update_mesh_set (scene_builder.cpp remove_mesh; csrc/flat_mesh_set.cpp: the mesh map and
// the runs of plan_mesh_compaction, plan_mesh_set's acceptance, the host re-statement of k_compact_tri_rows, update_mesh_set_flat_scene) for a sanitizer build, over the
// removal cases of tests/mesh_removal_cases.py: the last mesh, the first mesh, two holes with a kept mesh between them, a removal together with an append, every mesh but
// one, nothing removed, and a second removal on the result; synthetic descriptions made here, no fixture.
// tools/mesh_removal_host_check.sh compiles it with the host sources it needs, host code under -fsanitize=address,undefined, and runs it.
// Exit status 0 and "mesh removal host check ok" when, in every case, the builder after remove_mesh holds the arrays of a builder that never added the mesh, the compacted
// table equals triangle_woop_rows of the new description, the updated tree holds one entry per triangle of the new node set with its triangle inside the node's mesh, and
// the refusals leave builder and handle as they were.
#include "scene_builder.h"
#include "flatten.h"
#include "flat_nodes.h"
#include "flat_meshes.h"
#include "flat_mesh_set.h"
#include "flat_rebuild.h"
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

using namespace ctl;

// the builder's one reference into a device source (volume_eval.hip); this program creates no medium
namespace ctl { void volume_update(ctl_volume&) { throw std::runtime_error("mesh_removal_host_check: no media here"); } }

static uint32_t add_soup(scene_builder& b, uint32_t n_tri, uint32_t seed) {
    std::mt19937 rng(seed); std::uniform_real_distribution<float> u(-0.3f, 0.3f);
    std::vector<float> P; std::vector<uint32_t> I;
    for (uint32_t t = 0; t < n_tri; t++) {
        const float c[3] = { 0.7f * (float)(t % 7), 0.6f * (float)((t / 7) % 7), 0.5f * (float)(t / 49) };
        for (int v = 0; v < 3; v++) { for (int k = 0; k < 3; k++) P.push_back(c[k] + u(rng)); I.push_back(3 * t + v); }
    }
    ctl_material m{}; m.bsdf_type = CTL_BSDF_DIFFUSE;
    return b.add_mesh(P.data(), n_tri * 3, I.data(), n_tri, nullptr, nullptr, nullptr, &m, 1);
}
static ctl_float4x4 place(int k) {
    ctl_float4x4 m{}; m.m[0] = m.m[5] = m.m[10] = 0.8f + 0.05f * (float)k; m.m[15] = 1.0f;
    m.m[3] = -5.0f + 2.4f * (float)(k % 5); m.m[7] = 0.3f + 0.9f * (float)(k / 5); m.m[11] = -3.0f + 0.7f * (float)k;
    return m;
}
static void node(scene_builder& b, uint32_t mesh, int k) { const ctl_float4x4 m = place(k); b.add_node(mesh, &m); }

static const uint32_t kBase[] = { 2, 1, 4, 5, 63, 64, 65, 257 };
static const uint32_t kMeshes = 8;
// the base scene without the meshes whose bit is set in `never` (and without their nodes): mesh k of the base has one node, at place(k)
static void base(scene_builder& b, uint32_t never, ctl_scene_desc& d) {
    std::vector<uint32_t> mesh(kMeshes, kNodesNone);
    for (uint32_t k = 0; k < kMeshes; k++) if (!(never >> k & 1u)) mesh[k] = add_soup(b, kBase[k], 11 + k);
    for (uint32_t k = 0; k < kMeshes; k++) if (mesh[k] != kNodesNone) node(b, mesh[k], (int)k);
    const float pos[3] = { 0.5f, 5.5f, -13.0f }, target[3] = { 0, 1.2f, 0 }, up[3] = { 0, 1, 0 }, light[3] = { 1, 9, -2 }, power[3] = { 90, 90, 90 };
    b.add_point_light(light, power);
    b.set_camera_lookat(pos, target, up, 55.0f, 32, 32);
    b.finalize(d);
}
// the removal of the meshes in `gone` (bits over the CURRENT mesh indices, whose k-th mesh has the k-th node) from a finalized builder, nodes first
static void remove(scene_builder& b, uint32_t gone, ctl_scene_desc& d) {
    for (uint32_t k = (uint32_t)b.nodes.size(); k-- > 0;) if (gone >> b.nodes[k].mesh_index & 1u) b.remove_node(k);
    for (uint32_t m = (uint32_t)b.meshes.size(); m-- > 0;) if (gone >> m & 1u) b.remove_mesh(m);
    b.finalize(d);
}
static bool same_geometry(const ctl_scene_desc& a, const ctl_scene_desc& b) {
    if (a.n_tri_data != b.n_tri_data || a.n_woop != b.n_woop || a.n_bvh_nodes != b.n_bvh_nodes || a.n_meshes != b.n_meshes) return false;
    if (std::memcmp(a.tri_data, b.tri_data, (size_t)a.n_tri_data * sizeof(ctl_triangle_data)) || std::memcmp(a.woop, b.woop, (size_t)a.n_woop * sizeof(ctl_woop_tri)) ||
        std::memcmp(a.woop_index, b.woop_index, (size_t)a.n_woop * sizeof(ctl_woop_index)) || std::memcmp(a.bvh_nodes, b.bvh_nodes, (size_t)a.n_bvh_nodes * sizeof(ctl_bvh_node))) return false;
    for (uint32_t m = 0; m < a.n_meshes; m++)
        if (a.meshes[m].tri_offset != b.meshes[m].tri_offset || a.meshes[m].bvh_node_offset != b.meshes[m].bvh_node_offset || a.meshes[m].bvh_tri_offset != b.meshes[m].bvh_tri_offset ||
            a.meshes[m].bvh_index_offset != b.meshes[m].bvh_index_offset) return false;
    return true;
}
static void maps_of(uint32_t n_old_meshes, uint32_t n_old_nodes, uint32_t gone, const scene_builder& old_b, uint32_t appended_meshes, uint32_t added_nodes, std::vector<uint32_t>& mm, std::vector<uint32_t>& nm) {
    mm.clear(); nm.clear();
    for (uint32_t m = 0; m < n_old_meshes; m++) if (!(gone >> m & 1u)) mm.push_back(m);
    for (uint32_t k = 0; k < n_old_nodes; k++) if (!(gone >> old_b.nodes[k].mesh_index & 1u)) nm.push_back(k);
    mm.insert(mm.end(), appended_meshes, kNodesNone); nm.insert(nm.end(), added_nodes, kNodesNone);
}
// the tree of `F` against the description: every entry's triangle inside its node's mesh, one entry per triangle of every node
static void check_tree(const flat_scene& F, const ctl_scene_desc& d, const char* what) {
    const mesh_ranges R(d);
    std::vector<uint32_t> per_node(d.n_nodes, 0u);
    for (const flat_leaf& L : F.leaves) {
        if (L.node >= d.n_nodes) throw std::runtime_error(std::string(what) + ": an entry names a node outside the scene");
        const uint32_t m = d.nodes[L.node].mesh_index, t = L.index >> 1;
        if (t < R.tri0[m] || t >= R.tri1[m]) throw std::runtime_error(std::string(what) + ": an entry's triangle lies outside its node's mesh");
        per_node[L.node]++;
    }
    for (uint32_t k = 0; k < d.n_nodes; k++) if (per_node[k] != R.tri1[d.nodes[k].mesh_index] - R.tri0[d.nodes[k].mesh_index]) throw std::runtime_error(std::string(what) + ": a node has another number of entries than its mesh has triangles");
    if (F.refit.part_index.size() != F.leaves.size() || F.refit.xf0.size() != d.n_nodes || F.nodes.empty() || F.refit.level_nodes.size() != F.nodes.size()) throw std::runtime_error(std::string(what) + ": the updated tree has the wrong sizes");
}

struct handle { flat_scene F; node_set_basis basis; std::vector<uint32_t> missing; };
static void make(handle& h, const ctl_scene_desc& d) {
    if (!flatten_scene(d, h.F, (size_t)1 << 30, kFlatQ4)) throw std::runtime_error("nothing to flatten");
    hash_geometry(d, h.F.refit.geom); h.basis.fill(d);
}

// one removal case: meshes `gone` leave the base scene; append: a 5- and a 64-triangle mesh are appended in the same call, the first with a node
static void run_case(const char* name, uint32_t gone, bool append) {
    scene_builder b_old, b_new, b_never;
    ctl_scene_desc d_old{}, d_new{}, d_never{};
    base(b_old, 0, d_old);
    base(b_new, 0, d_new);
    if (append) { const uint32_t a = add_soup(b_new, 5, 41); add_soup(b_new, 64, 42); node(b_new, a, 9); }
    remove(b_new, gone, d_new);
    base(b_never, gone, d_never);
    if (append) { const uint32_t a = add_soup(b_never, 5, 41); add_soup(b_never, 64, 42); node(b_never, a, 9); b_never.finalize(d_never); }
    if (!same_geometry(d_new, d_never)) throw std::runtime_error(std::string(name) + ": the builder after remove_mesh differs from one that never added the mesh");
    std::vector<uint32_t> mm, nm;
    maps_of(d_old.n_meshes, d_old.n_nodes, gone, b_old, append ? 2u : 0u, append ? 1u : 0u, mm, nm);
    if (mm.size() != d_new.n_meshes || nm.size() != d_new.n_nodes) throw std::runtime_error(std::string(name) + ": the maps do not fit the new description");
    // the compacted table
    mesh_compaction cut; node_set_basis basis; basis.fill(d_old);
    plan_mesh_compaction(basis, mm.data(), (uint32_t)mm.size(), "check: ", cut);
    std::vector<uint32_t> held, want, got(cut.kept_tris);
    triangle_woop_rows(d_old, held); triangle_woop_rows(d_new, want);
    compact_tri_rows_host(cut, held.data(), (uint32_t)held.size(), got.data());
    if (want.size() < got.size() || !std::equal(got.begin(), got.end(), want.begin())) throw std::runtime_error(std::string(name) + ": the compacted table is not triangle_woop_rows of the new description");
    // the yardstick
    handle h; make(h, d_old);
    update_mesh_set_flat_scene(h.F, h.basis, d_new, mm.data(), (uint32_t)mm.size(), nm.data(), (uint32_t)nm.size(), h.missing);
    h.basis.fill(d_new);
    check_tree(h.F, d_new, name);
    rebuild_flat_scene(h.F, d_new, nullptr);
    std::printf("  %s: %u -> %u meshes, %u runs, %zu entries\n", name, d_old.n_meshes, d_new.n_meshes, cut.runs(), h.F.leaves.size());
}

int main() {
    try {
        run_case("the last mesh", 1u << 7, false);
        run_case("the first mesh", 1u << 0, false);
        run_case("two holes", (1u << 2) | (1u << 5), false);
        run_case("a removal with an append", 1u << 3, true);
        run_case("every mesh but one", 0xffu & ~(1u << 6), false);
        {   // nothing removed, then a removal and a second one on the result
            scene_builder b0, b1, b2; ctl_scene_desc d0{}, d1{}, d2{};
            base(b0, 0, d0); base(b1, 0, d1); remove(b1, (1u << 2) | (1u << 5), d1); base(b2, 0, d2); remove(b2, (1u << 2) | (1u << 5), d2); remove(b2, 1u << 0, d2);
            handle h; make(h, d0);
            const size_t n0 = h.F.leaves.size();
            std::vector<uint32_t> mm, nm;
            maps_of(d0.n_meshes, d0.n_nodes, 0u, b0, 0, 0, mm, nm);
            update_mesh_set_flat_scene(h.F, h.basis, d0, mm.data(), (uint32_t)mm.size(), nm.data(), (uint32_t)nm.size(), h.missing);
            if (h.F.leaves.size() != n0) throw std::runtime_error("an identity call changed the handle");
            // refusals: the handle and the builder stay as they were
            int refused = 0;
            maps_of(d0.n_meshes, d0.n_nodes, (1u << 2) | (1u << 5), b0, 0, 0, mm, nm);
            auto call = [&](const ctl_scene_desc& d, const std::vector<uint32_t>& m, const std::vector<uint32_t>& n) {
                try { update_mesh_set_flat_scene(h.F, h.basis, d, m.data(), (uint32_t)m.size(), n.data(), (uint32_t)n.size(), h.missing); } catch (const std::exception&) { refused++; } };
            { std::vector<uint32_t> m = mm; std::swap(m[0], m[1]); call(d1, m, nm); }                                             // a reordered map
            { std::vector<uint32_t> n = nm; n[2] = 2; call(d1, mm, n); }                                                            // a kept node on a removed mesh
            { std::vector<uint32_t> m = mm; m.pop_back(); call(d1, m, nm); }                                                        // a short map
            for (int step = -1; step <= 1; step += 2) { ctl_scene_desc x = d1; std::vector<ctl_kernel_mesh> k(d1.meshes, d1.meshes + d1.n_meshes); k.back().tri_offset += (uint32_t)step; x.meshes = k.data(); call(x, mm, nm); }
            { ctl_scene_desc x = d1; std::vector<ctl_woop_tri> w(d1.woop, d1.woop + d1.n_woop); w.back().a[3] += 0.25f; x.woop = w.data(); call(x, mm, nm); }          // changed values in a kept mesh
            { ctl_scene_desc x = d1; std::vector<ctl_woop_index> w(d1.woop_index, d1.woop_index + d1.n_woop); w.back().index ^= 2u; x.woop_index = w.data(); call(x, mm, nm); }   // changed structure
            { std::vector<uint32_t> m = mm; m.insert(m.begin(), kNodesNone); m.pop_back(); call(d1, m, nm); }                       // an appended mesh in front of a kept one
            try { update_nodes_flat_scene(h.F, h.basis, d1, nm.data(), (uint32_t)nm.size(), h.missing); } catch (const std::exception&) { refused++; }      // the older calls keep refusing
            try { update_meshes_flat_scene(h.F, h.basis, d1, nm.data(), (uint32_t)nm.size(), h.missing); } catch (const std::exception&) { refused++; }
            const size_t tris = b0.tri.size();
            try { b0.remove_mesh(3); } catch (const std::exception&) { refused++; }                                                  // a node still instances it
            try { b0.remove_mesh(kMeshes); } catch (const std::exception&) { refused++; }
            if (refused != 12 || h.F.leaves.size() != n0 || b0.tri.size() != tris || b0.meshes.size() != kMeshes) throw std::runtime_error("a refusal was not refused, or changed the handle or the builder");
            // the two removals
            update_mesh_set_flat_scene(h.F, h.basis, d1, mm.data(), (uint32_t)mm.size(), nm.data(), (uint32_t)nm.size(), h.missing); h.basis.fill(d1);
            check_tree(h.F, d1, "the first removal");
            maps_of(d1.n_meshes, d1.n_nodes, 1u << 0, b1, 0, 0, mm, nm);
            update_mesh_set_flat_scene(h.F, h.basis, d2, mm.data(), (uint32_t)mm.size(), nm.data(), (uint32_t)nm.size(), h.missing); h.basis.fill(d2);
            check_tree(h.F, d2, "the second removal");
        }
        std::printf("mesh removal host check ok\n");
        return 0;
    } catch (const std::exception& e) { std::fprintf(stderr, "mesh removal host check FAILED: %s\n", e.what()); return 1; }
}
