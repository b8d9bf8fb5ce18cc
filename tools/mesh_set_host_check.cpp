// mesh_set_host_check.cpp — a stand-alone run of the host side of ctl_scene_update_meshes (csrc/flat_meshes.cpp: the acceptance check of plan_node_set, the host
// re-statement of k_append_leaf_rows, update_meshes_flat_scene) for a sanitizer build, over the shapes of tests/mesh_set_cases.py: meshes of 1, 5, 64, 65 and 257
// triangles appended in two calls, one of them instanced twice, one never, together with a node removed; synthetic descriptions made here, no fixture.
// tools/mesh_set_host_check.sh compiles it with the host sources it needs, host code under -fsanitize=address,undefined, and runs it.
// Exit status 0 and "mesh set host check ok" when the table equals triangle_woop_rows of the new description, the updated tree holds one entry per triangle of the new
// node set, and the refusals leave the handle as it was.
#include "scene_builder.h"
#include "flatten.h"
#include "flat_nodes.h"
#include "flat_meshes.h"
#include "flat_rebuild.h"
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

using namespace ctl;

// the builder's one reference into a device source (volume_eval.hip); this program creates no medium
namespace ctl { void volume_update(ctl_volume&) { throw std::runtime_error("mesh_set_host_check: no media here"); } }

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

static const uint32_t kBase[] = { 2, 1, 4, 12, 5, 63 };
// a description points into its builder: one builder per description, each replaying the steps before it.  step 0: the base; 1: + a 1-triangle mesh and its node;
// 2: + meshes of 5, 64, 65, 257 triangles, the first instanced twice, the second never, and base node 3 removed
static void build(scene_builder& b, int steps, ctl_scene_desc& d) {
    std::vector<uint32_t> mesh;
    for (uint32_t k = 0; k < 6; k++) mesh.push_back(add_soup(b, kBase[k], 11 + k));
    for (int k = 0; k < 6; k++) node(b, mesh[k], k);
    const float pos[3] = { 0.5f, 5.5f, -13.0f }, target[3] = { 0, 1.2f, 0 }, up[3] = { 0, 1, 0 }, light[3] = { 1, 9, -2 }, power[3] = { 90, 90, 90 };
    b.add_point_light(light, power);
    b.set_camera_lookat(pos, target, up, 55.0f, 32, 32);
    b.finalize(d);
    if (steps >= 1) { node(b, add_soup(b, 1, 40), 7); b.finalize(d); }
    if (steps >= 2) {
        const uint32_t a5 = add_soup(b, 5, 41); add_soup(b, 64, 42); const uint32_t a65 = add_soup(b, 65, 43), a257 = add_soup(b, 257, 44);
        b.remove_node(3);
        node(b, a5, 8); node(b, a5, 9); node(b, a65, 10); node(b, a257, 11);
        b.finalize(d);
    }
}

int main() {
    try {
        scene_builder b0, b1, b2;
        ctl_scene_desc d0{}, d1{}, d2{};
        build(b0, 0, d0); build(b1, 1, d1); build(b2, 2, d2);
        flat_scene F;
        if (!flatten_scene(d0, F, (size_t)1 << 30, kFlatQ4)) throw std::runtime_error("nothing to flatten");
        hash_geometry(d0, F.refit.geom);
        node_set_basis basis; basis.fill(d0);
        const size_t n0 = F.leaves.size();
        std::vector<uint32_t> missing;
        const uint32_t map1[7] = { 0, 1, 2, 3, 4, 5, kNodesNone };
        const uint32_t map2[10] = { 0, 1, 2, 4, 5, 6, kNodesNone, kNodesNone, kNodesNone, kNodesNone };
        // the table, step by step, against triangle_woop_rows
        std::vector<uint32_t> table, want_table;
        triangle_woop_rows(d0, table);
        const ctl_scene_desc* seq[3] = { &d0, &d1, &d2 };
        for (int s = 1; s < 3; s++) {
            mesh_set_plan P; plan_mesh_growth(seq[s - 1]->n_meshes, seq[s - 1]->n_tri_data, seq[s - 1]->n_woop, seq[s - 1]->n_bvh_nodes, *seq[s], "check: ", P);
            table.resize(seq[s]->n_tri_data, 0u);
            std::vector<uint32_t> rows((size_t)P.rows_added * 16);
            append_leaf_rows_host(*seq[s], P, rows.data(), table.data());
            triangle_woop_rows(*seq[s], want_table);
            if (table != want_table) throw std::runtime_error("the extended table is not triangle_woop_rows of the new description");
            for (uint32_t w = 0; w < P.rows_added; w++)
                if (std::memcmp(&rows[(size_t)w * 16], &seq[s]->woop[P.old_woop + w], 48) != 0 || rows[(size_t)w * 16 + 12] != seq[s]->woop_index[P.old_woop + w].index) throw std::runtime_error("an appended row is not creation's interleave");
        }
        // refusals first: the handle stays as it was
        int refused = 0;
        try { update_meshes_flat_scene(F, basis, d1, map1, 6, missing); } catch (const std::exception&) { refused++; }          // a short map
        try { update_meshes_flat_scene(F, basis, d1, nullptr, 7, missing); } catch (const std::exception&) { refused++; }
        try { update_nodes_flat_scene(F, basis, d1, map1, 7, missing); } catch (const std::exception&) { refused++; }           // the node-set call keeps refusing appended meshes
        { ctl_scene_desc x = d1; std::vector<ctl_kernel_mesh> m(d1.meshes, d1.meshes + d1.n_meshes); m.back().tri_offset = d0.n_tri_data - 1; x.meshes = m.data();
          try { update_meshes_flat_scene(F, basis, x, map1, 7, missing); } catch (const std::exception&) { refused++; } }
        { ctl_scene_desc x = d1; x.n_woop = d0.n_woop - 1; try { update_meshes_flat_scene(F, basis, x, map1, 7, missing); } catch (const std::exception&) { refused++; } }
        { ctl_scene_desc x = d1; std::vector<ctl_woop_tri> w(d1.woop, d1.woop + d1.n_woop); w[0].a[3] += 0.25f; x.woop = w.data();
          try { update_meshes_flat_scene(F, basis, x, map1, 7, missing); } catch (const std::exception&) { refused++; } }
        if (refused != 6 || F.leaves.size() != n0) throw std::runtime_error("a refusal was not refused, or changed the handle");
        // the two calls
        update_meshes_flat_scene(F, basis, d1, map1, 7, missing); basis.fill(d1);
        if (F.leaves.size() < n0 + 1) throw std::runtime_error("the first call made no entry for the appended mesh");
        update_meshes_flat_scene(F, basis, d2, map2, 10, missing); basis.fill(d2);
        std::vector<uint32_t> per_node(10, 0);
        for (const flat_leaf& L : F.leaves) { if (L.node >= 10) throw std::runtime_error("an entry names a node outside the scene"); per_node[L.node]++; }
        if (per_node[5] != 1 || per_node[6] != 5 || per_node[7] != 5 || per_node[8] != 65 || per_node[9] != 257) throw std::runtime_error("the added nodes have another number of entries than their meshes have triangles");
        if (F.refit.part_index.size() != F.leaves.size() || F.refit.xf0.size() != 10 || F.nodes.empty() || F.refit.level_nodes.size() != F.nodes.size()) throw std::runtime_error("the updated tree has the wrong sizes");
        // nothing appended: the node-set call's own path; and what worked before works afterwards
        const uint32_t same[10] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9 };
        update_meshes_flat_scene(F, basis, d2, same, 10, missing);
        rebuild_flat_scene(F, d2, nullptr);
        std::printf("mesh set host check ok: %zu -> %zu entries, %zu nodes, depth %d\n", n0, F.leaves.size(), F.nodes.size(), F.max_depth);
        return 0;
    } catch (const std::exception& e) { std::fprintf(stderr, "mesh set host check FAILED: %s\n", e.what()); return 1; }
}
