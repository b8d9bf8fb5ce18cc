// node_set_host_check.cpp — a stand-alone run of the host yardstick of ctl_scene_update_nodes (csrc/flat_nodes.cpp update_nodes_flat_scene) for a sanitizer build:
// the arrays of the test case N7 (tests/node_set_cases.py: two nodes removed and two added in one call) from a synthetic description made here, no fixture.
// tools/node_set_host_check.sh compiles it with flat_nodes.cpp and the host sources that needs, host code under -fsanitize=address,undefined, and runs it.
// Exit status 0 and "node set host check ok" when the updated tree holds one entry per triangle of the new node set and the refusals leave the handle as it was.
#include "scene_builder.h"
#include "flatten.h"
#include "flat_nodes.h"
#include "flat_rebuild.h"
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

using namespace ctl;

// the builder's one reference into a device source (volume_eval.hip); this program creates no medium
namespace ctl { void volume_update(ctl_volume&) { throw std::runtime_error("node_set_host_check: no media here"); } }

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

int main() {
    try {
        const uint32_t sizes[] = { 2, 1, 4, 12, 5, 63, 64, 5, 65, 257 };
        scene_builder b;
        std::vector<uint32_t> mesh;
        for (uint32_t k = 0; k < 10; k++) mesh.push_back(add_soup(b, sizes[k], 11 + k));
        for (int k = 0; k < 10; k++) { const ctl_float4x4 m = place(k); b.add_node(mesh[k], &m); }
        const float pos[3] = { 0.5f, 5.5f, -13.0f }, target[3] = { 0, 1.2f, 0 }, up[3] = { 0, 1, 0 }, light[3] = { 1, 9, -2 }, power[3] = { 90, 90, 90 };
        b.add_point_light(light, power);
        b.set_camera_lookat(pos, target, up, 55.0f, 32, 32);
        ctl_scene_desc d0{}; b.finalize(d0);
        flat_scene F;
        if (!flatten_scene(d0, F, (size_t)1 << 30, kFlatQ4)) throw std::runtime_error("nothing to flatten");
        hash_geometry(d0, F.refit.geom);
        node_set_basis basis; basis.fill(d0);
        const size_t n0 = F.leaves.size();
        // N7: nodes 3 and 5 removed, instances of meshes 5 and 9 added
        b.remove_node(3); b.remove_node(4);
        { const ctl_float4x4 m = place(12); b.add_node(mesh[5], &m); } { const ctl_float4x4 m = place(14); b.add_node(mesh[9], &m); }
        ctl_scene_desc d1{}; b.finalize(d1);
        const uint32_t map[10] = { 0, 1, 2, 4, 6, 7, 8, 9, kNodesNone, kNodesNone };
        std::vector<uint32_t> missing;
        // refusals first: the handle stays as it was
        const uint32_t bad[10] = { 0, 2, 1, 4, 6, 7, 8, 9, kNodesNone, kNodesNone };
        int refused = 0;
        try { update_nodes_flat_scene(F, basis, d1, bad, 10, missing); } catch (const std::exception&) { refused++; }
        try { update_nodes_flat_scene(F, basis, d1, map, 9, missing); } catch (const std::exception&) { refused++; }
        try { update_nodes_flat_scene(F, basis, d1, nullptr, 10, missing); } catch (const std::exception&) { refused++; }
        if (refused != 3 || F.leaves.size() != n0) throw std::runtime_error("a refusal was not refused, or changed the handle");
        update_nodes_flat_scene(F, basis, d1, map, 10, missing);
        size_t want = 0; for (uint32_t k = 0; k < 10; k++) if (k != 3 && k != 5) want += sizes[k];
        want += sizes[5] + sizes[9];
        std::vector<uint32_t> per_node(10, 0);
        for (const flat_leaf& L : F.leaves) { if (L.node >= 10) throw std::runtime_error("an entry names a node outside the scene"); per_node[L.node]++; }
        if (per_node[8] != sizes[5] || per_node[9] != sizes[9]) throw std::runtime_error("the added nodes have another number of entries than their meshes have triangles");
        if (F.leaves.size() < want || F.refit.part_index.size() != F.leaves.size() || F.refit.xf0.size() != 10 || F.nodes.empty() || F.refit.level_nodes.size() != F.nodes.size())
            throw std::runtime_error("the updated tree has the wrong sizes");
        // and what worked before works afterwards: a refit, a rebuild, the change undone by a second one
        basis.fill(d1);
        rebuild_flat_scene(F, d1, nullptr);
        b.remove_node(9); b.remove_node(8);
        ctl_scene_desc d2{}; b.finalize(d2);
        const uint32_t map2[8] = { 0, 1, 2, 3, 4, 5, 6, 7 };
        update_nodes_flat_scene(F, basis, d2, map2, 8, missing);
        std::printf("node set host check ok: %zu -> %zu entries, %zu nodes, depth %d\n", n0, F.leaves.size(), F.nodes.size(), F.max_depth);
        return 0;
    } catch (const std::exception& e) { std::fprintf(stderr, "node set host check FAILED: %s\n", e.what()); return 1; }
}
