// ploc_host_check.cpp — a stand-alone run of the host twin of the rebuild (csrc/flat_rebuild.cpp rebuild_flat_scene) with BOTH builders for a sanitizer build: three
// synthetic descriptions made here, no fixture, in the manner of the test cases S1-M4 (sixty instances of a soup, every one moved to another's place), TW (two
// instances of one mesh under the same transform over a floor) and SAME (nine instances of a single triangle under one transform over a floor: every distance ties).
// tools/ploc_host_check.sh compiles it with flat_rebuild.cpp and the host sources that needs, host code under -fsanitize=address,undefined, and runs it.
// Exit status 0 and "ploc host check ok" when every rebuilt tree reaches every entry once, level by level, and PLOC's node area on the first scene is below the LBVH's.
#include "scene_builder.h"
#include "flatten.h"
#include "flat_rebuild.h"
#include "flat_ploc.h"
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

using namespace ctl;

// the builder's one reference into a device source (volume_eval.hip); this program creates no medium
namespace ctl { void volume_update(ctl_volume&) { throw std::runtime_error("ploc_host_check: no media here"); } }

static uint32_t add_soup(scene_builder& b, uint32_t n_tri, uint32_t seed, float size) {
    std::mt19937 rng(seed); std::uniform_real_distribution<float> u(-size, size);
    std::vector<float> P; std::vector<uint32_t> I;
    for (uint32_t t = 0; t < n_tri; t++) {
        const float c[3] = { 0.7f * (float)(t % 7), 0.6f * (float)((t / 7) % 7), 0.5f * (float)(t / 49) };
        for (int v = 0; v < 3; v++) { for (int k = 0; k < 3; k++) P.push_back(c[k] + u(rng)); I.push_back(3 * t + v); }
    }
    ctl_material m{}; m.bsdf_type = CTL_BSDF_DIFFUSE;
    return b.add_mesh(P.data(), n_tri * 3, I.data(), n_tri, nullptr, nullptr, nullptr, &m, 1);
}
static uint32_t add_floor(scene_builder& b) {
    const float P[12] = { -9, 0, -9, -9, 0, 9, 9, 0, 9, 9, 0, -9 }; const uint32_t I[6] = { 0, 1, 2, 0, 2, 3 };   // flat, as the tests' floors are
    ctl_material m{}; m.bsdf_type = CTL_BSDF_DIFFUSE;
    return b.add_mesh(P, 4, I, 2, nullptr, nullptr, nullptr, &m, 1);
}
static ctl_float4x4 place(int k, float scale) {
    ctl_float4x4 m{}; m.m[0] = m.m[5] = m.m[10] = scale; m.m[15] = 1.0f;
    m.m[3] = -8.0f + 5.1f * (float)(k % 6); m.m[7] = 0.3f + 4.3f * (float)((k / 6) % 5); m.m[11] = -3.0f + 4.7f * (float)(k / 30) + 0.1f * (float)k;
    return m;
}
static void finish(scene_builder& b, ctl_scene_desc& d) {
    const float pos[3] = { 0.5f, 5.5f, -13.0f }, target[3] = { 0, 1.2f, 0 }, up[3] = { 0, 1, 0 }, light[3] = { 1, 9, -2 }, power[3] = { 90, 90, 90 };
    b.add_point_light(light, power);
    b.set_camera_lookat(pos, target, up, 55.0f, 32, 32);
    b.finalize(d);
}

// every node and every entry once, in the order of the layout; leaves of 1 .. 4 entries closed by the last-entry bit
static void check_tree(const flat_scene& F, const std::string& what) {
    std::vector<uint32_t> level{ 0u };
    uint32_t next_node = 1, next_entry = 0; int depth = -1;
    while (!level.empty()) {
        std::vector<uint32_t> nxt; depth++;
        for (uint32_t i : level) {
            if (i >= F.nodes.size()) throw std::runtime_error(what + ": a link outside the nodes");
            const uint32_t exist = F.nodes[i].mask & 15u, leafm = (F.nodes[i].mask >> 4) & exist;
            for (int c = 0; c < 4; c++) {
                if (!((exist >> c) & 1u)) continue;
                const int32_t k = F.child_links[(size_t)i * 4 + c];
                if ((leafm >> c) & 1u) {
                    if ((uint32_t)~k != next_entry) throw std::runtime_error(what + ": leaf entries out of order");
                    uint32_t cnt = 0;
                    for (;;) { if (next_entry >= F.leaves.size() || ++cnt > 4u) throw std::runtime_error(what + ": a leaf that does not close"); if (F.leaves[next_entry++].index & 1u) break; }
                } else { if (k < 0 || (uint32_t)k / 4u != next_node) throw std::runtime_error(what + ": inner children out of order"); nxt.push_back(next_node++); }
            }
        }
        level.swap(nxt);
    }
    if (next_node != F.nodes.size() || next_entry != F.leaves.size() || depth != F.max_depth) throw std::runtime_error(what + ": not every node or entry is reached, or another depth");
}

static double run(const ctl_scene_desc& d0, const ctl_scene_desc& d1, int builder, const std::string& what, uint32_t* rounds) {
    flat_scene F;
    if (!flatten_scene(d0, F, (size_t)1 << 30, kFlatQ4)) throw std::runtime_error("nothing to flatten");
    hash_geometry(d0, F.refit.geom);
    const size_t n = F.leaves.size();
    double area[2] = { 0, 0 };
    rebuild_flat_scene(F, d1, area, builder);
    *rounds = rebuild_last_rounds();
    if (F.leaves.size() != n || F.refit.part_index.size() != n) throw std::runtime_error(what + ": the entry count changed");
    check_tree(F, what);
    refit_flat_scene(F, d0, nullptr);                       // what worked before works afterwards: a refit, and a rebuild by the other builder
    rebuild_flat_scene(F, d1, nullptr, builder == CTL_REBUILD_PLOC ? CTL_REBUILD_LBVH : CTL_REBUILD_PLOC);
    check_tree(F, what + " (then the other builder)");
    return area[1];
}

int main() {
    try {
        const char* names[2] = { "LBVH", "PLOC" };
        double s1_area[2] = { 0, 0 };
        for (int scene = 0; scene < 3; scene++) {
            for (int builder = 0; builder < 2; builder++) {
                // a description points into its builder: the pose the tree is built from and the pose it is rebuilt for come from two builders of the same scene
                scene_builder b0, b1;
                ctl_scene_desc d0{}, d1{};
                for (int moved = 0; moved < 2; moved++) {
                    scene_builder& b = moved ? b1 : b0;
                    if (scene == 0) {          // S1-M4
                        const uint32_t mesh = add_soup(b, 257, 5, 0.3f);
                        b.add_node(add_floor(b), nullptr);
                        for (int k = 0; k < 60; k++) { const ctl_float4x4 m = place(moved ? (k + 17) % 60 : k, 0.8f + 0.01f * (float)k); b.add_node(mesh, &m); }
                    } else {                   // TW, SAME
                        const uint32_t mesh = scene == 1 ? add_soup(b, 80, 9, 0.3f) : add_soup(b, 1, 3, 0.4f);
                        b.add_node(add_floor(b), nullptr);
                        const ctl_float4x4 m = moved ? place(8, 2.4f) : place(3, 1.7f);
                        for (int k = 0; k < (scene == 1 ? 2 : 9); k++) b.add_node(mesh, &m);
                    }
                    finish(b, moved ? d1 : d0);
                }
                uint32_t rounds = 0;
                const std::string what = std::string(scene == 0 ? "S1-M4" : scene == 1 ? "TW" : "SAME") + " " + names[builder];
                const double area = run(d0, d1, builder, what, &rounds);
                if ((builder == CTL_REBUILD_PLOC) != (rounds > 0)) throw std::runtime_error(what + ": the round count does not fit the builder");
                if (scene == 0) s1_area[builder] = area;
                std::printf("%s: node area %.6g, %u rounds\n", what.c_str(), area, rounds);
            }
        }
        if (!(s1_area[1] < s1_area[0])) throw std::runtime_error("PLOC's node area is not below the LBVH's");
        std::printf("ploc host check ok\n");
        return 0;
    } catch (const std::exception& e) { std::fprintf(stderr, "ploc host check FAILED: %s\n", e.what()); return 1; }
}
