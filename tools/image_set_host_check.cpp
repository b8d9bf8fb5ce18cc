// image_set_host_check.cpp — a stand-alone run of the host half of the image-set edit for a sanitizer build: the builder's remove_image / replace_image / set_material
// (csrc/scene_builder.cpp), the acceptance check with its pool layout and run table (csrc/scene_image_set.cpp plan_image_set) and the kernel's arithmetic on the host
// (move_texels_host over csrc/scene_image_set.h).  A floor whose plastic reads one of seven images of mixed sizes and texel types, made here, no fixture: builder A removes
// every second image, replaces one by another size and appends one; builder B registers the final set from the start; the two descriptions must agree byte for byte.  The
// plan of the edit moves the kept pyramids from a pool laid out by mip_pyramid_append into an exactly-sized new pool, which must equal B's own pool outside the fresh slots;
// tables whose sizes lie must not reach outside the pools.  Then the refusals.
// tools/image_set_host_check.sh compiles it with the host sources it needs, host code under -fsanitize=address,undefined, and runs it.
// Exit status 0 and "image set host check ok" when everything holds.
#include "scene_builder.h"
#include "scene_image_set.h"
#include "geometry_hash.h"
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

using namespace ctl;

// the builder's one reference into a device source (volume_eval.hip); this program creates no medium
namespace ctl { void volume_update(ctl_volume&) { throw std::runtime_error("image_set_host_check: no media here"); } }

struct image_spec { uint32_t w, h, type, seed; };

static std::vector<uint32_t> texels(const image_spec& s) {
    std::mt19937 rng(s.seed); std::vector<uint32_t> t((size_t)s.w * s.h);
    for (auto& v : t) { const uint32_t m = rng() & 0xffffffu; v = s.type == CTL_TEXEL_RGBE ? (m | ((120u + rng() % 16u) << 24)) : (m | 0xff000000u); }
    return t;
}
static uint32_t add(scene_builder& b, const image_spec& s) { const std::vector<uint32_t> t = texels(s); return b.add_image(t.data(), s.w, s.h, s.type, CTL_WRAP_REPEAT, CTL_FILTER_TRILINEAR); }

// the floor reads image `read`
static void fill(scene_builder& b, const std::vector<image_spec>& images, uint32_t read) {
    for (const image_spec& s : images) add(b, s);
    ctl_material m{}; m.bsdf_type = CTL_BSDF_PLASTIC; m.node_light_index = 0xffffffffu;
    m.tex[0].type = CTL_TEX_IMAGE; m.tex[0].image = read; m.tex[0].value[0] = m.tex[0].value[1] = m.tex[0].value[2] = 1.0f;
    m.tex[1].type = CTL_TEX_CONSTANT; m.tex[1].value[0] = m.tex[1].value[1] = m.tex[1].value[2] = 0.6f;
    const float P[12] = { -4, 0, -4, -4, 0, 4, 4, 0, 4, 4, 0, -4 }; const uint32_t I[6] = { 0, 1, 2, 0, 2, 3 };
    b.add_node(b.add_mesh(P, 4, I, 2, nullptr, nullptr, nullptr, &m, 1), nullptr);
    const float pos[3] = { 0, 2, -8 }, tar[3] = { 0, 0, 0 }, up[3] = { 0, 1, 0 };
    b.set_camera_lookat(pos, tar, up, 45.0f, 16, 16);
}
static bool same(const ctl_scene_desc& a, const ctl_scene_desc& b) {
    if (a.n_materials != b.n_materials || a.n_lights_buf != b.n_lights_buf || a.n_anim_bytes != b.n_anim_bytes || a.n_images != b.n_images) return false;
    if (std::memcmp(a.materials, b.materials, (size_t)a.n_materials * sizeof(ctl_material)) != 0) return false;
    for (uint32_t i = 0; i < a.n_images; i++) {
        const ctl_mipmap &x = a.images[i], &y = b.images[i];
        if (x.width != y.width || x.height != y.height || x.texel_type != y.texel_type || x.wrap_mode != y.wrap_mode || x.filter_mode != y.filter_mode) return false;
        if (std::memcmp(x.texels, y.texels, (size_t)x.width * x.height * 4) != 0) return false;
    }
    return true;
}
static std::vector<uint32_t> pool_of(const ctl_scene_desc& d) {
    std::vector<uint32_t> pool; mip_level_table L;
    for (uint32_t i = 0; i < d.n_images; i++) mip_pyramid_append(d.images[i], pool, L);
    return pool;
}
template <typename F> static bool refused(F f) { try { f(); } catch (const std::exception&) { return true; } return false; }

int main() {
    try {
        const std::vector<image_spec> start = { { 1, 1, CTL_TEXEL_RGBCOL, 1 }, { 2, 2, CTL_TEXEL_RGBE, 2 }, { 4, 2, CTL_TEXEL_RGBCOL, 3 }, { 5, 3, CTL_TEXEL_RGBE, 4 },
                                                { 8, 8, CTL_TEXEL_RGBCOL, 5 }, { 64, 32, CTL_TEXEL_RGBE, 6 }, { 13, 9, CTL_TEXEL_RGBCOL, 7 } };
        const image_spec bigger = { 33, 17, CTL_TEXEL_RGBCOL, 8 }, extra = { 5, 3, CTL_TEXEL_RGBE, 9 };
        scene_builder A, H, B; ctl_scene_desc da, dh, db;
        A.bvh_mode = H.bvh_mode = B.bvh_mode = CTL_BVH_BINNED;
        fill(A, start, 6); fill(H, start, 6);      // H: the description a scene would hold
        A.finalize(da); H.finalize(dh);
        // the edit: images 5, 3 and 1 leave, image 4 -> index 2 is replaced by another size, one image is appended, the floor is repointed to it
        if (!refused([&] { A.remove_image(6); }) || !refused([&] { A.remove_image(7); })) throw std::runtime_error("a referenced or missing image was removed");
        A.remove_image(5); A.remove_image(3); A.remove_image(1);
        { const std::vector<uint32_t> t = texels(bigger); A.replace_image(2, t.data(), bigger.w, bigger.h); }
        const uint32_t appended = add(A, extra);
        ctl_material m = A.material(da.nodes[0].material_offset); m.tex[0].image = appended; A.set_material(da.nodes[0].material_offset, m);
        if (!refused([&] { A.remove_image(appended); })) throw std::runtime_error("the image the floor reads now was removed");
        A.finalize(da);
        const std::vector<image_spec> final_set = { start[0], start[2], bigger, start[6], extra };
        fill(B, final_set, 4); B.finalize(db);
        if (!same(da, db)) throw std::runtime_error("the edited builder's description differs from the one that had the final images from the start");
        // the plan and the move
        const uint32_t map[5] = { 0, 2, kNodesNone, 6, kNodesNone };
        node_set_basis basis; basis.fill(dh);
        geometry_hashes held; hash_geometry(dh, held);
        image_set_plan plan; plan_image_set(basis, held, da, map, 5, nullptr, plan, "image_set_host_check");
        const std::vector<uint32_t> old_pool = pool_of(dh), want = pool_of(db);
        if (plan.total != want.size() || plan.old_total != old_pool.size() || plan.n_runs() != 3 || plan.kept != 3 || plan.fresh != 2 || plan.removed != 4) throw std::runtime_error("the plan's counts");
        const uint32_t mark = 0xdeadbeefu;
        std::vector<uint32_t> pool(plan.total, mark);     // exactly sized: a write past the end is the sanitizer's
        move_texels_host(old_pool.data(), old_pool.size(), plan.runs.data(), plan.n_runs(), pool.data(), pool.size());
        uint64_t moved = 0;
        for (uint32_t j = 0; j < 5; j++) {
            const uint64_t end = j + 1 < 5 ? plan.offsets[j + 1] : plan.total;
            for (uint64_t t = plan.offsets[j]; t < end; t++) {
                if (map[j] == kNodesNone ? pool[t] != mark : pool[t] != want[t]) throw std::runtime_error("the moved pool differs from a fresh one in image " + std::to_string(j));
                if (map[j] != kNodesNone) moved++;
            }
        }
        if (moved != plan.texels_moved) throw std::runtime_error("texels moved");
        // tables whose sizes lie: shorter pools than the table speaks of, a table without runs
        std::vector<uint32_t> short_old(old_pool.begin(), old_pool.end() - 40), short_new(plan.total - 30, mark);
        move_texels_host(short_old.data(), short_old.size(), plan.runs.data(), plan.n_runs(), short_new.data(), short_new.size());
        move_texels_host(old_pool.data(), old_pool.size(), plan.runs.data() + plan.n_runs(), 0, pool.data(), pool.size());
        // the refusals of the plan
        const uint32_t bad_short[4] = { 0, 2, kNodesNone, 6 }, bad_order[5] = { 2, 0, kNodesNone, 6, kNodesNone }, bad_range[5] = { 0, 2, 7, kNodesNone, kNodesNone }, bad_size[5] = { 0, 2, 4, 6, kNodesNone };
        image_set_plan p2;
        if (!refused([&] { plan_image_set(basis, held, da, bad_short, 4, nullptr, p2, "check"); }) || !refused([&] { plan_image_set(basis, held, da, bad_order, 5, nullptr, p2, "check"); }) ||
            !refused([&] { plan_image_set(basis, held, da, bad_range, 5, nullptr, p2, "check"); }) || !refused([&] { plan_image_set(basis, held, da, bad_size, 5, nullptr, p2, "check"); }) ||
            !refused([&] { plan_image_set(basis, held, da, nullptr, 5, nullptr, p2, "check"); }))
            throw std::runtime_error("a refusal of the plan did not refuse");
        std::printf("image set host check ok: %u runs, %llu texels moved, %llu of %llu texels in the new pool\n", plan.n_runs(), (unsigned long long)plan.texels_moved, (unsigned long long)moved, (unsigned long long)plan.total);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "image set host check FAILED: %s\n", e.what());
        return 1;
    }
}
