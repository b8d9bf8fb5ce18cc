// image_update_host_check.cpp — a stand-alone run of the host half of the in-place image update for a sanitizer build: ctl_builder_update_image's builder code
// (csrc/scene_builder.cpp update_image / environment_tables over csrc/env_tables.h) and the pyramid ctl_mip_pyramid_host hands out (csrc/mip_pyramid.h over csrc/mip_texel.h).
// A plastic floor whose diffuse reflectance is image 0 under an environment map over image 1, made here, no fixture: builder A registers the images X and is updated to Y,
// builder B registers Y from the start; the two descriptions must agree byte for byte in materials, lights and anim blob.  Then the refusals, and the pyramid of odd, tiny
// and non-square images of both texel types into exactly-sized buffers.
// tools/image_update_host_check.sh compiles it with the host sources it needs, host code under -fsanitize=address,undefined, and runs it.
// Exit status 0 and "image update host check ok" when everything holds.
#include "scene_builder.h"
#include "mip_pyramid.h"
#include "geometry_hash.h"
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

using namespace ctl;

// the builder's one reference into a device source (volume_eval.hip); this program creates no medium
namespace ctl { void volume_update(ctl_volume&) { throw std::runtime_error("image_update_host_check: no media here"); } }

static std::vector<uint32_t> texels(uint32_t w, uint32_t h, uint32_t type, uint32_t seed) {
    std::mt19937 rng(seed); std::vector<uint32_t> t((size_t)w * h);
    for (auto& v : t) {
        const uint32_t m = rng() & 0xffffffu;
        // RGBE: mid-range exponents plus, one texel in eight each, exponent 0, exponents 1 .. 3 and 253 .. 255 (mantissas below 128 there: a 2 x 2 sum stays finite)
        uint32_t e = 110u + rng() % 30u; const uint32_t kind = rng() % 8u;
        if (kind == 0) e = 0; else if (kind == 1) e = 1u + rng() % 3u; else if (kind == 2) e = 253u + rng() % 3u;
        v = type == CTL_TEXEL_RGBE ? ((kind == 2 ? (m & 0x7f7f7fu) : m) | (e << 24)) : (m | (rng() << 24));
    }
    return t;
}
static std::vector<uint32_t> bright(uint32_t w, uint32_t h, uint32_t seed) {   // an environment map whose every texel has luminance
    std::mt19937 rng(seed); std::vector<uint32_t> t((size_t)w * h);
    for (auto& v : t) v = ((rng() & 0xffffffu) | 0x808080u) | ((126u + rng() % 6u) << 24);
    return t;
}

static void fill(scene_builder& b, const std::vector<uint32_t>& tex, uint32_t tw, uint32_t th, const std::vector<uint32_t>& env, uint32_t ew, uint32_t eh) {
    const uint32_t ti = b.add_image(tex.data(), tw, th, CTL_TEXEL_RGBCOL, CTL_WRAP_CLAMP, CTL_FILTER_TRILINEAR);
    const uint32_t ei = b.add_image(env.data(), ew, eh, CTL_TEXEL_RGBE, CTL_WRAP_REPEAT, CTL_FILTER_BILINEAR);
    ctl_material m{}; m.bsdf_type = CTL_BSDF_PLASTIC; m.node_light_index = 0xffffffffu;
    m.tex[0].type = CTL_TEX_IMAGE; m.tex[0].image = ti; m.tex[0].value[0] = m.tex[0].value[1] = m.tex[0].value[2] = 1.0f;
    m.tex[1].type = CTL_TEX_CONSTANT; m.tex[1].value[0] = m.tex[1].value[1] = m.tex[1].value[2] = 0.6f;
    const float P[12] = { -4, 0, -4, -4, 0, 4, 4, 0, 4, 4, 0, -4 }; const uint32_t I[6] = { 0, 1, 2, 0, 2, 3 };
    b.add_node(b.add_mesh(P, 4, I, 2, nullptr, nullptr, nullptr, &m, 1), nullptr);
    const float scale[3] = { 1.0f, 0.9f, 0.8f };
    b.set_environment_map(ei, scale, nullptr);
    const float pos[3] = { 0, 2, -8 }, tar[3] = { 0, 0, 0 }, up[3] = { 0, 1, 0 };
    b.set_camera_lookat(pos, tar, up, 45.0f, 16, 16);
}
static bool same(const ctl_scene_desc& a, const ctl_scene_desc& b) {
    return a.n_materials == b.n_materials && a.n_lights_buf == b.n_lights_buf && a.n_anim_bytes == b.n_anim_bytes &&
           std::memcmp(a.materials, b.materials, (size_t)a.n_materials * sizeof(ctl_material)) == 0 && std::memcmp(a.lights, b.lights, (size_t)a.n_lights_buf * sizeof(ctl_light)) == 0 &&
           std::memcmp(a.anim, b.anim, a.n_anim_bytes) == 0;
}
template <typename F> static bool refused(F f) { try { f(); } catch (const std::exception&) { return true; } return false; }

int main() {
    try {
        const uint32_t tw = 13, th = 9, ew = 67, eh = 33;
        const std::vector<uint32_t> X0 = texels(tw, th, CTL_TEXEL_RGBCOL, 1), Y0 = texels(tw, th, CTL_TEXEL_RGBCOL, 2), X1 = bright(ew, eh, 3), Y1 = bright(ew, eh, 4);
        scene_builder A, B; ctl_scene_desc da, db;
        A.bvh_mode = B.bvh_mode = CTL_BVH_BINNED;
        fill(A, X0, tw, th, X1, ew, eh); fill(B, Y0, tw, th, Y1, ew, eh);
        A.finalize(da); B.finalize(db);
        if (same(da, db)) throw std::runtime_error("the two image sets give the same description: the check would show nothing");
        A.update_image(0, Y0.data(), tw, th); A.update_image(1, Y1.data(), ew, eh);
        A.finalize(da);
        if (!same(da, db)) throw std::runtime_error("the updated builder's description differs from the one that had the images from the start");
        geometry_hashes ga, gb; hash_geometry(da, ga); hash_geometry(db, gb);
        if (!ga.same_structure(gb) || ga.images.size() != 4) throw std::runtime_error("the image digests of the two descriptions differ");
        // the refusals leave the builder as it was
        const std::vector<uint8_t> anim = A.anim; const std::vector<ctl_light> lights = A.lights; const std::vector<std::vector<uint32_t>> tx = A.image_texels;
        if (!refused([&] { A.update_image(2, Y0.data(), tw, th); }) || !refused([&] { A.update_image(0, nullptr, tw, th); }) || !refused([&] { A.update_image(0, Y0.data(), tw + 1, th); }) ||
            !refused([&] { A.update_image(1, Y1.data(), eh, ew); }) || !refused([&] { A.update_image(0xffffffffu, Y0.data(), tw, th); }))
            throw std::runtime_error("a refusal did not refuse");
        if (A.anim != anim || std::memcmp(A.lights.data(), lights.data(), lights.size() * sizeof(ctl_light)) != 0 || A.image_texels != tx) throw std::runtime_error("a refused call changed the builder");
        // the pyramid: level table and texel count by the rule, for both texel types
        const uint32_t sizes[][2] = { { 1, 1 }, { 2, 2 }, { 4, 2 }, { 5, 3 }, { 8, 8 }, { 64, 32 }, { 1, 7 }, { 33, 65 } };
        size_t total = 0;
        for (auto& s : sizes) for (uint32_t type : { (uint32_t)CTL_TEXEL_RGBE, (uint32_t)CTL_TEXEL_RGBCOL }) {
            const std::vector<uint32_t> t = texels(s[0], s[1], type, 7 + s[0]);
            ctl_mipmap m{}; m.texels = t.data(); m.width = s[0]; m.height = s[1]; m.texel_type = type;
            std::vector<uint32_t> pool; mip_level_table L;
            mip_pyramid_append(m, pool, L);
            size_t want = 0; uint32_t levels = 0;
            for (uint32_t w = s[0], h = s[1]; w && h; w >>= 1, h >>= 1, levels++) { if (levels && L.offsets[levels - 1] != want) throw std::runtime_error("level offset"); want += (size_t)w * h; }
            if (L.levels != levels || pool.size() != want || std::memcmp(pool.data(), t.data(), t.size() * 4) != 0) throw std::runtime_error("pyramid size or level 0");
            std::vector<uint32_t> out(pool);   // an exactly-sized copy, as ctl_mip_pyramid_host fills the caller's buffer
            float avg[3]; mip_image_average(m, avg);
            if (!(avg[0] >= 0.0f) || !(avg[1] >= 0.0f) || !(avg[2] >= 0.0f)) throw std::runtime_error("average");
            total += out.size();
        }
        std::printf("image update host check ok: %u lights, %u anim bytes, %zu pyramid texels\n", da.n_lights_buf, da.n_anim_bytes, total);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "image update host check FAILED: %s\n", e.what());
        return 1;
    }
}
