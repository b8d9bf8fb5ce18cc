// mip_pyramid.h — host side of KernelMIPMap's pyramid: the levels behind level 0 as MIPMap::CompileToBinary builds them (Engine/MIPMap.cpp:41-95: nLevels = 1 + log2(min(w, h)),
// level i = the 2x2 box average of level i-1 — decoded, summed in the reference's order, scaled by 0.25 and re-encoded in the image's texel type), and what
// ImageTexture::Average() reads off it (SceneTypes/Texture.cu:31-37: getTexture().Sample(Vec2f(0), 1) = Texel(nLevels - 1, (0, 0)), Engine/MIPMap.cu:140-146, :21-44).
// Used by the device scene (tracer.hip: the texel pool of the filtered first-hit lookups) and by the scene builder (BSDF::Update() of models whose sampling weights
// come from texture averages, scene_builder.cpp finalize = the reference's UpdateMaterialsPhase2, Engine/DynamicScene.cpp:84-89).
#pragma once
#include "../../include/ctl_amd.h"
#include "mip_texel.h"   // the per-texel arithmetic (decode, 2x2 box, encode), which the device runs too
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace ctl {

struct mip_level_table { uint32_t levels; uint32_t offsets[15]; };   // = dev_mip_levels (device_scene.h): texel offsets of levels 1.. relative to the image's level 0

// appends level 0 and the pyramid of `m` to `pool`; returns the offset of level 0 in the pool
inline size_t mip_pyramid_append(const ctl_mipmap& m, std::vector<uint32_t>& pool, mip_level_table& L) {
    const size_t base = pool.size();
    pool.insert(pool.end(), m.texels, m.texels + (size_t)m.width * m.height);
    std::memset(&L, 0, sizeof(L)); L.levels = mip_level_count(m.width, m.height);
    uint32_t o = m.width * m.height, pw = m.width; size_t prev = base;
    for (uint32_t l = 1, j = m.width / 2, k = m.height / 2; l < L.levels; l++, j >>= 1, k >>= 1) {
        L.offsets[l - 1] = o; pool.resize(base + o + (size_t)j * k);
        for (uint32_t t = 0; t < k; t++) for (uint32_t x = 0; x < j; x++) {
            const uint32_t* r0 = &pool[prev + (size_t)(2 * t) * pw + 2 * x]; const uint32_t* r1 = r0 + pw;
            pool[base + o + (size_t)t * j + x] = mip_texel_box(r0[0], r0[1], r1[0], r1[1], m.texel_type);   // mip_texel.h
        }
        prev = base + o; pw = j; o += j * k;
    }
    return base;
}

// KernelMIPMap::Sample(Vec2f(0), 1) of the image's pyramid: the texel of the coarsest level that uv = (0, 0) addresses (WrapCoordinates, Engine/MIPMap_device.h:33-55:
// REPEAT / MIRROR / BLACK -> (0, 0); CLAMP -> x = 0, y = clamp01(1 - 0) * h = the last row)
// (the offset of that texel relative to the image's level 0: what a scene reads back after ctl_scene_update_image, scene_images.hip)
inline size_t mip_average_texel_offset(const ctl_mipmap& m, const mip_level_table& L) {
    const uint32_t level = L.levels - 1, wl = m.width >> level, hl = m.height >> level;
    const uint32_t y = m.wrap_mode == CTL_WRAP_CLAMP ? hl - 1 : 0u;
    return (level ? L.offsets[level - 1] : 0u) + (size_t)y * wl;
}
inline void mip_image_average(const ctl_mipmap& m, float rgb[3]) {
    rgb[0] = rgb[1] = rgb[2] = 0.0f;
    if (!m.texels || !m.width || !m.height) return;
    std::vector<uint32_t> pool; mip_level_table L;
    mip_pyramid_append(m, pool, L);
    mip_texel_decode(pool[mip_average_texel_offset(m, L)], m.texel_type, rgb);
}

} // namespace ctl
