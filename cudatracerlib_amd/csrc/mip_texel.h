// mip_texel.h — the per-texel arithmetic of KernelMIPMap's pyramid (MIPMap::CompileToBinary, Engine/MIPMap.cpp:41-95), single source for the host builder of the pyramid
// (mip_pyramid.h), the scene builder's environment tables (env_tables.h) and the device (scene_images.hip), in the style of shape_set.h: decode a texel, average a 2x2
// block in the reference's order, encode it again.  fp32 +, *, / in the order written (the library is built -ffp-contract=off on both sides); the power of two of an RGBE
// exponent comes from ldexp, which is exact.
//
// What the encoders see here is never negative, NaN or infinite: a decoded texel is a byte times a power of two (RGBE) or a byte / 255 (RGBCOL), and a box average of such
// values is inside their range.  For an RGBE texel the scale frexp(max) * 256 / max is a power of two, so every product is exact and below 256: the conversion to a byte
// never saturates, and the host's and the device's conversions agree.
#pragma once
#include "ctl_math.h"
#include <cmath>
#include <cstdint>

namespace ctl {

// the texel-type constants of include/ctl_amd.h (CTL_TEXEL_RGBE = 0, CTL_TEXEL_RGBCOL = 1), for sources that take no `type` from a ctl_mipmap
constexpr uint32_t kTexelRgbe = 0u, kTexelRgbcol = 1u;

HD void mip_texel_decode(uint32_t v, uint32_t type, float c[3]) {   // Spectrum::fromRGBE / fromRGBCOL (Math/Spectrum.cu:260-284)
    const uint32_t x = v & 0xff, y = (v >> 8) & 0xff, z = (v >> 16) & 0xff, w = v >> 24;
    if (type == kTexelRgbe) { if (!w) { c[0] = c[1] = c[2] = 0; return; } const float e = ldexpf(1.0f, (int)w - (128 + 8)); c[0] = x * e; c[1] = y * e; c[2] = z * e; }
    else { c[0] = float(x) / 255.0f; c[1] = float(y) / 255.0f; c[2] = float(z) / 255.0f; }
}
HD uint32_t mip_texel_to_rgbe(float r, float g, float b) {   // SpectrumConverter::Float3ToRGBE (Math/Spectrum.h:534-555) = image_io.h float3_to_rgbe
    float max_ = r > g ? r : g; max_ = max_ > b ? max_ : b;   // std::max(r, std::max(g, b)) over values that are no NaN
    if (max_ < 1e-32) return 0;
    int e;
    max_ = (float)frexp((double)max_, &e) * 256.0f / max_;
    const uint32_t x = (uint32_t)(r * max_) & 0xffu, y = (uint32_t)(g * max_) & 0xffu, z = (uint32_t)(b * max_) & 0xffu, w = (uint32_t)(e + 128) & 0xffu;
    return x | (y << 8) | (z << 16) | (w << 24);
}
HD uint32_t mip_texel_to_rgbcol(float r, float g, float b) {   // SpectrumConverter::Float3ToCOLORREF (Math/Spectrum.h:521-526) = image_io.h float3_to_rgbcol
    auto to_int = [](float x) { const float c = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); return (uint32_t)(c * 255.0f) & 0xffu; };
    return to_int(r) | (to_int(g) << 8) | (to_int(b) << 16) | (255u << 24);
}
// one texel of level l from the four of level l - 1 under it: a = (2x, 2y), b = (2x + 1, 2y), c = (2x, 2y + 1), e = (2x + 1, 2y + 1); the sum is ((a + b) + c) + e
HD uint32_t mip_texel_box(uint32_t a, uint32_t b, uint32_t c, uint32_t e, uint32_t type) {
    float fa[3], fb[3], fc[3], fe[3], v[3];
    mip_texel_decode(a, type, fa); mip_texel_decode(b, type, fb); mip_texel_decode(c, type, fc); mip_texel_decode(e, type, fe);
    for (int q = 0; q < 3; q++) { float s2 = fa[q] + fb[q]; s2 = s2 + fc[q]; s2 = s2 + fe[q]; v[q] = 0.25f * s2; }
    return type == kTexelRgbe ? mip_texel_to_rgbe(v[0], v[1], v[2]) : mip_texel_to_rgbcol(v[0], v[1], v[2]);
}
// the number of levels of a w x h image, 1 + floor(log2(min(w, h))), at most 16 (mip_level_table holds 15 offsets)
HD uint32_t mip_level_count(uint32_t w, uint32_t h) {
    uint32_t levels = 1;
    for (uint32_t mn = w < h ? w : h; (mn >>= 1) && levels < 16;) levels++;
    return levels;
}

}  // namespace ctl
