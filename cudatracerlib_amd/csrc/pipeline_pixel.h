// pipeline_pixel.h — what the image-pipeline kernels share per pixel (image_pipeline.hip, nlm_filter.hip): PixelData -> Spectrum and the RGBE
// encoding of the filtered plane
#pragma once
#include "kernels.h"

namespace ctl {

__device__ __forceinline__ f3 to_spectrum(const ctl_pixel_data& p, float splat_scale) {   // PixelData::toSpectrum (Engine/Image.h:21-28)
    const float r = 1.0f / (p.weight_sum != 0 ? p.weight_sum : 1);   // Spectrum / scalar multiplies by the reciprocal (Math/Spectrum.h:122-128): not the quotient's rounding
    return f3(p.rgb[0] * r + p.rgb_splat[0] * splat_scale, p.rgb[1] * r + p.rgb_splat[1] * splat_scale, p.rgb[2] * r + p.rgb_splat[2] * splat_scale);
}
// SpectrumConverter::Float3ToRGBE / RGBEToFloat3 (Math/Spectrum.h:534-565)
__device__ __forceinline__ uint32_t to_rgbe(f3 c) {
    float m = max2(max2(c.x, c.y), c.z);
    // a NaN or infinite maximum encodes as word 0: the reference's frexp_self leaves the exponent unwritten there, so it defines no bits
    if (!(m >= 1e-32f) || m > 3.402823466e+38f) return 0u;
    int e; m = (float)frexp((double)m, &e) * 256.0f / m;
    // float -> unsigned char saturates on the reference's device (negative lobes of the Mitchell / Lanczos filters reach here): say so explicitly
    auto u8 = [](float v) { return (uint32_t)min2(max2(v, 0.0f), 255.0f); };
    return u8(c.x * m) | (u8(c.y * m) << 8) | (u8(c.z * m) << 16) | ((uint32_t)(unsigned char)(e + 128) << 24);
}
__device__ __forceinline__ f3 from_rgbe(uint32_t v) {
    const uint32_t w = v >> 24;
    if (!w) return f3(0.0f);
    const float e = ldexpf(1.0f, (int)w - (128 + 8));
    return f3((v & 0xff) * e, ((v >> 8) & 0xff) * e, ((v >> 16) & 0xff) * e);
}

} // namespace ctl
