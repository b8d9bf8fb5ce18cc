// env_tables.h — the sampling tables of the environment light (InfiniteLight::InfiniteLight, SceneTypes/Light.cpp:10-61): the arithmetic, single source for the scene
// builder (scene_builder::environment_tables: ctl_builder_set_environment_map, ctl_builder_update_image) and the device (scene_images.hip: ctl_scene_update_image), in the
// style of shape_set.h.  fp32 +, *, / in the order written (the library is built -ffp-contract=off on both sides).
//
//   cdfCols   H rows of W + 1 floats.  Row y: entry 0 = 0, entry x + 1 = the RUNNING fp32 sum of the luminances of texels 0 .. x of image row y (colSum after the last);
//             then entries 1 .. W - 1 are multiplied by 1 / colSum and entry W is set to 1.  The sum is serial, in x order: fp32 addition is not associative, and a CDF that
//             differs in its last bit picks another texel for some samples.
//   cdfRows   H + 1 floats: entry 0 = 0, entry y + 1 = the running sum of colSum(y) * rowWeights[y] (rowSum after the last); then entries 1 .. H - 1 times 1 / rowSum, entry H = 1.
//   rowWeights[y] = sin((y + 0.5) pi / H): depends on the height only — made once, by ctl_builder_set_environment_map
//   normalization = 1 / (rowSum * (2 pi / W) * (pi / H)), in the light record
// A row without luminance gives 1 / 0 = inf and 0 * inf = NaN entries, as in the reference; the payload of such a NaN is the one thing host and device may differ in.
#pragma once
#include "mip_texel.h"

namespace ctl {

HD float env_texel_luminance(uint32_t texel, uint32_t type) {
    float c[3]; mip_texel_decode(texel, type, c);
    return c[0] * 0.212671f + c[1] * 0.715160f + c[2] * 0.072169f;   // Spectrum::getLuminance (Spectrum.cu:174-177)
}
// n steps of a running sum: out[i] = the sum after term(i) was added, i = 0 .. n - 1; returns it.  The columns of one image row (term = a texel's luminance, carry = 0 at
// x = 0), in pieces where the caller stages the row, and the rows (term(y) = colSum(y) * rowWeights[y])
template <typename TERM> HD float env_running_sum(TERM term, uint32_t n, float carry, float* out) {
    for (uint32_t i = 0; i < n; i++) { carry += term(i); out[i] = carry; }
    return carry;
}
// entry i of a row of n + 1 entries after the normalisation: entry 0 stays (it is 0), entries 1 .. n - 1 are scaled by inv = 1 / sum, entry n is 1
HD float env_normalized_entry(float v, uint32_t i, uint32_t n, float inv) { return i == 0 ? v : (i == n ? 1.0f : v * inv); }
HD float env_normalization(float rowSum, uint32_t W, uint32_t H) { return 1.0f / (rowSum * (2 * kPi / (float)W) * (kPi / (float)H)); }

}  // namespace ctl
