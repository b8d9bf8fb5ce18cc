// nlm_filter.hip — the reference's NonLocalMeansFilter (Kernel/ImagePipeline/Filter/NonLocalMeansFilter.{h,cu}): variance-guided non-local means over a
// 13 x 13 search window (R = 6) of 7 x 7 patches (F = 3), from the RGBE-quantised frame (copyToCached) and the half-precision per-pixel variance of the
// tracer's PixelVarianceBuffer, into the filtered RGBE plane.
//
// One fused kernel instead of computeWeights + applyWeights and their 169-floats-per-pixel weight buffer.  The patch distance of pixel p to candidate p + o is a
// sum over the 49 patch offsets d of a term that depends only on the pixel p + d and on o, so a workgroup that owns a 16 x 16 tile computes, per candidate offset,
// the term plane over the tile and its F-halo (22 x 22) ONCE into LDS and every pixel adds up its 49 terms from there, in the reference's order (patch x outer,
// y inner; candidates xo outer, yo inner).  The frame is decoded from RGBE once per tile into LDS, (r, g, b, sigma2Scale * variance) per pixel of the tile and its
// (R + F)-halo (34 x 34).  Nothing is reordered: every sum is the reference's sum in fp32, exp is ctl_fmath.h's (bit-identical on the host), and whether a term
// counts is decided from coordinates, never from its value (terms are NaN or infinite where the variance is).
#include "tracer.h"
#include "pipeline_pixel.h"
#include "ctl_fmath.h"

namespace ctl {

namespace {

constexpr int kR = 6, kF = 3;                        // NonLocalMeansFilter::Apply (NonLocalMeansFilter.cu:186)
constexpr int kTile = 16;                            // pixels per workgroup: 16 x 16, one per lane
constexpr int kRegion = kTile + 2 * (kR + kF);       // 34: decoded pixels per side
constexpr int kPlane = kTile + 2 * kF;               // 22: terms per side
// Row stride of the term plane in floats.  A wave holds 4 tile rows of 16 lanes and a ds_read_b32 serves 32 lanes (2 rows) per LDS cycle over 32 banks: with
// a stride of 16 mod 32 the two rows fall on disjoint halves of the banks whatever the patch offset is
constexpr int kPlaneStride = 48;
constexpr int kPlaneTerms = kPlane * kPlane;         // 484: at most two per lane

// one term of patchDistance (NonLocalMeansFilter.cu:80-86); a, b = (r, g, b, var * sigma2Scale) of p + d and q + d
__device__ __forceinline__ float patch_term(const float4 a, const float4 b, float kk) {
    const float dr = a.x - b.x, dg = a.y - b.y, db = a.z - b.z;
    const float u_diff = ((dr * dr + dg * dg) + db * db) * (1.0f / 3);   // math::sqr(c_p - c_q).avg() (Math/Spectrum.h:180-189)
    return (u_diff - (a.w + fminf(a.w, b.w))) / (1e-10f + kk * (a.w + b.w));
}

__global__ __launch_bounds__(256) void k_nlm_filter(const ctl_pixel_data* __restrict__ px, const float* __restrict__ variance, int w, int h, float splat_scale, float kk,
                                                    float sigma2_scale, uint32_t* __restrict__ filtered) {
    __shared__ float4 s_px[kRegion * kRegion];               // 18,496 B
    __shared__ float s_term[2][kPlane * kPlaneStride];       //  8,448 B: two planes, so that one barrier per candidate is enough
    const int t = threadIdx.x, lx = t & (kTile - 1), ly = t / kTile;
    const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile, x = x0 + lx, y = y0 + ly;

    // copyToCached + copyToShared: toSpectrum -> RGBE -> float, variance -> half -> float, scaled (NonLocalMeansFilter.cu:17-36,150-158,83).  Pixels outside
    // the image hold zeros; no term that reads them is ever added
    for (int i = t; i < kRegion * kRegion; i += 256) {
        const int gx = x0 - (kR + kF) + i % kRegion, gy = y0 - (kR + kF) + i / kRegion;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t g = (size_t)gy * w + gx;
            const f3 c = from_rgbe(to_rgbe(to_spectrum(px[g], splat_scale)));
            v = make_float4(c.x, c.y, c.z, (float)(_Float16)variance[g] * sigma2_scale);   // half(float): round to nearest even, above 65504 -> inf
        }
        s_px[i] = v;
    }

    // this lane's (at most two) terms of a plane: where p + d lies in the decoded region and in the plane
    const int t1 = t + 256; const bool has1 = t1 < kPlaneTerms;
    const int u0 = t % kPlane, v0 = t / kPlane, u1 = has1 ? t1 % kPlane : 0, v1 = has1 ? t1 / kPlane : 0;
    const int reg0 = (v0 + kR) * kRegion + u0 + kR, reg1 = (v1 + kR) * kRegion + u1 + kR;
    const int pl0 = v0 * kPlaneStride + u0, pl1 = v1 * kPlaneStride + u1;
    const int own = (ly + kF) * kPlaneStride + lx + kF;      // this lane's pixel in a plane
    const bool inside = x < w && y < h;
    // every patch of the tile, for every candidate, inside the image: no coordinate tests in the sums (uniform over the workgroup)
    const bool interior = x0 - (kR + kF) >= 0 && y0 - (kR + kF) >= 0 && x0 + kTile - 1 + kR + kF < w && y0 + kTile - 1 + kR + kF < h;
    __syncthreads();

    const float4 c_p = s_px[(ly + kR + kF) * kRegion + lx + kR + kF];
    float hat_r = 0.0f, hat_g = 0.0f, hat_b = 0.0f, C_p = 0.0f;   // applyWeights (NonLocalMeansFilter.cu:131-145)
    int buf = 0;
    for (int xo = -kR; xo <= kR; xo++)
        for (int yo = -kR; yo <= kR; yo++, buf ^= 1) {
            float* plane = s_term[buf];
            const int shift = yo * kRegion + xo;
            plane[pl0] = patch_term(s_px[reg0], s_px[reg0 + shift], kk);
            if (has1) plane[pl1] = patch_term(s_px[reg1], s_px[reg1 + shift], kk);
            __syncthreads();   // the plane is complete; the other plane is not written before every lane has passed the next barrier, i.e. has finished with it
            const int qx = x + xo, qy = y + yo;
            if (!inside || qx < 0 || qx >= w || qy < 0 || qy >= h) continue;   // (the loop bounds are uniform: every lane reaches every barrier)
            float d_range = 0.0f;
            if (interior) {
#pragma unroll
                for (int dx = -kF; dx <= kF; dx++)
#pragma unroll
                    for (int dy = -kF; dy <= kF; dy++) d_range += plane[own + dy * kPlaneStride + dx];
                d_range = d_range / (float)((2 * kF + 1) * (2 * kF + 1));
            } else {   // patchDistance's own tests (NonLocalMeansFilter.cu:76-78)
                int count = 0;
                for (int dx = -kF; dx <= kF; dx++) {
                    if (x + dx < 0 || x + dx >= w || qx + dx < 0 || qx + dx >= w) continue;
                    for (int dy = -kF; dy <= kF; dy++) {
                        if (y + dy < 0 || y + dy >= h || qy + dy < 0 || qy + dy >= h) continue;
                        d_range += plane[own + dy * kPlaneStride + dx]; count++;
                    }
                }
                d_range = count != 0 ? d_range / (float)count : 0.0f;
            }
            // weight (NonLocalMeansFilter.cu:93-99).  max is fmaxf: a NaN distance gives 0 and the weight 1.  exp(-m) < 0.05 from m = 3 on, so past 4 (a margin
            // far wider than exp's error) the cut-off is taken without the exponential
            const float m = fmaxf(0.0f, d_range);
            if (m > 4.0f) continue;
            float we = fm::exp(-m);
            we = we < 0.05f ? 0.0f : we;
            const float4 c_q = s_px[(ly + kR + kF + yo) * kRegion + lx + kR + kF + xo];
            C_p += we;
            hat_r += we * c_q.x; hat_g += we * c_q.y; hat_b += we * c_q.z;
        }
    if (!inside) return;
    f3 out(c_p.x, c_p.y, c_p.z);
    if (C_p > 1e-4f) { const float recip = 1.0f / C_p; out = f3(hat_r * recip, hat_g * recip, hat_b * recip); }   // Spectrum / float (Math/Spectrum.h:122-128)
    filtered[(size_t)y * w + x] = to_rgbe(out);
}

} // namespace

void launch_nlm_filter(hipStream_t s, const ctl_pixel_data* px, const float* variance, uint32_t w, uint32_t h, float splat_scale, float k, float sigma2_scale, uint32_t* filtered_rgbe) {
    hipLaunchKernelGGL(k_nlm_filter, dim3((w + kTile - 1) / kTile, (h + kTile - 1) / kTile), dim3(256), 0, s, px, variance, (int)w, (int)h, splat_scale, k * k, sigma2_scale, filtered_rgbe);
}

} // namespace ctl
