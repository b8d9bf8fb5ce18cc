// shading_eval.inc — the kernels of ctl_shading_eval (shading_eval.h): one lane = one query.  A kernel fills the record the way the oracle's call of the same name does
// (oracle/oracle_capi.cpp orc_bsdf_sample_uv, orc_light_sample_direct, ...: an identity frame at the origin, uv from the query), calls the __device__ function the shade
// kernels call, and stores the result row.  Nothing else: what the tests compare is shading.h itself, under the feature set of the including file (shading_eval_*.hip
// define CTL_EVAL_NAME and the CTL_SHADE_* / CTL_TEX_PARTIALS set of the product build they mirror).
#include "shading_eval.h"
#include "shading.h"

#define CTL_EVAL_CAT_(a, b) a##b
#define CTL_EVAL_CAT(a, b) CTL_EVAL_CAT_(a, b)
#define CTL_EVAL_NS CTL_EVAL_CAT(eval_, CTL_EVAL_NAME)
#define CTL_EVAL_LAUNCH CTL_EVAL_CAT(launch_shading_eval_, CTL_EVAL_NAME)

namespace ctl {
namespace CTL_EVAL_NS {

constexpr uint32_t kBlock = 256;

__device__ __forceinline__ uint32_t word(float f) { return __float_as_uint(f); }
__device__ __forceinline__ void put3(float* o, f3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
// the scene's small tables go to LDS where the build keeps them there (every lane of the workgroup, before the bounds check: scene_tables_to_lds has a barrier)
__device__ __forceinline__ void stage_tables(const dev_scene& S) {
#if CTL_SHADE_LDS_TABLES
    scene_tables_to_lds<kBlock>(S);
#endif
}
// dg of the oracle's probes: an identity frame at the origin, the scene's tables
__device__ __forceinline__ void probe_dg(const dev_scene& S, diff_geom& dg, float u, float v) {
    dg.P = f3(0.0f); dg.sys.s = f3(1.0f, 0.0f, 0.0f); dg.sys.t = f3(0.0f, 1.0f, 0.0f); dg.sys.n = f3(0.0f, 0.0f, 1.0f); dg.n = f3(0.0f, 0.0f, 1.0f); dg.uv = f2{ u, v };
    dg.images = S.images; dg.rough_transmittance = S.rough_transmittance; dg.mats = S.mats; dg.rt_reduced = S.rt_reduced;
#if (CTL_SHADE_FEATURES & 32) || defined(CTL_TEX_PARTIALS)
    dg.dpdu = f3(0.0f); dg.dpdv = f3(0.0f);
#endif
#ifdef CTL_TEX_PARTIALS
    dg.has_uv_partials = false; dg.dudx = dg.dudy = dg.dvdx = dg.dvdy = 0.0f; dg.mip_levels = S.mip_levels; dg.mip_weight_lut = S.mip_weight_lut;
#endif
}
// DirectSamplingRecord(ref, refN) with the fields its constructor leaves open set to zero (the oracle's batched calls do the same)
__device__ __forceinline__ void probe_direct(direct_rec& r, f3 ref, f3 refN) { r.ref = ref; r.refN = refN; r.p = ref; r.n = refN; r.d = f3(0.0f); r.dist = 0.0f; r.pdf = 0.0f; r.measure = kMeasureArea; }

#define CTL_EVAL_ROW                                                                  \
    stage_tables(S);                                                                  \
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x; if (i >= n) return;          \
    const float* __restrict__ a = q + (size_t)i * qs; float* __restrict__ o = out + (size_t)i * os;

// [material] wi(3) sample(2) uv(2) -> f(3) pdf wo(3) sampledType eta
__global__ __launch_bounds__(kBlock) void k_bsdf_sample(dev_scene S, uint32_t n, const float* __restrict__ q, uint32_t qs, float* __restrict__ out, uint32_t os) {
    CTL_EVAL_ROW
    bsdf_rec b; probe_dg(S, b.dg, a[6], a[7]);
    b.wi = f3(a[1], a[2], a[3]); b.wo = f3(0.0f); b.eta = 1.0f; b.type_mask = kEAll; b.sampled_type = 0;
    float pdf = 0.0f; const f3 f = bsdf_sample_top(S.mats[word(a[0])], b, pdf, f2{ a[4], a[5] });
    put3(o, f); o[3] = pdf; put3(o + 4, b.wo); o[7] = (float)b.sampled_type; o[8] = b.eta;
}
// [material] wi(3) wo(3) [type mask] uv(2) -> f(3) pdf, solid-angle measure
__global__ __launch_bounds__(kBlock) void k_bsdf_eval(dev_scene S, uint32_t n, const float* __restrict__ q, uint32_t qs, float* __restrict__ out, uint32_t os) {
    CTL_EVAL_ROW
    bsdf_rec b; probe_dg(S, b.dg, a[8], a[9]);
    b.wi = f3(a[1], a[2], a[3]); b.wo = f3(a[4], a[5], a[6]); b.eta = 1.0f; b.type_mask = word(a[7]); b.sampled_type = 0;
    const ctl_material& mat = S.mats[word(a[0])];
    put3(o, bsdf_f_top(mat, b)); o[3] = bsdf_pdf_top(mat, b);
}
// [material] wi(3) sample(2) uv(2) wo2(3) -> the sample's row, then f(3) pdf for wo2 on THE SAME record: next-event estimation as shade_kernel.inc does it
__global__ __launch_bounds__(kBlock) void k_bsdf_sample_eval(dev_scene S, uint32_t n, const float* __restrict__ q, uint32_t qs, float* __restrict__ out, uint32_t os) {
    CTL_EVAL_ROW
    bsdf_rec b; probe_dg(S, b.dg, a[6], a[7]);
    b.wi = f3(a[1], a[2], a[3]); b.wo = f3(0.0f); b.eta = 1.0f; b.type_mask = kEAll; b.sampled_type = 0;
    const ctl_material& mat = S.mats[word(a[0])];
    float pdf = 0.0f; const f3 f = bsdf_sample_top(mat, b, pdf, f2{ a[4], a[5] });
    put3(o, f); o[3] = pdf; put3(o + 4, b.wo); o[7] = (float)b.sampled_type; o[8] = b.eta;
    b.wo = f3(a[8], a[9], a[10]); b.type_mask = kEAll & ~kEDelta;
    const f3 bsdfVal = bsdf_f_top(mat, b);
    const float bp = bsdf_pdf_top(mat, b);
    put3(o + 9, bsdfVal); o[12] = bp;
}
__device__ __forceinline__ void put_direct(float* o, f3 value, const direct_rec& r) { put3(o, value); o[3] = r.pdf; put3(o + 4, r.d); o[7] = r.dist; put3(o + 8, r.p); put3(o + 11, r.n); }
// [light] ref(3) refN(3) sample(2) -> value(3) pdf d(3) dist p(3) n(3) measure
__global__ __launch_bounds__(kBlock) void k_light_sample(dev_scene S, uint32_t n, const float* __restrict__ q, uint32_t qs, float* __restrict__ out, uint32_t os) {
    CTL_EVAL_ROW
    direct_rec r; probe_direct(r, f3(a[1], a[2], a[3]), f3(a[4], a[5], a[6]));
    const f3 value = light_sample_direct(S, scene_lights(S)[word(a[0])], r, f2{ a[7], a[8] });
    put_direct(o, value, r); o[14] = (float)r.measure;
}
// ref(3) refN(3) sample(2) -> sampleEmitterDirect: value(3) pdf d(3) dist p(3) n(3) slot, emitter pdf, the re-scaled sample.x; then sample_emitter's slot and pdf
__global__ __launch_bounds__(kBlock) void k_emitter_sample(dev_scene S, uint32_t n, const float* __restrict__ q, uint32_t qs, float* __restrict__ out, uint32_t os) {
    CTL_EVAL_ROW
    direct_rec dr; probe_direct(dr, f3(a[0], a[1], a[2]), f3(a[3], a[4], a[5]));
    f2 sl{ a[6], a[7] }; f3 value(0.0f);
    float lpdf = 0.0f; const int li = sample_emitter_reuse(S, lpdf, sl.x);
    bool valid = false;
    if (li >= 0) {
        value = light_sample_direct(S, scene_lights(S)[li], dr, sl);
        valid = dr.pdf != 0;
        if (valid) { dr.pdf *= lpdf; value = sdiv(value, lpdf); } else value = f3(0.0f);
    }
    put_direct(o, value, dr); o[14] = valid ? (float)li : -1.0f; o[15] = lpdf; o[16] = sl.x;
    float lpdf2 = 0.0f; const int li2 = sample_emitter(S, lpdf2, a[6]);
    o[17] = (float)li2; o[18] = lpdf2;
}
// [light] ref(3) refN(3) d(3) dist n(3) -> pdfDirect in the solid-angle measure (the environment emitter through env_pdf_direct, as the miss branch of the shade kernel asks)
__global__ __launch_bounds__(kBlock) void k_light_pdf(dev_scene S, uint32_t n, const float* __restrict__ q, uint32_t qs, float* __restrict__ out, uint32_t os) {
    CTL_EVAL_ROW
    const ctl_light& L = scene_lights(S)[word(a[0])];
    const f3 d(a[7], a[8], a[9]);
    o[0] = L.type == CTL_LIGHT_INFINITE ? env_pdf_direct(S, L, d) : light_pdf_direct(L, d, f3(a[4], a[5], a[6]), f3(a[11], a[12], a[13]), a[10]);
}
// [light] p(3) n(3) d(3) -> DiffuseLight::eval
__global__ __launch_bounds__(kBlock) void k_light_eval(dev_scene S, uint32_t n, const float* __restrict__ q, uint32_t qs, float* __restrict__ out, uint32_t os) {
    CTL_EVAL_ROW
    put3(o, light_eval(S, scene_lights(S)[word(a[0])], f3(a[1], a[2], a[3]), f3(a[4], a[5], a[6]), f3(a[7], a[8], a[9])));
}
// dir(3) -> InfiniteLight::evalEnvironment of the scene's environment emitter
__global__ __launch_bounds__(kBlock) void k_env_eval(dev_scene S, uint32_t n, const float* __restrict__ q, uint32_t qs, float* __restrict__ out, uint32_t os) {
    CTL_EVAL_ROW
    put3(o, env_eval(S, scene_lights(S)[S.env_map_index], f3(a[0], a[1], a[2])));
}
// [kind] [index] uv(2) -> Texture::Evaluate(dg) without uv partials; kind 0..3 = tex[kind] of material `index`, 4 its map_tex, 5 its alpha_tex, 6 = rad_texture of light `index`
__global__ __launch_bounds__(kBlock) void k_texture(dev_scene S, uint32_t n, const float* __restrict__ q, uint32_t qs, float* __restrict__ out, uint32_t os) {
    CTL_EVAL_ROW
    const uint32_t kind = word(a[0]), idx = word(a[1]);
    diff_geom dg; probe_dg(S, dg, a[2], a[3]);
    const ctl_texture& t = kind == 6 ? scene_lights(S)[idx].rad_texture : (kind == 5 ? S.mats[idx].alpha_tex : (kind == 4 ? S.mats[idx].map_tex : S.mats[idx].tex[kind]));
    put3(o, tex_eval(t, dg));
}
#ifdef CTL_TEX_PARTIALS
// [image] uv(2) d0(2) d1(2) -> KernelMIPMap::eval(uv, d0, d1)
__global__ __launch_bounds__(kBlock) void k_mip(dev_scene S, uint32_t n, const float* __restrict__ q, uint32_t qs, float* __restrict__ out, uint32_t os) {
    CTL_EVAL_ROW
    const uint32_t im = word(a[0]);
    put3(o, mip_eval(S.images[im], S.mip_levels[im], S.mip_weight_lut, f2{ a[1], a[2] }, f2{ a[3], a[4] }, f2{ a[5], a[6] }));
}
#endif
#if CTL_SHADE_FEATURES & 32
// [material] uv(2) frame s t n (9) geometric normal, dpdu, dpdv (9) -> the perturbed frame
__global__ __launch_bounds__(kBlock) void k_normal_map(dev_scene S, uint32_t n, const float* __restrict__ q, uint32_t qs, float* __restrict__ out, uint32_t os) {
    CTL_EVAL_ROW
    diff_geom dg; probe_dg(S, dg, a[1], a[2]);
    dg.sys.s = f3(a[3], a[4], a[5]); dg.sys.t = f3(a[6], a[7], a[8]); dg.sys.n = f3(a[9], a[10], a[11]);
    dg.n = f3(a[12], a[13], a[14]); dg.dpdu = f3(a[15], a[16], a[17]); dg.dpdv = f3(a[18], a[19], a[20]);
    const ctl_material& mat = S.mats[word(a[0])];
    if (mat.map_kind != CTL_MAP_NONE) sample_normal_map(mat, dg);
    put3(o, dg.sys.s); put3(o + 3, dg.sys.t); put3(o + 6, dg.sys.n);
}
#endif

// Material::AlphaTest as the traversal asks it (alpha_survives): query i is triangle i of node i of the call's synthetic tri_data / node_info — node_info[i].x the material,
// all three vertices at the query's uv, so that the barycentrics (1, 0) give exactly that uv
__global__ __launch_bounds__(kBlock) void k_alpha_test(dev_scene S, uint32_t n, const float* __restrict__ q, uint32_t qs, float* __restrict__ out, uint32_t os) {
    CTL_EVAL_ROW
    (void)a;
    o[0] = alpha_survives(S.tri_data, S.node_info, S.mats, S.images, (int)i, (int)i, 1.0f, 0.0f) ? 1.0f : 0.0f;
}

} // namespace CTL_EVAL_NS

bool CTL_EVAL_LAUNCH(const dev_scene& S, int what, uint32_t n, const float* q, uint32_t qs, float* out, uint32_t os) {
    using namespace CTL_EVAL_NS;
    const dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
    if (n == 0) return true;
    switch (what) {
    case kEvalBsdfSample: hipLaunchKernelGGL(k_bsdf_sample, grid, block, 0, 0, S, n, q, qs, out, os); return true;
    case kEvalBsdfEval: hipLaunchKernelGGL(k_bsdf_eval, grid, block, 0, 0, S, n, q, qs, out, os); return true;
    case kEvalBsdfSampleEval: hipLaunchKernelGGL(k_bsdf_sample_eval, grid, block, 0, 0, S, n, q, qs, out, os); return true;
    case kEvalLightSample: hipLaunchKernelGGL(k_light_sample, grid, block, 0, 0, S, n, q, qs, out, os); return true;
    case kEvalEmitterSample: hipLaunchKernelGGL(k_emitter_sample, grid, block, 0, 0, S, n, q, qs, out, os); return true;
    case kEvalLightPdf: hipLaunchKernelGGL(k_light_pdf, grid, block, 0, 0, S, n, q, qs, out, os); return true;
    case kEvalLightEval: hipLaunchKernelGGL(k_light_eval, grid, block, 0, 0, S, n, q, qs, out, os); return true;
    case kEvalEnvEval: hipLaunchKernelGGL(k_env_eval, grid, block, 0, 0, S, n, q, qs, out, os); return true;
    case kEvalTexture: hipLaunchKernelGGL(k_texture, grid, block, 0, 0, S, n, q, qs, out, os); return true;
#ifdef CTL_TEX_PARTIALS
    case kEvalMip: hipLaunchKernelGGL(k_mip, grid, block, 0, 0, S, n, q, qs, out, os); return true;
#endif
#if CTL_SHADE_FEATURES & 32
    case kEvalNormalMap: hipLaunchKernelGGL(k_normal_map, grid, block, 0, 0, S, n, q, qs, out, os); return true;
#endif
    case kEvalAlphaTest: hipLaunchKernelGGL(k_alpha_test, grid, block, 0, 0, S, n, q, qs, out, os); return true;
    default: return false;
    }
}

} // namespace ctl
