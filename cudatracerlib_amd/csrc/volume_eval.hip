// volume_eval.hip — ctl_volume_update and ctl_volume_eval: the functions of volume.h one call per query, on the host (the yardstick: no device needed) or in one small
// kernel.  Both run volume_eval_row below, so a row differs between the two only where the compiler's device and host code differ — which the tests hold to nothing
// (tests/test_gpu_volume.py), as ctl_shared_math_eval does for ctl_fmath.h.
#include "volume_eval.h"
#include "tracer.h"
#include "scene_checks.h"
#include "scene_builder.h"   // mat_inverse
#include <cstring>
#include <stdexcept>
#include <string>

namespace ctl {

using namespace vol;

// one query row (CTL_VEVAL_QUERY_FLOATS floats) -> one result row (CTL_VEVAL_RESULT_FLOATS floats, zero where a function writes nothing); layouts: include/ctl_amd.h
HD void volume_eval_row(const table& T, int what, const float* __restrict__ a, float* __restrict__ o) {
    for (int k = 0; k < CTL_VEVAL_RESULT_FLOATS; k++) o[k] = 0.0f;
    auto word = [](float f) { return __builtin_bit_cast(uint32_t, f); };
    auto put3 = [](float* p, f3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; };
    auto put_rec = [&](bool ok, const medium_rec& m) {
        o[0] = ok ? 1.0f : 0.0f; o[1] = m.t; put3(o + 2, m.p); put3(o + 5, m.transmittance); put3(o + 8, m.sigmaA); put3(o + 11, m.sigmaS);
        o[14] = m.pdfSuccess; o[15] = m.pdfSuccessRev; o[16] = m.pdfFailure;
    };
    medium_rec m = zero_rec();
    switch (what) {
    case CTL_VEVAL_REGION_INTERSECT: { float t0 = 0, t1 = 0; o[0] = region_intersect(T.v[word(a[0])], f3(a[1], a[2], a[3]), f3(a[4], a[5], a[6]), a[7], a[8], t0, t1) ? 1.0f : 0.0f; o[1] = t0; o[2] = t1; break; }
    case CTL_VEVAL_INTERSECT: { float t0, t1; o[0] = intersect(T, f3(a[0], a[1], a[2]), f3(a[3], a[4], a[5]), a[6], a[7], t0, t1) ? 1.0f : 0.0f; o[1] = t0; o[2] = t1; break; }
    case CTL_VEVAL_REGION_TAU: put3(o, region_tau_d<true>(T, word(a[0]), f3(a[1], a[2], a[3]), f3(a[4], a[5], a[6]), a[7], a[8])); break;
    case CTL_VEVAL_TAU: put3(o, tau<true>(T, f3(a[0], a[1], a[2]), f3(a[3], a[4], a[5]), a[6], a[7])); break;
    case CTL_VEVAL_REGION_SAMPLE_DISTANCE: { const bool ok = region_sample_distance_d<true>(T, word(a[0]), f3(a[1], a[2], a[3]), f3(a[4], a[5], a[6]), a[7], a[8], a[9], m); put_rec(ok, m); break; }
    case CTL_VEVAL_SAMPLE_DISTANCE: { const bool ok = sample_distance<true>(T, f3(a[0], a[1], a[2]), f3(a[3], a[4], a[5]), a[6], a[7], a[8], m); put_rec(ok, m); break; }
    case CTL_VEVAL_SAMPLE_VOLUME: { float s = a[8], pdf = 0; o[0] = (float)sample_volume(T, f3(a[0], a[1], a[2]), f3(a[3], a[4], a[5]), a[6], a[7], s, pdf); o[1] = s; o[2] = pdf; break; }
    case CTL_VEVAL_PHASE_EVAL: o[0] = phase_eval(T.v[word(a[0])].phase, f3(a[1], a[2], a[3]), f3(a[4], a[5], a[6])); break;
    case CTL_VEVAL_PHASE_SAMPLE: { f3 wo(0.0f); float pdf = 0; o[0] = phase_sample(T.v[word(a[0])].phase, f3(a[1], a[2], a[3]), wo, pdf, f2{ a[4], a[5] }); o[1] = pdf; put3(o + 2, wo); break; }
    case CTL_VEVAL_P: o[0] = phase_p<true>(T, f3(a[0], a[1], a[2]), f3(a[3], a[4], a[5]), f3(a[6], a[7], a[8])); break;
    case CTL_VEVAL_SAMPLE: { f3 wo(0.0f); float pdf = 0; o[0] = phase_sample_aggregate(T, f3(a[0], a[1], a[2]), f3(a[3], a[4], a[5]), wo, pdf, f2{ a[6], a[7] }); o[1] = pdf; put3(o + 2, wo); break; }
    case CTL_VEVAL_TRANSMITTANCE: put3(o, transmittance<true>(T, f3(a[0], a[1], a[2]), f3(a[3], a[4], a[5]), a[6], a[7])); break;
    case CTL_VEVAL_EVAL_TRANSMITTANCE: put3(o, eval_transmittance<true>(T, f3(a[0], a[1], a[2]), f3(a[3], a[4], a[5]))); break;
    // the grid's own functions: the region is a CTL_VOLUME_GRID one (checked by volume_eval before anything runs)
    case CTL_VEVAL_GRID_VALUE: { const grid_region G = region_of(T, word(a[0])); o[0] = grid_trilinear(G.single ? G.g : (word(a[1]) ? G.gS : G.gA), f3(a[2], a[3], a[4])); break; }
    case CTL_VEVAL_REGION_SIGMA: { const grid_region G = region_of(T, word(a[0])); const f3 p(a[1], a[2], a[3]); put3(o, grid_sigma_a(G, p)); put3(o + 3, grid_sigma_s(G, p)); put3(o + 6, grid_sigma_t(G, p)); break; }
    default: { uint32_t steps; bool capped; grid_tau(region_of(T, word(a[0])), f3(a[1], a[2], a[3]), f3(a[4], a[5], a[6]), a[7], a[8], &steps, &capped); o[0] = (float)steps; o[1] = capped ? 1.0f : 0.0f; break; }   // CTL_VEVAL_GRID_MARCH
    }
}

__global__ __launch_bounds__(256) void k_volume_eval(table T, int what, uint32_t n, const float* __restrict__ q, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    volume_eval_row(T, what, q + (size_t)i * CTL_VEVAL_QUERY_FLOATS, out + (size_t)i * CTL_VEVAL_RESULT_FLOATS);
}

void volume_update(ctl_volume& v) {
    if (v.type != CTL_VOLUME_HOMOGENEOUS && v.type != CTL_VOLUME_GRID) throw std::runtime_error("ctl_volume_update: unknown volume type " + std::to_string(v.type));
    if (v.phase.type < CTL_PHASE_HG || v.phase.type > CTL_PHASE_RAYLEIGH) throw std::runtime_error("ctl_volume_update: unknown phase function type " + std::to_string(v.phase.type));
    mat_inverse(v.volume_to_world.m, v.world_to_volume.m);   // BaseVolumeRegion::Update
    if (v.phase.type == CTL_PHASE_KAJIYA_KAY) v.phase.normalization = kajiya_kay_normalization(v.phase.exponent);
}

void volume_eval(const ctl_scene_desc& d, int what, const float* queries, uint32_t n, float* out, bool on_device) {
    if (what < CTL_VEVAL_REGION_INTERSECT || what > CTL_VEVAL_GRID_MARCH) throw std::runtime_error("ctl_volume_eval: unknown function " + std::to_string(what));
    if (on_device) require_device();
    check_scene_desc(d, CTL_DIFF_VOLUMES, "ctl_volume_eval");
    const bool names_region = what == CTL_VEVAL_REGION_INTERSECT || what == CTL_VEVAL_REGION_TAU || what == CTL_VEVAL_REGION_SAMPLE_DISTANCE || what == CTL_VEVAL_PHASE_EVAL || what == CTL_VEVAL_PHASE_SAMPLE || what >= CTL_VEVAL_GRID_VALUE;
    if (names_region) for (uint32_t i = 0; i < n; i++) {   // everything a query names is checked before anything runs
        uint32_t vi; std::memcpy(&vi, queries + (size_t)i * CTL_VEVAL_QUERY_FLOATS, 4);
        if (vi >= d.n_volumes) throw std::runtime_error("ctl_volume_eval: query " + std::to_string(i) + " names volume " + std::to_string(vi) + " of " + std::to_string(d.n_volumes));
        if (what >= CTL_VEVAL_GRID_VALUE && d.volumes[vi].type != CTL_VOLUME_GRID) throw std::runtime_error("ctl_volume_eval: query " + std::to_string(i) + " names volume " + std::to_string(vi) + ", which is no VolumeGrid");
    }
    if (!n) return;
    grid_pack gp; pack_grids(d, gp);
    if (!on_device) {
        const table T = make_table(d.volumes, d.n_volumes, gp.recs.data(), gp.cells.data());
        for (uint32_t i = 0; i < n; i++) volume_eval_row(T, what, queries + (size_t)i * CTL_VEVAL_QUERY_FLOATS, out + (size_t)i * CTL_VEVAL_RESULT_FLOATS);
        return;
    }
    dbuf<ctl_volume> dv; dbuf<float> dq, dout, dcells; dbuf<grid_rec> dg;
    dg.upload(gp.recs.data(), gp.recs.size());
    if (!gp.cells.empty()) dcells.upload(gp.cells.data(), gp.cells.size());
    dv.alloc(CTL_MAX_VOL_COUNT); dq.alloc((size_t)n * CTL_VEVAL_QUERY_FLOATS); dout.alloc((size_t)n * CTL_VEVAL_RESULT_FLOATS);
    CTL_HIP(hipMemset(dv.p, 0, CTL_MAX_VOL_COUNT * sizeof(ctl_volume)));
    if (d.n_volumes) CTL_HIP(hipMemcpy(dv.p, d.volumes, (size_t)d.n_volumes * sizeof(ctl_volume), hipMemcpyHostToDevice));
    CTL_HIP(hipMemcpy(dq.p, queries, (size_t)n * CTL_VEVAL_QUERY_FLOATS * 4, hipMemcpyHostToDevice));
    const table T = make_table(dv.p, d.n_volumes, dg.p, dcells.p);
    hipLaunchKernelGGL(k_volume_eval, dim3((n + 255) / 256), dim3(256), 0, 0, T, what, n, (const float*)dq.p, dout.p);
    CTL_HIP(hipGetLastError());
    CTL_HIP(hipMemcpy(out, dout.p, (size_t)n * CTL_VEVAL_RESULT_FLOATS * 4, hipMemcpyDeviceToHost));
}

}  // namespace ctl
