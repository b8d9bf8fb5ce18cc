// traversal_probe.hip — TEST INFRASTRUCTURE (traversal_probe.h): a kernel that runs the single-ray traversal of the megakernel PathTracer and of the PrimTracer's delta chains
// and shadow rays (single_ray.h trace_single) on a list of rays, so that the tests hold it to the oracle ray by ray (tests/test_gpu_traversal_variants.py).
#include "kernels.h"
#define CTL_TEX_PARTIALS 1   // single_ray.h is included the way megakernel.hip includes it
#include "shading.h"
#include "compaction.h"
#include "tracer.h"
#include "single_ray.h"
#include "traversal_probe.h"

namespace ctl {

template <bool ANY_HIT>
__global__ __launch_bounds__(256) void k_trace_single_probe(dev_scene S, const float4* __restrict__ ro, const float4* __restrict__ rd, uint32_t n, float4* __restrict__ hit, int* __restrict__ hit_node) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        const float4 o = ro[i], d = rd[i];
        float t, u, v; int tri, node;
        const bool found = trace_single<ANY_HIT>(S, f3(o.x, o.y, o.z), f3(d.x, d.y, d.z), o.w, d.w, t, u, v, tri, node);
        hit[i] = found ? make_float4(t, u, v, __int_as_float(tri)) : make_float4(d.w, 0.0f, 0.0f, __int_as_float(-1));
        hit_node[i] = found ? node : -1;
    }
}

void launch_trace_single_probe(const launch_ctx& lc, const dev_scene& S, const float4* ro, const float4* rd, uint32_t n, float4* hit, int* hit_node, int any_hit) {
    if (!n) return;
    const dim3 grid((n + 255u) / 256u), block(256);
    if (any_hit) hipLaunchKernelGGL(k_trace_single_probe<true>, grid, block, 0, lc.stream, S, ro, rd, n, hit, hit_node);
    else hipLaunchKernelGGL(k_trace_single_probe<false>, grid, block, 0, lc.stream, S, ro, rd, n, hit, hit_node);
}

void traversal_lds_rows(uint32_t out5[5]) {
    out5[0] = kLdsStack; out5[1] = kFlatLdsRows; out5[2] = kQ8LdsRows; out5[3] = kSingleLdsRows; out5[4] = kQ8SingleLdsGroups;
}

} // namespace ctl
