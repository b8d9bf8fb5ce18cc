// single_ray.h — device helpers of the integrators that trace one ray at a time inside a lane: the megakernel PathTracer (megakernel.hip) and the
// PrimTracer's delta chains and shadow rays (prim_tracer.hip).  Include after shading.h (with CTL_TEX_PARTIALS defined) and compaction.h.
// The non-template functions are `inline` because two units include this header (the megakernel's device assembly is the same with and without it).
#pragma once
#include "traverse_flat.h"
#include "traverse_flat8.h"

namespace ctl {

// single-ray traversal of the flattened BVH (traverse_flat8.h for the 8-wide format, traverse_flat.h for the 4-wide one): closest hit, or any hit in (tmin, tmax).
// ONE LDS array serves both instantiations: a lane is never in a closest-hit and an any-hit search at the same time (20 KiB per 256-lane workgroup, not 40).
__device__ __forceinline__ lds_int* single_stack_column() {
    __shared__ int s_stack[kSingleLdsRows * 256];   // one column per lane of the 256-lane workgroup
    return (lds_int*)s_stack + threadIdx.x;
}
template <bool ANY_HIT>
__device__ __noinline__ bool trace_single(const dev_scene& S, f3 o, f3 d, float tmin, float tmax, float& ht, float& hu, float& hv, int& htri, int& hnode) {
    if (S.flat_format == kFmtQ8) return trace_single_flat8<ANY_HIT, true>(S, single_stack_column(), o, d, tmin, tmax, ht, hu, hv, htri, hnode);
    return trace_single_flat<ANY_HIT, true>(S, single_stack_column(), o, d, tmin, tmax, ht, hu, hv, htri, hnode);
}

// Light::samplePosition of the emitters the mollified connection uses (SceneTypes/Light.cu:33-40, :304-311, :246-258); area and environment emitters are skipped
__device__ inline f3 light_sample_position(const ctl_light& L, f2 sample, f3& p) {
    if (L.type == CTL_LIGHT_POINT || L.type == CTL_LIGHT_SPOT) { p = f3(L.position[0], L.position[1], L.position[2]); return f3(L.radiance[0], L.radiance[1], L.radiance[2]) * (4 * kPi); }
    if (L.type == CTL_LIGHT_DISTANT) {
        const f2 q = square_to_disk_concentric(sample);
        const frame F = light_frame(L);
        const f3 perpOffset = F.to_world(f3(q.x, q.y, 0) * L.bsphere_radius), d = F.to_world(f3(0.0f, 0.0f, 1.0f));
        p = d * L.bsphere_radius + perpOffset;
        const float surfaceArea = kPi * L.bsphere_radius * L.bsphere_radius, invSurfaceArea = 1.0f / surfaceArea;
        return sdiv(f3(L.radiance[0], L.radiance[1], L.radiance[2]), invSurfaceArea);
    }
    p = f3(0.0f); return f3(0.0f);
}
// InfiniteLight::evalEnvironment(ray, rX, rY) (SceneTypes/Light.cu:496-518)
__device__ inline f3 env_eval_differential(const dev_scene& S, const ctl_light& L, f3 dir, f3 dirX, f3 dirY) {
    const f3 v = xform_dir_transpose(L.to_world, dir);
    const f2 uv{ m_atan2(v.x, -v.z) * kInvTwoPi, m_acos(fminf(1.0f, fmaxf(-1.0f, v.y))) * kInvPi };
    const f3 dvdx = xform_dir_transpose(L.to_world, dirX) - v, dvdy = xform_dir_transpose(L.to_world, dirY) - v;
    const float t1 = kInvTwoPi / (v.x * v.x + v.z * v.z), t2 = -kInvPi / fmaxf(sqrtf(fmaxf(0.0f, 1.0f - v.y * v.y)), 1e-4f);
    const f2 dudx{ t1 * (dvdx.z * v.x - dvdx.x * v.z), t2 * dvdx.y }, dudy{ t1 * (dvdy.z * v.x - dvdy.x * v.z), t2 * dvdy.y };
    return mip_eval(S.images[L.env_image], S.mip_levels[L.env_image], S.mip_weight_lut, uv, dudx, dudy) * f3(L.env_scale[0], L.env_scale[1], L.env_scale[2]);
}

} // namespace ctl
