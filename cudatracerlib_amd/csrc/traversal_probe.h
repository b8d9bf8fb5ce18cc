// traversal_probe.h — TEST INFRASTRUCTURE: the single-ray traversal of single_ray.h behind a launch of its own (ctl_intersect_ex, CTL_ISECT_SINGLE), and the LDS row
// limits of the five traversal stacks for the tools and tests that read the stack histogram.
#pragma once
#include "kernels.h"

namespace ctl {

// One lane per ray, 256-lane workgroups: trace_single<ANY_HIT>(S, o, d, tmin, tmax, ...) as the megakernel calls it; (t, u, v, triangle) and the node for a hit,
// (tmax, 0, 0, -1) and -1 for a miss, as the wavefront kernels write them.  The scene must be flattened (the caller checks).
void launch_trace_single_probe(const launch_ctx& lc, const dev_scene& S, const float4* ro, const float4* rd, uint32_t n, float4* hit, int* hit_node, int any_hit);
// stack entries a lane keeps in LDS: two-level, Q4, Q8 (sibling groups), single-ray Q4, single-ray Q8 (groups); deeper entries live in scratch
void traversal_lds_rows(uint32_t out5[5]);

} // namespace ctl
