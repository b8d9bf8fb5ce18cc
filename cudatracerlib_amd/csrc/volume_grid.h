// volume_grid.h — VolumeGrid, the reference's heterogeneous medium (SceneTypes/Volumes.h:101-287, Volumes.cu:87-239, the grid march of
// Engine/SpatialStructures/Grid/SpatialGridTraversal.h:9-45), restated as written: fp32, the source's operation order, exp / log from ctl_fmath.h on the host and on the
// device.  Included by volume.h (which defines table, grid_rec, medium_rec and the region's box functions); single source for the megakernel's GRID instantiation, the
// call-by-call kernel and the host yardstick.  The oddities are restated, not repaired; each is marked where it stands with its source line.
#pragma once

namespace ctl {
namespace vol {

// float -> unsigned int as this project DEFINES it where the reference has no defined value (a C++ cast of a negative, NaN or too large float is undefined; the CUDA
// and HIP device conversions saturate): negative or NaN: 0, 2^32 and above: 0xffffffff.  Written out so that the host and the device run the same comparison
HD uint32_t f2u(float x) { return !(x > 0.0f) ? 0u : (x >= 4294967296.0f ? 0xffffffffu : (uint32_t)x); }
HD float rcp0(float a) { return a != 0.0f ? 1.0f / a : 0.0f; }                       // math::rcp (MathFunc.h:399): 0 for 0
HD f3 normalized0(f3 v) { return v * rcp0(length(v)); }                              // VectorBase::normalized (Vector.h:369-371)
HD uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
HD uint32_t uclamp(uint32_t v, uint32_t lo, uint32_t hi) { const uint32_t m = v > lo ? v : lo; return m < hi ? m : hi; }   // math::clamp = min(max(v, lo), hi)
HD float fsign(float f) { return f > 0.0f ? 1.0f : (f < 0.0f ? -1.0f : 0.0f); }    // math::sign (MathFunc.h:133-136)

// DenseVolGrid<float> (Volumes.h:116-182): its cells in the table's float buffer
struct grid_view { const float* data; uint32_t dx, dy, dz; float fx, fy, fz; };
HD grid_view view_of(const table& T, const uint32_t* dim, uint32_t off) { grid_view g; g.data = T.cells + off; g.dx = dim[0]; g.dy = dim[1]; g.dz = dim[2]; g.fx = (float)dim[0]; g.fy = (float)dim[1]; g.fz = (float)dim[2]; return g; }
HD f3 dimf(const grid_view& g) { return f3(g.fx, g.fy, g.fz); }
// DenseVolGrid::idx (Volumes.h:139-142), as written: the FIRST argument is the slowest axis and is clamped against dim.z, the last the fastest and clamped against
// dim.x.  The result is at most (dx-1) + (dy-1) dx + (dz-1) dx dy = dx dy dz - 1: always inside the grid's floats, and scrambled for a non-cubic grid
HD uint32_t grid_idx(const grid_view& g, uint32_t i, uint32_t j, uint32_t k) { return umin(k, g.dx - 1) + umin(j, g.dy - 1) * g.dx + umin(i, g.dz - 1) * g.dx * g.dy; }
HD float grid_value(const grid_view& g, uint32_t i, uint32_t j, uint32_t k) { return g.data[grid_idx(g, i, j, k)]; }
// DenseVolGrid::sampleTrilinear (Volumes.h:157-181), as written: the weights come from the UNCLAMPED corner (+1) while the fetch is clamped (:167-176), value() is called
// (x, y, z) although its first argument is the slowest axis.  The corner's conversion is f2u (defined here, not in the reference)
HD float grid_trilinear(const grid_view& g, f3 vsP) {
    const f3 p = vsP - f3(0.5f);
    const uint32_t cx = f2u(p.x), cy = f2u(p.y), cz = f2u(p.z);
    float val = 0.0f;
    for (uint32_t i = 0; i < 2; i++) {
        const uint32_t cur_x = cx + i;
        const float w0 = 1 - fabsf(p.x - (float)cur_x);
        for (uint32_t j = 0; j < 2; j++) {
            const uint32_t cur_y = cy + j;
            const float w1 = 1 - fabsf(p.y - (float)cur_y);
            for (uint32_t k = 0; k < 2; k++) {
                const uint32_t cur_z = cz + k;
                const float w2 = 1 - fabsf(p.z - (float)cur_z);
                val += w0 * w1 * w2 * grid_value(g, uclamp(cur_x, 0u, g.dx - 1), uclamp(cur_y, 0u, g.dy - 1), uclamp(cur_z, 0u, g.dz - 1));
            }
        }
    }
    return val;
}

// one VolumeGrid: the region, its record and its grids
struct grid_region { const ctl_volume* V; const grid_rec* R; grid_view g, gA, gS; bool single; };
HD grid_region region_of(const table& T, uint32_t i) {
    grid_region G; G.V = &T.v[i]; G.R = &T.g[i]; G.single = G.R->single != 0;
    G.g = view_of(T, G.R->dim, G.R->off); G.gA = view_of(T, G.R->dim_a, G.R->off_a); G.gS = view_of(T, G.R->dim_s, G.R->off_s);
    return G;
}
HD f3 clamp01_3(f3 v) { return f3(clampf(v.x, 0.0f, 1.0f), clampf(v.y, 0.0f, 1.0f), clampf(v.z, 0.0f, 1.0f)); }
// VolumeGrid::tr (Volumes.h:247-252)
HD f3 grid_tr(const grid_region& G, f3 p, f3 dimF) { return clamp01_3(transform_point(G.V->world_to_volume.m, p)) * dimF; }
HD float density_a(const grid_region& G, f3 p) { return G.single ? grid_trilinear(G.g, grid_tr(G, p, dimf(G.g))) : grid_trilinear(G.gA, grid_tr(G, p, dimf(G.gA))); }   // :253-258
HD float density_s(const grid_region& G, f3 p) { return G.single ? grid_trilinear(G.g, grid_tr(G, p, dimf(G.g))) : grid_trilinear(G.gS, grid_tr(G, p, dimf(G.gS))); }   // :259-264
// VolumeGrid::sigma_a / sigma_s / sigma_t (Volumes.h:192-212); no insideWorld test: tr clamps the point into the grid
HD f3 grid_sigma_a(const grid_region& G, f3 p) { return a3(G.R->sa_min) + (a3(G.R->sa_max) - a3(G.R->sa_min)) * density_a(G, p); }
HD f3 grid_sigma_s(const grid_region& G, f3 p) { return a3(G.R->ss_min) + (a3(G.R->ss_max) - a3(G.R->ss_min)) * density_s(G, p); }
HD f3 grid_sigma_t(const grid_region& G, f3 p) {
    float a, s;
    if (G.single) a = s = grid_trilinear(G.g, grid_tr(G, p, dimf(G.g)));
    else { a = grid_trilinear(G.gA, grid_tr(G, p, dimf(G.gA))); s = grid_trilinear(G.gS, grid_tr(G, p, dimf(G.gS))); }
    return a3(G.R->sa_min) + (a3(G.R->sa_max) - a3(G.R->sa_min)) * a + a3(G.R->ss_min) + (a3(G.R->ss_max) - a3(G.R->ss_min)) * s;
}

// TraverseGridRay (SpatialGridTraversal.h:9-45) over AABB(0, 1) as a loop; `clb(rayT, cellEndT)` returns true to cancel.  As written:
//  - a direction component of magnitude <= 2^-40 gets inv_d = 1 / copysign(2^-40, d) (:27-30): one segment of negative length per such axis;
//  - the exit test compares the unsigned Pos, converted to float, with the float gridSize (:40): a step below zero wraps to 2^32 and leaves.
// The reference's `for (;;)` is BOUNDED here, in the host and the device function alike.  The argument: for finite input each iteration steps ONE axis of Pos by its
// Step.  An axis with Step = +1 or -1 moves monotonically, so after at most dim[axis] steps Pos[axis] has left [0, dim[axis]) (upwards, or wrapped below zero) and the
// exit test ends the loop: at most dim[axis] iterations step such an axis.  An axis with Step = 0 (an exactly zero direction component) has
// NextCrossingT = rayT + (cell face - p) * (+-2^40), finite, and DeltaT = cell * 2^40 >= 2^18 (a grid has at most 2^22 cells): it can be chosen, leaving Pos where it
// is — the zero-step of a degenerate axis — and each time its NextCrossingT grows by DeltaT.  It starts no lower than rayT - DeltaT, so after the first zero-step it is
// at least rayT, and after a second it exceeds maxT (the unit box's diagonal, sqrt(3), bounds maxT - rayT for the normalised direction): `maxT < NextCrossingT` then
// ends the loop or the axis is never the smallest again.  Usually that is one zero-step per degenerate axis and at most two; a degenerate axis spends none of its own
// dim[axis] >= 1 steps, so with one, two or three degenerate axes the count stays within dim.x + dim.y + dim.z + 3 (2 <= dim + 3 - 1 per such axis).  With a NaN
// NextCrossingT every comparison is false, the chosen axis may have Step 0 and neither exit test can fire: the reference never returns; here reaching the cap ends
// the traversal and is counted (`capped`).
template <class F> HD uint32_t traverse_grid(f3 o, f3 d, float tmin, float tmax, f3 gridSize, bool& capped, F clb) {
    capped = false;
    const f3 cell = f3(1.0f - 0.0f) / gridSize;                                      // box.Size() / gridSize
    float rayT = 0.0f, maxT = 3.402823466e+38f;
    if (!aabb_intersect(f3(0.0f), f3(1.0f), o, d, rayT, maxT)) return 0;             // box.Intersect(r, &rayT, &maxT): bounds 0 and FLT_MAX, written on a hit
    rayT = clampf(rayT, tmin, tmax);
    maxT = clampf(maxT, tmin, tmax);
    const f3 at = o + rayT * d;
    const f3 q = (at - f3(0.0f)) / cell;
    uint32_t Pos[3] = { f2u(floorf(clampf(q.x, 0.0f, gridSize.x - 1))), f2u(floorf(clampf(q.y, 0.0f, gridSize.y - 1))), f2u(floorf(clampf(q.z, 0.0f, gridSize.z - 1))) };
    const int Step[3] = { d.x > 0.0f ? 1 : (d.x < 0.0f ? -1 : 0), d.y > 0.0f ? 1 : (d.y < 0.0f ? -1 : 0), d.z > 0.0f ? 1 : (d.z < 0.0f ? -1 : 0) };
    const float ooeps = 0x1p-40f;                                                    // math::exp2(-40.0f)
    const f3 inv_d(1.0f / (fabsf(d.x) > ooeps ? d.x : copysign_bits(ooeps, d.x)), 1.0f / (fabsf(d.y) > ooeps ? d.y : copysign_bits(ooeps, d.y)), 1.0f / (fabsf(d.z) > ooeps ? d.z : copysign_bits(ooeps, d.z)));
    const f3 up(max2(0.0f, fsign(d.x)), max2(0.0f, fsign(d.y)), max2(0.0f, fsign(d.z)));
    const f3 next = f3(rayT) + (f3(0.0f) + (f3((float)Pos[0], (float)Pos[1], (float)Pos[2]) + up) * cell - at) * inv_d;
    const f3 delta(fabsf(cell.x * inv_d.x), fabsf(cell.y * inv_d.y), fabsf(cell.z * inv_d.z));
    float N[3] = { next.x, next.y, next.z };
    const float D[3] = { delta.x, delta.y, delta.z }, gs[3] = { gridSize.x, gridSize.y, gridSize.z };
    const uint32_t cap = f2u(gridSize.x) + f2u(gridSize.y) + f2u(gridSize.z) + 3u;
    uint32_t steps = 0;
    for (;;) {
        if (steps == cap) { capped = true; break; }
        steps++;
        const int bits = ((N[0] < N[1]) << 2) + ((N[0] < N[2]) << 1) + (N[1] < N[2]);
        const int axis = (0x00000a66 >> (bits * 2)) & 3;
        const bool cancel = clb(rayT, min2(N[axis], maxT));
        Pos[axis] += (uint32_t)Step[axis];
        if ((float)Pos[axis] >= gs[axis] || maxT < N[axis]) break;
        rayT = N[axis];
        N[axis] += D[axis];
        if (cancel) break;                                                           // `for (; !cancelTraversal;)`: looked at after the step
    }
    return steps;
}

// the ray in the region's space, as integrateDensity and invertDensityIntegral set it up (Volumes.cu:147-152, 177-184)
struct grid_ray { f3 o, d; float minTL, maxTL; f3 dimF; };
HD grid_ray local_ray(const grid_region& G, f3 o, f3 d, float t0, float t1) {
    grid_ray r; r.o = transform_point(G.V->world_to_volume.m, o);
    const f3 dl = transform_direction(G.V->world_to_volume.m, d);
    const float Td = length(dl);
    r.minTL = t0 * Td; r.maxTL = t1 * Td;
    r.d = normalized0(dl);
    r.dimF = G.single ? dimf(G.g) : f3(max2(G.gS.fx, G.gA.fx), max2(G.gS.fy, G.gA.fy), max2(G.gS.fz, G.gA.fz));   // the traversal resolution: max(gridS.dimF, gridA.dimF) (:152)
    return r;
}
// the two trilinear samples of a step, halved (Volumes.cu:155-163)
HD void step_density(const grid_region& G, const grid_ray& r, float rayT, float cellEndT, float& d_s, float& d_a) {
    const f3 a = r.o + rayT * r.d, b = r.o + cellEndT * r.d;
    if (G.single) d_s = d_a = grid_trilinear(G.g, dimf(G.g) * a) + grid_trilinear(G.g, dimf(G.g) * b);
    else {
        d_s = grid_trilinear(G.gS, dimf(G.gS) * a) + grid_trilinear(G.gS, dimf(G.gS) * b);
        d_a = grid_trilinear(G.gA, dimf(G.gA) * a) + grid_trilinear(G.gA, dimf(G.gA) * b);
    }
    d_s /= 2; d_a /= 2;
}
// VolumeGrid::integrateDensity (Volumes.cu:145-171).  As written: (sigAMax - sigAMin) is paired with D_s and (sigSMax - sigSMin) with D_a (:170)
HD f3 grid_integrate_density(const grid_region& G, f3 o, f3 d, float t0, float t1, uint32_t* steps_out = nullptr, bool* capped_out = nullptr) {
    const grid_ray r = local_ray(G, o, d, t0, t1);
    float D_s = 0.0f, D_a = 0.0f;
    bool capped;
    const uint32_t steps = traverse_grid(r.o, r.d, r.minTL, r.maxTL, r.dimF, capped, [&](float rayT, float cellEndT) {
        float d_s, d_a; step_density(G, r, rayT, cellEndT, d_s, d_a);
        D_s += d_s * (cellEndT - rayT);
        D_a += d_a * (cellEndT - rayT);
        return false;
    });
    if (steps_out) *steps_out = steps;
    if (capped_out) *capped_out = capped;
    const float Lcl_To_World = (t1 - t0) / (r.maxTL - r.minTL);
    D_a *= Lcl_To_World;
    D_s *= Lcl_To_World;
    return a3(G.R->sa_min) + (a3(G.R->sa_max) - a3(G.R->sa_min)) * D_s + a3(G.R->ss_min) + (a3(G.R->ss_max) - a3(G.R->ss_min)) * D_a;
}
// VolumeGrid::invertDensityIntegral (Volumes.cu:173-214).  As written: d_a is computed from the already overwritten d_s (:196-197); t has no t0 in it (:203)
HD bool grid_invert_density_integral(const grid_region& G, f3 o, f3 d, float t0, float t1, float desiredDensity, float& integratedDensity, float& t, float& densityAtMinT, float& densityAtT) {
    integratedDensity = densityAtMinT = densityAtT = 0.0f;
    const grid_ray r = local_ray(G, o, d, t0, t1);
    bool found = false;
    densityAtMinT = savg(grid_sigma_t(G, o + t0 * d));
    const float Lcl_To_World = (t1 - t0) / (r.maxTL - r.minTL);
    bool capped;
    traverse_grid(r.o, r.d, r.minTL, r.maxTL, r.dimF, capped, [&](float rayT, float cellEndT) {
        float d_s, d_a; step_density(G, r, rayT, cellEndT, d_s, d_a);
        d_s = savg(a3(G.R->ss_min) + (a3(G.R->ss_max) - a3(G.R->ss_min)) * d_s);
        d_a = savg(a3(G.R->sa_min) + (a3(G.R->sa_max) - a3(G.R->sa_min)) * d_s);
        const float D = (d_s + d_a) * (cellEndT - rayT) * Lcl_To_World;
        if (integratedDensity + D >= desiredDensity) {
            densityAtT = d_s + d_a;
            t = (desiredDensity - integratedDensity) / densityAtT + rayT * Lcl_To_World;
            integratedDensity = desiredDensity;
            found = true;
            return true;
        }
        integratedDensity += D;
        return false;
    });
    return found;
}
// VolumeGrid::tau (Volumes.cu:135-143)
HD f3 grid_tau(const grid_region& G, f3 o, f3 d, float minT, float maxT, uint32_t* steps_out = nullptr, bool* capped_out = nullptr) {
    if (steps_out) *steps_out = 0;
    if (capped_out) *capped_out = false;
    const float len = length(d);
    if (len == 0.0f) return f3(0.0f);
    const f3 dn = d / len;
    float t0, t1;
    if (!region_intersect(*G.V, o, dn, minT * len, maxT * len, t0, t1)) return f3(0.0f);
    return grid_integrate_density(G, o, dn, t0, t1, steps_out, capped_out);
}
// VolumeGrid::sampleDistance (Volumes.cu:216-239).  As written: no medium sampling weight; sigmaA is written from sigma_s (:231); on failure t / p / sigma* stay as
// they were; the result is success && pdfSuccess > 0; a miss of the region's box returns before anything of the record is written
HD bool grid_sample_distance(const grid_region& G, f3 o, f3 d, float minT, float maxT, float sample, medium_rec& mRec) {
    const float len = length(d);
    if (len == 0.0f) return false;
    const f3 dn = d / len;
    float t0, t1;
    if (!region_intersect(*G.V, o, dn, minT * len, maxT * len, t0, t1)) return false;
    float integratedDensity, densityAtMinT, densityAtT;
    const float desiredDensity = -fm::log(1 - sample);
    bool success = false;
    if (grid_invert_density_integral(G, o, dn, t0, t1, desiredDensity, integratedDensity, mRec.t, densityAtMinT, densityAtT)) {
        success = true;
        mRec.p = o + mRec.t * d;
        mRec.sigmaS = grid_sigma_s(G, mRec.p);
        mRec.sigmaA = grid_sigma_s(G, mRec.p);
    }
    const float expVal = fm::exp(-integratedDensity);
    mRec.pdfFailure = expVal;
    mRec.pdfSuccess = expVal * densityAtT;
    mRec.pdfSuccessRev = expVal * densityAtMinT;
    mRec.transmittance = f3(expVal);
    return success && mRec.pdfSuccess > 0;
}

}  // namespace vol
}  // namespace ctl
