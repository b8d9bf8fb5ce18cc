// medium_stage.hip — the medium half of PathTrace<DIRECT> (Integrators/PathTracer.cu:17-58) as a stage of the wavefront: the WavefrontPathTracer plugin with
// ParticipatingMedia = true launches it once per depth, after the depth's closest hits are in Q.hit and the previous depth's shadow rays are resolved, in front of the
// shade stage.  One lane = one queued path vertex, as in the shade kernels (shade_kernel.inc), with the volume functions the megakernel's MEDIA instantiation runs
// (volume.h, volume_grid.h) in the megakernel's order (megakernel.hip path_trace), so that the two plugins draw the same numbers and multiply in the same order:
//   * the segment [0, dist] (dist = FLT_MAX for a miss) is intersected with the media; inside them ONE 1-D draw goes into sampleDistance;
//   * a sampled distance makes a medium vertex and the stage CONSUMES the slot: the pending NEE of the previous vertex is added, the throughput takes
//     sigmaS * transmittance / pdfSuccess, the attenuated emitter sample is deferred behind its shadow ray, the phase function gives the next direction, the
//     end-of-iteration rules of the shade kernel run, and the path goes to the next depth's queue (or ends); Q.hit[i].w = kHitConsumed tells the shade stage to skip the slot;
//   * otherwise the slot stays for the shade stage: the advanced 1-D sampler dimension is written back, and for a hit inside the media the throughput is rescaled by
//     transmittance / pdfFailure (:57-58).
// PathTrace's mRec lives across the bounces and sampleDistance does not always write it (no region found by sampleVolume; a VolumeGrid's box missed): the two fields
// a later bounce can then read stale — transmittance and pdfFailure — travel with the path in path_soa::mrec (DESIGN.md §11 has the lines).
#include "kernels.h"
#include "shading.h"
#include "compaction.h"
#include "volume.h"

namespace ctl {

template <bool GRID>
__device__ __forceinline__ void medium_stage(const dev_scene& S, const wave_queues& Q, const pass_params& P, const vol::table& V, int depth, ctl_pixel_data* __restrict__ image) {
    __shared__ uint32_t s_cnt[3][kWideBlock / 64]; __shared__ uint32_t s_base[3];
    const int cur = (depth - 1) & 1, nxt = depth & 1;
    const path_soa& A = Q.path[cur];
    const path_soa& B = Q.path[nxt];
    const uint32_t n = Q.counts[(depth - 1) * 4 + 0];
    uint32_t* n_next = &Q.counts[depth * 4 + 0];     // the shade kernel's own counters: it appends behind what this stage appended
    uint32_t* n_shadow = &Q.counts[depth * 4 + 1];
    uint32_t* n_final = &Q.counts[depth * 4 + 2];
    const uint32_t* occ_prev = Q.sh_occ[(depth - 1) & 1];
    float4* sh_o = Q.sh_o[depth & 1]; float4* sh_d = Q.sh_d[depth & 1];
    const uint32_t n_round = (n + (kBlock - 1u)) & ~(kBlock - 1u);   // whole workgroups iterate together (barriers in block_append3)
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n_round; i += gridDim.x * kBlock) {
        const bool active = i < n;
        bool consumed = false, alive = false, want_shadow = false;
        f3 cl(0.0f), cf(0.0f), directF(0.0f), new_o(0.0f), new_d(0.0f), sh_org(0.0f), sh_dir(0.0f);
        float sh_tmax = 0.0f; uint32_t pixel = 0, d1 = 0, d2 = 0, pass_b = 0, packed = 0; float2 px = make_float2(0.f, 0.f);
        float4 thr = make_float4(0.f, 0.f, 0.f, 0.f), nor = thr, carried = thr;
        if (active) {
            const float4 ro = A.ray_o[i], rd = A.ray_d[i], hit = Q.hit[i];
            thr = A.thr[i]; nor = A.nor[i];
            packed = __float_as_uint(nor.w);
            pass_b = (packed >> 16) & 0xffu;
            const float4 rad = A.rad[i];
            pixel = __float_as_uint(rad.w);
            const uint32_t n1 = CTL_SAMPLER_NUM_SEQUENCES * CTL_SAMPLER_SEQUENCE_LENGTH;
            sampler rng{ P.t1 + pass_b * n1, P.t2 + pass_b * n1, pixel, packed & 0xffu, (packed >> 8) & 0xffu };   // as the shade kernel rebuilds it
            const bool specularBounce = ((packed >> 24) & kFlagSpecular) != 0;
            cf = f3(thr.x, thr.y, thr.z);
            const f3 r_o(ro.x, ro.y, ro.z), r_d(rd.x, rd.y, rd.z);
            const int tri = __float_as_int(hit.w);
            const float dist = tri >= 0 ? hit.x : 3.402823466e+38f;   // r2.m_fDist of a miss is TraceResult::Init's FLT_MAX (megakernel.hip)
            vol::medium_rec mRec = vol::zero_rec();                    // a camera path starts from the megakernel's zero record ...
            if (depth > 1) { carried = A.mrec[i]; mRec.transmittance = f3(carried.x, carried.y, carried.z); mRec.pdfFailure = carried.w; }   // ... a later vertex from what the path carries
            float minT, maxT;
            const bool isInMedium = vol::intersect(V, r_o, r_d, 0.0f, dist, minT, maxT);
            // the distance draw is consumed whenever HasVolumes() && isInMedium, whatever the outcome
            if (V.n > 0 && isInMedium) consumed = vol::sample_distance<GRID>(V, r_o, r_d, 0.0f, dist, rng.next1(), mRec);
            carried = make_float4(mRec.transmittance.x, mRec.transmittance.y, mRec.transmittance.z, mRec.pdfFailure);
            if (!consumed) {
                // the slot is the shade stage's: it adds the pending NEE and shades the surface (or the miss) with the sampler where this stage left it
                if (V.n > 0 && isInMedium) {
                    A.nor[i].w = __uint_as_float((packed & 0xffffff00u) | (rng.d1 % CTL_SAMPLER_SEQUENCE_LENGTH));
                    if (tri >= 0) {   // PathTracer.cu:57-58, in the hasHit branch only
                        cf = cf * sdiv(mRec.transmittance, mRec.pdfFailure);
                        A.thr[i] = make_float4(cf.x, cf.y, cf.z, thr.w);
                    }
                    A.mrec[i] = carried;
                } else if (depth == 1) A.mrec[i] = carried;   // nothing has written the slot's record yet: the zero record
            } else {
                px = A.px[i];
                const float4 pend = A.pend[i];
                cl = f3(rad.x, rad.y, rad.z);
                // next-event estimation of the previous vertex, now that its shadow ray is resolved (shade_kernel.inc)
                const uint32_t sidx = __float_as_uint(pend.w);
                if (sidx != kNoShadow && !occ_prev[sidx]) cl = cl + f3(pend.x, pend.y, pend.z);
                if (depth == 1 && P.depth_buffer && tri >= 0) {   // IDepthTracer: the primary hit's depth, which the shade stage stores for the slots it keeps
                    const uint32_t dx = pixel % P.width, dy = pixel / P.width;
                    if (dx < P.depth_w && dy < P.depth_h) {
                        const float z = clampf(hit.x, P.depth_near, P.depth_far);
                        P.depth_buffer[(size_t)P.depth_w * dy + dx] = (P.depth_far / (P.depth_far - P.depth_near) * z - P.depth_far * P.depth_near / (P.depth_far - P.depth_near)) / z;
                    }
                }
                // PathTracer.cu:31-53 as megakernel.hip states it
                cf = cf * sdiv(mRec.sigmaS * mRec.transmittance, mRec.pdfSuccess);
                if (P.direct) {   // sampleAttenuatedEmitterDirect from DirectSamplingRecord(mRec.p, 0): ONE 2-D draw picks the emitter and, rescaled, samples it
                    direct_rec dr; dr.ref = mRec.p; dr.refN = f3(0.0f); dr.p = f3(0.0f); dr.pdf = 0.0f;
                    f2 sl = rng.next2();
                    f3 value(0.0f);
                    float lpdf; const int li = sample_emitter_reuse(S, lpdf, sl.x);
                    if (li >= 0) {
                        value = light_sample_direct(S, scene_lights(S)[li], dr, sl);
                        if (dr.pdf != 0) { dr.pdf *= lpdf; value = sdiv(value, lpdf); } else value = f3(0.0f);
                    }
                    value = value * vol::eval_transmittance<GRID>(V, dr.ref, dr.p);
                    if (!is_zero(value)) {
                        const float p = vol::phase_p<GRID>(V, mRec.p, -r_d, dr.d);
                        if (p != 0) {
                            const float weight = power_heuristic(dr.pdf, p);   // the phase value serves as f and as pdf
                            directF = cf * value * p * weight;
                            want_shadow = true;
                            sh_org = dr.ref; sh_dir = dr.d; sh_tmax = dr.dist - S.eps;   // Occluded(Ray(ref, d), 0, dist)
                        }
                    }
                }
                f3 wo(0.0f); float ppdf;   // no region found by Sample: weight 0, the path ends below
                cf = cf * vol::phase_sample_aggregate(V, mRec.p, -r_d, wo, ppdf, rng.next2());
                new_o = mRec.p; new_d = wo;
                // the end-of-iteration rules of the shade kernel; brdf_scattering_pdf (thr.w), last_nor and the specular flag stay those of the last surface
                alive = true;
                if (is_zero(cf)) alive = false;
                if (alive && depth >= P.max_path_length) {   // while (depth++ < maxPathLength).  PathTrace still plays the roulette of this iteration; its rescaled throughput is seen by the environment term below alone
                    alive = false;
                    if (tri < 0 && depth > P.rr_start_depth && !specularBounce) { const float q = max3c(cf); if (rng.next1() < q) cf = sdiv(cf, q); }
                }
                if (alive && depth > P.rr_start_depth && !specularBounce) {
                    const float q = max3c(cf);
                    if (rng.next1() >= q) alive = false; else cf = sdiv(cf, q);
                }
                if (!alive && tri < 0) {
                    // the path ends on a segment whose trace found nothing: PathTrace's `if (!r2.hasHit())` (PathTracer.cu:99-111) adds the environment along the ray as it
                    // now stands — the scattered direction — with the MIS weight of the last surface; without a map that is cf x Spectrum(0)
                    if (S.env_map_index != 0xffffffffu) {
                        const ctl_light& light = scene_lights(S)[S.env_map_index];
                        float misWeight = 1.0f;
                        if (!(!P.direct || depth == 1 || specularBounce)) misWeight = power_heuristic(thr.w, env_pdf_direct(S, light, new_d) * pdf_emitter(S, S.env_map_index));
                        cl = cl + misWeight * cf * env_eval(S, light, new_d);
                    } else cl = cl + cf * f3(0.0f);
                }
                d1 = rng.d1; d2 = rng.d2;
                Q.hit[i].w = __int_as_float(kHitConsumed);
            }
        }
        // ---- the shade kernel's stream compaction, on its counters: survivors, shadow rays and waiting terminations
        const block_slots bs = block_append3(n_shadow, want_shadow, n_next, alive, n_final, consumed && !alive && want_shadow, s_cnt, s_base);
        const uint32_t sslot = bs.s[0], nslot = bs.s[1], fslot = bs.s[2];
        if (!consumed) continue;
        if (want_shadow) { sh_o[sslot] = make_float4(sh_org.x, sh_org.y, sh_org.z, S.eps); sh_d[sslot] = make_float4(sh_dir.x, sh_dir.y, sh_dir.z, sh_tmax); }
        if (alive) {
            B.ray_o[nslot] = make_float4(new_o.x, new_o.y, new_o.z, S.eps);
            B.ray_d[nslot] = make_float4(new_d.x, new_d.y, new_d.z, 3.402823466e+38f);
            B.thr[nslot] = make_float4(cf.x, cf.y, cf.z, thr.w);
            B.rad[nslot] = make_float4(cl.x, cl.y, cl.z, __uint_as_float(pixel));
            B.nor[nslot] = make_float4(nor.x, nor.y, nor.z, __uint_as_float((d1 % CTL_SAMPLER_SEQUENCE_LENGTH) | ((d2 % CTL_SAMPLER_SEQUENCE_LENGTH) << 8) | (packed & 0xffff0000u)));
            B.pend[nslot] = make_float4(directF.x, directF.y, directF.z, __uint_as_float(want_shadow ? sslot : kNoShadow));
            B.px[nslot] = px;
            B.mrec[nslot] = carried;
        } else if (want_shadow) {
            Q.fin.rad[fslot] = make_float4(cl.x, cl.y, cl.z, __uint_as_float(sslot));
            Q.fin.dir[fslot] = make_float4(directF.x, directF.y, directF.z, 0.0f);
            Q.fin.px[fslot] = make_float4(px.x, px.y, __uint_as_float(pixel), __uint_as_float(pass_b));
        } else {
            add_sample_ordered(P, image, pixel, pass_b, px.x, px.y, cl);
        }
    }
}
// GRID = true is launched only for a table that holds a VolumeGrid region, so that the homogeneous kernel carries no march (as the megakernel's two media kernels)
template <bool GRID>
__global__ __launch_bounds__(kBlock) void k_medium_stage(dev_scene S, wave_queues Q, pass_params P, vol::table V, int depth, ctl_pixel_data* __restrict__ image) {
    medium_stage<GRID>(S, Q, P, V, depth, image);
}

void launch_medium_stage(const launch_ctx& lc, const dev_scene& S, const wave_queues& Q, const pass_params& P, const vol::table& V, int depth, ctl_pixel_data* image) {
    if (V.g) hipLaunchKernelGGL(k_medium_stage<true>, dim3(lc.grid_blocks), dim3(kBlock), 0, lc.stream, S, Q, P, V, depth, image);
    else hipLaunchKernelGGL(k_medium_stage<false>, dim3(lc.grid_blocks), dim3(kBlock), 0, lc.stream, S, Q, P, V, depth, image);
}

} // namespace ctl
