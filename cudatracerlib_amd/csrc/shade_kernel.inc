// shade_kernel.inc — the shading stage of the wavefront (pathIterateKernel, Integrators/PseudoRealtime/WavefrontPathTracer.cu:51-164).  Two sets of per-path rules,
// one kernel build each: the default follows PathTrace<DIRECT> (Integrators/PathTracer.cu:10-113) — what the reference's deterministic megakernel renders and the
// oracle pins; CTL_SHADE_WAVEFRONT_RULES follows pathIterateKernel's own rules (tracer parameter PathSemantics = Wavefront): Russian roulette before sampling at
// pathDepth >= RRStartDepth, no sampling and no next-event estimation at the last bounce, sampleEmitterDirect with one 2-D sample drawn after the BSDF sample, the
// 16-bit previous normal, the t >= dDist (1 - eps) shadow rule.  Compiled once per feature set: the including file (shade_*.hip) defines CTL_SHADE_NAME, CTL_SHADE_FEATURES
// (bit mask, shading.h), CTL_SHADE_BLOCK (workgroup size: 1024 caps the kernel at 128 VGPRs, 512 at 256) and, where it holds the register allocation, CTL_SHADE_WAVES.
#ifndef CTL_SHADE_WAVEFRONT_RULES
#define CTL_SHADE_WAVEFRONT_RULES 0
#endif
// kernel k_shade_<name> and its launch function launch_shade_<name>, both with a _wf suffix in a build with CTL_SHADE_WAVEFRONT_RULES (kernels.h declares the launch functions)
#define CTL_SHADE_CAT_(a, b, c) a##b##c
#define CTL_SHADE_CAT(a, b, c) CTL_SHADE_CAT_(a, b, c)
#if CTL_SHADE_WAVEFRONT_RULES
#define CTL_SHADE_KERNEL CTL_SHADE_CAT(k_shade_, CTL_SHADE_NAME, _wf)
#define CTL_SHADE_LAUNCH CTL_SHADE_CAT(launch_shade_, CTL_SHADE_NAME, _wf)
#else
#define CTL_SHADE_KERNEL CTL_SHADE_CAT(k_shade_, CTL_SHADE_NAME, )
#define CTL_SHADE_LAUNCH CTL_SHADE_CAT(launch_shade_, CTL_SHADE_NAME, )
#endif
// CTL_SHADE_WAVES: the waves per SIMD the register allocation is held to (undefined or 0: the compiler's choice under __launch_bounds__)
#if defined(CTL_SHADE_WAVES) && CTL_SHADE_WAVES > 0
#define CTL_SHADE_ATTR __attribute__((amdgpu_waves_per_eu(CTL_SHADE_WAVES, CTL_SHADE_WAVES)))
#else
#define CTL_SHADE_ATTR
#endif
#ifndef CTL_SHADE_LDS_TABLES
// KB of LDS for the emitter records + anim blob (shading.h scene_lights / scene_anim; + 4 KB for the normal table): synthetic-SM shade 1.447 -> 1.356 ms per pass
#define CTL_SHADE_LDS_TABLES 12
#endif
// A model-class build (shade_class_*.hip) defines CTL_SHADE_KEYS: bit k = this launch shades the vertices whose traversal key (Q.mat_key: the BSDF model of the hit, 0 = miss) is k;
// CTL_SHADE_MODELS (shading.h), the models its dispatch switches carry, defaults to the same set (the nesting class carries all: a coating's inner model can be any).
#ifndef CTL_SHADE_KEYS
#define CTL_SHADE_KEYS 0xFFFFu
#elif !defined(CTL_SHADE_MODELS)
#define CTL_SHADE_MODELS CTL_SHADE_KEYS
#endif
#ifdef CTL_SHADE_CLASS   // index of the slot list this build reads (wave_queues::class_order)
#define CTL_SHADE_CLASSED 1
// ctl_math.h: one out-of-line copy of each transcendental function instead of one per call site (class b: 293 -> 159 KB of code against a 64-KB instruction cache)
#define CTL_FMATH_OUTLINE
// shading.h: no out-of-line emitter function takes the scene by reference — out of line they cost a private copy of the dev_scene argument (496 B of scratch per lane,
// read back with vector loads): synthetic-bathroom shade 2.52 -> 2.26 ms per pass
#define CTL_LIGHT_INLINE
#else
#define CTL_SHADE_CLASSED 0
#endif
#define CTL_HAS_KEY(k) ((((unsigned)(CTL_SHADE_KEYS)) >> (k)) & 1u)
// CTL_SHADE_PARK (the basic build): per-lane words that live long and are touched seldom — the radiance, the throughput, the pixel position, the pass number, the next
// direction — wait in LDS (s_park[word][lane]) instead of in registers while the hit point is set up and the BSDF and the light are evaluated; the code takes them out where it
// needs them and puts them back.  A lane reads only what it wrote itself, so the parking needs no barrier of its own.  Every floating-point operation and its order stay.
#ifndef CTL_SHADE_PARK
#define CTL_SHADE_PARK 0
#endif
#if CTL_SHADE_PARK && CTL_SHADE_WAVEFRONT_RULES
#error "CTL_SHADE_PARK is written for the default path rules"
#endif
// CTL_SHADE_MEDIA (shade_full_media.hip: 1, shade_full_media_grid.hip: 2 = the table may hold VolumeGrid regions): the build the WavefrontPathTracer launches behind
// k_medium_stage (medium_stage.hip) for a scene with participating media.  It takes the volume table as a further kernel argument, leaves the slots that stage consumed
// (Q.hit[i].w == kHitConsumed) alone, attenuates the surface NEE by the media's transmittance where EstimateDirect does, and hands path_soa::mrec on to the next depth.
// Undefined or 0: none of that is compiled — the builds without media keep their code.
#ifndef CTL_SHADE_MEDIA
#define CTL_SHADE_MEDIA 0
#endif
#if CTL_SHADE_MEDIA && (CTL_SHADE_WAVEFRONT_RULES || CTL_SHADE_PARK || CTL_SHADE_CLASSED)
#error "CTL_SHADE_MEDIA is written for the default path rules of the unclassed, unparked build"
#endif
// CTL_TEX_PARTIALS (shade_full_partials.hip): the build the WavefrontPathTracer launches for the vertices of depth 1 with TextureFiltering = true.  It re-derives the pixel's
// differential rays from the film position the path carries (path_soa::px) and the pixel's aperture draw, runs DifferentialGeometry::computePartials where PathTrace does
// (PathTracer.cu:60-61) and so hands every texture lookup of the vertex — the NEE's bsdf.f included — uv partials (shading.h tex_eval -> mipmap.h mip_eval).
// Undefined: none of that is compiled.
#if defined(CTL_TEX_PARTIALS) && (CTL_SHADE_WAVEFRONT_RULES || CTL_SHADE_PARK || CTL_SHADE_CLASSED || CTL_SHADE_MEDIA)
#error "CTL_TEX_PARTIALS is written for the default path rules of the unclassed, unparked build without media"
#endif
#include "kernels.h"
#include "shading.h"
#include "compaction.h"
#if CTL_SHADE_MEDIA
#include "volume.h"
#define CTL_SHADE_MEDIA_PARAM vol::table V,
#define CTL_SHADE_MEDIA_ARG V,
#else
#define CTL_SHADE_MEDIA_PARAM
#define CTL_SHADE_MEDIA_ARG
#endif

namespace ctl {

// ------------------------------------------------------------------------------------------------ shading
#if CTL_SHADE_PARK
// the lane's own index, opaque to the compiler: a read through it is not forwarded from the store that parked the word (forwarding would keep the word in its register)
__device__ __forceinline__ uint32_t park_lane() { uint32_t t = threadIdx.x; asm volatile("" : "+v"(t)); return t; }
#define CTL_PARK3(k, v) (s_park[k][threadIdx.x] = (v).x, s_park[(k) + 1][threadIdx.x] = (v).y, s_park[(k) + 2][threadIdx.x] = (v).z)
#define CTL_UNPARK3(k, v) ((v) = f3(s_park[k][park_lane()], s_park[(k) + 1][park_lane()], s_park[(k) + 2][park_lane()]))
#else
#define CTL_PARK3(k, v) ((void)0)
#define CTL_UNPARK3(k, v) ((void)0)
#endif
enum { kParkCl = 0, kParkCf = 3, kParkNewD = 6, kParkPx = 9, kParkPass = 11, kParkWords = 12 };
// One lane = one queued path vertex.  `depth` is the megakernel's 1-based depth of this vertex.
__global__ __launch_bounds__(CTL_SHADE_BLOCK) CTL_SHADE_ATTR void CTL_SHADE_KERNEL(dev_scene S, wave_queues Q, pass_params P, CTL_SHADE_MEDIA_PARAM int depth, ctl_pixel_data* __restrict__ image) {
    __shared__ uint32_t s_cnt[3][kWideBlock / 64]; __shared__ uint32_t s_base[3];
#if CTL_SHADE_PARK
    __shared__ float s_park[kParkWords][CTL_SHADE_BLOCK];
#endif
#if CTL_SHADE_LDS_TABLES
    scene_tables_to_lds<CTL_SHADE_BLOCK>(S);   // emitter records, anim blob, normal table: LDS for the whole launch (shading.h scene_lights / scene_anim / scene_normal_lut)
#endif
    const int cur = (depth - 1) & 1, nxt = depth & 1;
    const path_soa& A = Q.path[cur];
    const path_soa& B = Q.path[nxt];
#if CTL_SHADE_CLASSED
    const uint32_t n = Q.class_counts[depth * 8 + CTL_SHADE_CLASS];
#else
    const uint32_t n = Q.counts[(depth - 1) * 4 + 0];
#endif
    uint32_t* n_next = &Q.counts[depth * 4 + 0];
    uint32_t* n_shadow = &Q.counts[depth * 4 + 1];
    uint32_t* n_final = &Q.counts[depth * 4 + 2];
    const uint32_t* occ_prev = Q.sh_occ[(depth - 1) & 1];
    float4* sh_o = Q.sh_o[depth & 1]; float4* sh_d = Q.sh_d[depth & 1];

    const uint32_t n_round = (n + (CTL_SHADE_BLOCK - 1u)) & ~(CTL_SHADE_BLOCK - 1u);   // whole workgroups iterate together (barriers in block_append3)
    for (uint32_t j = blockIdx.x * CTL_SHADE_BLOCK + threadIdx.x; j < n_round; j += gridDim.x * CTL_SHADE_BLOCK) {
        bool active = j < n;
        uint32_t i = j;
#ifndef CTL_SHADE_SORT_WINDOW
#define CTL_SHADE_SORT_WINDOW CTL_SHADE_BLOCK   // lanes that exchange slots: the whole workgroup, or a power-of-two part of it (smaller window = the permuted reads stay closer)
#endif
#if CTL_SHADE_CLASSED
        // Model-class build: this launch shades the vertices of ITS models (CTL_SHADE_KEYS), from the list k_class_partition (kernels.hip) made of them — window after window of the
        // queue, by model inside a window: every wave is full, (mostly) of one model, and reads slots of one window; the other launches of the depth take the other lists.
        i = active ? Q.class_order[CTL_SHADE_CLASS][j] : 0u;
#else
        if (CTL_SHADE_SORT_WINDOW > 0) {
            // Workgroup-local regrouping: the lanes of a window exchange their path slots so that every wave shades (mostly) one BSDF model.
            // The slots stay inside the window's consecutive slots, so the permuted path-state reads touch the same
            // lines as the straight ones (a device-wide sort turns them into random gathers and loses more than the coherence wins, DESIGN.md §4).
            constexpr uint32_t kWin = CTL_SHADE_SORT_WINDOW > 0 ? CTL_SHADE_SORT_WINDOW : 64, kGroups = CTL_SHADE_BLOCK / kWin;
            __shared__ uint32_t s_hist[kGroups][64]; __shared__ uint16_t s_perm[CTL_SHADE_BLOCK];
            const uint32_t grp = threadIdx.x / kWin, lane_w = threadIdx.x % kWin;
            if (threadIdx.x < kGroups * 64) s_hist[threadIdx.x >> 6][threadIdx.x & 63] = 0;
            __syncthreads();
            uint32_t key = 63u;   // lanes past the end of the queue
            if (CTL_SHADE_FEATURES == 0 && active && P.key_from_traversal) key = Q.mat_key[i];   // basic build: the model of the hit's material, 0 for a miss — one coalesced byte the traversal left, no dependent chain
            else if (active) {
                const int tri = __float_as_int(Q.hit[i].w);
                key = 0u;         // misses
                if (tri >= 0) {   // BSDF model, then two bits of the material's index: the floor and the walls of a room are both rough plastic, with different maps
                    const uint32_t mi = S.node_info[Q.hit_node[i]].x + tri_mat_index(S, tri);
                    key = min((S.mats[mi].bsdf_type & 15u) << 2 | (mi & 3u), 62u);
                }
            }
            const uint32_t rank = atomicAdd(&s_hist[grp][key], 1u);
            __syncthreads();
            uint32_t before = 0;
            for (uint32_t k = 0; k < key; k++) before += s_hist[grp][k];
            s_perm[grp * kWin + before + rank] = (uint16_t)lane_w;
            __syncthreads();
            const uint32_t src = s_perm[threadIdx.x];
            const uint32_t j2 = j - lane_w + src;
            active = j2 < n;
            i = j2;
        }
#endif
#if CTL_SHADE_MEDIA
        if (active && __float_as_int(Q.hit[i].w) == kHitConsumed) active = false;   // the path scattered in a medium before this hit and k_medium_stage has moved it on: the slot is empty, like one beyond n
#endif
        bool alive = false, want_shadow = false, terminated = false;
        f3 cl(0.0f), cf(0.0f), directF(0.0f), new_o(0.0f), new_d(0.0f), last_nor(0.0f), sh_org(0.0f), sh_dir(0.0f);
        float bsdf_pdf_out = 0.0f, sh_tmax = 0.0f; uint32_t pixel = 0, d1 = 0, d2 = 0, pass_b = 0; bool specular = false; float2 px = make_float2(0.f, 0.f);
        if (active) {
            const float4 ro = A.ray_o[i], rd = A.ray_d[i], thr = A.thr[i], rad = A.rad[i], nor = A.nor[i], pend = A.pend[i];
            float4 hit = Q.hit[i]; const int hnode = Q.hit_node[i];
            if (P.u16_bary && __float_as_int(hit.w) >= 0) {   // the traversal result's 16-bit barycentric pair (Kernel/TraceHelper.cu:722-731 -> :44-51), parameter U16Barycentrics
                hit.y = (float)(uint16_t)(hit.y * 65535) / 65535.0f; hit.z = (float)(uint16_t)(hit.z * 65535) / 65535.0f;
            }
            px = A.px[i];
            pixel = __float_as_uint(rad.w);
            const uint32_t packed = __float_as_uint(nor.w);
            pass_b = (packed >> 16) & 0xffu;
#if CTL_SHADE_PARK
            s_park[kParkPx][threadIdx.x] = px.x; s_park[kParkPx + 1][threadIdx.x] = px.y; s_park[kParkPass][threadIdx.x] = __uint_as_float(pass_b);
#endif
            const uint32_t n1 = CTL_SAMPLER_NUM_SEQUENCES * CTL_SAMPLER_SEQUENCE_LENGTH;
            sampler rng{ P.t1 + pass_b * n1, P.t2 + pass_b * n1, pixel, packed & 0xffu, (packed >> 8) & 0xffu };
            bool specularBounce = ((packed >> 24) & kFlagSpecular) != 0;
            cl = f3(rad.x, rad.y, rad.z); cf = f3(thr.x, thr.y, thr.z);
            float brdf_scattering_pdf = thr.w;
            last_nor = f3(nor.x, nor.y, nor.z);
            // next-event estimation of the previous vertex: add it now that its shadow ray is resolved
            // (deferred `cl += cf * UniformSampleOneLight(...)`, PathTracer.cu:81-82)
            const uint32_t sidx = __float_as_uint(pend.w);
            if (sidx != kNoShadow && !occ_prev[sidx]) cl = cl + f3(pend.x, pend.y, pend.z);
            CTL_PARK3(kParkCl, cl); CTL_PARK3(kParkCf, cf);
            const f3 r_o(ro.x, ro.y, ro.z), r_d(rd.x, rd.y, rd.z);
            const int tri = __float_as_int(hit.w);
            if (depth == 1 && P.depth_buffer) {   // IDepthTracer: g_DepthImageWPT.Store(x, y, res.m_fDist) at pathDepth 0 (WavefrontPathTracer.cu:76-77, Kernel/Tracer.h:16-31)
                const uint32_t dx = pixel % P.width, dy = pixel / P.width;
                if (dx < P.depth_w && dy < P.depth_h) {
                    const float z = clampf(hit.x, P.depth_near, P.depth_far);   // DeviceDepthImage::NormalizeDepthD3D
                    P.depth_buffer[(size_t)P.depth_w * dy + dx] = (P.depth_far / (P.depth_far - P.depth_near) * z - P.depth_far * P.depth_near / (P.depth_far - P.depth_near)) / z;
                }
            }
            if (tri >= 0 && (CTL_SHADE_KEYS & 0xFFFEu)) {
                // TraceResult::getBsdfSample (Kernel/TraceResult.cu:11-43)
                bsdf_rec b;
                b.eta = 1.0f; b.sampled_type = 0; b.type_mask = kEAll;
                b.dg.P = r_o + hit.x * r_d;
                fill_dg(S, hit.y, hit.z, tri, hnode, b.dg);
                b.wi = b.dg.sys.to_local(-r_d);
                const uint4 ninfo = S.node_info[hnode];
#ifdef CTL_SHADE_PROBE_MAT_L1
                // TIMING PROBE (wrong materials): the material record addressed from the hit record alone, as if the traversal had deposited the material's index next to the hit —
                // the record's loads then issue together with TriangleData's instead of behind node_info + TriangleData (profiles/r05_shade_experiments.log)
                const ctl_material& mat = S.mats[min((uint32_t)hnode + CTL_SHADE_PROBE_MAT_L1 - 1u, S.n_materials_probe - 1u)];
#else
                const ctl_material& mat = S.mats[ninfo.x + tri_mat_index(S, tri)];
#endif
#if CTL_SHADE_FEATURES & 32
                if (mat.map_kind != CTL_MAP_NONE) sample_normal_map(mat, b.dg);   // after wi, as TraceResult.cu:30-34
#endif
                if (mat.two_sided && b.wi.z < 0) { b.dg.n = -b.dg.n; b.dg.sys.n = -b.dg.sys.n; b.wi.z *= -1.0f; }
#ifdef CTL_TEX_PARTIALS
                if (depth == 1) {   // PathTracer.cu:60-61: r2.getBsdfSample(r, bRec, ...) then bRec.dg.computePartials(r, rX, rY) — the differential rays of pathKernel2's sampleSensorRay (:186-190)
                    // the aperture sample is the second 2-D draw of this sample of the pixel (k_raygen); the path's sampler stands one draw behind it and has drawn nothing since.
                    // Only the thin-lens and the telecentric sensor read it (wave-uniform)
                    f2 ap{ 0.0f, 0.0f };
                    if (S.cam.type == CTL_SENSOR_THINLENS || S.cam.type == CTL_SENSOR_TELECENTRIC) { sampler aps = rng; aps.d2 = rng.d2 - 1u; ap = aps.next2(); }
                    f3 m_o, m_d, r_ox, r_dx, r_oy, r_dy;   // the main ray again (unused: the path carries it), then its x / y neighbours
                    sensor_sample_ray_differential(S.cam, f2{ px.x, px.y }, ap, m_o, m_d, r_ox, r_dx, r_oy, r_dy);
                    compute_partials(b.dg, r_ox, r_dx, r_oy, r_dy);
                }
#endif
                // emission, MIS-weighted against NEE of the previous vertex (PathTracer.cu:64-77)
                const uint32_t nli = mat.node_light_index;
                if (nli != 0xffffffffu) {
                    const uint32_t li = nli == 0 ? ninfo.y : ninfo.z;
                    const ctl_light& light = scene_lights(S)[li];
                    float misWeight = 1.0f;
                    if (!(!P.direct || depth == 1 || specularBounce)) {
                        const float direct_pdf = light_pdf_direct(light, r_d, last_nor, b.dg.n, hit.x) * pdf_emitter(S, li);
                        misWeight = power_heuristic(brdf_scattering_pdf, direct_pdf);
                    }
#if CTL_SHADE_WAVEFRONT_RULES
                    cl = cl + misWeight * light_eval(S, light, b.dg.P, b.dg.sys.n, -r_d) * cf;   // payload.L += misWeight * res.Le(...) * payload.throughput (WavefrontPathTracer.cu:99): the OTHER order than PathTrace's — one ulp in 1 % of the pixels (round 6, tools/r06_diag_wf.py)
#else
                    CTL_UNPARK3(kParkCl, cl); CTL_UNPARK3(kParkCf, cf);
                    cl = cl + misWeight * cf * light_eval(S, light, b.dg.P, b.dg.sys.n, -r_d);   // cl += misWeight * cf * r2.Le(...) (PathTracer.cu:76)
                    CTL_PARK3(kParkCl, cl);
#endif
                }
#if CTL_SHADE_WAVEFRONT_RULES
                // pathIterateKernel's own rules (WavefrontPathTracer.cu:101-141; pathDepth = depth - 1)
                bool surviveRR = true;
                if (depth - 1 >= P.rr_start_depth) {
                    const float q = max3c(cf);
                    if (rng.next1() < q) cf = sdiv(cf, q); else surviveRR = false;
                }
                if (depth != P.max_path_length && surviveRR) {
                    const f3 f = bsdf_sample_top(mat, b, brdf_scattering_pdf, rng.next2());
                    new_o = b.dg.P; new_d = b.dg.sys.to_world(b.wo);
                    specularBounce = (b.sampled_type & kEDelta) != 0;
                    if (P.direct && (mat.combined_type & kESmooth) && S.num_lights) {
                        // KernelDynamicScene::sampleEmitterDirect (KernelDynamicScene.cu:98-117): one 2-D sample, the emitter choice re-uses its first coordinate
                        f2 sl = rng.next2();
                        float lpdf; const int li = sample_emitter_reuse(S, lpdf, sl.x);
                        if (li >= 0) {
                            direct_rec dr; dr.ref = b.dg.P; dr.refN = b.dg.sys.n;
                            f3 value = light_sample_direct(S, scene_lights(S)[li], dr, sl);
                            if (dr.pdf != 0) { dr.pdf *= lpdf; value = sdiv(value, lpdf); } else value = f3(0.0f);
                            if (!is_zero(value)) {
                                b.type_mask = kEAll & ~kEDelta; b.wo = b.dg.sys.to_local(dr.d);
                                const f3 bsdfVal = bsdf_f_top(mat, b);
                                const float bp = bsdf_pdf_top(mat, b);
                                const float directPdf = dr.measure == kMeasureArea ? dr.pdf * dr.dist / fabsf(dot(dr.n, dr.d)) : dr.pdf;
                                directF = cf * value * bsdfVal * power_heuristic(directPdf, bp);
                                want_shadow = true;
                                sh_org = dr.ref; sh_dir = dr.d; sh_tmax = dr.dist * (1 - S.eps);   // unoccluded iff the closest hit lies at t >= dDist (1 - eps) (:66-69)
                            }
                        }
                    }
                    last_nor = uchar2_to_normal(normal_to_uchar2(b.dg.sys.n));   // payload.prev_normal (:137)
                    cf = cf * f;
                    alive = !is_zero(cf);
                }
#else
                const f3 f = bsdf_sample_top(mat, b, brdf_scattering_pdf, rng.next2());
                last_nor = b.dg.sys.n;
                // what the continuation needs of the sampled record is taken now: next-event estimation below re-uses the record itself (a copy of it costs ~45 registers)
                new_o = b.dg.P; new_d = b.dg.sys.to_world(b.wo);
                specularBounce = (b.sampled_type & kEDelta) != 0;
                CTL_PARK3(kParkNewD, new_d);
                if (P.direct && (mat.combined_type & kESmooth)) {
                    // UniformSampleOneLight + EstimateDirect (Kernel/TraceAlgorithms.cu:44-101), occlusion deferred.
                    // `cl += cf * UniformSampleOneLight(...)` (PathTracer.cu:81-82) is executed WHATEVER the estimate is — no light, a zero light sample, a zero BSDF value, an occluded
                    // shadow ray all return Spectrum(0), and cf x 0 is NaN for a NaN / infinite throughput (a BSDF evaluated outside its domain some vertices earlier): the sample is
                    // poisoned and Image::AddSample drops it.  The deferred term below only exists for an unoccluded, non-zero estimate, so the zero case is added as well (just before
                    // `cf = cf * f` below, where it costs no register: + 0 for every finite throughput, bit for bit).  Found by round 6's strict parity fuzz, seed 392: a Phong lobe that
                    // returned NaN, two specular vertices, then an OCCLUDED light sample (profiles/r06_fuzz.log).
                    if (S.num_lights) {
                        const f2 sl = rng.next2();
                        float lpdf; const int li = sample_emitter(S, lpdf, sl.x);
                        if (li >= 0) {
                            direct_rec dr; dr.ref = b.dg.P; dr.refN = b.dg.sys.n;
                            const f3 value = light_sample_direct(S, scene_lights(S)[li], dr, rng.next2());
                            if (!is_zero(value)) {
                                b.wo = b.dg.sys.to_local(dr.d); b.type_mask = kEAll & ~kEDelta;   // EstimateDirect's bRec (TraceAlgorithms.cu:62-64)
                                const f3 bsdfVal = bsdf_f_top(mat, b);
                                if (!is_zero(bsdfVal)) {
                                    float weight = 1.0f;
                                    if (dr.measure != kMeasureDiscrete) {
                                        const float bp = bsdf_pdf_top(mat, b);
                                        const float directPdf = (dr.measure == kMeasureArea ? dr.pdf * dr.dist / fabsf(dot(dr.n, dr.d)) : dr.pdf) * lpdf;
                                        weight = power_heuristic(directPdf, bp);
                                    }
                                    CTL_UNPARK3(kParkCf, cf);
#if CTL_SHADE_MEDIA
                                    directF = cf * sdiv((value * bsdfVal * weight) * vol::transmittance<(CTL_SHADE_MEDIA == 2)>(V, dr.ref, dr.d, 0.0f, dr.dist), lpdf);   // EstimateDirect(..., attenuated = true) (TraceAlgorithms.cu:65-67), the megakernel's order
#else
                                    directF = cf * sdiv(value * bsdfVal * weight, lpdf);
#endif
                                    want_shadow = true;
                                    sh_org = dr.ref; sh_dir = dr.d; sh_tmax = dr.dist - S.eps;   // Occluded(r, 0, dist) (KernelDynamicScene.cu:70-80)
                                }
                            }
                        }
                    }
                }
                CTL_UNPARK3(kParkCf, cf);
                if (P.direct && (mat.combined_type & kESmooth)) { CTL_UNPARK3(kParkCl, cl); cl = cl + cf * f3(0.0f); CTL_PARK3(kParkCl, cl); }   // the zero estimate of `cl += cf * UniformSampleOneLight(...)` (see above): at the NEE site itself it cost the rough-plastic class kernel 16 B of scratch and synthetic-bathroom 1.3 %, here 0.3 %
                cf = cf * f;
                alive = true;
                // a path whose throughput became exactly zero cannot contribute any more (the reference keeps tracing it
                // until Russian roulette removes it; radiance is identical)
                if (is_zero(cf)) alive = false;
                if (alive && depth >= P.max_path_length) alive = false;   // while (depth++ < maxPathLength)
                if (alive && depth > P.rr_start_depth && !specularBounce) {   // PathTracer.cu:91-96
                    const float q = max3c(cf);
                    if (rng.next1() >= q) alive = false; else cf = sdiv(cf, q);
                }
#endif
            }
#if CTL_SHADE_FEATURES & 8
            else if (CTL_HAS_KEY(0) && S.env_map_index != 0xffffffffu) {
                // miss with an environment emitter (PathTracer.cu:99-111), MIS-weighted against NEE of the previous vertex
                const ctl_light& light = scene_lights(S)[S.env_map_index];
                float misWeight = 1.0f;
                if (!(!P.direct || depth == 1 || specularBounce)) {
                    const float direct_pdf = env_pdf_direct(S, light, r_d) * pdf_emitter(S, S.env_map_index);
                    misWeight = power_heuristic(brdf_scattering_pdf, direct_pdf);
                }
                CTL_UNPARK3(kParkCl, cl); CTL_UNPARK3(kParkCf, cf);
                cl = cl + misWeight * cf * env_eval(S, light, r_d);
                CTL_PARK3(kParkCl, cl);
            }
#endif
            // a miss without an environment map still executes `cl += misWeight * cf * EvalEnvironment(r)` with EvalEnvironment == Spectrum(0) (PathTracer.cu:99-111,
            // KernelDynamicScene.cu:54-60): nothing for a finite throughput, NaN for a NaN / infinite one — the sample is then dropped by AddSample, as in the reference
            else if (CTL_HAS_KEY(0) && tri < 0) { CTL_UNPARK3(kParkCl, cl); CTL_UNPARK3(kParkCf, cf); cl = cl + cf * f3(0.0f); CTL_PARK3(kParkCl, cl); }
            terminated = !alive;
            specular = specularBounce; bsdf_pdf_out = brdf_scattering_pdf; d1 = rng.d1; d2 = rng.d2;
        }
        // ---- stream compaction: survivors, shadow rays and waiting terminations are appended densely, one atomic per wave
        const block_slots bs = block_append3(n_shadow, want_shadow, n_next, alive, n_final, terminated && want_shadow, s_cnt, s_base);
        const uint32_t sslot = bs.s[0], nslot = bs.s[1], fslot = bs.s[2];
        if (!active) continue;
#if CTL_SHADE_PARK
        CTL_UNPARK3(kParkCl, cl); px = make_float2(s_park[kParkPx][park_lane()], s_park[kParkPx + 1][park_lane()]); pass_b = __float_as_uint(s_park[kParkPass][park_lane()]);
#endif
        if (want_shadow) { sh_o[sslot] = make_float4(sh_org.x, sh_org.y, sh_org.z, S.eps); sh_d[sslot] = make_float4(sh_dir.x, sh_dir.y, sh_dir.z, sh_tmax); }
        if (alive) {
            CTL_UNPARK3(kParkNewD, new_d);
            B.ray_o[nslot] = make_float4(new_o.x, new_o.y, new_o.z, S.eps);
            B.ray_d[nslot] = make_float4(new_d.x, new_d.y, new_d.z, 3.402823466e+38f);
            B.thr[nslot] = make_float4(cf.x, cf.y, cf.z, bsdf_pdf_out);
            B.rad[nslot] = make_float4(cl.x, cl.y, cl.z, __uint_as_float(pixel));
            B.nor[nslot] = make_float4(last_nor.x, last_nor.y, last_nor.z, __uint_as_float((d1 % CTL_SAMPLER_SEQUENCE_LENGTH) | ((d2 % CTL_SAMPLER_SEQUENCE_LENGTH) << 8) | (pass_b << 16)   /* only d mod 30 matters (Sampler_device.h:98,104) */ | ((specular ? kFlagSpecular : 0u) << 24)));
            B.pend[nslot] = make_float4(directF.x, directF.y, directF.z, __uint_as_float(want_shadow ? sslot : kNoShadow));
            B.px[nslot] = px;
#if CTL_SHADE_MEDIA
            B.mrec[nslot] = A.mrec[i];   // PathTrace's mRec lives across the bounces: what k_medium_stage left in it travels on
#endif
        } else if (want_shadow) {
            Q.fin.rad[fslot] = make_float4(cl.x, cl.y, cl.z, __uint_as_float(sslot));
            Q.fin.dir[fslot] = make_float4(directF.x, directF.y, directF.z, 0.0f);
            Q.fin.px[fslot] = make_float4(px.x, px.y, __uint_as_float(pixel), __uint_as_float(pass_b));
        } else {
            add_sample_ordered(P, image, pixel, pass_b, px.x, px.y, cl);   // img.AddSample(pX.x, pX.y, col) (PathTracer.cu:192)
        }
    }
}

#if CTL_SHADE_MEDIA
void CTL_SHADE_LAUNCH(const launch_ctx& lc, const dev_scene& S, const wave_queues& Q, const pass_params& P, const vol::table& V, int depth, ctl_pixel_data* image) {
#else
void CTL_SHADE_LAUNCH(const launch_ctx& lc, const dev_scene& S, const wave_queues& Q, const pass_params& P, int depth, ctl_pixel_data* image) {
#endif
#ifndef CTL_SHADE_GRID_WAVES
#define CTL_SHADE_GRID_WAVES 4   // waves per SIMD the grid is sized for (the kernels are grid-stride loops over the queue)
#endif
    hipLaunchKernelGGL(CTL_SHADE_KERNEL, dim3(lc.grid_blocks / 8 * (kWideBlock / CTL_SHADE_BLOCK) * CTL_SHADE_GRID_WAVES / 4), dim3(CTL_SHADE_BLOCK), 0, lc.stream, S, Q, P, CTL_SHADE_MEDIA_ARG depth, image);   // 16 waves per CU by default
}

} // namespace ctl
