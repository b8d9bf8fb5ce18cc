// prim_tracer.hip — the "PrimTracer" plugin ("direct" in main.cpp): the reference's non-progressive inspection tracer (Integrators/PrimTracer.{h,cu}),
// computePixel (PrimTracer.cu:19-106) re-cut at its primary trace:
//   k_prim_raygen        one lane per pixel of the rank's tiles: the aperture sample, sampleRayDifferential's main ray -> SoA rays of the wavefront traversal;
//   launch_intersect_closest  the primary rays through the shipped persistent traversal (alpha-tested, as traceRay always is);
//   k_prim_shade<CLASS>  one lane per pixel: re-derives its ray and differentials from the same sampler draw, reads the hit and evaluates the drawing mode.
// CLASS is chosen per launch from DrawingMode: kPrimGeometry (depth, normals, uv, barycentrics: no BSDF code) or kPrimShaded (the six first_* modes).
#include "kernels.h"
#define CTL_TEX_PARTIALS 1   // computePartials at the primary hit (PrimTracer.cu:36), image textures filtered with the ray differentials there
#include "shading.h"
#include "compaction.h"
#include "prim_tracer.h"
#include "single_ray.h"
#include "mitsuba_loader.h"   // unsupported_error
#include <climits>

namespace ctl {

// PathTrace_DrawMode (PrimTracer.h:7), in PTDM order
enum prim_mode { kLinearDepth, kD3DDepth, kVAbsdotNGeo, kVDotNGeo, kVDotNShade, kNGeoColored, kNShadeColored, kUv, kBaryCoords,
                 kFirstLe, kFirstF, kFirstFDirect, kFirstNonDeltaLe, kFirstNonDeltaF, kFirstNonDeltaFDirect };
enum { kPrimGeometry = 0, kPrimShaded = 1 };

struct prim_params {
    const float* t1; const float2* t2;   // sampler tables of the pass
    uint32_t width, height, tile_rank, tile_world, n_local_pixels;
    int mode, max_path_length;
    float near_depth, far_depth;         // SensorBase::m_fNearFarDepths
    float* depth_buffer; uint32_t depth_w, depth_h;   // IDepthTracer (nullptr = none)
    float* debug_out; uint32_t debug_x, debug_y;      // DebugInternal: one pixel, its L written here instead of the image
};

// local pixel index -> film pixel, the tile order of k_raygen / k_path_trace (kernels.h); Debug: the one pixel asked for
__device__ __forceinline__ void prim_pixel(const prim_params& P, uint32_t li, uint32_t& x, uint32_t& y) {
    if (P.debug_out) { x = P.debug_x; y = P.debug_y; return; }
    tile_order_pixel((P.width + 63) / 64, P.tile_rank, P.tile_world, li, x, y);
}
// rng = g_SamplerData(y * w + x); sampleRayDifferential(r, rX, rY, Vec2f(x, y), rng.randomFloat2()) — no sub-pixel jitter, the first draw is the aperture sample
__device__ __forceinline__ sampler prim_camera_ray(const dev_scene& S, const prim_params& P, uint32_t x, uint32_t y, f3& o, f3& d, f3& ox, f3& dx, f3& oy, f3& dy) {
    sampler rng{ P.t1, P.t2, y * P.width + x, 0, 0 };
    const f2 ap = rng.next2();
    sensor_sample_ray_differential(S.cam, f2{ (float)x, (float)y }, ap, o, d, ox, dx, oy, dy);
    return rng;
}
// DeviceDepthImage::NormalizeDepthD3D (Kernel/Tracer.h:26-31)
__device__ __forceinline__ float prim_depth_d3d(const prim_params& P, float t) {
    const float z = clampf(t, P.near_depth, P.far_depth);
    return (P.far_depth / (P.far_depth - P.near_depth) * z - P.far_depth * P.near_depth / (P.far_depth - P.near_depth)) / z;
}

// Rays of pixels outside the film (the last row / column of tiles) are still generated: the traversal gets a valid ray, the shade kernel drops the lane.
__global__ __launch_bounds__(256) void k_prim_raygen(dev_scene S, prim_params P, float4* __restrict__ ro, float4* __restrict__ rd, uint32_t* __restrict__ n_rays) {
    const uint32_t n = P.debug_out ? 1u : P.n_local_pixels;
    const uint32_t li = blockIdx.x * 256u + threadIdx.x;
    if (li == 0) *n_rays = n;
    if (li >= n) return;
    uint32_t x, y; prim_pixel(P, li, x, y);
    f3 o, d, ox, dx, oy, dy; (void)prim_camera_ray(S, P, x, y, o, d, ox, dx, oy, dy);
    ro[li] = make_float4(o.x, o.y, o.z, S.eps);              // traceRay(r): (eps, FLT_MAX), as trace_single(S, o, d, S.eps, FLT_MAX)
    rd[li] = make_float4(d.x, d.y, d.z, 3.402823466e+38f);
}

// TraceResult::getBsdfSample (Kernel/TraceResult.cu:16-43): fillDG, wi, the normal map, the two-sided flip
__device__ __forceinline__ const ctl_material& prim_bsdf_sample_rec(const dev_scene& S, f3 r_o, f3 r_d, float t, float u, float v, int tri, int node, bsdf_rec& b) {
    b.eta = 1.0f; b.sampled_type = 0; b.type_mask = kEAll;
    b.dg.P = r_o + t * r_d;
    fill_dg(S, u, v, tri, node, b.dg);
    b.wi = b.dg.sys.to_local(-r_d);
    const ctl_material& mat = S.mats[S.node_info[node].x + tri_mat_index(S, tri)];
    if (mat.map_kind != CTL_MAP_NONE) sample_normal_map(mat, b.dg);
    if (mat.two_sided && b.wi.z < 0) { b.dg.n = -b.dg.n; b.dg.sys.n = -b.dg.sys.n; b.wi.z *= -1.0f; }
    return mat;
}
// TraceResult::Le (TraceResult.cu:45-51)
__device__ __forceinline__ f3 prim_le(const dev_scene& S, const ctl_material& mat, int node, const bsdf_rec& b, f3 r_d) {
    const uint32_t nli = mat.node_light_index;
    if (nli == 0xffffffffu) return f3(0.0f);
    const uint4 ninfo = S.node_info[node];
    return light_eval(S, scene_lights(S)[nli == 0 ? ninfo.y : ninfo.z], b.dg.P, b.dg.sys.n, -r_d);
}
// UniformSampleOneLight + EstimateDirect (Kernel/TraceAlgorithms.cu:44-101), mask EAll & ~EDelta, with MIS; the shadow ray is traced inline
__device__ f3 prim_sample_one_light(const dev_scene& S, const ctl_material& mat, const bsdf_rec& b, sampler& rng, unsigned long long& rays) {
    if (!S.num_lights) return f3(0.0f);
    const f2 sl = rng.next2();
    float lpdf; const int li2 = sample_emitter(S, lpdf, sl.x);
    if (li2 < 0) return f3(0.0f);
    direct_rec dr; dr.ref = b.dg.P; dr.refN = b.dg.sys.n;
    const f3 value = light_sample_direct(S, scene_lights(S)[li2], dr, rng.next2());
    f3 r(0.0f);
    if (!is_zero(value)) {
        bsdf_rec b2 = b; b2.wo = b.dg.sys.to_local(dr.d); b2.type_mask = kEAll & ~kEDelta;
        const f3 bsdfVal = bsdf_f_top(mat, b2);
        if (!is_zero(bsdfVal)) {
            float st, su, sv; int stri, snode;
            rays++;
            if (!trace_single<true>(S, dr.ref, dr.d, S.eps, dr.dist - S.eps, st, su, sv, stri, snode)) {   // Occluded(r, 0, dist)
                float weight = 1.0f;
                if (dr.measure != kMeasureDiscrete) weight = power_heuristic((dr.measure == kMeasureArea ? dr.pdf * dr.dist / fabsf(dot(dr.n, dr.d)) : dr.pdf) * lpdf, bsdf_pdf_top(mat, b2));
                r = value * bsdfVal * weight;
            }
        }
    }
    return sdiv(r, lpdf);
}

// the first_* modes (PrimTracer.cu:50-96).  Delta chains and shadow rays are few (a chain starts only at a mirror / glass primary hit, a shadow ray only in the
// *_direct modes), so they are traced inline with the single-ray traversal instead of another queue round trip.  t is left at the last traced distance (for the depth buffer).
__device__ __noinline__ f3 prim_shade_first(const dev_scene& S, const prim_params& P, sampler& rng, f3 r_o, f3 r_d, f3 r_ox, f3 r_dx, f3 r_oy, f3 r_dy,
                                            float& t, float u, float v, int tri, int node, unsigned long long& rays) {
    bsdf_rec b;
    const ctl_material* mat = &prim_bsdf_sample_rec(S, r_o, r_d, t, u, v, tri, node, b);
    compute_partials(b.dg, r_ox, r_dx, r_oy, r_dy);
    b.wo = f3(0.0f, 0.0f, 1.0f);
    const f3 f_avg = bsdf_f_top(*mat, b);
    f3 Le = prim_le(S, *mat, node, b, r_d);
    f3 through(1.0f);   // Transmittance(r, 0, t): scenes with media are refused
    const bool isDelta = (mat->combined_type & kEDelta) != 0;
    const int mode = P.mode;
    if (mode == kFirstLe || (!isDelta && mode == kFirstNonDeltaLe)) return through * Le;
    if (mode == kFirstF || (!isDelta && mode == kFirstNonDeltaF)) return through * f_avg;
    if (mode == kFirstFDirect || (!isDelta && mode == kFirstNonDeltaFDirect)) return Le + through * (prim_sample_one_light(S, *mat, b, rng, rays) + f_avg * 0.5f);
    // a delta primary hit: follow the chain of non-smooth surfaces, as written (PrimTracer.cu:68-96) — `through *= f` on non-smooth hits only, the final Le and f unscaled
    float pdf_unused;
    f3 f = bsdf_sample_top(*mat, b, pdf_unused, rng.next2());
    through = through * f;
    int depth = 0; bool hit;
    do {
        r_o = b.dg.P; r_d = b.dg.sys.to_world(b.wo);
        int ntri, nnode;
        hit = trace_single<false>(S, r_o, r_d, S.eps, 3.402823466e+38f, t, u, v, ntri, nnode);
        rays++;
        if (!hit) t = 3.402823466e+38f;
        if (hit) {
            node = nnode;
            bsdf_rec nb;
            mat = &prim_bsdf_sample_rec(S, r_o, r_d, t, u, v, ntri, nnode, nb);
            b = nb;
            f = bsdf_sample_top(*mat, b, pdf_unused, rng.next2());
            if (!(mat->combined_type & kESmooth)) through = through * f;
        }
    } while (depth++ < P.max_path_length && hit && !(mat->combined_type & kESmooth));
    if (hit && (mat->combined_type & kESmooth)) {
        Le = prim_le(S, *mat, node, b, r_d);
        if (mode == kFirstNonDeltaLe) return Le;
        if (mode == kFirstNonDeltaF) return f;
        return Le + through * (prim_sample_one_light(S, *mat, b, rng, rays) + f * 0.5f);
    }
    return f3(0.0f);
}

template <int CLASS>
__global__ __launch_bounds__(256) void k_prim_shade(dev_scene S, prim_params P, const float4* __restrict__ hits, const int* __restrict__ hit_node, ctl_pixel_data* __restrict__ image,
                                                    unsigned long long* __restrict__ ray_count) {
    const uint32_t n = P.debug_out ? 1u : P.n_local_pixels;
    const uint32_t li = blockIdx.x * 256u + threadIdx.x;
    unsigned long long rays = 0;
    uint32_t x = 0, y = 0;
    if (li < n) prim_pixel(P, li, x, y);
    if (li < n && x < P.width && y < P.height) {
        f3 r_o, r_d, r_ox, r_dx, r_oy, r_dy;
        sampler rng = prim_camera_ray(S, P, x, y, r_o, r_d, r_ox, r_dx, r_oy, r_dy);
        const float4 h = hits[li];
        const int tri = __float_as_int(h.w);
        float t = tri >= 0 ? h.x : 3.402823466e+38f;
        rays = 1;   // traceRay(r)
        f3 L(0.0f);
        if (tri >= 0) {
            const int node = hit_node[li];
            if (CLASS == kPrimGeometry) {
                if (P.mode == kLinearDepth) L = f3((t - P.near_depth) / (P.far_depth - P.near_depth));
                else if (P.mode == kD3DDepth) L = f3(prim_depth_d3d(P, t));
                else {
                    // getBsdfSample without the BSDF record: the geometry modes read dg after the normal map and the two-sided flip.  computePartials changes
                    // none of n, sys.n, uv or the barycentrics, so it is left out here
                    diff_geom dg;
                    dg.P = r_o + t * r_d;
                    fill_dg(S, h.y, h.z, tri, node, dg);
                    const float wiz = dot(-r_d, dg.sys.n);   // dg.toLocal(-wi).z
                    const ctl_material& mat = S.mats[S.node_info[node].x + tri_mat_index(S, tri)];
                    if (mat.map_kind != CTL_MAP_NONE) sample_normal_map(mat, dg);
                    if (mat.two_sided && wiz < 0) { dg.n = -dg.n; dg.sys.n = -dg.sys.n; }
                    const int m = P.mode;
                    if (m == kVAbsdotNGeo) L = f3(absdot(-r_d, dg.n));
                    else if (m == kVDotNGeo) L = f3(dot(-r_d, dg.n));
                    else if (m == kVDotNShade) L = f3(dot(-r_d, dg.sys.n));
                    else if (m == kNGeoColored || m == kNShadeColored) { const f3 nn = ((m == kNGeoColored ? dg.n : dg.sys.n) + f3(1.0f)) / 2; L = nn; }
                    else if (m == kUv) L = f3(dg.uv.x, dg.uv.y, 0.0f);
                    else L = f3(h.y, h.z, 0.0f);   // bary_coords: fillDG's dg.bary = the hit's (u, v)
                }
            } else {
                L = prim_shade_first(S, P, rng, r_o, r_d, r_ox, r_dx, r_oy, r_dy, t, h.y, h.z, tri, node, rays);
            }
        } else if (S.env_map_index != 0xffffffffu) {   // EvalEnvironment(r, rX, rY)
            L = env_eval_differential(S, scene_lights(S)[S.env_map_index], r_d, r_dx, r_dy);
        }
        if (P.debug_out) { P.debug_out[0] = L.x; P.debug_out[1] = L.y; P.debug_out[2] = L.z; }
        else {
            add_sample(image, P.width, P.height, (float)x, (float)y, L);
            // g_DepthImage2.Store(x, y, prim_res.m_fDist): the LAST trace's distance, as the reference reuses prim_res along a delta chain
            if (P.depth_buffer && x < P.depth_w && y < P.depth_h) P.depth_buffer[(size_t)P.depth_w * y + x] = prim_depth_d3d(P, t);
        }
    }
    for (int off = 32; off > 0; off >>= 1) rays += __shfl_down(rays, off, 64);
    if ((threadIdx.x & 63) == 0 && rays) atomicAdd(ray_count, rays);
}

// ------------------------------------------------------------------------------------------------ PrimTracer
static const std::vector<std::string>& prim_mode_names() {
    static const std::vector<std::string> n = { "linear_depth", "D3D_depth", "v_absdot_n_geo", "v_dot_n_geo", "v_dot_n_shade", "n_geo_colored", "n_shade_colored", "uv", "bary_coords",
                                                "first_Le", "first_f", "first_f_direct", "first_non_delta_Le", "first_non_delta_f", "first_non_delta_f_direct" };
    return n;
}
PrimTracer::PrimTracer() {
    m_sParameters.addEnum("DrawingMode", kFirstF, prim_mode_names());   // PrimTracer.cu:244-248
    m_sParameters.addInterval("MaxPathLength", 7, 1, INT_MAX);
    grid_blocks = persistent_grid_blocks();   // the traversal's persistent grid, as the wavefront plugin sizes it
}
void PrimTracer::InitializeScene(Scene* s) {
    if (!s->S.flat_nodes) throw unsupported_error("PrimTracer: the scene must be created with CTL_SCENE_FLATTEN");
    s->refuse_volumes("PrimTracer");
    Tracer<false>::InitializeScene(s);
}
void PrimTracer::Resize(unsigned int _w, unsigned int _h) {
    const uint64_t n = shard_pixel_count(_w, _h, shard_rank, shard_world);
    if (n >= (1ull << 31)) throw std::runtime_error("PrimTracer::Resize: " + std::to_string(n) + " pixels exceed the 2^31 ray slots of the traversal");
    Tracer<false>::Resize(_w, _h);
    n_local_pixels = (uint32_t)n;
    const size_t cap = std::max<uint32_t>(1, n_local_pixels);
    ro_.alloc(cap); rd_.alloc(cap); hit_.alloc(cap); hit_node_.alloc(cap);
    if (!count_.p) { count_.alloc(1); n_rays_.alloc(1); work_.alloc(4); }
}
void PrimTracer::render(Image* I, const float* d_t1, const float* d_t2, float* debug_out, uint32_t dx, uint32_t dy) {
    const dev_scene& S = m_pScene->S;
    prim_params P{};
    P.t1 = d_t1; P.t2 = (const float2*)d_t2; P.width = w; P.height = h; P.tile_rank = shard_rank; P.tile_world = shard_world; P.n_local_pixels = n_local_pixels;
    P.mode = m_sParameters.getValue("DrawingMode"); P.max_path_length = m_sParameters.getValue("MaxPathLength");
    P.near_depth = m_pScene->near_depth; P.far_depth = m_pScene->far_depth;
    P.debug_out = debug_out; P.debug_x = dx; P.debug_y = dy;
    if (!debug_out) { P.depth_buffer = depth_buffer_; P.depth_w = depth_w_; P.depth_h = depth_h_; }
    const uint32_t n = debug_out ? 1u : n_local_pixels;
    if (n == 0) { host_count_ = 0; return; }   // more ranks than tiles: this rank owns nothing
    const uint32_t blocks = (n + 255) / 256;
    CTL_HIP(hipMemsetAsync(count_.p, 0, sizeof(unsigned long long), stream));
    CTL_HIP(hipMemsetAsync(work_.p, 0, 4 * sizeof(uint32_t), stream));
    const bool timed = !debug_out;
    if (timed) timer.begin(stream, 0);
    hipLaunchKernelGGL(k_prim_raygen, dim3(blocks), dim3(256), 0, stream, S, P, ro_.p, rd_.p, n_rays_.p);
    CTL_HIP(hipGetLastError());
    if (timed) { timer.end(stream); timer.begin(stream, 1); }
    const launch_ctx lc{ stream, grid_blocks, S.alpha_maps != 0 };   // traceRay always alpha-tests (TraceHelper.cu:88-180)
    launch_intersect_closest(lc, S, ro_.p, rd_.p, n_rays_.p, work_.p, hit_.p, hit_node_.p);
    CTL_HIP(hipGetLastError());
    if (timed) { timer.end(stream); timer.begin(stream, 2); }
    if (P.mode >= kFirstLe) hipLaunchKernelGGL(k_prim_shade<kPrimShaded>, dim3(blocks), dim3(256), 0, stream, S, P, (const float4*)hit_.p, (const int*)hit_node_.p, I->device(), count_.p);
    else hipLaunchKernelGGL(k_prim_shade<kPrimGeometry>, dim3(blocks), dim3(256), 0, stream, S, P, (const float4*)hit_.p, (const int*)hit_node_.p, I->device(), count_.p);
    CTL_HIP(hipGetLastError());
    if (timed) timer.end(stream);
    CTL_HIP(hipMemcpyAsync(&host_count_, count_.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    CTL_HIP(hipStreamSynchronize(stream));
}
void PrimTracer::DoRender(Image* I, const float* d_t1, const float* d_t2, unsigned int n_batch) {
    (void)n_batch;   // Tracer<false>: one pass per call of DoRender
    m_pScene->refuse_volumes("PrimTracer");
    render(I, d_t1, d_t2, nullptr, 0, 0);
    intersect_launches++;
    total_rays_ += host_count_;
}
void PrimTracer::takeRayCounts(uint64_t& path_rays, uint64_t& shadow_rays_) { path_rays = total_rays_; shadow_rays_ = 0; total_rays_ = 0; }
// PrimTracer::DebugInternal (PrimTracer.cu:214-221): computePixel for one pixel with the tables Debug() just generated; L is returned, the image is left as it is
void PrimTracer::DebugInternal(Image* I, unsigned int x, unsigned int y, const float* d_t1, const float* d_t2, float rgb[3]) {
    if (debug_.n < 3) debug_.alloc(3);
    if (!ro_.p) throw std::runtime_error("Debug: Resize was not called");
    render(I, d_t1, d_t2, debug_.p, x, y);
    CTL_HIP(hipMemcpyAsync(rgb, debug_.p, 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
    CTL_HIP(hipStreamSynchronize(stream));
}

} // namespace ctl
