// shape_set.hip — the shape sets of the area lights on a skinned mesh, recomputed on the device from the rows a pose has just written (ctl_scene_bind_skin_ex with
// CTL_SKIN_AREA_LIGHTS): what scene_builder::recalculate_shape_set does on the host after ctl_builder_update_mesh.  Next-event estimation samples these tables — per-triangle
// world-space corners, normal and area, the normalised area CDF (the anim blob) and sum_area (the light record) —, so without them a posed emitter is lit from where it was.
// The kernels run the functions of shape_set.h, which the builder and the host yardstick (shape_sets_host, what ctl_shape_sets_host runs) call too.
//
//   k_shape_triangles   one lane per triangle of one light's shape set: i_dat / t_dat from the record in the anim blob, the Woop row from the leaf stream, the TriangleData,
//                       the node's forward transform (a kernel argument) -> p[3], n, area back into the record; i_dat, t_dat and pad stay.
//   k_shape_cdf         one workgroup per light.  The CDF is ShapeSet's running fp32 sum cdf[i+1] = cdf[i] + area[i], every entry then divided by the sum; fp32 addition is not
//                       associative, and a CDF that differs in the last bit picks another triangle for some samples, so the sum is SERIAL, in index order: the workgroup stages
//                       the areas through LDS in chunks of 1024 (the next chunk's loads are in flight while the sum runs), lane 0 carries the sum across the chunks (sixteen areas per
//                       step, RESULTS.md "Emissive skins": 7.7 ns per area), all lanes
//                       write the unnormalised entries and then divide the ones they wrote; lane 0 stores sum_area into the light's record.
// One launch pair per light (at most CTL_MAX_NUM_LIGHTS are sampled).  Plain launches on the null stream, in order; 256-lane workgroups; no workgroup waits for another; no atomics.
#include "tracer.h"
#include "shape_set.h"
#include "geometry_hash.h"
#include <string>

namespace ctl {

namespace {

constexpr uint32_t kCdfChunk = 1024u;   // areas per LDS chunk: four per lane

struct shape_device {
    unsigned char* anim; ctl_light* lights; const float4* leaf_tris; const uint4* tri_data; const float2* lut;
    uint32_t light, tri_off, cdf_off, count, n_rows, n_tris;   // n_rows / n_tris: the sizes of leaf_tris (in rows) and tri_data (in triangles)
    m34 l2w;
};

struct lut_decode {
    const float2* __restrict__ lut;
    __device__ __forceinline__ f3 operator()(uint32_t v) const { const float2 t = lut[(v >> 8) & 0xff], p = lut[256 + (v & 0xff)]; return f3(t.x * p.y, t.x * p.x, t.y); }   // uchar2_to_normal: (st * cp, st * sp, ct)
};

__global__ void __launch_bounds__(256) k_shape_triangles(shape_device K) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= K.count) return;
    float4* __restrict__ R = reinterpret_cast<float4*>(K.anim + K.tri_off) + (size_t)i * 4;
    const float4 r3 = R[3];   // area, i_dat, t_dat, pad
    const uint32_t i_dat = __float_as_uint(r3.y), t_dat = __float_as_uint(r3.z);
    if (i_dat >= K.n_rows || t_dat >= K.n_tris) return;   // cannot happen for a description the builder made; never read outside the arrays
    const float4* __restrict__ W = K.leaf_tris + (size_t)i_dat * 4;
    const float4 wa = W[0], wb = W[1], wc = W[2];
    const uint4 d0 = K.tri_data[(size_t)t_dat * 2], d1 = K.tri_data[(size_t)t_dat * 2 + 1];
    const float a[4] = { wa.x, wa.y, wa.z, wa.w }, b[4] = { wb.x, wb.y, wb.z, wb.w }, c[4] = { wc.x, wc.y, wc.z, wc.w };
    const uint32_t T[8] = { d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w };
    f3 p[3], n; float area;
    shape_triangle(a, b, c, T, K.l2w, lut_decode{ K.lut }, p, n, area);
    R[0] = make_float4(p[0].x, p[0].y, p[0].z, p[1].x);
    R[1] = make_float4(p[1].y, p[1].z, p[2].x, p[2].y);
    R[2] = make_float4(p[2].z, n.x, n.y, n.z);
    R[3] = make_float4(area, r3.y, r3.z, r3.w);
}

__global__ void __launch_bounds__(256) k_shape_cdf(shape_device K) {
    __shared__ __attribute__((aligned(16))) float s_in[kCdfChunk], s_out[kCdfChunk];
    __shared__ float s_total;
    const float4* __restrict__ R = reinterpret_cast<const float4*>(K.anim + K.tri_off);
    float* __restrict__ cdf = reinterpret_cast<float*>(K.anim + K.cdf_off);
    const uint32_t t = threadIdx.x, count = K.count;
    float next[4];
    auto load = [&](uint32_t base) {
        for (uint32_t j = 0; j < 4; j++) { const uint32_t i = base + t + 256u * j; next[j] = i < count ? R[(size_t)i * 4 + 3].x : 0.0f; }
    };
    load(0);
    float run = 0.0f;   // lane 0's is the sum
    for (uint32_t base = 0; base < count; base += kCdfChunk) {
        for (uint32_t j = 0; j < 4; j++) s_in[t + 256u * j] = next[j];
        __syncthreads();
        if (base + kCdfChunk < count) load(base + kCdfChunk);   // in flight during the sum
        const uint32_t n = count - base < kCdfChunk ? count - base : kCdfChunk;
        if (t == 0) {   // the serial sum, the adds in index order: sixteen areas per step through 16-B LDS accesses, the next step's loads issued before this step's adds
            const float4* in4 = reinterpret_cast<const float4*>(s_in); float4* out4 = reinterpret_cast<float4*>(s_out);
            const uint32_t n16 = n & ~15u;
            float4 v[4];
            if (n16) for (int k = 0; k < 4; k++) v[k] = in4[k];
            for (uint32_t i = 0; i < n16; i += 16u) {
                const uint32_t nx = i + 16u < n16 ? i + 16u : i;   // (the last step reads its own group again: no branch)
                float4 w[4], o[4];
                for (int k = 0; k < 4; k++) w[k] = in4[nx / 4u + k];
                for (int k = 0; k < 4; k++) { run = run + v[k].x; o[k].x = run; run = run + v[k].y; o[k].y = run; run = run + v[k].z; o[k].z = run; run = run + v[k].w; o[k].w = run; }
                for (int k = 0; k < 4; k++) { out4[i / 4u + k] = o[k]; v[k] = w[k]; }
            }
            for (uint32_t i = n16; i < n; i++) { run = run + s_in[i]; s_out[i] = run; }
        }
        __syncthreads();
        for (uint32_t j = 0; j < 4; j++) { const uint32_t i = t + 256u * j; if (i < n) cdf[(size_t)base + i + 1] = s_out[i]; }
    }
    if (t == 0) { s_total = run; K.lights[K.light].sum_area = run; }
    __syncthreads();
    const float total = s_total;
    // every lane divides the entries it wrote itself: 1 + t + 256 k (and lane 0 entry 0, which the host divides too: 0 / 0 is a NaN there and here)
    if (t == 0) cdf[0] = 0.0f / total;
    for (size_t i = (size_t)t + 1; i <= count; i += 256u) cdf[i] = cdf[i] / total;
}

}  // namespace

bool shape_set_of_mesh(const ctl_scene_desc& d, uint32_t li, uint32_t mesh) {
    if (li >= d.n_lights_buf) return false;
    const ctl_light& L = d.lights[li];
    if (L.type != CTL_LIGHT_DIFFUSE || L.count == 0 || L.node_idx >= d.n_nodes || d.nodes[L.node_idx].mesh_index != mesh) return false;
    const uint64_t cdf_end = (uint64_t)L.area_dist_index + ((uint64_t)L.count + 1) * 4, tri_end = (uint64_t)L.triangles_index + (uint64_t)L.count * sizeof(ctl_shape_tri);
    return (L.area_dist_index % 4) == 0 && (L.triangles_index % 16) == 0 && cdf_end <= d.n_anim_bytes && tri_end <= d.n_anim_bytes;
}

void shape_sets_host(const ctl_scene_desc& d, uint32_t mesh, const ctl_triangle_data* tri_data, const ctl_woop_tri* woop, ctl_light* lights_out, uint8_t* anim_out) {
    const char* who = "ctl_shape_sets_host";
    if (mesh >= d.n_meshes) throw std::runtime_error(std::string(who) + ": bad mesh index");
    if (!tri_data || !woop || (d.n_lights_buf && !lights_out) || (d.n_anim_bytes && !anim_out)) throw std::runtime_error(std::string(who) + ": null argument");
    if ((d.n_lights_buf && !d.lights) || (d.n_anim_bytes && !d.anim) || !d.nodes || !d.node_transforms) throw std::runtime_error(std::string(who) + ": the description lacks its light tables or nodes");
    const mesh_ranges R(d);
    const uint32_t tri0 = R.tri0[mesh], tri1 = R.tri1[mesh], woop0 = R.woop0[mesh], woop1 = R.woop1[mesh];
    if (d.n_lights_buf) std::memcpy(lights_out, d.lights, (size_t)d.n_lights_buf * sizeof(ctl_light));
    if (d.n_anim_bytes) std::memcpy(anim_out, d.anim, d.n_anim_bytes);
    for (uint32_t li = 0; li < d.n_lights_buf; li++) {
        if (!shape_set_of_mesh(d, li, mesh)) continue;
        ctl_light& L = lights_out[li];
        m34 l2w; std::memcpy(l2w.r, d.node_transforms[L.node_idx].m, 48);
        std::vector<ctl_shape_tri> st(L.count); std::vector<float> cdf((size_t)L.count + 1);
        std::memcpy(st.data(), anim_out + L.triangles_index, st.size() * sizeof(ctl_shape_tri));
        float sum = 0.0f; cdf[0] = 0.0f;
        for (uint32_t i = 0; i < L.count; i++) {   // recalculate_shape_set (scene_builder.cpp), over the arrays handed in
            ctl_shape_tri& s = st[i];
            if (s.i_dat < woop0 || s.i_dat >= woop1 || s.t_dat < tri0 || s.t_dat >= tri1) throw std::runtime_error(std::string(who) + ": light " + std::to_string(li) + " names a triangle outside mesh " + std::to_string(mesh));
            const ctl_woop_tri& w = woop[s.i_dat - woop0];
            uint32_t T[8]; std::memcpy(T, &tri_data[s.t_dat - tri0], 32);
            f3 p[3], n; float area;
            shape_triangle(w.a, w.b, w.c, T, l2w, [](uint32_t code) { return uchar2_to_normal(code); }, p, n, area);
            for (int k = 0; k < 3; k++) { s.p[k][0] = p[k].x; s.p[k][1] = p[k].y; s.p[k][2] = p[k].z; }
            s.n[0] = n.x; s.n[1] = n.y; s.n[2] = n.z; s.area = area;
            sum += area; cdf[i + 1] = cdf[i] + area;
        }
        for (uint32_t i = 0; i <= L.count; i++) cdf[i] = cdf[i] / sum;
        std::memcpy(anim_out + L.area_dist_index, cdf.data(), cdf.size() * sizeof(float));
        std::memcpy(anim_out + L.triangles_index, st.data(), st.size() * sizeof(ctl_shape_tri));
        L.sum_area = sum;
    }
}

// the shape sets of every light on a node that instances a mesh bound with CTL_SKIN_AREA_LIGHTS, from the arrays HBM holds and d's lights and node transforms: `d` is the
// description whose light tables were uploaded last.  Launches only; the caller synchronises.  Returns whether anything was launched.
bool Scene::launch_shape_sets(const ctl_scene_desc& d) {
    bool any = false;
    for (uint32_t mesh : skin_lights_) for (uint32_t li = 0; li < d.n_lights_buf; li++) {
        if (!shape_set_of_mesh(d, li, mesh)) continue;
        const ctl_light& L = d.lights[li];
        if ((size_t)li >= lights_.n || (size_t)d.n_anim_bytes > anim_.n) continue;   // (the upload sized both from d)
        shape_device K{};
        K.anim = anim_.p; K.lights = lights_.p; K.leaf_tris = leaf_tris_.p; K.tri_data = tri_data_.p; K.lut = shape_lut_.p;
        K.light = li; K.tri_off = L.triangles_index; K.cdf_off = L.area_dist_index; K.count = L.count; K.n_rows = (uint32_t)(leaf_tris_.n / 4); K.n_tris = (uint32_t)(tri_data_.n / 2);
        std::memcpy(K.l2w.r, d.node_transforms[L.node_idx].m, 48);
        hipLaunchKernelGGL(k_shape_triangles, dim3((L.count + 255u) / 256u), dim3(256), 0, nullptr, K); CTL_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_shape_cdf, dim3(1), dim3(256), 0, nullptr, K); CTL_HIP(hipGetLastError());
        any = true;
    }
    return any;
}

void Scene::run_shape_sets(const ctl_scene_desc& d) {
    last_shape_set_ms_ = 0;
    if (skin_lights_.empty()) return;
    struct event_pair { hipEvent_t a = nullptr, b = nullptr; ~event_pair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev;
    CTL_HIP(hipEventCreate(&ev.a)); CTL_HIP(hipEventCreate(&ev.b));
    CTL_HIP(hipEventRecord(ev.a, nullptr));
    const bool any = launch_shape_sets(d);
    CTL_HIP(hipEventRecord(ev.b, nullptr));
    CTL_HIP(hipEventSynchronize(ev.b));
    float ms = 0; if (any) CTL_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
    last_shape_set_ms_ = ms;
}

void Scene::enable_skin_lights(uint32_t mesh) {
    if (!shape_lut_.p) {
        std::vector<float> lut(1024); shape_normal_lut(lut.data());
        shape_lut_.alloc(512);
        CTL_HIP(hipMemcpy(shape_lut_.p, lut.data(), 4096, hipMemcpyHostToDevice));
    }
    skin_lights_.insert(mesh);
}

void Scene::read_lights(ctl_light* lights_out, uint32_t n_lights, uint8_t* anim_out, size_t n_anim_bytes) {
    require_device();
    if (!snap_) throw std::runtime_error("ctl_scene_read_lights: the scene holds no description");
    if (n_lights > snap_->d.n_lights_buf || n_anim_bytes > snap_->d.n_anim_bytes || (n_lights && !lights_out) || (n_anim_bytes && !anim_out))
        throw std::runtime_error("ctl_scene_read_lights: the scene holds " + std::to_string(snap_->d.n_lights_buf) + " lights and " + std::to_string(snap_->d.n_anim_bytes) + " bytes of light tables");
    CTL_HIP(hipDeviceSynchronize());
    if (n_lights) CTL_HIP(hipMemcpy(lights_out, lights_.p, (size_t)n_lights * sizeof(ctl_light), hipMemcpyDeviceToHost));
    if (n_anim_bytes) CTL_HIP(hipMemcpy(anim_out, anim_.p, n_anim_bytes, hipMemcpyDeviceToHost));
}

}  // namespace ctl
