// ORACLE — TEST INFRASTRUCTURE ONLY.
// ref_pathtrace_driver.cpp — extern "C" driver around the reference's own path-tracing loop: PathTrace<DIRECT> / PathTraceRegularization<DIRECT>
// (Integrators/PathTracer.cu:10-170) with everything they call per vertex — the host traceRay and its alpha test, TraceResult, EstimateDirect /
// UniformSampleOneLight / UniformSampleAllLights, Occluded, EvalEnvironment — and the per-pixel body of pathKernel2 (:186-193: sensor ray, path, Image::AddSample).
// `make ref` builds them as ONE generated unit (oracle/_ref/gen/pathtrace.cpp, git-ignored; the line ranges are listed in oracle/Makefile).
//
// A render points the reference's globals at the product's compiled scene (ctl_scene_desc):
//   g_SceneDataHost        meshes, BVH arrays, nodes, materials, lights (rebuilt from the flat descriptors the way INTEGRATION.md's converter maps them back:
//                          ref_bsdf_all_of, ref_material_of, ref_light_of), the anim blob, TriangleData, images, the light CDF, the camera, m_rayTraceEps,
//                          doAlphaMapping, the volume aggregate (ref_volume_driver.cpp ref_bind_volumes; empty for a scene without media)
//   t_nodesA / t_SceneNodes the node arrays the host traversal reads (the generated unit's two hand-written pointers)
//   g_SamplerDataHost      a SequenceSamplerData laid out over one pass's sequence tables (element * num_sequences + sequence, Kernel/Sampler_device.h:20-24),
//                          rebound per pass; its members are private and its constructor allocates, so the object is laid out in raw storage in the member order of
//                          Kernel/Sampler_device.h:15-18 / Base/SynchronizedBuffer.h (checked against sizeof and the class's own accessors)
//   g_RayTracedCounterHost zeroed, then read around every pixel: the rays that pixel's path traced (traceRay's Platform::Increment, TraceHelper.cu:176)
// and renders every pixel of every pass, one thread, into the reference's Image (raw storage, ref_image_view).  The pixel's sampler index is y * w + x, what
// TracerBase::getPixelIndex returns (Kernel/Tracer.h:89-97).  ref_primtracer_render does the same for one pass of the PrimTracer's computePixel
// (Integrators/PrimTracer.cu:19-106), with g_DepthImage2 pointed at the caller's depth buffer.  This file contains no reference source.
#include <Kernel/TraceHelper.h>
#include <Engine/Material.h>
#include <Engine/Mesh.h>
#include <Engine/Image.h>
#include <Engine/TriangleData.h>
#include <Engine/TriIntersectorData.h>
#include <SceneTypes/Node.h>
#include <SceneTypes/Light.h>
#include <SceneTypes/Sensor.h>
#include <Math/float4x4.h>
#include "../include/ctl_amd.h"
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace CudaTracerLib {
extern const BVHNodeData* t_nodesA;       // the generated unit's two node pointers
extern const BVHNodeData* t_SceneNodes;
template<bool DIRECT, bool REGU> void ref_path_pixel(unsigned int w, unsigned int h, Vec2i pixel, Sampler rng, Image& img, float m, int maxPathLength, int rrStart);
void ref_prim_pixel(int x, int y, Sampler& rng, Image& img, bool depth, int mode, int maxPathLength);   // the PrimTracer's computePixel (PrimTracer.cu:19-106)
void ref_prim_depth_image(float* data, int w, int h);                                                  // g_DepthImage2 (PrimTracer.cu:16)
}
using namespace CudaTracerLib;

void ref_bind_scene(const ctl_scene_desc* d);                                          // ref_scene_light_driver.cpp
void ref_light_of(const ctl_scene_desc* d, const ctl_light& L, Light& out);            // ref_scene_light_driver.cpp
void ref_bsdf_all_of(const ctl_material* mats, uint32_t idx, BSDFALL& out);            // ref_bsdf_driver.cpp
Material ref_material_of(const ctl_material& M);                                       // ref_material_driver.cpp
Image* ref_image_view(void* raw, size_t raw_size, void* pixels, int w, int h);         // ref_image_driver.cpp
void ref_bind_volumes(const ctl_volume* v, uint32_t n);                                // ref_volume_driver.cpp

namespace {
struct sync_buffer_layout { void* vptr; int location; unsigned length; void* host; void* device; };
struct sampler_data_layout { void* vptr; int location; void* buffers[3]; sync_buffer_layout d1, d2; unsigned num_sequences, sequence_length; };
static_assert(sizeof(sampler_data_layout) == sizeof(SequenceSamplerData), "member layout of SequenceSamplerData");
static_assert(sizeof(KernelMesh) == sizeof(ctl_kernel_mesh) && sizeof(TriIntersectorData) == sizeof(ctl_woop_tri) && sizeof(TriIntersectorData2) == sizeof(ctl_woop_index), "scene arrays");
static_assert(sizeof(BVHNodeData) == sizeof(ctl_bvh_node) && sizeof(float4x4) == sizeof(ctl_float4x4) && sizeof(TriangleData) == sizeof(ctl_triangle_data), "scene arrays");

std::vector<Node> g_nodes; std::vector<Material> g_mats; std::vector<Light> g_lights;

void bind_path_scene(const ctl_scene_desc* d, bool alpha) {
    ref_bind_scene(d);   // anim blob, TriangleData, images
    KernelDynamicScene& S = g_SceneDataHost;
    S.m_sBVHIntData.Data = (TriIntersectorData*)const_cast<ctl_woop_tri*>(d->woop); S.m_sBVHIntData.UsedCount = S.m_sBVHIntData.Length = d->n_woop;
    S.m_sBVHIndexData.Data = (TriIntersectorData2*)const_cast<ctl_woop_index*>(d->woop_index); S.m_sBVHIndexData.UsedCount = S.m_sBVHIndexData.Length = d->n_woop;
    S.m_sBVHNodeData.Data = (BVHNodeData*)const_cast<ctl_bvh_node*>(d->bvh_nodes); S.m_sBVHNodeData.UsedCount = S.m_sBVHNodeData.Length = d->n_bvh_nodes;
    S.m_sMeshData.Data = (KernelMesh*)const_cast<ctl_kernel_mesh*>(d->meshes); S.m_sMeshData.UsedCount = S.m_sMeshData.Length = d->n_meshes;
    g_nodes.assign(d->n_nodes, Node());
    for (uint32_t i = 0; i < d->n_nodes; i++) {
        const ctl_node& n = d->nodes[i]; Node& N = g_nodes[i];
        N.m_uMeshIndex = n.mesh_index; N.m_uMaterialOffset = n.material_offset; N.m_uInstanciatedMaterial = n.instanciated_material;
        N.m_uLights.set(n.lights, n.n_lights);
    }
    S.m_sNodeData.Data = g_nodes.data(); S.m_sNodeData.UsedCount = S.m_sNodeData.Length = d->n_nodes;
    g_mats.clear();
    for (uint32_t i = 0; i < d->n_materials; i++) {
        g_mats.push_back(ref_material_of(d->materials[i]));
        ref_bsdf_all_of(d->materials, i, g_mats.back().bsdf);
        g_mats.back().NodeLightIndex = d->materials[i].node_light_index;
    }
    S.m_sMatData.Data = g_mats.data(); S.m_sMatData.UsedCount = S.m_sMatData.Length = d->n_materials;
    g_lights.assign(d->n_lights_buf, Light());
    for (uint32_t i = 0; i < d->n_lights_buf; i++) ref_light_of(d, d->lights[i], g_lights[i]);
    S.m_sLightBuf.Data = g_lights.data(); S.m_sLightBuf.UsedCount = S.m_sLightBuf.Length = d->n_lights_buf;
    S.m_numLights = d->num_lights;
    for (int i = 0; i < MAX_NUM_LIGHTS; i++) { S.m_pLightIndices[i] = d->light_indices[i]; S.m_pLightCDF[i] = d->light_cdf[i]; }
    S.m_pLightPDF = nullptr;   // pdfEmitterDiscrete: not on the path
    S.m_uEnvMapIndex = d->env_map_index;
    S.m_sSceneBVH.m_sStartNode = d->scene_start_node; S.m_sSceneBVH.m_uNumNodes = d->n_scene_bvh_nodes;
    S.m_sSceneBVH.m_pNodes = (BVHNodeData*)const_cast<ctl_bvh_node*>(d->scene_bvh_nodes);
    S.m_sSceneBVH.m_pNodeTransforms = (float4x4*)const_cast<ctl_float4x4*>(d->node_transforms);
    S.m_sSceneBVH.m_pInvNodeTransforms = (float4x4*)const_cast<ctl_float4x4*>(d->node_inv_transforms);
    ref_bind_volumes(d->volumes, d->n_volumes);   // m_sVolume: the scene's regions, built by the reference's own constructors (none: the count is 0)
    S.m_sBox = AABB(Vec3f(d->box_min[0], d->box_min[1], d->box_min[2]), Vec3f(d->box_max[0], d->box_max[1], d->box_max[2]));
    S.doAlphaMapping = alpha;
    S.m_rayTraceEps = d->ray_trace_eps;
    const ctl_sensor& c = d->camera;
    if (c.type != CTL_SENSOR_PERSPECTIVE) throw std::runtime_error("ref_pathtrace_render: perspective sensors only");
    PerspectiveSensor cam((int)c.resolution[0], (int)c.resolution[1], 90.0f);
    cam.SetNearFarDepth(c.near_depth, c.far_depth);
    cam.fov = c.fov;
    NormalizedT<OrthogonalAffineMap> m; std::memcpy(m.data, c.to_world, 64);
    cam.SetToWorld(m);   // -> Update()
    S.m_Camera.SetData(cam);
    t_nodesA = S.m_sBVHNodeData.Data; t_SceneNodes = S.m_sSceneBVH.m_pNodes;
}

void bind_sampler(const float* t1, const float* t2) {
    sampler_data_layout L; std::memset(&L, 0, sizeof L);
    const unsigned n = CTL_SAMPLER_NUM_SEQUENCES * CTL_SAMPLER_SEQUENCE_LENGTH;
    L.location = DataLocation::Synchronized;
    L.d1.location = L.d2.location = DataLocation::Synchronized; L.d1.length = L.d2.length = n;
    L.d1.host = const_cast<float*>(t1); L.d2.host = const_cast<float*>(t2);
    L.num_sequences = CTL_SAMPLER_NUM_SEQUENCES; L.sequence_length = CTL_SAMPLER_SEQUENCE_LENGTH;
    SequenceSamplerData& D = *g_SamplerDataHost;
    std::memcpy((void*)&D, &L, sizeof L);
    if (D.getNumSequences() != CTL_SAMPLER_NUM_SEQUENCES || &D.getSequenceElement1(1, 2) != t1 + 2 * CTL_SAMPLER_NUM_SEQUENCES + 1 ||
        (const float*)&D.getSequenceElement2(3, 1) != t2 + 2 * (CTL_SAMPLER_NUM_SEQUENCES + 3))
        throw std::runtime_error("ref_pathtrace_render: the raw layout does not answer SequenceSamplerData's accessors");
}
}  // namespace

extern "C" {

// Renders n_passes passes of W x H pixels, one sample per pixel and pass, with pathKernel2<direct, regularization>'s per-pixel body.
// tables1 / tables2: n_passes consecutive (t1[30*4096], t2[30*4096*2]) pairs (the product's / the oracle's sampler tables).  alpha: doAlphaMapping.
// img: W x H ctl_pixel_data, added to; rays: W x H counters, added to (may be NULL).  Regularization's mollifier radius follows PathTracer::RenderBlock
// (PathTracer.cu:196-201) with m_uPassesDone = pass + 1.  Returns 0, or -1 with the reason on stderr.
int ref_pathtrace_render(const ctl_scene_desc* d, uint32_t W, uint32_t H, uint32_t n_passes, const float* tables1, const float* tables2, int direct, int regularization,
                         int maxPathLength, int rrStart, int alpha, ctl_pixel_data* img, uint32_t* rays) {
    try {
        bind_path_scene(d, alpha != 0);
        alignas(16) unsigned char raw[sizeof(Image)];
        Image* I = ref_image_view(raw, sizeof raw, img, (int)W, (int)H);
        if (!I) throw std::runtime_error("ref_pathtrace_render: image layout");
        const size_t N1 = (size_t)CTL_SAMPLER_NUM_SEQUENCES * CTL_SAMPLER_SEQUENCE_LENGTH;
        for (uint32_t pass = 0; pass < n_passes; pass++) {
            bind_sampler(tables1 + pass * N1, tables2 + pass * 2 * N1);
            const Vec3f ext = g_SceneDataHost.m_sBox.maxV - g_SceneDataHost.m_sBox.minV;
            const float initialRadius = ext.sum() / 100, ALPHA = 0.75f;
            const float radius2 = math::pow(math::pow(initialRadius, float(2)) / math::pow(float(pass + 1), 0.5f * (1 - ALPHA)), 1.0f / 2.0f);
            for (uint32_t y = 0; y < H; y++)
                for (uint32_t x = 0; x < W; x++) {
                    g_RayTracedCounterHost = 0;
                    const Sampler rng = (*g_SamplerDataHost)(y * W + x);   // TracerBase::getPixelIndex (Kernel/Tracer.h:89-97)
                    if (direct && regularization) ref_path_pixel<true, true>(W, H, Vec2i((int)x, (int)y), rng, *I, radius2, maxPathLength, rrStart);
                    else if (direct) ref_path_pixel<true, false>(W, H, Vec2i((int)x, (int)y), rng, *I, radius2, maxPathLength, rrStart);
                    else if (regularization) ref_path_pixel<false, true>(W, H, Vec2i((int)x, (int)y), rng, *I, radius2, maxPathLength, rrStart);
                    else ref_path_pixel<false, false>(W, H, Vec2i((int)x, (int)y), rng, *I, radius2, maxPathLength, rrStart);
                    if (rays) rays[(size_t)y * W + x] += g_RayTracedCounterHost;
                }
        }
        return 0;
    } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return -1; }
}

// One pass of the PrimTracer (Integrators/PrimTracer.cu:19-106): computePixel for every pixel, one sample each, drawing mode `mode` (PathTrace_DrawMode's order,
// Integrators/PrimTracer.h:7), the sampler index y * W + x.  t1 / t2: one pass's sampler tables.  alpha: doAlphaMapping.  img: W x H ctl_pixel_data, added to;
// depth: W x H floats that g_DepthImage2 stores into (NULL: computePixel's depthImage = false); rays: W x H counters, added to (may be NULL).
// Returns 0, or -1 with the reason on stderr.
int ref_primtracer_render(const ctl_scene_desc* d, uint32_t W, uint32_t H, const float* t1, const float* t2, int mode, int maxPathLength, int alpha,
                          ctl_pixel_data* img, float* depth, uint32_t* rays) {
    try {
        if (mode < 0 || mode > 14) throw std::runtime_error("ref_primtracer_render: drawing mode out of range");
        bind_path_scene(d, alpha != 0);
        bind_sampler(t1, t2);
        alignas(16) unsigned char raw[sizeof(Image)];
        Image* I = ref_image_view(raw, sizeof raw, img, (int)W, (int)H);
        if (!I) throw std::runtime_error("ref_primtracer_render: image layout");
        ref_prim_depth_image(depth, (int)W, (int)H);
        for (uint32_t y = 0; y < H; y++)
            for (uint32_t x = 0; x < W; x++) {
                g_RayTracedCounterHost = 0;
                Sampler rng = (*g_SamplerDataHost)(y * W + x);   // TracerBase::getPixelIndex (Kernel/Tracer.h:89-97)
                ref_prim_pixel((int)x, (int)y, rng, *I, depth != nullptr, mode, maxPathLength);
                if (rays) rays[(size_t)y * W + x] += g_RayTracedCounterHost;
            }
        ref_prim_depth_image(nullptr, 0, 0);
        return 0;
    } catch (const std::exception& e) { ref_prim_depth_image(nullptr, 0, 0); std::fprintf(stderr, "%s\n", e.what()); return -1; }
}

}  // extern "C"
