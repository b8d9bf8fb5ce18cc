// tracer.h — host-side plugin API: the reference's TracerBase / Tracer<PROGRESSIVE> / WavefrontPathTracer surface
// (Kernel/Tracer.h:67-294, Integrators/PseudoRealtime/WavefrontPathTracer.h:24-67) over HIP.
// Same virtuals, same parameter keys, same counters; errors are std::runtime_error as in the reference.
#pragma once
#include "../../include/ctl_amd.h"
#include "device_scene.h"
#include "kernels.h"
#include "sequence_generator.h"
#include "block_sampler.h"
#include "flatten.h"
#include <hip/hip_runtime.h>
#include <map>
#include <set>
#include <string>
#include <vector>
#include <memory>
#include <stdexcept>
#include <climits>

namespace ctl {

struct hip_error : std::runtime_error { using std::runtime_error::runtime_error; };
void throw_hip(hipError_t e, const char* file, int line);
#define CTL_HIP(x) do { hipError_t _e = (x); if (_e != hipSuccess) ::ctl::throw_hip(_e, __FILE__, __LINE__); } while (0)   // ThrowCudaErrors (Defines.h:98-99)

template <typename T> struct dbuf {   // tracked device allocation (Base/CudaMemoryManager.h)
    T* p = nullptr; size_t n = 0;
    dbuf() {}
    dbuf(const dbuf&) = delete; dbuf& operator=(const dbuf&) = delete;
    ~dbuf() { free(); }
    void alloc(size_t count) { free(); n = count; if (count) CTL_HIP(hipMalloc((void**)&p, count * sizeof(T))); }
    void free() { if (p) { (void)hipFree(p); p = nullptr; } n = 0; }
    void upload(const T* h, size_t count, hipStream_t s = 0) { if (count > n) alloc(count); if (count) CTL_HIP(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s)); }
};

// ctl_scene_desc_diff: the CTL_DIFF_* bits of what differs between two descriptions.  a_geometry: when given, `a` is a snapshot without its geometry arrays
// (triangles, Woop rows, mesh BVHs, texels, transmittance tables) and they are compared through the hashes of geometry_hash.h instead.  b_geometry (may be null)
// receives the hashes of `b` where the function made them (always when a_geometry is given and the counts agree): the ONE pass over b's geometry arrays of an update
// ignore_values (may be null): per mesh, non-zero = the VALUES of that mesh are not compared (a device-owned mesh, mesh_skin.hip): b's hash of it is a's
uint32_t scene_desc_diff(const ctl_scene_desc& a, const ctl_scene_desc& b, const geometry_hashes* a_geometry = nullptr, geometry_hashes* b_geometry = nullptr, const std::vector<uint8_t>* ignore_values = nullptr);
struct skin_binding;   // mesh_skin.hip
struct scene_volumes;  // scene_volumes.h: a scene's participating media in HBM
namespace vol { struct table; }   // volume.h
struct node_set_basis;   // flat_nodes.h
struct flat_rebuilder;   // flat_device.h
// the host copy of a description that a scene keeps to diff an update against (scene_update.hip)
struct desc_snapshot {
    ctl_scene_desc d{};   // pointers into the vectors below; the geometry arrays are null
    std::vector<ctl_kernel_mesh> meshes; std::vector<ctl_node> nodes; std::vector<ctl_material> materials; std::vector<ctl_light> lights; std::vector<uint8_t> anim;
    std::vector<ctl_bvh_node> top; std::vector<ctl_float4x4> xf, ixf; std::vector<ctl_mipmap> images;
    geometry_hashes geom;   // structure + per-mesh values (geometry_hash.h)
};

// dev_scene::inst_w_one of a flattened scene: every node transform affine with w == 1 exactly (what add_node produces), so the kernels skip the load of w and the division by it
inline int inverse_transforms_have_w_one(const ctl_scene_desc& d) { for (uint32_t k = 0; k < d.n_nodes; k++) if (d.node_inv_transforms[k].m[15] != 1.0f) return 0; return 1; }

// KernelDynamicScene in HBM (UpdateKernel, Kernel/TraceHelper.cu:182-217)
class Scene {
public:
    // flatten: also build the single-level world-space BVH (flatten.cpp) and make the intersect kernels use it
    // flat_format: flat_format of flatten.h, or -1 for the default (Q4 / $CTL_FLAT_FORMAT)
    explicit Scene(const ctl_scene_desc& d, bool flatten = false, int flat_format = -1, bool reduced_rough_transmittance = false);
    ~Scene();
    bool flattened() const { return S.flat_nodes != nullptr; }
    // ctl_scene_update (scene_update.hip): applies what differs between the description the scene holds and `d` in place — everything but topology — and returns the CTL_DIFF_* mask.
    // Throws std::runtime_error (topology differs; nothing was changed) or unsupported_error (a transform change on a tree that cannot be refitted).  Synchronous.
    uint32_t update(const ctl_scene_desc& d, ctl_scene_update_stats* stats);
    uint32_t last_mask() const { return last_mask_; }   // the CTL_DIFF_* bits the last update() found, also when it refused
    const ctl_scene_update_stats& last_update() const { return last_update_; }
    // ctl_scene_rebuild_flat (flat_rebuild.hip): a new flattened Q4 tree over the entries the scene holds, made on the device in place; refusals (unsupported_error) and failed
    // allocations leave the scene as it was.  Synchronous.
    void rebuild_flat(ctl_scene_rebuild_stats* stats);
    // ctl_scene_update_nodes (flat_nodes.hip): the description `d` with another set of nodes — old_of_new[k] = the node of the held description that node k was, or UINT32_MAX
    // for an added one — applied in place; `basis`: the small arrays of the held description (flat_nodes.h).  Refusals and failed allocations leave the scene as it was.  Synchronous.
    void update_nodes(const ctl_scene_desc& d, const uint32_t* old_of_new, uint32_t n_new_nodes, const node_set_basis& basis, ctl_scene_nodes_stats* stats);
    void read_flat_bvh(flat_scene& out);   // the device tree copied back, un-stamped: what flatten_scene handed to the upload, after any refit
    // skinned meshes (mesh_skin.hip; ctl_scene_bind_skin, ctl_scene_animate_mesh, ctl_scene_read_mesh_geometry, ctl_scene_unbind_skin).  A bound mesh is device-owned: update()
    // neither compares nor uploads its values
    // flags: CTL_SKIN_* (ctl_scene_bind_skin_ex); 0 = the plain call, which refuses a mesh whose nodes carry area lights
    void bind_skin(uint32_t mesh, const float* rest_positions, const float* rest_normals, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri, const uint8_t* bone_indices, const uint8_t* bone_weights, uint32_t n_bones, uint32_t flags = 0);
    void unbind_skin(uint32_t mesh);
    void animate_mesh(uint32_t mesh, const ctl_float4x4* bones0, const ctl_float4x4* bones1, float lerp, ctl_scene_update_stats* stats);
    void read_mesh_geometry(uint32_t mesh, float* positions_out, float* normals_out, ctl_triangle_data* tri_data_out, ctl_woop_tri* woop_out);
    float last_skin_ms() const { return last_skin_ms_; }   // HIP-event time of the three pose kernels of the last animate_mesh
    // the area lights of a mesh bound with CTL_SKIN_AREA_LIGHTS (shape_set.hip): their shape sets — ranges of anim_ and the sum_area of their records — are device-owned,
    // recomputed after every pose and after every upload of the light tables or the instance transforms
    float last_shape_set_ms() const { return last_shape_set_ms_; }   // HIP-event time of the shape-set kernels of the last call that ran them
    // ctl_scene_update_image (scene_images.hip): new level-0 texels for image `image` of the scene, same size — host memory, or device memory with CTL_IMAGE_TEXELS_DEVICE —
    // and everything the library derives from texels rebuilt in place: the pyramid in the texel pool, the sampling weights of the materials that read the image's average,
    // the environment light's CDFs and normalization.  Refusals (std::runtime_error, before the device is touched) leave the scene as it was.  Synchronous.
    void update_image(uint32_t image, const uint32_t* texels, uint32_t width, uint32_t height, uint32_t flags, ctl_scene_image_stats* stats);
    // ctl_scene_read_image: level 0 and the pyramid of one image as the pool holds them; texels_out may be null (the level table alone)
    void read_image(uint32_t image, uint32_t* texels_out, size_t capacity, uint32_t* levels_out, uint32_t* level_offsets_out);
    void read_lights(ctl_light* lights_out, uint32_t n_lights, uint8_t* anim_out, size_t n_anim_bytes);   // ctl_scene_read_lights: the light table and the anim blob as HBM holds them
    // the participating media (scene_volumes.h): the kernel argument as the last creation / update left it (n == 0: no media), read at every pass by the PathTracer plugin
    // and by the WavefrontPathTracer with ParticipatingMedia = true; whoever runs no medium code refuses a scene that has media instead of rendering it without them: unsupported_error naming `who` and the PathTracer plugin
    vol::table volume_table() const;
    void refuse_volumes(const char* who) const;
    dev_scene S{};
    uint32_t n_nodes = 0;
    float box_min[3] = { 0, 0, 0 }, box_max[3] = { 0, 0, 0 };   // KernelDynamicScene::m_sBox
    float near_depth = 0, far_depth = 0;                        // SensorBase::m_fNearFarDepths of the scene's camera (DeviceDepthImage::NormalizeDepthD3D)
private:
    friend struct flat_rebuilder;   // flat_device.h: builds a new tree beside the scene's and swaps it in
    // the upload, block by block: the constructor runs all of them, update() those whose part of the description changed.  None of them judges the description:
    // check_scene_desc (scene_checks.h) has, before the first of them runs
    void upload_top_level(const ctl_scene_desc& d);
    void upload_instances(const ctl_scene_desc& d);
    static void pack_instances(const ctl_scene_desc& d, std::vector<float4>& inst, std::vector<float4>& fwd, std::vector<uint4>& node_info);   // the records upload_instances uploads
    void upload_lights(const ctl_scene_desc& d);
    void upload_materials(const ctl_scene_desc& d);
    void set_shading_state(const shading_state& s) { S.shade_features = s.features; S.shade_models = s.models; S.alpha_maps = s.alpha_maps; }   // derive_shading_state (device_scene.h)
    void bind(const ctl_scene_desc& d);                   // device pointers and the scalars of the description into S
    void set_camera(const ctl_scene_desc& d);
    void snapshot(const ctl_scene_desc& d, const geometry_hashes* geom = nullptr);   // host copy of the description an update diffs against (the geometry arrays as hashes; geom: already made)
    // mesh_changed (may be null): per mesh, whether its vertex values differ (CTL_DIFF_GEOMETRY): the entries of those meshes get their new Woop rows first
    void refit_flat(const ctl_scene_desc& d, bool boxes, bool restamp, const std::vector<uint8_t>* mesh_changed, ctl_scene_update_stats* stats);
    // P = M_new * M_0^-1 per node of `d` (flat_refit.h, 12 doubles each), M_0 from xf0; throws "<who>: singular node transform"
    static std::vector<double> carry_matrices(const ctl_scene_desc& d, const std::vector<ctl_float4x4>& xf0, const char* who);
    std::vector<uint8_t> device_owned_meshes() const;   // per mesh, non-zero = bound to a skin (mesh_skin.hip): its values are the device's, whatever a description says; empty without bound meshes
    void upload_mesh_geometry(const ctl_scene_desc& d, const mesh_ranges& R, uint32_t mesh);   // the two-level arrays of one mesh, re-laid-out as the constructor does, into the same allocations
    bool reduced_rough_transmittance_ = false;
    std::map<uint32_t, std::shared_ptr<skin_binding>> skins_; float last_skin_ms_ = 0;   // the bound meshes
    void enable_skin_lights(uint32_t mesh);                // `mesh` joins skin_lights_; the first call uploads the normal-code table
    bool launch_shape_sets(const ctl_scene_desc& d);       // the shape-set kernels of every light on a node of a mesh in skin_lights_, by d's lights and node transforms
    void run_shape_sets(const ctl_scene_desc& d);          // the same between two events; waits for them and sets last_shape_set_ms_
    std::set<uint32_t> skin_lights_; dbuf<float2> shape_lut_; float last_shape_set_ms_ = 0;   // meshes bound with CTL_SKIN_AREA_LIGHTS; shape_normal_lut (shape_set.h) in HBM
    // the texel pool on the host side: per image the offset of its level 0 in texels_, its level table and {r, g, b, 1} of ImageTexture::Average() (mip_image_average) — what
    // update_image re-runs material_update_textures with; env_scratch_: one colSum per row of the environment map and rowSum
    std::vector<size_t> image_off_; std::vector<dev_mip_levels> image_levels_; std::vector<float> image_avg_; dbuf<float> env_scratch_;
    bool lights_stale_ = false;   // an emissive skin was unbound: lights_ / anim_ hold no description's values, the next update uploads them whatever the diff says
    ctl_scene_update_stats last_update_{}; uint32_t last_mask_ = 0;
    std::unique_ptr<desc_snapshot> snap_;
    std::unique_ptr<scene_volumes> volumes_;   // made by the first snapshot(), written in place by every later one
    flat_scene::refit_side refit_;   // host part: xf0, level_start
    std::vector<uint32_t> flat_missing_tris_;   // triangles of instanced meshes without a leaf entry (flatten.h flat_missing_triangles): a geometry update cannot bring them back
    dbuf<uint32_t> refit_tri_row_, refit_node_changed_;   // made by the first geometry update: triangle -> row of leaf_tris_ (triangle_woop_rows); per node, whether its mesh changed
    std::vector<int32_t> flat_child_links_;
    size_t flat_n_nodes_ = 0, flat_n_entries_ = 0, flat_slab_nodes_ = 0; int flat_max_depth_ = 0; bool flat_root_slab_ = false;
    dbuf<uint32_t> refit_part_index_, refit_level_nodes_; dbuf<refit_box> refit_part_boxes_, refit_ebox_, refit_nbox_; dbuf<double> refit_carry_, refit_area_;
    dbuf<unsigned char> rebuild_temp_;   // rocPRIM's temporary storage (sort and scan), sized by its query calls, kept between rebuilds
    dbuf<float4> top_nodes_, bot_nodes_, leaf_tris_, inst_, inst_fwd_, flat_nodes_, flat_leaves_; dbuf<float2> normal_lut_;
    dbuf<uint4> tri_data_, node_info_;
    dbuf<ctl_material> mats_; dbuf<ctl_light> lights_; dbuf<unsigned char> anim_; dbuf<uint32_t> texels_; dbuf<ctl_mipmap> images_; dbuf<dev_mip_levels> mip_levels_; dbuf<float> mip_lut_; dbuf<float> rt_data_, rt_reduced_; dbuf<ctl_rough_transmittance> rt_;
};

// Engine/Image.h:31-91 (accumulator part)
class Image {
public:
    Image(uint32_t w, uint32_t h);
    ~Image() { for (auto e : ev_) if (e) (void)hipEventDestroy(e); }
    Image(const Image&) = delete; Image& operator=(const Image&) = delete;
    void Clear();
    uint32_t getWidth() const { return w_; }
    uint32_t getHeight() const { return h_; }
    ctl_pixel_data* device() { return px_.p; }
    bool holds_reduced_frame() const { return reduced_; }   // set on every rank by an in-place ctl_image_reduce / ctl_image_gather of more than one rank (comm.cpp), cleared by Clear() / write()
    void mark_reduced(bool v) { reduced_ = v; }
    void read(ctl_pixel_data* host);
    void write(const ctl_pixel_data* host);
    void add_samples(uint32_t n, const float* host_samples5);   // Image::AddSample (Engine/Image.cu:22-44) for n host samples {sx, sy, r, g, b}
    void resolve_rgb(float splat_scale, float* host_rgb);
    void apply_pipeline(float splat_scale, uint32_t* host_rgbcol);                 // applyImagePipeline without filter / post-process
    void apply_pipeline_ex(float splat_scale, const ctl_reconstruction_filter* filter, const ctl_tonemap* process, uint32_t* host_rgbcol);   // image_pipeline.hip
    // applyImagePipeline with the NonLocalMeansFilter (nlm_filter.hip).  The per-pixel variance (computeVariance(), w x h floats) comes from the tracer's
    // PixelVarianceBuffer (device to device) or from host memory: exactly one of the two is given
    void apply_pipeline_nlm(float splat_scale, const ctl_nlm_filter& nlm, const PixelVarianceBuffer* tracer_variance, hipStream_t tracer_stream, const float* host_variance,
                            const ctl_tonemap* process, uint32_t* host_rgbcol);
    void read_filtered(uint32_t* host_rgbe);                                       // Image::getFilteredData: the RGBE plane the last filter / post-process call left
    float last_filter_ms() const { return filter_ms_; }                            // HIP-event time of the NonLocalMeans kernels of the last apply_pipeline_nlm
    bool luminance_info(float out[4]) const { if (!have_lum_) return false; for (int i = 0; i < 4; i++) out[i] = lum_info_[i]; return true; }   // Image::ComputeLuminanceInfo as the last tone-mapped call used it
    void write_file(float splat_scale, const char* path);                          // Image::WriteDisplayImage (Engine/Image.cpp:67-75)
private:
    void pipeline_tail(const ctl_tonemap* process, uint32_t* host_rgbcol);         // the post-process or the plain conversion of the filtered plane, then the D2H
    bool have_lum_ = false; float lum_info_[4] = { 0, 0, 0, 0 };                    // (min, max, avg, logAvg) of the last pipeline_tail with a post-process
    bool reduced_ = false; float filter_ms_ = 0; hipEvent_t ev_[2] = { nullptr, nullptr };   // ev_: around the NonLocalMeans kernel, created on first use
    uint32_t w_, h_; dbuf<ctl_pixel_data> px_; dbuf<float> rgb_, variance_; dbuf<uint32_t> out_, filtered_; dbuf<int> lum_;   // filtered_: m_filteredColorsDevice (RGBE)
};
// nlm_filter.hip: one fused launch on `s`; variance = computeVariance() per pixel (device), filtered_rgbe = the RGBE plane written
// flat_refit.hip: the refit of the Q4 tree on the device, the arithmetic of flat_refit.h.  Plain launches on `s`, deepest level first; no kernel waits for another workgroup.
struct refit_device {
    float4* nodes; float4* leaves; uint32_t n_nodes, n_entries; int compact;
    uint32_t* part_index; const refit_box* part_boxes; const double* carry;   // side data; carry = P per scene node (12 doubles).  k_deform_entries writes part_index
    const float4* inst; const float4* inst_fwd;                                       // the scene's node transforms, as the two-level traversal keeps them
    refit_box* ebox; refit_box* nbox;                                                 // scratch: the new box of every entry / node
    // re-stamp of the model nibble (index bits 28..31) and the alpha bit (node bit 31) of every entry from node_info + tri_data + the materials;
    // restamp: 0 = leave the bits alone, else the NUMBER of materials (a material index beyond it is never read)
    int restamp, leaf_keys, alpha_maps; const uint4* tri_data; const uint4* node_info; const ctl_material* mats;
};
// a geometry update (k_deform_entries): the entries of the nodes marked in node_changed take rows 0..2 of their triangle from the two-level leaf stream (leaf_tris, 64-B
// stride, already holding the new values), through tri_row (triangle -> row), and stand for their whole triangle from then on
struct deform_device { const uint32_t* node_changed; uint32_t n_scene_nodes; const uint32_t* tri_row; uint32_t n_tris; const float4* leaf_tris; uint32_t n_rows; };
void launch_deform_entries(hipStream_t s, const refit_device& R, const deform_device& D);
void launch_refit_entries(hipStream_t s, const refit_device& R, bool boxes);
void launch_refit_level(hipStream_t s, const refit_device& R, const uint32_t* level_nodes, uint32_t count);
void launch_refit_area(hipStream_t s, const float4* nodes, uint32_t n_nodes, double* sum_out);   // adds the nodes' box areas to *sum_out
void launch_nlm_filter(hipStream_t s, const ctl_pixel_data* px, const float* variance, uint32_t w, uint32_t h, float splat_scale, float k, float sigma2_scale, uint32_t* filtered_rgbe);

// Kernel/TracerSettings.h:14-350 — typed parameters with interval / set constraints: bool, int and float intervals (IntervalParameterConstraint), and
// enumerations (SetParameterConstraint over the enum's values, addressed by value or by name as TracerParameter<enum> does through its string table)
struct TracerParameter {
    enum kind_t { Bool, Int, Float, Enum } kind; int value, lo, hi;
    float fvalue = 0, flo = 0, fhi = 0;
    std::vector<std::string> names;   // Enum: name of value i
};
class TracerParameterCollection {
public:
    void addBool(const std::string& key, bool v) { p_[key] = { TracerParameter::Bool, v ? 1 : 0, 0, 1 }; }
    void addInterval(const std::string& key, int v, int lo, int hi) { p_[key] = { TracerParameter::Int, v, lo, hi }; }
    void addFloatInterval(const std::string& key, float v, float lo, float hi) { TracerParameter p{ TracerParameter::Float, 0, 0, 0 }; p.fvalue = v; p.flo = lo; p.fhi = hi; p_[key] = p; }
    void addEnum(const std::string& key, int v, const std::vector<std::string>& names) { TracerParameter p{ TracerParameter::Enum, v, 0, (int)names.size() - 1 }; p.names = names; p_[key] = p; }
    int getValue(const std::string& key) const { const TracerParameter& p = find(key); if (p.kind == TracerParameter::Float) throw std::runtime_error("Parameter type mismatch for key: " + key); return p.value; }
    float getFloat(const std::string& key) const { const TracerParameter& p = find(key); if (p.kind != TracerParameter::Float) throw std::runtime_error("Parameter type mismatch for key: " + key); return p.fvalue; }
    const std::string& getEnumName(const std::string& key) const { const TracerParameter& p = find(key); if (p.kind != TracerParameter::Enum) throw std::runtime_error("Parameter type mismatch for key: " + key); return p.names[p.value]; }
    void setValue(const std::string& key, int v, TracerParameter::kind_t kind) {
        TracerParameter& p = find(key);
        if (p.kind != kind) throw std::runtime_error("Parameter type mismatch for key: " + key);
        if (v < p.lo || v > p.hi) throw std::runtime_error("Parameter value outside of its interval: " + key);
        p.value = v;
    }
    void setFloat(const std::string& key, float v) {
        TracerParameter& p = find(key);
        if (p.kind != TracerParameter::Float) throw std::runtime_error("Parameter type mismatch for key: " + key);
        if (!(v >= p.flo && v <= p.fhi)) throw std::runtime_error("Parameter value outside of its interval: " + key);
        p.fvalue = v;
    }
    void setEnumByName(const std::string& key, const std::string& name) {
        TracerParameter& p = find(key);
        if (p.kind != TracerParameter::Enum) throw std::runtime_error("Parameter type mismatch for key: " + key);
        for (size_t i = 0; i < p.names.size(); i++) if (p.names[i] == name) { p.value = (int)i; return; }
        throw std::runtime_error("Parameter value outside of its set: " + key + " = " + name);
    }
    TracerParameter::kind_t kindOf(const std::string& key) const { return find(key).kind; }
    bool has(const std::string& key) const { return p_.count(key) != 0; }
private:
    std::map<std::string, TracerParameter> p_;
    const TracerParameter& find(const std::string& key) const { auto it = p_.find(key); if (it == p_.end()) throw std::runtime_error("Unknown parameter key: " + key); return it->second; }
    TracerParameter& find(const std::string& key) { auto it = p_.find(key); if (it == p_.end()) throw std::runtime_error("Unknown parameter key: " + key); return it->second; }
};

class event_timer {   // hipEvent pairs on the tracer's stream, summed per kernel class after synchronisation
public:
    ~event_timer();
    void begin(hipStream_t s, int cls);
    void end(hipStream_t s);
    void collect(double ms_out[5]);   // adds elapsed ms per class, recycles the events
private:
    struct rec { hipEvent_t a, b; int cls; };
    std::vector<rec> used_; std::vector<hipEvent_t> free_;
    hipEvent_t get();
};

class TracerBase {
public:
    TracerBase();
    virtual ~TracerBase();
    virtual void InitializeScene(Scene* s) { m_pScene = s; }
    virtual void Resize(unsigned int _w, unsigned int _h) { w = _w; h = _h; }
    virtual void DoPass(Image* I, bool a_NewTrace) = 0;
    virtual bool isMultiPass() const = 0;
    virtual float getSplatScale() const = 0;
    unsigned int getNumPassesDone() const { return m_uPassesDone; }
    uint64_t getRaysInLastPass() const { return m_uLastNumRaysTraced; }
    float getLastTimeSpentRenderingSec() const { return m_fLastRuntime; }
    uint64_t getAccRays() const { return m_uAccNumRaysTraced; }
    float getAccTimeSpentRenderingSec() const { return m_fAccRuntime; }
    TracerParameterCollection& getParameters() { return m_sParameters; }
    // build-specific additions
    virtual void DoPasses(Image* I, bool a_NewTrace, unsigned int n) { for (unsigned int i = 0; i < n; i++) DoPass(I, a_NewTrace && i == 0); }
    // TracerBase::Debug(Image*, pixel) (Kernel/Tracer.h:119-123): UpdateKernel draws the NEXT set of sampling tables from the tracer's generator (so the following
    // DoPass uses the set after it), then DebugInternal follows one path for that pixel.  rgb (may be null): the radiance of that path (the reference discards it)
    virtual void Debug(Image* I, unsigned int x, unsigned int y, float rgb[3]) = 0;
    // IDepthTracer::setDepthBuffer (Kernel/Tracer.h:34-57; the wavefront plugin and the PrimTracer, prim_tracer.h): a device buffer of w x h floats that receives the normalised depth of every primary hit
    virtual void setDepthBuffer(float* device_data, unsigned int dw, unsigned int dh);   // default: refuses (the tracer is not an IDepthTracer)
    virtual void reservePasses(unsigned int n) { (void)n; }   // size the queues now for a DoPasses(n) to come (otherwise they grow inside that call)
    void setTileShard(uint32_t rank, uint32_t world) { if (world == 0 || rank >= world) throw std::runtime_error("bad tile shard"); shard_rank = rank; shard_world = world; if (w != 0xffffffffu) Resize(w, h); }
    void setSamplerTables(const float* t1, const float* t2);
    // IBlockSampler of Tracer<true> (Kernel/Tracer.h:151-152,181-190): chosen by the parameter BlockSamplerType (0 Uniform, 1 Variance,
    // 2 Difference, 3 Select), re-created by Resize; user weights as IUserPreferenceSampler::setWeight
    BlockSampler* getBlockSampler();
    void setBlockWeight(uint32_t block_x, uint32_t block_y, float w) { getBlockSampler()->set_weight(block_x, block_y, w); }
    // The PixelVarianceBuffer of Tracer<true> (Kernel/Tracer.h:151,233-237).  The reference updates it after every pass; here that is an opt-in (off by default): the
    // adaptive block samplers keep it up to date on their own, the switch adds the update where they do not run — inside the batch where the tracer can
    // (updatesVarianceInBatch), else by rendering one pass per launch.
    // Refused on a Tracer<false> (one sample per pixel: no variance) and on a tile shard (the NonLocalMeans filter, its consumer, needs the whole frame)
    void setPixelVariance(bool on);
    bool pixelVarianceOn() const { return pixel_variance_on_; }
    const PixelVarianceBuffer* getPixelVarianceBuffer();   // nullptr before Resize
    void readPixelVariance(float* host_out);                // computeVariance() of every pixel, w x h floats
    hipStream_t getStream() const { return stream; }
    unsigned int getWidth() const { return w; }
    unsigned int getHeight() const { return h; }
    void getKernelStats(ctl_tracer_stats& s) const;
protected:
    PixelVarianceBuffer* ensureVarianceBuffer();
    std::unique_ptr<PixelVarianceBuffer> var_buffer_; bool pixel_variance_on_ = false;
    Scene* m_pScene = nullptr;
    TracerParameterCollection m_sParameters;
    unsigned int w = 0xffffffffu, h = 0xffffffffu;
    unsigned int m_uPassesDone = 0;
    uint64_t m_uLastNumRaysTraced = 0, m_uAccNumRaysTraced = 0;
    float m_fLastRuntime = 0, m_fAccRuntime = 0;
    hipEvent_t start = nullptr, stop = nullptr;
    hipStream_t stream = nullptr;
    sequence_generator m_SamplingSequenceGenerator;   // IndependantSamplingSequenceGenerator
    std::vector<float> user_t1, user_t2; bool have_user_tables = false;
    uint32_t shard_rank = 0, shard_world = 1;
    std::unique_ptr<BlockSampler> block_sampler_; const unsigned char* pass_block_counts_ = nullptr; uint32_t pass_max_block_count_ = 1; uint64_t pass_paths_ = 0;
    event_timer timer; double kernel_ms[5] = { 0, 0, 0, 0, 0 };   // 0 raygen, 1 closest-hit intersect, 2 shade/finalize, 3 any-hit intersect, 4 fused closest + any-hit launches
    uint64_t intersect_rays = 0, intersect_launches = 0, shadow_rays = 0, shadow_launches = 0, fused_launches = 0, fused_shadow_rays = 0, fused_closest_rays = 0;
    bool counting = false; ctl_traversal_counts closest_counts{}, any_counts{};
public:
    void setCounting(bool on) { counting = on; }
};

template <bool PROGRESSIVE> class Tracer : public TracerBase {
public:
    void DoPass(Image* I, bool a_NewTrace) override { DoPasses(I, a_NewTrace, 1); }
    void DoPasses(Image* I, bool a_NewTrace, unsigned int n) override;
    void Debug(Image* I, unsigned int x, unsigned int y, float rgb[3]) override;
    bool isMultiPass() const override { return PROGRESSIVE; }
    float getSplatScale() const override { return PROGRESSIVE ? 1.0f / float(m_uPassesDone) : 0.0f; }
protected:
    // render `n_batch` passes together; their sampler tables are consecutive at (d_t1, d_t2) (device); asynchronous on `stream`
    virtual void DoRender(Image* I, const float* d_t1, const float* d_t2, unsigned int n_batch) = 0;
    virtual void takeRayCounts(uint64_t& path_rays, uint64_t& shadow_rays_) = 0;
    virtual void DebugInternal(Image* I, unsigned int x, unsigned int y, const float* d_t1, const float* d_t2, float rgb[3]) { (void)I; (void)x; (void)y; (void)d_t1; (void)d_t2; rgb[0] = rgb[1] = rgb[2] = 0.0f; }   // TracerBase::DebugInternal: nothing unless the integrator overrides it
    dbuf<float> d_t1, d_t2;                       // ring of sampler-table sets in HBM
    float *h_t1 = nullptr, *h_t2 = nullptr; size_t h_cap = 0;   // their pinned host staging (tables handed in by setSamplerTables, host-generated tables)
    // tables generated in HBM (k_sequence_fill): the chunk jump matrices, and a ring of the batches' pass start states
    dbuf<uint32_t> d_jumps, d_starts; sequence_generator::pass_start* h_starts = nullptr; size_t starts_cap = 0;
    std::vector<hipEvent_t> slot_done;
    virtual unsigned int passBatch() const { return 1; }
    // can DoRender update the PixelVarianceBuffer itself, after each pass of a batch of b (batch_variance_)?  Otherwise the passes are rendered one per launch
    virtual bool updatesVarianceInBatch(unsigned int b) { (void)b; return false; }
    pixel_variance* batch_variance_ = nullptr; unsigned int batch_first_pass_ = 0;   // set for a DoRender that has to: the buffer, and the passes rendered before this batch
    static constexpr unsigned int kTableRing = 2;
    void ensureTableRing(unsigned int B);   // device + pinned host staging for `kTableRing` batches of B passes
public:
    ~Tracer() override { if (h_t1) (void)hipHostFree(h_t1); if (h_t2) (void)hipHostFree(h_t2); if (h_starts) (void)hipHostFree(h_starts); for (auto e : slot_done) (void)hipEventDestroy(e); }
private:
    void stageTables(unsigned int slot, unsigned int B, unsigned int nb);   // the tables of nb passes into ring slot `slot`: the caller's first, then the tracer's stream
};

// Integrators/PseudoRealtime/WavefrontPathTracer.h:24-67
class WavefrontPathTracer : public Tracer<true> {
public:
    WavefrontPathTracer();
    void Resize(unsigned int w, unsigned int h) override;
    void InitializeScene(Scene* s) override { check_media(s); check_texture_filtering(); Tracer<true>::InitializeScene(s); }
    // what the plugin refuses (unsupported_error), judged when a scene is handed over and when a pass starts.  ParticipatingMedia = false: a scene with participating media
    // (Scene::refuse_volumes — the plugin then runs no medium code and would render the scene without them); true: PathSemantics = Wavefront (pathIterateKernel has no medium rules)
    void check_media(const Scene* s) const;
    // TextureFiltering = true is refused (unsupported_error) at the same two places with PathSemantics = Wavefront (pathIterateKernel has no ray differentials) and with
    // ParticipatingMedia = true (the media build of the shade kernel has none either)
    void check_texture_filtering() const;
    void setDepthBuffer(float* device_data, unsigned int dw, unsigned int dh) override { depth_buffer_ = device_data; depth_w_ = dw; depth_h_ = dh; }   // WavefrontPathTracer : IDepthTracer (WavefrontPathTracer.h:24)
    void reservePasses(unsigned int n) override { const unsigned int b = std::min(passBatch(), std::max(1u, n)); growBatch(b, "reservePasses"); ensureTableRing(b); if (w != 0xffffffffu) (void)ensureStage(b); }
protected:
    void DoRender(Image* I, const float* d_t1, const float* d_t2, unsigned int n_batch) override;
    void takeRayCounts(uint64_t& path_rays, uint64_t& shadow_rays_) override;
    unsigned int passBatch() const override;
    bool updatesVarianceInBatch(unsigned int b) override;   // where the ordered accumulation's stage holds the batch: its resolve walks the passes in order
private:
    void growBatch(unsigned int b, const char* who);
    float4* ensureStage(unsigned int b);   // queues for b passes per wavefront; validated before anything changes
    wave_queues Q{};
    uint32_t capacity = 0, n_local_pixels = 0, alloc_batch_ = 1;
    float* depth_buffer_ = nullptr; unsigned int depth_w_ = 0, depth_h_ = 0;
    std::vector<std::unique_ptr<dbuf<float4>>> f4_; dbuf<float2> px_[2]; dbuf<float4> stage_, stray_stage_, mrec_[2]; dbuf<int> hit_node_; dbuf<uint32_t> occ_[2], counts_, work_, class_order_, class_counts_; dbuf<unsigned char> mat_key_; dbuf<unsigned long long> stats_;
    int grid_blocks = 0;
    float4* new_f4(size_t n);
};

// Integrators/PathTracer.h:7-31 — the megakernel integrator behind the same plugin API (megakernel.hip)
class PathTracer : public Tracer<true> {
public:
    PathTracer();
    void Resize(unsigned int w, unsigned int h) override;
    void InitializeScene(Scene* s) override;
protected:
    void DoRender(Image* I, const float* d_t1, const float* d_t2, unsigned int n_batch) override;
    void takeRayCounts(uint64_t& path_rays, uint64_t& shadow_rays_) override;
    void DebugInternal(Image* I, unsigned int x, unsigned int y, const float* d_t1, const float* d_t2, float rgb[3]) override;
private:
    dbuf<float> debug_;
    dbuf<unsigned long long> count_; unsigned long long host_count_ = 0; uint64_t total_rays_ = 0; dbuf<float> mollifier_;
    uint32_t n_local_pixels = 0; int grid_blocks = 0;
};

int device_count();
void require_device();
int persistent_grid_blocks();   // grid of the persistent kernels: 8 x 256-thread workgroups per CU of the current device = 32 waves per CU

// comm.cpp: the framebuffer reduce of a multi-GPU render over RCCL (ctl_comm_* in include/ctl_amd.h)
struct Comm;
void comm_unique_id(unsigned char out[128]);
Comm* comm_create(const unsigned char id[128], int rank, int world, int timeout_ms = 0);
void comm_destroy(Comm* c);
void comm_reduce_image(Comm* c, Image* src, Image* dst, int root);
void comm_gather_image(Comm* c, Image* src, Image* dst, int root);
size_t comm_gather_bytes(Comm* c, uint32_t W, uint32_t H);
size_t image_packed_tile_bytes(uint32_t W, uint32_t H, uint32_t world);
void image_pack_tiles(Image* img, uint32_t rank, uint32_t world, void* host_out);
void image_unpack_tiles(Image* img, uint32_t world, const void* host_in_all_ranks);

} // namespace ctl
