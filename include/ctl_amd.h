/*
 * ctl_amd.h — C-ABI drop-in boundary of the MI355X-native wavefront path tracer.
 *
 * The reference (hhergeth/CudaTracerLib) exposes its tracer plugins as C++ classes
 * (`Tracer<true>` subclasses, Kernel/Tracer.h:193-294) fed by a `KernelDynamicScene`
 * POD of device arrays (Engine/KernelDynamicScene.h:28-109).  This header is the
 * plain-C restatement of exactly that boundary for the wavefront path-tracing hot
 * path: the same arrays (bit-compatible element layouts, cited per struct), the same
 * tracer life-cycle (Resize / InitializeScene / DoPass / counters / parameters) and
 * the same `Image` accumulator (`PixelData`, Engine/Image.h:10-29).
 *
 * All pointers are plain host or device pointers, all sizes are element counts,
 * no C++ or torch types appear.  Every function returns 0 on success or a negative
 * ctl_status; ctl_last_error() gives the message the reference would have thrown
 * as std::runtime_error (Defines.cpp:15-29).
 *
 * The library is libctl_amd.so (cudatracerlib_amd/csrc).  It needs a gfx950 device
 * for every entry point that renders or intersects; those fail with CTL_ERR_NO_DEVICE
 * instead of falling back to any CPU path.
 */
#ifndef CTL_AMD_H
#define CTL_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
typedef enum {
    CTL_OK = 0,
    CTL_ERR_INVALID = -1,      /* bad argument / bad handle                       */
    CTL_ERR_NO_DEVICE = -2,    /* no HIP device (product path never falls back)   */
    CTL_ERR_HIP = -3,          /* hipError_t != hipSuccess, message in last_error */
    CTL_ERR_OVERFLOW = -4,     /* ray queue overflow (DoubleRayBuffer.h:86-89)    */
    CTL_ERR_UNSUPPORTED = -5,  /* e.g. participating media, unknown plugin name   */
    CTL_ERR_IO = -6,           /* scene loader: file / parse errors               */
    CTL_ERR_INTERNAL = -7      /* a state the library's own arithmetic rules out  */
} ctl_status;

const char* ctl_last_error(void);
const char* ctl_version(void);
/* number of visible HIP devices (0 on a CPU-only box; never an error) */
int ctl_device_count(void);

/* ------------------------------------------------ reference-layout elements */
/* Engine/TriIntersectorData.h:42-117 — Aila–Laine node, 4 x float4 = 64 B.
 * a = (c0.lo.x, c0.hi.x, c0.lo.y, c0.hi.y), b = (c1...), c = (c0.lo.z, c0.hi.z, c1.lo.z, c1.hi.z)
 * child >= 0: float4 index of an inner node (nodeIdx*4); child < 0: ~firstLeafEntry;
 * 0x76543210: no child (SplitBVHBuilder.cpp:163-203). */
typedef struct { float a[4], b[4], c[4]; int32_t child0, child1; uint32_t parent; uint32_t pad; } ctl_bvh_node;
/* Engine/TriIntersectorData.h:30-40 — Woop unit-triangle rows, 48 B. */
typedef struct { float a[4], b[4], c[4]; } ctl_woop_tri;
/* Engine/TriIntersectorData.h:8-28 — (triangleIndex << 1) | lastInLeaf. */
typedef struct { uint32_t index; } ctl_woop_index;
/* Engine/TriangleData.h:10-54 (EXT_TRI, NUM_UV_SETS 1) — 32 B shading triangle. */
typedef struct { uint32_t nor_mat_extra[2]; uint32_t dpdu_dpdv[3]; uint32_t uv[3]; } ctl_triangle_data;
/* Engine/Mesh.h:12-19 */
typedef struct { uint32_t tri_offset, bvh_node_offset, bvh_tri_offset, bvh_index_offset, std_material_offset; } ctl_kernel_mesh;
/* SceneTypes/Node.h:13-24 (FixedSizeArray<unsigned,2>: buffer then length) — 24 B */
typedef struct { uint32_t mesh_index, material_offset, instanciated_material; uint32_t lights[2]; uint32_t n_lights; } ctl_node;
/* Math/float4x4.h:12-18 — row-major, column-vector convention */
typedef struct { float m[16]; } ctl_float4x4;
/* Kernel/TraceHelper.h:55-59 — a = (origin, tmin), b = (direction, tmax) */
typedef struct { float a[4]; float b[4]; } ctl_ray;
/* Kernel/TraceHelper.h:61-69 — dist, node, triangle, barycentrics.
 * The reference packs the barycentrics into 2 x u16 (TraceHelper.cu:728-729); this build
 * keeps them as full floats (the precision of the reference's single-ray traceRay,
 * TraceHelper.cu:159) and so the record is 20 B wide on the C-ABI. */
typedef struct { float dist; int32_t node_idx; int32_t tri_idx; float u, v; } ctl_hit;
/* Engine/Image.h:10-29 — 28 B accumulator */
typedef struct { float rgb[3]; float rgb_splat[3]; float weight_sum; } ctl_pixel_data;
/* Engine/ShapeSet.h:19-30 — area-light triangle, 64 B, lives in the anim blob */
typedef struct { float p[3][3]; float n[3]; float area; uint32_t i_dat; uint32_t t_dat; uint32_t pad; } ctl_shape_tri;   /* CUDA_ALIGN(16): 64 B */

/* --------------------------------------------- compact scene-type descriptors */
/* The reference stores BSDFs / lights / sensors as tagged C++ unions (Material 3344 B,
 * Light 592 B, Sensor 320 B) whose byte layout depends on the host compiler.  The
 * boundary carries the same parameters as flat descriptors; INTEGRATION.md shows the
 * conversion a maintainer adds next to DynamicScene::getKernelSceneData(). */
/* ids = TYPE_FUNC ids of SceneTypes/Texture.h:107,127,159 */
enum { CTL_TEX_CONSTANT = 2, CTL_TEX_CHECKER = 3, CTL_TEX_IMAGE = 4 };
typedef struct {
    uint32_t type;       /* CTL_TEX_*                                          */
    float value[3];      /* constant colour / checker colour 0                  */
    float value1[3];     /* checker colour 1                                    */
    float uv_scale[2], uv_offset[2];
    uint32_t image;      /* index into the scene's image table (CTL_TEX_IMAGE)  */
} ctl_texture;           /* 48 B */

/* CTL_TEX_IMAGE (ImageTexture, SceneTypes/Texture.h:159-183, Texture.cu:6-13): value = m_scale, uv_scale/uv_offset = the
 * diagonal TextureMapping2D (m11, m22, m13, m23), image = index into ctl_scene_desc::images. */

/* Engine/MIPMap_device.h:11-32,57-69 — level 0 of a KernelMIPMap.  The path samples level 0 only: ImageTexture::Evaluate
 * without uv partials -> Sample(uv) = Texel(0,uv) / triangle(0,uv) (MIPMap.cu:116-121), InfiniteLight -> Sample(uv, 0) =
 * triangle(0,uv) and Sample(0,x,y) (MIPMap.cu:139-165). */
enum { CTL_WRAP_REPEAT = 0, CTL_WRAP_CLAMP = 1, CTL_WRAP_MIRROR = 2, CTL_WRAP_BLACK = 3 };
enum { CTL_FILTER_POINT = 0, CTL_FILTER_BILINEAR = 1, CTL_FILTER_ANISOTROPIC = 2, CTL_FILTER_TRILINEAR = 3 };
enum { CTL_TEXEL_RGBE = 0, CTL_TEXEL_RGBCOL = 1 };   /* Texture_DataType; both are uchar4 (Math/Spectrum.h:323-324,528-565) */
typedef struct {
    const uint32_t* texels;    /* width*height level-0 texels, row-major, byte 0 = r (x), 1 = g, 2 = b, 3 = e / alpha */
    uint32_t width, height;
    uint32_t texel_type, wrap_mode, filter_mode;
} ctl_mipmap;

/* Engine/RoughTransmittance.h:9-27 — one table of Mitsuba's data/microfacet/{beckmann,phong,ggx}.dat (roughplastic).
 * trans[2*eta_samples][alpha_samples][theta_samples], diff_trans[2*eta_samples][alpha_samples] (the second half of each is
 * the eta < 1 block).  ctl_scene_desc::rough_transmittance points at THREE of them, indexed by the microfacet distribution
 * type exactly as RoughTransmittanceManager does (RoughTransmittance.cu:124-157: slot 0 beckmann.dat, 1 phong.dat, 2 ggx.dat). */
typedef struct {
    const float* trans; const float* diff_trans;
    uint32_t eta_samples, alpha_samples, theta_samples;
    float eta_min, eta_max, alpha_min, alpha_max;
} ctl_rough_transmittance;

/* ids = the reference's TYPE_FUNC ids (BSDF_Simple.h:6-401, BSDF_Complex.h:9-182) */
enum { CTL_BSDF_DIFFUSE = 1, CTL_BSDF_ROUGHDIFFUSE = 2, CTL_BSDF_DIELECTRIC = 3, CTL_BSDF_THINDIELECTRIC = 4,
       CTL_BSDF_ROUGHDIELECTRIC = 5, CTL_BSDF_CONDUCTOR = 6, CTL_BSDF_ROUGHCONDUCTOR = 7, CTL_BSDF_PLASTIC = 8,
       CTL_BSDF_ROUGHPLASTIC = 9, CTL_BSDF_PHONG = 10, CTL_BSDF_WARD = 11, CTL_BSDF_HK = 12,
       CTL_BSDF_COATING = 13, CTL_BSDF_ROUGHCOATING = 14, CTL_BSDF_BLEND = 15 };
/* SceneTypes/Samples.h:31-95 lobe flags */
enum { CTL_ENull = 0x1, CTL_EDiffuseReflection = 0x2, CTL_EDiffuseTransmission = 0x4, CTL_EGlossyReflection = 0x8,
       CTL_EGlossyTransmission = 0x10, CTL_EDeltaReflection = 0x20, CTL_EDeltaTransmission = 0x40,
       CTL_EDelta1DReflection = 0x80, CTL_EDelta1DTransmission = 0x100 };
/* Engine/MicrofacetDistribution.h:14-21 */
enum { CTL_MF_BECKMANN = 0, CTL_MF_GGX = 1, CTL_MF_PHONG = 2 };

/* Parameter slots by bsdf_type:
 *  diffuse        tex0 reflectance
 *  roughdiffuse   tex0 reflectance, tex1 alpha, u0 useFastApprox
 *  dielectric     tex0 specularTransmittance, tex1 specularReflectance, f0 Cauchy B (= eta), f1 Cauchy C
 *  thindielectric tex0 specularTransmittance, tex1 specularReflectance, f0 eta
 *  roughdielectric tex0 specT, tex1 specR, tex2 alphaU, tex3 alphaV, f0 eta, f1 invEta, u0 distribution, u1 sampleVisible
 *  conductor      tex0 specularReflectance, f0..2 eta rgb, f3..5 k rgb
 *  roughconductor tex0 specR, tex1 alphaU, tex2 alphaV, f0..2 eta, f3..5 k, u0 distribution, u1 sampleVisible
 *  plastic        tex0 diffuseReflectance, tex1 specularReflectance, f0 fdrInt, f1 fdrExt, f2 eta, f3 invEta2,
 *                 f4 specularSamplingWeight, u0 nonlinear
 *  roughplastic   tex0 diffuse, tex1 specular, tex2 alpha, f0 eta, f1 invEta2, f2 specularSamplingWeight,
 *                 u0 nonlinear, u1 sampleVisible, u2 distribution
 *  phong          tex0 diffuse, tex1 specular, tex2 exponent, f0 specularSamplingWeight
 *  coating        tex0 sigmaA, tex1 specularReflectance, f0 eta, f1 invEta, f2 thickness, f3 specularSamplingWeight, u2 nested material
 *  roughcoating   tex0 sigmaA, tex1 specularReflectance, tex2 alpha, f0 eta, f1 invEta, f2 thickness, f3 specularSamplingWeight,
 *                 u0 distribution, u1 sampleVisible, u2 nested material
 *  blend          tex0 weight, u2 / u3 nested materials (absolute indices, ctl_builder_add_material); combined_type of the three =
 *                 own lobes | the nested BSDFs' combined_type
 *  ward           tex0 diffuse, tex1 specular, tex2 alphaU, tex3 alphaV, f0 specularSamplingWeight, u0 variant (0 Ward, 1 Ward-Duer, 2 balanced) */
typedef struct {
    uint32_t bsdf_type;        /* CTL_BSDF_*                                       */
    uint32_t combined_type;    /* BSDF::m_combinedType (SceneTypes/BSDF.h:24)      */
    uint32_t two_sided;        /* BSDF::m_enableTwoSided (SceneTypes/BSDF.h:26)    */
    uint32_t node_light_index; /* Material::NodeLightIndex, UINT32_MAX = none      */
    ctl_texture tex[4];
    float f[8];
    uint32_t u[4];
    /* Material::NormalMap / HeightMap (Engine/Material.h:58-59,93-106: at most one of them) and Material::AlphaMap
     * (Material.h:13-36,60,107-111).  The normal / height map perturbs the shading frame in TraceResult::getBsdfSample
     * (Material::SampleNormalMap, Material.cu:96-138; parallax occlusion is never enabled by the reference and is not carried).
     * The alpha test runs inside single-ray traversal (TraceHelper.cu:135-153) — i.e. for the megakernel PathTracer; the
     * reference's wavefront intersectKernel has no alpha test, see the AlphaTest tracer parameter. */
    uint32_t map_kind;         /* CTL_MAP_NONE / CTL_MAP_NORMAL / CTL_MAP_HEIGHT                 */
    uint32_t alpha_state;      /* AlphaBlendState, CTL_ALPHA_*                                   */
    float alpha_test_scalar;   /* AlphaBlendData::test_val_scalar                                */
    float alpha_test_color[3]; /* AlphaBlendData::test_val_color                                 */
    uint32_t reserved_[2];
    ctl_texture map_tex;       /* the normal or height map                                      */
    ctl_texture alpha_tex;     /* AlphaBlendData::tex                                            */
} ctl_material;                /* 384 B */
enum { CTL_MAP_NONE = 0, CTL_MAP_NORMAL = 1, CTL_MAP_HEIGHT = 2 };
/* Material.h:13-22: low two bits = test (1 luminance >= scalar, 2 alpha channel >= scalar, 3 |colour - test colour| <= scalar),
 * bit 2 = take the BSDF's first texture instead of alpha_tex */
enum { CTL_ALPHA_DISABLED = 0, CTL_ALPHA_MAP_LUMINANCE = 1, CTL_ALPHA_MAP_ALPHA = 2, CTL_ALPHA_MAP_COLOR = 3,
       CTL_ALPHA_REFLECTANCE_LUMINANCE = 5, CTL_ALPHA_REFLECTANCE_ALPHA = 6, CTL_ALPHA_REFLECTANCE_COLOR = 7 };

/* ids = TYPE_FUNC ids of SceneTypes/Light.h:36,98,147,228,296 */
enum { CTL_LIGHT_POINT = 1, CTL_LIGHT_DIFFUSE = 2, CTL_LIGHT_DISTANT = 3, CTL_LIGHT_SPOT = 4, CTL_LIGHT_INFINITE = 5 };
typedef struct {
    uint32_t type;                 /* CTL_LIGHT_*                                              */
    float radiance[3];             /* DiffuseLight::m_rad_texture (constant) / intensity       */
    /* DiffuseLight: ShapeSet (Engine/ShapeSet.h:61-66) — byte offsets into the anim blob */
    uint32_t area_dist_index;      /* float[count+1] normalised area CDF                       */
    uint32_t triangles_index;      /* ctl_shape_tri[count]                                     */
    float sum_area;
    uint32_t count;
    uint32_t orthogonal;           /* DiffuseLight::m_bOrthogonal                              */
    uint32_t node_idx;             /* DiffuseLight::m_uNodeIdx                                 */
    /* Point / Spot / Distant */
    float position[3];
    float direction[3];
    float cutoff_angle, beam_width, cos_cutoff_angle, cos_beam_width, inv_transition_width;
    float to_world[16];            /* Spot / Distant: Frame ToWorld as rows s = [0..2], t = [4..6], n = [8..10];
                                      Infinite: m_worldTransform, row-major 4x4                */
    /* InfiniteLight (SceneTypes/Light.h:293-311, Light.cpp:10-61); the three tables are byte offsets into the anim blob */
    uint32_t env_image;            /* radianceMap: index into ctl_scene_desc::images           */
    float env_scale[3];            /* m_scale                                                  */
    float bsphere_center[3], bsphere_radius;   /* m_SceneCenter, m_SceneRadius; DistantLight::radius */
    uint32_t cdf_rows_index;       /* float[height + 1]                                        */
    uint32_t cdf_cols_index;       /* float[height * (width + 1)]                              */
    uint32_t row_weights_index;    /* float[height]                                            */
    float normalization;           /* m_normalization                                          */
    /* DiffuseLight::m_rad_texture when it is not a ConstantTexture (SceneTypes/Light.cu:50-53 needsUVSample): CTL_TEX_CHECKER / CTL_TEX_IMAGE;
     * any other type (0, CTL_TEX_CONSTANT) = the constant `radiance` above */
    ctl_texture rad_texture;
} ctl_light;

/* ids = TYPE_FUNC ids of SceneTypes/Sensor.h:107,191,272,364,445 */
enum { CTL_SENSOR_SPHERICAL = 1, CTL_SENSOR_PERSPECTIVE = 2, CTL_SENSOR_THINLENS = 3, CTL_SENSOR_ORTHOGRAPHIC = 4, CTL_SENSOR_TELECENTRIC = 5 };
typedef struct {
    uint32_t type;
    float to_world[16];            /* SensorBase::toWorld (row-major)                          */
    float fov;                     /* radians, horizontal (SceneTypes/Sensor.h:72-76)          */
    float near_depth, far_depth;   /* SensorBase::m_fNearFarDepths                             */
    float resolution[2];           /* film size in pixels                                      */
    float aperture_radius, focus_distance;   /* ThinLens / Telecentric: SensorBase::m_apertureRadius, m_focusDistance */
    float screen_scale[2];         /* Telecentric: screenScale (its aperture is aperture_radius / screen_scale[0]); 0 = 1 */
} ctl_sensor;

#define CTL_MAX_NUM_LIGHTS 16      /* Engine/KernelDynamicScene.h:26 */

/* Participating media (SceneTypes/Volumes.{h,cu}, SceneTypes/PhaseFunction.{h,cu}).  ids = the reference's TYPE_FUNC ids. */
enum { CTL_PHASE_HG = 1, CTL_PHASE_ISOTROPIC = 2, CTL_PHASE_KAJIYA_KAY = 3, CTL_PHASE_RAYLEIGH = 4 };
typedef struct {
    uint32_t type;             /* CTL_PHASE_*                                                                    */
    float g;                   /* HGPhaseFunction::m_g, |g| < 1                                                  */
    float ks, kd, exponent;    /* KajiyaKayPhaseFunction::m_ks, m_kd, m_exponent                                 */
    float normalization;       /* DERIVED: KajiyaKayPhaseFunction::m_normalization (ctl_volume_update)           */
} ctl_phase_function;          /* 24 B */
enum { CTL_VOLUME_HOMOGENEOUS = 1,     /* HomogeneousVolumeDensity */
       CTL_VOLUME_GRID = 2 };          /* VolumeGrid: a ctl_volume of this type plus exactly one ctl_volume_grid record (below); its sig_a / sig_s / le are 0 */
#define CTL_MAX_VOL_COUNT 16       /* KernelAggregateVolume::MAX_VOL_COUNT */
/* A region is the unit cube [0,1]^3 under volume_to_world (BaseVolumeRegion); its coefficients hold inside and are 0 outside. */
typedef struct {
    uint32_t type;                     /* CTL_VOLUME_*                                                           */
    ctl_phase_function phase;          /* BaseVolumeRegion::Func                                                 */
    ctl_float4x4 volume_to_world;      /* BaseVolumeRegion::VolumeToWorld                                        */
    ctl_float4x4 world_to_volume;      /* DERIVED: VolumeToWorld.inverse() (BaseVolumeRegion::Update; ctl_volume_update) */
    float sig_a[3], sig_s[3], le[3];   /* absorption, scattering, emission (the path tracer never reads le)      */
} ctl_volume;                          /* 192 B */
/* VolumeGrid (SceneTypes/Volumes.h:184-287): the density grids of one CTL_VOLUME_GRID region, a record in a side array of the description.  single_grid != 0: one grid
 * (`dim`, `data`) serves absorption and scattering (VolumeGrid(func, ToWorld, buffer, dim)); otherwise gridA (`dim_a`, `data_a`) and gridS (`dim_s`, `data_s`) (the
 * three-grid form; gridL is not carried: PathTrace never reads Lve, and m_stepSize is not carried: nothing reads it).  The floats lie in the reference's linear order,
 * DenseVolGrid::idx (Volumes.h:139-142), dim[0] * dim[1] * dim[2] of them per grid, in HOST memory.  A coefficient at a point is min + (max - min) * density. */
#define CTL_MAX_GRID_CELLS (1u << 22)  /* cells per grid: 16 MiB of floats, so that the 16 regions of a table, two grids each, stay within 512 MiB of device memory */
typedef struct {
    uint32_t volume;                   /* index of its ctl_volume, whose type is CTL_VOLUME_GRID                 */
    uint32_t single_grid;              /* VolumeGrid::singleGrid                                                 */
    uint32_t dim[3];                   /* grid.dim (single form)                                                 */
    uint32_t dim_a[3], dim_s[3];       /* gridA.dim, gridS.dim (three-grid form)                                 */
    float sig_a_min[3], sig_a_max[3], sig_s_min[3], sig_s_max[3], le_min[3], le_max[3];   /* sigAMin ... leMax (le*: carried, never read) */
    const float* data;                 /* grid   (single form; otherwise NULL)                                   */
    const float* data_a;               /* gridA  (three-grid form; otherwise NULL)                               */
    const float* data_s;               /* gridS  (three-grid form; otherwise NULL)                               */
} ctl_volume_grid;                     /* 144 B */

/* Engine/KernelDynamicScene.h:28-109 restated with plain pointers (HOST memory). */
typedef struct {
    const ctl_triangle_data* tri_data;   uint32_t n_tri_data;     /* m_sTriData       */
    const ctl_woop_tri* woop;            uint32_t n_woop;         /* m_sBVHIntData    */
    const ctl_woop_index* woop_index;                             /* m_sBVHIndexData (n_woop) */
    const ctl_bvh_node* bvh_nodes;       uint32_t n_bvh_nodes;    /* m_sBVHNodeData   */
    const ctl_kernel_mesh* meshes;       uint32_t n_meshes;       /* m_sMeshData      */
    const ctl_node* nodes;               uint32_t n_nodes;        /* m_sNodeData      */
    const ctl_material* materials;       uint32_t n_materials;    /* m_sMatData       */
    const ctl_light* lights;             uint32_t n_lights_buf;   /* m_sLightBuf      */
    const uint8_t* anim;                 uint32_t n_anim_bytes;   /* m_sAnimData      */
    /* KernelSceneBVH (Engine/SceneBVH_device.h:8-15) */
    int32_t scene_start_node;
    const ctl_bvh_node* scene_bvh_nodes; uint32_t n_scene_bvh_nodes;
    const ctl_float4x4* node_transforms;      /* n_nodes */
    const ctl_float4x4* node_inv_transforms;  /* n_nodes */
    uint32_t env_map_index;                   /* UINT32_MAX = none */
    float box_min[3], box_max[3];             /* m_sBox */
    ctl_sensor camera;                        /* m_Camera */
    uint32_t num_lights;                      /* m_numLights */
    uint32_t light_indices[CTL_MAX_NUM_LIGHTS];
    float light_cdf[CTL_MAX_NUM_LIGHTS];
    float ray_trace_eps;                      /* m_rayTraceEps = 1e-4 * |box diagonal| (DynamicScene.cpp:587) */
    const ctl_mipmap* images;            uint32_t n_images;       /* m_sTexData (level 0) */
    const ctl_rough_transmittance* rough_transmittance;           /* [3] or NULL (needed by roughplastic only) */
    const ctl_volume* volumes;           uint32_t n_volumes;      /* m_sVolume (KernelAggregateVolume): at most CTL_MAX_VOL_COUNT regions; NULL / 0 = no participating media */
    const ctl_volume_grid* volume_grids; uint32_t n_volume_grids; /* one record per CTL_VOLUME_GRID region of `volumes`; NULL / 0 = none (a zeroed description has none) */
} ctl_scene_desc;

/* BSDF::Update() (SceneTypes/BSDF_Simple.h:255-264 plastic, :298-304 roughplastic, :332-337 phong, :371-376 ward; BSDF_Complex.h:37-44 coating, :117-125
 * roughcoating): recomputes a material's DERIVED fields from its primary ones — fdrInt / fdrExt by the reference's adaptive Gauss-Lobatto quadrature
 * (FresnelHelper::fresnelDiffuseReflectance, Math/FresnelHelper.cu:57-60), invEta / invEta2, the specular sampling weights from the textures' average
 * luminance (constant and checkerboard textures; an image texture's average is the caller's, as ImageTexture::Average reads the coarsest MIP level).
 * Host only.  A caller converting the reference's own objects copies their fields instead and does not need this. */
int ctl_material_update(ctl_material* m);
/* BaseVolumeRegion::Update + KajiyaKayPhaseFunction::Update (SceneTypes/Volumes.h:31-34, PhaseFunction.cu:64-77): recomputes a volume's DERIVED fields from its primary
 * ones — world_to_volume = float4x4::inverse of volume_to_world, and for a Kajiya-Kay phase function the normalisation by the reference's 1000-step Simpson sum (with the
 * shared fp32 functions of csrc/ctl_fmath.h).  Host only.  An unknown phase or volume type: CTL_ERR_INVALID. */
int ctl_volume_update(ctl_volume* v);
/* FresnelHelper::fresnelDiffuseReflectance(eta, false) as above. */
float ctl_fresnel_diffuse_reflectance(float eta);

/* ------------------------------------------------------------- scene builder */
/* Host-side mirror of the subset of DynamicScene the loader drives
 * (Engine/DynamicScene.h:70-187; SURVEY §8b "Loader boundary"). */
typedef struct ctl_builder ctl_builder;
int ctl_builder_create(ctl_builder** out);
void ctl_builder_destroy(ctl_builder* b);
/* Mesh::CompileMesh (Engine/Mesh.cpp:199-290): positions[3*n_vert], indices[3*n_tri] (NULL = soup),
 * normals[3*n_vert] or NULL (computed as Mesh.cpp:151-190), uvs[2*n_vert] or NULL, tri_material[n_tri] local
 * material index or NULL (all 0), materials[n_mat]. Builds the mesh BVH (SAH, max leaf 8 as
 * BVHBuilderHelper.cpp:119).  Returns the mesh index. */
int ctl_builder_add_mesh(ctl_builder* b, const float* positions, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                         const float* normals, const float* uvs, const uint8_t* tri_material,
                         const ctl_material* materials, uint32_t n_mat, uint32_t* mesh_index_out);
/* Which builder ctl_builder_add_mesh uses from now on.  CTL_BVH_SBVH: the reference's SplitBVHBuilder restated
 * (Engine/SpatialStructures/BVH/SplitBVHBuilder.cpp:219-640 through ConstructBVH) — the same node / Woop / index arrays element for
 * element.  CTL_BVH_BINNED: binned SAH, object splits only, threaded.  CTL_BVH_AUTO (default; or $CTL_BVH_MODE = sbvh | binned):
 * SBVH for meshes of up to 65536 triangles, binned above. */
enum { CTL_BVH_AUTO = 0, CTL_BVH_SBVH = 1, CTL_BVH_BINNED = 2 };
int ctl_builder_set_bvh_mode(ctl_builder* b, uint32_t mode);
/* DynamicScene::CreateNode + SetNodeTransform (DynamicScene.cpp:269-346): one instance of a mesh. */
int ctl_builder_add_node(ctl_builder* b, uint32_t mesh_index, const ctl_float4x4* to_world, uint32_t* node_index_out);
/* DynamicScene::DeleteNode (Engine/DynamicScene.cpp:380-384): the nodes behind node_index move down by one and the node_idx of their area lights follows; the node's
 * material copies stay in the material table, unreferenced.  The next ctl_builder_finalize gives the new description (what ctl_scene_update_nodes takes).
 * CTL_ERR_UNSUPPORTED for a node that carries area lights (their records and shape sets would have to leave the light tables), CTL_ERR_INVALID for an index that is no
 * node's and for the last node of the builder; a refusal leaves the builder untouched. */
int ctl_builder_remove_node(ctl_builder* b, uint32_t node_index);
/* The counterpart of ctl_builder_add_mesh for a mesh that no node instances any more (the reference frees such a mesh's ranges in DynamicScene::UpdateScene,
 * Engine/DynamicScene.cpp:483-507; the arrays here are dense, so they are compacted): the mesh's ranges leave tri_data, woop, woop_index and bvh_nodes and its record
 * leaves meshes; every later mesh moves down by one index and by the erased sizes in its offsets, the mesh_index of its nodes and the i_dat / t_dat of their area
 * lights follow.  After ctl_builder_finalize those arrays equal, byte for byte, the ones of a builder that never added the mesh — except std_material_offset: the
 * MATERIALS ARE NOT COMPACTED, the removed mesh's standard materials stay in the builder as unreferenced rows (384 B each), so std_material_offset and material_offset of
 * everything kept are unchanged.  The compiled-mesh cache is not involved.  CTL_ERR_INVALID, the builder unchanged, for an index that is no mesh's and for a mesh a node
 * still instances (the message names the first such node).  ctl_builder_remove_node refuses a node that carries area lights, so a mesh with an emissive node cannot be
 * removed yet.  The next ctl_builder_finalize gives the description ctl_scene_update_mesh_set takes. */
int ctl_builder_remove_mesh(ctl_builder* b, uint32_t mesh_index);
/* the number of meshes the builder holds now, whoever added them (a loader included), without a ctl_builder_finalize */
int ctl_builder_mesh_count(const ctl_builder* b, uint32_t* count_out);
/* DynamicScene::CreateLight(node, matName, L) (DynamicScene.cpp:689-711): all triangles of the node whose local
 * material index is `local_material` become one DiffuseLight. */
int ctl_builder_add_area_light(ctl_builder* b, uint32_t node_index, uint32_t local_material, const float radiance[3]);
/* The same with the two DiffuseLight members an application sets on the light afterwards (SceneTypes/Light.h:100-101): a radiance texture that is
 * not constant (NULL = constant `radiance`) and m_bOrthogonal (the light emits along its surface normal only). */
int ctl_builder_add_area_light_ex(ctl_builder* b, uint32_t node_index, uint32_t local_material, const float radiance[3], const ctl_texture* rad_texture, int32_t orthogonal);
/* DynamicScene::CreateLight(Light) for point lights (SceneTypes/Light.h:31-94) */
int ctl_builder_add_point_light(ctl_builder* b, const float position[3], const float intensity[3]);
/* SpotLight(p, t, L, width, fall) (SceneTypes/Light.cu:268-277): cutoff/beam angles in degrees as the loader passes them
 * (cutoffAngle, beamWidth). */
int ctl_builder_add_spot_light(ctl_builder* b, const float position[3], const float target[3], const float intensity[3],
                               float cutoff_angle_degrees, float beam_width_degrees);
/* DistantLight(L, d, r) (SceneTypes/Light.h:155-163): d = ToWorld.n (sampleDirect returns dRec.d = -d); r = radius of the
 * scene's bounding sphere as the caller sees it (the light stores 1.1 r; the Mitsuba loader passes r = 1, ObjectParser.h:530). */
int ctl_builder_add_distant_light(ctl_builder* b, const float direction[3], const float irradiance[3], float scene_radius);
/* MIPMap level 0 handed over decoded (the reference decodes files with FreeImage, Engine/MIPMap.cpp): returns the image index */
int ctl_builder_add_image(ctl_builder* b, const uint32_t* texels, uint32_t width, uint32_t height, uint32_t texel_type,
                          uint32_t wrap_mode, uint32_t filter_mode, uint32_t* image_index_out);
/* DynamicScene::setEnvironementMap(scale, file) (Engine/DynamicScene.cpp:846-859) + InfiniteLight ctor (Light.cpp:10-61):
 * builds the row / column CDFs; to_world (row-major 4x4, orthogonal) may be NULL = identity. */
int ctl_builder_set_environment_map(ctl_builder* b, uint32_t image_index, const float scale[3], const ctl_float4x4* to_world);
/* Registers a BSDF that no triangle refers to directly: the nested BSDF (BSDFFirst, SceneTypes/BSDF.h:102) of a coating,
 * roughcoating or blend.  Returns its absolute index in ctl_scene_desc::materials, to be stored in the parent's u[2] (/u[3]). */
int ctl_builder_add_material(ctl_builder* b, const ctl_material* material, uint32_t* index_out);
/* RoughTransmittanceManager::StaticInitialize (Engine/RoughTransmittance.cu:124-131): install the table of one slot (0..2);
 * the arrays are copied.  ctl_builder_load_rough_transmittance parses a Mitsuba "MTS_TRANSMITTANCE" .dat file (:8-45). */
int ctl_builder_set_rough_transmittance(ctl_builder* b, uint32_t slot, const ctl_rough_transmittance* table);
int ctl_builder_load_rough_transmittance(ctl_builder* b, uint32_t slot, const char* dat_path);
/* DynamicScene::setCamera — perspective sensor as built by the Mitsuba loader (ObjectParser.h:292-297): */
int ctl_builder_set_camera_lookat(ctl_builder* b, const float pos[3], const float target[3], const float up[3],
                                  float fov_degrees, uint32_t width, uint32_t height);
int ctl_builder_set_camera(ctl_builder* b, const ctl_sensor* sensor);
/* DynamicScene::CreateVolume(VolumeRegion) (Engine/DynamicScene.cpp:787-792): adds a participating medium, at most CTL_MAX_VOL_COUNT; ctl_builder_set_volume replaces one
 * (the host edits the region CreateVolume returned).  The derived fields are recomputed as ctl_volume_update does; the next ctl_builder_finalize hands the array out and
 * ctl_scene_update applies it in place (CTL_DIFF_VOLUMES).  Only the PathTracer plugin renders media; the other plugins refuse a scene that has any. */
int ctl_builder_create_volume(ctl_builder* b, const ctl_volume* volume, uint32_t* index_out);
int ctl_builder_set_volume(ctl_builder* b, uint32_t index, const ctl_volume* volume);
/* DynamicScene::CreateVolume(w, h, d, toWorld, phase) and (wA, hA, dA, wS, hS, dS, wL, hL, dL, toWorld, phase) (Engine/DynamicScene.cpp:794-812): a VolumeGrid region with
 * n_dims = 3 (one grid) or 9 dims (gridA, gridS, gridL; the L dims are accepted and ignored).  As the reference's constructors leave it: the grids' floats and
 * sigAMin ... leMax are 0.  ctl_builder_set_volume_grid_data COPIES n = dim[0] * dim[1] * dim[2] floats, in DenseVolGrid::idx's linear order, into grid `which`
 * (0: grid / gridA, 1: gridS); ctl_builder_set_volume_grid_coefficients sets sigAMin, sigAMax, sigSMin, sigSMax (3 floats each).  ctl_builder_set_volume edits the
 * region (type, matrix, phase function) as before; made homogeneous there, the region loses its grids at the next finalize. */
int ctl_builder_create_volume_grid(ctl_builder* b, const uint32_t* dims, uint32_t n_dims, const ctl_float4x4* volume_to_world, const ctl_phase_function* phase, uint32_t* index_out);
int ctl_builder_set_volume_grid_data(ctl_builder* b, uint32_t index, uint32_t which, const float* data, uint32_t n);
int ctl_builder_set_volume_grid_coefficients(ctl_builder* b, uint32_t index, const float* sig_a_min, const float* sig_a_max, const float* sig_s_min, const float* sig_s_max);
/* DynamicScene::UpdateScene + getKernelSceneData (DynamicScene.cpp:480-589): builds the scene BVH and fills
 * `out` with pointers that stay valid until the builder is destroyed or finalized again. */
int ctl_builder_finalize(ctl_builder* b, ctl_scene_desc* out);
/* DynamicScene::SetNodeTransform (Engine/DynamicScene.cpp:338-346): a new to_world (affine, invertible) for a node.  The area lights of the node get their shape
 * sets recalculated (ShapeSet::triData::Recalculate, Engine/ShapeSet.cu:11-23); the next ctl_builder_finalize rebuilds the scene BVH, the scene box, ray_trace_eps
 * and the box-dependent lights from the new transforms. */
int ctl_builder_set_node_transform(ctl_builder* b, uint32_t node_index, const ctl_float4x4* to_world);
/* DynamicScene::AnimateMesh (Engine/DynamicScene.cpp:450-456; AnimatedMesh::k_ComputeState, Engine/AnimatedMesh.cpp:163-184) for a host that computes the vertex positions
 * itself (skinning, simulation): new vertex arrays for mesh `mesh_index`, with the argument conventions and compile options of ctl_builder_add_mesh (indices == NULL: a
 * triangle soup, normals == NULL: computed, uvs == NULL).  n_tri must be the mesh's triangle count; the materials and the per-triangle material indices stay those of the
 * mesh as added.  Rewritten for that mesh only: its TriangleData (the bytes a fresh ctl_builder_add_mesh of the new arrays compiles), every Woop row, the boxes of its BVH
 * nodes bottom-up — links, leaf references and their order stay; a spatial-split reference's clipped box gives way to the whole triangle's, so the tree culls less well
 * but never wrongly —, the mesh's box, and the shape sets of the area lights on the nodes that instance it.  The next ctl_builder_finalize rebuilds the scene BVH, the scene
 * box, ray_trace_eps and the box-dependent lights.  ctl_scene_update applies the result in place (CTL_DIFF_GEOMETRY).  The geometry cache is neither read nor written.
 * CTL_ERR_INVALID (a bad mesh index, another triangle count, an index out of range) leaves the builder untouched. */
int ctl_builder_update_mesh(ctl_builder* b, uint32_t mesh_index, const float* positions, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                            const float* normals, const float* uvs);
/* DynamicScene::ReloadTextures (Engine/DynamicScene.cpp:457-) for a host that supplies the bitmap: new level-0 texels for the registered image `image_index`.  width and
 * height must be the image's; texel type, wrap and filter mode stay.  If the image is the environment map's, the light's column and row CDFs are rewritten where they stand
 * in the anim blob and its `normalization` in its record (rowWeights depends on the height only and stays).  The sampling weights of the materials that read the image's
 * average (plastic, roughplastic, phong, ward, coating, roughcoating) are made by the next ctl_builder_finalize, as always.  This is the host yardstick of
 * ctl_scene_update_image (below), and what a host that keeps its builder calls beside it, so that the next ctl_scene_update finds no difference.
 * CTL_ERR_INVALID (a null builder or texels, a bad index, another width or height: ctl_builder_replace_image) leaves the builder untouched. */
int ctl_builder_update_image(ctl_builder* b, uint32_t image_index, const uint32_t* texels, uint32_t width, uint32_t height);
/* The counterpart of ctl_builder_add_image for an image nothing reads any more: the image and its texels leave the builder, every later image moves down by one, and every
 * ctl_texture::image above it is lowered by one — the materials' tex[0..3], map_tex and alpha_tex (textures of type CTL_TEX_IMAGE), the lights' rad_texture and the
 * environment light's env_image.  After ctl_builder_finalize the images, materials, lights and anim blob equal, byte for byte, those of a builder that never added the image.
 * CTL_ERR_INVALID, the builder untouched, for an index that is no image's and for an image that any row of the material table or any light still references;
 * ctl_last_error() names the first referrer.  The material table is never compacted, so rows orphaned by ctl_builder_remove_node / ctl_builder_remove_mesh count: the host
 * repoints them first (ctl_builder_set_material).  A mesh's standard materials, which only a later ctl_builder_add_node copies, follow the shift; a texture there that named
 * the removed image names none afterwards (0xffffffff: black).  The next ctl_builder_finalize gives the description ctl_scene_update_image_set takes. */
int ctl_builder_remove_image(ctl_builder* b, uint32_t image_index);
/* New level-0 texels of ANOTHER size for image `image_index`; texel type, wrap and filter mode stay (for ctl_scene_update_image_set the image is a fresh one).  Called with the
 * image's current size it is ctl_builder_update_image.  CTL_ERR_INVALID, the builder untouched, for a bad index, null texels, an empty size, and for the environment map's
 * image: its tables were laid out in the anim blob by ctl_builder_set_environment_map, for its size. */
int ctl_builder_replace_image(ctl_builder* b, uint32_t image_index, const uint32_t* texels, uint32_t width, uint32_t height);
/* the number of images the builder holds now, whoever added them (a loader included), without a ctl_builder_finalize */
int ctl_builder_image_count(const ctl_builder* b, uint32_t* count_out);
/* DynamicScene::getMaterials + Invalidate (Engine/DynamicScene.h) for one row of the material table: absolute_index as the kernels address it (ctl_node::material_offset +
 * the triangle's local index, or what ctl_builder_add_material returned).  ctl_builder_set_material stores the record as given — node_light_index included: a host edits what
 * ctl_builder_get_material handed it — after the checks a new record gets: a known BSDF model, map kind and alpha state, known texture types, image indices the builder
 * holds, and BSDFFirst in both directions (a nested index in u[2] / u[3] names another row that is a simple BSDF; a row some coating or blend nests stays simple).  The next
 * ctl_builder_finalize makes the derived sampling weights, as always; ctl_scene_update applies the result (CTL_DIFF_MATERIALS).  CTL_ERR_INVALID leaves the builder untouched. */
int ctl_builder_get_material(const ctl_builder* b, uint32_t absolute_index, ctl_material* out);
int ctl_builder_set_material(ctl_builder* b, uint32_t absolute_index, const ctl_material* material);
/* The pyramid a scene keeps of an image (MIPMap::CompileToBinary, Engine/MIPMap.cpp:41-95), host only: level 0 followed by levels 1 .. into texels_out[capacity]
 * (may be NULL: the level table alone), *levels_out = 1 + floor(log2(min(width, height))), level_offsets_out[l - 1] = the texel offset of level l >= 1; level l is
 * (width >> l) x (height >> l).  CTL_ERR_INVALID: a null or empty image, an unknown texel type, a capacity below the pyramid's texel count. */
int ctl_mip_pyramid_host(const ctl_mipmap* image, uint32_t* texels_out, size_t capacity, uint32_t* levels_out, uint32_t level_offsets_out[15]);

/* ------------------------------------------------------------------- scenes */
typedef struct ctl_scene ctl_scene;
/* UpdateKernel(scene) (Kernel/TraceHelper.cu:182-217): uploads + re-lays-out the arrays in HBM. */
int ctl_scene_create(const ctl_scene_desc* desc, ctl_scene** out);
/* flags: CTL_SCENE_FLATTEN = additionally build ONE world-space BVH over all instanced triangles (128 B of HBM per instanced
 * triangle) and traverse that.  The flattened tree only culls: every leaf entry is evaluated with the reference's instance
 * transform + object-space Woop arithmetic (Kernel/TraceHelper.cu:526-560,646-682), so t,u,v,triangle,node equal the two-level
 * traversal bit for bit.  A triangle much longer than its neighbours is entered under several leaf entries (early split
 * clipping, DESIGN.md §3: the same 128 B under the boxes of its parts; a hit is the whole triangle's), so the tree may hold more entries
 * than the scene has instanced triangles.  CTL_SCENE_FLAT_FORMAT(f) picks the node format (measurement; default Q4). */
enum { CTL_SCENE_FLATTEN = 1,
       /* opt-in: a rough plastic with a constant roughness looks RoughTransmittanceManager's table up through a per-material 1-D reduction (4 taps instead of 64; synthetic-bathroom
        * + 3 % rays/s).  Equal to the reference's 3-D lookup (Engine/RoughTransmittance.cu:55-88) up to fp32 rounding only: frames stay within the per-pixel tolerance in most
        * scenes but are no longer equal to the bit, and textured scenes can exceed it at texture boundaries.  Without the flag every lookup is the reference's own arithmetic. */
       CTL_SCENE_REDUCED_ROUGH_TRANSMITTANCE = 2 };
enum { CTL_FLAT_Q4 = 0,    /* 4-wide, 64-B nodes, 8-bit child boxes (default) */
                           /* 1 and 2 are retired (the fp32 formats F4 / F2, EXPERIMENTS.md): CTL_ERR_UNSUPPORTED */
       CTL_FLAT_Q8 = 3 };  /* 8-wide, 128-B nodes, 8-bit child boxes, octant-ordered slots, one-triangle leaf slots (csrc/flat8.h) */
#define CTL_SCENE_FLAT_FORMAT(f) ((((uint32_t)(f)) + 1u) << 8)
int ctl_scene_create_ex(const ctl_scene_desc* desc, uint32_t flags, ctl_scene** out);
void ctl_scene_destroy(ctl_scene* s);
/* ---- in-place updates: what UpdateKernel(m_pScene) does for a host that moves the camera, edits a material or calls SetNodeTransform between passes
 * (Kernel/Tracer.h:121,229; INTEGRATION.md "Updating a scene").
 * ctl_scene_desc_diff classifies what differs between two descriptions of the same scene (host only): */
enum { CTL_DIFF_CAMERA = 1,       /* ctl_scene_desc::camera                                                                                        */
       CTL_DIFF_MATERIALS = 2,    /* the contents of `materials`                                                                                   */
       CTL_DIFF_LIGHTS = 4,       /* lights, anim blob, num_lights, light_indices, light_cdf, env_map_index, the nodes' light slots                 */
       CTL_DIFF_TRANSFORMS = 8,   /* node_transforms, node_inv_transforms, the scene BVH and its start node, box_min / box_max, ray_trace_eps       */
       CTL_DIFF_TOPOLOGY = 16,    /* anything else: any count but the lights', woop_index, the mesh BVHs' links, meshes, node -> mesh / material assignment,
                                     images, rough-transmittance tables                                                                           */
       CTL_DIFF_GEOMETRY = 32,    /* only VALUES of the geometry arrays: the contents of tri_data and woop and the float boxes of bvh_nodes — a deformed mesh
                                     (ctl_builder_update_mesh) — with everything CTL_DIFF_TOPOLOGY names equal                                    */
       CTL_DIFF_VOLUMES = 64 };   /* `volumes` / `n_volumes` and the grid records with their floats: the participating media, and nothing else                                            */
int ctl_scene_desc_diff(const ctl_scene_desc* a, const ctl_scene_desc* b, uint32_t* mask_out);
/* Everything ctl_scene_create and ctl_scene_update refuse a description for that can be judged from the description alone (host only, no device call): node transforms,
 * sensor, lights, textures, materials, the depth of the two-level BVH.  parts == 0: as ctl_scene_create checks; else the CTL_DIFF_* parts to check, as ctl_scene_update
 * checks the parts it found changed (CTL_DIFF_TOPOLOGY among them: as creation checks them).  CTL_ERR_INVALID and ctl_last_error() name the first rule broken.
 * CTL_DIFF_GEOMETRY is not a part this call takes (CTL_ERR_INVALID, as for any unknown bit): what an update checks of a deformed mesh — its BVH next to the scene BVH on the
 * traversal stack — is what parts = CTL_DIFF_TRANSFORMS checks, and the range and leaf-entry rules need the scene itself.
 * state_out (may be NULL): dev_scene's shade_features (the kShade* bits of csrc/device_scene.h), shade_models (bit m: some material has bsdf_type m) and alpha_maps. */
int ctl_scene_desc_check(const ctl_scene_desc* desc, uint32_t parts, uint32_t state_out[3]);
/* Applies everything that differs between the description `scene` holds and `new_desc`, except topology, in place; *mask_out (may be NULL) = the CTL_DIFF_* bits found.
 * Camera, materials, lights: host -> HBM copies (a material whose bsdf_type or alpha_state changed has the leaf entries of a flattened scene re-stamped by a kernel).
 * Transforms: the two-level arrays are re-uploaded and the flattened Q4 tree is REFITTED on the device (csrc/flat_refit.h: links, masks and memory order stay, every
 * box is recomputed, oriented slabs are neutralised) — the traversal still returns the reference's (t, u, v, triangle, node) bit for bit, a refitted tree only culls
 * less well than a rebuilt one the further the nodes moved.  Synchronous; call between passes and start the next one with new_trace.
 * Geometry (CTL_DIFF_GEOMETRY): the tri_data, Woop and BVH-node ranges of the meshes whose values differ are re-uploaded into the same allocations; in the flattened Q4
 * tree the leaf entries of those meshes get their triangle's new Woop rows on the device and stand for the whole triangle from then on (a split reference's clip box was
 * cut from the triangle as it was), then the tree is refitted as for a transform change — once, also when transforms and lights changed in the same call.
 *   CTL_ERR_NO_DEVICE    no device (checked first)
 *   CTL_ERR_INVALID      CTL_DIFF_TOPOLOGY is set: the scene is untouched, re-create it.  Also, with CTL_DIFF_TOPOLOGY added to *mask_out, a CTL_DIFF_GEOMETRY update of a
 *                        flattened scene in which a triangle that was degenerate at creation (singular Woop matrix: it has no leaf entry) is regular now;
 *                        ctl_last_error() names the mesh.  The other direction is fine: a triangle that collapses keeps its entry and can never be hit
 *   CTL_ERR_UNSUPPORTED  CTL_DIFF_TRANSFORMS or CTL_DIFF_GEOMETRY on a CTL_FLAT_Q8 scene (the measurement format is not refitted); camera / material / light updates work there
 * The scene keeps its own host copy of the description (the geometry arrays as hashes: one of their structure, one per mesh of their values, which tell an update WHICH
 * meshes changed): new_desc's pointers are not kept. */
int ctl_scene_update(ctl_scene* scene, const ctl_scene_desc* new_desc, uint32_t* mask_out);
/* Report of the last ctl_scene_update: summed surface area of the flattened tree's node boxes before and after a refit (a SAH proxy: a host calls
 * ctl_scene_rebuild_flat, below, or re-creates the scene when the ratio says the tree has degraded — the library has no policy), both 0 when the update did not refit; HIP-event time of the refit kernels. */
typedef struct { double node_area_before, node_area_after; float refit_ms; uint32_t refit_levels; uint32_t mask; uint32_t restamped; } ctl_scene_update_stats;
int ctl_scene_get_update_stats(ctl_scene* scene, ctl_scene_update_stats* out);
/* ---- skinned meshes: the reference's AnimatedMesh::k_ComputeState with g_ComputeVertices / g_ComputeTriangles (Engine/AnimatedMesh.{h,cpp,cu}) — the host hands over bone
 * matrices, the device does the rest (csrc/mesh_skin.h, mesh_skin.hip; INTEGRATION.md "Skinned meshes").  The calls act on a scene, not on the builder.
 *
 * ctl_scene_bind_skin binds mesh `mesh_index` of the scene to a rest pose and uploads the arrays once.  rest_positions, rest_normals and indices follow the conventions of
 * ctl_builder_add_mesh: indices == NULL is a triangle soup (n_vert == 3 * n_tri); rest_normals == NULL means Mesh::ComputeVertexNormals of the rest pose, once, on the host.
 * bone_indices and bone_weights are uint8[n_vert][8], the bytes of AnimatedVertex::m_cBoneIndices / m_fBoneWeights in memory order; a weight is byte / 255.0f and all eight
 * influences are always summed, as d_Compute does (weights need not sum to 255: TransformPoint divides by w).  Refusals come before anything is allocated:
 *   CTL_ERR_NO_DEVICE    no device (checked first)
 *   CTL_ERR_INVALID      a bad mesh index, another triangle count than the mesh's, a vertex index out of range, n_bones of 0 or above 256, an index byte >= n_bones (under a
 *                        zero weight too: the matrix is still read)
 *   CTL_ERR_UNSUPPORTED  a scene that is not a flattened CTL_FLAT_Q4 scene with refit data; a mesh whose nodes carry an area light, unless it is bound through
 *                        ctl_scene_bind_skin_ex with CTL_SKIN_AREA_LIGHTS (below; without the flag its shape sets are host work: ctl_builder_update_mesh); a mesh with a
 *                        triangle that was degenerate when the scene was flattened (it has no leaf entry)
 * A bound mesh is DEVICE-OWNED: ctl_scene_update neither compares nor uploads its values, whatever new_desc holds for it, and never reports CTL_DIFF_GEOMETRY for it — a
 * camera, material or transform update during an animation keeps the pose and stays cheap.  Binding a bound mesh again replaces the binding.
 *
 * ctl_scene_animate_mesh poses a bound mesh: n_bones ctl_float4x4 per pose, row-major like the node transforms; bones1 == NULL means bones0; the vertex is
 * lerp(M0 p, M1 p, lerp) with M = the weighted sum of its eight bone matrices.  Three kernels write the skinned vertices, the mesh's TriangleData (uv words and material bytes
 * stay) and every Woop row of its leaf stream; then the flattened tree's entries of the nodes that instance the mesh take the new rows and the tree is refitted, as after a
 * CTL_DIFF_GEOMETRY update.  A matrix entry or a lerp that is not finite, or a mesh that is not bound: CTL_ERR_INVALID, before the device is touched.  Synchronous, like
 * ctl_scene_update: call it between passes and start the next pass with new_trace.  stats_out (may be NULL) as ctl_scene_get_update_stats reports it (mask = CTL_DIFF_GEOMETRY);
 * ctl_scene_get_skin_ms: the HIP-event time of the three pose kernels of the last call (refit_ms is the flat-tree half).
 * What a pose leaves alone: the scene box, ray_trace_eps and the box-dependent lights stay as created — a host whose character leaves the scene box re-creates the scene, or
 * runs a host update (ctl_builder_update_mesh) —, and so do the nodes of the mesh's two-level BVH, which a flattened scene never traverses.
 *
 * ctl_scene_bind_skin_ex is ctl_scene_bind_skin with `flags`: 0 is the plain call, refusals included; an unknown bit is CTL_ERR_INVALID (after CTL_ERR_NO_DEVICE, before anything
 * else).  CTL_SKIN_AREA_LIGHTS binds a mesh whose nodes carry area lights — a glowing character, a swinging lamp.  Next-event estimation samples a DiffuseLight's shape set
 * (ctl_shape_tri records and the area CDF in the anim blob, sum_area in the light record), so every pose recomputes, ON THE DEVICE and after the three pose kernels, the shape
 * sets of every CTL_LIGHT_DIFFUSE light with count > 0 whose node_idx names a node that instances the mesh (csrc/shape_set.h, shape_set.hip): one lane per triangle, then the CDF
 * as ShapeSet's own serial fp32 sum in index order, so that the tables equal those of a host-updated description bit for bit.  ctl_scene_get_shape_set_ms: the HIP-event time
 * of those kernels in the last call that ran them (ctl_scene_get_skin_ms stays the three pose kernels).  OWNERSHIP: while such a mesh is bound, those ranges of the anim blob
 * and the sum_area of those lights are the device's.  Whenever the library uploads the light tables or the instance transforms of the scene — ctl_scene_update with
 * CTL_DIFF_LIGHTS, CTL_DIFF_TRANSFORMS or CTL_DIFF_GEOMETRY, ctl_scene_update_nodes — it runs the kernels again afterwards, by the lights, nodes and node transforms of the new
 * description: another radiance or a moved emissive node arrives, the pose stays, and the shape sets the host made for new_desc from its rest-pose rows are overwritten.
 * ctl_scene_unbind_skin marks the light tables stale: the next ctl_scene_update uploads new_desc's lights and anim blob whole, whatever the diff says, and reports CTL_DIFF_LIGHTS.
 *
 * ctl_scene_read_lights copies back the first n_lights light records and the first n_anim_bytes of the anim blob as HBM holds them, for any scene (either count may be 0;
 * more than the scene holds: CTL_ERR_INVALID).
 *
 * ctl_scene_read_mesh_geometry copies back what HBM holds (any pointer may be NULL): positions_out / normals_out float[n_vert][3], the skinned vertices of the last pose
 * (CTL_ERR_INVALID unless the mesh is bound and posed); tri_data_out and woop_out, the mesh's ranges of tri_data and of the Woop rows, for any mesh of any scene.
 *
 * ctl_scene_unbind_skin frees the binding and hands the mesh back to the description: its value hash is invalid from then on, so the next ctl_scene_update sees the mesh as
 * changed (CTL_DIFF_GEOMETRY) and restores the description's values.
 *
 * ctl_skin_mesh_host is the yardstick, host only: `desc` = the description the scene was made from, the bind arguments, the pose; returns the positions, the normals, the
 * mesh's TriangleData and its Woop rows through the same functions the kernels run (csrc/mesh_skin.h), bit for bit what ctl_scene_read_mesh_geometry reads back.
 *
 * ctl_shape_sets_host is the yardstick of the shape sets, host only: desc's light table and anim blob copied into lights_out[desc->n_lights_buf] and
 * anim_out[desc->n_anim_bytes], with the shape sets of the lights on nodes that instance `mesh_index` recalculated from tri_data / woop — the mesh's ranges, as
 * ctl_skin_mesh_host returns them — and desc's node transforms, through the functions the kernels run (csrc/shape_set.h): what ctl_scene_read_lights reads back after the pose. */
enum { CTL_SKIN_AREA_LIGHTS = 1 };
int ctl_scene_bind_skin(ctl_scene* scene, uint32_t mesh_index, const float* rest_positions, const float* rest_normals, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                        const uint8_t* bone_indices, const uint8_t* bone_weights, uint32_t n_bones);
int ctl_scene_bind_skin_ex(ctl_scene* scene, uint32_t mesh_index, const float* rest_positions, const float* rest_normals, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                           const uint8_t* bone_indices, const uint8_t* bone_weights, uint32_t n_bones, uint32_t flags);
int ctl_scene_animate_mesh(ctl_scene* scene, uint32_t mesh_index, const ctl_float4x4* bones0, const ctl_float4x4* bones1, float lerp, ctl_scene_update_stats* stats_out);
int ctl_scene_get_skin_ms(ctl_scene* scene, float* ms_out);
int ctl_scene_get_shape_set_ms(ctl_scene* scene, float* ms_out);
int ctl_scene_read_lights(ctl_scene* scene, ctl_light* lights_out, uint32_t n_lights, uint8_t* anim_out, size_t n_anim_bytes);
int ctl_shape_sets_host(const ctl_scene_desc* desc, uint32_t mesh_index, const ctl_triangle_data* tri_data, const ctl_woop_tri* woop, ctl_light* lights_out, uint8_t* anim_out);
int ctl_scene_read_mesh_geometry(ctl_scene* scene, uint32_t mesh_index, float* positions_out, float* normals_out, ctl_triangle_data* tri_data_out, ctl_woop_tri* woop_out);
int ctl_scene_unbind_skin(ctl_scene* scene, uint32_t mesh_index);
int ctl_skin_mesh_host(const ctl_scene_desc* desc, uint32_t mesh_index, const float* rest_positions, const float* rest_normals, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                       const uint8_t* bone_indices, const uint8_t* bone_weights, uint32_t n_bones, const ctl_float4x4* bones0, const ctl_float4x4* bones1, float lerp,
                       float* positions_out, float* normals_out, ctl_triangle_data* tri_data_out, ctl_woop_tri* woop_out);
/* ---- images in place: DynamicScene::ReloadTextures + UpdateMaterialsPhase2 (Engine/DynamicScene.cpp:457-, :84-89) on a live scene (csrc/scene_images.hip; INTEGRATION.md
 * "Updating an image").  ctl_scene_update_image replaces the level-0 texels of image `image_index` — width and height must be the image's; texel type, wrap and filter mode
 * stay — and rebuilds, in place, in the scene's own texel pool, anim blob, light table and material table, everything the library derives from texels:
 *   1. level 0 into the image's slot of the pool: a host -> device copy, or device -> device with CTL_IMAGE_TEXELS_DEVICE (`texels` is then a device pointer:
 *      ctl_device_malloc, a torch tensor);
 *   2. the pyramid, one kernel launch per level (csrc/mip_texel.h: decode, ((a + b) + c) + e, times 0.25, encode — the host builder's own functions);
 *   3. the sampling weights of the materials whose BSDF::Update() reads the image's average (ImageTexture::Average(): one texel of the coarsest level, read back), made on
 *      the host and patched into the device records that changed;
 *   4. if the image is an environment light's: cdfCols, cdfRows (csrc/env_tables.h; the running sums stay serial, one lane per row, in the reference's order) and the
 *      record's `normalization`.  A row of the map without luminance gives the reference's 1 / 0 and 0 * inf: the NaN entries of such a row may differ from a host-built
 *      description's in their payload bits;
 *   5. the scene's host copy of the description: materials, the light record, the table ranges of the anim blob (read back) and the image's digest (from `texels`, or from a
 *      read-back under CTL_IMAGE_TEXELS_DEVICE).
 * Afterwards the scene equals, bit for bit, one created from the description of a builder that went through ctl_builder_update_image + ctl_builder_finalize, and
 * ctl_scene_desc_diff / ctl_scene_update against that description find nothing.  It takes no description and works on any scene, two-level or flattened, for every plugin.
 * Synchronous, like ctl_scene_update: call it between passes and start the next pass with new_trace.  ctl_scene_desc_diff and ctl_scene_update still call another texel in a
 * description CTL_DIFF_TOPOLOGY.  stats_out (may be NULL): wall-clock times of the steps, each ended by a device synchronisation (env_ms includes the read-back of the tables).
 *   CTL_ERR_NO_DEVICE    no device (checked first)
 *   CTL_ERR_INVALID      a null scene or texels, a bad image index, another width or height (ctl_scene_update_image_set takes a replaced image), an unknown flag bit: before the
 *                        device is touched, the scene stays as it was
 * ctl_scene_read_image copies back level 0 and the pyramid of an image as the pool holds them, with the arguments and the layout of ctl_mip_pyramid_host. */
enum { CTL_IMAGE_TEXELS_DEVICE = 1 };   /* `texels` is a device pointer */
typedef struct { uint32_t levels, texels_written, materials_patched, env_tables;
                 float upload_ms, pyramid_ms, env_ms, hash_ms, total_ms; } ctl_scene_image_stats;
int ctl_scene_update_image(ctl_scene* scene, uint32_t image_index, const uint32_t* texels, uint32_t width, uint32_t height, uint32_t flags, ctl_scene_image_stats* stats_out);
int ctl_scene_read_image(ctl_scene* scene, uint32_t image_index, uint32_t* texels_out, size_t capacity, uint32_t* levels_out, uint32_t level_offsets_out[15]);
/* ---- ANOTHER SET OF IMAGES on a live scene (csrc/scene_image_set.h, scene_image_set.hip, scene_image_set.cpp; INTEGRATION.md "Editing the image set").  ctl_scene_update and
 * the node- and mesh-set calls refuse a description with another image set, and keep doing so; ctl_scene_update_image keeps an image's size.  ctl_scene_update_image_set takes
 * one: new_desc is the scene's description after ctl_builder_add_image, ctl_builder_remove_image and ctl_builder_replace_image, with whatever ctl_builder_set_material and
 * the light calls changed beside them.
 *   old_image_of_new[j]  the index image j had in the description the scene holds, or UINT32_MAX for a FRESH image (added, or replaced by another size);
 *                        n_new_images == new_desc->n_images; the kept indices strictly increasing (images are not reordered), fresh images anywhere
 * Accepted when, besides the map's rules: a kept image has the held width, height, texel type, wrap and filter mode and the held digest (texels written through
 * ctl_scene_update_image are fine when the host mirrored them with ctl_builder_update_image; after an update from a device pointer it reads them back with
 * ctl_scene_read_image first); every image has texels; everything else in new_desc is what ctl_scene_update applies — camera, the contents of the materials (n_materials may
 * grow, not shrink), lights and anim blob (a scene may gain its first environment map this way), transforms, volumes.  Another mesh set, node set, geometry structure or
 * values, or other transmittance tables are refused: those edits go through their own calls, before or after, each on its own finalized description.  ONE hash pass runs over
 * new_desc (hash_ms).  Everything is checked before the device is touched and before a tracer is stalled.
 * On the device the texel pool is laid out anew, in image order, exactly as ctl_scene_create lays it out: afterwards ctl_scene_read_image of every image equals a fresh
 * scene's, word for word.  The pyramids of the kept images MOVE, whole, by one kernel launch (k_move_texels: one lane per kept texel, the source found through a table of
 * runs — maximal groups of kept images consecutive in both pools), so their levels are not recomputed and what stands in HBM is what survives; a fresh image's level 0 is
 * uploaded into its slot and its pyramid built there, level by level, all fresh images before one synchronisation.  Nothing moves in place: DURING THE CALL HBM HOLDS THE OLD
 * POOL AND THE NEW ONE, and the new one (with the image and level tables at the new counts) becomes the scene's only at the commit.  Then the ordinary stages of
 * ctl_scene_update run over the rest of new_desc (a flattened tree is re-stamped where a material gained or lost an alpha map, refitted where a node moved; no tree is
 * rebuilt).  Two-level and flattened scenes, Q4 and Q8, every plugin; tracers follow the new arrays: start the next pass with new_trace.  An identity map over the same
 * count makes the call ctl_scene_update.  Synchronous.  Only the rough-transmittance tables still need a new scene.
 *   CTL_ERR_NO_DEVICE    no device (checked first)
 *   CTL_ERR_INVALID      every rule above, ctl_last_error() naming it; the scene stays as it was.  A failed allocation leaves the scene as it was too
 *   CTL_ERR_UNSUPPORTED  a transform change in new_desc on a CTL_FLAT_Q8 scene or a tree without refit data, as ctl_scene_update answers
 * stats_out (may be NULL): the counts of the map, the runs, the texels moved (whole pyramids) and uploaded (level 0 of fresh images), what the pool shrank by; HIP-event
 * times of the move and of the fresh images' uploads + pyramids; host time of the hash pass and of the whole call; the ctl_scene_update_stats of the stages that follow. */
typedef struct {
    uint32_t images_kept, images_fresh, images_removed, runs;
    uint64_t texels_moved, texels_uploaded, bytes_freed;
    float move_ms, pyramid_ms, hash_ms, total_ms;
    ctl_scene_update_stats update;
} ctl_scene_image_set_stats;
int ctl_scene_update_image_set(ctl_scene* scene, const ctl_scene_desc* new_desc, const uint32_t* old_image_of_new, uint32_t n_new_images, ctl_scene_image_set_stats* stats_out);
/* test hooks (no GPU).  ctl_image_set_plan_host: the whole acceptance check of ctl_scene_update_image_set for a scene made from old_desc, and its plan — offsets_out
 * [n_new_images]: the texel offset of every image's level 0 in the new pool; *total_out: the pool's texels; run_table_out[4 * (n_new_images + 1)] (may be NULL): per run
 * { first destination texel, first source texel, length, kept texels in front of it }, then the sentinel { *total_out, texels of the old pool, 0, texels moved };
 * *n_runs_out: the runs without the sentinel.  ctl_move_texels_host: k_move_texels' arithmetic on the host over such a table; words of new_pool no run covers are untouched. */
int ctl_image_set_plan_host(const ctl_scene_desc* old_desc, const ctl_scene_desc* new_desc, const uint32_t* old_image_of_new, uint32_t n_new_images,
                            uint64_t* offsets_out, uint64_t* total_out, uint64_t* run_table_out, uint32_t* n_runs_out);
int ctl_move_texels_host(const uint32_t* old_pool, uint64_t n_old_texels, const uint64_t* run_table, uint32_t n_runs, uint32_t* new_pool, uint64_t n_new_texels);
/* On-disk cache of compiled geometry — the role of the reference's .xmsh files (Engine/Mesh.cpp:46-98,199-290; DynamicScene::CreateNode
 * compiles a mesh only when its .xmsh is missing).  With a directory set, ctl_builder_add_mesh stores / reloads a compiled mesh
 * (TriangleData, BVH nodes, Woop rows) and CTL_SCENE_FLATTEN stores / reloads the flattened BVH, both keyed by a hash of their
 * inputs.  NULL or "" disables; the default comes from the environment variable CTL_CACHE_DIR.  Host only. */
int ctl_set_cache_dir(const char* dir);
/* The host half of CTL_SCENE_FLATTEN without a device (tests, cache warming): builds (or loads) the flattened BVH of `desc` in
 * node format `format` (CTL_FLAT_*) and reports out4 = { inner nodes, leaf entries, depth of the tree, low 64 bits of a hash of the arrays }. */
int ctl_flatten_probe(const ctl_scene_desc* desc, uint32_t format, uint64_t* out4);
/* The same, handing out the arrays (host memory owned by the handle): what ctl_scene_create_ex uploads.  The test oracle
 * traverses these very arrays on the CPU (counts "with the same BVH").  Layouts: cudatracerlib_amd/csrc/flatten.h. */
typedef struct ctl_flat_bvh ctl_flat_bvh;
typedef struct {
    uint32_t format, max_depth;      /* CTL_FLAT_*, depth of the stored tree                                      */
    const void* nodes; uint64_t n_nodes; uint32_t node_bytes;   /* node 0 is the root; child >= 0: node index * node_bytes / 16 */
    const void* leaves; uint64_t n_leaves;   /* 128 B each: object-space Woop rows a,b,c, {globalTri << 1 | last, node, 0, 0}, rows 0..2 of the node's inverse transform, {w33,0,0,0} */
    const int32_t* child_links;      /* CTL_FLAT_Q4: 4 explicit links per node (>= 0: node index * 4, < 0: ~first leaf entry, 0x76543210: none); CTL_FLAT_Q8: 8 per node, slot order (>= 0: node index); else NULL */
    uint32_t compact;                /* CTL_FLAT_Q4: 1 = the kernels derive the links from the layout (flat4_node::links) and the nodes' last 16 B hold oriented slabs; CTL_FLAT_Q8: always 1 */
    uint32_t root_slab;              /* the root node carries a slab (Q4: bit 0 of the link a traversal starts with; Q8: the root's q5 is loaded)            */
    uint64_t n_slab_nodes;           /* nodes that carry an oriented slab (flat_slab.h)                                                  */
    /* the refit side data of a CTL_FLAT_Q4 tree (csrc/flat_refit.h; NULL / 0 otherwise), built or read back from a scene: per leaf entry UINT32_MAX or the index of its
     * clip box — the entry is a split reference —, and the clip boxes {lo xyz, hi xyz} in world space as they were when the tree was built.  A geometry refit sets the
     * entries of the deformed meshes to UINT32_MAX */
    const uint32_t* part_index; const float* part_boxes; uint64_t n_part_boxes;
} ctl_flat_bvh_desc;
int ctl_flat_bvh_build(const ctl_scene_desc* desc, uint32_t format, ctl_flat_bvh** out);
int ctl_flat_bvh_arrays(const ctl_flat_bvh* h, ctl_flat_bvh_desc* out);
void ctl_flat_bvh_destroy(ctl_flat_bvh* h);
/* The refit of ctl_scene_update on the arrays of a CTL_FLAT_Q4 handle, host only, with the same arithmetic (csrc/flat_refit.h): the yardstick of the device kernels.
 * new_desc = the description the handle was built from with other node transforms and / or other vertex values in some meshes (ctl_builder_update_mesh; the handle
 * tells them by the per-mesh hashes it keeps): the entries of those meshes take their new Woop rows and become whole, which the part_index of ctl_flat_bvh_arrays
 * shows afterwards.  CTL_ERR_INVALID where ctl_scene_update would refuse the geometry (another structure, a degenerate triangle that is regular now).
 * Other formats: CTL_ERR_UNSUPPORTED. */
int ctl_flat_bvh_refit(ctl_flat_bvh* h, const ctl_scene_desc* new_desc);
/* ---- rebuild of the flattened tree (csrc/flat_rebuild.h, flat_rebuild.hip, flat_rebuild.cpp; INTEGRATION.md "Updating a scene").  A refit keeps the tree correct, not
 * good: after large motions the node area grows and the rays/s fall (RESULTS.md "In-place scene updates").  ctl_scene_rebuild_flat makes a NEW tree on the device, in
 * place, from what the scene holds — the leaf entries as they stand in HBM after any number of updates, deformations and poses, and the transforms of the last update:
 * entry boxes, a 63-bit Morton code per entry, a radix sort, Karras's binary hierarchy over the sorted codes collapsed 4-wide level by level, the entries gathered into
 * their new order, the boxes by the refit kernels.  The set of entries does not change (a triangle that was degenerate at creation still needs a new scene); split
 * references keep their clip box; the rebuilt tree carries no oriented slabs.  Hits stay the reference's bit for bit: the tree only culls.  Synchronous like
 * ctl_scene_update: call it between passes and start the next pass with new_trace; tracers follow the new arrays by themselves.  Everything that worked on the old tree
 * works on the new one (ctl_scene_update, ctl_scene_animate_mesh, ctl_scene_read_flat_bvh, another rebuild).  The library has no policy: the host decides when to call
 * (an LBVH without slabs or split decisions of its own may trace slower than a lightly refitted tree).
 * Memory: during the call the entries exist twice (a second buffer of 128 B per entry — 1.1 GB more on an 8.6 M-entry scene) next to the sort's keys and a node buffer
 * of 32 B per entry; the old node and entry buffers are freed after the swap.
 * Refusals, all before anything is written: CTL_ERR_NO_DEVICE (checked first); CTL_ERR_UNSUPPORTED for a scene that is not flattened, a CTL_FLAT_Q8 scene, a tree
 * without refit data or with explicit links, and a rebuilt tree whose depth does not fit the traversal stack (the new tree is made in buffers of its own; the old one
 * stays in place).  A failed allocation leaves the scene as it was.
 * stats_out (may be NULL): the node areas as ctl_scene_update_stats reports them (before = the tree as it stood, after = the rebuilt one); HIP-event times of the key +
 * sort stage, the topology + gather stage, the box stages (entry boxes + node boxes) and the whole call.
 * ctl_flat_bvh_rebuild does the same to a host handle for the pose of new_desc — a ctl_flat_bvh_refit to new_desc followed by the rebuild, with the same single-source
 * arithmetic: the yardstick of the device, byte for byte (nodes, entries, part_index, levels).  Too deep a tree: CTL_ERR_UNSUPPORTED with the handle left refitted.
 * ctl_flat_bvh_levels: the nodes by depth as the refit walks them (level l = level_nodes[level_start[l] .. level_start[l + 1])); after a rebuild level_nodes is 0, 1, 2 .. */
typedef struct { uint32_t n_nodes, n_entries, max_depth, levels; double node_area_before, node_area_after; float sort_ms, topology_ms, refit_ms, total_ms; } ctl_scene_rebuild_stats;
int ctl_scene_rebuild_flat(ctl_scene* scene, ctl_scene_rebuild_stats* stats_out);
int ctl_flat_bvh_rebuild(ctl_flat_bvh* h, const ctl_scene_desc* new_desc);
int ctl_flat_bvh_levels(const ctl_flat_bvh* h, const uint32_t** level_start, uint32_t* n_levels, const uint32_t** level_nodes, uint64_t* n_level_nodes);
/* ---- the builder of a rebuild (csrc/flat_ploc.h; DESIGN.md "PLOC", INTEGRATION.md "Updating a scene").  Every call that rebuilds the flattened tree has an _ex form
 * that names the builder of the binary tree the wide nodes are collapsed from; the plain forms are the _ex forms with CTL_REBUILD_LBVH, byte for byte.
 *   CTL_REBUILD_LBVH   Karras's radix tree over the sorted Morton codes: the cheapest call, the largest node area
 *   CTL_REBUILD_PLOC   parallel locally-ordered clustering (Meister & Bittner): from the same sorted order, rounds in which every cluster picks, among the 8 clusters to
 *                      either side, the one whose union box with its own is smallest (ties: the smaller XOR of the two positions), and clusters that picked each other merge; then the same collapse, layout and box
 *                      stages.  A smaller node area (tests/test_flat_ploc_host.py) for some tens of rounds of launches more (RESULTS.md has the measured cost and rays/s)
 * Entries, clip boxes, hits and everything a later call may do to the tree are as after the plain call; host handle and device agree byte for byte as they do there.
 * Memory: CTL_REBUILD_PLOC takes 88 B per entry more during the call (the cluster boxes and ids twice — one read, one written per round —, every cluster's pick,
 * the round's flag words and their scan, the binary tree's child and count arrays): 0.76 GB on an 8.6 M-entry scene, next to what the plain call takes, freed when it
 * returns.  topology_ms includes the clustering.
 * Refusals besides the plain calls', all before anything is written: CTL_ERR_INVALID for a builder that is none of the constants; CTL_ERR_UNSUPPORTED when the clustering
 * has not finished after 8 ceil(log2 entries) + 16 rounds; CTL_ERR_INTERNAL for a round that merged nothing (the tie rule excludes it).  The tree that was there stays.
 * ctl_rebuild_last_rounds: the clustering rounds of the calling thread's last rebuild of either kind (0 after CTL_REBUILD_LBVH). */
enum { CTL_REBUILD_LBVH = 0, CTL_REBUILD_PLOC = 1 };
int ctl_scene_rebuild_flat_ex(ctl_scene* scene, int builder, ctl_scene_rebuild_stats* stats_out);
int ctl_flat_bvh_rebuild_ex(ctl_flat_bvh* h, const ctl_scene_desc* new_desc, int builder);
uint32_t ctl_rebuild_last_rounds(void);
/* TEST SUPPORT, not part of the product interface (no host needs it; it may change with the rebuild's internals): what stages 1 - 4 hand to either builder, for a host handle as it stands (refitted to desc) and the transforms of desc, nothing written: sorted_entry[s] = the entry at
 * sorted position s (n_leaves elements), entry_boxes = lo xyz, hi xyz of every entry BY ENTRY INDEX (6 n_leaves floats; an entry without a box has lo > hi),
 * bounds = lo xyz, hi xyz of the boxes that are not inverted.  tests/ploc_ref.py restates stages 5 - 7 from these.  Refuses what ctl_flat_bvh_rebuild refuses (a handle
 * whose description has gained a triangle since a node was added included). */
int ctl_flat_bvh_rebuild_order(const ctl_flat_bvh* h, const ctl_scene_desc* desc, uint32_t* sorted_entry, float* entry_boxes, float* bounds);
/* ---- another SET OF NODES on a live scene (csrc/flat_nodes.h, flat_nodes.hip, flat_nodes.cpp; INTEGRATION.md "Updating a scene").  ctl_scene_update refuses a
 * description with other nodes (CTL_DIFF_TOPOLOGY), and keeps doing so; ctl_scene_update_nodes takes one: new_desc is the scene's description after
 * ctl_builder_remove_node and / or ctl_builder_add_node of further instances of meshes the scene already holds.
 *   old_of_new[k]   the index new node k had in the description the scene holds, or UINT32_MAX for an added node; the kept indices strictly increasing (the builder
 *                   never reorders: a removal shifts down, an addition appends); n_new_nodes == new_desc->n_nodes
 * On a flattened CTL_FLAT_Q4 scene, on the device: the leaf entries of removed nodes are dropped and the kept ones renumbered (a flag per entry, a scan, a stable move);
 * one entry per regular triangle of every added node is made from the mesh's Woop rows AS THEY STAND IN HBM (a deformed or posed mesh gives the new instance its current
 * shape; a triangle whose Woop matrix is singular gets no entry, and a later geometry update that makes it regular is refused as for a triangle that was degenerate at
 * creation); then the tree is rebuilt over the new set by the stages of ctl_scene_rebuild_flat.  Added instances get WHOLE-triangle entries (part_index UINT32_MAX, no
 * early split clipping): they cull less well on long triangles, never wrongly.  On a two-level scene the call is host work: top level, instances, node info and the
 * material table go into buffers of the new size.  Tracers follow the new arrays by themselves; start the next pass with new_trace.  Bound meshes stay bound.
 * Accepted besides the node set: everything ctl_scene_update applies (camera, the contents of kept materials, lights — an added node may carry area lights —, the
 * transforms of kept nodes, the scene BVH, box, ray_trace_eps, volumes), in the same call; n_materials may grow (the added nodes' copies), not shrink.  An identity map
 * over the same count is valid: the call then is ctl_scene_update, without a rebuild.
 * Refusals, all before anything is written and before a tracer is stalled, the scene as it was and ctl_last_error() naming the rule: CTL_ERR_NO_DEVICE (checked first);
 * CTL_ERR_INVALID for a null, short, non-increasing or out-of-range map, a kept node with another mesh or material assignment, another mesh set, geometry structure,
 * image set or transmittance tables, other geometry VALUES in a mesh that is not device-owned (ctl_scene_update first), a description ctl_scene_desc_check refuses, no
 * node left; CTL_ERR_UNSUPPORTED for a CTL_FLAT_Q8 scene, a tree without refit data or with explicit links, and a rebuilt tree too deep for the traversal stack (it is
 * made in buffers of its own; the old one stays).  A failed allocation leaves the scene as it was.  The library has no policy: whether this call or a new scene is the
 * better answer (the result is an LBVH without slabs or split decisions) is the host's decision.
 * stats_out (may be NULL): the entry counts, what ctl_scene_rebuild_stats reports (rebuild), HIP-event times of the drop + generate stage and of the whole call.
 * ctl_flat_bvh_update_nodes does the same to a host handle (of ctl_flat_bvh_build or ctl_scene_read_flat_bvh) with the same single-source functions, reading the Woop
 * rows from new_desc: the yardstick — after the device call ctl_scene_read_flat_bvh equals it byte for byte (nodes, entries, part_index, level lists, max_depth). */
typedef struct {
    uint32_t entries_before, entries_after, entries_dropped, entries_generated, degenerate_skipped, rebuilt;   /* rebuilt: 0 = an identity map (no rebuild) or a two-level scene */
    ctl_scene_rebuild_stats rebuild;
    float edit_ms, total_ms;   /* drop + generate; the whole device work of the call */
} ctl_scene_nodes_stats;
int ctl_scene_update_nodes(ctl_scene* scene, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes, ctl_scene_nodes_stats* stats_out);
int ctl_flat_bvh_update_nodes(ctl_flat_bvh* h, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes);
/* the same with the builder of the rebuild stage named (CTL_REBUILD_LBVH: the plain calls; see "the builder of a rebuild" above).  After a node-set edit the host has no
 * refitted tree to fall back on, so the builder is the whole choice: INTEGRATION.md says which to ask for. */
int ctl_scene_update_nodes_ex(ctl_scene* scene, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes, int builder, ctl_scene_nodes_stats* stats_out);
int ctl_flat_bvh_update_nodes_ex(ctl_flat_bvh* h, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes, int builder);
/* ---- NEW MESHES on a live scene (csrc/flat_meshes.h, flat_meshes.hip, flat_meshes.cpp; INTEGRATION.md "Adding meshes").  ctl_scene_update and ctl_scene_update_nodes
 * refuse a description with another mesh set, and keep doing so; ctl_scene_update_meshes takes one that APPENDS meshes: new_desc is the scene's description after further
 * ctl_builder_add_mesh calls (the builder only ever appends to tri_data, woop, woop_index, bvh_nodes and meshes) and any node-set edit ctl_scene_update_nodes takes —
 * added nodes may instance held or appended meshes, an appended mesh may have no node.  old_of_new, n_new_nodes: as for ctl_scene_update_nodes.
 * Accepted when: n_meshes, n_tri_data, n_woop and n_bvh_nodes are at least the held counts; the held mesh records are a byte-equal prefix of meshes; every appended mesh
 * lies wholly behind the old ends of the arrays (tri_offset >= the held n_tri_data; bvh_tri_offset / 3 and bvh_index_offset >= the held n_woop; bvh_node_offset / 4 >= the
 * held n_bvh_nodes) and inside the new ones, the first appended mesh starting, in each of the three arrays, exactly where the held elements end; the geometry hashes of new_desc restricted to the held
 * counts equal the scene's (other VALUES in a held mesh that is not device-owned: ctl_scene_update first); images, transmittance tables, materials and kept nodes follow the
 * rules of ctl_scene_update_nodes (a new mesh's materials may only name images the scene has); ctl_scene_desc_check accepts new_desc, the two-level stack depth with the
 * new meshes' BVHs included.  Nothing appended: the call is ctl_scene_update_nodes, the append part of the stats zero.
 * On the device: tri_data, the mesh BVH nodes, the two-level leaf stream and — where the scene has one — the triangle -> row table grow into NEW buffers: the old contents
 * are copied device to device (deformed and posed values live nowhere else), the tails are uploaded in creation's layouts, k_append_leaf_rows interleaves the appended
 * Woop rows with their index words and extends the table (the first row in stream order that names a triangle).  The node-set stages of ctl_scene_update_nodes then read
 * the grown buffers, and the buffers become the scene's only after the new tree stands.  Any growth rebuilds the flattened tree, an identity node map included.
 * During the call HBM holds a second copy of the three geometry arrays.  Tracers follow the new arrays; start the next pass with new_trace.  Bound meshes stay bound.
 * Refusals leave the scene as it was: CTL_ERR_NO_DEVICE first; CTL_ERR_INVALID for wrong arguments and every rule above; CTL_ERR_UNSUPPORTED exactly where
 * ctl_scene_update_nodes answers so.  A failed allocation leaves the scene as it was.  New images go through ctl_scene_update_image_set, on a description of its own; new tables still need a new scene.
 * ctl_flat_bvh_update_meshes is the host yardstick (no GPU): the same acceptance, then ctl_flat_bvh_update_nodes' stages, which read the Woop rows from new_desc. */
typedef struct {
    uint32_t meshes_added, triangles_added, rows_added, bvh_nodes_added;   /* rows: of the two-level leaf stream (n_woop) */
    float append_ms, hash_ms;      /* HIP events around the growth copies, the uploads and k_append_leaf_rows; host time hashing new_desc (twice: the held part, the whole) */
    ctl_scene_nodes_stats nodes;   /* the stages that follow */
} ctl_scene_meshes_stats;
int ctl_scene_update_meshes(ctl_scene* scene, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes, ctl_scene_meshes_stats* stats_out);
int ctl_scene_update_meshes_ex(ctl_scene* scene, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes, int builder, ctl_scene_meshes_stats* stats_out);
int ctl_flat_bvh_update_meshes(ctl_flat_bvh* h, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes);
int ctl_flat_bvh_update_meshes_ex(ctl_flat_bvh* h, const ctl_scene_desc* new_desc, const uint32_t* old_of_new, uint32_t n_new_nodes, int builder);
/* test hooks (no GPU).  ctl_triangle_woop_rows: per triangle of desc->tri_data the first row of the leaf stream that names it, UINT32_MAX for none (n_tri_data words).
 * ctl_append_leaf_rows_host: k_append_leaf_rows' arithmetic on the host for the rows new_desc appends to held counts — tri_row holds new_desc->n_tri_data words, the first
 * old_n_tri_data of them the held table; leaf_rows_out (may be NULL) receives 16 words per appended row. */
int ctl_triangle_woop_rows(const ctl_scene_desc* desc, uint32_t* rows_out);
/* ctl_scene_read_triangle_rows (test hook): the triangle -> row table as HBM holds it.  *count_out = its words (0: the scene has none yet — the first geometry update,
 * skin binding or node-set change makes it); rows_out (may be NULL) receives them when capacity is at least that. */
int ctl_scene_read_triangle_rows(ctl_scene* scene, uint32_t* rows_out, size_t capacity, size_t* count_out);
int ctl_append_leaf_rows_host(const ctl_scene_desc* new_desc, uint32_t old_n_meshes, uint32_t old_n_tri_data, uint32_t old_n_woop, uint32_t old_n_bvh_nodes, uint32_t* tri_row, uint32_t* leaf_rows_out);
/* ---- REMOVED MESHES on a live scene (csrc/flat_mesh_set.h, flat_mesh_set.hip, flat_mesh_set.cpp; INTEGRATION.md "Removing meshes").  ctl_scene_update,
 * ctl_scene_update_nodes and ctl_scene_update_meshes refuse a description with a mesh removed, and keep doing so; ctl_scene_update_mesh_set takes one: new_desc is the
 * scene's description after ctl_builder_remove_mesh, further ctl_builder_add_mesh calls and any node-set edit — removal, append and node set in one call.
 *   old_mesh_of_new[m]  the index new mesh m had in the description the scene holds, or UINT32_MAX for an appended mesh; n_new_meshes == new_desc->n_meshes.  The kept
 *                       indices strictly increasing (no reordering), the appended meshes all behind the kept ones, as the builder appends
 *   old_of_new          as for ctl_scene_update_nodes;   builder: CTL_REBUILD_LBVH or CTL_REBUILD_PLOC
 * A map that removes nothing makes the call ctl_scene_update_meshes_ex (and one that appends nothing either, ctl_scene_update_nodes_ex), the removal part of the stats zero.
 * Accepted when, besides the map's rules: no kept node (through old_of_new) instances a removed mesh, and a kept node's mesh is its old mesh through the map, its material
 * assignment unchanged; no removed mesh is bound to a skin (ctl_scene_unbind_skin first); every kept mesh's record equals the held record with its offsets lowered by
 * exactly the triangles, leaf rows and BVH nodes removed in front of it, std_material_offset equal; the appended meshes follow the compacted ends exactly, as in
 * ctl_scene_update_meshes; structure (woop_index and mesh BVH links, which are mesh-relative: per-mesh hash words) and values of every kept mesh are unchanged — the values
 * of a device-owned mesh are neither read nor compared —; images, transmittance tables and materials follow the rules of ctl_scene_update_nodes; ctl_scene_desc_check
 * accepts new_desc.  Everything is checked before anything is written or a tracer is stalled.
 * On the device the kept ranges of tri_data, the mesh BVH nodes, the two-level leaf stream and — where the scene has one — the triangle -> row table are COMPACTED into
 * NEW, smaller buffers: k_compact_quads moves 16-B quads, one lane per destination quad, the source found through a table of runs (maximal groups of consecutive kept
 * meshes); k_compact_tri_rows lowers the table's words by each run's row delta.  The source is what stands in HBM, so deformed and posed meshes keep their shape.  Nothing
 * moves in place: DURING THE CALL HBM HOLDS THE OLD ARRAYS AND THE COMPACTED ONES, and the new buffers become the scene's only after the new tree stands.  The appended
 * tails and the node-set stages follow as in ctl_scene_update_meshes; the leaf entries of kept nodes get their triangle words lowered while they move.  Any removal
 * rebuilds the flattened tree, an identity node map included.  Bound meshes stay bound under their new indices; tracers follow the new arrays: start the next pass with
 * new_trace.  Refusals leave the scene as it was: CTL_ERR_NO_DEVICE first; CTL_ERR_INVALID for wrong arguments and every rule above; CTL_ERR_UNSUPPORTED exactly where
 * ctl_scene_update_nodes answers so.  The material table is not compacted; another image set goes through ctl_scene_update_image_set (a removed mesh's textures: INTEGRATION.md "Editing the image set"); new tables still need a new scene.
 * ctl_flat_bvh_update_mesh_set is the host yardstick (no GPU): the same acceptance, then ctl_flat_bvh_update_nodes' stages with the triangle words lowered. */
typedef struct {
    uint32_t meshes_removed, triangles_removed, rows_removed, bvh_nodes_removed;   /* rows: of the two-level leaf stream (n_woop) */
    uint32_t runs, reserved;                /* the runs of kept meshes the compaction kernels searched */
    uint64_t bytes_moved, bytes_freed;      /* by the compaction kernels; what the scene's geometry arrays shrank by through the removal */
    float compact_ms, hash_ms;              /* HIP events around the compaction launches; host time of the ONE hash pass over new_desc */
    ctl_scene_meshes_stats meshes;          /* the append and the node-set stages that follow (its hash_ms repeats hash_ms) */
} ctl_scene_mesh_set_stats;
int ctl_scene_update_mesh_set(ctl_scene* scene, const ctl_scene_desc* new_desc, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes,
                              const uint32_t* old_of_new, uint32_t n_new_nodes, int builder, ctl_scene_mesh_set_stats* stats_out);
int ctl_flat_bvh_update_mesh_set(ctl_flat_bvh* h, const ctl_scene_desc* new_desc, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes,
                                 const uint32_t* old_of_new, uint32_t n_new_nodes, int builder);
/* test hook (no GPU): k_compact_tri_rows' arithmetic on the host.  held_rows: the table of old_desc (old_desc->n_tri_data words); rows_out (as many words of room) receives
 * the compacted table of the kept meshes, *count_out its length. */
int ctl_compact_tri_rows_host(const ctl_scene_desc* old_desc, const uint32_t* old_mesh_of_new, uint32_t n_new_meshes, const uint32_t* held_rows, uint32_t* rows_out, uint32_t* count_out);
/* The flattened tree of a CTL_SCENE_FLATTEN scene copied back from HBM into a handle for ctl_flat_bvh_arrays, with the BSDF-model bits (28..31 of the index word)
 * and the alpha bit (31 of the node word) that ctl_scene_create_ex stamps into the device copy removed: the arrays the test oracle traverses. */
int ctl_scene_read_flat_bvh(ctl_scene* scene, ctl_flat_bvh** out);
/* ParseMitsubaScene (Engine/SceneLoader/Mitsuba/MitsubaLoader.h:13): fills a builder from a Mitsuba-0.5 XML file. */
int ctl_parse_mitsuba_scene(ctl_builder* b, const char* xml_path, int32_t* width_inout, int32_t* height_inout);
/* The same with ParseMitsubaScene's create_exterior_bssrdf / create_interior_bssrdf (flags = 0: ctl_parse_mitsuba_scene, which creates no media and refuses <medium>).
 * With a flag set, ObjectParser.h:1066-1101 and MediumParser::homogeneous (:177-214) as written: a shape WITHOUT a BSDF whose `exterior` / `interior` is a homogeneous
 * medium — inline, or a <ref> to a <medium id=...> — creates a volume and has its node removed when the parse ends.  An inline medium lies over the scene box as it
 * stands at that point of the parse (Translate(box.min) % Scale(box.Size()), the shape's own node included); a referenced medium keeps the transform it was parsed with,
 * the identity for a top-level <medium>: the reference resolves the <ref> before it looks at the transform.  sigmaA / sigmaS or sigmaT / albedo, scale, and
 * <phase type="isotropic|hg|rayleigh|kkay">.  Refused (CTL_ERR_UNSUPPORTED; skipped under CTL_LOADER_LENIENT): material= presets (MaterialLibrary), heterogeneous media,
 * a medium on a shape that has a BSDF (Material::bssrdf).  Unknown flag bits: CTL_ERR_INVALID. */
enum { CTL_PARSE_EXTERIOR_MEDIA = 1, CTL_PARSE_INTERIOR_MEDIA = 2 };
int ctl_parse_mitsuba_scene_ex(ctl_builder* b, const char* xml_path, int32_t* width_inout, int32_t* height_inout, uint32_t flags);
/* The bitmap reader behind the loader's textures and environment maps (the reference goes through FreeImage, Engine/MIPMap.cu:542-592): PNG, JPEG
 * (sequential and progressive), BMP, TGA, PNM, PFM, Radiance HDR, OpenEXR (scanline; NONE / RLE / ZIPS / ZIP).  Rows top-down.  *is_float = 1: `rgb`
 * receives 3 floats per pixel; 0: `rgba8` receives 4 bytes per pixel.  With both buffers NULL only the size and kind are returned. */
int ctl_decode_image_file(const char* path, uint32_t* width, uint32_t* height, int32_t* is_float, float* rgb, uint8_t* rgba8);

/* ------------------------------------------------------------------ sampler */
/* SequenceSamplerData(4096, 30) (Kernel/Sampler_device.h:11-57). tables_1d[30*4096], tables_2d[30*4096*2]:
 * element (seq, e) at e*4096+seq. */
#define CTL_SAMPLER_NUM_SEQUENCES 4096
#define CTL_SAMPLER_SEQUENCE_LENGTH 30
typedef struct ctl_sequence_generator ctl_sequence_generator;
/* IndependantSamplingSequenceGenerator (Kernel/Sampler.h:57-85): XORWOW curand_init(1234, 7539414, 0). */
int ctl_sequence_generator_create(ctl_sequence_generator** out);
void ctl_sequence_generator_destroy(ctl_sequence_generator* g);
/* SamplingSequenceGeneratorHost::Compute (Kernel/Sampler.h:36-55): next pass's tables into host buffers. */
int ctl_sequence_generator_compute(ctl_sequence_generator* g, float* tables_1d, float* tables_2d);
/* the tables of the next n_passes passes (consecutive [30*4096] / [30*4096*2] blocks), generated by up to `threads` host
 * threads; same values as n_passes calls of ctl_sequence_generator_compute (XORWOW skip-ahead) */
int ctl_sequence_generator_compute_many(ctl_sequence_generator* g, uint32_t n_passes, float* tables_1d, float* tables_2d, uint32_t threads);
/* The same tables written in HBM by the kernel the tracers use (k_sequence_fill: the host only advances the stream) and copied back: bit-identical to
 * ctl_sequence_generator_compute_many.  Needs a HIP device. */
int ctl_sequence_generator_compute_many_device(ctl_sequence_generator* g, uint32_t n_passes, float* tables_1d, float* tables_2d);

/* -------------------------------------------------------------------- image */
typedef struct ctl_image ctl_image;
int ctl_image_create(uint32_t width, uint32_t height, ctl_image** out);   /* Image::Image (Engine/Image.h:34) */
void ctl_image_destroy(ctl_image* img);
int ctl_image_clear(ctl_image* img);                                        /* Image::Clear                    */
int ctl_image_read_pixels(ctl_image* img, ctl_pixel_data* host_out);        /* D2H of the PixelData array      */
int ctl_image_write_pixels(ctl_image* img, const ctl_pixel_data* host_in);
/* Image::AddSample (Engine/Image.h:56, Image.cu:22-44) for `n` samples {sx, sy, r, g, b} in host memory: negatives clamped, a NaN / infinite radiance or a position outside the
 * film dropped, the pixel floor(sx), floor(sy) receives rgb += L, weightSum += 1 (float atomics, as the reference's device branch).  What a plugin that does not use the
 * tracer's own accumulation calls to deposit its radiance. */
int ctl_image_add_samples(ctl_image* img, uint32_t n, const float* host_samples5);
void* ctl_image_device_ptr(ctl_image* img);                                 /* PixelData* in HBM (RCCL gather) */
/* copySamplesToOutput (Kernel/ImagePipeline/ImagePipeline.cu:14-30): rgb/weight + splat*scale -> linear RGB float */
int ctl_image_resolve_rgb(ctl_image* img, float splat_scale, float* host_rgb_out);
/* applyImagePipeline(tracer, img, filter = 0, process = 0) (Kernel/ImagePipeline/ImagePipeline.cu:54-63): the display image,
 * sRGB transfer curve + 8-bit RGBCOL per pixel (byte 0 = r, alpha = 255).  splat_scale = TracerBase::getSplatScale() = 1/passes. */
int ctl_image_apply_pipeline(ctl_image* img, float splat_scale, uint32_t* host_rgbcol_out);
/* The other three branches of applyImagePipeline (ImagePipeline.cu:64-81): an ImageSamplesFilter and / or a PostProcess.
 * filter  = CanonicalFilter over a reconstruction Filter (Kernel/ImagePipeline/Filter/CanonicalFilter.cu:6-44, SceneTypes/Filter.h:
 *           ids = TYPE_FUNC ids; p0 / p1 = Gaussian alpha | Mitchell B, C | Lanczos tau); the filtered image is kept as RGBE.
 * process = ToneMapPostProcess, Reinhard et al. (PostProcess/ToneMapPostProcess.cu:6-42) driven by Image::ComputeLuminanceInfo
 *           (Engine/Image.cu:88-168) of the RGBE image; the result is quantised to RGBCOL and then gamma-corrected, as there.
 * Either may be NULL (both NULL = ctl_image_apply_pipeline). */
enum { CTL_RFILTER_BOX = 1, CTL_RFILTER_GAUSSIAN = 2, CTL_RFILTER_MITCHELL = 3, CTL_RFILTER_LANCZOS = 4, CTL_RFILTER_TRIANGLE = 5 };
typedef struct { uint32_t type; float x_width, y_width, p0, p1; } ctl_reconstruction_filter;
typedef struct { float key, burn; } ctl_tonemap;           /* defaults of the reference: key 0.18, burn 0 */
int ctl_image_apply_pipeline_ex(ctl_image* img, float splat_scale, const ctl_reconstruction_filter* filter, const ctl_tonemap* process,
                                uint32_t* host_rgbcol_out);
/* Image::WriteDisplayImage (Engine/Image.cpp:67-75): .png writes the display image, .hdr / .pfm the linear float image.
 * Other formats (the reference saves through FreeImage) -> CTL_ERR_UNSUPPORTED. */
int ctl_image_write_file(ctl_image* img, float splat_scale, const char* path);

/* ---------------------------------------------------------------- multi-GPU */
/* The one exchange step of a multi-GPU render (the reference is single-device): rank r renders the 64x64 image tiles t with
 * t % world == r (ctl_tracer_set_tile_shard) into a cleared full-size Image.  ctl_image_gather brings every rank's own tiles to `root`'s image
 * with ONE ncclGather over RCCL / xGMI; ctl_image_reduce (the fallback) sums the whole PixelData frames with ONE ncclReduce — the tiles are
 * disjoint, so the sum is the gather, at 8x the bytes.  One rank per process and GPU: call ctl_set_device first.  ctl_comm_get_unique_id on one rank, hand the 128 bytes to the others by any means (MPI_Bcast, a file,
 * torch.distributed), then ctl_comm_create on every rank (collective).  RCCL is loaded on first use. */
typedef struct ctl_comm ctl_comm;
int ctl_comm_get_unique_id(uint8_t out128[128]);
int ctl_comm_create(const uint8_t id128[128], int32_t rank, int32_t world, ctl_comm** out);
void ctl_comm_destroy(ctl_comm* c);
/* ctl_comm_create with a deadline: ncclCommInitRank is collective and waits for ever for a rank that never arrives; after timeout_ms (<= 0: $CTL_COMM_TIMEOUT_MS, else
 * 120 000) the call fails with CTL_ERR_INVALID and a message naming the rank, so that the host can fall back or stop the job.  ctl_comm_create uses the default. */
int ctl_comm_create_timeout(const uint8_t id128[128], int32_t rank, int32_t world, int32_t timeout_ms, ctl_comm** out);
/* In place: the root's image becomes the sum over the ranks.  ONE call per render: with more than one rank a second call on an image that already went through an in-place
 * exchange is refused with CTL_ERR_INVALID on EVERY rank, before any of them enters the collective (it would add the other ranks' cumulative tiles onto sums that contain
 * them), until the image is cleared or rewritten. */
int ctl_image_reduce(ctl_image* img, ctl_comm* comm, int32_t root);
/* Out of place — the per-pass gather of a progressive display (the reference shows the frame after every DoPass, main.cpp:164-172): dst on the root receives the sum over the
 * ranks of `src`; every rank's src (its own cumulative tile frame) is left as it is, so the call can be repeated after every pass.  dst may be NULL on the other ranks.
 * K per-pass gathers end with the frame one end-of-render ctl_image_reduce gives, bit for bit (same ncclReduce over the same inputs). */
int ctl_image_reduce_to(ctl_image* src, ctl_image* dst, ctl_comm* comm, int32_t root);
/* The gather of BASELINE's north_star.  Every rank packs the tiles it owns into ceil(tiles / world) slots of 65 x 65 x 28 B: [slot k = tile k * world + rank][row-major
 * pixel][7 floats]; rows / columns 0..63 are the tile, row 64 / column 64 its HALO — the frame's pixels just right of and below the tile where they belong to another rank
 * (a sample's film position pixel + jitter rounds into the next pixel once in ~10^4 samples, as Image::AddSample's floor does in the reference, and at a tile edge that
 * pixel is another rank's: the rank accumulated it in its own full-size frame).  The clipped part of a border tile and a missing last slot are zero.  7.6 MB per rank at
 * 1920x1080 / 8 against the reduce's 58 MB.  ONE ncclGather moves the slots to the root; a streaming kernel there copies every tile into the frame, a second one adds the
 * halos.  Result: weights equal to the reduce's / the one-rank frame's exactly, colours to float rounding in the ~10^-5 of pixels that received a halo sample (bit-equal
 * elsewhere).  _to writes all of `dst` (root only; NULL elsewhere), leaves every rank's `src` alone and can be repeated — the per-pass progressive exchange; the in-place
 * form is ONE call per render like ctl_image_reduce (refused on every rank on a repeat).  Same deadline as the reduce: after the communicator's time-out the communicator
 * is aborted (ncclCommAbort), the call fails with CTL_ERR_INVALID and every later call on that communicator is refused. */
int ctl_image_gather(ctl_image* img, ctl_comm* comm, int32_t root);
int ctl_image_gather_to(ctl_image* src, ctl_image* dst, ctl_comm* comm, int32_t root);
/* The same packed slots for a host that moves them itself (MPI_Gather, a socket; bench.py's gloo fallback): bytes of one rank's buffer; D2H of `rank`'s slots of img;
 * H2D of ALL ranks' buffers, rank-major (MPI_Gather's receive buffer), into img on the root: every tile is copied, then every halo added. */
int ctl_image_packed_tile_bytes(uint32_t width, uint32_t height, uint32_t world, uint64_t* out_bytes);
int ctl_image_pack_tiles(ctl_image* img, uint32_t rank, uint32_t world, void* host_out);
int ctl_image_unpack_tiles(ctl_image* img, uint32_t world, const void* host_in_all_ranks);

/* ------------------------------------------------------------------- tracer */
typedef struct ctl_tracer ctl_tracer;
/* plugin names: "WavefrontPathTracer" / "PT_Wave" (Integrators/PseudoRealtime/WavefrontPathTracer.h:24), "PathTracer" / "PT" (Integrators/PathTracer.h:7),
 * "PrimTracer" / "direct" (Integrators/PrimTracer.h:10: non-progressive, one sample per pixel, parameters DrawingMode (enum, 15 names) and MaxPathLength). */
int ctl_tracer_create(const char* plugin, ctl_tracer** out);
void ctl_tracer_destroy(ctl_tracer* t);
/* TracerParameterCollection (Kernel/TracerSettings.h:221-350): keys Direct(bool), MaxPathLength(int>=1),
 * RRStartDepth(int>=1) (WavefrontPathTracer.h:29-39). Out-of-interval values -> CTL_ERR_INVALID.
 * Build-specific, WavefrontPathTracer: ParticipatingMedia(bool, default 0) — 1: the plugin renders scenes with participating media (PathTrace's rules; refused together
 * with PathSemantics = Wavefront); 0: it answers CTL_ERR_UNSUPPORTED for such a scene, at ctl_tracer_initialize_scene and when a pass starts.
 * TextureFiltering(bool, default 0) — 1: the first hit of every path is shaded with ray differentials and its image textures are filtered through the mip pyramid
 * (trilinear / EWA, the image's filter mode), as the PathTracer plugin does; deeper vertices read level 0.  0: every lookup reads level 0.  Refused with
 * CTL_ERR_UNSUPPORTED, at the same two places, together with PathSemantics = Wavefront and together with ParticipatingMedia = 1 (the PathTracer plugin renders both).
 * The PathTracer and PrimTracer plugins do not have the key. */
int ctl_tracer_set_param_bool(ctl_tracer* t, const char* key, int value);
int ctl_tracer_set_param_int(ctl_tracer* t, const char* key, int value);
int ctl_tracer_get_param_int(ctl_tracer* t, const char* key, int* value_out);   /* bool, int and enum (its index) parameters */
/* float intervals and enumerations (TracerParameter<float>, TracerParameter<enum> with its string table, Kernel/TracerSettings.h:14-195):
 * an enum is set by the NAME of the value ("Uniform", "Variance", ...) or, through ctl_tracer_set_param_int, by its index */
int ctl_tracer_set_param_float(ctl_tracer* t, const char* key, float value);
int ctl_tracer_get_param_float(ctl_tracer* t, const char* key, float* value_out);
int ctl_tracer_set_param_enum(ctl_tracer* t, const char* key, const char* value_name);
int ctl_tracer_resize(ctl_tracer* t, uint32_t width, uint32_t height);       /* Tracer::Resize (Tracer.h:196-208)          */
int ctl_tracer_initialize_scene(ctl_tracer* t, ctl_scene* s);                /* TracerBase::InitializeScene (Tracer.h:102) */
/* image-tile sharding for multi-GPU: this tracer renders the 64x64 tiles t with t % world == rank. */
int ctl_tracer_set_tile_shard(ctl_tracer* t, uint32_t rank, uint32_t world);
/* Use caller-provided sampler tables for the next pass instead of the tracer's own generator (tests). */
int ctl_tracer_set_sampler_tables(ctl_tracer* t, const float* tables_1d, const float* tables_2d);
/* Tracer<true>::DoPass (Tracer.h:209-248). */
int ctl_tracer_do_pass(ctl_tracer* t, ctl_image* img, int new_trace);
/* n passes back-to-back without host synchronisation in between (throughput mode). */
int ctl_tracer_do_passes(ctl_tracer* t, ctl_image* img, int new_trace, uint32_t n_passes);
/* TracerBase::Debug(Image*, Vec2i) (Kernel/Tracer.h:119-123): UpdateKernel(scene, generator) draws the NEXT set of sampling tables from the tracer's stream —
 * the pass that follows uses the set after it — then DebugInternal follows ONE path for the pixel: PathTracer::DebugInternal (Integrators/PathTracer.cu:172-180)
 * = PathTrace<true> from the pixel's own position (no jitter) with that set; the WavefrontPathTracer has no DebugInternal of its own (nothing is traced).
 * rgb_out (3 floats, may be NULL) receives the path's radiance, which the reference computes and drops (it is looked at in a debugger). */
int ctl_tracer_debug_pixel(ctl_tracer* t, ctl_image* img, uint32_t x, uint32_t y, float* rgb_out);
/* IDepthTracer::setDepthBuffer(DeviceDepthImage{m_pData, w, h}) (Kernel/Tracer.h:16-57; WavefrontPathTracer : IDepthTracer): device_depth = width*height floats in
 * DEVICE memory (ctl_device_malloc); every pass stores DeviceDepthImage::NormalizeDepthD3D of the primary hit distance of pixel (x, y) — clamped to the camera's
 * [near, far], 1 for a miss — as pathIterateKernel does at pathDepth 0 (WavefrontPathTracer.cu:76-77).  NULL, 0, 0 removes it.  Wavefront and PrimTracer plugins. */
int ctl_tracer_set_depth_buffer(ctl_tracer* t, float* device_depth, uint32_t width, uint32_t height);
/* traversal statistics for the roofline: sums over rays of inner-node visits, triangle tests and instance entries
 * (B_ray = 32 + 16 + 64*N_inner + 52*N_tri + 108*N_inst). */
typedef struct { uint64_t n_inner, n_tri, n_inst;
                 uint64_t wave_inner_iters, wave_tri_iters;   /* wave-level loop iterations: n_inner / (64 * wave_inner_iters) = lane utilisation */
} ctl_traversal_counts;
typedef struct {
    uint64_t rays_last_pass;       /* getRaysInLastPass (64-bit; the reference wraps at 2^32)            */
    uint64_t rays_total;           /* getAccRays                                                         */
    double seconds_last_pass;      /* getLastTimeSpentRenderingSec                                       */
    double seconds_total;          /* getAccTimeSpentRenderingSec                                        */
    uint32_t passes_done;          /* getNumPassesDone                                                   */
    /* per-kernel HIP-event timing of the last do_pass/do_passes call, milliseconds (events on the tracer's stream) */
    double ms_intersect;           /* closest-hit intersect kernel (path rays)                           */
    double ms_shade, ms_raygen;
    double ms_intersect_any;       /* any-hit intersect kernel (NEE shadow rays)                         */
    uint64_t intersect_rays;       /* path rays through the closest-hit kernel in that call              */
    uint64_t intersect_launches;
    uint64_t shadow_rays;          /* shadow rays through the any-hit kernel in that call                */
    uint64_t shadow_launches;
    /* traversal statistics, filled only while ctl_tracer_set_counting(t, 1): sums over all rays of the call */
    ctl_traversal_counts closest_counts, any_counts;
    /* FuseTraversal (default): the path rays of bounce d >= 2 and the shadow rays of bounce d - 1 are traced by ONE persistent launch (k_intersect_pair).
     * Those launches, the rays they carried and their time are reported here; ms_intersect / intersect_launches and ms_intersect_any / shadow_launches
     * then cover only the launches that stayed separate (the first bounce's path rays, the last bounce's shadow rays).  intersect_rays and shadow_rays
     * remain the totals of the call. */
    uint64_t fused_launches, fused_shadow_rays, fused_closest_rays;
    double ms_fused;
} ctl_tracer_stats;
int ctl_tracer_get_stats(ctl_tracer* t, ctl_tracer_stats* out);
/* Block samplers of Tracer<true> (Kernel/BlockSampler/, Kernel/Tracer.h:209-248; wavefront plugin only).  The int parameter
 * "BlockSamplerType" selects Uniform (0, default), Variance (1), Difference (2) or Select (3); "FractionDeterministic" (2) and
 * "FractionWeighted" (4) are the mixed-sampling settings of the Variance / Difference samplers.  Blocks are 64 x 64 pixels, indexed
 * (block_x, block_y); ctl_tracer_set_block_weight = IUserPreferenceSampler::setWeight (call after ctl_tracer_resize).
 * ctl_tracer_get_block_counts returns the samples per block (row-major, blocks_x = ceil(width / 64)) of the last rendered pass, all ones
 * while the sampler takes every block once. */
/* Build-specific: allocate the ray queues now for a ctl_tracer_do_passes(n) to come; without it they grow inside that call. */
int ctl_tracer_reserve_passes(ctl_tracer* t, uint32_t n_passes);
int ctl_tracer_set_block_weight(ctl_tracer* t, uint32_t block_x, uint32_t block_y, float weight);
int ctl_tracer_get_block_counts(ctl_tracer* t, uint8_t* counts_out, uint32_t n_blocks);
/* The PixelVarianceBuffer of Tracer<true> (Kernel/Tracer.h:233-237, Kernel/PixelVarianceBuffer.h): per-pixel moments of the pass estimates' luminance, what the
 * NonLocalMeans filter is guided by.  Off by default: with it on, a progressive tracer updates the buffer after every pass (the adaptive block samplers do that on
 * their own) — the wavefront tracer inside its batches, a tracer without the ordered accumulation's stage by rendering one pass per launch; a new trace clears it.
 * Frame and variance are those of the passes rendered one at a time, bit for bit.  Against the frame with the switch off: bit-equal, except that a pixel into which a
 * sample of the neighbouring pixel strayed (its position rounded up: ~1 in 10^4 samples at 1080p) may differ by a rounding — there a batch with the switch off adds the strays
 * of all its passes first.  CTL_ERR_UNSUPPORTED on a Tracer<false> (PrimTracer),
 * CTL_ERR_INVALID on a tile shard (world > 1).  ctl_tracer_read_pixel_variance: computeVariance() per pixel, width * height floats, NaN before the first pass. */
int ctl_tracer_set_pixel_variance(ctl_tracer* t, int on);
int ctl_tracer_read_pixel_variance(ctl_tracer* t, float* host_out);
/* applyImagePipeline with the other ImageSamplesFilter, NonLocalMeansFilter (Kernel/ImagePipeline/Filter/NonLocalMeansFilter.{h,cu}): variance-guided non-local means,
 * search window 13 x 13 (R = 6), patches 7 x 7 (F = 3), from the RGBE frame into the filtered RGBE plane; then `process` (may be NULL) as above.
 * nlm      = the reference's settings k (default 0.45) and sigma2Scale (default 0.005); both >= 0.  The weights are computed on every call (the reference reuses them
 *            for UpdateWeightPeriodicity passes; that setting is not offered) and there is no feature buffer (the reference fills one and never reads it).
 * variance = PixelVarianceInfo::computeVariance() per pixel, from exactly ONE of: `tracer` (its PixelVarianceBuffer, device to device; needs
 *            ctl_tracer_set_pixel_variance(tracer, 1) and the image's size) or `host_variance` (width * height floats).
 * Argument values are checked before the device (both or neither variance source, a negative or NaN setting, a null pointer -> CTL_ERR_INVALID), then
 * CTL_ERR_NO_DEVICE, then what needs the handles (size mismatch, variance switch off -> CTL_ERR_INVALID). */
typedef struct { float k, sigma2_scale; } ctl_nlm_filter;
int ctl_image_apply_pipeline_nlm(ctl_image* img, float splat_scale, const ctl_nlm_filter* nlm, ctl_tracer* tracer, const float* host_variance, const ctl_tonemap* process,
                                 uint32_t* host_rgbcol_out);
/* Image::getFilteredData: the RGBE plane (r | g << 8 | b << 16 | e << 24 per pixel) that the last pipeline call with a filter or a post-process left. */
int ctl_image_read_filtered(ctl_image* img, uint32_t* host_rgbe_out);
/* Image::ComputeLuminanceInfo, read-only: out4 = (min, max, avg, logAvg) of the filtered plane's luminance as the last pipeline call with a post-process computed
 * and used them (stored then, not recomputed here).  CTL_ERR_INVALID before the first such call. */
int ctl_image_luminance_info(ctl_image* img, float* out4);
/* Measurement: HIP-event time in ms of the NonLocalMeans kernel of the last ctl_image_apply_pipeline_nlm on this image (0 before the first). */
int ctl_image_last_filter_ms(ctl_image* img, float* ms_out);
/* run the intersect kernels in counting mode (N_inner / N_tri / N_inst of SURVEY §8d); slower, for measurement only */
int ctl_tracer_set_counting(ctl_tracer* t, int on);

/* ---------------------------------------------------- intersect (row a7 alone) */
/* __internal__IntersectBuffers (Kernel/TraceHelper.cu:736-746): n rays -> n hits; host pointers.
 * any_hit = 1 selects intersectKernel<true>. */
int ctl_intersect(ctl_scene* s, const ctl_ray* rays, uint32_t n, ctl_hit* hits, int any_hit);
/* TracerBase::TraceSingleRay(Ray, DynamicScene*) (Kernel/Tracer.cu:74-78): the closest hit of one ray (tmin = the scene's ray epsilon as the caller sets it in `ray`).
 * It is ctl_intersect with n = 1, i.e. it runs the WAVEFRONT kernel; the single-ray traversal the PathTracer and PrimTracer plugins run inside their kernels
 * (csrc/single_ray.h) is reached with ctl_intersect_ex and CTL_ISECT_SINGLE. */
int ctl_trace_single_ray(ctl_scene* s, const ctl_ray* ray, ctl_hit* hit_out);
/* TEST INFRASTRUCTURE: every traversal kernel variant on a list of rays, so that the tests hold each to the oracle ray by ray (tests/test_gpu_traversal_variants.py).
 * ctl_intersect_ex is ctl_intersect with a choice of variant:
 *   CTL_ISECT_ANY_HIT  as any_hit of ctl_intersect
 *   CTL_ISECT_ALPHA    the kernels that run Material::AlphaTest on candidate hits, under the tracers' rule: only when the scene has alpha maps
 *   CTL_ISECT_SINGLE   the single-ray traversal (csrc/single_ray.h trace_single, what the PathTracer and PrimTracer plugins call per lane) from a probe kernel with one lane
 *                      per ray.  It alpha-tests whenever the scene has alpha maps, with or without CTL_ISECT_ALPHA, and needs a scene created with CTL_SCENE_FLATTEN
 *                      (CTL_ERR_UNSUPPORTED otherwise, as the PathTracer answers).
 * ctl_intersect_pair is the tracer's fused launch (FuseTraversal): closest hits of `rays` into `hits`, then occlusion (1 / 0) of `shadow_rays` into `occ_out`, in ONE
 * persistent launch with a ray cursor per queue.  flags: CTL_ISECT_ALPHA or 0.  n == 0 or sn == 0 is legal and still launches while the other is not.
 * Both fill their device outputs before the launch with values no kernel writes (triangle -2, node -2, occlusion 0xffffffff): a ray that was never traced shows in the
 * result.  Unknown flag bits and null pointers with a non-zero count are refused (CTL_ERR_INVALID) before anything is launched. */
enum { CTL_ISECT_ANY_HIT = 1, CTL_ISECT_ALPHA = 2, CTL_ISECT_SINGLE = 4 };
int ctl_intersect_ex(ctl_scene* s, const ctl_ray* rays, uint32_t n, ctl_hit* hits, uint32_t flags);
int ctl_intersect_pair(ctl_scene* s, const ctl_ray* rays, uint32_t n, ctl_hit* hits, const ctl_ray* shadow_rays, uint32_t sn, uint32_t* occ_out, uint32_t flags);
/* device-pointer variant (the layout the tracer itself uses): d_ray_o[n], d_ray_d[n] = float4 (origin,tmin) / (direction,tmax);
 * d_hit4[n] = float4 (t, u, v, triangle index bits, -1 = miss); d_hit_node[n] = int32.  Synchronous; ms_out (may be NULL) =
 * HIP-event time of the kernel launch. */
int ctl_intersect_device(ctl_scene* s, const void* d_ray_o, const void* d_ray_d, uint32_t n, void* d_hit4, void* d_hit_node, int any_hit, float* ms_out);
/* traversal statistics for the roofline: sums over the n rays of inner-node visits, triangle tests and
 * instance entries (B_ray = 32 + 16 + 64*N_inner + 52*N_tri + 108*N_inst). */
int ctl_intersect_count(ctl_scene* s, const ctl_ray* rays, uint32_t n, int any_hit, ctl_traversal_counts* out);

/* Measurement: rays of all COUNTING traversals so far (ctl_intersect_count, ctl_tracer_set_counting) over the flattened BVH, by the deepest traversal-stack entry they
 * used; bin n_bins - 1 collects everything deeper.  The kernels keep the first entries of a lane in LDS and deeper ones in scratch (csrc/traverse_flat.h): the
 * histogram says how often that happens.  reset != 0 clears it.
 * ctl_traversal_lds_rows: how many entries that is, out5 = two-level kernel, Q4, Q8 (sibling groups), single-ray Q4, single-ray Q8 (groups); host only. */
int ctl_traversal_stack_histogram(uint64_t* out, uint32_t n_bins, int reset);
int ctl_traversal_lds_rows(uint32_t out5[5]);

/* The shared fp32 transcendental functions of the shading code (cudatracerlib_amd/csrc/ctl_fmath.h; the oracle's -DORC_SHARED_MATH build runs the same source):
 * which = 0 sin, 1 cos, 2 tan, 3 acos, 4 atan, 5 atan2(x, y), 6 exp, 7 log, 8 log2, 9 pow(x, y); on_device = 0 evaluates on the host, 1 in a kernel — the two are
 * bit-identical (tests/test_fmath.py).  No reference counterpart: the reference calls the CUDA / C library's functions. */
int ctl_shared_math_eval(int32_t which, uint32_t n, const float* x, const float* y, float* out, int32_t on_device);

/* TEST INFRASTRUCTURE: the device BSDF, emitter and texture functions (csrc/shading.h) evaluated one call per query, so that the tests hold them to the oracle call by
 * call (tests/test_gpu_shading_eval.py).  One lane per query fills the record as the oracle's call of the same name does — an identity frame at the origin, uv from
 * the query — calls the function the shade kernels call and stores the result row.  No reference counterpart.
 *   scene      supplies images, mip pyramids, the EWA weights, the rough-transmittance tables, emitters, the emitter CDF, shape sets and eps
 *   build      CTL_EVAL_BUILD_*: the feature set the functions are compiled under, mirroring a product build
 *   what       CTL_EVAL_*: the function; a query row / result row holds the floats listed below, an [index] travels as the BITS of its float
 *   materials  NULL, or an array that replaces the scene's materials for this call (nested indices of coating / blend refer to it)
 * Everything a query names is checked on the host before anything is launched: a material, nested material, image or light index out of range, a rough BSDF whose
 * transmittance table the scene does not carry, an unknown `what` / `build` -> CTL_ERR_INVALID; a model, texture or emitter kind the chosen build does not carry ->
 * CTL_ERR_UNSUPPORTED.  CTL_ERR_NO_DEVICE without a device (checked first). */
enum { CTL_EVAL_BUILD_BASIC = 0,      /* shade_basic.hip: the basic feature set (diffuse, dielectric, conductor, rough conductor; constant / checker textures; point and plain area lights) */
       CTL_EVAL_BUILD_FULL = 1,       /* shade_full / shade_class_*: every model, texture and emitter kind, transcendental functions out of line, scene tables in LDS */
       CTL_EVAL_BUILD_PARTIALS = 2 }; /* megakernel.hip / prim_tracer.hip: the full set with uv partials (CTL_TEX_PARTIALS), scene tables in global memory */
enum { CTL_EVAL_BSDF_SAMPLE = 0,      /* [material] wi(3) sample(2) uv(2)          -> f(3) pdf wo(3) sampledType eta                       (bsdf_sample_top)                    */
       CTL_EVAL_BSDF_EVAL = 1,        /* [material] wi(3) wo(3) [typeMask] uv(2)   -> f(3) pdf, solid-angle measure                        (bsdf_f_top, bsdf_pdf_top)           */
       CTL_EVAL_BSDF_SAMPLE_EVAL = 2, /* [material] wi(3) sample(2) uv(2) wo2(3)   -> the sample's row, then f(3) pdf for wo2 under EAll & ~EDelta ON THE SAME RECORD (next-event estimation as the shade kernels do it) */
       CTL_EVAL_LIGHT_SAMPLE = 3,     /* [light] ref(3) refN(3) sample(2)          -> value(3) pdf d(3) dist p(3) n(3) measure             (light_sample_direct)                */
       CTL_EVAL_EMITTER_SAMPLE = 4,   /* ref(3) refN(3) sample(2)                  -> sampleEmitterDirect: value(3) pdf d(3) dist p(3) n(3) slot, emitter pdf, re-scaled sample.x; sample_emitter's slot, pdf */
       CTL_EVAL_LIGHT_PDF = 5,        /* [light] ref(3) refN(3) d(3) dist n(3)     -> pdfDirect, solid-angle measure                       (light_pdf_direct / env_pdf_direct)  */
       CTL_EVAL_LIGHT_EVAL = 6,       /* [light] p(3) n(3) d(3)                    -> radiance(3)                                          (light_eval)                         */
       CTL_EVAL_ENV_EVAL = 7,         /* dir(3)                                    -> radiance(3) of the scene's environment emitter       (env_eval)                           */
       CTL_EVAL_TEXTURE = 8,          /* [slot] [index] uv(2)                      -> rgb(3), unfiltered; slot 0..3 = tex[slot] of material `index`, 4 its map_tex, 5 its alpha_tex, 6 = rad_texture of light `index` (tex_eval) */
       CTL_EVAL_MIP = 9,              /* [image] uv(2) d0(2) d1(2)                 -> rgb(3), KernelMIPMap::eval; CTL_EVAL_BUILD_PARTIALS only (mip_eval)                       */
       CTL_EVAL_NORMAL_MAP = 10,     /* [material] uv(2) frame s,t,n(9) n_geo,dpdu,dpdv(9) -> the perturbed frame s,t,n(9)                (sample_normal_map)                  */
       CTL_EVAL_ALPHA_TEST = 11 };    /* [material] uv(2), each representable in half precision -> 1 / 0: Material::AlphaTest as the traversal asks it (alpha_survives), through one synthetic triangle per query whose vertices carry the uv; every build */
int ctl_shading_eval(const ctl_scene* scene, int32_t build, int32_t what, const ctl_material* materials, uint32_t n_materials,
                     uint32_t n, const float* queries, uint32_t query_stride, float* out, uint32_t out_stride);

/* TEST INFRASTRUCTURE: the participating-media functions (csrc/volume.h) one call per query, after ctl_shading_eval and ctl_shared_math_eval.  `desc` supplies volumes /
 * n_volumes and volume_grids / n_volume_grids (nothing else of it is read; the derived fields must be current: ctl_volume_update, or a description from the builder).  on_device = 0 runs the functions
 * on the host and needs no GPU — the yardstick; 1 runs one small kernel, one lane per query (CTL_ERR_NO_DEVICE without a device).  The two are bit-identical.
 * A query row is CTL_VEVAL_QUERY_FLOATS floats, a result row CTL_VEVAL_RESULT_FLOATS floats, unused ones 0; a [volume] index travels as the BITS of its float and is
 * checked against n_volumes before anything runs (CTL_ERR_INVALID, as for a description the validator refuses or an unknown `what`).  No reference counterpart. */
#define CTL_VEVAL_QUERY_FLOATS 10
#define CTL_VEVAL_RESULT_FLOATS 17
enum { CTL_VEVAL_REGION_INTERSECT = 0,        /* [volume] o(3) d(3) minT maxT        -> hit t0 t1 (0 0 on a miss)                          (BaseVolumeRegion::IntersectP)            */
       CTL_VEVAL_INTERSECT = 1,               /* o(3) d(3) minT maxT                 -> hit t0 t1 (FLT_MAX, -FLT_MAX on a miss)            (KernelAggregateVolume::IntersectP)       */
       CTL_VEVAL_REGION_TAU = 2,              /* [volume] o(3) d(3) minT maxT        -> tau(3)                                             (HomogeneousVolumeDensity::tau)           */
       CTL_VEVAL_TAU = 3,                     /* o(3) d(3) minT maxT                 -> tau(3)                                             (KernelAggregateVolume::tau)              */
       CTL_VEVAL_REGION_SAMPLE_DISTANCE = 4,  /* [volume] o(3) d(3) minT maxT sample -> success t p(3) transmittance(3) sigmaA(3) sigmaS(3) pdfSuccess pdfSuccessRev pdfFailure, into a
                                                 record of zeros                                                                           (HomogeneousVolumeDensity::sampleDistance) */
       CTL_VEVAL_SAMPLE_DISTANCE = 5,         /* o(3) d(3) minT maxT sample          -> the same row                                       (KernelAggregateVolume::sampleDistance)   */
       CTL_VEVAL_SAMPLE_VOLUME = 6,           /* o(3) d(3) minT maxT sample          -> region index (-1: none), the sample after sampleReuse, pdf (sampleVolume, with ffsn)         */
       CTL_VEVAL_PHASE_EVAL = 7,              /* [volume] wi(3) wo(3)                -> value, of the region's phase function              (PhaseFunction::Evaluate)                 */
       CTL_VEVAL_PHASE_SAMPLE = 8,            /* [volume] wi(3) sample(2)            -> weight pdf wo(3)                                   (PhaseFunction::Sample(pRec, pdf, sample)) */
       CTL_VEVAL_P = 9,                       /* p(3) wi(3) wo(3)                    -> value                                              (KernelAggregateVolume::p)                */
       CTL_VEVAL_SAMPLE = 10,                 /* p(3) wi(3) sample(2)                -> weight pdf wo(3), pdf and wo 0 where no region is found (KernelAggregateVolume::Sample)      */
       CTL_VEVAL_TRANSMITTANCE = 11,          /* o(3) d(3) tmin tmax                 -> T(3)                                               (Transmittance, TraceAlgorithms.cu:22-31) */
       CTL_VEVAL_EVAL_TRANSMITTANCE = 12,     /* p1(3) p2(3)                         -> T(3)                                               (KernelDynamicScene::evalTransmittance)   */
       /* the codes above dispatch on the region's type; the ones below need a CTL_VOLUME_GRID region (CTL_ERR_INVALID otherwise) */
       CTL_VEVAL_GRID_VALUE = 13,             /* [volume] which(bits: 0 grid / gridA, 1 gridS) p(3) in voxel space -> value                (DenseVolGrid::sampleTrilinear)           */
       CTL_VEVAL_REGION_SIGMA = 14,           /* [volume] p(3)                       -> sigma_a(3) sigma_s(3) sigma_t(3)                   (VolumeGrid::sigma_a / sigma_s / sigma_t) */
       CTL_VEVAL_GRID_MARCH = 15 };           /* [volume] o(3) d(3) minT maxT        -> march steps, 1 if the step cap was reached         (VolumeGrid::tau's TraverseGridRay)       */
int ctl_volume_eval(const ctl_scene_desc* desc, int32_t what, const float* queries, uint32_t n, float* out, int32_t on_device);

/* device memory helpers so that Python callers need no HIP binding */
int ctl_device_malloc(size_t bytes, void** out);
int ctl_device_free(void* p);
int ctl_memcpy_h2d(void* dst, const void* src, size_t bytes);
int ctl_memcpy_d2h(void* dst, const void* src, size_t bytes);
int ctl_memcpy_d2d(void* dst, const void* src, size_t bytes);
int ctl_device_synchronize(void);
int ctl_set_device(int ordinal);

#ifdef __cplusplus
}
#endif
#endif /* CTL_AMD_H */
