// scene_builder.h — host scene assembly (see scene_builder.cpp).
#pragma once
#include "../../include/ctl_amd.h"
#include "bvh_builder.h"
#include "ctl_math.h"
#include <vector>

namespace ctl {

void mat_inverse(const float* m16, float* out16);   // float4x4::inverse (Math/float4x4.h:132-193)
void mat_mul(const float* l16, const float* r16, float* out16);
void woop_set_data(ctl_woop_tri& w, f3 a, f3 b, f3 c);
// Mesh::ComputeVertexNormals (Engine/Mesh.cpp:151-190); I == nullptr: a triangle soup.  Also what ctl_scene_bind_skin makes of a rest pose without normals
void compute_vertex_normals(const float* V, const uint32_t* I, uint32_t nv, uint32_t nt, std::vector<f3>& N, bool flip = false);
void woop_get_data(const ctl_woop_tri& w, f3& v0, f3& v1, f3& v2);

struct mesh_rec { uint32_t tri_offset, n_tris, node_offset, n_nodes, woop_offset, n_woop, mat_offset, n_mat; aabb box; int max_depth; };

struct scene_builder {
    std::vector<ctl_triangle_data> tri;
    std::vector<ctl_woop_tri> woop;
    std::vector<ctl_woop_index> widx;
    std::vector<ctl_bvh_node> bvh, scene_bvh;
    std::vector<ctl_kernel_mesh> meshes;
    std::vector<mesh_rec> mesh_info;
    std::vector<ctl_material> mesh_materials;   // per-mesh standard materials (Mesh::m_sMatInfo)
    std::vector<ctl_material> mats;             // per-node copies (m_sMatData)
    std::vector<ctl_node> nodes;
    std::vector<ctl_float4x4> xf, ixf;
    std::vector<ctl_light> lights;
    std::vector<uint8_t> anim;
    std::vector<std::vector<uint32_t>> image_texels;   // level-0 texels of every registered KernelMIPMap
    std::vector<ctl_mipmap> images;
    uint32_t env_light = 0xffffffffu;
    std::vector<float> rt_trans[3], rt_diff[3];        // RoughTransmittanceManager's three tables
    ctl_rough_transmittance rt[3] = {};
    bool have_rt = false;
    ctl_sensor camera{};
    bool have_camera = false;
    std::vector<ctl_volume> volumes;                   // DynamicScene::m_pVolumes

    // mesh BVH builder: CTL_BVH_SBVH = the reference's SplitBVHBuilder restated (sbvh_builder.cpp, identical arrays), CTL_BVH_BINNED = binned
    // SAH without spatial splits (bvh_builder.cpp, threaded), CTL_BVH_AUTO = SBVH up to kSbvhAutoLimit = 65536 triangles (its sweep sorts the
    // references three times per node: the reference quotes minutes for San Miguel), binned above.  Default from $CTL_BVH_MODE.
    static constexpr uint32_t kSbvhAutoLimit = 1u << 16;
    uint32_t bvh_mode = default_bvh_mode();
    static uint32_t default_bvh_mode();
    uint32_t finish_mesh(const mesh_rec& mr);   // registers a compiled (or cache-loaded) mesh, returns its index
    uint32_t add_mesh(const float* positions, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri, const float* normals, const float* uvs,
                      const uint8_t* tri_material, const ctl_material* materials, uint32_t n_mat,
                      bool flip_normals = false, bool face_normals = false, float max_smooth_angle = 0.0f);   // Mesh::CompileMesh options (Mesh.cpp:199)
    // new vertex arrays for a mesh, same triangle count (ctl_builder_update_mesh): TriangleData, Woop rows, the mesh BVH's boxes, the mesh box, the area lights of its nodes
    void update_mesh(uint32_t mesh_index, const float* positions, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri, const float* normals, const float* uvs);
    void recalculate_node_lights(uint32_t node_index);   // ShapeSet::Recalculate of every area light of a node
    uint32_t add_node(uint32_t mesh_index, const ctl_float4x4* to_world);
    void set_node_transform(uint32_t node_index, const ctl_float4x4& to_world, bool recalculate_lights = false);
    float recalculate_shape_set(uint32_t node_index, uint32_t cdf_off, uint32_t tri_off, uint32_t count);   // ShapeSet::Recalculate of one area light in the anim blob
    void set_node_bsdf(uint32_t node_index, uint32_t local_material, const ctl_material& m);
    uint32_t add_aux_material(const ctl_material& m);   // a material no triangle refers to: the nested BSDF of a coating / roughcoating / blend; returns its absolute index
    const ctl_material& node_material(uint32_t node_index, uint32_t local_material) const;
    aabb scene_box() const;
    uint32_t add_area_light(uint32_t node_index, uint32_t local_material, const float radiance[3], const ctl_texture* rad_texture = nullptr, bool orthogonal = false);
    uint32_t add_point_light(const float position[3], const float intensity[3]);
    uint32_t add_spot_light(const float position[3], const float target[3], const float intensity[3], float cutoff_deg, float beam_deg);
    uint32_t add_distant_light(const float direction[3], const float irradiance[3], float scene_radius);
    uint32_t add_image(const uint32_t* texels, uint32_t w, uint32_t h, uint32_t texel_type, uint32_t wrap, uint32_t filter);
    uint32_t set_environment_map(uint32_t image, const float scale[3], const ctl_float4x4* to_world);
    // new level-0 texels for a registered image, same size (ctl_builder_update_image): the environment light's CDFs and normalization follow if the image is its map
    void update_image(uint32_t image, const uint32_t* texels, uint32_t w, uint32_t h);
    void environment_tables(ctl_light& L);   // cdfCols, cdfRows and normalization of an infinite light from its image's texels, at the light's offsets in the anim blob (env_tables.h)
    void set_rough_transmittance(uint32_t slot, const ctl_rough_transmittance& t);
    void load_rough_transmittance(uint32_t slot, const char* path);
    void set_camera_lookat(const float pos[3], const float target[3], const float up[3], float fov_degrees, uint32_t w, uint32_t h);
    void set_camera(const ctl_sensor& s);
    // DynamicScene::CreateVolume(VolumeRegion) (Engine/DynamicScene.cpp:787-792) / an edit of the region it returned; the derived fields are recomputed (ctl_volume_update)
    uint32_t create_volume(const ctl_volume& v);
    void set_volume(uint32_t index, const ctl_volume& v);
    // DynamicScene::CreateVolume(w, h, d, ...) / (wA, ..., dL, ...) (Engine/DynamicScene.cpp:794-812): a VolumeGrid with zeroed grids and coefficients (VolumeGrid's
    // constructors, Volumes.cu:99-111); n_dims = 3 or 9, the L dims are accepted and ignored.  The floats are the builder's own copies
    struct grid_store { ctl_volume_grid rec{}; std::vector<float> data[2]; };   // data[0]: grid / gridA, data[1]: gridS
    std::vector<grid_store> grid_stores; std::vector<ctl_volume_grid> grid_records;   // grid_records: what finalize hands out
    uint32_t create_volume_grid(const uint32_t* dims, uint32_t n_dims, const ctl_float4x4& volume_to_world, const ctl_phase_function& phase);
    void set_volume_grid_data(uint32_t index, uint32_t which, const float* data, uint32_t n);
    void set_volume_grid_coefficients(uint32_t index, const float* sig_a_min, const float* sig_a_max, const float* sig_s_min, const float* sig_s_max);
    // DynamicScene::DeleteNode (Engine/DynamicScene.cpp:380-384) for a node without lights (the loader's medium-only shapes): the nodes behind it move up one index, the
    // area lights of those nodes follow; the node's material copies stay in the array, unreferenced
    void remove_node(uint32_t node_index);
    // ctl_builder_remove_mesh: a mesh without nodes leaves tri, woop, widx, bvh, meshes and mesh_info; the later meshes' offsets, the mesh_index of their nodes and the
    // i_dat / t_dat of their area lights move down.  mesh_materials is not compacted.  Refused (nothing changed) for a bad index or a mesh a node still instances
    void remove_mesh(uint32_t mesh_index);
    // ctl_builder_remove_image: an image no material row and no light references leaves images / image_texels; every image index above it, in mats, mesh_materials and
    // lights, moves down.  ctl_builder_replace_image: level-0 texels of another size at the same index (not the environment map's).  Refused: nothing changed
    void remove_image(uint32_t image);
    void replace_image(uint32_t image, const uint32_t* texels, uint32_t w, uint32_t h);
    // one row of the material table by its absolute index (ctl_builder_get_material / _set_material): DynamicScene::getMaterials + Invalidate
    const ctl_material& material(uint32_t index) const;
    void set_material(uint32_t index, const ctl_material& m);
    void finalize(ctl_scene_desc& out);
};

} // namespace ctl
