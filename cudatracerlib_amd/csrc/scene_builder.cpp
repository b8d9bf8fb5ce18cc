// scene_builder.cpp — host scene assembly behind the ctl_builder_* C-ABI: the subset of the reference's
// DynamicScene that the Mitsuba loader drives (Engine/DynamicScene.h:70-187), emitting the reference's
// KernelDynamicScene arrays (Engine/KernelDynamicScene.h:28-109) as a ctl_scene_desc.
#include "scene_builder.h"
#include "scene_cache.h"
#include "material_textures.h"
#include <cstdio>
#include <cstdlib>
#include <string>
#include "ctl_math.h"
#include "mesh_skin.h"
#include "shape_set.h"
#include "env_tables.h"
#include "volume_eval.h"
#include "device_scene.h"   // the BSDF model classifiers
#include <cstring>
#include <algorithm>
#include <stdexcept>

namespace ctl {

// float4x4::inverse (Math/float4x4.h:132-193): the one restatement is mesh_skin.h's, which the device runs too
void mat_inverse(const float* Q, float* out) { float r[16]; mat4_inverse(Q, r); std::memcpy(out, r, sizeof(r)); }
void mat_mul(const float* l, const float* r, float* o) {   // float4x4.h:373-381
    float t[16];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) { float s = 0.0f; for (int k = 0; k < 4; k++) s += l[i * 4 + k] * r[k * 4 + j]; t[i * 4 + j] = s; }
    std::memcpy(o, t, sizeof(t));
}
static m34 as_m34(const float* m) { m34 r; std::memcpy(r.r, m, 48); return r; }

// Woop rows from the three vertices (Engine/TriIntersectorData.cu:5-18)
void woop_set_data(ctl_woop_tri& w, f3 a, f3 b, f3 c) {
    float r[12]; woop_rows_from_vertices(r, a, b, c);
    std::memcpy(w.a, r, 16); std::memcpy(w.b, r + 4, 16); std::memcpy(w.c, r + 8, 16);
}
// and back (Engine/TriIntersectorData.cu:20-32) — area lights take their vertices from this round trip (shape_set.h)
void woop_get_data(const ctl_woop_tri& w, f3& v0, f3& v1, f3& v2) { woop_get_data(w.a, w.b, w.c, v0, v1, v2); }

// TriangleData::setUvSetData + setData (Engine/TriangleData.cu:18-65)
static void tri_data_pack(ctl_triangle_data& T, const f3 p[3], const f3 n[3], const f2 t[3], uint32_t mat_index) {
    uint32_t uv[3], words[8];
    for (int i = 0; i < 3; i++) uv[i] = (uint32_t)float_to_half(t[i].x) | ((uint32_t)float_to_half(t[i].y) << 16);
    tri_data_words<false>(words, p, n, uv, mat_index);   // mesh_skin.h; the normal codec over libm, as these arrays always were
    static_assert(sizeof(ctl_triangle_data) == sizeof(words), "TriangleData is eight words");
    std::memcpy(&T, words, sizeof(words));
}

// Mesh::ComputeVertexNormals (Engine/Mesh.cpp:151-190), "sphere inscribed polytope" weights
static aabb box_transform(const aabb& b, const float* m);

void compute_vertex_normals(const float* V, const uint32_t* I, uint32_t nv, uint32_t nt, std::vector<f3>& N, bool flip) {
    N.assign(nv, f3(0.0f));
    auto vtx = [&](uint32_t i) { return f3(V[3 * i], V[3 * i + 1], V[3 * i + 2]); };
    const float flip_coeff = flip ? -1.0f : 1.0f;
    for (uint32_t f = 0; f < nt; f++) {
        uint32_t i1 = I ? I[f * 3] : f * 3, i2 = I ? I[f * 3 + 1] : f * 3 + 1, i3 = I ? I[f * 3 + 2] : f * 3 + 2;
        f3 v1 = vtx(i1), v2 = vtx(i2), v3 = vtx(i3);
        auto nor = [&](f3 pb, f3 n1, f3 n2) { return flip_coeff * cross(n1 - pb, n2 - pb) / (len_sqr(n1 - pb) * len_sqr(n2 - pb)); };
        N[i1] = N[i1] + nor(v1, v3, v2); N[i2] = N[i2] + nor(v2, v1, v3); N[i3] = N[i3] + nor(v3, v2, v1);
    }
    for (uint32_t a = 0; a < nv; a++) N[a] = normalize(N[a]);
}

// Mesh::CompileMesh (Engine/Mesh.cpp:216-272): the TriangleData of every triangle into out[0 .. n_tri), its box into boxes[] and the mesh's box.  One function for
// add_mesh and update_mesh: a mesh updated to new arrays holds the bytes a fresh add_mesh of those arrays compiles
static void compile_triangles(const float* positions, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri, const float* normals, const float* uvs, const uint8_t* tri_material, uint32_t n_mat,
                              bool flip_normals, bool face_normals, float max_smooth_angle, ctl_triangle_data* out, aabb* boxes, aabb& box) {
    std::vector<f3> comp;
    if (!normals || flip_normals) compute_vertex_normals(positions, indices, n_vert, n_tri, comp, flip_normals);   // Mesh.cpp:216-217
    auto vidx = [&](uint32_t ti, int j) { return indices ? indices[ti * 3 + j] : ti * 3 + j; };
    auto vtx = [&](uint32_t i) { return f3(positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]); };
    box.reset();
    for (uint32_t ti = 0; ti < n_tri; ti++) {   // Mesh::CompileMesh (Engine/Mesh.cpp:225-272)
        f3 p[3], n[3]; f2 t[3];
        boxes[ti].reset();
        for (int j = 0; j < 3; j++) {
            uint32_t l = vidx(ti, j);
            if (l >= n_vert) throw std::runtime_error("ctl_builder_add_mesh: vertex index out of range");
            p[j] = vtx(l);
            t[j] = uvs ? f2{ uvs[2 * l], uvs[2 * l + 1] } : f2{ 0.0f, 0.0f };
            n[j] = (normals && !flip_normals) ? normalize(f3(normals[3 * l], normals[3 * l + 1], normals[3 * l + 2])) : comp[l];
            float pp[3] = { p[j].x, p[j].y, p[j].z };
            boxes[ti].grow(pp); box.grow(pp);
        }
        if (face_normals || max_smooth_angle != 0) {   // Mesh.cpp:247-267
            f3 n_face = normalize(cross(p[0] - p[1], p[2] - p[1]));
            if (flip_normals) n_face = -n_face;
            bool use_face = face_normals;
            if (!face_normals) for (int j = 0; j < 3; j++) if (acosf(dot(n_face, n[j])) > max_smooth_angle) use_face = true;
            if (use_face) n[0] = n[1] = n[2] = n_face;
        }
        uint32_t mi = tri_material ? tri_material[ti] : 0;
        if (mi >= n_mat) throw std::runtime_error("ctl_builder_add_mesh: triangle material index out of range");
        tri_data_pack(out[ti], p, n, t, mi);
    }
}

uint32_t scene_builder::add_mesh(const float* positions, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri, const float* normals,
                                 const float* uvs, const uint8_t* tri_material, const ctl_material* materials, uint32_t n_mat,
                                 bool flip_normals, bool face_normals, float max_smooth_angle) {
    if (!positions || n_tri == 0 || n_mat == 0 || !materials) throw std::runtime_error("ctl_builder_add_mesh: empty mesh or no material");
    if (!indices && n_vert != n_tri * 3) throw std::runtime_error("ctl_builder_add_mesh: triangle soup needs n_vert == 3*n_tri");
    if (indices) for (size_t i = 0; i < (size_t)n_tri * 3; i++) if (indices[i] >= n_vert) throw std::runtime_error("ctl_builder_add_mesh: vertex index out of range");   // before anything dereferences them
    if (tri_material) for (uint32_t i = 0; i < n_tri; i++) if (tri_material[i] >= n_mat) throw std::runtime_error("ctl_builder_add_mesh: triangle material index out of range");
    mesh_rec mr{};
    mr.tri_offset = (uint32_t)tri.size(); mr.n_tris = n_tri;
    mr.mat_offset = (uint32_t)mesh_materials.size(); mr.n_mat = n_mat;
    mesh_materials.insert(mesh_materials.end(), materials, materials + n_mat);
    // compiled-mesh cache (scene_cache.h; the reference's .xmsh, Engine/Mesh.cpp:46-98): keyed by every input of the compile step
    const bool use_sbvh = bvh_mode == CTL_BVH_SBVH || (bvh_mode == CTL_BVH_AUTO && n_tri <= kSbvhAutoLimit);
    std::string key;
    if (!cache_dir().empty()) {
        content_hash H; const uint32_t version = 2, flags = (use_sbvh ? 64u : 0u) |(flip_normals ? 1u : 0u) | (face_normals ? 2u : 0u) | (indices ? 4u : 0u) | (normals ? 8u : 0u) | (uvs ? 16u : 0u) | (tri_material ? 32u : 0u);
        H.add_value(version); H.add_value(flags); H.add_value(n_vert); H.add_value(n_tri); H.add_value(n_mat); H.add_value(max_smooth_angle);
        H.add(positions, (size_t)n_vert * 12);
        if (indices) H.add(indices, (size_t)n_tri * 12);
        if (normals) H.add(normals, (size_t)n_vert * 12);
        if (uvs) H.add(uvs, (size_t)n_vert * 8);
        if (tri_material) H.add(tri_material, n_tri);
        key = H.hex();
        cache_reader rd("mesh", key);
        std::vector<ctl_triangle_data> c_tri; std::vector<ctl_bvh_node> c_nodes; std::vector<ctl_woop_tri> c_woop; std::vector<ctl_woop_index> c_widx; aabb c_box; int c_depth = 0;
        if (rd.found() && rd.vector(c_tri) && rd.vector(c_nodes) && rd.vector(c_woop) && rd.vector(c_widx) && rd.value(c_box) && rd.value(c_depth) && rd.verify() &&
            c_tri.size() == n_tri && c_woop.size() == c_widx.size() && c_woop.size() >= n_tri) {
            tri.insert(tri.end(), c_tri.begin(), c_tri.end());
            mr.box = c_box; mr.max_depth = c_depth;
            mr.node_offset = (uint32_t)bvh.size(); mr.n_nodes = (uint32_t)c_nodes.size(); bvh.insert(bvh.end(), c_nodes.begin(), c_nodes.end());
            mr.woop_offset = (uint32_t)woop.size(); mr.n_woop = (uint32_t)c_woop.size(); woop.insert(woop.end(), c_woop.begin(), c_woop.end()); widx.insert(widx.end(), c_widx.begin(), c_widx.end());
            return finish_mesh(mr);
        }
    }
    std::vector<aabb> boxes(n_tri);
    tri.resize(mr.tri_offset + n_tri);
    compile_triangles(positions, n_vert, indices, n_tri, normals, uvs, tri_material, n_mat, flip_normals, face_normals, max_smooth_angle, tri.data() + mr.tri_offset, boxes.data(), mr.box);
    auto vidx = [&](uint32_t ti, int j) { return indices ? indices[ti * 3 + j] : ti * 3 + j; };
    auto vtx = [&](uint32_t i) { return f3(positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]); };
    // ConstructBVH (Engine/MeshLoader/BVHBuilderHelper.cpp:116-147): max leaf size 8
    bvh_result R;
    if (use_sbvh) build_sbvh(positions, indices, n_tri, 8, R);   // the reference's own tree: SplitBVHBuilder with spatial splits
    else build_bvh(boxes, 8, true, 44, R);                        // binned SAH, object splits only, threaded: for meshes the sweep builder takes minutes on
    mr.node_offset = (uint32_t)bvh.size(); mr.n_nodes = (uint32_t)R.nodes.size();
    bvh.insert(bvh.end(), R.nodes.begin(), R.nodes.end());
    mr.woop_offset = (uint32_t)woop.size(); mr.n_woop = (uint32_t)R.leaf_prims.size();
    woop.resize(mr.woop_offset + mr.n_woop); widx.resize(mr.woop_offset + mr.n_woop);
    for (uint32_t i = 0; i < mr.n_woop; i++) {   // createLeafNode (BVHBuilderHelper.cpp:51-62)
        uint32_t t = R.leaf_prims[i];
        woop_set_data(woop[mr.woop_offset + i], vtx(vidx(t, 0)), vtx(vidx(t, 1)), vtx(vidx(t, 2)));
        widx[mr.woop_offset + i].index = (t << 1) | (R.leaf_last[i] ? 1u : 0u);
    }
    mr.max_depth = R.max_depth;
    if (!key.empty()) {
        cache_writer wr("mesh", key);
        if (wr.active()) {
            wr.section(tri.data() + mr.tri_offset, (size_t)n_tri * sizeof(ctl_triangle_data)); wr.vector(R.nodes);
            wr.section(woop.data() + mr.woop_offset, (size_t)mr.n_woop * sizeof(ctl_woop_tri)); wr.section(widx.data() + mr.woop_offset, (size_t)mr.n_woop * sizeof(ctl_woop_index));
            wr.value(mr.box); wr.value(mr.max_depth); wr.commit();
        }
    }
    return finish_mesh(mr);
}

uint32_t scene_builder::default_bvh_mode() {
    const char* e = std::getenv("CTL_BVH_MODE");
    if (!e) return CTL_BVH_AUTO;
    const std::string s(e);
    return s == "sbvh" ? CTL_BVH_SBVH : (s == "binned" ? CTL_BVH_BINNED : CTL_BVH_AUTO);
}

uint32_t scene_builder::finish_mesh(const mesh_rec& mr) {
    mesh_info.push_back(mr);
    ctl_kernel_mesh km;   // Mesh::getKernelData (Engine/Mesh.cpp:100-109)
    km.tri_offset = mr.tri_offset; km.bvh_node_offset = mr.node_offset * 4; km.bvh_tri_offset = mr.woop_offset * 3;
    km.bvh_index_offset = mr.woop_offset; km.std_material_offset = mr.mat_offset;
    meshes.push_back(km);
    return (uint32_t)meshes.size() - 1;
}

// DynamicScene::AnimateMesh (Engine/DynamicScene.cpp:450-456; AnimatedMesh::k_ComputeState, Engine/AnimatedMesh.cpp:163-184) for a host that supplies the vertex
// positions: the TriangleData and the Woop rows of the mesh from the new arrays, its BVH REFITTED (links, the leaves' references and their order stay; a spatial-split
// reference's clipped box gives way to the whole triangle's: the tree culls less well, never wrongly), its box, and the shape sets of the area lights on its nodes.
// Everything that can refuse the arrays runs before the first byte is written.  The geometry cache is neither read nor written.
void scene_builder::update_mesh(uint32_t mesh_index, const float* positions, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri, const float* normals, const float* uvs) {
    if (mesh_index >= mesh_info.size()) throw std::runtime_error("ctl_builder_update_mesh: bad mesh index");
    mesh_rec& mr = mesh_info[mesh_index];
    if (!positions || n_tri != mr.n_tris) throw std::runtime_error("ctl_builder_update_mesh: mesh " + std::to_string(mesh_index) + " has " + std::to_string(mr.n_tris) + " triangles; an update keeps the triangle count");
    if (!indices && n_vert != n_tri * 3) throw std::runtime_error("ctl_builder_update_mesh: triangle soup needs n_vert == 3*n_tri");
    if (indices) for (size_t i = 0; i < (size_t)n_tri * 3; i++) if (indices[i] >= n_vert) throw std::runtime_error("ctl_builder_update_mesh: vertex index out of range");
    for (uint32_t i = 0; i < mr.n_woop; i++) if ((widx[mr.woop_offset + i].index >> 1) >= n_tri) throw std::runtime_error("ctl_builder_update_mesh: the mesh's leaf references are out of range");
    std::vector<uint8_t> tri_material(n_tri);   // the materials stay those of the mesh as added (TriangleData::getMatIndex)
    for (uint32_t ti = 0; ti < n_tri; ti++) tri_material[ti] = (uint8_t)((tri[mr.tri_offset + ti].nor_mat_extra[1] >> 16) & 0xffu);
    std::vector<ctl_triangle_data> compiled(n_tri); std::vector<aabb> boxes(n_tri); aabb box;
    compile_triangles(positions, n_vert, indices, n_tri, normals, uvs, tri_material.data(), 256, false, false, 0.0f, compiled.data(), boxes.data(), box);
    std::copy(compiled.begin(), compiled.end(), tri.begin() + mr.tri_offset);
    mr.box = box;
    auto vidx = [&](uint32_t ti, int j) { return indices ? indices[ti * 3 + j] : ti * 3 + j; };
    auto vtx = [&](uint32_t i) { return f3(positions[3 * i], positions[3 * i + 1], positions[3 * i + 2]); };
    for (uint32_t i = 0; i < mr.n_woop; i++) {   // createLeafNode (BVHBuilderHelper.cpp:51-62)
        const uint32_t t = widx[mr.woop_offset + i].index >> 1;
        woop_set_data(woop[mr.woop_offset + i], vtx(vidx(t, 0)), vtx(vidx(t, 1)), vtx(vidx(t, 2)));
    }
    // the child boxes, bottom-up: the builders emit a node's children after the node, so the reverse index order visits them first
    ctl_bvh_node* N = bvh.data() + mr.node_offset;
    auto child_box = [&](int code, aabb& b) -> bool {   // false: no child, or a link this mesh does not hold (the box stays as built)
        if (code == 0x76543210) return false;
        b.reset();
        if (code >= 0) {
            const uint32_t k = (uint32_t)code / 4;
            if (k >= mr.n_nodes) return false;
            const ctl_bvh_node& c = N[k];
            if (c.child0 != 0x76543210) { const float lo[3] = { c.a[0], c.a[2], c.c[0] }, hi[3] = { c.a[1], c.a[3], c.c[1] }; b.grow(lo); b.grow(hi); }
            if (c.child1 != 0x76543210) { const float lo[3] = { c.b[0], c.b[2], c.c[2] }, hi[3] = { c.b[1], c.b[3], c.c[3] }; b.grow(lo); b.grow(hi); }
            return true;
        }
        for (uint32_t e = (uint32_t)~code; e < mr.n_woop; e++) {
            const uint32_t w = widx[mr.woop_offset + e].index;
            b.grow(boxes[w >> 1]);
            if (w & 1u) break;
        }
        return true;
    };
    for (uint32_t v = mr.n_nodes; v-- > 0;) {
        ctl_bvh_node& n = N[v]; aabb b;
        if (child_box(n.child0, b)) { n.a[0] = b.lo[0]; n.a[1] = b.hi[0]; n.a[2] = b.lo[1]; n.a[3] = b.hi[1]; n.c[0] = b.lo[2]; n.c[1] = b.hi[2]; }
        if (child_box(n.child1, b)) { n.b[0] = b.lo[0]; n.b[1] = b.hi[0]; n.b[2] = b.lo[1]; n.b[3] = b.hi[1]; n.c[2] = b.lo[2]; n.c[3] = b.hi[2]; }
    }
    for (uint32_t k = 0; k < nodes.size(); k++) if (nodes[k].mesh_index == mesh_index) recalculate_node_lights(k);
}

// the shape sets of a node's area lights from its current transform and its mesh's current triangles
void scene_builder::recalculate_node_lights(uint32_t node_index) {
    const ctl_node& N = nodes[node_index];
    for (uint32_t k = 0; k < N.n_lights && k < 2; k++) {
        if (N.lights[k] >= lights.size()) continue;
        ctl_light& L = lights[N.lights[k]];
        if (L.type == CTL_LIGHT_DIFFUSE && L.node_idx == node_index && L.count) L.sum_area = recalculate_shape_set(node_index, L.area_dist_index, L.triangles_index, L.count);
    }
}

uint32_t scene_builder::add_node(uint32_t mesh_index, const ctl_float4x4* to_world) {
    if (mesh_index >= meshes.size()) throw std::runtime_error("ctl_builder_add_node: bad mesh index");
    const mesh_rec& mr = mesh_info[mesh_index];
    // validate the transform before anything is appended: a rejected call must leave nodes / mats / xf / ixf untouched
    ctl_float4x4 m;
    if (to_world) m = *to_world; else { std::memset(&m, 0, sizeof(m)); m.m[0] = m.m[5] = m.m[10] = m.m[15] = 1.0f; }
    if (m.m[12] != 0.0f || m.m[13] != 0.0f || m.m[14] != 0.0f || m.m[15] != 1.0f)
        throw std::runtime_error("ctl_builder_add_node: node transform must be affine (last row 0 0 0 1)");
    ctl_float4x4 inv; mat_inverse(m.m, inv.m);   // kept as computed: the reference divides by the inverse's own w (float4x4.h:402-406)
    if (inv.m[12] != 0.0f || inv.m[13] != 0.0f || inv.m[14] != 0.0f || !(inv.m[15] > 0.0f))
        throw std::runtime_error("ctl_builder_add_node: node transform is singular");
    ctl_node n{};   // Node::Node (SceneTypes/Node.cpp:10-17): every node owns a copy of the mesh's materials
    n.mesh_index = mesh_index; n.material_offset = (uint32_t)mats.size(); n.instanciated_material = 0;
    n.lights[0] = n.lights[1] = 0xffffffffu; n.n_lights = 0;
    mats.insert(mats.end(), mesh_materials.begin() + mr.mat_offset, mesh_materials.begin() + mr.mat_offset + mr.n_mat);
    nodes.push_back(n);
    xf.push_back(m); ixf.push_back(inv);
    return (uint32_t)nodes.size() - 1;
}

// DynamicScene::SetNodeTransform (Engine/DynamicScene.cpp:338-346).  recalculate_lights: the area lights of the node have their shape sets recalculated for the
// new transform, as the reference does (ctl_builder_set_node_transform).  The Mitsuba loader sets a transform before it creates the node's lights — except for the
// first instance of a shapegroup, whose lights keep the triangles of the group's own transform as they always did here — and passes false.
void scene_builder::set_node_transform(uint32_t node_index, const ctl_float4x4& m, bool recalculate_lights) {
    if (node_index >= nodes.size()) throw std::runtime_error("set_node_transform: bad node index");
    if (m.m[12] != 0.0f || m.m[13] != 0.0f || m.m[14] != 0.0f || m.m[15] != 1.0f) throw std::runtime_error("set_node_transform: node transform must be affine (last row 0 0 0 1)");
    ctl_float4x4 inv; mat_inverse(m.m, inv.m);
    if (inv.m[12] != 0.0f || inv.m[13] != 0.0f || inv.m[14] != 0.0f || !(inv.m[15] > 0.0f)) throw std::runtime_error("set_node_transform: node transform is singular");
    xf[node_index] = m; ixf[node_index] = inv;
    if (recalculate_lights) recalculate_node_lights(node_index);
}
// `mat->bsdf = ...; mat->bsdf.As()->m_enableTwoSided = ...` of BsdfParser::apply_bsdf (ObjectParser.h:996-1010): replaces the BSDF
// of one of the node's materials and keeps its NodeLightIndex
void scene_builder::set_node_bsdf(uint32_t node_index, uint32_t local_material, const ctl_material& m) {
    if (node_index >= nodes.size()) throw std::runtime_error("set_node_bsdf: bad node index");
    const ctl_node& N = nodes[node_index];
    if (local_material >= mesh_info[N.mesh_index].n_mat) throw std::runtime_error("set_node_bsdf: bad material index");
    ctl_material& dst = mats[N.material_offset + local_material];
    const uint32_t nli = dst.node_light_index;
    dst = m; dst.node_light_index = nli;
}
uint32_t scene_builder::add_aux_material(const ctl_material& m) {
    if (m.bsdf_type >= CTL_BSDF_HK) throw std::runtime_error("add_aux_material: a nested BSDF must be one of the simple models (BSDFFirst, SceneTypes/BSDF.h:102)");
    mats.push_back(m); mats.back().node_light_index = 0xffffffffu;
    return (uint32_t)mats.size() - 1;
}
const ctl_material& scene_builder::node_material(uint32_t node_index, uint32_t local_material) const {
    const ctl_node& N = nodes.at(node_index);
    if (local_material >= mesh_info[N.mesh_index].n_mat) throw std::runtime_error("node_material: bad material index");
    return mats[N.material_offset + local_material];
}
// AABB of all nodes (DynamicScene::getSceneBox)
aabb scene_builder::scene_box() const {
    aabb scene; scene.reset();
    for (size_t i = 0; i < nodes.size(); i++) { const aabb b = box_transform(mesh_info[nodes[i].mesh_index].box, xf[i].m); scene.grow(b); }
    return scene;
}

// ShapeSet::Recalculate (Engine/ShapeSet.cpp:17-59 / triData::Recalculate, ShapeSet.cu:11-23) of one area light: world-space corners, normal and area of its
// triangles (named by i_dat / t_dat of the records in the anim blob) from the node's CURRENT transform, and the normalised area CDF.  Returns the summed area.
float scene_builder::recalculate_shape_set(uint32_t node_index, uint32_t cdf_off, uint32_t tri_off, uint32_t count) {
    m34 l2w = as_m34(xf[node_index].m);
    std::vector<float> cdf(count + 1); std::vector<ctl_shape_tri> st(count);
    std::memcpy(st.data(), anim.data() + tri_off, st.size() * sizeof(ctl_shape_tri));
    float sumArea = 0; cdf[0] = 0.0f;
    for (uint32_t i = 0; i < count; i++) {
        ctl_shape_tri& s = st[i];
        const ctl_woop_tri& w = woop[s.i_dat];
        uint32_t T[8]; std::memcpy(T, &tri[s.t_dat], 32);
        f3 p[3], n; float area;
        shape_triangle(w.a, w.b, w.c, T, l2w, [](uint32_t code) { return uchar2_to_normal(code); }, p, n, area);   // shape_set.h: the device's kernels run the same function
        for (int k = 0; k < 3; k++) { s.p[k][0] = p[k].x; s.p[k][1] = p[k].y; s.p[k][2] = p[k].z; }
        s.n[0] = n.x; s.n[1] = n.y; s.n[2] = n.z; s.area = area;
        sumArea += area; cdf[i + 1] = cdf[i] + area;
    }
    for (uint32_t i = 0; i <= count; i++) cdf[i] = cdf[i] / sumArea;
    std::memcpy(anim.data() + cdf_off, cdf.data(), cdf.size() * sizeof(float));
    std::memcpy(anim.data() + tri_off, st.data(), st.size() * sizeof(ctl_shape_tri));
    return sumArea;
}

// DynamicScene::CreateLight(node, matName, L) + CreateShape (Engine/DynamicScene.cpp:689-767) + ShapeSet (Engine/ShapeSet.cpp:17-59)
uint32_t scene_builder::add_area_light(uint32_t node_index, uint32_t local_material, const float radiance[3], const ctl_texture* rad_texture, bool orthogonal) {
    if (node_index >= nodes.size()) throw std::runtime_error("ctl_builder_add_area_light: bad node index");
    ctl_node& N = nodes[node_index];
    const mesh_rec& mr = mesh_info[N.mesh_index];
    if (local_material >= mr.n_mat) throw std::runtime_error("Could not find material name in mesh!");
    ctl_material& mat = mats[N.material_offset + local_material];
    if (mat.node_light_index == 0xffffffffu && N.n_lights >= 2) throw std::runtime_error("Node already has maximum number of area lights!");
    std::vector<uint32_t> sel_woop, sel_tri;
    for (uint32_t i = 0; i < mr.n_woop; i++) {
        uint32_t i2 = widx[mr.woop_offset + i].index >> 1;
        const ctl_triangle_data& d = tri[mr.tri_offset + i2];
        if (((d.nor_mat_extra[1] >> 16) & 0xff) != local_material) continue;
        if (std::find(sel_tri.begin(), sel_tri.end(), mr.tri_offset + i2) != sel_tri.end()) continue;
        sel_woop.push_back(mr.woop_offset + i); sel_tri.push_back(mr.tri_offset + i2);
    }
    if (sel_woop.empty()) throw std::runtime_error("ctl_builder_add_area_light: material has no triangles");
    uint32_t count = (uint32_t)sel_woop.size();
    auto align_to = [&](size_t a) { while (anim.size() % a) anim.push_back(0); };
    align_to(4); uint32_t cdf_off = (uint32_t)anim.size(); anim.resize(anim.size() + (count + 1) * sizeof(float));
    align_to(16); uint32_t tri_off = (uint32_t)anim.size(); anim.resize(anim.size() + (size_t)count * sizeof(ctl_shape_tri));
    std::vector<ctl_shape_tri> st(count);
    for (uint32_t i = 0; i < count; i++) { st[i] = ctl_shape_tri{}; st[i].i_dat = sel_woop[i]; st[i].t_dat = sel_tri[i]; }
    std::memcpy(anim.data() + tri_off, st.data(), st.size() * sizeof(ctl_shape_tri));
    const float sumArea = recalculate_shape_set(node_index, cdf_off, tri_off, count);
    ctl_light L{};
    L.type = CTL_LIGHT_DIFFUSE; L.radiance[0] = radiance[0]; L.radiance[1] = radiance[1]; L.radiance[2] = radiance[2];
    L.area_dist_index = cdf_off; L.triangles_index = tri_off; L.sum_area = sumArea; L.count = count; L.orthogonal = orthogonal ? 1u : 0u; L.node_idx = node_index;
    if (rad_texture) {
        if (rad_texture->type != CTL_TEX_CONSTANT && rad_texture->type != CTL_TEX_CHECKER && rad_texture->type != CTL_TEX_IMAGE) throw std::runtime_error("ctl_builder_add_area_light_ex: unknown texture type");
        L.rad_texture = *rad_texture;
        if (rad_texture->type == CTL_TEX_CONSTANT) { L.radiance[0] = rad_texture->value[0]; L.radiance[1] = rad_texture->value[1]; L.radiance[2] = rad_texture->value[2]; }
    }
    uint32_t li;
    if (mat.node_light_index != 0xffffffffu) { li = N.lights[mat.node_light_index]; lights[li] = L; }
    else { li = (uint32_t)lights.size(); lights.push_back(L); mat.node_light_index = N.n_lights; N.lights[N.n_lights++] = li; }
    return li;
}

uint32_t scene_builder::add_point_light(const float position[3], const float intensity[3]) {
    ctl_light L{};
    L.type = CTL_LIGHT_POINT;
    for (int i = 0; i < 3; i++) { L.position[i] = position[i]; L.radiance[i] = intensity[i]; }
    lights.push_back(L);
    return (uint32_t)lights.size() - 1;
}

// Frame(n) (Math/Frame.h:31-35) -> rows s, t, n of ctl_light::to_world
static void store_frame(ctl_light& L, f3 n) {
    f3 s, t; coordinate_system(n, s, t);
    std::memset(L.to_world, 0, sizeof(L.to_world));
    L.to_world[0] = s.x; L.to_world[1] = s.y; L.to_world[2] = s.z;
    L.to_world[4] = t.x; L.to_world[5] = t.y; L.to_world[6] = t.z;
    L.to_world[8] = n.x; L.to_world[9] = n.y; L.to_world[10] = n.z;
}

// SpotLight::SpotLight (SceneTypes/Light.cu:268-277): width = cutoff angle, fall = beam width, both in degrees
uint32_t scene_builder::add_spot_light(const float position[3], const float target[3], const float intensity[3], float cutoff_deg, float beam_deg) {
    ctl_light L{};
    L.type = CTL_LIGHT_SPOT;
    for (int i = 0; i < 3; i++) { L.position[i] = position[i]; L.direction[i] = target[i]; L.radiance[i] = intensity[i]; }
    L.cutoff_angle = cutoff_deg * (kPi / 180.0f); L.beam_width = beam_deg * (kPi / 180.0f);
    L.cos_beam_width = cosf(L.beam_width); L.cos_cutoff_angle = cosf(L.cutoff_angle);
    L.inv_transition_width = 1.0f / (L.cutoff_angle - L.beam_width);
    store_frame(L, normalize(f3(target[0], target[1], target[2]) - f3(position[0], position[1], position[2])));
    lights.push_back(L);
    return (uint32_t)lights.size() - 1;
}

// DistantLight(L, d, r) (SceneTypes/Light.h:155-163): radius = r * 1.1 (the Mitsuba loader passes r = 1, ObjectParser.h:530)
uint32_t scene_builder::add_distant_light(const float direction[3], const float irradiance[3], float scene_radius) {
    ctl_light L{};
    L.type = CTL_LIGHT_DISTANT;
    for (int i = 0; i < 3; i++) { L.direction[i] = direction[i]; L.radiance[i] = irradiance[i]; }
    store_frame(L, normalize(f3(direction[0], direction[1], direction[2])));
    L.bsphere_radius = scene_radius * 1.1f;
    lights.push_back(L);
    return (uint32_t)lights.size() - 1;
}

uint32_t scene_builder::add_image(const uint32_t* texels, uint32_t w, uint32_t h, uint32_t texel_type, uint32_t wrap, uint32_t filter) {
    if (!texels || w == 0 || h == 0) throw std::runtime_error("ctl_builder_add_image: empty image");
    if (texel_type > CTL_TEXEL_RGBCOL || wrap > CTL_WRAP_BLACK || filter > CTL_FILTER_TRILINEAR) throw std::runtime_error("ctl_builder_add_image: bad texel type / wrap / filter mode");
    image_texels.emplace_back(texels, texels + (size_t)w * h);
    ctl_mipmap m{}; m.width = w; m.height = h; m.texel_type = texel_type; m.wrap_mode = wrap; m.filter_mode = filter;
    images.push_back(m);
    return (uint32_t)images.size() - 1;
}

// the level-0 texels of a registered image replaced (ctl_builder_update_image): size, texel type, wrap and filter mode stay.  What the builder derives from texels follows:
// the environment light's column / row CDFs and its normalization, rewritten where they stand if the image is the environment map's; the sampling weights of the materials
// that read the image's average are made by the next finalize, as they always are (material_update_textures).  A refused call leaves the builder as it was
void scene_builder::update_image(uint32_t image, const uint32_t* texels, uint32_t w, uint32_t h) {
    if (image >= images.size()) throw std::runtime_error("ctl_builder_update_image: bad image index " + std::to_string(image) + " of " + std::to_string(images.size()));
    if (!texels) throw std::runtime_error("ctl_builder_update_image: null texels");
    if (w != images[image].width || h != images[image].height)
        throw std::runtime_error("ctl_builder_update_image: image " + std::to_string(image) + " is " + std::to_string(images[image].width) + " x " + std::to_string(images[image].height) + "; an update keeps the size");
    image_texels[image].assign(texels, texels + (size_t)w * h);
    if (env_light < lights.size() && lights[env_light].type == CTL_LIGHT_INFINITE && lights[env_light].env_image == image) environment_tables(lights[env_light]);
}

// InfiniteLight::InfiniteLight (SceneTypes/Light.cpp:10-61), the part that reads texels: cdfCols and cdfRows at the light's offsets in the anim blob and its normalization,
// from the image's texels and the rowWeights already there.  The arithmetic is env_tables.h's, which the device runs too (scene_images.hip)
void scene_builder::environment_tables(ctl_light& L) {
    const ctl_mipmap& M = images[L.env_image]; const uint32_t* tx = image_texels[L.env_image].data();
    const uint32_t W = M.width, H = M.height, type = M.texel_type;
    std::vector<float> cdfCols((size_t)(W + 1) * H), cdfRows(H + 1), colSums(H), rowWeights(H);
    std::memcpy(rowWeights.data(), anim.data() + L.row_weights_index, rowWeights.size() * sizeof(float));
    for (uint32_t y = 0; y < H; ++y) {
        float* row = &cdfCols[(size_t)y * (W + 1)]; const uint32_t* t = tx + (size_t)y * W;
        row[0] = 0;
        const float colSum = env_running_sum([&](uint32_t x) { return env_texel_luminance(t[x], type); }, W, 0.0f, row + 1);
        const float normalization = 1.0f / colSum;
        for (uint32_t x = 0; x <= W; ++x) row[x] = env_normalized_entry(row[x], x, W, normalization);
        colSums[y] = colSum;
    }
    cdfRows[0] = 0;
    const float rowSum = env_running_sum([&](uint32_t y) { return colSums[y] * rowWeights[y]; }, H, 0.0f, cdfRows.data() + 1);
    const float normalization = 1.0f / rowSum;
    for (uint32_t y = 0; y <= H; ++y) cdfRows[y] = env_normalized_entry(cdfRows[y], y, H, normalization);
    std::memcpy(anim.data() + L.cdf_cols_index, cdfCols.data(), cdfCols.size() * sizeof(float));
    std::memcpy(anim.data() + L.cdf_rows_index, cdfRows.data(), cdfRows.size() * sizeof(float));
    L.normalization = env_normalization(rowSum, W, H);
}

// DynamicScene::setEnvironementMap (Engine/DynamicScene.cpp:846-859) + InfiniteLight::InfiniteLight (SceneTypes/Light.cpp:10-61)
uint32_t scene_builder::set_environment_map(uint32_t image, const float scale[3], const ctl_float4x4* to_world) {
    if (env_light != 0xffffffffu) throw std::runtime_error("Can't set environment map when it is already set!");
    if (image >= images.size()) throw std::runtime_error("ctl_builder_set_environment_map: bad image index");
    const ctl_mipmap& M = images[image];
    const uint32_t W = M.width, H = M.height;
    auto align_to = [&](size_t a) { while (anim.size() % a) anim.push_back(0); };
    align_to(16); uint32_t cols_off = (uint32_t)anim.size(); anim.resize(anim.size() + (size_t)(W + 1) * H * sizeof(float));
    align_to(16); uint32_t rows_off = (uint32_t)anim.size(); anim.resize(anim.size() + (size_t)(H + 1) * sizeof(float));
    align_to(16); uint32_t wts_off = (uint32_t)anim.size(); anim.resize(anim.size() + (size_t)H * sizeof(float));
    std::vector<float> rowWeights(H);
    const float sizeY = (float)H;
    for (uint32_t y = 0; y < H; ++y) rowWeights[y] = sinf((y + 0.5f) * kPi / sizeY);
    std::memcpy(anim.data() + wts_off, rowWeights.data(), rowWeights.size() * sizeof(float));
    ctl_light L{};
    L.type = CTL_LIGHT_INFINITE;
    L.env_image = image;
    for (int i = 0; i < 3; i++) L.env_scale[i] = scale[i];
    L.cdf_cols_index = cols_off; L.cdf_rows_index = rows_off; L.row_weights_index = wts_off;
    environment_tables(L);
    static const float ident[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1 };
    std::memcpy(L.to_world, to_world ? to_world->m : ident, 64);
    lights.push_back(L);
    env_light = (uint32_t)lights.size() - 1;
    return env_light;
}

// RoughTransmittanceManager::StaticInitialize (Engine/RoughTransmittance.cu:124-131): one slot
void scene_builder::set_rough_transmittance(uint32_t slot, const ctl_rough_transmittance& t) {
    if (slot >= 3) throw std::runtime_error("ctl_builder_set_rough_transmittance: slot must be 0..2");
    if (!t.trans || !t.diff_trans || t.eta_samples < 2 || t.alpha_samples < 2 || t.theta_samples < 2) throw std::runtime_error("ctl_builder_set_rough_transmittance: bad table");
    const size_t nt = (size_t)2 * t.eta_samples * t.alpha_samples * t.theta_samples, nd = (size_t)2 * t.eta_samples * t.alpha_samples;
    rt_trans[slot].assign(t.trans, t.trans + nt); rt_diff[slot].assign(t.diff_trans, t.diff_trans + nd);
    rt[slot] = t; have_rt = true;
}
// RoughTransmittance::RoughTransmittance(name) (Engine/RoughTransmittance.cu:8-45): "MTS_TRANSMITTANCE", three size_t counts,
// four float bounds, then per (eta, alpha): theta_samples transmittances followed by one diffuse transmittance
void scene_builder::load_rough_transmittance(uint32_t slot, const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("Could not open file : ") + path);
    std::vector<unsigned char> buf;
    std::fseek(f, 0, SEEK_END); long sz = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    buf.resize(sz > 0 ? (size_t)sz : 0);
    if (sz > 0 && std::fread(buf.data(), 1, buf.size(), f) != buf.size()) { std::fclose(f); throw std::runtime_error("short read"); }
    std::fclose(f);
    const char header[] = "MTS_TRANSMITTANCE"; const size_t hl = sizeof(header) - 1;
    if (buf.size() < hl + 3 * 8 + 4 * 4 || std::memcmp(buf.data(), header, hl) != 0) throw std::runtime_error("Invalid filetype for rough transmittance!");
    size_t pos = hl; uint64_t cnt[3]; float bnd[4];
    std::memcpy(cnt, buf.data() + pos, 24); pos += 24;
    std::memcpy(bnd, buf.data() + pos, 16); pos += 16;
    const size_t E = cnt[0], A = cnt[1], T = cnt[2], nt = 2 * E * A * T, nd = 2 * E * A;
    if (buf.size() != pos + (nt + nd) * sizeof(float)) throw std::runtime_error("RoughTransmittance: unexpected file size");
    const float* ptr = (const float*)(buf.data() + pos);
    std::vector<float> trans(nt), diff(nd); size_t de = 0, fe = 0;
    for (size_t i = 0; i < 2 * E; ++i) for (size_t j = 0; j < A; ++j) { for (size_t k = 0; k < T; ++k) trans[de++] = *ptr++; diff[fe++] = *ptr++; }
    ctl_rough_transmittance t{}; t.trans = trans.data(); t.diff_trans = diff.data();
    t.eta_samples = (uint32_t)E; t.alpha_samples = (uint32_t)A; t.theta_samples = (uint32_t)T;
    t.eta_min = bnd[0]; t.eta_max = bnd[1]; t.alpha_min = bnd[2]; t.alpha_max = bnd[3];
    set_rough_transmittance(slot, t);
}

// Sensor::SetToWorld(pos, tar, up) (SceneTypes/Sensor.cu:691-699) with the loader's frame reconstruction
// (ObjectParser.h:292-297, Sensor.cu:682-689): r = f x up, u = r x f, columns (r, u, f), translation pos.
void scene_builder::set_camera_lookat(const float pos[3], const float target[3], const float up_in[3], float fov_degrees, uint32_t w, uint32_t h) {
    f3 p(pos[0], pos[1], pos[2]), tar(target[0], target[1], target[2]), u(up_in[0], up_in[1], up_in[2]);
    f3 f = normalize(tar - p);
    f3 r = normalize(cross(f, u));
    std::memset(&camera, 0, sizeof(camera));
    camera.type = CTL_SENSOR_PERSPECTIVE;
    float rot[16] = { r.x, u.x, f.x, 0, r.y, u.y, f.y, 0, r.z, u.z, f.z, 0, 0, 0, 0, 1 };
    float tr[16] = { 1, 0, 0, p.x, 0, 1, 0, p.y, 0, 0, 1, p.z, 0, 0, 0, 1 };
    mat_mul(tr, rot, camera.to_world);   // float4x4::Translate(pos) % rot (Sensor.cu:672-678)
    camera.fov = fov_degrees * (kPi / 180.0f);   // math::Radians (SceneTypes/Sensor.h:72-76)
    camera.near_depth = 1e-2f; camera.far_depth = 1e4f;   // loader defaults (ObjectParser.h:242)
    camera.resolution[0] = (float)w; camera.resolution[1] = (float)h;
    have_camera = true;
}
void scene_builder::set_camera(const ctl_sensor& s) { camera = s; have_camera = true; }

// AABB::Transform (Math/AABB.h:32-45)
static aabb box_transform(const aabb& b, const float* m) {
    aabb o;
    for (int i = 0; i < 3; i++) {
        float lo = m[i * 4 + 3], hi = m[i * 4 + 3];   // + Translation()
        float s_lo = 0, s_hi = 0;
        for (int k = 0; k < 3; k++) { float a = m[i * 4 + k] * b.lo[k], c = m[i * 4 + k] * b.hi[k]; s_lo += min2(a, c); s_hi += max2(a, c); }
        o.lo[i] = s_lo + lo; o.hi[i] = s_hi + hi;
    }
    return o;
}

uint32_t scene_builder::create_volume(const ctl_volume& v) {
    if (volumes.size() >= CTL_MAX_VOL_COUNT) throw std::runtime_error("ctl_builder_create_volume: the aggregate holds at most " + std::to_string(CTL_MAX_VOL_COUNT) + " volumes (KernelAggregateVolume::MAX_VOL_COUNT)");
    ctl_volume c = v; volume_update(c);
    volumes.push_back(c);
    return (uint32_t)volumes.size() - 1;
}
void scene_builder::set_volume(uint32_t index, const ctl_volume& v) {
    if (index >= volumes.size()) throw std::runtime_error("ctl_builder_set_volume: bad volume index");
    ctl_volume c = v; volume_update(c);
    volumes[index] = c;
}
uint32_t scene_builder::create_volume_grid(const uint32_t* dims, uint32_t n_dims, const ctl_float4x4& volume_to_world, const ctl_phase_function& phase) {
    if (n_dims != 3 && n_dims != 9) throw std::runtime_error("ctl_builder_create_volume_grid: 3 dims (one grid) or 9 (gridA, gridS, gridL)");
    grid_store g; g.rec.single_grid = n_dims == 3 ? 1u : 0u;
    auto grid = [&](uint32_t* to, const uint32_t* from, std::vector<float>& data) {
        if (!from[0] || !from[1] || !from[2] || from[0] > CTL_MAX_GRID_CELLS || from[1] > CTL_MAX_GRID_CELLS || from[2] > CTL_MAX_GRID_CELLS || (uint64_t)from[0] * from[1] > CTL_MAX_GRID_CELLS || (uint64_t)from[0] * from[1] * from[2] > CTL_MAX_GRID_CELLS)
            throw std::runtime_error("ctl_builder_create_volume_grid: a grid has a zero dimension or more than " + std::to_string(CTL_MAX_GRID_CELLS) + " cells (CTL_MAX_GRID_CELLS)");
        for (int c = 0; c < 3; c++) to[c] = from[c];
        data.assign((size_t)from[0] * from[1] * from[2], 0.0f);
    };
    if (n_dims == 3) grid(g.rec.dim, dims, g.data[0]);
    else { grid(g.rec.dim_a, dims, g.data[0]); grid(g.rec.dim_s, dims + 3, g.data[1]); }   // dims[6..8], gridL: not carried
    ctl_volume v{}; v.type = CTL_VOLUME_GRID; v.phase = phase; v.volume_to_world = volume_to_world;
    g.rec.volume = create_volume(v);
    grid_stores.push_back(std::move(g));
    return grid_stores.back().rec.volume;
}
static scene_builder::grid_store& grid_store_of(scene_builder& b, uint32_t index, const char* who) {
    for (auto& g : b.grid_stores) if (g.rec.volume == index) return g;
    throw std::runtime_error(std::string(who) + ": volume " + std::to_string(index) + " is no VolumeGrid of this builder");
}
void scene_builder::set_volume_grid_data(uint32_t index, uint32_t which, const float* data, uint32_t n) {
    grid_store& g = grid_store_of(*this, index, "ctl_builder_set_volume_grid_data");
    if (which > 1 || (which == 1 && g.rec.single_grid)) throw std::runtime_error("ctl_builder_set_volume_grid_data: which = 0 (grid / gridA) or, in the three-grid form, 1 (gridS)");
    if (!data || n != g.data[which].size()) throw std::runtime_error("ctl_builder_set_volume_grid_data: " + std::to_string(n) + " floats for a grid of " + std::to_string(g.data[which].size()));
    g.data[which].assign(data, data + n);
}
void scene_builder::set_volume_grid_coefficients(uint32_t index, const float* sig_a_min, const float* sig_a_max, const float* sig_s_min, const float* sig_s_max) {
    grid_store& g = grid_store_of(*this, index, "ctl_builder_set_volume_grid_coefficients");
    for (int c = 0; c < 3; c++) { g.rec.sig_a_min[c] = sig_a_min[c]; g.rec.sig_a_max[c] = sig_a_max[c]; g.rec.sig_s_min[c] = sig_s_min[c]; g.rec.sig_s_max[c] = sig_s_max[c]; }
}

void scene_builder::remove_node(uint32_t i) {
    if (i >= nodes.size()) throw std::runtime_error("remove_node: bad node index");
    if (nodes[i].n_lights) throw std::runtime_error("remove_node: node " + std::to_string(i) + " carries area lights");
    nodes.erase(nodes.begin() + i); xf.erase(xf.begin() + i); ixf.erase(ixf.begin() + i);
    for (auto& L : lights) if (L.type == CTL_LIGHT_DIFFUSE && L.node_idx != 0xffffffffu && L.node_idx > i) L.node_idx--;
}

// The counterpart of add_mesh for a mesh no node instances any more (the reference frees such a mesh's ranges, DynamicScene.cpp:483-507 / Mesh::Free; the arrays here are
// dense, so the later meshes move down): the builder afterwards holds, in tri, woop, widx, bvh, meshes and mesh_info, what a builder holds that never added the mesh.
// Everything that can refuse runs before the first byte is written.  mesh_materials (and with it every std_material_offset) stays as it is.
void scene_builder::remove_mesh(uint32_t mesh_index) {
    if (mesh_index >= mesh_info.size()) throw std::runtime_error("ctl_builder_remove_mesh: bad mesh index");
    for (size_t k = 0; k < nodes.size(); k++) if (nodes[k].mesh_index == mesh_index)
        throw std::runtime_error("ctl_builder_remove_mesh: node " + std::to_string(k) + " still instances mesh " + std::to_string(mesh_index) + " (ctl_builder_remove_node first)");
    const mesh_rec mr = mesh_info[mesh_index];
    if ((size_t)mr.tri_offset + mr.n_tris > tri.size() || (size_t)mr.woop_offset + mr.n_woop > woop.size() || woop.size() != widx.size() || (size_t)mr.node_offset + mr.n_nodes > bvh.size())
        throw std::runtime_error("ctl_builder_remove_mesh: the mesh's ranges reach outside the builder's arrays");
    tri.erase(tri.begin() + mr.tri_offset, tri.begin() + mr.tri_offset + mr.n_tris);
    woop.erase(woop.begin() + mr.woop_offset, woop.begin() + mr.woop_offset + mr.n_woop);
    widx.erase(widx.begin() + mr.woop_offset, widx.begin() + mr.woop_offset + mr.n_woop);
    bvh.erase(bvh.begin() + mr.node_offset, bvh.begin() + mr.node_offset + mr.n_nodes);
    mesh_info.erase(mesh_info.begin() + mesh_index); meshes.erase(meshes.begin() + mesh_index);
    for (size_t m = mesh_index; m < mesh_info.size(); m++) {   // add_mesh only ever appends: every later mesh lies behind the erased ranges
        mesh_rec& r = mesh_info[m];
        r.tri_offset -= mr.n_tris; r.woop_offset -= mr.n_woop; r.node_offset -= mr.n_nodes;
        ctl_kernel_mesh& km = meshes[m];
        km.tri_offset = r.tri_offset; km.bvh_node_offset = r.node_offset * 4; km.bvh_tri_offset = r.woop_offset * 3; km.bvh_index_offset = r.woop_offset;
    }
    // the shape sets of area lights name global rows and triangles (i_dat, t_dat): those on nodes of later meshes follow, while the nodes still carry the old mesh indices
    for (const ctl_light& L : lights) {
        if (L.type != CTL_LIGHT_DIFFUSE || L.node_idx >= nodes.size() || nodes[L.node_idx].mesh_index <= mesh_index) continue;
        if ((size_t)L.triangles_index + (size_t)L.count * sizeof(ctl_shape_tri) > anim.size()) continue;
        for (uint32_t i = 0; i < L.count; i++) {
            ctl_shape_tri s; std::memcpy(&s, anim.data() + L.triangles_index + (size_t)i * sizeof(ctl_shape_tri), sizeof(s));
            s.i_dat -= mr.n_woop; s.t_dat -= mr.n_tris;
            std::memcpy(anim.data() + L.triangles_index + (size_t)i * sizeof(ctl_shape_tri), &s, sizeof(s));
        }
    }
    for (ctl_node& n : nodes) if (n.mesh_index > mesh_index) n.mesh_index--;
}

// ---- the image set and the material table edited after the fact (ctl_builder_remove_image, _replace_image, _get_material, _set_material)
namespace {
const char* const kTextureSlots[6] = { "tex[0]", "tex[1]", "tex[2]", "tex[3]", "map_tex", "alpha_tex" };
ctl_texture& texture_slot(ctl_material& m, int k) { return k < 4 ? m.tex[k] : (k == 4 ? m.map_tex : m.alpha_tex); }
const ctl_texture& texture_slot(const ctl_material& m, int k) { return k < 4 ? m.tex[k] : (k == 4 ? m.map_tex : m.alpha_tex); }
bool names_image(const ctl_texture& t, uint32_t image) { return t.type == CTL_TEX_IMAGE && t.image == image; }
void lower_image(ctl_texture& t, uint32_t removed) { if (t.type == CTL_TEX_IMAGE && t.image != 0xffffffffu && t.image > removed) t.image--; }
}  // namespace

// The counterpart of add_image for an image nothing reads any more: the builder afterwards holds, in images, image_texels, mats and lights, what a builder holds that never
// added the image.  Everything that can refuse runs before the first byte is written.  A referrer is any texture slot of type CTL_TEX_IMAGE of any row of `mats` — a row
// orphaned by remove_node / remove_mesh included: the table is not compacted, and the row would reach a scene with a dangling index —, a DiffuseLight's radiance texture
// and the environment light's map.  mesh_materials, which only a later add_node copies from, follow the shift; a slot there that names the removed image becomes "no
// image" (0xffffffff, black: Texture.cu:33-34), for the host to set on the node's copy
void scene_builder::remove_image(uint32_t image) {
    const std::string who = "ctl_builder_remove_image: ";
    if (image >= images.size()) throw std::runtime_error(who + "bad image index " + std::to_string(image) + " of " + std::to_string(images.size()));
    for (size_t i = 0; i < mats.size(); i++) for (int k = 0; k < 6; k++) if (names_image(texture_slot(mats[i], k), image))
        throw std::runtime_error(who + "material " + std::to_string(i) + " (" + kTextureSlots[k] + ") still references image " + std::to_string(image) + " (ctl_builder_set_material first)");
    for (size_t i = 0; i < lights.size(); i++) {
        if (lights[i].type == CTL_LIGHT_DIFFUSE && names_image(lights[i].rad_texture, image)) throw std::runtime_error(who + "the radiance texture of light " + std::to_string(i) + " still references image " + std::to_string(image));
        if (lights[i].type == CTL_LIGHT_INFINITE && lights[i].env_image == image) throw std::runtime_error(who + "light " + std::to_string(i) + " (the environment map) still references image " + std::to_string(image));
    }
    images.erase(images.begin() + image); image_texels.erase(image_texels.begin() + image);
    for (ctl_material& m : mats) for (int k = 0; k < 6; k++) lower_image(texture_slot(m, k), image);
    for (ctl_material& m : mesh_materials) for (int k = 0; k < 6; k++) { ctl_texture& t = texture_slot(m, k); if (names_image(t, image)) t.image = 0xffffffffu; else lower_image(t, image); }
    for (ctl_light& L : lights) {
        if (L.type == CTL_LIGHT_DIFFUSE) lower_image(L.rad_texture, image);
        if (L.type == CTL_LIGHT_INFINITE && L.env_image > image) L.env_image--;
    }
}

// new level-0 texels of ANOTHER size at the same index; texel type, wrap and filter mode stay.  With the image's own size it is update_image.  The environment map's image
// is refused: its tables were laid out in the anim blob by set_environment_map for its size
void scene_builder::replace_image(uint32_t image, const uint32_t* texels, uint32_t w, uint32_t h) {
    const std::string who = "ctl_builder_replace_image: ";
    if (image >= images.size()) throw std::runtime_error(who + "bad image index " + std::to_string(image) + " of " + std::to_string(images.size()));
    if (!texels || w == 0 || h == 0) throw std::runtime_error(who + "empty image");
    if (w == images[image].width && h == images[image].height) { update_image(image, texels, w, h); return; }
    for (size_t i = 0; i < lights.size(); i++) if (lights[i].type == CTL_LIGHT_INFINITE && lights[i].env_image == image)
        throw std::runtime_error(who + "image " + std::to_string(image) + " is the environment map of light " + std::to_string(i) + ": its tables in the anim blob were laid out for " +
                                 std::to_string(images[image].width) + " x " + std::to_string(images[image].height));
    image_texels[image].assign(texels, texels + (size_t)w * h);
    images[image].width = w; images[image].height = h;
}

const ctl_material& scene_builder::material(uint32_t index) const {
    if (index >= mats.size()) throw std::runtime_error("ctl_builder_get_material: bad material index " + std::to_string(index) + " of " + std::to_string(mats.size()));
    return mats[index];
}
// DynamicScene::getMaterials + Invalidate for one row of the material table, addressed as the kernels address it (ctl_node::material_offset + local index, or what
// add_aux_material returned).  The record is stored as given, node_light_index included (a host edits what get_material handed it); what can be judged of it without the
// transmittance tables is judged here, the rest by ctl_scene_desc_check as for any description
void scene_builder::set_material(uint32_t index, const ctl_material& m) {
    const std::string who = "ctl_builder_set_material: ";
    if (index >= mats.size()) throw std::runtime_error(who + "bad material index " + std::to_string(index) + " of " + std::to_string(mats.size()));
    if (!is_simple_bsdf(m.bsdf_type) && !is_nesting_bsdf(m.bsdf_type)) throw std::runtime_error(who + "BSDF type " + std::to_string(m.bsdf_type) + " has no HIP implementation yet");
    if (m.map_kind > CTL_MAP_HEIGHT) throw std::runtime_error(who + "unknown surface map kind");
    if (m.alpha_state > CTL_ALPHA_REFLECTANCE_COLOR || m.alpha_state == 4) throw std::runtime_error(who + "unknown alpha blend state");
    for (int k = 0; k < 6; k++) {
        if ((k == 4 && m.map_kind == CTL_MAP_NONE) || (k == 5 && m.alpha_state == CTL_ALPHA_DISABLED)) continue;   // counted only where they are read, as check_scene_desc counts them
        const ctl_texture& t = texture_slot(m, k);
        if (t.type != CTL_TEX_CONSTANT && t.type != CTL_TEX_CHECKER && t.type != CTL_TEX_IMAGE && t.type != 0) throw std::runtime_error(who + "texture type " + std::to_string(t.type) + " has no HIP implementation yet");
        if (t.type == CTL_TEX_IMAGE && t.image != 0xffffffffu && t.image >= images.size()) throw std::runtime_error(who + std::string(kTextureSlots[k]) + " references image " + std::to_string(t.image) + " of " + std::to_string(images.size()));
    }
    // BSDFFirst (SceneTypes/BSDF.h:102): a nested BSDF is one of the simple models — the rule add_aux_material holds a new row to, in both directions here
    for (int k = 0; k < nested_bsdf_count(m.bsdf_type); k++) {
        const uint32_t ni = m.u[2 + k];
        if (ni >= mats.size() || ni == index || mats[ni].bsdf_type >= CTL_BSDF_HK) throw std::runtime_error(who + "nested material index " + std::to_string(ni) + " is out of range or names no simple BSDF (BSDFFirst)");
    }
    if (m.bsdf_type >= CTL_BSDF_HK) for (size_t i = 0; i < mats.size(); i++) for (int k = 0; k < nested_bsdf_count(mats[i].bsdf_type); k++) if (mats[i].u[2 + k] == index && i != index)
        throw std::runtime_error(who + "material " + std::to_string(i) + " nests material " + std::to_string(index) + ", which must stay a simple BSDF (BSDFFirst)");
    mats[index] = m;
}

void scene_builder::finalize(ctl_scene_desc& out) {
    if (nodes.empty()) throw std::runtime_error("ctl_builder_finalize: scene has no nodes");
    if (!have_camera) throw std::runtime_error("ctl_builder_finalize: no camera set");
    if (nodes.size() != xf.size() || nodes.size() != ixf.size()) throw std::runtime_error("ctl_builder_finalize: node / transform arrays out of step");
    // SceneBVH::Build (Engine/SceneBVH.cpp:11-54): one scene-BVH leaf per node (BVHRebuilder.cpp:380-383)
    std::vector<aabb> nb(nodes.size());
    aabb scene; scene.reset();
    for (size_t i = 0; i < nodes.size(); i++) { nb[i] = box_transform(mesh_info[nodes[i].mesh_index].box, xf[i].m); scene.grow(nb[i]); }
    bvh_result R;
    build_bvh(nb, 1, false, 20, R);
    scene_bvh = R.nodes;
    // leaves ~k index leaf_prims (one entry each) -> encode ~nodeIdx directly as the reference does
    auto fix = [&](int c) { return (c < 0) ? ~(int)R.leaf_prims[~c] : c; };
    for (auto& n : scene_bvh) { n.child0 = fix(n.child0); n.child1 = fix(n.child1); }
    int start = R.root < 0 ? ~(int)R.leaf_prims[~R.root] : R.root;
    int top_depth = R.max_depth, bottom_depth = 0;
    for (auto& m : mesh_info) bottom_depth = std::max(bottom_depth, m.max_depth);
    if (top_depth + bottom_depth + 4 > 64) throw std::runtime_error("ctl_builder_finalize: BVH too deep for the traversal stack");

    std::memset(&out, 0, sizeof(out));
    out.tri_data = tri.data(); out.n_tri_data = (uint32_t)tri.size();
    out.woop = woop.data(); out.n_woop = (uint32_t)woop.size(); out.woop_index = widx.data();
    out.bvh_nodes = bvh.data(); out.n_bvh_nodes = (uint32_t)bvh.size();
    out.meshes = meshes.data(); out.n_meshes = (uint32_t)meshes.size();
    out.nodes = nodes.data(); out.n_nodes = (uint32_t)nodes.size();
    out.materials = mats.data(); out.n_materials = (uint32_t)mats.size();
    out.lights = lights.data(); out.n_lights_buf = (uint32_t)lights.size();
    out.anim = anim.data(); out.n_anim_bytes = (uint32_t)anim.size();
    out.scene_start_node = start;
    out.scene_bvh_nodes = scene_bvh.data(); out.n_scene_bvh_nodes = (uint32_t)scene_bvh.size();
    out.node_transforms = xf.data(); out.node_inv_transforms = ixf.data();
    out.env_map_index = env_light;
    for (int i = 0; i < 3; i++) { out.box_min[i] = scene.lo[i]; out.box_max[i] = scene.hi[i]; }
    for (size_t i = 0; i < images.size(); i++) images[i].texels = image_texels[i].data();
    out.images = images.data(); out.n_images = (uint32_t)images.size();
    {   // BSDF::Update() now that every image is there (MaterialStream::UpdateMaterialsPhase2 after LoadTextures, Engine/DynamicScene.cpp:74-89): the sampling weights that come
        // from the average of an IMAGE texture were made with the bitmap counted as white (material_textures.h)
        image_set I; I.images = images.data(); I.n = (uint32_t)images.size();
        std::vector<float> avg_cache(4 * images.size() + 4, 0.0f); I.cache = reinterpret_cast<float (*)[4]>(avg_cache.data());
        for (auto& m : mats) material_update_textures(m, I);
    }
    for (int i = 0; i < 3; i++) { rt[i].trans = rt_trans[i].empty() ? nullptr : rt_trans[i].data(); rt[i].diff_trans = rt_diff[i].empty() ? nullptr : rt_diff[i].data(); }
    out.rough_transmittance = have_rt ? rt : nullptr;
    out.volumes = volumes.empty() ? nullptr : volumes.data(); out.n_volumes = (uint32_t)volumes.size();
    grid_records.clear();
    for (auto& g : grid_stores) {
        if (g.rec.volume >= volumes.size() || volumes[g.rec.volume].type != CTL_VOLUME_GRID) continue;   // ctl_builder_set_volume made the region a homogeneous one
        ctl_volume_grid r = g.rec; r.data = r.single_grid ? g.data[0].data() : nullptr; r.data_a = r.single_grid ? nullptr : g.data[0].data(); r.data_s = r.single_grid ? nullptr : g.data[1].data();
        grid_records.push_back(r);
    }
    out.volume_grids = grid_records.empty() ? nullptr : grid_records.data(); out.n_volume_grids = (uint32_t)grid_records.size();
    {   // the light that depends on the scene box: InfiniteLight::Update (SceneTypes/Light.h:318-325)
        f3 lo(scene.lo[0], scene.lo[1], scene.lo[2]), hi(scene.hi[0], scene.hi[1], scene.hi[2]);
        f3 center = (lo + hi) * 0.5f;   // AABB::Center (Math/AABB.h)
        f3 size = hi - lo;
        for (auto& L : lights) {
            if (L.type == CTL_LIGHT_INFINITE) { L.bsphere_center[0] = center.x; L.bsphere_center[1] = center.y; L.bsphere_center[2] = center.z; L.bsphere_radius = length(size) / 1.5f; }
        }
    }
    out.camera = camera;
    // LightStream::fillDeviceData (Engine/DynamicScene.cpp:172-196): uniform weights, first MAX_NUM_LIGHTS lights
    out.num_lights = std::min<uint32_t>(CTL_MAX_NUM_LIGHTS, (uint32_t)lights.size());
    float accum = 0; for (size_t i = 0; i < lights.size(); i++) accum += 1.0f;
    for (uint32_t i = 0; i < out.num_lights; i++) {
        out.light_indices[i] = i;
        float pdf = 1.0f / accum;
        out.light_cdf[i] = (i > 0 ? out.light_cdf[i - 1] : 0.0f) + pdf;
    }
    // m_rayTraceEps = MIN_RAYTRACE_DISTANCE_RELATIVE * |box.Size()| (Engine/DynamicScene.cpp:587)
    f3 sz(scene.hi[0] - scene.lo[0], scene.hi[1] - scene.lo[1], scene.hi[2] - scene.lo[2]);
    out.ray_trace_eps = 1e-4f * length(sz);
}

} // namespace ctl
