// mesh_skin.hip — skinned meshes: a mesh bound to a scene is posed on the device from bone matrices (ctl_scene_bind_skin / ctl_scene_animate_mesh), the front half of
// what ctl_builder_update_mesh + ctl_scene_update do on the host for a deformed mesh.  The kernels around the functions of mesh_skin.h, which the host yardstick
// (skin_mesh_host, what ctl_skin_mesh_host runs) calls too — same functions, same order of operations, so the device arrays equal the host's bit for bit
// (tests/test_gpu_skin.py).
//
//   k_skin_vertices      one lane per vertex: rest position and normal (16-B loads), 16 B of bone index and weight bytes; both bone palettes (2 x n_bones x 64 B, at most
//                        32 KB) are staged through LDS, because the per-lane bone bytes diverge and eight gathers from LDS beat eight divergent global loads.  Writes the
//                        skinned position and normal = normalize(lerp(n0, n1)) into the binding's scratch arrays (16 B each).
//   k_compile_triangles  one lane per triangle of the mesh: gathers three skinned vertices, keeps the triangle's uv words and material byte (read from tri_data: uvs and
//                        materials do not animate), recomputes dpdu / dpdv and the normal codes, writes the 32 B back into the same rows of tri_data.
//   k_woop_rows          one lane per row of the mesh's range of the two-level leaf stream (a mesh with spatial splits has more rows than triangles): index word ->
//                        mesh-local triangle -> three skinned vertices -> TriIntersectorData::setData -> rows 0..2; the index word stays.
// then Scene::refit_flat with the mesh marked as changed: k_deform_entries for the nodes that instance it, the refit, the re-stamp — as after a CTL_DIFF_GEOMETRY update.
// Plain launches on the null stream, in order; 256-lane workgroups; no workgroup waits for another; no atomics.
#include "tracer.h"
#include "mesh_skin.h"
#include "flat_device.h"
#include "flat_mesh_set.h"
#include "scene_builder.h"
#include "geometry_hash.h"
#include "mitsuba_loader.h"   // unsupported_error
#include <cmath>
#include <string>

namespace ctl {

// what a bound mesh keeps in HBM: the bind arrays, uploaded once, and the scratch of a pose
struct skin_binding {
    uint32_t n_vert = 0, n_tri = 0, n_bones = 0, tri0 = 0, woop0 = 0, n_rows = 0;
    bool indexed = false, posed = false;
    dbuf<float4> rest_p, rest_n, skinned_p, skinned_n, bones;   // bones: pose 0 then pose 1, four float4 per matrix
    dbuf<uint4> bone_bytes;                                     // per vertex: 8 index bytes (x, y), 8 weight bytes (z, w)
    dbuf<uint32_t> indices;                                     // three per triangle; empty for a soup
};

namespace {

struct skin_device {
    const float4* rest_p; const float4* rest_n; const uint4* bone_bytes; const float4* bones; const uint32_t* indices;   // indices == nullptr: a soup
    float4* skinned_p; float4* skinned_n;
    uint4* tri_data; float4* leaf_tris;
    uint32_t n_vert, n_tri, n_bones, tri0, woop0, n_rows; float lerp;
};

__device__ __forceinline__ void unpack_bone_bytes(uint4 b, uint8_t idx[8], uint8_t wgt[8]) {
    for (int i = 0; i < 4; i++) { idx[i] = (uint8_t)(b.x >> (8 * i)); idx[4 + i] = (uint8_t)(b.y >> (8 * i)); wgt[i] = (uint8_t)(b.z >> (8 * i)); wgt[4 + i] = (uint8_t)(b.w >> (8 * i)); }
}

__global__ void __launch_bounds__(256) k_skin_vertices(skin_device K) {
    extern __shared__ float4 s_bones[];   // 2 x n_bones x 4
    const uint32_t n4 = K.n_bones * 8u;
    for (uint32_t i = threadIdx.x; i < n4; i += 256u) s_bones[i] = K.bones[i];
    __syncthreads();
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= K.n_vert) return;
    const float4 p = K.rest_p[v], n = K.rest_n[v];
    uint8_t idx[8], wgt[8];
    unpack_bone_bytes(K.bone_bytes[v], idx, wgt);
    for (int i = 0; i < 8; i++) if (idx[i] >= K.n_bones) return;   // cannot happen after ctl_scene_bind_skin's checks; never read outside the palette
    const float* b0 = reinterpret_cast<const float*>(s_bones);
    f3 po, no;
    skin_vertex(b0, b0 + (size_t)K.n_bones * 16u, K.lerp, f3(p.x, p.y, p.z), f3(n.x, n.y, n.z), idx, wgt, po, no);
    K.skinned_p[v] = make_float4(po.x, po.y, po.z, 0.0f);
    K.skinned_n[v] = make_float4(no.x, no.y, no.z, 0.0f);
}

__device__ __forceinline__ bool triangle_vertices(const skin_device& K, uint32_t t, uint32_t v[3]) {
    for (int j = 0; j < 3; j++) { v[j] = K.indices ? K.indices[(size_t)t * 3 + j] : t * 3u + (uint32_t)j; if (v[j] >= K.n_vert) return false; }
    return true;
}

__global__ void __launch_bounds__(256) k_compile_triangles(skin_device K) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= K.n_tri) return;
    uint32_t v[3];
    if (!triangle_vertices(K, t, v)) return;
    uint4* __restrict__ D = K.tri_data + (size_t)(K.tri0 + t) * 2;
    const uint4 d0 = D[0], d1 = D[1];
    uint32_t T[8] = { d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w };
    f3 p[3], n[3];
    for (int j = 0; j < 3; j++) { const float4 a = K.skinned_p[v[j]], b = K.skinned_n[v[j]]; p[j] = f3(a.x, a.y, a.z); n[j] = f3(b.x, b.y, b.z); }
    skin_compile_triangle(T, p, n);
    D[0] = make_uint4(T[0], T[1], T[2], T[3]); D[1] = make_uint4(T[4], T[5], T[6], T[7]);
}

__global__ void __launch_bounds__(256) k_woop_rows(skin_device K) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= K.n_rows) return;
    float4* __restrict__ W = K.leaf_tris + (size_t)(K.woop0 + i) * 4;
    const uint32_t t = __float_as_uint(W[3].x) >> 1;
    uint32_t v[3];
    if (t >= K.n_tri || !triangle_vertices(K, t, v)) return;
    const float4 a = K.skinned_p[v[0]], b = K.skinned_p[v[1]], c = K.skinned_p[v[2]];
    float r[12];
    woop_rows_from_vertices(r, f3(a.x, a.y, a.z), f3(b.x, b.y, b.z), f3(c.x, c.y, c.z));
    W[0] = make_float4(r[0], r[1], r[2], r[3]); W[1] = make_float4(r[4], r[5], r[6], r[7]); W[2] = make_float4(r[8], r[9], r[10], r[11]);
}

bool finite16(const float* m) { for (int i = 0; i < 16; i++) if (!std::isfinite(m[i])) return false; return true; }

}  // namespace

void skin_check_arguments(const char* who, const float* rest_positions, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri, const uint8_t* bone_indices, const uint8_t* bone_weights, uint32_t n_bones) {
    const std::string w(who);
    if (!rest_positions || !bone_indices || !bone_weights || n_vert == 0 || n_tri == 0) throw std::runtime_error(w + ": null or empty bind arrays");
    if (n_bones == 0 || n_bones > 256) throw std::runtime_error(w + ": n_bones must be 1..256");
    if (!indices && n_vert != n_tri * 3) throw std::runtime_error(w + ": triangle soup needs n_vert == 3*n_tri");
    if (indices) for (size_t i = 0; i < (size_t)n_tri * 3; i++) if (indices[i] >= n_vert) throw std::runtime_error(w + ": vertex index out of range");
    // under a zero weight too: d_Compute reads the matrix of every influence
    for (size_t i = 0; i < (size_t)n_vert * 8; i++) if (bone_indices[i] >= n_bones) throw std::runtime_error(w + ": bone index " + std::to_string(bone_indices[i]) + " of vertex " + std::to_string(i / 8) + " is not below n_bones");
}

void skin_check_pose(const char* who, const ctl_float4x4* bones0, const ctl_float4x4* bones1, uint32_t n_bones, float lerp) {
    const std::string w(who);
    if (!bones0) throw std::runtime_error(w + ": null bone matrices");
    if (!std::isfinite(lerp)) throw std::runtime_error(w + ": lerp is not finite");
    for (uint32_t b = 0; b < n_bones; b++) if (!finite16(bones0[b].m) || (bones1 && !finite16(bones1[b].m))) throw std::runtime_error(w + ": bone matrix " + std::to_string(b) + " has an entry that is not finite");
}

void skin_mesh_host(const ctl_scene_desc& d, uint32_t mesh, const float* rest_positions, const float* rest_normals, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                    const uint8_t* bone_indices, const uint8_t* bone_weights, uint32_t n_bones, const ctl_float4x4* bones0, const ctl_float4x4* bones1, float lerp,
                    float* positions_out, float* normals_out, ctl_triangle_data* tri_data_out, ctl_woop_tri* woop_out) {
    const char* who = "ctl_skin_mesh_host";
    if (mesh >= d.n_meshes) throw std::runtime_error("ctl_skin_mesh_host: bad mesh index");
    const mesh_ranges R(d);
    if (n_tri != R.tri1[mesh] - R.tri0[mesh]) throw std::runtime_error("ctl_skin_mesh_host: mesh " + std::to_string(mesh) + " has " + std::to_string(R.tri1[mesh] - R.tri0[mesh]) + " triangles; a skin keeps the triangle count");
    skin_check_arguments(who, rest_positions, n_vert, indices, n_tri, bone_indices, bone_weights, n_bones);
    skin_check_pose(who, bones0, bones1, n_bones, lerp);
    std::vector<f3> computed;
    if (!rest_normals) compute_vertex_normals(rest_positions, indices, n_vert, n_tri, computed);
    const float* b0 = bones0[0].m; const float* b1 = bones1 ? bones1[0].m : b0;
    std::vector<f3> P(n_vert), N(n_vert);
    for (uint32_t v = 0; v < n_vert; v++) {
        const f3 rp(rest_positions[3 * v], rest_positions[3 * v + 1], rest_positions[3 * v + 2]);
        const f3 rn = rest_normals ? f3(rest_normals[3 * v], rest_normals[3 * v + 1], rest_normals[3 * v + 2]) : computed[v];
        skin_vertex(b0, b1, lerp, rp, rn, bone_indices + (size_t)v * 8, bone_weights + (size_t)v * 8, P[v], N[v]);
        if (positions_out) { positions_out[3 * v] = P[v].x; positions_out[3 * v + 1] = P[v].y; positions_out[3 * v + 2] = P[v].z; }
        if (normals_out) { normals_out[3 * v] = N[v].x; normals_out[3 * v + 1] = N[v].y; normals_out[3 * v + 2] = N[v].z; }
    }
    auto vidx = [&](uint32_t t, int j) { return indices ? indices[(size_t)t * 3 + j] : t * 3 + (uint32_t)j; };
    if (tri_data_out) for (uint32_t t = 0; t < n_tri; t++) {
        uint32_t T[8]; std::memcpy(T, &d.tri_data[R.tri0[mesh] + t], 32);
        const f3 p[3] = { P[vidx(t, 0)], P[vidx(t, 1)], P[vidx(t, 2)] }, n[3] = { N[vidx(t, 0)], N[vidx(t, 1)], N[vidx(t, 2)] };
        skin_compile_triangle(T, p, n);
        std::memcpy(&tri_data_out[t], T, 32);
    }
    if (woop_out) for (uint32_t w = R.woop0[mesh]; w < R.woop1[mesh]; w++) {
        const size_t at = (size_t)d.meshes[mesh].bvh_index_offset + (w - R.woop0[mesh]);
        const uint32_t t = (at < d.n_woop ? d.woop_index[at].index : 1u) >> 1;   // the index word as the upload lays it next to the row (tracer.hip)
        ctl_woop_tri& o = woop_out[w - R.woop0[mesh]];
        o = d.woop[w];
        if (t >= n_tri) continue;
        float r[12];
        woop_rows_from_vertices(r, P[vidx(t, 0)], P[vidx(t, 1)], P[vidx(t, 2)]);
        std::memcpy(o.a, r, 16); std::memcpy(o.b, r + 4, 16); std::memcpy(o.c, r + 8, 16);
    }
}

void Scene::bind_skin(uint32_t mesh, const float* rest_positions, const float* rest_normals, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                      const uint8_t* bone_indices, const uint8_t* bone_weights, uint32_t n_bones, uint32_t flags) {
    require_device();
    const char* who = "ctl_scene_bind_skin";
    if (flags & ~(uint32_t)CTL_SKIN_AREA_LIGHTS) throw std::runtime_error("ctl_scene_bind_skin_ex: unknown CTL_SKIN_* bits");
    if (!snap_) throw std::runtime_error("ctl_scene_bind_skin: the scene holds no description");
    const ctl_scene_desc& d = snap_->d;
    if (mesh >= d.n_meshes) throw std::runtime_error("ctl_scene_bind_skin: bad mesh index");
    const mesh_ranges R(d);
    const uint32_t tri0 = R.tri0[mesh], tri1 = R.tri1[mesh], woop0 = R.woop0[mesh], woop1 = R.woop1[mesh];
    if (n_tri != tri1 - tri0) throw std::runtime_error("ctl_scene_bind_skin: mesh " + std::to_string(mesh) + " has " + std::to_string(tri1 - tri0) + " triangles; a skin keeps the triangle count");
    skin_check_arguments(who, rest_positions, n_vert, indices, n_tri, bone_indices, bone_weights, n_bones);
    if (!flattened() || S.flat_format != kFlatQ4 || refit_.level_start.size() < 2) throw unsupported_error("ctl_scene_bind_skin: needs a scene flattened in the CTL_FLAT_Q4 format with refit data (CTL_SCENE_FLATTEN)");
    if (!(flags & CTL_SKIN_AREA_LIGHTS)) for (uint32_t k = 0; k < d.n_nodes; k++) if (d.nodes[k].mesh_index == mesh && d.nodes[k].n_lights)
        throw unsupported_error("ctl_scene_bind_skin: node " + std::to_string(k) + " of mesh " + std::to_string(mesh) + " carries an area light, whose shape set is host work (ctl_builder_update_mesh)");
    for (uint32_t t : flat_missing_tris_) if (t >= tri0 && t < tri1)
        throw unsupported_error("ctl_scene_bind_skin: mesh " + std::to_string(mesh) + " has a triangle that was degenerate when the scene was flattened: the flattened tree has no leaf entry for it");
    if ((size_t)tri1 * 2 > tri_data_.n || (size_t)woop1 * 4 > leaf_tris_.n) throw std::runtime_error("ctl_scene_bind_skin: mesh " + std::to_string(mesh) + " reaches outside the scene's geometry arrays");
    std::vector<f3> computed;
    if (!rest_normals) compute_vertex_normals(rest_positions, indices, n_vert, n_tri, computed);   // Mesh::ComputeVertexNormals of the rest pose, once
    std::vector<float4> p4(n_vert), n4(n_vert); std::vector<uint4> bytes(n_vert);
    for (uint32_t v = 0; v < n_vert; v++) {
        p4[v] = make_float4(rest_positions[3 * v], rest_positions[3 * v + 1], rest_positions[3 * v + 2], 1.0f);
        n4[v] = rest_normals ? make_float4(rest_normals[3 * v], rest_normals[3 * v + 1], rest_normals[3 * v + 2], 0.0f) : make_float4(computed[v].x, computed[v].y, computed[v].z, 0.0f);
        std::memcpy(&bytes[v].x, bone_indices + (size_t)v * 8, 8); std::memcpy(&bytes[v].z, bone_weights + (size_t)v * 8, 8);
    }
    CTL_HIP(hipDeviceSynchronize());
    if (!refit_tri_row_.p) {
        // triangle -> row of the leaf stream (flatten.h triangle_woop_rows), from the index words the device holds next to the rows: the snapshot keeps no woop_index
        std::vector<uint32_t> words(d.n_woop), rows(d.n_tri_data, 0xffffffffu);
        if (d.n_woop) CTL_HIP(hipMemcpy2D(words.data(), 4, reinterpret_cast<const char*>(leaf_tris_.p) + 48, 64, 4, d.n_woop, hipMemcpyDeviceToHost));
        for (uint32_t m = 0; m < d.n_meshes; m++) for (uint32_t w = R.woop1[m]; w-- > R.woop0[m];) {   // backwards: the first reference in stream order stays
            if ((size_t)d.meshes[m].bvh_index_offset + (w - R.woop0[m]) >= d.n_woop) continue;   // no woop_index slot: the upload's filler word, which triangle_woop_rows skips too
            const uint64_t tri = (uint64_t)d.meshes[m].tri_offset + (words[w] >> 1);
            if (tri < d.n_tri_data) rows[tri] = w;
        }
        refit_tri_row_.upload(rows.data(), rows.size());
        CTL_HIP(hipStreamSynchronize(nullptr));
    }
    std::shared_ptr<skin_binding> B(new skin_binding());
    B->n_vert = n_vert; B->n_tri = n_tri; B->n_bones = n_bones; B->tri0 = tri0; B->woop0 = woop0; B->n_rows = woop1 - woop0; B->indexed = indices != nullptr;
    B->rest_p.upload(p4.data(), n_vert); B->rest_n.upload(n4.data(), n_vert); B->bone_bytes.upload(bytes.data(), n_vert);
    if (indices) B->indices.upload(indices, (size_t)n_tri * 3);
    B->skinned_p.alloc(n_vert); B->skinned_n.alloc(n_vert); B->bones.alloc((size_t)n_bones * 8);
    CTL_HIP(hipStreamSynchronize(nullptr));   // the staging vectors are pageable: the copies have left them
    if (flags & CTL_SKIN_AREA_LIGHTS) enable_skin_lights(mesh);   // its lights' shape sets follow every pose (shape_set.hip)
    else if (skin_lights_.erase(mesh)) lights_stale_ = true;     // bound again without the flag: the tables go back to the description's with the next update
    skins_[mesh] = B;
}

void Scene::unbind_skin(uint32_t mesh) {
    auto it = skins_.find(mesh);
    if (it == skins_.end()) throw std::runtime_error("ctl_scene_unbind_skin: mesh " + std::to_string(mesh) + " is not bound");
    CTL_HIP(hipDeviceSynchronize());
    skins_.erase(it);
    if (skin_lights_.erase(mesh)) lights_stale_ = true;   // the shape sets in HBM are the last pose's: the next ctl_scene_update uploads the description's light tables
    // the values the device holds are no description's: the next ctl_scene_update must see the mesh as changed and restore its description's values
    if (snap_) snap_->geom.invalidate_values(mesh);
}

void Scene::animate_mesh(uint32_t mesh, const ctl_float4x4* bones0, const ctl_float4x4* bones1, float lerp, ctl_scene_update_stats* stats) {
    auto it = skins_.find(mesh);
    if (it == skins_.end()) throw std::runtime_error("ctl_scene_animate_mesh: mesh " + std::to_string(mesh) + " is not bound (ctl_scene_bind_skin)");
    skin_binding& B = *it->second;
    skin_check_pose("ctl_scene_animate_mesh", bones0, bones1, B.n_bones, lerp);   // before the device is touched
    require_device();
    CTL_HIP(hipDeviceSynchronize());   // no trace reads the arrays any more
    const size_t pose_bytes = (size_t)B.n_bones * 64;
    CTL_HIP(hipMemcpy(B.bones.p, bones0, pose_bytes, hipMemcpyHostToDevice));
    CTL_HIP(hipMemcpy(B.bones.p + (size_t)B.n_bones * 4, bones1 ? bones1 : bones0, pose_bytes, hipMemcpyHostToDevice));
    skin_device K{};
    K.rest_p = B.rest_p.p; K.rest_n = B.rest_n.p; K.bone_bytes = B.bone_bytes.p; K.bones = B.bones.p; K.indices = B.indexed ? B.indices.p : nullptr;
    K.skinned_p = B.skinned_p.p; K.skinned_n = B.skinned_n.p; K.tri_data = tri_data_.p; K.leaf_tris = leaf_tris_.p;
    K.n_vert = B.n_vert; K.n_tri = B.n_tri; K.n_bones = B.n_bones; K.tri0 = B.tri0; K.woop0 = B.woop0; K.n_rows = B.n_rows; K.lerp = lerp;
    struct event_pair { hipEvent_t a = nullptr, b = nullptr; ~event_pair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } ev;
    CTL_HIP(hipEventCreate(&ev.a)); CTL_HIP(hipEventCreate(&ev.b));
    CTL_HIP(hipEventRecord(ev.a, nullptr));
    hipLaunchKernelGGL(k_skin_vertices, dim3((B.n_vert + 255u) / 256u), dim3(256), pose_bytes * 2, nullptr, K); CTL_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_compile_triangles, dim3((B.n_tri + 255u) / 256u), dim3(256), 0, nullptr, K); CTL_HIP(hipGetLastError());
    if (B.n_rows) { hipLaunchKernelGGL(k_woop_rows, dim3((B.n_rows + 255u) / 256u), dim3(256), 0, nullptr, K); CTL_HIP(hipGetLastError()); }
    CTL_HIP(hipEventRecord(ev.b, nullptr));
    B.posed = true;
    float shape_ms = 0;
    if (skin_lights_.count(mesh)) { run_shape_sets(snap_->d); shape_ms = last_shape_set_ms_; }   // the lights on the mesh's nodes, from the rows just written; before the refit
    // the flat-tree half, as after a CTL_DIFF_GEOMETRY update of this mesh: its nodes' entries take the new rows and become whole, the refit, the re-stamp
    std::vector<uint8_t> mesh_changed(snap_->d.n_meshes, 0); mesh_changed[mesh] = 1;
    ctl_scene_update_stats st{}; st.mask = CTL_DIFF_GEOMETRY;
    refit_flat(snap_->d, true, true, &mesh_changed, &st);   // ends with a device synchronisation
    st.restamped = 1u;
    float ms = 0; CTL_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
    last_skin_ms_ = ms; last_shape_set_ms_ = shape_ms; last_update_ = st; last_mask_ = st.mask;
    if (stats) *stats = st;
}

// ctl_scene_update_mesh_set removed meshes (flat_mesh_set.hip): the bindings under the new mesh indices, the offsets each one caches from the new description.  A bound mesh
// is never removed (plan_mesh_set), so every binding has a new index.  Here, because skin_binding is this file's
void flat_rebuilder::remap_skins(Scene& A, const mesh_compaction& cut, const ctl_scene_desc& d) {
    if (A.skins_.empty() && A.skin_lights_.empty()) return;
    const mesh_ranges R(d);
    std::map<uint32_t, std::shared_ptr<skin_binding>> skins;
    for (const auto& kv : A.skins_) {
        const uint32_t k = kv.first < cut.new_of_old.size() ? cut.new_of_old[kv.first] : kNodesNone;
        if (k == kNodesNone || k >= d.n_meshes) continue;
        kv.second->tri0 = R.tri0[k]; kv.second->woop0 = R.woop0[k];
        skins[k] = kv.second;
    }
    A.skins_.swap(skins);
    std::set<uint32_t> lights;
    for (uint32_t m : A.skin_lights_) { const uint32_t k = m < cut.new_of_old.size() ? cut.new_of_old[m] : kNodesNone; if (k != kNodesNone) lights.insert(k); }
    A.skin_lights_.swap(lights);
}

void Scene::read_mesh_geometry(uint32_t mesh, float* positions_out, float* normals_out, ctl_triangle_data* tri_data_out, ctl_woop_tri* woop_out) {
    require_device();
    if (!snap_ || mesh >= snap_->d.n_meshes) throw std::runtime_error("ctl_scene_read_mesh_geometry: bad mesh index");
    CTL_HIP(hipDeviceSynchronize());
    if (positions_out || normals_out) {
        auto it = skins_.find(mesh);
        if (it == skins_.end() || !it->second->posed) throw std::runtime_error("ctl_scene_read_mesh_geometry: mesh " + std::to_string(mesh) + " holds no pose (ctl_scene_bind_skin, ctl_scene_animate_mesh)");
        const skin_binding& B = *it->second;
        std::vector<float4> tmp(B.n_vert);
        for (int pass = 0; pass < 2; pass++) {
            float* out = pass ? normals_out : positions_out;
            if (!out) continue;
            CTL_HIP(hipMemcpy(tmp.data(), pass ? B.skinned_n.p : B.skinned_p.p, (size_t)B.n_vert * 16, hipMemcpyDeviceToHost));
            for (uint32_t v = 0; v < B.n_vert; v++) { out[3 * v] = tmp[v].x; out[3 * v + 1] = tmp[v].y; out[3 * v + 2] = tmp[v].z; }
        }
    }
    const mesh_ranges R(snap_->d);
    const uint32_t tri0 = R.tri0[mesh], tri1 = R.tri1[mesh], woop0 = R.woop0[mesh], woop1 = R.woop1[mesh];
    if ((size_t)tri1 * 2 > tri_data_.n || (size_t)woop1 * 4 > leaf_tris_.n) throw std::runtime_error("ctl_scene_read_mesh_geometry: mesh " + std::to_string(mesh) + " reaches outside the scene's geometry arrays");
    if (tri_data_out && tri1 > tri0) CTL_HIP(hipMemcpy(tri_data_out, tri_data_.p + (size_t)tri0 * 2, (size_t)(tri1 - tri0) * 32, hipMemcpyDeviceToHost));
    if (woop_out && woop1 > woop0) {
        std::vector<float4> tmp((size_t)(woop1 - woop0) * 4);
        CTL_HIP(hipMemcpy(tmp.data(), leaf_tris_.p + (size_t)woop0 * 4, tmp.size() * 16, hipMemcpyDeviceToHost));
        for (uint32_t w = 0; w < woop1 - woop0; w++) std::memcpy(&woop_out[w], &tmp[(size_t)w * 4], 48);
    }
}

}  // namespace ctl
