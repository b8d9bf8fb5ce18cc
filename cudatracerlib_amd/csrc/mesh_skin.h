// mesh_skin.h — a bound mesh posed from bone matrices (ctl_scene_animate_mesh): the arithmetic, single source for the host yardstick (ctl_skin_mesh_host) and
// the device (mesh_skin.hip), in the style of flat_refit.h.  What the reference's AnimatedMesh::k_ComputeState does on the device (Engine/AnimatedMesh.cu
// g_ComputeVertices / g_ComputeTriangles) plus what its host side does afterwards (TriangleData::setData, TriIntersectorData::setData per leaf reference).
//
// Arithmetic: fp32 +, -, *, /, sqrt, conversions and bit manipulation, evaluated in the order written (the library is built -ffp-contract=off on both sides), and
// the transcendental functions of the normal codec through ctl_fmath.h on BOTH sides (skin_normal_code), so the host's bits are the device's bits.
//
// The restatements of the scene builder that a pose needs live here too, once: float4x4::inverse, TriIntersectorData::setData, TriangleData::setData.  The builder
// (scene_builder.cpp) calls the same functions, with libm's acos / atan2 in the normal codec as before (its arrays are pinned on the reference's glibc results).
#pragma once
#include "../../include/ctl_amd.h"
#include "ctl_math.h"
#include <cstring>

namespace ctl {

// float4x4::inverse (Math/float4x4.h:132-193) — cofactor expansion in the reference's expression order
HD void mat4_inverse(const float* Q, float* out) {
#define M(i, j) Q[(i) * 4 + (j)]
    float m00 = M(0, 0), m01 = M(0, 1), m02 = M(0, 2), m03 = M(0, 3), m10 = M(1, 0), m11 = M(1, 1), m12 = M(1, 2), m13 = M(1, 3);
    float m20 = M(2, 0), m21 = M(2, 1), m22 = M(2, 2), m23 = M(2, 3), m30 = M(3, 0), m31 = M(3, 1), m32 = M(3, 2), m33 = M(3, 3);
#undef M
    float v0 = m20 * m31 - m21 * m30, v1 = m20 * m32 - m22 * m30, v2 = m20 * m33 - m23 * m30;
    float v3 = m21 * m32 - m22 * m31, v4 = m21 * m33 - m23 * m31, v5 = m22 * m33 - m23 * m32;
    float t00 = +(v5 * m11 - v4 * m12 + v3 * m13), t10 = -(v5 * m10 - v2 * m12 + v1 * m13);
    float t20 = +(v4 * m10 - v2 * m11 + v0 * m13), t30 = -(v3 * m10 - v1 * m11 + v0 * m12);
    float invDet = 1 / (t00 * m00 + t10 * m01 + t20 * m02 + t30 * m03);
    float d00 = t00 * invDet, d10 = t10 * invDet, d20 = t20 * invDet, d30 = t30 * invDet;
    float d01 = -(v5 * m01 - v4 * m02 + v3 * m03) * invDet, d11 = +(v5 * m00 - v2 * m02 + v1 * m03) * invDet;
    float d21 = -(v4 * m00 - v2 * m01 + v0 * m03) * invDet, d31 = +(v3 * m00 - v1 * m01 + v0 * m02) * invDet;
    v0 = m10 * m31 - m11 * m30; v1 = m10 * m32 - m12 * m30; v2 = m10 * m33 - m13 * m30;
    v3 = m11 * m32 - m12 * m31; v4 = m11 * m33 - m13 * m31; v5 = m12 * m33 - m13 * m32;
    float d02 = +(v5 * m01 - v4 * m02 + v3 * m03) * invDet, d12 = -(v5 * m00 - v2 * m02 + v1 * m03) * invDet;
    float d22 = +(v4 * m00 - v2 * m01 + v0 * m03) * invDet, d32 = -(v3 * m00 - v1 * m01 + v0 * m02) * invDet;
    v0 = m21 * m10 - m20 * m11; v1 = m22 * m10 - m20 * m12; v2 = m23 * m10 - m20 * m13;
    v3 = m22 * m11 - m21 * m12; v4 = m23 * m11 - m21 * m13; v5 = m23 * m12 - m22 * m13;
    float d03 = -(v5 * m01 - v4 * m02 + v3 * m03) * invDet, d13 = +(v5 * m00 - v2 * m02 + v1 * m03) * invDet;
    float d23 = -(v4 * m00 - v2 * m01 + v0 * m03) * invDet, d33 = +(v3 * m00 - v1 * m01 + v0 * m02) * invDet;
    out[0] = d00; out[1] = d01; out[2] = d02; out[3] = d03; out[4] = d10; out[5] = d11; out[6] = d12; out[7] = d13;
    out[8] = d20; out[9] = d21; out[10] = d22; out[11] = d23; out[12] = d30; out[13] = d31; out[14] = d32; out[15] = d33;
}

// Woop rows from the three vertices (Engine/TriIntersectorData.cu:5-18): rows[0..3] = a, rows[4..7] = b, rows[8..11] = c of ctl_woop_tri
HD void woop_rows_from_vertices(float rows[12], f3 a, f3 b, f3 c) {
    f3 e0 = a - c, e1 = b - c, n = cross(a - c, b - c);
    float m[16] = { e0.x, e1.x, n.x, c.x, e0.y, e1.y, n.y, c.y, e0.z, e1.z, n.z, c.z, 0, 0, 0, 1 }, inv[16];
    mat4_inverse(m, inv);
    rows[0] = inv[8]; rows[1] = inv[9]; rows[2] = inv[10]; rows[3] = -inv[11];
    for (int j = 0; j < 4; j++) { rows[4 + j] = inv[j]; rows[8 + j] = inv[4 + j]; }
}

// the 8+8 bit normal codec (Math/Compression.h:12-31) with the shared fp32 acos / atan2 on the host AND the device: what a pose encodes with.  (normal_to_uchar2 of
// ctl_math.h is the same expression over m_acos / m_atan2, which on the host are libm's.)  The codec's float -> unsigned short conversions are undefined for a NaN —
// the normal of a vertex whose bones all have zero scale normalises to one — and host and device compilers need not agree there, so that case is spelled out: 0, which
// is what the x86 conversion the builder's arrays come from leaves in the low 16 bits.  Every angle of a real normal is in [0, 255] and converts as before.
HD uint32_t skin_code_byte(float a) { return (a >= 0.0f && a < 65536.0f) ? (uint32_t)a : 0u; }
HD uint16_t skin_normal_code(f3 v) {
    float theta = (fm::acos(v.z) * (255.0f / kPi));
    float phi = (fm::atan2(v.y, v.x) * (255.0f / (2.0f * kPi)));
    phi = phi < 0 ? (phi + 255) : phi;
    return (uint16_t)((skin_code_byte(theta) << 8) | skin_code_byte(phi));
}

// TriangleData::setUvSetData + setData (Engine/TriangleData.cu:18-65) for uv words that are already half-rounded (uv[i] = half(u) | half(v) << 16: what setUvSetData
// stores and setData reads back) and a material byte.  SHARED_CODEC: skin_normal_code instead of normal_to_uchar2.  T = the eight words of a ctl_triangle_data (nor_mat_extra, dpdu_dpdv, uv).
template <bool SHARED_CODEC> HD void tri_data_words(uint32_t T[8], const f3 p[3], const f3 n[3], const uint32_t uv[3], uint32_t mat_index) {
    const f2 t0{ half_to_float((uint16_t)uv[0]), half_to_float((uint16_t)(uv[0] >> 16)) }, t1{ half_to_float((uint16_t)uv[1]), half_to_float((uint16_t)(uv[1] >> 16)) },
             t2{ half_to_float((uint16_t)uv[2]), half_to_float((uint16_t)(uv[2] >> 16)) };
    f3 dP1 = p[1] - p[0], dP2 = p[2] - p[0];
    f2 dUV1{ t1.x - t0.x, t1.y - t0.y }, dUV2{ t2.x - t0.x, t2.y - t0.y };
    float determinant = dUV1.x * dUV2.y - dUV1.y * dUV2.x;
    f3 dpdu, dpdv;
    if (determinant == 0) { f3 a, b, nn = normalize(cross(dP1, dP2)); coordinate_system(nn, a, b); dpdu = a; dpdv = b; }
    else {
        float invDet = 1.0f / determinant;
        dpdu = ((dUV2.y * dP1 - dUV1.y * dP2) * invDet);
        dpdv = ((-dUV2.x * dP1 + dUV1.x * dP2) * invDet);
    }
    uint32_t ax = float_to_half(dpdu.x), ay = float_to_half(dpdu.y), az = float_to_half(dpdu.z);
    uint32_t bx = float_to_half(dpdv.x), by = float_to_half(dpdv.y), bz = float_to_half(dpdv.z);
    uint32_t c[3];
    for (int i = 0; i < 3; i++) c[i] = SHARED_CODEC ? (uint32_t)skin_normal_code(n[i]) : (uint32_t)normal_to_uchar2(n[i]);
    T[0] = c[0] | (c[1] << 16); T[1] = c[2] | ((mat_index & 0xff) << 16);        // nor_mat_extra
    T[2] = ax | (ay << 16); T[3] = az | (bx << 16); T[4] = by | (bz << 16);      // dpdu_dpdv
    T[5] = uv[0]; T[6] = uv[1]; T[7] = uv[2];                                    // uv
}

// ---- skinning: Engine/AnimatedMesh.cu

// d_Compute (AnimatedMesh.cu:13-28): mat.zeros(), then for the eight influences in byte order m = M[j] * w (float4x4 * float, float4x4.h:384-396: element * w),
// mat = mat + m (float4x4.h:347-354), w = byte / 255.0f.  All eight are summed, a zero weight included.  bones: row-major, 16 floats per bone.
template <typename P> HD void skin_blend_matrix(P bones, const uint8_t idx[8], const uint8_t wgt[8], float mat[16]) {
    for (int e = 0; e < 16; e++) mat[e] = 0.0f;
    for (int i = 0; i < 8; i++) {
        const uint32_t j = idx[i];
        const float w = (float)(int)wgt[i] / 255.0f;
        for (int e = 0; e < 16; e++) { const float m = bones[j * 16u + e] * w; mat[e] = mat[e] + m; }
    }
}
// float4x4 * Vec4f (float4x4.h:374-382): dot(row, v) with Vector.h:97's accumulation r = 0; r += a[i] * b[i]
HD float skin_row_dot(const float* row, f3 v, float w) { float r = 0.0f; r += row[0] * v.x; r += row[1] * v.y; r += row[2] * v.z; r += row[3] * w; return r; }
// float4x4::TransformPoint (float4x4.h:398-402): f = M * (p, 1); f.xyz / f.w — a true division per component (Vector.h:88); blended weights need not sum to one
HD f3 skin_transform_point(const float mat[16], f3 p) {
    const float x = skin_row_dot(mat, p, 1.0f), y = skin_row_dot(mat + 4, p, 1.0f), z = skin_row_dot(mat + 8, p, 1.0f), w = skin_row_dot(mat + 12, p, 1.0f);
    return f3(x / w, y / w, z / w);
}
// float4x4::TransformDirection (float4x4.h:404-408): (M * (d, 0)).xyz
HD f3 skin_transform_direction(const float mat[16], f3 d) { return f3(skin_row_dot(mat, d, 0.0f), skin_row_dot(mat + 4, d, 0.0f), skin_row_dot(mat + 8, d, 0.0f)); }
// math::lerp<Vec3f, float> (MathFunc.h:161): a * (1 - t) + b * t
HD f3 skin_lerp(f3 a, f3 b, float t) { const float s = 1.0f - t; return f3(a.x * s + b.x * t, a.y * s + b.y * t, a.z * s + b.z * t); }
// normalize (Vector.h:369-376): v * math::rcp(length), rcp(a) = a ? 1 / a : 0 (MathFunc.h:399); lenSqr accumulates from 0 (Vector.h:46)
HD f3 skin_normalize(f3 v) {
    float l2 = 0.0f; l2 += v.x * v.x; l2 += v.y * v.y; l2 += v.z * v.z;
    const float l = sqrtf(l2), r = (l != 0.0f) ? 1.0f / l : 0.0f;
    return f3(v.x * r, v.y * r, v.z * r);
}
// g_ComputeVertices (AnimatedMesh.cu:30-44) of one vertex
template <typename P> HD void skin_vertex(P bones0, P bones1, float lerp, f3 rest_p, f3 rest_n, const uint8_t idx[8], const uint8_t wgt[8], f3& p_out, f3& n_out) {
    float mat0[16], mat1[16];
    skin_blend_matrix(bones0, idx, wgt, mat0);
    skin_blend_matrix(bones1, idx, wgt, mat1);
    const f3 v0 = skin_transform_point(mat0, rest_p), v1 = skin_transform_point(mat1, rest_p);
    p_out = skin_lerp(v0, v1, lerp);
    const f3 n0 = skin_transform_direction(mat0, rest_n), n1 = skin_transform_direction(mat1, rest_n);
    n_out = skin_normalize(skin_lerp(n0, n1, lerp));
}
// One triangle of the posed mesh: what compile_triangles (scene_builder.cpp; Mesh::CompileMesh, Engine/Mesh.cpp:225-272) makes of caller-supplied positions and normals —
// the normals normalised once more, as it does to any normals it is handed — with the triangle's uv words and material byte kept (T holds the old words on entry).
HD void skin_compile_triangle(uint32_t T[8], const f3 p[3], const f3 n_in[3]) {
    const uint32_t uv[3] = { T[5], T[6], T[7] }, mat = (T[1] >> 16) & 0xffu;
    const f3 n[3] = { normalize(n_in[0]), normalize(n_in[1]), normalize(n_in[2]) };
    tri_data_words<true>(T, p, n, uv, mat);
}

// Host yardstick (mesh_skin.hip, no device call): the pose of one mesh of `d` on the host with the functions above.  indices == nullptr: a soup.  Outputs may be null.
void skin_mesh_host(const ctl_scene_desc& d, uint32_t mesh, const float* rest_positions, const float* rest_normals, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri,
                    const uint8_t* bone_indices, const uint8_t* bone_weights, uint32_t n_bones, const ctl_float4x4* bones0, const ctl_float4x4* bones1, float lerp,
                    float* positions_out, float* normals_out, ctl_triangle_data* tri_data_out, ctl_woop_tri* woop_out);
// the argument checks ctl_scene_bind_skin and ctl_skin_mesh_host share (std::runtime_error): everything that can be judged without the scene
void skin_check_arguments(const char* who, const float* rest_positions, uint32_t n_vert, const uint32_t* indices, uint32_t n_tri, const uint8_t* bone_indices, const uint8_t* bone_weights, uint32_t n_bones);
void skin_check_pose(const char* who, const ctl_float4x4* bones0, const ctl_float4x4* bones1, uint32_t n_bones, float lerp);

}  // namespace ctl
