// shape_set.h — the shape set of an area light (ShapeSet::Recalculate, Engine/ShapeSet.cpp:17-59; triData::Recalculate, Engine/ShapeSet.cu:11-23): the arithmetic,
// single source for the scene builder (scene_builder::recalculate_shape_set), the host yardstick (ctl_shape_sets_host) and the device (shape_set.hip), in the style of
// mesh_skin.h.  fp32 +, -, *, /, sqrt in the order written (the library is built -ffp-contract=off on both sides).
//
// The one step that is not plain arithmetic is the decode of the 8+8 bit normal codes (uchar2_to_normal, ctl_math.h): the builder's arrays are pinned on libm's sinf / cosf,
// the device's decode runs ctl_fmath.h's.  So the decode is a parameter: the host hands in uchar2_to_normal itself, the device a lookup in shape_normal_lut — the 2 x 256
// (sin, cos) pairs that the HOST's uchar2_to_normal multiplies, filled on the host and uploaded — and the products are the same products.
#pragma once
#include "mesh_skin.h"

namespace ctl {

// TriIntersectorData::getData (Engine/TriIntersectorData.cu:20-32): the vertices back from the Woop rows a, b, c of a ctl_woop_tri — area lights take theirs from this round trip
HD void woop_get_data(const float* a, const float* b, const float* c, f3& v0, f3& v1, f3& v2) {
    float m[16] = { b[0], b[1], b[2], b[3], c[0], c[1], c[2], c[3], a[0], a[1], a[2], a[3] * -1.0f, 0, 0, 0, 1 }, inv[16];
    mat4_inverse(m, inv);
    f3 e02(inv[0], inv[4], inv[8]), e12(inv[1], inv[5], inv[9]);
    v2 = f3(inv[3], inv[7], inv[11]);
    v0 = v2 + e02; v1 = v2 + e12;
}

// shading normal of a triangle at barycentrics (1/3,1/3) under `l2w` — the dg.sys.n of TriangleData::fillDG (Engine/TriangleData.cu:75-103), used for ShapeSet::triData::n.
// T = the eight words of a ctl_triangle_data; decode(code) = the unit vector of a 16-bit normal code
template <typename DEC> HD f3 tri_data_center_normal(const uint32_t* T, const m34& l2w, DEC decode) {
    f3 na = decode(T[0] & 0xffff), nb = decode(T[0] >> 16), nc = decode(T[1] & 0xffff);
    float u = 1.0f / 3.0f, v = 1.0f / 3.0f, w = 1.0f - u - v;
    f3 n = normalize(u * na + v * nb + w * nc);
    f3 dpdu(half_to_float((uint16_t)T[2]), half_to_float((uint16_t)(T[2] >> 16)), half_to_float((uint16_t)T[3]));
    f3 s = dpdu - n * dot(n, dpdu);
    f3 t = cross(s, n);
    s = xform_dir(l2w, s); t = xform_dir(l2w, t);
    return normalize(cross(t, s));
}

// one triangle of a shape set: world-space corners, normal and area from its Woop rows, its TriangleData words and the node's forward transform
template <typename DEC> HD void shape_triangle(const float* a, const float* b, const float* c, const uint32_t* T, const m34& l2w, DEC decode, f3 p[3], f3& n, float& area) {
    woop_get_data(a, b, c, p[0], p[1], p[2]);
    n = tri_data_center_normal(T, l2w, decode);
    for (int k = 0; k < 3; k++) p[k] = xform_point(l2w, p[k]);
    area = 0.5f * length(cross(p[2] - p[0], p[1] - p[0]));
}

// the tables the device decodes with: lut[x] = (sin, cos) of theta of byte x, lut[256 + y] those of phi of byte y, made by the host's own m_sin / m_cos, angle for angle what
// the host's uchar2_to_normal evaluates
inline void shape_normal_lut(float* out /* 512 x {sin, cos} */) {
    const float PI_4 = kPi / 4.0f, PI_2 = kPi / 2.0f;
    for (uint32_t x = 0; x < 256; x++) {
        const float theta = x == 63 ? PI_4 : (x == 127 ? PI_2 : (x == 191 ? 3 * PI_4 : float(x) * (1.0f / 255.0f) * kPi));
        const float phi = x == 63 ? PI_2 : (x == 127 ? kPi : (x == 191 ? 3 * PI_2 : float(x) * (1.0f / 255.0f) * kPi * 2.0f));
        out[2 * x] = m_sin(theta); out[2 * x + 1] = m_cos(theta);
        out[2 * (256 + x)] = m_sin(phi); out[2 * (256 + x) + 1] = m_cos(phi);
    }
}

// Host yardstick (shape_set.hip, no device call; ctl_shape_sets_host): d's light table and anim blob copied into lights_out[d.n_lights_buf] / anim_out[d.n_anim_bytes], with the
// shape sets of the diffuse lights on nodes that instance `mesh` recalculated from the given arrays — tri_data / woop: the mesh's ranges, as ctl_skin_mesh_host returns them —
// and d's node transforms
void shape_sets_host(const ctl_scene_desc& d, uint32_t mesh, const ctl_triangle_data* tri_data, const ctl_woop_tri* woop, ctl_light* lights_out, uint8_t* anim_out);
// is light `li` of `d` one whose shape set a pose of `mesh` changes: a diffuse light with triangles on a node that instances the mesh, its tables inside the anim blob
bool shape_set_of_mesh(const ctl_scene_desc& d, uint32_t li, uint32_t mesh);

}  // namespace ctl
