// flat_refit.h — refit of the flattened Q4 tree (flatten.h) to new node transforms: the arithmetic, single source for the host (flatten.cpp
// refit_flat_scene, what ctl_flat_bvh_refit runs) and the device (flat_refit.hip, what ctl_scene_update runs).
//
// The tree only culls (flatten.h), so a refit has to keep one property: every box contains what lies under it.  Links, masks and memory order stay
// as built; per leaf entry the instance's inverse transform is rewritten and a new world-space box is made, per node — deepest level first — the
// child boxes are re-quantised against the node's new own box.
//
// Arithmetic: IEEE double / float +, -, *, /, conversions and bit manipulation only, evaluated in the order written (the library is built
// -ffp-contract=off on both sides), so the host's bits are the device's bits — the style of ctl_fmath.h.  An entry's world-space vertices are made
// the way flatten.cpp makes them: the Woop matrix inverted in double, the vertices carried through the node's to_world in double, rounded outwards,
// padded by 8 ulp of the magnitudes involved.
//
// Side data (flat_scene::refit, made once by flatten_scene):
//   part_index[entry]   0xffffffff: the entry stands for its whole triangle; else an index into part_boxes — the entry is a split reference
//                       (early split clipping) and part_boxes[] is the world-space clip box of its part AT CREATION
//   xf0[node]           the node transforms at creation: a part box is carried to the new pose through P = M_new * M_0^-1 (eight corners) and
//                       intersected with the whole triangle's new box.  Always from the creation pose: a refit never reads what an earlier one wrote,
//                       so refitting twice to the same transforms gives the same bytes
//   level_start / level_nodes   node ids grouped by depth (CSR); children come later in memory than their parent, but below the breadth-first top
//                       the order is depth-first clusters, so a level is a list, not an index range
//
// Oriented slabs (flat_slab.h): a refit NEUTRALISES the slab of every node that carries one — direction 0, an interval that no ray leaves — so the
// slab flag in the parent's link stays true and the culling stays conservative; the boxes alone cull afterwards.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define CTL_REFIT_HD __host__ __device__ inline
#else
#define CTL_REFIT_HD inline
#endif

namespace ctl {

struct refit_box { float lo[3], hi[3]; };   // 24 B

constexpr float kRefitBig = 3.402823466e+38f;
constexpr uint32_t kRefitNoPart = 0xffffffffu;
// the neutral slab: n = (0, 0, 0), step = 2^39, base = -2^40.  slab_setup then gives s = r = 0, 1 / r = 2^80 (the guarded reciprocal), entry distance
// (base - pad) * 2^80 = -2^120 and exit distance (255 * 2^39 + base + pad) * 2^80 = 253 * 2^119 for codes 0 .. 255: every ray interval lies inside
constexpr uint32_t kRefitNeutralSlabN = 0x53000000u;     // bits of 2^39f: the normal's 18 bits are zero
constexpr uint32_t kRefitNeutralSlabBase = 0xd3800000u;  // bits of -2^40f

CTL_REFIT_HD float refit_u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
CTL_REFIT_HD uint32_t refit_f2u(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
CTL_REFIT_HD float refit_next_down(float f) { uint32_t b = refit_f2u(f); if (f > 0.0f) b--; else if (f < 0.0f) b++; else b = 0x80000001u; return refit_u2f(b); }
CTL_REFIT_HD float refit_next_up(float f) { uint32_t b = refit_f2u(f); if (f > 0.0f) b++; else if (f < 0.0f) b--; else b = 0x00000001u; return refit_u2f(b); }
CTL_REFIT_HD float refit_round_down(double x) { const float f = (float)x; return ((double)f > x) ? refit_next_down(f) : f; }
CTL_REFIT_HD float refit_round_up(double x) { const float f = (float)x; return ((double)f < x) ? refit_next_up(f) : f; }
CTL_REFIT_HD float refit_fabs(float x) { return x < 0.0f ? -x : x; }
CTL_REFIT_HD double refit_dabs(double x) { return x < 0.0 ? -x : x; }
CTL_REFIT_HD float refit_max(float a, float b) { return a > b ? a : b; }
CTL_REFIT_HD float refit_min(float a, float b) { return a < b ? a : b; }

// 4x4 inverse in double by cofactors (flatten.cpp inv4, same expressions)
CTL_REFIT_HD bool refit_inv4(const double m[16], double out[16]) {
    double inv[16];
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    const double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    if (det == 0.0 || !(det - det == 0.0)) return false;   // zero, infinite or NaN
    const double id = 1.0 / det;
    for (int i = 0; i < 16; i++) out[i] = inv[i] * id;
    return true;
}

// P = M_new * M_0^-1 of one node (rows 0..2 of an affine matrix, double); false when M_0 cannot be inverted (the builder refuses such a node)
CTL_REFIT_HD bool refit_carry_matrix(const float m_new[16], const float m_0[16], double P[12]) {
    double a[16], ia[16];
    for (int i = 0; i < 16; i++) a[i] = (double)m_0[i];
    if (!refit_inv4(a, ia)) return false;
    for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) {
        double s = 0.0;
        for (int k = 0; k < 4; k++) s = s + (double)m_new[r * 4 + k] * ia[k * 4 + c];
        P[r * 4 + c] = s;
    }
    return true;
}

// The new world-space box of one leaf entry.  wa / wb / wc: its Woop rows (object space, unchanged); M: the node's new to_world (row-major, 12 or 16 floats);
// part0 / P: the entry's clip box at creation and its node's carry matrix, or nullptr for an entry that stands for its whole triangle.
// An entry whose Woop matrix cannot be inverted (the builder drops those) gets an inverted box.
CTL_REFIT_HD void refit_entry_box(const float wa[4], const float wb[4], const float wc[4], const float* M, const refit_box* part0, const double* P, refit_box& out) {
    // vertices of the Woop triangle (TriIntersectorData::getData), as flatten.cpp woop_vertices
    const double wm[16] = { (double)wb[0], (double)wb[1], (double)wb[2], (double)wb[3], (double)wc[0], (double)wc[1], (double)wc[2], (double)wc[3],
                            (double)wa[0], (double)wa[1], (double)wa[2], -(double)wa[3], 0.0, 0.0, 0.0, 1.0 };
    double inv[16];
    if (!refit_inv4(wm, inv)) { for (int r = 0; r < 3; r++) { out.lo[r] = kRefitBig; out.hi[r] = -kRefitBig; } return; }
    double v[3][3];
    for (int k = 0; k < 3; k++) { v[2][k] = inv[k * 4 + 3]; v[0][k] = v[2][k] + inv[k * 4 + 0]; v[1][k] = v[2][k] + inv[k * 4 + 1]; }
    refit_box b;
    for (int r = 0; r < 3; r++) { b.lo[r] = kRefitBig; b.hi[r] = -kRefitBig; }
    for (int j = 0; j < 3; j++) for (int r = 0; r < 3; r++) {
        const double w = (double)M[r * 4] * v[j][0] + (double)M[r * 4 + 1] * v[j][1] + (double)M[r * 4 + 2] * v[j][2] + (double)M[r * 4 + 3];
        const float lo = refit_round_down(w), hi = refit_round_up(w);
        if (lo < b.lo[r]) b.lo[r] = lo;
        if (hi > b.hi[r]) b.hi[r] = hi;
    }
    // the padding of flatten.cpp: 8 ulp of the box's largest coordinate, of its extent and of the object-space magnitude carried through the instance (woop_slack)
    double vm = 0.0, rs = 0.0;
    for (int j = 0; j < 3; j++) for (int k = 0; k < 3; k++) { const double x = refit_dabs(v[j][k]); if (x > vm) vm = x; }
    for (int r = 0; r < 3; r++) { const double x = refit_dabs((double)M[r * 4]) + refit_dabs((double)M[r * 4 + 1]) + refit_dabs((double)M[r * 4 + 2]); if (x > rs) rs = x; }
    const float off = (float)(vm * rs);
    float pad[3];
    for (int r = 0; r < 3; r++) {
        const float mag = refit_max(refit_max(refit_max(refit_fabs(b.lo[r]), refit_fabs(b.hi[r])), b.hi[r] - b.lo[r]), off);
        const float t = mag * 9.5367431640625e-7f;
        pad[r] = t + 1e-30f;
    }
    if (!part0) { for (int r = 0; r < 3; r++) { out.lo[r] = b.lo[r] - pad[r]; out.hi[r] = b.hi[r] + pad[r]; } return; }
    // a split reference: the creation clip box through P, eight corners; padded like the whole triangle and kept inside the whole triangle's padded box
    double plo[3] = { 1e300, 1e300, 1e300 }, phi[3] = { -1e300, -1e300, -1e300 };
    for (int c = 0; c < 8; c++) {
        const double x = (double)((c & 1) ? part0->hi[0] : part0->lo[0]), y = (double)((c & 2) ? part0->hi[1] : part0->lo[1]), z = (double)((c & 4) ? part0->hi[2] : part0->lo[2]);
        for (int r = 0; r < 3; r++) {
            const double w = P[r * 4] * x + P[r * 4 + 1] * y + P[r * 4 + 2] * z + P[r * 4 + 3];
            if (w < plo[r]) plo[r] = w;
            if (w > phi[r]) phi[r] = w;
        }
    }
    for (int r = 0; r < 3; r++) {
        const float lo = refit_round_down(plo[r]) - pad[r], hi = refit_round_up(phi[r]) + pad[r];
        out.lo[r] = refit_max(b.lo[r] - pad[r], lo); out.hi[r] = refit_min(b.hi[r] + pad[r], hi);
    }
}

// One node: cb[c] = the new box of every child that exists (bit c of `exist`).  Rewrites origin, the three step exponents and the six code words the way
// flatten.cpp chooses them — origin = the node's own box's low corner, 2^(e - 127) the smallest power of two (strictly) above extent / 255, codes
// rounded outwards, also under the fp32 evaluation origin + step * code — and returns the node's own box.  Slots without a child keep lo = 255, hi = 0, and so
// does a child whose box is inverted.
// words[0..9]: origin x y z, meta (e x, e y, e z, mask), qlo_x, qhi_x, qlo_y, qhi_y, qlo_z, qhi_z.
CTL_REFIT_HD void refit_node_boxes(uint32_t words[10], uint32_t exist, const refit_box cb[4], refit_box& own) {
    for (int r = 0; r < 3; r++) { own.lo[r] = kRefitBig; own.hi[r] = -kRefitBig; }
    for (int c = 0; c < 4; c++) if ((exist >> c) & 1u) for (int r = 0; r < 3; r++) {
        if (cb[c].lo[r] < own.lo[r]) own.lo[r] = cb[c].lo[r];
        if (cb[c].hi[r] > own.hi[r]) own.hi[r] = cb[c].hi[r];
    }
    // a child with an inverted box — a leaf slot whose entries all collapsed (singular Woop matrices after a geometry update), a node under which nothing is left — keeps
    // the codes of a missing child on every axis: nothing reaches it, and its +-kRefitBig never enters the conversions below
    uint32_t empty = 0u;
    for (int c = 0; c < 4; c++) if ((exist >> c) & 1u) for (int r = 0; r < 3; r++) if (!(cb[c].lo[r] <= cb[c].hi[r])) empty |= 1u << c;
    uint32_t meta = words[3] & 0xff000000u;
    for (int k = 0; k < 3; k++) {
        const float origin = own.lo[k];
        words[k] = refit_f2u(origin);
        const double ext = (double)own.hi[k] - (double)origin;
        int e = 1;
        if (ext > 0.0) {
            const double q = ext / 255.0;
            uint64_t qb; memcpy(&qb, &q, 8);
            e = (int)((qb >> 52) & 0x7ffu) - 1022 + 127;   // frexp's exponent: 2^(e - 127) > q
            if (e < 1) e = 1;
            if (e > 254) e = 254;
        }
        meta |= (uint32_t)e << (8 * k);
        const uint64_t sb = (uint64_t)(e - 127 + 1023) << 52, ib = (uint64_t)(127 - e + 1023) << 52;
        double step, istep; memcpy(&step, &sb, 8); memcpy(&istep, &ib, 8);
        uint32_t wlo = 0u, whi = 0u;
        for (int c = 0; c < 4; c++) {
            long long lo = 255, hi = 0;
            if (((exist >> c) & 1u) && !((empty >> c) & 1u)) {
                const double dl = ((double)cb[c].lo[k] - (double)origin) * istep, dh = ((double)cb[c].hi[k] - (double)origin) * istep;
                lo = (long long)dl; if ((double)lo > dl) lo--;        // floor
                hi = (long long)dh; if ((double)hi < dh) hi++;        // ceil
                if (lo > 255) lo = 255;
                if (hi < 0) hi = 0;
                while (lo > 0 && (float)((double)origin + step * (double)lo) > cb[c].lo[k]) lo--;
                while (hi < 255 && (float)((double)origin + step * (double)hi) < cb[c].hi[k]) hi++;
                if (lo < 0) lo = 0;
                if (hi > 255) hi = 255;
            }
            wlo |= (uint32_t)lo << (8 * c); whi |= (uint32_t)hi << (8 * c);
        }
        words[4 + 2 * k] = wlo; words[5 + 2 * k] = whi;
    }
    words[3] = meta;
}

// box of child c as the traversal decodes it (flatten.h:32), for the surface-area report
CTL_REFIT_HD double refit_node_area(const uint32_t words[10]) {
    const uint32_t exist = (words[3] >> 24) & 15u;
    double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };
    for (int k = 0; k < 3; k++) {
        const double origin = (double)refit_u2f(words[k]), step = (double)refit_u2f(((words[3] >> (8 * k)) & 0xffu) << 23);
        for (int c = 0; c < 4; c++) if ((exist >> c) & 1u) {
            const double l = origin + step * (double)((words[4 + 2 * k] >> (8 * c)) & 0xffu), h = origin + step * (double)((words[5 + 2 * k] >> (8 * c)) & 0xffu);
            if (l < lo[k]) lo[k] = l;
            if (h > hi[k]) hi[k] = h;
        }
    }
    if (!exist) return 0.0;
    const double x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
    return 2.0 * (x * y + y * z + z * x);
}

}  // namespace ctl
