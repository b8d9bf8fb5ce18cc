// flat_refit.hip — the refit of the flattened Q4 tree on the device (ctl_scene_update): the kernels around the functions of flat_refit.h, which the host refit
// (flatten.cpp refit_flat_scene) runs too — same functions, same order of operations, so the device tree equals the host's byte for byte
// (tests/test_gpu_scene_update.py).
//
//   k_deform_entries  a geometry update (CTL_DIFF_GEOMETRY), before k_refit_entries: one lane per leaf entry; the lane of an entry whose node instances a changed mesh copies the
//                     three Woop rows of its triangle from the two-level leaf stream — which the update has re-uploaded, so the rows are the new ones — into the first 48 B of
//                     the entry and marks the entry as standing for its whole triangle (part_index = kRefitNoPart: its clip box was cut from the triangle as it was).  Every
//                     other lane leaves after the 16-B load of its index / node words.  The model / alpha bits and the box of the entry are k_refit_entries' work, which runs
//                     next in stream order and reads what this kernel wrote.  The entry -> row mapping is a table per TRIANGLE (flatten.h triangle_woop_rows: 4 B per
//                     triangle, made from woop_index on the first geometry update) instead of a word per ENTRY kept from creation: the entries already name their triangle,
//                     so the flattened-tree cache and the creation path stay as they are.
//   k_refit_entries   one lane per leaf entry: rows 0..2 and w33 of the node's new inverse transform into the entry, the model / alpha bits re-stamped if asked,
//                     the entry's new world-space box into scratch.  A lane reads the first 64 B of its 128-B entry (four 16-B loads that share one line) and writes
//                     the second 64 B; the arithmetic — a 4 x 4 inverse in double per entry — outweighs the traffic.
//   k_refit_level     one lane per node of ONE depth, launched deepest level first: the box of a leaf slot is the union of its entries' boxes, the box of an inner
//                     slot the child's own box from scratch (written by the launch before); re-quantises the node and writes its own box to scratch.
//   k_refit_area      the surface-area report.
// Plain launches in stream order; no kernel waits for another workgroup.
#include "tracer.h"
#include "flat_refit.h"

namespace ctl {

namespace {

__global__ void __launch_bounds__(256) k_deform_entries(refit_device R, deform_device D) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= R.n_entries) return;
    float4* __restrict__ E = R.leaves + (size_t)i * 8;
    const float4 q3 = E[3];
    const uint32_t index = __float_as_uint(q3.x), node = __float_as_uint(q3.y) & 0x7fffffffu;
    if (node >= D.n_scene_nodes || !D.node_changed[node]) return;
    const uint32_t tri = (R.leaf_keys ? (index & 0x0fffffffu) : index) >> 1;
    if (tri >= D.n_tris) return;   // cannot happen in a tree the update has checked; never read outside the arrays
    const uint32_t row = D.tri_row[tri];
    if (row >= D.n_rows) return;
    const float4* __restrict__ W = D.leaf_tris + (size_t)row * 4;
    E[0] = W[0]; E[1] = W[1]; E[2] = W[2];
    R.part_index[i] = kRefitNoPart;
}

__global__ void __launch_bounds__(256) k_refit_entries(refit_device R, int boxes) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= R.n_entries) return;
    float4* __restrict__ E = R.leaves + (size_t)i * 8;
    const float4 q3 = E[3];
    uint32_t index = __float_as_uint(q3.x), node_w = __float_as_uint(q3.y);
    const uint32_t node = node_w & 0x7fffffffu;
    if (R.restamp) {
        // as ctl_scene_create_ex stamps the upload (tracer.hip): TriangleData::getMatIndex, the BSDF model into bits 28..31 of the index word, "has an alpha map" into bit 31 of the node word
        const uint32_t tri = (R.leaf_keys ? (index & 0x0fffffffu) : index) >> 1;
        const uint32_t mi = R.node_info[node].x + ((R.tri_data[(size_t)tri * 2].y >> 16) & 0xffu);
        // a material index outside the scene's materials: the upload refuses it where it stamps keys, and counts it as "has an alpha map" where it does not (tracer.hip)
        const bool known = mi < (uint32_t)R.restamp;   // restamp = the number of materials
        const uint32_t bsdf = known ? R.mats[mi].bsdf_type : 0u, alpha = known ? R.mats[mi].alpha_state : 1u;
        if (R.leaf_keys) index = (index & 0x0fffffffu) | ((bsdf & 15u) << 28);
        node_w = node | ((R.alpha_maps && alpha != CTL_ALPHA_DISABLED) ? 0x80000000u : 0u);
        E[3] = make_float4(__uint_as_float(index), __uint_as_float(node_w), q3.z, q3.w);
    }
    if (!boxes) return;
    const float4 a = E[0], b = E[1], c = E[2];
    const float4 i0 = R.inst[(size_t)node * 4], i1 = R.inst[(size_t)node * 4 + 1], i2 = R.inst[(size_t)node * 4 + 2], i3 = R.inst[(size_t)node * 4 + 3];
    E[4] = i0; E[5] = i1; E[6] = i2; E[7] = make_float4(i3.x, 0.0f, 0.0f, 0.0f);
    const float4 f0 = R.inst_fwd[(size_t)node * 3], f1 = R.inst_fwd[(size_t)node * 3 + 1], f2 = R.inst_fwd[(size_t)node * 3 + 2];
    const float M[12] = { f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w, f2.x, f2.y, f2.z, f2.w };
    const float wa[4] = { a.x, a.y, a.z, a.w }, wb[4] = { b.x, b.y, b.z, b.w }, wc[4] = { c.x, c.y, c.z, c.w };
    const uint32_t pi = R.part_index[i];
    refit_box part, out;
    if (pi != kRefitNoPart) part = R.part_boxes[pi];
    refit_entry_box(wa, wb, wc, M, pi != kRefitNoPart ? &part : nullptr, R.carry + (size_t)node * 12, out);
    R.ebox[i] = out;
}

__global__ void __launch_bounds__(256) k_refit_level(refit_device R, const uint32_t* __restrict__ level_nodes, uint32_t count) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= count) return;
    const uint32_t ni = level_nodes[j];
    if (ni >= R.n_nodes) return;
    float4* __restrict__ N = R.nodes + (size_t)ni * 4;
    const float4 q0 = N[0], q1 = N[1], q2 = N[2], q3 = N[3];
    uint32_t w[10] = { __float_as_uint(q0.x), __float_as_uint(q0.y), __float_as_uint(q0.z), __float_as_uint(q0.w), __float_as_uint(q1.x), __float_as_uint(q1.y),
                       __float_as_uint(q1.z), __float_as_uint(q1.w), __float_as_uint(q2.x), __float_as_uint(q2.y) };
    const uint32_t meta = w[3], exist = (meta >> 24) & 15u, leafm = (meta >> 28) & exist;
    int32_t link[4];
    if (R.compact) {   // flat4_implied_links (flatten.h)
        const uint32_t w0 = __float_as_uint(q2.z), w1 = __float_as_uint(q2.w), lm = meta >> 28;
        const uint32_t ib4 = w0 & 0x03fffffcu, nlb15 = (w1 >> 6) | 0xfc000000u;
        const uint32_t t[4] = { 0u, (w0 >> 26) & 15u, (w1 >> 2) & 15u, (w0 >> 30) | ((w1 & 3u) << 2) };
        link[0] = (lm & 1u) ? (int32_t)(nlb15 + 15u) : (int32_t)(w0 & 0x03ffffffu);
        for (int k = 1; k < 4; k++) link[k] = (int32_t)((((lm >> k) & 1u) ? nlb15 : ib4) + t[k]);
    } else { link[0] = __float_as_int(q3.x); link[1] = __float_as_int(q3.y); link[2] = __float_as_int(q3.z); link[3] = __float_as_int(q3.w); }
    refit_box cb[4];
    uint32_t ok = exist;
    for (int c = 0; c < 4; c++) {
        if (!((exist >> c) & 1u)) continue;
        if (!((leafm >> c) & 1u)) {
            const uint32_t k = (uint32_t)link[c] >> 2;
            if (k >= R.n_nodes) { ok &= ~(1u << c); continue; }   // cannot happen in a tree flat_links_valid passed; never read outside the arrays
            cb[c] = R.nbox[k];
            continue;
        }
        for (int r = 0; r < 3; r++) { cb[c].lo[r] = kRefitBig; cb[c].hi[r] = -kRefitBig; }
        for (uint32_t e = (uint32_t)~link[c]; e < R.n_entries; e++) {   // up to the entry that closes the leaf, as the host walks it; the last entry of the array closes its leaf (flat_links_valid)
            const refit_box b = R.ebox[e];
            for (int r = 0; r < 3; r++) { cb[c].lo[r] = refit_min(cb[c].lo[r], b.lo[r]); cb[c].hi[r] = refit_max(cb[c].hi[r], b.hi[r]); }
            if (__float_as_uint(R.leaves[(size_t)e * 8 + 3].x) & 1u) break;
        }
    }
    refit_box own;
    refit_node_boxes(w, ok, cb, own);
    R.nbox[ni] = own;
    N[0] = make_float4(__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2]), __uint_as_float(w[3]));
    N[1] = make_float4(__uint_as_float(w[4]), __uint_as_float(w[5]), __uint_as_float(w[6]), __uint_as_float(w[7]));
    N[2] = make_float4(__uint_as_float(w[8]), __uint_as_float(w[9]), q2.z, q2.w);
    if (R.compact && __float_as_uint(q3.x) != 0u) {   // the node carries an oriented slab: neutralised (flat_refit.h)
        uint32_t lo = 0u, hi = 0u;
        for (int c = 0; c < 4; c++) { if ((exist >> c) & 1u) hi |= 255u << (8 * c); else lo |= 255u << (8 * c); }
        N[3] = make_float4(__uint_as_float(kRefitNeutralSlabN), __uint_as_float(kRefitNeutralSlabBase), __uint_as_float(lo), __uint_as_float(hi));
    }
}

__global__ void __launch_bounds__(256) k_refit_area(const float4* __restrict__ nodes, uint32_t n_nodes, double* __restrict__ sum_out) {
    __shared__ double s_part[4];
    double a = 0.0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n_nodes; i += gridDim.x * 256u) {
        const float4 q0 = nodes[(size_t)i * 4], q1 = nodes[(size_t)i * 4 + 1], q2 = nodes[(size_t)i * 4 + 2];
        const uint32_t w[10] = { __float_as_uint(q0.x), __float_as_uint(q0.y), __float_as_uint(q0.z), __float_as_uint(q0.w), __float_as_uint(q1.x), __float_as_uint(q1.y),
                                 __float_as_uint(q1.z), __float_as_uint(q1.w), __float_as_uint(q2.x), __float_as_uint(q2.y) };
        a += refit_node_area(w);
    }
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sum_out, s_part[0] + s_part[1] + s_part[2] + s_part[3]);
}

}  // namespace

void launch_deform_entries(hipStream_t s, const refit_device& R, const deform_device& D) {
    if (!R.n_entries) return;
    hipLaunchKernelGGL(k_deform_entries, dim3((R.n_entries + 255u) / 256u), dim3(256), 0, s, R, D);
    CTL_HIP(hipGetLastError());
}
void launch_refit_entries(hipStream_t s, const refit_device& R, bool boxes) {
    if (!R.n_entries) return;
    hipLaunchKernelGGL(k_refit_entries, dim3((R.n_entries + 255u) / 256u), dim3(256), 0, s, R, boxes ? 1 : 0);
    CTL_HIP(hipGetLastError());
}
void launch_refit_level(hipStream_t s, const refit_device& R, const uint32_t* level_nodes, uint32_t count) {
    if (!count) return;
    hipLaunchKernelGGL(k_refit_level, dim3((count + 255u) / 256u), dim3(256), 0, s, R, level_nodes, count);
    CTL_HIP(hipGetLastError());
}
void launch_refit_area(hipStream_t s, const float4* nodes, uint32_t n_nodes, double* sum_out) {
    if (!n_nodes) return;
    const uint32_t blocks = std::min<uint32_t>((n_nodes + 255u) / 256u, 2048u);
    hipLaunchKernelGGL(k_refit_area, dim3(blocks), dim3(256), 0, s, nodes, n_nodes, sum_out);
    CTL_HIP(hipGetLastError());
}

}  // namespace ctl
