// geometry_hash.cpp — hash_geometry / mesh_ranges (geometry_hash.h): host arithmetic over a description.
#include "geometry_hash.h"
#include "scene_cache.h"
#include <algorithm>
#include <utility>

namespace ctl {

namespace {
void ranges_of(const std::vector<uint32_t>& start, uint32_t count, std::vector<uint32_t>& first, std::vector<uint32_t>& last) {
    const size_t n = start.size();
    std::vector<std::pair<uint32_t, uint32_t>> order(n);
    for (size_t m = 0; m < n; m++) order[m] = { std::min(start[m], count), (uint32_t)m };
    std::sort(order.begin(), order.end());
    first.assign(n, 0u); last.assign(n, 0u);
    for (size_t r = 0; r < n; r++) { first[order[r].second] = order[r].first; last[order[r].second] = r + 1 < n ? order[r + 1].first : count; }
}
}  // namespace

mesh_ranges::mesh_ranges(const ctl_scene_desc& d) {
    std::vector<uint32_t> s(d.n_meshes);
    for (uint32_t m = 0; m < d.n_meshes; m++) s[m] = d.meshes[m].tri_offset;
    ranges_of(s, d.n_tri_data, tri0, tri1);
    for (uint32_t m = 0; m < d.n_meshes; m++) s[m] = d.meshes[m].bvh_tri_offset / 3;
    ranges_of(s, d.n_woop, woop0, woop1);
    for (uint32_t m = 0; m < d.n_meshes; m++) s[m] = d.meshes[m].bvh_node_offset / 4;
    ranges_of(s, d.n_bvh_nodes, node0, node1);
}

void hash_image(uint32_t width, uint32_t height, const uint32_t* texels, uint64_t out[2]) {
    content_hash H; H.add_value(width); H.add_value(height);
    if (texels) H.add(texels, (size_t)width * height * 4);
    H.digest(out);
}

void hash_geometry(const ctl_scene_desc& d, geometry_hashes& out, const std::vector<uint8_t>* skip_values) {
    const mesh_ranges R(d);
    content_hash S, T; std::vector<content_hash> V(d.n_meshes), MS(d.n_meshes);
    uint32_t tri_front = d.n_tri_data, woop_front = d.n_woop, node_front = d.n_bvh_nodes;
    for (uint32_t m = 0; m < d.n_meshes; m++) { tri_front = std::min(tri_front, R.tri0[m]); woop_front = std::min(woop_front, R.woop0[m]); node_front = std::min(node_front, R.node0[m]); }
    S.add_value(d.n_tri_data); S.add_value(d.n_woop); S.add_value(d.n_bvh_nodes);
    if (tri_front) S.add(d.tri_data, (size_t)tri_front * sizeof(ctl_triangle_data));
    if (woop_front) S.add(d.woop, (size_t)woop_front * sizeof(ctl_woop_tri));
    if (node_front) S.add(d.bvh_nodes, (size_t)node_front * sizeof(ctl_bvh_node));
    if (d.n_woop) S.add(d.woop_index, (size_t)d.n_woop * sizeof(ctl_woop_index));
    static_assert(sizeof(ctl_bvh_node) == 64, "Aila-Laine node: 48 B of boxes, 16 B of links");
    for (uint32_t m = 0; m < d.n_meshes; m++) {
        content_hash& H = V[m];
        {   // the mesh's index words: slot bvh_index_offset + (row - first row), as far as the array has them
            const uint64_t at = d.meshes[m].bvh_index_offset, have = at < d.n_woop ? std::min<uint64_t>(R.woop1[m] - R.woop0[m], d.n_woop - at) : 0;
            if (have) MS[m].add(&d.woop_index[at], (size_t)have * sizeof(ctl_woop_index));
        }
        for (uint32_t i = R.node0[m]; i < R.node1[m]; i++) MS[m].add(&d.bvh_nodes[i].child0, 16);
        const bool skip = skip_values && m < skip_values->size() && (*skip_values)[m];
        if (skip) { for (uint32_t i = R.node0[m]; i < R.node1[m]; i++) S.add(&d.bvh_nodes[i].child0, 16); continue; }
        if (R.tri1[m] > R.tri0[m]) H.add(d.tri_data + R.tri0[m], (size_t)(R.tri1[m] - R.tri0[m]) * sizeof(ctl_triangle_data));
        if (R.woop1[m] > R.woop0[m]) H.add(d.woop + R.woop0[m], (size_t)(R.woop1[m] - R.woop0[m]) * sizeof(ctl_woop_tri));
        for (uint32_t i = R.node0[m]; i < R.node1[m]; i++) { H.add(&d.bvh_nodes[i], 48); S.add(&d.bvh_nodes[i].child0, 16); }
    }
    out.images.resize((size_t)d.n_images * 2);
    for (uint32_t i = 0; i < d.n_images; i++) hash_image(d.images[i].width, d.images[i].height, d.images[i].texels, &out.images[(size_t)i * 2]);
    // the transmittance tables: into the whole-structure hash as always, and into a hash of their own (geometry_hashes::tables) — one statement of what is hashed for both
    const auto add_tables = [&d](content_hash& H) {
        const int have_rt = d.rough_transmittance ? 1 : 0; H.add_value(have_rt);
        if (d.rough_transmittance) for (int i = 0; i < 3; i++) {
            const ctl_rough_transmittance& t = d.rough_transmittance[i];
            H.add_value(t.eta_samples); H.add_value(t.alpha_samples); H.add_value(t.theta_samples); H.add_value(t.eta_min); H.add_value(t.eta_max); H.add_value(t.alpha_min); H.add_value(t.alpha_max);
            const int have = (t.trans && t.diff_trans) ? 1 : 0; H.add_value(have);
            if (have) { H.add(t.trans, (size_t)2 * t.eta_samples * t.alpha_samples * t.theta_samples * 4); H.add(t.diff_trans, (size_t)2 * t.eta_samples * t.alpha_samples * 4); }
        }
    };
    add_tables(S); add_tables(T);
    S.digest(out.structure); T.digest(out.tables);
    out.mesh_structure.resize((size_t)d.n_meshes * 2);
    for (uint32_t m = 0; m < d.n_meshes; m++) MS[m].digest(&out.mesh_structure[(size_t)m * 2]);
    out.values.resize((size_t)d.n_meshes * 2);
    for (uint32_t m = 0; m < d.n_meshes; m++) {
        if (skip_values && m < skip_values->size() && (*skip_values)[m]) { out.values[(size_t)m * 2] = out.values[(size_t)m * 2 + 1] = 0; continue; }
        V[m].digest(&out.values[(size_t)m * 2]);
    }
}

}  // namespace ctl
