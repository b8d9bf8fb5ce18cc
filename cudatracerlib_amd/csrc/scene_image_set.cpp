// scene_image_set.cpp — the host side of editing the image set of a live scene (scene_image_set.h): the checks ctl_scene_update_image_set and its test hook share
// (plan_image_set), which also lay out the new texel pool and make the run table, and the host re-statement of k_move_texels.
#include "scene_image_set.h"
#include "scene_checks.h"
#include <chrono>
#include <cstring>
#include <stdexcept>

namespace ctl {

void move_texels_host(const uint32_t* old_pool, uint64_t n_old, const image_run* runs, uint32_t n_runs, uint32_t* new_pool, uint64_t n_new) {
    const uint64_t lanes = n_runs ? runs[n_runs].lane : 0u;
    for (uint64_t lane = 0; lane < lanes; lane++) image_set_move_lane(runs, n_runs, lane, old_pool, n_old, new_pool, n_new);
}

void plan_image_set(const node_set_basis& old, const geometry_hashes& old_geom, const ctl_scene_desc& nd, const uint32_t* old_image_of_new, uint32_t n_new_images,
                    const std::vector<uint8_t>* device_owned, image_set_plan& out, const char* who_) {
    const std::string who = std::string(who_) + ": ";
    if (!old.filled) throw std::runtime_error(who + "the description the scene was made from is not known");
    out = image_set_plan();
    const uint32_t n_old = (uint32_t)old.images.size();
    // the map
    if (n_new_images != nd.n_images) throw std::runtime_error(who + "the image map has " + std::to_string(n_new_images) + " elements, the new description " + std::to_string(nd.n_images) + " images");
    if (n_new_images && !old_image_of_new) throw std::runtime_error(who + "null image map");
    if (nd.n_images && !nd.images) throw std::runtime_error(who + "the new description lacks its image array");
    std::vector<uint32_t> new_of_old(n_old, kNodesNone);
    uint32_t last = kNodesNone;
    for (uint32_t j = 0; j < n_new_images; j++) {
        const uint32_t o = old_image_of_new[j];
        if (o == kNodesNone) { out.fresh++; continue; }
        if (o >= n_old) throw std::runtime_error(who + "image map element " + std::to_string(j) + " names image " + std::to_string(o) + " of " + std::to_string(n_old));
        if (last != kNodesNone && o <= last) throw std::runtime_error(who + "the kept images of the map are not strictly increasing at element " + std::to_string(j) + ": images are not reordered");
        last = o; new_of_old[o] = j; out.kept++;
    }
    out.removed = n_old - out.kept;
    out.identity = n_new_images == n_old && out.fresh == 0;
    // the images themselves
    for (uint32_t j = 0; j < n_new_images; j++) {
        const ctl_mipmap& y = nd.images[j];
        if (!y.texels || !y.width || !y.height) throw std::runtime_error(who + "image " + std::to_string(j) + " of the new description is empty");
        if (y.texel_type > CTL_TEXEL_RGBCOL || y.wrap_mode > CTL_WRAP_BLACK || y.filter_mode > CTL_FILTER_TRILINEAR) throw std::runtime_error(who + "image " + std::to_string(j) + " has an unknown texel type, wrap or filter mode");
        const uint32_t o = old_image_of_new[j];
        if (o == kNodesNone) continue;
        const ctl_mipmap& x = old.images[o];
        if (x.width != y.width || x.height != y.height || x.texel_type != y.texel_type || x.wrap_mode != y.wrap_mode || x.filter_mode != y.filter_mode)
            throw std::runtime_error(who + "kept image " + std::to_string(j) + " (was " + std::to_string(o) + ") has another size, texel type, wrap or filter mode (" + std::to_string(y.width) + " x " + std::to_string(y.height) +
                                     ", held " + std::to_string(x.width) + " x " + std::to_string(x.height) + "): a replaced image is a fresh one in the map");
    }
    // everything else must be what ctl_scene_update applies
    if (nd.n_meshes != old.meshes.size() || (nd.n_meshes && (!nd.meshes || std::memcmp(nd.meshes, old.meshes.data(), (size_t)nd.n_meshes * sizeof(ctl_kernel_mesh)) != 0)) ||
        nd.n_tri_data != old.n_tri_data || nd.n_woop != old.n_woop || nd.n_bvh_nodes != old.n_bvh_nodes)
        throw std::runtime_error(who + "the set of meshes differs: meshes are added and removed by ctl_scene_update_meshes / ctl_scene_update_mesh_set, on a description of their own");
    if (nd.n_nodes != old.nodes.size() || (nd.n_nodes && !nd.nodes)) throw std::runtime_error(who + "the set of nodes differs (" + std::to_string(nd.n_nodes) + " of " + std::to_string(old.nodes.size()) + "): nodes are added and removed by ctl_scene_update_nodes, on a description of its own");
    for (uint32_t k = 0; k < nd.n_nodes; k++) {
        const ctl_node &x = old.nodes[k], &y = nd.nodes[k];
        if (x.mesh_index != y.mesh_index || x.material_offset != y.material_offset || x.instanciated_material != y.instanciated_material)
            throw std::runtime_error(who + "the set of nodes differs: node " + std::to_string(k) + " has another mesh or material assignment");
    }
    if ((nd.rough_transmittance != nullptr) != old.rough_transmittance) throw std::runtime_error(who + "the transmittance tables differ; re-create the scene");
    if (nd.n_materials < old.n_materials) throw std::runtime_error(who + "the material table shrank (" + std::to_string(nd.n_materials) + " of " + std::to_string(old.n_materials) + "): it is not compacted");
    check_scene_desc(nd, kCheckAllParts, who_);   // what ctl_scene_desc_check refuses
    // the one hash pass over the new description
    if (!old_geom.empty()) {
        if (old_geom.images.size() != (size_t)n_old * 2) throw std::runtime_error(who + "the hashes the scene holds carry no image digests");
        const auto t0 = std::chrono::steady_clock::now();
        if (device_owned && device_owned->size() != nd.n_meshes) device_owned = nullptr;
        hash_geometry(nd, out.geom, device_owned);
        out.hash_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (device_owned && out.geom.values.size() == old_geom.values.size())
            for (uint32_t m = 0; m < nd.n_meshes; m++) if ((*device_owned)[m]) { out.geom.values[2 * (size_t)m] = old_geom.values[2 * (size_t)m]; out.geom.values[2 * (size_t)m + 1] = old_geom.values[2 * (size_t)m + 1]; }
        if (out.geom.structure[0] != old_geom.structure[0] || out.geom.structure[1] != old_geom.structure[1] || out.geom.values.size() != old_geom.values.size())
            throw std::runtime_error(who + "the structure of the geometry arrays (woop_index, mesh BVH links, transmittance tables) differs; re-create the scene");
        for (uint32_t m = 0; m < nd.n_meshes; m++) if (!out.geom.same_values(old_geom, m))
            throw std::runtime_error(who + "mesh " + std::to_string(m) + " has other vertex values than the scene holds: apply them with ctl_scene_update first");
        for (uint32_t j = 0; j < n_new_images; j++) {
            const uint32_t o = old_image_of_new[j];
            if (o == kNodesNone) continue;
            if (out.geom.images[2 * (size_t)j] != old_geom.images[2 * (size_t)o] || out.geom.images[2 * (size_t)j + 1] != old_geom.images[2 * (size_t)o + 1])
                throw std::runtime_error(who + "kept image " + std::to_string(j) + " (was " + std::to_string(o) + ") has another digest: its texels are not the ones the scene holds (mirror ctl_scene_update_image with ctl_builder_update_image, or name the image fresh)");
        }
    }
    // the two layouts and the runs
    out.old_offsets.resize(n_old);
    for (uint32_t o = 0; o < n_old; o++) { mip_level_table L; out.old_offsets[o] = out.old_total; out.old_total += image_pyramid_layout(old.images[o].width, old.images[o].height, L); }
    out.offsets.resize(n_new_images); out.levels.resize(n_new_images);
    uint32_t prev_old = kNodesNone;   // the held index of new image j - 1, where that one is kept
    for (uint32_t j = 0; j < n_new_images; j++) {
        const uint64_t size = image_pyramid_layout(nd.images[j].width, nd.images[j].height, out.levels[j]);
        out.offsets[j] = out.total;
        const uint32_t o = old_image_of_new[j];
        if (o == kNodesNone) { out.texels_uploaded += (uint64_t)nd.images[j].width * nd.images[j].height; prev_old = kNodesNone; }
        else {
            if (prev_old == kNodesNone || o != prev_old + 1u) out.runs.push_back(image_run{ out.total, out.old_offsets[o], 0u, out.texels_moved });
            out.runs.back().len += size; out.texels_moved += size; prev_old = o;
        }
        out.total += size;
    }
    out.runs.push_back(image_run{ out.total, out.old_total, 0u, out.texels_moved });   // the sentinel
}

}  // namespace ctl
