// scene_image_set.h — another SET OF IMAGES for a live scene (ctl_scene_update_image_set): images removed, added and replaced by ones of another size, beside what
// ctl_scene_update applies.  The texel pool of a scene is dense: in image order, level 0 of every image followed by its pyramid, exactly what ctl_scene_create lays out with
// mip_pyramid_append (mip_pyramid.h), and every descriptor the kernels read points into it.  An edit of the set is a NEW pool in the new description's layout:
//   kept images    their whole pyramids move, device to device, from where they stand in the old pool: nothing is recomputed, and what stands in HBM survives (texels a
//                  ctl_scene_update_image wrote).  The kept images form RUNS: maximal groups of kept images that are consecutive in the old pool and in the new one.  A run
//                  is a first destination texel, a first source texel and a length; removing one image of ten thousand gives two runs
//   fresh images   (added, or replaced by another size) level 0 is uploaded into its slot and the pyramid built there by k_mip_level (scene_images.hip)
// The arithmetic of the move is single source for the kernel (scene_image_set.hip k_move_texels) and the host hook (ctl_move_texels_host): lane -> destination texel ->
// source texel, both through a binary search over the run table.
#pragma once
#include "flat_nodes.h"
#include "mip_pyramid.h"
#include <string>

namespace ctl {

constexpr uint64_t kImageNotKept = ~0ull;   // image_set_source_texel: the destination texel belongs to no kept image

// one run of kept images, in texels of the pools.  lane: the kept texels in front of the run — the lanes of k_move_texels count kept texels only.  The table ends with a
// sentinel { texels of the new pool, texels of the old pool, 0, kept texels }
struct image_run { uint64_t dst, src, len, lane; };

// the destination texel of lane `lane` (lanes count the kept texels in pool order), or kImageNotKept for a lane beyond them
CTL_REFIT_HD uint64_t image_set_lane_texel(const image_run* runs, uint32_t n_runs, uint64_t lane) {
    if (!n_runs || lane >= runs[n_runs].lane) return kImageNotKept;
    uint32_t lo = 0u, hi = n_runs;   // runs[lo].lane <= lane < runs[hi].lane
    while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (runs[mid].lane <= lane) lo = mid; else hi = mid; }
    return runs[lo].dst + (lane - runs[lo].lane);
}
// the texel of the old pool that texel `dst_texel` of the new pool is a copy of, or kImageNotKept: a texel of a fresh image, or outside the pool
CTL_REFIT_HD uint64_t image_set_source_texel(const image_run* runs, uint32_t n_runs, uint64_t dst_texel) {
    if (!n_runs || dst_texel < runs[0].dst) return kImageNotKept;
    uint32_t lo = 0u, hi = n_runs;   // runs[lo].dst <= dst_texel, and dst_texel < runs[hi].dst where hi < n_runs
    while (hi - lo > 1u) { const uint32_t mid = lo + ((hi - lo) >> 1); if (runs[mid].dst <= dst_texel) lo = mid; else hi = mid; }
    const uint64_t at = dst_texel - runs[lo].dst;
    return at < runs[lo].len ? runs[lo].src + at : kImageNotKept;
}
// what one lane of k_move_texels does: one load, one store, every index checked against the size of the array it goes into
CTL_REFIT_HD void image_set_move_lane(const image_run* runs, uint32_t n_runs, uint64_t lane, const uint32_t* old_pool, uint64_t n_old, uint32_t* new_pool, uint64_t n_new) {
    const uint64_t dst = image_set_lane_texel(runs, n_runs, lane);
    if (dst >= n_new) return;      // (kImageNotKept included)
    const uint64_t src = image_set_source_texel(runs, n_runs, dst);
    if (src >= n_old) return;      // cannot happen: the runs lie inside the old pool (plan_image_set); never read outside it
    new_pool[dst] = old_pool[src];
}

// ---- host side
// the level table of a width x height image and the texels of its whole pyramid: mip_pyramid_append's layout without the texels
inline uint64_t image_pyramid_layout(uint32_t width, uint32_t height, mip_level_table& L) {
    std::memset(&L, 0, sizeof(L)); L.levels = mip_level_count(width, height);
    uint32_t o = width * height;
    for (uint32_t l = 1, j = width / 2, k = height / 2; l < L.levels; l++, j >>= 1, k >>= 1) { L.offsets[l - 1] = o; o += j * k; }
    return o;
}

// a checked change of the image set
struct image_set_plan {
    bool identity = false;                     // same count, old_image_of_new[j] == j: the call is ctl_scene_update
    std::vector<uint64_t> offsets, old_offsets;   // per new / per held image: the texel offset of its level 0 in the new / old pool
    std::vector<mip_level_table> levels;       // per new image
    uint64_t total = 0, old_total = 0;         // texels of the new / old pool
    std::vector<image_run> runs;               // the runs and the sentinel
    uint32_t n_runs() const { return runs.empty() ? 0u : (uint32_t)runs.size() - 1u; }
    uint32_t kept = 0, fresh = 0, removed = 0;
    uint64_t texels_moved = 0, texels_uploaded = 0;   // of kept pyramids; level-0 texels of fresh images
    geometry_hashes geom;                      // of the new description, from the one hash pass (values of device-owned meshes carried over)
    float hash_ms = 0;
};
// Everything ctl_scene_update_image_set refuses before anything is written (std::runtime_error -> CTL_ERR_INVALID), each rule with a message of its own: the map
// (old_image_of_new[j] = the held image that new image j was, or UINT32_MAX for a fresh one; n == nd.n_images; kept indices strictly increasing and inside the held set);
// a kept image with another size, texel type, wrap or filter mode, or another digest than the scene holds; an image without texels; another mesh set, node set, geometry
// structure, geometry values (outside device-owned meshes) or transmittance tables; a material table that shrank; what ctl_scene_desc_check refuses.  old_geom empty: the
// held description is not known by hashes and nothing is compared through them (the caller hashes it first).  device_owned: one byte per mesh, or null.
void plan_image_set(const node_set_basis& old, const geometry_hashes& old_geom, const ctl_scene_desc& nd, const uint32_t* old_image_of_new, uint32_t n_new_images,
                    const std::vector<uint8_t>* device_owned, image_set_plan& out, const char* who);
// the host re-statement of k_move_texels: every lane of the kept texels, in order
void move_texels_host(const uint32_t* old_pool, uint64_t n_old, const image_run* runs, uint32_t n_runs, uint32_t* new_pool, uint64_t n_new);
// the CTL_DIFF_* bits of everything ctl_scene_update applies that differs between the held description `a` and `b`, judged without the geometry arrays and the images (the
// caller has compared those through the hashes): camera, materials (b may hold more of them), lights, transforms, volumes.  scene_update.hip
uint32_t scene_desc_diff_small(const ctl_scene_desc& a, const ctl_scene_desc& b);

}  // namespace ctl
