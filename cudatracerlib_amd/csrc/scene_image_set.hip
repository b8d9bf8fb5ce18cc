// scene_image_set.hip — the image set of a live scene edited on the device (ctl_scene_update_image_set): images removed, added and replaced by ones of another size.  The
// functions of scene_image_set.h, which the host hook (scene_image_set.cpp move_texels_host) runs too.
//
//   k_move_texels       one lane per texel of the KEPT pyramids, consecutive lanes consecutive texels of the new pool: the lane's destination texel by a binary search
//                       over the run table's lane column, its source texel by image_set_source_texel over the destination column (the table lies in global memory: a handful
//                       of 32-B entries, read by every lane of a wave at the same addresses except around a run boundary), one 4-B load from the old pool, one 4-B store.
//                       Whole pyramids move: a kept image's levels are not recomputed, and what stands in HBM — texels of a ctl_scene_update_image — survives.  4-B accesses:
//                       a pyramid such as 5 x 3 + 2 x 1 texels is no multiple of 16 B, so neither the run starts nor source against destination are aligned for wider ones
//   k_mip_level         (scene_images.hip launch_mip_levels) the pyramids of the fresh images, level by level, all of them launched before the one synchronisation
//   k_gather_texels     one lane per fresh image: the texel ImageTexture::Average() addresses into a small array, so that ONE read-back brings all of them
// Nothing moves in place: source and destination overlap, and until the commit the scene's own pool is what a refusal or a failed allocation leaves behind.  During the call
// HBM holds the old pool and the new one.  Plain launches on the null stream between two synchronisations; no workgroup waits for another, no atomics, no LDS; every index is
// checked against the size of the array it goes into.
#include "flat_device.h"
#include "scene_image_set.h"
#include "mitsuba_loader.h"   // unsupported_error
#include <algorithm>
#include <chrono>
#include <cstring>

namespace ctl {

namespace {

struct move_texels { const uint32_t* src; uint32_t* dst; const image_run* runs; uint32_t n_runs; uint64_t n_src, n_dst, lanes; };

__global__ void __launch_bounds__(256) k_move_texels(move_texels K) {
    const uint64_t lane = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (lane >= K.lanes) return;
    image_set_move_lane(K.runs, K.n_runs, lane, K.src, K.n_src, K.dst, K.n_dst);
}

__global__ void __launch_bounds__(64) k_gather_texels(const uint32_t* __restrict__ pool, uint64_t n_pool, const uint64_t* __restrict__ at, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    out[i] = at[i] < n_pool ? pool[at[i]] : 0u;
}

struct event_trio { hipEvent_t e[3] = { nullptr, nullptr, nullptr }; ~event_trio() { for (auto x : e) if (x) (void)hipEventDestroy(x); } };   // destroyed also when a call throws

using clk = std::chrono::steady_clock;

}  // namespace

void flat_rebuilder::update_image_set(Scene& A, const ctl_scene_desc& d, const uint32_t* old_image_of_new, uint32_t n_new_images, const node_set_basis& basis, ctl_scene_image_set_stats* stats) {
    const clk::time_point t_all = clk::now();
    require_device();
    const char* who = "ctl_scene_update_image_set";
    // ---- everything that can refuse the call, before the device is touched and before a tracer is stalled
    if (!A.snap_) throw std::runtime_error(std::string(who) + ": the scene holds no description");
    const std::vector<uint8_t> device_owned = A.device_owned_meshes();
    image_set_plan plan;
    plan_image_set(basis, A.snap_->geom, d, old_image_of_new, n_new_images, device_owned.empty() ? nullptr : &device_owned, plan, who);
    const uint32_t mask = scene_desc_diff_small(A.snap_->d, d) | (A.lights_stale_ ? (uint32_t)CTL_DIFF_LIGHTS : 0u);
    if ((mask & CTL_DIFF_TRANSFORMS) && A.flattened()) {   // what the stages of ctl_scene_update would refuse behind the image stages
        if (A.S.flat_format != kFlatQ4) throw unsupported_error(std::string(who) + ": the Q8 node format is not refitted; a transform change needs a scene in the default format (or a new scene)");
        if (A.refit_.level_start.size() < 2) throw unsupported_error(std::string(who) + ": the flattened tree carries no refit data");
    }
    ctl_scene_image_set_stats st{};
    st.images_kept = plan.kept; st.images_fresh = plan.fresh; st.images_removed = plan.removed; st.hash_ms = plan.hash_ms;
    if (plan.identity) {   // nothing of the image set changes: ctl_scene_update (the digests of the kept images are the held ones)
        apply_update(A, d, mask, plan.geom, &st.update);
        st.total_ms = std::chrono::duration<float, std::milli>(clk::now() - t_all).count();
        if (stats) *stats = st;
        return;
    }
    const uint32_t n_old = (uint32_t)basis.images.size(), n_new = n_new_images, n_runs = plan.n_runs();
    // the pool the scene holds must be the held description's (it is: creation laid it out, and every later call kept the layout)
    if (A.image_off_.size() != n_old || A.image_levels_.size() != n_old || A.image_avg_.size() != (size_t)n_old * 4 || A.texels_.n != std::max<uint64_t>(4, plan.old_total))
        throw std::runtime_error(std::string(who) + ": the scene's texel pool has another layout than the description it holds");
    for (uint32_t o = 0; o < n_old; o++) if (A.image_off_[o] != plan.old_offsets[o]) throw std::runtime_error(std::string(who) + ": the scene's texel pool has another layout than the description it holds");
    const uint64_t move_blocks = (plan.texels_moved + 255u) / 256u;
    if (move_blocks > 0x7fffffffull) throw std::runtime_error(std::string(who) + ": too many texels to move in one launch");
    // the host side of the new tables
    std::vector<size_t> off_new(n_new); std::vector<dev_mip_levels> lv_new(std::max<uint32_t>(1, n_new)); std::vector<float> avg_new((size_t)n_new * 4, 0.0f);
    std::vector<uint32_t> fresh; std::vector<uint64_t> avg_at;
    static_assert(sizeof(mip_level_table) == sizeof(dev_mip_levels), "one layout");
    for (uint32_t j = 0; j < n_new; j++) {
        off_new[j] = (size_t)plan.offsets[j]; std::memcpy(&lv_new[j], &plan.levels[j], sizeof(dev_mip_levels));
        const uint32_t o = old_image_of_new[j];
        if (o != kNodesNone) { std::memcpy(&avg_new[(size_t)j * 4], &A.image_avg_[(size_t)o * 4], 16); continue; }
        fresh.push_back(j); avg_at.push_back(plan.offsets[j] + mip_average_texel_offset(d.images[j], plan.levels[j]));
    }
    CTL_HIP(hipDeviceSynchronize());   // no trace reads the pool any more; a ctl_scene_update_image has finished (the call is synchronous)
    // ---- 1. every allocation before the first launch
    dbuf<uint32_t> pool_new, avg_out; dbuf<image_run> runs_dev; dbuf<ctl_mipmap> images_new; dbuf<dev_mip_levels> levels_new; dbuf<uint64_t> avg_at_dev;
    pool_new.alloc((size_t)std::max<uint64_t>(4, plan.total)); runs_dev.alloc(plan.runs.size());
    images_new.alloc(std::max<uint32_t>(1, n_new)); levels_new.alloc(lv_new.size());
    avg_out.alloc(std::max<size_t>(1, fresh.size())); avg_at_dev.alloc(std::max<size_t>(1, fresh.size()));
    event_trio ev; for (auto& x : ev.e) CTL_HIP(hipEventCreate(&x));
    CTL_HIP(hipMemcpy(runs_dev.p, plan.runs.data(), plan.runs.size() * sizeof(image_run), hipMemcpyHostToDevice));
    if (!fresh.empty()) CTL_HIP(hipMemcpy(avg_at_dev.p, avg_at.data(), avg_at.size() * 8, hipMemcpyHostToDevice));
    {   // 4. the image table and the level table at the new counts: the descriptors point into the new pool
        std::vector<ctl_mipmap> tab(n_new);
        for (uint32_t j = 0; j < n_new; j++) { tab[j] = d.images[j]; tab[j].texels = pool_new.p + off_new[j]; }
        if (n_new) CTL_HIP(hipMemcpy(images_new.p, tab.data(), tab.size() * sizeof(ctl_mipmap), hipMemcpyHostToDevice));
        CTL_HIP(hipMemcpy(levels_new.p, lv_new.data(), lv_new.size() * sizeof(dev_mip_levels), hipMemcpyHostToDevice));
    }
    if (plan.total < pool_new.n) CTL_HIP(hipMemsetAsync(pool_new.p, 0, pool_new.n * 4, nullptr));   // the four words an image-less scene holds
    // ---- 2. the kept pyramids, from the scene's pool into the new one
    CTL_HIP(hipEventRecord(ev.e[0], nullptr));
    if (plan.texels_moved && n_runs) {
        const move_texels K{ A.texels_.p, pool_new.p, runs_dev.p, n_runs, (uint64_t)A.texels_.n, (uint64_t)pool_new.n, plan.texels_moved };
        hipLaunchKernelGGL(k_move_texels, dim3((uint32_t)move_blocks), dim3(256), 0, nullptr, K);
        CTL_HIP(hipGetLastError());
    }
    CTL_HIP(hipEventRecord(ev.e[1], nullptr));
    // ---- 3. the fresh images: level 0 into its slot, the pyramid behind it; one read-back of the texels ImageTexture::Average() addresses
    for (uint32_t j : fresh) {
        const ctl_mipmap& M = d.images[j];
        const uint64_t n0 = (uint64_t)M.width * M.height;
        if (plan.offsets[j] + n0 > pool_new.n) throw std::runtime_error(std::string(who) + ": a fresh image reaches outside the new texel pool");   // cannot happen: the plan laid the pool out
        CTL_HIP(hipMemcpyAsync(pool_new.p + off_new[j], M.texels, n0 * 4, hipMemcpyHostToDevice, nullptr));
        launch_mip_levels(pool_new.p + off_new[j], M.width, M.height, M.texel_type, lv_new[j]);
    }
    std::vector<uint32_t> avg_texels(fresh.size());
    if (!fresh.empty()) {
        hipLaunchKernelGGL(k_gather_texels, dim3((uint32_t)((fresh.size() + 63u) / 64u)), dim3(64), 0, nullptr, pool_new.p, (uint64_t)pool_new.n, avg_at_dev.p, (uint32_t)fresh.size(), avg_out.p);
        CTL_HIP(hipGetLastError());
    }
    CTL_HIP(hipEventRecord(ev.e[2], nullptr));
    if (!fresh.empty()) CTL_HIP(hipMemcpy(avg_texels.data(), avg_out.p, fresh.size() * 4, hipMemcpyDeviceToHost));
    CTL_HIP(hipDeviceSynchronize());
    CTL_HIP(hipEventElapsedTime(&st.move_ms, ev.e[0], ev.e[1])); CTL_HIP(hipEventElapsedTime(&st.pyramid_ms, ev.e[1], ev.e[2]));
    for (size_t f = 0; f < fresh.size(); f++) { float* a = &avg_new[(size_t)fresh[f] * 4]; mip_texel_decode(avg_texels[f], d.images[fresh[f]].texel_type, a); a[3] = 1.0f; }
    // ---- the commit: from here on the scene is written.  The new pool and tables become the scene's, the old ones are freed with the locals
    swap_buffers(A.texels_, pool_new); swap_buffers(A.images_, images_new); swap_buffers(A.mip_levels_, levels_new);
    A.S.images = A.images_.p; A.S.mip_levels = A.mip_levels_.p;
    A.image_off_ = std::move(off_new); A.image_levels_.assign(lv_new.begin(), lv_new.begin() + n_new); A.image_avg_ = std::move(avg_new);
    {   // the snapshot's images and digests: the scene holds the old description with the new image set until the stages below bring the rest
        desc_snapshot& s = *A.snap_;
        s.images.assign(d.images, d.images + n_new); for (auto& m : s.images) m.texels = nullptr;
        s.d.images = s.images.data(); s.d.n_images = n_new;
        s.geom.images = plan.geom.images;
        if (!A.refit_.geom.empty()) A.refit_.geom.images = plan.geom.images;
    }
    // ---- 5. the ordinary stages of ctl_scene_update over the rest of the description, 6. bind.  Nothing else differs: the snapshot alone follows
    if (mask) apply_update(A, d, mask, plan.geom, &st.update);
    else { A.last_mask_ = 0; A.last_update_ = ctl_scene_update_stats{}; A.bind(d); A.snapshot(d, &plan.geom); }
    st.runs = n_runs; st.texels_moved = plan.texels_moved; st.texels_uploaded = plan.texels_uploaded;
    st.bytes_freed = plan.old_total > plan.total ? (plan.old_total - plan.total) * 4u : 0u;
    st.total_ms = std::chrono::duration<float, std::milli>(clk::now() - t_all).count();
    if (stats) *stats = st;
}

}  // namespace ctl
