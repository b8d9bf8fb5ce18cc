// scene_images.hip — ctl_scene_update_image: the level-0 texels of one image of a live scene replaced in place, and everything the library derives from texels rebuilt on
// the device into the buffers the scene already owns — what DynamicScene::ReloadTextures + UpdateMaterialsPhase2 do in the reference (Engine/DynamicScene.cpp:457-, :84-89)
// for a host that swaps a bitmap.  The host yardstick is ctl_builder_update_image + ctl_builder_finalize (scene_builder.cpp); the kernels run the functions of mip_texel.h
// and env_tables.h, which the builder calls too, so the pool, the tables and the records end up equal to the builder's bit for bit.
//
//   k_mip_level            one lane per OUTPUT texel of a level: the 2x2 block of the level below, decoded, summed ((a + b) + c) + e, times 0.25, encoded.  Launched level by
//                          level (a level reads the one before it); an odd width or height drops the last column or row, as the host loop does.
//   k_env_row_sums         the running luminance sums of the environment map's rows, raw, into cdfCols, and one colSum per row into the scratch.  The sum of a row is SERIAL in
//                          x (fp32 addition order is the contract): one lane per row, each walking its row in global memory.  The lanes of an access are a whole image row
//                          apart, but a lane's next sixteen texels come from the 64-B line its last load brought in; a form that staged 64 x 64 tiles through LDS to read and
//                          write with the lanes along x was measured and lost (RESULTS.md "Image updates in place": 4096 x 2048, tables 1.8 against 2.1 ms), and is gone.
//   k_env_normalize_cols   element-wise: entries 1 .. W - 1 of every row times 1 / colSum, entry W = 1, entry 0 stays 0
//   k_env_rows             one workgroup: rowSum += colSum * rowWeight, H dependent adds by one lane (the products are staged through LDS by all lanes, 1024 at a time), the raw
//                          sums into cdfRows, rowSum into the scratch
//   k_env_normalize_rows   element-wise over the H + 1 entries of cdfRows
// Plain launches on the null stream, in order, between two device synchronisations; no workgroup waits for another; no atomics.  The host computes `normalization` from the
// read-back rowSum with the builder's own expression and patches the light record.
#include "tracer.h"
#include "mip_pyramid.h"
#include "env_tables.h"
#include "material_textures.h"
#include "geometry_hash.h"
#include "flat_device.h"
#include <chrono>
#include <cstddef>
#include <memory>
#include <string>

namespace ctl {

namespace {

constexpr uint32_t kRowChunk = 1024u;   // products per LDS chunk of k_env_rows: four per lane

__global__ void __launch_bounds__(256) k_mip_level(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, uint32_t pw, uint32_t j, uint32_t k, uint32_t type) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (size_t)j * k) return;
    const uint32_t t = (uint32_t)(i / j), x = (uint32_t)(i - (size_t)t * j);
    const uint32_t* r0 = src + (size_t)(2u * t) * pw + 2u * x; const uint32_t* r1 = r0 + pw;   // 2x + 1 < pw and 2t + 1 < the level's height: j = pw / 2, k = height / 2
    dst[i] = mip_texel_box(r0[0], r0[1], r1[0], r1[1], type);
}

struct env_device {
    const uint32_t* texels; float* cols; float* rows; const float* weights; float* scratch;   // scratch: H colSums, then rowSum
    uint32_t W, H, type;
};

__global__ void __launch_bounds__(64) k_env_row_sums(env_device E) {
    const uint32_t y = blockIdx.x * 64u + threadIdx.x;
    if (y >= E.H) return;
    const uint32_t* __restrict__ t = E.texels + (size_t)y * E.W;
    float* __restrict__ row = E.cols + (size_t)y * (E.W + 1u);
    const uint32_t type = E.type;
    row[0] = 0.0f;
    E.scratch[y] = env_running_sum([&](uint32_t x) { return env_texel_luminance(t[x], type); }, E.W, 0.0f, row + 1);
}

__global__ void __launch_bounds__(256) k_env_normalize_cols(env_device E) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x, n = (size_t)E.H * (E.W + 1u);
    if (i >= n) return;
    const uint32_t y = (uint32_t)(i / (E.W + 1u)), x = (uint32_t)(i - (size_t)y * (E.W + 1u));
    const float normalization = 1.0f / E.scratch[y];
    E.cols[i] = env_normalized_entry(E.cols[i], x, E.W, normalization);
}

__global__ void __launch_bounds__(256) k_env_rows(env_device E) {
    __shared__ float s[kRowChunk];
    const uint32_t t = threadIdx.x, H = E.H;
    float rowSum = 0.0f;   // lane 0's is the sum
    for (uint32_t base = 0; base < H; base += kRowChunk) {
        const uint32_t n = H - base < kRowChunk ? H - base : kRowChunk;
        for (uint32_t i = t; i < n; i += 256u) s[i] = E.scratch[base + i] * E.weights[base + i];
        __syncthreads();
        if (t == 0) rowSum = env_running_sum([&](uint32_t i) { return s[i]; }, n, rowSum, s);   // in place
        __syncthreads();
        for (uint32_t i = t; i < n; i += 256u) E.rows[base + i + 1u] = s[i];
        __syncthreads();
    }
    if (t == 0) { E.rows[0] = 0.0f; E.scratch[H] = rowSum; }
}

__global__ void __launch_bounds__(256) k_env_normalize_rows(env_device E) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > E.H) return;
    const float normalization = 1.0f / E.scratch[E.H];
    E.rows[i] = env_normalized_entry(E.rows[i], i, E.H, normalization);
}

// is light `li` of the snapshot an environment light over `image` whose tables lie inside the anim blob (what the kernels write)?
bool env_light_of_image(const ctl_scene_desc& d, uint32_t li, uint32_t image, uint32_t W, uint32_t H) {
    const ctl_light& L = d.lights[li];
    if (L.type != CTL_LIGHT_INFINITE || L.env_image != image) return false;
    const uint64_t cols_end = (uint64_t)L.cdf_cols_index + (uint64_t)(W + 1u) * H * 4u, rows_end = (uint64_t)L.cdf_rows_index + ((uint64_t)H + 1u) * 4u, wts_end = (uint64_t)L.row_weights_index + (uint64_t)H * 4u;
    if ((L.cdf_cols_index % 4u) || (L.cdf_rows_index % 4u) || (L.row_weights_index % 4u) || cols_end > d.n_anim_bytes || rows_end > d.n_anim_bytes || wts_end > d.n_anim_bytes)
        throw std::runtime_error("ctl_scene_update_image: the tables of environment light " + std::to_string(li) + " do not lie inside the scene's anim blob");
    return true;
}

using clk = std::chrono::steady_clock;
float ms_since(clk::time_point t0) { return std::chrono::duration<float, std::milli>(clk::now() - t0).count(); }

}  // namespace

void launch_mip_levels(uint32_t* level0, uint32_t width, uint32_t height, uint32_t type, const dev_mip_levels& L) {
    const uint32_t* src = level0; uint32_t pw = width;
    for (uint32_t l = 1, j = width / 2, k = height / 2; l < L.levels; l++, j >>= 1, k >>= 1) {
        uint32_t* dst = level0 + L.offsets[l - 1];
        const size_t n = (size_t)j * k;
        hipLaunchKernelGGL(k_mip_level, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, nullptr, src, dst, pw, j, k, type); CTL_HIP(hipGetLastError());
        src = dst; pw = j;
    }
}

void Scene::read_image(uint32_t image, uint32_t* texels_out, size_t capacity, uint32_t* levels_out, uint32_t* level_offsets_out) {
    require_device();
    if (!snap_ || image >= snap_->images.size() || image >= image_off_.size()) throw std::runtime_error("ctl_scene_read_image: bad image index " + std::to_string(image));
    const ctl_mipmap& M = snap_->images[image]; const dev_mip_levels& L = image_levels_[image];
    const uint32_t last = L.levels - 1;
    const size_t total = (last ? L.offsets[last - 1] : 0u) + (size_t)(M.width >> last) * (M.height >> last);
    if (levels_out) *levels_out = L.levels;
    if (level_offsets_out) for (int k = 0; k < 15; k++) level_offsets_out[k] = L.offsets[k];
    if (!texels_out) return;
    if (capacity < total) throw std::runtime_error("ctl_scene_read_image: image " + std::to_string(image) + " holds " + std::to_string(total) + " texels in " + std::to_string(L.levels) + " levels");
    CTL_HIP(hipDeviceSynchronize());
    CTL_HIP(hipMemcpy(texels_out, texels_.p + image_off_[image], total * 4, hipMemcpyDeviceToHost));
}

void Scene::update_image(uint32_t image, const uint32_t* texels, uint32_t width, uint32_t height, uint32_t flags, ctl_scene_image_stats* stats) {
    const char* who = "ctl_scene_update_image";
    const clk::time_point t_all = clk::now();
    require_device();
    // ---- everything that can refuse the call, before the device is touched and before a tracer is stalled
    if (!snap_) throw std::runtime_error(std::string(who) + ": the scene holds no description");
    if (flags & ~(uint32_t)CTL_IMAGE_TEXELS_DEVICE) throw std::runtime_error(std::string(who) + ": unknown flag bits");
    if (image >= snap_->images.size() || image >= image_off_.size()) throw std::runtime_error(std::string(who) + ": bad image index " + std::to_string(image) + " of " + std::to_string(snap_->images.size()));
    if (!texels) throw std::runtime_error(std::string(who) + ": null texels");
    const ctl_mipmap M = snap_->images[image]; const dev_mip_levels L = image_levels_[image];
    if (width != M.width || height != M.height)
        throw std::runtime_error(std::string(who) + ": image " + std::to_string(image) + " is " + std::to_string(M.width) + " x " + std::to_string(M.height) + "; an update keeps the size");
    const size_t n0 = (size_t)M.width * M.height, base = image_off_[image];
    const uint32_t last = L.levels - 1;
    const size_t total = (last ? L.offsets[last - 1] : 0u) + (size_t)(M.width >> last) * (M.height >> last);
    if (base + total > texels_.n) throw std::runtime_error(std::string(who) + ": the image's pyramid reaches outside the scene's texel pool");
    std::vector<uint32_t> env_lights;
    for (uint32_t li = 0; li < snap_->d.n_lights_buf; li++) if (env_light_of_image(snap_->d, li, image, M.width, M.height)) env_lights.push_back(li);
    if (!env_lights.empty() && ((size_t)snap_->d.n_anim_bytes > anim_.n || (size_t)snap_->d.n_lights_buf > lights_.n)) throw std::runtime_error(std::string(who) + ": the scene's light tables are smaller than its description");
    std::vector<uint32_t> reading;   // the materials whose Update() reads this image's average
    for (uint32_t i = 0; i < snap_->materials.size(); i++) {
        const ctl_material& m = snap_->materials[i];
        if (!material_reads_texture_average(m)) continue;
        const bool nesting = m.bsdf_type == CTL_BSDF_COATING || m.bsdf_type == CTL_BSDF_ROUGHCOATING;
        if ((m.tex[0].type == CTL_TEX_IMAGE && m.tex[0].image == image) || (!nesting && m.tex[1].type == CTL_TEX_IMAGE && m.tex[1].image == image)) reading.push_back(i);
    }
    if (!reading.empty() && snap_->materials.size() > mats_.n) throw std::runtime_error(std::string(who) + ": the scene's material table is smaller than its description");
    std::unique_ptr<uint32_t[]> level0;   // under the device flag: the read-back the digest is made from (not value-initialised: the copy fills it)
    if (flags & CTL_IMAGE_TEXELS_DEVICE) level0.reset(new uint32_t[n0]);
    if (!env_lights.empty() && env_scratch_.n < (size_t)M.height + 1u) env_scratch_.alloc((size_t)M.height + 1u);

    ctl_scene_image_stats st{};
    CTL_HIP(hipDeviceSynchronize());   // no trace reads the pool or the tables any more
    // ---- 1. level 0 into the image's slot of the pool
    clk::time_point t0 = clk::now();
    uint32_t* pool = texels_.p + base;
    CTL_HIP(hipMemcpy(pool, texels, n0 * 4, (flags & CTL_IMAGE_TEXELS_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    CTL_HIP(hipDeviceSynchronize());
    st.upload_ms = ms_since(t0);
    // ---- 2. the pyramid, level by level, and the one texel ImageTexture::Average() addresses
    t0 = clk::now();
    launch_mip_levels(pool, M.width, M.height, M.texel_type, L);
    uint32_t avg_texel = 0;
    {
        mip_level_table T; static_assert(sizeof(T) == sizeof(L), "one layout"); std::memcpy(&T, &L, sizeof(T));
        CTL_HIP(hipMemcpy(&avg_texel, pool + mip_average_texel_offset(M, T), 4, hipMemcpyDeviceToHost));   // (synchronises: the levels are written)
    }
    st.pyramid_ms = ms_since(t0);
    st.levels = L.levels; st.texels_written = (uint32_t)total;
    // ---- 3. BSDF::Update() of the materials that read the image's average, on the host, with the averages the scene holds of every other image
    float* avg = &image_avg_[(size_t)image * 4];
    mip_texel_decode(avg_texel, M.texel_type, avg); avg[3] = 1.0f;
    {
        image_set I; I.images = snap_->images.data(); I.n = (uint32_t)snap_->images.size(); I.cache = reinterpret_cast<float (*)[4]>(image_avg_.data());
        for (uint32_t i : reading) {
            ctl_material m = snap_->materials[i];
            material_update_textures(m, I);
            if (std::memcmp(&m, &snap_->materials[i], sizeof(m)) == 0) continue;
            // the device record is the description's with its reserved_ words set by the upload (upload_materials, tracer.hip), which needs the transmittance tables of a
            // whole description; Update() writes the sampling weight in `f` and nothing else, so those words are what is patched
            CTL_HIP(hipMemcpy(reinterpret_cast<unsigned char*>(mats_.p + i) + offsetof(ctl_material, f), m.f, sizeof(m.f), hipMemcpyHostToDevice));
            snap_->materials[i] = m; st.materials_patched++;
        }
    }
    // ---- 4. the environment light's tables
    t0 = clk::now();
    for (uint32_t li : env_lights) {
        ctl_light& Lt = snap_->lights[li];
        env_device E{ pool, reinterpret_cast<float*>(anim_.p + Lt.cdf_cols_index), reinterpret_cast<float*>(anim_.p + Lt.cdf_rows_index), reinterpret_cast<const float*>(anim_.p + Lt.row_weights_index),
                      env_scratch_.p, M.width, M.height, M.texel_type };
        hipLaunchKernelGGL(k_env_row_sums, dim3((M.height + 63u) / 64u), dim3(64), 0, nullptr, E); CTL_HIP(hipGetLastError());
        const size_t n_cols = (size_t)M.height * (M.width + 1u);
        hipLaunchKernelGGL(k_env_normalize_cols, dim3((uint32_t)((n_cols + 255u) / 256u)), dim3(256), 0, nullptr, E); CTL_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_env_rows, dim3(1), dim3(256), 0, nullptr, E); CTL_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_env_normalize_rows, dim3((M.height + 256u) / 256u), dim3(256), 0, nullptr, E); CTL_HIP(hipGetLastError());
        float rowSum = 0.0f;
        CTL_HIP(hipMemcpy(&rowSum, env_scratch_.p + M.height, 4, hipMemcpyDeviceToHost));
        Lt.normalization = env_normalization(rowSum, M.width, M.height);
        CTL_HIP(hipMemcpy(reinterpret_cast<unsigned char*>(lights_.p + li) + offsetof(ctl_light, normalization), &Lt.normalization, 4, hipMemcpyHostToDevice));
        // the snapshot's copy of the tables: what the next ctl_scene_update compares a description against
        CTL_HIP(hipMemcpy(snap_->anim.data() + Lt.cdf_cols_index, anim_.p + Lt.cdf_cols_index, n_cols * 4, hipMemcpyDeviceToHost));
        CTL_HIP(hipMemcpy(snap_->anim.data() + Lt.cdf_rows_index, anim_.p + Lt.cdf_rows_index, ((size_t)M.height + 1u) * 4, hipMemcpyDeviceToHost));
        st.env_tables++;
    }
    CTL_HIP(hipDeviceSynchronize());
    st.env_ms = env_lights.empty() ? 0.0f : ms_since(t0);
    // ---- 5. the image's digest, in every copy of the hashes the scene holds
    t0 = clk::now();
    const uint32_t* host_level0 = texels;
    if (flags & CTL_IMAGE_TEXELS_DEVICE) { CTL_HIP(hipMemcpy(level0.get(), pool, n0 * 4, hipMemcpyDeviceToHost)); host_level0 = level0.get(); }
    uint64_t words[2]; hash_image(M.width, M.height, host_level0, words);
    for (geometry_hashes* g : { &snap_->geom, &refit_.geom }) if (g->images.size() > (size_t)image * 2 + 1) { g->images[(size_t)image * 2] = words[0]; g->images[(size_t)image * 2 + 1] = words[1]; }
    st.hash_ms = ms_since(t0);
    st.total_ms = ms_since(t_all);
    if (stats) *stats = st;
}

}  // namespace ctl
