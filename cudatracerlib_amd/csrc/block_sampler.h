// block_sampler.h — the reference's block samplers and pixel-variance buffer behind `Tracer<true>` (Kernel/BlockSampler/*.h,
// Kernel/PixelVarianceBuffer.{h,cu}, Kernel/Tracer.h:209-248): every pass, a sampler decides how many samples each 64x64-pixel block of the
// film gets (0, 1 or 2) from statistics of the frame so far.  Blocks are this build's image tiles (BLOCK_SAMPLER_BlockSize = 32 *
// BLOCK_FACTOR = 64 in the reference's default build, IBlockSampler_device.h:7-22), flattened as block_y * blocks_x + block_x.
//   Uniform     every block once per pass; with user weights: the heaviest first, weight <= 0 never (UniformBlockSampler.h)
//   Variance    after 10 uniform passes: the quarter of the blocks with the largest weight 0.85 sigma_estimator + 0.15 sigma_colour
//               (both min-max normalised over the blocks) plus every second block in turn (VarianceBlockSampler.{h,cu}, MixedBlockIterate)
//   Difference  the same scheme on the mean per-pixel error |I - A| / sqrt(I) between the frame and its half buffer (DifferenceBlockSampler)
//   Select      only the blocks the user gave a weight (SelectBlockSampler.h)
// Statistics are reduced on the device (one workgroup per block), the ordering is done on the host as in the reference.
#pragma once
#include "../../include/ctl_amd.h"
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

namespace ctl {

constexpr uint32_t kSamplerBlock = 64;

// PixelVarianceInfo (Kernel/PixelVarianceBuffer.h:10-63)
struct pixel_variance { float prev_I[3]; float half_buffer[3]; int iterations_done; float weight; float sum_x, sum_x2; int num_samples_var; int pad_; };
#if defined(__HIPCC__)
// PixelVarianceInfo::updateMoments (PixelVarianceBuffer.h:21-41) for a pixel whose sum after the pass is (n0, n1, n2) = rgb + rgbSplat * splatScale and which got
// `performed` >= 1 samples in it.  Shared by the update kernel (block_sampler.hip) and the batch resolve of the wavefront tracer (kernels.hip)
__device__ __forceinline__ void update_moments(pixel_variance& v, float n0, float n1, float n2, float weight_sum, float performed) {
    const float e0 = (n0 - v.prev_I[0]) / performed, e1 = (n1 - v.prev_I[1]) / performed, e2 = (n2 - v.prev_I[2]) / performed;
    v.prev_I[0] = n0; v.prev_I[1] = n1; v.prev_I[2] = n2;
    v.weight = weight_sum;
    if (v.iterations_done++ % 2 == 1) { v.half_buffer[0] += e0; v.half_buffer[1] += e1; v.half_buffer[2] += e2; }
    const float l = e0 * 0.212671f + e1 * 0.715160f + e2 * 0.072169f;
    v.sum_x += l; v.sum_x2 += l * l; v.num_samples_var++;
}
#endif
// per block: VarianceBlockSampler::TmpBlockInfo + DifferenceBlockSampler::blockInfo
struct block_stats { float var_i; uint32_t n_var; float e_i, e_i2; uint32_t n_e; float sum_err; uint32_t n_err; uint32_t pad_; };

// PixelVarianceBuffer (Kernel/PixelVarianceBuffer.{h,cu}): the per-pixel moments, owned by the tracer (Tracer.h:151) and read by the block samplers and by the
// NonLocalMeans filter (nlm_filter.hip)
class PixelVarianceBuffer {
public:
    PixelVarianceBuffer(uint32_t w, uint32_t h);
    ~PixelVarianceBuffer();
    PixelVarianceBuffer(const PixelVarianceBuffer&) = delete; PixelVarianceBuffer& operator=(const PixelVarianceBuffer&) = delete;
    uint32_t width() const { return w_; }
    uint32_t height() const { return h_; }
    const pixel_variance* device() const { return d_var_; }
    pixel_variance* device() { return d_var_; }
    void clear(hipStream_t s);                                // PixelVarianceBuffer::Clear
    // PixelVarianceBuffer::AddPass: updateMoments of every pixel whose 64x64 block was sampled in this pass.  d_counts = samples per block on the device,
    // or nullptr: every block once.  Asynchronous on `s`
    void add_pass(const ctl_pixel_data* image, float splat_scale, const unsigned char* d_counts, hipStream_t s);
    // PixelVarianceInfo::computeVariance of every pixel into w * h floats on the device (NaN where num_samples_var is 0).  Asynchronous on `s`
    void compute_variance(float* d_out, hipStream_t s) const;
private:
    uint32_t w_, h_; pixel_variance* d_var_ = nullptr;
};

class BlockSampler {
public:
    enum Type { Uniform = 0, Variance = 1, Difference = 2, Select = 3 };
    BlockSampler(Type t, uint32_t w, uint32_t h);
    ~BlockSampler();
    BlockSampler(const BlockSampler&) = delete; BlockSampler& operator=(const BlockSampler&) = delete;
    Type type() const { return type_; }
    uint32_t blocks_x() const { return bx_; }
    uint32_t width() const { return w_; }
    uint32_t height() const { return h_; }
    uint32_t n_blocks() const { return bx_ * by_; }
    bool every_block_once() const;                            // the plain uniform case: nothing to do per pass
    void set_weight(uint32_t block_x, uint32_t block_y, float w);   // IUserPreferenceSampler::setWeight
    float get_weight(uint32_t block_x, uint32_t block_y) const;
    int fraction_deterministic = 2, fraction_weighted = 4;   // KEY_FractionDeterministic / KEY_FractionWeighted (IBlockSampler.h:157-163)

    void start_new_rendering() { passes_done_ = 0; }          // StartNewRendering (the tracer clears its PixelVarianceBuffer)
    // IterateBlocks -> BlockSamplerBuffer::Update (BlockSamplerBuffer.h:32-49): samples per block for the NEXT pass
    void counts(std::vector<unsigned char>& per_block) const;
    const unsigned char* upload_counts(const std::vector<unsigned char>& per_block, hipStream_t s);
    // after a pass and the tracer's PixelVarianceBuffer::add_pass: sampler->AddPass(img, tracer, varBuffer) (Tracer.h:233-237).
    // Synchronises the stream (the reference reads the block statistics back on the host here too).
    void add_pass(const PixelVarianceBuffer& var, const std::vector<unsigned char>& per_block, hipStream_t s);
    const std::vector<unsigned char>& last_counts() const { return last_counts_; }
    const std::vector<block_stats>& last_stats() const { return stats_host_; }
private:
    Type type_; uint32_t w_, h_, bx_, by_;
    std::vector<float> user_w_; std::vector<int> indices_; bool non_zero_ = false;
    unsigned int passes_done_ = 0;                            // m_uPassesDone of the Variance / Difference samplers
    block_stats* d_stats_ = nullptr; unsigned char* d_counts_ = nullptr;
    std::vector<block_stats> stats_host_; std::vector<unsigned char> last_counts_;
    void mixed(std::vector<unsigned char>& c) const;
};

} // namespace ctl
