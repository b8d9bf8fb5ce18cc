// prim_tracer.h — the PrimTracer plugin's host class (prim_tracer.hip); its pass loop, Debug and table staging are Tracer<false>'s, from the template in tracer.hip.
#pragma once
#include "tracer.h"

namespace ctl {

// Integrators/PrimTracer.h:10-27 — PrimTracer : Tracer<false>, IDepthTracer (prim_tracer.hip): one non-progressive pass per call, 15 drawing modes
class PrimTracer : public Tracer<false> {
public:
    PrimTracer();
    void Resize(unsigned int w, unsigned int h) override;
    void InitializeScene(Scene* s) override;
    void setDepthBuffer(float* device_data, unsigned int dw, unsigned int dh) override { depth_buffer_ = device_data; depth_w_ = dw; depth_h_ = dh; }
protected:
    void DoRender(Image* I, const float* d_t1, const float* d_t2, unsigned int n_batch) override;
    void takeRayCounts(uint64_t& path_rays, uint64_t& shadow_rays_) override;
    void DebugInternal(Image* I, unsigned int x, unsigned int y, const float* d_t1, const float* d_t2, float rgb[3]) override;
private:
    void render(Image* I, const float* d_t1, const float* d_t2, float* debug_out, uint32_t dx, uint32_t dy);   // raygen -> primary traversal -> shade; debug_out: one pixel
    dbuf<float4> ro_, rd_, hit_; dbuf<int> hit_node_; dbuf<uint32_t> n_rays_, work_; dbuf<float> debug_;
    dbuf<unsigned long long> count_; unsigned long long host_count_ = 0; uint64_t total_rays_ = 0;
    float* depth_buffer_ = nullptr; unsigned int depth_w_ = 0, depth_h_ = 0;
    uint32_t n_local_pixels = 0; int grid_blocks = 0;
};

} // namespace ctl
