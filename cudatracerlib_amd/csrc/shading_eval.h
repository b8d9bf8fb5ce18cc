// shading_eval.h — ctl_shading_eval (TEST INFRASTRUCTURE, include/ctl_amd.h): the device BSDF, emitter and texture functions of shading.h evaluated one call per
// query, so that the tests hold them to the oracle call by call.  Three builds of one shading_eval.inc mirror what the product compiles (shading_eval_*.hip).
#pragma once
#include "device_scene.h"
#include <hip/hip_runtime.h>

namespace ctl {

// `what` of ctl_shading_eval (CTL_EVAL_* of include/ctl_amd.h) with the query / result row sizes in floats; index words travel as the bits of a float
enum { kEvalBsdfSample = 0, kEvalBsdfEval = 1, kEvalBsdfSampleEval = 2, kEvalLightSample = 3, kEvalEmitterSample = 4, kEvalLightPdf = 5, kEvalLightEval = 6, kEvalEnvEval = 7,
       kEvalTexture = 8, kEvalMip = 9, kEvalNormalMap = 10, kEvalAlphaTest = 11, kEvalCount = 12 };
constexpr uint32_t kEvalQueryFloats[kEvalCount] = { 8, 10, 11, 9, 8, 14, 10, 3, 4, 7, 21, 3 };
constexpr uint32_t kEvalResultFloats[kEvalCount] = { 9, 4, 13, 15, 19, 1, 3, 3, 3, 3, 9, 1 };

// kEvalAlphaTest reads no query row on the device: ctl_shading_eval points tri_data / node_info of its copy of the scene at one synthetic triangle per query, whose three
// vertices carry the query's uv (alpha_survives takes its uv from a triangle)
// one launch of n queries (device pointers, strides in floats) on the null stream; false: this build does not carry the function
bool launch_shading_eval_basic(const dev_scene& S, int what, uint32_t n, const float* q, uint32_t q_stride, float* out, uint32_t out_stride);
bool launch_shading_eval_full(const dev_scene& S, int what, uint32_t n, const float* q, uint32_t q_stride, float* out, uint32_t out_stride);
bool launch_shading_eval_partials(const dev_scene& S, int what, uint32_t n, const float* q, uint32_t q_stride, float* out, uint32_t out_stride);

} // namespace ctl
