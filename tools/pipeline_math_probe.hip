// pipeline_math_probe.hip — measured accuracy of the device functions the image pipeline calls (csrc/image_pipeline.hip): powf(v, 1 / 2.4) of the sRGB curve,
// expf of the Gaussian filter, sinf of the Lanczos filter, logf of the luminance info.  Each against the host's double function, in units of the last place of the
// fp32 result.  tests/test_gpu_image_pipeline.py takes its powf margin from the figure this prints (RESULTS.md).
//   hipcc -O3 -ffp-contract=off --offload-arch=gfx950 tools/pipeline_math_probe.hip -o tools/pipeline_math_probe.bin && tools/pipeline_math_probe.bin
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(c) do { hipError_t e_ = (c); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #c, hipGetErrorString(e_)); return 1; } } while (0)

__global__ void k_eval(const float* __restrict__ in, int n, int fn, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = in[i];
    out[i] = fn == 0 ? powf(v, (float)(1.0 / 2.4)) : fn == 1 ? expf(v) : fn == 2 ? sinf(v) : logf(v);
}

static double ulp_of(float r) { int e; std::frexp((double)r, &e); return std::ldexp(1.0, e - 24); }

int main() {
    const int n = 1 << 22;
    const char* names[4] = { "powf(v, 1/2.4), v in [0.0031308, 1]", "expf(v), v in [-20, 20]", "sinf(v), v in [0, 60]", "logf(v), v in [2.3e-5, 1e5]" };
    std::vector<float> in(n), out(n);
    float *din, *dout;
    CHECK(hipMalloc(&din, n * sizeof(float))); CHECK(hipMalloc(&dout, n * sizeof(float)));
    for (int fn = 0; fn < 4; fn++) {
        for (int i = 0; i < n; i++) {
            const double t = (i + 0.5) / n;
            in[i] = fn == 0 ? (float)std::exp(std::log(0.0031308) * (1 - t)) : fn == 1 ? (float)(-20 + 40 * t) : fn == 2 ? (float)(60 * t) : (float)std::exp(std::log(2.3e-5) + t * (std::log(1e5) - std::log(2.3e-5)));
        }
        CHECK(hipMemcpy(din, in.data(), n * sizeof(float), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_eval, dim3((n + 255) / 256), dim3(256), 0, nullptr, din, n, fn, dout);
        CHECK(hipGetLastError()); CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(out.data(), dout, n * sizeof(float), hipMemcpyDeviceToHost));
        double worst = 0; float at = 0;
        for (int i = 0; i < n; i++) {
            const double x = in[i];
            const double want = fn == 0 ? std::pow(x, (double)(float)(1.0 / 2.4)) : fn == 1 ? std::exp(x) : fn == 2 ? std::sin(x) : std::log(x);
            // sinf near a multiple of pi: the result's own ulp shrinks with it; measure against the ulp of max(|want|, 2^-10) so a tiny result does not inflate the figure
            const double err = std::fabs((double)out[i] - want) / ulp_of((float)std::fmax(std::fabs(want), fn == 2 ? 0x1p-10 : 0.0));
            if (err > worst) { worst = err; at = in[i]; }
        }
        std::printf("%-40s max error %.3f ulp (at %.9g)\n", names[fn], worst, at);
    }
    // GaussianFilter::Update evaluates exp(-alpha * width^2) on the host, Evaluate on the device: do the two agree where a tap lies exactly on the filter's edge?
    const float edge[8] = { 8.0f, -8.0f, 2.0f, -2.0f, 72.0f, -72.0f, 4.5f, -4.5f };
    CHECK(hipMemcpy(din, edge, sizeof edge, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_eval, dim3(1), dim3(256), 0, nullptr, din, 8, 1, dout);
    CHECK(hipGetLastError()); CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), dout, sizeof edge, hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; i++) std::printf("expf(%g): device %.9g host %.9g %s\n", edge[i], out[i], std::exp(edge[i]), out[i] == std::exp(edge[i]) ? "same" : "DIFFERENT");
    (void)hipFree(din); (void)hipFree(dout);
    return 0;
}
