// ORACLE — TEST INFRASTRUCTURE ONLY.
// ref_pipeline_driver.cpp — extern "C" driver around the reference's own canonical image pipeline: evalFilter (Kernel/ImagePipeline/Filter/CanonicalFilter.cu:6-26) followed by
// Spectrum::toRGBE as rtm_Copy does, the per-pixel body of Reinhard05Kernel (PostProcess/ToneMapPostProcess.cu:11-22) and gammaCorrecture (ImagePipeline.cu:7-12).  `make ref`
// extracts those line ranges at build time into oracle/_ref/gen/pipeline.cpp (git-ignored) behind the reference's own headers; Spectrum::toSRGB / toYxy / fromYxy come from the
// extract of Math/Spectrum.cu (spectrum_codecs.cpp).  The Image of the tone-map body is laid out in raw storage as in ref_image_driver.cpp, here with the filtered (RGBE) and
// the processed (RGBCOL) plane bound.  This file contains no reference source.
#include <Engine/Image.h>
#include <SceneTypes/Filter.h>
#include <cstdint>
#include <cstring>

using namespace CudaTracerLib;

namespace CudaTracerLib {
void ref_reinhard_pixel(Image& img, unsigned int _x, unsigned int _y, float scale, float invWp2);                       // generated (oracle/Makefile)
Spectrum ref_eval_filter(const Filter& filter, PixelData* P, float splatScale, int x, int y, int w, int h);
RGBCOL ref_gamma_correcture(const Spectrum& c);
}

namespace {
struct sync_buffer_layout { void* vptr; int location; unsigned length; void* host; void* device; };
struct image_layout { void* vptr; int location; void* buffers[3]; int xres, yres; sync_buffer_layout pixels; void* filtered; bool owns; void* view; };   // Engine/Image.h:83-90
static_assert(sizeof(image_layout) == sizeof(Image), "member layout of Image");
static_assert(sizeof(RGBE) == 4 && sizeof(RGBCOL) == 4, "RGBE / RGBCOL are four bytes");

uint32_t word(uchar4 v) { return (uint32_t)v.x | ((uint32_t)v.y << 8) | ((uint32_t)v.z << 16) | ((uint32_t)v.w << 24); }

bool make_filter(Filter& f, int type, float xw, float yw, float p0, float p1) {
    if (type == 1) f.SetData(BoxFilter(xw, yw));
    else if (type == 2) f.SetData(GaussianFilter(xw, yw, p0));
    else if (type == 3) f.SetData(MitchellFilter(p0, p1, xw, yw));
    else if (type == 4) f.SetData(LanczosSincFilter(xw, yw, p0));
    else if (type == 5) f.SetData(TriangleFilter(xw, yw));
    else return false;
    return true;
}
}  // namespace

extern "C" {

// rtm_Copy over a w x h PixelData frame: spectrum_out = evalFilter's value per pixel (3 floats), rgbe_out = its toRGBE() word.  Returns 0, -1 on a bad argument.
int ref_pipeline_filter(void* pixels, int w, int h, float splat_scale, int type, float xw, float yw, float p0, float p1, uint32_t* rgbe_out, float* spectrum_out) {
    Filter f;
    if (!pixels || w < 1 || h < 1 || !make_filter(f, type, xw, yw, p0, p1)) return -1;
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++) {
            const Spectrum c = ref_eval_filter(f, (PixelData*)pixels, splat_scale, x, y, w, h);
            float r, g, b; c.toLinearRGB(r, g, b);
            const size_t i = (size_t)y * w + x;
            spectrum_out[3 * i] = r; spectrum_out[3 * i + 1] = g; spectrum_out[3 * i + 2] = b;
            rgbe_out[i] = word(c.toRGBE());
        }
    return 0;
}

// the Reinhard05Kernel body on one filtered pixel -> its RGBCOL word (alpha 255, so never 0).  Returns 0 when the raw Image layout does not answer the accessors.
uint32_t ref_pipeline_reinhard(uint32_t rgbe, float scale, float inv_wp2) {
    RGBE filtered[2]; RGBCOL view[2]; PixelData px[2];
    std::memset(view, 0, sizeof view);
    for (auto& v : filtered) { v.x = rgbe & 255; v.y = (rgbe >> 8) & 255; v.z = (rgbe >> 16) & 255; v.w = rgbe >> 24; }
    alignas(16) unsigned char raw[sizeof(Image)];
    image_layout L; std::memset(&L, 0, sizeof L);
    L.location = DataLocation::Synchronized; L.xres = 2; L.yres = 1;
    L.pixels.location = DataLocation::Synchronized; L.pixels.length = 2; L.pixels.host = px;
    L.filtered = filtered; L.view = view;
    std::memcpy(raw, &L, sizeof L);
    Image* img = reinterpret_cast<Image*>(raw);
    if (img->getWidth() != 2 || img->getHeight() != 1 || &img->getFilteredData(1, 0) != filtered + 1 || &img->getProcessedData(1, 0) != view + 1) return 0;
    ref_reinhard_pixel(*img, 0, 0, scale, inv_wp2);
    return word(view[0]);
}

uint32_t ref_pipeline_gamma(float r, float g, float b) { return word(ref_gamma_correcture(Spectrum(r, g, b))); }

}  // extern "C"
