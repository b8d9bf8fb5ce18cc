// ORACLE — TEST INFRASTRUCTURE ONLY.
// ref_volume_driver.cpp — extern "C" driver around the reference's own participating media: BaseVolumeRegion::IntersectP, HomogeneousVolumeDensity::tau /
// sampleDistance, KernelAggregateVolume::IntersectP / tau / sampleDistance / sampleVolume / p / Sample (SceneTypes/Volumes.{h,cu}), the four phase functions
// (SceneTypes/PhaseFunction.{h,cu}), Transmittance (Kernel/TraceAlgorithms.cu:22-31) and KernelDynamicScene::evalTransmittance (Engine/KernelDynamicScene.cu:90-96).
// `make ref` builds Volumes.cu and PhaseFunction.cu whole (without their curand include) as generated units under oracle/_ref/gen/ (git-ignored; oracle/Makefile).
//
// ref_bind_volumes builds g_SceneDataHost.m_sVolume from a ctl_volume[]: every region a HomogeneousVolumeDensity through its own constructor and Update() (the
// reference inverts VolumeToWorld itself), its phase function through CreateAggregate<PhaseFunction> — Kajiya-Kay through its own constructor, so the reference
// computes its own normalisation.  Slots past the count are not touched.  ref_pathtrace_driver.cpp binds the same aggregate for a render.
//
// Where the reference's behaviour is undefined it is not called: sampleVolume with several regions indexes m_pVolumes with ffsn's bit MASK, past the table for most
// masks — the caller decides from its own restatement which rows may be sent (`sent`), and a row that is not sent is left as zeros.  A MediumSamplingRecord is
// zero-filled before each call (PathTrace's is an uninitialised local).  This file contains no reference source.
#include <Kernel/TraceHelper.h>
#include <Kernel/TraceAlgorithms.h>
#include <SceneTypes/Volumes.h>
#include <SceneTypes/PhaseFunction.h>
#include <SceneTypes/Samples.h>
#include <Math/float4x4.h>
#include "../include/ctl_amd.h"
#include <cstdint>
#include <cstring>
#include <stdexcept>

using namespace CudaTracerLib;

static_assert(sizeof(float4x4) == sizeof(ctl_float4x4), "matrix layout");

namespace {
PhaseFunction phase_of(const ctl_phase_function& F) {
    switch (F.type) {
    case CTL_PHASE_HG: return CreateAggregate<PhaseFunction>(HGPhaseFunction(F.g));
    case CTL_PHASE_ISOTROPIC: return CreateAggregate<PhaseFunction>(IsotropicPhaseFunction());
    case CTL_PHASE_KAJIYA_KAY: return CreateAggregate<PhaseFunction>(KajiyaKayPhaseFunction(F.ks, F.kd, F.exponent));
    case CTL_PHASE_RAYLEIGH: return CreateAggregate<PhaseFunction>(RayleighPhaseFunction());
    }
    throw std::runtime_error("ref_bind_volumes: unknown phase function type");
}
uint32_t index_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
void put(float* o, const Spectrum& s) { float r, g, b; s.toLinearRGB(r, g, b); o[0] = r; o[1] = g; o[2] = b; }
void put(float* o, const Vec3f& v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
void put_rec(float* o, bool ok, const MediumSamplingRecord& m) {
    o[0] = ok ? 1.0f : 0.0f; o[1] = m.t; put(o + 2, m.p); put(o + 5, m.transmittance); put(o + 8, m.sigmaA); put(o + 11, m.sigmaS);
    o[14] = m.pdfSuccess; o[15] = m.pdfSuccessRev; o[16] = m.pdfFailure;
}
}  // namespace

// g_SceneDataHost.m_sVolume from a ctl_volume[] (n <= MAX_VOL_COUNT); throws on a description the reference has no type for
void ref_bind_volumes(const ctl_volume* v, uint32_t n) {
    KernelAggregateVolume& A = g_SceneDataHost.m_sVolume;
    if (n > (uint32_t)KernelAggregateVolume::MAX_VOL_COUNT) throw std::runtime_error("ref_bind_volumes: more than MAX_VOL_COUNT regions");
    A.m_uVolumeCount = n;
    AABB box = AABB::Identity();
    for (uint32_t i = 0; i < n; i++) {
        if (v[i].type != CTL_VOLUME_HOMOGENEOUS) throw std::runtime_error("ref_bind_volumes: homogeneous regions only");
        float4x4 m; std::memcpy(&m, &v[i].volume_to_world, sizeof m);
        HomogeneousVolumeDensity H(phase_of(v[i].phase), m, Spectrum(v[i].sig_a[0], v[i].sig_a[1], v[i].sig_a[2]), Spectrum(v[i].sig_s[0], v[i].sig_s[1], v[i].sig_s[2]),
                                   Spectrum(v[i].le[0], v[i].le[1], v[i].le[2]));
        H.Update();
        A.m_pVolumes[i].SetData(H);
        box = box.Extend(A.m_pVolumes[i].WorldBound());
    }
    A.box = box;   // KernelAggregateVolume's constructor does the same; none of the driven functions reads it
}

extern "C" {

// The thirteen CTL_VEVAL_* functions over n regions, row for row in ctl_volume_eval's layout (include/ctl_amd.h): q = nq rows of CTL_VEVAL_QUERY_FLOATS floats,
// out = nq rows of CTL_VEVAL_RESULT_FLOATS floats (zeroed here).  sent[i] == 0: row i is not run (see the head of this file).  Returns 0, or -1 with the reason on stderr.
int ref_volume_eval(const ctl_volume* vols, uint32_t n, int what, const float* q, uint32_t nq, const uint8_t* sent, float* out) {
    try {
        ref_bind_volumes(vols, n);
        const KernelAggregateVolume& A = g_SceneDataHost.m_sVolume;
        std::memset(out, 0, sizeof(float) * CTL_VEVAL_RESULT_FLOATS * (size_t)nq);
        for (uint32_t i = 0; i < nq; i++) {
            if (sent && !sent[i]) continue;
            const float* a = q + (size_t)CTL_VEVAL_QUERY_FLOATS * i; float* o = out + (size_t)CTL_VEVAL_RESULT_FLOATS * i;
            const bool region = what == CTL_VEVAL_REGION_INTERSECT || what == CTL_VEVAL_REGION_TAU || what == CTL_VEVAL_REGION_SAMPLE_DISTANCE ||
                                what == CTL_VEVAL_PHASE_EVAL || what == CTL_VEVAL_PHASE_SAMPLE;
            const uint32_t vi = region ? index_of(a[0]) : 0;
            if (region && vi >= n) throw std::runtime_error("ref_volume_eval: region index out of range");
            const float* b = region ? a + 1 : a;
            const Vec3f v0(b[0], b[1], b[2]), v1(b[3], b[4], b[5]);
            MediumSamplingRecord mRec; std::memset((void*)&mRec, 0, sizeof mRec);
            switch (what) {
            case CTL_VEVAL_REGION_INTERSECT: { float t0 = 0, t1 = 0; const bool h = A.m_pVolumes[vi].IntersectP(Ray(v0, v1), b[6], b[7], &t0, &t1); o[0] = h; o[1] = h ? t0 : 0; o[2] = h ? t1 : 0; break; }
            case CTL_VEVAL_INTERSECT: { float t0 = 0, t1 = 0; o[0] = A.IntersectP(Ray(v0, v1), b[6], b[7], &t0, &t1); o[1] = t0; o[2] = t1; break; }
            case CTL_VEVAL_REGION_TAU: put(o, A.m_pVolumes[vi].tau(Ray(v0, v1), b[6], b[7])); break;
            case CTL_VEVAL_TAU: put(o, A.tau(Ray(v0, v1), b[6], b[7])); break;
            case CTL_VEVAL_REGION_SAMPLE_DISTANCE: { const bool ok = A.m_pVolumes[vi].sampleDistance(Ray(v0, v1), b[6], b[7], b[8], mRec); put_rec(o, ok, mRec); break; }
            case CTL_VEVAL_SAMPLE_DISTANCE: { const bool ok = A.sampleDistance(Ray(v0, v1), b[6], b[7], b[8], mRec); put_rec(o, ok, mRec); break; }
            case CTL_VEVAL_SAMPLE_VOLUME: {
                float s = b[8], pdf = 0;
                const VolumeRegion* R = A.sampleVolume(Ray(v0, v1), b[6], b[7], s, pdf);
                o[0] = R ? (float)(R - A.m_pVolumes) : -1.0f; o[1] = s; o[2] = pdf; break;
            }
            case CTL_VEVAL_PHASE_EVAL: {
                PhaseFunctionSamplingRecord pRec(NormalizedT<Vec3f>(b[0], b[1], b[2]), NormalizedT<Vec3f>(b[3], b[4], b[5]));
                o[0] = A.m_pVolumes[vi].As()->Func.Evaluate(pRec); break;
            }
            case CTL_VEVAL_PHASE_SAMPLE: {
                PhaseFunctionSamplingRecord pRec(NormalizedT<Vec3f>(b[0], b[1], b[2]), NormalizedT<Vec3f>(0.0f, 0.0f, 0.0f)); float pdf = 0;
                o[0] = A.m_pVolumes[vi].As()->Func.Sample(pRec, pdf, Vec2f(b[3], b[4])); o[1] = pdf; put(o + 2, pRec.wo); break;
            }
            case CTL_VEVAL_P: {
                PhaseFunctionSamplingRecord pRec(NormalizedT<Vec3f>(b[3], b[4], b[5]), NormalizedT<Vec3f>(b[6], b[7], b[8]));
                o[0] = A.p(v0, pRec); break;
            }
            case CTL_VEVAL_SAMPLE: {
                PhaseFunctionSamplingRecord pRec(NormalizedT<Vec3f>(b[3], b[4], b[5]), NormalizedT<Vec3f>(0.0f, 0.0f, 0.0f)); float pdf = 0;
                o[0] = A.Sample(v0, pRec, pdf, Vec2f(b[6], b[7])); o[1] = pdf; put(o + 2, pRec.wo); break;
            }
            case CTL_VEVAL_TRANSMITTANCE: put(o, Transmittance(Ray(v0, v1), b[6], b[7])); break;
            case CTL_VEVAL_EVAL_TRANSMITTANCE: put(o, g_SceneDataHost.evalTransmittance(v0, v1)); break;
            default: throw std::runtime_error("ref_volume_eval: unknown function");
            }
        }
        g_SceneDataHost.m_sVolume.m_uVolumeCount = 0;
        return 0;
    } catch (const std::exception& e) { g_SceneDataHost.m_sVolume.m_uVolumeCount = 0; std::fprintf(stderr, "%s\n", e.what()); return -1; }
}

// KajiyaKayPhaseFunction::m_normalization as its own constructor's Update() computes it (PhaseFunction.cu:64-77: cosf / sinf / math::pow, glibc on the host)
float ref_kajiya_kay_normalization(float ks, float kd, float exponent) { return KajiyaKayPhaseFunction(ks, kd, exponent).m_normalization; }

}  // extern "C"
