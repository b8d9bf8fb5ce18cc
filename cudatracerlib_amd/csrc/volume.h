// volume.h — participating media: the homogeneous regions, their aggregate (which dispatches to the VolumeGrid regions of volume_grid.h) and the four phase functions of the reference (SceneTypes/Volumes.{h,cu},
// SceneTypes/PhaseFunction.{h,cu}, Kernel/TraceAlgorithms.cu:22-31, Engine/KernelDynamicScene.cu:90-96), single source for the megakernel's MEDIA instantiation
// (megakernel.hip), the call-by-call kernel and the host yardstick (ctl_volume_eval, volume_eval.hip).  fp32 throughout, the operation order of the reference's source
// (the library is built -ffp-contract=off), transcendental functions from ctl_fmath.h on the host AND on the device — never libm — so that the two agree bit for bit.
// The reference's oddities are restated, not repaired; each is marked where it stands.
#pragma once
#include "../../include/ctl_amd.h"
#include "ctl_math.h"
#include <cstring>
#include <vector>

namespace ctl {
namespace vol {

// KernelAggregateVolume as a kernel argument: the regions stay in global memory and are read with wave-uniform indices (scalar loads).  KernelAggregateVolume::box is
// not carried: none of the reference's functions restated here reads it (IntersectP, tau and sampleVolume walk the regions), and a box test in front of them would be
// arithmetic the reference does not do
// A CTL_VOLUME_GRID region's record (ctl_volume_grid) as the kernels read it: slot i of `g` belongs to region i (CTL_MAX_VOL_COUNT slots, zeros for the other regions),
// the grids' floats lie in ONE buffer `cells` at the record's offsets (pack_grids below).  g / cells are null in a table without grids; only the GRID = true
// instantiations of the functions below read them
struct grid_rec { uint32_t single; uint32_t dim[3], dim_a[3], dim_s[3]; uint32_t off, off_a, off_s; float sa_min[3], sa_max[3], ss_min[3], ss_max[3]; };
struct table { const ctl_volume* v; uint32_t n; const grid_rec* g; const float* cells; };

struct medium_rec {   // MediumSamplingRecord (Volumes.h:13-24) without the fields nothing reads
    float t; f3 p; f3 transmittance, sigmaA, sigmaS; float pdfSuccess, pdfSuccessRev, pdfFailure;
};

// a record with every field 0.  The reference's PathTrace reads mRec.transmittance / pdfFailure of a record that nothing may have written yet (the aggregate finds no
// region to sample although IntersectP found the ray inside the medium): uninitialised memory there, zeros here — the division 0 / 0 poisons the sample, which
// Image::AddSample then drops
HD medium_rec zero_rec() { medium_rec m; m.t = 0; m.p = f3(0.0f); m.transmittance = m.sigmaA = m.sigmaS = f3(0.0f); m.pdfSuccess = m.pdfSuccessRev = m.pdfFailure = 0; return m; }
HD f3 a3(const float* a) { return f3(a[0], a[1], a[2]); }
HD float ssum(f3 s) { float r = 0.0f; r += s.x; r += s.y; r += s.z; return r; }   // TSpectrum::sum (Spectrum.h:185-190)
HD float savg(f3 s) { return ssum(s) * (1.0f / 3); }                                // TSpectrum::avg (:180-182)
HD f3 sexp(f3 s) { return f3(fm::exp(s.x), fm::exp(s.y), fm::exp(s.z)); }           // TSpectrum::exp (:225-230)
HD float chan(f3 s, uint32_t i) { return i == 0 ? s.x : (i == 1 ? s.y : s.z); }

// float4x4::TransformPoint / TransformDirection (Math/float4x4.h:398-408) of a general matrix: the point is divided by its own w
HD float row4(const float* r, f3 p, float w) { float s = 0.0f; s += r[0] * p.x; s += r[1] * p.y; s += r[2] * p.z; s += r[3] * w; return s; }   // Vec4f::dot: from 0, in component order
HD f3 transform_point(const float* m, f3 p) { const float w = row4(m + 12, p, 1.0f); return f3(row4(m, p, 1.0f) / w, row4(m + 4, p, 1.0f) / w, row4(m + 8, p, 1.0f) / w); }
HD f3 transform_direction(const float* m, f3 d) { return f3(row4(m, d, 0.0f), row4(m + 4, d, 0.0f), row4(m + 8, d, 0.0f)); }

// kepler_math::spanBeginKepler / spanEndKepler (Math/MathFunc.h:405-444): the inner min / max compare the floats' BITS as signed integers (vmin.s32 / vmax.s32; the
// host branch does the same on the reinterpreted ints) — two negative values order the other way round, a NaN orders by its bit pattern
HD int fbits(float f) { return __builtin_bit_cast(int, f); }
HD float bfloat(int i) { return __builtin_bit_cast(float, i); }
HD int imin(int a, int b) { return a < b ? a : b; }
HD int imax(int a, int b) { return a > b ? a : b; }
HD float span_begin(float a0, float a1, float b0, float b1, float c0, float c1, float d) {
    const float c = bfloat(imax(imin(fbits(c0), fbits(c1)), fbits(d)));                       // fmin_fmax
    return bfloat(imax(imax(fbits(min2(a0, a1)), fbits(min2(b0, b1))), fbits(c)));           // fmax_fmax
}
HD float span_end(float a0, float a1, float b0, float b1, float c0, float c1, float d) {
    const float c = bfloat(imin(imax(fbits(c0), fbits(c1)), fbits(d)));                       // fmax_fmin
    return bfloat(imin(imin(fbits(max2(a0, a1)), fbits(max2(b0, b1))), fbits(c)));           // fmin_fmin
}
// AABB::Intersect<true>(ray, &min, &max) (Math/AABB.h:142-158): the bounds are read, and written only on a hit
HD bool aabb_intersect(f3 lo, f3 hi, f3 o, f3 d, float& mn, float& mx) {
    const float tx1 = (lo.x - o.x) / d.x, tx2 = (hi.x - o.x) / d.x;
    const float ty1 = (lo.y - o.y) / d.y, ty2 = (hi.y - o.y) / d.y;
    const float tz1 = (lo.z - o.z) / d.z, tz2 = (hi.z - o.z) / d.z;
    const float mi = span_begin(tx1, tx2, ty1, ty2, tz1, tz2, mn);
    const float ma = span_end(tx1, tx2, ty1, ty2, tz1, tz2, mx);
    const bool b = ma > mi && ma > 0;
    if (b) { mn = mi; mx = ma; }
    return b;
}
HD f3 vmin(f3 a, f3 b) { return f3(min2(a.x, b.x), min2(a.y, b.y), min2(a.z, b.z)); }
HD f3 vmax(f3 a, f3 b) { return f3(max2(a.x, b.x), max2(a.y, b.y), max2(a.z, b.z)); }
// VolumeRegion::WorldBound (Volumes.h:253-256): AABB(0, 1).Transform(VolumeToWorld) (Math/AABB.h:32-45)
HD void world_bound(const ctl_volume& V, f3& lo, f3& hi) {
    const float* m = V.volume_to_world.m;
    const f3 right = transform_direction(m, f3(1.0f, 0.0f, 0.0f)), up = transform_direction(m, f3(0.0f, 1.0f, 0.0f)), fwd = transform_direction(m, f3(0.0f, 0.0f, 1.0f));
    const f3 xa = right * 0.0f, xb = right * 1.0f, ya = up * 0.0f, yb = up * 1.0f, za = fwd * 0.0f, zb = fwd * 1.0f;
    const f3 tr = transform_point(m, f3(0.0f));
    lo = vmin(xa, xb) + vmin(ya, yb) + vmin(za, zb) + tr;
    hi = vmax(xa, xb) + vmax(ya, yb) + vmax(za, zb) + tr;
}
HD bool aabb_contains(f3 lo, f3 hi, f3 p) { return lo.x <= p.x && p.x <= hi.x && lo.y <= p.y && p.y <= hi.y && lo.z <= p.z && p.z <= hi.z; }
// BaseVolumeRegion::insideWorld (Volumes.h:35-40)
HD bool inside_world(const ctl_volume& V, f3 p) {
    const f3 pl = transform_point(V.world_to_volume.m, p);
    return pl.x >= 0 && pl.y >= 0 && pl.z >= 0 && pl.x <= 1 && pl.y <= 1 && pl.z <= 1;
}
// BaseVolumeRegion::IntersectP (Volumes.cu:8-18): t0 / t1 are written on a hit only
HD bool region_intersect(const ctl_volume& V, f3 o, f3 d, float minT, float maxT, float& t0, float& t1) {
    const f3 ol = transform_point(V.world_to_volume.m, o), dl = transform_direction(V.world_to_volume.m, d);
    const bool b = aabb_intersect(f3(0.0f), f3(1.0f), ol, dl, minT, maxT);
    if (b) { t0 = minT; t1 = maxT; }
    return b;
}
// HomogeneousVolumeDensity::tau (Volumes.cu:19-27)
HD f3 region_tau(const ctl_volume& V, f3 o, f3 d, float minT, float maxT) {
    float t0, t1;
    if (!region_intersect(V, o, d, minT, maxT, t0, t1)) return f3(0.0f);
    return length((o + t0 * d) - (o + t1 * d)) * (a3(V.sig_a) + a3(V.sig_s));
}
// HomogeneousVolumeDensity::sampleDistance (Volumes.cu:28-74).  As written: the distance is sampled over the WHOLE [minT, maxT] the caller hands in — the region's box
// never clips it; the sampling weight starts at -1, takes the largest albedo among the channels with sig_t != 0 and is raised to 0.5 only when positive (sig_s = 0: weight 0,
// no distance is ever sampled, pdfFailure = 1; sig_t = 0: the albedo is NaN, the weight stays -1)
HD bool region_sample_distance(const ctl_volume& V, f3 o, f3 d, float minT, float maxT, float rand, medium_rec& mRec) {
    float m_mediumSamplingWeight = -1;
    const f3 sig_a = a3(V.sig_a), sig_s = a3(V.sig_s);
    const f3 sig_t = sig_a + sig_s, albedo = sig_s / sig_t;
    for (uint32_t i = 0; i < 3; i++)
        if (chan(albedo, i) > m_mediumSamplingWeight && chan(sig_t, i) != 0) m_mediumSamplingWeight = chan(albedo, i);
    if (m_mediumSamplingWeight > 0) m_mediumSamplingWeight = max2(m_mediumSamplingWeight, 0.5f);
    float sampledDistance = FLT_MAX;
    if (rand < m_mediumSamplingWeight) {
        rand /= m_mediumSamplingWeight;
        const uint32_t channel = (uint32_t)(int)(rand * 3);   // MonteCarlo::sampleReuse(N, pdf, slot) (MonteCarlo.cu:16-20); rand < 1, so the channel is 0..2
        rand = rand * 3 - channel;
        const float samplingDensity = chan(sig_t, channel);
        sampledDistance = -fm::log(1 - rand) / samplingDensity;
    }
    bool success = true;
    if (sampledDistance < maxT - minT) {
        mRec.t = minT + sampledDistance;
        mRec.p = o + mRec.t * d;
        mRec.sigmaA = sig_a;
        mRec.sigmaS = sig_s;
        if (mRec.p.x == o.x && mRec.p.y == o.y && mRec.p.z == o.z) success = false;
    } else {
        sampledDistance = maxT - minT;
        success = false;
    }
    const f3 tmp = sexp(-sig_t * sampledDistance);
    mRec.pdfFailure = savg(tmp);
    mRec.pdfSuccess = savg(sig_t * tmp);
    mRec.transmittance = sexp(sig_t * (-sampledDistance));
    mRec.pdfSuccessRev = mRec.pdfSuccess = mRec.pdfSuccess * m_mediumSamplingWeight;
    mRec.pdfFailure = m_mediumSamplingWeight * mRec.pdfFailure + (1 - m_mediumSamplingWeight);
    if (max3c(mRec.transmittance) < 1e-8f) mRec.transmittance = f3(0.0f);
    return success;
}

}  // namespace vol
}  // namespace ctl
#include "volume_grid.h"
namespace ctl {
namespace vol {

// ---- VolumeRegion's dispatch on the type (CALLER(tau), CALLER(sampleDistance), CALLER(sigma_s), Volumes.h:289-337).  GRID = false is the code of a table without grid
// regions — what it was before VolumeGrid was carried, so that the kernels of such scenes keep their code; GRID = true adds the type test
template <bool GRID> HD f3 region_tau_d(const table& T, uint32_t i, f3 o, f3 d, float minT, float maxT) {
    if constexpr (GRID) { if (T.v[i].type == CTL_VOLUME_GRID) return grid_tau(region_of(T, i), o, d, minT, maxT); }
    return region_tau(T.v[i], o, d, minT, maxT);
}
template <bool GRID> HD bool region_sample_distance_d(const table& T, uint32_t i, f3 o, f3 d, float minT, float maxT, float rand, medium_rec& mRec) {
    if constexpr (GRID) { if (T.v[i].type == CTL_VOLUME_GRID) return grid_sample_distance(region_of(T, i), o, d, minT, maxT, rand, mRec); }
    return region_sample_distance(T.v[i], o, d, minT, maxT, rand, mRec);
}
template <bool GRID> HD f3 region_sigma_s_d(const table& T, uint32_t i, f3 p) {
    if constexpr (GRID) { if (T.v[i].type == CTL_VOLUME_GRID) return grid_sigma_s(region_of(T, i), p); }
    return inside_world(T.v[i], p) ? a3(T.v[i].sig_s) : f3(0.0f);
}

// ---- KernelAggregateVolume (Volumes.cu:219-336)
HD bool intersect(const table& T, f3 o, f3 d, float minT, float maxT, float& t0, float& t1) {
    t0 = FLT_MAX; t1 = -FLT_MAX;
    for (uint32_t i = 0; i < T.n; i++) {
        float a, b;
        if (region_intersect(T.v[i], o, d, minT, maxT, a, b)) { t0 = min2(t0, a); t1 = max2(t1, b); }
    }
    return t0 < t1;
}
template <bool GRID = false> HD f3 tau(const table& T, f3 o, f3 d, float minT, float maxT) {
    f3 s(0.0f);
    for (uint32_t i = 0; i < T.n; i++) s = s + region_tau_d<GRID>(T, i, o, d, minT, maxT);
    return s;
}
// ffsn (Volumes.cu:303-308): the n-th set bit as a MASK — which sampleVolume then uses as an index, as written
HD int ffsn(unsigned int v, int n) { for (int i = 0; i < n - 1; i++) v &= v - 1; return (int)(v & ~(v - 1)); }
// KernelAggregateVolume::sampleVolume (Volumes.cu:310-336): -1 = none.  minT / maxT travel by value.  With one region the sample is untouched; with more, sampleReuse
// rescales it and `nth` (0-based) goes into ffsn (1-based) whose result, a bit mask, indexes the table: as written.  An index past the table reads nothing here (-1);
// the reference reads whatever follows its array
HD int sample_volume(const table& T, f3 o, f3 d, float minT, float maxT, float& sample, float& pdf) {
    if (T.n == 0) return -1;
    if (T.n == 1) { f3 lo, hi; world_bound(T.v[0], lo, hi); return aabb_intersect(lo, hi, o, d, minT, maxT) ? 0 : -1; }
    unsigned int n = 0, flag = 0;
    for (uint32_t i = 0; i < T.n; i++) {
        float a = minT, b = maxT; f3 lo, hi; world_bound(T.v[i], lo, hi);
        if (aabb_intersect(lo, hi, o, d, a, b)) { n++; flag |= 1u << i; }
    }
    if (!n) return -1;
    const unsigned int nth = (unsigned int)(int)(sample * n);
    sample = sample * n - nth;
    const int i = ffsn(flag, (int)nth);
    pdf = 1.0f / n;
    return (i >= 0 && (uint32_t)i < T.n) ? i : -1;
}
template <bool GRID = false> HD bool sample_distance(const table& T, f3 o, f3 d, float minT, float maxT, float sample, medium_rec& mRec) {
    float vol_sample_pdf = 0;
    const int vi = sample_volume(T, o, d, minT, maxT, sample, vol_sample_pdf);
    return vi >= 0 && region_sample_distance_d<GRID>(T, (uint32_t)vi, o, d, minT, maxT, sample, mRec);
}

// ---- phase functions (PhaseFunction.cu)
HD f3 square_to_uniform_sphere(f2 s) {   // Warp.h:29-36
    const float z = 1.0f - 2.0f * s.y, r = sqrtf(1.0f - z * z);
    float sinPhi, cosPhi; fm::sincos(2.0f * kPi * s.x, &sinPhi, &cosPhi);
    return f3(r * cosPhi, r * sinPhi, z);
}
HD frame frame_of(f3 n) { frame f; f.n = n; coordinate_system(n, f.s, f.t); return f; }   // Frame(n) (Math/Frame.h:32-34)
HD float phase_eval(const ctl_phase_function& F, f3 wi, f3 wo) {
    switch (F.type) {
    case CTL_PHASE_HG: {
        const float temp = 1.0f + F.g * F.g + 2.0f * F.g * dot(wi, wo);
        return (1.0f / (4.0f * kPi)) * (1 - F.g * F.g) / (temp * sqrtf(temp));
    }
    case CTL_PHASE_KAJIYA_KAY: {
        if (max3c(wi) == 0) return F.kd / (4 * kPi);
        const frame fr = frame_of(wi);
        f3 reflectedLocal = fr.to_local(wo);
        reflectedLocal.z = -dot(wi, fr.n);
        const float a = sqrtf((1 - reflectedLocal.z * reflectedLocal.z) / (reflectedLocal.x * reflectedLocal.x + reflectedLocal.y * reflectedLocal.y));
        reflectedLocal.y *= a;
        reflectedLocal.x *= a;
        const f3 R = fr.to_world(reflectedLocal);
        return fm::pow(max2(0.0f, dot(R, wo)), F.exponent) * F.normalization * F.ks + F.kd / (4 * kPi);
    }
    case CTL_PHASE_RAYLEIGH: {
        const float mu = dot(wi, wo);
        return (3.0f / (16.0f * kPi)) * (1 + mu * mu);
    }
    default: return 1.0f / (4.0f * kPi);   // isotropic: Warp::squareToUniformSpherePdf
    }
}
// PhaseFunction::Sample(pRec, pdf, sample): returns the weight, writes wo and the pdf.  Rayleigh as written: pow of a negative base is NaN and propagates
HD float phase_sample(const ctl_phase_function& F, f3 wi, f3& wo, float& pdf, f2 sample) {
    switch (F.type) {
    case CTL_PHASE_HG: {
        float cosTheta;
        if (fabsf(F.g) < 0.000001f) cosTheta = 1 - 2 * sample.x;
        else {
            const float sqrTerm = (1 - F.g * F.g) / (1 - F.g + 2 * F.g * sample.x);
            cosTheta = (1 + F.g * F.g - sqrTerm * sqrTerm) / (2 * F.g);
        }
        const float sinTheta = sqrtf(1.0f - cosTheta * cosTheta);
        float sinPhi, cosPhi; fm::sincos(2 * kPi * sample.y, &sinPhi, &cosPhi);
        wo = frame_of(-wi).to_world(f3(sinTheta * cosPhi, sinTheta * sinPhi, cosTheta));
        pdf = phase_eval(F, wi, wo);
        return 1.0f;
    }
    case CTL_PHASE_KAJIYA_KAY:
        wo = square_to_uniform_sphere(sample);
        pdf = 1.0f / (4.0f * kPi);
        return phase_eval(F, wi, wo) * (4 * kPi);
    case CTL_PHASE_RAYLEIGH: {
        const float z = 2 * (2 * sample.x - 1), tmp = sqrtf(z * z + 1);
        const float A = fm::pow(z + tmp, (float)(1.0f / 3.0f)), B = fm::pow(z - tmp, (float)(1.0f / 3.0f));
        const float cosTheta = A + B, sinTheta = sqrtf(1.0f - cosTheta * cosTheta), phi = 2 * kPi * sample.y;
        float sinPhi, cosPhi; fm::sincos(phi, &sinPhi, &cosPhi);
        wo = frame_of(-wi).to_world(f3(sinTheta * cosPhi, sinTheta * sinPhi, cosTheta));
        pdf = phase_eval(F, wi, wo);
        return 1.0f;
    }
    default:
        wo = square_to_uniform_sphere(sample);
        pdf = 1.0f / (4.0f * kPi);
        return 1.0f;
    }
}
// KernelAggregateVolume::p (Volumes.cu:278-289): weighted by the regions' average sigma_s, over the regions whose WorldBound() holds the point — 0 outside all of them
template <bool GRID = false> HD float phase_p(const table& T, f3 p, f3 wi, f3 wo) {
    float ph = 0, sumWt = 0;
    for (uint32_t i = 0; i < T.n; i++) {
        f3 lo, hi; world_bound(T.v[i], lo, hi);
        if (aabb_contains(lo, hi, p)) {
            const float wt = savg(region_sigma_s_d<GRID>(T, i, p));
            sumWt += wt;
            ph += wt * phase_eval(T.v[i].phase, wi, wo);
        }
    }
    return sumWt != 0 ? ph / sumWt : 0.0f;
}
// KernelAggregateVolume::Sample (Volumes.cu:269-277): the region comes from sampleVolume(Ray(p, wi), 0, FLT_MAX, sample.x, ...); none: 0, and wo stays as it was
HD float phase_sample_aggregate(const table& T, f3 p, f3 wi, f3& wo, float& pdf, f2 sample) {
    float vol_sample_pdf = 0;
    const int vi = sample_volume(T, p, wi, 0.0f, FLT_MAX, sample.x, vol_sample_pdf);
    if (vi >= 0) return phase_sample(T.v[vi].phase, wi, wo, pdf, sample);
    return 0.0f;
}
// Transmittance (Kernel/TraceAlgorithms.cu:22-31): the aggregate's (a, b) — FLT_MAX / -FLT_MAX on a miss — go into tau, which intersects again
template <bool GRID = false> HD f3 transmittance(const table& T, f3 o, f3 d, float tmin, float tmax) {
    if (T.n > 0) {
        float a, b; intersect(T, o, d, tmin, tmax, a, b);
        return sexp(-tau<GRID>(T, o, d, a, b));
    }
    return f3(1.0f);
}
// KernelDynamicScene::evalTransmittance (Engine/KernelDynamicScene.cu:90-96)
template <bool GRID = false> HD f3 eval_transmittance(const table& T, f3 p1, f3 p2) {
    f3 d = p2 - p1;
    const float l = length(d);
    d = d / l;
    return sexp(-tau<GRID>(T, p1, d, 0.0f, l));
}

// ---- host: the table of a description.  `where` = the array the kernels read (device memory, or the host array itself for the host yardstick)
inline table make_table(const ctl_volume* where, uint32_t n, const grid_rec* g = nullptr, const float* cells = nullptr) { table T{}; T.v = where; T.n = n; T.g = g; T.cells = cells; return T; }
// ---- host: the grid records of a (validated) description, one slot per region, and their floats in one buffer
struct grid_pack {
    std::vector<grid_rec> recs; std::vector<float> cells; bool any = false;
    bool same(const grid_pack& o) const {
        return any == o.any && cells.size() == o.cells.size() && (recs.empty() || std::memcmp(recs.data(), o.recs.data(), recs.size() * sizeof(grid_rec)) == 0) &&
               (cells.empty() || std::memcmp(cells.data(), o.cells.data(), cells.size() * 4) == 0);
    }
};
inline void pack_grids(const ctl_scene_desc& d, grid_pack& P) {
    P.recs.assign(CTL_MAX_VOL_COUNT, grid_rec{}); P.cells.clear(); P.any = d.n_volume_grids != 0;
    auto put = [&](const float* data, const uint32_t* dim) { const uint32_t off = (uint32_t)P.cells.size(); P.cells.insert(P.cells.end(), data, data + (size_t)dim[0] * dim[1] * dim[2]); return off; };
    for (uint32_t k = 0; k < d.n_volume_grids; k++) {
        const ctl_volume_grid& G = d.volume_grids[k]; grid_rec& R = P.recs[G.volume];
        R.single = G.single_grid ? 1u : 0u;
        for (int c = 0; c < 3; c++) { R.sa_min[c] = G.sig_a_min[c]; R.sa_max[c] = G.sig_a_max[c]; R.ss_min[c] = G.sig_s_min[c]; R.ss_max[c] = G.sig_s_max[c]; }
        if (R.single) { for (int c = 0; c < 3; c++) R.dim[c] = G.dim[c]; R.off = put(G.data, G.dim); }
        else { for (int c = 0; c < 3; c++) { R.dim_a[c] = G.dim_a[c]; R.dim_s[c] = G.dim_s[c]; } R.off_a = put(G.data_a, G.dim_a); R.off_s = put(G.data_s, G.dim_s); }
    }
}
// ---- host: the derived fields
// KajiyaKayPhaseFunction::Update (PhaseFunction.cu:64-77), with the shared fp32 functions
inline float kajiya_kay_normalization(float exponent) {
    const int nParts = 1000;
    float stepSize = kPi / nParts, m = 4, theta = stepSize;
    float normalization = 0;
    for (int i = 1; i < nParts; ++i) {
        const float value = fm::pow(fm::cos(theta - kPi / 2), exponent) * fm::sin(theta);
        normalization += value * m;
        theta += stepSize;
        m = 6 - m;
    }
    return 1 / (normalization * stepSize / 3 * 2 * kPi);
}

}  // namespace vol
}  // namespace ctl
