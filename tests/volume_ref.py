"""The independent yardstick of the participating media (not collected by pytest): a numpy float32 restatement of the reference's homogeneous volumes, their aggregate
and the four phase functions, written from the reference's source (SceneTypes/Volumes.{h,cu}, SceneTypes/PhaseFunction.{h,cu}, Math/AABB.h, Math/MathFunc.h,
Kernel/TraceAlgorithms.cu:22-31, Engine/KernelDynamicScene.cu:90-123) — not from csrc/volume.h — one fp32 operation per numpy operation, in the source's order.
exp / log / sin / cos / pow come from the shared-math oracle (orc_math_eval), sqrt and the four operations are numpy's (correctly rounded), so a result can match the
library's to the bit.

Volumes(orc, list of ctl_volume) offers every function ctl_volume_eval offers; eval_rows(V, what, queries) lays the results out as ctl_volume_eval does.
path_trace(orc, desc, w, h, tables, ...) is pathKernel2 + PathTrace<DIRECT> (Integrators/PathTracer.cu:10-113, 182-194) with media, per pixel.  The loop, the medium vertex
and the roulette are restated here from the oracle's exports (sampler draws, sensor rays, traversal of the product's flattened tree, emitter sampling); the surface
vertex and the escaped path's environment term are the oracle's own pathVertex / pathEscape (oracle/ocore.h: the two functions its pathTrace is made of, exported as
orc_path_vertex / orc_path_escape), with this file's Transmittance hooked into EstimateDirect — so any scene the oracle renders can carry media here, with first-hit
partials where asked.  tests/test_media_fuzz_host.py pins the join: without volumes path_trace is the oracle's render, bit for bit.
Three things are the product's, not the reference's, and are stated where they stand: a path ends when its throughput is exactly zero (every kernel of the library makes
that cut), and a medium record or a last_nor nothing has written yet reads as zeros (the reference reads uninitialised memory).
With the glibc oracle (oracle.Oracle()) instead of the shared-math one, and path_trace's reference_rules, this file is held to the reference's OWN Volumes.cu,
PhaseFunction.cu and PathTrace bit for bit (tests/test_oracle_volume.py over tests/golden/volumes.npz and pathtrace_media.npz); path_trace counts, per pixel, the places
where the reference reads what nothing wrote, so that no such case is ever recorded from it.
"""
import ctypes as C
import struct

import numpy as np

f32 = np.float32
FLT_MAX = f32(3.402823466e+38)
PI = f32(3.14159265358979)
PHASE_HG, PHASE_ISOTROPIC, PHASE_KAJIYA_KAY, PHASE_RAYLEIGH = 1, 2, 3, 4
E_DELTA = 0x1 | 0x20 | 0x40
E_SMOOTH = 0x2 | 0x4 | 0x8 | 0x10
E_ALL = 0x1ff
CTL_LIGHT_POINT, CTL_LIGHT_DIFFUSE, CTL_LIGHT_DISTANT, CTL_LIGHT_SPOT, CTL_LIGHT_INFINITE = 1, 2, 3, 4, 5

_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def v3(x, y=None, z=None):
    return np.array([x, x, x] if y is None else [x, y, z], np.float32)


def _bits(x):
    return struct.unpack("<i", struct.pack("<f", float(x)))[0]


def _from_bits(i):
    return f32(struct.unpack("<f", struct.pack("<i", i))[0])


def dot(a, b):   # VectorBase::dot (Math/Vector.h:97): r = 0; r += a[i] * b[i]
    r = f32(0)
    for i in range(len(a)):
        r = f32(r + f32(f32(a[i]) * f32(b[i])))
    return r


def length(a):
    r = f32(0)
    for i in range(3):
        r = f32(r + f32(f32(a[i]) * f32(a[i])))
    return f32(np.sqrt(r))


def fmin(a, b):   # CudaTracerLib::min: (a < b) ? a : b
    return a if a < b else b


def fmax(a, b):
    return a if a > b else b


class Math:
    """the transcendental functions the library's device code runs, through the shared-math oracle"""

    def __init__(self, orc):
        self.lib = orc.lib
        self.lib.orc_math_eval.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        self.x = np.zeros(1, np.float32); self.y = np.zeros(1, np.float32); self.o = np.zeros(1, np.float32)

    def _f(self, which, x, y=0.0):
        self.x[0] = x; self.y[0] = y
        self.lib.orc_math_eval(which, 1, self.x.ctypes.data, self.y.ctypes.data, self.o.ctypes.data)
        return f32(self.o[0])

    def sin(self, x): return self._f(0, x)
    def cos(self, x): return self._f(1, x)
    def exp(self, x): return self._f(6, x)
    def log(self, x): return self._f(7, x)
    def pow(self, x, y): return self._f(9, x, y)

    def exp3(self, s):
        return np.array([self.exp(s[0]), self.exp(s[1]), self.exp(s[2])], np.float32)


def transform_point(m, p):   # float4x4::TransformPoint (float4x4.h:398-402): (M * (p, 1)).xyz / w
    q = (p[0], p[1], p[2], f32(1))
    f = [dot(m[i], q) for i in range(4)]
    return np.array([f32(f[0] / f[3]), f32(f[1] / f[3]), f32(f[2] / f[3])], np.float32)


def transform_direction(m, d):
    q = (d[0], d[1], d[2], f32(0))
    return np.array([dot(m[i], q) for i in range(3)], np.float32)


def _imin(a, b): return a if a < b else b
def _imax(a, b): return a if a > b else b


def span_begin(a0, a1, b0, b1, c0, c1, d):
    """kepler_math::spanBeginKepler (MathFunc.h:405-444): fmax_fmax(min(a0, a1), min(b0, b1), fmin_fmax(c0, c1, d)); the three-operand forms compare the floats'
    bit patterns as signed integers"""
    c = _imax(_imin(_bits(c0), _bits(c1)), _bits(d))
    return _from_bits(_imax(_imax(_bits(fmin(a0, a1)), _bits(fmin(b0, b1))), c))


def span_end(a0, a1, b0, b1, c0, c1, d):
    c = _imin(_imax(_bits(c0), _bits(c1)), _bits(d))
    return _from_bits(_imin(_imin(_bits(fmax(a0, a1)), _bits(fmax(b0, b1))), c))


def aabb_intersect(lo, hi, o, d, mn, mx):
    """AABB::Intersect<true>(Ray, &min, &max) (AABB.h:142-158) -> (hit, min, max); the bounds change on a hit only"""
    tx1 = f32(f32(lo[0] - o[0]) / d[0]); tx2 = f32(f32(hi[0] - o[0]) / d[0])
    ty1 = f32(f32(lo[1] - o[1]) / d[1]); ty2 = f32(f32(hi[1] - o[1]) / d[1])
    tz1 = f32(f32(lo[2] - o[2]) / d[2]); tz2 = f32(f32(hi[2] - o[2]) / d[2])
    mi = span_begin(tx1, tx2, ty1, ty2, tz1, tz2, mn)
    ma = span_end(tx1, tx2, ty1, ty2, tz1, tz2, mx)
    b = bool(ma > mi and ma > 0)
    return (True, mi, ma) if b else (False, mn, mx)


def coordinate_system(a):   # Frame.h:9-22 -> (s, t)
    if abs(a[0]) > abs(a[1]):
        il = f32(f32(1) / f32(np.sqrt(f32(f32(a[0] * a[0]) + f32(a[2] * a[2])))))
        t = np.array([f32(a[2] * il), f32(0), f32(f32(-a[0]) * il)], np.float32)
    else:
        il = f32(f32(1) / f32(np.sqrt(f32(f32(a[1] * a[1]) + f32(a[2] * a[2])))))
        t = np.array([f32(0), f32(a[2] * il), f32(f32(-a[1]) * il)], np.float32)
    c = np.array([f32(f32(t[1] * a[2]) - f32(t[2] * a[1])), f32(f32(t[2] * a[0]) - f32(t[0] * a[2])), f32(f32(t[0] * a[1]) - f32(t[1] * a[0]))], np.float32)
    s = (c * f32(f32(1) / length(c))).astype(np.float32)   # normalized(): v * rcp(length)
    return s, t


def frame_to_world(s, t, n, v):   # Frame::toWorld: s * v.x + t * v.y + n * v.z
    return ((s * v[0]).astype(np.float32) + (t * v[1]).astype(np.float32) + (n * v[2]).astype(np.float32)).astype(np.float32)


def _sum3(s):   # TSpectrum::sum: from 0
    r = f32(0)
    for i in range(3):
        r = f32(r + s[i])
    return r


def _avg(s):
    return f32(_sum3(s) * f32(f32(1.0) / f32(3)))


def _max3(s):
    r = s[0]
    r = fmax(r, s[1]); r = fmax(r, s[2])
    return r


def zero_rec():
    return dict(t=f32(0), p=v3(0), transmittance=v3(0), sigmaA=v3(0), sigmaS=v3(0), pdfSuccess=f32(0), pdfSuccessRev=f32(0), pdfFailure=f32(0), written=False)


class Volumes:
    """KernelAggregateVolume over a list of ctl_volume (their derived fields current)"""

    def __init__(self, orc, volumes):
        self.m = Math(orc)
        self.v = []
        for V in volumes:
            self.v.append(dict(v2w=np.array(list(V.volume_to_world.m), np.float32).reshape(4, 4), w2v=np.array(list(V.world_to_volume.m), np.float32).reshape(4, 4),
                               sig_a=np.array(list(V.sig_a), np.float32), sig_s=np.array(list(V.sig_s), np.float32), type=int(V.phase.type), g=f32(V.phase.g),
                               ks=f32(V.phase.ks), kd=f32(V.phase.kd), exponent=f32(V.phase.exponent), normalization=f32(V.phase.normalization)))
        self.n = len(self.v)
        self.past_table = 0   # (bookkeeping) how often sample_volume formed an index >= n, where the reference reads past its table
        for V in self.v:
            V["bound"] = self.world_bound(V)   # a function of the region alone: made once

    # ---- regions
    def world_bound(self, V):   # AABB(0, 1).Transform(VolumeToWorld) (AABB.h:32-45)
        m = V["v2w"]
        right = transform_direction(m, v3(1, 0, 0)); up = transform_direction(m, v3(0, 1, 0)); fwd = transform_direction(m, v3(0, 0, 1))
        with np.errstate(**_ERR):
            xa, xb = (right * f32(0)).astype(np.float32), (right * f32(1)).astype(np.float32)
            ya, yb = (up * f32(0)).astype(np.float32), (up * f32(1)).astype(np.float32)
            za, zb = (fwd * f32(0)).astype(np.float32), (fwd * f32(1)).astype(np.float32)
            tr = transform_point(m, v3(0))
            vmin = lambda a, b: np.array([fmin(a[i], b[i]) for i in range(3)], np.float32)
            vmax = lambda a, b: np.array([fmax(a[i], b[i]) for i in range(3)], np.float32)
            lo = (((vmin(xa, xb) + vmin(ya, yb)).astype(np.float32) + vmin(za, zb)).astype(np.float32) + tr).astype(np.float32)
            hi = (((vmax(xa, xb) + vmax(ya, yb)).astype(np.float32) + vmax(za, zb)).astype(np.float32) + tr).astype(np.float32)
        return lo, hi

    def inside_world(self, V, p):
        with np.errstate(**_ERR):
            pl = transform_point(V["w2v"], p)
        return bool(pl[0] >= 0 and pl[1] >= 0 and pl[2] >= 0 and pl[0] <= 1 and pl[1] <= 1 and pl[2] <= 1)

    def region_intersect(self, V, o, d, minT, maxT):
        """BaseVolumeRegion::IntersectP -> (hit, t0, t1); t0 / t1 None on a miss (the reference leaves them unwritten)"""
        with np.errstate(**_ERR):
            ol = transform_point(V["w2v"], o); dl = transform_direction(V["w2v"], d)
            b, mn, mx = aabb_intersect(v3(0), v3(1), ol, dl, f32(minT), f32(maxT))
        return (True, mn, mx) if b else (False, None, None)

    def region_tau(self, V, o, d, minT, maxT):
        b, t0, t1 = self.region_intersect(V, o, d, minT, maxT)
        if not b:
            return v3(0)
        with np.errstate(**_ERR):
            p0 = (o + (t0 * d).astype(np.float32)).astype(np.float32); p1 = (o + (t1 * d).astype(np.float32)).astype(np.float32)
            return (length((p0 - p1).astype(np.float32)) * (V["sig_a"] + V["sig_s"]).astype(np.float32)).astype(np.float32)

    def region_sample_distance(self, V, o, d, minT, maxT, rand, mRec):
        """HomogeneousVolumeDensity::sampleDistance (Volumes.cu:28-74), as written"""
        m = self.m
        minT, maxT, rand = f32(minT), f32(maxT), f32(rand)
        with np.errstate(**_ERR):
            weight = f32(-1)
            sig_a, sig_s = V["sig_a"], V["sig_s"]
            sig_t = (sig_a + sig_s).astype(np.float32); albedo = (sig_s / sig_t).astype(np.float32)
            for i in range(3):
                if albedo[i] > weight and sig_t[i] != 0:
                    weight = albedo[i]
            if weight > 0:
                weight = fmax(weight, f32(0.5))
            sampled = FLT_MAX
            if rand < weight:
                rand = f32(rand / weight)
                channel = int(f32(rand * f32(3)))   # MonteCarlo::sampleReuse(N, pdf, slot)
                rand = f32(f32(rand * f32(3)) - f32(channel))
                density = sig_t[channel]
                sampled = f32(f32(-m.log(f32(f32(1) - rand))) / density)
            success = True
            if sampled < f32(maxT - minT):
                mRec["t"] = f32(minT + sampled)
                mRec["p"] = (o + (mRec["t"] * d).astype(np.float32)).astype(np.float32)
                mRec["sigmaA"] = sig_a.copy(); mRec["sigmaS"] = sig_s.copy()
                if (mRec["p"] == o).all():
                    success = False
            else:
                sampled = f32(maxT - minT)
                success = False
            tmp = m.exp3(((-sig_t).astype(np.float32) * sampled).astype(np.float32))
            pdfFailure = _avg(tmp)
            pdfSuccess = _avg((sig_t * tmp).astype(np.float32))
            mRec["transmittance"] = m.exp3((sig_t * f32(-sampled)).astype(np.float32))
            mRec["written"] = True   # (bookkeeping: the record's probabilities and transmittance hold values of some sampleDistance from here on)
            mRec["pdfSuccess"] = mRec["pdfSuccessRev"] = f32(pdfSuccess * weight)
            mRec["pdfFailure"] = f32(f32(weight * pdfFailure) + f32(f32(1) - weight))
            if _max3(mRec["transmittance"]) < f32(1e-8):
                mRec["transmittance"] = v3(0)
        return success

    # ---- the aggregate
    def intersect(self, o, d, minT, maxT):
        t0, t1 = FLT_MAX, f32(-FLT_MAX)
        for V in self.v:
            b, a, c = self.region_intersect(V, o, d, minT, maxT)
            if b:
                t0 = fmin(t0, a); t1 = fmax(t1, c)
        return bool(t0 < t1), t0, t1

    def tau(self, o, d, minT, maxT):
        s = v3(0)
        for V in self.v:
            s = (s + self.region_tau(V, o, d, minT, maxT)).astype(np.float32)
        return s

    @staticmethod
    def ffsn(v, n):   # Volumes.cu:303-308: returns a bit MASK
        for _ in range(n - 1):
            v &= v - 1
        return v & ~(v - 1)

    def sample_volume(self, o, d, minT, maxT, sample):
        """KernelAggregateVolume::sampleVolume -> (index or -1, sample, pdf).  As written: with several regions the 0-based slot of sampleReuse goes into the 1-based
        ffsn, and ffsn's mask is used as the index; an index past the table is 'none' here (the reference reads past its array)"""
        i, sample, pdf, _ = self.sample_volume_raw(o, d, minT, maxT, sample)
        if i >= self.n:
            self.past_table += 1
        return (i if 0 <= i < self.n else -1), sample, pdf

    def sample_volume_raw(self, o, d, minT, maxT, sample):
        """sampleVolume before the table's bound is applied -> (the index the reference forms, or -1 where it returns no region; sample; pdf; the mask of the regions
        whose WorldBound() the segment meets, 0 with fewer than two regions).  An index >= n is where the reference reads past m_pVolumes: the fixtures of
        tests/golden never send such a row to it (tests/golden/generate.py)"""
        sample = f32(sample); pdf = f32(0)
        if self.n == 0:
            return -1, sample, pdf, 0
        with np.errstate(**_ERR):
            if self.n == 1:
                lo, hi = self.v[0]["bound"]
                return (0 if aabb_intersect(lo, hi, o, d, f32(minT), f32(maxT))[0] else -1), sample, pdf, 0
            n = 0; flag = 0
            for i, V in enumerate(self.v):
                lo, hi = V["bound"]
                if aabb_intersect(lo, hi, o, d, f32(minT), f32(maxT))[0]:
                    n += 1; flag |= 1 << i
            if not n:
                return -1, sample, pdf, 0
            nth = int(f32(sample * f32(n)))
            sample = f32(f32(sample * f32(n)) - f32(nth))
            i = self.ffsn(flag, nth)
            pdf = f32(f32(1.0) / f32(n))
        return i, sample, pdf, flag

    def sample_distance(self, o, d, minT, maxT, sample, mRec):
        vi, sample, _ = self.sample_volume(o, d, minT, maxT, sample)
        return vi >= 0 and self.region_sample_distance(self.v[vi], o, d, minT, maxT, sample, mRec)

    # ---- phase functions
    def uniform_sphere(self, s):   # Warp::squareToUniformSphere
        z = f32(f32(1) - f32(f32(2) * s[1])); r = f32(np.sqrt(f32(f32(1) - f32(z * z))))
        phi = f32(f32(f32(2) * PI) * s[0])
        return np.array([f32(r * self.m.cos(phi)), f32(r * self.m.sin(phi)), z], np.float32)

    def phase_eval(self, F, wi, wo):
        m = self.m
        INV_FOURPI = f32(f32(1) / f32(f32(4) * PI))
        with np.errstate(**_ERR):
            if F["type"] == PHASE_HG:
                g = F["g"]
                temp = f32(f32(f32(1) + f32(g * g)) + f32(f32(f32(2) * g) * dot(wi, wo)))
                return f32(f32(INV_FOURPI * f32(f32(1) - f32(g * g))) / f32(temp * f32(np.sqrt(temp))))
            if F["type"] == PHASE_KAJIYA_KAY:
                kd4 = f32(F["kd"] / f32(f32(4) * PI))
                if _max3(wi) == 0:
                    return kd4
                s, t = coordinate_system(wi)
                rl = np.array([dot(wo, s), dot(wo, t), dot(wo, wi)], np.float32)
                rl[2] = f32(-dot(wi, wi))
                a = f32(np.sqrt(f32(f32(f32(1) - f32(rl[2] * rl[2])) / f32(f32(rl[0] * rl[0]) + f32(rl[1] * rl[1])))))
                rl[1] = f32(rl[1] * a); rl[0] = f32(rl[0] * a)
                R = frame_to_world(s, t, wi, rl)
                return f32(f32(f32(m.pow(fmax(f32(0), dot(R, wo)), F["exponent"]) * F["normalization"]) * F["ks"]) + kd4)
            if F["type"] == PHASE_RAYLEIGH:
                mu = dot(wi, wo)
                return f32(f32(f32(3) / f32(f32(16) * PI)) * f32(f32(1) + f32(mu * mu)))
            return INV_FOURPI

    def phase_sample(self, F, wi, sample):
        """PhaseFunction::Sample(pRec, pdf, sample) -> (weight, pdf, wo)"""
        m = self.m
        FOURPI = f32(f32(4) * PI)
        with np.errstate(**_ERR):
            if F["type"] == PHASE_HG:
                g = F["g"]
                if abs(g) < f32(0.000001):
                    cosT = f32(f32(1) - f32(f32(2) * sample[0]))
                else:
                    sq = f32(f32(f32(1) - f32(g * g)) / f32(f32(f32(1) - g) + f32(f32(f32(2) * g) * sample[0])))
                    cosT = f32(f32(f32(f32(1) + f32(g * g)) - f32(sq * sq)) / f32(f32(2) * g))
                sinT = f32(np.sqrt(f32(f32(1) - f32(cosT * cosT))))
                phi = f32(f32(f32(2) * PI) * sample[1])
                sinP, cosP = m.sin(phi), m.cos(phi)
                nw = (-wi).astype(np.float32); s, t = coordinate_system(nw)
                wo = frame_to_world(s, t, nw, np.array([f32(sinT * cosP), f32(sinT * sinP), cosT], np.float32))
                return f32(1), self.phase_eval(F, wi, wo), wo
            if F["type"] == PHASE_KAJIYA_KAY:
                wo = self.uniform_sphere(sample)
                return f32(self.phase_eval(F, wi, wo) * FOURPI), f32(f32(1) / FOURPI), wo
            if F["type"] == PHASE_RAYLEIGH:
                z = f32(f32(2) * f32(f32(f32(2) * sample[0]) - f32(1)))
                tmp = f32(np.sqrt(f32(f32(z * z) + f32(1))))
                third = f32(f32(1.0) / f32(3.0))
                A = m.pow(f32(z + tmp), third); B = m.pow(f32(z - tmp), third)   # the second base is negative: NaN, kept
                cosT = f32(A + B); sinT = f32(np.sqrt(f32(f32(1) - f32(cosT * cosT))))
                phi = f32(f32(f32(2) * PI) * sample[1])
                sinP, cosP = m.sin(phi), m.cos(phi)
                nw = (-wi).astype(np.float32); s, t = coordinate_system(nw)
                wo = frame_to_world(s, t, nw, np.array([f32(sinT * cosP), f32(sinT * sinP), cosT], np.float32))
                return f32(1), self.phase_eval(F, wi, wo), wo
            wo = self.uniform_sphere(sample)
            return f32(1), f32(f32(1) / FOURPI), wo

    def p(self, p, wi, wo):   # KernelAggregateVolume::p
        ph = f32(0); sumWt = f32(0)
        with np.errstate(**_ERR):
            for V in self.v:
                lo, hi = V["bound"]
                if all(lo[i] <= p[i] <= hi[i] for i in range(3)):
                    wt = _avg(V["sig_s"] if self.inside_world(V, p) else v3(0))
                    sumWt = f32(sumWt + wt)
                    ph = f32(ph + f32(wt * self.phase_eval(V, wi, wo)))
            return f32(ph / sumWt) if sumWt != 0 else f32(0)

    def sample(self, p, wi, sample):
        """KernelAggregateVolume::Sample -> (weight, pdf, wo); no region: (0, 0, 0-vector)"""
        s = np.array(sample, np.float32)
        vi, s[0], _ = self.sample_volume(p, wi, f32(0), FLT_MAX, s[0])
        if vi < 0:
            return f32(0), f32(0), v3(0)
        return self.phase_sample(self.v[vi], wi, s)

    def transmittance(self, o, d, tmin, tmax):   # TraceAlgorithms.cu:22-31
        if self.n == 0:
            return v3(1)
        _, a, b = self.intersect(o, d, tmin, tmax)
        with np.errstate(**_ERR):
            return self.m.exp3((-self.tau(o, d, a, b)).astype(np.float32))

    def eval_transmittance(self, p1, p2):   # KernelDynamicScene.cu:90-96
        with np.errstate(**_ERR):
            d = (p2 - p1).astype(np.float32)
            l = length(d)
            d = (d / l).astype(np.float32)
            return self.m.exp3((-self.tau(p1, d, f32(0), l)).astype(np.float32))


def kajiya_kay_normalization(m, exponent):
    """KajiyaKayPhaseFunction::Update (PhaseFunction.cu:78-93): the 999-term Simpson sum in fp32; m: a Math"""
    step = f32(PI / f32(1000)); mm = f32(4); theta = step; acc = f32(0)
    for _ in range(1, 1000):
        value = f32(m.pow(m.cos(f32(theta - f32(PI / f32(2)))), f32(exponent)) * m.sin(theta))
        acc = f32(acc + f32(value * mm)); theta = f32(theta + step); mm = f32(f32(6) - mm)
    return f32(f32(1) / f32(f32(f32(f32(acc * step) / f32(3)) * f32(2)) * PI))


def _word(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def eval_rows(V, what, queries):
    """the rows ctl_volume_eval returns (include/ctl_amd.h CTL_VEVAL_*) from the restatement: (n, 17) float32"""
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 10)
    out = np.zeros((len(q), 17), np.float32)

    def put_rec(o, ok, r):
        o[0] = 1 if ok else 0; o[1] = r["t"]; o[2:5] = r["p"]; o[5:8] = r["transmittance"]; o[8:11] = r["sigmaA"]; o[11:14] = r["sigmaS"]
        o[14] = r["pdfSuccess"]; o[15] = r["pdfSuccessRev"]; o[16] = r["pdfFailure"]
    for a, o in zip(q, out):
        if what == 0:
            b, t0, t1 = V.region_intersect(V.v[_word(a[0])], a[1:4], a[4:7], a[7], a[8]); o[0] = b; o[1] = t0 if b else 0; o[2] = t1 if b else 0
        elif what == 1:
            b, t0, t1 = V.intersect(a[0:3], a[3:6], a[6], a[7]); o[0] = b; o[1] = t0; o[2] = t1
        elif what == 2:
            o[0:3] = V.region_tau(V.v[_word(a[0])], a[1:4], a[4:7], a[7], a[8])
        elif what == 3:
            o[0:3] = V.tau(a[0:3], a[3:6], a[6], a[7])
        elif what == 4:
            r = zero_rec(); put_rec(o, V.region_sample_distance(V.v[_word(a[0])], a[1:4], a[4:7], a[7], a[8], a[9], r), r)
        elif what == 5:
            r = zero_rec(); put_rec(o, V.sample_distance(a[0:3], a[3:6], a[6], a[7], a[8], r), r)
        elif what == 6:
            o[0], o[1], o[2] = V.sample_volume(a[0:3], a[3:6], a[6], a[7], a[8])
        elif what == 7:
            o[0] = V.phase_eval(V.v[_word(a[0])], a[1:4], a[4:7])
        elif what == 8:
            w, pdf, wo = V.phase_sample(V.v[_word(a[0])], a[1:4], a[4:6]); o[0] = w; o[1] = pdf; o[2:5] = wo
        elif what == 9:
            o[0] = V.p(a[0:3], a[3:6], a[6:9])
        elif what == 10:
            w, pdf, wo = V.sample(a[0:3], a[3:6], a[6:8]); o[0] = w; o[1] = pdf; o[2:5] = wo
        elif what == 11:
            o[0:3] = V.transmittance(a[0:3], a[3:6], a[6], a[7])
        elif what == 12:
            o[0:3] = V.eval_transmittance(a[0:3], a[3:6])
        else:
            raise ValueError(what)
    return out


# ------------------------------------------------------------------------------------------------------------------ pathKernel2 + PathTrace<DIRECT>
def _bind(lib):
    lib.orc_sampler_float.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]; lib.orc_sampler_float.restype = C.c_float
    lib.orc_sampler_float2.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.orc_sensor_sample_ray_differential.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.orc_triangle_fill_dg.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_void_p]
    lib.orc_bsdf_sample_uv.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
    lib.orc_bsdf_eval_uv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_void_p]
    lib.orc_sample_emitter_direct.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    lib.orc_light_sample_direct.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    lib.orc_emitter_select.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.orc_light_pdf_direct.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]; lib.orc_light_pdf_direct.restype = C.c_float
    lib.orc_light_eval.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.orc_env_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.orc_sensor_sample_rays.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    lib.orc_path_state_size.restype = C.c_uint32; lib.orc_path_state_size.argtypes = []
    lib.orc_path_state_init.argtypes = [C.c_void_p]; lib.orc_path_state_init.restype = None
    lib.orc_path_ctx_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p]; lib.orc_path_ctx_create.restype = C.c_void_p
    lib.orc_path_ctx_destroy.argtypes = [C.c_void_p]; lib.orc_path_ctx_destroy.restype = None
    lib.orc_path_vertex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, TRANSMITTANCE_HOOK, C.c_void_p, C.c_void_p]
    lib.orc_path_vertex.restype = None
    lib.orc_path_escape.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float]; lib.orc_path_escape.restype = None


# EstimateDirect's attenuation as the oracle's vertex calls it (oracle/ocore.h TransmittanceHook): (p, d, tmin, tmax, out, user)
TRANSMITTANCE_HOOK = C.CFUNCTYPE(None, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float, C.c_float, C.POINTER(C.c_float), C.c_void_p)


def _power_heuristic(f, g):   # MonteCarlo::PowerHeuristic(1, f, 1, g)
    with np.errstate(**_ERR):
        f = f32(f32(1) * f); g = f32(f32(1) * g)
        return f32(f32(f * f) / f32(f32(f * f) + f32(g * g)))


def _sdiv(s, x):   # Spectrum / scalar multiplies by the reciprocal (Spectrum.h:122-128)
    with np.errstate(**_ERR):
        return (s * f32(f32(1) / x)).astype(np.float32)


def _mul(a, b):
    with np.errstate(**_ERR):
        return (a * b).astype(np.float32)


def _add(a, b):
    with np.errstate(**_ERR):
        return (a + b).astype(np.float32)


class _Path:
    """one path_trace call's scene: the media (Python), the closest-hit and occlusion rays of the loop and of the medium vertex, and the oracle's own surface vertex and
    escape term (oracle_capi.cpp orc_path_vertex / orc_path_escape — the two functions the oracle's pathTrace is made of) behind one state buffer"""
    handle = None

    def __init__(self, orc, desc, volumes, flat, half_host_quirk=False, partials=False):
        self.orc, self.lib, self.desc, self.flat = orc, orc.lib, desc, flat
        _bind(self.lib)
        self.V = Volumes(orc, volumes)
        self.eps = f32(desc.ray_trace_eps)
        self.rays = 0
        self.half_host_quirk = half_host_quirk
        self.unwritten_reads = 0; self.unwritten_normal_reads = 0; self.unset_directions = 0; self.zero_walks = 0; self.zero_rays = 0; self.zero_now = False
        # orc_render's bits: 1 half::ToFloat's host branch, 2 the alpha test (as trace() below), 4 first-hit ray differentials
        self.handle = self.lib.orc_path_ctx_create(C.addressof(desc), (1 if half_host_quirk else 0) | 2 | (4 if partials else 0), C.addressof(flat) if flat is not None else None)
        self.buf = C.create_string_buffer(int(self.lib.orc_path_state_size()))
        # the named fields of orc_path_state: cl, cf, ro, rd, brdf_scattering_pdf, last_nor | specular_bounce, d1, d2, light_index, mis_taken
        self.sf = np.frombuffer(self.buf, np.float32, 16); self.si = np.frombuffer(self.buf, np.int32, 5, offset=64)
        self.hits = None; self.shadow = C.c_uint64(0); self.hook_error = None
        self.hook = TRANSMITTANCE_HOOK(self._transmittance) if self.V.n else C.cast(None, TRANSMITTANCE_HOOK)   # a null hook: the oracle's own EstimateDirect

    def close(self):
        if self.handle:
            self.lib.orc_path_ctx_destroy(self.handle); self.handle = None

    __del__ = close   # (a path_trace call that raises)

    def _transmittance(self, p, d, tmin, tmax, out, user):   # Transmittance(Ray(dRec.ref, dRec.d), 0, dRec.dist) for EstimateDirect(attenuated = true)
        try:
            T = self.V.transmittance(np.array([p[0], p[1], p[2]], np.float32), np.array([d[0], d[1], d[2]], np.float32), f32(tmin), f32(tmax))
            out[0], out[1], out[2] = float(T[0]), float(T[1]), float(T[2])
        except BaseException as e:   # (an exception cannot cross the C frames: it is raised again when the vertex call returns)
            self.hook_error = e

    def trace(self, o, d, tmax=FLT_MAX, any_hit=False):
        r = np.zeros((1, 8), np.float32); r[0, :3] = o; r[0, 3] = self.eps; r[0, 4:7] = d; r[0, 7] = tmax
        self.rays += 1
        if self.zero_now:
            self.zero_rays += 1
        self.hits = self.orc.intersect(self.desc, r, any_hit=any_hit, alpha_test=True, threads=1, flat=self.flat, half_host_quirk=self.half_host_quirk)
        return self.hits[0]

    def vertex(self, t1, t2, idx, depth, direct, diff):
        """PathTrace's surface vertex at the hit trace() returned last, on the state buffer; the shadow rays it traced are counted like trace()'s"""
        self.shadow.value = 0
        self.lib.orc_path_vertex(self.handle, t1.ctypes.data, t2.ctypes.data, idx, self.buf, self.hits.ctypes.data, depth, 1 if direct else 0,
                                 diff.ctypes.data if diff is not None else None, self.hook, None, C.byref(self.shadow))
        if self.hook_error is not None:
            e, self.hook_error = self.hook_error, None
            raise e
        self.rays += self.shadow.value
        if self.zero_now:
            self.zero_rays += self.shadow.value


def path_trace(orc, desc, volumes, w, h, tables, direct=True, max_path_length=6, rr_start=5, flat=None, debug_pixels=None, ray_count=None, reference_rules=False,
               undefined=None, pixel_rays=None, partials=False, walk_on_zero=None, vertex_counts=None):
    """pathKernel2<DIRECT> over every pixel and every pass of `tables` -> pixel data (h, w, 7): rgb, splat (0), weightSum, as Image::AddSample accumulates them.
    The loop, the medium vertex and the roulette are restated here; the surface vertex (getBsdfSample, first-hit partials, emission MIS, BSDF sample, UniformSampleOneLight
    with the transmittance of this file's media hooked into EstimateDirect) and the escaped path's environment term are the oracle's own pathVertex / pathEscape, the
    functions its pathTrace is made of — every BSDF model, texture, surface map and emitter the oracle has.
    volumes: the list of ctl_volume of the scene (empty: no media — then this is the oracle's render).  flat: the product's flattened tree (FlatBvh(...).desc), so that a
    ray grazing a shared edge resolves as on the device.  debug_pixels = [(x, y), ...]: instead PathTracer::DebugInternal for those pixels — Direct on, no jitter, the first
    table set — returning their radiances (n, 3).  ray_count: a list that receives the number of rays traced.
    partials: as Oracle.render(partials=True) — the sensor's ray differentials, the image pyramids, filtered lookups at the first hit (what the PathTracer plugin and its
    Debug do).
    reference_rules: the two places where this restatement follows the product and not the reference as compiled for the host are switched to the reference's: a path
    whose throughput is exactly zero walks on (PathTrace has no such cut; walk_on_zero switches this one alone), and fillDG decodes the triangles' normals with the host
    branch of half::ToFloat (half_host_quirk, as tests/test_oracle_pathtrace.py).
    vertex_counts: an int array (h, w, 3), added to — per pixel the medium vertices, the surface vertices, and the paths whose escape term was evaluated, with an
    environment map in the scene, for a ray that left a MEDIUM vertex.
    undefined: an int32 array (h, w, 6), added to — per pixel the places where the reference's PathTrace reads
    what nothing has written (media): [..., 0] reads of a medium record that no sampleDistance had written; [..., 1] sampleVolume indices past the table;
    [..., 2] emission MIS weights taken with a last_nor no surface had set (the path's only vertices so far were medium vertices); [..., 3] medium vertices at which
    Sample found no region, so that the reference walks on — with a throughput of exactly zero — along a pRec.wo nothing has set; [..., 4] samples whose throughput
    became exactly zero anywhere (after a failed BSDF sample the reference walks on along the record's previous wo); [..., 5] the rays traced after that point.
    Channels 0 to 2 can change the radiance; 3 to 5 only the number of rays (whatever such a path meets is multiplied by zero) — unless the scene has an environment
    map: a ray along the unset direction of channel 3 that escapes makes 0 * EvalEnvironment(garbage) = NaN in the reference, which drops the sample
    (tests/golden/generate.py MEDIA_PAIR_LEFT_OUT).
    pixel_rays: a uint32 array (h, w), added to: the rays each pixel traced."""
    lib = orc.lib
    ctx = _Path(orc, desc, volumes, flat, half_host_quirk=reference_rules, partials=partials)
    walk = reference_rules if walk_on_zero is None else walk_on_zero
    V = ctx.V
    sf, si = ctx.sf, ctx.si
    img = np.zeros((h, w, 7), np.float32)
    o3 = np.zeros(3, np.float32); d3 = np.zeros(3, np.float32); dX = np.zeros(3, np.float32); dY = np.zeros(3, np.float32)
    rays18 = np.zeros(18, np.float32); ray6 = np.zeros(6, np.float32)
    debug = debug_pixels is not None
    debug_out = []
    counts = np.zeros(3, np.int64)   # of the current path: medium vertices, surface vertices, escape terms with a map after a medium vertex

    def one_path(t1, t2, x, y):
        idx = y * w + x
        k1 = [0]; k2 = [0]
        ctx.zero_now = False
        counts[:] = 0

        def draw1():
            r = f32(lib.orc_sampler_float(t1.ctypes.data, t2.ctypes.data, idx, k1[0])); k1[0] += 1
            return r

        def draw2():
            out = np.zeros(2, np.float32)
            lib.orc_sampler_float2(t1.ctypes.data, t2.ctypes.data, idx, k2[0], out.ctypes.data); k2[0] += 1
            return out
        j = np.zeros(2, np.float32) if debug else draw2()
        px, py = f32(f32(x) + j[0]), f32(f32(y) + j[1])
        ap = draw2()   # the aperture sample (a perspective sensor ignores it)
        diff = None
        if partials:   # sampleRayDifferential: its own ray, then the x and the y ray (origin, direction each), as orc_render with partials hands them to pathTrace
            lib.orc_sensor_sample_rays(C.addressof(desc.camera), float(px), float(py), float(ap[0]), float(ap[1]), rays18.ctypes.data, ray6.ctypes.data)
            ro, rd = ray6[0:3].copy(), ray6[3:6].copy()
            diff = np.ascontiguousarray(rays18[6:18])
        else:
            lib.orc_sensor_sample_ray_differential(C.addressof(desc.camera), float(px), float(py), o3.ctypes.data, d3.ctypes.data, dX.ctypes.data, dY.ctypes.data)
            ro, rd = o3.copy(), d3.copy()
        cl, cf = v3(0), v3(1)
        depth = 0; specular = False; had_hit = False; after_medium = False
        nor_written = False; zero_seen = False
        lib.orc_path_state_init(ctx.buf)   # brdf_scattering_pdf = 0, last_nor = 0 (the reference's last_nor is uninitialised), an empty BSDF record
        mRec = zero_rec()   # (the reference's is uninitialised)
        is_direct = True if debug else direct
        exhausted = False
        while depth < max_path_length:
            depth += 1
            hd = ctx.trace(ro, rd)
            had_hit = hd["tri_idx"] >= 0
            dist = f32(hd["dist"]) if had_hit else FLT_MAX   # TraceResult::Init leaves FLT_MAX
            in_medium = False; interaction = False
            if V.n:
                in_medium = V.intersect(ro, rd, f32(0), dist)[0]
                if in_medium and V.sample_distance(ro, rd, f32(0), dist, draw1(), mRec):   # the WHOLE segment, and the draw whenever in the medium
                    interaction = True
                    counts[0] += 1; after_medium = True
                    cf = _mul(cf, _sdiv(_mul(mRec["sigmaS"], mRec["transmittance"]), mRec["pdfSuccess"]))
                    if is_direct:
                        out = np.zeros(15, np.float32); ref = np.ascontiguousarray(mRec["p"]); refN = v3(0)
                        sl = draw2()
                        lib.orc_sample_emitter_direct(C.addressof(desc), ref.ctypes.data, refN.ctypes.data, float(sl[0]), float(sl[1]), out.ctypes.data)
                        value, dpdf, dd, ddist, dp = out[0:3].copy(), f32(out[3]), out[4:7].copy(), f32(out[7]), out[8:11].copy()
                        if desc.num_lights == 0:
                            dp = v3(0)
                        value = _mul(value, V.eval_transmittance(ref, dp))   # sampleAttenuatedEmitterDirect
                        if not (value == 0).all():
                            p = V.p(mRec["p"], (-rd).astype(np.float32), dd)
                            if p != 0:
                                if ctx.trace(ref, dd, f32(ddist - ctx.eps), any_hit=True)["tri_idx"] < 0:   # Occluded(Ray(ref, d), 0, dist)
                                    weight = _power_heuristic(dpdf, p)
                                    cl = _add(cl, _mul(_mul(_mul(cf, value), p), weight))
                    wgt, _, wo = V.sample(mRec["p"], (-rd).astype(np.float32), draw2())
                    if wgt == 0 and not wo.any():
                        ctx.unset_directions += 1   # no region found: the reference walks on along pRec.wo, which nothing has set
                    cf = _mul(cf, wgt)
                    rd = wo; ro = mRec["p"].copy()
            if not interaction and had_hit:
                if in_medium:
                    if not mRec["written"]:
                        ctx.unwritten_reads += 1
                    cf = _mul(cf, _sdiv(mRec["transmittance"], mRec["pdfFailure"]))
                # the oracle's own vertex (ocore.h pathVertex): getBsdfSample, first-hit partials, emission with its MIS weight, the BSDF sample, UniformSampleOneLight +
                # EstimateDirect(attenuated = true) through the transmittance hook, specularBounce / cf / the next ray.  The state buffer carries what lives across vertices
                sf[0:3] = cl; sf[3:6] = cf; sf[6:9] = ro; sf[9:12] = rd; si[1] = k1[0]; si[2] = k2[0]
                ctx.vertex(t1, t2, idx, depth, is_direct, diff)
                if si[4] and not nor_written:   # the emission's MIS weight read last_nor (DirectSamplingRecFromRay) and no surface vertex had set it
                    ctx.unwritten_normal_reads += 1
                nor_written = True
                cl, cf, ro, rd = sf[0:3].copy(), sf[3:6].copy(), sf[6:9].copy(), sf[9:12].copy(); k1[0] = int(si[1]); k2[0] = int(si[2])
                specular = bool(si[0])
                counts[1] += 1; after_medium = False
            if not interaction and not had_hit:
                break
            if (cf == 0).all():   # the library's cut: a path whose throughput is exactly zero ends (the reference walks on and adds zeros)
                if not walk:
                    break
                if not zero_seen:
                    ctx.zero_walks += 1; zero_seen = ctx.zero_now = True
            if depth > rr_start and not specular:
                q = _max3(cf)
                if draw1() >= q:
                    break
                cf = _sdiv(cf, q)
        else:
            exhausted = True
        if not had_hit:   # PathTracer.cu:98-111, the oracle's pathEscape: the environment map with its MIS weight (InfiniteLight::pdfDirect reads d alone, not refN), or cf * 0
            sf[0:3] = cl; sf[3:6] = cf; sf[6:9] = ro; sf[9:12] = rd
            lib.orc_path_escape(ctx.handle, ctx.buf, depth + 1 if exhausted else depth, 1 if is_direct else 0, float(FLT_MAX))   # `while (depth++ < maxPathLength)` leaves depth + 1 behind when it runs out
            cl = sf[0:3].copy()
            if after_medium and desc.env_map_index != 0xffffffff:
                counts[2] += 1
        return px, py, cl

    if debug:
        t1, t2 = (np.ascontiguousarray(a, np.float32) for a in tables[0])
        for (x, y) in debug_pixels:
            debug_out.append(one_path(t1, t2, x, y)[2])
        if ray_count is not None:
            ray_count.append(ctx.rays)
        ctx.close()
        return np.array(debug_out, np.float32)
    for t1, t2 in tables:
        t1 = np.ascontiguousarray(t1, np.float32); t2 = np.ascontiguousarray(t2, np.float32)
        for y in range(h):
            for x in range(w):
                before = (ctx.rays, ctx.unwritten_reads, V.past_table, ctx.unwritten_normal_reads, ctx.unset_directions, ctx.zero_walks, ctx.zero_rays)
                px, py, L = one_path(t1, t2, x, y)
                if vertex_counts is not None:
                    vertex_counts[y, x] += counts
                if pixel_rays is not None:
                    pixel_rays[y, x] += ctx.rays - before[0]
                if undefined is not None:
                    undefined[y, x, 0] += ctx.unwritten_reads - before[1]; undefined[y, x, 1] += V.past_table - before[2]
                    undefined[y, x, 2] += ctx.unwritten_normal_reads - before[3]; undefined[y, x, 3] += ctx.unset_directions - before[4]
                    undefined[y, x, 4] += ctx.zero_walks - before[5]; undefined[y, x, 5] += ctx.zero_rays - before[6]
                with np.errstate(**_ERR):
                    L = np.array([fmax(f32(0), L[0]), fmax(f32(0), L[1]), fmax(f32(0), L[2])], np.float32)   # clampNegative: (0 > s) ? 0 : s keeps a NaN
                ix, iy = int(np.floor(px)), int(np.floor(py))
                if ix < 0 or ix >= w or iy < 0 or iy >= h or not np.isfinite(L).all():
                    continue
                img[iy, ix, 0:3] = (img[iy, ix, 0:3] + L).astype(np.float32)
                img[iy, ix, 6] = f32(img[iy, ix, 6] + f32(1))
    if ray_count is not None:
        ray_count.append(ctx.rays)
    ctx.close()
    return img
