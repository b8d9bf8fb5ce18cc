"""ORACLE (test infrastructure, never imported by the product): numpy restatement of the reference's image pipeline —
applyImagePipeline (Kernel/ImagePipeline/ImagePipeline.cu:54-84), CanonicalFilter (Filter/CanonicalFilter.cu:6-44) over the
reconstruction filters of SceneTypes/Filter.h, ToneMapPostProcess (PostProcess/ToneMapPostProcess.cu:6-42) and
Image::ComputeLuminanceInfo (Engine/Image.cu:88-168).  All arithmetic in float32, loops in the reference's order (rows of the
filter footprint outermost).  Parity: pinned on the reference's own code (oracle/ref_pipeline_driver.cpp -> tests/golden/pipeline.npz,
tests/test_oracle_pipeline.py) — evalFilter + toRGBE, the Reinhard05Kernel body and gammaCorrecture bit for bit where the arithmetic is
polynomial, under a derived ambiguity rule where exp / sin / pow differ between the C library and numpy.  Two places where the reference's
C++ defines no value are defined here as the device defines them: a float -> unsigned char conversion out of range saturates (NaN -> 0),
and a NaN or infinite pixel maximum encodes as RGBE word 0 (frexp_self leaves the exponent unwritten there).
ComputeLuminanceInfo is a kernel of atomics and does not extract; its sums are restated in float64.
"""
import numpy as np

F = np.float32


def to_spectrum(px, splat_scale):
    """PixelData::toSpectrum (Engine/Image.h:21-28); px = (h, w, 7) float32"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = (F(1) / np.where(px[..., 6] != 0, px[..., 6], F(1)))[..., None].astype(F)   # Spectrum / scalar multiplies by the reciprocal (Math/Spectrum.h:122-128)
        return ((px[..., 0:3] * r).astype(F) + (px[..., 3:6] * F(splat_scale)).astype(F)).astype(F)


def rgbe_scaled(c):
    """the inside of Float3ToRGBE: (ok, v, e) with ok = the pixel takes the else-branch with a finite maximum, v = c * f the scaled channels before the cast, e = the exponent"""
    c = np.asarray(c, F)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.where(c[..., 0] > c[..., 1], c[..., 0], c[..., 1]); m = np.where(m > c[..., 2], m, c[..., 2])   # max(a, b) = a > b ? a : b, twice: a NaN wins only from the last place
        ok = (m >= F(1e-32)) & np.isfinite(m)                                     # a NaN / infinite maximum: word 0 (the reference leaves the exponent unwritten)
        safe = np.where(ok, m, F(1))
        mant, e = np.frexp(safe.astype(np.float64))
        f = (mant.astype(F) * F(256.0) / safe).astype(F)
        return ok, (c * f[..., None]).astype(F), e


def to_rgbe(c):
    """SpectrumConverter::Float3ToRGBE (Math/Spectrum.h:534-555) -> uint32 (r | g << 8 | b << 16 | e << 24)"""
    ok, v, e = rgbe_scaled(c)
    with np.errstate(invalid="ignore"):
        q = np.minimum(np.where(v > 0, v, F(0)), F(255)).astype(np.uint32)        # (unsigned char)(c * f), saturating as on the device: negative and NaN -> 0
    out = q[..., 0] | (q[..., 1] << 8) | (q[..., 2] << 16) | (((e + 128) & 0xff).astype(np.uint32) << 24)
    return np.where(ok, out, np.uint32(0)).astype(np.uint32)


def from_rgbe(v):
    """RGBEToFloat3 (Math/Spectrum.h:557-565)"""
    v = np.asarray(v, np.uint32)
    w = (v >> 24).astype(np.int32)
    e = np.ldexp(F(1.0), w - (128 + 8)).astype(F)
    rgb = np.stack([(v & 0xff), ((v >> 8) & 0xff), ((v >> 16) & 0xff)], axis=-1).astype(F) * e[..., None]
    return np.where((w != 0)[..., None], rgb, F(0)).astype(F)


def to_rgbcol(c):
    """Float3ToCOLORREF (Math/Spectrum.h:521-526) -> (…, 4) uint8"""
    c = np.asarray(c, F)
    with np.errstate(invalid="ignore"):
        v = np.where(c > 0, c, F(0)); v = np.where(v < 1, v, F(1))               # clamp01 = min(max(x, 0), 1) with a > b ? a : b: NaN -> 0
    q = (v * F(255.0)).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], axis=-1)


def from_rgbcol(q):
    return (np.asarray(q)[..., :3].astype(F) / F(255.0)).astype(F)


def srgb(v):
    """toSRGBComponent (Math/Spectrum.cu:229-235)"""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        return np.where(v <= F(0.0031308), F(12.92) * v, F(1.055) * np.power(np.maximum(v, F(0)), F(1.0 / 2.4)) - F(0.055)).astype(F)


def gamma_correct(c):
    return to_rgbcol(srgb(c))


def luminance(c):
    c = np.asarray(c, F)
    return (c[..., 0] * F(0.212671) + c[..., 1] * F(0.715160) + c[..., 2] * F(0.072169)).astype(F)


def filter_eval(flt, x, y):
    """Filter::Evaluate(|dx|, |dy|) (SceneTypes/Filter.h); flt = dict(type, xw, yw, p0, p1)"""
    x, y = F(x), F(y)
    t = flt["type"]
    if t == 1:
        return F(1)
    if t == 2:
        a = F(flt["p0"])
        with np.errstate(over="ignore", invalid="ignore"):                     # alpha < 0 with a wide filter: exp overflows, inf - inf = NaN
            ex, ey = np.exp(-a * F(flt["xw"]) * F(flt["xw"])), np.exp(-a * F(flt["yw"]) * F(flt["yw"]))
            gx, gy = F(np.exp(-a * x * x)) - F(ex), F(np.exp(-a * y * y)) - F(ey)
            return F(F(0) if F(0) > gx else gx) * F(F(0) if F(0) > gy else gy)   # max(0.f, v) = 0 > v ? 0 : v: a NaN stays
    if t == 3:
        B, Cc = F(flt["p0"]), F(flt["p1"])

        def m1(v):
            v = F(abs(F(2) * v))
            if v > 1:
                return F(((-B - 6 * Cc) * v * v * v + (6 * B + 30 * Cc) * v * v + (-12 * B - 48 * Cc) * v + (8 * B + 24 * Cc)) * F(1.0 / 6.0))
            return F(((12 - 9 * B - 6 * Cc) * v * v * v + (-18 + 12 * B + 6 * Cc) * v * v + (6 - 2 * B)) * F(1.0 / 6.0))
        return F(m1(x * F(1.0 / flt["xw"])) * m1(y * F(1.0 / flt["yw"])))
    if t == 4:
        tau = F(flt["p0"])

        def s1(v):
            v = F(abs(v))
            if v < 1e-5:
                return F(1)
            if v > 1:
                return F(0)
            v = F(v * F(np.pi))
            return F((np.sin(v) / v) * (np.sin(v * tau) / (v * tau)))
        return F(s1(x * F(1.0 / flt["xw"])) * s1(y * F(1.0 / flt["yw"])))
    return F(max(F(0), F(flt["xw"]) - abs(x))) * F(max(F(0), F(flt["yw"]) - abs(y)))


def canonical_filter(px, splat_scale, flt):
    """rtm_Copy (CanonicalFilter.cu:28-36) -> RGBE image (h, w) uint32"""
    return to_rgbe(eval_filter(px, splat_scale, flt))


def eval_filter(px, splat_scale, flt):
    """evalFilter (CanonicalFilter.cu:6-26) per pixel -> (h, w, 3) float32, the value before toRGBE"""
    h, w = px.shape[:2]
    spec = to_spectrum(px, splat_scale)
    rx, ry = int(np.floor(flt["xw"])), int(np.floor(flt["yw"]))
    acc = np.zeros((h, w, 3), F); accw = np.zeros((h, w), F)
    ys, xs = np.mgrid[0:h, 0:w]
    ry, rx = min(ry, h - 1), min(rx, w - 1)   # (offsets beyond the image reach no pixel)
    for dy in range(-ry, ry + 1):          # y0..y1 ascending = dy ascending, then x
        for dx in range(-rx, rx + 1):
            if abs(dx) > flt["xw"] or abs(dy) > flt["yw"]:
                continue
            wt = filter_eval(flt, abs(dx), abs(dy))
            yy, xx = ys + dy, xs + dx
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            src = spec[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
            with np.errstate(invalid="ignore", over="ignore"):
                acc = np.where(ok[..., None], (acc + src * wt).astype(F), acc)
            accw = np.where(ok, (accw + wt).astype(F), accw)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return (acc * (F(1) / accw).astype(F)[..., None]).astype(F)   # Spectrum / scalar: times the reciprocal


def luminance_info(filtered):
    """Image::ComputeLuminanceInfo: (min, max, avg, exp(mean log(2.3e-5 + Y)))"""
    Y = luminance(from_rgbe(filtered))
    n = F(Y.size)
    return F(Y.min()), F(Y.max()), F(Y.sum(dtype=np.float64) / n), F(np.exp(F(np.log(F(2.3e-5) + Y).sum(dtype=np.float64) / n)))


def tonemap_params(key, burn, max_lum, log_avg):
    """ToneMapPostProcess::Apply (ToneMapPostProcess.cu:32-35): (scale, invWp2) from the settings and the luminance info"""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        scale = F(F(key) / F(log_avg)); lwhite = F(F(max_lum) * scale)
        b = min(F(1.0), max(F(1e-8), F(F(1.0) - F(burn))))
        return scale, F(F(1) / F(F(lwhite * lwhite) * F(np.power(np.float64(b), 4.0))))   # std::pow(float, float): the correctly rounded value


def reinhard(filtered, key=0.18, burn=0.0):
    """ToneMapPostProcess::Apply + Reinhard05Kernel -> RGBCOL (h, w, 4) BEFORE the final gamma pass"""
    _, max_lum, _, log_avg = luminance_info(filtered)
    return reinhard_pixels(filtered, *tonemap_params(key, burn, max_lum, log_avg))


def reinhard_pixels(filtered, scale, inv_wp2):
    """Reinhard05Kernel (ToneMapPostProcess.cu:6-24) with Spectrum::toYxy / fromYxy (Spectrum.cu:286-302) -> RGBCOL (..., 4)"""
    scale, inv_wp2 = F(scale), F(inv_wp2)
    c = from_rgbe(filtered)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        return _reinhard_of(c, scale, inv_wp2)


def _reinhard_of(c, scale, inv_wp2):
    X = c[..., 0] * F(0.412453) + c[..., 1] * F(0.357580) + c[..., 2] * F(0.180423)
    Y0 = c[..., 0] * F(0.212671) + c[..., 1] * F(0.715160) + c[..., 2] * F(0.072169)
    Z = c[..., 0] * F(0.019334) + c[..., 1] * F(0.119193) + c[..., 2] * F(0.950227)
    s = np.clip(X + Y0 + Z, F(0.001), F(100000.0))
    x, y = X / s, Y0 / s
    Lp = scale * Y0
    Y = Lp * (F(1) + Lp * inv_wp2) / (F(1) + Lp)
    yc = np.clip(y, F(0.001), F(100000.0))
    X2, Z2 = Y / yc * x, Y / yc * (F(1) - x - y)
    rgb = np.stack([F(3.240479) * X2 + F(-1.537150) * Y + F(-0.498535) * Z2, F(-0.969256) * X2 + F(1.875991) * Y + F(0.041556) * Z2,
                    F(0.055648) * X2 + F(-0.204043) * Y + F(1.057311) * Z2], axis=-1).astype(F)
    return to_rgbcol(rgb)


def apply_image_pipeline(px, splat_scale, flt=None, process=None):
    """applyImagePipeline (ImagePipeline.cu:54-84) -> (h, w, 4) uint8"""
    if flt is None and process is None:
        return gamma_correct(to_spectrum(px, splat_scale))
    filtered = canonical_filter(px, splat_scale, flt) if flt is not None else to_rgbe(to_spectrum(px, splat_scale))
    if process is None:
        return gamma_correct(from_rgbe(filtered))
    out = reinhard(filtered, process.get("key", 0.18), process.get("burn", 0.0))
    return gamma_correct(from_rgbcol(out))
