"""Helper of the NonLocalMeans tests (not collected): numpy restatement of the reference's NonLocalMeansFilter
(Kernel/ImagePipeline/Filter/NonLocalMeansFilter.cu: copyToCached :150-158, patchDistance :68-91, weight :93-99, applyWeights :122-148) and of
PixelVarianceInfo::updateMoments / computeVariance (Kernel/PixelVarianceBuffer.h:21-46, Math/VarAccumulator.h:7-11).

Everything is float32 in the reference's operation order: patch offsets x outer / y inner, candidates xo outer / yo inner.  Vectorised over pixels, looped over
offsets.  `min` / `max` are the device's fminf / fmaxf (a NaN operand yields the other one: np.fmin / np.fmax), half(float) is round-to-nearest-even with
overflow to infinity (numpy's float16), exp is the library's own (ctl_fmath.h through ctl_shared_math_eval on the host: the one the kernel evaluates), RGBE is
oracle/pipeline.py's.  The reference's kernels cannot be compiled here, so this file is held by reading them and by the closed forms of tests/test_nlm_host.py.
"""
import ctypes as C

import numpy as np

from oracle.pipeline import to_spectrum, to_rgbe, from_rgbe

F = np.float32
R, FP = 6, 3   # NonLocalMeansFilter::Apply: search radius, patch radius


def shared_exp(x):
    """ctl_fmath.h's exp on the host (needs no GPU)"""
    import cudatracerlib_amd as ctl
    x = np.ascontiguousarray(x, F)
    out = np.empty_like(x)
    rc = ctl.lib.ctl_shared_math_eval(C.c_int32(6), C.c_uint32(x.size), x.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_int32(0))
    assert rc == 0, ctl.lib.ctl_last_error()
    return out


def half_round_trip(v):
    """half(float).ToFloat() (Math/half.h:21-84)"""
    with np.errstate(all="ignore"):
        return np.asarray(v, F).astype(np.float16).astype(F)


def copy_to_cached(px, splat_scale):
    """copyToCached: PixelData::toSpectrum(splatScale).toRGBE() -> (h, w) uint32"""
    return to_rgbe(to_spectrum(np.asarray(px, F), splat_scale))


def _window(a, dx, dy, pad):
    """b[y, x] = a_padded[y + dy, x + dx] for an array padded by `pad` on every side"""
    h, w = a.shape[0] - 2 * pad, a.shape[1] - 2 * pad
    return a[pad + dy:pad + dy + h, pad + dx:pad + dx + w]


def nlm_weights(col, variance, k=0.45, sigma2_scale=0.005):
    """computeWeights: yields (xo, yo, inside, weight) per candidate offset in the reference's order; inside = candidate within the image.
    col = (h, w, 3) float32 decoded from RGBE, variance = (h, w) computeVariance()"""
    h, w = col.shape[:2]
    P = R + FP
    var = (half_round_trip(variance) * F(sigma2_scale)).astype(F)
    colp = np.zeros((h + 2 * P, w + 2 * P, 3), F); colp[P:P + h, P:P + w] = col
    varp = np.zeros((h + 2 * P, w + 2 * P), F); varp[P:P + h, P:P + w] = var
    okp = np.zeros((h + 2 * P, w + 2 * P), bool); okp[P:P + h, P:P + w] = True
    kk = F(F(k) * F(k)); eps = F(1e-10); third = F(1.0) / F(3)
    with np.errstate(all="ignore"):
        for xo in range(-R, R + 1):
            for yo in range(-R, R + 1):
                # the term of patchDistance for every pixel p' (as p + d) of the image and its F-halo, and whether p' and p' + o are both inside
                ext = (h + 2 * FP, w + 2 * FP)
                cp = colp[R:R + ext[0], R:R + ext[1]]; cq = colp[R + yo:R + yo + ext[0], R + xo:R + xo + ext[1]]
                vp = varp[R:R + ext[0], R:R + ext[1]]; vq = varp[R + yo:R + yo + ext[0], R + xo:R + xo + ext[1]]
                ok = okp[R:R + ext[0], R:R + ext[1]] & okp[R + yo:R + yo + ext[0], R + xo:R + xo + ext[1]]
                d = cp - cq; sq = d * d
                u_diff = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]) * third
                term = (u_diff - (vp + np.fmin(vp, vq))) / (eps + kk * (vp + vq))
                d_range = np.zeros((h, w), F); count = np.zeros((h, w), F)
                for dx in range(-FP, FP + 1):
                    for dy in range(-FP, FP + 1):
                        t, v = _window(term, dx, dy, FP), _window(ok, dx, dy, FP)
                        d_range = np.where(v, d_range + t, d_range).astype(F)
                        count = np.where(v, count + F(1), count).astype(F)
                d_range = np.where(count != 0, d_range / np.where(count != 0, count, F(1)), F(0)).astype(F)
                we = shared_exp(-np.fmax(F(0), d_range))
                we = np.where(we < F(0.05), F(0), we).astype(F)
                yield xo, yo, _window(okp, xo, yo, P), we


def nlm_filter(px, splat_scale, variance, k=0.45, sigma2_scale=0.005, return_weights=False):
    """NonLocalMeansFilter::Apply with fresh weights -> the filtered RGBE plane (h, w) uint32 (and, on request, the weights of the candidates inside the image)"""
    col = from_rgbe(copy_to_cached(px, splat_scale))
    h, w = col.shape[:2]
    colp = np.zeros((h + 2 * R, w + 2 * R, 3), F); colp[R:R + h, R:R + w] = col
    c_hat = np.zeros((h, w, 3), F); C_p = np.zeros((h, w), F)
    kept = []
    with np.errstate(all="ignore"):
        for xo, yo, inside, we in nlm_weights(col, np.asarray(variance, F).reshape(h, w), k, sigma2_scale):
            use = inside & ~np.isnan(we)
            c_q = colp[R + yo:R + yo + h, R + xo:R + xo + w]
            C_p = np.where(use, C_p + we, C_p).astype(F)
            c_hat = np.where(use[..., None], c_hat + we[..., None] * c_q, c_hat).astype(F)
            if return_weights:
                kept.append(we[inside])
        recip = (F(1.0) / np.where(C_p > F(1e-4), C_p, F(1))).astype(F)
        out = np.where((C_p > F(1e-4))[..., None], c_hat * recip[..., None], col).astype(F)
    plane = to_rgbe(out)
    return (plane, np.concatenate(kept)) if return_weights else plane


class PixelVariance:
    """PixelVarianceBuffer: updateMoments per pass with every block sampled once, computeVariance"""

    def __init__(self, h, w):
        self.prev_I = np.zeros((h, w, 3), F); self.half_buffer = np.zeros((h, w, 3), F)
        self.iterations_done = 0
        self.sum_x = np.zeros((h, w), F); self.sum_x2 = np.zeros((h, w), F); self.num_samples_var = 0

    def update_moments(self, px, splat_scale, performed=1.0):
        px = np.asarray(px, F)
        new_sum = (px[..., 0:3] + px[..., 3:6] * F(splat_scale)).astype(F)
        est = ((new_sum - self.prev_I) / F(performed)).astype(F)
        self.prev_I = new_sum
        if self.iterations_done % 2 == 1:
            self.half_buffer = (self.half_buffer + est).astype(F)
        self.iterations_done += 1
        lum = (est[..., 0] * F(0.212671) + est[..., 1] * F(0.715160) + est[..., 2] * F(0.072169)).astype(F)
        self.sum_x = (self.sum_x + lum).astype(F); self.sum_x2 = (self.sum_x2 + lum * lum).astype(F)
        self.num_samples_var += 1

    def compute_variance(self):
        with np.errstate(all="ignore"):
            inv_n = F(1.0) / F(self.num_samples_var)
            return ((self.sum_x2 - (self.sum_x * self.sum_x) * inv_n) * inv_n).astype(F)


def synthetic_frame(w, h, sigma=0.05, seed=7, sigma2_scale=0.005):
    """two flat regions with an edge, a sine ramp across them, Gaussian noise of `sigma` per channel; the variance a tracer would report for it,
    sigma^2 / sigma2_scale times a factor in [0.5, 2].  Returns (noise-free (h, w, 3), PixelData (h, w, 7), variance (h, w), splat_scale)"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    base = np.where(xs < w // 2, 0.25, 0.7)[..., None] * np.array([1.0, 0.8, 0.6]) + 0.1 * np.sin(ys / 5.0)[..., None] * np.array([0.5, 1.0, 0.7]) + 0.15
    clean = base.astype(F)
    noisy = np.maximum(clean + rng.normal(0.0, sigma, clean.shape), 0.0).astype(F)
    # a non-trivial PixelData: weightSum of a few samples, a quarter of the value carried by the splat term at splat_scale = 0.25
    splat_scale = 0.25
    wsum = rng.integers(3, 9, (h, w)).astype(F)
    px = np.zeros((h, w, 7), F)
    px[..., 6] = wsum
    px[..., 0:3] = (noisy * F(0.75)) * wsum[..., None]
    px[..., 3:6] = noisy * F(0.25) / F(splat_scale)
    variance = (F(sigma * sigma / sigma2_scale) * rng.uniform(0.5, 2.0, (h, w))).astype(F)
    return clean, px, variance, splat_scale
