"""What the image-pipeline tests share (tests/test_oracle_pipeline.py, tests/test_gpu_image_pipeline.py, tests/golden/generate.py): the synthetic frames, the filters,
the edge pixels, and the two ambiguity rules — which channels of a filtered plane, and which bytes of a display image, may differ by one step between two
implementations whose exp / sin / pow differ in the last places.  Both rules are derived here from stated accuracies, never from an observed run."""
import numpy as np

from oracle import pipeline as P

F = np.float32
U = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)
SPLAT_SCALE = 0.25

FILTER_PARAMS = {"box": (1, 0.0, 0.0), "gaussian": (2, 2.0, 0.0), "gaussian_default": (2, -2.0, 0.0), "mitchell": (3, 1.0 / 3.0, 1.0 / 3.0), "lanczos": (4, 3.0, 0.0),
                 "triangle": (5, 0.0, 0.0), "mitchell_b3": (3, 3.0, 0.0)}   # mitchell_b3: Mitchell1D(0) = (6 - 2B) / 6 = 0, a filter whose own-pixel weight is exactly 0
POLYNOMIAL = ("box", "mitchell", "triangle")
WIDTHS = ((0.4, 0.4), (1.0, 1.0), (1.5, 1.5), (1.0, 2.0), (2.0, 1.0), (2.0, 2.0), (6.0, 6.0), (64.0, 64.0))


def flt(name, xw, yw=None):
    t, p0, p1 = FILTER_PARAMS[name]
    return dict(type=t, xw=float(xw), yw=float(xw if yw is None else yw), p0=p0, p1=p1)


def api_filter(api, f):
    return api.ctl_reconstruction_filter(f["type"], f["xw"], f["yw"], f["p0"], f["p1"])


def plain_frame(w, h, seed=1):
    """weights 1..4, rgb over seven binades (neighbouring pixels differ in their RGBE exponent), non-zero rgb_splat"""
    rs = np.random.RandomState(seed)
    px = np.zeros((h, w, 7), F)
    px[..., 6] = rs.randint(1, 5, (h, w))
    px[..., :3] = rs.rand(h, w, 3) * 2.0 * px[..., 6:7] * np.exp2(rs.randint(-3, 4, (h, w, 1)))
    px[..., 3:6] = rs.rand(h, w, 3) * 0.4
    return px


NAN, INF = float("nan"), float("inf")
EDGE_PIXELS = (("weight 0 (rgb undivided)", (0.7, 0.2, 1.3, 0, 0, 0, 0)),
               ("negative rgb, positive maximum", (-0.5, 0.3, -2.0, 0, 0, 0, 1)),
               ("negative maximum", (-1.0, -2.0, -3.0, 0, 0, 0, 2)),
               ("splat only", (0, 0, 0, 0.8, 0.4, 0.2, 0)),
               ("1e30", (1e30, 5e29, 1e28, 0, 0, 0, 1)),
               ("below 1e-32", (5e-33, 1e-33, 0, 0, 0, 0, 1)),
               ("NaN in r (finite maximum)", (NAN, 0.5, 0.25, 0, 0, 0, 1)),
               ("NaN in b (NaN maximum)", (0.5, 0.25, NAN, 0, 0, 0, 1)),
               ("+Inf in g", (0.5, INF, 0.1, 0, 0, 0, 1)),
               ("large negative beside positive", (3.0, -40.0, 0.5, 0, 0, 0, 1)))


def edge_positions(w, h):
    """a 5-pixel lattice from (2, 2): the 5 x 5 windows of the widest filter used on a salted frame (width 2) around two edge pixels never overlap"""
    return [(x, y) for y in range(2, h - 2, 5) for x in range(2, w - 2, 5)]


def salted_frame(w, h, seed=2):
    px = plain_frame(w, h, seed)
    pos = edge_positions(w, h)
    assert len(pos) >= len(EDGE_PIXELS), (w, h)
    for (x, y), (_, v) in zip(pos, EDGE_PIXELS):
        px[y, x] = v
    return px


def zero_sum_frame():
    """3 x 2: the values under a whole-image box window sum to exactly 0 (a, -a, zeros)"""
    px = np.zeros((2, 3, 7), F)
    px[..., 6] = 1
    px[0, 0, :3] = (0.75, 1.5, 0.375); px[0, 1, :3] = (-0.75, -1.5, -0.375)
    return px


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# Rule 1: the filtered plane of the Gaussian and the Lanczos filter
#
# Two implementations evaluate  r = (sum_i w_i s_i) / (sum_i w_i)  per channel over the same n taps in the same order in fp32, with weights that differ:
# |w_i - w'_i| <= EPS_W * max(|w_i|, 1e-3), the bound tests/test_oracle_pipeline.py::test_filter_functions_against_the_reference asserts between numpy and the C library
# (4 ulp of the larger factor: 4 * 1.2e-7 * 8 = 32 ulp of the weight).  The device's expf and sinf are measured at 0.84 and 1.53 ulp against float64
# (tools/pipeline_math_probe.hip, RESULTS.md): a device weight — two such factors, two subtractions or four divisions and a product — lies within 2 * (2 * 1.53 + 2.5) < 12 ulp,
# inside the same bound.  Against the float64 value of the sums with the weights w_i:
#   numerator:    |num' - num| <= EPS_W * sum max(|w_i|, 1e-3) |s_i|  +  (n + 1) U sum |w_i s_i|      (weights; one rounding per product and per addition, n taps)
#   denominator:  |den' - den| <= EPS_W * sum max(|w_i|, 1e-3)        +  n U sum |w_i|
#   quotient:     |r' - r| <= (dnum + |r| dden) / (|den| - dden) + U |r|                                 (first-order quotient perturbation with the exact remainder; one rounding)
# Float3ToRGBE scales by f = fl(mant * 256 / max) = 2^(8 - e) (1 + d), |d| <= U, and rounds the product once: the scaled channel v = r * 2^(8 - e) <= 256 carries
#   margin = 2^(8 - e) |r' - r| + 3 * 256 * U.
# A byte may differ by one step only where v (float64) lies within `margin` of an integer; the exponent may differ only where the maximum's v lies within `margin` of 128 or
# 256 (the pixel then counts with all three channels); a pixel whose |den| <= dden has no bound and counts as ambiguous with all three channels;
# a pixel whose maximum is negative beyond |r' - r| (negative lobes) is word 0 on either side.
EPS_W = 4 * 1.2e-7 * 8
AMBIGUOUS_SHARE_CAP = 0.02


def filtered_rule(px, splat_scale, f):
    """float64 evaluation of the filtered plane with the restatement's fp32 weights -> (v, margin, zero, unbounded): scaled channels (h, w, 3), their margins, the pixels
    whose word is 0 on either side and the pixels without a bound"""
    h, w = px.shape[:2]
    spec = P.to_spectrum(px, splat_scale).astype(np.float64)
    rx, ry = min(int(np.floor(f["xw"])), w - 1), min(int(np.floor(f["yw"])), h - 1)
    num = np.zeros((h, w, 3)); a_num = np.zeros((h, w, 3)); c_num = np.zeros((h, w, 3))
    den = np.zeros((h, w)); a_den = np.zeros((h, w)); c_den = np.zeros((h, w)); n = np.zeros((h, w))
    ys, xs = np.mgrid[0:h, 0:w]
    for dy in range(-ry, ry + 1):
        for dx in range(-rx, rx + 1):
            wt = float(P.filter_eval(f, abs(dx), abs(dy))); wa = max(abs(wt), 1e-3)
            yy, xx = ys + dy, xs + dx
            ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            src = spec[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)] * ok[..., None]
            num += src * wt; a_num += np.abs(src * wt); c_num += np.abs(src) * wa
            den += ok * wt; a_den += ok * abs(wt); c_den += ok * wa; n += ok
    d_num = EPS_W * c_num + (n + 1)[..., None] * U * a_num
    d_den = EPS_W * c_den + n * U * a_den
    unbounded = np.abs(den) <= d_den
    safe = np.where(unbounded, 1.0, den)
    r = num / safe[..., None]
    d_r = (d_num + np.abs(r) * d_den[..., None]) / (np.abs(safe) - np.where(unbounded, 0.0, d_den))[..., None] + U * np.abs(r)
    m = r.max(axis=-1); d_m = np.take_along_axis(d_r, r.argmax(axis=-1)[..., None], axis=-1)[..., 0]
    zero = ~unbounded & (m < -d_m)                   # a maximum below 0 beyond its bound (negative lobes): word 0 on either side
    unbounded |= ~zero & ~(m > 1e-30 + d_m)          # (a maximum within its bound of the 1e-32 threshold: no rule)
    _, e = np.frexp(np.where(unbounded | zero, 1.0, m))
    scale = np.exp2(8.0 - e)[..., None]
    return r * scale, d_r * scale + 3 * 256 * U, zero, unbounded


def ambiguous_channels(px, splat_scale, f):
    """-> (amb (h, w, 3), exp_amb (h, w), zero (h, w), v, margin): the channels that may differ by a step, the pixels whose exponent may differ, the pixels that are word 0"""
    v, margin, zero, unbounded = filtered_rule(px, splat_scale, f)
    dist = np.where(v >= 0, np.abs(v - np.rint(v)), -v)      # a negative channel saturates to 0: ambiguous only within its margin of 0
    vmax = v.max(axis=-1); mmax = np.take_along_axis(margin, v.argmax(axis=-1)[..., None], axis=-1)[..., 0]
    exp_amb = unbounded | (np.abs(vmax - 128) <= mmax) | (np.abs(vmax - 256) <= mmax)
    return ((dist <= margin) | exp_amb[..., None]) & ~zero[..., None], exp_amb, zero, v, margin


def compare_filtered_with_rule(got, want, px, splat_scale, f, what):
    """got, want: RGBE planes.  Asserts the rule; returns the share of ambiguous channels (printed)"""
    amb, exp_amb, zero, v, margin = ambiguous_channels(px, splat_scale, f)
    gb = np.stack([(got >> s) & 0xff for s in (0, 8, 16)], axis=-1).astype(int); wb = np.stack([(want >> s) & 0xff for s in (0, 8, 16)], axis=-1).astype(int)
    step = np.abs(gb - wb)
    bad = ((step > 0) & ~amb) | ((step > 1) & ~exp_amb[..., None])
    bad_exp = (((got >> 24) != (want >> 24)) & ~exp_amb) | (zero & ((got != 0) | (want != 0)))
    share = float(amb.mean())
    print("%s: %d of %d channels ambiguous (%.4f), %d differ, %d pixels differ in the exponent" % (what, int(amb.sum()), amb.size, share, int((step > 0).sum()), int(((got >> 24) != (want >> 24)).sum())))
    assert not bad.any() and not bad_exp.any(), (what, int(bad.sum()), int(bad_exp.sum()), np.argwhere(bad)[:8].tolist(), gb[bad][:8].tolist(), wb[bad][:8].tolist(), v[bad][:8].tolist(), margin[bad][:8].tolist())
    assert share <= AMBIGUOUS_SHARE_CAP, (what, share)
    return share


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# Rule 2: the bytes of the display image
#
# gammaCorrecture: s = v <= 0.0031308 ? 12.92 v : 1.055 powf(v, 1 / 2.4) - 0.055, byte = (unsigned char)(clamp01(s) * 255), all in fp32.  With a powf of at most k ulp
# (p <= 1, so an ulp is at most 2^-23 p <= 2^-23) and one rounding (relative U) per product and difference, every operand at most 1.055:
#   |t' - t| <= 255 (1.055 k 2^-23 + 1.055 U + U + U) = 255 U (2.11 k + 3.055)        for t = 255 s
# The linear branch has two roundings and is inside the same figure.  k: the ROCm documents installed with the toolchain state no figure for powf, so it is measured
# against float64 on the device (tools/pipeline_math_probe.hip: 1.29 ulp over 2^22 arguments in [0.0031308, 1], RESULTS.md) and doubled: POWF_ULP = 2.58.  glibc states
# 1 ulp for powf, numpy's float32 power calls it.  A byte may differ by one step from floor(t) of the float64 evaluation only where t lies within SRGB_MARGIN of an integer.
POWF_ULP = 2 * 1.29
SRGB_MARGIN = 255 * U * (2.11 * POWF_ULP + 3.055)
SRGB_AMBIGUOUS_CAP = 0.01


def srgb_float64(lin):
    """t = 255 srgb(v), before the clamp, in float64 with the fp32 constants of the reference (Spectrum.cu:229-235)"""
    v = np.asarray(lin, F).astype(np.float64)
    with np.errstate(invalid="ignore"):
        s = np.where(v <= float(F(0.0031308)), float(F(12.92)) * v, float(F(1.055)) * np.power(np.maximum(v, 0.0), float(F(1.0 / 2.4))) - float(F(0.055)))
    return 255.0 * s


T_ONE = 255.0 * (float(F(1.055)) - float(F(0.055)))      # srgb_float64(1.0)


def srgb_ambiguous(t_raw):
    """t_raw = 255 srgb(v) before the clamp: certain below 0 and above 255 beyond the margin (the clamp), at an exact 0 (12.92 * 0) and at v = 1 (T_ONE: powf(1, y) is
    exactly 1 (C Annex F), the rest is IEEE arithmetic: fl(fl(1.055f - 0.055f) * 255) = 254.99998, the same byte everywhere); else within the margin of an integer"""
    with np.errstate(invalid="ignore"):
        inside = (t_raw > -SRGB_MARGIN) & (t_raw < 255 + SRGB_MARGIN) & (t_raw != 0) & (t_raw != T_ONE)
        return inside & (np.abs(t_raw - np.rint(t_raw)) <= SRGB_MARGIN)


def compare_display_with_rule(got, lin, what, cap=SRGB_AMBIGUOUS_CAP):
    """got: (..., 4) uint8 display image; lin: (..., 3) float32 linear input of gammaCorrecture"""
    t = srgb_float64(lin)
    with np.errstate(invalid="ignore"):
        want = np.floor(np.where(t > 0, np.where(t < 255, t, 255.0), 0.0)).astype(int)      # clamp01 with a > b ? a : b: NaN -> 0
    amb = srgb_ambiguous(t)
    step = np.abs(got[..., :3].astype(int) - want)
    bad = ((step > 0) & ~amb) | (step > 1)
    share = float(amb.mean())
    print("%s: %d of %d bytes ambiguous (%.5f), %d differ from the float64 value" % (what, int(amb.sum()), amb.size, share, int((step > 0).sum())))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:8].tolist(), got[..., :3][bad][:8].tolist(), want[bad][:8].tolist(), t[bad][:8].tolist())
    assert (got[..., 3] == 255).all(), what
    assert share <= cap, (what, share)
    return share


def assert_same_plane(got, want, what, exempt=None):
    """bit for bit, but for the pixels of `exempt`; prints the first differing pixels"""
    bad = got != want
    if exempt is not None:
        bad &= ~exempt
    print("%s: %d of %d pixels differ" % (what, int(bad.sum()), bad.size))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:8].tolist(), [hex(v) for v in got[bad][:8]], [hex(v) for v in want[bad][:8]])


def grey_rgbe_words():
    """every grey RGBE value <= 1 with top mantissa 128..255 over the exponents that reach a non-zero byte: m * 2^(e - 136), e = 116 (255 * 2^-20 * 12.92 * 255 = 0.8: the
    last all-zero exponent) .. 128, and 1.0 itself (128 * 2^-7): 13 * 128 + 1 values"""
    m, e = np.meshgrid(np.arange(128, 256, dtype=np.uint32), np.arange(116, 129, dtype=np.uint32))
    m, e = np.append(m.ravel(), np.uint32(128)), np.append(e.ravel(), np.uint32(129))
    return (m | (m << 8) | (m << 16) | (e << 24)).astype(np.uint32)


def coloured_rgbe_words(seed=5, n=384):
    """top mantissa 128..255 in a random channel, small second and third mantissas (0..40), exponents around 1"""
    rs = np.random.RandomState(seed)
    q = rs.randint(0, 41, (n, 3)).astype(np.uint32)
    q[np.arange(n), rs.randint(0, 3, n)] = rs.randint(128, 256, n)
    e = rs.randint(118, 129, n).astype(np.uint32)
    return (q[:, 0] | (q[:, 1] << 8) | (q[:, 2] << 16) | (e << 24)).astype(np.uint32)


def frame_of_rgbe(words, w):
    """a frame (weight 1, no splat) whose pixels are the exact values of `words`, padded with zeros to whole rows of w"""
    n = len(words); h = (n + w - 1) // w
    px = np.zeros((h * w, 7), F)
    px[:n, :3] = P.from_rgbe(words); px[:, 6] = 1
    return px.reshape(h, w, 7)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/golden/pipeline.npz (inputs are rebuilt from here; the fixture holds the reference's outputs)
GOLDEN_SALTED_WIDTHS = ((0.4, 0.4), (1.0, 1.0), (1.5, 1.5), (2.0, 2.0))


def golden_filter_cases():
    """(key, frame, filter): the 12 x 8 frame under all filters and widths, the 3 x 2 frame (smaller than any footprint), the edge pixels in a 22 x 15 frame under the
    polynomial filters, the zero-sum frame, the filter whose only weight is 0"""
    out = []
    main, tiny, salted, zs = plain_frame(12, 8, seed=2), plain_frame(3, 2), salted_frame(22, 15), zero_sum_frame()
    for name in ("box", "gaussian", "gaussian_default", "mitchell", "lanczos", "triangle"):
        for wd in WIDTHS:
            out.append(("plain12x8/%s/%gx%g" % (name, wd[0], wd[1]), main, flt(name, *wd)))
        for wd in ((1.0, 1.0), (2.0, 2.0), (64.0, 64.0)):
            out.append(("plain3x2/%s/%gx%g" % (name, wd[0], wd[1]), tiny, flt(name, *wd)))
    for name in ("box", "mitchell"):
        for wd in GOLDEN_SALTED_WIDTHS:
            out.append(("salted22x15/%s/%gx%g" % (name, wd[0], wd[1]), salted, flt(name, *wd)))
    out.append(("salted22x15/triangle/2x2", salted, flt("triangle", 2.0)))
    for name, wd in (("box", 0.4), ("box", 64.0), ("mitchell", 2.0)):
        out.append(("zerosum3x2/%s/%gx%g" % (name, wd, wd), zs, flt(name, wd)))
    out.append(("plain9x5/mitchell_b3/0.4x0.4", plain_frame(9, 5), flt("mitchell_b3", 0.4)))
    return out


def golden_reinhard_inputs():
    """(words, scale, invWp2): random RGBE words over 50 exponents, the greys, word 0; scales and white points from nothing to everything (0, inf, the burn = 1 clamp)"""
    rs = np.random.RandomState(11)
    n = 768
    words = (rs.randint(0, 256, n).astype(np.uint32) | (rs.randint(0, 256, n).astype(np.uint32) << 8) | (rs.randint(0, 256, n).astype(np.uint32) << 16) |
             (rs.randint(100, 150, n).astype(np.uint32) << 24))
    words[:128] = grey_rgbe_words()[::13][:128]; words[128] = 0; words[129] = 0x80ffffff; words[130] = 0xff010101
    scale = rs.choice(np.array([0.18 / 0.3, 1.7, 1e-3, 40.0, 1e20, 0.0], F), n).astype(F)
    inv = rs.choice(np.array([0.0, 0.37, 12.5, 1e-6, 1e32, np.inf], F), n).astype(F)
    k = 600                                                                    # the everyday range: luminances around the key, a white point above them
    words[131:k] = (words[131:k] & np.uint32(0x00ffffff)) | (rs.randint(124, 134, k - 131).astype(np.uint32) << 24)
    scale[:k] = F(0.18) / rs.uniform(0.05, 2.0, k).astype(F); inv[:k] = (F(1) / rs.uniform(0.5, 30.0, k).astype(F) ** 2).astype(F)
    return words, scale, inv


def golden_gamma_inputs():
    """spectra for gammaCorrecture: the clamp range and beyond, the branch point 0.0031308 and its neighbours, the 256 values of an RGBCOL byte, non-finite values"""
    rs = np.random.RandomState(12)
    c = rs.uniform(-0.2, 1.2, (1024, 3)).astype(F)
    t = F(0.0031308)
    near = np.array([np.nextafter(t, F(0)), t, np.nextafter(t, F(1)), t * F(0.5), t * F(2), 0.0, -0.0, 1.0, np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2))], F)
    c[:10, 0] = near; c[10:20, 1] = near; c[20:30, 2] = near
    c[30:286] = (np.arange(256, dtype=F) / F(255.0))[:, None]
    c[286:542] = rs.uniform(0, 0.0031308, (256, 3)).astype(F)                  # the linear branch: no pow
    c[542] = (NAN, 0.5, 0.25); c[543] = (0.5, INF, -INF); c[544] = (1e30, 1e-30, -1e30)
    return c
