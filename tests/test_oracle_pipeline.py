"""Image-pipeline oracle (oracle/pipeline.py <- Kernel/ImagePipeline/*, Engine/Image.cu:88-168): closed forms."""
import numpy as np
from oracle import pipeline as P
from cudatracerlib_amd import api


def _frame(h=12, w=16, seed=1):
    rs = np.random.RandomState(seed)
    px = np.zeros((h, w, 7), np.float32)
    px[..., 6] = rs.randint(1, 5, (h, w))
    px[..., :3] = rs.rand(h, w, 3).astype(np.float32) * 2.0 * px[..., 6:7]
    px[..., 3:6] = rs.rand(h, w, 3).astype(np.float32) * 0.1
    return px


def test_rgbe_matches_the_texture_codec_and_round_trips():
    c = (np.random.RandomState(2).rand(64, 3).astype(np.float32) * np.float32(50.0)) ** 2
    c[0] = 0; c[1] = 1e-35
    enc = P.to_rgbe(c)
    assert np.array_equal(enc, api.float3_to_rgbe(c[None])[0])      # the same Float3ToRGBE the bitmap loader uses
    dec = P.from_rgbe(enc)
    assert np.all(dec[:2] == 0)
    m = c.max(axis=1)
    assert np.all(np.abs(dec[2:] - c[2:]) <= (m[2:] / 128)[:, None] + 1e-30)   # 8-bit mantissa under a shared exponent


def test_no_filter_no_process_is_gamma_of_to_spectrum():
    px = _frame()
    out = P.apply_image_pipeline(px, 0.5)
    lin = px[..., :3] / px[..., 6:7] + px[..., 3:6] * 0.5
    want = np.where(lin <= 0.0031308, 12.92 * lin, 1.055 * np.power(lin, 1 / 2.4) - 0.055)
    assert np.abs(out[..., :3].astype(int) - np.floor(np.clip(want, 0, 1) * 255).astype(int)).max() <= 1
    assert np.all(out[..., 3] == 255)


def test_box_filter_is_the_window_mean_and_constant_images_stay_constant():
    px = _frame()
    flt = dict(type=1, xw=1.0, yw=2.0, p0=0, p1=0)
    got = P.from_rgbe(P.canonical_filter(px, 0.0, flt))
    spec = P.to_spectrum(px, 0.0)
    h, w = spec.shape[:2]
    for (y, x) in ((0, 0), (5, 7), (11, 15), (3, 0)):
        win = spec[max(0, y - 2):min(h, y + 3), max(0, x - 1):min(w, x + 2)].reshape(-1, 3)
        want = win.mean(axis=0)
        assert np.all(np.abs(got[y, x] - want) <= want.max() / 100)
    flat = np.zeros((8, 8, 7), np.float32); flat[..., :3] = (0.25, 0.5, 0.75); flat[..., 6] = 1
    for t, p0, p1 in ((1, 0, 0), (2, 2.0, 0), (3, 1 / 3, 1 / 3), (4, 3.0, 0), (5, 0, 0)):
        f = dict(type=t, xw=2.0, yw=2.0, p0=p0, p1=p1)
        out = P.from_rgbe(P.canonical_filter(flat, 0.0, f))
        assert np.allclose(out, (0.25, 0.5, 0.75), atol=0.75 / 100), t


def test_filter_shapes():
    g = dict(type=2, xw=2.0, yw=2.0, p0=-2.0, p1=0)     # the reference's default alpha is NEGATIVE: the "Gaussian" grows outwards and is clipped at 0
    assert P.filter_eval(g, 0, 0) == 0.0 and P.filter_eval(g, 2, 2) == 0.0
    g = dict(type=2, xw=2.0, yw=2.0, p0=2.0, p1=0)
    assert P.filter_eval(g, 0, 0) > P.filter_eval(g, 1, 0) > P.filter_eval(g, 1, 1) > 0 and P.filter_eval(g, 2, 0) == 0
    t = dict(type=5, xw=2.0, yw=2.0, p0=0, p1=0)
    assert P.filter_eval(t, 0, 0) == 4 and P.filter_eval(t, 1, 1) == 1 and P.filter_eval(t, 2, 0) == 0
    m = dict(type=3, xw=2.0, yw=2.0, p0=1 / 3, p1=1 / 3)
    assert abs(P.filter_eval(m, 0, 0) - (8 / 9) ** 2) < 1e-6 and abs(P.filter_eval(m, 2, 0)) < 1e-6
    l = dict(type=4, xw=3.0, yw=3.0, p0=3.0, p1=0)
    assert P.filter_eval(l, 0, 0) == 1 and abs(P.filter_eval(l, 3, 0)) < 1e-6


def test_reinhard_of_a_grey_image():
    """uniform luminance L: Lp = key, Lwhite = key -> Y = key (1 + key / key^2 ... ) / (1 + key) = key (1 + 1/key) / (1 + key) = 1"""
    grey = np.zeros((6, 6, 7), np.float32); grey[..., :3] = 0.5; grey[..., 6] = 1
    filtered = P.to_rgbe(P.to_spectrum(grey, 0.0))
    mn, mx, avg, log_avg = P.luminance_info(filtered)
    assert abs(mn - 0.5) < 1e-6 and abs(mx - 0.5) < 1e-6 and abs(avg - 0.5) < 1e-6 and abs(log_avg - (0.5 + 2.3e-5)) < 1e-5
    out = P.reinhard(filtered, 0.18, 0.0)
    assert np.all(out[..., :3] >= 253)                             # maps to white: the brightest pixel is the white point
    final = P.apply_image_pipeline(grey, 0.0, None, dict(key=0.18, burn=0.0))
    assert np.all(final[..., :3] >= 253)
    # two luminance levels, half the pixels each: the operator in closed form
    two = grey.copy(); two[:, :3, :3] = 0.05
    out = P.reinhard(P.to_rgbe(P.to_spectrum(two, 0.0)), 0.18, 0.0).astype(int)
    lo = P.from_rgbe(P.to_rgbe(np.float32([0.05] * 3)))[0]       # what RGBE keeps of 0.05
    scale = 0.18 / np.exp(0.5 * (np.log(2.3e-5 + lo) + np.log(2.3e-5 + 0.5)))
    lw = 0.5 * scale
    y = lambda L: (L * scale) * (1 + L * scale / lw ** 2) / (1 + L * scale)
    assert abs(out[0, 0, 0] - int(y(lo) * 255)) <= 1 and out[0, 5, 0] >= 253


def test_filter_functions_against_the_reference():
    """Box / Gaussian / Mitchell / Lanczos-sinc / triangle Evaluate (SceneTypes/Filter.h:28-171) of the numpy restatement against values computed by the
    reference's own header (tests/golden/filters.npz).  Box, Mitchell and triangle are polynomial: bit for bit.  Gaussian and Lanczos go through
    exp / sin of the C library there and of numpy here: 4 ulp of the larger factor."""
    import os
    from oracle import pipeline as P
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filters.npz"))
    worst = {}
    for cfg, xy, want in zip(g["cfg"], g["xy"], g["value"]):
        t = int(cfg[0])
        got = np.float32(P.filter_eval(dict(type=t, xw=float(cfg[1]), yw=float(cfg[2]), p0=float(cfg[3]), p1=float(cfg[4])), xy[0], xy[1]))
        if t in (1, 3, 5):
            assert got.view(np.uint32) == want.view(np.uint32), (t, cfg, xy, got, want)
        else:
            err = abs(float(got) - float(want)); worst[t] = max(worst.get(t, 0.0), err / max(abs(float(want)), 1e-3))
    assert set(worst) == {2, 4} and max(worst.values()) <= 4 * 1.2e-7 * 8, worst


# ---- the restatement against the reference's own evalFilter / Reinhard05Kernel / gammaCorrecture (tests/golden/pipeline.npz <- oracle/ref_pipeline_driver.cpp)
def _golden_pipeline():
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here)
    import pipeline_cases as K
    g = np.load(os.path.join(here, "golden", "pipeline.npz"))
    cases, at = [], 0
    for key, px, f in K.golden_filter_cases():
        h, w = px.shape[:2]
        cases.append((key, px, f, g["planes"][at:at + h * w].reshape(h, w), g["undef"][at:at + h * w].reshape(h, w)))
        at += h * w
    assert at == len(g["planes"]) == len(g["undef"])
    return K, g, cases


def _defined(plane, undef):
    """the golden plane's defined bits: (mask per word, pixels whose whole word the reference leaves undefined)"""
    mask = np.full(plane.shape, 0xffffffff, np.uint32)
    for c in range(3):
        mask &= ~(((undef >> c) & 1).astype(np.uint32) * np.uint32(0xff << (8 * c)))
    return mask, (undef & 8) != 0


def test_polynomial_filters_against_the_reference_bit_for_bit():
    """Box, Mitchell, triangle: P.canonical_filter equals evalFilter + toRGBE of the reference's own code in every defined bit — all widths (0.4: own pixel only; 1.5: a
    non-integer ceil / floor; 1 x 2 and 2 x 1; 6; 64: a whole-image window), a frame smaller than any footprint, and the edge pixels (weight 0, negative values, splat only,
    1e30, below 1e-32, NaN, +Inf, a window summing to exactly 0, a filter whose only weight is 0).  The reference's C++ defines no value in two places, which the fixture
    marks per pixel and which are the only exemptions: the whole word where the maximum is NaN or infinite (the exponent stays unwritten), and a channel byte whose scaled
    value is NaN or <= -1 (float -> unsigned char out of range; the host wraps, the device saturates).  There the restatement must give what the project defines: 0."""
    K, g, cases = _golden_pipeline()
    n = 0
    for key, px, f, want, undef in cases:
        if f["type"] not in (1, 3, 5):
            continue
        got = P.canonical_filter(px, K.SPLAT_SCALE, f)
        mask, whole = _defined(want, undef)
        K.assert_same_plane(got & mask, want & mask, key, exempt=whole)
        assert (got[whole] == 0).all(), key
        for c in range(3):                                             # an undefined byte saturates: 0 (NaN, negative) or 255 (a NaN in g hid a larger r from the maximum)
            b = ((got >> (8 * c)) & 0xff)[((undef >> c) & 1) != 0]
            assert ((b == 0) | (b == 255)).all(), key
        n += 1
    assert n >= 3 * len(K.WIDTHS) + 12
    # the edge pixels are in the fixture, and most of the salted planes is defined
    salted = [(u, w) for key, _, f, w, u in cases if key.startswith("salted")]
    assert all(((u & 8) != 0).any() and (u & 7).any() and ((u == 0).mean() > 0.5) for u, _ in salted)


def test_gaussian_and_lanczos_against_the_reference_under_the_ambiguity_rule():
    """exp and sin come from the C library there and from numpy here, so a weight may differ in its last places and a channel that lands next to an integer may fall on
    either side.  The rule, with its derivation, is tests/pipeline_cases.py "Rule 1": a byte may differ by one step only where the float64 value of the same sums lies
    within a margin of an integer, the margin being the weight bound of test_filter_functions_against_the_reference (4 * 1.2e-7 * 8, relative to max(|w|, 1e-3)) carried
    through the quotient plus the fp32 accumulation over the taps ((n + 1) U sum |w s|) and the three roundings of the RGBE scaling.  At most 2 % of a plane's channels
    may be ambiguous — checked on the fixture's own frames.  The default Gaussian (alpha = -2) weighs every tap 0: each pixel is 0 / 0, which the reference leaves
    undefined (NaN maximum) and the project defines as word 0."""
    K, g, cases = _golden_pipeline()
    shares = []
    for key, px, f, want, undef in cases:
        if f["type"] not in (2, 4):
            continue
        got = P.canonical_filter(px, K.SPLAT_SCALE, f)
        if f["p0"] < 0:
            assert ((undef & 8) != 0).all() and (got == 0).all(), key
            continue
        assert ((undef & 8) == 0).all(), key                          # (negative lobes: channels below 0 are stored as 0, which is what saturation gives)
        shares.append(K.compare_filtered_with_rule(got, want, px, K.SPLAT_SCALE, f, key))
    assert len(shares) == 2 * (len(K.WIDTHS) + 3) and max(shares) <= K.AMBIGUOUS_SHARE_CAP


def test_reinhard_against_the_reference_bit_for_bit():
    """the per-pixel body of Reinhard05Kernel with Spectrum::toYxy / fromYxy: products, sums, quotients and clamps only, so every RGBCOL word is held — greys, random
    words over 50 exponents, word 0, scales and white points including 0, infinity and the 1e-32 of burn = 1"""
    K, g, _ = _golden_pipeline()
    words, scale, inv = K.golden_reinhard_inputs()
    got = P.reinhard_pixels(words, scale, inv)
    got = got[:, 0].astype(np.uint32) | (got[:, 1].astype(np.uint32) << 8) | (got[:, 2].astype(np.uint32) << 16) | (got[:, 3].astype(np.uint32) << 24)
    bad = got != g["reinhard_rgbcol"]
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:8].ravel().tolist(), [hex(v) for v in got[bad][:8]], [hex(v) for v in g["reinhard_rgbcol"][bad][:8]])
    assert len(np.unique(got)) > 300                              # not a degenerate set: the outputs spread over the byte range


def test_gamma_correcture_against_the_reference():
    """gammaCorrecture = toSRGB + toRGBCOL.  The linear branch (v <= 0.0031308) and the clamps are held bit for bit.  The other branch goes through powf of the C library
    there and numpy's here: tests/pipeline_cases.py "Rule 2" — a byte may differ by one step from the float64 value only where 255 srgb(v) lies within SRGB_MARGIN of an
    integer (the device's measured powf error, doubled, carried through the two products and the difference — wider than glibc's 1 ulp); both sides are held to that, and to each other outside it."""
    K, g, _ = _golden_pipeline()
    c = K.golden_gamma_inputs()
    want = g["gamma_rgbcol"]
    want = np.stack([(want >> s) & 0xff for s in (0, 8, 16, 24)], axis=-1).astype(np.uint8)
    got = P.gamma_correct(c)
    with np.errstate(invalid="ignore"):
        linear = (c <= np.float32(0.0031308)) | ~np.isfinite(c)
    assert np.array_equal(got[..., :3][linear], want[..., :3][linear]) and linear.mean() > 0.25
    K.compare_display_with_rule(want, c, "gammaCorrecture, reference")
    K.compare_display_with_rule(got, c, "gammaCorrecture, restatement")
    assert not ((got[..., :3] != want[..., :3]) & ~K.srgb_ambiguous(K.srgb_float64(c))).any()


def test_to_rgbe_of_a_non_finite_maximum_is_word_zero():
    """the project's definition where the reference has none; max(a, b, c) is the reference's a > b ? a : b chain, so a NaN counts only from the last place
    (a NaN in g hides r from the maximum: r then scales past 255 and saturates)"""
    nan, inf = np.float32("nan"), np.float32("inf")
    c = np.array([[0.5, 0.25, nan], [0.5, inf, 0.1], [inf, inf, inf], [nan, nan, nan], [nan, 0.5, 0.25], [0.5, nan, 0.25], [-inf, 0.5, 0.25]], np.float32)
    got = P.to_rgbe(c)
    assert (got[:4] == 0).all()
    assert got[4] == P.to_rgbe(np.float32([0, 0.5, 0.25])) and got[5] == (255 | (128 << 16) | (127 << 24)) and got[6] == P.to_rgbe(np.float32([0, 0.5, 0.25]))


def test_luminance_info_entry_point_is_exported_and_checks_its_arguments():
    """ctl_image_luminance_info (Image.getLuminanceInfo): null arguments are CTL_ERR_INVALID with a message, with or without a device"""
    import ctypes as C
    out = np.zeros(4, np.float32)
    assert api.lib.ctl_image_luminance_info(None, out.ctypes.data_as(C.c_void_p)) == -1 and api.lib.ctl_last_error() != b""
    assert api.lib.ctl_image_luminance_info(C.cast(C.create_string_buffer(64), C.c_void_p), None) == -1
    assert hasattr(api.Image, "getLuminanceInfo")
