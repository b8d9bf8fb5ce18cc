"""The canonical image pipeline on the GPU, stage by stage, against the numpy restatement (oracle/pipeline.py, pinned on the reference's own code by
tests/test_oracle_pipeline.py): the filtered RGBE plane of the five reconstruction filters (csrc/image_pipeline.hip k_filter, k_to_filtered), the output stage
(k_filtered_to_output, k_apply_pipeline, k_resolve_rgb) and the tone map (k_luminance_info, k_reinhard, k_gamma_in_place).  Synthetic frames through
Image.setPixelData, no tracer.  The frames, the edge pixels and the two ambiguity rules, with their derivations, are in tests/pipeline_cases.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pipeline_cases as K   # noqa: E402
from oracle import pipeline as P   # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
U = K.U

# 9 x 5: 45 pixels, a partial wave; 64 x 4: exactly one block of k_filter; 65 x 5, 67 x 7: the block seam in x and in y; 130 x 9: three blocks in x; 3 x 2: smaller than any footprint;
# 128 x 3: two whole blocks and no spare lane — a block stride one short of the block width leaves the last column unwritten only at such a width
SIZES = [(9, 5), (64, 4), (65, 5), (67, 7), (130, 9), (3, 2), (128, 3)]


def _widths(size):
    """0.4: own pixel only; 1.5: a non-integer ceilf / floorf; 1 x 2 and 2 x 1: a transposition shows; 64, the largest accepted width, on 9 x 5: a whole-image window"""
    return [wd for wd in K.WIDTHS if wd[0] < 64 or size == (9, 5)]


def _image(gpu, px):
    h, w = px.shape[:2]
    img = gpu.Image(w, h)
    img.setPixelData(px)
    return img


def _plane(gpu, img, f, process=None, splat_scale=K.SPLAT_SCALE):
    out = img.applyImagePipeline(splat_scale, None if f is None else K.api_filter(gpu.api, f), process)
    return img.getFilteredData(), out


@pytest.mark.parametrize("size", SIZES)
def test_polynomial_filters_bit_for_bit(gpu, size):
    """a. box, Mitchell, triangle: products and sums only, and the library is built without contraction, so the plane is the restatement's bit for bit"""
    px = K.plain_frame(*size)
    img = _image(gpu, px)
    for name in K.POLYNOMIAL:
        for wd in _widths(size):
            f = K.flt(name, *wd)
            K.assert_same_plane(_plane(gpu, img, f)[0], P.canonical_filter(px, K.SPLAT_SCALE, f), "%dx%d %s %gx%g" % (size + (name,) + wd))


@pytest.mark.parametrize("size", SIZES)
def test_gaussian_and_lanczos_under_the_ambiguity_rule(gpu, size):
    """b. Gaussian (alpha = 2) at every width and Lanczos (6, tau 3): expf / sinf of the device against numpy's, so tests/pipeline_cases.py "Rule 1" — a byte may
    differ by one step only where the float64 value of the same sums lies within the derived margin of an integer, at most 2 % of the channels are ambiguous (the
    frames keep that cap by themselves: tests/test_oracle_pipeline.py checks it without a GPU).  The default Gaussian, alpha = -2, weighs every tap 0 (the tap on the
    filter's edge included: exp(-alpha d^2) - exp(-alpha w^2) with d = w), every pixel is 0 / 0 and the plane is all zeros."""
    px = K.plain_frame(*size)
    img = _image(gpu, px)
    for f in [K.flt("gaussian", *wd) for wd in _widths(size)] + [K.flt("lanczos", 6.0)]:
        K.compare_filtered_with_rule(_plane(gpu, img, f)[0], P.canonical_filter(px, K.SPLAT_SCALE, f), px, K.SPLAT_SCALE, f,
                                     "%dx%d %s %gx%g" % (size + ("gaussian" if f["type"] == 2 else "lanczos", f["xw"], f["yw"])))
    d = gpu.api.gaussian_filter()
    assert (d.x_width, d.y_width, d.p0) == (2.0, 2.0, -2.0)                      # the reference's defaults
    for f in [None] + [K.flt("gaussian_default", *wd) for wd in _widths(size)]:
        got = img.applyImagePipeline(K.SPLAT_SCALE, d, None) if f is None else _plane(gpu, img, f)[1]
        plane = img.getFilteredData()
        assert (plane == 0).all(), (size, f, int((plane != 0).sum()), np.argwhere(plane != 0)[:8].tolist(), [hex(v) for v in plane[plane != 0][:8]])
        assert (got[..., :3] == 0).all() and (got[..., 3] == 255).all()


def test_edge_pixels_under_box_and_mitchell_bit_for_bit(gpu):
    """c. weight 0, negative rgb (under a positive and under a negative maximum), splat only, 1e30, below 1e-32, NaN in r and in b, +Inf, a large negative channel — salted
    into a 67 x 7 frame on a lattice that keeps their windows apart; then a frame whose whole-image box window sums to exactly 0, and a Mitchell filter (B = 3) whose only
    weight is exactly 0 (0 / 0 in every pixel)"""
    w, h = 67, 7
    px = K.salted_frame(w, h)
    img = _image(gpu, px)
    own = P.canonical_filter(px, K.SPLAT_SCALE, K.flt("box", 0.4))
    at = dict(zip([n for n, _ in K.EDGE_PIXELS], K.edge_positions(w, h)))
    word = lambda name: int(own[at[name][1], at[name][0]])
    # the restatement's own-pixel words say what each edge pixel is there to show
    assert word("weight 0 (rgb undivided)") == int(P.to_rgbe(F([0.7, 0.2, 1.3])))
    assert word("negative rgb, positive maximum") & 0xff00ff == 0 and word("negative rgb, positive maximum") >> 24 != 0
    assert word("splat only") == int(P.to_rgbe(F([0.8, 0.4, 0.2]) * F(K.SPLAT_SCALE)))
    assert word("1e30") >> 24 == 128 + 100 and word("NaN in r (finite maximum)") & 0xff == 0 and word("NaN in r (finite maximum)") >> 24 == 128
    for name in ("negative maximum", "below 1e-32", "NaN in b (NaN maximum)", "+Inf in g"):
        assert word(name) == 0, name
    for name in ("box", "mitchell"):
        for wd in K.GOLDEN_SALTED_WIDTHS:
            f = K.flt(name, *wd)
            K.assert_same_plane(_plane(gpu, img, f)[0], P.canonical_filter(px, K.SPLAT_SCALE, f), "salted %s %gx%g" % ((name,) + wd))
    zs = K.zero_sum_frame()
    img = _image(gpu, zs)
    for f in (K.flt("box", 0.4), K.flt("box", 64.0), K.flt("mitchell", 2.0)):
        want = P.canonical_filter(zs, 0.0, f)
        K.assert_same_plane(_plane(gpu, img, f, splat_scale=0.0)[0], want, "zero-sum frame %s" % f)
    assert (P.canonical_filter(zs, 0.0, K.flt("box", 64.0)) == 0).all()
    px = K.plain_frame(9, 5)
    plane = _plane(gpu, _image(gpu, px), K.flt("mitchell_b3", 0.4))[0]
    assert (plane == 0).all() and (P.canonical_filter(px, K.SPLAT_SCALE, K.flt("mitchell_b3", 0.4)) == 0).all()


@pytest.mark.parametrize("frame", ["plain 9x5", "salted 67x7"])
def test_no_filter_copies_the_samples_to_the_filtered_plane(gpu, frame):
    """d. with a post-process and no filter, k_to_filtered is to_rgbe(to_spectrum), bit for bit — edge pixels included"""
    px = K.plain_frame(9, 5) if frame == "plain 9x5" else K.salted_frame(67, 7)
    plane, _ = _plane(gpu, _image(gpu, px), None, gpu.api.tonemap())
    K.assert_same_plane(plane, P.to_rgbe(P.to_spectrum(px, K.SPLAT_SCALE)), frame)


def _luminance_checks(info, plane, what):
    """f. the accessor's (min, max, avg, logAvg) against the plane they were computed from.
    min and max: exact (comparisons only).
    avg = fl(S' / n), S' an fp32 sum of the n luminances in some order (per lane, per wave, then atomics): |S' - S| <= g sum |Y_i|, g = (n - 1) U / (1 - (n - 1) U), the
    standard bound for any order of summation; the quotient adds one rounding.
    logAvg = expf(fl(T' / n)), T' such a sum of t_i = logf(fl(2.3e-5 + Y_i)): the inner sum's rounding moves the logarithm by at most U (d log x = dx / x), the device's
    logf by at most 4 ulp <= 2^-21 |t_i| (measured 1.88 ulp, doubled: tools/pipeline_math_probe.hip, RESULTS.md), so |t'_i - t_i| <= U + 8 U |t_i|; then the summation bound, one rounding for the quotient,
    and the host's expf (1 ulp): |logAvg - exp(q)| <= exp(q) (expm1(dq) + 2 U)."""
    Y = P.luminance(P.from_rgbe(plane)).ravel()
    n = Y.size
    g = (n - 1) * U / (1 - (n - 1) * U)
    assert info.dtype == np.float32 and info[0].view(np.uint32) == Y.min().view(np.uint32) and info[1].view(np.uint32) == max(Y.max(), F(0)).view(np.uint32), (what, info, Y.min(), Y.max())
    Y64 = Y.astype(np.float64)
    avg = Y64.sum() / n
    d_avg = g * np.abs(Y64).sum() / n + U * (abs(avg) + g * np.abs(Y64).sum() / n)
    t = np.log((F(2.3e-5) + Y).astype(np.float64))
    q = t.sum() / n
    d_q = (g * np.abs(t).sum() + (U + 8 * U * np.abs(t)).sum() * (1 + g)) / n
    d_q += U * (abs(q) + d_q)
    d_log = np.exp(q) * (np.expm1(d_q) + 2 * U)
    print("%s: n = %d, avg off by %.3g (bound %.3g), logAvg off by %.3g (bound %.3g)" % (what, n, abs(info[2] - avg), d_avg, abs(info[3] - np.exp(q)), d_log))
    assert abs(info[2] - avg) <= d_avg and abs(info[3] - np.exp(q)) <= d_log, (what, info, avg, d_avg, np.exp(q), d_log)


def _tonemap_checks(gpu, img, plane, got, key, burn, what):
    """the display image recomputed from the plane with the scale and white point the call itself used (built from the accessor's max and logAvg as
    ToneMapPostProcess::Apply builds them): Reinhard05Kernel is products, sums and quotients — its RGBCOL is the restatement's — and the gamma pass over it is held
    under tests/pipeline_cases.py "Rule 2" """
    info = img.getLuminanceInfo()
    _luminance_checks(info, plane, what)
    scale, inv_wp2 = P.tonemap_params(key, burn, info[1], info[3])
    mapped = P.reinhard_pixels(plane, scale, inv_wp2)
    assert np.array_equal(np.asarray(mapped)[..., 3], np.full(plane.shape, 255, np.uint8))
    K.compare_display_with_rule(got, P.from_rgbcol(mapped), what)
    return mapped


@pytest.mark.parametrize("settings", [(0.18, 0.0), (0.3, 0.2), (0.18, 1.0)])   # the defaults; a key and a burn; burn = 1: the 1e-8 clamp
@pytest.mark.parametrize("size", [(9, 5), (67, 7)])
def test_tonemap_after_a_filter(gpu, size, settings):
    """f. filter and post-process together: the plane is the filter's, the luminance info is the plane's, the display image follows from both"""
    key, burn = settings
    px = K.plain_frame(*size)
    img = _image(gpu, px)
    with pytest.raises(gpu.CtlError):                                            # nothing tone-mapped yet on this image
        img.getLuminanceInfo()
    f = K.flt("mitchell", 2.0)
    plane, got = _plane(gpu, img, f, gpu.api.tonemap(key, burn))
    K.assert_same_plane(plane, P.canonical_filter(px, K.SPLAT_SCALE, f), "%dx%d mitchell" % size)
    mapped = _tonemap_checks(gpu, img, plane, got, key, burn, "%dx%d key %g burn %g" % (size + settings))
    if burn < 1.0:                                                               # not a burnt-out image: the operator's curve is in the picture
        assert len(np.unique(np.asarray(mapped)[..., :3])) > 20
    before = img.getLuminanceInfo()
    img.applyImagePipeline(K.SPLAT_SCALE, K.api_filter(gpu.api, K.flt("box", 1.0)), None)   # a call without a post-process leaves the stored values alone
    assert np.array_equal(img.getLuminanceInfo().view(np.uint32), before.view(np.uint32))


def test_frame_beyond_the_grid_stride_cap(gpu):
    """d / f. 2048 x 513 is 2048 pixels more than the 4096 * 256 lanes the grid-stride kernels launch: the last row is the second iteration of k_to_filtered,
    k_luminance_info, k_reinhard and k_gamma_in_place.  The frame's brightest and darkest pixel lie in that row, so a kernel that stops after one iteration shows in the
    plane, in min / max (exact) and in the display image."""
    w, h = 2048, 513
    px = K.plain_frame(w, h)
    px[h - 1, 5, :3] = (900.0, 800.0, 700.0); px[h - 1, 5, 3:] = (0, 0, 0, 1)
    px[h - 1, 9] = (2.0 ** -14, 2.0 ** -15, 2.0 ** -16, 0, 0, 0, 1)
    img = _image(gpu, px)
    plane, got = _plane(gpu, img, None, gpu.api.tonemap(0.18, 0.0))
    want = P.to_rgbe(P.to_spectrum(px, K.SPLAT_SCALE))
    K.assert_same_plane(plane, want, "2048x513 no filter")
    Y = P.luminance(P.from_rgbe(want))
    assert np.unravel_index(Y.argmax(), Y.shape) == (h - 1, 5) and np.unravel_index(Y.argmin(), Y.shape) == (h - 1, 9)
    _tonemap_checks(gpu, img, plane, got, 0.18, 0.0, "2048x513 key 0.18 burn 0")
    for key, burn in ((0.3, 0.2), (0.18, 1.0)):
        plane2, got = _plane(gpu, img, None, gpu.api.tonemap(key, burn))
        assert np.array_equal(plane2, plane)
        _tonemap_checks(gpu, img, plane, got, key, burn, "2048x513 key %g burn %g" % (key, burn))
    got = img.applyImagePipeline(K.SPLAT_SCALE, None, None)                      # the direct path at this size: k_apply_pipeline
    K.compare_display_with_rule(got, P.to_spectrum(px, K.SPLAT_SCALE), "2048x513 direct")


def test_output_stage_over_every_grey(gpu):
    """e. the sRGB curve and the byte conversion over every grey RGBE value <= 1 with top mantissa 128..255 across the exponents that reach a non-zero byte (1665
    values), and coloured triples with small second and third mantissas.  A box filter of width 0.4 is the identity on values RGBE represents (asserted), so
    k_filtered_to_output sees exactly these; the direct path k_apply_pipeline and getRGB (k_resolve_rgb) get the same frame.  Bytes equal the float64 evaluation's,
    but for one step where 255 srgb(v) lies within SRGB_MARGIN of an integer (tests/pipeline_cases.py "Rule 2": the device's powf, measured and doubled); at most
    1 % of the bytes may be that close."""
    for what, words in (("greys", K.grey_rgbe_words()), ("coloured", K.coloured_rgbe_words())):
        px = K.frame_of_rgbe(words, 67)
        lin = px[..., :3]
        img = _image(gpu, px)
        plane, got = _plane(gpu, img, K.flt("box", 0.4), splat_scale=0.0)
        assert np.array_equal(plane.ravel()[:len(words)], words) and (plane.ravel()[len(words):] == 0).all()
        K.compare_display_with_rule(got, lin, what + ", k_filtered_to_output")
        K.compare_display_with_rule(img.applyImagePipeline(0.0, None, None), lin, what + ", k_apply_pipeline")
        assert np.array_equal(img.getRGB(0.0).view(np.uint32), lin.view(np.uint32))
    # the direct path with weights, splats and the edge pixels: to_spectrum, bit for bit through getRGB, then the same rule
    px = K.salted_frame(67, 7)
    img = _image(gpu, px)
    lin = P.to_spectrum(px, K.SPLAT_SCALE)
    rgb = img.getRGB(K.SPLAT_SCALE)
    assert np.array_equal(rgb.view(np.uint32)[~np.isnan(lin)], lin.view(np.uint32)[~np.isnan(lin)]) and np.array_equal(np.isnan(rgb), np.isnan(lin))
    K.compare_display_with_rule(img.applyImagePipeline(K.SPLAT_SCALE, None, None), lin, "salted 67x7, k_apply_pipeline")
