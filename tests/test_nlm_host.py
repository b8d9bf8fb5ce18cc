"""The NonLocalMeans filter without a GPU: closed forms of the numpy restatement (tests/nlm_ref.py) that the GPU tests compare the kernel with, a denoising
property, and the argument checks of the C entry point."""
import ctypes as C

import numpy as np
import pytest

import nlm_ref as N
from oracle.pipeline import to_rgbe, from_rgbe

F = np.float32


def _frame(col):
    """PixelData with weightSum 1 and no splat term: toSpectrum gives `col` back"""
    px = np.zeros(col.shape[:2] + (7,), F)
    px[..., 0:3] = col; px[..., 6] = 1
    return px


def _window_mean(col):
    """sum over the 13 x 13 window clipped at the borders (xo outer, yo inner), times the reciprocal of the count: what all-ones weights give"""
    h, w = col.shape[:2]
    acc = np.zeros((h, w, 3), F); cnt = np.zeros((h, w), F)
    ys, xs = np.mgrid[0:h, 0:w]
    for xo in range(-N.R, N.R + 1):
        for yo in range(-N.R, N.R + 1):
            ok = (xs + xo >= 0) & (xs + xo < w) & (ys + yo >= 0) & (ys + yo < h)
            src = col[np.clip(ys + yo, 0, h - 1), np.clip(xs + xo, 0, w - 1)]
            acc = np.where(ok[..., None], acc + src, acc).astype(F); cnt = np.where(ok, cnt + F(1), cnt).astype(F)
    return (acc * (F(1) / cnt)[..., None]).astype(F)


def _all_weights(col, var, **kw):
    return np.concatenate([we[inside] for _, _, inside, we in N.nlm_weights(col, var, **kw)])


def test_half_round_trip_is_round_to_nearest_even_with_overflow():
    v = np.array([0.0, 1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0, 65519.9, 65520.0, 1e9, -2.5, 6e-8, 1e-9, np.nan, np.inf], F)
    got = N.half_round_trip(v)
    want = np.array([0.0, 1.0, 1.0, 1.0 + 2.0 ** -9, 65504.0, 65504.0, np.inf, np.inf, -2.5, 2.0 ** -24, 0.0, np.nan, np.inf], F)
    assert np.array_equal(got, want, equal_nan=True)


def test_constant_image_is_its_own_rgbe_round_trip():
    col = np.broadcast_to(np.array([0.31, 0.62, 0.17], F), (20, 23, 3)).copy()
    for var in (0.0, 0.7, 300.0):
        got = N.nlm_filter(_frame(col), 0.0, np.full((20, 23), var, F))
        assert np.array_equal(got, to_rgbe(col)), var


def test_zero_variance_and_distinct_colours_is_the_identity():
    rng = np.random.default_rng(3)
    col = rng.uniform(0.1, 1.0, (17, 19, 3)).astype(F)
    px = _frame(col)
    cached = N.copy_to_cached(px, 0.0)
    plane, weights = N.nlm_filter(px, 0.0, np.zeros((17, 19), F), return_weights=True)
    assert np.array_equal(plane, cached)                       # RGBE of a decoded RGBE value is that value
    assert (weights == 1).sum() == 17 * 19 and (weights == 0).sum() == weights.size - 17 * 19   # every weight but the pixel's own is 0


@pytest.mark.parametrize("shape", [(21, 30), (5, 9)])   # the second is narrower than the window and lower than a patch
def test_large_variance_gives_the_clipped_window_mean(shape):
    rng = np.random.default_rng(5)
    col = from_rgbe(to_rgbe(rng.uniform(0.0, 1.0, shape + (3,)).astype(F)))
    var = np.full(shape, 1000.0, F)                            # sigma2Scale * var = 5 per pixel: u_diff <= 1 < var_p + min(var_p, var_q), every d <= 0
    assert (_all_weights(col, var) == 1).all()
    assert np.array_equal(N.nlm_filter(_frame(col), 0.0, var), to_rgbe(_window_mean(col)))


def test_nan_negative_and_overflowing_variances():
    """fminf / fmaxf and the half overflow as the reference's device evaluates them: NaN distances give max(0, NaN) = 0 and the weight 1"""
    rng = np.random.default_rng(9)
    col = rng.uniform(0.1, 1.0, (15, 16, 3)).astype(F)
    # above 65504 the half is inf: d = (u - inf) / (eps + k^2 inf) = NaN -> weight 1
    assert (_all_weights(col, np.full((15, 16), 1e5, F)) == 1).all()
    # NaN variance: NaN terms, NaN distance -> weight 1
    assert (_all_weights(col, np.full((15, 16), np.nan, F)) == 1).all()
    # negative variance: positive numerator over a negative denominator, d < 0 -> weight 1
    assert (_all_weights(col, np.full((15, 16), -40.0, F)) == 1).all()
    # one overflowing pixel in a frame of zero variance.  As p + d its term is (u - (inf + min(inf, 0))) / (eps + k^2 inf) = -inf / inf = NaN: the pairs whose OWN patch
    # contains it weigh 1.  As q + d the term is (u - (0 + min(0, inf))) / inf = 0, a finite term among huge ones: those pairs stay 0, as all others but the pixel's own
    var = np.zeros((15, 16), F); var[7, 8] = 7e4
    ys, xs = np.mgrid[0:15, 0:16]
    for xo, yo, inside, we in N.nlm_weights(col, var):
        touched = np.zeros((15, 16), bool)
        for dx in range(-N.FP, N.FP + 1):
            for dy in range(-N.FP, N.FP + 1):
                px_, py_, qx_, qy_ = xs + dx, ys + dy, xs + dx + xo, ys + dy + yo
                valid = (px_ >= 0) & (px_ < 16) & (py_ >= 0) & (py_ < 15) & (qx_ >= 0) & (qx_ < 16) & (qy_ >= 0) & (qy_ < 15)
                touched |= valid & (px_ == 8) & (py_ == 7)
        want = np.where(touched | ((xo == 0) & (yo == 0)), F(1), F(0))
        assert np.array_equal(we[inside], want[inside]), (xo, yo)
    # and the filter still returns finite colours for all of it
    for v in (np.full((15, 16), 1e5, F), np.full((15, 16), np.nan, F), var):
        assert np.isfinite(from_rgbe(N.nlm_filter(_frame(col), 0.0, v))).all()


def test_the_filter_denoises_a_synthetic_frame():
    clean, px, variance, splat_scale = N.synthetic_frame(61, 45)
    before = from_rgbe(N.copy_to_cached(px, splat_scale))
    plane, weights = N.nlm_filter(px, splat_scale, variance, return_weights=True)
    after = from_rgbe(plane)
    mse_before, mse_after = float(np.mean((before - clean) ** 2)), float(np.mean((after - clean) ** 2))
    print("mse before %.3e after %.3e; weights 0: %.3f 1: %.3f between: %.3f" % (mse_before, mse_after, (weights == 0).mean(), (weights == 1).mean(), ((weights > 0) & (weights < 1)).mean()))
    assert mse_after < mse_before
    # the frame the GPU parity test uses exercises all three classes of weight
    assert (weights == 0).mean() >= 0.10 and (weights == 1).mean() >= 0.10 and ((weights > 0) & (weights < 1)).mean() >= 0.10


def test_moments_restate_var_accumulator():
    rng = np.random.default_rng(11)
    pv = N.PixelVariance(4, 5)
    assert np.isnan(pv.compute_variance()).all()               # Var(0): 0 * inf
    acc = np.zeros((4, 5, 7), F); lums = []
    for k in range(6):
        e = rng.uniform(0, 1, (4, 5, 3)).astype(F)
        acc[..., 0:3] += e; acc[..., 6] += 1
        pv.update_moments(acc, 1.0 / (k + 1))
        lums.append(e @ np.array([0.212671, 0.715160, 0.072169]))
    assert np.allclose(pv.compute_variance(), np.var(np.stack(lums), axis=0), rtol=2e-3, atol=1e-5)   # population variance of the pass estimates' luminance


def test_new_symbols_are_exported(ctl):
    for name in ("ctl_image_apply_pipeline_nlm", "ctl_image_read_filtered", "ctl_image_last_filter_ms", "ctl_tracer_set_pixel_variance", "ctl_tracer_read_pixel_variance"):
        assert getattr(ctl.lib, name) is not None
    header = open(__import__("os").path.join(__import__("os").path.dirname(ctl.__file__), "..", "include", "ctl_amd.h")).read()
    assert "not part of this build" not in header
    flt = ctl.api.nlm_filter()
    assert abs(flt.k - 0.45) < 1e-7 and abs(flt.sigma2_scale - 0.005) < 1e-9   # NonLocalMeansFilter.h:103-113


def test_entry_point_checks_its_arguments_before_the_device(ctl):
    """every argument error that can be judged without the handles is CTL_ERR_INVALID with a message, with or without a device; a call whose arguments are in order
    then needs a device.  Where there is none no image or tracer can exist, so the handles are stand-ins that the entry point must not touch before the device check."""
    lib, api = ctl.lib, ctl.api
    out = np.zeros(4, np.uint32); var = np.zeros(4, F)
    stand_in = C.create_string_buffer(64)
    img, tr = C.cast(stand_in, C.c_void_p), C.cast(stand_in, C.c_void_p)
    o, v = out.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p)
    ok = api.nlm_filter()

    def call(img_, nlm, tracer, variance, out_):
        return lib.ctl_image_apply_pipeline_nlm(img_, C.c_float(0.25), None if nlm is None else C.byref(nlm), tracer, variance, None, out_)
    bad = [(None, ok, None, v, o), (img, None, None, v, o), (img, ok, None, v, None),        # null image / settings / output
           (img, ok, None, None, o), (img, ok, tr, v, o),                                      # neither source of variance, both
           (img, api.nlm_filter(-0.1, 0.005), None, v, o), (img, api.nlm_filter(0.45, -1.0), None, v, o),
           (img, api.nlm_filter(float("nan"), 0.005), None, v, o), (img, api.nlm_filter(0.45, float("nan")), None, v, o)]
    for args in bad:
        assert call(*args) == -1, args            # CTL_ERR_INVALID
        assert lib.ctl_last_error() != b""
    assert lib.ctl_image_read_filtered(None, o) == -1 and lib.ctl_tracer_set_pixel_variance(None, 1) == -1 and lib.ctl_tracer_read_pixel_variance(None, v) == -1


def test_entry_point_needs_a_device_once_its_arguments_are_in_order(ctl):
    if ctl.device_count() > 0:
        pytest.skip("a device is present: the stand-in handles would be used")
    lib, api = ctl.lib, ctl.api
    out = np.zeros(4, np.uint32); var = np.zeros(4, F)
    stand_in = C.create_string_buffer(64)
    img, tr = C.cast(stand_in, C.c_void_p), C.cast(stand_in, C.c_void_p)
    o, v = out.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p)
    ok = api.nlm_filter()

    def call(img_, nlm, tracer, variance, out_):
        return lib.ctl_image_apply_pipeline_nlm(img_, C.c_float(0.25), None if nlm is None else C.byref(nlm), tracer, variance, None, out_)
    assert call(img, ok, None, v, o) == -2       # CTL_ERR_NO_DEVICE
    assert b"no HIP device" in lib.ctl_last_error()
    assert call(img, api.nlm_filter(0.0, 0.0), tr, None, o) == -2
