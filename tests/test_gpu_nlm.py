"""The NonLocalMeans filter and the per-pixel variance switch on the GPU against the numpy restatement (tests/nlm_ref.py): the filtered RGBE plane and the
variance bit for bit, the display image under the canonical filters' bound, the switch's neutrality, the refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nlm_ref as N   # noqa: E402
from cudatracerlib_amd import scenes   # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def _filtered(gpu, px, splat_scale, variance, flt, **kw):
    h, w = px.shape[:2]
    img = gpu.Image(w, h)
    img.setPixelData(px)
    img.applyImagePipeline(splat_scale, flt, None, variance=variance, **kw)
    return img.getFilteredData()


def _assert_same_plane(got, want, what):
    bad = got != want
    print("%s: %d of %d pixels differ" % (what, int(bad.sum()), bad.size))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:8].tolist(), [hex(v) for v in got[bad][:8]], [hex(v) for v in want[bad][:8]])


@pytest.mark.parametrize("settings", [(0.45, 0.005), (1.0, 0.02)])
@pytest.mark.parametrize("size", [(9, 5), (61, 45), (200, 37), (211, 203)])   # no multiple of the tile; one crosses 200, the reference's launch-block seam
def test_filtered_plane_equals_the_restatement_bit_for_bit(gpu, size, settings):
    w, h = size
    k, s2 = settings
    _, px, variance, splat_scale = N.synthetic_frame(w, h, sigma2_scale=0.005)
    want, weights = N.nlm_filter(px, splat_scale, variance, k, s2, return_weights=True)
    if size == (61, 45) and settings == (0.45, 0.005):   # not a degenerate input: all three classes of weight are well represented
        zero, one = (weights == 0).mean(), (weights == 1).mean()
        print("weights: %.3f zero, %.3f one, %.3f between" % (zero, one, 1 - zero - one))
        assert zero >= 0.10 and one >= 0.10 and ((weights > 0) & (weights < 1)).mean() >= 0.10
    got = _filtered(gpu, px, splat_scale, variance, gpu.api.nlm_filter(k, s2))
    _assert_same_plane(got, want, "%dx%d k=%g sigma2_scale=%g" % (w, h, k, s2))


def test_filtered_plane_with_nan_negative_and_overflowing_variances(gpu):
    w, h = 61, 45
    _, px, variance, splat_scale = N.synthetic_frame(w, h)
    rng = np.random.default_rng(21)
    salt = rng.integers(0, 40, (h, w))
    variance = variance.copy()
    variance[salt == 0] = np.nan; variance[salt == 1] = -3.0; variance[salt == 2] = 7e4; variance[salt == 3] = np.inf; variance[salt == 4] = 65520.0
    want = N.nlm_filter(px, splat_scale, variance)
    got = _filtered(gpu, px, splat_scale, variance, gpu.api.nlm_filter())
    _assert_same_plane(got, want, "salted variance")


def test_display_image_with_and_without_tonemap(gpu):
    """the pipeline's tail after the filter is the canonical filters' tail: same bound as tests/test_gpu_render.py::test_image_pipeline_filters_and_tonemap
    (powf and the atomic log-average may differ in the last ulp: at most 2 steps, at most 3 % of the pixels)"""
    from oracle import pipeline as P
    w, h = 61, 45
    _, px, variance, splat_scale = N.synthetic_frame(w, h)
    plane = N.nlm_filter(px, splat_scale, variance)
    img = gpu.Image(w, h); img.setPixelData(px)
    api = gpu.api
    for proc in (None, api.tonemap(), api.tonemap(0.3, 0.2)):
        got = img.applyImagePipeline(splat_scale, api.nlm_filter(), proc, variance=variance)
        want = P.gamma_correct(P.from_rgbe(plane)) if proc is None else P.gamma_correct(P.from_rgbcol(P.reinhard(plane, proc.key, proc.burn)))
        d = np.abs(got.astype(int) - want.astype(int))
        print("tonemap %s: max step %d, share differing %.4f" % (proc is not None, d.max(), (d > 0).mean()))
        assert d.max() <= 2 and (d > 0).mean() <= 0.03, (proc is not None, d.max(), (d > 0).mean())
        assert np.array_equal(img.getFilteredData(), plane)
    # getFilteredData serves the canonical filters too
    img.applyImagePipeline(splat_scale, api.box_filter(1.0, 1.0), None)
    assert np.array_equal(img.getFilteredData(), P.canonical_filter(px, splat_scale, dict(type=1, xw=1.0, yw=1.0, p0=0.0, p1=0.0)))


def _tracer(gpu, scene, w, h, cls=None):
    tr = (cls or gpu.WavefrontPathTracer)()
    tr.getParameters().setValue("MaxPathLength", 4)
    tr.Resize(w, h); tr.InitializeScene(scene)
    return tr


@pytest.mark.parametrize("ordered", [True, False, "megakernel"])
def test_pixel_variance_equals_the_restated_moments(gpu, ordered):
    """ordered: the moments are updated inside the batch resolve of the ordered accumulation; without it, and in the PathTracer (megakernel) plugin, the passes are rendered one
    per launch and the update kernel runs after each (the frame's atomics may then order a pixel's rare second sample of a pass either way, so only the variance is compared
    with the frames it came from)"""
    w, h = 48, 40
    sc = scenes.cornell_box(w, h, glass_sphere=True)   # (owns the host arrays the description points to)
    scene = gpu.Scene(sc.desc, flatten=True) if ordered == "megakernel" else gpu.Scene(sc.desc)
    tr = _tracer(gpu, scene, w, h, gpu.PathTracer if ordered == "megakernel" else None); tr.setPixelVariance(True)
    if ordered != "megakernel":
        tr.getParameters().setValue("OrderedAccumulation", ordered)
    assert np.isnan(tr.getPixelVariance()).all()                   # Var(0)
    img = gpu.Image(w, h)
    pv = N.PixelVariance(h, w)
    for k in range(6):
        tr.DoPass(img, new_trace=(k == 0))
        frame = img.getPixelData()
        pv.update_moments(frame, 1.0 / (k + 1))
        got, want = tr.getPixelVariance(), pv.compute_variance()
        assert got.shape == (h, w)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert (want[np.isfinite(want)] > 0).mean() > 0.5              # a rendered frame: most pixels have a positive variance
    frame6, var6 = frame, got
    if ordered is True:   # the same 6 passes in one call (one batch): same frame, same variance
        tr2 = _tracer(gpu, scene, w, h); tr2.setPixelVariance(True)
        img2 = gpu.Image(w, h)
        tr2.DoPasses(img2, 6, new_trace=True)
        assert np.array_equal(img2.getPixelData(), frame6)
        assert np.array_equal(tr2.getPixelVariance().view(np.uint32), var6.view(np.uint32))
    # a new trace clears the buffer (PixelVarianceBuffer::Clear)
    tr.DoPass(img, new_trace=True)
    pv1 = N.PixelVariance(h, w); pv1.update_moments(img.getPixelData(), 1.0)
    assert np.array_equal(tr.getPixelVariance().view(np.uint32), pv1.compute_variance().view(np.uint32))


def test_a_batch_equals_its_passes_where_samples_stray_into_the_next_pixel(gpu):
    """pixel + jitter rounds into the NEXT pixel where the jitter is within an ulp of 1: from x = 1024 on about 6 in 10^5 samples (ulp 2^-13), ~12 of the 196 608 samples that
    6 passes put there.  Such a sample is a second sample of its landing pixel in that pass and none of its own; inside a batch it must count for ITS pass, in the frame and in the
    moments: DoPasses(6) as one batch gives the frame and the variance of six single passes, bit for bit, and the variance is the restated one"""
    w, h = 2048, 32
    sc = scenes.cornell_box(w, h, glass_sphere=True)
    scene = gpu.Scene(sc.desc)
    tr = _tracer(gpu, scene, w, h); tr.setPixelVariance(True)
    img = gpu.Image(w, h)
    pv = N.PixelVariance(h, w)
    for k in range(6):
        tr.DoPass(img, new_trace=(k == 0))
        pv.update_moments(img.getPixelData(), 1.0 / (k + 1))
    frame, var = img.getPixelData(), tr.getPixelVariance()
    strayed = int((frame[..., 6] != 6).sum())
    print("pixels whose sample count is not the pass count: %d" % strayed)
    assert strayed >= 2                                             # the case is present (a stray sample leaves one pixel short and one over)
    assert np.array_equal(var.view(np.uint32), pv.compute_variance().view(np.uint32))
    tr2 = _tracer(gpu, scene, w, h); tr2.setPixelVariance(True)
    img2 = gpu.Image(w, h)
    tr2.DoPasses(img2, 6, new_trace=True)
    assert tr2.getParameters().getValue("PassBatch") == 0           # (the default: six passes of 65 536 pixels are one batch)
    assert np.array_equal(img2.getPixelData(), frame)
    got = tr2.getPixelVariance()
    assert np.array_equal(got.view(np.uint32), var.view(np.uint32)), int((got.view(np.uint32) != var.view(np.uint32)).sum())


def test_reading_the_block_counts_keeps_the_variance(gpu):
    """ctl_tracer_get_block_counts / setBlockWeight create the (Uniform) block sampler outside a render: the variance the filter is about to use stays"""
    w, h = 48, 40
    sc = scenes.cornell_box(w, h)
    scene = gpu.Scene(sc.desc)
    tr = _tracer(gpu, scene, w, h); tr.setPixelVariance(True)
    img = gpu.Image(w, h)
    tr.DoPasses(img, 4, new_trace=True)
    before = tr.getPixelVariance()
    assert np.isfinite(before).all()
    assert (tr.getBlockCounts(w, h) == 1).all()
    tr.setBlockWeight(0, 0, 1.0)
    assert np.array_equal(tr.getPixelVariance().view(np.uint32), before.view(np.uint32))


def test_the_switch_changes_no_frame(gpu):
    w, h = 48, 40
    sc = scenes.cornell_box(w, h, glass_sphere=True)   # (owns the host arrays the description points to)
    scene = gpu.Scene(sc.desc)
    frames = {}
    for name in ("untouched", "on_then_off", "fresh", "on"):
        tr = _tracer(gpu, scene, w, h)
        if name == "on_then_off":
            tr.setPixelVariance(True); tr.setPixelVariance(False)
        if name == "on":
            tr.setPixelVariance(True)
        img = gpu.Image(w, h)
        tr.DoPasses(img, 6, new_trace=True)
        frames[name] = img.getPixelData()
        if name == "on_then_off":
            with pytest.raises(gpu.CtlError):                      # nothing is kept once it is off
                tr.getPixelVariance()
    assert np.array_equal(frames["untouched"], frames["fresh"])
    assert np.array_equal(frames["untouched"], frames["on_then_off"])
    # updating the moments inside the batch changes no sum.  (No sample strays into a neighbouring pixel at this width; where one does, the switch-on frame is that of the passes
    # rendered one at a time — the test above — and the switch-off batch may differ from both in that pixel by a rounding, as it did before the switch existed)
    assert np.array_equal(frames["untouched"], frames["on"])


def test_end_to_end_through_the_tracer_handle(gpu):
    w, h = 48, 40
    sc = scenes.cornell_box(w, h, glass_sphere=True)   # (owns the host arrays the description points to)
    scene = gpu.Scene(sc.desc)
    tr = _tracer(gpu, scene, w, h); tr.setPixelVariance(True)
    img = gpu.Image(w, h)
    tr.DoPasses(img, 8, new_trace=True)
    variance = tr.getPixelVariance()
    frame = img.getPixelData()
    cached = N.copy_to_cached(frame, 1.0 / 8)
    # the reference's defaults, and a sigma2Scale of the order of 1 / passes: at 8 passes the frame's own noise is ~ variance / 8, far above 0.005 * variance, so the
    # defaults leave such an early frame as it is (every weight but the pixel's own is cut off); the second setting is where the filter acts on it
    for k, s2 in ((0.45, 0.005), (0.45, 0.25)):
        flt = gpu.api.nlm_filter(k, s2)
        img.applyImagePipeline(1.0 / 8, flt, None, tracer=tr)
        by_handle = img.getFilteredData()
        img.applyImagePipeline(1.0 / 8, flt, None, variance=variance)
        by_array = img.getFilteredData()
        assert np.array_equal(by_handle, by_array)
        _assert_same_plane(by_handle, N.nlm_filter(frame, 1.0 / 8, variance, k, s2), "cornell box, 8 passes, sigma2_scale=%g" % s2)
        print("sigma2_scale=%g: %.3f of the pixels changed by the filter" % (s2, (by_handle != cached).mean()))
    assert (by_handle != cached).mean() > 0.25
    assert img.lastFilterMs() > 0


def test_refusals(gpu):
    w, h = 48, 40
    sc = scenes.cornell_box(w, h)
    scene = gpu.Scene(sc.desc)
    flt = gpu.api.nlm_filter()
    img = gpu.Image(w, h)
    # a tile shard has no whole frame
    tr = _tracer(gpu, scene, w, h); tr.setTileShard(0, 2)
    with pytest.raises(gpu.CtlError) as e:
        tr.setPixelVariance(True)
    assert e.value.code == -1
    tr = _tracer(gpu, scene, w, h); tr.setPixelVariance(True); tr.setTileShard(0, 2)
    with pytest.raises(gpu.CtlError) as e:
        tr.DoPass(img, new_trace=True)
    assert e.value.code == -1
    # Tracer<false>: one sample per pixel, no variance
    prim = gpu.PrimTracer()
    with pytest.raises(gpu.CtlError) as e:
        prim.setPixelVariance(True)
    assert e.value.code == -5
    # tracer and image of different sizes; a tracer whose switch is off
    tr = _tracer(gpu, scene, w, h); tr.setPixelVariance(True)
    tr.DoPass(img, new_trace=True)
    small = gpu.Image(40, 32)
    with pytest.raises(gpu.CtlError) as e:
        small.applyImagePipeline(1.0, flt, None, tracer=tr)
    assert e.value.code == -1 and "size" in str(e.value)
    tr.setPixelVariance(False)
    with pytest.raises(gpu.CtlError) as e:
        img.applyImagePipeline(1.0, flt, None, tracer=tr)
    assert e.value.code == -1 and "variance" in str(e.value)
    # both sources, neither, a negative setting
    tr.setPixelVariance(True)
    v = np.zeros((h, w), F)
    for kw in (dict(tracer=tr, variance=v), dict()):
        with pytest.raises(gpu.CtlError) as e:
            img.applyImagePipeline(1.0, flt, None, **kw)
        assert e.value.code == -1
    with pytest.raises(gpu.CtlError) as e:
        img.applyImagePipeline(1.0, gpu.api.nlm_filter(-1.0, 0.005), None, variance=v)
    assert e.value.code == -1
    with pytest.raises(gpu.CtlError):                              # nothing filtered yet on a new image
        gpu.Image(8, 8).getFilteredData()
