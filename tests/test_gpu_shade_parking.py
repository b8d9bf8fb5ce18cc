"""k_shade_basic keeps the radiance, the throughput, the pixel position, the pass number and the next direction of a path vertex in LDS (one column per lane,
shade_kernel.inc CTL_SHADE_PARK) while it sets up the hit point and evaluates the BSDF and the light.  The frames against the oracle, held the way
tests/test_gpu_render.py holds them, on the smallest shapes at which the parking can go wrong:

  * 24 x 20 pixels = 480 paths: one full 256-lane workgroup and a partial one — lanes past the end of the queue exist, and take part in the barriers without parking;
  * the Cornell box with a GGX rough-conductor block and a smooth-conductor block: diffuse walls, an area light that paths hit (the emission term takes the radiance
    out of its park and puts it back), the open front through which paths leave (a miss parks without a hit point).  All regrouping keys meet in one 256-slot
    window, so a lane shades another slot than its own — and still reads its OWN column;
  * depth 8, next-event estimation on, 2 passes as one batch (two pass numbers in one queue) and as two batches of one;
  * one large single-pass frame: more vertices than the grid has lanes, so a lane's column is used again by its next iteration.  640 x 480 outgrows the grid of four
    workgroups per CU (262 144 lanes), 704 x 480 the grid of five (327 680) that the kernel runs with now;
  * both rule sets (PathSemantics): the wavefront rules have a build of their own (shade_basic_wf.hip, not parked).
"""
import numpy as np
import pytest
from cudatracerlib_amd import api, scenes

pytestmark = pytest.mark.gpu

DEPTH = 8


def assert_close(got, want, exact_min=0.98):
    """tests/test_gpu_render.py assert_close"""
    assert np.array_equal(got[..., 6], want[..., 6]), "weightSum differs"
    g, w = got[..., :3], want[..., :3]
    frac = (np.abs(g - w) <= 2e-3 * (1 + np.abs(w))).all(axis=2).mean()
    exact = (g == w).all(axis=2).mean()
    print("within tolerance %.5f, bit-equal %.5f, means %.6g / %.6g" % (frac, exact, g.mean(), w.mean()))
    assert frac >= 0.9995, frac
    assert exact >= exact_min, exact
    assert abs(g.mean() - w.mean()) <= 1e-3 * w.mean()


def _scene(w, h):
    sc = scenes.cornell_box(w, h, extra_materials=True)
    assert api.scene_desc_check(sc.desc)["features"] == 0      # the basic feature set: k_shade_basic shades it
    return sc


def _tracer(gpu, scene, w, h, wavefront, batch):
    tr = gpu.WavefrontPathTracer(); p = tr.getParameters()
    p.setValue("MaxPathLength", DEPTH); p.setValue("Direct", True); p.setValue("PassBatch", batch)
    if wavefront: p.setValue("PathSemantics", "Wavefront")
    tr.Resize(w, h); tr.InitializeScene(scene)
    return tr


@pytest.mark.parametrize("wavefront", [False, True], ids=["default_rules", "wavefront_rules"])
def test_small_frame_two_passes_batched_and_not(gpu, orc, wavefront):
    w, h = 24, 20
    sc = _scene(w, h)
    tables = orc.sequence_tables(2)      # the stream the tracer's own generator draws from (DoPasses)
    want, _ = orc.render(sc.desc, w, h, n_passes=2, tables=tables, max_path_length=DEPTH, wavefront_rules=wavefront)
    assert (want[..., :3].sum(axis=2) == 0).any() and (want[..., :3].max(axis=2) > 1.0).any()      # paths that leave through the opening; pixels that see the light
    scene = gpu.Scene(sc.desc)
    frames = []
    for batch in (2, 1):
        tr = _tracer(gpu, scene, w, h, wavefront, batch)
        img = gpu.Image(w, h)
        tr.DoPasses(img, 2, new_trace=True)
        got = img.getPixelData()
        assert_close(got, want)
        frames.append(got)
    assert np.array_equal(frames[0].view(np.uint32), frames[1].view(np.uint32))      # ordered accumulation: the frame does not depend on the batching
    # the same two passes one by one, with the tables handed over
    tr = _tracer(gpu, scene, w, h, wavefront, 1)
    img = gpu.Image(w, h)
    for k in range(2):
        tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == 0))
    assert np.array_equal(img.getPixelData().view(np.uint32), frames[0].view(np.uint32))


@pytest.mark.parametrize("wavefront", [False, True], ids=["default_rules", "wavefront_rules"])
@pytest.mark.parametrize("size", [(640, 480), (704, 480)], ids=["640x480", "704x480"])
def test_a_lane_parks_again_in_its_next_iteration(gpu, orc, size, wavefront):
    w, h = size
    sc = _scene(w, h)
    tables = orc.sequence_tables(1)
    want, _ = orc.render(sc.desc, w, h, n_passes=1, tables=tables, max_path_length=DEPTH, wavefront_rules=wavefront)
    tr = _tracer(gpu, gpu.Scene(sc.desc), w, h, wavefront, 1)
    img = gpu.Image(w, h)
    tr.setSamplerTables(*tables[0]); tr.DoPass(img, new_trace=True)
    assert_close(img.getPixelData(), want)
