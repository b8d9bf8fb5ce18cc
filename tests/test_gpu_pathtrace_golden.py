"""Both GPU path tracers against the reference's OWN PathTrace (tests/golden/pathtrace.npz: PathTrace<DIRECT> / PathTraceRegularization<DIRECT> and the per-pixel body of
pathKernel2, Integrators/PathTracer.cu:10-170, 186-193, built from the reference's sources and run on the host with glibc — tests/test_oracle_pathtrace.py pins the oracle
on the same fixture bit for bit).

Every case of the fixture is rendered with the recorded sampler tables by the WavefrontPathTracer plugin (default, PathTrace rules; AlphaTest on where the case tests
alpha; not for the regularized cases, which only the PathTracer plugin has) and by the megakernel PathTracer plugin, and each frame is held to the FIXTURE:
  * weightSum equal in every pixel,
  * >= 99 % of pixels within 2e-3 * (1 + |ref|) in every channel of the accumulated radiance,
  * the frame mean within 2e-3 relative,
  * and the GPU is no further from the reference than the shared-math oracle (oracle/liboracle_sm.so, the checker of tests/test_gpu_render.py, rendered on the host in
    the plugin's own mode): the GPU's count of pixels outside the tolerance exceeds the shared-math oracle's by at most 0.05 % of the frame.
The bars are looser than test_gpu_render.py's (>= 99.95 % within tolerance, 98 % bit-equal): there both sides run csrc/ctl_fmath.h; here the reference runs glibc's
transcendental functions, <= 1 ulp per call away (tests/test_fmath.py), and the host branch of half::ToFloat for the triangles' normals — last-bit differences that a
discrete decision along the path (roulette, a refraction's choice, a shadow ray grazing an edge) turns into a different path in a few pixels.  The wavefront plugin
does no first-hit texture filtering (the reference's PathTrace does); the shared-math oracle it is compared with runs in the same mode.
Reads nothing but the fixture and the product's host code."""
import os
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generate():
    sys.path.insert(0, G)
    import generate
    return generate


# PathTraceRegularization is the PathTracer plugin's alone (Regularization = true): the wavefront plugin renders the other cases
CASES = [(c[0], plugin) for c in _generate().pathtrace_cases() for plugin in ("WavefrontPathTracer", "PathTracer") if not (c[6] and plugin == "WavefrontPathTracer")]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "pathtrace.npz"))


@pytest.fixture(scope="module")
def orc_sm():
    return oracle.Oracle(shared_math=True)


def _outside(img, rgb):
    return (np.abs(img[..., :3] - rgb) > 2e-3 * (1 + np.abs(rgb))).any(axis=2)


@pytest.mark.parametrize("key,plugin", CASES)
def test_gpu_path_tracers_against_the_references_own_path_trace(gpu, golden, orc_sm, key, plugin):
    generate = _generate()
    _, make, w, h, spp, direct, regu, alpha = next(c for c in generate.pathtrace_cases() if c[0] == key)
    sc = make()
    tables = generate.pathtrace_tables(spp)
    assert generate.pathtrace_input_digest(sc.desc, tables) == str(golden[key + "_digest"]), "regenerate tests/golden/pathtrace.npz"
    mega = plugin == "PathTracer"
    tr = getattr(gpu, plugin)()
    p = tr.getParameters()
    p.setValue("Direct", direct); p.setValue("MaxPathLength", 8); p.setValue("RRStartDepth", 5)
    if regu:
        p.setValue("Regularization", True)
    if alpha and not mega:
        p.setValue("AlphaTest", True)   # the megakernel plugin always alpha-tests (TraceHelper.cu:135-154, 179)
    tr.Resize(w, h); tr.InitializeScene(gpu.Scene(sc.desc, flatten=mega))
    img = gpu.Image(w, h)
    for k in range(spp):
        tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == 0))
    got = img.getPixelData()
    rgb, weight = golden[key + "_rgb"], golden[key + "_weight"]
    sm, _ = orc_sm.render(sc.desc, w, h, n_passes=spp, tables=tables, direct=direct, regularization=regu, alpha_test=alpha, partials=mega)
    out_gpu, out_sm = _outside(got, rgb), _outside(sm, rgb)
    frac = 1.0 - out_gpu.mean()
    print("%s %s: within tolerance GPU %.4f, shared-math oracle %.4f" % (key, plugin, frac, 1.0 - out_sm.mean()))
    assert out_gpu.sum() <= out_sm.sum() + 5e-4 * w * h, (out_gpu.sum(), out_sm.sum())
    assert np.array_equal(got[..., 6], weight), "weightSum differs in %d pixels" % (got[..., 6] != weight).sum()
    assert frac >= 0.99, frac
    assert abs(got[..., :3].mean() - rgb.mean()) <= 2e-3 * rgb.mean()
