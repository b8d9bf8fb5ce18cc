"""Participating media on the device against the reference's OWN code: the PathTracer plugin's frames against tests/golden/pathtrace_media.npz (PathTrace<DIRECT> with a
bound volume aggregate, built from the reference's sources and run on the host with glibc — tests/test_oracle_volume.py pins the restatement tests/volume_ref.py on the
same fixture bit for bit), and ctl_volume_eval(on_device = 1) against tests/golden/volumes.npz (the reference's own Volumes.cu / PhaseFunction.cu, row by row).

Every frame case is rendered with the recorded sampler tables and held to the FIXTURE with the bars of tests/test_gpu_pathtrace_golden.py (the two arithmetic paths are
the same: the reference runs glibc's transcendental functions and the host branch of half::ToFloat, the device csrc/ctl_fmath.h):
  * weightSum equal in every pixel,
  * >= 99 % of pixels within 2e-3 * (1 + |ref|) in every channel of the accumulated radiance,
  * the frame mean within 2e-3 relative,
  * the GPU is no further from the reference than the restatement run with the shared-math oracle (volume_ref.path_trace over the product's flattened tree, the checker
    of tests/test_gpu_volume.py): its count of pixels outside the tolerance exceeds the restatement's by at most ONE pixel — these frames have 1536 to 1650 pixels,
    where the 0.05 % of test_gpu_pathtrace_golden.py rounds below one.
The call-by-call kernel is held to the fixture under the bounds of the host yardstick (test_oracle_volume.ULP_BOUND: twice the measured distance of the glibc and the
shared-math restatement), discrete outputs equal.  Reads only the fixtures and the product's host code."""
import os
import sys

import numpy as np
import pytest

import oracle
import test_oracle_volume as T
import volume_cases as K
import volume_ref
from cudatracerlib_amd import api

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generate():
    sys.path.insert(0, G)
    import generate
    return generate


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "volumes.npz"))


@pytest.fixture(scope="module")
def frames():
    return np.load(os.path.join(G, "pathtrace_media.npz"))


@pytest.fixture(scope="module")
def orc_libm():
    return oracle.Oracle()


def _outside(img, rgb):
    return (np.abs(img[..., :3] - rgb) > 2e-3 * (1 + np.abs(rgb))).any(axis=2)


@pytest.mark.parametrize("key", [c[0] for c in _generate().pathtrace_media_cases() if not c[0].startswith("clear")])
def test_gpu_path_tracer_with_media_against_the_references_own_path_trace(gpu, frames, orc_sm, key):
    generate = _generate()
    _, make, w, h, direct, first = next(c for c in generate.pathtrace_media_cases() if c[0] == key)
    sc = make(); d = sc.desc
    tables = generate.pathtrace_media_tables(first)
    assert generate.pathtrace_media_digest(d, tables) == str(frames[key + "_digest"]), "regenerate tests/golden/pathtrace_media.npz"
    tr = gpu.PathTracer()
    p = tr.getParameters()
    p.setValue("Direct", direct); p.setValue("MaxPathLength", generate.MEDIA_MAX_PATH_LENGTH); p.setValue("RRStartDepth", generate.MEDIA_RR_START)
    tr.Resize(w, h); tr.InitializeScene(gpu.Scene(d, flatten=True))
    img = gpu.Image(w, h)
    for k in range(len(tables)):
        tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == 0))
    got = img.getPixelData()
    rgb, weight = frames[key + "_rgb"], frames[key + "_weight"]
    fb = api.FlatBvh(d, api.FLAT_Q4)
    sm = volume_ref.path_trace(orc_sm, d, generate.media_volumes(d), w, h, tables, direct=direct, max_path_length=generate.MEDIA_MAX_PATH_LENGTH, rr_start=generate.MEDIA_RR_START, flat=fb.desc)
    out_gpu, out_sm = _outside(got, rgb), _outside(sm, rgb)
    frac = 1.0 - out_gpu.mean()
    print("%s PathTracer: within tolerance GPU %.4f, shared-math restatement %.4f" % (key, frac, 1.0 - out_sm.mean()))
    assert out_gpu.sum() <= out_sm.sum() + 1, (out_gpu.sum(), out_sm.sum())
    assert np.array_equal(got[..., 6], weight), "weightSum differs in %d pixels" % (got[..., 6] != weight).sum()
    assert frac >= 0.99, frac
    assert abs(got[..., :3].mean() - rgb.mean()) <= 2e-3 * rgb.mean()


@pytest.mark.parametrize("what", sorted(K.FUNCTIONS))
def test_volume_eval_device_against_the_references_own_volumes(gpu, golden, orc_libm, orc_sm, what):
    """ctl_volume_eval(on_device = 1) against the fixture: every function on every recorded set, the sent rows, under the host yardstick's bounds"""
    for name in T.sets_of(what):
        c = T.case_rows(golden, orc_libm, orc_sm, what, name)
        dev = api.volume_eval(api.volumes_desc(c["vols"]), what, c["q"], on_device=True)
        n, aside, worst = T.against_fixture(c, what, name, dev, "device")
        print("%s on %s: %d rows, %d set aside, device %d ulp from the reference (bound %d)" % (K.FUNCTIONS[what], name, n, aside, worst, T.ULP_BOUND[what]))
