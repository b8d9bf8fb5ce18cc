"""The PrimTracer's per-pixel restatement (tests/prim_tracer_ref.py, the checker of tests/test_gpu_prim_tracer.py) against the reference's OWN computePixel
(Integrators/PrimTracer.cu:19-106, with g_DepthImage2 at :16), built from the reference's sources with everything it calls (oracle/Makefile, ref_primtracer_render
in oracle/ref_pathtrace_driver.cpp) and recorded in tests/golden/primtracer.npz.

The restatement runs on the glibc oracle, traverses the reference's two-level structure (flat=None) and decodes the triangles' halves with half::ToFloat's host
branch, as the reference compiled for the host does.  In every case and drawing mode, every restated pixel must equal the fixture BIT FOR BIT (rgb and weightSum),
trace the same number of rays (g_RayTracedCounter around one pixel: traceRay and Occluded) and store the same depth (g_DepthImage2: the last traced distance).
Pixels whose path meets an image texture are not restated (the device filters the primary hit's texture with ray differentials; the oracle's BSDF probes do not):
tests/test_gpu_prim_tracer_golden.py holds the GPU to the fixture there.  Reads only the .npz and the product's host code."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import prim_tracer_ref as R   # noqa: E402

# Pixels that cannot be restated bit for bit: {(case, mode): [(y, x), ...]}.  Each entry must still differ, so that it cannot go stale.
EXCLUDED = {}
# cases where no emitter is seen at the primary hit or at the end of a delta chain: their *_Le frames are black in the reference as well
NO_EMITTER_IN_VIEW = ("cornell", "extra_materials", "maps", "maps_height")


def _generate():
    sys.path.insert(0, G)
    import generate
    return generate


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "primtracer.npz"))


@functools.lru_cache(maxsize=None)
def _orc():
    import oracle
    return oracle.Oracle()


def _case(key):
    return next(c for c in _generate().primtracer_cases() if c[0] == key)


@functools.lru_cache(maxsize=None)
def restate(key):
    """{mode: (rgb (h, w, 3), restated (h, w), rays (h, w), last traced distance (h, w))}, the primary hits and the scene"""
    _, make, w, h, modes, max_path_length = _case(key)
    orc = _orc()
    sc = make()
    tables = _generate().primtracer_tables()
    pr = R.primary(orc, sc.desc, w, h, tables, flat=None, half_host_quirk=True)
    env = R.environment(orc, pr, sc.desc, w, h)
    hit = pr["hit"].reshape(h, w)
    out = {}
    for mode in modes:
        if mode in R.GEOMETRY_MODES:
            out[mode] = (R.geometry_frame(pr, sc.desc, w, h, mode) + env, np.ones((h, w), bool), np.ones((h, w), np.int64), pr["t"].reshape(h, w))
    if any(m in R.SHADED_MODES for m in modes):
        shaded, ok = R.shaded_modes(orc, pr, sc.desc, w, h, tables, max_path_length)
        for mode in modes:
            if mode in R.SHADED_MODES:
                rgb, _, rays, last_t = shaded[mode]
                out[mode] = (rgb + env, ok | ~hit, rays, last_t)
    return out, pr, sc


@pytest.mark.parametrize("key", [c[0] for c in _generate().primtracer_cases()])
def test_restatement_equals_the_references_own_compute_pixel(golden, key):
    generate = _generate()
    _, make, w, h, modes, _ = _case(key)
    res, pr, sc = restate(key)
    assert generate.pathtrace_input_digest(sc.desc, [generate.primtracer_tables()]) == str(golden[key + "_digest"]), \
        "the compiled scene or the sampler tables changed: regenerate tests/golden/primtracer.npz (python tests/golden/generate.py primtracer)"
    near, far = sc.desc.camera.near_depth, sc.desc.camera.far_depth
    for mode in modes:
        k = "%s_%s" % (key, mode)
        rgb, ok, rays, last_t = res[mode]
        want_rgb, want_w, want_rays = golden[k + "_rgb"], golden[k + "_weight"], golden[k + "_rays"].astype(np.int64)
        assert want_rgb.shape == (h, w, 3)
        mask = ok.copy()
        for y, x in EXCLUDED.get((key, mode), []):
            assert (rgb[y, x].view(np.uint32) != want_rgb[y, x].view(np.uint32)).any() or rays[y, x] != want_rays[y, x], \
                "%s: excluded pixel (%d, %d) agrees now: drop the exclusion" % (k, x, y)
            mask[y, x] = False
        same = np.all(rgb.view(np.uint32) == want_rgb.view(np.uint32), axis=2)
        bad = mask & ~same
        assert not bad.any(), "%s: %d restated pixels differ from the reference's computePixel, first (y, x) %s: %s vs %s" % (
            k, bad.sum(), np.argwhere(bad)[:3].tolist(), rgb[bad][:3].tolist(), want_rgb[bad][:3].tolist())
        assert (want_w == 1).all(), k                                           # one valid sample per pixel at its own position
        bad = mask & (rays != want_rays)
        assert not bad.any(), "%s: ray counts differ in %d pixels, first (y, x) %s: %s vs %s" % (
            k, bad.sum(), np.argwhere(bad)[:3].tolist(), rays[bad][:3].tolist(), want_rays[bad][:3].tolist())
        if k + "_depth" in golden:
            depth = np.array([R.d3d_depth(near, far, t) for t in last_t.ravel()], np.float32).reshape(h, w)
            want = golden[k + "_depth"]
            assert np.isfinite(want).all(), k
            bad = mask & (depth.view(np.uint32) != want.view(np.uint32))
            assert not bad.any(), "%s: depth differs in %d pixels, first (y, x) %s" % (k, bad.sum(), np.argwhere(bad)[:3].tolist())


def test_prim_tracer_fixture_covers_the_drawing_modes(golden):
    """every case is recorded with its shapes and holds what its scene is there for: hits and misses where there is an environment, delta chains, chains that
    MaxPathLength 1 cuts short, v_dot_n_* values that AddSample clamps to 0, and enough restated pixels"""
    generate = _generate()
    for key, make, w, h, modes, max_path_length in generate.primtracer_cases():
        res, pr, sc = restate(key)
        hit = pr["hit"].reshape(h, w)
        assert hit.mean() > 0.3, key
        if sc.desc.env_map_index != 0xffffffff:
            assert (~hit).sum() > 0.05 * w * h, key
            assert (golden["%s_%s_rgb" % (key, modes[0])][~hit] > 0).any(axis=1).all(), key   # EvalEnvironment is not black
        for mode in modes:
            k = "%s_%s" % (key, mode)
            assert golden[k + "_rgb"].shape == (h, w, 3) and golden[k + "_rays"].shape == (h, w), k
            if mode.endswith("_Le") and key in NO_EMITTER_IN_VIEW:
                assert golden[k + "_rgb"].max() == 0, k
            else:
                assert golden[k + "_rgb"].max() > 0, k
            assert int(golden[k + "_rays"].min()) >= 1, k                      # the primary traceRay of every pixel
            assert res[mode][1].mean() >= (0.5 if key.startswith("env") else 0.9), (k, res[mode][1].mean())
            if mode in R.GEOMETRY_MODES:
                assert (golden[k + "_rays"] == 1).all(), k
        if "first_non_delta_f" in modes and key.startswith(("glass", "extra", "env")):
            chain = golden[key + "_first_non_delta_f_rays"] > 1
            assert chain.sum() >= 10, key                                       # delta primaries whose chain was traced
        if "first_f_direct" in modes:
            assert (golden[key + "_first_f_direct_rays"] > 1).any(), key        # shadow rays
    # a chain that MaxPathLength 1 ends inside the glass sphere and 7 lets out (at 1 the do-while still traces twice: in and out of the sphere, so only
    # paths with a total internal reflection are cut)
    for mode in ("first_non_delta_f", "first_non_delta_f_direct"):
        l1, l7 = golden["glass_l1_%s_rgb" % mode], golden["glass_%s_rgb" % mode]
        cut = (l1 == 0).all(axis=2) & (l7 > 0).any(axis=2)
        assert cut.sum() >= 1, mode
        r1, r7 = golden["glass_l1_%s_rays" % mode], golden["glass_%s_rays" % mode]
        assert (r1 <= r7).all() and r1.sum() < r7.sum(), mode
    # negative dot products that Image::AddSample clamps to 0
    clamped = 0
    for key, make, w, h, modes, _ in generate.primtracer_cases():
        if "v_dot_n_shade" not in modes:
            continue
        _, pr, _ = restate(key)
        raw = np.array([R._dot(-pr["rays"][i, 4:7], pr["sn"][i]) for i in range(w * h)], np.float32).reshape(h, w)
        neg = pr["hit"].reshape(h, w) & (raw < 0)
        assert (golden[key + "_v_dot_n_shade_rgb"][neg] == 0).all(), key
        clamped += int(neg.sum())
    assert clamped >= 5, clamped
