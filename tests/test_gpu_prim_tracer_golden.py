"""The PrimTracer plugin against the reference's OWN computePixel (tests/golden/primtracer.npz: Integrators/PrimTracer.cu:19-106 built from the reference's sources
and run on the host with glibc — tests/test_oracle_prim_tracer.py pins tests/prim_tracer_ref.py on the same fixture bit for bit).

Every case and drawing mode of the fixture is rendered with the recorded sampler tables and MaxPathLength, and each frame is held to the FIXTURE:
  * weightSum equal in every pixel,
  * >= 99 % of pixels within 1e-5 (geometry modes) or 2e-3 * (1 + |ref|) (shaded modes) in every channel.  In the geometry modes the tolerance of a pixel is
    widened by the host branch of half::ToFloat's own effect there: the reference compiled for the host decodes a zero half (a normal's or a uv's
    zero component) to 2^-15, the device to 0, so n_geo / uv / v_dot_n_* values move by up to a few 1e-5 (more behind a normal map).  That effect is measured per
    pixel with the CPU-pinned restatement on the glibc oracle (host branch against device branch), not estimated;
  * the frame mean within 2e-3 relative (plus, in the geometry modes, the mean of the same per-pixel widening: a uv frame of a scene without uvs is nothing but it),
  * and the GPU is no further from the reference than the shared-math restatement (prim_tracer_ref.py on oracle/liboracle_sm.so with the product's flattened BVH,
    the checker of tests/test_gpu_prim_tracer.py): over the pixels it restates, the GPU's count of pixels outside the tolerance exceeds the restatement's by at
    most 0.05 % of the frame (and at least 1 pixel);
  * the pixels the restatement skips (an image texture at the primary hit, filtered with the ray differentials) are held to the fixture alone: >= 99 % within
    the shaded tolerance;
  * rays_last_pass within 0.2 % of the fixture's total;
  * the depth buffer (g_DepthImage2: the last traced distance) bit-equal to the fixture's in >= 99.5 % of pixels, and finite everywhere.
The bars are looser than test_gpu_prim_tracer.py's for the reasons test_gpu_pathtrace_golden.py gives: the reference runs glibc's transcendental functions and the
host branch of half::ToFloat, and a ray grazing the edge two triangles share may resolve to the other triangle in the reference's two-level BVH than in the
flattened one.  Reads nothing but the fixture and the product's host code."""
import os
import sys

import numpy as np
import pytest

import oracle
from cudatracerlib_amd import api

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
import prim_tracer_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu


def _generate():
    sys.path.insert(0, G)
    import generate
    return generate


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(G, "primtracer.npz"))


def _outside(rgb, ref, geometric, quirk=0.0):
    tol = 1e-5 + quirk if geometric else 2e-3 * (1 + np.abs(ref))
    return (np.abs(rgb - ref) > tol).any(axis=2)


@pytest.mark.parametrize("key", [c[0] for c in _generate().primtracer_cases()])
def test_gpu_prim_tracer_against_the_references_own_compute_pixel(gpu, golden, orc_sm, key):
    generate = _generate()
    _, make, w, h, modes, max_path_length = next(c for c in generate.primtracer_cases() if c[0] == key)
    sc = make()
    tables = generate.primtracer_tables()
    assert generate.pathtrace_input_digest(sc.desc, [tables]) == str(golden[key + "_digest"]), "regenerate tests/golden/primtracer.npz"
    fb = api.FlatBvh(sc.desc, api.FLAT_Q4)
    pr = R.primary(orc_sm, sc.desc, w, h, tables, flat=fb.desc)
    env = R.environment(orc_sm, pr, sc.desc, w, h)
    hit = pr["hit"].reshape(h, w)
    orc = oracle.Oracle()   # glibc: the host branch of half::ToFloat against the device branch, on the reference's two-level structure
    pr_host, pr_dev = (R.primary(orc, sc.desc, w, h, tables, half_host_quirk=q) for q in (True, False))
    shaded, ok = (R.shaded_modes(orc_sm, pr, sc.desc, w, h, tables, max_path_length) if any(m in R.SHADED_MODES for m in modes) else (None, None))
    scene = gpu.Scene(sc.desc, flatten=True)
    for mode in modes:
        k = "%s_%s" % (key, mode)
        geometric = mode in R.GEOMETRY_MODES
        tr = gpu.PrimTracer()
        tr.getParameters().setValue("DrawingMode", mode)
        tr.getParameters().setValue("MaxPathLength", max_path_length)
        tr.Resize(w, h)
        tr.InitializeScene(scene)
        if k + "_depth" in golden:
            tr.setDepthBuffer(w, h)
        img = gpu.Image(w, h)
        tr.setSamplerTables(*tables)
        tr.DoPass(img)
        got = img.getPixelData()
        rgb, weight, rays = golden[k + "_rgb"], golden[k + "_weight"], golden[k + "_rays"].astype(np.int64)
        quirk = 0.0
        if geometric:
            sm, restated = R.geometry_frame(pr, sc.desc, w, h, mode) + env, np.ones((h, w), bool)
            quirk = np.abs(R.geometry_frame(pr_host, sc.desc, w, h, mode) - R.geometry_frame(pr_dev, sc.desc, w, h, mode))
        else:
            sm, restated = shaded[mode][0] + env, ok | ~hit
        out_gpu, out_sm = _outside(got[..., :3], rgb, geometric, quirk), _outside(sm, rgb, geometric, quirk)
        frac = 1.0 - out_gpu.mean()
        print("%s: within tolerance GPU %.4f, shared-math restatement %.4f (over %d restated pixels of %d)" % (
            k, frac, 1.0 - out_sm[restated].mean(), restated.sum(), w * h))
        assert np.array_equal(got[..., 6], weight), "%s: weightSum differs in %d pixels" % (k, (got[..., 6] != weight).sum())
        assert frac >= 0.99, (k, frac)
        assert abs(got[..., :3].mean() - rgb.mean()) <= 2e-3 * abs(rgb.mean()) + np.mean(quirk), (k, got[..., :3].mean(), rgb.mean())   # cornell uv: all quirk
        assert (out_gpu & restated).sum() <= (out_sm & restated).sum() + max(1.0, 5e-4 * w * h), (k, (out_gpu & restated).sum(), (out_sm & restated).sum())
        if (~restated).any():
            skipped = 1.0 - _outside(got[..., :3], rgb, False)[~restated].mean()
            print("%s: %d pixels not restated, within tolerance GPU %.4f" % (k, (~restated).sum(), skipped))
            assert skipped >= 0.99, (k, skipped)
        total = int(rays.sum())
        assert abs(int(tr.stats().rays_last_pass) - total) <= 2e-3 * total, (k, tr.stats().rays_last_pass, total)
        if k + "_depth" in golden:
            depth, want = tr.getDepthBuffer(), golden[k + "_depth"]
            assert depth.shape == (h, w) and np.isfinite(depth).all(), k
            same = (depth.view(np.uint32) == want.view(np.uint32)).mean()
            print("%s: depth bit-equal %.4f" % (k, same))
            assert same >= 0.995, (k, same)
