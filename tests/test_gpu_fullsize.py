"""The hot path at BASELINE's full size — synthetic-SM, 1920x1080, depth 8, NEE on (bench.py's workload) — through properties
that do not need the oracle to render the whole frame:
  * a band of rows rendered by the oracle (PathTrace<DIRECT> on the CPU) equals the same rows of the GPU frame, per pixel;
  * the frame does not depend on how the passes are batched, nor on how many ranks the tiles are sharded over;
  * the megakernel plugin and the wavefront plugin produce the same frame and count the same rays;
  * linearity: 2 x (k passes) accumulates to the same sums as 2k passes.
"""
import os
import numpy as np
import pytest
from cudatracerlib_amd import scenes

pytestmark = pytest.mark.gpu
W, H, DEPTH = 1920, 1080, 8


@pytest.fixture(scope="module")
def workload(gpu, orc_sm, tmp_path_factory):
    orc = orc_sm
    gpu.api.set_cache_dir(os.environ.get("CTL_CACHE_DIR") or os.path.join(os.environ.get("TMPDIR", "/tmp"), "ctl_amd_cache"))
    sc = scenes.synthetic_sm(W, H, n_instances=2000, subdiv=4)
    d = sc.desc
    flat = gpu.Scene(d, flatten=True)
    gpu.api.set_cache_dir(None)
    tables = orc.sequence_tables(4)
    return sc, d, flat, tables


def render(gpu, cls, scene, tables, passes=None, shard=None, **params):
    tr = cls()
    p = tr.getParameters(); p.setValue("MaxPathLength", DEPTH)
    for k, v in params.items():
        p.setValue(k, v)
    if shard:
        tr.setTileShard(*shard)
    tr.Resize(W, H); tr.InitializeScene(scene)
    img = gpu.Image(W, H)
    for k in (range(len(tables)) if passes is None else passes):
        tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == (0 if passes is None else passes[0])))
    return img.getPixelData(), tr.stats().rays_total


def test_oracle_band_equals_the_gpu_rows(gpu, orc, workload):
    """Bands of the full-size frame rendered by the oracle against the same rows of the GPU frame, for the two-level layout (the
    reference's traversal arithmetic, bit for bit) and the flattened layout that bench.py times — held to the SAME thresholds: its leaf
    entries are evaluated with the reference's instance-transform + Woop arithmetic, the world-space tree only culls."""
    sc, d, flat, tables = workload
    two_level = gpu.Scene(d)
    bands = (0, 531, 1072)                                            # top edge, middle, bottom edge of the frame
    want = {}
    for depth in (2, DEPTH):
        for y0 in bands:
            want[depth, y0] = orc.render(d, W, H, n_passes=2, tables=tables[:2], max_path_length=depth, rows=(y0, y0 + 8), threads=os.cpu_count() or 8)[0]

    def check(scene, depth, frac, mean_tol):
        tr_tables = tables[:2]
        tr = gpu.WavefrontPathTracer(); tr.getParameters().setValue("MaxPathLength", depth)
        tr.Resize(W, H); tr.InitializeScene(scene)
        img = gpu.Image(W, H)
        for k in range(2):
            tr.setSamplerTables(*tr_tables[k]); tr.DoPass(img, new_trace=(k == 0))
        got = img.getPixelData()
        assert tr.stats().rays_total > 2 * W * H                       # every pixel traced at least its primary ray, twice
        for y0 in bands:
            # (y + jitter) can round up to y + 1 in fp32, so a few samples cross a row boundary: the band's edge rows trade samples with rows
            # the oracle did not render.  Compare the interior rows, on the pixels whose sample count agrees.
            g, w = got[y0 + 1:y0 + 7, :, :3], want[depth, y0][y0 + 1:y0 + 7, :, :3]
            same_n = got[y0 + 1:y0 + 7, :, 6] == want[depth, y0][y0 + 1:y0 + 7, :, 6]
            assert same_n.mean() >= 0.999
            g, w = g[same_n][None], w[same_n][None]
            ok = (np.abs(g - w) <= 2e-3 * (1 + np.abs(w))).all(axis=2)
            assert ok.mean() >= frac, (depth, y0, ok.mean())
            assert abs(g.mean() - w.mean()) <= mean_tol * w.mean(), (depth, y0, g.mean(), w.mean())
    # Every bounce off one of the 2000 small spheres multiplies a direction error by roughly distance / radius (tens): a 1-ulp difference between libm and the
    # device library's sin / cos / acos used to reach the 2e-3 pixel tolerance after three or four bounces and made the depth-8 bar statistical (97 % of pixels).
    # Kernels and checker now run the same transcendental functions (csrc/ctl_fmath.h; the oracle's shared-math build), and depth 8 holds the depth-2 bar.
    check(two_level, 2, 0.998, 1e-3)
    check(two_level, DEPTH, 0.998, 1e-3)
    check(flat, 2, 0.998, 1e-3)
    check(flat, DEPTH, 0.998, 1e-3)
    outside = np.ones(H, bool); outside[1072:1080] = False
    assert not np.any(want[DEPTH, 1072][outside])                     # the oracle really rendered the band only


def test_batching_and_sharding_do_not_change_the_frame(gpu, workload):
    sc, d, flat, tables = workload
    def own_tables(batch):   # the tracer's own generator: passes 1..4 of a fresh XORWOW stream, rendered `batch` passes per wavefront
        tr = gpu.WavefrontPathTracer(); p = tr.getParameters(); p.setValue("MaxPathLength", DEPTH); p.setValue("PassBatch", batch)
        tr.Resize(W, H); tr.InitializeScene(flat)
        img = gpu.Image(W, H)
        tr.DoPasses(img, 4, new_trace=True)
        return img.getPixelData(), tr.stats().rays_total
    single, rays_single = own_tables(1)
    four, rays_four = own_tables(4)
    assert rays_single == rays_four
    assert np.array_equal(single[..., 6], four[..., 6])
    assert np.allclose(single[..., :3], four[..., :3], rtol=1e-5, atol=1e-5)
    one, rays_one = render(gpu, gpu.WavefrontPathTracer, flat, tables)
    parts =[render(gpu, gpu.WavefrontPathTracer, flat, tables, shard=(r, 8)) for r in range(8)]   # what 8 ranks would render
    s = sum(p[0] for p in parts)
    assert sum(p[1] for p in parts) == rays_one
    assert np.array_equal(s[..., 6], one[..., 6])
    assert np.allclose(s[..., :3], one[..., :3], rtol=1e-5, atol=1e-5)
    # ... and what ONE gather of their packed tiles (ctl_image_gather: 64 slots of 65 x 65 pixels per rank, the halo carrying the samples a rank accumulated one pixel inside
    # another rank's tile) gives the root: each shard frame through the device pack kernel, all eight buffers through the device unpack — the frame of the sum (= of the
    # reduce).  Weights exactly; colours bit for bit except where a halo sample was added (another order of the same additions).
    import tile_shards
    img = gpu.Image(W, H); packed = []
    for r in range(8):
        img.setPixelData(parts[r][0]); packed.append(img.packTiles(r, 8))
        own = tile_shards.tile_mask(W, H, r, 8)
        assert (parts[r][0][..., 6][~own] != 0).sum() < 200                # the spill into other ranks' tiles exists and is rare (~1e-5 of the samples)
    assert packed[0].nbytes == 7571200
    img.setPixelData(parts[0][0]); img.unpackTiles(8, np.stack(packed))
    g = img.getPixelData()
    assert np.array_equal(g[..., 6], s[..., 6])
    assert np.allclose(g[..., :3], s[..., :3], rtol=1e-6, atol=1e-6) and (g[..., :3] == s[..., :3]).all(axis=2).mean() > 0.9999
    assert sum((parts[r][0][..., 6][~tile_shards.tile_mask(W, H, r, 8)] != 0).sum() for r in range(8)) > 0   # (the halo path was exercised)
    share = np.array([p[1] for p in parts], np.float64) / rays_one
    assert share.min() > 0.09 and share.max() < 0.16                  # round-robin tiles balance the ranks (ideal 0.125)


def test_linearity_and_plugin_agreement(gpu, workload):
    sc, d, flat, tables = workload
    ab, rays_ab = render(gpu, gpu.WavefrontPathTracer, flat, tables)
    a, rays_a = render(gpu, gpu.WavefrontPathTracer, flat, tables, passes=[0, 1])
    b, rays_b = render(gpu, gpu.WavefrontPathTracer, flat, tables, passes=[2, 3])
    assert rays_a + rays_b == rays_ab
    assert np.array_equal(a[..., 6] + b[..., 6], ab[..., 6])
    assert np.allclose(a[..., :3] + b[..., :3], ab[..., :3], rtol=1e-5, atol=1e-5)
    mega, rays_mega = render(gpu, gpu.PathTracer, flat, tables[:2])
    assert abs(int(rays_mega) - int(rays_a)) <= 1e-4 * rays_a
    assert np.array_equal(mega[..., 6], a[..., 6])
    close = np.isclose(mega[..., :3], a[..., :3], rtol=1e-3, atol=1e-3).all(axis=2)
    assert close.mean() >= 0.999 and abs(mega[..., :3].mean() - a[..., :3].mean()) <= 1e-4 * a[..., :3].mean()


def test_loader_fed_frame_equals_the_builder_fed_frame(gpu, orc, tmp_path):
    """row J1 at BASELINE size: the bench workload written as a Mitsuba-0.5 scene (XML + .serialized meshes), loaded through ctl_parse_mitsuba_scene,
    flattened and rendered at 1920x1080, against the same description through the builder API.  Geometry, transforms, materials and lights of the two
    scenes are bit-identical (tests/test_mitsuba_loader.py).  The loader derives the camera frame the reference's way (Sensor::SetToWorld(pos, f)), one unit
    in the last place away from DynamicScene.setCamera's — enough to move every path by an ulp, which eight bounces off small spheres amplify past any
    tight tolerance — so the builder-fed scene is given the loader's ctl_sensor: then the two frames must agree like two runs of one scene (same ray count,
    same samples per pixel, sums to rtol 1e-5: float atomics accumulate in another order)."""
    d = scenes.with_explicit_normals(scenes.synthetic_sm_description(W, H, n_instances=2000, subdiv=4))
    sc_b = scenes.load_mitsuba(scenes.export_mitsuba(d, str(tmp_path)))
    sc_a = scenes.build_scene(d, sensor=sc_b.desc.camera)
    assert sc_a.desc.n_tri_data == sc_b.desc.n_tri_data and sc_a.desc.n_nodes == sc_b.desc.n_nodes
    tables = orc.sequence_tables(2)
    frames = []
    gpu.api.set_cache_dir(os.environ.get("CTL_CACHE_DIR") or os.path.join(os.environ.get("TMPDIR", "/tmp"), "ctl_amd_cache"))
    try:
        for sc in (sc_a, sc_b):
            scene = gpu.Scene(sc.desc, flatten=True)
            frames.append(render(gpu, gpu.WavefrontPathTracer, scene, tables))
    finally:
        gpu.api.set_cache_dir(None)
    (a, rays_a), (b, rays_b) = frames
    assert rays_a == rays_b and rays_a > 2 * W * H
    assert np.array_equal(a[..., 6], b[..., 6])
    assert np.allclose(a[..., :3], b[..., :3], rtol=1e-5, atol=1e-5)


def test_bathroom_workload_at_full_size(gpu, orc):
    """synthetic-bathroom (the stand-in for BASELINE config 5: rough plastic / conductor / dielectric, coating, textures, height map, environment
    emitter) at 1920x1080, depth 8, through the full shade kernel:
      * two bands of rows rendered by the oracle equal the same rows of the GPU frame (per pixel where paths are short, band mean at full depth);
      * the one kernel with every model (ShadeByModelClass off) instead of a launch per model class only reorders work: same frame, same rays;
      * 2 x (1 pass) accumulates to the same sums as 2 passes; the megakernel plugin renders the same frame."""
    gpu.api.set_cache_dir(os.environ.get("CTL_CACHE_DIR") or os.path.join(os.environ.get("TMPDIR", "/tmp"), "ctl_amd_cache"))
    sc = scenes.synthetic_bathroom(W, H)
    d = sc.desc
    flat = gpu.Scene(d, flatten=True)
    gpu.api.set_cache_dir(None)
    tables = orc.sequence_tables(2)
    bands = (531, 1040)                                               # spheres and back wall; the textured, height-mapped floor
    for depth, frac, mean_tol in ((2, 0.998, 1e-3), (DEPTH, 0.998, 1e-3)):
        tr = gpu.WavefrontPathTracer(); tr.getParameters().setValue("MaxPathLength", depth)
        tr.Resize(W, H); tr.InitializeScene(flat)
        img = gpu.Image(W, H)
        for k in range(2):
            tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == 0))
        got = img.getPixelData()
        assert np.isfinite(got[..., :3]).all() and (got[..., :3] >= 0).all()
        for y0 in bands:
            want = orc.render(d, W, H, n_passes=2, tables=tables, max_path_length=depth, rows=(y0, y0 + 8), threads=os.cpu_count() or 8)[0]
            g, w = got[y0 + 1:y0 + 7, :, :3], want[y0 + 1:y0 + 7, :, :3]
            same_n = got[y0 + 1:y0 + 7, :, 6] == want[y0 + 1:y0 + 7, :, 6]
            assert same_n.mean() >= 0.999
            g, w = g[same_n][None], w[same_n][None]
            ok = (np.abs(g - w) <= 2e-3 * (1 + np.abs(w))).all(axis=2)
            assert ok.mean() >= frac, (depth, y0, ok.mean())
            assert abs(g.mean() - w.mean()) <= mean_tol * w.mean(), (depth, y0, g.mean(), w.mean())
            # round 5: rough plastic runs the reference's own transmittance lookup on the device — the bands are equal to the BIT (rounds 2-4: the tolerance only)
            assert (g == w).all(axis=2).mean() >= 0.97, (depth, y0, float((g == w).all(axis=2).mean()))
    base, rays = render(gpu, gpu.WavefrontPathTracer, flat, tables)
    assert rays > 4 * W * H
    for params in (dict(ShadeByModelClass=False),):
        other, rays_o = render(gpu, gpu.WavefrontPathTracer, flat, tables, **params)
        assert rays_o == rays
        assert np.array_equal(other[..., 6], base[..., 6])
        assert np.allclose(other[..., :3], base[..., :3], rtol=1e-5, atol=1e-5)
    a, rays_a = render(gpu, gpu.WavefrontPathTracer, flat, tables, passes=[0])
    b, rays_b = render(gpu, gpu.WavefrontPathTracer, flat, tables, passes=[1])
    assert rays_a + rays_b == rays
    assert np.allclose(a[..., :3] + b[..., :3], base[..., :3], rtol=1e-5, atol=1e-5)
    mega, rays_mega = render(gpu, gpu.PathTracer, flat, tables)
    assert abs(int(rays_mega) - int(rays)) <= 1e-3 * rays
    close = np.isclose(mega[..., :3], base[..., :3], rtol=1e-3, atol=1e-3).all(axis=2)
    assert close.mean() >= 0.995 and abs(mega[..., :3].mean() - base[..., :3].mean()) <= 1e-3 * base[..., :3].mean()


def test_cornell_glass_at_full_size(gpu, orc):
    """BASELINE configs[1]: Cornell box + glass sphere, 1024x1024, depth 8, both layouts: oracle bands (through the sphere, across the light),
    batching invariance and plugin agreement at the configuration's own size."""
    w = h = 1024
    sc = scenes.cornell_box(w, h, glass_sphere=True)
    d = sc.desc
    tables = orc.sequence_tables(2)
    bands = (96, 640)                                                 # ceiling light; the glass sphere and its caustic
    want = {y0: orc.render(d, w, h, n_passes=2, tables=tables, max_path_length=DEPTH, rows=(y0, y0 + 8), threads=os.cpu_count() or 8)[0] for y0 in bands}
    frames = []
    for scene in (gpu.Scene(d), gpu.Scene(d, flatten=True)):
        tr = gpu.WavefrontPathTracer(); tr.getParameters().setValue("MaxPathLength", DEPTH)
        tr.Resize(w, h); tr.InitializeScene(scene)
        img = gpu.Image(w, h)
        for k in range(2):
            tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == 0))
        got = img.getPixelData(); frames.append((got, tr.stats().rays_total))
        for y0 in bands:
            g, wv = got[y0 + 1:y0 + 7, :, :3], want[y0][y0 + 1:y0 + 7, :, :3]
            same_n = got[y0 + 1:y0 + 7, :, 6] == want[y0][y0 + 1:y0 + 7, :, 6]
            assert same_n.mean() >= 0.999
            g, wv = g[same_n][None], wv[same_n][None]
            ok = (np.abs(g - wv) <= 2e-3 * (1 + np.abs(wv))).all(axis=2)
            assert ok.mean() >= 0.998, (y0, ok.mean())                 # the bar of the other full-size frames (kernels and checker share their transcendental functions)
            assert abs(g.mean() - wv.mean()) <= 1e-3 * wv.mean(), (y0, g.mean(), wv.mean())
    (two, rays_two), (flat, rays_flat) = frames
    assert rays_two == rays_flat and rays_two > 4 * w * h            # both layouts return the same hits, so the same paths
    assert np.array_equal(two[..., 6], flat[..., 6]) and np.allclose(two[..., :3], flat[..., :3], rtol=1e-5, atol=1e-5)
    # one call of two passes (one wavefront, GPU-generated tables replaced by the same tables pass by pass is not possible here, so: linearity)
    flat_scene = gpu.Scene(d, flatten=True)

    def run(cls, passes):
        tr = cls(); tr.getParameters().setValue("MaxPathLength", DEPTH); tr.Resize(w, h); tr.InitializeScene(flat_scene)
        img = gpu.Image(w, h)
        for k in passes:
            tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == passes[0]))
        return img.getPixelData(), tr.stats().rays_total
    a, ra = run(gpu.WavefrontPathTracer, [0]); b, rb = run(gpu.WavefrontPathTracer, [1])
    assert ra + rb == rays_flat and np.allclose(a[..., :3] + b[..., :3], flat[..., :3], rtol=1e-5, atol=1e-5)
    mega, rm = run(gpu.PathTracer, [0, 1])
    assert abs(int(rm) - int(rays_flat)) <= 1e-3 * rays_flat
    close = np.isclose(mega[..., :3], flat[..., :3], rtol=1e-3, atol=1e-3).all(axis=2)
    assert close.mean() >= 0.995 and abs(mega[..., :3].mean() - flat[..., :3].mean()) <= 1e-3 * flat[..., :3].mean()


def test_synthetic_sm_hard_at_full_size(gpu, orc):
    """synthetic-sm-hard (scenes.write_sm_hard_mitsuba: 8.4 M UNIQUE sliver-terrain triangles in 32 meshes, 4000 alpha-masked foliage cards, 3000 thin beams, bitmap-textured
    diffuse / plastic / rough-conductor materials, the `sun` emitter's spot lights + area lights) through the Mitsuba loader at 1920x1080, depth 8:
      * bands of rows rendered by the oracle equal the same rows of the GPU frame, at the bar of the other full-size workloads;
      * the 4-wide and the 8-wide flattened trees render the same frame and count the same rays (same hits, another tree);
      * with the alpha test on (tracer parameter AlphaTest; the reference's wavefront kernel has none) a band equals the oracle's alpha-tested band."""
    d0 = os.path.join(os.environ.get("TMPDIR", "/tmp"), "ctl_scene_sm_hard_4096x1024_%dx%d" % (W, H))
    gpu.api.set_cache_dir(os.environ.get("CTL_CACHE_DIR") or os.path.join(os.environ.get("TMPDIR", "/tmp"), "ctl_amd_cache"))
    sc = scenes.synthetic_sm_hard(d0, W, H)
    d = sc.desc
    assert d.n_tri_data > 8_400_000 and d.num_lights == 10
    flat = gpu.Scene(d, flatten=True)
    flat8 = gpu.Scene(d, flatten=True, flat_format="q8")
    gpu.api.set_cache_dir(None)
    tables = orc.sequence_tables(2)
    bands = (400, 800)                                                # beams and cards against the far terrain; the near terrain
    frames = {}
    for name, scene, params in (("q4", flat, {}), ("q8", flat8, {}), ("alpha", flat, dict(AlphaTest=True))):
        for depth in ((2, DEPTH) if name == "q4" else (DEPTH,)):
            tr = gpu.WavefrontPathTracer(); p = tr.getParameters(); p.setValue("MaxPathLength", depth)
            for k, v in params.items():
                p.setValue(k, v)
            tr.Resize(W, H); tr.InitializeScene(scene)
            img = gpu.Image(W, H)
            for k in range(2):
                tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == 0))
            got = img.getPixelData(); frames[name, depth] = (got, tr.stats().rays_total)
            assert np.isfinite(got[..., :3]).all() and (got[..., :3] >= 0).all()
            if name == "q8":
                continue
            for y0 in bands:
                want = orc.render(d, W, H, n_passes=2, tables=tables, max_path_length=depth, rows=(y0, y0 + 8), threads=os.cpu_count() or 8, alpha_test=(name == "alpha"))[0]
                g, w = got[y0 + 1:y0 + 7, :, :3], want[y0 + 1:y0 + 7, :, :3]
                same_n = got[y0 + 1:y0 + 7, :, 6] == want[y0 + 1:y0 + 7, :, 6]
                assert same_n.mean() >= 0.999
                g, w = g[same_n][None], w[same_n][None]
                ok = (np.abs(g - w) <= 2e-3 * (1 + np.abs(w))).all(axis=2)
                assert ok.mean() >= 0.998, (name, depth, y0, ok.mean())
                assert abs(g.mean() - w.mean()) <= 1e-3 * w.mean(), (name, depth, y0, g.mean(), w.mean())
    (a, ra), (b, rb) = frames["q4", DEPTH], frames["q8", DEPTH]
    assert abs(int(ra) - int(rb)) <= 1e-4 * ra and np.array_equal(a[..., 6], b[..., 6])
    close = np.isclose(a[..., :3], b[..., :3], rtol=1e-4, atol=1e-5).all(axis=2)
    assert close.mean() >= 0.9995                                     # equal-t ties between the two trees' visiting orders aside
    assert frames["alpha", DEPTH][1] != ra                            # the alpha test changes which rays exist
