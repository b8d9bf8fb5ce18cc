"""Media parity fuzz: the random scenes of tests/test_gpu_fuzz.py — every BSDF model, nested models, image and checker textures, normal and height maps, the five
emitter kinds — under participating media, rendered by both plugins that have medium code: WavefrontPathTracer with ParticipatingMedia = true (k_medium_stage in front of
the media build of the shade kernel) and PathTracer (k_path_trace_media / _grid, with first-hit ray differentials).  The hand-made media scenes are all the Cornell box
with diffuse walls, one area light and the camera inside the fog; these put a point, spot, distant or environment light at the far end of a transmittance, a glossy or
delta lobe in front of a medium vertex, a normal map behind one, the camera outside the medium.

The yardstick is tests/volume_ref.path_trace: PathTrace's loop and medium vertex restated in Python (pinned on the reference's own frames, tests/test_oracle_volume.py),
its surface vertex and environment term the oracle's own (pinned to be the oracle's render without volumes, tests/test_media_fuzz_host.py).  It is computed once per
(seed, partials) and shared.  What qualifies a scene as an input is asserted from the restatement and the descriptions alone, never from a GPU frame."""
import numpy as np
import pytest

import volume_grid_ref
from cudatracerlib_amd import api, scenes

pytestmark = pytest.mark.gpu

W, H, PASSES, DEPTH, RR = 32, 24, 2, 5, 2   # RRStartDepth 2: roulette runs after a medium vertex, with the stale specularBounce of the last surface
# Extinction per scene unit.  The scenes are about 20 units across, so 0.05 is an optical depth of about one along a camera ray (derived, not measured); a grid's
# coefficients are those at density 1 and its seeded density averages about one half, hence the factor 2.
SIGMA_T = 0.05
SEEDS = tuple(range(8))
_memo = {}


def size_of(seed):
    """the frame of a seed: 32 x 24, and 24 x 16 for the grid seeds, whose march makes the restatement of the larger frame slower than the 48 x 32 fog_box
    restatement of tests/test_gpu_wavefront_media.py (RESULTS.md has both times)"""
    return (24, 16) if seed % 2 else (W, H)


def media_fuzz_scene(seed, w, h):
    """scenes.fuzz_scene(seed) plus media from RandomState(seed).  Even seeds: one to three homogeneous regions with random phase functions (isotropic, or Henyey-Greenstein with a
    random g.  Not Rayleigh or Kajiya-Kay: their Sample returns NaN — pow of a negative base, tests/test_volume_host.py — for most draws of the one and 4.5 % of the
    other, which dropped a sample in 80 % and in 19 to 28 % of the pixels of the seeds that drew them, far above the cap; tests/test_gpu_volume.py holds both call by
    call) and albedos — the first over the scene box shrunk by 10 % about its centre (the camera stands outside it), the others over random boxes inside that
    one, so that regions overlap.  Odd seeds: one VolumeGrid of dims (3, 4, 5) — non-cubic, which keeps the index scramble in play — over the same shrunk box."""
    sc = scenes.fuzz_scene(seed, w, h)
    rs = np.random.RandomState(seed)
    lo = np.array(sc.desc.box_min, np.float64); hi = np.array(sc.desc.box_max, np.float64)
    c, half = (lo + hi) / 2, (hi - lo) / 2 * 0.9
    lo, hi = c - half, c + half

    def phase():
        return api.phase_isotropic() if rs.randint(3) == 0 else api.phase_hg(rs.uniform(-0.8, 0.8))

    def coefficients(scale):
        albedo = rs.uniform(0.5, 0.95, 3)
        return tuple(float(x) for x in SIGMA_T * scale * (1 - albedo)), tuple(float(x) for x in SIGMA_T * scale * albedo)
    if seed % 2 == 0:
        for k in range(rs.randint(1, 4)):
            a, b = (lo, hi) if k == 0 else np.sort(rs.uniform(lo, hi, (2, 3)), axis=0)
            sa, ss = coefficients(1.0)
            sc.CreateVolume(api.homogeneous_volume(api.box_to_volume_matrix(a, b), sa, ss, phase()))
    else:
        sa, ss = coefficients(2.0)
        sc.grid = api.grid_volume(api.box_to_volume_matrix(lo, hi), density=scenes.smoke_density((3, 4, 5), seed), sig_a=(0.0, sa), sig_s=(0.0, ss), phase=phase())
        sc.CreateGridVolume(sc.grid)
    sc.UpdateScene()
    return sc


def scene_of(seed, w=None, h=None):
    w, h = (w, h) if w else size_of(seed)
    key = ("scene", seed, w, h)
    if key not in _memo:
        _memo[key] = media_fuzz_scene(seed, w, h)
    return _memo[key]


def restatement(orc_sm, seed, partials):
    """the yardstick's frame of seed's scene, once: (frame, rays, march stats, medium vertices per pixel, vertex counts per pixel)"""
    key = ("frame", seed, partials)
    if key not in _memo:
        d = scene_of(seed).desc
        w, h = size_of(seed)
        rays, stats = [], {}
        vertices = np.zeros((h, w), np.int64); counts = np.zeros((h, w, 3), np.int64)
        fb = api.FlatBvh(d, api.FLAT_Q4)
        want = volume_grid_ref.path_trace(orc_sm, d, w, h, orc_sm.sequence_tables(PASSES), stats=stats, vertices=vertices, vertex_counts=counts, partials=partials,
                                          direct=True, max_path_length=DEPTH, rr_start=RR, flat=fb.desc, ray_count=rays)
        want.setflags(write=False)
        _memo[key] = (want, rays[0], stats, vertices, counts)
    return _memo[key]


def features(d):
    """what the description holds, from its tables alone"""
    out = set()
    for i in range(d.num_lights):
        out.add(("light", int(d.lights[int(d.light_indices[i])].type)))
    if d.env_map_index != 0xffffffff:
        out.add("env_map")
    for i in range(d.n_materials):
        m = d.materials[i]
        if any(m.tex[k].type == 4 for k in range(4)): out.add("image_texture")   # CTL_TEX_IMAGE
        if m.map_kind == api.MAP_NORMAL: out.add("normal_map")
        if m.map_kind == api.MAP_HEIGHT: out.add("height_map")
        if m.bsdf_type in (3, 4, 6): out.add("delta_bsdf")      # dielectric, thin dielectric, conductor
        if m.bsdf_type in (13, 14, 15): out.add("nested_bsdf")   # coating, rough coating, blend
    return out


WANTED = {("light", 1), ("light", 2), ("light", 3), ("light", 4), ("light", 5), "env_map", "image_texture", "normal_map", "height_map", "delta_bsdf", "nested_bsdf"}


def qualify(seed, frame, stats, vertices, counts):
    """the conditions on a scene as an input, from the restatement alone"""
    medium, surface, dropped = float((vertices > 0).mean()), float((counts[..., 1] > 0).mean()), float((frame[..., 6] < PASSES).mean())
    print("seed %d: %.0f %% of the pixels have a medium vertex, %.0f %% a surface vertex, %.1f %% a dropped sample; march %s" % (seed, 100 * medium, 100 * surface, 100 * dropped, stats))
    assert np.array_equal(vertices, counts[..., 0])   # the hook of tests/test_gpu_volume_grid.py and path_trace's own counter agree
    assert medium >= 0.25 and surface >= 0.25, (seed, medium, surface)
    assert stats.get("cap_hits", 0) == 0, (seed, stats)
    assert dropped <= 0.05, (seed, dropped)


def check_the_seeds_cover_the_feature_set():
    """between them the scenes hold all five emitter kinds (the environment map included), an image texture, a normal map, a height map, a delta BSDF and a nested
    BSDF; even seeds have homogeneous regions only, odd seeds one grid.  (Needs no GPU: tests/test_media_fuzz_host.py runs it.)"""
    have = set()
    for seed in SEEDS:
        d = scene_of(seed).desc
        have |= features(d)
        assert (d.n_volume_grids == 1 and d.n_volumes == 1) if seed % 2 else (d.n_volume_grids == 0 and 1 <= d.n_volumes <= 3), seed
    print("features of seeds %s: %s" % (SEEDS, sorted(map(str, have))))
    assert WANTED <= have, WANTED - have


def test_the_seeds_cover_the_feature_set():
    check_the_seeds_cover_the_feature_set()


def hold(name, got, want, rays_got, rays_want):
    g, w = got[..., :3], want[..., :3]
    exact = (g.view(np.uint32) == w.view(np.uint32)).all(axis=2).mean()
    print("%s: %.2f %% of pixels bit-equal, mean %g vs %g, rays %d vs %d" % (name, 100 * exact, g.mean(), w.mean(), rays_got, rays_want))
    assert np.array_equal(got[..., 6], want[..., 6]), ("weightSum", name, np.argwhere(got[..., 6] != want[..., 6])[:4].tolist())
    assert np.isfinite(g).all()
    ok = (np.abs(g - w) <= 2e-3 * (1 + np.abs(w))).all(axis=2)
    assert ok.all(), (name, int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), g[~ok][:2].tolist(), w[~ok][:2].tolist())
    assert abs(float(g.mean()) - float(w.mean())) <= 1e-3 * max(float(w.mean()), 1e-6), name
    assert exact >= 0.98, (name, exact)
    assert abs(rays_got - rays_want) <= 1e-2 * rays_want, (name, rays_got, rays_want)


def tracer(gpu, mode, w, h, direct=True, **params):
    tr = gpu.PathTracer() if mode == "plugin" else gpu.WavefrontPathTracer()
    p = tr.getParameters(); p.setValue("Direct", direct); p.setValue("MaxPathLength", DEPTH); p.setValue("RRStartDepth", RR)
    if mode == "wavefront":
        p.setValue("ParticipatingMedia", True)
    for k, v in params.items():
        p.setValue(k, v)
    tr.Resize(w, h)
    return tr


def frame(gpu, tr, scene, w, h, tables):
    tr.InitializeScene(scene)
    img = gpu.Image(w, h)
    for k in range(len(tables)):
        tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == 0))
    return img.getPixelData()


@pytest.mark.parametrize("mode", ["wavefront", "plugin"])
@pytest.mark.parametrize("seed", SEEDS)
def test_media_fuzz_scene_gpu_equals_the_restatement(gpu, orc_sm, seed, mode):
    """wavefront: ParticipatingMedia = true over the two-level structure and the flattened Q4 and Q8 trees against the plain restatement; plugin: PathTracer on the
    flattened scene against the restatement with first-hit partials.  Bars: weightSum equal in every pixel, every pixel within 2e-3 (1 + |ref|), the frame mean within
    1e-3 relative, at least 98 % of the pixels bit-equal, the ray count within 1 %"""
    want, rays, stats, vertices, counts = restatement(orc_sm, seed, partials=(mode == "plugin"))
    qualify(seed, want, stats, vertices, counts)
    d = scene_of(seed).desc
    w, h = size_of(seed)
    tables = orc_sm.sequence_tables(PASSES)
    layouts = [("flat q4", dict(flatten=True, flat_format=api.FLAT_Q4))] if mode == "plugin" else [
        ("two-level", dict(flatten=False)), ("flat q4", dict(flatten=True, flat_format=api.FLAT_Q4)), ("flat q8", dict(flatten=True, flat_format=api.FLAT_Q8))]
    for name, kw in layouts:
        tr = tracer(gpu, mode, w, h)
        got = frame(gpu, tr, gpu.Scene(d, **kw), w, h, tables)
        hold("seed %d %s %s" % (seed, mode, name), got, want, tr.stats().rays_total, rays)


def _env_pair(direct, partials, orc_sm):
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import generate
    key = ("env", direct, partials)
    if key not in _memo:
        sc = generate.media_pair_scene("env", True)   # scenes.env_scene(48, 32) under the region pair of the fixture tests/golden/pathtrace_media.npz
        d = sc.desc
        rays = []; counts = np.zeros((32, 48, 3), np.int64)
        fb = api.FlatBvh(d, api.FLAT_Q4)
        want = volume_grid_ref.path_trace(orc_sm, d, 48, 32, orc_sm.sequence_tables(PASSES), vertex_counts=counts, partials=partials, direct=direct, max_path_length=DEPTH, rr_start=RR,
                                          flat=fb.desc, ray_count=rays)
        _memo[key] = (sc, want, rays[0], counts)
    return _memo[key]


@pytest.mark.parametrize("mode", ["wavefront", "plugin"])
@pytest.mark.parametrize("direct", [True, False], ids=["direct", "no_direct"])
def test_env_map_after_a_medium_vertex(gpu, orc_sm, direct, mode):
    """env_scene(48, 32) under the fixture's region pair: the environment term for a ray that left a medium vertex — with the MIS weight from the last surface's stale
    pdf when Direct is on — in both plugins, at the fuzz's bars; the restatement takes that branch for at least 50 paths"""
    sc, want, rays, counts = _env_pair(direct, mode == "plugin", orc_sm)
    n = int(counts[..., 2].sum())
    print("env_scene direct=%s: %d paths end on the environment term after a medium vertex" % (direct, n))
    assert n >= 50, n
    tr = tracer(gpu, mode, 48, 32, direct=direct)
    got = frame(gpu, tr, gpu.Scene(sc.desc, flatten=True), 48, 32, orc_sm.sequence_tables(PASSES))
    hold("env_scene %s direct=%s" % (mode, direct), got, want, tr.stats().rays_total, rays)


@pytest.mark.parametrize("filter_mode", ["anisotropic", "trilinear"])
def test_first_hit_partials_under_fog(gpu, orc_sm, filter_mode):
    """the megakernel's first-hit ray differentials with media on.  The images of the fuzz scenes are point- and bilinear-filtered, for which KernelMIPMap::eval reads
    level 0 whatever the partials are, so this is the ground plane of tests/test_gpu_render.py::test_first_hit_ray_differentials_and_filtered_textures — a noise
    texture under the EWA or the trilinear filter, seen at a grazing angle — with a homogeneous region over the scene box (an optical depth of one half across its
    80 units): PathTracer against the restatement with partials at the fuzz's bars.  The restatement alone says that the input tests something: its frames with and
    without partials differ in at least a quarter of the pixels, and at least a quarter of the pixels have a medium vertex"""
    w, h = W, H
    sc = api.DynamicScene()
    rs = np.random.RandomState(4)
    tex = rs.uniform(0.05, 0.95, size=(64, 64, 3)).astype(np.float32)
    tex[::2, ::2] *= 0.2
    img = sc.add_image(api.float3_to_rgbcol(tex), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_ANISOTROPIC if filter_mode == "anisotropic" else api.FILTER_TRILINEAR)
    P = np.array([[-40, 0, -40], [-40, 0, 40], [40, 0, 40], [40, 0, -40]], np.float32)
    ground = api.diffuse((1, 1, 1)); ground.tex[0] = api.image_texture(img)
    sc.CreateNode(sc.add_mesh(P, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=np.tile(np.array([0, 1, 0], np.float32), (4, 1)),
                              uvs=np.array([[0, 0], [0, 12], [12, 12], [12, 0]], np.float32), materials=[ground]))
    L = np.array([[-6, 12, -6], [6, 12, -6], [6, 12, 6], [-6, 12, 6]], np.float32)
    ln = sc.CreateNode(sc.add_mesh(L, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=np.tile(np.array([0, -1, 0], np.float32), (4, 1)), materials=[api.diffuse((0.5, 0.5, 0.5))]))
    sc.CreateLight(ln, 0, (30.0, 30.0, 30.0))
    sc.setCamera((0, 1.5, -30), (0, 0.5, 0), (0, 1, 0), 50.0, w, h)
    d = sc.UpdateScene()
    sc.CreateVolume(api.homogeneous_volume(api.box_to_volume_matrix(np.array(d.box_min, np.float32), np.array(d.box_max, np.float32)), 0.00125, 0.005, api.phase_hg(0.3)))
    d = sc.UpdateScene()
    tables = orc_sm.sequence_tables(PASSES)
    fb = api.FlatBvh(d, api.FLAT_Q4)
    rays = []; counts = np.zeros((h, w, 3), np.int64)
    plain = volume_grid_ref.path_trace(orc_sm, d, w, h, tables, direct=True, max_path_length=DEPTH, rr_start=RR, flat=fb.desc)
    want = volume_grid_ref.path_trace(orc_sm, d, w, h, tables, vertex_counts=counts, partials=True, direct=True, max_path_length=DEPTH, rr_start=RR, flat=fb.desc, ray_count=rays)
    differ, medium = float((plain[..., :3] != want[..., :3]).any(axis=2).mean()), float((counts[..., 0] > 0).mean())
    print("filtered ground under fog (%s): partials change %.0f %% of the restatement's pixels, %.0f %% have a medium vertex" % (filter_mode, 100 * differ, 100 * medium))
    assert differ >= 0.25 and medium >= 0.25, (differ, medium)
    tr = tracer(gpu, "plugin", w, h)
    got = frame(gpu, tr, gpu.Scene(d, flatten=True), w, h, tables)
    hold("filtered ground under fog %s" % filter_mode, got, want, tr.stats().rays_total, rays[0])


def test_debug_pixel_on_a_fuzz_scene(gpu, orc_sm):
    """PathTracer.Debug (Direct on, the pixel's own position, first-hit partials, the tracer's first table set) of four pixels of an environment-map seed against the
    restatement's unjittered path: bit for bit.  The pixels are chosen from the restatement alone: the first four of a fixed scan whose path has a medium vertex and
    carries radiance"""
    seed = next(s for s in SEEDS if "env_map" in features(scene_of(s).desc))
    d = scene_of(seed).desc
    w, h = size_of(seed)
    fb = api.FlatBvh(d, api.FLAT_Q4)
    tables = orc_sm.sequence_tables(1)
    pixels, want = [], []
    for (x, y) in [(x, y) for y in (h // 2, h // 4, 3 * h // 4, 3 * h // 8, 5 * h // 8) for x in range(2, w - 2, 3)]:
        stats = {}
        r = volume_grid_ref.path_trace(orc_sm, d, w, h, tables, stats=stats, partials=True, max_path_length=DEPTH, rr_start=RR, flat=fb.desc, debug_pixels=[(x, y)])
        if stats["scatters"] > 0 and stats["cap_hits"] == 0 and r[0].any() and np.isfinite(r[0]).all():
            pixels.append((x, y)); want.append(r[0])
        if len(pixels) == 4:
            break
    assert len(pixels) == 4, pixels
    scene = gpu.Scene(d, flatten=True)
    img = gpu.Image(w, h)
    for (x, y), wv in zip(pixels, want):
        tr = tracer(gpu, "plugin", w, h)
        tr.InitializeScene(scene)
        got = tr.Debug(img, x, y)
        print("debug pixel", seed, (x, y), got, wv)
        assert np.array_equal(got.view(np.uint32), wv.view(np.uint32)), (x, y, got, wv)


GRID_SEED = 1


def test_a_batch_equals_its_passes_on_a_grid_seed(gpu, orc_sm):
    """PassBatch = 2 against two single passes over the same two table sets, on a grid fuzz scene (k_medium_stage<true>, k_shade_full_media_grid): bit-equal"""
    d = scene_of(GRID_SEED).desc
    W, H = size_of(GRID_SEED)
    assert d.n_volume_grids == 1
    tables = orc_sm.sequence_tables(2)
    scene = gpu.Scene(d, flatten=True)
    single = tracer(gpu, "wavefront", W, H, PassBatch=1)
    one = frame(gpu, single, scene, W, H, tables)
    tr = tracer(gpu, "wavefront", W, H, PassBatch=2)
    tr.InitializeScene(scene)
    img = gpu.Image(W, H)
    tr.DoPasses(img, 2, new_trace=True)
    both = img.getPixelData()
    assert one[..., :3].any() and (one[..., 6] == 2).mean() > 0.9
    assert np.array_equal(both.view(np.uint32), one.view(np.uint32)), (both.view(np.uint32) != one.view(np.uint32)).any(axis=2).sum()
    assert single.stats().rays_total == tr.stats().rays_total


def test_tile_shards_add_up_on_a_grid_seed(gpu, orc_sm):
    """tile_world = 2 over a 130 x 66 frame (3 x 2 tiles, clipped at both borders) of a grid fuzz scene: the two ranks' images add up to the unsharded frame bit for bit"""
    w, h = 130, 66
    d = scene_of(GRID_SEED, w, h).desc
    assert d.n_volume_grids == 1
    scene = gpu.Scene(d, flatten=True)
    tables = orc_sm.sequence_tables(1)

    def run(rank, world):
        tr = tracer(gpu, "wavefront", w, h)
        tr.setTileShard(rank, world)
        return frame(gpu, tr, scene, w, h, tables)
    full = run(0, 1)
    parts = run(0, 2) + run(1, 2)
    assert full[..., :3].any()
    assert np.array_equal(parts.view(np.uint32), full.view(np.uint32)), (parts != full).any(axis=2).sum()
