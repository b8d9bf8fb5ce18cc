"""Heterogeneous media on the device: ctl_volume_eval in a kernel against the host yardstick bit for bit, every code on the four grid sets; PathTracer frames of
scenes.smoke_box — the k_path_trace_media_grid kernel — against the per-pixel restatement tests/volume_grid_ref.path_trace; ctl_tracer_debug_pixel; a constant grid
against the homogeneous medium of the same coefficients; in-place updates of the grid records and their cells; the plugins that refuse media."""
import numpy as np
import pytest

import volume_ref
import volume_grid_ref
from cudatracerlib_amd import api, scenes
from volume_grid_cases import SETS, make_set, queries, same_rows, FUNCTIONS

pytestmark = pytest.mark.gpu
W, H = 24, 16
MAX_LEN, RR = 4, 2
# the density scale, chosen from the restatement alone (the box is ~550 units deep, the mean density ~0.5: an optical depth near 1 along a camera ray) so that at least
# a quarter of the pixels have a medium vertex — asserted where the frames are made
SIGMA_A, SIGMA_S = 0.0005, 0.004
VARIANTS = {"single": dict(dims=(3, 4, 5)), "three_grids": dict(three_grid_dims=((2, 3, 2), (4, 2, 3)))}
_memo = {}


def smoke(variant, **kw):
    return scenes.smoke_box(W, H, sigma_a=SIGMA_A, sigma_s=SIGMA_S, **dict(VARIANTS[variant], **kw))


def tables_of(orc):
    if "tables" not in _memo:
        _memo["tables"] = orc.sequence_tables(1)
    return _memo["tables"]


def gpu_frame(gpu, scene, tables, direct=True):
    tr = gpu.PathTracer()
    p = tr.getParameters(); p.setValue("Direct", direct); p.setValue("MaxPathLength", MAX_LEN); p.setValue("RRStartDepth", RR)
    tr.Resize(W, H); tr.InitializeScene(scene)
    img = gpu.Image(W, H)
    for k in range(len(tables)):
        tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == 0))
    return img.getPixelData(), tr


@pytest.mark.parametrize("what", sorted(FUNCTIONS))
def test_volume_eval_device_equals_host(gpu, what):
    """ctl_volume_eval(on_device = 1) equals on_device = 0 bit for bit, NaN for NaN, for every `what`, old and new, on the four grid sets: the queries of the host test"""
    for name in SETS:
        vols = make_set(name)
        d = api.volumes_desc(vols)
        q = queries(name, vols, what)
        host = api.volume_eval(d, what, q, on_device=False)
        dev = api.volume_eval(d, what, q, on_device=True)
        bad = same_rows(dev, host)
        assert not bad, "%s on set %s: %d of %d rows differ, first %s\ndevice %s\n  host %s\n query %s" % (FUNCTIONS[what], name, len(bad), len(q), bad[0], dev[bad[0]], host[bad[0]], q[bad[0]])


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "no_direct"])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_smoke_box_frames_against_the_restatement(gpu, orc, variant, direct):
    """PathTracer frames of smoke_box(24, 16) — the single 3 x 4 x 5 grid and the three-grid form — 1 pass with recorded tables, MaxPathLength 4, RRStartDepth 2, against
    volume_grid_ref.path_trace over the product's flattened tree.  Bars as tests/test_gpu_volume.py: weightSum equal in every pixel, >= 98 % of the pixels bit-equal,
    frame mean within 2e-3, ray count within 1e-2.  The restatement's march never reaches its step cap, in any pixel, and at least a quarter of the pixels have a
    medium vertex."""
    sc = smoke(variant); d = sc.desc
    tables = tables_of(orc)
    fb = api.FlatBvh(d, api.FLAT_Q4)
    rays, stats, vertices = [], {}, np.zeros((H, W), np.int64)
    want = volume_grid_ref.path_trace(orc, d, W, H, tables, stats=stats, vertices=vertices, direct=direct, max_path_length=MAX_LEN, rr_start=RR, flat=fb.desc, ray_count=rays)
    share = float((vertices > 0).mean())
    print("smoke_box %s direct=%s: restatement %s, %.0f %% of the pixels have a medium vertex" % (variant, direct, stats, 100 * share))
    assert stats["cap_hits"] == 0 and share >= 0.25, (stats, share)
    got, tr = gpu_frame(gpu, gpu.Scene(d, flatten=True), tables, direct=direct)
    g, w = got[..., :3], want[..., :3]
    exact = (g.view(np.uint32) == w.view(np.uint32)).all(axis=2).mean()
    print("smoke_box %s direct=%s: %.2f %% of pixels bit-equal, mean %g vs %g, rays %d vs %d" % (variant, direct, 100 * exact, g.mean(), w.mean(), tr.stats().rays_total, rays[0]))
    assert np.array_equal(got[..., 6], want[..., 6]), "weightSum differs"
    assert exact >= 0.98, exact
    assert abs(float(g.mean()) - float(w.mean())) <= 2e-3 * float(w.mean())
    assert abs(tr.stats().rays_total - rays[0]) <= 1e-2 * rays[0]


def test_debug_pixel_against_the_restatement(gpu, orc):
    """ctl_tracer_debug_pixel on three pixels whose unjittered path scatters in the grid (found from the restatement alone, scanning the frame's middle rows): bit-equal"""
    sc = smoke("single"); d = sc.desc
    scene = gpu.Scene(d, flatten=True)
    fb = api.FlatBvh(d, api.FLAT_Q4)
    tables = orc.sequence_tables(1)
    pixels, want = [], []
    for (x, y) in [(x, y) for y in (8, 5, 11) for x in range(3, W - 3, 2)]:
        stats = {}
        r = volume_grid_ref.path_trace(orc, d, W, H, tables, stats=stats, max_path_length=MAX_LEN, rr_start=RR, flat=fb.desc, debug_pixels=[(x, y)])
        assert stats["cap_hits"] == 0
        if stats["scatters"] > 0 and r[0].any():
            pixels.append((x, y)); want.append(r[0])
        if len(pixels) == 3:
            break
    assert len(pixels) == 3, pixels
    img = gpu.Image(W, H)
    for (x, y), wv in zip(pixels, want):
        tr = gpu.PathTracer(); p = tr.getParameters(); p.setValue("MaxPathLength", MAX_LEN); p.setValue("RRStartDepth", RR)
        tr.Resize(W, H); tr.InitializeScene(scene)
        got = tr.Debug(img, x, y)
        print("debug pixel", (x, y), got, wv)
        assert np.array_equal(got.view(np.uint32), wv.view(np.uint32)), (x, y, got, wv)


def _const_pair():
    """a constant 8 x 8 x 8 grid over the scene box and the homogeneous region of the same coefficients (sigma * density)"""
    c = 0.75
    grid = scenes.smoke_box(W, H, dims=(8, 8, 8), sigma_a=SIGMA_A, sigma_s=SIGMA_S)
    gv = api.grid_volume(np.array(list(grid.volume.volume.volume_to_world.m), np.float32).reshape(4, 4), density=np.full((8, 8, 8), c, np.float32), sig_a=(0.0, SIGMA_A), sig_s=(0.0, SIGMA_S))
    sc = scenes.cornell_box(W, H); sc.CreateGridVolume(gv); sc.UpdateScene()
    hom = scenes.fog_box(W, H, sigma_a=SIGMA_A * c, sigma_s=SIGMA_S * c)
    return sc, hom


def test_constant_grid_against_the_homogeneous_medium(gpu, orc):
    """a constant grid against the homogeneous region of the same coefficients.  The frames are not bit-equal and not the same estimator: the grid samples without a
    medium sampling weight, its march takes d_a from the overwritten d_s, and sampleTrilinear's weights fall off over the half cell at the low faces.  The device's
    relative difference of the two frame means must lie within the restatement's own, measured here on its two frames, times 2 (for the device's 2 % of differing
    pixels)"""
    g_sc, h_sc = _const_pair()
    tables = tables_of(orc)
    ref_g = volume_grid_ref.path_trace(orc, g_sc.desc, W, H, tables, max_path_length=MAX_LEN, rr_start=RR, flat=api.FlatBvh(g_sc.desc, api.FLAT_Q4).desc)[..., :3]
    ref_h = volume_ref.path_trace(orc, h_sc.desc, [h_sc.desc.volumes[0]], W, H, tables, max_path_length=MAX_LEN, rr_start=RR, flat=api.FlatBvh(h_sc.desc, api.FLAT_Q4).desc)[..., :3]
    margin = abs(float(ref_g.mean()) - float(ref_h.mean())) / float(ref_h.mean())
    dev_g, _ = gpu_frame(gpu, gpu.Scene(g_sc.desc, flatten=True), tables)
    dev_h, _ = gpu_frame(gpu, gpu.Scene(h_sc.desc, flatten=True), tables)
    diff = abs(float(dev_g[..., :3].mean()) - float(dev_h[..., :3].mean())) / float(dev_h[..., :3].mean())
    print("constant grid vs homogeneous: restatement means %g / %g (relative difference %g), device means %g / %g (relative difference %g)"
          % (ref_g.mean(), ref_h.mean(), margin, dev_g[..., :3].mean(), dev_h[..., :3].mean(), diff))
    for name, dev, ref in (("grid", dev_g, ref_g), ("homogeneous", dev_h, ref_h)):   # (for the record: the frame means are carried by a few bright pixels)
        print("  %s: %.2f %% of the device's pixels bit-equal to the restatement's" % (name, 100 * (dev[..., :3].view(np.uint32) == ref.view(np.uint32)).all(axis=2).mean()))
    assert not np.array_equal(dev_g, dev_h)
    assert diff <= 2 * margin, (diff, margin)


def test_in_place_grid_update(gpu, orc):
    """ctl_scene_update through homogeneous -> grid -> other cells -> bigger dims -> none -> homogeneous: each mask is CTL_DIFF_VOLUMES alone with no refit, and each
    next frame is bit-equal to the frame of a scene created fresh from the new description; the homogeneous fog_box frame of the scene that once held a grid is
    bit-equal to a fresh one"""
    tables = tables_of(orc)
    fog = scenes.fog_box(W, H, sigma_a=SIGMA_A, sigma_s=SIGMA_S)
    plain = scenes.cornell_box(W, H)
    steps = [("grid", smoke("single")), ("other cells", smoke("single", seed=11)), ("bigger dims", smoke("single", dims=(6, 7, 9))), ("three grids", smoke("three_grids")),
             ("none", plain), ("grid again", smoke("single")), ("homogeneous", fog)]
    s = gpu.Scene(fog.desc, flatten=True)
    last, _ = gpu_frame(gpu, s, tables)
    fog_fresh = last
    for name, sc in steps:
        fresh, _ = gpu_frame(gpu, gpu.Scene(sc.desc, flatten=True), tables)
        assert s.update(sc.desc) == api.DIFF_VOLUMES, name
        assert s.update_stats()["refit_levels"] == 0, name
        frame, _ = gpu_frame(gpu, s, tables)
        assert np.array_equal(frame.view(np.uint32), fresh.view(np.uint32)), name
        assert not np.array_equal(frame, last), name
        assert s.update(sc.desc) == 0, name
        last = frame
    assert np.array_equal(last.view(np.uint32), fog_fresh.view(np.uint32))


def test_plugins_that_refuse_grids(gpu):
    """WavefrontPathTracer, PrimTracer and Regularization = true answer CTL_ERR_UNSUPPORTED for a scene whose only medium is a grid"""
    sc = smoke("single")
    smoky = gpu.Scene(sc.desc, flatten=True)
    for kind in ("wavefront", "prim", "regularization"):
        tr = {"wavefront": gpu.WavefrontPathTracer, "prim": gpu.PrimTracer, "regularization": gpu.PathTracer}[kind]()
        if kind == "regularization":
            tr.getParameters().setValue("Regularization", True)
        tr.Resize(W, H)
        with pytest.raises(gpu.CtlError, match="PathTracer") as e:
            tr.InitializeScene(smoky)
        assert e.value.code == -5, kind
