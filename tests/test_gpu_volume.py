"""Participating media on the device: ctl_volume_eval in a kernel against the host yardstick bit for bit; PathTracer frames of scenes.fog_box against the per-pixel
restatement tests/volume_ref.path_trace (which tests/test_volume_host.py pins on the oracle's render and on the host yardstick); ctl_tracer_debug_pixel; in-place
updates of the volume table; the plugins that refuse media.
The restatement itself is pinned on the reference's own Volumes.cu / PhaseFunction.cu / PathTrace by tests/test_oracle_volume.py (tests/golden/volumes.npz,
pathtrace_media.npz), and tests/test_gpu_volume_golden.py holds the device to those fixtures directly."""
import numpy as np
import pytest

import volume_ref
from cudatracerlib_amd import api, scenes
from volume_cases import SETS, make_set, queries, same_rows, FUNCTIONS

pytestmark = pytest.mark.gpu
W, H = 48, 32
MAX_LEN, RR = 6, 3   # RRStartDepth = 3: roulette runs after a medium vertex, with the stale specularBounce

MEDIA = {   # sigma_a, sigma_s, phase, fraction of the scene box
    "absorbing": dict(sigma_a=0.0012, sigma_s=0.0, phase=None, fraction=(1, 1, 1)),
    "isotropic": dict(sigma_a=0.0005, sigma_s=0.002, phase=None, fraction=(1, 1, 1)),                      # albedo 0.8
    "hg_coloured": dict(sigma_a=(0.0004, 0.0008, 0.0002), sigma_s=(0.0012, 0.002, 0.003), phase=("hg", 0.7), fraction=(1, 1, 1)),
    "half_box": dict(sigma_a=0.0005, sigma_s=0.002, phase=None, fraction=(1, 0.5, 1)),
}
_memo = {}


def fog(name):
    m = MEDIA[name]
    phase = api.phase_hg(m["phase"][1]) if m["phase"] else None
    return scenes.fog_box(W, H, sigma_a=m["sigma_a"], sigma_s=m["sigma_s"], phase=phase, fraction=m["fraction"])


def tables_of(orc):
    if "tables" not in _memo:
        _memo["tables"] = orc.sequence_tables(2)
    return _memo["tables"]


def gpu_frame(gpu, scene, tables, direct=True, new_tracer=None):
    tr = new_tracer or gpu.PathTracer()
    p = tr.getParameters(); p.setValue("Direct", direct); p.setValue("MaxPathLength", MAX_LEN); p.setValue("RRStartDepth", RR)
    tr.Resize(W, H); tr.InitializeScene(scene)
    img = gpu.Image(W, H)
    for k in range(len(tables)):
        tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == 0))
    return img.getPixelData(), tr


@pytest.mark.parametrize("what", sorted(FUNCTIONS))
def test_volume_eval_device_equals_host(gpu, what):
    """ctl_volume_eval(on_device = 1) equals on_device = 0 bit for bit, NaN for NaN, on the queries of the host test: 1024 seeded rows per volume set — 4096 per
    function — plus the branch points"""
    for name in SETS:
        vols = make_set(name)
        d = api.volumes_desc(vols)
        q = queries(name, vols, what, 1024)
        host = api.volume_eval(d, what, q, on_device=False)
        dev = api.volume_eval(d, what, q, on_device=True)
        bad = same_rows(dev, host)
        assert not bad, "%s on set %s: %d of %d rows differ, first %s\ndevice %s\n  host %s\n query %s" % (FUNCTIONS[what], name, len(bad), len(q), bad[0], dev[bad[0]], host[bad[0]], q[bad[0]])


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "no_direct"])
@pytest.mark.parametrize("medium", sorted(MEDIA))
def test_fog_box_frames_against_the_restatement(gpu, orc, medium, direct):
    """PathTracer frames of fog_box(48, 32), 2 passes with recorded tables, MaxPathLength 6, RRStartDepth 3, against volume_ref.path_trace over the product's flattened
    tree.  Bars as tests/test_gpu_render.py (the same two arithmetic paths): weightSum equal in every pixel, >= 98 % of the pixels bit-equal, frame mean within 2e-3."""
    sc = fog(medium); d = sc.desc
    tables = tables_of(orc)
    fb = api.FlatBvh(d, api.FLAT_Q4)
    rays = []
    want = volume_ref.path_trace(orc, d, [d.volumes[0]], W, H, tables, direct=direct, max_path_length=MAX_LEN, rr_start=RR, flat=fb.desc, ray_count=rays)
    got, tr = gpu_frame(gpu, gpu.Scene(d, flatten=True), tables, direct=direct)
    g, w = got[..., :3], want[..., :3]
    exact = (g.view(np.uint32) == w.view(np.uint32)).all(axis=2).mean()
    print("fog_box %s direct=%s: %.2f %% of pixels bit-equal, mean %g vs %g, rays %d vs %d" % (medium, direct, 100 * exact, g.mean(), w.mean(), tr.stats().rays_total, rays[0]))
    assert np.array_equal(got[..., 6], want[..., 6]), "weightSum differs"
    assert exact >= 0.98, exact
    assert abs(float(g.mean()) - float(w.mean())) <= 2e-3 * float(w.mean())
    assert abs(tr.stats().rays_total - rays[0]) <= 1e-2 * rays[0]   # the medium vertex's shadow rays are counted like the others (a flipped decision changes a path's length)


def test_debug_pixel_against_the_restatement(gpu, orc):
    """ctl_tracer_debug_pixel (PathTracer::DebugInternal: Direct on, the pixel's own position, the tracer's next table set) on three pixels against the restatement's
    unjittered path: equal, bit for bit"""
    sc = fog("isotropic"); d = sc.desc
    scene = gpu.Scene(d, flatten=True)
    fb = api.FlatBvh(d, api.FLAT_Q4)
    tables = orc.sequence_tables(1)   # the set a fresh tracer's generator draws first
    pixels = [(23, 10), (33, 18), (8, 26)]   # spread over the frame, chosen from the restatement alone among the pixels whose unjittered path carries radiance
    want = volume_ref.path_trace(orc, d, [d.volumes[0]], W, H, tables, max_path_length=MAX_LEN, rr_start=RR, flat=fb.desc, debug_pixels=pixels)
    img = gpu.Image(W, H)
    for (x, y), wv in zip(pixels, want):
        tr = gpu.PathTracer(); p = tr.getParameters(); p.setValue("MaxPathLength", MAX_LEN); p.setValue("RRStartDepth", RR)
        tr.Resize(W, H); tr.InitializeScene(scene)
        got = tr.Debug(img, x, y)
        print("debug pixel", (x, y), got, wv, "bit-equal" if np.array_equal(got.view(np.uint32), wv.view(np.uint32)) else "differs")
        assert np.array_equal(got.view(np.uint32), wv.view(np.uint32)), (x, y, got, wv)
    assert want.any(axis=1).all()


def test_in_place_volume_update(gpu, orc):
    """ctl_scene_update with other coefficients, and separately 0 -> 1 volumes: the mask is CTL_DIFF_VOLUMES alone and the next frame is bit-equal to the frame of a
    scene created from the new description"""
    tables = tables_of(orc)[:1]
    plain = scenes.cornell_box(W, H)
    a = fog("isotropic"); b = fog("hg_coloured")
    fresh, _ = gpu_frame(gpu, gpu.Scene(b.desc, flatten=True), tables)
    # other coefficients and another phase function
    s1 = gpu.Scene(a.desc, flatten=True)
    before, _ = gpu_frame(gpu, s1, tables)
    assert s1.update(b.desc) == api.DIFF_VOLUMES
    assert s1.update_stats()["refit_levels"] == 0   # no refit
    after, _ = gpu_frame(gpu, s1, tables)
    assert np.array_equal(after.view(np.uint32), fresh.view(np.uint32)) and not np.array_equal(after, before)
    # 0 -> 1 volumes: the table was allocated at creation
    s0 = gpu.Scene(plain.desc, flatten=True)
    clear, _ = gpu_frame(gpu, s0, tables)
    assert s0.update(b.desc) == api.DIFF_VOLUMES
    after0, _ = gpu_frame(gpu, s0, tables)
    assert np.array_equal(after0.view(np.uint32), fresh.view(np.uint32)) and not np.array_equal(after0, clear)
    # ... and back: 1 -> 0 is the frame of the scene without media
    assert s0.update(plain.desc) == api.DIFF_VOLUMES
    back, _ = gpu_frame(gpu, s0, tables)
    assert np.array_equal(back.view(np.uint32), clear.view(np.uint32))
    assert s0.update(plain.desc) == 0


def test_plugins_that_refuse_volumes(gpu, orc):
    """WavefrontPathTracer, PrimTracer and Regularization = true contain no medium code: InitializeScene answers CTL_ERR_UNSUPPORTED and names the PathTracer plugin
    (the reference would render the scene without its media); a scene without volumes is accepted by all three as before"""
    fog_sc = fog("isotropic"); clear_sc = scenes.cornell_box(W, H)   # the builders own the arrays the descriptions point at
    foggy = gpu.Scene(fog_sc.desc, flatten=True)
    clear_desc = clear_sc.desc
    assert clear_desc.n_volumes == 0
    clear = gpu.Scene(clear_desc, flatten=True)

    def make(kind):
        tr = {"wavefront": gpu.WavefrontPathTracer, "prim": gpu.PrimTracer, "regularization": gpu.PathTracer}[kind]()
        if kind == "regularization":
            tr.getParameters().setValue("Regularization", True)
        tr.Resize(W, H)
        return tr
    for kind in ("wavefront", "prim", "regularization"):
        tr = make(kind)
        with pytest.raises(gpu.CtlError, match="PathTracer") as e:
            tr.InitializeScene(foggy)
        assert e.value.code == -5, kind   # CTL_ERR_UNSUPPORTED
        tr = make(kind)
        tr.InitializeScene(clear)
        img = gpu.Image(W, H)
        tr.DoPass(img, new_trace=True)
        assert img.getPixelData()[..., :3].any(), kind
    # media that arrive by an update after InitializeScene are refused when the pass starts
    s = gpu.Scene(clear_desc, flatten=True)
    tr = make("wavefront"); tr.InitializeScene(s)
    assert s.update(fog_sc.desc) == api.DIFF_VOLUMES
    with pytest.raises(gpu.CtlError, match="PathTracer") as e:
        tr.DoPass(gpu.Image(W, H), new_trace=True)
    assert e.value.code == -5
    # Regularization switched on after InitializeScene of a foggy scene: refused at render time
    tr = gpu.PathTracer(); tr.Resize(W, H); tr.InitializeScene(foggy)
    tr.getParameters().setValue("Regularization", True)
    with pytest.raises(gpu.CtlError, match="PathTracer") as e:
        tr.DoPass(gpu.Image(W, H), new_trace=True)
    assert e.value.code == -5


def test_two_scenes_two_media_tables(gpu, orc):
    """every scene owns its volume table: two scenes with different homogeneous media (the sets `one` and `half` of volume_cases.py over the Cornell box, 16 x 16 pixels,
    one PathTracer each, 2 passes with recorded tables) render, alive together and passes interleaved, the bytes each renders alone; B still does after A is destroyed;
    the WavefrontPathTracer refuses either with ERR_UNSUPPORTED and today's message"""
    import gc
    import weakref
    w = h = 16
    tables = tables_of(orc)

    def box_with(name):
        sc = scenes.cornell_box(w, h)
        for v in make_set(name):
            sc.CreateVolume(v)
        sc.UpdateScene()
        return sc

    def tracer_for(scene):
        tr = gpu.PathTracer(); p = tr.getParameters(); p.setValue("MaxPathLength", MAX_LEN); p.setValue("RRStartDepth", RR)
        tr.Resize(w, h); tr.InitializeScene(scene)
        return tr

    def one_pass(tr, img, k):
        tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == 0))

    def alone(sc):
        scene = gpu.Scene(sc.desc, flatten=True); tr = tracer_for(scene); img = gpu.Image(w, h)
        for k in range(len(tables)):
            one_pass(tr, img, k)
        return img.getPixelData().copy()
    sa, sb = box_with("one"), box_with("half")
    assert sa.desc.n_volumes == sb.desc.n_volumes == 1
    want_a = alone(sa); gc.collect()
    want_b = alone(sb); gc.collect()
    assert not np.array_equal(want_a, want_b) and want_a[..., :3].any() and want_b[..., :3].any()
    A, B = gpu.Scene(sa.desc, flatten=True), gpu.Scene(sb.desc, flatten=True)
    ta, tb = tracer_for(A), tracer_for(B)
    ia, ib = gpu.Image(w, h), gpu.Image(w, h)
    for k in range(len(tables)):
        one_pass(ta, ia, k); one_pass(tb, ib, k)
    assert np.array_equal(ia.getPixelData().view(np.uint32), want_a.view(np.uint32)), "scene A beside scene B"
    assert np.array_equal(ib.getPixelData().view(np.uint32), want_b.view(np.uint32)), "scene B beside scene A"
    for scene in (A, B):
        wf = gpu.WavefrontPathTracer(); wf.Resize(w, h)
        with pytest.raises(gpu.CtlError, match=r"WavefrontPathTracer: the scene has participating media \(1 volumes\), which only the PathTracer plugin with Regularization = false renders") as e:
            wf.InitializeScene(scene)
        assert e.value.code == api.ERR_UNSUPPORTED
    gone = weakref.ref(A)
    del ta, A, wf, scene, e; gc.collect()
    assert gone() is None   # ctl_scene_destroy has run
    for k in range(len(tables)):
        one_pass(tb, ib, k)
    assert np.array_equal(ib.getPixelData().view(np.uint32), want_b.view(np.uint32)), "scene B after scene A was destroyed"
