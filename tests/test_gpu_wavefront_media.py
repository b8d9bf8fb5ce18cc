"""Participating media in the WavefrontPathTracer plugin (tracer parameter ParticipatingMedia = true): k_medium_stage (csrc/medium_stage.hip) in front of the media
build of the shade kernel (csrc/shade_full_media*.hip), held to the yardsticks of the PathTracer plugin's media —

  * the per-pixel restatements tests/volume_ref.path_trace and tests/volume_grid_ref.path_trace over the product's flattened tree, under the bars of
    tests/test_gpu_volume.py and tests/test_gpu_volume_grid.py (weightSum equal in every pixel, >= 98 % of the pixels bit-equal, frame mean within 2e-3 relative, ray
    count within 1 %);
  * the reference's own PathTrace, tests/golden/pathtrace_media.npz, under the four conditions of tests/test_gpu_volume_golden.py;

and to itself: batches against single passes, tile shards against the whole frame, in-place volume updates against fresh scenes, a scene without media against the
parameter switched off, bit for bit; what the plugin refuses.  The scenes, sizes and parameters are those of the PathTracer tests mirrored."""
import os
import sys

import numpy as np
import pytest

import volume_ref
import volume_grid_ref
import test_gpu_volume as TV
import test_gpu_volume_grid as TG
from cudatracerlib_amd import api, scenes

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_memo = {}


def _generate():
    sys.path.insert(0, G)
    import generate
    return generate


def wavefront(gpu, w, h, max_len, rr, direct=True, media=True, **params):
    tr = gpu.WavefrontPathTracer()
    p = tr.getParameters()
    p.setValue("Direct", direct); p.setValue("MaxPathLength", max_len); p.setValue("RRStartDepth", rr); p.setValue("ParticipatingMedia", media)
    for k, v in params.items():
        p.setValue(k, v)
    tr.Resize(w, h)
    return tr


def frame(gpu, tr, scene, w, h, tables, initialize=True):
    if initialize:
        tr.InitializeScene(scene)
    img = gpu.Image(w, h)
    for k in range(len(tables)):
        tr.setSamplerTables(*tables[k]); tr.DoPass(img, new_trace=(k == 0))
    return img.getPixelData()


def fog_restatement(orc_sm, medium, w, h, direct, first):
    """volume_ref.path_trace of fog_box with the medium `medium`, table sets first, first + 1 of a fresh generator: computed once per module, read by every test that needs it"""
    key = ("fog", medium, w, h, direct, first)
    if key not in _memo:
        generate = _generate()
        m = TV.MEDIA[medium]
        sc = scenes.fog_box(w, h, sigma_a=m["sigma_a"], sigma_s=m["sigma_s"], phase=api.phase_hg(m["phase"][1]) if m["phase"] else None, fraction=m["fraction"])
        d = sc.desc
        tables = generate.pathtrace_media_tables(first)
        rays = []
        fb = api.FlatBvh(d, api.FLAT_Q4)
        want = volume_ref.path_trace(orc_sm, d, [d.volumes[0]], w, h, tables, direct=direct, max_path_length=TV.MAX_LEN, rr_start=TV.RR, flat=fb.desc, ray_count=rays)
        want.setflags(write=False)
        _memo[key] = (want, rays[0])
    return _memo[key]


def hold_to_restatement(name, got, want, rays_got, rays_want):
    g, w = got[..., :3], want[..., :3]
    exact = (g.view(np.uint32) == w.view(np.uint32)).all(axis=2).mean()
    print("%s: %.2f %% of pixels bit-equal, mean %g vs %g, rays %d vs %d" % (name, 100 * exact, g.mean(), w.mean(), rays_got, rays_want))
    assert np.array_equal(got[..., 6], want[..., 6]), "weightSum differs"
    assert exact >= 0.98, exact
    assert abs(float(g.mean()) - float(w.mean())) <= 2e-3 * float(w.mean())
    assert abs(rays_got - rays_want) <= 1e-2 * rays_want


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "no_direct"])
@pytest.mark.parametrize("medium", sorted(TV.MEDIA))
def test_fog_box_frames_against_the_restatement(gpu, orc_sm, medium, direct):
    """the four media of tests/test_gpu_volume.py, fog_box(48, 32), Direct on and off, 2 passes with the oracle's recorded tables (the first two sets of a fresh
    generator), MaxPathLength 6, RRStartDepth 3: the wavefront's frame against volume_ref.path_trace under that file's bars"""
    assert (TV.W, TV.H, TV.MAX_LEN, TV.RR) == (48, 32, 6, 3)
    want, rays = fog_restatement(orc_sm, medium, TV.W, TV.H, direct, 0)
    tables = orc_sm.sequence_tables(2)
    tr = wavefront(gpu, TV.W, TV.H, TV.MAX_LEN, TV.RR, direct)
    sc = TV.fog(medium)   # (the builder owns the arrays its description points at)
    got = frame(gpu, tr, gpu.Scene(sc.desc, flatten=True), TV.W, TV.H, tables)
    hold_to_restatement("wavefront fog_box %s direct=%s" % (medium, direct), got, want, tr.stats().rays_total, rays)


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "no_direct"])
@pytest.mark.parametrize("variant", sorted(TG.VARIANTS))
def test_smoke_box_frames_against_the_restatement(gpu, orc_sm, variant, direct):
    """both variants of smoke_box(24, 16) of tests/test_gpu_volume_grid.py (MaxPathLength 4, RRStartDepth 2, 1 pass), Direct on and off — k_medium_stage<true> and
    k_shade_full_media_grid — against volume_grid_ref.path_trace under the same bars; the restatement's march never reaches its step cap"""
    assert (TG.W, TG.H, TG.MAX_LEN, TG.RR) == (24, 16, 4, 2)
    sc = TG.smoke(variant); d = sc.desc
    tables = orc_sm.sequence_tables(1)
    rays, stats, vertices = [], {}, np.zeros((TG.H, TG.W), np.int64)
    fb = api.FlatBvh(d, api.FLAT_Q4)
    want = volume_grid_ref.path_trace(orc_sm, d, TG.W, TG.H, tables, stats=stats, vertices=vertices, direct=direct, max_path_length=TG.MAX_LEN, rr_start=TG.RR, flat=fb.desc, ray_count=rays)
    share = float((vertices > 0).mean())
    assert stats["cap_hits"] == 0 and share >= 0.25, (stats, share)
    tr = wavefront(gpu, TG.W, TG.H, TG.MAX_LEN, TG.RR, direct)
    got = frame(gpu, tr, gpu.Scene(d, flatten=True), TG.W, TG.H, tables)
    hold_to_restatement("wavefront smoke_box %s direct=%s" % (variant, direct), got, want, tr.stats().rays_total, rays[0])


def _outside(img, rgb):
    return (np.abs(img[..., :3] - rgb) > 2e-3 * (1 + np.abs(rgb))).any(axis=2)


@pytest.mark.parametrize("key", [c[0] for c in _generate().pathtrace_media_cases() if not c[0].startswith("clear")])
def test_against_the_references_own_path_trace(gpu, orc_sm, key):
    """every media case of tests/golden/pathtrace_media.npz (PathTrace<DIRECT> run by the reference's own code) rendered by the wavefront plugin, under the four
    conditions of tests/test_gpu_volume_golden.py: weightSum equal in every pixel, >= 99 % of the pixels within 2e-3 (1 + |ref|), the frame mean within 2e-3 relative,
    and at most ONE pixel more outside the tolerance than the shared-math restatement"""
    generate = _generate()
    frames = _memo.setdefault("frames", np.load(os.path.join(G, "pathtrace_media.npz")))
    _, make, w, h, direct, first = next(c for c in generate.pathtrace_media_cases() if c[0] == key)
    sc = make(); d = sc.desc
    tables = generate.pathtrace_media_tables(first)
    assert generate.pathtrace_media_digest(d, tables) == str(frames[key + "_digest"]), "regenerate tests/golden/pathtrace_media.npz"
    tr = wavefront(gpu, w, h, generate.MEDIA_MAX_PATH_LENGTH, generate.MEDIA_RR_START, direct)
    got = frame(gpu, tr, gpu.Scene(d, flatten=True), w, h, tables)
    rgb, weight = frames[key + "_rgb"], frames[key + "_weight"]
    medium = key.rsplit("_", 1)[0]
    if medium in TV.MEDIA and (generate.MEDIA_MAX_PATH_LENGTH, generate.MEDIA_RR_START) == (TV.MAX_LEN, TV.RR):   # a fog_box case: the restatement the first test reads, where the tables agree
        sm = fog_restatement(orc_sm, medium, w, h, direct, first)[0]
    else:
        fb = api.FlatBvh(d, api.FLAT_Q4)
        sm = volume_ref.path_trace(orc_sm, d, generate.media_volumes(d), w, h, tables, direct=direct, max_path_length=generate.MEDIA_MAX_PATH_LENGTH, rr_start=generate.MEDIA_RR_START, flat=fb.desc)
    out_gpu, out_sm = _outside(got, rgb), _outside(sm, rgb)
    frac = 1.0 - out_gpu.mean()
    print("%s wavefront: within tolerance GPU %.4f, shared-math restatement %.4f" % (key, frac, 1.0 - out_sm.mean()))
    assert out_gpu.sum() <= out_sm.sum() + 1, (out_gpu.sum(), out_sm.sum())
    assert np.array_equal(got[..., 6], weight), "weightSum differs in %d pixels" % (got[..., 6] != weight).sum()
    assert frac >= 0.99, frac
    assert abs(got[..., :3].mean() - rgb.mean()) <= 2e-3 * rgb.mean()


def test_a_batch_equals_its_passes_one_at_a_time(gpu, orc_sm):
    """PassBatch = 2 over two recorded table sets — the first two of a fresh tracer's own stream, which the batch draws itself — against the same two sets handed in
    and rendered one pass per launch: bit-equal (the medium stage reads each path's pass-in-batch for its tables and deposits finished paths in the ordered
    accumulation's stage, which adds them in pass order)"""
    tables = orc_sm.sequence_tables(2)
    sc = TV.fog("hg_coloured")
    scene = gpu.Scene(sc.desc, flatten=True)
    single = wavefront(gpu, TV.W, TV.H, TV.MAX_LEN, TV.RR, PassBatch=1)
    one = frame(gpu, single, scene, TV.W, TV.H, tables)
    tr = wavefront(gpu, TV.W, TV.H, TV.MAX_LEN, TV.RR, PassBatch=2)
    tr.InitializeScene(scene)
    img = gpu.Image(TV.W, TV.H)
    tr.DoPasses(img, 2, new_trace=True)
    both = img.getPixelData()
    assert one[..., :3].any() and (one[..., 6] == 2).mean() > 0.9
    assert np.array_equal(both.view(np.uint32), one.view(np.uint32)), (both.view(np.uint32) != one.view(np.uint32)).any(axis=2).sum()
    assert single.stats().rays_total == tr.stats().rays_total


def test_tile_shards_add_up_to_the_frame(gpu, orc_sm):
    """tile_world = 2 on a frame of more than one 64 x 64 tile (130 x 66: 3 x 2 tiles, clipped at both borders), the isotropic medium: the two ranks' images added
    together equal the unsharded frame bit for bit (disjoint tiles; a sample that strays over a tile border is one float addition to a zero)"""
    w, h = 130, 66
    m = TV.MEDIA["isotropic"]
    sc = scenes.fog_box(w, h, sigma_a=m["sigma_a"], sigma_s=m["sigma_s"])
    scene = gpu.Scene(sc.desc, flatten=True)
    tables = orc_sm.sequence_tables(1)

    def run(rank, world):
        tr = wavefront(gpu, w, h, TV.MAX_LEN, TV.RR)
        tr.setTileShard(rank, world)
        return frame(gpu, tr, scene, w, h, tables)
    full = run(0, 1)
    parts = run(0, 2) + run(1, 2)
    assert full[..., :3].any()
    assert np.array_equal(parts.view(np.uint32), full.view(np.uint32)), (parts != full).any(axis=2).sum()


def test_media_arrive_and_leave_by_update(gpu, orc_sm):
    """a scene created without volumes, InitializeScene with the parameter on; update() to the hg_coloured description: the next frame is bit-equal to the frame of a
    scene created foggy — no re-initialising; update back: bit-equal to the clear frame"""
    tables = orc_sm.sequence_tables(1)
    plain = scenes.cornell_box(TV.W, TV.H); foggy = TV.fog("hg_coloured")
    fresh = frame(gpu, wavefront(gpu, TV.W, TV.H, TV.MAX_LEN, TV.RR), gpu.Scene(foggy.desc, flatten=True), TV.W, TV.H, tables)
    s = gpu.Scene(plain.desc, flatten=True)
    tr = wavefront(gpu, TV.W, TV.H, TV.MAX_LEN, TV.RR)
    clear = frame(gpu, tr, s, TV.W, TV.H, tables)
    assert s.update(foggy.desc) == api.DIFF_VOLUMES
    after = frame(gpu, tr, s, TV.W, TV.H, tables, initialize=False)
    assert np.array_equal(after.view(np.uint32), fresh.view(np.uint32)) and not np.array_equal(after, clear)
    assert s.update(plain.desc) == api.DIFF_VOLUMES
    back = frame(gpu, tr, s, TV.W, TV.H, tables, initialize=False)
    assert np.array_equal(back.view(np.uint32), clear.view(np.uint32))


@pytest.mark.parametrize("which", ["cornell", "bathroom"])
def test_a_scene_without_media_renders_as_with_the_parameter_off(gpu, orc_sm, which):
    """an empty volume table: the pass launches today's kernels — the Cornell box (k_shade_basic) and a full-feature scene (the model-class builds), parameter on
    against off, bit for bit, and as many rays"""
    w, h = 64, 48
    sc = scenes.cornell_box(w, h, glass_sphere=True) if which == "cornell" else scenes.synthetic_bathroom(w, h, n_instances=12, subdiv=1)
    scene = gpu.Scene(sc.desc, flatten=True)
    tables = orc_sm.sequence_tables(2)
    out = {}
    for media in (False, True):
        tr = wavefront(gpu, w, h, 5, 3, media=media)
        out[media] = (frame(gpu, tr, scene, w, h, tables), tr.stats().rays_total)
    assert out[True][0][..., :3].any()
    assert np.array_equal(out[True][0].view(np.uint32), out[False][0].view(np.uint32)) and out[True][1] == out[False][1]


def test_refusals(gpu):
    """the parameter's default is false; with it on, PathSemantics = Wavefront is refused with ERR_UNSUPPORTED at InitializeScene and at DoPass after the parameter is
    flipped; a default-constructed tracer still refuses a foggy scene"""
    fog_sc = TV.fog("isotropic"); clear_sc = scenes.cornell_box(TV.W, TV.H)   # the builders own the arrays the descriptions point at
    foggy = gpu.Scene(fog_sc.desc, flatten=True)
    clear = gpu.Scene(clear_sc.desc, flatten=True)
    tr = gpu.WavefrontPathTracer()
    assert tr.getParameters().getValue("ParticipatingMedia") == 0
    tr.Resize(TV.W, TV.H)
    with pytest.raises(gpu.CtlError, match="PathTracer") as e:
        tr.InitializeScene(foggy)
    assert e.value.code == api.ERR_UNSUPPORTED
    for scene in (foggy, clear):
        tr = wavefront(gpu, TV.W, TV.H, TV.MAX_LEN, TV.RR, PathSemantics="Wavefront")
        with pytest.raises(gpu.CtlError, match="ParticipatingMedia = true with PathSemantics = Wavefront") as e:
            tr.InitializeScene(scene)
        assert e.value.code == api.ERR_UNSUPPORTED
    tr = wavefront(gpu, TV.W, TV.H, TV.MAX_LEN, TV.RR)
    tr.InitializeScene(foggy)
    img = gpu.Image(TV.W, TV.H)
    tr.DoPass(img, new_trace=True)
    assert img.getPixelData()[..., :3].any()
    tr.getParameters().setValue("PathSemantics", "Wavefront")
    with pytest.raises(gpu.CtlError, match="ParticipatingMedia = true with PathSemantics = Wavefront") as e:
        tr.DoPass(img, new_trace=True)
    assert e.value.code == api.ERR_UNSUPPORTED
    tr.getParameters().setValue("PathSemantics", "PathTrace"); tr.getParameters().setValue("ParticipatingMedia", False)
    with pytest.raises(gpu.CtlError, match="PathTracer") as e:   # switched off over a foggy scene: today's refusal when the pass starts
        tr.DoPass(img, new_trace=True)
    assert e.value.code == api.ERR_UNSUPPORTED
