"""ctl_scene_update on the device: the refit kernels against the host refit (byte for byte), the traversal of the updated scene against the oracle, the cheap
updates (camera, materials) against a freshly created scene (bit-equal frames), frames after a transform update against the oracle by the bars of
tests/test_gpu_render.py, and the refusals.  Scenes S1..S3 and motions M1..M3: tests/scene_update_cases.py."""
import ctypes as C

import numpy as np
import pytest

from cudatracerlib_amd import api
from scene_update_cases import SCENES, MOTIONS, build, rays_for_update, node_transforms

pytestmark = pytest.mark.gpu
W, H = 48, 48
CASES = [(s, m) for s in SCENES for m in MOTIONS]


def moved_nodes(old, new):
    return [k for k in range(new.n_nodes) if not np.array_equal(node_transforms(new)[k], node_transforms(old)[k])]


@pytest.mark.parametrize("scene,motion", CASES)
def test_device_refit_equals_the_host_refit(gpu, scene, motion):
    old, new = build(scene), build(scene, motion)
    s = gpu.Scene(old.desc, flatten=True)
    built = s.flat_bvh()
    host = api.FlatBvh(old.desc)
    assert np.array_equal(built.nodes(), host.nodes()) and np.array_equal(built.leaves(), host.leaves()) and np.array_equal(built.child_links(), host.child_links())   # the read-back un-stamps
    mask = s.update(new.desc)
    assert mask & api.DIFF_TRANSFORMS and not mask & api.DIFF_TOPOLOGY
    host.refit(new.desc)
    dev = s.flat_bvh()
    assert np.array_equal(dev.nodes(), host.nodes()), "nodes: %d of %d differ" % ((dev.nodes() != host.nodes()).any(axis=1).sum(), len(host.nodes()))
    assert np.array_equal(dev.leaves(), host.leaves())
    st = s.update_stats()
    assert st["node_area_before"] > 0 and st["node_area_after"] > 0 and st["refit_levels"] >= 2 and st["mask"] == mask
    print("%s %s: refit %.3f ms, %d levels, node area %.6g -> %.6g" % (scene, motion, st["refit_ms"], st["refit_levels"], st["node_area_before"], st["node_area_after"]))
    # a second update with the same description finds nothing to do and changes nothing
    assert s.update(new.desc) == 0 and np.array_equal(s.flat_bvh().nodes(), host.nodes())


def check_flat_updated(gpu, orc, scene, desc, rays, any_hit):
    """tests/test_gpu_intersect.py::check_flat restated for a scene that exists already: the flattened layout against the oracle's restatement of the
    reference's TWO-LEVEL traversal, bit for bit, equal-t ties excepted"""
    got = gpu.intersect(scene, rays, any_hit=any_hit)
    want = orc.intersect(desc, rays, any_hit=any_hit)
    if any_hit:   # which triangle is found first depends on the visiting order; occlusion itself must agree
        assert np.array_equal(got["tri_idx"] >= 0, want["tri_idx"] >= 0)
        return got
    for k in ("tri_idx", "node_idx"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert all(got["dist"][i] == want["dist"][i] for i in bad), (k, bad[:10])      # only rays that hit two triangles at the same t
        assert len(bad) <= len(rays) // 1000
    same = got["tri_idx"] == want["tri_idx"]
    for k in ("dist", "u", "v"):
        assert np.array_equal(got[k][same].view(np.uint32), want[k][same].view(np.uint32)), k
    assert (want["tri_idx"] >= 0).mean() > 0.2
    return got


@pytest.mark.parametrize("scene,motion", CASES)
def test_hits_of_the_updated_scene(gpu, orc, scene, motion):
    old, new = build(scene), build(scene, motion)
    s = gpu.Scene(old.desc, flatten=True)
    s.update(new.desc)
    moved = moved_nodes(old.desc, new.desc)
    rays = rays_for_update(new.desc, 30000, 29, aim_nodes=moved)
    got = check_flat_updated(gpu, orc, s, new.desc, rays, False)
    assert np.isin(got["node_idx"], moved).sum() > 20
    check_flat_updated(gpu, orc, s, new.desc, rays, True)
    # the two-level layout of the same update
    s2 = gpu.Scene(old.desc)
    assert s2.update(new.desc) & api.DIFF_TRANSFORMS
    check_flat_updated(gpu, orc, s2, new.desc, rays, False)
    check_flat_updated(gpu, orc, s2, new.desc, rays, True)


def tracers(gpu):
    def prim(mode):
        def make():
            t = gpu.PrimTracer(); t.getParameters().setValue("DrawingMode", mode); return t
        return make
    return (("WavefrontPathTracer", gpu.WavefrontPathTracer, 2), ("PathTracer", gpu.PathTracer, 2), ("PrimTracer n_geo_colored", prim("n_geo_colored"), 1), ("PrimTracer first_f_direct", prim("first_f_direct"), 1))


def render(gpu, make, scene, tables, n_passes, tr=None, max_len=5):
    if tr is None:
        tr = make()
        tr.getParameters().setValue("MaxPathLength", max_len)
        tr.Resize(W, H); tr.InitializeScene(scene)
    img = gpu.Image(W, H)
    for k in range(n_passes):
        tr.setSamplerTables(*tables[k])
        tr.DoPass(img, new_trace=(k == 0))
    return img.getPixelData(), tr


def assert_bit_equal(a, b, what):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "%s: %d of %d pixels differ" % (what, (a.view(np.uint32) != b.view(np.uint32)).any(axis=2).sum(), a.shape[0] * a.shape[1])


@pytest.mark.parametrize("change", ["camera", "material"])
def test_cheap_updates_render_like_a_fresh_scene(gpu, orc, change):
    """the tree is untouched by a camera or a material update, so nothing may differ from a scene created from the new description: every pixel bit-equal, for every
    tracer.  The material change turns the diffuse ball mesh into a metal (another bsdf_type: the entries' model nibble is re-stamped)."""
    old = build("S3", width=W, height=H)
    if change == "camera":
        new = build("S3", width=W, height=H, edit=lambda sc: sc.setCamera((120, 330, -700), (300, 250, 100), (0, 1, 0), 45.0, W, H))
        want_mask = api.DIFF_CAMERA
    else:
        new = build("S3", width=W, height=H, ball_material=api.conductor(eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14)))
        want_mask = api.DIFF_MATERIALS
    tables = orc.sequence_tables(2)
    for name, make, n_passes in tracers(gpu):
        s = gpu.Scene(old.desc, flatten=True)
        before, tr = render(gpu, make, s, tables, n_passes)
        assert s.update(new.desc) == want_mask
        assert s.update_stats()["restamped"] == (1 if change == "material" else 0)
        got, _ = render(gpu, make, s, tables, n_passes, tr=tr)
        want, _ = render(gpu, make, gpu.Scene(new.desc, flatten=True), tables, n_passes)
        assert_bit_equal(got, want, "%s after a %s update" % (name, change))
        assert not np.array_equal(got, before) or (change == "material" and "n_geo" in name), name   # (geometric normals do not depend on a material)
        a, b = s.flat_bvh(), api.FlatBvh(new.desc)                  # the tree itself was not touched
        assert np.array_equal(a.leaves(), b.leaves()) and np.array_equal(a.nodes(), b.nodes())


def close_to_oracle(got, want, exact_min=0.98):
    """the bars of tests/test_gpu_render.py::assert_close"""
    assert np.array_equal(got[..., 6], want[..., 6]), "weightSum differs"
    g, w = got[..., :3], want[..., :3]
    frac = (np.abs(g - w) <= 2e-3 * (1 + np.abs(w))).all(axis=2).mean()
    exact = (g == w).all(axis=2).mean()
    print("within tolerance %.5f, bit-equal %.5f" % (frac, exact))
    assert frac >= 0.9995, frac
    assert exact >= exact_min, exact


@pytest.mark.parametrize("flatten", [True, False])
def test_frames_after_a_transform_update(gpu, orc, flatten):
    """render A, update with M2 (a ball and the emissive panel turn and stretch: the area light's shape set and CDF move with it), new_trace, render B: B is the
    oracle's frame of the new description — traversing the refitted tree the device holds, or the two-level layout"""
    old, new = build("S3", width=W, height=H), build("S3", "M2", width=W, height=H)
    tables = orc.sequence_tables(2)
    s = gpu.Scene(old.desc, flatten=flatten)
    a, tr = render(gpu, gpu.WavefrontPathTracer, s, tables, 2)
    fa = s.flat_bvh() if flatten else None
    want_a, _ = orc.render(old.desc, W, H, n_passes=2, tables=tables, max_path_length=5, **({"flat": fa.desc} if flatten else {}))
    close_to_oracle(a, want_a)
    assert s.update(new.desc) == api.DIFF_TRANSFORMS | api.DIFF_LIGHTS
    b, _ = render(gpu, gpu.WavefrontPathTracer, s, tables, 2, tr=tr)
    if flatten:
        fb = s.flat_bvh()
        want_b, _ = orc.render(new.desc, W, H, n_passes=2, tables=tables, max_path_length=5, flat=fb.desc)
    else:
        want_b, _ = orc.render(new.desc, W, H, n_passes=2, tables=tables, max_path_length=5)
    close_to_oracle(b, want_b)
    assert not np.array_equal(a, b)


def test_refusals_leave_the_scene_as_it_was(gpu, orc):
    old = build("S3", width=W, height=H)
    tables = orc.sequence_tables(1)
    s = gpu.Scene(old.desc, flatten=True)
    a, tr = render(gpu, gpu.WavefrontPathTracer, s, tables, 1)

    def one_more_mesh(sc):
        from cudatracerlib_amd import scenes
        V, F = scenes.icosphere(1)
        sc.CreateNode(sc.add_mesh(V, F, normals=V, materials=[api.diffuse((0.5, 0.5, 0.5))]))
    grown = build("S3", width=W, height=H, edit=one_more_mesh)
    with pytest.raises(api.CtlError) as e:
        s.update(grown.desc)
    assert e.value.code == api.ERR_INVALID and s.last_mask & api.DIFF_TOPOLOGY
    again, _ = render(gpu, gpu.WavefrontPathTracer, s, tables, 1, tr=tr)
    assert_bit_equal(again, a, "frame A after a refused update")
    # the Q8 measurement format is not refitted; its cheap updates work
    q8 = gpu.Scene(old.desc, flatten=True, flat_format="q8")
    moved = build("S3", "M1", width=W, height=H)       # (a description points into its builder: the builder has to outlive the call)
    with pytest.raises(api.CtlError) as e:
        q8.update(moved.desc)
    assert e.value.code == api.ERR_UNSUPPORTED
    cam = build("S3", width=W, height=H, edit=lambda sc: sc.setCamera((120, 330, -700), (300, 250, 100), (0, 1, 0), 45.0, W, H))
    assert q8.update(cam.desc) == api.DIFF_CAMERA
    got, _ = render(gpu, gpu.WavefrontPathTracer, q8, tables, 1)
    want, _ = render(gpu, gpu.WavefrontPathTracer, gpu.Scene(cam.desc, flatten=True, flat_format="q8"), tables, 1)
    assert_bit_equal(got, want, "Q8 after a camera update")


def with_top_level(desc, nodes, start):
    """a copy of `desc` with another scene BVH: nodes (n, 16) uint32 in the reference's BVHNodeData layout"""
    d = api.ctl_scene_desc.from_buffer_copy(desc)
    buf = np.ascontiguousarray(nodes, np.uint32)
    d.scene_bvh_nodes = buf.ctypes.data; d.n_scene_bvh_nodes = len(buf); d.scene_start_node = start
    d._keep = (buf, desc)
    return d


@pytest.mark.parametrize("flatten", [True, False])
def test_a_top_level_bvh_that_does_not_fit_the_traversal_stack_is_refused(gpu, orc, flatten):
    """the two-level kernels keep scene-BVH depth + mesh-BVH depth + 3 entries on a per-lane stack of 96: an update whose new scene BVH is deeper than that, has
    a cycle or a link outside its array is refused like a scene of that kind is at creation, before anything is uploaded — the scene renders frame A bit-equal.
    (The check needs a scene, and a scene needs a device: hence a GPU test.)"""
    old = build("S3", width=W, height=H)
    d = old.desc
    tables = orc.sequence_tables(1)
    s = gpu.Scene(d, flatten=flatten)
    a, tr = render(gpu, gpu.WavefrontPathTracer, s, tables, 1)
    lo, hi = np.array(d.box_min[:], np.float32), np.array(d.box_max[:], np.float32)

    def chain(n, last_link):
        """n nodes, each with node 0 as its first child (a leaf) and the next chain node as its second; both child boxes = the scene box"""
        nodes = np.zeros((n, 16), np.uint32); f = nodes.view(np.float32)
        f[:, 0:4] = f[:, 4:8] = (lo[0], hi[0], lo[1], hi[1]); f[:, 8:12] = (lo[2], hi[2], lo[2], hi[2])
        nodes[:, 12] = np.uint32(0xffffffff)                                # ~0: the leaf of scene node 0
        nodes[:, 13] = (np.arange(1, n + 1) * 4).astype(np.uint32); nodes[-1, 13] = np.uint32(last_link & 0xffffffff)
        return nodes
    cases = {"too deep": chain(120, ~1), "cycle": chain(8, 0), "link outside the array": chain(8, 4 * 4000)}
    for what, nodes in cases.items():
        with pytest.raises(api.CtlError) as e:
            s.update(with_top_level(d, nodes, 0))
        assert e.value.code == api.ERR_INVALID and s.last_mask == api.DIFF_TRANSFORMS, what
        again, _ = render(gpu, gpu.WavefrontPathTracer, s, tables, 1, tr=tr)
        assert_bit_equal(again, a, "frame A after the refused update (%s)" % what)
    # a chain that fits is taken (every ray then also visits node 0 once per level: slower, same hits)
    ok = with_top_level(d, chain(20, ~1), 0)
    assert s.update(ok) == api.DIFF_TRANSFORMS


def test_the_validator_and_the_scene_agree(gpu, orc):
    """ctl_scene_desc_check is what creation and update themselves ask (csrc/scene_checks.cpp): a malformed description (tests/scene_check_cases.py) is refused by
    gpu.Scene with the status and message the host-only check gives, and as an update it is refused with the update's prefix, before anything is written — the mask
    is reported as for any refusal and the next frame is the one rendered before."""
    import scene_check_cases as K
    for name in ("forward transform not affine", "bad sensor type", "unknown light type", "unknown texture type", "nested index out of range", "scene BVH too deep"):
        d, _, message = K.make(name)
        with pytest.raises(api.CtlError) as want:
            api.scene_desc_check(d, 0)
        assert want.value.code == api.ERR_INVALID and str(want.value).endswith(message), name
        for flatten in (False, True):
            with pytest.raises(api.CtlError) as got:
                gpu.Scene(d, flatten=flatten)
            assert (got.value.code, str(got.value)) == (want.value.code, str(want.value)), name
    base = K.base("cornell").desc
    tables = orc.sequence_tables(1)
    s = gpu.Scene(base, flatten=True)
    tr = gpu.WavefrontPathTracer(); tr.getParameters().setValue("MaxPathLength", 5); tr.Resize(64, 64); tr.InitializeScene(s)

    def frame():
        img = gpu.Image(64, 64)
        tr.setSamplerTables(*tables[0]); tr.DoPass(img, new_trace=True)
        return img.getPixelData()
    a = frame()
    for name, mask in (("unknown texture type", api.DIFF_MATERIALS), ("bad sensor type", api.DIFF_CAMERA)):
        d, _, message = K.make(name)
        assert api.scene_desc_diff(base, d) == mask
        with pytest.raises(api.CtlError) as want:
            api.scene_desc_check(d, mask)
        assert str(want.value).split(": ", 1)[1].startswith("ctl_scene_update: "), str(want.value)
        with pytest.raises(api.CtlError) as got:
            s.update(d)
        assert (got.value.code, str(got.value)) == (api.ERR_INVALID, str(want.value)) and s.last_mask == mask, name
        assert_bit_equal(frame(), a, "frame A after the refused update (%s)" % name)
