"""ctl_scene_update with CTL_DIFF_GEOMETRY on the device: a mesh deformed through DynamicScene.UpdateMesh is applied in place.  The flattened Q4 tree after the
update against the host refit (byte for byte: nodes, leaf entries, refit side data), the traversal of the updated scene against the oracle in both layouts, the
two-level layout's frames against a freshly created scene (bit-equal, every tracer), the flattened layout's frames against the oracle by the bars of
tests/test_gpu_render.py, sequences of updates, and the refusals.  Cases D1..D4: tests/scene_deform_cases.py."""
import numpy as np
import pytest

from cudatracerlib_amd import api
from scene_update_cases import build, rays_for_update
from scene_deform_cases import CASES, IDS, NO_PART, build_pair, build_deformed_and_moved, nodes_of, entries_of

pytestmark = pytest.mark.gpu
W, H = 48, 48


def same_tree(a, b):
    pa, pb = a.parts(), b.parts()
    assert np.array_equal(a.nodes(), b.nodes()), "nodes: %d of %d differ" % ((a.nodes() != b.nodes()).any(axis=1).sum(), len(b.nodes()))
    assert np.array_equal(a.leaves(), b.leaves()), "leaf entries: %d of %d differ" % ((a.leaves() != b.leaves()).any(axis=1).sum(), len(b.leaves()))
    assert pa[0] is not None and np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1]), "refit side data"


@pytest.mark.parametrize("case,scene", CASES, ids=IDS)
def test_device_refit_equals_the_host_refit(gpu, case, scene):
    old, new, mesh = build_pair(case, scene)
    s = gpu.Scene(old.desc, flatten=True)
    host = api.FlatBvh(old.desc)
    same_tree(s.flat_bvh(), host)                                    # the read-back un-stamps, and hands out the side data the device holds
    mask = s.update(new.desc)
    assert mask & api.DIFF_GEOMETRY and not mask & api.DIFF_TOPOLOGY
    host.refit(new.desc)
    dev = s.flat_bvh()
    same_tree(dev, host)
    ours = entries_of(dev, new.desc, mesh)
    assert ours.any() and (dev.parts()[0][ours] == NO_PART).all()
    st = s.update_stats()
    assert st["node_area_before"] > 0 and st["node_area_after"] > 0 and st["refit_levels"] >= 2 and st["mask"] == mask and st["refit_ms"] > 0
    print("%s %s: refit %.3f ms, %d levels, node area %.6g -> %.6g" % (case, scene, st["refit_ms"], st["refit_levels"], st["node_area_before"], st["node_area_after"]))
    # a second update with the same description finds nothing to do and changes nothing
    assert s.update(new.desc) == 0
    same_tree(s.flat_bvh(), host)


def check_flat_updated(gpu, orc, scene, desc, rays, any_hit):
    """tests/test_gpu_scene_update.py::check_flat_updated restated: the scene's traversal against the oracle's restatement of the reference's TWO-LEVEL traversal,
    bit for bit, equal-t ties excepted"""
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


@pytest.mark.parametrize("case,scene", CASES, ids=IDS)
def test_hits_of_the_updated_scene(gpu, orc, case, scene):
    old, new, mesh = build_pair(case, scene)
    aim = nodes_of(new.desc, mesh)
    rays = rays_for_update(new.desc, 30000, 29, aim_nodes=aim)
    s = gpu.Scene(old.desc, flatten=True)
    assert s.update(new.desc) & api.DIFF_GEOMETRY
    got = check_flat_updated(gpu, orc, s, new.desc, rays, False)
    assert np.isin(got["node_idx"], aim).sum() > 20
    check_flat_updated(gpu, orc, s, new.desc, rays, True)
    # the two-level layout of the same update
    s2 = gpu.Scene(old.desc)
    assert s2.update(new.desc) & api.DIFF_GEOMETRY
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


@pytest.mark.parametrize("case,scene", CASES, ids=IDS)
def test_two_level_frames_equal_a_fresh_scene(gpu, orc, case, scene):
    """the two-level arrays after the update are those of a scene created from the new description — in the SAME allocations: the tracers that rendered before the
    update keep rendering, and every pixel equals the fresh scene's.  Of the four tracers the WavefrontPathTracer takes a two-level scene; the PathTracer plugin (the
    megakernel) and the PrimTracer take flattened scenes only — they refuse a two-level one at InitializeScene, before and after this change —, so they are held to
    the same bar on the flattened layout: the refitted tree against a freshly built one, whose traversals report the same hits bit for bit (equal-t ties excepted,
    and tests/test_scene_deform_host.py finds none in these scenes)."""
    old, new, _ = build_pair(case, scene, width=W, height=H)
    tables = orc.sequence_tables(2)
    fresh = {}
    two_level = []
    for name, make, n in tracers(gpu):
        flatten = False
        s = gpu.Scene(old.desc)
        try:
            a, tr = render(gpu, make, s, tables, n)
            two_level.append(name)
        except api.CtlError as e:
            assert e.code == api.ERR_UNSUPPORTED and "CTL_SCENE_FLATTEN" in str(e), name
            flatten = True
            s = gpu.Scene(old.desc, flatten=True)
            a, tr = render(gpu, make, s, tables, n)
        mask = s.update(new.desc)
        assert mask & api.DIFF_GEOMETRY and not mask & api.DIFF_TOPOLOGY and (mask & api.DIFF_LIGHTS or case != "D4")
        got, _ = render(gpu, make, s, tables, n, tr=tr)
        if flatten not in fresh:
            fresh[flatten] = gpu.Scene(new.desc, flatten=flatten)
        want, _ = render(gpu, make, fresh[flatten], tables, n)
        assert_bit_equal(got, want, "%s after %s (%s)" % (name, case, "flattened" if flatten else "two-level"))
        assert not np.array_equal(got, a), name
    assert "WavefrontPathTracer" in two_level


def close_to_oracle(got, want, exact_min=0.98):
    """the bars of tests/test_gpu_render.py::assert_close"""
    assert np.array_equal(got[..., 6], want[..., 6]), "weightSum differs"
    g, w = got[..., :3], want[..., :3]
    frac = (np.abs(g - w) <= 2e-3 * (1 + np.abs(w))).all(axis=2).mean()
    exact = (g == w).all(axis=2).mean()
    print("within tolerance %.5f, bit-equal %.5f" % (frac, exact))
    assert frac >= 0.9995, frac
    assert exact >= exact_min, exact


@pytest.mark.parametrize("case", ["D4", "D1"])
def test_flattened_frames_after_a_geometry_update(gpu, orc, case):
    """render A, deform (D4: the emissive panel, whose shape set and CDF change with it; D1: the ball under two nodes), new_trace, render B: both are the oracle's
    frames of their description, traversing the tree the device holds"""
    old, new, _ = build_pair(case, "S3", width=W, height=H)
    tables = orc.sequence_tables(2)
    s = gpu.Scene(old.desc, flatten=True)
    a, tr = render(gpu, gpu.WavefrontPathTracer, s, tables, 2)
    fa = s.flat_bvh()                                                # (the handle owns the arrays its desc points to)
    want_a, _ = orc.render(old.desc, W, H, n_passes=2, tables=tables, max_path_length=5, flat=fa.desc)
    close_to_oracle(a, want_a)
    mask = s.update(new.desc)
    assert mask & api.DIFF_GEOMETRY and (mask & api.DIFF_LIGHTS or case != "D4")
    b, _ = render(gpu, gpu.WavefrontPathTracer, s, tables, 2, tr=tr)
    fb = s.flat_bvh()
    want_b, _ = orc.render(new.desc, W, H, n_passes=2, tables=tables, max_path_length=5, flat=fb.desc)
    close_to_oracle(b, want_b)
    assert not np.array_equal(a, b)


def test_a_transform_update_after_a_geometry_update(gpu, orc):
    """D2, then M2 of the same node: the device tree equals the host handle refitted the same way, and the entries that became whole stay whole (a transform refit
    must not carry their stale clip boxes)"""
    old, new, mesh = build_pair("D2", "S2")
    moved = build_deformed_and_moved("D2", "S2", "M2")
    s = gpu.Scene(old.desc, flatten=True)
    host = api.FlatBvh(old.desc)
    ours = entries_of(host, old.desc, mesh)
    assert (host.parts()[0][ours] != NO_PART).sum() > 0
    assert s.update(new.desc) & api.DIFF_GEOMETRY
    mask = s.update(moved.desc)
    assert mask & api.DIFF_TRANSFORMS and not mask & (api.DIFF_GEOMETRY | api.DIFF_TOPOLOGY)
    host.refit(new.desc).refit(moved.desc)
    dev = s.flat_bvh()
    same_tree(dev, host)
    assert (dev.parts()[0][ours] == NO_PART).all()
    rays = rays_for_update(moved.desc, 30000, 29, aim_nodes=nodes_of(moved.desc, mesh))
    check_flat_updated(gpu, orc, s, moved.desc, rays, False)
    check_flat_updated(gpu, orc, s, moved.desc, rays, True)


def test_refusals(gpu, orc):
    """D3 in reverse — the scene is created from the collapsed ball, whose zero-area triangles have no leaf entry, and updated to the round one: the flattened tree
    has nowhere to put them (refused, scene untouched), the two-level layout takes it.  A Q8 scene is not refitted."""
    old, new, mesh = build_pair("D3", "S3", width=W, height=H, reverse=True)
    tables = orc.sequence_tables(1)
    s = gpu.Scene(old.desc, flatten=True)
    a, tr = render(gpu, gpu.WavefrontPathTracer, s, tables, 1)
    tree = s.flat_bvh()
    with pytest.raises(api.CtlError) as e:
        s.update(new.desc)
    assert e.value.code == api.ERR_INVALID and s.last_mask & api.DIFF_TOPOLOGY and s.last_mask & api.DIFF_GEOMETRY and "mesh %d" % mesh in str(e.value)
    same_tree(s.flat_bvh(), tree)
    again, _ = render(gpu, gpu.WavefrontPathTracer, s, tables, 1, tr=tr)
    assert_bit_equal(again, a, "frame A after the refused update")
    s2 = gpu.Scene(old.desc)
    mask = s2.update(new.desc)
    assert mask & api.DIFF_GEOMETRY and not mask & api.DIFF_TOPOLOGY
    aim = nodes_of(new.desc, mesh)
    rays = rays_for_update(new.desc, 30000, 29, aim_nodes=aim)
    got = check_flat_updated(gpu, orc, s2, new.desc, rays, False)
    assert np.isin(got["node_idx"], aim).sum() > 20
    check_flat_updated(gpu, orc, s2, new.desc, rays, True)
    # the Q8 measurement format is not refitted; its cheap updates still work afterwards
    plain, bent, _ = build_pair("D1", "S3", width=W, height=H)
    q8 = gpu.Scene(plain.desc, flatten=True, flat_format="q8")
    with pytest.raises(api.CtlError) as e:
        q8.update(bent.desc)
    assert e.value.code == api.ERR_UNSUPPORTED
    cam = build("S3", width=W, height=H, edit=lambda sc: sc.setCamera((120, 330, -700), (300, 250, 100), (0, 1, 0), 45.0, W, H))
    assert q8.update(cam.desc) == api.DIFF_CAMERA
    got, _ = render(gpu, gpu.WavefrontPathTracer, q8, tables, 1)
    want, _ = render(gpu, gpu.WavefrontPathTracer, gpu.Scene(cam.desc, flatten=True, flat_format="q8"), tables, 1)
    assert_bit_equal(got, want, "Q8 after a camera update")
