"""Emissive skins on the device: ctl_scene_bind_skin_ex with CTL_SKIN_AREA_LIGHTS.  The light tables HBM holds after a pose (ctl_scene_read_lights) against the host
yardstick (ctl_shape_sets_host) and against a description updated on the host to the same pose, float words bit for bit (a NaN for a NaN), everything else byte for
byte; frames of every tracer against a scene brought to the same pose through DynamicScene.UpdateMesh + ctl_scene_update (bit-equal); sequences of poses; the
ownership rule under ctl_scene_update and ctl_scene_update_nodes; unbinding; the refusals.  Cases E1..E6: tests/skin_emitter_cases.py."""
import numpy as np
import pytest

from cudatracerlib_amd import api
from scene_update_cases import build, node_transforms
from scene_deform_cases import mesh_arrays
from skin_cases import yardstick, animate, same_bits
from skin_emitter_cases import CASES, FRAME_CASES, emitter_case, tables_of, assert_tables_equal, light_table, posed_lights, bind
from test_gpu_scene_deform import tracers, render, assert_bit_equal, W, H

pytestmark = pytest.mark.gpu


def posed_scene(gpu, K):
    s = gpu.Scene(K["plain"].desc, flatten=True)
    bind(s, K)
    st = animate(s, K)
    return s, st


def all_tracers(gpu):
    """tracers(gpu) — the Wavefront tracer as it comes (Direct on), the PathTracer, the PrimTracer — plus the Wavefront tracer with next-event estimation off"""
    def no_direct():
        t = gpu.WavefrontPathTracer(); t.getParameters().setValue("Direct", False); return t
    return tracers(gpu) + (("WavefrontPathTracer, Direct off", no_direct, 2),)


@pytest.mark.parametrize("name", CASES)
def test_tables_after_a_pose_equal_the_yardstick_and_the_host_update(gpu, name):
    K, Y, bent, S = emitter_case(name)
    d = K["plain"].desc
    s, st = posed_scene(gpu, K)
    got = s.read_lights()
    assert_tables_equal(got, S, d, K["mesh"], "%s against ctl_shape_sets_host" % name)
    assert_tables_equal(got, tables_of(bent.desc), d, K["mesh"], "%s against the host-updated description" % name)
    assert st["shape_set_ms"] > 0 and st["skin_ms"] > 0
    print("%s: pose kernels %.3f ms, shape-set kernels %.3f ms (%d lights, %d triangles)" % (name, st["skin_ms"], st["shape_set_ms"], len(K["lights"]), sum(int(light_table(d)[li, 7]) for li in K["lights"])))
    geo = s.read_mesh_geometry(K["mesh"])
    assert np.array_equal(geo["tri"], Y["tri"]) and same_bits(geo["woop"], Y["woop"])


@pytest.mark.parametrize("name", FRAME_CASES)
def test_frames_equal_a_host_updated_scene(gpu, orc, name):
    K, Y, bent, S = emitter_case(name, W)
    tables = orc.sequence_tables(2)
    s, _ = posed_scene(gpu, K)
    u = gpu.Scene(K["plain"].desc, flatten=True)
    mask = u.update(bent.desc)
    assert mask & api.DIFF_GEOMETRY and mask & api.DIFF_LIGHTS
    rest = gpu.Scene(K["plain"].desc, flatten=True)
    for tname, make, n in all_tracers(gpu):
        a, _ = render(gpu, make, s, tables, n)
        b, _ = render(gpu, make, u, tables, n)
        assert_bit_equal(a, b, "%s, %s" % (tname, name))
        r, _ = render(gpu, make, rest, tables, n)
        assert not np.array_equal(a, r), tname


def test_a_second_pose_equals_that_pose_alone(gpu, orc):
    K, Y, _, S = emitter_case("E2", W)
    K2 = dict(K); K2["lerp"] = 0.8
    Y2 = yardstick(K2)
    S2 = api.shape_sets_host(K["plain"].desc, K["mesh"], Y2["tri"], Y2["woop"])
    assert not np.array_equal(S2["anim"], S["anim"])
    tables = orc.sequence_tables(2)
    s, _ = posed_scene(gpu, K)
    assert_tables_equal(s.read_lights(), S, K["plain"].desc, K["mesh"], "first pose")
    animate(s, K2)
    assert_tables_equal(s.read_lights(), S2, K["plain"].desc, K["mesh"], "second pose")
    alone, _ = posed_scene(gpu, K2)
    assert_tables_equal(alone.read_lights(), S2, K["plain"].desc, K["mesh"], "that pose alone")
    for tname, make, n in all_tracers(gpu):
        a, _ = render(gpu, make, s, tables, n)
        b, _ = render(gpu, make, alone, tables, n)
        assert_bit_equal(a, b, "%s after a second pose" % tname)


def test_updates_keep_the_pose_and_take_the_new_lights_and_transforms(gpu):
    """after a pose, update() with a description that still holds the REST pose but another radiance on the emissive light, then another transform of the emissive node:
    the new values arrive, the shape sets are those of the pose under the description's transform — the host's own rest-pose sets are overwritten"""
    K, Y, _, S = emitter_case("E3")
    node = K["nodes"][1]
    li = posed_lights(K["plain"].desc, K["mesh"])[2]               # the second node's own light (its material 0)

    def setup_and(more):
        def edit(sc):
            K["setup"](sc); more(sc)
        return edit

    def radiance(sc):
        sc.CreateLight(node, 0, (1.5, 9.0, 4.0))                   # the material has its light: CreateLight replaces the record
    X = node_transforms(K["plain"].desc)[node].copy(); X[:3, 3] += (-25.0, 30.0, 12.0); X[:3, :3] = X[:3, :3] @ np.diag([1.1, 0.8, 1.3])

    def moved(sc):
        radiance(sc); sc.SetNodeTransform(node, X.astype(np.float32))
    s, _ = posed_scene(gpu, K)
    for what, more, want in (("radiance", radiance, api.DIFF_LIGHTS), ("transform", moved, api.DIFF_TRANSFORMS | api.DIFF_LIGHTS)):
        rest = build("S3", edit=setup_and(more))                     # (held: a description points into its builder)
        assert light_table(rest.desc)[li, 9] == node and not np.array_equal(light_table(rest.desc)[li, 1:4], light_table(K["plain"].desc)[li, 1:4])
        mask = s.update(rest.desc)
        assert (mask & want) == want and not mask & (api.DIFF_GEOMETRY | api.DIFF_TOPOLOGY), (what, mask)
        assert s.shape_set_ms() > 0
        want_tables = api.shape_sets_host(rest.desc, K["mesh"], Y["tri"], Y["woop"])
        got = s.read_lights()
        assert_tables_equal(got, want_tables, rest.desc, K["mesh"], "after the %s update: the yardstick over the new description" % what)
        assert np.array_equal(got["lights"][li, 1:4], light_table(rest.desc)[li, 1:4]), what
        # the same edit on a builder that then brings the mesh to the pose.  (In this order: CreateLight on a material that has a light appends a new range to the anim
        # blob and leaves the old one behind, which UpdateMesh no longer visits — so it holds the rest pose here as it does in `rest`.)
        bent = build("S3", edit=setup_and(lambda sc: (more(sc), sc.UpdateMesh(K["mesh"], Y["positions"], K["I"], normals=Y["normals"], uvs=None))))
        assert_tables_equal(got, tables_of(bent.desc), rest.desc, K["mesh"], "after the %s update: the host-updated description" % what)
        assert s.update(rest.desc) == 0
    assert not np.array_equal(want_tables["anim"], S["anim"])        # the moved node's sets are other sets


def test_update_nodes_keeps_the_pose_and_follows_the_node_indices(gpu):
    K, Y, _, S = emitter_case("E1")
    s, _ = posed_scene(gpu, K)
    removed = build("S3", edit=lambda sc: sc.DeleteNode(2))          # a ball instance goes: the emissive panel is node 3 now
    st = s.update_nodes(removed)
    assert st["rebuilt"] == 1 and st["entries_dropped"] > 0
    d = removed.desc
    before, after = light_table(K["plain"].desc), light_table(d)
    li = K["lights"][0]
    assert before[li, 9] == 4 and after[li, 9] == 3
    got = s.read_lights()
    assert got["lights"][li, 9] == 3
    assert_tables_equal(got, api.shape_sets_host(d, K["mesh"], Y["tri"], Y["woop"]), d, K["mesh"], "after update_nodes")
    assert np.array_equal(got["anim"], S["anim"])                  # the node kept its transform: the posed sets to the bit
    assert s.shape_set_ms() > 0
    geo = s.read_mesh_geometry(K["mesh"])
    assert np.array_equal(geo["tri"], Y["tri"]) and same_bits(geo["woop"], Y["woop"])


def test_unbind_then_update_restores_the_description(gpu, orc):
    K, Y, _, S = emitter_case("E2", W)
    d = K["plain"].desc
    tables = orc.sequence_tables(2)
    s, _ = posed_scene(gpu, K)
    s.unbind_skin(K["mesh"])
    assert_tables_equal(s.read_lights(), S, d, K["mesh"], "unbinding itself writes nothing")
    mask = s.update(d)
    assert mask & api.DIFF_GEOMETRY and mask & api.DIFF_LIGHTS and not mask & api.DIFF_TOPOLOGY, mask
    got, want = s.read_lights(), tables_of(d)
    assert np.array_equal(got["lights"], want["lights"]) and np.array_equal(got["anim"], want["anim"])
    A = mesh_arrays(d, K["mesh"])
    geo = s.read_mesh_geometry(K["mesh"])
    assert np.array_equal(geo["tri"], A["tri"]) and same_bits(geo["woop"], A["woop"])
    assert s.update(d) == 0
    fresh = gpu.Scene(d, flatten=True)
    for tname, make, n in all_tracers(gpu):
        a, _ = render(gpu, make, s, tables, n)
        b, _ = render(gpu, make, fresh, tables, n)
        assert_bit_equal(a, b, "%s after unbind + update" % tname)


def test_refusals_leave_the_frame_alone(gpu, orc):
    K, _, _, _ = emitter_case("E1", W)
    d = K["plain"].desc
    tables = orc.sequence_tables(1)
    scene = gpu.Scene(d, flatten=True)
    a, tr = render(gpu, gpu.WavefrontPathTracer, scene, tables, 1)
    before = scene.read_lights()
    for flags, code in ((0, api.ERR_UNSUPPORTED), (2, api.ERR_INVALID), (api.SKIN_AREA_LIGHTS | 0x80000000, api.ERR_INVALID)):
        with pytest.raises(api.CtlError) as e:
            bind(scene, K, flags=flags)
        assert e.value.code == code, flags
    with pytest.raises(api.CtlError) as e:
        bind(scene, K, area_lights=False)                            # the plain call
    assert e.value.code == api.ERR_UNSUPPORTED and "carries an area light" in str(e.value)
    for what, other in (("two-level", gpu.Scene(d)), ("Q8", gpu.Scene(d, flatten=True, flat_format="q8"))):
        with pytest.raises(api.CtlError) as e:
            bind(other, K)
        assert e.value.code == api.ERR_UNSUPPORTED, what
    with pytest.raises(api.CtlError) as e:
        animate(scene, K)                                            # nothing was bound
    assert e.value.code == api.ERR_INVALID
    again, _ = render(gpu, gpu.WavefrontPathTracer, scene, tables, 1, tr=tr)
    assert_bit_equal(again, a, "the frame after the refused calls")
    after = scene.read_lights()
    assert np.array_equal(after["lights"], before["lights"]) and np.array_equal(after["anim"], before["anim"])
    want = tables_of(d)
    assert np.array_equal(after["lights"], want["lights"]) and np.array_equal(after["anim"], want["anim"])      # read_lights of any scene: what the description holds
