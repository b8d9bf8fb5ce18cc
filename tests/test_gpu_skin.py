"""Skinned meshes on the device: ctl_scene_bind_skin / ctl_scene_animate_mesh / ctl_scene_read_mesh_geometry / ctl_scene_unbind_skin.  What the three pose kernels
leave in HBM against the host yardstick (ctl_skin_mesh_host) bit for bit, the flattened tree against the host refit of the host-updated description row for row, the
traversal against the oracle, frames of every tracer against a scene updated through DynamicScene.UpdateMesh + ctl_scene_update to the same pose (bit-equal), sequences
of poses, two bound meshes, the ownership rule and the refusals.  Cases K1..K5: tests/skin_cases.py."""
import numpy as np
import pytest

from cudatracerlib_amd import api
from scene_update_cases import build, rays_for_update, node_transforms
from scene_deform_cases import NO_PART, nodes_of, entries_of, mesh_arrays
from skin_cases import CASES, make_case, yardstick, host_updated, bind, animate, same_bits
from test_gpu_scene_deform import check_flat_updated, tracers, render, assert_bit_equal, W, H

pytestmark = pytest.mark.gpu
_cache = {}


def case_of(name, size=32):
    """(case, yardstick, host-updated builder), made once and left unchanged"""
    if (name, size) not in _cache:
        K = make_case(name, width=size, height=size)
        Y = yardstick(K)
        _cache[(name, size)] = (K, Y, host_updated(K, Y))
    return _cache[(name, size)]


def same_tree(a, b):
    """test_gpu_scene_deform.same_tree with a NaN for a NaN in the leaf entries: the Woop rows of a collapsed triangle are NaN / inf, and a device-made NaN need not
    carry x86's sign bit"""
    pa, pb = a.parts(), b.parts()
    assert np.array_equal(a.nodes(), b.nodes()), "nodes: %d of %d differ" % ((a.nodes() != b.nodes()).any(axis=1).sum(), len(b.nodes()))
    la, lb = a.leaves(), b.leaves()
    assert same_bits(la[:, :12], lb[:, :12]) and np.array_equal(la[:, 12:], lb[:, 12:]), "leaf entries"
    assert pa[0] is not None and np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1]), "refit side data"


def posed_scene(gpu, K):
    s = gpu.Scene(K["plain"].desc, flatten=True)
    bind(s, K)
    st = animate(s, K)
    return s, st


def read_back(s, K):
    return s.read_mesh_geometry(K["mesh"], vertices=True)


def assert_equals_yardstick(got, Y, what=""):
    for k in ("positions", "normals", "woop"):
        assert same_bits(got[k], Y[k]), "%s %s: %d words differ" % (what, k, (got[k].view(np.uint32) != Y[k].view(np.uint32)).sum())
    assert np.array_equal(got["tri"], Y["tri"]), "%s TriangleData: %d rows differ" % (what, (got["tri"] != Y["tri"]).any(axis=1).sum())


@pytest.mark.parametrize("name", CASES)
def test_device_pose_equals_the_yardstick_and_the_host_refit(gpu, name):
    K, Y, bent = case_of(name)
    s, st = posed_scene(gpu, K)
    assert_equals_yardstick(read_back(s, K), Y, name)
    assert st["skin_ms"] > 0 and st["refit_ms"] > 0 and st["refit_levels"] >= 2 and st["mask"] == api.DIFF_GEOMETRY and st["node_area_after"] > 0
    print("%s: pose kernels %.3f ms, refit %.3f ms" % (name, st["skin_ms"], st["refit_ms"]))
    # the flat-tree half: the host refit of the host-updated description, row for row
    host = api.FlatBvh(K["plain"].desc)
    host.refit(bent.desc)
    dev = s.flat_bvh()
    same_tree(dev, host)
    ours = entries_of(dev, bent.desc, K["mesh"])
    assert ours.any() and (dev.parts()[0][ours] == NO_PART).all()
    if name == "K6":
        got = read_back(s, K)
        assert K["n_rows"] > K["n_tri"] and got["woop"].shape[0] == K["n_rows"] and got["tri"].shape[0] == K["n_tri"]
    if name == "K2":
        before = api.FlatBvh(K["plain"].desc)
        assert (before.parts()[0][entries_of(before, K["plain"].desc, K["mesh"])] != NO_PART).sum() > 0, "the beams carry split references before the pose"
    # the other meshes' arrays are untouched
    for other in range(K["plain"].desc.n_meshes):
        if other != K["mesh"]:
            A = mesh_arrays(K["plain"].desc, other)
            got = s.read_mesh_geometry(other)
            assert got["tri"].shape == A["tri"].shape and got["woop"].shape == A["woop"].shape
            assert np.array_equal(got["tri"], A["tri"]) and same_bits(got["woop"], A["woop"]), other


@pytest.mark.parametrize("name", ["K1", "K2", "K3-0.37", "K4", "K5", "K6"])
def test_hits_of_the_posed_scene(gpu, orc, name):
    K, Y, bent = case_of(name)
    aim = nodes_of(bent.desc, K["mesh"])
    rays = rays_for_update(bent.desc, 30000, 31, aim_nodes=aim)
    s, _ = posed_scene(gpu, K)
    got = check_flat_updated(gpu, orc, s, bent.desc, rays, False)
    assert np.isin(got["node_idx"], aim).sum() > 20
    check_flat_updated(gpu, orc, s, bent.desc, rays, True)


@pytest.mark.parametrize("name", ["K1", "K2", "K3-0.37", "K4", "K5", "K6"])
def test_frames_equal_a_host_updated_scene(gpu, orc, name):
    """tests/test_skin_host.py finds the yardstick's arrays byte-equal to UpdateMesh's in every case (asserted again here from the readback), so every tracer renders the
    animated scene and a scene updated through UpdateMesh + ctl_scene_update to the same pose to the same bits"""
    K, Y, bent = case_of(name, W)
    tables = orc.sequence_tables(2)
    s, _ = posed_scene(gpu, K)
    got = read_back(s, K)
    A = mesh_arrays(bent.desc, K["mesh"])
    assert np.array_equal(got["tri"], A["tri"]) and same_bits(got["woop"], A["woop"])
    u = gpu.Scene(K["plain"].desc, flatten=True)
    assert u.update(bent.desc) & api.DIFF_GEOMETRY
    rest = gpu.Scene(K["plain"].desc, flatten=True)
    for tname, make, n in tracers(gpu):
        a, _ = render(gpu, make, s, tables, n)
        b, _ = render(gpu, make, u, tables, n)
        assert_bit_equal(a, b, "%s, %s" % (tname, name))
        r, _ = render(gpu, make, rest, tables, n)
        assert not np.array_equal(a, r), tname


def test_a_second_pose_equals_that_pose_alone(gpu):
    K0, Y0, _ = case_of("K3-0")
    K1, Y1, bent1 = case_of("K3-1")
    s, _ = posed_scene(gpu, K0)
    assert_equals_yardstick(read_back(s, K0), Y0, "first pose")
    animate(s, K1)                                   # the same binding: K3's cases differ in the lerp alone
    assert_equals_yardstick(read_back(s, K1), Y1, "second pose")
    alone, _ = posed_scene(gpu, K1)
    same_tree(s.flat_bvh(), alone.flat_bvh())
    host = api.FlatBvh(K1["plain"].desc); host.refit(bent1.desc)
    same_tree(s.flat_bvh(), host)
    # binding again replaces the binding; the pose it makes is the same
    bind(s, K1); animate(s, K1)
    assert_equals_yardstick(read_back(s, K1), Y1, "after a second bind")


def second_skin(K):
    """S3's glass sphere (mesh of node 1) under two bones, next to the ball of K"""
    plain = K["plain"]
    mesh = int(plain.desc.view("nodes", np.uint32, plain.desc.n_nodes, 6)[1, 0])
    assert mesh != K["mesh"]
    inp = plain.mesh_inputs[mesh]
    P = inp["positions"]; c = 0.5 * (P.min(axis=0).astype(np.float64) + P.max(axis=0))
    t = (P[:, 1] - P[:, 1].min()) / (P[:, 1].max() - P[:, 1].min())
    BI = np.zeros((len(P), 8), np.uint8); BW = np.zeros((len(P), 8), np.uint8)
    BI[:, 1] = 1; BW[:, 1] = np.round(t * 255); BW[:, 0] = 255 - BW[:, 1]
    B = np.tile(np.eye(4), (2, 1, 1)); B[1, :3, :3] = np.diag([0.8, 0.9, 0.8]); B[1, :3, 3] = c - B[1, :3, :3] @ c
    A = mesh_arrays(plain.desc, mesh)
    return dict(case="glass", scene=K["scene"], width=K["width"], height=K["height"], plain=plain, mesh=mesh, P=np.ascontiguousarray(P, np.float32), I=inp["indices"],
                N=None if inp["normals"] is None else np.ascontiguousarray(inp["normals"], np.float32), BI=BI, BW=BW, n_bones=2, B0=B.astype(np.float32), B1=None, lerp=0.0,
                n_tri=len(A["tri"]), n_rows=len(A["woop"]))


def test_two_bound_meshes_do_not_disturb_each_other(gpu):
    K, Y, _ = case_of("K3-0.37")
    G = second_skin(K); YG = yardstick(G)
    s = gpu.Scene(K["plain"].desc, flatten=True)
    bind(s, K); bind(s, G)
    animate(s, K); animate(s, G)
    assert_equals_yardstick(read_back(s, K), Y, "the ball after the sphere's pose")
    assert_equals_yardstick(read_back(s, G), YG, "the sphere")
    animate(s, K)
    assert_equals_yardstick(read_back(s, G), YG, "the sphere after the ball's second pose")
    assert_equals_yardstick(read_back(s, K), Y, "the ball")

    def both(sc):
        sc.UpdateMesh(G["mesh"], YG["positions"], G["I"], normals=YG["normals"], uvs=None)
    bent = host_updated(K, Y, edit=both)
    host = api.FlatBvh(K["plain"].desc); host.refit(bent.desc)
    same_tree(s.flat_bvh(), host)


def test_a_bound_mesh_is_device_owned(gpu, orc):
    """camera and SetNodeTransform updates on a bound, posed mesh: the masks carry no DIFF_GEOMETRY, the pose stays, and the frames are those of a scene that was
    updated on the host to the same pose and the same camera / transform.  After unbind_skin the description's values come back."""
    K, Y, bent = case_of("K3-0.37", W)
    tables = orc.sequence_tables(2)
    s, _ = posed_scene(gpu, K)
    u = gpu.Scene(K["plain"].desc, flatten=True)
    assert u.update(bent.desc) & api.DIFF_GEOMETRY

    def camera(sc):
        sc.setCamera((120, 330, -700), (300, 250, 100), (0, 1, 0), 45.0, W, H)
    node = nodes_of(K["plain"].desc, K["mesh"])[0]
    X = node_transforms(K["plain"].desc)[node].copy(); X[:3, 3] += (12.0, 9.0, -15.0); X[:3, :3] *= 0.9

    def moved(sc):
        camera(sc); sc.SetNodeTransform(node, X.astype(np.float32))
    for what, edit, want in (("camera", camera, api.DIFF_CAMERA), ("transform", moved, api.DIFF_TRANSFORMS)):
        rest = build(K["scene"], width=W, height=W, edit=edit)        # the host's description still holds the rest pose: the mesh's values are not the host's to say
        mask = s.update(rest.desc)
        assert mask & want and not mask & (api.DIFF_GEOMETRY | api.DIFF_TOPOLOGY), (what, mask)
        assert_equals_yardstick(read_back(s, K), Y, "after the %s update" % what)
        bent_too = host_updated(K, Y, edit=edit)                      # (held: a description points into its builder)
        mask_u = u.update(bent_too.desc)
        assert mask_u & want and not mask_u & api.DIFF_TOPOLOGY
        for tname, make, n in tracers(gpu):
            a, _ = render(gpu, make, s, tables, n)
            b, _ = render(gpu, make, u, tables, n)
            assert_bit_equal(a, b, "%s after the %s update" % (tname, what))
    same_tree(s.flat_bvh(), u.flat_bvh())
    # a second update with the same description finds nothing, bound mesh or not
    assert s.update(rest.desc) == 0
    # unbind: the mesh's value hash is invalid, the next update restores the description's values
    s.unbind_skin(K["mesh"])
    with pytest.raises(api.CtlError) as e:
        animate(s, K)
    assert e.value.code == api.ERR_INVALID
    mask = s.update(K["plain"].desc)
    assert mask & api.DIFF_GEOMETRY and not mask & api.DIFF_TOPOLOGY
    A = mesh_arrays(K["plain"].desc, K["mesh"])
    got = s.read_mesh_geometry(K["mesh"])
    assert np.array_equal(got["tri"], A["tri"]) and same_bits(got["woop"], A["woop"])
    fresh = gpu.Scene(K["plain"].desc, flatten=True)
    for tname, make, n in tracers(gpu):
        a, _ = render(gpu, make, s, tables, n)
        b, _ = render(gpu, make, fresh, tables, n)
        assert_bit_equal(a, b, "%s after unbind + update" % tname)


def test_unbinding_twice_still_hands_the_mesh_back(gpu, orc):
    """bind / animate / unbind, and again with other weights, with no update in between: the mesh's value hash stays invalid (the invalidation is no toggle), so the
    next update reports DIFF_GEOMETRY, restores the description's values, and every tracer renders a fresh scene's frames"""
    K, Y, _ = case_of("K3-0.37", W)
    tables = orc.sequence_tables(2)
    s, _ = posed_scene(gpu, K)
    s.unbind_skin(K["mesh"])
    K2 = dict(K); K2["BW"] = K["BW"].copy(); K2["BW"][:, 2] //= 2
    bind(s, K2); animate(s, K2)
    assert_equals_yardstick(read_back(s, K2), yardstick(K2), "the second binding")
    s.unbind_skin(K["mesh"])
    with pytest.raises(api.CtlError) as e:
        s.unbind_skin(K["mesh"])
    assert e.value.code == api.ERR_INVALID
    mask = s.update(K["plain"].desc)
    assert mask & api.DIFF_GEOMETRY and not mask & api.DIFF_TOPOLOGY, mask
    A = mesh_arrays(K["plain"].desc, K["mesh"])
    got = s.read_mesh_geometry(K["mesh"])
    assert np.array_equal(got["tri"], A["tri"]) and same_bits(got["woop"], A["woop"])
    assert s.update(K["plain"].desc) == 0
    fresh = gpu.Scene(K["plain"].desc, flatten=True)
    for tname, make, n in tracers(gpu):
        a, _ = render(gpu, make, s, tables, n)
        b, _ = render(gpu, make, fresh, tables, n)
        assert_bit_equal(a, b, "%s after two unbinds + update" % tname)
    # bound in between: an update with the rest description neither reports nor restores, the invalid hash is carried along
    bind(s, K); animate(s, K)
    assert s.update(K["plain"].desc) == 0
    assert_equals_yardstick(read_back(s, K), Y, "bound again")
    s.unbind_skin(K["mesh"])
    assert s.update(K["plain"].desc) & api.DIFF_GEOMETRY


def test_refusals_leave_the_frame_alone(gpu, orc):
    K, Y, _ = case_of("K3-0.37", W)
    tables = orc.sequence_tables(1)
    d = K["plain"].desc
    panel = int(d.view("nodes", np.uint32, d.n_nodes, 6)[4, 0])       # S3's emissive panel: an area light on its node
    pin = K["plain"].mesh_inputs[panel]
    for what, scene in (("two-level", gpu.Scene(d)), ("Q8", gpu.Scene(d, flatten=True, flat_format="q8")), ("flattened", gpu.Scene(d, flatten=True))):
        a, tr = render(gpu, gpu.WavefrontPathTracer, scene, tables, 1)
        codes = []

        def refused(call):
            with pytest.raises(api.CtlError) as e:
                call()
            codes.append(e.value.code)
            return e.value.code
        if what != "flattened":
            assert refused(lambda: bind(scene, K)) == api.ERR_UNSUPPORTED, what
        else:
            zeros = np.zeros((len(pin["positions"]), 8), np.uint8)
            assert refused(lambda: scene.bind_skin(panel, pin["positions"], pin["indices"], zeros, zeros, 1, rest_normals=pin["normals"])) == api.ERR_UNSUPPORTED     # the area light
            bad = K["BI"].copy(); bad[3, 7] = 255
            assert refused(lambda: scene.bind_skin(K["mesh"], K["P"], K["I"], bad, K["BW"], 200)) == api.ERR_INVALID                                        # an index byte >= n_bones
            assert refused(lambda: scene.bind_skin(d.n_meshes, K["P"], K["I"], K["BI"], K["BW"], 256)) == api.ERR_INVALID                                 # a bad mesh index
            assert refused(lambda: scene.bind_skin(K["mesh"], K["P"], K["I"][:-1], K["BI"], K["BW"], 256)) == api.ERR_INVALID                             # another triangle count
            nan = K["B0"].copy(); nan[17, 1, 1] = np.nan
            bind(scene, K)
            assert refused(lambda: scene.read_mesh_geometry(K["mesh"], vertices=True)) == api.ERR_INVALID                                                 # bound, but no pose yet
            assert refused(lambda: scene.animate_mesh(K["mesh"], nan, K["B1"], K["lerp"])) == api.ERR_INVALID                                             # not finite
            assert refused(lambda: scene.animate_mesh(K["mesh"], K["B0"], K["B1"], float("nan"))) == api.ERR_INVALID
            scene.unbind_skin(K["mesh"])
        assert refused(lambda: animate(scene, K)) == api.ERR_INVALID, what                                                                                  # an unbound mesh
        assert refused(lambda: scene.read_mesh_geometry(K["mesh"], vertices=True)) == api.ERR_INVALID                      # no pose to read
        again, _ = render(gpu, gpu.WavefrontPathTracer, scene, tables, 1, tr=tr)
        assert_bit_equal(again, a, "%s: the frame after the refused calls" % what)
        # the arrays as HBM holds them can be read from any scene
        A = mesh_arrays(d, K["mesh"])
        got = scene.read_mesh_geometry(K["mesh"])
        assert np.array_equal(got["tri"], A["tri"]) and same_bits(got["woop"], A["woop"]), what
