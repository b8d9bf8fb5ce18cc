"""Emissive skins shared by tests/test_skin_emitters_host.py and tests/test_gpu_skin_emitters.py: ctl_scene_bind_skin_ex with CTL_SKIN_AREA_LIGHTS on meshes whose
nodes carry area lights, all in S3 of tests/scene_update_cases.py (a Cornell box with its own area light, which no pose touches).  Bones as in tests/skin_cases.py.

E1  S3's emissive panel (the D4 mesh: 2 triangles), 2 bones: a bend plus a stretch
E2  one more node: a 24 x 24 emissive grid, 1152 triangles, 3 bones — more than one 1024-area LDS chunk of k_shape_cdf, a last workgroup of k_shape_triangles that is half
    full (1152 = 4 * 256 + 128), the serial sum crossing a chunk border
E3  a mesh with two emissive materials — two lights on one node — instanced by a second node with a rotated, non-uniformly scaled transform and a light of its own: three
    shape sets from one pose
E4  a one-triangle emissive mesh: count == 1
E5  K6's long thin soup made emissive: more Woop rows than triangles, i_dat naming the first reference
E6  K4's zero-scale bone on S3's ball made emissive on both of its nodes: collapsed triangles, singular Woop rows, NaN areas and CDF.  Tables only, no frames

Every pose stays inside the rest scene's box (skin_cases.host_updated asserts it), and for every case the yardstick's TriangleData and Woop rows equal
DynamicScene.UpdateMesh's byte for byte — emitter_case() asserts it: the kernels' normal codec (ctl_fmath.h) and the builder's (glibc) may straddle a code step for some
normal, and a pose where they do is no pose for these tests, because the shape-set normals are decoded from those codes."""
import numpy as np

from cudatracerlib_amd import api
from scene_update_cases import build
from scene_deform_cases import mesh_arrays, node_meshes
from skin_cases import _affine, _bands, _rot, add_ribbons, yardstick, host_updated, same_bits

CASES = ("E1", "E2", "E3", "E4", "E5", "E6")
FRAME_CASES = CASES[:5]


def _grid(n, wave):
    """(n + 1)^2 vertices on [-1, 1]^2 in the x-z plane, y = a gentle wave; 2 n^2 triangles"""
    u = np.linspace(-1.0, 1.0, n + 1)
    X, Z = np.meshgrid(u, u, indexing="ij")
    Y = wave * np.sin(2.0 * X) * np.cos(1.5 * Z)
    V = np.stack([X, Y, Z], axis=-1).reshape(-1, 3).astype(np.float32)
    k = np.arange(n)
    a = (k[:, None] * (n + 1) + k[None, :]).reshape(-1)
    F = np.concatenate([np.stack([a, a + 1, a + n + 2], axis=1), np.stack([a, a + n + 2, a + n + 1], axis=1)]).astype(np.uint32)
    return V, F


def _place(scale, at, lin=None):
    M = np.eye(4); M[:3, :3] = (np.eye(3) if lin is None else lin) * scale; M[:3, 3] = at
    return M.astype(np.float32)


def _add_grid(sc):
    V, F = _grid(24, 0.08)
    mesh = sc.add_mesh(V, F, materials=[api.diffuse((0.6, 0.6, 0.6), two_sided=True)])
    node = sc.CreateNode(mesh, _place(90.0, (278.0, 300.0, 280.0)))
    sc.CreateLight(node, 0, (9.0, 8.0, 6.0))


def _add_two_materials(sc):
    V, F = _grid(6, 0.05)
    tm = (np.arange(len(F)) % 3 == 0).astype(np.uint8)                   # material 1 on every third triangle
    mesh = sc.add_mesh(V, F, tri_material=tm, materials=[api.diffuse((0.6, 0.5, 0.4), two_sided=True), api.diffuse((0.3, 0.5, 0.6), two_sided=True)])
    a = sc.CreateNode(mesh, _place(60.0, (200.0, 330.0, 250.0)))
    sc.CreateLight(a, 0, (7.0, 6.0, 5.0)); sc.CreateLight(a, 1, (2.0, 5.0, 9.0))
    b = sc.CreateNode(mesh, _place(1.0, (380.0, 200.0, 330.0), _rot((0.4, 1.0, -0.3), 0.9) @ np.diag([70.0, 35.0, 50.0])))
    sc.CreateLight(b, 0, (6.0, 3.0, 2.0))


def _add_triangle(sc):
    V = np.array([[-1, 0, -0.6], [1, 0.1, -0.4], [0.1, -0.1, 0.9]], np.float32)
    mesh = sc.add_mesh(V, np.array([[0, 1, 2]], np.uint32), materials=[api.diffuse((0.5, 0.5, 0.5), two_sided=True)])
    node = sc.CreateNode(mesh, _place(80.0, (278.0, 320.0, 260.0)))
    sc.CreateLight(node, 0, (20.0, 18.0, 15.0))


def _add_emissive_ribbons(sc):
    add_ribbons(sc)
    sc.CreateLight(_last_node(sc), 0, (6.0, 5.0, 3.0))


def _last_node(sc):
    return len(sc.node_ids()) - 1


def _glowing_balls(sc):
    sc.CreateLight(2, 0, (4.0, 5.0, 6.0)); sc.CreateLight(3, 0, (6.0, 4.0, 3.0))


SETUP = {"E1": None, "E2": _add_grid, "E3": _add_two_materials, "E4": _add_triangle, "E5": _add_emissive_ribbons, "E6": _glowing_balls}


def make_case(case, width=32, height=32):
    """the dict of skin_cases.make_case, plus nodes (the nodes that instance the mesh) and lights (the lights whose shape sets a pose recomputes)"""
    setup = SETUP[case]
    plain = build("S3", width=width, height=height, edit=setup)
    d = plain.desc
    nm = node_meshes(d)
    mesh = int(nm[2]) if case == "E6" else int(nm[4]) if case == "E1" else int(nm[5])
    inp = plain.mesh_inputs[mesh]
    P, I, N = inp["positions"], inp["indices"], inp["normals"]
    c = 0.5 * (P.min(axis=0).astype(np.float64) + P.max(axis=0))
    B1 = None; lerp = 0.0
    if case == "E1":
        n_bones = 2
        BI, BW, ax = _bands(P, n_bones, False)
        B0 = np.stack([_affine(_rot((0, 0, 1), -0.3), c), _affine(_rot((0, 0, 1), 0.25) @ np.diag([1.5, 1.0, 1.2]), c, (0.1, -0.2, 0.0))])
    elif case in ("E2", "E5"):
        n_bones = 3
        BI, BW, ax = _bands(P, n_bones, False)
        axis = np.eye(3)[(ax + 1) % 3]
        B0 = np.stack([_affine(_rot(axis, a), c) for a in (-0.35, 0.0, 0.35)])
        B1 = np.stack([_affine(_rot(axis, a) @ np.diag([1.0, 0.9, 1.1]), c, s) for a, s in ((-0.2, (0.05, 0, 0)), (0.1, (0, 0.05, 0)), (0.3, (0, 0, -0.05)))])
        lerp = 0.25
    elif case == "E3":
        n_bones = 2
        BI, BW, ax = _bands(P, n_bones, False)
        B0 = np.stack([_affine(_rot((0, 0, 1), -0.4), c), _affine(_rot((1, 0, 0), 0.3) @ np.diag([1.2, 1.0, 0.8]), c)])
        B1 = np.stack([_affine(np.diag([0.9, 1.0, 1.1]), c, (0, 0.1, 0)), _affine(_rot((0, 0, 1), 0.5), c)])
        lerp = 0.6
    elif case == "E4":
        n_bones = 2
        BI, BW, ax = _bands(P, n_bones, False)
        B0 = np.stack([_affine(_rot((0, 0, 1), 0.4), c), _affine(_rot((1, 0, 0), -0.5) @ np.diag([1.3, 1.0, 0.7]), c, (0, 0.2, 0))])
    elif case == "E6":                                  # skin_cases K4
        n_bones = 4
        BI, BW, ax = _bands(P, 3, False)
        B0 = np.stack([_affine(_rot((0, 0, 1), a), c) for a in (-0.1, 0.0, 0.1)] + [np.zeros((4, 4))])
        radius = np.linalg.norm(P - c, axis=1).max()
        plane = c[1] - 0.35 * radius
        B0[3, :3, 3] = (c[0], plane, c[2]); B0[3, 3, 3] = 1.0
        cap = P[:, 1] < plane
        assert 10 < cap.sum() < len(P) // 2
        BI[cap] = 3; BW[cap] = 0; BW[cap, 0] = 255
    else:
        raise ValueError(case)
    A = mesh_arrays(d, mesh)
    n_tri = len(A["tri"])
    assert n_tri == (len(I) if I is not None else len(P) // 3)
    nodes = [int(k) for k in np.nonzero(nm == mesh)[0]]
    lights = posed_lights(d, mesh)
    counts = [int(light_table(d)[li, 7]) for li in lights]
    want = {"E1": (1, [2]), "E2": (1, [1152]), "E3": (2, [48, 24, 48]), "E4": (1, [1]), "E5": (1, [130]), "E6": (2, [n_tri, n_tri])}[case]
    assert len(nodes) == want[0] and counts == want[1], (case, nodes, counts)
    if case == "E5":
        assert len(A["woop"]) > n_tri + 20, "E5 is the case with duplicated references"
    return dict(case=case, scene="S3", setup=setup, width=width, height=height, plain=plain, mesh=mesh, P=np.ascontiguousarray(P, np.float32), N=None if N is None else np.ascontiguousarray(N, np.float32),
                I=I, BI=BI, BW=BW, n_bones=n_bones, B0=B0.astype(np.float32), B1=None if B1 is None else B1.astype(np.float32), lerp=lerp, n_tri=n_tri, n_rows=len(A["woop"]), nodes=nodes, lights=lights)


def light_table(desc):
    """the description's light records as uint32 words, (n_lights_buf, sizeof(ctl_light) / 4): type 0, area_dist_index 4, triangles_index 5, sum_area 6, count 7, node_idx 9"""
    import ctypes as C
    w = C.sizeof(api.ctl_light) // 4
    if not desc.n_lights_buf:
        return np.zeros((0, w), np.uint32)
    buf = (C.c_char * (desc.n_lights_buf * w * 4)).from_address(C.addressof(desc.lights.contents))
    return np.frombuffer(buf, dtype=np.uint32).reshape(-1, w).copy()


def anim_blob(desc):
    return desc.view("anim", np.uint8, desc.n_anim_bytes, 1)[:, 0].copy()


def tables_of(desc):
    return dict(lights=light_table(desc), anim=anim_blob(desc))


def posed_lights(desc, mesh):
    """the lights whose shape sets a pose of `mesh` recomputes: diffuse, with triangles, on a node that instances the mesh"""
    L = light_table(desc); nm = node_meshes(desc)
    return [int(i) for i in range(len(L)) if L[i, 0] == 2 and L[i, 7] > 0 and L[i, 9] < len(nm) and nm[L[i, 9]] == mesh]


def float_masks(desc, mesh):
    """(lights mask, anim mask in 32-bit words): the words a pose rewrites with floats — sum_area of the posed lights, their CDFs, and p, n, area (words 0..12) of their
    ctl_shape_tri records.  i_dat, t_dat, pad and everything else are outside"""
    L = light_table(desc)
    ml = np.zeros(L.shape, bool); ma = np.zeros(desc.n_anim_bytes // 4, bool)
    for li in posed_lights(desc, mesh):
        ml[li, 6] = True
        cdf, tri, count = int(L[li, 4]), int(L[li, 5]), int(L[li, 7])
        assert cdf % 4 == 0 and tri % 16 == 0
        ma[cdf // 4: cdf // 4 + count + 1] = True
        rec = ma[tri // 4: tri // 4 + 16 * count].reshape(count, 16)
        rec[:, :13] = True
    return ml, ma


def assert_tables_equal(got, want, desc, mesh, what=""):
    """the float words of the posed sets by same_bits (a NaN for a NaN); i_dat / t_dat / pad and every byte outside the posed sets exactly"""
    ml, ma = float_masks(desc, mesh)
    assert got["lights"].shape == want["lights"].shape and got["anim"].shape == want["anim"].shape, what
    gl, wl = got["lights"], want["lights"]
    assert np.array_equal(gl[~ml], wl[~ml]), "%s: light records outside sum_area of the posed lights differ" % what
    assert same_bits(gl[ml], wl[ml]), "%s: sum_area: %s against %s" % (what, gl[ml].view(np.float32), wl[ml].view(np.float32))
    n4 = len(ma) * 4
    ga, wa = got["anim"][:n4].view(np.uint32), want["anim"][:n4].view(np.uint32)
    assert np.array_equal(got["anim"][n4:], want["anim"][n4:]) and np.array_equal(ga[~ma], wa[~ma]), "%s: the anim blob outside the posed sets differs (%d words)" % (what, (ga[~ma] != wa[~ma]).sum())
    bad = (ga[ma] != wa[ma]) & ~(np.isnan(ga[ma].view(np.float32)) & np.isnan(wa[ma].view(np.float32)))
    assert not bad.any(), "%s: %d of %d float words of the posed shape sets differ" % (what, bad.sum(), ma.sum())


_cache = {}


def emitter_case(name, size=32):
    """(case, skin yardstick, host-updated builder, shape-set yardstick), made once and left unchanged.  Asserts that the skin yardstick's arrays are UpdateMesh's byte
    for byte (Woop rows: a NaN for a NaN)"""
    if (name, size) not in _cache:
        K = make_case(name, width=size, height=size)
        Y = yardstick(K)
        bent = host_updated(K, Y)
        A = mesh_arrays(bent.desc, K["mesh"])
        assert np.array_equal(Y["tri"], A["tri"]), "%s: %d TriangleData rows of the yardstick differ from UpdateMesh's: choose another pose" % (name, (Y["tri"] != A["tri"]).any(axis=1).sum())
        assert same_bits(Y["woop"], A["woop"]), "%s: Woop rows" % name
        S = api.shape_sets_host(K["plain"].desc, K["mesh"], Y["tri"], Y["woop"])
        _cache[(name, size)] = (K, Y, bent, S)
    return _cache[(name, size)]


def bind(scene, K, **kw):
    scene.bind_skin(K["mesh"], K["P"], K["I"], K["BI"], K["BW"], K["n_bones"], rest_normals=K["N"], **({"area_lights": True} if not kw else kw))
