"""Skins and poses shared by tests/test_skin_host.py and tests/test_gpu_skin.py: ctl_scene_bind_skin / ctl_scene_animate_mesh on the scenes S1..S3 of
tests/scene_update_cases.py.  Bones come from position bands along the mesh's long axis, with blended weights (uint8, a weight is byte / 255).

K1  S1's instanced icosphere, 3 bones: a bend
K2  S2's beams, 2 bones: a twist about the vertical axis plus a stretch; the split references of the flattened tree become whole
K3  S3's ball, 256 bones with index byte 255 in use, weights that do NOT sum to 255 (TransformPoint divides by w), lerp in {0, 0.37, 1} and bones1 == NULL
K4  S3's ball with every influence of the lower cap on one zero-scale bone: collapsed triangles, singular Woop rows
K5  S2's beams bound as a triangle soup (indices None) and without rest normals (computed once at bind time)
K6  S3 with one more node: 130 long thin triangles (the soup tests/test_sbvh.py builds its spatial splits from), 390 vertices — two workgroups of k_skin_vertices, the
    second one partly filled — whose mesh BVH duplicates references: MORE ROWS THAN TRIANGLES in the Woop stream.  3 bones: a bend

Every pose keeps its mesh inside the box of the rest of the scene, so that the host-updated description (DynamicScene.UpdateMesh of the yardstick's vertices) keeps
box_min, box_max and ray_trace_eps of the original and frames of the two can be compared; host_updated() asserts it.  S2's beams carry the top of their scene's box:
K2 / K5 leave y alone — rows 1 and 3 of both bones are those of the identity and every weight pair sums to exactly 1.0f (EXACT_PAIRS), so y' = (1 * y) / 1.
"""
import numpy as np

from cudatracerlib_amd import api
from scene_update_cases import build
from scene_deform_cases import mesh_of, mesh_arrays, node_meshes

CASES = ("K1", "K2", "K3-0", "K3-0.37", "K3-1", "K3-null", "K4", "K5", "K6")
SCENE_OF = {"K1": "S1", "K2": "S2", "K3": "S3", "K4": "S3", "K5": "S2", "K6": "S3"}
DEFORM_OF = {"K1": "D1", "K2": "D2", "K3": "D1", "K4": "D1", "K5": "D2"}     # which mesh: scene_deform_cases.mesh_of

# byte pairs (a, 255 - a) whose weights add up to 1.0f exactly, in fp32, in d_Compute's order
_f = np.float32
EXACT_PAIRS = [a for a in range(256) if (_f(a) / _f(255.0)) + (_f(255 - a) / _f(255.0)) == _f(1.0)]
assert 0 in EXACT_PAIRS and 255 in EXACT_PAIRS and len(EXACT_PAIRS) > 32


def _rot(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _affine(lin, about, shift=(0, 0, 0)):
    """x -> lin (x - about) + about + shift as a row-major 4 x 4"""
    M = np.eye(4); M[:3, :3] = lin; M[:3, 3] = np.asarray(about) - lin @ np.asarray(about) + np.asarray(shift)
    return M


def _bands(P, n_bones, exact):
    """bone bytes from position bands along the long axis: a vertex is held by the two bones whose band centres enclose it, linearly blended.  exact: weight pairs
    from EXACT_PAIRS only"""
    P = np.asarray(P, np.float64)
    ax = int(np.argmax(P.max(axis=0) - P.min(axis=0)))
    t = (P[:, ax] - P[:, ax].min()) / (P[:, ax].max() - P[:, ax].min()) * (n_bones - 1)
    lo = np.minimum(np.floor(t).astype(np.int64), n_bones - 2) if n_bones > 1 else np.zeros(len(P), np.int64)
    w_hi = np.clip(np.round((t - lo) * 255.0), 0, 255).astype(np.int64)
    if exact:
        E = np.array(EXACT_PAIRS)
        w_hi = E[np.abs(E[None, :] - w_hi[:, None]).argmin(axis=1)]
    BI = np.zeros((len(P), 8), np.uint8); BW = np.zeros((len(P), 8), np.uint8)
    BI[:, 0] = lo; BI[:, 1] = np.minimum(lo + 1, n_bones - 1); BW[:, 0] = 255 - w_hi; BW[:, 1] = w_hi
    return BI, BW, ax


def add_ribbons(sc):
    """K6's extra node: a mesh of long thin triangles in the middle of S3's room, far enough from the walls for any rotation"""
    rs = np.random.RandomState(11)
    n = 130
    c = rs.uniform(-5, 5, (n, 1, 3)); d = rs.normal(size=(n, 1, 3)) * rs.uniform(0.1, 6, (n, 1, 1)); e = rs.normal(size=(n, 3, 3)) * 0.15
    T = (c + d * np.array([[-1], [0], [1]])[None] + e).reshape(-1, 3)
    V = (T / np.abs(T).max()).astype(np.float32)
    mesh = sc.add_mesh(V, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), materials=[api.diffuse((0.7, 0.4, 0.2), two_sided=True)])
    sc.CreateNode(mesh, np.array([[100, 0, 0, 278.0], [0, 100, 0, 275.0], [0, 0, 100, 280.0], [0, 0, 0, 1]], np.float32))


def make_case(case, width=32, height=32):
    """dict(scene, plain (the DynamicScene), mesh, P, N, I (None: soup), BI, BW, n_bones, B0, B1 (None: bones0), lerp, n_tri, n_rows)"""
    key = case.split("-")[0]
    scene = SCENE_OF[key]
    setup = add_ribbons if key == "K6" else None
    plain = build(scene, width=width, height=height, edit=setup)
    mesh = int(node_meshes(plain.desc)[-1]) if key == "K6" else mesh_of(DEFORM_OF[key], scene, plain.desc)
    inp = plain.mesh_inputs[mesh]
    P, I, N = inp["positions"], inp["indices"], inp["normals"]
    assert inp["uvs"] is None
    c = 0.5 * (P.min(axis=0).astype(np.float64) + P.max(axis=0))
    B1 = None; lerp = 0.0
    if key in ("K1", "K6"):
        n_bones = 3
        BI, BW, ax = _bands(P, n_bones, False)
        axis = np.eye(3)[(ax + 1) % 3]
        B0 = np.stack([_affine(_rot(axis, a), c) for a in (-0.35, 0.0, 0.35)])
        B1 = np.stack([_affine(_rot(axis, a) @ np.diag([1.0, 0.9, 1.1]), c, s) for a, s in ((-0.2, (0.05, 0, 0)), (0.1, (0, 0.05, 0)), (0.3, (0, 0, -0.05)))])
        lerp = 0.25
    elif key in ("K2", "K5"):
        n_bones = 2
        if key == "K5":                       # a soup: three vertices of its own per triangle, no normals
            P = P[I.reshape(-1)].copy(); I = None; N = None
        BI, BW, ax = _bands(P, n_bones, True)
        about = np.array([c[0], 0.0, c[2]])
        B0 = np.stack([_affine(_rot((0, 1, 0), a) @ np.diag([sx, 1.0, sz]), about) for a, sx, sz in ((-0.22, 0.72, 0.7), (0.2, 0.66, 0.74))])
        B0[:, 1, :] = (0, 1, 0, 0)            # y stays, to the bit
        if key == "K5":
            B1 = np.stack([_affine(np.diag([0.7, 1.0, 0.7]), about), _affine(_rot((0, 1, 0), 0.1) @ np.diag([0.6, 1.0, 0.75]), about)]); B1[:, 1, :] = (0, 1, 0, 0)
            lerp = 0.5                        # y * 0.5 + y * 0.5 == y
    elif key == "K3":
        n_bones = 256
        BI, BW, ax = _bands(P, n_bones, False)
        assert BI.max() == 255
        rs = np.random.RandomState(5)
        # four influences, none of the sums 255: the two band bones at a reduced or raised weight, two neighbours further off
        BI[:, 2] = np.maximum(BI[:, 0].astype(np.int64) - 3, 0); BI[:, 3] = np.minimum(BI[:, 1].astype(np.int64) + 5, 255)
        BW[:, 0] = (BW[:, 0] * 0.7).astype(np.uint8); BW[:, 1] = (BW[:, 1] * 0.7).astype(np.uint8); BW[:, 2] = rs.randint(1, 60, len(P)); BW[:, 3] = rs.randint(1, 200, len(P))
        BI[:, 4:] = rs.randint(0, 256, (len(P), 4))      # zero weights: the matrix is read all the same
        sums = BW.astype(np.int64).sum(axis=1)
        assert (sums != 255).all() and (sums < 255).any() and (sums > 255).any()
        k = np.arange(256) / 255.0
        axis = np.eye(3)[(ax + 1) % 3]
        B0 = np.stack([_affine(_rot(axis, 0.5 * (x - 0.5)) * (0.9 + 0.05 * np.sin(7 * x)), c, (0.0, 0.03 * np.cos(5 * x), 0.0)) for x in k])   # inside the unit ball: the instances nearly touch the floor
        B1 = np.stack([_affine(_rot((0.3, 1.0, 0.2), 0.6 * (0.5 - x)), c, (0.05 * x, 0.0, -0.05 * x)) for x in k])
        tail = case.split("-")[1]
        if tail == "null":
            B1 = None; lerp = 0.37
        else:
            lerp = float(tail)
    elif key == "K4":
        n_bones = 4
        BI, BW, ax = _bands(P, 3, False)
        B0 = np.stack([_affine(_rot((0, 0, 1), a), c) for a in (-0.1, 0.0, 0.1)] + [np.zeros((4, 4))])
        radius = np.linalg.norm(P - c, axis=1).max()
        plane = c[1] - 0.35 * radius
        B0[3, :3, 3] = (c[0], plane, c[2]); B0[3, 3, 3] = 1.0        # zero scale: everything it holds lands on one point
        cap = P[:, 1] < plane
        assert 10 < cap.sum() < len(P) // 2
        BI[cap] = 3; BW[cap] = 0; BW[cap, 0] = 255
    else:
        raise ValueError(case)
    n_vert = len(P)
    assert n_vert % 64 != 0, "the tail lanes of the last wave must be covered"
    A = mesh_arrays(plain.desc, mesh)
    n_tri = len(A["tri"])
    assert n_tri == (len(I) if I is not None else n_vert // 3)
    if key == "K6":
        assert len(A["woop"]) > n_tri + 20 and n_vert > 256 and n_vert % 256 != 0, "K6 is the case with duplicated references and more than one workgroup of vertices"
        assert len(np.unique(A["widx"] >> 1)) == n_tri
    return dict(case=case, scene=scene, setup=setup, width=width, height=height, plain=plain, mesh=mesh, P=np.ascontiguousarray(P, np.float32), N=None if N is None else np.ascontiguousarray(N, np.float32), I=I, BI=BI, BW=BW, n_bones=n_bones,
                B0=B0.astype(np.float32), B1=None if B1 is None else B1.astype(np.float32), lerp=lerp, n_tri=n_tri, n_rows=len(A["woop"]))


def yardstick(K):
    """ctl_skin_mesh_host of a case"""
    return api.skin_mesh_host(K["plain"].desc, K["mesh"], K["P"], K["I"], K["BI"], K["BW"], K["n_bones"], K["B0"], K["B1"], K["lerp"], rest_normals=K["N"], n_rows=K["n_rows"])


def host_updated(K, Y, edit=None):
    """the case's scene built again and updated on the host to the yardstick's vertices: DynamicScene.UpdateMesh.  edit(sc): further calls before UpdateScene().
    Asserts that the pose left the scene box alone."""
    def apply(sc):
        if K["setup"]:
            K["setup"](sc)
        sc.UpdateMesh(K["mesh"], Y["positions"], K["I"], normals=Y["normals"], uvs=None)
        if edit:
            edit(sc)
    bent = build(K["scene"], width=K["width"], height=K["height"], edit=apply)
    if edit is None:
        a, b = K["plain"].desc, bent.desc
        assert list(a.box_min) == list(b.box_min) and list(a.box_max) == list(b.box_max) and a.ray_trace_eps == b.ray_trace_eps, "the pose moves the scene box"
    return bent


def bind(scene, K):
    scene.bind_skin(K["mesh"], K["P"], K["I"], K["BI"], K["BW"], K["n_bones"], rest_normals=K["N"])


def animate(scene, K):
    return scene.animate_mesh(K["mesh"], K["B0"], K["B1"], K["lerp"])


def same_bits(a, b):
    """uint32 words equal, a NaN for a NaN (a device-made NaN need not carry x86's sign bit), -0 is not +0; arrays of float32 or of uint32 words that hold floats"""
    a = np.ascontiguousarray(a).view(np.uint32); b = np.ascontiguousarray(b).view(np.uint32)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a.view(np.float32)) & np.isnan(b.view(np.float32))
    return bool(((a == b) | both_nan).all())


def normal_codes(tri):
    """the three 16-bit normal codes of every TriangleData row, (n, 3)"""
    return np.stack([tri[:, 0] & 0xffff, tri[:, 0] >> 16, tri[:, 1] & 0xffff], axis=1).astype(np.int64)


def without_codes(tri):
    t = tri.copy(); t[:, 0] = 0; t[:, 1] &= 0xffff0000
    return t


def code_steps(a, b):
    """(codes that differ, codes that differ by more than one step in theta or in phi — phi modulo 255)"""
    ca, cb = normal_codes(a), normal_codes(b)
    dt = np.abs((ca >> 8) - (cb >> 8)); dp = np.abs((ca & 255) - (cb & 255)); dp = np.minimum(dp, 255 - dp)
    return int(((dt != 0) | (dp != 0)).sum()), int(((dt > 1) | (dp > 1)).sum())
