"""Scenes, motions and checks shared by tests/test_scene_update_host.py and tests/test_gpu_scene_update.py.

A ctl_scene_desc points into its builder, and a second UpdateScene() of the same builder rewrites the arrays the first one points to.  So the "old" and
the "new" description of a pair always come from two builders that build the same scene: build(scene, motion) makes one, with `motion` applied through
DynamicScene.SetNodeTransform before its UpdateScene().

S1  the multi-node scene of test_oracle_flat.py::test_flat_traversal_equals_two_level (61 nodes)
S2  the long-beam scene of test_early_split_clipping_keeps_every_hit: the beam node (and the floor) carry split references
S3  a Cornell box with its glass sphere, two instances of a ball mesh and an emissive panel (an area light on a node that M2 moves)

M1  a small rigid move of one node
M2  a rotation by an arbitrary angle plus a non-uniform scale of two nodes
M3  a large move that carries one node through another
"""
import ctypes as C

import numpy as np

from cudatracerlib_amd import api, scenes

SCENES = ("S1", "S2", "S3")
MOTIONS = ("M1", "M2", "M3")


def _base(scene, width=32, height=32, ball_material=None):
    if scene == "S1":
        return scenes.synthetic_sm(width, height, n_instances=60, subdiv=2)
    if scene == "S2":
        return scenes.beams_over_spheres(width, height)
    sc = scenes.cornell_box(width, height, glass_sphere=True)     # node 0 the room (area light on its material 3), node 1 the glass sphere
    V, F = scenes.icosphere(2)
    ball = sc.add_mesh(V, F, normals=V, materials=[ball_material if ball_material is not None else api.diffuse((0.3, 0.5, 0.7))])
    for r, p in ((55.0, (400.0, 60.0, 150.0)), (40.0, (120.0, 300.0, 380.0))):                                   # nodes 2 and 3: two instances of one mesh
        sc.CreateNode(ball, np.array([[r, 0, 0, p[0]], [0, r, 0, p[1]], [0, 0, r, p[2]], [0, 0, 0, 1]], np.float32))
    P = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], np.float32)
    panel = sc.add_mesh(P, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), normals=np.tile(np.array([0, -1, 0], np.float32), (4, 1)), materials=[api.diffuse((0.5, 0.5, 0.5), two_sided=True)])
    node = sc.CreateNode(panel, np.array([[40, 0, 0, 420.0], [0, 40, 0, 420.0], [0, 0, 40, 300.0], [0, 0, 0, 1]], np.float32))   # node 4: an emissive panel
    sc.CreateLight(node, 0, (30.0, 26.0, 20.0))
    sc.UpdateScene()
    return sc


def node_transforms(desc):
    return desc.view("node_transforms", np.float32, desc.n_nodes, 16).reshape(-1, 4, 4).astype(np.float64)


def _rot(axis, angle):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _about(X, lin):
    """X with the linear map `lin` applied about the node's own world position"""
    Y = X.copy(); Y[:3, :3] = lin @ X[:3, :3]
    return Y


def motion_of(scene, motion, desc):
    """{node: new to_world (4 x 4, float32)}"""
    X = node_transforms(desc)
    lo, hi = np.array(desc.box_min[:]), np.array(desc.box_max[:]); size = hi - lo
    if scene == "S1":
        a, b = 7, 23
    elif scene == "S2":
        a, b = desc.n_nodes - 1, 5          # the beams (split references), a sphere
    else:
        a, b = 2, 4                         # a sphere instance, the emissive panel
    out = {}
    if motion == "M1":
        Y = X[a].copy(); Y[:3, 3] += 0.013 * size * np.array([1.0, 0.4, -0.7])
        out[a] = Y
    elif motion == "M2":
        out[a] = _about(X[a], _rot((0.3, 1.0, 0.2), 0.7312) @ np.diag([1.3, 0.8, 1.1]))
        out[b] = _about(X[b], _rot((1.0, 0.1, -0.4), -1.234) @ np.diag([0.7, 1.25, 1.6]))
        if scene == "S2":                   # the beams span the hall: also shift them, so that parts leave their old cells
            out[a][:3, 3] += 0.05 * size
    else:
        if scene == "S1":
            Y = X[a].copy(); Y[:3, 3] = X[b][:3, 3] + 0.02 * size   # into node b
        elif scene == "S2":
            Y = X[a].copy(); Y[:3, 3] += np.array([0.0, -0.35, 0.0]) * size + np.array([0.3, 0.0, 0.2]) * size   # the beams down through the spheres
        else:
            Y = X[a].copy(); Y[:3, 3] = np.array([368.0, 200.0, 351.0])   # the sphere into the tall block
        out[a] = Y
    return {k: v.astype(np.float32) for k, v in out.items()}


def build(scene, motion=None, width=32, height=32, edit=None, ball_material=None):
    """a DynamicScene after UpdateScene(); motion: None or M1 / M2 / M3; edit(sc): further calls on the builder before UpdateScene(); ball_material: the BSDF of
    S3's instanced ball mesh (default: a blue diffuse)"""
    sc = _base(scene, width, height, ball_material)
    if motion:
        for node, xf in motion_of(scene, motion, sc.desc).items():
            sc.SetNodeTransform(node, xf)
    if edit:
        edit(sc)
    if motion or edit:
        sc.UpdateScene()
    return sc


def with_materials(desc, edit):
    """a copy of `desc` whose materials are a private array, after edit(materials); the copy keeps the array alive"""
    d = api.ctl_scene_desc.from_buffer_copy(desc)
    mats = (api.ctl_material * desc.n_materials)()
    C.memmove(mats, desc.materials, C.sizeof(mats))
    edit(mats)
    d.materials = C.cast(mats, type(desc.materials))
    d._keep = (mats, desc)
    return d


def rays_for_update(desc, n, seed, aim_nodes=()):
    """n rays: a third through the camera's film, the rest random through the scene box (test_oracle_flat.rays_for), a tenth of those turned towards the
    origins of `aim_nodes` (the nodes that moved)"""
    from test_oracle_flat import rays_for
    r = rays_for(desc, n, seed)
    rs = np.random.RandomState(seed + 1)
    k = n // 3
    cam = np.array(desc.camera.to_world[:], np.float64).reshape(4, 4)
    t = np.tan(desc.camera.fov / 2.0); aspect = desc.camera.resolution[0] / desc.camera.resolution[1]
    xy = rs.uniform(-1, 1, size=(k, 2))
    d = cam[:3, 2][None, :] + xy[:, :1] * t * cam[:3, 0][None, :] + xy[:, 1:] * (t / aspect) * cam[:3, 1][None, :]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r[6:6 + k, :3] = cam[:3, 3]; r[6:6 + k, 4:7] = d
    if len(aim_nodes):
        m = n // 10
        X = node_transforms(desc)[np.asarray(aim_nodes)[rs.randint(0, len(aim_nodes), size=m)]]
        target = X[:, :3, 3] + np.einsum("nij,nj->ni", X[:, :3, :3], rs.uniform(-0.3, 0.3, size=(m, 3)))
        d = target - r[n - m:, :3]; d /= np.linalg.norm(d, axis=1, keepdims=True)
        r[n - m:, 4:7] = d
    return r


def assert_same_hits(got, want, what=""):
    """(t, u, v, triangle, node) bit for bit; a ray may differ only as a verified tie: bit-equal t on both sides and another triangle"""
    differs = np.zeros(len(want), bool)
    for k in ("dist", "u", "v"):
        differs |= got[k].view(np.uint32) != want[k].view(np.uint32)
    for k in ("tri_idx", "node_idx"):
        differs |= got[k] != want[k]
    tie = (got["dist"].view(np.uint32) == want["dist"].view(np.uint32)) & (got["tri_idx"] != want["tri_idx"]) & (got["tri_idx"] >= 0) & (want["tri_idx"] >= 0)
    bad = differs & ~tie
    assert not bad.any(), "%s: %d rays differ (first %d: got %s, want %s)" % (what, bad.sum(), np.nonzero(bad)[0][0], got[bad][0], want[bad][0])
    return int(tie.sum())


def decode_q4(N):
    """Q4 nodes (n, 16) uint32 -> lo, hi (n, 4, 3) float64 by the formula of csrc/flatten.h:32, exist and leaf masks"""
    origin = N[:, :3].copy().view(np.float32).astype(np.float64)
    e = np.stack([(N[:, 3] >> (8 * k)) & 255 for k in range(3)], axis=1).astype(np.int64)
    step = np.ldexp(1.0, e - 127)
    lo = np.zeros((len(N), 4, 3)); hi = np.zeros((len(N), 4, 3))
    for k in range(3):
        for c in range(4):
            lo[:, c, k] = origin[:, k] + step[:, k] * ((N[:, 4 + 2 * k] >> (8 * c)) & 255)
            hi[:, c, k] = origin[:, k] + step[:, k] * ((N[:, 5 + 2 * k] >> (8 * c)) & 255)
    exist = (N[:, 3] >> 24) & 15
    return lo, hi, exist, (N[:, 3] >> 28) & exist


def entry_vertices(L, desc):
    """world-space vertices (n, 3, 3) of every leaf entry in float64: the object-space vertices from the Woop rows, through the node's to_world"""
    R = L[:, :12].copy().view(np.float32).astype(np.float64).reshape(-1, 3, 4)
    M = np.zeros((len(L), 4, 4)); M[:, 0] = R[:, 1]; M[:, 1] = R[:, 2]; M[:, 2] = R[:, 0]; M[:, 2, 3] *= -1; M[:, 3, 3] = 1
    Mi = np.linalg.inv(M)
    v2 = Mi[:, :3, 3]; v0 = v2 + Mi[:, :3, 0]; v1 = v2 + Mi[:, :3, 1]
    V = np.stack([v0, v1, v2], axis=1)
    X = node_transforms(desc)[L[:, 13]]
    return np.einsum("nij,nvj->nvi", X[:, :3, :3], V) + X[:, None, :3, 3]


# The allowance of the containment checks: 4 fp32 ulps of the largest coordinate magnitude involved.  It accounts for the fp32 rounding of the transform (the
# library rounds its float64 vertices outwards to fp32, and pads), not for the quantisation, which rounds outwards.  (The high side of the inner-slot check needs
# more; how much is measured on a freshly built tree of the same pose: see check_structure.)
ULP4 = 4 * 2.0 ** -23


def clip_polygon(poly, lo, hi):
    """Sutherland-Hodgman in float64: the convex polygon (n, 3) inside the box [lo, hi]"""
    for ax in range(3):
        for bound, keep_below in ((hi[ax], True), (lo[ax], False)):
            out = []
            for i in range(len(poly)):
                a, c = poly[i], poly[(i + 1) % len(poly)]
                ia = a[ax] <= bound if keep_below else a[ax] >= bound
                ic = c[ax] <= bound if keep_below else c[ax] >= bound
                if ia:
                    out.append(a)
                if ia != ic:
                    t = (bound - a[ax]) / (c[ax] - a[ax]); p = a + t * (c - a); p[ax] = bound
                    out.append(p)
            poly = np.array(out).reshape(-1, 3)
            if len(poly) == 0:
                return poly
    return poly


def check_structure(fb, desc, built_from=None, inner_high_steps=None):
    """The containment checks of a Q4 tree that holds the pose of `desc`; built_from: the description the tree was BUILT from (default: desc itself).
      * every inner child's slot box contains that child's own slot boxes: on the low side within the fp32 allowance; on the high side the child's boxes, codes on
        the child's own grid rounded up, can stand out.  By how much is MEASURED, in steps of the child's grid: with inner_high_steps=None the function only measures
        and returns the figure; the caller measures a freshly built tree of the same pose and hands that figure, in whole steps, in for the tree under test;
      * every leaf slot box contains its entries' world-space part, in float64 from the object-space vertices and to_world: the three vertices of an entry that stands
        for its whole triangle; for a split reference the triangle of the built pose clipped against the reference's clip box (the tree's side data) and carried to
        the pose of `desc` — the moved triangle clipped against the moved clip box.
    Returns (split references, high-side excess of the inner slots in steps of the child's grid)."""
    N, L, ch = fb.nodes(), fb.leaves(), fb.child_links()
    lo, hi, exist, leafm = decode_q4(N)
    V = entry_vertices(L, desc)
    tol = ULP4 * np.abs(V).max()
    slot_of = np.full((len(L), 2), -1, np.int64)
    excess = 0.0
    for c in range(4):
        inner = (((exist & ~leafm) >> c) & 1) == 1
        kids = ch[inner, c] // 4
        has = (((exist[kids][:, None] >> np.arange(4)[None, :]) & 1) == 1)[..., None]
        klo = np.where(has, lo[kids], np.inf).min(axis=1)
        khi = np.where(has, hi[kids], -np.inf).max(axis=1)
        e = np.stack([(N[kids, 3] >> (8 * k)) & 255 for k in range(3)], axis=1).astype(np.int64)
        grid = np.ldexp(1.0, e - 127)
        assert (klo >= lo[inner, c] - tol).all(), "an inner slot box does not contain its child's boxes (low side)"
        over = np.maximum(khi - hi[inner, c] - tol, 0.0) / grid
        if over.size:
            excess = max(excess, float(over.max()))
        if inner_high_steps is not None:
            assert (over <= inner_high_steps).all(), "an inner slot box does not contain its child's boxes (high side: %.4f steps of the child's grid, a fresh tree needs %.4f)" % (over.max(), inner_high_steps)
        for i in np.nonzero(((leafm >> c) & 1) == 1)[0]:
            e = ~ch[i, c]
            while True:
                slot_of[e] = (i, c)
                if L[e, 12] & 1:
                    break
                e += 1
    assert (slot_of[:, 0] >= 0).all()
    slo, shi = lo[slot_of[:, 0], slot_of[:, 1]], hi[slot_of[:, 0], slot_of[:, 1]]
    part_index, part_boxes = fb.parts()
    assert part_index is not None, "the tree carries no refit side data"
    whole = part_index == 0xffffffff
    assert (V[whole] >= slo[whole, None, :] - tol).all() and (V[whole] <= shi[whole, None, :] + tol).all(), "a leaf slot box does not contain its triangle"
    d0 = built_from if built_from is not None else desc
    V0 = entry_vertices(L, d0)
    X0, X1 = node_transforms(d0), node_transforms(desc)
    for e in np.nonzero(~whole)[0]:
        b = part_boxes[part_index[e]].astype(np.float64)
        poly = clip_polygon(V0[e].copy(), b[:3], b[3:])
        assert len(poly) >= 3, "a split reference whose clip box misses its triangle"
        P = X1[L[e, 13]] @ np.linalg.inv(X0[L[e, 13]])
        moved = poly @ P[:3, :3].T + P[:3, 3]
        t = ULP4 * max(np.abs(moved).max(), np.abs(V[e]).max())
        assert (moved >= slo[e] - t).all() and (moved <= shi[e] + t).all(), "a leaf slot box does not contain the part of its split reference (entry %d)" % e
    return int((~whole).sum()), excess
