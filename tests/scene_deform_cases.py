"""Deformations shared by tests/test_scene_deform_host.py and tests/test_gpu_scene_deform.py: DynamicScene.UpdateMesh on the scenes S1..S3 of
tests/scene_update_cases.py.  As there, the "old" and the "new" description of a pair come from two builders that build the same scene; the second one calls
UpdateMesh (and, where asked, SetNodeTransform) before its UpdateScene().

D1  a ripple along the normals, amplitude 4 % of the mesh radius: S1's instanced mesh (60 nodes), S3's ball (nodes 2 and 3) — one mesh, many nodes
D2  S2's beam mesh twisted by about 1 rad end to end and stretched 1.6 x across: the parts of its split references leave their clip boxes
D3  S3's ball with every vertex below a plane moved onto one point: tens of zero-area triangles (singular Woop rows); REVERSE builds the collapsed ball first
D4  S3's emissive panel stretched 1.8 x and bent: the area light's shape set, sum_area and CDF change with it
"""
import numpy as np

from cudatracerlib_amd import api
from scene_update_cases import build, motion_of, check_structure

CASES = (("D1", "S1"), ("D1", "S3"), ("D2", "S2"), ("D3", "S3"), ("D4", "S3"))
IDS = ["%s-%s" % c for c in CASES]
NO_PART = 0xffffffff


def node_meshes(desc):
    return desc.view("nodes", np.uint32, desc.n_nodes, 6)[:, 0].copy()


def mesh_of(case, scene, desc):
    """the mesh a case deforms"""
    nm = node_meshes(desc)
    if scene == "S1":
        return int(np.bincount(nm).argmax())        # the instanced mesh
    if scene == "S2":
        return int(nm[-1])                          # the beams
    return int(nm[4]) if case == "D4" else int(nm[2])   # S3: the emissive panel (node 4), the ball (nodes 2 and 3)


def nodes_of(desc, mesh):
    return [int(k) for k in np.nonzero(node_meshes(desc) == mesh)[0]]


def deformed_positions(case, P):
    P = np.asarray(P, np.float64)
    c = 0.5 * (P.min(axis=0) + P.max(axis=0))
    Q = P - c
    radius = np.linalg.norm(Q, axis=1).max()
    if case == "D1":
        n = Q / np.maximum(np.linalg.norm(Q, axis=1, keepdims=True), 1e-30)
        phase = 5.0 * Q[:, 0] / radius + 3.0 * Q[:, 1] / radius + 0.7
        out = P + n * (0.04 * radius * np.sin(phase))[:, None]
    elif case == "D2":
        ax = int(np.argmax(P.max(axis=0) - P.min(axis=0)))            # the long axis
        u, v = [k for k in range(3) if k != ax]
        a = 1.0 * (Q[:, ax] / (P[:, ax].max() - P[:, ax].min()))     # -0.5 .. 0.5 rad
        out = Q.copy()
        out[:, u] = np.cos(a) * Q[:, u] - np.sin(a) * Q[:, v]
        out[:, v] = np.sin(a) * Q[:, u] + np.cos(a) * Q[:, v]
        out[:, v] *= 1.6
        out += c
    elif case == "D3":
        plane = c[1] - 0.35 * radius
        out = P.copy()
        out[P[:, 1] < plane] = (c[0], plane, c[2])
    elif case == "D4":
        out = Q.copy()
        out[:, 0] *= 1.8
        out[:, 1] += 0.35 * Q[:, 0] * Q[:, 2] / radius
        out += c
    else:
        raise ValueError(case)
    return out.astype(np.float32)


def deform(case, scene, store=None):
    """edit(sc) for scene_update_cases.build: UpdateMesh of the case's mesh; store (a dict) receives mesh, positions and the arrays handed in"""
    def edit(sc):
        mesh = mesh_of(case, scene, sc.desc)
        inp = sc.mesh_inputs[mesh]
        P = deformed_positions(case, inp["positions"])
        sc.UpdateMesh(mesh, P, inp["indices"], normals=inp["normals"], uvs=inp["uvs"])
        if store is not None:
            store.update(mesh=mesh, positions=P, indices=inp["indices"], normals=inp["normals"], uvs=inp["uvs"])
    return edit


def build_pair(case, scene, width=32, height=32, reverse=False):
    """(old, new, mesh): new = old with the case's mesh deformed; reverse: the deformed scene is the old one"""
    info = {}
    plain, bent = build(scene, width=width, height=height), build(scene, width=width, height=height, edit=deform(case, scene, info))
    return (bent, plain, info["mesh"]) if reverse else (plain, bent, info["mesh"])


def build_deformed_and_moved(case, scene, motion, width=32, height=32):
    """the deformed scene with `motion` (scene_update_cases.motion_of) applied on top"""
    def edit(sc):
        deform(case, scene)(sc)
        for node, xf in motion_of(scene, motion, sc.desc).items():
            sc.SetNodeTransform(node, xf)
    return build(scene, width=width, height=height, edit=edit)


def mesh_arrays(desc, mesh):
    """the mesh's ranges of the geometry arrays as copies: tri_data (n, 8) uint32, woop (n, 12) uint32, woop_index (n,), bvh nodes (n, 16) uint32"""
    M = desc.view("meshes", np.uint32, desc.n_meshes, 5)
    def rng(col, div, total):
        starts = np.sort(M[:, col] // div)
        first = int(M[mesh, col] // div)
        later = starts[starts > first]
        return first, int(later[0]) if len(later) else total
    t0, t1 = rng(0, 1, desc.n_tri_data); n0, n1 = rng(1, 4, desc.n_bvh_nodes); w0, w1 = rng(2, 3, desc.n_woop)
    i0 = int(M[mesh, 3])
    return dict(tri=desc.view("tri_data", np.uint32, desc.n_tri_data, 8)[t0:t1].copy(), woop=desc.view("woop", np.uint32, desc.n_woop, 12)[w0:w1].copy(),
                widx=desc.view("woop_index", np.uint32, desc.n_woop, 1)[i0:i0 + (w1 - w0), 0].copy(), nodes=desc.view("bvh_nodes", np.uint32, desc.n_bvh_nodes, 16)[n0:n1].copy(),
                tri_range=(t0, t1))


def entries_of(fb, desc, mesh):
    """mask over the leaf entries of a flattened tree: those whose node instances `mesh`"""
    return np.isin(fb.leaves()[:, 13], nodes_of(desc, mesh))


def check_structure_with_collapsed(fb, desc, built_from, inner_high_steps):
    """scene_update_cases.check_structure for a tree that holds COLLAPSED triangles (D3): an entry whose Woop rows are singular has no vertices to contain — the
    function there inverts every entry's matrix — and can never be hit, so it is left out; every other entry and every inner slot is held to the same conditions,
    restated here with that one exception.  Returns (split references, collapsed entries, high-side excess of the inner slots in steps of the child's grid)."""
    from scene_update_cases import decode_q4, entry_vertices, clip_polygon, ULP4
    N, L, ch = fb.nodes(), fb.leaves(), fb.child_links()
    lo, hi, exist, leafm = decode_q4(N)
    rows = L[:, :12].copy().view(np.float32).astype(np.float64).reshape(-1, 3, 4)
    M = np.zeros((len(L), 4, 4)); M[:, 0] = rows[:, 1]; M[:, 1] = rows[:, 2]; M[:, 2] = rows[:, 0]; M[:, 2, 3] *= -1; M[:, 3, 3] = 1
    with np.errstate(all="ignore"):
        det = np.linalg.det(M)
    regular = np.isfinite(rows).all(axis=(1, 2)) & np.isfinite(det) & (det != 0)
    if regular.all():
        n, excess = check_structure(fb, desc, built_from=built_from, inner_high_steps=inner_high_steps)
        return n, 0, excess
    V = np.full((len(L), 3, 3), np.nan); V[regular] = entry_vertices(L[regular], desc)
    tol = ULP4 * np.nanmax(np.abs(V))
    slot_of = np.full((len(L), 2), -1, np.int64)
    excess = 0.0
    inverted = np.zeros((len(N), 4), bool)
    for k in range(3):
        for c in range(4):
            inverted[:, c] |= ((N[:, 4 + 2 * k] >> (8 * c)) & 255) > ((N[:, 5 + 2 * k] >> (8 * c)) & 255)
    for c in range(4):
        inner = (((exist & ~leafm) >> c) & 1) == 1
        kids = ch[inner, c] // 4
        # a slot under which only collapsed triangles are left carries the codes of a missing child (lo > hi): nothing to contain, and nothing reaches it
        has = ((((exist[kids][:, None] >> np.arange(4)[None, :]) & 1) == 1) & ~inverted[kids])[..., None]
        klo = np.where(has, lo[kids], np.inf).min(axis=1); khi = np.where(has, hi[kids], -np.inf).max(axis=1)
        e = np.stack([(N[kids, 3] >> (8 * k)) & 255 for k in range(3)], axis=1).astype(np.int64)
        grid = np.ldexp(1.0, e - 127)
        assert inverted[inner, c][~has.any(axis=(1, 2))].all(), "a node without anything under it must not be reachable"
        assert (klo >= lo[inner, c] - tol).all(), "an inner slot box does not contain its child's boxes (low side)"
        over = np.maximum(khi - hi[inner, c] - tol, 0.0) / grid
        if over.size:
            excess = max(excess, float(over.max()))
            assert (over <= inner_high_steps).all(), "an inner slot box does not contain its child's boxes (high side: %.4f steps)" % over.max()
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
    whole = part_index == NO_PART
    assert whole[~regular].all()
    w = whole & regular
    assert (V[w] >= slo[w, None, :] - tol).all() and (V[w] <= shi[w, None, :] + tol).all(), "a leaf slot box does not contain its triangle"
    V0 = np.full_like(V, np.nan); V0[regular] = entry_vertices(L[regular], built_from)
    X0 = desc.view("node_transforms", np.float32, desc.n_nodes, 16).reshape(-1, 4, 4).astype(np.float64); X1 = X0
    X0 = built_from.view("node_transforms", np.float32, built_from.n_nodes, 16).reshape(-1, 4, 4).astype(np.float64)
    for e in np.nonzero(~whole)[0]:
        b = part_boxes[part_index[e]].astype(np.float64)
        poly = clip_polygon(V0[e].copy(), b[:3], b[3:])
        assert len(poly) >= 3
        P = X1[L[e, 13]] @ np.linalg.inv(X0[L[e, 13]])
        moved = poly @ P[:3, :3].T + P[:3, 3]
        t = ULP4 * max(np.abs(moved).max(), np.abs(V[e]).max())
        assert (moved >= slo[e] - t).all() and (moved <= shi[e] + t).all(), "a leaf slot box does not contain the part of its split reference (entry %d)" % e
    return int((~whole).sum()), int((~regular).sum()), excess
