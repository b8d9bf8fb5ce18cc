"""Scenes, ray sets and the comparison rule of the traversal-variant tests: shared by tests/test_oracle_traversal_cases.py (CPU: the inputs are what they claim to be) and
tests/test_gpu_traversal_variants.py (GPU: every traversal kernel variant against the oracle, ray by ray).  Plain Python, no test in here.

 * telescope(): one mesh whose triangles shrink geometrically towards the origin along the z axis.  Its BVHs are as deep as a few hundred triangles can make them, and a
   ray that starts near the apex and runs OUTWARD finds, level after level, that the child it enters first is the inner "rest of the chain": the siblings wait on the
   stack, which grows past the rows the kernels keep in LDS.  The same scene walked inward is shallow.
 * alpha_thicket(): a floor and a few hundred overlapping two-sided cards whose triangles cycle through the three alpha-map kinds and no alpha map at all, so that leaves
   mix alpha-tested and plain entries and a rejected candidate is regularly followed by a farther one.
"""
import numpy as np
from cudatracerlib_amd import api, scenes

FLT_MAX = np.float32(3.402823466e+38)
LAYOUTS = (None, "q4", "q8")                  # None: the two-level structure


def make_rays(o, d, tmin, tmax):
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((len(o), 8), np.float32)
    rays[:, :3] = o; rays[:, 3] = tmin; rays[:, 4:7] = d; rays[:, 7] = tmax
    return rays


def random_rays(desc, n, seed, any_tmax=False):
    """origins in the scene's box (10 % margin), uniform directions; any_tmax: tmax inside the scene; six axis-aligned directions first"""
    rs = np.random.RandomState(seed)
    lo, hi = np.array(desc.box_min[:]), np.array(desc.box_max[:])
    o = rs.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), size=(n, 3))
    rays = make_rays(o, rs.normal(size=(n, 3)), desc.ray_trace_eps, FLT_MAX)
    if any_tmax:
        rays[:, 7] = rs.uniform(0.05, 1.0, size=n) * np.linalg.norm(hi - lo)
    k = min(n, 6)
    rays[:k, 4:7] = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)[:k]
    return rays


# ---------------------------------------------------------------------------------------------------------------- telescope
# Three sizes of the telescope, because the five stacks fill under different conditions (measured with the oracle's stack figures, RESULTS.md "Traversal variants"):
#  chain  the mesh of the issue: 140 single triangles, ratio 0.85.  The 4-wide tree is a chain that pushes three siblings per level: Q4 stacks reach entry 56.
#  long   268 triangles from 1.5e9 down to 1e-10.  A binary SAH tree over a geometric chain peels about eleven shells per level whatever the ratio, so its depth
#         grows only with the RANGE of sizes.  This is the whole range in which the builder keeps every triangle; it gives the two-level stack 28 entries.
#  fan    30 shells of ten triangles with a gap of half a turn, ratio 0.5.  An 8-wide node keeps single triangles in leaf slots, which never wait on the stack; only
#         shells of many triangles become inner children, and only then does a level leave a sibling GROUP waiting.
# exps: the outward rays start at 0.5 first ratio^U(exps) — deep enough in the chain that the entries the hit depends on lie beyond the LDS rows.
TELESCOPES = {
    "chain": dict(n_shells=140, ratio=0.85, first=1.0, fan=1, gap=0.0, exps=(20, 120)),
    "long": dict(n_shells=268, ratio=0.85, first=1.5e9, fan=1, gap=0.0, exps=(242, 264)),
    "fan": dict(n_shells=30, ratio=0.5, first=1.0, fan=10, gap=0.5, exps=(25, 29)),
}
# the five kernel families: (name, layout, single-ray, LDS rows, telescope).  The rows are csrc/traverse.h kLdsStack, traverse_flat.h kFlatLdsRows / kSingleLdsRows and
# traverse_flat8.h kQ8LdsRows / kQ8SingleLdsGroups; the GPU test holds this table to the library's own answer (api.traversal_lds_rows)
FAMILIES = (("two_level", None, False, 24, "long"), ("q4", "q4", False, 23, "chain"), ("q8", "q8", False, 10, "fan"),
            ("single_q4", "q4", True, 20, "chain"), ("single_q8", "q8", True, 10, "fan"))


def telescope_mesh(n_shells, ratio, first=1.0, fan=1, gap=0.0, seed=1):
    """shell k lies across the z axis at z = s = first ratio^k, is 0.6 s large and slightly tilted, and is turned about z by a random angle.  fan = 1: one triangle that
    straddles the axis; fan > 1: that many triangles around a centre vertex ON the axis, leaving `gap` of the turn open"""
    rs = np.random.RandomState(seed)
    V = []
    for k in range(n_shells):
        s = first * ratio ** k
        a0 = rs.uniform(0, 2 * np.pi)
        if fan == 1:
            a = a0 + np.arange(3) * (2 * np.pi / 3)
            V.append(np.stack([0.6 * s * np.cos(a), 0.6 * s * np.sin(a), s * (1 + 0.05 * np.arange(3))], 1))
        else:
            for j in range(fan):
                a = a0 + 2 * np.pi * (1 - gap) * np.array([j, j + 1]) / fan
                V.append(np.array([[0, 0, s], [0.6 * s * np.cos(a[0]), 0.6 * s * np.sin(a[0]), s * 1.03], [0.6 * s * np.cos(a[1]), 0.6 * s * np.sin(a[1]), s * 1.06]]))
    V = np.concatenate(V).astype(np.float32)
    return V, np.arange(len(V), dtype=np.uint32).reshape(-1, 3)


def telescope(which="chain", seed=1):
    """a telescope mesh on one node plus a light quad (scaled instances of a mesh this small are refused as singular: the depth has to come from one mesh)"""
    T = TELESCOPES[which]
    V, F = telescope_mesh(T["n_shells"], T["ratio"], T["first"], T["fan"], T["gap"], seed)
    P, I, Nq = scenes._quad([[-5, 30, -5], [5, 30, -5], [5, 30, 5], [-5, 30, 5]], [0, -1, 0])
    meshes = [dict(V=V, F=F, N=None, material=("diffuse", (0.7, 0.7, 0.7))), dict(V=P, F=I, N=Nq, material=("diffuse", (0.5, 0.5, 0.5)))]
    return scenes.build_scene(dict(meshes=meshes, nodes=[(0, None), (1, None)], lights=[(1, (10.0, 10.0, 10.0))], camera=scenes._camera((0, 0.05, -2), (0, 0, 0), 40.0, 32, 32)))


def telescope_rays(which, kind, n, seed=5):
    """outward: from between the inner shells along +z, starting OFF the axis (0.5 .. 1.1 of the start height, so that the shells next to the origin are hit or missed
    as their random turn has it): the deep-stack direction.  A ray that starts ON the axis meets its first shell by plain descent, and nothing it pops afterwards matters:
        axis: that set — on the axis at 0.5 ratio^U(20, n - 20), 0.15 normal jitter in direction;
    inward: from three times the first shell towards the apex (shallow stacks, the control); miss: sideways between two shells and down, away from the light — through
    nodes, into no triangle; between: outward with a tmax that ends between shells (any-hit)"""
    T = TELESCOPES[which]
    ratio, first, ns = T["ratio"], T["first"], T["n_shells"]
    rs = np.random.RandomState(seed)
    if kind in ("outward", "between"):
        z = 0.5 * first * ratio ** rs.uniform(T["exps"][0], T["exps"][1], size=n)
        a = rs.uniform(0, 2 * np.pi, size=n); rho = rs.uniform(0.5, 1.1, size=n) * z
        o = np.stack([rho * np.cos(a), rho * np.sin(a), z], 1)
        d = np.stack([rs.normal(size=n) * 0.02, rs.normal(size=n) * 0.02, np.ones(n)], 1)
        rays = make_rays(o, d, 0.0, FLT_MAX)
        if kind == "between":
            rays[:, 7] = z * rs.uniform(0.1, 3.0, size=n)        # off the axis by rho, the first shell that can be hit has 0.6 s > rho and the first that must be 0.3 s > rho
        return rays
    if kind == "axis":
        z = 0.5 * first * ratio ** rs.uniform(min(20, ns // 2), ns - min(20, ns // 4), size=n)
        o = np.stack([np.zeros(n), np.zeros(n), z], 1)
        d = np.stack([rs.normal(size=n) * 0.15, rs.normal(size=n) * 0.15, np.ones(n)], 1)
        return make_rays(o, d, 0.0, FLT_MAX)
    if kind == "inward":
        o = np.tile([0.0, 0.0, 3.0 * first], (n, 1))
        d = np.stack([rs.normal(size=n) * 0.02, rs.normal(size=n) * 0.02, -np.ones(n)], 1)
        return make_rays(o, d, 0.0, FLT_MAX)
    if kind == "miss":
        k = rs.randint(2, ns - 2, size=n)
        z = first * ratio ** (k + 0.5)                           # between shell k + 1 and shell k
        a = rs.uniform(np.pi, 2 * np.pi, size=n)                 # downwards: the light is above
        o = np.stack([np.zeros(n), np.zeros(n), z], 1)
        d = np.stack([np.cos(a), np.sin(a), rs.uniform(-0.01, 0.01, size=n)], 1)
        return make_rays(o, d, 0.0, FLT_MAX)
    raise ValueError(kind)


# ---------------------------------------------------------------------------------------------------------------- alpha thicket
CARD_KINDS = ("luminance", "alpha", "color", "plain")           # local material index of a card triangle -> how it is alpha-tested


def _card_materials(sc):
    lum = api.diffuse((0.2, 0.6, 0.8), two_sided=True)
    api.set_alpha_map(lum, api.checker_texture(1.0, 0.0, uv_scale=(4.0, 3.0)), api.ALPHA_MAP_LUMINANCE, 0.5)
    yy, xx = np.mgrid[0:32, 0:32]
    rgba = np.zeros((32, 32), np.uint32) | 0x00808080
    rgba |= np.where(((xx - 16) ** 2 + (yy - 16) ** 2) < 144, np.uint32(0xff000000), np.uint32(0x20000000))
    aimg = sc.add_image(rgba.astype(np.uint32), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_POINT)
    alp = api.diffuse((0.7, 0.5, 0.2), two_sided=True)
    api.set_alpha_map(alp, api.image_texture(aimg, uv_scale=(2.0, 2.0)), api.ALPHA_MAP_ALPHA, 0.5)
    col = api.diffuse((0.6, 0.2, 0.6), two_sided=True)
    api.set_alpha_map(col, api.checker_texture((0.9, 0.1, 0.1), (0.1, 0.1, 0.9), uv_scale=(3.0, 3.0)), api.ALPHA_MAP_COLOR, 0.25, (1.0, 0.0, 0.0))
    return [lum, alp, col, api.diffuse((0.5, 0.7, 0.3), two_sided=True)]


def _card_meshes():
    """three card meshes (positions, triangles, uvs, local material per triangle): a 2 x 2 grid of quads, one quad, two crossed quads"""
    g = np.array([[x, y, 0.0] for y in (-0.5, 0.0, 0.5) for x in (-0.5, 0.0, 0.5)])
    Fg = []
    for j in range(2):
        for i in range(2):
            a = 3 * j + i
            Fg += [[a, a + 1, a + 4], [a, a + 4, a + 3]]
    grid = (g, np.array(Fg), g[:, :2] + 0.5, [0, 3, 1, 0, 2, 1, 3, 2])
    q = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [0.5, 0.5, 0], [-0.5, 0.5, 0.0]])
    quad = (q, np.array([[0, 1, 2], [0, 2, 3]]), q[:, :2] + 0.5, [1, 2])
    c = np.concatenate([q, q[:, [2, 1, 0]]])                    # the same quad in the xy and in the zy plane
    cross = (c, np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]]), np.concatenate([q[:, :2] + 0.5] * 2), [0, 1, 2, 3])
    return [grid, quad, cross]


def alpha_thicket(seed=3, n_cards=300):
    """-> (scene, info).  info: dict(cards = [(node index, mesh number, 4x4)], meshes = the three card meshes, tri_kind = CARD_KINDS index by the triangle index a hit
    reports (triangles are numbered through the meshes in the order they were added; 3 = plain also stands for the floor and the light))"""
    rs = np.random.RandomState(seed)
    sc = api.DynamicScene()
    mats = _card_materials(sc)
    P, I, N = scenes._quad([[-9, 0, -9], [-9, 0, 9], [9, 0, 9], [9, 0, -9]], [0, 1, 0])
    sc.CreateNode(sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.6, 0.6, 0.6))]))
    meshes = _card_meshes()
    ids = [sc.add_mesh(V.astype(np.float32), F.astype(np.uint32), uvs=UV.astype(np.float32), tri_material=np.array(tm, np.uint8), materials=mats) for V, F, UV, tm in meshes]
    cards = []
    tri_kind = np.array([3, 3] + [k for V, F, UV, tm in meshes for k in tm] + [3, 3])          # floor, the card meshes, light
    for i in range(n_cards):
        m = i % 3
        xf = np.eye(4)
        xf[:3, :3] = scenes._rotation(rs) * rs.uniform(1.0, 2.5)
        xf[:3, 3] = rs.uniform([-4, 0.8, -4], [4, 5.5, 4])
        node = sc.CreateNode(ids[m], xf.astype(np.float32))
        cards.append((node, m, xf))
    P, I, N = scenes._quad([[-3, 9, -3], [3, 9, -3], [3, 9, 3], [-3, 9, 3]], [0, -1, 0])
    sc.CreateLight(sc.CreateNode(sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.5, 0.5, 0.5))])), 0, (20.0, 20.0, 20.0))
    sc.setCamera((0, 4, 14), (0, 3, 0), (0, 1, 0), 45.0, 64, 64)
    sc.UpdateScene()
    return sc, dict(cards=cards, meshes=meshes, tri_kind=tri_kind)


def _card_points(info, rs, card, tri, n):
    """n points inside triangle `tri` of card `card`, at least 0.12 (barycentric) away from its edges: never a vertex, never an edge"""
    node, m, xf = info["cards"][card]
    V, F = info["meshes"][m][0], info["meshes"][m][1]
    b = rs.dirichlet([1.0, 1.0, 1.0], size=n) * 0.64 + 0.12
    p = b @ V[F[tri]]
    return p @ xf[:3, :3].T + xf[:3, 3]


def thicket_rays(desc, info, kind, n, seed=7):
    """random: as random_rays; aimed: at interior points of random card triangles, from anywhere in the scene's box; aimed_tmax: the same with tmax drawn around the
    target's distance (any-hit: the target and what stands before it may or may not count); one_card: every ray at the interior of ONE alpha-mapped triangle from a
    distance, so that all lanes of the waves hold an alpha candidate at the same time"""
    rs = np.random.RandomState(seed)
    if kind == "random":
        return random_rays(desc, n, seed)
    lo, hi = np.array(desc.box_min[:]), np.array(desc.box_max[:])
    if kind == "one_card":
        card = next(i for i, (node, m, xf) in enumerate(info["cards"]) if m == 2)     # a crossed card: triangle 0 is luminance-tested
        tgt = _card_points(info, rs, card, 0, n)
        xf = info["cards"][card][2]
        nrm = xf[:3, 2] / np.linalg.norm(xf[:3, 2])
        o = tgt + nrm * 25.0 + rs.normal(size=(n, 3)) * 0.5                            # from outside the thicket: other cards may stand in the way, this one is always met
        return make_rays(o, tgt - o, desc.ray_trace_eps, FLT_MAX)
    tgt = np.zeros((n, 3))
    cards = rs.randint(len(info["cards"]), size=n)
    for i in range(n):
        m = info["cards"][cards[i]][1]
        tgt[i] = _card_points(info, rs, cards[i], rs.randint(len(info["meshes"][m][1])), 1)[0]
    o = rs.uniform(lo, hi, size=(n, 3))
    o[:, 1] = np.maximum(o[:, 1], 0.3)                                                  # above the floor
    rays = make_rays(o, tgt - o, desc.ray_trace_eps, FLT_MAX)
    if kind == "aimed_tmax":
        rays[:, 7] = np.linalg.norm(tgt - o, axis=1) * rs.uniform(0.3, 1.3, size=n)
    elif kind != "aimed":
        raise ValueError(kind)
    return rays


def maps_grid_rays():
    """the grid of tests/test_oracle_maps.py test_trace_ray_alpha_test_lets_rays_through_the_holes: straight at the card of scenes.maps_scene"""
    xs, ys = np.meshgrid(np.linspace(-2.9, 2.9, 24), np.linspace(0.3, 4.1, 16))
    rays = np.zeros((xs.size, 8), np.float32)
    rays[:, 0] = xs.ravel(); rays[:, 1] = ys.ravel(); rays[:, 2] = 5.0; rays[:, 3] = 1e-3
    rays[:, 6] = -1.0; rays[:, 7] = 1e30
    return rays


# ---------------------------------------------------------------------------------------------------------------- the comparison rule
def assert_same_hits(got, want, any_hit, what=""):
    """check_flat of tests/test_gpu_intersect.py on two result arrays: any-hit — occlusion equal; closest hit — triangle or node may differ only on rays whose distances are
    equal (two triangles at the same t) and on at most n / 1000 rays, and (t, u, v) are equal to the bit wherever the triangle agrees.  No tolerance."""
    assert len(got) == len(want), what
    assert (got["tri_idx"] != -2).all() and (got["node_idx"] != -2).all(), (what, "a slot no kernel wrote")
    if any_hit:
        bad = np.nonzero((got["tri_idx"] >= 0) != (want["tri_idx"] >= 0))[0]
        assert len(bad) == 0, (what, "occlusion", bad[:10])
        return
    for k in ("tri_idx", "node_idx"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert all(got["dist"][i] == want["dist"][i] for i in bad), (what, k, bad[:10])
        assert len(bad) <= len(want) // 1000, (what, k, len(bad))
    same = got["tri_idx"] == want["tri_idx"]
    for k in ("dist", "u", "v"):
        bad = np.nonzero(got[k][same].view(np.uint32) != want[k][same].view(np.uint32))[0]
        assert len(bad) == 0, (what, k, np.nonzero(same)[0][bad[:10]])


def assert_identical(got, want, what=""):
    """ray for ray, bit for bit"""
    assert len(got) == len(want), what
    for k in ("tri_idx", "node_idx"):
        assert np.array_equal(got[k], want[k]), (what, k, np.nonzero(got[k] != want[k])[0][:10])
    for k in ("dist", "u", "v"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k)
