"""The inputs of tests/test_gpu_traversal_variants.py are what they claim to be — checked on the CPU, with the oracle alone: the scenes are valid, the oracle's own walks
(two-level, flat Q4, flat Q8) agree on every ray set under the rule the GPU is held to, the alpha test really decides a large share of the thicket's rays, and on the
telescopes the reported hits really come out of stack entries beyond the rows the kernels keep in LDS."""
import numpy as np
import pytest
from cudatracerlib_amd import api, scenes
import traversal_cases as tc


@pytest.fixture(scope="module")
def thicket():
    sc, info = tc.alpha_thicket()
    return sc, info, {lay: api.FlatBvh(sc.desc, api.FLAT_FORMATS[lay]) for lay in ("q4", "q8")}


@pytest.fixture(scope="module")
def telescopes():
    out = {}
    for which in tc.TELESCOPES:
        sc = tc.telescope(which)
        out[which] = (sc, {lay: api.FlatBvh(sc.desc, api.FLAT_FORMATS[lay]) for lay in ("q4", "q8")})
    return out


def test_scenes_are_valid_and_within_the_stack_limits(thicket, telescopes):
    """api.scene_desc_check accepts them; the flattened trees fit the traversal stacks (tracer.hip: 3 * depth + 1 + 2 <= 96 entries for Q4, depth + 2 <= 64 groups for Q8);
    the meshes stay small: every telescope below a few hundred triangles, the thicket far below synthetic_sm(64, 64, 300, 2)"""
    st = api.scene_desc_check(thicket[0].desc)
    assert st["alpha_maps"] == 1
    assert thicket[2]["q4"].desc.n_leaves < 2000
    for which, (sc, fbs) in telescopes.items():
        assert api.scene_desc_check(sc.desc)["alpha_maps"] == 0
        T = tc.TELESCOPES[which]
        n_tris = T["n_shells"] * T["fan"]
        assert n_tris <= 300
        assert 0.97 * n_tris <= fbs["q4"].desc.n_leaves - 2 <= n_tris + 16, which   # the tree holds the mesh (but for the innermost triangles of the chain, which the builder drops as degenerate; a few as two references) and the light quad
        assert 3 * fbs["q4"].desc.max_depth + 1 + 2 <= 96 and fbs["q8"].desc.max_depth + 2 <= 64, which
        print(which, "triangles", n_tris, "Q4 depth", fbs["q4"].desc.max_depth, "nodes", fbs["q4"].desc.n_nodes, "Q8 depth", fbs["q8"].desc.max_depth, "nodes", fbs["q8"].desc.n_nodes)


@pytest.mark.parametrize("alpha_test", [False, True])
def test_oracle_walks_agree_on_the_thicket(orc, thicket, alpha_test):
    """0 rays differ between the oracle's own walks — the GPU comparison adds no tolerance to that"""
    sc, info, fbs = thicket
    for kind, n, any_hit in (("random", 20000, False), ("aimed", 20000, False), ("one_card", 256, False), ("random", 20000, True), ("aimed_tmax", 20000, True), ("one_card", 256, True)):
        rays = tc.thicket_rays(sc.desc, info, kind, n)
        if any_hit and kind == "random":
            rays = tc.random_rays(sc.desc, n, 7, any_tmax=True)
        two = orc.intersect(sc.desc, rays, any_hit=any_hit, alpha_test=alpha_test)
        for lay, fb in fbs.items():
            tc.assert_same_hits(orc.intersect(sc.desc, rays, any_hit=any_hit, alpha_test=alpha_test, flat=fb.desc), two, any_hit, (kind, lay))


def test_oracle_walks_agree_on_the_telescopes(orc, telescopes):
    for which, (sc, fbs) in telescopes.items():
        for kind in ("outward", "axis", "inward", "miss", "between"):
            rays = tc.telescope_rays(which, kind, 4000)
            any_hit = kind == "between"
            two = orc.intersect(sc.desc, rays, any_hit=any_hit)
            hit = (two["tri_idx"] >= 0).mean()
            if kind in ("outward", "axis", "inward"):
                assert hit > 0.99, (which, kind, hit)
            elif kind == "miss":
                assert hit < 0.15, (which, kind, hit)
            else:
                assert 0.2 < hit < 0.8, (which, kind, hit)                          # tmax ends before the first shell for some rays and behind it for others
            for lay, fb in fbs.items():
                tc.assert_same_hits(orc.intersect(sc.desc, rays, any_hit=any_hit, flat=fb.desc), two, any_hit, (which, kind, lay))
        assert len(np.unique(orc.intersect(sc.desc, tc.telescope_rays(which, "outward", 4000))["tri_idx"])) >= 20     # many different triangles win


def thicket_shares(orc, sc, info, rays):
    plain, alpha = orc.intersect(sc.desc, rays), orc.intersect(sc.desc, rays, alpha_test=True)
    changed = (plain["tri_idx"] != alpha["tri_idx"]) | (plain["node_idx"] != alpha["node_idx"])
    hit = alpha["tri_idx"] >= 0
    tested = np.zeros(len(rays), bool)
    tested[hit] = info["tri_kind"][alpha["tri_idx"][hit]] != 3          # the reported hit is on an alpha-mapped triangle: its test was evaluated and let it stand
    return dict(changed=changed.mean(), survives=tested.mean(), rejected=changed.mean(), behind_rejected=(changed & hit).mean())


def test_the_alpha_test_decides_on_the_thicket(orc, thicket):
    """the input conditions of the alpha-testing kernels' test (A), from the oracle alone, on the rays aimed at card interiors: the alpha test changes the reported hit on
    at least 20 % of the rays; both outcomes — a candidate on an alpha-mapped triangle survives and is reported / the nearest candidate is rejected — occur on at least
    10 % each; at least 5 % of the rays report a hit that lies behind a rejected candidate of the same ray"""
    sc, info, fbs = thicket
    s = thicket_shares(orc, sc, info, tc.thicket_rays(sc.desc, info, "aimed", 20000))
    print("thicket, aimed rays:", s)
    assert s["changed"] >= 0.20 and s["survives"] >= 0.10 and s["rejected"] >= 0.10 and s["behind_rejected"] >= 0.05, s
    one = thicket_shares(orc, sc, info, tc.thicket_rays(sc.desc, info, "one_card", 256))
    print("thicket, one card:", one)
    assert one["changed"] >= 0.2 and one["survives"] >= 0.2, one         # the card's checker passes some and stops some
    # the triangle numbering the shares rest on: every plain hit on a card node names a triangle of that card's mesh
    plain = orc.intersect(sc.desc, tc.thicket_rays(sc.desc, info, "aimed", 2000))
    first = np.cumsum([2] + [len(m[1]) for m in info["meshes"]])
    mesh_of_node = {node: m for node, m, xf in info["cards"]}
    for h in plain[plain["tri_idx"] >= 0]:
        if h["node_idx"] in mesh_of_node:
            m = mesh_of_node[h["node_idx"]]
            assert first[m] <= h["tri_idx"] < first[m + 1]
    # flat leaves mix alpha-mapped and plain entries: the entries of one leaf (a run that ends with the `last` bit) name triangles of both sorts
    L = fbs["q4"].leaves()
    kinds = info["tri_kind"][(L[:, 12] & 0x0fffffff) >> 1] != 3
    ends = np.nonzero(L[:, 12] & 1)[0]
    mixed = sum(1 for a, b in zip(np.concatenate([[0], ends[:-1] + 1]), ends + 1) if kinds[a:b].any() and not kinds[a:b].all())
    assert mixed >= 20, mixed


@pytest.mark.parametrize("family", tc.FAMILIES, ids=[f[0] for f in tc.FAMILIES])
def test_hits_come_out_of_entries_beyond_the_lds_rows(orc, telescopes, family):
    """the input condition of the deep-stack test (D): for each kernel family, on its telescope, at least 25 % of the outward rays report a hit whose subtree was popped
    from a stack index at or beyond the family's LDS rows (the oracle's stack figures, under the family's stack discipline); the inward rays are the control: same scene,
    no entry beyond index 5"""
    name, lay, single, rows, which = family
    sc, fbs = telescopes[which]
    flat = fbs[lay].desc if lay else None
    hits, su = orc.intersect(sc.desc, tc.telescope_rays(which, "outward", 4000), flat=flat, stack_use=True)
    share, used = (su[:, 1] >= rows).mean(), (su[:, 0] >= rows).mean()
    print("%s on %s: hit popped from an entry >= %d on %.1f %% of the outward rays, %.1f %% use such an entry, deepest %d" % (name, which, rows, 100 * share, 100 * used, su[:, 0].max()))
    assert share >= 0.25
    assert (su[:, 1][hits["tri_idx"] < 0] == -1).all()
    _, su_in = orc.intersect(sc.desc, tc.telescope_rays(which, "inward", 4000), flat=flat, stack_use=True)
    assert su_in[:, 0].max() <= 5
    _, su_axis = orc.intersect(sc.desc, tc.telescope_rays(which, "axis", 4000), flat=flat, stack_use=True)
    print("   rays that start on the axis: %.1f %% use such an entry, %.1f %% have their hit popped from one" % (100 * (su_axis[:, 0] >= rows).mean(), 100 * (su_axis[:, 1] >= rows).mean()))


def test_stack_figures_of_a_small_case(orc):
    """the oracle's stack figures on a case small enough to check by hand: a single-leaf scene never pushes; a miss reports -1; and the figures do not depend on asking for them"""
    sc = scenes.cornell_box(32, 32)
    rays = tc.random_rays(sc.desc, 500, 3)
    for lay in tc.LAYOUTS:
        fb = api.FlatBvh(sc.desc, api.FLAT_FORMATS[lay]) if lay else None          # (the description points into the object: keep it alive)
        flat = fb.desc if fb else None
        a = orc.intersect(sc.desc, rays, flat=flat)
        b, su = orc.intersect(sc.desc, rays, flat=flat, stack_use=True)
        tc.assert_identical(a, b, lay)
        assert su.shape == (500, 2) and (su[:, 0] >= 0).all() and (su[:, 1] >= -1).all() and (su[:, 1] <= su[:, 0]).all(), lay
        assert (su[:, 1][b["tri_idx"] < 0] == -1).all(), lay
        assert su[:, 0].max() <= (3 * 8 if lay != "q8" else 8), lay          # a Cornell box is a few levels deep
