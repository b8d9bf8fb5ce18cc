"""Every traversal kernel variant against the oracle, ray by ray (tests/test_gpu_intersect.py holds k_intersect<ANY_HIT, COUNT, LAYOUT, ALPHA = false> on shallow scenes; the
rest of the traversal code is reached here, through ctl_intersect_ex / ctl_intersect_pair):
 A  the alpha-testing kernels (two-level: inline test; Q4: deferred candidates and the alpha phase; Q8: inline test);
 B  the single-ray traversals of the PathTracer / PrimTracer plugins (single_ray.h trace_single, Q4 and Q8);
 C  the fused launch k_intersect_pair against the two separate launches;
 D  stack entries beyond the LDS rows, in all five stacks (the telescopes of tests/traversal_cases.py).
The rule is check_flat's of test_gpu_intersect.py (traversal_cases.assert_same_hits): (t, u, v) equal to the bit, triangle / node may differ only between triangles at the
same distance and on at most n / 1000 rays, occlusion equal; no tolerance.  tests/test_oracle_traversal_cases.py shows on the CPU that the oracle's own walks stay within
it with 0 rays to spare and that the inputs exercise what they are meant to."""
import ctypes as C
import numpy as np
import pytest
from cudatracerlib_amd import api, scenes
import traversal_cases as tc

pytestmark = pytest.mark.gpu

_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def the_scene(name):
    """-> (DynamicScene, info or None), built once per session of this file"""
    def make():
        if name == "thicket":
            return tc.alpha_thicket()
        if name.startswith("maps_"):
            return scenes.maps_scene(32, 24, None, name[5:]), None
        if name.startswith("telescope_"):
            return tc.telescope(name[10:]), None
        return {"cornell": lambda: scenes.cornell_box(64, 64, glass_sphere=True), "synthetic": lambda: scenes.synthetic_sm(64, 64, n_instances=300, subdiv=2),
                "beams": scenes.beams_over_spheres}[name](), None
    return cached(("scene", name), make)


def flat_bvh(name, layout):
    return cached(("fb", name, layout), lambda: api.FlatBvh(the_scene(name)[0].desc, api.FLAT_FORMATS[layout]))


def device_scene(gpu, name, layout):
    return cached(("dev", name, layout), lambda: gpu.Scene(the_scene(name)[0].desc, flatten=layout is not None, flat_format=layout))


def the_rays(name, kind, n):
    def make():
        sc, info = the_scene(name)
        if name == "thicket" and kind != "random_tmax":
            return tc.thicket_rays(sc.desc, info, kind, n)
        if name.startswith("telescope_"):
            return tc.telescope_rays(name[10:], kind, n)
        if kind == "grid+random":
            return np.concatenate([tc.maps_grid_rays(), tc.random_rays(sc.desc, n, 3)])
        if kind == "grid+random_tmax":
            g = tc.maps_grid_rays(); g[:, 7] = 7.0                                  # tmax between card and wall (tests/test_oracle_maps.py)
            return np.concatenate([g, tc.random_rays(sc.desc, n, 3, any_tmax=True)])
        return tc.random_rays(sc.desc, n, 7, any_tmax=kind == "random_tmax")
    return cached(("rays", name, kind, n), make)


def want(orc, name, kind, n, any_hit, alpha, same_arrays=None):
    """the oracle on the description, once per case: the two-level walk, or (same_arrays = a layout) its walk of the very arrays the kernel walks"""
    def make():
        flat = flat_bvh(name, same_arrays).desc if same_arrays else None
        return orc.intersect(the_scene(name)[0].desc, the_rays(name, kind, n), any_hit=any_hit, alpha_test=alpha, flat=flat)
    return cached(("want", name, kind, n, any_hit, alpha, same_arrays), make)


def hold(gpu, orc, name, layout, kind, n, counts, any_hit, alpha_flag, alpha_want, single=False, ends_inside=False):
    """the kernel variant on prefixes of a ray set (every count its own launch) against the oracle's results for the whole set"""
    scene, rays = device_scene(gpu, name, layout), the_rays(name, kind, n)
    w = want(orc, name, kind, n, any_hit, alpha_want, layout if (ends_inside and layout) else None)
    for k in counts:
        got = gpu.intersect_ex(scene, rays[:k], any_hit=any_hit, alpha=alpha_flag, single=single)
        tc.assert_same_hits(got, w[:k], any_hit, (name, layout, kind, k, "any" if any_hit else "closest", "alpha" if alpha_flag else "plain", "single" if single else "wavefront"))
    return w


SMALL = (1, 11, 12, 13, 63, 64, 65)      # on either side of the Q4 alpha phase's batch of 12 and of a wave: the phases run only because nothing else is left


# ---------------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_refuse_on_the_host(gpu):
    """unknown flag bits, null pointers with a non-zero count and CTL_ISECT_SINGLE on a two-level scene are refused before anything is launched; n = 0 is legal; the
    library's LDS row limits are the ones the case table assumes"""
    sc, _ = the_scene("cornell")
    two, flat = device_scene(gpu, "cornell", None), device_scene(gpu, "cornell", "q4")
    rays = tc.random_rays(sc.desc, 8, 1)
    for bad in (8, 16, 0x80000000, 7 | 64):
        with pytest.raises(api.CtlError) as e:
            gpu.intersect_ex(flat, rays, flags=bad)
        assert e.value.code == api.ERR_INVALID
    for bad in (api.ISECT_ANY_HIT, api.ISECT_SINGLE, 8):
        with pytest.raises(api.CtlError) as e:
            gpu.intersect_pair(flat, rays, rays, flags=bad)
        assert e.value.code == api.ERR_INVALID
    for flags in (api.ISECT_SINGLE, api.ISECT_SINGLE | api.ISECT_ANY_HIT | api.ISECT_ALPHA):
        with pytest.raises(api.CtlError) as e:
            gpu.intersect_ex(two, rays, flags=flags)
        assert e.value.code == api.ERR_UNSUPPORTED and "FLATTEN" in str(e.value)      # the PathTracer's own answer to a two-level scene
    r, rp = api._rays_struct(rays)
    hits = np.zeros(8, dtype=api._HIT_DTYPE); occ = np.zeros(8, np.uint32)
    hp, op = hits.ctypes.data_as(C.c_void_p), occ.ctypes.data_as(C.c_void_p)
    assert api.lib.ctl_intersect_ex(flat._h, None, 8, hp, 0) == api.ERR_INVALID and api.lib.ctl_intersect_ex(flat._h, rp, 8, None, 0) == api.ERR_INVALID
    assert api.lib.ctl_intersect_ex(None, rp, 8, hp, 0) == api.ERR_INVALID
    for args in ((None, 8, hp, rp, 8, op), (rp, 8, None, rp, 8, op), (rp, 8, hp, None, 8, op), (rp, 8, hp, rp, 8, None)):
        assert api.lib.ctl_intersect_pair(flat._h, *args, 0) == api.ERR_INVALID
    assert api.lib.ctl_intersect_ex(flat._h, None, 0, None, 0) == 0 and api.lib.ctl_intersect_pair(flat._h, None, 0, None, None, 0, None, 0) == 0
    assert len(gpu.intersect_ex(flat, np.zeros((0, 8), np.float32), single=True)) == 0
    assert gpu.traversal_lds_rows() == {f[0]: f[3] for f in tc.FAMILIES}


@pytest.mark.parametrize("layout", tc.LAYOUTS)
def test_the_plain_entry_point_and_the_new_one_agree(gpu, layout):
    """ctl_intersect_ex without flags launches what ctl_intersect launches; and on a scene WITHOUT alpha maps CTL_ISECT_ALPHA changes nothing, bit for bit"""
    sc, _ = the_scene("cornell")
    scene = device_scene(gpu, "cornell", layout)
    for any_hit in (False, True):
        rays = tc.random_rays(sc.desc, 5000, 5, any_tmax=any_hit)
        plain = gpu.intersect(scene, rays, any_hit=any_hit)
        tc.assert_identical(gpu.intersect_ex(scene, rays, any_hit=any_hit), plain, (layout, any_hit))
        tc.assert_identical(gpu.intersect_ex(scene, rays, any_hit=any_hit, alpha=True), plain, (layout, any_hit, "alpha flag"))


# ---------------------------------------------------------------------------------------------------------------- A: alpha-testing kernels
@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("layout", tc.LAYOUTS, ids=["two_level", "q4", "q8"])
def test_alpha_kernels_on_the_thicket(gpu, orc, layout, any_hit):
    """with the flag: orc.intersect(alpha_test=True); without it: the plain oracle.  Closest hit on the rays aimed at card interiors, occlusion on the same with tmax drawn
    around the target (against the oracle's walk of the same arrays: there only WHETHER something is found is defined); and one launch whose rays all hold an alpha
    candidate of the same card at once"""
    kind = "aimed_tmax" if any_hit else "aimed"
    for flag in (True, False):
        w = hold(gpu, orc, "thicket", layout, kind, 20000, SMALL + (20000,), any_hit, flag, flag, ends_inside=any_hit)
        hold(gpu, orc, "thicket", layout, "one_card", 256, (256,), any_hit, flag, flag)
        hold(gpu, orc, "thicket", layout, "random", 20000, (20000,), any_hit, flag, flag)
    assert 0.3 < (w["tri_idx"] >= 0).mean()


@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("layout", tc.LAYOUTS, ids=["two_level", "q4", "q8"])
@pytest.mark.parametrize("alpha_kind", ["luminance", "alpha", "color"])
def test_alpha_kernels_on_the_three_map_kinds(gpu, orc, alpha_kind, layout, any_hit):
    """scenes.maps_scene with each alpha kind: the grid straight at the card (tests/test_oracle_maps.py; for occlusion with tmax between card and wall) and random rays"""
    name, kind = "maps_" + alpha_kind, "grid+random_tmax" if any_hit else "grid+random"
    n = 384 + 20000
    plain = hold(gpu, orc, name, layout, kind, 20000, (n,), any_hit, False, False, ends_inside=any_hit)
    alpha = hold(gpu, orc, name, layout, kind, 20000, SMALL + (n,), any_hit, True, True, ends_inside=any_hit)
    differ = ((plain["tri_idx"] >= 0) != (alpha["tri_idx"] >= 0)) if any_hit else (plain["tri_idx"] != alpha["tri_idx"])
    assert differ[:384].mean() > 0.1                                                  # the holes are there: the test decides a good part of the grid


# ---------------------------------------------------------------------------------------------------------------- B: single-ray traversals
@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("layout", ["q4", "q8"])
@pytest.mark.parametrize("name,n", [("cornell", 20000), ("synthetic", 30000), ("beams", 30000), ("thicket", 20000)])
def test_single_ray_traversal(gpu, orc, name, n, layout, any_hit):
    """trace_single_flat / trace_single_flat8 as the megakernel calls them, against the oracle's two-level walk (beams: split references, a triangle met twice is accepted
    once; thicket: alpha-tested, as the single-ray traversal always is on a scene with alpha maps — with or without the flag)"""
    alpha = name == "thicket"
    kind = ("aimed_tmax" if any_hit else "aimed") if alpha else ("random_tmax" if any_hit else "random")
    w = hold(gpu, orc, name, layout, kind, n, (1, 255, 256, 257, n), any_hit, False, alpha, single=True, ends_inside=any_hit)
    assert 0.2 < (w["tri_idx"] >= 0).mean()
    if alpha:
        hold(gpu, orc, name, layout, kind, n, (257,), any_hit, True, True, single=True, ends_inside=any_hit)


# ---------------------------------------------------------------------------------------------------------------- C: the fused launch
def check_pair(gpu, scene, rays, shadow, alpha, sep_hits, sep_occ, what):
    hits, occ = gpu.intersect_pair(scene, rays, shadow, alpha=alpha)
    assert (hits["tri_idx"] != -2).all() and (hits["node_idx"] != -2).all() and np.isin(occ, (0, 1)).all(), (what, "a slot no kernel wrote")
    tc.assert_identical(hits, sep_hits, what)
    assert np.array_equal(occ == 1, sep_occ), (what, "occlusion")


@pytest.mark.parametrize("alpha", [False, True], ids=["plain", "alpha"])
@pytest.mark.parametrize("layout", tc.LAYOUTS, ids=["two_level", "q4", "q8"])
def test_fused_launch_equals_the_two_launches(gpu, layout, alpha):
    """k_intersect_pair — closest hits of one queue, then occlusion of a second, in one persistent launch with shared LDS and two cursors — gives, ray for ray and bit for
    bit, what the two separate launches of the same rays give (those are held to the oracle above and in test_gpu_intersect.py); either queue may be empty"""
    sc, info = the_scene("thicket")
    scene = device_scene(gpu, "thicket", layout)
    rays, shadow = the_rays("thicket", "aimed", 20000), the_rays("thicket", "aimed_tmax", 20000)
    sizes = (0, 1, 65, 4097)
    sep_hits = {n: gpu.intersect_ex(scene, rays[:n], alpha=alpha) for n in sizes}
    sep_occ = {n: gpu.intersect_ex(scene, shadow[:n], any_hit=True, alpha=alpha)["tri_idx"] >= 0 for n in sizes}
    assert (sep_hits[4097]["tri_idx"] >= 0).mean() > 0.5 and 0.2 < sep_occ[4097].mean() < 0.9
    for n in sizes:
        for sn in sizes:
            if n or sn:
                check_pair(gpu, scene, rays[:n], shadow[:sn], alpha, sep_hits[n], sep_occ[sn], (layout, alpha, n, sn))


@pytest.mark.parametrize("layout", tc.LAYOUTS, ids=["two_level", "q4", "q8"])
def test_fused_launch_beyond_the_static_shares(gpu, layout):
    """both queues longer than the waves' static first claims (traverse.h ray_claims; test_gpu_intersect.py test_ray_claims_across_the_static_shares): every wave goes
    through both cursors, with a last partial wave on both sides.  The alpha-testing kernels, on the thicket."""
    sc, info = the_scene("thicket")
    scene = device_scene(gpu, "thicket", layout)
    waves = 256 * 6 * 4          # resident traversal waves on an MI355X (kernels.hip traversal_blocks)
    n = waves * 64 + 64 * 37 + 5
    rays, shadow = tc.random_rays(sc.desc, n, 11), tc.random_rays(sc.desc, n, 12, any_tmax=True)
    sep_hits = gpu.intersect_ex(scene, rays, alpha=True)
    sep_occ = gpu.intersect_ex(scene, shadow, any_hit=True, alpha=True)["tri_idx"] >= 0
    assert (sep_hits["tri_idx"] >= 0).mean() > 0.2 and 0.05 < sep_occ.mean() < 0.9
    check_pair(gpu, scene, rays, shadow, True, sep_hits, sep_occ, (layout, n))


# ---------------------------------------------------------------------------------------------------------------- D: deep stacks
@pytest.mark.parametrize("any_hit", [False, True], ids=["closest", "any"])
@pytest.mark.parametrize("family", tc.FAMILIES, ids=[f[0] for f in tc.FAMILIES])
def test_deep_stacks(gpu, orc, family, any_hit):
    """each kernel family on its telescope: the outward rays, whose hits come out of stack entries beyond the family's LDS rows (test_oracle_traversal_cases.py:
    two-level 54 %, Q4 48 %, Q8 43 %, single-ray Q4 58 %, single-ray Q8 43 % of them), in ragged launches; rays from on the axis; and the inward rays and the misses
    as the control: the same scene with shallow stacks"""
    name, layout, single, rows, which = family
    scene = "telescope_" + which
    if any_hit:
        w = hold(gpu, orc, scene, layout, "between", 4000, (1, 63, 65, 4000), True, False, False, single=single, ends_inside=True)
        assert 0.2 < (w["tri_idx"] >= 0).mean() < 0.8
        hold(gpu, orc, scene, layout, "outward", 4000, (4000,), True, False, False, single=single)
    else:
        hold(gpu, orc, scene, layout, "outward", 4000, (1, 63, 65, 4000), False, False, False, single=single)
        for kind in ("axis", "inward", "miss"):
            hold(gpu, orc, scene, layout, kind, 4000, (4000,), False, False, False, single=single)


@pytest.mark.parametrize("family", [f for f in tc.FAMILIES if f[1] and not f[2]], ids=["q4", "q8"])
def test_deep_stacks_show_in_the_histogram(gpu, orc, family):
    """the kernel confirms that the path was taken: after a counting traversal of the outward rays the stack histogram holds exactly these rays, and at least as many
    of them beyond the LDS rows as the oracle's depth-first walk puts there (the kernels postpone leaves: their hit distance shrinks later, they go at least as deep);
    the inward rays stay below entry 8"""
    name, layout, single, rows, which = family
    sc, _ = the_scene("telescope_" + which)
    scene = device_scene(gpu, "telescope_" + which, layout)
    rays = the_rays("telescope_" + which, "outward", 4000)
    _, su = orc.intersect(sc.desc, rays, flat=flat_bvh("telescope_" + which, layout).desc, stack_use=True)
    gpu.traversal_stack_histogram(reset=True)
    gpu.intersect_count(scene, rays)
    h = gpu.traversal_stack_histogram(reset=True)
    print("%s: rays by deepest entry, kernel %s; beyond the %d LDS rows: kernel %d, oracle %d of %d" % (name, np.nonzero(h)[0].tolist(), rows, h[rows:].sum(), (su[:, 0] >= rows).sum(), len(rays)))
    assert h.sum() == len(rays)
    assert h[rows:].sum() >= (su[:, 0] >= rows).sum() >= len(rays) // 4
    gpu.intersect_count(scene, the_rays("telescope_" + which, "inward", 4000))
    h = gpu.traversal_stack_histogram(reset=True)
    assert h.sum() == 4000 and h[8:].sum() == 0


def test_deep_stacks_in_the_fused_launch(gpu):
    """the fused launch with deep stacks in both halves (Q4, the chain): equal to the two launches"""
    scene = device_scene(gpu, "telescope_chain", "q4")
    rays, shadow = the_rays("telescope_chain", "outward", 4000), the_rays("telescope_chain", "between", 4000)
    check_pair(gpu, scene, rays, shadow, False, gpu.intersect_ex(scene, rays), gpu.intersect_ex(scene, shadow, any_hit=True)["tri_idx"] >= 0, "chain")
