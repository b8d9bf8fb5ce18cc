"""The device BSDF, emitter, texture and surface-map functions (csrc/shading.h, bsdf_more.h, bsdf_rough.h, bsdf_complex.h, mipmap.h) held to the oracle CALL BY CALL.

ctl_shading_eval runs one lane per query: the record filled as the oracle's probe fills it, the __device__ function the shade kernels call, the result row stored.  The
oracle's batched probes read the same query rows (tests/shading_cases.py), in the shared-math build (the `orc` fixture of a gpu test): same fp32 expressions,
-ffp-contract=off, one ctl_fmath.h, correctly rounded / and sqrt on both sides.  So every row is compared as uint32 words — a NaN equals any NaN, -0 does not equal +0 —
and there is no tolerance anywhere: the filtered texture lookup, the one place where last-bit differences were expected, measured bit-equal as well (RESULTS.md,
"Shading functions call by call").

The three builds of the entry point mirror what the product compiles: basic (shade_basic.hip), full (shade_full / shade_class_*), partials (megakernel / prim_tracer)."""
import ctypes as C
import sys

import numpy as np
import pytest

import shading_cases as K
from cudatracerlib_amd import api

pytestmark = pytest.mark.gpu
f32 = np.float32
BASIC, FULL, PARTIALS = api.EVAL_BUILD_BASIC, api.EVAL_BUILD_FULL, api.EVAL_BUILD_PARTIALS


def check(got, want, q, what):
    assert K.same(got, want).all(), "%s: %s" % (what, K.report(got, want, q))


def basic_carries(m):
    """the models shade_basic.hip compiles: diffuse, dielectric, conductor, rough conductor with GGX or full-distribution Beckmann sampling; no image textures"""
    if any(m.tex[k].type == 4 for k in range(4)): return False
    return m.bsdf_type in (1, 3, 6) or (m.bsdf_type == 7 and not (m.u[0] == 2 or (m.u[0] == 0 and m.u[1])))


@pytest.fixture(scope="module")
def grid(gpu, orc_sm):
    """the material array of the edge grid and the roughness variants, a scene that carries synthetic rough-transmittance tables, the oracle over the same two"""
    mats, index, names, rough = K.grid_materials()
    tables = K.synthetic_tables()
    sc = K.probe_scene(tables)
    scene = gpu.Scene(sc.desc)
    ob = K.OracleBsdf(orc_sm.lib, mats, tables)
    return dict(mats=mats, index=index, names=names, rough=rough, scene=scene, sc=sc, ob=ob)


def dev(g, build, what, q):
    return api.shading_eval(g["scene"], build, what, q, materials=g["mats"])


# ------------------------------------------------------------------------------------------------ BSDFs
@pytest.mark.parametrize("rough", [False, True])
def test_the_references_own_bsdf_queries(gpu, orc, rough):
    """2a: the sample and eval rows of bsdf.npz (31 parameter sets) / bsdf_rough.npz (6 sets, over the fixture's transmittance tables), the fixture's raw material array as
    the override, eval under the masks 0x1ff, 0x6, 0x18, 0x60: full == oracle, partials == full, basic == full where basic carries the model"""
    sets, tables = K.fixture_bsdf_sets(rough)
    sc = K.probe_scene(tables); scene = gpu.Scene(sc.desc)
    n_basic = 0
    for name, mats, mi, sq, eq, g in sets:
        with K.OracleBsdf(orc.lib, mats, tables) as ob:
            want = ob.sample(sq)
            got = api.shading_eval(scene, FULL, api.EVAL_BSDF_SAMPLE, sq, materials=mats)
            check(got, want, sq, name + " sample")
            check(api.shading_eval(scene, PARTIALS, api.EVAL_BSDF_SAMPLE, sq, materials=mats), got, sq, name + " sample, partials against full")
            basic = all(basic_carries(mats[k]) for k in range(len(mats)))
            if basic:
                n_basic += 1
                check(api.shading_eval(scene, BASIC, api.EVAL_BSDF_SAMPLE, sq, materials=mats), got, sq, name + " sample, basic against full")
            for mask, q in eq.items():
                want = ob.eval(q, 1)
                got = api.shading_eval(scene, FULL, api.EVAL_BSDF_EVAL, q, materials=mats)
                check(got, want, q, "%s eval mask %x" % (name, mask))
                check(api.shading_eval(scene, PARTIALS, api.EVAL_BSDF_EVAL, q, materials=mats), got, q, "%s eval mask %x, partials against full" % (name, mask))
                if basic:
                    check(api.shading_eval(scene, BASIC, api.EVAL_BSDF_EVAL, q, materials=mats), got, q, "%s eval mask %x, basic against full" % (name, mask))
    assert rough or n_basic >= 3


def test_the_edge_grid(grid, orc):
    """2b: 4212 sample queries per material — cos(theta_i) down to 1e-6, 0 and below, the 0.99999 threshold of sample_visible, sample coordinates at 0, 1e-7, 0.5 +- one
    step and 1 - one step — for the 20 models of test_oracle_bsdf.MODELS, a coating, a rough coating and a blend with a delta child: full == oracle NaN for NaN (the grid's
    rows are live and do contain NaN rows: tests/test_oracle_shading_cases.py), partials == full, basic == full where basic carries the model"""
    n_basic = 0
    with grid["ob"] as ob:
        for name in grid["names"]:
            mi = grid["index"][name]; q = K.edge_grid(mi)
            want = ob.sample(q); got = dev(grid, FULL, api.EVAL_BSDF_SAMPLE, q)
            check(got, want, q, name)
            check(dev(grid, PARTIALS, api.EVAL_BSDF_SAMPLE, q), got, q, name + ", partials against full")
            if basic_carries(grid["mats"][mi]):
                n_basic += 1
                check(dev(grid, BASIC, api.EVAL_BSDF_SAMPLE, q), got, q, name + ", basic against full")
    assert n_basic >= 3


def test_threshold_samples(grid, orc):
    """2c: smp.x at the branch point of the lobe choice and one float step on either side — F of the dielectric, R of the thin dielectric, the specular probability of the
    plastic, Phong's sampling weight, k / 10 for the rough dielectric's sample_z"""
    with grid["ob"] as ob:
        q = K.threshold_rows(ob, grid["index"])
        assert len(q) > 1000
        want = ob.sample(q)
        types = set(want[:, 7].astype(int).tolist())
        assert {0x20, 0x40} <= types and (0x2 in types) and (0x8 in types) and (0x10 in types), types    # the rows do fall on both sides of the branches
        got = dev(grid, FULL, api.EVAL_BSDF_SAMPLE, q)
        check(got, want, q, "thresholds")
        check(dev(grid, PARTIALS, api.EVAL_BSDF_SAMPLE, q), got, q, "thresholds, partials against full")
        d = [k for k in range(len(q)) if int(q[k, 0:1].view(np.uint32)[0]) == grid["index"]["dielectric"]]
        check(dev(grid, BASIC, api.EVAL_BSDF_SAMPLE, q[d]), want[d], q[d], "thresholds of the dielectric, basic")


def test_eval_directions(grid, orc):
    """2d: f and pdf for the exact mirror direction, wo = -wi, wo on and one step off the horizon, wo beyond the critical angle from inside, a 16 x 8 hemisphere grid on both
    sides — every grid model and every roughness variant of 2e, under EAll and under EAll & ~EDelta"""
    n_live = 0
    with grid["ob"] as ob:
        for name in grid["names"] + [n for n in grid["index"] if n.startswith(("rc_", "rd_"))]:
            mi = grid["index"][name]
            for mask in (K.EALL, K.EALL & ~K.DELTA):
                q = K.eval_direction_rows(mi, mask)
                want = ob.eval(q, 1); got = dev(grid, FULL, api.EVAL_BSDF_EVAL, q)
                check(got, want, q, "%s mask %x" % (name, mask))
                check(dev(grid, PARTIALS, api.EVAL_BSDF_EVAL, q), got, q, "%s mask %x, partials against full" % (name, mask))
                n_live += int((want[:, 3] > 0).sum())
                if basic_carries(grid["mats"][mi]):
                    check(dev(grid, BASIC, api.EVAL_BSDF_EVAL, q), got, q, "%s mask %x, basic against full" % (name, mask))
    assert n_live > 50000


def test_roughness_variants(grid, orc):
    """2e: the edge grid for rough conductor and rough dielectric with alpha 1e-4, 1e-3, 0.5, 1, one anisotropic pair each way round, Beckmann / GGX / Phong, with and
    without visible-normal sampling"""
    with grid["ob"] as ob:
        for name in [n for n in grid["index"] if n.startswith(("rc_", "rd_"))]:
            mi = grid["index"][name]; q = K.edge_grid(mi)
            want = ob.sample(q); got = dev(grid, FULL, api.EVAL_BSDF_SAMPLE, q)
            check(got, want, q, name)
            check(dev(grid, PARTIALS, api.EVAL_BSDF_SAMPLE, q), got, q, name + ", partials against full")
            if basic_carries(grid["mats"][mi]):
                check(dev(grid, BASIC, api.EVAL_BSDF_SAMPLE, q), got, q, name + ", basic against full")


def test_sample_then_eval_on_one_record(grid, orc):
    """shade_kernel.inc samples the BSDF and then evaluates f / pdf for the light direction ON THE SAME RECORD (sampled_type, eta and the memo of the rough transmittance are
    left over from the sample); the reference's EstimateDirect starts a fresh record.  That departure must be invisible: for every (wi, smp) of the edge grid and four wo2 —
    the mirror of wi, one above, one below, -wi: the memo is hit with the same key and, through a nested BSDF, with another one — the kernel's row equals the oracle's
    sample followed by a FRESH-record eval(wi, wo2, EAll & ~EDelta), bit for bit, in full and in partials"""
    with grid["ob"] as ob:
        for name in grid["names"]:
            mi = grid["index"][name]; q = K.sample_eval_grid(mi)
            want = ob.sample_then_eval(q); got = dev(grid, FULL, api.EVAL_BSDF_SAMPLE_EVAL, q)
            check(got, want, q, name)
            check(dev(grid, PARTIALS, api.EVAL_BSDF_SAMPLE_EVAL, q), got, q, name + ", partials against full")
            if basic_carries(grid["mats"][mi]):
                check(dev(grid, BASIC, api.EVAL_BSDF_SAMPLE_EVAL, q), got, q, name + ", basic against full")


# ------------------------------------------------------------------------------------------------ emitters
def _light_checks(gpu, lib, d, scene, builds, name, rows_of):
    n = 0
    for li in range(d.n_lights_buf):
        q = rows_of(li)
        if q is None: continue
        want = K.oracle_rows(lib.orc_light_sample_direct_n, d, q, 15)
        got = api.shading_eval(scene, FULL, api.EVAL_LIGHT_SAMPLE, q)
        check(got, want, q, "%s light %d sampleDirect" % (name, li))
        pq = K.light_pdf_rows(q, want); eq = K.light_eval_rows(q, want)
        gp = api.shading_eval(scene, FULL, api.EVAL_LIGHT_PDF, pq); check(gp, K.oracle_rows(lib.orc_light_pdf_direct_n, d, pq, 1), pq, "%s light %d pdfDirect" % (name, li))
        ge = api.shading_eval(scene, FULL, api.EVAL_LIGHT_EVAL, eq); check(ge, K.oracle_rows(lib.orc_light_eval_n, d, eq, 3), eq, "%s light %d eval" % (name, li))
        for b in builds:
            check(api.shading_eval(scene, b, api.EVAL_LIGHT_SAMPLE, q), got, q, "%s light %d sampleDirect, build %d against full" % (name, li, b))
            check(api.shading_eval(scene, b, api.EVAL_LIGHT_PDF, pq), gp, pq, "%s light %d pdfDirect, build %d against full" % (name, li, b))
            check(api.shading_eval(scene, b, api.EVAL_LIGHT_EVAL, eq), ge, eq, "%s light %d eval, build %d against full" % (name, li, b))
        n += len(q)
    return n


def test_emitters(gpu, orc):
    """2f: env_scene(extra_lights=True) — environment map, spot, distant and point light — and area_lights_scene of all four kinds, plus the Cornell panel (the one scene
    the basic build can answer): reference points on the emitter's plane, one step behind it, at the spot cone's two cut-off cosines +- one step, exactly below the
    orthogonal panel's edge, at distances 1e-4 and 1e4; sampleDirect (with the measure), pdfDirect, eval, evalEnvironment, and the emitter pick on the CDF's steps"""
    lib = orc.lib; measures = set()
    for name, sc in K.emitter_scenes().items():
        d = sc.desc; scene = gpu.Scene(d)
        builds = [PARTIALS] + ([BASIC] if name == "cornell" else [])
        assert _light_checks(gpu, lib, d, scene, builds, name, lambda li: K.light_sample_rows(d, li)) > 500
        for li in range(d.n_lights_buf):
            q = K.light_sample_rows(d, li); w = K.oracle_rows(lib.orc_light_sample_direct_n, d, q, 15)
            measures |= {(d.lights[li].type, bool(d.lights[li].orthogonal), int(m)) for m in w[w[:, 3] != 0][:, 14]}
        pk = K.emitter_pick_rows(d)
        want = K.oracle_rows(lib.orc_sample_emitter_direct_n, d, pk, 19); got = api.shading_eval(scene, FULL, api.EVAL_EMITTER_SAMPLE, pk)
        check(got, want, pk, name + " sampleEmitterDirect")
        for b in builds:
            check(api.shading_eval(scene, b, api.EVAL_EMITTER_SAMPLE, pk), got, pk, "%s sampleEmitterDirect, build %d against full" % (name, b))
        assert len(set(want[:, 17].astype(int).tolist())) == d.num_lights, name     # every listed emitter is picked
        if d.env_map_index != 0xffffffff:
            eq = K.env_eval_rows()
            ge = api.shading_eval(scene, FULL, api.EVAL_ENV_EVAL, eq); check(ge, K.oracle_rows(lib.orc_env_eval_n, d, eq, 3), eq, name + " evalEnvironment")
            check(api.shading_eval(scene, PARTIALS, api.EVAL_ENV_EVAL, eq), ge, eq, name + " evalEnvironment, partials against full")
    # live samples of every emitter kind, each with the measure the reference gives it: the orthogonal panel DISCRETE (4), the plain one and the environment map SOLID ANGLE (1)
    assert {(2, True, 4), (2, False, 1), (5, False, 1), (1, False, 4), (4, False, 4), (3, False, 4)} <= measures, measures


def test_the_references_own_emitter_queries(gpu, orc):
    """2a: the rows of lights.npz (14 point / spot / distant lights), emitters.npz (six light lists, samples on the CDF's steps) and scene_lights.npz (area and environment
    emitters of nine scenes: sampleDirect, pdfDirect, eval)"""
    lib = orc.lib
    for k, (sc, q, _, _) in enumerate(K.fixture_light_sets()):
        d = sc.desc; scene = gpu.Scene(d)
        check(api.shading_eval(scene, FULL, api.EVAL_LIGHT_SAMPLE, q), K.oracle_rows(lib.orc_light_sample_direct_n, d, q, 15), q, "lights.npz %d" % k)
    for name, sc, q, _, smp, *_ in K.fixture_emitter_sets():
        d = sc.desc; scene = gpu.Scene(d)
        q2 = np.zeros((len(smp), 8), f32); q2[:, 4] = 1; q2[:, 6:8] = smp
        for rows in (q, q2):
            check(api.shading_eval(scene, FULL, api.EVAL_EMITTER_SAMPLE, rows), K.oracle_rows(lib.orc_sample_emitter_direct_n, d, rows, 19), rows, "emitters.npz " + name)
    sys.path.insert(0, K.GOLDEN)
    from generate import scene_light_cases
    g = K.load("scene_lights.npz")
    for name, sc in scene_light_cases().items():
        d = sc.desc; scene = gpu.Scene(d)
        _light_checks(gpu, lib, d, scene, [], "scene_lights.npz " + name, lambda li: K.light_rows(li, g["%s_light%d_q" % (name, li)]) if "%s_light%d_q" % (name, li) in g.files else None)
        for key in [k for k in g.files if k.startswith(name + "_") and k.endswith("_uv") and k[len(name) + 1:].split("_")[0].rstrip("0123456789") in ("mat", "light")]:
            tn = key[len(name) + 1:-3]; uv = g[key]
            if tn.startswith("mat"):
                idx = int(tn[3:].split("_")[0]); slot = 4 if tn.endswith("_map") else (5 if tn.endswith("_alpha") else int(tn[-1]))
            else:
                idx = int(tn[5:].split("_")[0]); slot = 6
            q = np.zeros((len(uv), 4), f32); q[:, 0] = K.word(slot); q[:, 1] = K.word(idx); q[:, 2:4] = uv
            check(api.shading_eval(scene, FULL, api.EVAL_TEXTURE, q), K.oracle_rows(lib.orc_texture_eval_n, d, q, 3, d.materials), q, "scene_lights.npz %s %s" % (name, tn))


# ------------------------------------------------------------------------------------------------ textures and surface maps
@pytest.fixture(scope="module")
def textures(gpu):
    sc = K.texture_scene()
    return sc, gpu.Scene(sc.desc)


def test_unfiltered_texture_lookups(textures, orc):
    """2g: Texture::Evaluate without partials — uv at 0, -0, 1, texel centres and borders +- one step, negative and beyond 1, every wrap mode with the point and the bilinear
    filter, a 5 x 3, a 20 x 12 and a 1 x 1 image, RGBCOL and RGBE texels, a scaled / mirrored / offset mapping, a checkerboard and a constant: full == oracle,
    partials == full (its dg says `no partials`), basic == full for the checkerboard and the constant"""
    sc, scene = textures; d = sc.desc
    q = K.texture_rows(d)
    assert len(q) > 10000
    want = K.oracle_rows(orc.lib.orc_texture_eval_n, d, q, 3, d.materials)
    got = api.shading_eval(scene, FULL, api.EVAL_TEXTURE, q)
    check(got, want, q, "tex_eval")
    check(api.shading_eval(scene, PARTIALS, api.EVAL_TEXTURE, q), got, q, "tex_eval, partials against full")
    plain = np.array([d.materials[int(i)].tex[0].type != 4 for i in q[:, 1].view(np.uint32)])
    assert plain.sum() > 500
    check(api.shading_eval(scene, BASIC, api.EVAL_TEXTURE, q[plain]), got[plain], q[plain], "tex_eval, basic against full")


def test_surface_maps(gpu, orc):
    """2a: Material::SampleNormalMap for the rows of material_maps.npz — every material of the four map scenes (normal map, height map through evalGradient, none) — and
    the edge uv of 2g on the normal-mapped and the height-mapped ground: full == oracle, partials == full"""
    sys.path.insert(0, K.GOLDEN)
    from generate import material_map_cases, material_map_queries
    g = K.load("material_maps.npz"); scs, hand = material_map_cases(); n = 0
    base = material_map_queries(np.random.RandomState(11), 8).astype(f32)
    for name, sc in scs.items():
        d = sc.desc; scene = gpu.Scene(d)
        for mi in range(d.n_materials):
            key = "%s_mat%d" % (name, mi)
            if key + "_frame_q" not in g.files: continue
            q20 = g[key + "_frame_q"]
            uv = K.uv_edges(64, 64)[::7]; edge = np.repeat(base, (len(uv) + 7) // 8, 0)[:len(uv)].copy(); edge[:, :2] = uv
            q = K.normal_map_rows(mi, np.concatenate([q20, edge]))
            want = K.oracle_rows(orc.lib.orc_sample_normal_map_n, d, q, 10, d.materials)[:, 1:]
            got = api.shading_eval(scene, FULL, api.EVAL_NORMAL_MAP, q)
            check(got, want, q, key)
            check(api.shading_eval(scene, PARTIALS, api.EVAL_NORMAL_MAP, q), got, q, key + ", partials against full")
            n += 1
    assert n >= 3


def test_filtered_texture_lookups(textures, gpu, orc):
    """KernelMIPMap::eval (mip_eval, partials build) against orc_mip_eval: point, bilinear, trilinear and anisotropic images (16 x 16 RGBE under every wrap mode, 20 x 12, 1 x 1),
    footprints that select level 0, the last level, the trilinear fall-back of a degenerate ellipse, the clamped anisotropy and the EWA sum, a zero footprint, and 48
    footprints over four decades.  Measured on an MI355X (RESULTS.md, "Shading functions call by call"): the level, the weights and the texels agree in EVERY row — the
    level goes through ctl_fmath.h's log / log2 on both sides, which tests/test_fmath.py holds bit-identical between host and device — so equality is asserted everywhere
    and no bound is needed."""
    sc, scene = textures; d = sc.desc
    q = K.mip_rows(sc)
    assert len(q) > 6000
    want = K.oracle_rows(orc.lib.orc_mip_eval_n, d, q, 3)
    got = api.shading_eval(scene, PARTIALS, api.EVAL_MIP, q)
    for name, im, w, h in sc._images:   # the footprints do change what is returned: at an interior uv, at least as many answers as the smallest pyramid here has levels (20 x 12: 4)
        sel = (q[:, 0].view(np.uint32) == im) & (q[:, 1] == f32(0.3))
        assert not sel.any() or w == 1 or len(np.unique(want[sel].view(np.uint32), axis=0)) >= 4, name
    check(got, want, q, "mip_eval")


def test_the_references_own_mipmap_queries(gpu, orc):
    """2a: mipmap.npz — the reference's four images (32 x 16 and 20 x 12 RGBCOL, 64 x 64 and 8 x 128 RGBE) under every wrap mode and every filter mode, loaded into one
    scene: KernelMIPMap::eval over the fixture's `args3` rows (uv inside and outside [0, 1], derivatives over four decades incl. degenerate ones) in the partials build,
    and Texture::Evaluate over its Sample(uv) rows (`args4`) for the point and the bilinear filter in all three builds — each against the oracle over the same
    description (the glibc oracle equals the fixture's recorded rows: tests/test_oracle_shading_cases.py)"""
    g = K.load("mipmap.npz")
    sc, images, mat_of = K.mipmap_fixture_scene(g); d = sc.desc; scene = gpu.Scene(d)
    a3, a4 = g["args3"], g["args4"]
    q = np.concatenate([np.concatenate([np.tile(K.word(im), (len(a3), 1)), a3[:, :6]], 1) for im in images.values()]).astype(f32)
    assert len(q) == 64 * 96
    check(api.shading_eval(scene, PARTIALS, api.EVAL_MIP, q), K.oracle_rows(orc.lib.orc_mip_eval_n, d, q, 3), q, "mipmap.npz eval")
    rows = []
    for key, mi in mat_of.items():
        t = np.zeros((len(a4), 4), f32); t[:, 0] = K.word(0); t[:, 1] = K.word(mi); t[:, 2:4] = a4[:, :2]; rows.append(t)
    q = np.concatenate(rows)
    assert len(q) == 32 * 96
    want = K.oracle_rows(orc.lib.orc_texture_eval_n, d, q, 3, d.materials); got = api.shading_eval(scene, FULL, api.EVAL_TEXTURE, q)
    check(got, want, q, "mipmap.npz Sample(uv)")
    assert (want != 0).any(1).mean() > 0.5
    check(api.shading_eval(scene, PARTIALS, api.EVAL_TEXTURE, q), got, q, "mipmap.npz Sample(uv), partials against full")


def test_the_alpha_test(textures, gpu, orc):
    """Material::AlphaTest as the traversal asks it (alpha_survives) against orc_alpha_test: the uv of material_maps.npz's rows and the edge uv of 2g, each rounded to
    half precision — the device function takes its uv from a triangle's half-precision vertex coordinates, so the entry point gives it one synthetic triangle per query whose
    vertices carry the uv, and refuses a uv it cannot represent.  Every material with an alpha state among the map scenes (luminance-tested checker, the alpha channel of a
    bitmap through mip_sample_alpha, a colour key) and the hand-made ones of the fixture (all reflectance-map modes, alpha mode on a non-image texture): the decisions agree
    one for one in all three builds, and both outcomes occur"""
    sys.path.insert(0, K.GOLDEN)
    from generate import material_map_cases
    g = K.load("material_maps.npz"); scs, hand = material_map_cases(); n = 0; outcomes = set()
    edge = K.uv_edges(16, 16)

    def run(scene, desc, mat, mi, key, materials=None):
        nonlocal n
        q = K.alpha_rows(mi, np.concatenate([g[key + "_alpha_q"][:, 2:4], edge]))
        want = K.oracle_alpha(orc.lib, desc, mat, q)
        for b in (FULL, PARTIALS, BASIC):
            check(api.shading_eval(scene, b, api.EVAL_ALPHA_TEST, q, materials=materials), want, q, "%s, build %d" % (key, b))
        outcomes.update((key, int(v)) for v in want[:, 0]); n += 1
    for name, sc in scs.items():
        d = sc.desc; scene = gpu.Scene(d)
        for mi in range(d.n_materials):
            if "%s_mat%d_alpha_q" % (name, mi) in g.files:
                run(scene, d, d.materials[mi], mi, "%s_mat%d" % (name, mi))
    for name, m in hand.items():
        if "hand_%s_alpha_q" % name in g.files:
            one = (api.ctl_material * 1)(m)
            run(textures[1], None, one[0], 0, "hand_" + name, materials=one)
    assert n >= 11
    assert sum(1 for k in {k for k, _ in outcomes} if (k, 0) in outcomes and (k, 1) in outcomes) >= 6, sorted(outcomes)   # the three map scenes and the three hand-made checkers: the textures that vary with uv
    with pytest.raises(api.CtlError) as e:      # a uv that no half-precision vertex can carry
        api.shading_eval(textures[1], FULL, api.EVAL_ALPHA_TEST, np.array([[K.word(0), 0.1, 0.5]], f32))
    assert e.value.code == api.ERR_INVALID


# ------------------------------------------------------------------------------------------------ refusals
def _frame(gpu, orc, scene):
    tables = orc.sequence_tables(1)
    tr = gpu.WavefrontPathTracer(); tr.getParameters().setValue("MaxPathLength", 4)
    tr.Resize(32, 32); tr.InitializeScene(scene)
    img = gpu.Image(32, 32); tr.setSamplerTables(*tables[0]); tr.DoPass(img, new_trace=True)
    return img.getPixelData()


def test_refusals_launch_nothing(grid, textures, gpu, orc):
    """every input the entry point must refuse returns its error before anything is launched, and the scene renders the same frame afterwards"""
    sc = K.emitter_scenes()["panel_image"]; d = sc.desc; scene = gpu.Scene(d)
    before = _frame(gpu, orc, scene)
    mats, index = grid["mats"], grid["index"]
    sq = lambda mi: K.sample_rows(mi, K.direction(0.5, 0.3), (0.3, 0.6))

    def refused(code, sc_, build, what, q, materials=None):
        with pytest.raises(api.CtlError) as e:
            api.shading_eval(sc_, build, what, q, materials=materials)
        assert e.value.code == code, (e.value.code, str(e.value))
    refused(api.ERR_INVALID, scene, FULL, api.EVAL_BSDF_SAMPLE, sq(len(mats)), mats)                      # material index out of range (override)
    refused(api.ERR_INVALID, scene, FULL, api.EVAL_BSDF_SAMPLE, sq(d.n_materials))                         # ... and of the scene's own array
    bad = (api.ctl_material * len(mats))(*[mats[k] for k in range(len(mats))])
    bad[index["coating_diffuse"]].u[2] = len(mats) + 5
    refused(api.ERR_INVALID, scene, FULL, api.EVAL_BSDF_SAMPLE, sq(index["coating_diffuse"]), bad)         # nested index of a coating
    bad[index["blend_glass_diffuse"]].u[3] = 0xfffffff0
    refused(api.ERR_INVALID, scene, FULL, api.EVAL_BSDF_EVAL, K.eval_rows(index["blend_glass_diffuse"], (0, 0, 1), (0, 0, 1), K.EALL), bad)   # ... of a blend
    bad[index["diffuse"]].tex[0] = api.image_texture(d.n_images + 3)
    refused(api.ERR_INVALID, scene, FULL, api.EVAL_BSDF_SAMPLE, sq(index["diffuse"]), bad)                 # image index >= the scene's image count
    refused(api.ERR_INVALID, scene, PARTIALS, api.EVAL_MIP, np.array([[K.word(d.n_images), 0, 0, 0.1, 0, 0, 0.1]], f32))
    lq = K.light_sample_rows(d, 0)[:4].copy(); lq[:, 0] = K.word(d.n_lights_buf)
    refused(api.ERR_INVALID, scene, FULL, api.EVAL_LIGHT_SAMPLE, lq)                                       # light index >= n_lights_buf
    refused(api.ERR_INVALID, scene, FULL, 12, sq(0)); refused(api.ERR_INVALID, scene, FULL, -1, sq(0))     # unknown what
    refused(api.ERR_INVALID, scene, 3, api.EVAL_BSDF_SAMPLE, sq(0)); refused(api.ERR_INVALID, scene, -1, api.EVAL_BSDF_SAMPLE, sq(0))   # unknown build
    refused(api.ERR_INVALID, scene, FULL, api.EVAL_BSDF_SAMPLE, sq(index["roughplastic_beckmann"]), mats)  # a rough BSDF, and this scene has no tables
    refused(api.ERR_INVALID, scene, FULL, api.EVAL_BSDF_SAMPLE, sq(index["roughcoating_ggx_metal"]), mats)
    refused(api.ERR_INVALID, scene, FULL, api.EVAL_ENV_EVAL, K.env_eval_rows())                            # no environment emitter
    # what the chosen build does not carry is refused, not answered with zero
    refused(api.ERR_UNSUPPORTED, grid["scene"], BASIC, api.EVAL_BSDF_SAMPLE, sq(index["plastic"]), mats)
    refused(api.ERR_UNSUPPORTED, grid["scene"], BASIC, api.EVAL_BSDF_SAMPLE, sq(index["roughconductor_beck_vis_aniso"]), mats)
    refused(api.ERR_UNSUPPORTED, grid["scene"], BASIC, api.EVAL_BSDF_SAMPLE, sq(index["coating_diffuse"]), mats)
    tq = K.texture_rows(textures[0].desc)[:4]
    refused(api.ERR_UNSUPPORTED, textures[1], BASIC, api.EVAL_TEXTURE, tq)                                 # an image texture
    refused(api.ERR_UNSUPPORTED, scene, BASIC, api.EVAL_LIGHT_SAMPLE, K.light_sample_rows(d, 0)[:4])       # a textured area light
    refused(api.ERR_UNSUPPORTED, textures[1], FULL, api.EVAL_MIP, K.mip_rows(textures[0])[:4])             # filtered lookups live in the partials build
    refused(api.ERR_UNSUPPORTED, scene, BASIC, api.EVAL_NORMAL_MAP, np.zeros((1, 21), f32))
    # the accepted neighbours of the refused calls do run
    assert api.shading_eval(grid["scene"], FULL, api.EVAL_BSDF_SAMPLE, sq(index["roughplastic_beckmann"]), materials=mats).shape == (1, 9)
    assert api.shading_eval(scene, FULL, api.EVAL_BSDF_SAMPLE, np.zeros((0, 8), f32)).shape == (0, 9)
    after = _frame(gpu, orc, scene)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
