"""The oracle's side of the call-by-call shading tests (tests/shading_cases.py; the kernels' side is tests/test_gpu_shading_eval.py):
  * every batched probe of oracle/oracle_capi.cpp (orc_*_n) equals its one-call form bit for bit;
  * the edge grid is not hollow: the oracle alone gives >= 0.35 live rows (pdf > 0 and a non-zero weight) per model, NaN rows exist, and `diffuse` has some;
  * the glibc build, through the batched calls, reproduces the reference's own rows of tests/golden/*.npz."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle
import shading_cases as K
from cudatracerlib_amd import api

f32 = np.float32


def _sample_single(lib, mats, q):
    out = np.zeros((len(q), 9), f32)
    for i, a in enumerate(q):
        lib.orc_bsdf_sample_uv(C.byref(mats, int(a[0:1].view(np.uint32)[0]) * K.MSZ), a[1:4].ctypes.data, float(a[4]), float(a[5]), float(a[6]), float(a[7]), out[i].ctypes.data)
    return out


def _eval_single(lib, mats, q, mode=1):
    out = np.zeros((len(q), 4), f32)
    for i, a in enumerate(q):
        lib.orc_bsdf_eval_uv(C.byref(mats, int(a[0:1].view(np.uint32)[0]) * K.MSZ), a[1:4].ctypes.data, a[4:7].ctypes.data, int(a[7:8].view(np.uint32)[0]), mode, float(a[8]), float(a[9]), out[i].ctypes.data)
    return out


@pytest.fixture(scope="module")
def grid():
    return K.grid_materials()


def test_batched_bsdf_probes_equal_the_single_ones(orc, grid):
    lib = orc.lib
    mats, index, names, rough = grid
    with K.OracleBsdf(lib, mats, K.synthetic_tables()) as ob:
        for name in names + ["rc_a0.001_d0_v1", "rd_aniso0.4_d2_v0"]:
            q = K.edge_grid(index[name])[::13]          # 324 of the 4212: every wi, every sample coordinate
            got = ob.sample(q); want = _sample_single(lib, mats, q)
            assert K.same(got, want).all(), (name, K.report(got, want, q))
            wo2 = np.tile(K.direction(0.6, 1.1), (len(q), 1)); wo2[::2] = np.stack([-q[::2, 1], -q[::2, 2], q[::2, 3]], 1)
            se = ob.sample_then_eval(K.sample_eval_rows(q, wo2))
            assert K.same(se[:, :9], want).all(), name
            e = K.eval_rows(index[name], q[:, 1:4], wo2, K.EALL & ~K.DELTA)
            assert K.same(se[:, 9:], _eval_single(lib, mats, e)).all(), name
            for mode in (1, 2):
                e2 = K.eval_rows(index[name], q[:, 1:4], wo2, K.EALL)
                assert K.same(ob.eval(e2, mode), _eval_single(lib, mats, e2, mode)).all(), (name, mode)


def test_batched_scene_probes_equal_the_single_ones(orc):
    lib = orc.lib
    lib.orc_light_pdf_direct.restype = C.c_float
    for name, sc in K.emitter_scenes().items():
        d = sc.desc
        for li in range(d.n_lights_buf):
            q = K.light_sample_rows(d, li)[::3]
            got = K.oracle_rows(lib.orc_light_sample_direct_n, d, q, 15)
            want = np.zeros((len(q), 14), f32)
            for i, a in enumerate(q):
                lib.orc_light_sample_direct(C.addressof(d), li, a[1:4].ctypes.data, a[4:7].ctypes.data, float(a[7]), float(a[8]), want[i].ctypes.data)
            # a rejected sample leaves d / dist (and, for the distant light, pdf) of the one-call form's record as its constructor found them: value alone there
            live = (got[:, 3] != 0)
            assert K.same(got[live, :14], want[live]).all(), (name, li)
            assert K.same(got[~live, :3], want[~live, :3]).all(), (name, li)
            pq = K.light_pdf_rows(q, got)
            gp = K.oracle_rows(lib.orc_light_pdf_direct_n, d, pq, 1)[:, 0]
            wp = np.array([lib.orc_light_pdf_direct(C.addressof(d), li, a[1:4].ctypes.data, a[4:7].ctypes.data, a[7:10].ctypes.data, float(a[10]), a[11:14].ctypes.data) for a in pq], f32)
            assert K.same(gp[:, None], wp[:, None]).all(), (name, li)
            eq = K.light_eval_rows(q, got)
            ge = K.oracle_rows(lib.orc_light_eval_n, d, eq, 3); we = np.zeros_like(ge)
            for i, a in enumerate(eq):
                lib.orc_light_eval(C.addressof(d), li, a[1:4].ctypes.data, a[4:7].ctypes.data, a[7:10].ctypes.data, we[i].ctypes.data)
            assert K.same(ge, we).all(), (name, li)
        pk = K.emitter_pick_rows(d)
        got = K.oracle_rows(lib.orc_sample_emitter_direct_n, d, pk, 19); want = np.zeros((len(pk), 15), f32)
        for i, a in enumerate(pk):
            lib.orc_sample_emitter_direct(C.addressof(d), a[0:3].ctypes.data, a[3:6].ctypes.data, float(a[6]), float(a[7]), want[i].ctypes.data)
        live = got[:, 14] >= 0
        assert K.same(got[live, :15], want[live]).all() and K.same(got[~live, :3], want[~live, :3]).all() and (got[~live, 14] == want[~live, 14]).all(), name
        slot = np.zeros(len(pk), np.int32); pdf = np.zeros(len(pk), f32); res = np.zeros(len(pk), f32); pe = np.zeros(16, f32)
        smp = np.ascontiguousarray(pk[:, 6:8])
        lib.orc_emitter_select(C.addressof(d), 0, len(pk), smp.ctypes.data, slot.ctypes.data, pdf.ctypes.data, res.ctypes.data, pe.ctypes.data)
        assert K.same(got[:, 15:19], np.stack([pdf, res, slot.astype(f32), pdf], 1)).all(), name
        if d.env_map_index != 0xffffffff:
            eq = K.env_eval_rows(); ge = K.oracle_rows(lib.orc_env_eval_n, d, eq, 3); we = np.zeros_like(ge)
            for i, a in enumerate(eq):
                lib.orc_env_eval(C.addressof(d), a.ctypes.data, we[i].ctypes.data)
            assert K.same(ge, we).all(), name


def test_batched_texture_and_map_probes_equal_the_single_ones(orc):
    lib = orc.lib
    sc = K.texture_scene(); d = sc.desc
    q = K.texture_rows(d)[::5]
    got = K.oracle_rows(lib.orc_texture_eval_n, d, q, 3, d.materials); want = np.zeros_like(got)
    for i, a in enumerate(q):
        lib.orc_texture_eval(C.addressof(d), C.byref(d.materials[int(a[1:2].view(np.uint32)[0])].tex[0]), float(a[2]), float(a[3]), want[i].ctypes.data)
    assert K.same(got, want).all(), K.report(got, want, q)
    q = K.mip_rows(sc)[::7]
    got = K.oracle_rows(lib.orc_mip_eval_n, d, q, 3); want = np.zeros_like(got)
    for i, a in enumerate(q):
        lib.orc_mip_eval(C.byref(d.images[int(a[0:1].view(np.uint32)[0])]), float(a[1]), float(a[2]), a[3:5].ctypes.data, a[5:7].ctypes.data, want[i].ctypes.data)
    assert K.same(got, want).all(), K.report(got, want, q)
    sys.path.insert(0, K.GOLDEN)
    from generate import material_map_cases, material_map_queries
    scs, hand = material_map_cases()
    q20 = material_map_queries(np.random.RandomState(3), 64).astype(f32)
    md = scs["maps_normal_luminance"].desc
    for mi in range(md.n_materials):
        q = K.normal_map_rows(mi, q20)
        got = K.oracle_rows(lib.orc_sample_normal_map_n, md, q, 10, md.materials); want = np.zeros_like(got)
        for i, a in enumerate(q20):
            f = a[2:11].copy(); geo = a[11:20].copy()
            want[i, 0] = lib.orc_sample_normal_map(C.addressof(md), C.byref(md.materials[mi]), float(a[0]), float(a[1]), f.ctypes.data, geo.ctypes.data); want[i, 1:] = f
        assert K.same(got, want).all(), mi
        uv = np.ascontiguousarray(q20[:, :2]); ga = np.zeros(len(uv), np.int32)
        lib.orc_alpha_test_n(C.addressof(md), C.byref(md.materials[mi]), len(uv), uv.ctypes.data, ga.ctypes.data)
        assert ga.tolist() == [lib.orc_alpha_test(C.addressof(md), C.byref(md.materials[mi]), float(a[0]), float(a[1])) for a in uv], mi


@pytest.mark.parametrize("shared_math", [False, True])
def test_the_edge_grid_is_not_hollow(shared_math, grid):
    """Conditions on the ORACLE alone (both builds), so that the GPU comparison over the grid cannot pass by comparing zeros: per model at least 0.35 of the 4212 rows are
    live (the lowest measured: 0.42, the GGX visible-normal conductor); the grid does reach the inputs where the reference's own arithmetic gives NaN — at least one
    model has NaN rows and `diffuse` is one of them (160 rows with glibc's sincos, 192 with the shared one: squareToCosineHemisphere's x^2 + y^2 one step above 1)."""
    lib = oracle.load(shared_math)
    mats, index, names, rough = grid
    nan_rows = {}
    with K.OracleBsdf(lib, mats, K.synthetic_tables()) as ob:
        for name in names:
            q = K.edge_grid(index[name]); assert len(q) == 4212
            r = ob.sample(q)
            live = (r[:, 3] > 0) & (np.abs(r[:, :3]) > 0).any(1)
            assert live.mean() >= 0.35, (name, live.mean())
            nan_rows[name] = int(np.isnan(r).any(1).sum())
    assert nan_rows["diffuse"] > 0 and sum(1 for v in nan_rows.values() if v) >= 10, nan_rows   # measured: 13 of the 24 materials in either build


def test_the_glibc_build_equals_the_fixtures_through_the_batched_bsdf_calls(orc):
    lib = orc.lib
    for rough in (False, True):
        sets, tables = K.fixture_bsdf_sets(rough)
        assert len(sets) == (6 if rough else 31)
        for name, mats, mi, sq, eq, g in sets:
            with K.OracleBsdf(lib, mats, tables) as ob:
                got = ob.sample(sq); want = g[name + "_sample"]
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, K.report(got, want, sq))
                for mask, q in eq.items():
                    for mode in (1, 2):
                        got = ob.eval(q, mode); want = g["%s_eval_mode%d_mask%x" % (name, mode, mask)]
                        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, mode, hex(mask), K.report(got, want, q))


def test_the_glibc_build_equals_the_fixtures_through_the_batched_scene_calls(orc):
    lib = orc.lib
    for sc, q, want, typ in K.fixture_light_sets():
        got = K.oracle_rows(lib.orc_light_sample_direct_n, sc.desc, q, 15)[:, :14]
        ok = got.view(np.uint32) == want.view(np.uint32)
        void = (want[:, :3] == 0).all(1) & (typ == 3)   # a distant light behind the point: the reference's record stays unset past the value
        ok[void, 3:] = True
        assert ok.all(), (typ, K.report(got, want, q))
    for name, sc, q, want, smp, slot, pdf, res in K.fixture_emitter_sets():
        got = K.oracle_rows(lib.orc_sample_emitter_direct_n, sc.desc, q, 19)
        ok = got[:, :15].view(np.uint32) == want.view(np.uint32)
        void = (want[:, :3] == 0).all(1) & (want[:, 14] < 0)
        ok[void, 3:14] = True
        assert ok.all(), (name, K.report(got[:, :15], want, q))
        q2 = np.zeros((len(smp), 8), f32); q2[:, 4] = 1; q2[:, 6:8] = smp
        got = K.oracle_rows(lib.orc_sample_emitter_direct_n, sc.desc, q2, 19)
        assert K.same(got[:, 15:18], np.stack([pdf, res, slot.astype(f32)], 1)).all(), name
    sys.path.insert(0, K.GOLDEN)
    from generate import scene_light_cases, material_map_cases
    g = K.load("scene_lights.npz"); n_lights = 0
    for name, sc in scene_light_cases().items():
        d = sc.desc
        for li in range(d.n_lights_buf):
            key = "%s_light%d" % (name, li)
            if key + "_q" not in g.files:
                continue
            n_lights += 1
            image_radiance = d.lights[li].type == 2 and d.lights[li].rad_texture.type == 4   # (the reference's value is undefined there: tests/test_oracle_golden.py)
            q = K.light_rows(li, g[key + "_q"]); want = g[key + "_sample"].copy()
            got = K.oracle_rows(lib.orc_light_sample_direct_n, d, q, 15)[:, :14]
            dead = want[:, 3] == 0
            got[dead, 4:] = want[dead, 4:]
            if image_radiance: got[:, :3] = want[:, :3]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (key, K.report(got, want, q))
            a = g[key + "_pdf_q"]; pq = np.zeros((len(a), 14), f32); pq[:, 0] = K.word(li); pq[:, 1:14] = a[:, :13]
            gp = K.oracle_rows(lib.orc_light_pdf_direct_n, d, pq, 1)[:, 0]
            assert np.array_equal(gp.view(np.uint32), g[key + "_pdf"].view(np.uint32)), key
            if key + "_eval_q" in g.files and not image_radiance:
                a = g[key + "_eval_q"]; eq = np.zeros((len(a), 10), f32); eq[:, 0] = K.word(li); eq[:, 1:10] = a
                ge = K.oracle_rows(lib.orc_light_eval_n, d, eq, 3)
                assert np.array_equal(ge.view(np.uint32), g[key + "_eval"].view(np.uint32)), key
    assert n_lights >= 13
    g = K.load("mipmap.npz"); q = K.mipmap_fixture_rows(g)
    for ii in range(4):
        for wrap in range(4):
            for filt in (2, 3, 0, 1):
                d, keep = K.mipmap_fixture_desc(g, ii, wrap, filt)
                got = K.oracle_rows(lib.orc_mip_eval_n, d, q, 3); want = g["img%d_wrap%d_what3_filter%d" % (ii, wrap, filt)]
                assert K.same(got, want).all(), (ii, wrap, filt, K.report(got, want, q))
    g = K.load("material_maps.npz"); scs, hand = material_map_cases(); n_frames = n_alpha = 0
    for name, sc in scs.items():
        d = sc.desc
        for mi in range(d.n_materials):
            key = "%s_mat%d" % (name, mi)
            if key + "_frame_q" in g.files:
                q = K.normal_map_rows(mi, g[key + "_frame_q"]); want = g[key + "_frame"]
                got = K.oracle_rows(lib.orc_sample_normal_map_n, d, q, 10, d.materials)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), key
                n_frames += 1
            if key + "_alpha_q" in g.files:
                a = g[key + "_alpha_q"]; uv = np.ascontiguousarray(a[:, 2:4], f32); ga = np.zeros(len(uv), np.int32)
                lib.orc_alpha_test_n(C.addressof(d), C.byref(d.materials[mi]), len(uv), uv.ctypes.data, ga.ctypes.data)
                assert np.array_equal(ga, g[key + "_alpha"]), key
                n_alpha += 1
    for name, m in hand.items():
        key = "hand_" + name; one = (api.ctl_material * 1)(m)
        if key + "_frame_q" in g.files:
            q = K.normal_map_rows(0, g[key + "_frame_q"]); got = np.zeros((len(q), 10), f32)
            lib.orc_sample_normal_map_n(None, C.addressof(one), len(q), q.ctypes.data, q.shape[1], got.ctypes.data, 10)
            assert np.array_equal(got.view(np.uint32), g[key + "_frame"].view(np.uint32)), key
            n_frames += 1
        if key + "_alpha_q" in g.files:
            a = g[key + "_alpha_q"]; uv = np.ascontiguousarray(a[:, 2:4], f32); ga = np.zeros(len(uv), np.int32)
            lib.orc_alpha_test_n(None, C.addressof(one), len(uv), uv.ctypes.data, ga.ctypes.data)
            assert np.array_equal(ga, g[key + "_alpha"]), key
            n_alpha += 1
    assert n_frames >= 8 and n_alpha >= 11


def test_shading_eval_without_a_device():
    """ctl_shading_eval asks for the device before it looks at its arguments, like every entry point that launches: CTL_ERR_NO_DEVICE on a machine without one; a null
    scene is what a machine with a device complains about"""
    q = np.zeros((1, 8), f32); out = np.zeros((1, 9), f32)
    code = api.lib.ctl_shading_eval(None, api.EVAL_BUILD_FULL, api.EVAL_BSDF_SAMPLE, None, 0, 1, q.ctypes.data, 8, out.ctypes.data, 9)
    if api.device_count() == 0:
        assert code == api.ERR_NO_DEVICE and b"no HIP device" in api.lib.ctl_last_error()
    else:
        assert code == api.ERR_INVALID
