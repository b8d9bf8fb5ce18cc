"""Heterogeneous media, the host half (no GPU): ctl_volume_eval(on_device = 0) — csrc/volume_grid.h on the host — against the numpy restatement
tests/volume_grid_ref.py, every function, every row bit for bit; the restatement's condition (the march's step cap is never reached); closed forms in float64; the
idx scramble cell by cell; validator, diff and builder; the resource figures of the two kernels that must keep their code.  Sets and queries: volume_grid_cases.py."""
import ctypes as C

import numpy as np
import pytest

from cudatracerlib_amd import api, scenes
import volume_grid_ref
import volume_grid_cases as cases
from volume_grid_cases import SETS, make_set, queries, same_rows, FUNCTIONS

f32 = np.float32
U = 2.0 ** -24   # fp32 unit roundoff


@pytest.mark.parametrize("what", sorted(FUNCTIONS), ids=[FUNCTIONS[w].replace(" ", "_").replace("/", "") for w in sorted(FUNCTIONS)])
def test_volume_eval_host_equals_the_restatement(orc_sm, what):
    """ctl_volume_eval(on_device = 0) against volume_grid_ref, EVERY row bit for bit, NaN for NaN: 256 seeded queries per function and set plus the branch points
    (volume_grid_cases.queries), the old codes 0-12 through the type dispatch and the three new ones.  The restatement alone must leave the march's step cap un-hit on
    every row (its condition), and so must the library."""
    for name in SETS:
        vols = make_set(name)
        d = api.volumes_desc(vols)
        q = queries(name, vols, what)
        got = api.volume_eval(d, what, q, on_device=False)
        V = volume_grid_ref.volumes_of_desc(orc_sm, d)
        want = volume_grid_ref.eval_rows(V, what, q)
        assert V.stats["cap_hits"] == 0, (name, FUNCTIONS[what], V.stats)
        bad = same_rows(got, want)
        assert not bad, (name, FUNCTIONS[what], len(bad), len(q), q[bad[0]], got[bad[0]], want[bad[0]])
        if what == api.VEVAL_GRID_MARCH:
            assert not got[:, 1].any() and got[:, 0].max() > 3, (name, got[:, 0].max())


def test_the_march_is_exercised(orc_sm):
    """the queries are no row of misses: on every set a good share of the tau rows is non-zero, sampleDistance succeeds in some and fails in some, the march takes
    several steps, and sampleVolume picks the grid (index 1) of grid_two through the mask-as-index"""
    for name in SETS:
        vols = make_set(name); d = api.volumes_desc(vols)
        tau = api.volume_eval(d, api.VEVAL_TAU, queries(name, vols, api.VEVAL_TAU))
        sd = api.volume_eval(d, api.VEVAL_SAMPLE_DISTANCE, queries(name, vols, api.VEVAL_SAMPLE_DISTANCE))
        assert (tau[:, 0] != 0).sum() >= 50 and 10 <= sd[:, 0].sum() <= len(sd) - 10, (name, (tau[:, 0] != 0).sum(), sd[:, 0].sum())
    vols = make_set("grid_two"); d = api.volumes_desc(vols)
    sv = api.volume_eval(d, api.VEVAL_SAMPLE_VOLUME, queries("grid_two", vols, api.VEVAL_SAMPLE_VOLUME))
    assert (sv[:, 0] == 1).sum() >= 20


def _const_rows(L_frac=1.0, sample=0.5):
    """rays inside grid_const's region that keep half a cell from its LOW faces (where sampleTrilinear's unclamped weights no longer sum to 1): start inside, maxT
    inside.  -> (q for REGION_TAU / REGION_SAMPLE_DISTANCE, world lengths)"""
    rs = np.random.RandomState(5)
    lo, hi = cases.BOX_LO.astype(np.float64), cases.BOX_HI.astype(np.float64)
    a = lo + (hi - lo) * rs.uniform(0.07, 0.5, (24, 3)); b = lo + (hi - lo) * rs.uniform(0.5, 0.97, (24, 3))
    L = np.linalg.norm(b - a, axis=1)
    q = np.zeros((24, 10), np.float32)
    q[:, 1:4] = a; q[:, 4:7] = (b - a) / L[:, None]; q[:, 8] = L * L_frac; q[:, 9] = sample
    return q, L * L_frac


def test_constant_grid_against_the_homogeneous_formulas():
    """grid_const (8 x 8 x 8 of c = 0.75, sigAMin = sigSMin = 0, sigAMax = 0.001, sigSMax = 0.004) against float64 closed forms, for rays that start inside the region,
    end inside it and keep half a cell from its low faces:
      tau           = (sigAMax + sigSMax) c L                 (the swapped pairing of integrateDensity is symmetric for one grid);
      sampled t     = -log(1 - s) / D with D = d_s + d_a, d_s = sigSMax c, d_a = sigAMax d_s AS WRITTEN (d_a from the overwritten d_s), t0 = 0;
      pdfSuccess    = (1 - s) D,  pdfFailure = transmittance = 1 - s,  pdfSuccessRev = (1 - s) (sigAMax + sigSMax) c.
    Bounds, derived, not tuned (u = 2^-24; n = the march's step count of the row, from CTL_VEVAL_GRID_MARCH):  a step costs two trilinear samples (8 products of four
    factors and 8 additions each: <= 16 u), their sum, the halving (exact), the segment length (an absolute error of u * maxT per crossing, n crossings: <= n u
    relative to the total) and its product and addition into the sum (2 u + n u for the running sum): <= (16 + 3) u per step plus 2 n u in all; the two transforms,
    the normalisation, Lcl_To_World and the final products add <= 64 u.  tau: (21 n + 64) u relative.  The sampled t adds the division, log and exp (<= 4 u each,
    ctl_fmath.h's functions are good to 2 ulp): (21 n + 80) u relative to max(t, L); the probabilities likewise relative to their own values."""
    vols = make_set("grid_const"); d = api.volumes_desc(vols)
    c, sa, ss = 0.75, float(f32(0.001)), float(f32(0.004))
    q, L = _const_rows()
    n = api.volume_eval(d, api.VEVAL_GRID_MARCH, q)[:, 0].astype(np.float64)
    assert n.min() >= 3
    tau = api.volume_eval(d, api.VEVAL_REGION_TAU, q).astype(np.float64)
    want = (sa + ss) * c * L
    err = np.abs(tau[:, 0] - want) / want
    print("tau rel err / bound", (err / ((21 * n + 64) * U)).max())
    assert (err <= (21 * n + 64) * U).all() and (tau[:, 0] == tau[:, 1]).all() and (tau[:, 1] == tau[:, 2]).all()
    D = ss * c + sa * (ss * c)
    for s in (0.1, 0.5):
        q[:, 9] = s
        s32 = float(f32(s))
        r = api.volume_eval(d, api.VEVAL_REGION_SAMPLE_DISTANCE, q).astype(np.float64)
        t_want = -np.log1p(-s32) / D
        hit = t_want < L * 0.999
        assert hit.sum() >= 8 and (r[hit, 0] == 1).all()
        bound = (21 * n + 80) * U
        e_t = np.abs(r[hit, 1] - t_want) / np.maximum(t_want, L[hit])
        e_ps = np.abs(r[hit, 14] - (1 - s32) * D) / ((1 - s32) * D)
        e_pf = np.abs(r[hit, 16] - (1 - s32)) / (1 - s32)
        e_rev = np.abs(r[hit, 15] - (1 - s32) * (sa + ss) * c) / ((1 - s32) * (sa + ss) * c)
        print("s", s, "t / pdfSuccess / pdfFailure / pdfSuccessRev rel err over bound", (e_t / bound[hit]).max(), (e_ps / bound[hit]).max(), (e_pf / bound[hit]).max(), (e_rev / bound[hit]).max())
        assert (e_t <= bound[hit]).all() and (e_ps <= bound[hit]).all() and (e_pf <= bound[hit]).all() and (e_rev <= bound[hit]).all()
        assert (r[hit, 5] == r[hit, 16]).all()   # transmittance = Spectrum(expVal) = pdfFailure
        far = ~hit   # the density is never reached: failure, transmittance exp(-tau_effective) with the AS-WRITTEN density D
        if far.any():
            assert (r[far, 0] == 0).all()
            assert (np.abs(r[far, 16] - np.exp(-D * L[far])) / np.exp(-D * L[far]) <= bound[far]).all()


def test_linear_ramp_against_the_analytic_integral():
    """a cubic 6 x 6 x 6 grid whose value is a + b x along its first axis (for a cubic grid idx is the plain x-slowest order, so data.reshape(6, 6, 6)[x, y, z] is the
    value value(x, y, z) returns): inside [0.5, 5.5]^3 voxel units the trilinear field is a + b (vx - 0.5) exactly, linear along any ray, so the march's trapezoid rule
    is exact and tau = (sigAMax + sigSMax) L (f(start) + f(end)) / 2.  Rays start and end inside that core.  Bound as in the constant test: (21 n + 64) u relative."""
    dm = 6; a0, b0 = 0.2, 0.1
    data = (a0 + b0 * np.arange(dm, dtype=np.float64))[:, None, None] * np.ones((dm, dm, dm))
    lo, hi = cases.BOX_LO.astype(np.float64), cases.BOX_HI.astype(np.float64)
    sa, ss = float(f32(0.002)), float(f32(0.003))
    vols = [api.grid_volume(api.box_to_volume_matrix(cases.BOX_LO, cases.BOX_HI), density=data.astype(np.float32), sig_a=(0.0, sa), sig_s=(0.0, ss))]
    d = api.volumes_desc(vols)
    rs = np.random.RandomState(9)
    ua = rs.uniform(0.6 / dm, 5.4 / dm, (24, 3)); ub = rs.uniform(0.6 / dm, 5.4 / dm, (24, 3))
    pa = lo + (hi - lo) * ua; pb = lo + (hi - lo) * ub
    L = np.linalg.norm(pb - pa, axis=1)
    q = np.zeros((24, 10), np.float32); q[:, 1:4] = pa; q[:, 4:7] = (pb - pa) / L[:, None]; q[:, 8] = L
    n = api.volume_eval(d, api.VEVAL_GRID_MARCH, q)[:, 0].astype(np.float64)
    tau = api.volume_eval(d, api.VEVAL_REGION_TAU, q).astype(np.float64)[:, 0]
    data32 = data.astype(np.float32).astype(np.float64)
    f = lambda u: np.interp(u[:, 0] * dm - 0.5, np.arange(dm), data32[:, 0, 0])
    want = (sa + ss) * L * (f(ua) + f(ub)) / 2
    err = np.abs(tau - want) / want
    print("ramp tau rel err / bound", (err / ((21 * n + 64) * U)).max())
    assert (err <= (21 * n + 64) * U).all()


def test_idx_scramble_cell_by_cell():
    """DenseVolGrid::idx on 3 x 4 x 5 pinned against the formula idx(i, j, k) = min(k, dx-1) + min(j, dy-1) dx + min(i, dz-1) dx dy: a grid whose floats are their own
    linear index, sampled at the voxel centres (vx + 0.5: the corner's weights are 1 and 0 exactly), returns data[idx(x, y, z)] — NOT the cell (x, y, z) of a plain
    layout, for a non-cubic grid"""
    dx, dy, dz = 3, 4, 5
    data = np.arange(dx * dy * dz, dtype=np.float32).reshape(dx, dy, dz)
    d = api.volumes_desc([api.grid_volume(np.eye(4), density=data, sig_s=(0.0, 1.0))])
    pts = [(x, y, z) for x in range(dx) for y in range(dy) for z in range(dz)]
    q = np.zeros((len(pts), 10), np.float32); q[:, 2:5] = np.array(pts, np.float32) + 0.5
    got = api.volume_eval(d, api.VEVAL_GRID_VALUE, q)[:, 0]
    want = np.array([min(z, dx - 1) + min(y, dy - 1) * dx + min(x, dz - 1) * dx * dy for x, y, z in pts], np.float32)
    assert np.array_equal(got, want)
    plain = np.array([x * dy * dz + y * dz + z for x, y, z in pts], np.float32)
    assert not np.array_equal(got, plain) and want.max() < dx * dy * dz


@pytest.fixture(scope="module")
def box_scene():
    return scenes.cornell_box(24, 16)


def _copy_grid(g):
    c = api.ctl_volume_grid(); C.memmove(C.addressof(c), C.addressof(g), C.sizeof(c)); return c


@pytest.mark.parametrize("rule", ["no_record", "two_records", "record_for_homogeneous", "record_past_table", "zero_dim", "too_many_cells", "null_data", "nan_value", "negative_value",
                                  "negative_coefficient", "max_below_min", "region_coefficients", "null_array"])
def test_validator_refuses(box_scene, rule):
    gv = api.grid_volume(np.eye(4), density=np.full((2, 2, 2), 0.5, np.float32), sig_a=(0.0, 0.1), sig_s=(0.1, 0.2))
    hom = api.homogeneous_volume(np.eye(4), 0.1, 0.2)
    api.scene_desc_check(api.volumes_desc([gv, hom]), api.DIFF_VOLUMES)   # the good description passes
    g = _copy_grid(gv.grid); g.volume = 0
    vols, grids, message = [gv.volume, hom], [g], None
    keep = []
    if rule == "no_record":
        grids = []; message = "needs exactly one grid record, the description has 0"
    elif rule == "two_records":
        grids = [g, _copy_grid(g)]; message = "needs exactly one grid record, the description has 2"
    elif rule == "record_for_homogeneous":
        h = _copy_grid(g); h.volume = 1; grids = [g, h]; message = "names a volume that is no VolumeGrid"
    elif rule == "record_past_table":
        h = _copy_grid(g); h.volume = 7; grids = [g, h]; message = "names volume 7 of 2"
    elif rule == "zero_dim":
        g.dim[1] = 0; message = "zero dimension"
    elif rule == "too_many_cells":
        g.dim[0], g.dim[1], g.dim[2] = 4096, 4096, 4096; message = "more than 4194304 cells"
    elif rule == "null_data":
        g.data = None; message = "has no data"
    elif rule in ("nan_value", "negative_value"):
        a = np.full(8, 0.5, np.float32); a[3] = float("nan") if rule == "nan_value" else -0.25; keep.append(a)
        g.data = a.ctypes.data_as(C.POINTER(api.f32)); message = "values must be finite and non-negative"
    elif rule == "negative_coefficient":
        g.sig_a_min[1] = -0.1; message = "must be finite and non-negative"
    elif rule == "max_below_min":
        g.sig_s_max[2] = 0.05; message = "maximum lies below its minimum"
    elif rule == "region_coefficients":
        v = api.ctl_volume(); C.memmove(C.addressof(v), C.addressof(gv.volume), C.sizeof(v)); v.sig_s[0] = 0.1; vols = [v, hom]; message = "must be 0"
    d = api.ctl_scene_desc(); C.memmove(C.addressof(d), C.addressof(box_scene.desc), C.sizeof(d))
    api.set_desc_volumes(d, vols, grids)
    if rule == "null_array":
        d.volume_grids = None; message = "grid record|without a volume_grids array"
    for parts in (0, api.DIFF_VOLUMES):
        with pytest.raises(api.CtlError, match=message):
            api.scene_desc_check(d, parts)
    with pytest.raises(api.CtlError, match=message):
        api.volume_eval(d, api.VEVAL_TAU, np.zeros((1, 10), np.float32))


def test_grid_codes_need_a_grid_region():
    d = api.volumes_desc([api.homogeneous_volume(np.eye(4), 0.1, 0.2)])
    with pytest.raises(api.CtlError, match="no VolumeGrid"):
        api.volume_eval(d, api.VEVAL_GRID_MARCH, np.zeros((1, 10), np.float32))


def _desc_with(base, volumes):
    d = api.ctl_scene_desc()
    C.memmove(C.addressof(d), C.addressof(base), C.sizeof(d))
    return api.set_desc_volumes(d, volumes)


def test_diff_reports_volumes_alone(box_scene):
    m = api.box_to_volume_matrix((0, 0, 0), (10, 10, 10))
    dens = scenes.smoke_density((3, 4, 5), 1)
    base = _desc_with(box_scene.desc, [api.grid_volume(m, density=dens, sig_s=(0.0, 0.2))])
    same = _desc_with(box_scene.desc, [api.grid_volume(m, density=dens.copy(), sig_s=(0.0, 0.2))])
    assert api.scene_desc_diff(base, same) == 0                                       # other arrays, the same floats
    cell = dens.copy(); cell[1, 2, 3] += 0.125
    assert api.scene_desc_diff(base, _desc_with(box_scene.desc, [api.grid_volume(m, density=cell, sig_s=(0.0, 0.2))])) == api.DIFF_VOLUMES
    assert api.scene_desc_diff(base, _desc_with(box_scene.desc, [api.grid_volume(m, density=dens.reshape(4, 3, 5), sig_s=(0.0, 0.2))])) == api.DIFF_VOLUMES   # dims alone
    assert api.scene_desc_diff(base, _desc_with(box_scene.desc, [api.grid_volume(m, density=dens, sig_s=(0.0, 0.25))])) == api.DIFF_VOLUMES                  # a maximum
    assert api.scene_desc_diff(base, _desc_with(box_scene.desc, [api.grid_volume(m, density=dens, sig_s=(0.01, 0.2))])) == api.DIFF_VOLUMES                  # a minimum
    assert api.scene_desc_diff(box_scene.desc, base) == api.DIFF_VOLUMES              # 0 -> 1 grid regions
    assert api.scene_desc_diff(base, _desc_with(box_scene.desc, [api.homogeneous_volume(m, 0.0, 0.2)])) == api.DIFF_VOLUMES                                  # grid -> homogeneous
    three = api.grid_volume(m, density_a=dens, density_s=dens, sig_s=(0.0, 0.2))
    assert api.scene_desc_diff(base, _desc_with(box_scene.desc, [three])) == api.DIFF_VOLUMES


def test_builder_round_trip():
    """CreateVolume(w, h, d, ...) and the nine-int form through the builder: the description hands out the records with the builder's own copies of the floats, the
    region's derived fields, and the reference's zeroed coefficients until they are set"""
    sc = scenes.cornell_box(24, 16)
    m = api.box_to_volume_matrix((0, 0, 0), (100, 200, 300))
    i = sc.CreateVolume(3, 4, 5, volume_to_world=m, phase=api.phase_hg(0.25))
    j = sc.CreateVolume(2, 3, 2, 4, 2, 3, 9, 9, 9, volume_to_world=m)   # the L dims are accepted and ignored
    assert (i, j) == (0, 1)
    sc.UpdateScene(); d = sc.desc
    assert d.n_volumes == 2 and d.n_volume_grids == 2 and d.volumes[0].type == api.VOLUME_GRID
    g = d.volume_grids[0]
    assert g.volume == 0 and g.single_grid == 1 and list(g.dim) == [3, 4, 5] and not any(g.sig_s_max) and not np.ctypeslib.as_array(g.data, shape=(60,)).any()
    assert np.array_equal(np.array(list(d.volumes[0].world_to_volume.m), np.float32), np.array(list(api.homogeneous_volume(m, 0, 0).world_to_volume.m), np.float32))
    dens = scenes.smoke_density((3, 4, 5), 2); dens_s = scenes.smoke_density((4, 2, 3), 3)
    sc.SetVolumeGridData(0, dens); sc.SetVolumeGridCoefficients(0, sig_a=(0.0, 0.001), sig_s=(0.0, (0.004, 0.002, 0.001)))
    sc.SetVolumeGridData(1, dens_s, which=1); sc.SetVolumeGridCoefficients(1, sig_s=(0.001, 0.002))
    before = sc.desc
    keep = api.ctl_scene_desc(); C.memmove(C.addressof(keep), C.addressof(before), C.sizeof(keep))
    dens[:] = 0   # the builder copied the floats
    sc.UpdateScene(); d = sc.desc
    g0, g1 = d.volume_grids[0], d.volume_grids[1]
    assert np.array_equal(np.ctypeslib.as_array(g0.data, shape=(60,)), scenes.smoke_density((3, 4, 5), 2).reshape(-1))
    assert g1.single_grid == 0 and list(g1.dim_a) == [2, 3, 2] and list(g1.dim_s) == [4, 2, 3] and np.array_equal(np.ctypeslib.as_array(g1.data_s, shape=(24,)), dens_s.reshape(-1))
    assert f32(g0.sig_s_max[1]) == f32(0.002) and f32(g1.sig_s_min[0]) == f32(0.001)
    api.scene_desc_check(d, api.DIFF_VOLUMES)
    with pytest.raises(api.CtlError, match="floats for a grid of 60"):
        sc.SetVolumeGridData(0, np.zeros(59, np.float32))
    with pytest.raises(api.CtlError, match="no VolumeGrid"):
        sc.SetVolumeGridData(5, np.zeros(60, np.float32))
    with pytest.raises(api.CtlError, match="zero dimension or more than"):
        sc.CreateVolumeGrid(0, 4, 5)
    # smoke_box is fog_box with a grid: one region over the scene box, a non-constant density on a non-cubic grid
    sb = scenes.smoke_box(24, 16, dims=(3, 4, 5))
    gs = sb.desc.volume_grids[0]
    cells = np.ctypeslib.as_array(gs.data, shape=(60,))
    assert sb.desc.n_volumes == 1 and list(gs.dim) == [3, 4, 5] and cells.min() > 0 and cells.max() > 2 * cells.min()
    assert np.array_equal(cells, scenes.smoke_box(24, 16, dims=(3, 4, 5)).volume._arrays[0])   # seeded


def test_geometry_cache_hash_does_not_see_grids(box_scene):
    assert api.flatten_probe(box_scene.desc) == api.flatten_probe(scenes.smoke_box(24, 16).desc)


def test_other_kernels_keep_their_resources(tmp_path):
    """k_path_trace and k_path_trace_media must keep the code they had before the grid instantiation existed: their VGPR / AGPR / scratch / occupancy remarks equal the
    figures DESIGN §11 records for the parent commit (209 + 3 / 1536 B / 2 waves and 223 + 3 / 1600 B / 2 waves); the grid kernel is there beside them"""
    from test_kernel_resources import _resources
    res = _resources("megakernel.hip", tmp_path)
    pick = lambda tail: [v for n, v in res.items() if n.startswith("_ZN3ctl") and tail in n]
    plain, media, grid = pick("12k_path_traceE"), pick("18k_path_trace_mediaE"), pick("23k_path_trace_media_gridE")
    assert len(plain) == 1 and len(media) == 1 and len(grid) == 1, sorted(res)
    print("k_path_trace", plain[0]); print("k_path_trace_media", media[0]); print("k_path_trace_media_grid", grid[0])
    fig = lambda k: (k["VGPRs"], k["AGPRs"], k["ScratchSize"], k["Occupancy"], k["VGPRs Spill"])
    assert fig(plain[0]) == (209, 3, 1536, 2, 0)
    assert fig(media[0]) == (223, 3, 1600, 2, 0)
