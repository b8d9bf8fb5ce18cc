"""The queries that hold the device BSDF, emitter and texture functions to the oracle call by call (tests/test_gpu_shading_eval.py on the GPU,
tests/test_oracle_shading_cases.py on the CPU).  A query row is a row of ctl_shading_eval (include/ctl_amd.h CTL_EVAL_*): the oracle's batched calls (orc_*_n) read
the same rows, so one array goes to both sides and the result rows compare word for word.

  a. the reference's own queries: the rows of tests/golden/bsdf.npz, bsdf_rough.npz, lights.npz, scene_lights.npz, emitters.npz, mipmap.npz, material_maps.npz
  b. the edge grid: 13 cos(theta_i) x 4 phi x 9 x 9 sample coordinates = 4212 queries per material
  c. threshold samples: smp.x at the branch point the oracle reports and one float step on either side
  d. eval directions: the mirror direction, -wi, the horizon, beyond the critical angle, a 16 x 8 grid on both sides
  e. roughness: alpha 1e-4 .. 1, anisotropic both ways, three distributions with and without visible-normal sampling
  f. emitters: reference points on / behind the emitter, at the spot cone's cut-offs, below the panel's edge, very near and very far
  g. textures: uv at 0, 1, texel centres +- one step, outside [0, 1], every wrap mode, a 1 x 1 and a non-power-of-two image, footprints for every branch of the filter
"""
import ctypes as C
import os
import sys

import numpy as np

from cudatracerlib_amd import api, scenes, rough_tables

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
EALL, DELTA = 0x1FF, 0x1 | 0x20 | 0x40
MASKS = (0x1FF, 0x2 | 0x4, 0x8 | 0x10, 0x20 | 0x40)
MSZ = C.sizeof(api.ctl_material)
f32 = np.float32


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def word(i):
    """an index column: the bits of a uint32 in a float32"""
    return np.asarray(i, np.uint32).view(np.float32)


def up(x):
    return np.nextafter(f32(x), f32(np.inf))


def down(x):
    return np.nextafter(f32(x), f32(-np.inf))


def same(got, want):
    """per row: every word equal (-0 is not +0), a NaN equal to any NaN"""
    got = np.ascontiguousarray(got, np.float32); want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    return ((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).reshape(len(got), int(np.prod(got.shape[1:], dtype=np.int64))).all(1)


def report(got, want, q, k=3):
    bad = np.flatnonzero(~same(got, want))
    return "%d of %d rows differ; first: %s" % (len(bad), len(got), [(int(i), q[i].tolist(), got[i].tolist(), want[i].tolist()) for i in bad[:k]])


# ------------------------------------------------------------------------------------------------ rows
def sample_rows(mat, wi, smp, uv=None):
    wi = np.asarray(wi, f32).reshape(-1, 3); smp = np.asarray(smp, f32).reshape(-1, 2)
    q = np.zeros((len(wi), 8), f32); q[:, 0] = word(mat); q[:, 1:4] = wi; q[:, 4:6] = smp
    if uv is not None: q[:, 6:8] = uv
    return q


def eval_rows(mat, wi, wo, mask, uv=None):
    wi = np.asarray(wi, f32).reshape(-1, 3); wo = np.asarray(wo, f32).reshape(-1, 3)
    q = np.zeros((len(wi), 10), f32); q[:, 0] = word(mat); q[:, 1:4] = wi; q[:, 4:7] = wo; q[:, 7] = word(mask)
    if uv is not None: q[:, 8:10] = uv
    return q


def sample_eval_rows(sample_q, wo2):
    q = np.zeros((len(sample_q), 11), f32); q[:, :8] = sample_q; q[:, 8:11] = wo2
    return q


def direction(cos_t, phi):
    c = np.float64(f32(cos_t)); s = np.sqrt(max(0.0, 1.0 - c * c))
    return np.array([s * np.cos(phi), s * np.sin(phi), c], np.float64).astype(f32)


# ------------------------------------------------------------------------------------------------ b. the edge grid
GRID_COS = (1.0, 0.999995, 0.99999, 0.9, 0.5, 0.1, 1e-3, 1e-6, 0.0, -1e-6, -1e-3, -0.5, -1.0)
GRID_PHI = (0.0, 0.3, np.pi / 2, np.pi)
GRID_SAMPLES = (f32(0), f32(1e-7), f32(0.1), f32(0.25), down(0.5), f32(0.5), up(0.5), f32(0.75), down(1.0))


def grid_wi():
    return np.array([direction(c, p) for c in GRID_COS for p in GRID_PHI], f32)


def grid_samples():
    return np.array([(a, b) for a in GRID_SAMPLES for b in GRID_SAMPLES], f32)


def edge_grid(mat):
    """the 4212 sample queries of one material"""
    wi, s = grid_wi(), grid_samples()
    return sample_rows(mat, np.repeat(wi, len(s), 0), np.tile(s, (len(wi), 1)))


def models():
    sys.path.insert(0, HERE)
    from test_oracle_bsdf import MODELS
    return MODELS


def grid_materials():
    """One material array for b - e: the 20 models of tests/test_oracle_bsdf.py::MODELS, then the nested BSDFs and one coating, one rough coating, one blend with a
    delta child and one blend of two rough plastics, then the roughness variants of e.  Returns (ctypes array, name -> index, names of the b grid)."""
    mats = []; index = {}

    def add(name, m):
        index[name] = len(mats); mats.append(m); return index[name]
    for name, make in models().items():
        add(name, make())
    grid = list(index)
    base = api.diffuse((0.8, 0.7, 0.6)); metal = api.roughconductor(alpha=0.2); glass = api.dielectric(int_ior=1.5, ext_ior=1.0)
    ib, im, ig = add("_child_diffuse", base), add("_child_roughconductor", metal), add("_child_dielectric", glass)
    add("coating_diffuse", api.coating(ib, base, int_ior=1.5, ext_ior=1.0, thickness=1.0, sigma_a=(0.1, 0.2, 0.4)))
    add("roughcoating_ggx_metal", api.roughcoating(im, metal, alpha=0.3, int_ior=1.5, ext_ior=1.0, distribution=1, sigma_a=0.1))
    add("blend_glass_diffuse", api.blend(ig, glass, ib, base, weight=0.5))
    # two rough plastics that differ in alpha ALONE under one blend: both children ask the record's transmittance memo with the same cos(wi), eta and table
    rp_a = api.roughplastic((0.5, 0.5, 0.5), alpha=0.1, distribution=0); rp_b = api.roughplastic((0.3, 0.5, 0.7), alpha=0.4, distribution=0)
    add("blend_roughplastics", api.blend(add("_child_roughplastic_a", rp_a), rp_a, add("_child_roughplastic_b", rp_b), rp_b, weight=0.4))
    grid += ["coating_diffuse", "roughcoating_ggx_metal", "blend_glass_diffuse", "blend_roughplastics"]
    rough = []
    for alpha in (1e-4, 1e-3, 0.5, 1.0):
        for dist in (0, 1, 2):
            for vis in (False, True):
                rough.append(add("rc_a%g_d%d_v%d" % (alpha, dist, vis), api.roughconductor(alpha=alpha, distribution=dist, sample_visible=vis)))
                rough.append(add("rd_a%g_d%d_v%d" % (alpha, dist, vis), api.roughdielectric(alpha=alpha, int_ior=1.5, ext_ior=1.0, distribution=dist, sample_visible=vis)))
    for dist in (0, 1, 2):
        for vis in (False, True):
            for au, av in ((0.4, 0.05), (0.05, 0.4)):
                rough.append(add("rc_aniso%g_d%d_v%d" % (au, dist, vis), api.roughconductor(alpha=au, alpha_v=av, distribution=dist, sample_visible=vis)))
                rough.append(add("rd_aniso%g_d%d_v%d" % (au, dist, vis), api.roughdielectric(alpha=au, alpha_v=av, int_ior=1.5, ext_ior=1.0, distribution=dist, sample_visible=vis)))
    arr = (api.ctl_material * len(mats))(*mats)
    return arr, index, grid, rough


def synthetic_tables():
    """rough-transmittance tables for the grid's rough plastics / coatings (synthetic stand-ins for Mitsuba's microfacet/*.dat, as tests/test_oracle_bsdf.py makes them)"""
    out = []
    for slot in (0, 1, 2):
        tr, df, er, ar = rough_tables.make_table(min(slot, 1), n_eta=4, n_alpha=5, n_theta=8, quad=16)
        out.append((np.ascontiguousarray(tr, f32), np.ascontiguousarray(df, f32), tuple(float(x) for x in er), tuple(float(x) for x in ar)))
    return out


def fixture_tables(g):
    return [(np.ascontiguousarray(g["table%d_trans" % s], f32), np.ascontiguousarray(g["table%d_diff" % s], f32), tuple(float(x) for x in g["table%d_ranges" % s][:2]),
             tuple(float(x) for x in g["table%d_ranges" % s][2:])) for s in range(3)]


def table_structs(tables):
    """(ctl_rough_transmittance * 3) over the arrays of `tables` — what orc_set_probe_rough_transmittance takes; keep `tables` alive"""
    T = (api.ctl_rough_transmittance * 3)()
    for s, (tr, df, er, ar) in enumerate(tables):
        T[s].trans, T[s].diff_trans = tr.ctypes.data, df.ctypes.data
        T[s].eta_samples, T[s].alpha_samples, T[s].theta_samples = tr.shape[0] // 2, tr.shape[1], tr.shape[2]
        T[s].eta_min, T[s].eta_max, T[s].alpha_min, T[s].alpha_max = er[0], er[1], ar[0], ar[1]
    return T


def probe_scene(tables=None):
    """the smallest scene a BSDF query needs: one quad, and the rough-transmittance tables when given"""
    sc = api.DynamicScene()
    P, I, N = scenes._quad([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], [0, 1, 0])
    sc.CreateNode(sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.5, 0.5, 0.5))]), None)
    sc.CreatePointLight((0, 2, 0), (1, 1, 1))
    for s, (tr, df, er, ar) in enumerate(tables or ()):
        sc.setRoughTransmittance(s, tr, df, er, ar)
    sc.setCamera((0, 1, -3), (0, 0, 0), (0, 1, 0), 40.0, 8, 8); sc.UpdateScene()
    sc._tables = tables
    return sc


# ------------------------------------------------------------------------------------------------ the oracle's side of a BSDF query set
class OracleBsdf:
    """the batched BSDF probes of one oracle library over one material array (+ tables)"""

    def __init__(self, lib, mats, tables=None):
        self.lib, self.mats, self.tables = lib, mats, tables
        self.T = table_structs(tables) if tables else None

    def __enter__(self):
        self.lib.orc_set_probe_materials(C.addressof(self.mats))
        self.lib.orc_set_probe_rough_transmittance(C.addressof(self.T) if self.T is not None else None)
        return self

    def __exit__(self, *a):
        self.lib.orc_set_probe_materials(None); self.lib.orc_set_probe_rough_transmittance(None)

    def _run(self, fn, q, width, *head):
        q = np.ascontiguousarray(q, f32); out = np.zeros((len(q), width), f32)
        fn(C.addressof(self.mats), *head, len(q), q.ctypes.data, q.shape[1], out.ctypes.data, width)
        return out

    def sample(self, q): return self._run(self.lib.orc_bsdf_sample_uv_n, q, 9)
    def eval(self, q, mode=1): return self._run(self.lib.orc_bsdf_eval_uv_n, q, 4, mode)
    def sample_then_eval(self, q): return self._run(self.lib.orc_bsdf_sample_then_eval_n, q, 13)


def oracle_rows(fn, desc, q, width, *head):
    """a batched scene probe (orc_light_sample_direct_n, ...): fn(desc, *head, n, q, stride, out, stride)"""
    q = np.ascontiguousarray(q, f32); out = np.zeros((len(q), width), f32)
    fn(C.addressof(desc), *head, len(q), q.ctypes.data, q.shape[1], out.ctypes.data, width)
    return out


# ------------------------------------------------------------------------------------------------ a. the reference's own BSDF queries
def fixture_bsdf_sets(rough=False):
    """[(name, material array, index of the material under test, sample rows, {mask: eval rows}, fixture)] of bsdf.npz (31 sets) or bsdf_rough.npz (6 sets)"""
    g = load("bsdf_rough.npz" if rough else "bsdf.npz")
    names = sorted(k[:-len("_materials")] for k in g.files if k.endswith("_materials"))
    out = []
    for name in names:
        raw = bytes(g[name + "_materials"]); n_m = len(raw) // MSZ
        mats = (api.ctl_material * n_m).from_buffer_copy(raw)
        q = g[name + "_sample_q"]; q2 = g[name + "_eval_q"]
        sq = sample_rows(n_m - 1, q[:, :3], q[:, 3:5], q[:, 6:8])
        eq = {m: eval_rows(n_m - 1, q2[:, :3], q2[:, 3:6], m, q2[:, 6:8]) for m in MASKS if "%s_eval_mode1_mask%x" % (name, m) in g.files}
        out.append((name, mats, n_m - 1, sq, eq, g))
    return out, (fixture_tables(g) if rough else None)


# ------------------------------------------------------------------------------------------------ c. threshold samples
def threshold_rows(ob, index):
    """smp.x at the branch point of the lobe choice and one step on either side: the Fresnel term F of the dielectric (`smp.x <= F`), R of the thin dielectric
    (`smp.x <= R`), the specular probability of the plastic (`smp.x < ps`) — each read off the ORACLE's own sample at smp.x = 0, which takes the reflection branch and reports
    the term as its pdf — Phong's specular sampling weight (`smp.x <= w`, the material's f[0]), and k / 10 for the rough dielectric's `sample_z > F` (sample_z = floor(10 smp.x) / 10)"""
    wis = np.array([direction(c, 0.3) for c in (1.0, 0.9, 0.5, 0.1, 1e-3, -0.5, -0.9)], f32)
    rows = []
    for name in ("dielectric", "thindielectric", "plastic", "plastic_nonlinear"):
        m = index[name]
        first = ob.sample(sample_rows(m, wis, np.zeros((len(wis), 2), f32)))
        for wi, r in zip(wis, first):
            if int(r[7]) == 0x20 and np.isfinite(r[3]) and 0 < r[3] < 1:
                for x in (down(r[3]), f32(r[3]), up(r[3])):
                    for y in (f32(0.25), f32(0.75)):
                        rows.append(sample_rows(m, wi, (x, y)))
    m = index["phong"]; w = f32(ob.mats[m].f[0])
    for wi in wis:
        for x in (down(w), w, up(w)):
            rows.append(sample_rows(m, wi, (x, f32(0.3))))
    for name in [n for n in index if n.startswith("roughdielectric") or n.startswith("rd_a0.5")]:
        for wi in wis:
            for k in range(11):
                t = f32(k) / f32(10.0) if k < 10 else down(1.0)
                for x in (down(t) if k else f32(0), t, up(t) if k < 10 else t):
                    rows.append(sample_rows(index[name], wi, (x, f32(0.6))))
    return np.concatenate(rows)


# ------------------------------------------------------------------------------------------------ d. eval directions
def hemisphere_grid():
    """16 x 8 regular directions on either side"""
    d = []
    for side in (1.0, -1.0):
        for i in range(8):
            c = side * (i + 0.5) / 8
            for j in range(16):
                d.append(direction(c, 2 * np.pi * j / 16))
    return np.array(d, f32)


def eval_directions(wi, eta=1.5):
    """wo for one wi: the exact mirror, -wi, the horizon and one step off it, beyond the critical angle of `eta` seen from inside, the hemisphere grid"""
    wi = np.asarray(wi, f32)
    crit = np.sqrt(1 - 1 / eta ** 2)   # cos of the critical angle
    special = [(-wi[0], -wi[1], wi[2]), -wi, (1, 0, 0), direction(1e-6, 0.3), direction(-1e-6, 0.3), (np.sqrt(0.5), np.sqrt(0.5), 0), direction(-0.5 * crit, 0.3), direction(-0.1, 2.0),
               direction(0.5 * crit, 0.3)]
    return np.concatenate([np.array(special, f32), hemisphere_grid()])


def eval_direction_rows(mat, mask=EALL):
    wis = np.array([direction(c, 0.3) for c in (1.0, 0.99999, 0.9, 0.5, 0.1, 1e-6, 0.0, -1e-6, -0.5, -0.74, -0.75, -1.0)], f32)
    rows = []
    for wi in wis:
        wo = eval_directions(wi)
        rows.append(eval_rows(mat, np.repeat(wi[None], len(wo), 0), wo, mask))
    return np.concatenate(rows)


def sample_eval_grid(mat):
    """every (wi, smp) of the edge grid with four wo2: the mirror of wi (the lobe the sample took, for a specular sample), a fixed direction above, one below, and -wi —
    the record's memo of the rough transmittance is keyed by cos(wi), so the evaluation hits it with the same key and, through a nested BSDF, with another one"""
    g = edge_grid(mat)
    wi = g[:, 1:4]
    wo2 = [np.stack([-wi[:, 0], -wi[:, 1], wi[:, 2]], 1), np.tile(direction(0.6, 1.1), (len(g), 1)), np.tile(direction(-0.45, 4.0), (len(g), 1)), -wi]
    return np.concatenate([sample_eval_rows(g, w) for w in wo2])


# ------------------------------------------------------------------------------------------------ f. emitters
def emitter_scenes():
    return {"env_extra": scenes.env_scene(extra_lights=True), "panel_checker": scenes.area_lights_scene(kind="checker"), "panel_orthogonal": scenes.area_lights_scene(kind="orthogonal"),
            "panel_image": scenes.area_lights_scene(kind="image"), "panel_orthogonal_image": scenes.area_lights_scene(kind="orthogonal_image"), "cornell": scenes.cornell_box(64, 64)}


def light_sample_rows(d, li):
    """reference points for light `li` of description d: on the emitter's plane, behind it, at the spot cone's cut-off cosines +- one step, exactly below the panel's edge, at
    distances 1e-4 and 1e4, and inside the scene box; each with the corner / centre samples and a few of the edge grid's"""
    L = d.lights[li]
    smp = np.array([(0, 0), (down(1.0), down(1.0)), (0.5, 0.5), (0, down(1.0)), (1e-7, 0.25), (down(0.5), up(0.5)), (0.75, 0.1)], f32)
    lo, hi = np.array(d.box_min[:], np.float64), np.array(d.box_max[:], np.float64)
    rs = np.random.RandomState(100 + li)
    refs = [lo + (hi - lo) * rs.uniform(0.02, 0.98, 3) for _ in range(12)]
    nrm = [np.array([0, 1.0, 0]), np.array([0, -1.0, 0]), np.array([0.6, 0.8, 0])]
    if L.type == 2:   # area light: its first triangle's plane
        tri = C.cast(d.anim + L.triangles_index, C.POINTER(ShapeTri))[0]
        p = np.array([[tri.p[k][j] for j in range(3)] for k in range(3)], np.float64); n = np.array(tri.n[:], np.float64)
        cen = p.mean(0)
        refs += [cen, p[0], 0.5 * (p[0] + p[1]), cen + n * 1e-4, cen - n * 1e-4, cen - n * 1.0, cen + n * 1e4, cen + n * 2.0, 0.5 * (p[0] + p[1]) + n * 2.0, p[0] + n * 2.0,
                 p[0] + n * 2.0 + (p[0] - cen) * 1e-6, cen + n * 1.0 + (p[1] - p[0]) * 3.0]
        nrm += [n, -n]
    else:
        pos = np.array(L.position[:], np.float64); dirn = np.array([L.to_world[8], L.to_world[9], L.to_world[10]], np.float64)   # the frame's n: the axis of a spot, the direction of a distant light
        refs += [pos, pos + np.array([1e-4, 0, 0]), pos + np.array([0, -1e4, 0]), pos - dirn * 1.1, pos + dirn * 1.1, dirn * 1.1, dirn * 1.1000001, dirn * 1.0999999]
        if L.type == 4:   # spot: points whose direction from the light makes exactly the cut-off / beam cosine with the axis, +- one step
            axis = dirn
            side = np.array([L.to_world[0], L.to_world[1], L.to_world[2]], np.float64)
            for c0 in (L.cos_cutoff_angle, L.cos_beam_width):
                for c in (down(c0), f32(c0), up(c0)):
                    c = float(c); refs.append(pos + 3.0 * (c * axis + np.sqrt(max(0.0, 1 - c * c)) * side))
    rows = []
    for r in refs:
        for n in nrm:
            q = np.zeros((len(smp), 9), f32); q[:, 0] = word(li); q[:, 1:4] = np.asarray(r, f32); q[:, 4:7] = np.asarray(n, f32); q[:, 7:9] = smp
            rows.append(q)
    return np.concatenate(rows)


class ShapeTri(C.Structure):   # ctl_shape_tri (include/ctl_amd.h)
    _fields_ = [("p", (C.c_float * 3) * 3), ("n", C.c_float * 3), ("area", C.c_float), ("i_dat", C.c_uint32), ("t_dat", C.c_uint32), ("pad", C.c_uint32)]


def light_pdf_rows(sample_q, sample_out):
    """pdfDirect for the sampled directions, and for every fourth an unrelated one; (n, 14) rows"""
    n = len(sample_q); q = np.zeros((n, 14), f32)
    q[:, :7] = sample_q[:, :7]; q[:, 7:10] = sample_out[:, 4:7]; q[:, 10] = sample_out[:, 7]; q[:, 11:14] = sample_out[:, 11:14]
    rs = np.random.RandomState(5); alt = rs.normal(size=(n, 3)); alt /= np.linalg.norm(alt, axis=1, keepdims=True)
    bad = ~(np.linalg.norm(q[:, 7:10], axis=1) > 0.5) | (np.arange(n) % 4 == 0)
    q[bad, 7:10] = alt[bad].astype(f32); q[bad, 10] = np.where(q[bad, 10] > 0, q[bad, 10], 1.0)
    return q


def light_eval_rows(sample_q, sample_out):
    """DiffuseLight::eval at the sampled emitter points, seen from the reference point, from behind (every fourth) and along the normal; (n, 10) rows"""
    live = sample_out[:, 3] > 0; n = int(live.sum()); q = np.zeros((n, 10), f32)
    q[:, 0] = sample_q[live, 0]; q[:, 1:4] = sample_out[live, 8:11]; q[:, 4:7] = sample_out[live, 11:14]; q[:, 7:10] = -sample_out[live, 4:7]
    q[::4, 7:10] *= -1; q[1::4, 7:10] = q[1::4, 4:7]
    return q


def emitter_pick_rows(d):
    """sampleEmitterDirect: samples on the emitter CDF's steps +- one float step and the corner samples, from points inside the box"""
    lo, hi = np.array(d.box_min[:], np.float64), np.array(d.box_max[:], np.float64)
    xs = [f32(0), down(1.0), f32(0.5), f32(1e-7)]
    for k in range(d.num_lights):
        c = f32(d.light_cdf[k]); xs += [down(c), c, up(c)]
    xs = [x for x in xs if 0 <= x < 1]
    rs = np.random.RandomState(9); rows = []
    for x in xs:
        for y in (f32(0), f32(0.3), down(1.0)):
            for _ in range(4):
                r = lo + (hi - lo) * rs.uniform(0.05, 0.95, 3); n = rs.normal(size=3); n /= np.linalg.norm(n)
                rows.append(np.concatenate([r, n, [x, y]]).astype(f32))
    return np.array(rows, f32)


def env_eval_rows():
    d = [direction(c, p) for c in (1.0, 0.99999, 0.5, 1e-6, 0.0, -1e-6, -0.5, -1.0) for p in (0.0, 0.3, np.pi / 2, np.pi, -np.pi / 2, 3.0)]
    d += [(0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (-1, 0, 0), (1e-20, 0, -1), (-1e-20, 0, -1), (0, 0.5, 0), (0, 2.0, 0)]
    return np.array(d, f32)


# ------------------------------------------------------------------------------------------------ g. textures
def texture_scene():
    """images for the texture queries: every wrap mode x point / bilinear over a 5 x 3 (non-power-of-two) RGBCOL bitmap, a 1 x 1 image, a 16 x 16 RGBE bitmap with the
    trilinear and the anisotropic (EWA) filter; one diffuse material per image (tex[0]) plus a checker and a constant one"""
    sc = api.DynamicScene()
    rs = np.random.RandomState(77)
    small = api.float3_to_rgbcol(rs.uniform(0, 1, size=(3, 5, 3)).astype(f32)); one = api.float3_to_rgbcol(np.array([[[0.25, 0.5, 0.75]]], f32))
    big = api.float3_to_rgbe((4.0 * rs.uniform(0, 1, size=(16, 16, 3))).astype(f32)); odd = api.float3_to_rgbcol(rs.uniform(0, 1, size=(12, 20, 3)).astype(f32))
    images = []
    for wrap in (api.WRAP_REPEAT, api.WRAP_CLAMP, api.WRAP_MIRROR, api.WRAP_BLACK):
        for filt in (api.FILTER_POINT, api.FILTER_BILINEAR):
            images.append(("small_w%d_f%d" % (wrap, filt), sc.add_image(small, api.TEXEL_RGBCOL, wrap, filt), 5, 3))
    images.append(("one", sc.add_image(one, api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_BILINEAR), 1, 1))
    for wrap in (api.WRAP_REPEAT, api.WRAP_CLAMP, api.WRAP_MIRROR, api.WRAP_BLACK):
        images.append(("big_tri_w%d" % wrap, sc.add_image(big, api.TEXEL_RGBE, wrap, api.FILTER_TRILINEAR), 16, 16))
        images.append(("big_ewa_w%d" % wrap, sc.add_image(big, api.TEXEL_RGBE, wrap, api.FILTER_ANISOTROPIC), 16, 16))
    images.append(("odd_tri", sc.add_image(odd, api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_TRILINEAR), 20, 12))
    images.append(("odd_ewa", sc.add_image(odd, api.TEXEL_RGBCOL, api.WRAP_MIRROR, api.FILTER_ANISOTROPIC), 20, 12))
    images.append(("one_ewa", sc.add_image(one, api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_ANISOTROPIC), 1, 1))
    mats = [api.diffuse(api.image_texture(i, scale=(0.9, 0.8, 0.7), uv_scale=(1.0, 1.0))) for _, i, _, _ in images]
    mats.append(api.diffuse(api.image_texture(images[0][1], scale=(1.0, 1.0, 1.0), uv_scale=(3.0, -2.0), uv_offset=(0.25, 0.5))))
    mats.append(api.diffuse(api.checker_texture((0.9, 0.1, 0.1), (0.1, 0.1, 0.9), uv_scale=(3.0, 2.0), uv_offset=(0.1, 0.0))))
    mats.append(api.diffuse((0.3, 0.6, 0.9)))
    P, I, N = scenes._quad([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], [0, 1, 0])
    for k in range(0, len(mats), 8):   # a mesh carries up to 8 materials here
        sc.CreateNode(sc.add_mesh(P, I, normals=N, uvs=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], f32), materials=mats[k:k + 8]), None)
    sc.CreatePointLight((0, 2, 0), (1, 1, 1))
    sc.setCamera((0, 1, -3), (0, 0, 0), (0, 1, 0), 40.0, 8, 8); sc.UpdateScene()
    sc._images = images
    return sc


def uv_edges(w, h):
    """uv at 0, 1, texel centres and texel borders +- one step, negative and beyond 1"""
    us = [f32(0), f32(-0.0), f32(1), down(1.0), up(1.0), f32(-0.25), f32(-1.0), f32(-1.5), f32(1.75), f32(2.0), f32(3.5), f32(1e-7), f32(-1e-7)]
    for n in (w, h):
        for k in (0, n // 2, n - 1):
            c = f32((k + 0.5) / n); b = f32(k / n)
            us += [down(c), c, up(c), down(b), b, up(b)]
    us = sorted(set(float(x) for x in us))
    return np.array([(a, b) for a in us for b in us[::3]] + [(b, a) for a in us for b in us[1::3]], f32)


def texture_rows(d):
    """unfiltered lookups of tex[0] of every material of the texture scene"""
    rows = []
    for mi in range(d.n_materials):
        t = d.materials[mi].tex[0]
        w, h = (d.images[t.image].width, d.images[t.image].height) if t.type == 4 else (4, 4)
        uv = uv_edges(w, h); q = np.zeros((len(uv), 4), f32); q[:, 0] = word(0); q[:, 1] = word(mi); q[:, 2:4] = uv
        rows.append(q)
    return np.concatenate(rows)


def mip_rows(sc):
    """KernelMIPMap::eval: footprints that select level 0, the last level, the trilinear fallback (a degenerate ellipse), the clamped anisotropy and the EWA branch, and a zero one"""
    foot = [((0, 0), (0, 0)), ((1e-4, 0), (0, 1e-4)), ((0.02, 0), (0, 0.02)), ((0.06, 0.01), (-0.01, 0.07)), ((0.2, 0), (0, 0.2)), ((0.5, 0.1), (0.1, 0.5)), ((0.9, 0), (0, 0.9)),
            ((0.3, 0), (0, 0.005)), ((0.005, 0), (0, 0.3)), ((0.1, 0.1), (0.1, 0.1)), ((0.2, 0), (0, 0)), ((0.07, -0.03), (0.04, 0.09)), ((0.12, 0.0), (0.0, 0.12)),
            ((0.0625, 0), (0, 0.0625)), ((0.125, 0), (0, 0.125)), ((0.25, 0), (0, 0.25))]
    rs = np.random.RandomState(21)   # and 48 footprints spread over four decades, up to the whole image
    for _ in range(48):
        a = (10.0 ** rs.uniform(-4, -0.05, 4)) * rs.choice([-1.0, 1.0], 4)
        foot.append(((a[0], a[1] * rs.choice([0.0, 0.1, 1.0])), (a[2] * rs.choice([0.0, 0.1, 1.0]), a[3])))
    uvs = np.array([(0, 0), (1, 1), (0.5, 0.5), (0.3, 0.7), (-0.25, 1.75), (0.96875, 0.03125), (down(1.0), up(0.0)), (2.4, -1.3)], f32)
    rows = []
    for name, im, w, h in sc._images:
        if "tri" in name or "ewa" in name or name == "one":
            for d0, d1 in foot:
                q = np.zeros((len(uvs), 7), f32); q[:, 0] = word(im); q[:, 1:3] = uvs; q[:, 3:5] = d0; q[:, 5:7] = d1
                rows.append(q)
    return np.concatenate(rows)


# ------------------------------------------------------------------------------------------------ a. the reference's own emitter, texture and surface-map queries
def _light_scene(types, params):
    """the scene tests/test_oracle_golden.py builds for lights.npz / emitters.npz: a quad and the listed point / spot / distant lights"""
    sc = api.DynamicScene()
    P, I, N = scenes._quad([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], [0, 1, 0])
    sc.CreateNode(sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.5, 0.5, 0.5))]), None)
    for t, p in zip(types, params):
        if t == 1: sc.CreatePointLight(p[:3], p[3:6])
        elif t == 4: sc.CreateSpotLight(p[:3], p[3:6], p[6:9], cutoff_angle=float(p[9]), beam_width=float(p[10]))
        else: sc.CreateDistantLight(p[:3], p[3:6], scene_radius=float(p[6]))
    sc.setCamera((0, 1, -3), (0, 0, 0), (0, 1, 0), 40.0, 8, 8); sc.UpdateScene()
    return sc


def light_rows(li, q8):
    """fixture rows (ref, refN, sample) -> CTL_EVAL_LIGHT_SAMPLE rows of light li"""
    q = np.zeros((len(q8), 9), f32); q[:, 0] = word(li); q[:, 1:9] = q8[:, :8]
    return q


def fixture_light_sets():
    """lights.npz: [(scene, light-sample rows, the reference's rows (n, 14), type)] for its 14 point / spot / distant lights"""
    g = load("lights.npz"); out = []
    for i in range(len([k for k in g.files if k.endswith("_type")])):
        typ = int(g["light%d_type" % i])
        sc = _light_scene([typ], [g["light%d_params" % i]])
        out.append((sc, light_rows(0, g["light%d_q" % i]), g["light%d_out" % i], typ))
    return out


def fixture_emitter_sets():
    """emitters.npz: [(name, scene with the reference run's light list and CDF, emitter rows, the reference's sampleEmitterDirect rows (n, 15), its slot / pdf / re-scaled sample)]"""
    g = load("emitters.npz"); out = []
    names = sorted({k.rsplit("_cdf", 1)[0] for k in g.files if k.endswith("_cdf")})
    for name in names:
        G = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "_") and (name != "deleted" or not k.startswith("deleted_first_"))}
        sc = _light_scene(G["types"], G["params"]); d = sc.desc
        idx, cdf = G["indices"], G["cdf"]
        d.num_lights = len(idx)
        for i in range(16):
            d.light_indices[i] = int(idx[i]) if i < len(idx) else 0; d.light_cdf[i] = float(cdf[i]) if i < len(idx) else 0.0
        out.append((name, sc, np.ascontiguousarray(G["q"][:, :8], f32), G["direct"], G["samples"], G["slot"], G["pdf"], G["resampled"]))
    return out


def mipmap_fixture_desc(g, ii, wrap, filt):
    """a description that carries nothing but one image of mipmap.npz (what orc_mip_eval_n reads); returns (desc, keepalive)"""
    tex = np.ascontiguousarray(g["img%d_texels" % ii]); w, h, typ, levels = (int(x) for x in g["img%d_hdr" % ii])
    M = (api.ctl_mipmap * 1)(api.ctl_mipmap(tex.ctypes.data, w, h, typ, wrap, filt))
    d = api.ctl_scene_desc(); d.images = C.cast(M, C.POINTER(api.ctl_mipmap)); d.n_images = 1
    return d, (tex, M)


def mipmap_fixture_rows(g):
    a = g["args3"]; q = np.zeros((len(a), 7), f32); q[:, 0] = word(0); q[:, 1:7] = a[:, :6]
    return q


def normal_map_rows(mi, q20):
    q = np.zeros((len(q20), 21), f32); q[:, 0] = word(mi); q[:, 1:21] = q20
    return q


def mipmap_fixture_scene(g):
    """the four images of mipmap.npz under every wrap mode and filter in ONE scene (what the device reads; the oracle reads the same description): returns
    (scene, {(image, wrap, filter): image index}, {(image, wrap, filter): index of a diffuse material whose tex[0] is that image with the identity mapping}) — the
    materials for the point and the bilinear filter, the lookups Texture::Evaluate makes without partials"""
    sc = api.DynamicScene(); images = {}; mats = []; mat_of = {}
    for ii in range(4):
        tex = np.ascontiguousarray(g["img%d_texels" % ii]); w, h, typ, levels = (int(x) for x in g["img%d_hdr" % ii])
        assert tex.shape == (h, w)
        for wrap in range(4):
            for filt in range(4):
                images[(ii, wrap, filt)] = sc.add_image(tex, typ, wrap, filt)
                if filt in (api.FILTER_POINT, api.FILTER_BILINEAR):
                    mat_of[(ii, wrap, filt)] = len(mats); mats.append(api.diffuse(api.image_texture(images[(ii, wrap, filt)], scale=(1.0, 1.0, 1.0))))
    P, I, N = scenes._quad([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], [0, 1, 0])
    for k in range(0, len(mats), 8):
        sc.CreateNode(sc.add_mesh(P, I, normals=N, uvs=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], f32), materials=mats[k:k + 8]), None)
    sc.CreatePointLight((0, 2, 0), (1, 1, 1))
    sc.setCamera((0, 1, -3), (0, 0, 0), (0, 1, 0), 40.0, 8, 8); sc.UpdateScene()
    return sc, images, mat_of


def half_uv(uv):
    """uv rounded to half precision: the device's alpha test reads its uv from a triangle's half-precision vertex coordinates, so only such a uv can be asked of it"""
    with np.errstate(over="ignore"):
        return np.asarray(uv, f32).astype(np.float16).astype(f32)


def alpha_rows(mi, uv):
    uv = half_uv(uv); q = np.zeros((len(uv), 3), f32); q[:, 0] = word(mi); q[:, 1:3] = uv
    return q


def oracle_alpha(lib, desc, mat, q):
    """orc_alpha_test_n for the rows of alpha_rows -> (n, 1) float32 of 1 / 0"""
    uv = np.ascontiguousarray(q[:, 1:3], f32); out = np.zeros(len(uv), np.int32)
    lib.orc_alpha_test_n(C.addressof(desc) if desc is not None else None, C.byref(mat), len(uv), uv.ctypes.data, out.ctypes.data)
    return out.astype(f32)[:, None]
