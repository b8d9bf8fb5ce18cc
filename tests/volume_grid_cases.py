"""Volume sets and query rows of the heterogeneous-media tests (not collected): shared by tests/test_volume_grid_host.py (ctl_volume_eval on the host against the
restatement tests/volume_grid_ref.py) and tests/test_gpu_volume_grid.py (the same queries on the device against the host).

SETS:  grid_one    one single-grid VolumeGrid, dims 3 x 4 x 5, rotated and scaled (HG 0.3, coloured sigSMax)
       grid_three  the three-grid form: gridA 2 x 3 x 2, gridS 4 x 2 x 3 (traversal resolution 4 x 3 x 3) over the Cornell box, non-zero minima
       grid_two    a homogeneous region first and a grid second: sampleVolume's mask-as-index (mask 2 = both hit, slot 0 -> index 1 ... as written) picks the grid
       grid_const  an 8 x 8 x 8 grid of one value
queries(set, volumes, what, n): n seeded rows plus the branch points — volume_cases.queries' rows for the codes 0-12 (its ray, sample and phase branch points), then
the grid's own: a ray that misses, one starting inside, one whose maxT lies inside the grid, rays with one and with two exactly-zero direction components, a ray along
a cell face; sample = 0, a sample so close to 1 that the density is never reached, samples landing in the first and in the last cell; for the point functions, points
on the clamped border of sampleTrilinear (voxel coordinates in [0, 0.5) and [dim - 0.5, dim]) and slightly outside."""
import numpy as np

from cudatracerlib_amd import api, scenes
import volume_cases
from volume_cases import BOX_LO, BOX_HI, _rot_y, _unit, _idx, same_rows   # noqa: F401

f32 = np.float32
SETS = ("grid_one", "grid_three", "grid_two", "grid_const")
ROWS = 256
FUNCTIONS = dict(volume_cases.FUNCTIONS)
FUNCTIONS.update({api.VEVAL_GRID_VALUE: "sampleTrilinear", api.VEVAL_REGION_SIGMA: "sigma_a / sigma_s / sigma_t", api.VEVAL_GRID_MARCH: "march steps"})
_BASE = dict(grid_one="one", grid_three="half", grid_two="two", grid_const="sixteen")   # whose seeds volume_cases.queries uses
ONE_MATRIX = _rot_y(30.0, (300, 320, 280), (200, 100, 150))


def make_set(name):
    """-> list of ctl_volume / api.GridVolume, for api.volumes_desc"""
    box = api.box_to_volume_matrix
    if name == "grid_one":
        return [api.grid_volume(ONE_MATRIX, density=scenes.smoke_density((3, 4, 5), 3), sig_a=(0.0, 0.002), sig_s=(0.0, (0.008, 0.004, 0.006)), phase=api.phase_hg(0.3))]
    if name == "grid_three":
        return [api.grid_volume(box(BOX_LO, BOX_HI), density_a=scenes.smoke_density((2, 3, 2), 4), density_s=scenes.smoke_density((4, 2, 3), 5),
                                sig_a=(0.0002, 0.003), sig_s=((0.0005, 0.0, 0.001), 0.006), phase=api.phase_isotropic())]
    if name == "grid_two":
        return [api.homogeneous_volume(box((0, 0, 0), (400, 548.8, 400)), 0.0005, 0.002, api.phase_rayleigh()),
                api.grid_volume(box((100, 50, 100), (556, 500, 559.2)), density=scenes.smoke_density((4, 3, 2), 6), sig_a=(0.0, 0.001), sig_s=(0.0, 0.005), phase=api.phase_hg(-0.4))]
    if name == "grid_const":
        return [api.grid_volume(box(BOX_LO, BOX_HI), density=np.full((8, 8, 8), 0.75, np.float32), sig_a=(0.0, 0.001), sig_s=(0.0, 0.004))]
    raise ValueError(name)


def regions(volumes):
    """the ctl_volume of every entry"""
    return [v.volume if isinstance(v, api.GridVolume) else v for v in volumes]


def grid_indices(volumes):
    return [i for i, v in enumerate(volumes) if isinstance(v, api.GridVolume)]


def _to_world(m, p):
    q = np.asarray(m, np.float64).reshape(4, 4) @ np.append(np.asarray(p, np.float64), 1.0)
    return (q[:3] / q[3]).astype(np.float32)


def _ray_rows(volumes, gi):
    """(o, d, minT, maxT, sample) branch rows for grid region gi, built in its unit cube and mapped to the world"""
    V = volumes[gi]; m = np.array(list(V.volume.volume_to_world.m), np.float32).reshape(4, 4)
    g = V.grid; dim = list(g.dim) if g.single_grid else [max(a, b) for a, b in zip(g.dim_a, g.dim_s)]
    W = lambda p: _to_world(m, p)
    rows = []

    def ray(a, b, max_frac=2.0, sample=0.5):
        pa, pb = W(a), W(b)
        L = float(np.linalg.norm(pb.astype(np.float64) - pa.astype(np.float64)))
        rows.append((pa, _unit(pb.astype(np.float64) - pa.astype(np.float64)), 0.0, L * max_frac, sample))
    ray((-0.5, 0.3, 0.4), (-1.5, 0.2, 0.3))                      # a miss: pointing away
    ray((0.31, 0.42, 0.53), (1.3, 0.9, 1.2))                     # starts inside
    ray((-0.4, 0.37, 0.61), (0.55, 0.52, 0.48), max_frac=1.0)    # maxT inside the grid
    c = (0.5 + 0.13) / dim[1]
    # exactly-zero direction components need an axis-aligned region: they are made in the local frame and are exact only there; in the world they are what they are
    rows.append((W((-0.3, 0.37, 0.61)), _unit(W((1.3, 0.37, 0.61)).astype(np.float64) - W((-0.3, 0.37, 0.61)).astype(np.float64)), 0.0, 3.0e3, 0.4))
    rows.append((W((0.2, c, -0.2)), _unit(W((0.2, c, 1.2)).astype(np.float64) - W((0.2, c, -0.2)).astype(np.float64)), 0.0, 3.0e3, 0.6))
    face = 1.0 / dim[0]
    ray((face, -0.2, 0.3), (face, 1.2, 0.8))                     # along a cell face
    for s in (0.0, float(np.nextafter(f32(1), f32(0))), 1e-4, 0.97):   # sample 0; never reached; the first cell; (with the densities here) the last cells
        ray((-0.2, 0.45, 0.55), (1.2, 0.5, 0.6), sample=s)
    return rows


def queries(set_name, volumes, what, n=ROWS):
    regs = regions(volumes); gis = grid_indices(volumes)
    rs = np.random.RandomState(7000 + 31 * what + SETS.index(set_name))
    if what <= api.VEVAL_EVAL_TRANSMITTANCE:
        q = volume_cases.queries(_BASE[set_name], regs, what, n)
        extra = []
        for gi in gis:
            for (o, d, minT, maxT, s) in _ray_rows(volumes, gi):
                r = np.zeros(10, np.float32)
                if what in (api.VEVAL_REGION_INTERSECT, api.VEVAL_REGION_TAU, api.VEVAL_REGION_SAMPLE_DISTANCE):
                    r[0] = _idx(np.uint32(gi)); r[1:4] = o; r[4:7] = d; r[7] = minT; r[8] = maxT; r[9] = s
                elif what in (api.VEVAL_INTERSECT, api.VEVAL_TAU, api.VEVAL_SAMPLE_DISTANCE, api.VEVAL_SAMPLE_VOLUME, api.VEVAL_TRANSMITTANCE):
                    r[0:3] = o; r[3:6] = d; r[6] = minT; r[7] = maxT; r[8] = s
                elif what == api.VEVAL_EVAL_TRANSMITTANCE:
                    r[0:3] = o; r[3:6] = (o + d * f32(min(maxT, 1500.0))).astype(np.float32)
                elif what == api.VEVAL_P:
                    r[0:3] = (o + d * f32(min(maxT, 1500.0) * 0.4)).astype(np.float32); r[3:6] = d; r[6:9] = _unit(rs.normal(size=3))
                else:
                    continue
                extra.append(r)
        if what in (api.VEVAL_REGION_TAU, api.VEVAL_REGION_SAMPLE_DISTANCE, api.VEVAL_TAU, api.VEVAL_SAMPLE_DISTANCE, api.VEVAL_TRANSMITTANCE) and set_name in ("grid_three", "grid_const"):
            # the Cornell-box regions are axis-aligned: rays with one and with two EXACTLY zero direction components, through cell interiors
            for o, d in (((-50, 130.3, 200.7), (1, 0, 0)), ((120.1, 600, 333.3), (0, -1, 0)), ((-20, 100.5, 77.7), _unit((1, 0, 0.4))), ((300.3, 50.2, -10), _unit((0, 0.3, 1)))):
                r = np.zeros(10, np.float32)
                if what in (api.VEVAL_REGION_TAU, api.VEVAL_REGION_SAMPLE_DISTANCE):
                    r[0] = _idx(np.uint32(gis[0])); r[1:4] = o; r[4:7] = d; r[7] = 0; r[8] = 2000; r[9] = 0.3
                else:
                    r[0:3] = o; r[3:6] = d; r[6] = 0; r[7] = 2000; r[8] = 0.3
                extra.append(r)
        if extra:
            q = np.concatenate([q, np.array(extra, np.float32)])
        return np.ascontiguousarray(q, np.float32)
    # ---- the grid's own functions
    rows = []
    for gi in gis:
        V = volumes[gi]; g = V.grid
        m = np.array(list(V.volume.volume_to_world.m), np.float32).reshape(4, 4)
        grids = [(0, list(g.dim))] if g.single_grid else [(0, list(g.dim_a)), (1, list(g.dim_s))]
        per = max(1, n // (len(gis) * (len(grids) if what == api.VEVAL_GRID_VALUE else 1)))
        if what == api.VEVAL_GRID_VALUE:
            for which, dim in grids:
                dm = np.array(dim, np.float32)
                p = (rs.uniform(-0.1, 1.1, (per, 3)) * dm).astype(np.float32)
                border = [(0.0, 0.0, 0.0), (0.25, 0.49, 0.1), tuple(dm), tuple(dm - 0.25), tuple(dm - 0.5), (0.5, 0.5, 0.5), (-0.3, 1.0, 1.0), tuple(dm + 0.3), (0.2, float(dm[1]) - 0.1, 1.5),
                          (float("nan"), 1.0, 1.0), (-1e9, 1e9, 5e9)]
                for pt in list(p) + border:
                    r = np.zeros(10, np.float32); r[0] = _idx(np.uint32(gi)); r[1] = _idx(np.uint32(which)); r[2:5] = pt; rows.append(r)
        elif what == api.VEVAL_REGION_SIGMA:
            u = rs.uniform(-0.15, 1.15, (per, 3))
            edge = [(0, 0, 0), (1, 1, 1), (0.01, 0.5, 0.99), (-0.01, 0.5, 1.01), (0.5, 0.5, 0.5)]
            for pt in list(u) + edge:
                r = np.zeros(10, np.float32); r[0] = _idx(np.uint32(gi)); r[1:4] = _to_world(m, pt); rows.append(r)
        else:   # api.VEVAL_GRID_MARCH
            a = rs.uniform(-0.5, 1.5, (per, 3)); b = rs.uniform(0, 1, (per, 3))
            for pa, pb in zip(a, b):
                o = _to_world(m, pa); e = _to_world(m, pb)
                r = np.zeros(10, np.float32); r[0] = _idx(np.uint32(gi)); r[1:4] = o; r[4:7] = _unit(e.astype(np.float64) - o.astype(np.float64)); r[7] = 0
                r[8] = 3.402823466e+38 if rs.rand() < 0.5 else float(np.linalg.norm(e - o)) * rs.uniform(0.3, 1.5)
                rows.append(r)
            for (o, d, minT, maxT, s) in _ray_rows(volumes, gi):
                r = np.zeros(10, np.float32); r[0] = _idx(np.uint32(gi)); r[1:4] = o; r[4:7] = d; r[7] = minT; r[8] = maxT; rows.append(r)
    return np.ascontiguousarray(np.array(rows, np.float32), np.float32)
