"""The independent yardstick of the heterogeneous media (not collected by pytest): a numpy float32 restatement of the reference's VolumeGrid, written from the
reference's source — SceneTypes/Volumes.h:101-287 (DenseVolGrid, VolumeGrid), SceneTypes/Volumes.cu:87-239 (tau, integrateDensity, invertDensityIntegral,
sampleDistance), Engine/SpatialStructures/Grid/SpatialGridTraversal.h:9-45 (TraverseGridRay) and the AABB::Intersect they call — not from csrc/volume_grid.h: one fp32
operation per numpy operation, in the source's order, exp / log from the shared-math oracle as volume_ref does.

GridVolumes subclasses volume_ref.Volumes: the aggregate, the phase functions and the homogeneous regions are its parent's; a region of type 2 dispatches to the grid
functions here (VolumeRegion's CALLER(...) dispatch).  path_trace(...) is volume_ref.path_trace with GridVolumes standing in for Volumes for that one call.

Two things are defined HERE where the reference has no defined value, as the library defines them: a float -> unsigned conversion gives 0 for a negative or
NaN argument and 0xffffffff from 2^32 on; and the march loop, which the reference never leaves once a NextCrossingT is NaN, ends after dim.x + dim.y + dim.z + 3
iterations — `cap_hits` counts how often, and the tests hold it to zero on every row and pixel.
"""
import struct

import numpy as np

import volume_ref
from volume_ref import f32, v3, FLT_MAX, fmin, fmax, length, transform_point, transform_direction, aabb_intersect, _avg, _ERR

VOLUME_GRID = 2
U32 = 0xffffffff


def f2u(x):
    """float -> unsigned int, defined: negative / NaN -> 0, >= 2^32 -> 0xffffffff, otherwise truncation"""
    x = f32(x)
    if not (x > 0):
        return 0
    if x >= f32(4294967296.0):
        return U32
    return int(x)


def _clamp(v, lo, hi):   # math::clamp = min(max(v, lo), hi) with (a < b) ? a : b
    return fmin(fmax(v, lo), hi)


def _rcp(a):   # math::rcp: a ? 1 / a : 0
    return f32(f32(1) / a) if a != 0 else f32(0)


def _sign(f):
    return f32(1) if f > 0 else (f32(-1) if f < 0 else f32(0))


def _copysign(a, b):
    ia = struct.unpack("<I", struct.pack("<f", float(a)))[0]; ib = struct.unpack("<I", struct.pack("<f", float(b)))[0]
    return f32(struct.unpack("<f", struct.pack("<I", (ib & 0x80000000) | (ia & 0x7fffffff)))[0])


def _ray_at(o, d, t):   # Ray::operator(): origin + d * direction
    return np.array([f32(o[i] + f32(t * d[i])) for i in range(3)], np.float32)


class DenseGrid:
    """DenseVolGrid<float> (Volumes.h:116-182): dim (x, y, z), the floats in its linear order"""

    def __init__(self, dim, data):
        self.dim = [int(x) for x in dim]
        self.dimF = np.array([f32(x) for x in self.dim], np.float32)
        self.data = np.ascontiguousarray(data, np.float32).reshape(-1)
        assert len(self.data) == self.dim[0] * self.dim[1] * self.dim[2]

    def idx(self, i, j, k):   # :139-142, as written: the first argument is clamped against dim.z and is the slowest
        dx, dy, dz = self.dim
        return min(k, dx - 1) + min(j, dy - 1) * dx + min(i, dz - 1) * dx * dy

    def value(self, i, j, k):
        return self.data[self.idx(i, j, k)]

    def trilinear(self, vsP):   # :157-181: weights from the unclamped corner, clamped fetch
        with np.errstate(**_ERR):
            p = [f32(vsP[0] - f32(0.5)), f32(vsP[1] - f32(0.5)), f32(vsP[2] - f32(0.5))]
            corner = [f2u(p[0]), f2u(p[1]), f2u(p[2])]
            val = f32(0)
            for i in range(2):
                cx = (corner[0] + i) & U32
                w0 = f32(f32(1) - abs(f32(p[0] - f32(cx))))
                for j in range(2):
                    cy = (corner[1] + j) & U32
                    w1 = f32(f32(1) - abs(f32(p[1] - f32(cy))))
                    for k in range(2):
                        cz = (corner[2] + k) & U32
                        w2 = f32(f32(1) - abs(f32(p[2] - f32(cz))))
                        v = self.value(min(max(cx, 0), self.dim[0] - 1), min(max(cy, 0), self.dim[1] - 1), min(max(cz, 0), self.dim[2] - 1))
                        val = f32(val + f32(f32(f32(w0 * w1) * w2) * v))
            return val


def traverse_grid_ray(o, d, tmin, tmax, gridSize, clb, stats):
    """TraverseGridRay (SpatialGridTraversal.h:9-45) over AABB(0, 1); clb(rayT, cellEndT) -> True to cancel.  stats: dict with 'steps' and 'cap_hits', added to"""
    with np.errstate(**_ERR):
        cell = np.array([f32(f32(f32(1) - f32(0)) / gridSize[i]) for i in range(3)], np.float32)
        hit, rayT, maxT = aabb_intersect(v3(0), v3(1), o, d, f32(0), FLT_MAX)   # Intersect<false>: bounds 0 and FLT_MAX
        if not hit:
            return
        rayT = _clamp(rayT, tmin, tmax)
        maxT = _clamp(maxT, tmin, tmax)
        at = _ray_at(o, d, rayT)
        q = [f32(f32(at[i] - f32(0)) / cell[i]) for i in range(3)]
        Pos = [f2u(np.floor(_clamp(q[i], f32(0), f32(gridSize[i] - f32(1))))) for i in range(3)]
        Step = [1 if d[i] > 0 else (-1 if d[i] < 0 else 0) for i in range(3)]
        ooeps = f32(2.0 ** -40)
        inv_d = [f32(f32(1) / (d[i] if abs(d[i]) > ooeps else _copysign(ooeps, d[i]))) for i in range(3)]
        N = []; D = []
        for i in range(3):
            up = fmax(f32(0), _sign(d[i]))
            face = f32(f32(0) + f32(f32(f32(Pos[i]) + up) * cell[i]))
            N.append(f32(rayT + f32(f32(face - at[i]) * inv_d[i])))
            D.append(f32(abs(f32(cell[i] * inv_d[i]))))
        cap = f2u(gridSize[0]) + f2u(gridSize[1]) + f2u(gridSize[2]) + 3
        steps = 0
        while True:
            if steps == cap:
                stats["cap_hits"] += 1
                break
            steps += 1
            bits = (int(N[0] < N[1]) << 2) + (int(N[0] < N[2]) << 1) + int(N[1] < N[2])
            axis = (0x00000a66 >> (bits * 2)) & 3
            cancel = clb(rayT, fmin(N[axis], maxT))
            Pos[axis] = (Pos[axis] + Step[axis]) & U32
            if f32(Pos[axis]) >= gridSize[axis] or maxT < N[axis]:
                break
            rayT = N[axis]
            N[axis] = f32(N[axis] + D[axis])
            if cancel:
                break
        stats["steps"] += steps


class GridVolumes(volume_ref.Volumes):
    """KernelAggregateVolume whose regions may be VolumeGrids.  volumes: a list of ctl_volume; grids: {volume index: dict(single, grid | gridA + gridS (DenseGrid),
    sigAMin, sigAMax, sigSMin, sigSMax (fp32 triples))} (grids_of_desc makes it from a description)"""

    def __init__(self, orc, volumes, grids):
        super().__init__(orc, volumes)
        self.stats = dict(steps=0, cap_hits=0, scatters=0)   # march steps, cap hits, successful aggregate sampleDistance calls (medium vertices)
        for i, (V, src) in enumerate(zip(self.v, volumes)):
            V["kind"] = int(src.type)
            if V["kind"] == VOLUME_GRID:
                V["G"] = grids[i]

    # ---- VolumeGrid
    def _tr(self, V, p, dimF):   # :247-252
        with np.errstate(**_ERR):
            c = transform_point(V["w2v"], p)
            return np.array([f32(_clamp(c[i], f32(0), f32(1)) * dimF[i]) for i in range(3)], np.float32)

    def _density_a(self, V, p):
        G = V["G"]; g = G["grid"] if G["single"] else G["gridA"]
        return g.trilinear(self._tr(V, p, g.dimF))

    def _density_s(self, V, p):
        G = V["G"]; g = G["grid"] if G["single"] else G["gridS"]
        return g.trilinear(self._tr(V, p, g.dimF))

    @staticmethod
    def _lerp(lo, hi, x):   # min + (max - min) * x on spectra
        with np.errstate(**_ERR):
            return (lo + ((hi - lo).astype(np.float32) * f32(x)).astype(np.float32)).astype(np.float32)

    def grid_sigma_a(self, V, p):
        G = V["G"]
        return self._lerp(G["sigAMin"], G["sigAMax"], self._density_a(V, p))

    def grid_sigma_s(self, V, p):
        G = V["G"]
        return self._lerp(G["sigSMin"], G["sigSMax"], self._density_s(V, p))

    def grid_sigma_t(self, V, p):   # :207-212
        G = V["G"]
        if G["single"]:
            a = s = G["grid"].trilinear(self._tr(V, p, G["grid"].dimF))
        else:
            a = G["gridA"].trilinear(self._tr(V, p, G["gridA"].dimF)); s = G["gridS"].trilinear(self._tr(V, p, G["gridS"].dimF))
        with np.errstate(**_ERR):
            r = self._lerp(G["sigAMin"], G["sigAMax"], a)
            r = (r + G["sigSMin"]).astype(np.float32)
            return (r + ((G["sigSMax"] - G["sigSMin"]).astype(np.float32) * f32(s)).astype(np.float32)).astype(np.float32)

    def _local(self, V, o, d, t0, t1):
        with np.errstate(**_ERR):
            G = V["G"]
            ol = transform_point(V["w2v"], o); dl = transform_direction(V["w2v"], d)
            Td = length(dl)
            minTL = f32(t0 * Td); maxTL = f32(t1 * Td)
            dl = (dl * _rcp(Td)).astype(np.float32)
            if G["single"]:
                dimF = G["grid"].dimF
            else:
                dimF = np.array([fmax(G["gridS"].dimF[i], G["gridA"].dimF[i]) for i in range(3)], np.float32)
            return ol, dl, minTL, maxTL, dimF

    def _step_density(self, V, ol, dl, rayT, cellEndT):
        G = V["G"]
        with np.errstate(**_ERR):
            a = _ray_at(ol, dl, rayT); b = _ray_at(ol, dl, cellEndT)
            if G["single"]:
                g = G["grid"]
                d_s = d_a = f32(g.trilinear((g.dimF * a).astype(np.float32)) + g.trilinear((g.dimF * b).astype(np.float32)))
            else:
                gs, ga = G["gridS"], G["gridA"]
                d_s = f32(gs.trilinear((gs.dimF * a).astype(np.float32)) + gs.trilinear((gs.dimF * b).astype(np.float32)))
                d_a = f32(ga.trilinear((ga.dimF * a).astype(np.float32)) + ga.trilinear((ga.dimF * b).astype(np.float32)))
            return f32(d_s / f32(2)), f32(d_a / f32(2))

    def integrate_density(self, V, o, d, t0, t1):   # Volumes.cu:145-171
        G = V["G"]
        ol, dl, minTL, maxTL, dimF = self._local(V, o, d, t0, t1)
        acc = [f32(0), f32(0)]   # D_s, D_a

        def clb(rayT, cellEndT):
            d_s, d_a = self._step_density(V, ol, dl, rayT, cellEndT)
            with np.errstate(**_ERR):
                acc[0] = f32(acc[0] + f32(d_s * f32(cellEndT - rayT)))
                acc[1] = f32(acc[1] + f32(d_a * f32(cellEndT - rayT)))
            return False
        traverse_grid_ray(ol, dl, minTL, maxTL, dimF, clb, self.stats)
        with np.errstate(**_ERR):
            L = f32(f32(t1 - t0) / f32(maxTL - minTL))
            D_a = f32(acc[1] * L); D_s = f32(acc[0] * L)
            r = self._lerp(G["sigAMin"], G["sigAMax"], D_s)     # as written: the A range with D_s
            r = (r + G["sigSMin"]).astype(np.float32)
            return (r + ((G["sigSMax"] - G["sigSMin"]).astype(np.float32) * D_a).astype(np.float32)).astype(np.float32)

    def invert_density_integral(self, V, o, d, t0, t1, desired):
        """-> (found, integratedDensity, t or None, densityAtMinT, densityAtT)   (Volumes.cu:173-214)"""
        G = V["G"]
        ol, dl, minTL, maxTL, dimF = self._local(V, o, d, t0, t1)
        st = dict(integrated=f32(0), t=None, atT=f32(0), found=False)
        with np.errstate(**_ERR):
            atMin = _avg(self.grid_sigma_t(V, _ray_at(o, d, t0)))
            L = f32(f32(t1 - t0) / f32(maxTL - minTL))

        def clb(rayT, cellEndT):
            d_s, d_a = self._step_density(V, ol, dl, rayT, cellEndT)
            with np.errstate(**_ERR):
                d_s = _avg(self._lerp(G["sigSMin"], G["sigSMax"], d_s))
                d_a = _avg(self._lerp(G["sigAMin"], G["sigAMax"], d_s))   # as written: from the overwritten d_s
                D = f32(f32(f32(d_s + d_a) * f32(cellEndT - rayT)) * L)
                if f32(st["integrated"] + D) >= desired:
                    st["atT"] = f32(d_s + d_a)
                    st["t"] = f32(f32(f32(desired - st["integrated"]) / st["atT"]) + f32(rayT * L))
                    st["integrated"] = desired
                    st["found"] = True
                    return True
                st["integrated"] = f32(st["integrated"] + D)
                return False
        traverse_grid_ray(ol, dl, minTL, maxTL, dimF, clb, self.stats)
        return st["found"], st["integrated"], st["t"], atMin, st["atT"]

    def grid_tau(self, V, o, d, minT, maxT):   # Volumes.cu:135-143
        with np.errstate(**_ERR):
            ln = length(d)
            if ln == 0:
                return v3(0)
            dn = (d / ln).astype(np.float32)
            b, t0, t1 = self.region_intersect(V, o, dn, f32(f32(minT) * ln), f32(f32(maxT) * ln))
            if not b:
                return v3(0)
            return self.integrate_density(V, o, dn, t0, t1)

    def grid_sample_distance(self, V, o, d, minT, maxT, sample, mRec):   # Volumes.cu:216-239
        m = self.m
        with np.errstate(**_ERR):
            ln = length(d)
            if ln == 0:
                return False
            dn = (d / ln).astype(np.float32)
            b, t0, t1 = self.region_intersect(V, o, dn, f32(f32(minT) * ln), f32(f32(maxT) * ln))
            if not b:
                return False
            desired = f32(-m.log(f32(f32(1) - f32(sample))))
            found, integrated, t, atMin, atT = self.invert_density_integral(V, o, dn, t0, t1, desired)
            success = False
            if found:
                success = True
                mRec["t"] = t
                mRec["p"] = _ray_at(o, d, t)
                mRec["sigmaS"] = self.grid_sigma_s(V, mRec["p"])
                mRec["sigmaA"] = self.grid_sigma_s(V, mRec["p"])   # as written
            expVal = m.exp(f32(-integrated))
            mRec["pdfFailure"] = expVal
            mRec["pdfSuccess"] = f32(expVal * atT)
            mRec["pdfSuccessRev"] = f32(expVal * atMin)
            mRec["transmittance"] = v3(expVal)
            mRec["written"] = True
            return bool(success and mRec["pdfSuccess"] > 0)

    def march(self, V, o, d, minT, maxT):
        """(steps, cap hit) of grid_tau's march"""
        before = dict(self.stats)
        self.grid_tau(V, o, d, minT, maxT)
        return self.stats["steps"] - before["steps"], self.stats["cap_hits"] - before["cap_hits"]

    # ---- VolumeRegion's dispatch
    def region_tau(self, V, o, d, minT, maxT):
        if V.get("kind") == VOLUME_GRID:
            return self.grid_tau(V, np.asarray(o, np.float32), np.asarray(d, np.float32), minT, maxT)
        return super().region_tau(V, o, d, minT, maxT)

    def region_sample_distance(self, V, o, d, minT, maxT, rand, mRec):
        if V.get("kind") == VOLUME_GRID:
            return self.grid_sample_distance(V, np.asarray(o, np.float32), np.asarray(d, np.float32), minT, maxT, rand, mRec)
        return super().region_sample_distance(V, o, d, minT, maxT, rand, mRec)

    def sample_distance(self, o, d, minT, maxT, sample, mRec):
        ok = super().sample_distance(o, d, minT, maxT, sample, mRec)
        if ok:
            self.stats["scatters"] += 1
        return ok

    def p(self, p, wi, wo):   # KernelAggregateVolume::p with sigma_s(p) through the dispatch
        ph = f32(0); sumWt = f32(0)
        with np.errstate(**_ERR):
            for V in self.v:
                lo, hi = V["bound"]
                if all(lo[i] <= p[i] <= hi[i] for i in range(3)):
                    if V.get("kind") == VOLUME_GRID:
                        wt = _avg(self.grid_sigma_s(V, np.asarray(p, np.float32)))
                    else:
                        wt = _avg(V["sig_s"] if self.inside_world(V, p) else v3(0))
                    sumWt = f32(sumWt + wt)
                    ph = f32(ph + f32(wt * self.phase_eval(V, wi, wo)))
            return f32(ph / sumWt) if sumWt != 0 else f32(0)


def grids_of_desc(desc):
    """{volume index: grid dict} from a description's volume_grids"""
    out = {}
    for k in range(desc.n_volume_grids):
        g = desc.volume_grids[k]

        def grid(dim, ptr):
            n = int(dim[0]) * int(dim[1]) * int(dim[2])
            return DenseGrid(list(dim), np.ctypeslib.as_array(ptr, shape=(n,)).copy())
        rec = dict(single=bool(g.single_grid), sigAMin=np.array(list(g.sig_a_min), np.float32), sigAMax=np.array(list(g.sig_a_max), np.float32),
                   sigSMin=np.array(list(g.sig_s_min), np.float32), sigSMax=np.array(list(g.sig_s_max), np.float32))
        if rec["single"]:
            rec["grid"] = grid(g.dim, g.data)
        else:
            rec["gridA"] = grid(g.dim_a, g.data_a); rec["gridS"] = grid(g.dim_s, g.data_s)
        out[int(g.volume)] = rec
    return out


def volumes_of_desc(orc, desc):
    return GridVolumes(orc, [desc.volumes[i] for i in range(desc.n_volumes)], grids_of_desc(desc))


def eval_rows(V, what, queries):
    """the rows ctl_volume_eval returns, codes 0-15, from the restatement"""
    if what <= 12:
        return volume_ref.eval_rows(V, what, queries)
    q = np.ascontiguousarray(queries, np.float32).reshape(-1, 10)
    out = np.zeros((len(q), 17), np.float32)
    for a, o in zip(q, out):
        R = V.v[volume_ref._word(a[0])]; G = R["G"]
        if what == 13:
            g = G["grid"] if G["single"] else (G["gridS"] if volume_ref._word(a[1]) else G["gridA"])
            o[0] = g.trilinear(a[2:5])
        elif what == 14:
            o[0:3] = V.grid_sigma_a(R, a[1:4]); o[3:6] = V.grid_sigma_s(R, a[1:4]); o[6:9] = V.grid_sigma_t(R, a[1:4])
        elif what == 15:
            o[0], o[1] = V.march(R, a[1:4], a[4:7], a[7], a[8])
        else:
            raise ValueError(what)
    return out


class _PixelHook:
    """stands in for path_trace's pixel_rays array: `hook[y, x] += rays` is what path_trace does when a pixel's path has ended, so the medium vertices counted since
    the previous pixel are that pixel's"""

    def __init__(self, made, vertices):
        self.made, self.vertices, self.seen = made, vertices, 0

    def __getitem__(self, idx):
        return 0

    def __setitem__(self, idx, value):
        n = self.made[0].stats["scatters"]
        self.vertices[idx] += n - self.seen
        self.seen = n


def path_trace(orc, desc, w, h, tables, stats=None, vertices=None, **kw):
    """volume_ref.path_trace of a description whose media may hold VolumeGrids: GridVolumes stands in for volume_ref.Volumes for this one call (volume_ref._Path looks
    the class up by name when it is called).  stats: a dict that receives the march's 'steps', 'cap_hits' and 'scatters'; vertices: an int array (h, w), added to —
    the medium vertices of each pixel's paths (frames only)"""
    grids = grids_of_desc(desc)
    made = []
    if vertices is not None:
        kw["pixel_rays"] = _PixelHook(made, vertices)

    def stand_in(orc_, volumes):
        made.append(GridVolumes(orc_, volumes, grids))
        return made[-1]
    keep = volume_ref.Volumes
    volume_ref.Volumes = stand_in
    try:
        return volume_ref.path_trace(orc, desc, [desc.volumes[i] for i in range(desc.n_volumes)], w, h, tables, **kw)
    finally:
        volume_ref.Volumes = keep
        if stats is not None and made:
            stats.update(made[0].stats)
