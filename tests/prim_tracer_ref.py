"""Per-pixel restatement of the PrimTracer's computePixel (Integrators/PrimTracer.cu:19-106) from the shared-math oracle's exports (not collected by pytest).

primary(orc, desc, w, h, tables, flat) follows every pixel to its first hit as the reference does — rng = g_SamplerData(y * w + x), the aperture sample is the first
2-D draw, sampleRayDifferential's own ray from the pixel's position (no jitter), traceRay with the alpha test — and returns, per pixel, the quantities the drawing
modes read after TraceResult::getBsdfSample: the flipped geometric / shading normals, uv, the barycentrics, the local wi, the material, the emission.
flat: the product's flattened BVH (cudatracerlib_amd.api.FlatBvh(...).desc), so that a ray grazing the edge two triangles share resolves to the triangle the
device's traversal picks; None traverses the reference's two-level structure.  half_host_quirk: the triangles' halves (normals, uv) are decoded with
half::ToFloat's host branch, as the reference compiled for the host decodes them (tests/test_oracle_prim_tracer.py pins this file on it).
geometry_frame(...) turns that into the frame of a geometry mode; environment(...) gives the misses' EvalEnvironment(r, rX, rY); shaded_modes(...) runs
computePixel in full for the six shaded modes (next-event estimation with MIS and its shadow ray, the BSDF-sampled delta chain with its quirks) and counts its
traceRay / Occluded calls; shaded_first(...) gives the material's delta flag.
"""
import ctypes as C

import numpy as np

f32 = np.float32
FLT_MAX = f32(3.402823466e+38)
CTL_MAP_NONE = 0
GEOMETRY_MODES = ("linear_depth", "D3D_depth", "v_absdot_n_geo", "v_dot_n_geo", "v_dot_n_shade", "n_geo_colored", "n_shade_colored", "uv", "bary_coords")
SHADED_MODES = ("first_Le", "first_f", "first_f_direct", "first_non_delta_Le", "first_non_delta_f", "first_non_delta_f_direct")
E_DELTA = 0x1 | 0x20 | 0x40
E_ALL = 0x1ff


def _dot(a, b):   # ctl_math.h dot: fp32, left to right, no contraction
    r = f32(a[0]) * f32(b[0]); r = f32(r + f32(a[1]) * f32(b[1])); return f32(r + f32(a[2]) * f32(b[2]))


def _bind(lib):
    lib.orc_sensor_sample_rays.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    lib.orc_bsdf_eval_uv.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_void_p]
    lib.orc_light_eval.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


class _Ctx:
    """the scene's arrays and the oracle calls computePixel is made of"""

    def __init__(self, orc, desc, half_host_quirk=False):
        self.orc, self.lib, self.desc, self.quirk = orc, orc.lib, desc, half_host_quirk
        _bind(self.lib)
        self.tri_data = np.frombuffer(C.string_at(desc.tri_data, desc.n_tri_data * 32), np.uint32).reshape(-1, 8)
        self.xforms = np.frombuffer(C.string_at(desc.node_transforms, desc.n_nodes * 64), np.float32).reshape(-1, 16)
        self.nodes = np.frombuffer(C.string_at(desc.nodes, desc.n_nodes * 24), np.uint32).reshape(-1, 6)
        self.eps = f32(desc.ray_trace_eps)

    def surface(self, o, d, hd):
        """TraceResult::getBsdfSample (Kernel/TraceResult.cu:16-43): fillDG, wi, the normal map, the two-sided flip"""
        lib, desc = self.lib, self.desc
        dg = np.zeros(21, np.float32)
        tri, node = int(hd["tri_idx"]), int(hd["node_idx"])
        t, u, v = f32(hd["dist"]), f32(hd["u"]), f32(hd["v"])
        T = np.ascontiguousarray(self.tri_data[tri]); M = np.ascontiguousarray(self.xforms[node])
        lib.orc_triangle_fill_dg(T.ctypes.data, M.ctypes.data, float(u), float(v), 1 if self.quirk else 0, dg.ctypes.data)
        P = np.array([f32(o[k] + f32(t * d[k])) for k in range(3)], np.float32)
        s_, t_, sn, gn = dg[0:3].copy(), dg[3:6].copy(), dg[6:9].copy(), dg[9:12].copy()
        md = -np.asarray(d, np.float32)
        wi = np.array([_dot(md, s_), _dot(md, t_), _dot(md, sn)], np.float32)   # bRec.wi = dg.toLocal(-r.dir()), before the normal map
        mi = int(self.nodes[node, 1]) + int((T[1] >> 16) & 0xff)
        mat = desc.materials[mi]
        if mat.map_kind != CTL_MAP_NONE:
            frame = np.concatenate([s_, t_, sn]).astype(np.float32); geo = np.ascontiguousarray(dg[9:18])
            lib.orc_sample_normal_map(C.addressof(desc), C.byref(mat), float(dg[18]), float(dg[19]), frame.ctypes.data, geo.ctypes.data)
            s_, t_, sn = frame[0:3], frame[3:6], frame[6:9]
        if mat.two_sided and wi[2] < 0:
            gn = -gn; sn = -sn; wi[2] = -wi[2]
        return dict(t=t, n=gn, uv=dg[18:20].copy(), bary=(u, v), wi=wi, P=P, frame=np.concatenate([s_, t_, sn]).astype(np.float32), mat=mi, node=node)


def add_sample_clamp(L):
    """Image::AddSample (Engine/Image.cu:22-28) clamps negative components to 0: a shading normal that a normal map turned away from the viewer gives
    v_dot_n_shade = 0 in the frame, not the negative dot"""
    return np.maximum(L, f32(0)).astype(np.float32)


def d3d_depth(near, far, t):
    """DeviceDepthImage::NormalizeDepthD3D (Kernel/Tracer.h:26-31) in fp32"""
    near, far = f32(near), f32(far)
    z = f32(min(max(f32(t), near), far))
    return f32(f32(f32(far / f32(far - near)) * z - f32(far * near) / f32(far - near)) / z)


def primary(orc, desc, w, h, tables, flat=None, half_host_quirk=False):
    lib = orc.lib
    _bind(lib)
    t1, t2 = (np.ascontiguousarray(a, np.float32) for a in tables)
    n = w * h
    rays = np.zeros((n, 8), np.float32)
    dX = np.zeros((n, 3), np.float32); dY = np.zeros((n, 3), np.float32)
    ap = np.zeros(2, np.float32); o18 = np.zeros(18, np.float32); o6 = np.zeros(6, np.float32)
    eps = f32(desc.ray_trace_eps)
    for y in range(h):
        for x in range(w):
            i = y * w + x
            lib.orc_sampler_float2(t1.ctypes.data, t2.ctypes.data, i, 0, ap.ctypes.data)   # the first 2-D draw: the aperture sample
            lib.orc_sensor_sample_rays(C.addressof(desc.camera), float(x), float(y), float(ap[0]), float(ap[1]), o18.ctypes.data, o6.ctypes.data)
            rays[i, :3] = o6[:3]; rays[i, 3] = eps; rays[i, 4:7] = o6[3:]; rays[i, 7] = FLT_MAX
            dX[i] = o18[9:12]; dY[i] = o18[15:18]
    hits = orc.intersect(desc, rays, alpha_test=True, flat=flat, half_host_quirk=half_host_quirk)
    out = dict(quirk=half_host_quirk, hit=np.zeros(n, bool), t=np.full(n, FLT_MAX, np.float32), n=np.zeros((n, 3), np.float32), sn=np.zeros((n, 3), np.float32),
               uv=np.zeros((n, 2), np.float32), bary=np.zeros((n, 2), np.float32), wi=np.zeros((n, 3), np.float32), P=np.zeros((n, 3), np.float32),
               frame=np.zeros((n, 9), np.float32), mat=np.full(n, -1, np.int64), node=np.full(n, -1, np.int64), rays=rays, dX=dX, dY=dY, flat=flat, tri=hits["tri_idx"].copy())
    ctx = _Ctx(orc, desc, half_host_quirk)
    for i in range(n):
        hd = hits[i]
        if hd["tri_idx"] < 0:
            continue
        rec = ctx.surface(rays[i, :3], rays[i, 4:7], hd)
        out["hit"][i] = True; out["t"][i] = rec["t"]; out["n"][i] = rec["n"]; out["sn"][i] = rec["frame"][6:9]; out["uv"][i] = rec["uv"]; out["bary"][i] = rec["bary"]
        out["wi"][i] = rec["wi"]; out["P"][i] = rec["P"]; out["frame"][i] = rec["frame"]; out["mat"][i] = rec["mat"]; out["node"][i] = rec["node"]
    return out


def geometry_frame(pr, desc, w, h, mode):
    """L of a geometry mode at every hit pixel (h, w, 3); misses are left 0 (the caller handles EvalEnvironment)"""
    near, far = f32(desc.camera.near_depth), f32(desc.camera.far_depth)
    L = np.zeros((w * h, 3), np.float32)
    for i in np.nonzero(pr["hit"])[0]:
        md = -pr["rays"][i, 4:7]
        if mode == "linear_depth":
            L[i] = f32(f32(pr["t"][i] - near) / f32(far - near))
        elif mode == "D3D_depth":
            L[i] = d3d_depth(near, far, pr["t"][i])
        elif mode == "v_absdot_n_geo":
            L[i] = abs(_dot(md, pr["n"][i]))
        elif mode == "v_dot_n_geo":
            L[i] = _dot(md, pr["n"][i])
        elif mode == "v_dot_n_shade":
            L[i] = _dot(md, pr["sn"][i])
        elif mode in ("n_geo_colored", "n_shade_colored"):
            nn = pr["n"][i] if mode == "n_geo_colored" else pr["sn"][i]
            L[i] = (nn + f32(1)) / f32(2)
        elif mode == "uv":
            L[i] = (pr["uv"][i, 0], pr["uv"][i, 1], 0)
        elif mode == "bary_coords":
            L[i] = (pr["bary"][i, 0], pr["bary"][i, 1], 0)
        else:
            raise ValueError(mode)
    return add_sample_clamp(L).reshape(h, w, 3)


def environment(orc, pr, desc, w, h):
    """EvalEnvironment(r, rX, rY) (KernelDynamicScene.cu:62-68 -> InfiniteLight::evalEnvironment(r, rX, rY)) at every pixel whose primary ray misses (h, w, 3), with
    the ray differentials of sampleRayDifferential; 0 at hits, and everywhere without an environment map"""
    lib = orc.lib
    lib.orc_env_eval_differential_n.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    miss = np.nonzero(~pr["hit"])[0]
    d = np.ascontiguousarray(pr["rays"][miss, 4:7]); dx = np.ascontiguousarray(pr["dX"][miss]); dy = np.ascontiguousarray(pr["dY"][miss])
    out = np.zeros((len(miss), 3), np.float32)
    if len(miss):
        lib.orc_env_eval_differential_n(C.addressof(desc), len(miss), d.ctypes.data, dx.ctypes.data, dy.ctypes.data, out.ctypes.data)
    L = np.zeros((w * h, 3), np.float32)
    L[miss] = out
    return add_sample_clamp(L).reshape(h, w, 3)


def shaded_first(orc, pr, desc, w, h):
    """f_avg (bsdf.f with wo = (0, 0, 1), mask EAll), Le (TraceResult::Le) and whether the material has a delta lobe, at every hit pixel.
    The BSDF is evaluated at the hit's uv: meant for scenes with constant or checkerboard textures, where the ray differentials do not enter."""
    lib = orc.lib
    _bind(lib)
    lib.orc_set_probe_materials(C.cast(desc.materials, C.c_void_p))
    lib.orc_set_probe_rough_transmittance(C.cast(desc.rough_transmittance, C.c_void_p) if desc.rough_transmittance else None)
    nodes = np.frombuffer(C.string_at(desc.nodes, desc.n_nodes * 24), np.uint32).reshape(-1, 6)
    n = w * h
    f_avg = np.zeros((n, 3), np.float32); Le = np.zeros((n, 3), np.float32); delta = np.zeros(n, bool)
    wo = np.array([0, 0, 1], np.float32); out = np.zeros(4, np.float32); le = np.zeros(3, np.float32)
    try:
        for i in np.nonzero(pr["hit"])[0]:
            mat = desc.materials[int(pr["mat"][i])]
            wi = np.ascontiguousarray(pr["wi"][i])
            lib.orc_bsdf_eval_uv(C.byref(mat), wi.ctypes.data, wo.ctypes.data, E_ALL, 1, float(pr["uv"][i, 0]), float(pr["uv"][i, 1]), out.ctypes.data)
            f_avg[i] = out[:3]
            delta[i] = (mat.combined_type & E_DELTA) != 0
            if mat.node_light_index != 0xffffffff:
                light = int(nodes[int(pr["node"][i]), 3 if mat.node_light_index == 0 else 4])
                P = np.ascontiguousarray(pr["P"][i]); sn = np.ascontiguousarray(pr["frame"][i, 6:9]); md = np.ascontiguousarray(-pr["rays"][i, 4:7])
                lib.orc_light_eval(C.addressof(desc), light, P.ctypes.data, sn.ctypes.data, md.ctypes.data, le.ctypes.data)
                Le[i] = le
    finally:
        lib.orc_set_probe_materials(None); lib.orc_set_probe_rough_transmittance(None)
    return f_avg.reshape(h, w, 3), Le.reshape(h, w, 3), delta.reshape(h, w)


E_SMOOTH = 0x2 | 0x4 | 0x8 | 0x10
CTL_TEX_IMAGE = 4
CTL_LIGHT_POINT, CTL_LIGHT_DIFFUSE, CTL_LIGHT_DISTANT, CTL_LIGHT_SPOT, CTL_LIGHT_INFINITE = 1, 2, 3, 4, 5


class _NotRestated(Exception):
    """the pixel reaches a surface with an image texture: the device filters it (with ray differentials at the primary hit), the oracle's BSDF probes do not"""


def shaded_modes(orc, pr, desc, w, h, tables, max_path_length):
    """computePixel (PrimTracer.cu:19-106) for the six shaded modes, every pixel that hits: {mode: (frame (h, w, 3), rays of the pass, rays of each pixel (h, w),
    the distance of each pixel's last traceRay (h, w): what g_DepthImage2.Store receives)} and the mask of the pixels restated (hits whose path meets no image
    texture).  The rays are one per traceRay / Occluded, the misses' primary rays included.
    Built from the oracle's probes: orc_sampler_float2 (the draws, in the device's order), orc_emitter_select + orc_light_sample_direct (UniformSampleOneLight's
    sampleEmitter and sampleDirect), orc_bsdf_eval_uv / orc_bsdf_sample_uv, Oracle.intersect (closest and any hit, alpha-tested) and orc_light_eval."""
    lib = orc.lib
    ctx = _Ctx(orc, desc, pr.get("quirk", False))
    lib.orc_bsdf_sample_uv.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
    lib.orc_light_sample_direct.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    lib.orc_emitter_select.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    t1, t2 = (np.ascontiguousarray(a, np.float32) for a in tables)
    n = w * h
    eps = ctx.eps
    mats = desc.materials

    def has_image(mat):
        return any(mat.tex[k].type == CTL_TEX_IMAGE for k in range(4))

    def to_local(fr, v):
        return np.array([_dot(v, fr[0:3]), _dot(v, fr[3:6]), _dot(v, fr[6:9])], np.float32)

    def to_world(fr, v):   # ctl_math.h frame::to_world: s * v.x + t * v.y + n * v.z
        return (fr[0:3] * v[0] + fr[3:6] * v[1] + fr[6:9] * v[2]).astype(np.float32)

    def bsdf_f(mat, rec, wo, mask):
        if has_image(mat):
            raise _NotRestated()
        out = np.zeros(4, np.float32); wi = np.ascontiguousarray(rec["wi"]); wo = np.ascontiguousarray(wo, np.float32)
        lib.orc_bsdf_eval_uv(C.byref(mat), wi.ctypes.data, wo.ctypes.data, mask, 1, float(rec["uv"][0]), float(rec["uv"][1]), out.ctypes.data)
        return out[:3].copy(), f32(out[3])

    def bsdf_sample(mat, rec, smp):
        if has_image(mat):
            raise _NotRestated()
        out = np.zeros(9, np.float32); wi = np.ascontiguousarray(rec["wi"])
        lib.orc_bsdf_sample_uv(C.byref(mat), wi.ctypes.data, float(smp[0]), float(smp[1]), float(rec["uv"][0]), float(rec["uv"][1]), out.ctypes.data)
        return out[:3].copy(), out[4:7].copy()

    def le(mat, rec, d):
        if mat.node_light_index == 0xffffffff:
            return np.zeros(3, np.float32)
        light = int(ctx.nodes[rec["node"], 3 if mat.node_light_index == 0 else 4])
        out = np.zeros(3, np.float32); P = np.ascontiguousarray(rec["P"]); sn = np.ascontiguousarray(rec["frame"][6:9]); md = np.ascontiguousarray(-d)
        lib.orc_light_eval(C.addressof(desc), light, P.ctypes.data, sn.ctypes.data, md.ctypes.data, out.ctypes.data)
        return out

    def trace(o, d, tmax=FLT_MAX, any_hit=False):
        r = np.zeros((1, 8), np.float32); r[0, :3] = o; r[0, 3] = eps; r[0, 4:7] = d; r[0, 7] = tmax
        return orc.intersect(desc, r, any_hit=any_hit, alpha_test=True, threads=1, flat=pr["flat"], half_host_quirk=ctx.quirk)[0]

    def one_light(mat, rec, draw, cnt):
        """UniformSampleOneLight + EstimateDirect (Kernel/TraceAlgorithms.cu:44-101), mask EAll & ~EDelta, MIS"""
        if desc.num_lights == 0:
            return np.zeros(3, np.float32)
        sl = draw()
        slot = np.zeros(1, np.int32); lpdf = np.zeros(1, np.float32); rs = np.zeros(1, np.float32); pe = np.zeros(1, np.float32)
        lib.orc_emitter_select(C.addressof(desc), 0, 1, sl.ctypes.data, slot.ctypes.data, lpdf.ctypes.data, rs.ctypes.data, pe.ctypes.data)
        if slot[0] < 0:
            return np.zeros(3, np.float32)
        s2 = draw()
        out = np.zeros(14, np.float32); P = np.ascontiguousarray(rec["P"]); sn = np.ascontiguousarray(rec["frame"][6:9])
        lib.orc_light_sample_direct(C.addressof(desc), int(slot[0]), P.ctypes.data, sn.ctypes.data, float(s2[0]), float(s2[1]), out.ctypes.data)
        value, pdf, dd, dist = out[0:3], f32(out[3]), out[4:7].copy(), f32(out[7])
        r = np.zeros(3, np.float32)
        if (value != 0).any():
            f, bpdf = bsdf_f(mat, rec, to_local(rec["frame"], dd), E_ALL & ~E_DELTA)
            if (f != 0).any():
                cnt[0] += 1
                if trace(P, dd, f32(dist - eps), any_hit=True)["tri_idx"] < 0:   # Occluded(r, 0, dist)
                    L = desc.lights[int(slot[0])]
                    discrete = L.type in (CTL_LIGHT_POINT, CTL_LIGHT_SPOT, CTL_LIGHT_DISTANT) or (L.type == CTL_LIGHT_DIFFUSE and L.orthogonal)
                    weight = f32(1)
                    if not discrete:   # solid-angle measure: PowerHeuristic(1, pdf * lightPdf, 1, bsdfPdf)
                        a = f32(pdf * lpdf[0]); weight = f32(f32(a * a) / f32(f32(a * a) + f32(bpdf * bpdf)))
                    r = (value * f * weight).astype(np.float32)
        return (r * f32(f32(1) / lpdf[0])).astype(np.float32)   # / pdf (Spectrum::operator/ multiplies by the reciprocal)

    res = {m: np.zeros((n, 3), np.float32) for m in SHADED_MODES}
    rays = {m: np.ones(n, np.int64) for m in SHADED_MODES}   # the primary traceRay of every pixel
    last_t = {m: pr["t"].copy() for m in SHADED_MODES}
    ok = np.zeros(n, bool)
    for i in np.nonzero(pr["hit"])[0]:
        rec0 = dict(t=pr["t"][i], n=pr["n"][i], uv=pr["uv"][i], wi=pr["wi"][i], P=pr["P"][i], frame=pr["frame"][i], mat=int(pr["mat"][i]), node=int(pr["node"][i]))
        d0 = pr["rays"][i, 4:7]
        try:
            for mode in SHADED_MODES:
                k = [1]   # d2 of the next 2-D draw: the aperture sample was draw 0

                def draw():
                    out = np.zeros(2, np.float32)
                    lib.orc_sampler_float2(t1.ctypes.data, t2.ctypes.data, int(i), k[0], out.ctypes.data); k[0] += 1
                    return out
                cnt = [0]
                mat = mats[rec0["mat"]]; rec = rec0
                f_avg, _ = bsdf_f(mat, rec, np.array([0, 0, 1], np.float32), E_ALL)
                Le = le(mat, rec, d0)
                is_delta = (mat.combined_type & E_DELTA) != 0
                if mode == "first_Le" or (not is_delta and mode == "first_non_delta_Le"):
                    L = Le
                elif mode == "first_f" or (not is_delta and mode == "first_non_delta_f"):
                    L = f_avg
                elif mode == "first_f_direct" or (not is_delta and mode == "first_non_delta_f_direct"):
                    L = Le + (one_light(mat, rec, draw, cnt) + f_avg * f32(0.5))
                else:   # the delta chain, as written (PrimTracer.cu:68-96)
                    f, wo = bsdf_sample(mat, rec, draw())
                    through = f.copy()
                    depth = 0
                    while True:
                        o = rec["P"]; d = to_world(rec["frame"], wo)
                        hd = trace(o, d); cnt[0] += 1
                        hit = hd["tri_idx"] >= 0
                        last_t[mode][i] = hd["dist"] if hit else FLT_MAX
                        if hit:
                            rec = ctx.surface(o, d, hd); mat = mats[rec["mat"]]
                            f, wo = bsdf_sample(mat, rec, draw())
                            if not (mat.combined_type & E_SMOOTH):
                                through = (through * f).astype(np.float32)
                        go = depth < max_path_length
                        depth += 1
                        if not (go and hit and not (mat.combined_type & E_SMOOTH)):
                            break
                    L = np.zeros(3, np.float32)
                    if hit and (mat.combined_type & E_SMOOTH):
                        Le2 = le(mat, rec, d)
                        if mode == "first_non_delta_Le":
                            L = Le2
                        elif mode == "first_non_delta_f":
                            L = f
                        else:
                            L = Le2 + through * (one_light(mat, rec, draw, cnt) + f * f32(0.5))
                res[mode][i] = L
                rays[mode][i] += cnt[0]
            ok[i] = True
        except _NotRestated:
            pass
    return {m: (add_sample_clamp(res[m]).reshape(h, w, 3), int(rays[m].sum()), rays[m].reshape(h, w), last_t[m].reshape(h, w)) for m in SHADED_MODES}, ok.reshape(h, w)
