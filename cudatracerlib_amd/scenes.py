"""In-repo scene generators (no assets ship with the reference or this repo; SURVEY §8d "Synthetic inputs").

* ``cornell_box``      — C1/C2: the classic Cornell box (5 walls, 2 blocks, ceiling quad light), optional glass sphere.
* ``synthetic_sm``     — the seeded procedural stress scene that stands in for San Miguel when the asset is absent:
                          instanced icospheres / boxes in a 100^3 volume inside a room, 4 quad lights.
All builders go through DynamicScene (the loader-facing API) and return it after UpdateScene().
"""
import numpy as np
from . import api


def _quad(p, n):
    """two triangles of a quad with a given normal; vertices are not shared between quads"""
    p = np.asarray(p, np.float32)
    return p, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), np.tile(np.asarray(n, np.float32), (4, 1))


def _quad_normal(p, inward_point):
    p = np.asarray(p, np.float64)
    n = np.cross(p[1] - p[0], p[3] - p[0])
    n /= np.linalg.norm(n)
    if np.dot(np.asarray(inward_point, np.float64) - p.mean(0), n) < 0:
        n = -n
    return n


class _MeshAcc:
    def __init__(self):
        self.P, self.I, self.N, self.M = [], [], [], []
        self.nv = 0

    def add(self, P, I, N, mat):
        self.P.append(P); self.I.append(I + self.nv); self.N.append(N); self.M.append(np.full(len(I), mat, np.uint8))
        self.nv += len(P)

    def arrays(self):
        return np.concatenate(self.P), np.concatenate(self.I), np.concatenate(self.N), np.concatenate(self.M)


def icosphere(subdiv):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int64)
    for _ in range(subdiv):
        verts = list(map(tuple, v)); cache = {}; nf = []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = (np.array(verts[a]) + np.array(verts[b])) / 2.0
                verts.append(tuple(m / np.linalg.norm(m))); cache[k] = len(verts) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        v = np.array(verts, np.float64); f = np.array(nf, np.int64)
    # clockwise-outward winding: the reference's importers reverse the index order of OBJ / .serialized faces
    # (ObjParser.cpp:861-866, ObjectParser.cpp:187-188) and Mesh::ComputeVertexNormals (Mesh.cpp:151-190) expects it
    return v.astype(np.float32), np.ascontiguousarray(f[:, ::-1]).astype(np.uint32)


def unit_box():
    m = _MeshAcc()
    c = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], np.float32)
    for idx, n in (([0, 3, 2, 1], [0, 0, -1]), ([4, 5, 6, 7], [0, 0, 1]), ([0, 1, 5, 4], [0, -1, 0]), ([3, 7, 6, 2], [0, 1, 0]), ([0, 4, 7, 3], [-1, 0, 0]), ([1, 2, 6, 5], [1, 0, 0])):
        P, I, N = _quad(c[idx], n)
        m.add(P, I, N, 0)
    P, I, N, _ = m.arrays()
    return P, I, N


WHITE, RED, GREEN = (0.725, 0.71, 0.68), (0.63, 0.065, 0.05), (0.14, 0.45, 0.091)
LIGHT_RADIANCE = (17.0, 12.0, 4.0)


def cornell_box(width=256, height=256, glass_sphere=False, extra_materials=False):
    """C1 (glass_sphere=False) / C2 (glass_sphere=True).  Materials of the room mesh: 0 white, 1 red, 2 green, 3 light."""
    sc = api.DynamicScene()
    center = (278, 274, 280)
    m = _MeshAcc()
    quads = [
        ([[552.8, 0, 0], [0, 0, 0], [0, 0, 559.2], [549.6, 0, 559.2]], 0),                   # floor
        ([[556, 548.8, 0], [556, 548.8, 559.2], [0, 548.8, 559.2], [0, 548.8, 0]], 0),        # ceiling
        ([[549.6, 0, 559.2], [0, 0, 559.2], [0, 548.8, 559.2], [556, 548.8, 559.2]], 0),      # back wall
        ([[0, 0, 559.2], [0, 0, 0], [0, 548.8, 0], [0, 548.8, 559.2]], 2),                    # right wall (green)
        ([[552.8, 0, 0], [549.6, 0, 559.2], [556, 548.8, 559.2], [556, 548.8, 0]], 1),        # left wall (red)
    ]
    for p, mat in quads:
        P, I, N = _quad(p, _quad_normal(p, center))
        m.add(P, I, N, mat)
    P, I, N = _quad([[343, 548.3, 227], [343, 548.3, 332], [213, 548.3, 332], [213, 548.3, 227]], [0, -1, 0])
    m.add(P, I, N, 3)
    short = [[[130, 165, 65], [82, 165, 225], [240, 165, 272], [290, 165, 114]], [[290, 0, 114], [290, 165, 114], [240, 165, 272], [240, 0, 272]],
             [[130, 0, 65], [130, 165, 65], [290, 165, 114], [290, 0, 114]], [[82, 0, 225], [82, 165, 225], [130, 165, 65], [130, 0, 65]],
             [[240, 0, 272], [240, 165, 272], [82, 165, 225], [82, 0, 225]]]
    tall = [[[423, 330, 247], [265, 330, 296], [314, 330, 456], [472, 330, 406]], [[423, 0, 247], [423, 330, 247], [472, 330, 406], [472, 0, 406]],
            [[472, 0, 406], [472, 330, 406], [314, 330, 456], [314, 0, 456]], [[314, 0, 456], [314, 330, 456], [265, 330, 296], [265, 0, 296]],
            [[265, 0, 296], [265, 330, 296], [423, 330, 247], [423, 0, 247]]]
    for block, mat in ((short, 4 if extra_materials else 0), (tall, 5 if extra_materials else 0)):
        c = np.mean(np.asarray(block, np.float64).reshape(-1, 3), axis=0); c[1] = 80.0
        for p in block:
            n = -_quad_normal(p, c)
            P, I, N = _quad(p, n)
            m.add(P, I, N, mat)
    P, I, N, M = m.arrays()
    mats = [api.diffuse(WHITE), api.diffuse(RED), api.diffuse(GREEN), api.diffuse((0.78, 0.78, 0.78))]
    if extra_materials == 2:      # short block plastic, tall block rough glass (GGX, visible normals)
        mats += [api.plastic(diffuse_reflectance=(0.2, 0.3, 0.7), int_ior=1.49), api.roughdielectric(alpha=0.1, int_ior=1.5, ext_ior=1.0, distribution=1, sample_visible=True)]
    elif extra_materials == 3:    # short block phong, tall block thin glass
        mats += [api.phong(diffuse_reflectance=(0.5, 0.3, 0.1), specular_reflectance=(0.3, 0.3, 0.3), exponent=40.0), api.thindielectric(int_ior=1.5, ext_ior=1.0)]
    elif extra_materials == 4:    # short block nonlinear plastic, tall block Beckmann rough glass sampled from the full distribution
        mats += [api.plastic(diffuse_reflectance=(0.6, 0.2, 0.2), int_ior=1.9, nonlinear=True), api.roughdielectric(alpha=0.25, alpha_v=0.1, int_ior=1.33, ext_ior=1.0, distribution=0, sample_visible=False)]
    elif extra_materials == 5:    # short block Oren-Nayar (full model), tall block anisotropic balanced Ward; fast Oren-Nayar on the floor via variant 7
        mats += [api.roughdiffuse((0.7, 0.5, 0.2), alpha=0.4), api.ward((0.3, 0.3, 0.5), (0.05, 0.05, 0.05), alpha_u=0.08, alpha_v=0.25, variant=2)]   # (the reference's balanced variant gains energy, see tests/test_oracle_bsdf.py)
    elif extra_materials == 6:    # short block Beckmann rough plastic, tall block GGX nonlinear rough plastic (synthetic transmittance tables)
        from . import rough_tables
        for slot in (0, 1):
            tr, df, er, ar = rough_tables.make_table(slot, n_eta=4, n_alpha=5, n_theta=8, quad=16)
            sc.setRoughTransmittance(slot, tr, df, er, ar)
        mats += [api.roughplastic((0.2, 0.5, 0.25), alpha=0.15, distribution=0), api.roughplastic((0.6, 0.25, 0.2), alpha=0.3, int_ior=1.6, distribution=1, nonlinear=True)]
    elif extra_materials in (8, 9, 10):   # the nesting models: coating / roughcoating / blend over simple BSDFs registered as auxiliary materials
        add = lambda m: (sc.add_material(m), m)
        if extra_materials == 8:      # absorbing smooth coating over diffuse; blend of diffuse and GGX metal
            i0, n0 = add(api.diffuse((0.7, 0.6, 0.3)))
            i1, n1 = add(api.diffuse((0.2, 0.3, 0.6))); i2, n2 = add(api.roughconductor(alpha=0.2))
            mats += [api.coating(i0, n0, int_ior=1.5, ext_ior=1.0, thickness=2.0, sigma_a=(0.1, 0.4, 0.8)), api.blend(i1, n1, i2, n2, weight=0.35)]
        elif extra_materials == 9:    # rough coating (Beckmann table) over diffuse; blend of a delta mirror and diffuse
            from . import rough_tables
            tr, df, er, ar = rough_tables.make_table(0, n_eta=4, n_alpha=5, n_theta=8, quad=16)
            sc.setRoughTransmittance(0, tr, df, er, ar)
            i0, n0 = add(api.diffuse((0.6, 0.3, 0.2)))
            i1, n1 = add(api.conductor(eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14))); i2, n2 = add(api.diffuse((0.3, 0.6, 0.3)))
            mats += [api.roughcoating(i0, n0, alpha=0.2, int_ior=1.5, ext_ior=1.0, distribution=0), api.blend(i1, n1, i2, n2, weight=0.6)]
        else:                         # coating over a delta conductor; coating over plastic (delta + diffuse nested lobes)
            i0, n0 = add(api.conductor(eta=(0.14, 0.37, 1.44), k=(3.98, 2.38, 1.6)))
            i1, n1 = add(api.plastic(diffuse_reflectance=(0.2, 0.5, 0.3), int_ior=1.49))
            mats += [api.coating(i0, n0, int_ior=1.4, ext_ior=1.0, thickness=1.0, sigma_a=0.0), api.coating(i1, n1, int_ior=1.6, ext_ior=1.0, thickness=0.5, sigma_a=(0.3, 0.1, 0.1))]
    elif extra_materials == 11:   # short block anisotropic Beckmann metal sampled from the visible normals, tall block rough glass with the Phong distribution
        mats += [api.roughconductor(alpha=0.25, alpha_v=0.1, distribution=0, sample_visible=True), api.roughdielectric(alpha=0.2, int_ior=1.5, ext_ior=1.0, distribution=2, sample_visible=False)]
    elif extra_materials == 12:   # short block Beckmann rough glass from the visible normals, tall block Phong-distribution metal
        mats += [api.roughdielectric(alpha=0.15, int_ior=1.5, ext_ior=1.0, distribution=0, sample_visible=True), api.roughconductor(alpha=0.2, alpha_v=0.35, distribution=2, sample_visible=False)]
    elif extra_materials == 7:    # short block fast-approximation Oren-Nayar, tall block original Ward
        mats += [api.roughdiffuse((0.7, 0.5, 0.2), alpha=0.6, use_fast_approx=True), api.ward((0.2, 0.4, 0.3), (0.3, 0.3, 0.3), alpha_u=0.15, alpha_v=0.15, variant=0)]
    elif extra_materials:
        mats += [api.roughconductor(alpha=0.15, distribution=1, sample_visible=True), api.conductor(eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14))]
    room = sc.add_mesh(P, I, normals=N, tri_material=M, materials=mats)
    node = sc.CreateNode(room)
    sc.CreateLight(node, 3, LIGHT_RADIANCE)
    if glass_sphere:
        V, F = icosphere(4)
        sph = sc.add_mesh(V, F, normals=V, materials=[api.dielectric(int_ior=1.5, ext_ior=1.0)])
        r = 90.0
        xf = np.array([[r, 0, 0, 186.0], [0, r, 0, 165.0 + r + 0.5], [0, 0, r, 169.0], [0, 0, 0, 1]], np.float32)
        sc.CreateNode(sph, xf)
    sc.setCamera((278, 273, -800), (278, 273, 0), (0, 1, 0), 39.3077, width, height)
    sc.UpdateScene()
    return sc


def fog_box(width=256, height=256, sigma_a=0.0005, sigma_s=0.002, phase=None, fraction=(1.0, 1.0, 1.0), glass_sphere=False):
    """The Cornell box plus ONE homogeneous medium over the scene box (sigma_a / sigma_s: a scalar or rgb, per scene unit — the box is ~550 units wide; phase: an
    api.phase_*(), default isotropic).  fraction: the part of the scene box, from its minimum corner, that the medium fills per axis — (1, 0.5, 1) is fog over the
    lower half.  Only the PathTracer plugin renders it.  The builder is returned after UpdateScene(); .volume is the ctl_volume, .volume_index its slot."""
    sc = cornell_box(width, height, glass_sphere=glass_sphere)
    lo = np.array(sc.desc.box_min, np.float32); hi = np.array(sc.desc.box_max, np.float32)
    hi = (lo + (hi - lo) * np.asarray(fraction, np.float32)).astype(np.float32)
    sc.volume = api.homogeneous_volume(api.box_to_volume_matrix(lo, hi), sigma_a, sigma_s, phase)
    sc.volume_index = sc.CreateVolume(sc.volume)
    sc.UpdateScene()
    return sc


def smoke_density(dims, seed=7):
    """a seeded, smooth, non-constant density in [0.05, 1] on a grid of shape `dims`: a few low-frequency cosines"""
    rs = np.random.RandomState(seed)
    x, y, z = np.meshgrid(*[(np.arange(n) + 0.5) / n for n in dims], indexing="ij")
    f = np.zeros(dims, np.float64)
    for _ in range(4):
        k = rs.uniform(0.5, 2.5, 3); ph = rs.uniform(0, 2 * np.pi)
        f += np.cos(2 * np.pi * (k[0] * x + k[1] * y + k[2] * z) + ph)
    f = (f - f.min()) / max(f.max() - f.min(), 1e-30)
    return (0.05 + 0.95 * f).astype(np.float32)


def smoke_box(width=256, height=256, dims=(3, 4, 5), sigma_a=0.0005, sigma_s=0.002, phase=None, fraction=(1.0, 1.0, 1.0), seed=7, three_grid_dims=None):
    """fog_box with a heterogeneous medium: ONE VolumeGrid over the scene box whose density (smoke_density(dims, seed)) is seeded, smooth and non-constant, on a
    non-cubic grid by default.  sigma_a / sigma_s are the coefficients at density 1 (sigAMax / sigSMax; the minima are 0).  three_grid_dims = (dimsA, dimsS): the
    three-grid form with two densities of those shapes instead.  Only the PathTracer plugin renders it.  The builder is returned after UpdateScene(); .volume is the
    api.GridVolume, .volume_index its slot."""
    sc = cornell_box(width, height)
    lo = np.array(sc.desc.box_min, np.float32); hi = np.array(sc.desc.box_max, np.float32)
    hi = (lo + (hi - lo) * np.asarray(fraction, np.float32)).astype(np.float32)
    m = api.box_to_volume_matrix(lo, hi)
    if three_grid_dims is None:
        sc.volume = api.grid_volume(m, density=smoke_density(tuple(dims), seed), sig_a=(0.0, sigma_a), sig_s=(0.0, sigma_s), phase=phase)
    else:
        sc.volume = api.grid_volume(m, density_a=smoke_density(tuple(three_grid_dims[0]), seed), density_s=smoke_density(tuple(three_grid_dims[1]), seed + 1),
                                    sig_a=(0.0, sigma_a), sig_s=(0.0, sigma_s), phase=phase)
    sc.volume_index = sc.CreateGridVolume(sc.volume)
    sc.UpdateScene()
    return sc


def _rotation(rs):
    q = rs.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# ---- scene descriptions: one description, two ways into the library ------------------------------------------------------------------
# (optionally volumes: [ ctl_volume ], participating media, which build_scene creates and export_mitsuba refuses.)
# A description is a plain dict { meshes: [ {V, F, N | None, material} ], nodes: [ (mesh, 4x4 | None) ], lights: [ (node, radiance) ], camera: (pos, target, up,
# fov_deg, w, h) } with material = ("diffuse", rgb) | ("roughconductor", alpha, eta, k)  (GGX, visible-normal sampling).
# build_scene() feeds it to the builder API (DynamicScene); export_mitsuba() writes it as a Mitsuba-0.5 scene (scene.xml + meshes.serialized) that
# ctl_parse_mitsuba_scene loads — the reference's flow ParseMitsubaScene -> UpdateScene -> tracer (MitsubaLoader.cpp:11-73, main.cpp:135-180).
def _material_of(m):
    if m[0] == "diffuse":
        return api.diffuse(m[1])
    if m[0] == "roughconductor":
        return api.roughconductor(alpha=m[1], distribution=1, sample_visible=True, eta=m[2], k=m[3])
    raise ValueError("unknown material " + str(m[0]))


def build_scene(desc, sensor=None):
    """the description through the builder API -> DynamicScene (after UpdateScene).  sensor: a ctl_sensor that replaces the description's camera."""
    sc = api.DynamicScene()
    meshes = [sc.add_mesh(m["V"], m["F"], normals=m.get("N"), materials=[_material_of(m["material"])]) for m in desc["meshes"]]
    nodes = [sc.CreateNode(meshes[mi], None if xf is None else np.asarray(xf, np.float32)) for mi, xf in desc["nodes"]]
    for ni, rad in desc["lights"]:
        sc.CreateLight(nodes[ni], 0, rad)
    pos, target, up, fov, w, h = desc["camera"]
    sc.setCamera(pos, target, up, fov, w, h)
    if sensor is not None:
        sc.setSensor(sensor)
    for v in desc.get("volumes", ()):   # participating media: ctl_volume records (api.homogeneous_volume) or api.GridVolume (api.grid_volume)
        sc.CreateGridVolume(v) if isinstance(v, api.GridVolume) else sc.CreateVolume(v)
    sc.UpdateScene()
    return sc


def vertex_normals(V, F):
    """area-weighted vertex normals of an indexed mesh with the clockwise-outward winding used here (float32); gives a description explicit normals, so that
    both ways into the library see the same numbers"""
    V64 = np.asarray(V, np.float64); F = np.asarray(F, np.int64)
    fn = -np.cross(V64[F[:, 1]] - V64[F[:, 0]], V64[F[:, 2]] - V64[F[:, 0]])
    N = np.zeros_like(V64)
    for k in range(3):
        np.add.at(N, F[:, k], fn)
    N /= np.maximum(np.linalg.norm(N, axis=1, keepdims=True), 1e-30)
    return N.astype(np.float32)


def with_explicit_normals(desc):
    """the description as a scene file can carry it: every mesh with explicit normals, meshes in the order the nodes first use them, unused ones dropped
    (a loader creates a mesh when a shape first names it)"""
    order, new_nodes = [], []
    for mi, xf in desc["nodes"]:
        if mi not in order:
            order.append(mi)
        new_nodes.append((order.index(mi), xf))
    meshes = [dict(desc["meshes"][mi]) for mi in order]
    for m in meshes:
        if m.get("N") is None:
            m["N"] = vertex_normals(m["V"], m["F"])
    return dict(desc, meshes=meshes, nodes=new_nodes)


def _f32s(a):
    return " ".join("%.9g" % float(np.float32(x)) for x in np.asarray(a, np.float32).ravel())   # nine significant digits round-trip a float32


def _serialized_mesh(V, F, N):
    """one sub-mesh of a Mitsuba .serialized file, format version 4 (ObjectParser.cpp:9-204): u16 0x041C, u16 4, then a zlib stream of
    flags u32, name \\0, #vertices u64, #triangles u64, positions, normals, indices u32.  The importers reverse the index order of every face, so it is stored reversed."""
    import struct, zlib
    V = np.ascontiguousarray(V, np.float32); N = np.ascontiguousarray(N, np.float32); F = np.ascontiguousarray(np.asarray(F, np.uint32)[:, ::-1])
    body = struct.pack("<I", 0x0001 | 0x1000) + b"mesh\0" + struct.pack("<QQ", len(V), len(F)) + V.tobytes() + N.tobytes() + F.tobytes()
    return struct.pack("<HH", 0x041C, 4) + zlib.compress(body, 6)


def export_mitsuba(desc, directory, name="scene.xml"):
    """writes <directory>/<name> and <directory>/meshes.serialized; returns the path of the XML file.  Every mesh needs explicit normals (with_explicit_normals)."""
    import os, struct
    if desc.get("volumes"):
        raise ValueError("export_mitsuba: a scene with participating media is not exported")
    os.makedirs(directory, exist_ok=True)
    blobs, offsets, pos = [], [], 0
    for m in desc["meshes"]:
        if m.get("N") is None:
            raise ValueError("export_mitsuba: mesh without normals (use with_explicit_normals)")
        b = _serialized_mesh(m["V"], m["F"], m["N"]); offsets.append(pos); blobs.append(b); pos += len(b)
    with open(os.path.join(directory, "meshes.serialized"), "wb") as fh:
        for b in blobs:
            fh.write(b)
        fh.write(struct.pack("<%dQ" % len(offsets), *offsets)); fh.write(struct.pack("<I", len(offsets)))
    light_of = {ni: rad for ni, rad in desc["lights"]}
    cam_pos, target, up, fov, w, h = desc["camera"]
    x = ['<?xml version="1.0" encoding="utf-8"?>', '<scene version="0.5.0">', '  <integrator type="path"/>',
         '  <sensor type="perspective">', '    <float name="fov" value="%s"/>' % _f32s([fov]), '    <string name="fovAxis" value="x"/>',
         '    <transform name="toWorld"><lookat origin="%s" target="%s" up="%s"/></transform>' % (_f32s(cam_pos).replace(" ", ", "), _f32s(target).replace(" ", ", "), _f32s(up).replace(" ", ", ")),
         '    <film type="hdrfilm"><integer name="width" value="%d"/><integer name="height" value="%d"/></film>' % (w, h), '  </sensor>']
    for ni, (mi, xf) in enumerate(desc["nodes"]):
        mat = desc["meshes"][mi]["material"]
        x.append('  <shape type="serialized">')
        x.append('    <string name="filename" value="meshes.serialized"/><integer name="shapeIndex" value="%d"/>' % mi)
        if xf is not None:
            x.append('    <transform name="toWorld"><matrix value="%s"/></transform>' % _f32s(xf))
        if mat[0] == "diffuse":
            x.append('    <bsdf type="diffuse"><rgb name="reflectance" value="%s"/></bsdf>' % _f32s(mat[1]).replace(" ", ", "))
        else:
            x.append('    <bsdf type="roughconductor"><string name="distribution" value="ggx"/><float name="alpha" value="%s"/><float name="extEta" value="1"/>'
                     '<rgb name="eta" value="%s"/><rgb name="k" value="%s"/></bsdf>' % (_f32s([mat[1]]), _f32s(mat[2]).replace(" ", ", "), _f32s(mat[3]).replace(" ", ", ")))
        if ni in light_of:
            x.append('    <emitter type="area"><rgb name="radiance" value="%s"/></emitter>' % _f32s(light_of[ni]).replace(" ", ", "))
        x.append('  </shape>')
    x.append('</scene>')
    path = os.path.join(directory, name)
    open(path, "w").write("\n".join(x) + "\n")
    return path


def load_mitsuba(path, width=-1, height=-1):
    """ParseMitsubaScene -> UpdateScene: the DynamicScene of a Mitsuba XML file"""
    sc = api.DynamicScene()
    sc.ParseMitsubaScene(path, width, height)
    sc.UpdateScene()
    return sc


def _camera(pos, target, fov, w, h):
    """camera tuple with the up vector perpendicular to the view direction (Sensor::SetToWorld(pos, f), SceneTypes/Sensor.cu:680-686: r = f x (0,1,0), u = r x f):
    DynamicScene.setCamera takes its up vector as given, a scene loader derives it this way"""
    f = np.asarray(target, np.float64) - np.asarray(pos, np.float64); f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 1.0, 0.0]); r /= np.linalg.norm(r)
    u = np.cross(r, f); u /= np.linalg.norm(u)
    return (tuple(float(x) for x in pos), tuple(float(x) for x in target), tuple(float(np.float32(x)) for x in u), fov, w, h)


def synthetic_sm_description(width=1920, height=1080, n_instances=2000, subdiv=4, seed=42):
    """"synthetic-SM": n_instances instanced icosphere / box meshes (icosphere(4) = 5120 triangles) with seeded random
    rotations, scales and positions in a 100^3 volume inside a closed room; 4 diffuse + 2 microfacet materials; 4 quad lights."""
    rs = np.random.RandomState(seed)   # MT19937
    mats = [("diffuse", (0.7, 0.7, 0.7)), ("diffuse", (0.7, 0.25, 0.2)), ("diffuse", (0.2, 0.55, 0.25)), ("diffuse", (0.25, 0.3, 0.7)),
            ("roughconductor", 0.2, (0.2, 0.92, 1.1), (3.9, 2.45, 2.14)), ("roughconductor", 0.05, (0.14, 0.37, 1.44), (3.98, 2.38, 1.6))]
    meshes, nodes, lights = [], [], []
    V, F = icosphere(subdiv)
    base = []
    for mi in range(len(mats)):
        # a bumpy variant per material keeps the per-mesh BVHs distinct
        bump = 1.0 + 0.08 * np.sin(V[:, :1] * (3 + mi)) * np.cos(V[:, 1:2] * (5 + mi))
        base.append(len(meshes)); meshes.append(dict(V=(V * bump).astype(np.float32), F=F, N=None, material=mats[mi]))
    Pb, Ib, Nb = unit_box()
    box_meshes = []
    for i in range(4):
        box_meshes.append(len(meshes)); meshes.append(dict(V=Pb, F=Ib, N=Nb, material=mats[i]))
    for i in range(n_instances):
        pos = rs.uniform(-50, 50, size=3)
        s = rs.uniform(1.0, 3.5)
        R = _rotation(rs)
        xf = np.eye(4)
        if rs.uniform() < 0.85:
            mesh = base[rs.randint(len(base))]
            xf[:3, :3] = R * s
        else:
            mesh = box_meshes[rs.randint(len(box_meshes))]
            xf[:3, :3] = R @ np.diag(rs.uniform(0.6, 2.5, size=3) * s * 0.6)
        xf[:3, 3] = pos
        nodes.append((mesh, xf.astype(np.float32)))
    # room (inward-facing; one mesh per wall material) and 4 quad lights under the ceiling
    R0 = 70.0
    c = np.array([[-R0, -R0, -R0], [R0, -R0, -R0], [R0, R0, -R0], [-R0, R0, -R0], [-R0, -R0, R0], [R0, -R0, R0], [R0, R0, R0], [-R0, R0, R0]], np.float32)
    walls = {0: _MeshAcc(), 1: _MeshAcc(), 2: _MeshAcc()}
    for idx, n, mat in (([0, 3, 2, 1], [0, 0, 1], 0), ([4, 5, 6, 7], [0, 0, -1], 0), ([0, 1, 5, 4], [0, 1, 0], 0), ([3, 7, 6, 2], [0, -1, 0], 0), ([0, 4, 7, 3], [1, 0, 0], 1), ([1, 2, 6, 5], [-1, 0, 0], 2)):
        P, I, N = _quad(c[idx], n)
        walls[mat].add(P, I, N, 0)
    for mat, col in ((0, WHITE), (1, RED), (2, GREEN)):
        P, I, N, _ = walls[mat].arrays()
        nodes.append((len(meshes), None)); meshes.append(dict(V=P, F=I, N=N, material=("diffuse", tuple(col))))
    for lx, lz in ((-35, -35), (35, -35), (-35, 35), (35, 35)):
        P, I, N = _quad([[lx - 12, R0 - 0.5, lz - 12], [lx + 12, R0 - 0.5, lz - 12], [lx + 12, R0 - 0.5, lz + 12], [lx - 12, R0 - 0.5, lz + 12]], [0, -1, 0])
        lights.append((len(nodes), (40.0, 38.0, 34.0)))
        nodes.append((len(meshes), None)); meshes.append(dict(V=P, F=I, N=N, material=("diffuse", (0.5, 0.5, 0.5))))
    return dict(meshes=meshes, nodes=nodes, lights=lights, camera=_camera((0, 5, -68.0), (0, 0, 0), 60.0, width, height))


def synthetic_sm(width=1920, height=1080, n_instances=2000, subdiv=4, seed=42):
    return build_scene(synthetic_sm_description(width, height, n_instances, subdiv, seed))


def procedural_envmap(w=64, h=32):
    """lat-long HDR environment: sky gradient, a bright sun lobe and a dim ground, as RGBE texels (h, w) uint32"""
    y, x = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    theta, phi = y * np.pi, x * 2 * np.pi
    d = np.stack([np.sin(phi) * np.sin(theta), np.cos(theta), -np.cos(phi) * np.sin(theta)], -1)
    sky = np.where(d[..., 1:2] > 0, np.array([0.35, 0.55, 0.9]) * (0.3 + 0.7 * d[..., 1:2]) , np.array([0.12, 0.1, 0.08]))
    sun_dir = np.array([0.4, 0.75, -0.53]); sun_dir /= np.linalg.norm(sun_dir)
    c = np.clip((d * sun_dir).sum(-1, keepdims=True), 0, 1)
    rgb = sky + np.array([40.0, 34.0, 25.0]) * c ** 60
    return api.float3_to_rgbe(rgb.astype(np.float32))


def checker_image(n=16, a=(0.8, 0.8, 0.75), b=(0.15, 0.2, 0.5)):
    """n x n RGBCOL bitmap with a 4x4 checker and a per-texel gradient (so that bilinear filtering matters)"""
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    m = (((x * 4) // n + (y * 4) // n) % 2)[..., None]
    g = (0.6 + 0.4 * (x + y)[..., None] / (2 * n - 2))
    rgb = np.where(m == 0, np.asarray(a), np.asarray(b)) * g
    return api.float3_to_rgbcol(rgb.astype(np.float32))


def env_scene(width=96, height=64, rotate_env=False, point_filter=False, extra_lights=False):
    """C5-style shading stress in miniature: ground quad with a bitmap texture, glass / rough-glass / metal / plastic spheres
    and a box, lit by a lat-long environment map (+ optionally a spot, a distant and a point light)."""
    sc = api.DynamicScene()
    img = sc.add_image(checker_image(), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_POINT if point_filter else api.FILTER_BILINEAR)
    P, I, N = _quad([[-12, 0, -12], [-12, 0, 12], [12, 0, 12], [12, 0, -12]], [0, 1, 0])
    uv = np.array([[0, 0], [0, 3], [3, 3], [3, 0]], np.float32)
    ground = sc.add_mesh(P, I, normals=N, uvs=uv, materials=[api.diffuse(api.image_texture(img, scale=(0.9, 0.9, 0.9)))])
    sc.CreateNode(ground)
    V, F = icosphere(3)
    mats = [api.dielectric(int_ior=1.5, ext_ior=1.0), api.roughdielectric(alpha=0.12, int_ior=1.5, ext_ior=1.0),
            api.roughconductor(alpha=0.1), api.plastic(diffuse_reflectance=(0.7, 0.15, 0.1)), api.diffuse((0.6, 0.6, 0.6))]
    for k, m in enumerate(mats):
        mesh = sc.add_mesh(V, F, normals=V, materials=[m])
        r = 1.0 + 0.15 * k
        xf = np.array([[r, 0, 0, -6.0 + 3.0 * k], [0, r, 0, r + 0.01], [0, 0, r, 0.5 * (k % 2)], [0, 0, 0, 1]], np.float32)
        sc.CreateNode(mesh, xf)
    Pb, Ib, Nb = unit_box()
    box = sc.add_mesh(Pb, Ib, normals=Nb, materials=[api.phong((0.2, 0.5, 0.3), (0.3, 0.3, 0.3), 50.0)])
    sc.CreateNode(box, np.array([[1.2, 0, 0.5, 1.5], [0, 0.8, 0, 0.8], [-0.5, 0, 1.2, 4.0], [0, 0, 0, 1]], np.float32))
    env = sc.add_image(procedural_envmap(), api.TEXEL_RGBE, api.WRAP_REPEAT, api.FILTER_BILINEAR)
    T = None
    if rotate_env:
        a = 0.7; c, s = np.cos(a), np.sin(a)
        T = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], np.float32)
    sc.setEnvironementMap(env, (1.0, 1.0, 1.0), T)
    if extra_lights:
        sc.CreateSpotLight((0, 8, 6), (0, 0, 0), (300, 280, 250), cutoff_angle=25.0, beam_width=15.0)
        # r = 1 as the Mitsuba loader passes it (ObjectParser.h:530): the reference puts the emitter disk at +1.1 d, so only
        # points with dot(P, d) > 1.1 receive light (DistantLight::sampleDirect, Light.cu:224-245)
        sc.CreateDistantLight((-0.3, 0.8, 0.5), (1.5, 1.4, 1.2), scene_radius=1.0)
        sc.CreatePointLight((5, 3, -4), (40, 50, 60))
    sc.setCamera((0, 5, 14), (0, 1, 0), (0, 1, 0), 45.0, width, height)
    sc.UpdateScene()
    return sc


def synthetic_bathroom(width=1920, height=1080, n_instances=300, subdiv=4, seed=17, material_set="all"):
    """"synthetic-bathroom": the seeded stand-in for BASELINE config 5 (Bitterli bathroom: rough plastic / rough conductor / rough
    dielectric surfaces under an environment emitter — the shading-divergence stress).  A tiled floor with a bitmap texture and a
    height map, walls of rough plastic, n_instances spheres / boxes cycling through nine BSDF models (Beckmann and GGX, visible-normal
    sampling, rough glass, coated metal, Oren-Nayar), lit by a lat-long environment map through a window-less open top plus one area light.
    material_set (probes only, tools/shade_class_probe.py): "basic" / "single" swap every material for one of the shade kernel's model class a / class b (same geometry, lights and maps)."""
    from . import rough_tables
    rs = np.random.RandomState(seed)
    sc = api.DynamicScene()
    for slot in (0, 1):
        tr, df, er, ar = rough_tables.make_table(slot, n_eta=6, n_alpha=8, n_theta=16, quad=24)
        sc.setRoughTransmittance(slot, tr, df, er, ar)
    tiles = sc.add_image(checker_image(), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_BILINEAR)
    bumps = sc.add_image(api.float3_to_rgbcol(bump_image()), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_BILINEAR)
    floor_mat = api.roughplastic(api.image_texture(tiles, scale=(0.8, 0.8, 0.8), uv_scale=(12.0, 12.0)), alpha=0.08, distribution=0)
    if material_set == "basic":
        floor_mat = api.diffuse(api.image_texture(tiles, scale=(0.8, 0.8, 0.8), uv_scale=(12.0, 12.0)))
    api.set_height_map(floor_mat, api.image_texture(bumps, scale=(0.02, 0.02, 0.02), uv_scale=(24.0, 24.0)))
    P, I, N = _quad([[-30, 0, -30], [-30, 0, 30], [30, 0, 30], [30, 0, -30]], [0, 1, 0])
    sc.CreateNode(sc.add_mesh(P, I, normals=N, uvs=np.array([[0, 0], [0, 1], [1, 1], [1, 0]], np.float32), materials=[floor_mat]))
    wall = api.roughplastic((0.75, 0.74, 0.7), alpha=0.2, distribution=1) if material_set != "basic" else api.diffuse((0.75, 0.74, 0.7))
    m = _MeshAcc()
    for p, n in (([[-30, 0, 30], [-30, 25, 30], [30, 25, 30], [30, 0, 30]], [0, 0, -1]), ([[-30, 0, -30], [-30, 25, -30], [-30, 25, 30], [-30, 0, 30]], [1, 0, 0]),
                 ([[30, 0, 30], [30, 25, 30], [30, 25, -30], [30, 0, -30]], [-1, 0, 0])):
        Pq, Iq, Nq = _quad(p, n)
        m.add(Pq, Iq, Nq, 0)
    Pw, Iw, Nw, _ = m.arrays()
    sc.CreateNode(sc.add_mesh(Pw, Iw, normals=Nw, materials=[wall]))
    i0 = sc.add_material(api.roughconductor(alpha=0.15, distribution=1))
    n0 = api.roughconductor(alpha=0.15, distribution=1)
    mats = [api.roughplastic((0.7, 0.2, 0.15), alpha=0.1, distribution=0), api.roughplastic((0.2, 0.3, 0.7), alpha=0.3, int_ior=1.6, distribution=1, nonlinear=True),
            api.roughconductor(alpha=0.1, distribution=0, sample_visible=True), api.roughconductor(alpha=0.25, alpha_v=0.05, distribution=1, sample_visible=True, eta=(0.14, 0.37, 1.44), k=(3.98, 2.38, 1.6)),
            api.roughdielectric(alpha=0.08, int_ior=1.5, ext_ior=1.0, distribution=1, sample_visible=True), api.roughdielectric(alpha=0.2, int_ior=1.33, ext_ior=1.0, distribution=0, sample_visible=True),
            api.dielectric(int_ior=1.5, ext_ior=1.0), api.coating(i0, n0, int_ior=1.5, ext_ior=1.0, thickness=1.0, sigma_a=(0.2, 0.5, 0.9)), api.roughdiffuse((0.6, 0.6, 0.55), alpha=0.4)]
    if material_set == "basic":      # class a only: diffuse / rough conductor / smooth glass / mirror
        mats = [api.diffuse((0.7, 0.2, 0.15)), api.diffuse((0.2, 0.3, 0.7)), mats[2], mats[3], api.dielectric(int_ior=1.5, ext_ior=1.0), api.conductor(), mats[6], api.roughconductor(alpha=0.15, distribution=1), api.diffuse((0.6, 0.6, 0.55))]
    elif material_set == "single":   # class b only: rough plastic / rough dielectric / rough diffuse / plastic
        mats = [mats[0], mats[1], api.plastic((0.5, 0.5, 0.2)), mats[0], mats[4], mats[5], mats[1], mats[8], mats[8]]
    V, F = icosphere(subdiv)
    spheres = [sc.add_mesh(V, F, normals=V, materials=[mm]) for mm in mats]
    Pb, Ib, Nb = unit_box()
    boxes = [sc.add_mesh(Pb, Ib, normals=Nb, materials=[mm]) for mm in mats[:4]]
    for i in range(n_instances):
        s = rs.uniform(0.6, 2.2)
        pos = np.array([rs.uniform(-26, 26), 0.0, rs.uniform(-26, 26)])
        xf = np.eye(4)
        if rs.uniform() < 0.8:
            mesh = spheres[i % len(spheres)]; xf[:3, :3] = np.eye(3) * s; pos[1] = s + 0.02 + rs.uniform(0, 6) * (i % 3 == 0)
        else:
            mesh = boxes[i % len(boxes)]; xf[:3, :3] = _rotation(rs) @ np.diag(rs.uniform(0.5, 1.5, size=3) * s); pos[1] = 2.5 * s + 0.05
        xf[:3, 3] = pos
        sc.CreateNode(mesh, xf.astype(np.float32))
    env = sc.add_image(procedural_envmap(), api.TEXEL_RGBE, api.WRAP_REPEAT, api.FILTER_BILINEAR)
    sc.setEnvironementMap(env, (1.0, 1.0, 1.0), None)
    P, I, N = _quad([[-6, 24.5, -6], [6, 24.5, -6], [6, 24.5, 6], [-6, 24.5, 6]], [0, -1, 0])
    sc.CreateLight(sc.CreateNode(sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.5, 0.5, 0.5))])), 0, (30.0, 28.0, 25.0))
    sc.setCamera((0, 12, -29.0), (0, 3, 0), (0, 1, 0), 65.0, width, height)
    sc.UpdateScene()
    return sc


def beams_over_spheres(width=64, height=64, n_instances=40, n_beams=24, seed=5):
    """A floor, `n_instances` small icospheres and `n_beams` long thin quads that cross the room diagonally: triangles hundreds of times longer than their neighbours, whose boxes are
    mostly empty — what early split clipping (csrc/flatten.cpp) enters as several references."""
    rs = np.random.RandomState(seed)
    sc = api.DynamicScene()
    P, I, N = _quad([[-12, 0, -12], [-12, 0, 12], [12, 0, 12], [12, 0, -12]], [0, 1, 0])
    sc.CreateNode(sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.6, 0.6, 0.6))]))
    V, F = icosphere(2)
    ball = sc.add_mesh(V, F, normals=V, materials=[api.diffuse((0.7, 0.3, 0.2))])
    for _ in range(n_instances):
        xf = np.eye(4); xf[:3, :3] *= rs.uniform(0.2, 0.5); xf[:3, 3] = [rs.uniform(-10, 10), rs.uniform(0.5, 6), rs.uniform(-10, 10)]
        sc.CreateNode(ball, xf.astype(np.float32))
    m = _MeshAcc()
    for _ in range(n_beams):
        a = np.array([rs.uniform(-11, -6), rs.uniform(0.3, 7), rs.uniform(-11, 11)]); b = np.array([rs.uniform(6, 11), rs.uniform(0.3, 7), rs.uniform(-11, 11)])
        side = np.cross(b - a, rs.normal(size=3)); side *= 0.04 / np.linalg.norm(side)
        q = [a - side, a + side, b + side, b - side]
        Pq, Iq, Nq = _quad(q, _quad_normal(q, [0, 20, 0]))
        m.add(Pq, Iq, Nq, 0)
    Pb, Ib, Nb, _ = m.arrays()
    sc.CreateNode(sc.add_mesh(Pb, Ib, normals=Nb, materials=[api.diffuse((0.3, 0.3, 0.35), two_sided=True)]))
    sc.CreatePointLight((0, 9, 0), (60, 60, 60))
    sc.setCamera((0, 4, -11.5), (0, 2, 0), (0, 1, 0), 60.0, width, height)
    sc.UpdateScene()
    return sc


def bump_image(n=64, seed=3):
    """Smooth procedural height field, (n, n, 3) floats in [0, 1] (also the source of the tangent-space normal map below)."""
    y, x = np.mgrid[0:n, 0:n].astype(np.float32) / n
    h = 0.5 + 0.25 * np.sin(6.2831853 * 3 * x) * np.cos(6.2831853 * 2 * y) + 0.2 * np.sin(6.2831853 * (x + 2 * y))
    return np.repeat(np.clip(h, 0, 1)[..., None], 3, axis=2).astype(np.float32)


def normal_image(n=64, strength=0.08):
    """Tangent-space normal map (rgb = n * 0.5 + 0.5) of ``bump_image``."""
    h = bump_image(n)[..., 0]
    gx = (np.roll(h, -1, axis=1) - np.roll(h, 1, axis=1)) * 0.5 * n * strength
    gy = (np.roll(h, -1, axis=0) - np.roll(h, 1, axis=0)) * 0.5 * n * strength
    nrm = np.stack([-gx, -gy, np.ones_like(h)], axis=2)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    return (nrm * 0.5 + 0.5).astype(np.float32)


def area_lights_scene(width=96, height=64, kind="checker"):
    """A floor, two diffuse boxes and a ceiling panel whose DiffuseLight carries the members an application sets after CreateLight
    (SceneTypes/Light.h:100-101): kind "checker" / "image" = a radiance texture that needs the panel's uv, "orthogonal" = m_bOrthogonal (the panel
    lights only what lies straight below it), "orthogonal_image" = both.  A weak point light keeps the rest of the room visible."""
    sc = api.DynamicScene()
    P, I, N = _quad([[-6, 0, -6], [-6, 0, 6], [6, 0, 6], [6, 0, -6]], [0, 1, 0])
    sc.CreateNode(sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.7, 0.7, 0.7))]))
    Pb, Ib, Nb = unit_box()
    box = sc.add_mesh(Pb, Ib, normals=Nb, materials=[api.diffuse((0.7, 0.3, 0.2))])
    for pos, s in (((-2.0, 0.8, 0.5), 0.8), ((1.8, 0.5, -1.0), 0.5)):
        xf = np.eye(4, dtype=np.float32); xf[:3, :3] *= s; xf[:3, 3] = pos
        sc.CreateNode(box, xf)
    P, I, N = _quad([[-2.5, 4.0, -2.0], [2.5, 4.0, -2.0], [2.5, 4.0, 2.0], [-2.5, 4.0, 2.0]], [0, -1, 0])
    panel = sc.CreateNode(sc.add_mesh(P, I, normals=N, uvs=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), materials=[api.diffuse((0.5, 0.5, 0.5))]))
    tex = None
    if kind == "checker":
        tex = api.checker_texture((9.0, 8.0, 6.0), (0.5, 1.0, 3.0), uv_scale=(3.0, 2.0))
    elif kind in ("image", "orthogonal_image"):
        img = sc.add_image(api.float3_to_rgbe(8.0 * bump_image(16, seed=5) * np.array([1.0, 0.8, 0.5], np.float32) + 0.2), api.TEXEL_RGBE, api.WRAP_REPEAT, api.FILTER_BILINEAR)
        tex = api.image_texture(img, scale=(1.0, 1.0, 1.0), uv_scale=(1.0, 1.0))
    sc.CreateLight(panel, 0, (9.0, 8.0, 6.0), rad_texture=tex, orthogonal=kind.startswith("orthogonal"))
    sc.CreatePointLight((0.0, 2.5, -5.0), (3.0, 3.0, 3.0))
    sc.setCamera((0, 3.0, -9.0), (0, 1.5, 0), (0, 1, 0), 55.0, width, height)
    sc.UpdateScene()
    return sc


def maps_scene(width=96, height=64, surface_map="normal", alpha="luminance"):
    """Material maps in miniature: a ground quad with a normal map (``surface_map`` = "normal"), a height map ("height") or neither
    (None) under a glossy BSDF, and an upright card whose material carries an alpha map (``alpha`` = "luminance": checkerboard
    texture tested by luminance; "alpha": the alpha channel of an RGBA bitmap; "color": colour key; None: no alpha map) in front
    of a red wall, lit by an area light and a point light."""
    sc = api.DynamicScene()
    P, I, N = _quad([[-6, 0, -6], [-6, 0, 6], [6, 0, 6], [6, 0, -6]], [0, 1, 0])
    uv = np.array([[0, 0], [0, 2], [2, 2], [2, 0]], np.float32)
    ground_mat = api.roughconductor(alpha=0.25, distribution=1, sample_visible=True)
    if surface_map == "normal":
        img = sc.add_image(api.float3_to_rgbcol(normal_image()), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_BILINEAR)
        api.set_normal_map(ground_mat, api.image_texture(img))
    elif surface_map == "height":
        img = sc.add_image(api.float3_to_rgbcol(bump_image()), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_BILINEAR)
        api.set_height_map(ground_mat, api.image_texture(img, scale=(0.3, 0.3, 0.3)))
    sc.CreateNode(sc.add_mesh(P, I, normals=N, uvs=uv, materials=[ground_mat]))
    # back wall (red) and the card in front of it
    P, I, N = _quad([[-6, 0, -4], [6, 0, -4], [6, 6, -4], [-6, 6, -4]], [0, 0, 1])
    sc.CreateNode(sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.7, 0.1, 0.1))]))
    card_mat = api.diffuse((0.2, 0.6, 0.8), two_sided=True)
    if alpha == "luminance":
        api.set_alpha_map(card_mat, api.checker_texture(1.0, 0.0, uv_scale=(4.0, 3.0)), api.ALPHA_MAP_LUMINANCE, 0.5)
    elif alpha == "alpha":
        yy, xx = np.mgrid[0:32, 0:32]
        rgba = np.zeros((32, 32), np.uint32) | 0x00808080
        rgba |= np.where(((xx - 16) ** 2 + (yy - 16) ** 2) < 144, np.uint32(0xff000000), np.uint32(0x20000000))
        aimg = sc.add_image(rgba.astype(np.uint32), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_POINT)
        api.set_alpha_map(card_mat, api.image_texture(aimg, uv_scale=(2.0, 2.0)), api.ALPHA_MAP_ALPHA, 0.5)
    elif alpha == "color":
        api.set_alpha_map(card_mat, api.checker_texture((0.9, 0.1, 0.1), (0.1, 0.1, 0.9), uv_scale=(3.0, 3.0)), api.ALPHA_MAP_COLOR, 0.25, (1.0, 0.0, 0.0))
    P, I, N = _quad([[-3, 0.2, -1], [3, 0.2, -1], [3, 4.2, -1], [-3, 4.2, -1]], [0, 0, 1])
    sc.CreateNode(sc.add_mesh(P, I, normals=N, uvs=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), materials=[card_mat]))
    P, I, N = _quad([[-2, 7.5, 0], [2, 7.5, 0], [2, 7.5, 3], [-2, 7.5, 3]], [0, -1, 0])
    lm = sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.5, 0.5, 0.5))])
    sc.CreateLight(sc.CreateNode(lm), 0, (25.0, 24.0, 22.0))
    sc.CreatePointLight((0, 3, 6), (30, 30, 30))
    sc.setCamera((0, 3.5, 11), (0, 2, 0), (0, 1, 0), 45.0, width, height)
    sc.UpdateScene()
    return sc


def write_cornell_mitsuba(directory, width=256, height=256, glass_sphere=False):
    """C1 / C2 as a Mitsuba-0.5 scene (SURVEY §8d "Cornell box authored in-repo as Mitsuba XML"): <directory>/cornell.xml plus
    one OBJ per surface group under meshes/.  Geometry and materials are those of ``cornell_box``; returns the XML path."""
    import os
    os.makedirs(os.path.join(directory, "meshes"), exist_ok=True)
    center = (278, 274, 280)

    def obj(name, quads, normals_from=None, inward=True):
        lines, k = [], 0
        for p in quads:
            n = _quad_normal(p, center if normals_from is None else normals_from)
            if not inward:
                n = -n
            P = np.asarray(p, np.float64)
            # counter-clockwise as seen from the side the normal points to (the importer reverses the order)
            if np.dot(np.cross(P[1] - P[0], P[2] - P[0]), n) < 0:
                P = P[::-1]
            lines += ["v %.9g %.9g %.9g" % tuple(v) for v in P] + ["vn %.9g %.9g %.9g" % tuple(n)] * 4
            lines += ["f %d//%d %d//%d %d//%d %d//%d" % tuple(np.repeat(np.arange(k + 1, k + 5), 2))]
            k += 4
        with open(os.path.join(directory, "meshes", name + ".obj"), "w") as f:
            f.write("\n".join(lines) + "\n")
    white = [[[552.8, 0, 0], [0, 0, 0], [0, 0, 559.2], [549.6, 0, 559.2]], [[556, 548.8, 0], [556, 548.8, 559.2], [0, 548.8, 559.2], [0, 548.8, 0]],
             [[549.6, 0, 559.2], [0, 0, 559.2], [0, 548.8, 559.2], [556, 548.8, 559.2]]]
    obj("white", white)
    obj("green", [[[0, 0, 559.2], [0, 0, 0], [0, 548.8, 0], [0, 548.8, 559.2]]])
    obj("red", [[[552.8, 0, 0], [549.6, 0, 559.2], [556, 548.8, 559.2], [556, 548.8, 0]]])
    obj("light", [[[343, 548.3, 227], [343, 548.3, 332], [213, 548.3, 332], [213, 548.3, 227]]])
    short = [[[130, 165, 65], [82, 165, 225], [240, 165, 272], [290, 165, 114]], [[290, 0, 114], [290, 165, 114], [240, 165, 272], [240, 0, 272]],
             [[130, 0, 65], [130, 165, 65], [290, 165, 114], [290, 0, 114]], [[82, 0, 225], [82, 165, 225], [130, 165, 65], [130, 0, 65]],
             [[240, 0, 272], [240, 165, 272], [82, 165, 225], [82, 0, 225]]]
    tall = [[[423, 330, 247], [265, 330, 296], [314, 330, 456], [472, 330, 406]], [[423, 0, 247], [423, 330, 247], [472, 330, 406], [472, 0, 406]],
            [[472, 0, 406], [472, 330, 406], [314, 330, 456], [314, 0, 456]], [[314, 0, 456], [314, 330, 456], [265, 330, 296], [265, 0, 296]],
            [[265, 0, 296], [265, 330, 296], [423, 330, 247], [423, 0, 247]]]
    for name, block in (("short", short), ("tall", tall)):
        c = np.mean(np.asarray(block, np.float64).reshape(-1, 3), axis=0); c[1] = 80.0
        obj(name, block, normals_from=c, inward=False)
    rgb = lambda c: "%g, %g, %g" % tuple(c)
    shape = lambda name, bsdf, extra="": '  <shape type="obj"><string name="filename" value="meshes/%s.obj"/><ref id="%s"/>%s</shape>\n' % (name, bsdf, extra)
    xml = ('<?xml version="1.0" encoding="utf-8"?>\n<scene version="0.5.0">\n'
           '  <integrator type="path"><integer name="maxDepth" value="8"/></integrator>\n'
           '  <sensor type="perspective">\n    <float name="fov" value="39.3077"/>\n    <string name="fovAxis" value="x"/>\n'
           '    <transform name="toWorld"><lookat origin="278, 273, -800" target="278, 273, 0" up="0, 1, 0"/></transform>\n'
           '    <film type="hdrfilm"><integer name="width" value="%d"/><integer name="height" value="%d"/></film>\n  </sensor>\n' % (width, height))
    for name, c in (("white", WHITE), ("red", RED), ("green", GREEN), ("lamp", (0.78, 0.78, 0.78))):
        xml += '  <bsdf type="diffuse" id="%s"><rgb name="reflectance" value="%s"/></bsdf>\n' % (name, rgb(c))
    xml += shape("white", "white") + shape("red", "red") + shape("green", "green") + shape("short", "white") + shape("tall", "white")
    xml += shape("light", "lamp", '<emitter type="area"><rgb name="radiance" value="%s"/></emitter>' % rgb(LIGHT_RADIANCE))
    if glass_sphere:
        xml += ('  <shape type="sphere"><float name="radius" value="90"/><point name="center" x="186" y="255.5" z="169"/>'
                '<bsdf type="dielectric"><float name="intIOR" value="1.5"/><float name="extIOR" value="1.0"/></bsdf></shape>\n')
    xml += "</scene>\n"
    path = os.path.join(directory, "cornell.xml")
    with open(path, "w") as f:
        f.write(xml)
    return path


def write_interior_mitsuba(directory, width=128, height=72):
    """A small interior in the form the Tungsten -> Mitsuba exporter writes (the distributions BASELINE configs 3 and 5 come in): `scene version="0.5.0"`,
    a 4x4 `<matrix>` toWorld on the sensor and on every shape, `ldrfilm` + `rfilter`, a `sobol` sampler element, `twosided` wrappers with ids and `<ref id>`
    from the shapes, one OBJ per shape with v / vt / vn and `f a/b/c`, a bitmap texture with `filterType`, a `rectangle` area emitter and an `envmap` with its
    own transform.  Geometry: textured rough-plastic floor, a rough-conductor and a glass ball, a light panel, a Radiance .hdr environment.  Returns the XML path."""
    import os
    import struct
    import zlib
    os.makedirs(os.path.join(directory, "models"), exist_ok=True); os.makedirs(os.path.join(directory, "textures"), exist_ok=True)

    def obj(name, V, F, N, T):
        with open(os.path.join(directory, "models", name), "w") as f:
            f.write("# exported mesh\no %s\n" % name[:-4])
            f.writelines("v %.6f %.6f %.6f\n" % tuple(v) for v in V)
            f.writelines("vt %.6f %.6f\n" % tuple(t) for t in T)
            f.writelines("vn %.6f %.6f %.6f\n" % tuple(n) for n in N)
            f.write("s off\n")
            f.writelines("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (a + 1, a + 1, a + 1, b + 1, b + 1, b + 1, c + 1, c + 1, c + 1) for a, b, c in F)
    quad = np.array([[-1, 0, -1], [1, 0, -1], [1, 0, 1], [-1, 0, 1]], np.float64) * 5
    obj("Mesh000.obj", quad, [(0, 2, 1), (0, 3, 2)], np.array([[0, 1, 0]] * 4, np.float64), np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64))
    Vs, Fs = icosphere(2)
    Ns = Vs / np.linalg.norm(Vs, axis=1, keepdims=True)
    obj("Mesh001.obj", Vs * 0.7 + np.array([0, 0.7, 0]), Fs, Ns, np.zeros((len(Vs), 2)))
    obj("Mesh002.obj", Vs * 0.5 + np.array([1.5, 0.5, 0.5]), Fs, Ns, np.zeros((len(Vs), 2)))
    rs = np.random.RandomState(11)
    tex = (64 + rs.rand(16, 16, 3) * 160).astype(np.uint8)
    raw = b"".join(b"\x00" + tex[y].tobytes() for y in range(16))
    ch = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    with open(os.path.join(directory, "textures", "wood.png"), "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + ch(b"IHDR", struct.pack(">IIBBBBB", 16, 16, 8, 2, 0, 0, 0)) + ch(b"IDAT", zlib.compress(raw)) + ch(b"IEND", b""))
    env = (0.2 + rs.rand(8, 16, 3) * 1.5).astype(np.float32)
    m = env.max(axis=2); man, ex = np.frexp(m); scale = man * 256.0 / m
    rgbe = np.concatenate([(env * scale[..., None]).astype(np.uint8), (ex + 128).astype(np.uint8)[..., None]], axis=2)
    with open(os.path.join(directory, "textures", "envmap.hdr"), "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y 8 +X 16\n" + rgbe.tobytes())   # flat (not run-length encoded) scanlines
    ident = '<transform name="toWorld" >\n\t\t\t<matrix value="1 0 0 0 0 1 0 0 0 0 1 0 0 0 0 1"/>\n\t\t</transform>'
    xml = """<?xml version="1.0" encoding="utf-8"?>

<scene version="0.5.0" >
	<integrator type="path" >
		<integer name="maxDepth" value="65" />
		<boolean name="strictNormals" value="true" />
	</integrator>
	<sensor type="perspective" >
		<float name="fov" value="55" />
		<transform name="toWorld" >
			<matrix value="-0.999914 0.000835626 0.013058 -0.587317 -5.82126e-011 0.997959 -0.063863 2.7623 -0.0130847 -0.0638576 -0.997873 9.71429 0 0 0 1"/>
		</transform>
		<sampler type="sobol" >
			<integer name="sampleCount" value="64" />
		</sampler>
		<film type="ldrfilm" >
			<integer name="width" value="%d" />
			<integer name="height" value="%d" />
			<string name="fileFormat" value="png" />
			<string name="pixelFormat" value="rgb" />
			<float name="gamma" value="2.2" />
			<boolean name="banner" value="false" />
			<rfilter type="tent" />
		</film>
	</sensor>
	<bsdf type="twosided" id="Chrome" >
		<bsdf type="roughconductor" >
			<float name="alpha" value="0.05" />
			<string name="distribution" value="ggx" />
			<float name="extEta" value="1" />
			<rgb name="specularReflectance" value="1, 1, 1"/>
			<rgb name="eta" value="4.36968, 2.9167, 1.6547"/>
			<rgb name="k" value="5.20643, 4.23136, 3.75495"/>
		</bsdf>
	</bsdf>
	<bsdf type="twosided" id="WoodFloor" >
		<bsdf type="roughplastic" >
			<float name="alpha" value="0.1" />
			<string name="distribution" value="ggx" />
			<float name="intIOR" value="1.5" />
			<float name="extIOR" value="1" />
			<boolean name="nonlinear" value="true" />
			<texture name="diffuseReflectance" type="bitmap" >
				<string name="filename" value="textures/wood.png" />
				<string name="filterType" value="trilinear" />
			</texture>
		</bsdf>
	</bsdf>
	<bsdf type="dielectric" id="Glass" >
		<float name="intIOR" value="1.5" />
		<float name="extIOR" value="1" />
	</bsdf>
	<bsdf type="twosided" id="Panel" >
		<bsdf type="diffuse" >
			<rgb name="reflectance" value="0.578596, 0.578596, 0.578596"/>
		</bsdf>
	</bsdf>
	<shape type="obj" >
		<string name="filename" value="models/Mesh000.obj" />
		%s
		<boolean name="faceNormals" value="true" />
		<ref id="WoodFloor" />
	</shape>
	<shape type="obj" >
		<string name="filename" value="models/Mesh001.obj" />
		%s
		<ref id="Chrome" />
	</shape>
	<shape type="obj" >
		<string name="filename" value="models/Mesh002.obj" />
		%s
		<ref id="Glass" />
	</shape>
	<shape type="rectangle" >
		<transform name="toWorld" >
			<matrix value="0.5 0 0 0 0 -2.18557e-008 0.5 4 0 -0.5 -2.18557e-008 0 0 0 0 1"/>
		</transform>
		<ref id="Panel" />
		<emitter type="area" >
			<rgb name="radiance" value="17, 12, 4"/>
		</emitter>
	</shape>
	<emitter type="envmap" >
		<transform name="toWorld" >
			<matrix value="-0.922278 0 0.386527 0 0 1 0 0 -0.386527 0 -0.922278 1.17369 0 0 0 1"/>
		</transform>
		<string name="filename" value="textures/envmap.hdr" />
	</emitter>
</scene>
""" % (width, height, ident, ident, ident)
    path = os.path.join(directory, "scene.xml")
    with open(path, "w") as f:
        f.write(xml)
    return path


# ------------------------------------------------------------------------------------------------ synthetic-sm-hard
def _png_rgb(path, img):
    """8-bit RGB (h, w, 3) or grey (h, w) PNG, no filtering"""
    import struct
    import zlib
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]; ctype = 2 if img.ndim == 3 else 0
    raw = b"".join(b"\x00" + img[y].tobytes() for y in range(h))
    ch = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + ch(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) + ch(b"IDAT", zlib.compress(raw, 6)) + ch(b"IEND", b""))


def _serialized_mesh_uv(V, F, N, UV, level=1):
    """as _serialized_mesh, with texture coordinates (flag 0x0002, ObjectParser.cpp:9-204)"""
    import struct
    import zlib
    V = np.ascontiguousarray(V, np.float32); N = np.ascontiguousarray(N, np.float32); UV = np.ascontiguousarray(UV, np.float32); F = np.ascontiguousarray(np.asarray(F, np.uint32)[:, ::-1])
    body = struct.pack("<I", 0x0001 | 0x0002 | 0x1000) + b"mesh\0" + struct.pack("<QQ", len(V), len(F)) + V.tobytes() + N.tobytes() + UV.tobytes() + F.tobytes()
    return struct.pack("<HH", 0x041C, 4) + zlib.compress(body, level)


def sm_hard_height(x, z):
    """the terrain of synthetic-sm-hard: ridged multi-octave height over [-50, 50]^2 (float64 arrays in, float64 out); high octaves with amplitude above the grid spacing
    give steep sliver triangles"""
    h = np.zeros_like(x, np.float64); amp, f = 5.0, 0.045
    for k in range(9):
        h += amp * (1.0 - np.abs(np.sin(f * x * (1.0 + 0.37 * k) + 1.7 * k) * np.cos(f * z * (1.0 + 0.23 * k) + 0.9 * k + 0.3 * np.sin(0.05 * x))))
        amp *= 0.55; f *= 2.1
    return h - 6.0


def write_sm_hard_mitsuba(directory, width=1920, height=1080, nx=4096, nz=1024, tiles=(8, 4), cards=4000, beams=3000, seed=7):
    """"synthetic-sm-hard" (VERDICT r3 item 6): a second stand-in for San Miguel that is as deep and ragged as the real scene is expected to be, written as a Mitsuba-0.5 scene
    (scene.xml + meshes.serialized + textures/*.png) for the loader: nx x nz x 2 UNIQUE (non-instanced) terrain triangles in tiles[0] x tiles[1] meshes — anisotropic grid,
    ridged displacement: slivers —, `cards` alpha-masked two-sided foliage quads with bitmap textures (mask over plastic: AlphaMap_Luminance through the loader), `beams` thin
    long boxes criss-crossing the volume, eight terrain materials (diffuse and plastic over bitmaps, one rough conductor), a `sun` emitter (the loader's eight
    far-side spot lights, CTL_SUN_SEED fixed at 0) plus two area lights, all inside a closed room so that paths live their eight bounces.  Returns the XML path."""
    import os
    import struct
    os.makedirs(os.path.join(directory, "textures"), exist_ok=True)
    rs = np.random.RandomState(seed)
    # ---- textures: eight 256^2 colour noises, two leaf colour + opacity pairs, one wood
    def noise(n, base, var, freq):
        yy, xx = np.mgrid[0:n, 0:n].astype(np.float64) / n
        v = np.zeros((n, n))
        for k in range(5):
            ph = rs.uniform(0, 6.28, 4)
            v += 0.5 ** k * np.sin(2 * np.pi * freq * (k + 1) * xx + ph[0] + 2 * np.sin(2 * np.pi * (k + 1) * yy + ph[1])) * np.cos(2 * np.pi * freq * (k + 1) * yy + ph[2])
        v = (v - v.min()) / (v.max() - v.min())
        return np.clip((np.asarray(base)[None, None, :] + (v[..., None] - 0.5) * np.asarray(var)[None, None, :]) * 255, 0, 255).astype(np.uint8)
    palette = [((0.45, 0.42, 0.38), (0.5, 0.45, 0.4), 3), ((0.25, 0.45, 0.18), (0.3, 0.4, 0.2), 5), ((0.7, 0.62, 0.45), (0.3, 0.3, 0.25), 2), ((0.35, 0.25, 0.18), (0.3, 0.25, 0.2), 4),
               ((0.6, 0.6, 0.62), (0.5, 0.5, 0.5), 7), ((0.5, 0.3, 0.25), (0.4, 0.3, 0.3), 3), ((0.3, 0.35, 0.4), (0.3, 0.3, 0.4), 6), ((0.55, 0.5, 0.3), (0.4, 0.4, 0.3), 2)]
    for i, (b, v, f) in enumerate(palette):
        _png_rgb(os.path.join(directory, "textures", "ground%d.png" % i), noise(256, b, v, f))
    _png_rgb(os.path.join(directory, "textures", "wood.png"), noise(128, (0.45, 0.3, 0.18), (0.3, 0.2, 0.15), 9))
    yy, xx = np.mgrid[0:128, 0:128].astype(np.float64) / 127.0 - 0.5
    for i in range(2):
        _png_rgb(os.path.join(directory, "textures", "leaf%d.png" % i), noise(128, (0.2 + 0.1 * i, 0.5 - 0.1 * i, 0.15), (0.2, 0.3, 0.1), 4))
        ang = np.arctan2(yy, xx); rad = np.hypot(xx, yy)
        shape = rad < (0.33 + 0.12 * np.cos((5 + 2 * i) * ang)) * (0.9 + 0.1 * np.sin(31 * ang))   # a lobed leaf cluster: ~40 % of the card is opaque
        _png_rgb(os.path.join(directory, "textures", "leaf%d_alpha.png" % i), np.where(shape, 255, 0).astype(np.uint8))
    # ---- meshes
    blobs, shapes = [], []   # shapes: (material id, emitter radiance or None)
    def add(V, F, N, UV, mat, emit=None):
        blobs.append(_serialized_mesh_uv(V, F, N, UV)); shapes.append((mat, emit))
    X0, X1 = -50.0, 50.0
    gx = np.linspace(X0, X1, nx + 1); gz = np.linspace(X0, X1, nz + 1)
    tx, tz = tiles; qx, qz = nx // tx, nz // tz
    eps = 1e-3
    n_terrain = 0
    for j in range(tz):
        for i in range(tx):
            xs = gx[i * qx:(i + 1) * qx + 1]; zs = gz[j * qz:(j + 1) * qz + 1]
            Xg, Zg = np.meshgrid(xs, zs)   # (qz + 1, qx + 1)
            H = sm_hard_height(Xg, Zg)
            dhdx = (sm_hard_height(Xg + eps, Zg) - sm_hard_height(Xg - eps, Zg)) / (2 * eps); dhdz = (sm_hard_height(Xg, Zg + eps) - sm_hard_height(Xg, Zg - eps)) / (2 * eps)
            Nn = np.stack([-dhdx, np.ones_like(H), -dhdz], -1); Nn /= np.linalg.norm(Nn, axis=-1, keepdims=True)
            V = np.stack([Xg, H, Zg], -1).reshape(-1, 3); UV = np.stack([Xg * 0.1, Zg * 0.1], -1).reshape(-1, 2)
            a = (np.arange(qz)[:, None] * (qx + 1) + np.arange(qx)[None, :]).reshape(-1)
            F = np.concatenate([np.stack([a, a + qx + 1, a + 1], -1), np.stack([a + 1, a + qx + 1, a + qx + 2], -1)])   # clockwise seen from above = outward (+y), as the other scenes here
            add(V, F, Nn.reshape(-1, 3), UV, "ground%d" % ((i + 3 * j) % 8)); n_terrain += len(F)
    def quad_soup(centres, ax_u, ax_v, n_vec):
        """len(centres) quads centre +- ax_u +- ax_v as one mesh"""
        c = centres[:, None, :]; V = (c + np.array([-1, 1, 1, -1])[None, :, None] * ax_u[:, None, :] + np.array([-1, -1, 1, 1])[None, :, None] * ax_v[:, None, :]).reshape(-1, 3)
        b = 4 * np.arange(len(centres))[:, None]
        F = np.concatenate([b + np.array([0, 2, 1]), b + np.array([0, 3, 2])]).reshape(-1, 3)
        N = np.repeat(n_vec, 4, axis=0); UV = np.tile(np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), (len(centres), 1))
        return V, F, N, UV
    per = max(1, cards // 8)
    for g in range(8 if cards else 0):
        px = rs.uniform(X0 + 2, X1 - 2, per); pz = rs.uniform(X0 + 2, X1 - 2, per); size = rs.uniform(0.8, 3.0, per)
        yaw = rs.uniform(0, 2 * np.pi, per); tilt = rs.uniform(-0.4, 0.4, per)
        u = np.stack([np.cos(yaw), np.zeros(per), np.sin(yaw)], -1) * size[:, None]
        v = np.stack([-np.sin(yaw) * np.sin(tilt), np.cos(tilt), np.cos(yaw) * np.sin(tilt)], -1) * size[:, None]
        c = np.stack([px, sm_hard_height(px, pz) + size * np.cos(tilt) * rs.uniform(0.9, 2.5, per), pz], -1)
        n = np.cross(u, v); n /= np.linalg.norm(n, axis=1, keepdims=True)
        add(*quad_soup(c, u, v, n), "leaf%d" % (g % 2))
    perb = max(1, beams // 6)
    Pb, Ib, Nb = unit_box()   # 24 vertices, 12 triangles, [-1, 1]^3
    for g in range(6 if beams else 0):
        Vs, Fs, Ns, Us = [], [], [], []
        for k in range(perb):
            R = _rotation(rs); half = np.array([rs.uniform(0.02, 0.08), rs.uniform(0.02, 0.08), rs.uniform(5.0, 16.0)])
            c = np.array([rs.uniform(X0 + 5, X1 - 5), rs.uniform(2.0, 28.0), rs.uniform(X0 + 5, X1 - 5)])
            Vs.append((Pb.astype(np.float64) * half) @ R.T + c); Ns.append(Nb.astype(np.float64) @ R.T); Fs.append(np.asarray(Ib, np.int64).reshape(-1, 3) + 24 * k)
            Us.append(np.tile(np.array([[0, 0], [1, 0], [1, 8], [0, 8]], np.float32), (6, 1)))
        add(np.concatenate(Vs), np.concatenate(Fs), np.concatenate(Ns), np.concatenate(Us), "wood")
    # closed room and two light panels
    R0, Y0, Y1 = 90.0, -14.0, 78.0
    c8 = np.array([[-R0, Y0, -R0], [R0, Y0, -R0], [R0, Y1, -R0], [-R0, Y1, -R0], [-R0, Y0, R0], [R0, Y0, R0], [R0, Y1, R0], [-R0, Y1, R0]], np.float32)
    walls = _MeshAcc()
    for idx, n in (([0, 3, 2, 1], [0, 0, 1]), ([4, 5, 6, 7], [0, 0, -1]), ([0, 1, 5, 4], [0, 1, 0]), ([3, 7, 6, 2], [0, -1, 0]), ([0, 4, 7, 3], [1, 0, 0]), ([1, 2, 6, 5], [-1, 0, 0])):
        P, I, N = _quad(c8[idx], n); walls.add(P, I, N, 0)
    P, I, N, _ = walls.arrays()
    add(P, np.asarray(I).reshape(-1, 3), N, np.zeros((len(P), 2), np.float32), "wall")
    for lx in (-25.0, 25.0):
        P, I, N = _quad([[lx - 10, Y1 - 0.5, -10], [lx + 10, Y1 - 0.5, -10], [lx + 10, Y1 - 0.5, 10], [lx - 10, Y1 - 0.5, 10]], [0, -1, 0])
        add(P, np.asarray(I).reshape(-1, 3), N, np.zeros((4, 2), np.float32), "panel", emit=(60.0, 56.0, 50.0))
    offsets, pos = [], 0
    with open(os.path.join(directory, "meshes.serialized"), "wb") as fh:
        for b in blobs:
            offsets.append(pos); fh.write(b); pos += len(b)
        fh.write(struct.pack("<%dQ" % len(offsets), *offsets)); fh.write(struct.pack("<I", len(offsets)))
    # ---- XML
    tex = lambda name, f, s=1.0: '<texture name="%s" type="bitmap"><string name="filename" value="textures/%s"/><float name="uscale" value="%g"/><float name="vscale" value="%g"/></texture>' % (name, f, s, s)
    bsdfs = []
    for i in range(8):
        if i in (2, 5):
            bsdfs.append('<bsdf type="plastic" id="ground%d"><float name="intIOR" value="%g"/>%s</bsdf>' % (i, 1.45 + 0.05 * i, tex("diffuseReflectance", "ground%d.png" % i)))   # (rough plastic would need Mitsuba's transmittance tables installed next to the scene file)
        elif i == 6:
            bsdfs.append('<bsdf type="roughconductor" id="ground6"><string name="distribution" value="ggx"/><float name="alpha" value="0.25"/><float name="extEta" value="1"/><rgb name="eta" value="0.2, 0.92, 1.1"/><rgb name="k" value="3.9, 2.45, 2.14"/></bsdf>')
        else:
            bsdfs.append('<bsdf type="diffuse" id="ground%d">%s</bsdf>' % (i, tex("reflectance", "ground%d.png" % i)))
    for i in range(2):
        bsdfs.append('<bsdf type="twosided" id="leaf%d"><bsdf type="mask">%s<bsdf type="plastic"><float name="intIOR" value="1.4"/>%s</bsdf></bsdf></bsdf>'
                     % (i, tex("opacity", "leaf%d_alpha.png" % i), tex("diffuseReflectance", "leaf%d.png" % i)))
    bsdfs.append('<bsdf type="diffuse" id="wood">%s</bsdf>' % tex("reflectance", "wood.png"))
    bsdfs.append('<bsdf type="diffuse" id="wall"><rgb name="reflectance" value="0.55, 0.6, 0.7"/></bsdf>')
    bsdfs.append('<bsdf type="diffuse" id="panel"><rgb name="reflectance" value="0.5, 0.5, 0.5"/></bsdf>')
    cam = _camera((0.0, float(sm_hard_height(np.array(0.0), np.array(-46.0))) + 7.0, -46.0), (0.0, 2.0, 10.0), 60.0, width, height)
    x = ['<?xml version="1.0" encoding="utf-8"?>', '<scene version="0.5.0">', '  <integrator type="path"/>',
         '  <sensor type="perspective">', '    <float name="fov" value="%s"/>' % _f32s([cam[3]]), '    <string name="fovAxis" value="x"/>',
         '    <transform name="toWorld"><lookat origin="%s" target="%s" up="%s"/></transform>' % (_f32s(cam[0]).replace(" ", ", "), _f32s(cam[1]).replace(" ", ", "), _f32s(cam[2]).replace(" ", ", ")),
         '    <film type="hdrfilm"><integer name="width" value="%d"/><integer name="height" value="%d"/></film>' % (width, height), '  </sensor>']
    x += ["  " + b for b in bsdfs]
    for si, (mat, emit) in enumerate(shapes):
        if mat == "wall":
            # The reference turns `sun` into eight 90-degree spot lights at centre - d R / 2 for the direction d TOWARDS the sun (ObjectParser.h:476-491), R = the diagonal of
            # what has been loaded SO FAR: placed here — after the terrain, the cards and the beams, before the room — and with d pointing down, they stand ~70 units above
            # the terrain's centre, inside the room, and light it
            x.append('  <emitter type="sun"><vector name="sunDirection" x="0.35" y="-0.8" z="-0.45"/><float name="scale" value="2"/></emitter>')
        x.append('  <shape type="serialized"><string name="filename" value="meshes.serialized"/><integer name="shapeIndex" value="%d"/><ref id="%s"/>%s</shape>'
                 % (si, mat, ('<emitter type="area"><rgb name="radiance" value="%s"/></emitter>' % _f32s(emit).replace(" ", ", ")) if emit else ""))
    x.append('</scene>')
    path = os.path.join(directory, "scene.xml")
    open(path, "w").write("\n".join(x) + "\n")
    return path


def synthetic_sm_hard(directory, width=1920, height=1080, **kw):
    """the DynamicScene of synthetic-sm-hard through the loader (the scene files are written into `directory` unless they are there already)"""
    import os
    xml = os.path.join(directory, "scene.xml")
    if not os.path.exists(xml):
        write_sm_hard_mitsuba(directory, width, height, **kw)
    return load_mitsuba(xml, width, height)


def fuzz_scene(seed, width=48, height=32):
    """A seeded RANDOM scene for the parity fuzz tests (tests/test_gpu_fuzz.py, tests/test_oracle_fuzz.py): a floor (bitmap, checker or plain) and up to two walls, 8-20 instances
    of spheres / boxes under random affine transforms — rotation x non-uniform scale, one in four MIRRORED (negative determinant), one in five sheared —, materials drawn from all
    fourteen BSDF models with random parameters (both microfacet distributions, visible-normal sampling on and off, anisotropy, nested models under coatings and blends, textures
    in every slot that takes one, a normal or height map now and then), and one to three emitters of the five kinds (area with constant / checker radiance, point, spot,
    distant, environment map plain or rotated).  Everything comes from RandomState(seed): the same seed is the same scene on every box."""
    from . import rough_tables
    rs = np.random.RandomState(1000 + seed)
    sc = api.DynamicScene()
    for slot in (0, 1):
        tr, df, er, ar = rough_tables.make_table(slot, n_eta=4, n_alpha=4, n_theta=8, quad=12)
        sc.setRoughTransmittance(slot, tr, df, er, ar)
    tiles = sc.add_image(checker_image(), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_BILINEAR if seed % 2 else api.FILTER_POINT)
    bumps = sc.add_image(api.float3_to_rgbcol(bump_image(32, seed=seed)), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_BILINEAR)
    nmap = sc.add_image(api.float3_to_rgbcol(normal_image(32)), api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_BILINEAR)

    def colour(lo=0.05, hi=0.9):
        return tuple(float(x) for x in rs.uniform(lo, hi, size=3))

    def texture():
        k = rs.randint(4)
        if k == 0:
            return api.image_texture(tiles, scale=colour(0.4, 1.0), uv_scale=(float(rs.choice([1.0, 2.0, 5.0])),) * 2)
        if k == 1:
            return api.checker_texture(colour(), colour(), uv_scale=(float(rs.choice([2.0, 4.0])), float(rs.choice([2.0, 3.0]))))
        return colour()

    def simple(kind=None):
        kind = rs.randint(11) if kind is None else kind
        a = float(rs.uniform(0.03, 0.5)); dist = int(rs.randint(2)); vis = bool(rs.randint(2))
        if kind == 0: return api.diffuse(texture(), two_sided=bool(rs.randint(2)))
        if kind == 1: return api.roughdiffuse(texture(), alpha=a, use_fast_approx=bool(rs.randint(2)))
        if kind == 2: return api.dielectric(int_ior=float(rs.uniform(1.2, 1.8)), ext_ior=1.0)
        if kind == 3: return api.thindielectric(int_ior=float(rs.uniform(1.2, 1.8)), ext_ior=1.0)
        if kind == 4: return api.roughdielectric(alpha=a, int_ior=float(rs.uniform(1.2, 1.8)), ext_ior=1.0, distribution=dist, sample_visible=vis, alpha_v=(float(rs.uniform(0.03, 0.5)) if rs.randint(3) == 0 else None))
        if kind == 5: return api.conductor(eta=colour(0.1, 1.5), k=colour(1.5, 4.0))
        if kind == 6: return api.roughconductor(alpha=a, eta=colour(0.1, 1.5), k=colour(1.5, 4.0), distribution=dist, sample_visible=vis, alpha_v=(float(rs.uniform(0.03, 0.5)) if rs.randint(3) == 0 else None))
        if kind == 7: return api.plastic(texture(), int_ior=float(rs.uniform(1.3, 1.7)), ext_ior=1.0, nonlinear=bool(rs.randint(2)))
        if kind == 8: return api.roughplastic(texture(), alpha=a, int_ior=float(rs.uniform(1.3, 1.7)), ext_ior=1.0, distribution=dist, nonlinear=bool(rs.randint(2)))
        if kind == 9: return api.phong(colour(0.1, 0.6), colour(0.05, 0.35), exponent=float(rs.uniform(5, 120)))
        return api.ward(colour(0.1, 0.6), colour(0.05, 0.35), alpha_u=float(rs.uniform(0.05, 0.4)), alpha_v=float(rs.uniform(0.05, 0.4)), variant=int(rs.randint(3)))

    def material():
        k = rs.randint(14)
        if k < 11:
            m = simple(k)
        elif k == 11:
            n = simple(int(rs.choice([0, 6, 9]))); m = api.coating(sc.add_material(n), n, int_ior=1.5, ext_ior=1.0, thickness=float(rs.uniform(0.2, 2.0)), sigma_a=colour(0.0, 1.0))
        elif k == 12:
            n = simple(int(rs.choice([0, 6, 1]))); m = api.roughcoating(sc.add_material(n), n, alpha=float(rs.uniform(0.05, 0.3)), int_ior=1.5, ext_ior=1.0, thickness=float(rs.uniform(0.2, 2.0)), sigma_a=colour(0.0, 1.0), distribution=int(rs.randint(2)))
        else:
            n0, n1 = simple(int(rs.choice([0, 7, 9]))), simple(int(rs.choice([5, 6, 10]))); m = api.blend(sc.add_material(n0), n0, sc.add_material(n1), n1, weight=float(rs.uniform(0.2, 0.8)))
        r = rs.randint(8)
        if r == 0 and k not in (2, 3): api.set_normal_map(m, api.image_texture(nmap, uv_scale=(3.0, 3.0)))
        elif r == 1 and k not in (2, 3): api.set_height_map(m, api.image_texture(bumps, scale=(0.05, 0.05, 0.05), uv_scale=(2.0, 2.0)))
        return m

    P, I, N = _quad([[-10, 0, -10], [-10, 0, 10], [10, 0, 10], [10, 0, -10]], [0, 1, 0])
    sc.CreateNode(sc.add_mesh(P, I, normals=N, uvs=np.array([[0, 0], [0, 4], [4, 4], [4, 0]], np.float32), materials=[simple(int(rs.choice([0, 1, 7, 8])))]))
    for p, n in ((([-10, 0, -10], [10, 0, -10], [10, 9, -10], [-10, 9, -10]), [0, 0, 1]), (([-10, 0, 10], [-10, 0, -10], [-10, 9, -10], [-10, 9, 10]), [1, 0, 0]))[:rs.randint(3)]:
        Pq, Iq, Nq = _quad([list(x) for x in p], n)
        sc.CreateNode(sc.add_mesh(Pq, Iq, normals=Nq, uvs=np.array([[0, 0], [2, 0], [2, 1], [0, 1]], np.float32), materials=[simple(int(rs.choice([0, 1, 9])))]))
    V, F = icosphere(2)
    uv_s = np.stack([np.arctan2(V[:, 2], V[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(V[:, 1], -1, 1)) / np.pi], axis=1).astype(np.float32)
    Pb, Ib, Nb = unit_box()
    uv_b = (Pb[:, [0, 2]] * 0.5 + 0.5).astype(np.float32)
    for i in range(rs.randint(8, 21)):
        m = material()
        mesh = sc.add_mesh(V, F, normals=V, uvs=uv_s, materials=[m]) if rs.randint(3) else sc.add_mesh(Pb, Ib, normals=Nb, uvs=uv_b, materials=[m])
        A = _rotation(rs) @ np.diag(rs.uniform(0.5, 1.6, size=3))
        if rs.randint(4) == 0: A = A @ np.diag([1.0, 1.0, -1.0])           # mirrored instance
        if rs.randint(5) == 0: A = A @ np.array([[1, 0.4, 0], [0, 1, 0], [0, 0.3, 1.0]])   # sheared instance
        xf = np.eye(4); xf[:3, :3] = A; xf[:3, 3] = [rs.uniform(-7, 7), rs.uniform(0.8, 4.5), rs.uniform(-7, 6)]
        sc.CreateNode(mesh, xf.astype(np.float32))
    kinds = list(rs.choice(5, size=rs.randint(1, 4), replace=False))
    for k in kinds:
        if k == 0:
            P, I, N = _quad([[-2.5, 8.9, -2], [2.5, 8.9, -2], [2.5, 8.9, 2], [-2.5, 8.9, 2]], [0, -1, 0])
            lm = sc.add_mesh(P, I, normals=N, uvs=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), materials=[api.diffuse((0.5, 0.5, 0.5))])
            rt = api.checker_texture((1.0, 0.9, 0.8), (0.2, 0.3, 0.9), uv_scale=(3.0, 2.0)) if rs.randint(2) else None
            sc.CreateLight(sc.CreateNode(lm), 0, tuple(float(x) for x in rs.uniform(10, 40, size=3)), rad_texture=rt)
        elif k == 1:
            sc.CreatePointLight((float(rs.uniform(-5, 5)), float(rs.uniform(3, 8)), float(rs.uniform(-5, 5))), tuple(float(x) for x in rs.uniform(30, 120, size=3)))
        elif k == 2:
            sc.CreateSpotLight((float(rs.uniform(-6, 6)), 8.0, float(rs.uniform(-3, 8))), (float(rs.uniform(-2, 2)), 0.0, float(rs.uniform(-2, 2))), tuple(float(x) for x in rs.uniform(200, 500, size=3)),
                               cutoff_angle=float(rs.uniform(15, 40)), beam_width=float(rs.uniform(5, 14)))
        elif k == 3:
            d = rs.normal(size=3); d[1] = abs(d[1]) + 0.5; d /= np.linalg.norm(d)
            sc.CreateDistantLight(tuple(float(x) for x in d), tuple(float(x) for x in rs.uniform(0.8, 2.5, size=3)), scene_radius=1.0)
        else:
            env = sc.add_image(procedural_envmap(), api.TEXEL_RGBE, api.WRAP_REPEAT, api.FILTER_BILINEAR)
            T = None
            if rs.randint(2):
                a = float(rs.uniform(0, 6.28)); c, s = np.cos(a), np.sin(a)
                T = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]], np.float32)
            sc.setEnvironementMap(env, (1.0, 1.0, 1.0), T)
    sc.setCamera((float(rs.uniform(-3, 3)), float(rs.uniform(3, 7)), float(rs.uniform(11, 15))), (0.0, 2.0, 0.0), (0, 1, 0), float(rs.uniform(40, 65)), width, height)
    sc.UpdateScene()
    return sc


def coating_from_behind(width=32, height=24, env=True):
    """A one-sided rough coating seen from BEHIND under an environment map: the reference's roughcoating::sample has no side check before its microfacet sample
    (SceneTypes/BSDF_Complex.cu:159-223) and returns NaN there when the specular lobe is chosen; the sample's radiance becomes NaN and Image::AddSample drops it (Engine/Image.cu:25-28) — the
    panel's pixels receive fewer samples than passes.  tests/test_oracle_fuzz.py and tests/test_gpu_fuzz.py hold oracle and kernels to that."""
    from . import rough_tables
    sc = api.DynamicScene()
    for slot in (0, 1):
        tr, df, er, ar = rough_tables.make_table(slot, n_eta=4, n_alpha=4, n_theta=8, quad=12)
        sc.setRoughTransmittance(slot, tr, df, er, ar)
    inner = api.diffuse((0.6, 0.3, 0.2))
    m = api.roughcoating(sc.add_material(inner), inner, alpha=0.2, int_ior=1.5, ext_ior=1.0, thickness=1.0, sigma_a=(0.1, 0.2, 0.3), distribution=0)
    P, I, N = _quad([[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], [0, 0, -1])      # faces -z; the camera sits at +z
    sc.CreateNode(sc.add_mesh(P, I, normals=N, uvs=np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32), materials=[m]))
    P, I, N = _quad([[-8, -3, -8], [-8, -3, 8], [8, -3, 8], [8, -3, -8]], [0, 1, 0])
    sc.CreateNode(sc.add_mesh(P, I, normals=N, materials=[api.diffuse((0.5, 0.5, 0.5))]))
    if env:
        e = sc.add_image(procedural_envmap(), api.TEXEL_RGBE, api.WRAP_REPEAT, api.FILTER_BILINEAR)
        sc.setEnvironementMap(e, (1.0, 1.0, 1.0), None)
    else:
        sc.CreatePointLight((0, 4, 6), (60, 60, 60))
    sc.setCamera((0, 0, 9), (0, 0, 0), (0, 1, 0), 40.0, width, height)
    sc.UpdateScene()
    return sc
