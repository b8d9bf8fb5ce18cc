"""Skinned meshes, the host half: ctl_skin_mesh_host — the yardstick of ctl_scene_animate_mesh, the functions of csrc/mesh_skin.h on the host — against a float32
numpy restatement of the reference's formulas (Engine/AnimatedMesh.cu g_ComputeVertices, Math/float4x4.h, Math/MathFunc.h, Math/Vector.h) bit for bit, and its
TriangleData and Woop rows against DynamicScene.UpdateMesh of the same vertices; the argument checks; the exported symbols.  Cases K1..K5: tests/skin_cases.py.
No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from cudatracerlib_amd import api
from scene_deform_cases import mesh_arrays
from skin_cases import CASES, make_case, yardstick, host_updated, same_bits, without_codes, code_steps, normal_codes

f32 = np.float32
_cache = {}


def case_of(name):
    if name not in _cache:
        K = make_case(name)
        _cache[name] = (K, yardstick(K))
    return _cache[name]


def skin_numpy(P, N, BI, BW, B0, B1, lerp):
    """g_ComputeVertices in float32, operation by operation (NumPy's float32 arithmetic does not contract):
      d_Compute           mat = 0; for i in 0..7: mat = mat + M[idx_i] * (byte_i / 255.0f)                       (AnimatedMesh.cu:13-28, float4x4.h:347-354,384-396)
      float4x4 * Vec4f    dot(row, v): r = 0; r += row[k] * v[k]                                                   (float4x4.h:374-382, Vector.h:97)
      TransformPoint      (M * (p, 1)).xyz / .w; TransformDirection (M * (d, 0)).xyz                              (float4x4.h:398-408)
      math::lerp          a * (1 - t) + b * t                                                                      (MathFunc.h:161)
      normalize           v * rcp(length(v)), rcp(a) = a ? 1 / a : 0, lenSqr from 0                                (Vector.h:46,369-376, MathFunc.h:399)"""
    n = len(P)
    B0 = B0.reshape(-1, 16); B1 = B0 if B1 is None else B1.reshape(-1, 16)

    def blend(B):
        mat = np.zeros((n, 16), f32)
        for i in range(8):
            w = BW[:, i].astype(np.int32).astype(f32) / f32(255.0)
            mat = mat + B[BI[:, i]] * w[:, None]
        return mat

    def row_dot(mat, r, v, w):
        acc = np.zeros(n, f32)
        for k in range(3):
            acc = acc + mat[:, 4 * r + k] * v[:, k]
        return acc + mat[:, 4 * r + 3] * f32(w)

    def point(mat, p):
        w = row_dot(mat, 3, p, 1.0)
        return np.stack([row_dot(mat, r, p, 1.0) / w for r in range(3)], axis=1)

    def direction(mat, d):
        return np.stack([row_dot(mat, r, d, 0.0) for r in range(3)], axis=1)

    def lerp3(a, b, t):
        t = f32(t); s = f32(1.0) - t
        return a * s + b * t

    with np.errstate(all="ignore"):
        m0, m1 = blend(B0), blend(B1)
        pos = lerp3(point(m0, P), point(m1, P), lerp)
        v = lerp3(direction(m0, N), direction(m1, N), lerp)
        l2 = np.zeros(n, f32)
        for k in range(3):
            l2 = l2 + v[:, k] * v[:, k]
        l = np.sqrt(l2)
        r = np.where(l != 0, f32(1.0) / l, f32(0.0)).astype(f32)
        nor = v * r[:, None]
    assert pos.dtype == f32 and nor.dtype == f32
    return pos, nor


def vertex_normals_numpy(P, I):
    """Mesh::ComputeVertexNormals (Engine/Mesh.cpp:151-190) in float32, face by face in order: N[i] += cross(a - p, b - p) / (|a - p|^2 |b - p|^2) at every corner,
    then N * (1 / |N|)"""
    I = np.arange(len(P)).reshape(-1, 3) if I is None else I
    N = np.zeros((len(P), 3), f32)

    def len_sqr(v):
        r = v[0] * v[0]; r = r + v[1] * v[1]; r = r + v[2] * v[2]
        return r

    def nor(pb, n1, n2):
        a, v = n1 - pb, n2 - pb
        c = np.array([a[1] * v[2] - a[2] * v[1], a[2] * v[0] - a[0] * v[2], a[0] * v[1] - a[1] * v[0]], f32)
        return c / (len_sqr(a) * len_sqr(v))
    with np.errstate(all="ignore"):
        for i1, i2, i3 in I:
            v1, v2, v3 = P[i1], P[i2], P[i3]
            N[i1] = N[i1] + nor(v1, v3, v2); N[i2] = N[i2] + nor(v2, v1, v3); N[i3] = N[i3] + nor(v3, v2, v1)
        l2 = N[:, 0] * N[:, 0]; l2 = l2 + N[:, 1] * N[:, 1]; l2 = l2 + N[:, 2] * N[:, 2]
        N = N * (f32(1.0) / np.sqrt(l2))[:, None]
    assert N.dtype == f32
    return N


@pytest.mark.parametrize("name", CASES)
def test_yardstick_vertices_equal_the_numpy_restatement(name):
    K, Y = case_of(name)
    N = K["N"]
    if N is None:
        N = vertex_normals_numpy(K["P"], K["I"])          # K1, K5: what a bind without normals computes, once
    pos, nor = skin_numpy(K["P"], N, K["BI"], K["BW"], K["B0"], K["B1"], K["lerp"])
    assert same_bits(pos, Y["positions"]), "positions: %d of %d words differ" % ((pos.view(np.uint32) != Y["positions"].view(np.uint32)).sum(), pos.size)
    assert same_bits(nor, Y["normals"]), "normals: %d of %d words differ" % ((nor.view(np.uint32) != Y["normals"].view(np.uint32)).sum(), nor.size)
    assert not np.array_equal(pos, K["P"])
    if name == "K4":
        assert (np.linalg.norm(nor, axis=1) == 0).sum() > 10          # the zero-scale bone: rcp(0) = 0, not a NaN
    else:
        assert np.abs(np.linalg.norm(nor.astype(np.float64), axis=1) - 1).max() < 1e-5


@pytest.mark.parametrize("name", CASES)
def test_yardstick_triangles_and_woop_rows_equal_update_mesh(name):
    """UpdateMesh is given the yardstick's positions and normals.  Every word equal, a NaN for a NaN, except the 16-bit normal codes: the yardstick encodes with the
    kernels' fm::acos / fm::atan2, UpdateMesh with glibc's, and the two may straddle a code step — one step in theta or in phi (phi modulo 255), in at most 1 of
    1000 codes.  The cap is a condition on the poses, not a measurement."""
    K, Y = case_of(name)
    bent = host_updated(K, Y)
    A = mesh_arrays(bent.desc, K["mesh"])
    assert same_bits(Y["woop"], A["woop"]), "Woop rows"
    assert np.array_equal(without_codes(Y["tri"]), without_codes(A["tri"])), "TriangleData outside the normal codes"
    differ, far = code_steps(Y["tri"], A["tri"])
    total = normal_codes(Y["tri"]).size
    print("%s: %d of %d normal codes differ between fm:: and glibc, %d by more than one step; arrays byte-equal: %s" % (name, differ, total, far, differ == 0))
    assert far == 0 and differ * 1000 <= total
    rest = mesh_arrays(K["plain"].desc, K["mesh"])
    assert not np.array_equal(rest["woop"], Y["woop"]) and not np.array_equal(rest["tri"], Y["tri"])
    assert np.array_equal(rest["tri"][:, 5:], Y["tri"][:, 5:]) and np.array_equal(rest["tri"][:, 1] >> 16, Y["tri"][:, 1] >> 16)      # uv words and material byte stay
    if name == "K6":           # duplicated references: every row of a triangle holds that triangle's rows
        widx = mesh_arrays(K["plain"].desc, K["mesh"])["widx"] >> 1
        assert len(widx) > K["n_tri"]
        first = {}
        for j, t in enumerate(widx):
            first.setdefault(int(t), j)
        assert all(np.array_equal(Y["woop"][j], Y["woop"][first[int(t)]]) for j, t in enumerate(widx))
    if name == "K4":
        assert (~np.isfinite(Y["woop"].view(np.float32))).any(axis=1).sum() > 10, "the collapsed cap has singular Woop rows"


def _call_host(K, **over):
    a = dict(mesh=K["mesh"], P=K["P"], I=K["I"], BI=K["BI"], BW=K["BW"], n_bones=K["n_bones"], B0=K["B0"], B1=K["B1"], lerp=K["lerp"]); a.update(over)
    return api.skin_mesh_host(K["plain"].desc, a["mesh"], a["P"], a["I"], a["BI"], a["BW"], a["n_bones"], a["B0"], a["B1"], a["lerp"], rest_normals=K["N"], n_rows=K["n_rows"])


def test_refusals_leave_the_arguments_untouched():
    K, _ = case_of("K1")
    keep = {k: K[k].copy() for k in ("P", "I", "BI", "BW", "B0", "B1")}
    bad_index = K["I"].copy(); bad_index[7, 1] = len(K["P"])
    bad_bone = K["BI"].copy(); bad_bone[5, 6] = K["n_bones"]; assert K["BW"][5, 6] == 0        # under a zero weight too
    nan_bone = K["B0"].copy(); nan_bone[1, 2, 3] = np.nan
    inf_bone = K["B1"].copy(); inf_bone[2, 0, 0] = np.inf
    for what, over in (("a bad mesh index", dict(mesh=K["plain"].desc.n_meshes)), ("another triangle count", dict(I=K["I"][:-1])), ("a vertex index out of range", dict(I=bad_index)),
                       ("an index byte >= n_bones", dict(BI=bad_bone)), ("a matrix entry that is not finite", dict(B0=nan_bone)), ("a matrix entry that is not finite", dict(B1=inf_bone)),
                       ("a lerp that is not finite", dict(lerp=float("nan"))), ("a lerp that is not finite", dict(lerp=float("inf")))):
        with pytest.raises(api.CtlError) as e:
            _call_host(K, **over)
        assert e.value.code == api.ERR_INVALID, what
    # n_bones of 0 and above 256 (the Python wrapper checks the matrix count against n_bones: call the library directly)
    P, BI, BW, I = K["P"], K["BI"], K["BW"], np.ascontiguousarray(K["I"], np.uint32)
    for n_bones in (0, 257):
        B = np.zeros((max(n_bones, 1), 16), f32)
        code = api.lib.ctl_skin_mesh_host(C.addressof(K["plain"].desc), K["mesh"], P.ctypes.data, None, len(P), I.ctypes.data, len(I), BI.ctypes.data, BW.ctypes.data, n_bones, B.ctypes.data, None, 0.0,
                                          None, None, None, None)
        assert code == api.ERR_INVALID, n_bones
    for k, v in keep.items():
        assert np.array_equal(K[k], v, equal_nan=True), k
    again = _call_host(K)
    assert all(same_bits(again[k], case_of("K1")[1][k]) for k in ("positions", "normals", "tri", "woop"))


def test_the_new_symbols_are_exported():
    for name in ("ctl_scene_bind_skin", "ctl_scene_animate_mesh", "ctl_scene_get_skin_ms", "ctl_scene_read_mesh_geometry", "ctl_scene_unbind_skin", "ctl_skin_mesh_host"):
        assert getattr(api.lib, name) is not None
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctl_amd.h")).read()
    for name in ("ctl_scene_bind_skin", "ctl_scene_animate_mesh", "ctl_scene_read_mesh_geometry", "ctl_scene_unbind_skin", "ctl_skin_mesh_host", "ctl_scene_get_skin_ms"):
        assert "int %s(" % name in header


def test_the_device_calls_answer_no_device_first():
    """without a device every scene call reports CTL_ERR_NO_DEVICE before it looks at its arguments (a null scene among them); with one, a null scene is invalid"""
    want = api.ERR_NO_DEVICE if api.device_count() < 1 else api.ERR_INVALID
    assert api.lib.ctl_scene_bind_skin(None, 0, None, None, 0, None, 0, None, None, 0) == want
    assert api.lib.ctl_scene_animate_mesh(None, 0, None, None, 0.0, None) == want
    assert api.lib.ctl_scene_read_mesh_geometry(None, 0, None, None, None, None) == want
    assert api.lib.ctl_scene_unbind_skin(None, 0) == want


def test_desc_diff_reports_a_host_updated_pose_as_geometry():
    """the description the frame tests compare against — UpdateMesh of the yardstick's vertices — differs from the rest pose in DIFF_GEOMETRY and not in topology: it is
    the update a host without ctl_scene_animate_mesh runs.  (The per-mesh ignore mask of a bound mesh has no host-only entry point: ctl_scene_desc_diff takes none, the
    scene builds its own; tests/test_gpu_skin.py::test_a_bound_mesh_is_device_owned holds it.)"""
    K, Y = case_of("K2")
    bent = host_updated(K, Y)
    mask = api.scene_desc_diff(K["plain"].desc, bent.desc)           # (the mesh box changed, and with it the scene BVH: DIFF_TRANSFORMS comes along)
    assert mask & api.DIFF_GEOMETRY and not mask & api.DIFF_TOPOLOGY
