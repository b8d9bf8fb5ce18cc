#!/usr/bin/env python3
"""Cost of ctl_scene_update against re-creating the scene, and the traversal rate of a refitted tree against a freshly built one.

    python tools/scene_update_bench.py [--workloads synthetic-sm,synthetic-sm-hard] [--hard-scale full|small] [--passes 4] [--out profiles/scene_update.jsonl] [--results RESULTS.md]

Per workload, on one GPU, in one process:
  1. ctl_scene_update for a camera change, a material change (a reflectance; and one that changes a bsdf_type, which re-stamps the leaf entries) and a one-node
     transform change: wall time around the (synchronous) call, median of 10, and the HIP-event time of the refit kernels alone;
  2. what a host without ctl_scene_update pays for the same transform change: ctl_builder_finalize + ctl_scene_create_ex, once with the geometry cache disabled and
     once with the cache warm for the NEW transforms (its best case);
  3. Mrays/s of the WavefrontPathTracer (depth 8) on the refitted tree against a freshly built tree of the same description, for three motions of one node
     (M1 small move, M2 rotation + non-uniform scale, M3 a move across a third of the scene), next to the surface-area ratio ctl_scene_get_update_stats reports.
  4. a one-mesh deformation (DynamicScene.UpdateMesh: a ripple along the normals, 4 % of the mesh radius, on the mesh of the moved node): wall time around
     UpdateMesh + ctl_builder_finalize + ctl_scene_update, median of 10, and the refit kernels' HIP-event time; against what a host without CTL_DIFF_GEOMETRY pays in
     the same run — the scene built again in a new builder with the cache warm for every untouched mesh, ctl_builder_add_mesh of the deformed arrays (cold: a new
     content hash) and ctl_scene_create_ex (the flattened tree is necessarily cold too); and the refitted tree's Mrays/s and node-area ratio against a fresh tree.
     A workload that comes from a Mitsuba file has no vertex arrays on the Python side: the mesh's triangles are taken back from its Woop rows as a triangle soup.
--only deform runs step 4 (and the camera update of step 1) alone.
  5. (--only skin) a pose change of the same mesh under four bones (position bands along its long axis, blended weights), median of 10 each, in one run:
     (a) the host path: DynamicScene.UpdateMesh + ctl_builder_finalize + ctl_scene_update with the positions and normals skinned BEFOREHAND (ctl_skin_mesh_host, not timed);
     (b) ctl_scene_animate_mesh on the mesh bound with ctl_scene_bind_skin (the bind is timed once, apart): wall time and the HIP-event times of the three pose kernels
         and of the refit.  After (b) a camera update on the bound scene is timed too: the bound mesh is neither hashed nor compared.
  6. (--only rebuild) ctl_scene_rebuild_flat after M3 (one node carried across a third of the scene) and after the deformation D1 of step 4, each on a scene of its
     own: wall time around the (synchronous) call — the first call, which also loads the kernels and allocates rocPRIM's storage, and the median of 5 further calls —
     with the stage times of ctl_scene_rebuild_stats; against the re-creation of the same pose measured in the same run (M3: warm cache; D1: as in step 4, the
     flattened tree necessarily cold); and the Mrays/s of the refitted, the rebuilt and a fresh tree with the node-area ratios.
  7. (--only nodes) ctl_scene_update_nodes: one more instance of the moved node's mesh added (at the M3 place), then one node removed, each timed once — wall
     time around the (synchronous) call with the stage times of ctl_scene_nodes_stats — against the warm-cache re-creation of the same description in the same run,
     and the Mrays/s of the updated scene (an LBVH, the added instance with whole-triangle entries) against the freshly created one.
  8. (--only meshes) ctl_scene_update_meshes: one mesh appended — a copy of the moved node's mesh — with one node of it (at the M3 place), timed once: wall time around
     the (synchronous) call, the host hashing, the append stage and the stage times of ctl_scene_nodes_stats, against the warm-cache re-creation of the same
     description in the same run, and the rays/s of the updated scene against the fresh one's.
  9. (--only mesh-remove) ctl_scene_update_mesh_set: step 8's append, then the ORIGINAL mesh of the moved node — it stands in front of the copy — removed together with
     its nodes, timed once: wall time, the host hashing, the compaction kernels between HIP events with the bytes they moved, a plain device-to-device copy of the same
     byte count in the same run (warm-up, median of 10) as their yardstick, the node-set stages, warm-cache re-creation of the same description, rays/s, HBM freed.
One JSON line per workload is appended to --out; --results appends a section to that Markdown file.  bench.py is not involved.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cudatracerlib_amd import api, scenes   # noqa: E402
import cudatracerlib_amd as ctl              # noqa: E402


def build(workload, args):
    if workload == "synthetic-sm":
        return scenes.synthetic_sm(args.width, args.height)
    if workload == "synthetic-sm-hard":
        nx, nz = (4096, 1024) if args.hard_scale == "full" else (1024, 256)
        d = os.path.join(os.environ.get("TMPDIR", "/tmp"), "ctl_scene_sm_hard_%dx%d_%dx%d" % (nx, nz, args.width, args.height))
        if not os.path.exists(os.path.join(d, "scene.xml")):
            scenes.write_sm_hard_mitsuba(d, args.width, args.height, nx=nx, nz=nz, cards=4000 if args.hard_scale == "full" else 1000, beams=3000 if args.hard_scale == "full" else 600)
        return scenes.load_mitsuba(os.path.join(d, "scene.xml"), args.width, args.height)
    raise SystemExit("unknown workload " + workload)


def transforms(desc):
    return desc.view("node_transforms", np.float32, desc.n_nodes, 16).reshape(-1, 4, 4).astype(np.float64)


def rot(axis, angle):
    a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def motion(X0, size, which, step=0):
    Y = X0.copy()
    if which == "M1":
        Y[:3, 3] += 0.01 * size * np.array([1.0, 0.3, -0.6]) * (1 + step)
    elif which == "M2":
        Y[:3, :3] = rot((0.3, 1.0, 0.2), 0.7312) @ np.diag([1.3, 0.8, 1.1]) @ X0[:3, :3]
    else:
        Y[:3, 3] += size * np.array([0.33, 0.0, 0.2])
    return Y.astype(np.float32)


def mrays(scene, args):
    tr = ctl.WavefrontPathTracer()
    tr.getParameters().setValue("MaxPathLength", args.depth)
    tr.Resize(args.width, args.height); tr.InitializeScene(scene)
    img = ctl.Image(args.width, args.height)
    tr.DoPasses(img, 1, new_trace=True)                  # warm-up
    t0 = tr.stats()
    tr.DoPasses(img, args.passes, new_trace=False)
    t1 = tr.stats()
    return (t1.rays_total - t0.rays_total) / max(1e-9, t1.seconds_total - t0.seconds_total) / 1e6


def mesh_soup(d, mesh):
    """the triangles of one mesh of a description as a soup (3 * n_tri, 3) float32: the vertices back from the Woop rows (TriIntersectorData::getData), one row per triangle"""
    M = d.view("meshes", np.uint32, d.n_meshes, 5)
    first = int(M[mesh, 2] // 3); later = np.sort(M[:, 2] // 3); later = later[later > first]
    last = int(later[0]) if len(later) else d.n_woop
    tris = d.view("woop_index", np.uint32, d.n_woop, 1)[int(M[mesh, 3]):int(M[mesh, 3]) + last - first, 0] >> 1
    _, pick = np.unique(tris, return_index=True)             # sorted by triangle id: triangle t of the mesh is row pick[t]
    R = d.view("woop", np.float32, d.n_woop, 12)[first:last][pick].astype(np.float64).reshape(-1, 3, 4)
    A = np.zeros((len(R), 4, 4)); A[:, 0] = R[:, 1]; A[:, 1] = R[:, 2]; A[:, 2] = R[:, 0]; A[:, 2, 3] *= -1; A[:, 3, 3] = 1
    Ai = np.linalg.inv(A)
    v2 = Ai[:, :3, 3]
    return np.stack([v2 + Ai[:, :3, 0], v2 + Ai[:, :3, 1], v2], axis=1).reshape(-1, 3).astype(np.float32)


def ripple(P, k=0):
    """D1 of tests/scene_deform_cases.py: along the direction from the mesh's centre, amplitude 4 % of its radius; k shifts the phase (every step of a timing loop differs)"""
    P = np.asarray(P, np.float64)
    c = 0.5 * (P.min(axis=0) + P.max(axis=0)); Q = P - c
    radius = np.linalg.norm(Q, axis=1).max()
    n = Q / np.maximum(np.linalg.norm(Q, axis=1, keepdims=True), 1e-30)
    return (P + n * (0.04 * radius * np.sin(5.0 * Q[:, 0] / radius + 3.0 * Q[:, 1] / radius + 0.7 + 0.37 * k))[:, None]).astype(np.float32)


def deformation(workload, args, sc, scene, node, rec):
    d = sc.desc
    mesh = int(d.view("nodes", np.uint32, d.n_nodes, 6)[node, 0])
    inp = sc.mesh_inputs.get(mesh)
    P0, I, N, UV = (inp["positions"], inp["indices"], inp["normals"], inp["uvs"]) if inp else (mesh_soup(d, mesh), None, None, None)
    rec["deformed_mesh"] = mesh; rec["deformed_triangles"] = int(len(I) if I is not None else len(P0) // 3)
    rec["deformed_instances"] = int((d.view("nodes", np.uint32, d.n_nodes, 6)[:, 0] == mesh).sum())
    refit = []

    def deform(k):
        sc.UpdateMesh(mesh, ripple(P0, k), I, normals=N, uvs=UV); assert scene.update(sc.UpdateScene()) & api.DIFF_GEOMETRY; refit.append(scene.update_stats()["refit_ms"])
    rec["update_deform_ms"] = timed(deform)
    rec["deform_refit_kernels_ms"] = float(np.median(refit))
    P1 = ripple(P0, 100)
    sc.UpdateMesh(mesh, P1, I, normals=N, uvs=UV); scene.update(sc.UpdateScene())
    st = scene.update_stats()
    r = mrays(scene, args)
    # what the same change costs without CTL_DIFF_GEOMETRY: the cache is warmed by a first build of the untouched scene; then a new builder (every untouched mesh from
    # the cache), the deformed arrays compiled (cold) and the scene created (the flattened tree cold)
    with tempfile.TemporaryDirectory() as cache:
        api.set_cache_dir(cache)
        warm = build(workload, args); del warm
        t = time.perf_counter()
        again = build(workload, args)
        cold = api.DynamicScene(); cold.add_mesh(P1, I, normals=N, uvs=UV)
        rec["recreate_deformed_builder_ms"] = (time.perf_counter() - t) * 1e3
        again.UpdateMesh(mesh, P1, I, normals=N, uvs=UV); again.UpdateScene()     # (not timed: stands in for the new builder holding the deformed mesh)
        t = time.perf_counter(); fresh = ctl.Scene(again.desc, flatten=True); rec["recreate_deformed_create_ms"] = (time.perf_counter() - t) * 1e3
        api.set_cache_dir(None)
    rec["recreate_deformed_ms"] = rec["recreate_deformed_builder_ms"] + rec["recreate_deformed_create_ms"]
    f = mrays(fresh, args)
    del fresh
    rec["traversal_deformed"] = dict(refit_mrays=r, fresh_mrays=f, ratio=r / f, node_area_before=st["node_area_before"], node_area_after=st["node_area_after"],
                                     area_ratio=st["node_area_after"] / st["node_area_before"], refit_ms=st["refit_ms"])
    rec["deform_faster_than_recreate"] = bool(rec["update_deform_ms"] < rec["recreate_deformed_ms"])


def skin_pose(c, axis, k):
    """four bone matrices of pose k: small rotations about the mesh centre that grow along the band, plus a stretch; the mesh stays within a few percent of its rest box"""
    out = np.tile(np.eye(4), (4, 1, 1))
    for b in range(4):
        lin = rot(axis, 0.02 * (b - 1.5) * (1 + 0.3 * np.sin(0.9 * k + b))) @ np.diag([1.0, 1.0 - 0.01 * b, 1.0 + 0.005 * b])
        out[b, :3, :3] = lin; out[b, :3, 3] = c - lin @ c
    return out.astype(np.float32)


def skinning(workload, args, sc, scene, node, rec):
    d = sc.desc
    mesh = int(d.view("nodes", np.uint32, d.n_nodes, 6)[node, 0])
    inp = sc.mesh_inputs.get(mesh)
    P0, I, N, UV = (inp["positions"], inp["indices"], inp["normals"], inp["uvs"]) if inp else (mesh_soup(d, mesh), None, None, None)
    P0 = np.ascontiguousarray(P0, np.float32)
    rec["skinned_mesh"] = mesh; rec["skinned_triangles"] = int(len(I) if I is not None else len(P0) // 3); rec["skinned_vertices"] = int(len(P0))
    rec["skinned_instances"] = int((d.view("nodes", np.uint32, d.n_nodes, 6)[:, 0] == mesh).sum())
    lo, hi = P0.min(axis=0).astype(np.float64), P0.max(axis=0).astype(np.float64)
    c = 0.5 * (lo + hi); ax = int(np.argmax(hi - lo)); axis = np.eye(3)[(ax + 1) % 3]
    t = (P0[:, ax] - lo[ax]) / max(hi[ax] - lo[ax], 1e-30) * 3.0
    b0 = np.minimum(np.floor(t).astype(np.int64), 2)
    BI = np.zeros((len(P0), 8), np.uint8); BW = np.zeros((len(P0), 8), np.uint8)
    BI[:, 0] = b0; BI[:, 1] = b0 + 1; BW[:, 1] = np.clip(np.round((t - b0) * 255.0), 0, 255); BW[:, 0] = 255 - BW[:, 1]
    n = 10
    poses = [(skin_pose(c, axis, k), skin_pose(c, axis, k + 0.5), 0.25) for k in range(n + 1)]
    # (a) the host path, with the vertices skinned beforehand: ctl_skin_mesh_host makes the very positions and normals (b) leaves in HBM
    skinned = [api.skin_mesh_host(d, mesh, P0, I, BI, BW, 4, B0, B1, lerp, rest_normals=N) for B0, B1, lerp in poses[:n]]
    refit_a = []

    def host_path(k):
        sc.UpdateMesh(mesh, skinned[k]["positions"], I, normals=skinned[k]["normals"], uvs=UV); assert scene.update(sc.UpdateScene()) & api.DIFF_GEOMETRY; refit_a.append(scene.update_stats()["refit_ms"])
    rec["skin_host_path_ms"] = timed(host_path, n)
    rec["skin_host_path_refit_kernels_ms"] = float(np.median(refit_a))
    del skinned
    # (b) the device path
    tb = time.perf_counter(); scene.bind_skin(mesh, P0, I, BI, BW, 4, rest_normals=N); rec["skin_bind_ms"] = (time.perf_counter() - tb) * 1e3
    scene.animate_mesh(mesh, *poses[n])          # (first launch of the kernels: not timed)
    stats = []

    def device_path(k):
        stats.append(scene.animate_mesh(mesh, *poses[k]))
    rec["skin_animate_ms"] = timed(device_path, n)
    rec["skin_kernels_ms"] = float(np.median([s["skin_ms"] for s in stats])); rec["skin_refit_kernels_ms"] = float(np.median([s["refit_ms"] for s in stats]))
    cam0 = api.ctl_sensor.from_buffer_copy(d.camera)

    def camera(k):
        s = api.ctl_sensor.from_buffer_copy(cam0); s.to_world[3] += 0.0007 * (k + 1); sc.setSensor(s); assert scene.update(sc.UpdateScene()) == api.DIFF_CAMERA
    rec["skin_bound_camera_update_ms"] = timed(camera, n)
    rec["skin_mrays"] = mrays(scene, args)
    rec["skin_faster_than_host_path"] = bool(rec["skin_animate_ms"] < rec["skin_host_path_ms"])


def rebuild_block(scene, args):
    """Mrays/s of the tree as it stands (refitted), then the rebuild: first call, median of 5 more, the last call's stats, Mrays/s of the rebuilt tree"""
    r = mrays(scene, args)
    t = time.perf_counter(); first = scene.rebuild_flat(builder=args.builder); first_ms = (time.perf_counter() - t) * 1e3
    stats = []
    wall = timed(lambda k: stats.append(scene.rebuild_flat(builder=args.builder)), 5)
    st = dict(stats[-1]); st.update(sort_ms=float(np.median([x["sort_ms"] for x in stats])), topology_ms=float(np.median([x["topology_ms"] for x in stats])),
                                    refit_ms=float(np.median([x["refit_ms"] for x in stats])), total_ms=float(np.median([x["total_ms"] for x in stats])))
    return dict(refit_mrays=r, rebuilt_mrays=mrays(scene, args), rebuild_first_ms=first_ms, rebuild_ms=wall, stats=st, node_area_refitted=first["node_area_before"], node_area_rebuilt=first["node_area_after"])


def rebuilding(workload, args, sc, scene, node, X0, size, rec):
    # after M3
    sc.SetNodeTransform(node, motion(X0, size, "M3")); assert scene.update(sc.UpdateScene()) & api.DIFF_TRANSFORMS
    b = rebuild_block(scene, args)
    with tempfile.TemporaryDirectory() as cache:
        api.set_cache_dir(cache)
        s2 = ctl.Scene(sc.desc, flatten=True); del s2     # warms the cache for exactly this pose
        t = time.perf_counter(); fresh = ctl.Scene(sc.UpdateScene(), flatten=True); b["recreate_warmcache_ms"] = (time.perf_counter() - t) * 1e3
        api.set_cache_dir(None)
    fb = fresh.flat_bvh(); b["fresh_nodes"] = int(fb.desc.n_nodes); del fb
    b["fresh_mrays"] = mrays(fresh, args); del fresh
    b["faster_than_recreate"] = bool(b["rebuild_ms"] < b["recreate_warmcache_ms"] and b["rebuild_first_ms"] < b["recreate_warmcache_ms"])
    rec["rebuild_M3"] = b
    del scene
    # after D1, on a scene of its own (the tree as built, refitted to the deformed mesh)
    sc.SetNodeTransform(node, X0.astype(np.float32))
    scene = ctl.Scene(sc.UpdateScene(), flatten=True)
    d = sc.desc
    mesh = int(d.view("nodes", np.uint32, d.n_nodes, 6)[node, 0])
    inp = sc.mesh_inputs.get(mesh)
    P0, I, N, UV = (inp["positions"], inp["indices"], inp["normals"], inp["uvs"]) if inp else (mesh_soup(d, mesh), None, None, None)
    P1 = ripple(P0, 100)
    sc.UpdateMesh(mesh, P1, I, normals=N, uvs=UV); assert scene.update(sc.UpdateScene()) & api.DIFF_GEOMETRY
    b = rebuild_block(scene, args)
    del scene
    with tempfile.TemporaryDirectory() as cache:   # the re-creation of step 4: every untouched mesh from the cache, the deformed one and the flattened tree cold
        api.set_cache_dir(cache)
        warm = build(workload, args); del warm
        t = time.perf_counter()
        again = build(workload, args)
        cold = api.DynamicScene(); cold.add_mesh(P1, I, normals=N, uvs=UV)
        builder_ms = (time.perf_counter() - t) * 1e3
        again.UpdateMesh(mesh, P1, I, normals=N, uvs=UV); again.UpdateScene()
        t = time.perf_counter(); fresh = ctl.Scene(again.desc, flatten=True); b["recreate_deformed_ms"] = builder_ms + (time.perf_counter() - t) * 1e3
        api.set_cache_dir(None)
    b["fresh_mrays"] = mrays(fresh, args); del fresh
    b["faster_than_recreate"] = bool(b["rebuild_ms"] < b["recreate_deformed_ms"] and b["rebuild_first_ms"] < b["recreate_deformed_ms"])
    rec["rebuild_D1"] = b


def node_set(workload, args, sc, scene, node, X0, size, rec):
    d = sc.desc
    mesh = int(d.view("nodes", np.uint32, d.n_nodes, 6)[node, 0])

    def one(what, edit):
        edit()
        t = time.perf_counter(); st = scene.update_nodes(sc.UpdateScene(), builder=args.builder); wall = (time.perf_counter() - t) * 1e3
        b = dict(wall_ms=wall, stats=st, updated_mrays=mrays(scene, args))
        with tempfile.TemporaryDirectory() as cache:
            api.set_cache_dir(cache)
            s2 = ctl.Scene(sc.desc, flatten=True); del s2     # warms the cache for exactly this description
            t = time.perf_counter(); fresh = ctl.Scene(sc.UpdateScene(), flatten=True); b["recreate_warmcache_ms"] = (time.perf_counter() - t) * 1e3
            api.set_cache_dir(None)
        b["fresh_mrays"] = mrays(fresh, args); del fresh
        rec["nodes_" + what] = b
    one("add", lambda: sc.CreateNode(mesh, motion(X0, size, "M3")))
    one("remove", lambda: sc.DeleteNode(node))


def mesh_set(workload, args, sc, scene, node, X0, size, rec):
    """--only meshes: one mesh appended — a copy of the middle node's mesh, its triangles taken back from the Woop rows — and one node of it at the M3 place"""
    d = sc.desc
    mesh = int(d.view("nodes", np.uint32, d.n_nodes, 6)[node, 0])
    P = mesh_soup(d, mesh)
    t = time.perf_counter(); new_mesh = sc.add_mesh(P, np.arange(len(P), dtype=np.uint32).reshape(-1, 3), materials=[api.diffuse((0.6, 0.5, 0.4))]); compile_ms = (time.perf_counter() - t) * 1e3
    sc.CreateNode(new_mesh, motion(X0, size, "M3"))
    t = time.perf_counter(); st = scene.update_meshes(sc.UpdateScene(), builder=args.builder); wall = (time.perf_counter() - t) * 1e3
    b = dict(wall_ms=wall, add_mesh_ms=compile_ms, stats=st, updated_mrays=mrays(scene, args))
    with tempfile.TemporaryDirectory() as cache:
        api.set_cache_dir(cache)
        s2 = ctl.Scene(sc.desc, flatten=True); del s2     # warms the cache for exactly this description
        t = time.perf_counter(); fresh = ctl.Scene(sc.UpdateScene(), flatten=True); b["recreate_warmcache_ms"] = (time.perf_counter() - t) * 1e3
        api.set_cache_dir(None)
    b["fresh_mrays"] = mrays(fresh, args); del fresh
    rec["meshes_add"] = b


def device_copy_gbs(n_bytes):
    """(ms, GB/s read + written) of a plain device-to-device hipMemcpy of n_bytes: the yardstick of the compaction kernels.  Three warm-up copies, HIP events on the null
    stream, median of 10.  The HIP runtime is the one the library has loaded"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    def ok(code):
        if code != 0:
            raise RuntimeError("HIP error %d in device_copy_gbs" % code)
    n = max(1, int(n_bytes))
    src, dst, a, b = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    ok(hip.hipMalloc(C.byref(src), C.c_size_t(n))); ok(hip.hipMalloc(C.byref(dst), C.c_size_t(n)))
    ok(hip.hipMemset(src, 0, C.c_size_t(n)))
    ok(hip.hipEventCreate(C.byref(a))); ok(hip.hipEventCreate(C.byref(b)))
    ts = []
    for k in range(13):
        ok(hip.hipEventRecord(a, None))
        ok(hip.hipMemcpyAsync(dst, src, C.c_size_t(n), C.c_int(3), None))      # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(b, None)); ok(hip.hipEventSynchronize(b))
        ms = C.c_float(0); ok(hip.hipEventElapsedTime(C.byref(ms), a, b))
        if k >= 3:
            ts.append(ms.value)
    hip.hipEventDestroy(a); hip.hipEventDestroy(b); hip.hipFree(src); hip.hipFree(dst)
    ms = float(np.median(ts))
    return ms, 2.0 * n / (ms * 1e-3) / 1e9


def mesh_remove(workload, args, sc, scene, node, X0, size, rec):
    """--only mesh-remove: mesh_set's append (a copy of the middle node's mesh with one node), then the ORIGINAL mesh — it stands in front of the copy — removed together
    with its nodes through ctl_scene_update_mesh_set.  Each call is timed once."""
    mesh_set(workload, args, sc, scene, node, X0, size, rec)
    d = sc.desc
    nodes = d.view("nodes", np.uint32, d.n_nodes, 6)
    mesh = int(nodes[node, 0])
    mine = [k for k in range(d.n_nodes) if int(nodes[k, 0]) == mesh]
    bytes_before = d.n_tri_data * 32 + (d.n_woop + d.n_bvh_nodes) * 64
    for k in reversed(mine):
        sc.DeleteNode(k)
    sc.RemoveMesh(mesh)
    t = time.perf_counter(); st = scene.update_mesh_set(sc.UpdateScene(), builder=args.builder); wall = (time.perf_counter() - t) * 1e3
    b = dict(wall_ms=wall, nodes_removed=len(mine), stats=st, updated_mrays=mrays(scene, args), geometry_bytes_before=int(bytes_before))
    b["compact_gbs"] = 2.0 * st["bytes_moved"] / (st["compact_ms"] * 1e-3) / 1e9 if st["compact_ms"] > 0 else 0.0
    b["copy_ms"], b["copy_gbs"] = device_copy_gbs(int(st["bytes_moved"]))
    with tempfile.TemporaryDirectory() as cache:
        api.set_cache_dir(cache)
        s2 = ctl.Scene(sc.desc, flatten=True); del s2     # warms the cache for exactly this description
        t = time.perf_counter(); fresh = ctl.Scene(sc.UpdateScene(), flatten=True); b["recreate_warmcache_ms"] = (time.perf_counter() - t) * 1e3
        api.set_cache_dir(None)
    b["fresh_mrays"] = mrays(fresh, args); del fresh
    rec["meshes_remove"] = b


def markdown_mesh_remove(recs):
    out = ["", "## Removing meshes in place (tools/scene_update_bench.py --only mesh-remove)", "",
           "| workload | removed (meshes / triangles / rows / BVH nodes, nodes) | runs | entries | ctl_scene_update_mesh_set, wall | hashing (host) | compaction: bytes moved, time, read + written | plain device copy of the same bytes | drop + generate | rebuild | node-set stages, device total | re-creation, warm cache | HBM freed | updated scene | fresh scene | ratio |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        b = r["meshes_remove"]; st = b["stats"]; n = st["meshes"]["nodes"]; rb = n["rebuild"]
        out.append("| %s | %d / %d / %d / %d, %d | %d | %d -> %d | %.1f ms | %.1f ms | %.1f MB, %.3f ms, %.0f GB/s | %.3f ms, %.0f GB/s | %.2f ms | %.2f ms | %.2f ms | %.0f ms | %.2f MB | %.0f Mrays/s | %.0f Mrays/s | %.3f |" % (
                   r["workload"], st["meshes_removed"], st["triangles_removed"], st["rows_removed"], st["bvh_nodes_removed"], b["nodes_removed"], st["runs"], n["entries_before"], n["entries_after"], b["wall_ms"],
                   st["hash_ms"], st["bytes_moved"] / 1e6, st["compact_ms"], b["compact_gbs"], b["copy_ms"], b["copy_gbs"], n["edit_ms"], rb["total_ms"], n["total_ms"], b["recreate_warmcache_ms"], st["bytes_freed"] / 1e6,
                   b["updated_mrays"], b["fresh_mrays"], b["updated_mrays"] / b["fresh_mrays"]))
    return "\n".join(out) + "\n"


def markdown_meshes(recs):
    out = ["", "## Adding meshes in place (tools/scene_update_bench.py --only meshes)", "",
           "| workload | appended (triangles / rows / BVH nodes) | entries | generated | ctl_scene_update_meshes, wall | hashing (host) | append (copies + uploads + kernel) | drop + generate | rebuild (key + sort / topology + gather / boxes) | node-set stages, device total | re-creation, warm cache | updated scene | fresh scene | ratio |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        b = r["meshes_add"]; st = b["stats"]; n = st["nodes"]; rb = n["rebuild"]
        out.append("| %s | %d / %d / %d | %d -> %d | %d | %.1f ms | %.1f ms | %.2f ms | %.2f ms | %.2f ms (%.2f / %.2f / %.2f) | %.2f ms | %.0f ms | %.0f Mrays/s | %.0f Mrays/s | %.3f |" % (r["workload"], st["triangles_added"], st["rows_added"],
                   st["bvh_nodes_added"], n["entries_before"], n["entries_after"], n["entries_generated"], b["wall_ms"], st["hash_ms"], st["append_ms"], n["edit_ms"], rb["total_ms"], rb["sort_ms"], rb["topology_ms"], rb["refit_ms"],
                   n["total_ms"], b["recreate_warmcache_ms"], b["updated_mrays"], b["fresh_mrays"], b["updated_mrays"] / b["fresh_mrays"]))
    return "\n".join(out) + "\n"


def markdown_nodes(recs):
    out = ["", "## Adding and removing nodes in place (tools/scene_update_bench.py --only nodes)", "",
           "| workload | edit | entries | dropped | generated | ctl_scene_update_nodes, wall | drop + generate | rebuild (key + sort / topology + gather / boxes) | device total | re-creation, warm cache | updated scene | fresh scene | ratio |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        for what in ("add", "remove"):
            b = r["nodes_" + what]; st = b["stats"]; rb = st["rebuild"]
            out.append("| %s | %s one node | %d -> %d | %d | %d | %.1f ms | %.2f ms | %.2f ms (%.2f / %.2f / %.2f) | %.2f ms | %.0f ms | %.0f Mrays/s | %.0f Mrays/s | %.3f |" % (r["workload"], what, st["entries_before"], st["entries_after"],
                       st["entries_dropped"], st["entries_generated"], b["wall_ms"], st["edit_ms"], rb["total_ms"], rb["sort_ms"], rb["topology_ms"], rb["refit_ms"], st["total_ms"], b["recreate_warmcache_ms"],
                       b["updated_mrays"], b["fresh_mrays"], b["updated_mrays"] / b["fresh_mrays"]))
    return "\n".join(out) + "\n"


def markdown_rebuild(recs):
    out = ["", "## Rebuilding the flattened tree on the device (tools/scene_update_bench.py --only rebuild)", "",
           "| workload | after | entries | nodes (fresh tree) | depth | ctl_scene_rebuild_flat: first call | median of 5 | key + sort | topology + gather | boxes | re-creation of the same pose |",
           "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        for what, key in (("M3", "recreate_warmcache_ms"), ("D1", "recreate_deformed_ms")):
            b = r["rebuild_" + what]; st = b["stats"]
            out.append("| %s | %s | %d | %d (%s) | %d | %.1f ms | %.1f ms | %.2f ms | %.2f ms | %.2f ms | %.0f ms (%s) |" % (r["workload"], what, st["n_entries"], st["n_nodes"], b.get("fresh_nodes", "-"), st["max_depth"],
                       b["rebuild_first_ms"], b["rebuild_ms"], st["sort_ms"], st["topology_ms"], st["refit_ms"], b[key], "warm cache" if what == "M3" else "flattened tree cold"))
    out += ["", "| workload | after | refitted tree | rebuilt tree | fresh tree | rebuilt / refitted | rebuilt / fresh | node area: rebuilt / refitted |", "|---|---|---|---|---|---|---|---|"]
    for r in recs:
        for what in ("M3", "D1"):
            b = r["rebuild_" + what]
            out.append("| %s | %s | %.0f Mrays/s | %.0f Mrays/s | %.0f Mrays/s | %.3f | %.3f | %.3f |" % (r["workload"], what, b["refit_mrays"], b["rebuilt_mrays"], b["fresh_mrays"], b["rebuilt_mrays"] / b["refit_mrays"],
                       b["rebuilt_mrays"] / b["fresh_mrays"], b["node_area_rebuilt"] / b["node_area_refitted"]))
    return "\n".join(out) + "\n"


def markdown_skin(recs):
    out = ["", "## Skinned meshes: a pose from bone matrices (tools/scene_update_bench.py --only skin)", "",
           "| workload | skinned mesh (triangles x instances) | (a) UpdateMesh + finalize + ctl_scene_update, vertices skinned beforehand (refit kernels) | (b) ctl_scene_animate_mesh, wall | pose kernels | refit kernels | bind, once | camera update, mesh bound |",
           "|---|---|---|---|---|---|---|---|"]
    for r in recs:
        out.append("| %s | %d x %d | %.2f ms (%.2f ms) | %.2f ms | %.3f ms | %.2f ms | %.0f ms | %.2f ms |" % (r["workload"], r["skinned_triangles"], r["skinned_instances"], r["skin_host_path_ms"],
                   r["skin_host_path_refit_kernels_ms"], r["skin_animate_ms"], r["skin_kernels_ms"], r["skin_refit_kernels_ms"], r["skin_bind_ms"], r["skin_bound_camera_update_ms"]))
    return "\n".join(out) + "\n"


def timed(f, n=10):
    ts = []
    for k in range(n):
        t = time.perf_counter(); f(k); ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def run(workload, args):
    api.set_cache_dir(None)
    sc = build(workload, args)
    d = sc.desc
    size = np.array(d.box_max[:]) - np.array(d.box_min[:])
    node = d.n_nodes // 2
    X0 = transforms(d)[node].copy()
    t = time.perf_counter(); scene = ctl.Scene(d, flatten=True); create_ms = (time.perf_counter() - t) * 1e3
    fb = scene.flat_bvh()
    rec = dict(workload=workload, width=args.width, height=args.height, nodes=int(d.n_nodes), flat_nodes=int(fb.desc.n_nodes), flat_entries=int(fb.desc.n_leaves), create_ms=create_ms, moved_node=int(node))
    del fb
    cam0 = api.ctl_sensor.from_buffer_copy(d.camera)

    def camera(k):
        s = api.ctl_sensor.from_buffer_copy(cam0); s.to_world[3] += 0.001 * size[0] * (k + 1); sc.setSensor(s); assert scene.update(sc.UpdateScene()) == api.DIFF_CAMERA
    rec["update_camera_ms"] = timed(camera)
    if args.only == "deform":
        deformation(workload, args, sc, scene, node, rec)
        return rec
    if args.only == "skin":
        skinning(workload, args, sc, scene, node, rec)
        return rec
    if args.only == "rebuild":
        rebuilding(workload, args, sc, scene, node, X0, size, rec)
        return rec
    if args.only == "nodes":
        node_set(workload, args, sc, scene, node, X0, size, rec)
        return rec
    if args.only == "mesh-remove":
        mesh_remove(workload, args, sc, scene, node, X0, size, rec)
        return rec
    if args.only == "meshes":
        mesh_set(workload, args, sc, scene, node, X0, size, rec)
        return rec

    def material(k):
        sc.desc.materials[0].tex[0].value[0] = 0.3 + 0.01 * k; assert scene.update(sc.desc) == api.DIFF_MATERIALS
    rec["update_material_ms"] = timed(material)

    def material_type(k):
        m = sc.desc.materials[0]; m.bsdf_type, m.combined_type = (2, m.combined_type) if m.bsdf_type == 1 else (1, m.combined_type); assert scene.update(sc.desc) == api.DIFF_MATERIALS
    if sc.desc.materials[0].bsdf_type in (1, 2):          # diffuse <-> rough diffuse: same parameter slots, another model nibble
        rec["update_material_restamp_ms"] = timed(material_type, 10)
    refit = []

    def transform(k):
        sc.SetNodeTransform(node, motion(X0, size, "M1", k)); assert scene.update(sc.UpdateScene()) & api.DIFF_TRANSFORMS; refit.append(scene.update_stats()["refit_ms"])
    rec["update_transform_ms"] = timed(transform)
    rec["refit_kernels_ms"] = float(np.median(refit))
    # the same change without ctl_scene_update: finalize + create, cache off / cache warm for the new transforms
    sc.SetNodeTransform(node, motion(X0, size, "M1", 20))
    t = time.perf_counter(); s2 = ctl.Scene(sc.UpdateScene(), flatten=True); rec["recreate_nocache_ms"] = (time.perf_counter() - t) * 1e3; del s2
    with tempfile.TemporaryDirectory() as cache:
        api.set_cache_dir(cache)
        s2 = ctl.Scene(sc.desc, flatten=True); del s2     # warms the cache for exactly these transforms
        t = time.perf_counter(); s2 = ctl.Scene(sc.UpdateScene(), flatten=True); rec["recreate_warmcache_ms"] = (time.perf_counter() - t) * 1e3; del s2
        api.set_cache_dir(None)
    # traversal rate: refitted against fresh, per motion (the scene is refitted from the tree it was created with; a refit never reads an earlier one's result)
    rec["traversal"] = {}
    for which in ("M1", "M2", "M3"):
        sc.SetNodeTransform(node, motion(X0, size, which))
        scene.update(sc.UpdateScene())
        st = scene.update_stats()
        r = mrays(scene, args)
        fresh = ctl.Scene(sc.desc, flatten=True)
        f = mrays(fresh, args)
        del fresh
        rec["traversal"][which] = dict(refit_mrays=r, fresh_mrays=f, ratio=r / f, node_area_before=st["node_area_before"], node_area_after=st["node_area_after"],
                                       area_ratio=st["node_area_after"] / st["node_area_before"], refit_ms=st["refit_ms"])
    rec["faster_than_warm_recreate"] = bool(rec["update_transform_ms"] < rec["recreate_warmcache_ms"])
    sc.SetNodeTransform(node, X0.astype(np.float32)); scene.update(sc.UpdateScene())
    deformation(workload, args, sc, scene, node, rec)
    return rec


def markdown_deform(recs):
    out = ["", "## Deforming one mesh in place (tools/scene_update_bench.py)", "",
           "| workload | deformed mesh (triangles x instances) | update: camera | one-mesh deformation (refit kernels) | re-create: new builder + add_mesh | + ctl_scene_create_ex | re-create, total |", "|---|---|---|---|---|---|---|"]
    for r in recs:
        out.append("| %s | %d x %d | %.2f ms | %.2f ms (%.2f ms) | %.0f ms | %.0f ms | %.0f ms |" % (r["workload"], r["deformed_triangles"], r["deformed_instances"], r["update_camera_ms"], r["update_deform_ms"],
                   r["deform_refit_kernels_ms"], r["recreate_deformed_builder_ms"], r["recreate_deformed_create_ms"], r["recreate_deformed_ms"]))
    out += ["", "| workload | change | refitted tree | fresh tree | ratio | node-area ratio (SAH proxy) |", "|---|---|---|---|---|---|"]
    for r in recs:
        t = r["traversal_deformed"]
        out.append("| %s | D1 | %.0f Mrays/s | %.0f Mrays/s | %.3f | %.3f |" % (r["workload"], t["refit_mrays"], t["fresh_mrays"], t["ratio"], t["area_ratio"]))
    return "\n".join(out) + "\n"


def markdown(recs):
    if "meshes_remove" in recs[0]:
        return markdown_mesh_remove(recs) + markdown_meshes(recs)
    if "skin_animate_ms" in recs[0]:
        return markdown_skin(recs)
    if "rebuild_M3" in recs[0]:
        return markdown_rebuild(recs)
    if "nodes_add" in recs[0]:
        return markdown_nodes(recs)
    if "meshes_add" in recs[0]:
        return markdown_meshes(recs)
    if "update_transform_ms" not in recs[0]:
        return markdown_deform(recs)
    out = ["", "## In-place scene updates (tools/scene_update_bench.py)", "",
           "| workload | entries | update: camera | material | material + re-stamp | one-node transform (refit kernels) | re-create, no cache | re-create, warm cache |", "|---|---|---|---|---|---|---|---|"]
    for r in recs:
        out.append("| %s | %d | %.2f ms | %.2f ms | %s | %.2f ms (%.2f ms) | %.0f ms | %.0f ms |" % (r["workload"], r["flat_entries"], r["update_camera_ms"], r["update_material_ms"],
                   ("%.2f ms" % r["update_material_restamp_ms"]) if "update_material_restamp_ms" in r else "-", r["update_transform_ms"], r["refit_kernels_ms"], r["recreate_nocache_ms"], r["recreate_warmcache_ms"]))
    out += ["", "| workload | motion | refitted tree | fresh tree | ratio | node-area ratio (SAH proxy) |", "|---|---|---|---|---|---|"]
    for r in recs:
        for m, t in r["traversal"].items():
            out.append("| %s | %s | %.0f Mrays/s | %.0f Mrays/s | %.3f | %.3f |" % (r["workload"], m, t["refit_mrays"], t["fresh_mrays"], t["ratio"], t["area_ratio"]))
    return "\n".join(out) + "\n" + markdown_deform(recs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="synthetic-sm,synthetic-sm-hard")
    ap.add_argument("--hard-scale", default="full", choices=["full", "small"])
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--depth", type=int, default=8); ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_update.jsonl"))
    ap.add_argument("--results", default=None)
    ap.add_argument("--only", default=None, choices=["deform", "skin", "rebuild", "nodes", "meshes", "mesh-remove"], help="mesh-remove: the append of --only meshes, then the original mesh in front of the copy removed with its nodes through ctl_scene_update_mesh_set, against a plain device copy of the bytes the compaction moved and the re-creation of the same description; meshes: the camera update and ctl_scene_update_meshes appending one mesh the size of the middle node's, with one node of it, against the re-creation of the same description; nodes: the camera update and ctl_scene_update_nodes adding and removing one node against the re-creation of the same description; rebuild: the camera update and ctl_scene_rebuild_flat after M3 and after D1 against the re-creation of the same pose; deform: the camera update and the one-mesh deformation alone; skin: the camera update and the pose change of a bound mesh against the host path")
    ap.add_argument("--builder", default="lbvh", choices=["lbvh", "ploc"], help="the builder of --only rebuild and --only nodes (csrc/flat_ploc.h); the record carries it")
    ap.add_argument("--tag", default=None, help="a word for the record: which library ran (an A/B against another commit's library through $CTL_AMD_LIB)")
    args = ap.parse_args()
    if ctl.device_count() < 1:
        raise SystemExit("scene_update_bench needs a HIP device")
    recs = []
    for w in args.workloads.split(","):
        rec = run(w, args)
        if args.only in ("rebuild", "nodes", "meshes", "mesh-remove"):
            rec["builder"] = args.builder
        if args.tag:
            rec["tag"] = args.tag
        recs.append(rec)
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    if args.results:
        with open(args.results, "a") as f:
            f.write(markdown(recs))


if __name__ == "__main__":
    main()
