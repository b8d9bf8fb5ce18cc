"""Emissive skins: what a pose of a mesh that carries an area light costs (RESULTS.md "Emissive skins").  HIP-event times as the library reports them.

  python tools/emissive_skin_bench.py [--workloads E2,synthetic-sm-hard] [--hard-scale full|small] [--out FILE]

Per workload, medians of 10 poses in one run:
  * skin_ms, shape_set_ms, refit_ms and the wall time of ctl_scene_animate_mesh on the mesh bound with CTL_SKIN_AREA_LIGHTS;
  * the host route for the same poses: DynamicScene.UpdateMesh (which recalculates the shape sets) + UpdateScene + ctl_scene_update, vertices skinned beforehand.
E2 is the 1152-triangle grid of tests/skin_emitter_cases.py; synthetic-sm-hard is bench.py's hard workload with an area light put on its 262 144-triangle mesh
(tools/scene_update_bench.py's skinned mesh and poses).  The time of k_shape_cdf alone comes from a rocprofv3 --kernel-trace --stats run of this script
(--poses-only skips the host route)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))

from cudatracerlib_amd import api   # noqa: E402
import cudatracerlib_amd as ctl      # noqa: E402


def med(xs):
    return float(np.median(xs))


def measure(rec, sc, d, mesh, P0, I, N, UV, BI, BW, n_bones, poses, host_route):
    """poses: n + 1 (bones0, bones1, lerp); the last one warms the kernels up"""
    n = len(poses) - 1
    scene = ctl.Scene(d, flatten=True)
    if host_route:
        skinned = [api.skin_mesh_host(d, mesh, P0, I, BI, BW, n_bones, B0, B1, lerp, rest_normals=N) for B0, B1, lerp in poses[:n]]
        ts = []
        for k in range(n):
            t = time.perf_counter()
            sc.UpdateMesh(mesh, skinned[k]["positions"], I, normals=skinned[k]["normals"], uvs=UV)
            mask = scene.update(sc.UpdateScene())
            ts.append((time.perf_counter() - t) * 1e3)
            assert mask & api.DIFF_GEOMETRY and mask & api.DIFF_LIGHTS
        rec["host_route_ms"] = med(ts)
        del skinned
    t = time.perf_counter(); scene.bind_skin(mesh, P0, I, BI, BW, n_bones, rest_normals=N, area_lights=True); rec["bind_ms"] = (time.perf_counter() - t) * 1e3
    scene.animate_mesh(mesh, *poses[n])
    stats, ts = [], []
    for k in range(n):
        t = time.perf_counter(); stats.append(scene.animate_mesh(mesh, *poses[k])); ts.append((time.perf_counter() - t) * 1e3)
    rec["animate_wall_ms"] = med(ts)
    for k in ("skin_ms", "shape_set_ms", "refit_ms"):
        rec[k] = med([s[k] for s in stats])


def run_e2(args):
    from skin_emitter_cases import make_case, SETUP
    from scene_update_cases import build
    K = make_case("E2")
    sc = build("S3", edit=SETUP["E2"])                      # the builder the host route updates
    rec = dict(workload="E2", triangles=K["n_tri"], vertices=int(len(K["P"])), lights=len(K["lights"]))
    poses = [(K["B0"], K["B1"], 0.05 + 0.08 * k) for k in range(11)]
    measure(rec, sc, sc.desc, K["mesh"], K["P"], K["I"], K["N"], None, K["BI"], K["BW"], K["n_bones"], poses, not args.poses_only)
    return rec


def run_hard(args):
    import scene_update_bench as sub
    a = argparse.Namespace(width=args.width, height=args.height, hard_scale=args.hard_scale)
    api.set_cache_dir(args.cache)                           # (a second run — the one under the profiler — finds the compiled meshes and the flattened tree)
    sc = sub.build("synthetic-sm-hard", a)
    d = sc.desc
    node = d.n_nodes // 2
    mesh = int(d.view("nodes", np.uint32, d.n_nodes, 6)[node, 0])
    t = time.perf_counter(); sc.CreateLight(node, 0, (3.0, 3.0, 2.5)); d = sc.UpdateScene(); create_light_ms = (time.perf_counter() - t) * 1e3
    inp = sc.mesh_inputs.get(mesh)
    P0, I, N, UV = (inp["positions"], inp["indices"], inp["normals"], inp["uvs"]) if inp else (sub.mesh_soup(d, mesh), None, None, None)
    P0 = np.ascontiguousarray(P0, np.float32)
    lo, hi = P0.min(axis=0).astype(np.float64), P0.max(axis=0).astype(np.float64)
    c = 0.5 * (lo + hi); ax = int(np.argmax(hi - lo)); axis = np.eye(3)[(ax + 1) % 3]
    t = (P0[:, ax] - lo[ax]) / max(hi[ax] - lo[ax], 1e-30) * 3.0
    b0 = np.minimum(np.floor(t).astype(np.int64), 2)
    BI = np.zeros((len(P0), 8), np.uint8); BW = np.zeros((len(P0), 8), np.uint8)
    BI[:, 0] = b0; BI[:, 1] = b0 + 1; BW[:, 1] = np.clip(np.round((t - b0) * 255.0), 0, 255); BW[:, 0] = 255 - BW[:, 1]
    L = d.lights[d.n_lights_buf - 1]
    rec = dict(workload="synthetic-sm-hard", hard_scale=args.hard_scale, triangles=int(len(I) if I is not None else len(P0) // 3), vertices=int(len(P0)), lights=1,
               light_triangles=int(L.count), instances=int((d.view("nodes", np.uint32, d.n_nodes, 6)[:, 0] == mesh).sum()), create_light_ms=create_light_ms)
    poses = [(sub.skin_pose(c, axis, k), sub.skin_pose(c, axis, k + 0.5), 0.25) for k in range(11)]
    measure(rec, sc, d, mesh, P0, I, N, UV, BI, BW, 4, poses, not args.poses_only)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="E2,synthetic-sm-hard")
    ap.add_argument("--hard-scale", default="full", choices=["full", "small"])
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--poses-only", action="store_true", help="no host route: the run to put under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--cache", default=None, help="a geometry cache directory for the synthetic-sm-hard scene (ctl_set_cache_dir)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if ctl.device_count() < 1:
        raise SystemExit("needs a HIP device")
    for w in args.workloads.split(","):
        rec = run_e2(args) if w == "E2" else run_hard(args)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
