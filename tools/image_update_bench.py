#!/usr/bin/env python3
"""Cost of ctl_scene_update_image against re-creating the scene.

    python tools/image_update_bench.py [--width 1920 --height 1080] [--instances 2000] [--repeat 5] [--out profiles/image_update.jsonl]

synthetic-SM (cudatracerlib_amd/scenes.py) with two large images: a 4096 x 2048 RGBE environment map, and a 4096 x 4096 RGBCOL bitmap as the diffuse reflectance of a
plastic on one of its meshes.  On one GPU, in one process:
  1. ctl_scene_update_image of each image, from a host array and from a device pointer (CTL_IMAGE_TEXELS_DEVICE, memory of ctl_device_malloc): the stages of ctl_scene_image_stats
     (wall clock, each ended by a device synchronisation) — upload / pyramid / tables / hash / total — median of --repeat calls after one warm-up call, and the wall time
     around the call;
  2. what a host without the call pays: the same scene made again with the new image — a new builder (every mesh from the warm geometry cache), ctl_builder_finalize
     (which builds the pyramid of every image on the host for the texture averages) and ctl_scene_create_ex with CTL_SCENE_FLATTEN (the flattened tree from the warm cache).
One JSON line is appended to --out.  bench.py is not involved.
"""
import argparse
import ctypes as C
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

ENV, TEX = (4096, 2048), (4096, 4096)


def env_texels(seed):
    rs = np.random.RandomState(seed)
    return ((rs.randint(0, 1 << 24, size=(ENV[1], ENV[0])).astype(np.uint32) | np.uint32(0x404040)) | (rs.randint(124, 134, size=(ENV[1], ENV[0])).astype(np.uint32) << 24)).astype(np.uint32)


def tex_texels(seed):
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 1 << 24, size=(TEX[1], TEX[0])).astype(np.uint32) | np.uint32(0xff000000)).astype(np.uint32)


def build(args, env, tex):
    desc = scenes.synthetic_sm_description(args.width, args.height, n_instances=args.instances, subdiv=args.subdiv)
    sc = api.DynamicScene()
    ti = sc.add_image(tex, api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_ANISOTROPIC)
    ei = sc.add_image(env, api.TEXEL_RGBE, api.WRAP_REPEAT, api.FILTER_BILINEAR)
    meshes = []
    for k, m in enumerate(desc["meshes"]):
        mat = api.plastic(api.image_texture(ti), specular_reflectance=0.5) if k == 0 else scenes._material_of(m["material"])
        meshes.append(sc.add_mesh(m["V"], m["F"], normals=m.get("N"), materials=[mat]))
    nodes = [sc.CreateNode(meshes[mi], None if xf is None else np.asarray(xf, np.float32)) for mi, xf in desc["nodes"]]
    for ni, rad in desc["lights"]:
        sc.CreateLight(nodes[ni], 0, rad)
    sc.setEnvironementMap(ei, (1.0, 1.0, 1.0))
    sc.setCamera(*desc["camera"])
    sc.UpdateScene()
    return sc, ti, ei


def device_copy(t):
    p = C.c_void_p()
    api._check(api.lib.ctl_device_malloc(C.c_size_t(t.nbytes), C.byref(p)))
    api._check(api.lib.ctl_memcpy_h2d(p, t.ctypes.data_as(C.c_void_p), C.c_size_t(t.nbytes)))
    return p


def median_stats(runs):
    return {k: float(np.median([r[k] for r in runs])) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--instances", type=int, default=2000); ap.add_argument("--subdiv", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-recreate", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    envs = [env_texels(s) for s in (1, 2)]; texs = [tex_texels(s) for s in (3, 4)]
    out = dict(workload="synthetic-SM %dx%d, %d instances + env %dx%d RGBE + texture %dx%d RGBCOL" % ((args.width, args.height, args.instances) + ENV + TEX),
               library=os.path.basename(os.environ.get("CTL_AMD_LIB", "libctl_amd.so")))
    with tempfile.TemporaryDirectory() as cache:
        api.set_cache_dir(cache)
        t = time.perf_counter(); sc, ti, ei = build(args, envs[0], texs[0]); out["first_build_s"] = time.perf_counter() - t
        t = time.perf_counter(); scene = ctl.Scene(sc.desc, flatten=True); out["first_create_s"] = time.perf_counter() - t
        for name, image, sets in (("env", ei, envs), ("tex", ti, texs)):
            dev = [device_copy(s) for s in sets]
            for source in ("host", "device"):
                runs, walls = [], []
                for k in range(args.repeat + 1):
                    t = time.perf_counter()
                    st = scene.update_image(image, sets[k % 2]) if source == "host" else scene.update_image(image, dev[k % 2].value, width=sets[0].shape[1], height=sets[0].shape[0], device=True)
                    walls.append((time.perf_counter() - t) * 1e3); runs.append(st)
                out["%s_%s" % (name, source)] = dict(median_stats(runs[1:]), wall_ms=float(np.median(walls[1:])), first_wall_ms=walls[0])
            for p in dev:
                api.lib.ctl_device_free(p)
        if not args.no_recreate:
            # the host without the call: everything again with the other image set, caches warm (the first build above filled them)
            t = time.perf_counter(); sc2, _, _ = build(args, envs[1], texs[1]); out["recreate_build_s"] = time.perf_counter() - t
            t = time.perf_counter(); fresh = ctl.Scene(sc2.desc, flatten=True); out["recreate_create_s"] = time.perf_counter() - t
            out["recreate_total_s"] = out["recreate_build_s"] + out["recreate_create_s"]
            # and the updated scene is that scene: the same images in place, nothing left to update
            scene.update_image(ei, envs[1]); scene.update_image(ti, texs[1])
            try:
                out["update_after_matches_fresh"] = bool(scene.update(sc2.desc) == 0)
            except api.CtlError as e:
                out["update_after_matches_fresh"] = "refused: %s" % e
            del fresh
        api.set_cache_dir(None)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "a").write(line + "\n")


if __name__ == "__main__":
    main()
