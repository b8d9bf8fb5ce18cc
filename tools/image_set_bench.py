#!/usr/bin/env python3
"""Cost of ctl_scene_update_image_set against re-creating the scene.

    python tools/image_set_bench.py [--width 1920 --height 1080] [--instances 2000] [--repeat 3] [--out profiles/image_set.jsonl]

synthetic-SM (cudatracerlib_amd/scenes.py) with sixteen 1024 x 1024 RGBCOL textures — texture k the diffuse reflectance of a plastic on mesh k, texture 0 read by nothing —
and, behind them in the pool, a 4096 x 2048 RGBE environment map.  On one GPU, in one process, --repeat times on a scene made anew each time, three edits one after the
other, each through DynamicScene + Scene.update_image_set:
  append    one more 1024 x 1024 texture: nothing moves but the pool is laid out anew, so every kept pyramid is copied (one run)
  replace   texture 5 by a 2048 x 2048 one: two runs around a fresh image
  remove    texture 0, the first image of the pool: the worst case, everything behind it moves
For each: the stats of the call (HIP-event times of the move and of the fresh images' upload + pyramid, host time of the hash pass and of the whole call), the wall time
around it, the bytes moved, and move GB/s (read + write).  Then what a host without the call pays: a new builder over the final image set (meshes from the warm geometry
cache), ctl_builder_finalize and ctl_scene_create_ex with CTL_SCENE_FLATTEN (the tree from the warm cache).  One JSON line is appended to --out.  bench.py is not involved.
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

ENV, TEX, BIG, N_TEX = (4096, 2048), (1024, 1024), (2048, 2048), 16


def env_texels(seed):
    rs = np.random.RandomState(seed)
    return ((rs.randint(0, 1 << 24, size=(ENV[1], ENV[0])).astype(np.uint32) | np.uint32(0x404040)) | (rs.randint(124, 134, size=(ENV[1], ENV[0])).astype(np.uint32) << 24)).astype(np.uint32)


def tex_texels(size, seed):
    rs = np.random.RandomState(seed)
    return (rs.randint(0, 1 << 24, size=(size[1], size[0])).astype(np.uint32) | np.uint32(0xff000000)).astype(np.uint32)


def build(args, textures, env):
    """textures: list of (h, w) arrays, registered in order in front of the environment map; texture k >= 1 is read by mesh k where the scene has that many meshes"""
    desc = scenes.synthetic_sm_description(args.width, args.height, n_instances=args.instances, subdiv=args.subdiv)
    sc = api.DynamicScene()
    tex = [sc.add_image(t, api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_ANISOTROPIC) for t in textures]
    ei = sc.add_image(env, api.TEXEL_RGBE, api.WRAP_REPEAT, api.FILTER_BILINEAR)
    meshes = []
    for k, m in enumerate(desc["meshes"]):
        mat = api.plastic(api.image_texture(tex[k]), specular_reflectance=0.5) if 1 <= k < len(tex) else scenes._material_of(m["material"])
        meshes.append(sc.add_mesh(m["V"], m["F"], normals=m.get("N"), materials=[mat]))
    nodes = [sc.CreateNode(meshes[mi], None if xf is None else np.asarray(xf, np.float32)) for mi, xf in desc["nodes"]]
    for ni, rad in desc["lights"]:
        sc.CreateLight(nodes[ni], 0, rad)
    sc.setEnvironementMap(ei, (1.0, 1.0, 1.0))
    sc.setCamera(*desc["camera"])
    sc.UpdateScene()
    return sc


def edit(sc, scene, what, extra, big):
    if what == "append":
        sc.add_image(extra, api.TEXEL_RGBCOL, api.WRAP_REPEAT, api.FILTER_ANISOTROPIC)
    elif what == "replace":
        sc.replace_image(5, big)
    else:
        sc.remove_image(0)
    t = time.perf_counter(); sc.UpdateScene(); finalize_ms = (time.perf_counter() - t) * 1e3
    t = time.perf_counter(); st = scene.update_image_set(sc); wall_ms = (time.perf_counter() - t) * 1e3
    upd = st.pop("update")
    st.update(wall_ms=wall_ms, finalize_ms=finalize_ms, mask=upd["mask"], bytes_moved=st["texels_moved"] * 4)
    st["move_gb_s"] = 2.0 * st["bytes_moved"] / (st["move_ms"] * 1e-3) / 1e9 if st["move_ms"] > 0 else 0.0
    return st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920); ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--instances", type=int, default=2000); ap.add_argument("--subdiv", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    textures = [tex_texels(TEX, 10 + k) for k in range(N_TEX)]; env = env_texels(1); extra = tex_texels(TEX, 99); big = tex_texels(BIG, 98)
    out = dict(workload="synthetic-SM %dx%d, %d instances + %d textures %dx%d RGBCOL + env %dx%d RGBE" % ((args.width, args.height, args.instances, N_TEX) + TEX + ENV),
               move_access_bytes=4)
    runs = {"append": [], "replace": [], "remove": []}
    with tempfile.TemporaryDirectory() as cache:
        api.set_cache_dir(cache)
        for r in range(args.repeat + 1):       # the first round fills the caches and warms the kernels up; it is not counted
            t = time.perf_counter(); sc = build(args, textures, env); build_s = time.perf_counter() - t
            t = time.perf_counter(); scene = ctl.Scene(sc.desc, flatten=True); create_s = time.perf_counter() - t
            if r == 0:
                out["first_build_s"], out["first_create_s"] = build_s, create_s
            for what in ("append", "replace", "remove"):
                st = edit(sc, scene, what, extra, big)
                if r:
                    runs[what].append(st)
            if r == args.repeat:
                # the edited scene is the scene of the final description: nothing left to update, and a texture behind the removed one reads back as the host's pyramid
                out["update_after_is_empty"] = bool(scene.update(sc.desc) == 0)
                out["pool_matches_host_pyramid"] = bool(scene.read_image(4)["texels"].tobytes() == api.mip_pyramid_host(big, api.TEXEL_RGBCOL)["texels"].tobytes())
            del scene
        for what, rr in runs.items():
            out[what] = {k: float(np.median([x[k] for x in rr])) for k in rr[0]}
        # the host without the call: the final image set in a new builder, caches warm
        final = textures[1:5] + [big] + textures[6:] + [extra]
        t = time.perf_counter(); sc2 = build(args, [textures[0]] + final, env); sc2.remove_image(0); sc2.UpdateScene(); out["recreate_build_s"] = time.perf_counter() - t
        t = time.perf_counter(); fresh = ctl.Scene(sc2.desc, flatten=True); out["recreate_create_s"] = time.perf_counter() - t
        out["recreate_total_s"] = out["recreate_build_s"] + out["recreate_create_s"]
        del fresh
        api.set_cache_dir(None)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "a").write(line + "\n")


if __name__ == "__main__":
    main()
