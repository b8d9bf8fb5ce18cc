"""First-hit texture filtering in the wavefront, measured: scenes.synthetic_bathroom at the benchmark's resolution and depth (1920 x 1080, MaxPathLength 8), its images
(built FILTER_BILINEAR, which KernelMIPMap::eval answers from level 0) set to FILTER_ANISOTROPIC, the reference's MIPMap default, in the description before the scene
is created.  Per configuration one warm-up call, then REPEATS timed DoPasses calls of PASSES passes each; ms per pass and the shade stage's ms per pass
(ctl_tracer_get_stats) as median [min .. max] over the repeats:
  * WavefrontPathTracer, TextureFiltering off and on, at depth 8 — and at MaxPathLength 1, where the shade stage is the depth-1 launch (plus the last finalize and the
    resolve of the ordered accumulation, the same in both): the cost of k_shade_full_partials against the class launches it replaces;
  * the same one-bounce pass with ShadeByModelClass = false (k_shade_full): what the unclassed launch costs without the partials;
  * the PathTracer plugin on the same scene, for the side-by-side.
Then the share of bit-equal pixels between the two plugins on the ground scene of tests/test_gpu_texture_filtering.py, per filter mode.
RESULTS.md "First-hit texture filtering in the wavefront" records one run.

    python tools/texture_filtering_probe.py [passes] [repeats]      (default 16, 5)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import cudatracerlib_amd as ctl
from cudatracerlib_amd import api, scenes

W, H, DEPTH = 1920, 1080, 8
PASSES = int(sys.argv[1]) if len(sys.argv) > 1 else 16
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def measure(scene, plugin, depth, filtering, by_class=True):
    tr = ctl.PathTracer() if plugin == "PathTracer" else ctl.WavefrontPathTracer()
    p = tr.getParameters(); p.setValue("MaxPathLength", depth)
    if plugin != "PathTracer":
        p.setValue("TextureFiltering", filtering); p.setValue("ShadeByModelClass", by_class)
    tr.Resize(W, H); tr.InitializeScene(scene)
    img = ctl.Image(W, H)
    tr.DoPasses(img, PASSES, new_trace=True)   # warm-up: queues, stage and table ring are allocated here
    total, shade = [], []
    for _ in range(REPEATS):
        t = time.perf_counter(); tr.DoPasses(img, PASSES, new_trace=False); dt = time.perf_counter() - t
        total.append(dt * 1e3 / PASSES); shade.append(tr.stats().ms_shade / PASSES)   # (the stage times are those of the last call)
    return total, shade


def show(v):
    return "%7.3f [%7.3f .. %7.3f]" % (float(np.median(v)), min(v), max(v))


sc = scenes.synthetic_bathroom(W, H)
for i in range(sc.desc.n_images):
    sc.desc.images[i].filter_mode = api.FILTER_ANISOTROPIC
scene = ctl.Scene(sc.desc, flatten=True)
print("synthetic-bathroom %d x %d, %d images set to FILTER_ANISOTROPIC; %d passes per call, %d timed calls; ms per pass: median [min .. max]" % (W, H, sc.desc.n_images, PASSES, REPEATS), flush=True)
# (the last row repeats the first: drift over the run.  ShadeByModelClass = false at depth 1: k_shade_full, the unclassed build without partials)
for plugin, depth, filtering, by_class in (("WavefrontPathTracer", DEPTH, False, True), ("WavefrontPathTracer", DEPTH, True, True), ("WavefrontPathTracer", 1, False, True),
                                           ("WavefrontPathTracer", 1, True, True), ("WavefrontPathTracer", 1, False, False), ("PathTracer", DEPTH, None, True), ("WavefrontPathTracer", DEPTH, False, True)):
    total, shade = measure(scene, plugin, depth, filtering, by_class)
    print("%-19s MaxPathLength %d  TextureFiltering %-3s  %-9s  pass %s   shade stage %s" % (plugin, depth, {None: "-", False: "off", True: "on"}[filtering], "by class" if by_class else "unclassed", show(total), show(shade)), flush=True)

import filtering_scenes as F
for filter_mode in ("anisotropic", "trilinear", "point"):
    g = F.ground_scene("anisotropic" if filter_mode == "point" else filter_mode)
    if filter_mode == "point":      # partials change nothing there: the plugins' agreement apart from the filtering
        g.desc.images[0].filter_mode = api.FILTER_POINT
    s = ctl.Scene(g.desc, flatten=True)
    frames = []
    for plugin in ("PathTracer", "WavefrontPathTracer"):
        tr = ctl.PathTracer() if plugin == "PathTracer" else ctl.WavefrontPathTracer()
        p = tr.getParameters(); p.setValue("MaxPathLength", 3)
        if plugin != "PathTracer":
            p.setValue("TextureFiltering", True); p.setValue("PassBatch", 1)
        tr.Resize(F.W, F.H); tr.InitializeScene(s)
        img = ctl.Image(F.W, F.H)
        tr.DoPasses(img, 2, new_trace=True)
        frames.append(img.getPixelData())
    a, b = frames
    print("ground %-11s %6.2f %% of pixels bit-equal between the plugins (2 passes)" % (filter_mode, 100 * (a.view(np.uint32) == b.view(np.uint32)).all(axis=2).mean()), flush=True)
