"""Participating media, the two plugins side by side: scenes.fog_box and scenes.smoke_box at 1920 x 1080, MaxPathLength 8 — the PathTracer plugin (the megakernel's
media kernels) and the WavefrontPathTracer with ParticipatingMedia = true (k_medium_stage + the media build of the shade kernel), each after a warm-up call, in ms per
pass and Mrays/s; then the share of pixels in which the two plugins' frames are bit-equal on the scenes of the GPU tests.  RESULTS.md "Participating media in the
wavefront" records one run.

    python tools/wavefront_media_probe.py [passes]      (default 32)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cudatracerlib_amd as ctl
from cudatracerlib_amd import scenes

W, H, DEPTH = 1920, 1080, 8
PASSES = int(sys.argv[1]) if len(sys.argv) > 1 else 32


def tracer(plugin, w, h, depth, rr=5):
    tr = ctl.PathTracer() if plugin == "PathTracer" else ctl.WavefrontPathTracer()
    p = tr.getParameters(); p.setValue("MaxPathLength", depth); p.setValue("RRStartDepth", rr)
    if plugin != "PathTracer":
        p.setValue("ParticipatingMedia", True)
    tr.Resize(w, h)
    return tr


for name, sc in (("fog_box", scenes.fog_box(W, H)), ("smoke_box", scenes.smoke_box(W, H))):
    scene = ctl.Scene(sc.desc, flatten=True)
    ms = {}
    for plugin in ("PathTracer", "WavefrontPathTracer"):
        tr = tracer(plugin, W, H, DEPTH); tr.InitializeScene(scene)
        img = ctl.Image(W, H)
        tr.DoPasses(img, PASSES, new_trace=True)   # warm-up: queues, stage and table ring are allocated here
        t = time.perf_counter(); tr.DoPasses(img, PASSES, new_trace=False); dt = time.perf_counter() - t
        st = tr.stats()
        ms[plugin] = dt * 1e3 / PASSES
        print("%-9s %-19s %7.2f ms per pass  %7.0f Mrays/s  (%d passes, %.1f rays per pixel and pass; shade + medium stage %.2f ms per pass)"
              % (name, plugin, ms[plugin], st.rays_last_pass / dt / 1e6, PASSES, st.rays_last_pass / PASSES / (W * H), st.ms_shade / PASSES), flush=True)
        del tr, img
    print("%-9s wavefront / megakernel time per pass: %.2f" % (name, ms["WavefrontPathTracer"] / ms["PathTracer"]), flush=True)

# the two plugins' frames on the test scenes, the tracers' own tables (both start the same stream): share of bit-equal pixels
small = [("fog_box(48, 32) isotropic", scenes.fog_box(48, 32), 48, 32, 6, 3), ("fog_box(48, 32) hg 0.7 coloured", scenes.fog_box(48, 32, sigma_a=(0.0004, 0.0008, 0.0002), sigma_s=(0.0012, 0.002, 0.003), phase=ctl.api.phase_hg(0.7)), 48, 32, 6, 3),
         ("smoke_box(24, 16) single grid", scenes.smoke_box(24, 16, sigma_a=0.0005, sigma_s=0.004), 24, 16, 4, 2),
         ("smoke_box(24, 16) three grids", scenes.smoke_box(24, 16, sigma_a=0.0005, sigma_s=0.004, three_grid_dims=((2, 3, 2), (4, 2, 3))), 24, 16, 4, 2)]
for name, sc, w, h, depth, rr in small:
    scene = ctl.Scene(sc.desc, flatten=True)
    frames = []
    for plugin in ("PathTracer", "WavefrontPathTracer"):
        tr = tracer(plugin, w, h, depth, rr); tr.InitializeScene(scene)
        if plugin != "PathTracer":
            tr.getParameters().setValue("PassBatch", 1)
        img = ctl.Image(w, h)
        tr.DoPasses(img, 2, new_trace=True)
        frames.append(img.getPixelData())
    a, b = frames
    print("%-32s %6.2f %% of pixels bit-equal between the plugins (2 passes)" % (name, 100 * (a.view(np.uint32) == b.view(np.uint32)).all(axis=2).mean()), flush=True)
