"""ms per pass of scenes.fog_box at 512 x 512 on the PathTracer plugin, with its volume (k_path_trace_media) and without (the Cornell box alone, k_path_trace): both
tracers warmed up, then six alternating batches of 500 passes each (about a second of work), a host clock around work that ends in a device synchronise; median, minimum and maximum per pass.
Prints one JSON line (RESULTS.md "Participating media").  Needs a GPU.

    python tools/fog_bench.py
"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import cudatracerlib_amd as ctl
from cudatracerlib_amd import scenes

W = H = 512
N = 500   # ~1 s per timed batch
fog = scenes.fog_box(W, H)
clear = scenes.cornell_box(W, H)
runs = {}
for name, sc in (("fog", fog), ("clear", clear)):
    scene = ctl.Scene(sc.desc, flatten=True)
    tr = ctl.PathTracer(); tr.Resize(W, H); tr.InitializeScene(scene)
    img = ctl.Image(W, H)
    tr.DoPasses(img, 20, True)   # warm-up
    runs[name] = (scene, tr, img, [])
for rep in range(6):
    for name in ("fog", "clear"):
        scene, tr, img, ms = runs[name]
        ctl.lib.ctl_device_synchronize()
        t = time.perf_counter()
        tr.DoPasses(img, N, rep == 0)
        ctl.lib.ctl_device_synchronize()
        ms.append(1e3 * (time.perf_counter() - t) / N)
out = {}
for name in runs:
    ms = runs[name][3]
    st = runs[name][1].stats()
    out[name] = dict(ms_per_pass_median=float(np.median(ms)), ms_per_pass_min=float(min(ms)), ms_per_pass_max=float(max(ms)), rays_last_pass=int(st.rays_last_pass))
print(json.dumps(out))
