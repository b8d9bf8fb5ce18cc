"""PrimTracer timing: synthetic_sm at 1920x1080, one JSON line per drawing mode.

    python tools/prim_bench.py [--modes n_geo_colored,first_f,first_f_direct] [--warmup 3] [--steps 10] [--mode-timeout 300]

Each mode runs in a child process of its own under a time limit: warm-up passes, then `steps` single passes timed by the tracer
(seconds_last_pass, rays_last_pass and the ms_raygen / ms_intersect / ms_shade kernel times of its event timers), reported as medians.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_mode(mode, warmup, steps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import cudatracerlib_amd as ctl
    from cudatracerlib_amd import scenes
    w, h = 1920, 1080
    sc = scenes.synthetic_sm(w, h)
    scene = ctl.Scene(sc.desc, flatten=True)
    tr = ctl.PrimTracer()
    tr.getParameters().setValue("DrawingMode", mode)
    tr.Resize(w, h)
    tr.InitializeScene(scene)
    img = ctl.Image(w, h)
    for _ in range(warmup):
        tr.DoPass(img)
    rec = {k: [] for k in ("ms_pass", "rays", "ms_raygen", "ms_intersect", "ms_shade")}
    for _ in range(steps):
        tr.DoPass(img)
        s = tr.stats()
        rec["ms_pass"].append(1e3 * s.seconds_last_pass); rec["rays"].append(s.rays_last_pass)
        rec["ms_raygen"].append(s.ms_raygen); rec["ms_intersect"].append(s.ms_intersect); rec["ms_shade"].append(s.ms_shade)
    out = {"scene": "synthetic_sm", "width": w, "height": h, "mode": mode, "steps": steps, "warmup": warmup}
    out.update({k: float(np.median(v)) for k, v in rec.items()})
    out["rays"] = int(out["rays"])
    out["grays_per_s"] = out["rays"] / out["ms_pass"] / 1e6
    out["intersect_share"] = out["ms_intersect"] / out["ms_pass"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="n_geo_colored,first_f,first_f_direct")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--mode-timeout", type=int, default=300)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        run_mode(a.child, a.warmup, a.steps)
        return 0
    for mode in a.modes.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--warmup", str(a.warmup), "--steps", str(a.steps)],
                               timeout=a.mode_timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"mode": mode, "error": "timeout"}), flush=True)
            return 1
        if r.returncode != 0:   # a failed child ends the run: nothing more is started on the device
            print(json.dumps({"mode": mode, "error": "exit %d" % r.returncode}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
