"""NonLocalMeans filter and pixel-variance timing: synthetic_sm at 1920x1080, one JSON line per configuration.

    python tools/nlm_bench.py [--configs filter,variance,variance_per_launch,apply] [--passes 20] [--warmup 3] [--steps 20] [--config-timeout 300]

Each configuration runs in a child process of its own under a time limit:
  filter    `passes` passes with the variance switch on, then `steps` applications of the filter through the tracer handle after `warmup`: median device time of the
            NonLocalMeans kernel (HIP events around it, Image.lastFilterMs: no D2H of the display image), at the reference's settings and at sigma2_scale = 1 / passes
            (where the filter acts on so early a frame), next to the time of one render pass of the same run
  variance  ms per pass of DoPasses(passes) with the variance switch off and on, same process, same scene (off first, median of 3 calls each): what keeping the
            PixelVarianceBuffer up to date costs — the update inside the batch resolve and its second stage
  variance_per_launch  the same with OrderedAccumulationMaxMB too small for the variance update's second stage: the switch then renders one pass per launch (the fallback
            of tracers without the stage, and the first design of the switch)
  apply     the filter applied `steps` times and nothing reported: the workload for a profiler (rocprofv3 --kernel-trace --stats, or counters in a run of their own)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080


def setup(variance_on):
    sys.path.insert(0, ROOT)
    import cudatracerlib_amd as ctl
    from cudatracerlib_amd import scenes
    sc = scenes.synthetic_sm(W, H)
    scene = ctl.Scene(sc.desc, flatten=True)
    tr = ctl.WavefrontPathTracer()
    tr.Resize(W, H)
    tr.InitializeScene(scene)
    if variance_on:
        tr.setPixelVariance(True)
    return ctl, sc, scene, tr, ctl.Image(W, H)


def ms_per_pass(tr, img, passes, steps):
    import numpy as np
    tr.reservePasses(passes)
    tr.DoPasses(img, passes, new_trace=True)   # warm-up: allocations, first launches
    t = []
    for _ in range(steps):
        tr.DoPasses(img, passes, new_trace=True)
        t.append(1e3 * tr.stats().seconds_last_pass / passes)
    return float(np.median(t))


def run_config(config, passes, warmup, steps):
    import numpy as np
    base = {"scene": "synthetic_sm", "width": W, "height": H, "config": config, "passes": passes}
    if config in ("variance", "variance_per_launch"):
        ctl, sc, scene, tr, img = setup(False)
        if config == "variance_per_launch":   # room for the batch's stage (16 B per pixel and pass) but not for the second one the variance update needs: the fallback, one launch per pass
            stage_mb = W * H * passes * 16 / 2 ** 20
            tr.getParameters().setValue("OrderedAccumulationMaxMB", int(1.5 * stage_mb))
        off = ms_per_pass(tr, img, passes, 3)
        tr.setPixelVariance(True)
        on = ms_per_pass(tr, img, passes, 3)
        base.update({"ms_per_pass_variance_off": off, "ms_per_pass_variance_on": on, "variance_cost_ms_per_pass": on - off, "variance_cost_share": (on - off) / off})
        print(json.dumps(base), flush=True)
        return
    ctl, sc, scene, tr, img = setup(True)
    pass_ms = ms_per_pass(tr, img, passes, 1)
    img.applyImagePipeline(1.0 / passes, None, ctl.api.tonemap())   # (leaves the unfiltered RGBE plane: copySamplesToFiltered)
    unfiltered = img.getFilteredData()
    for k, s2 in ((0.45, 0.005), (0.45, 1.0 / passes)):
        flt = ctl.api.nlm_filter(k, s2)
        t = []
        for i in range(warmup + steps):
            img.applyImagePipeline(1.0 / passes, flt, None, tracer=tr)
            if i >= warmup:
                t.append(img.lastFilterMs())
        if config == "apply":
            continue
        changed = float((img.getFilteredData() != unfiltered).mean())
        out = dict(base, k=k, sigma2_scale=s2, steps=steps, warmup=warmup, ms_filter=float(np.median(t)), ms_filter_min=float(np.min(t)), ms_filter_max=float(np.max(t)),
                   ms_render_pass_variance_on=pass_ms, pixels_changed_share=changed)
        out["filter_in_render_passes"] = out["ms_filter"] / pass_ms
        out["pair_terms_per_s"] = W * H * 169 * 49 / (out["ms_filter"] * 1e-3)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="filter,variance,variance_per_launch")
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--config-timeout", type=int, default=300)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        run_config(a.child, a.passes, a.warmup, a.steps)
        return 0
    for config in a.configs.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", config, "--passes", str(a.passes), "--warmup", str(a.warmup), "--steps", str(a.steps)],
                               timeout=a.config_timeout)
        except subprocess.TimeoutExpired:
            print(json.dumps({"config": config, "error": "timeout"}), flush=True)
            return 1
        if r.returncode != 0:   # a failed child ends the run: nothing more is started on the device
            print(json.dumps({"config": config, "error": "exit %d" % r.returncode}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
