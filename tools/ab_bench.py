#!/usr/bin/env python3
"""A/B of library variants on one box: python tools/ab_bench.py OUT_DIR RUNS lib1,lib2,... [bench args]
Alternates the libraries, RUNS rounds, each bench run under its own time limit; the first failure ends the job."""
import json, os, subprocess, sys, statistics

out, runs, libs = os.path.abspath(sys.argv[1]), int(sys.argv[2]), sys.argv[3].split(",")
extra = sys.argv[4:]
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.makedirs(out, exist_ok=True)   # ab.txt is appended to there
log = open(os.path.join(out, "ab.txt"), "a")
def say(s):
    print(s, flush=True); log.write(s + "\n"); log.flush()
say("# bench.py --steps 20 --warmup 5 --full --no-cpu-baseline %s; libraries alternating on one box" % " ".join(extra))
res = {l: [] for l in libs}
for i in range(runs):
    for l in libs:
        env = dict(os.environ, CTL_AMD_LIB=os.path.join(root, "cudatracerlib_amd", "libctl_%s.so" % l), TMPDIR="/tmp")
        cmd = ["timeout", "-k", "10", "420", sys.executable, "bench.py", "--steps", "20", "--warmup", "5", "--full", "--no-cpu-baseline"] + extra
        p = subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True)
        if p.returncode != 0:
            say("FAILED lib %s run %d: exit %d\n%s" % (l, i, p.returncode, p.stderr[-1500:])); sys.exit(p.returncode if p.returncode > 0 else 1)
        b = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
        rf = b["roofline"]
        r = dict(value=b["value"], ms_per_step=b["ms_per_step"], ms_shade=round(rf["ms_shade"] / b["steps"], 4), ms_intersect=round(rf["ms_intersect"] / b["steps"], 4))
        res[l].append(r)
        say("%-8s run %d  %s" % (l, i, json.dumps(r)))
base = libs[0]
for l in libs:
    v = [r["value"] for r in res[l]]
    say("%-8s value min %.1f median %.1f max %.1f   median ratio to %s: %.4f   shade median %.4f ms  intersect median %.4f ms" % (
        l, min(v), statistics.median(v), max(v), base, statistics.median(v) / statistics.median([r["value"] for r in res[base]]),
        statistics.median([r["ms_shade"] for r in res[l]]), statistics.median([r["ms_intersect"] for r in res[l]])))
