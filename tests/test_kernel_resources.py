"""What the compiler makes of the two hot kernels under the flags of the library that ships (cudatracerlib_amd/build.py FLAGS), read from its own resource remarks
(-Rpass-analysis=kernel-resource-usage; device side only, no GPU needed):

  k_shade_basic                       no scratch, no spilled VGPR, and the waves per SIMD that shade_basic.hip declares (CTL_BASIC_SHADE_WAVES) — the kernel is
                                      latency-bound, and a spill reload goes through the vector-memory counter in front of which every queued load waits
  k_intersect_pair<1, false> and      no spilled VGPR, at least six waves per SIMD (their memory waits are only just hidden behind six), and no scratch but
  the flat k_intersect (closest, any) the overflow part of the traversal stack (kOverflowBytes below)
"""
import os
import re
import runpy
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cudatracerlib_amd", "csrc")
kOverflowBytes = 300   # bytes per lane of the traversal stack's overflow part, the only scratch the traversal kernels may have


def _resources(unit, tmp_path):
    """{mangled kernel name: {field: int}} of one translation unit"""
    mod = runpy.run_path(os.path.join(ROOT, "cudatracerlib_amd", "build.py"))
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc] + mod["FLAGS"] + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, unit), "-o", str(tmp_path / (unit + ".o"))]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"remark: (?:\s*)Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {}); continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def _declared_waves():
    text = open(os.path.join(CSRC, "shade_basic.hip")).read()
    return int(re.search(r"#define CTL_BASIC_SHADE_WAVES (\d+)", text).group(1))


def test_shade_basic_is_spill_free_at_its_declared_occupancy(tmp_path):
    res = _resources("shade_basic.hip", tmp_path)
    k = [v for n, v in res.items() if "k_shade_basic" in n]
    assert len(k) == 1, list(res)
    k = k[0]
    print(k)
    assert k["ScratchSize"] == 0, k
    assert k["VGPRs Spill"] == 0, k
    assert k["Occupancy"] == _declared_waves(), k
    assert _declared_waves() * k["LDS Size"] <= 160 * 1024, k   # one 256-lane workgroup per declared wave and SIMD: they fit a CU's LDS together


def test_traversal_kernels_keep_six_waves_and_only_the_overflow_stack_in_scratch(tmp_path):
    res = _resources("kernels.hip", tmp_path)
    def pick(pred):
        k = {n: v for n, v in res.items() if pred(n)}
        assert k, sorted(res)
        return k
    want = {}
    want.update(pick(lambda n: "k_intersect_pairILi1ELb0EE" in n))                       # k_intersect_pair<format 1, ALPHA = false>
    want.update(pick(lambda n: re.search(r"k_intersectILb[01]ELb0ELi1ELb0EE", n)))       # the flat k_intersect<ANY = false / true, COUNT = false, format 1, ALPHA = false>
    assert len(want) == 3, sorted(want)
    for n, k in want.items():
        print(n, k)
        assert k["VGPRs Spill"] == 0, (n, k)
        assert k["Occupancy"] >= 6, (n, k)
        assert k["ScratchSize"] == kOverflowBytes, (n, k)
