"""Participating media in the wavefront, the host half (no GPU): what the compiler makes of the kernels under the flags of the library that ships, read from its
resource remarks as tests/test_kernel_resources.py and tests/test_volume_grid_host.py read them.

  * the four new kernels exist for gfx950: k_medium_stage<false> / <true> (csrc/medium_stage.hip), k_shade_full_media, k_shade_full_media_grid;
  * every kernel of the wavefront's own translation units that existed before the medium path — the fourteen shade builds of shade_kernel.inc, which gained the
    CTL_SHADE_MEDIA conditionals, and the 39 kernels of kernels.hip, which take the path queues that gained path_soa::mrec — reports the figures it reported on the
    commit before: VGPRs, AGPRs, scratch, waves per SIMD, spilled VGPRs, LDS (tests/golden/wavefront_kernel_resources.json, recorded there with the same remarks).
    A build without CTL_SHADE_MEDIA must keep its code."""
import json
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

from test_kernel_resources import _resources, ROOT

FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "wavefront_kernel_resources.json")))
NEW_UNITS = ("medium_stage.hip", "shade_full_media.hip", "shade_full_media_grid.hip")


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    """{unit: {kernel: {field: int}}}: every unit compiled once (device side only), a few at a time"""
    units = sorted(FIXTURE["units"]) + list(NEW_UNITS)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        got = list(pool.map(lambda u: _resources(u, tmp_path_factory.mktemp(u.replace(".", "_"))), units))
    return dict(zip(units, got))


def test_the_new_kernels_exist_for_gfx950(remarks):
    pick = lambda unit, part: [v for n, v in remarks[unit].items() if n.startswith("_ZN3ctl") and part in n]
    stage, stage_grid = pick("medium_stage.hip", "14k_medium_stageILb0EE"), pick("medium_stage.hip", "14k_medium_stageILb1EE")
    shade, shade_grid = pick("shade_full_media.hip", "18k_shade_full_mediaE"), pick("shade_full_media_grid.hip", "23k_shade_full_media_gridE")
    for name, k in (("k_medium_stage<false>", stage), ("k_medium_stage<true>", stage_grid), ("k_shade_full_media", shade), ("k_shade_full_media_grid", shade_grid)):
        assert len(k) == 1, (name, sorted(remarks))
        print(name, k[0])
        assert k[0]["Occupancy"] >= 1 and k[0]["VGPRs"] > 0
    # the stage keeps its registers: nothing of its state goes through scratch as a spilled VGPR
    assert stage[0]["VGPRs Spill"] == 0 and stage_grid[0]["VGPRs Spill"] == 0
    # the media builds are built like k_shade_full: 1024 lanes, four waves per SIMD
    assert shade[0]["Occupancy"] == 4 and shade_grid[0]["Occupancy"] == 4


@pytest.mark.parametrize("unit", sorted(FIXTURE["units"]))
def test_the_kernels_that_existed_keep_their_figures(remarks, unit):
    fields = FIXTURE["fields"]
    want = FIXTURE["units"][unit]
    got = {n: [v[f] for f in fields] for n, v in remarks[unit].items() if n.startswith("_ZN3ctl")}
    assert sorted(got) == sorted(want), sorted(set(got) ^ set(want))
    moved = {n: (dict(zip(fields, want[n])), dict(zip(fields, got[n]))) for n in want if got[n] != want[n]}
    assert not moved, moved
