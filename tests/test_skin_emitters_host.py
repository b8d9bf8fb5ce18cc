"""Emissive skins, the host half: ctl_shape_sets_host — the yardstick of the shape sets ctl_scene_animate_mesh recomputes for a mesh bound with CTL_SKIN_AREA_LIGHTS,
the functions of csrc/shape_set.h on the host — against the light tables of a description updated on the host to the same pose (DynamicScene.UpdateMesh of the skin
yardstick's vertices: scene_builder::recalculate_shape_set through the same header); the exported symbols; the no-device answer.  Cases E1..E6:
tests/skin_emitter_cases.py.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from cudatracerlib_amd import api
from skin_emitter_cases import CASES, emitter_case, tables_of, assert_tables_equal, float_masks, light_table

NEW = ("ctl_scene_bind_skin_ex", "ctl_scene_get_shape_set_ms", "ctl_scene_read_lights", "ctl_shape_sets_host")


def test_the_new_symbols_are_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctl_amd.h")).read()
    for name in NEW:
        assert getattr(api.lib, name) is not None
        assert "int %s(" % name in header
    assert "CTL_SKIN_AREA_LIGHTS = 1" in header and api.SKIN_AREA_LIGHTS == 1


@pytest.mark.parametrize("name", CASES)
def test_yardstick_equals_the_host_updated_description(name):
    K, Y, bent, S = emitter_case(name)
    d = K["plain"].desc
    assert_tables_equal(S, tables_of(bent.desc), d, K["mesh"], name)
    # the pose changed the sets, and nothing else: the rest description's tables outside the float words of the posed sets
    rest = tables_of(d)
    ml, ma = float_masks(d, K["mesh"])
    n4 = len(ma) * 4
    assert np.array_equal(S["lights"][~ml], rest["lights"][~ml]) and np.array_equal(S["anim"][:n4].view(np.uint32)[~ma], rest["anim"][:n4].view(np.uint32)[~ma])
    assert not np.array_equal(S["anim"][:n4].view(np.uint32)[ma], rest["anim"][:n4].view(np.uint32)[ma])
    L = light_table(d)
    for li in K["lights"]:
        cdf = S["anim"][int(L[li, 4]): int(L[li, 4]) + 4 * (int(L[li, 7]) + 1)].view(np.float32)
        area = S["lights"][li, 6:7].view(np.float32)[0]
        if name == "E6":
            assert np.isnan(area) and np.isnan(cdf).all()        # collapsed triangles: a NaN area poisons the running sum, and 0 / NaN the first entry
        else:
            assert area > 0 and cdf[0] == 0 and cdf[-1] == 1 and (np.diff(cdf) >= 0).all()


def test_yardstick_of_the_rest_arrays_is_the_description():
    """handed the description's own arrays, the yardstick recalculates what the builder calculated: byte for byte"""
    from scene_deform_cases import mesh_arrays
    K, _, _, _ = emitter_case("E3")
    d = K["plain"].desc
    A = mesh_arrays(d, K["mesh"])
    S = api.shape_sets_host(d, K["mesh"], A["tri"], A["woop"])
    rest = tables_of(d)
    assert np.array_equal(S["lights"], rest["lights"]) and np.array_equal(S["anim"], rest["anim"])


def test_yardstick_refusals():
    K, Y, _, _ = emitter_case("E1")
    d = K["plain"].desc
    L = np.zeros((d.n_lights_buf, C.sizeof(api.ctl_light) // 4), np.uint32); A = np.zeros(d.n_anim_bytes, np.uint8)
    T, W = Y["tri"], Y["woop"]
    assert api.lib.ctl_shape_sets_host(C.addressof(d), d.n_meshes, T.ctypes.data, W.ctypes.data, L.ctypes.data, A.ctypes.data) == api.ERR_INVALID
    assert api.lib.ctl_shape_sets_host(C.addressof(d), K["mesh"], None, W.ctypes.data, L.ctypes.data, A.ctypes.data) == api.ERR_INVALID
    assert api.lib.ctl_shape_sets_host(None, K["mesh"], T.ctypes.data, W.ctypes.data, L.ctypes.data, A.ctypes.data) == api.ERR_INVALID


def test_the_device_calls_answer_no_device_first():
    """without a device the scene calls report CTL_ERR_NO_DEVICE before they look at their arguments (a null scene and unknown flag bits among them); with one, a null
    scene is invalid"""
    want = api.ERR_NO_DEVICE if api.device_count() < 1 else api.ERR_INVALID
    assert api.lib.ctl_scene_bind_skin_ex(None, 0, None, None, 0, None, 0, None, None, 0, api.SKIN_AREA_LIGHTS) == want
    assert api.lib.ctl_scene_bind_skin_ex(None, 0, None, None, 0, None, 0, None, None, 0, 0xfffffffe) == want
    assert api.lib.ctl_scene_read_lights(None, None, 0, None, 0) == want
    assert api.lib.ctl_scene_get_shape_set_ms(None, None) == api.ERR_INVALID
