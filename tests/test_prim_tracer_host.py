"""The PrimTracer plugin ("direct") on a host without a GPU: the C ABI knows its two names and refuses for want of a device, not for want of a plugin;
the Python mirror carries the reference's drawing modes (Integrators/PrimTracer.h:7)."""
import ctypes as C

import pytest


def test_prim_tracer_names_need_a_device(ctl):
    if ctl.device_count() > 0:
        pytest.skip("a device is present")
    h = C.c_void_p()
    for name in (b"PrimTracer", b"direct"):   # main.cpp:91-92 maps "direct" to PrimTracer
        assert ctl.lib.ctl_tracer_create(name, C.byref(h)) == -2, name   # CTL_ERR_NO_DEVICE, not CTL_ERR_UNSUPPORTED (-5)
        assert b"no HIP device" in ctl.lib.ctl_last_error()
    assert ctl.lib.ctl_tracer_create(b"BDPT", C.byref(h)) == -5   # other estimators stay out


def test_draw_modes_are_the_references(ctl):
    assert ctl.PathTrace_DrawMode == ("linear_depth", "D3D_depth", "v_absdot_n_geo", "v_dot_n_geo", "v_dot_n_shade", "n_geo_colored", "n_shade_colored", "uv",
                                      "bary_coords", "first_Le", "first_f", "first_f_direct", "first_non_delta_Le", "first_non_delta_f", "first_non_delta_f_direct")
    assert issubclass(ctl.PrimTracer, ctl.WavefrontPathTracer) and ctl.PrimTracer.PLUGIN == b"PrimTracer"
