"""Images updated in place, the host half: ctl_builder_update_image — DynamicScene::ReloadTextures for a caller that supplies the bitmap, the yardstick of
ctl_scene_update_image — and ctl_mip_pyramid_host, the pyramid a scene keeps of an image.  The pyramid against a numpy restatement (tests/image_update_cases.py); a builder
that registered image X and was updated to Y against a builder that registered Y from the start, byte for byte; the refusals; the exported symbols; the no-device answer of
the device calls.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from cudatracerlib_amd import api
import image_update_cases as K

NEW = ("ctl_builder_update_image", "ctl_mip_pyramid_host", "ctl_scene_update_image", "ctl_scene_read_image")


def test_the_new_symbols_are_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctl_amd.h")).read()
    for name in NEW:
        assert getattr(api.lib, name) is not None
        assert "int %s(" % name in header
    assert "CTL_IMAGE_TEXELS_DEVICE = 1" in header and api.IMAGE_TEXELS_DEVICE == 1
    assert C.sizeof(api.ctl_scene_image_stats) == 36


@pytest.mark.parametrize("texel_type", [api.TEXEL_RGBE, api.TEXEL_RGBCOL])
@pytest.mark.parametrize("size", K.PYRAMID_SIZES)
def test_pyramid_against_numpy(size, texel_type):
    w, h = size
    t = K.rgbe_texels(w, h, 3 + w) if texel_type == api.TEXEL_RGBE else K.rgbcol_texels(w, h, 5 + w)
    if texel_type == api.TEXEL_RGBE and w * h >= 64:
        e = t >> 24
        assert (e == 0).any() and ((e >= 1) & (e <= 3)).any() and (e >= 253).any()      # zero-exponent texels and exponents at both ends
    got, want = api.mip_pyramid_host(t, texel_type), K.numpy_pyramid(t, texel_type)
    assert got["levels"] == want["levels"] == 1 + int(np.floor(np.log2(min(w, h))))
    assert np.array_equal(got["offsets"], want["offsets"])
    assert got["texels"].tobytes() == want["texels"].tobytes()
    assert np.array_equal(got["texels"][:w * h], t.reshape(-1))                          # level 0 is the image


def test_pyramid_refusals():
    t = K.rgbcol_texels(4, 4, 1)
    m = api.ctl_mipmap(); m.texels = t.ctypes.data; m.width = m.height = 4; m.texel_type = api.TEXEL_RGBCOL
    levels = api.u32(); off = (api.u32 * 15)(); out = np.zeros(21, np.uint32)
    assert api.lib.ctl_mip_pyramid_host(None, out.ctypes.data, 21, C.byref(levels), off) == api.ERR_INVALID
    assert api.lib.ctl_mip_pyramid_host(C.addressof(m), out.ctypes.data, 20, C.byref(levels), off) == api.ERR_INVALID      # 16 + 4 + 1 texels
    assert not out.any()
    assert api.lib.ctl_mip_pyramid_host(C.addressof(m), out.ctypes.data, 21, C.byref(levels), off) == 0 and levels.value == 3 and list(off[:3]) == [16, 20, 0]
    m.texel_type = 2
    assert api.lib.ctl_mip_pyramid_host(C.addressof(m), out.ctypes.data, 21, C.byref(levels), off) == api.ERR_INVALID
    m.texel_type = api.TEXEL_RGBCOL; m.texels = None
    assert api.lib.ctl_mip_pyramid_host(C.addressof(m), out.ctypes.data, 21, C.byref(levels), off) == api.ERR_INVALID


def _pair(kind, wrap=api.WRAP_REPEAT):
    """(builder A: registered X, updated to Y, finalized; builder B: registered Y) and the images that were updated"""
    tw, th, ew, eh = 16, 8, 12, 7
    X = dict(tex=K.bright_rgbcol(tw, th, 1), env=K.bright_rgbe(ew, eh, 2))
    Y = dict(tex=K.bright_rgbcol(tw, th, 11) & np.uint32(0xff3f7fff), env=K.bright_rgbe(ew, eh, 12))      # another average: the red and green bytes are cut
    if kind == "both":
        X["tex"], Y["tex"] = K.bright_rgbe(tw, th, 3), K.bright_rgbe(tw, th, 13)
    tt = api.TEXEL_RGBE if kind == "both" else api.TEXEL_RGBCOL
    A = K.floor_scene(kind, X["tex"], X["env"], tex_type=tt, wrap=wrap)
    B = K.floor_scene(kind, Y["tex"], Y["env"], tex_type=tt, wrap=wrap)
    return A, B, Y


@pytest.mark.parametrize("wrap", [api.WRAP_REPEAT, api.WRAP_CLAMP])
@pytest.mark.parametrize("kind", ["plastic", "roughcoating", "env", "both", "floor_env"])
def test_updated_builder_equals_a_builder_that_had_the_image_from_the_start(kind, wrap):
    A, B, Y = _pair(kind, wrap)
    before = K.desc_bytes(A.desc); want = K.desc_bytes(B.desc)
    differing = [k for k in want if not np.array_equal(before[k], want[k])]
    # the update has something to do in every part it is supposed to reach
    assert ("materials" in differing) == (kind != "env") and (("lights" in differing) and ("anim" in differing)) == (kind != "plastic" and kind != "roughcoating")
    done = set()
    for key, idx in A.images.items():
        if idx in done:
            continue
        done.add(idx)
        A.update_image(idx, Y["tex" if (key == "tex" or kind == "both") else "env"])
    A.UpdateScene()
    got = K.desc_bytes(A.desc)
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), (kind, k, int((got[k] != want[k]).sum()))
    assert api.scene_desc_diff(A.desc, B.desc) == 0


def test_environment_tables_follow_without_a_finalize():
    """the CDFs and the normalization are rewritten by the call itself, where they stand: the description a finalize handed out before points at them"""
    A, B, Y = _pair("env")
    d = A.desc
    A.update_image(A.images["env"], Y["env"])
    got, want = K.light_tables(d), K.light_tables(B.desc)
    assert np.array_equal(got["anim"], want["anim"]) and np.array_equal(got["lights"], want["lights"])


def test_refusals_leave_the_builder_as_it_was():
    A, _, Y = _pair("both")
    d = A.desc
    before = {k: v.copy() for k, v in K.desc_bytes(d).items()}
    idx = A.images["tex"]
    t = np.ascontiguousarray(Y["tex"], np.uint32); h, w = t.shape
    calls = [(None, idx, t.ctypes.data, w, h), (A._h, d.n_images, t.ctypes.data, w, h), (A._h, 0xffffffff, t.ctypes.data, w, h), (A._h, idx, None, w, h),
             (A._h, idx, t.ctypes.data, w + 1, h), (A._h, idx, t.ctypes.data, w, h - 1), (A._h, idx, t.ctypes.data, h, w), (A._h, idx, t.ctypes.data, 0, 0)]
    for b, i, p, ww, hh in calls:
        assert api.lib.ctl_builder_update_image(b, api.u32(i), p, api.u32(ww), api.u32(hh)) == api.ERR_INVALID, (i, ww, hh)
        assert api.lib.ctl_last_error()
        after = K.desc_bytes(d)
        assert all(np.array_equal(before[k], after[k]) for k in before)
    with pytest.raises(api.CtlError) as e:
        A.update_image(idx, t[:, :-1])
    assert e.value.code == api.ERR_INVALID and "keeps the size" in str(e.value)
    A.UpdateScene()
    after = K.desc_bytes(A.desc)
    assert all(np.array_equal(before[k], after[k]) for k in before)


def test_another_texel_is_still_topology():
    """ctl_scene_desc_diff keeps its answer: the per-image words of the geometry hashes are compared with the structure"""
    A, B, _ = _pair("floor_env")
    assert api.scene_desc_diff(A.desc, B.desc) & api.DIFF_TOPOLOGY
    C2 = K.floor_scene("floor_env", K.bright_rgbcol(16, 8, 1), K.bright_rgbe(12, 7, 2))
    assert api.scene_desc_diff(A.desc, C2.desc) == 0


def test_the_device_calls_answer_no_device_first():
    """without a device the scene calls report CTL_ERR_NO_DEVICE before they look at their arguments; with one, a null scene is invalid"""
    want = api.ERR_NO_DEVICE if api.device_count() < 1 else api.ERR_INVALID
    assert api.lib.ctl_scene_update_image(None, 0, None, 0, 0, 0, None) == want
    assert api.lib.ctl_scene_update_image(None, 0, None, 0, 0, 0xfffffffe, None) == want
    assert api.lib.ctl_scene_read_image(None, 0, None, 0, None, None) == want
