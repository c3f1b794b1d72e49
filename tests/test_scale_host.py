"""Host-side checks of the scaled streams (include/mi355x_h264.h, mi355x_h264_stream_open_scaled) that need no device: the
exports, what the open call refuses before the device is touched, and how the plugin class reads its two source-size keys."""
import ctypes as C
import re
import os
import pytest
from media_amd import capi
from media_amd import videocodec as vc

E_ARG = -1
NEW = ("mi355x_h264_stream_open_scaled", "mi355x_h264_stream_source_width", "mi355x_h264_stream_source_height")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355x_h264.h")


def _cfg(**kw):
    cfg = capi.Config()
    capi.lib().mi355x_h264_default_config(C.byref(cfg))
    cfg.width, cfg.height = 64, 48
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _open(cfg, flags, sw, sh):
    h = C.c_void_p()
    rc = capi.lib().mi355x_h264_stream_open_scaled(C.byref(cfg), flags, sw, sh, C.byref(h))
    return rc, h.value


def test_exports_abi_version_and_config_size():
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(L, name)
    text = open(HEADER).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, text), name + " is not declared in the header"
    assert L.mi355x_h264_abi_version() == 3, "functions are added: the ABI version stays"
    cfg = _cfg()
    assert cfg.struct_size == C.sizeof(capi.Config) == 72, "mi355x_h264_config keeps its size (struct_size is compared for equality)"


def test_null_arguments():
    L = capi.lib()
    h = C.c_void_p()
    assert L.mi355x_h264_stream_open_scaled(None, 0, 96, 64, C.byref(h)) == E_ARG
    assert L.mi355x_h264_stream_open_scaled(C.byref(_cfg()), 0, 96, 64, None) == E_ARG
    assert L.mi355x_h264_stream_source_width(None) == 0 and L.mi355x_h264_stream_source_height(None) == 0
    short = _cfg()
    short.struct_size -= 4
    assert _open(short, 0, 96, 64) == (E_ARG, None)


@pytest.mark.parametrize("sw,sh,why", [
    (97, 64, "odd width"), (96, 65, "odd height"), (95, 63, "both odd"),
    (62, 48, "narrower than the coded picture"), (64, 46, "lower than the coded picture"), (14, 48, "below 16"),
    (258, 48, "more than 4 times the width"), (64, 194, "more than 4 times the height"), (4098, 64, "above 4096"), (64, 4098, "above 4096"),
    (0, 0, "zero"), (-96, -64, "negative")])
def test_source_sizes_that_are_refused_before_the_device_is_touched(sw, sh, why):
    for fmt in (capi.INPUT_I420, capi.INPUT_NV12, capi.INPUT_RGBA):
        assert _open(_cfg(input_format=fmt), 0, sw, sh) == (E_ARG, None), why
    assert _open(_cfg(), capi.STREAM_MULTIREF, sw, sh) == (E_ARG, None), why


def test_the_limits_of_the_source_range_at_the_largest_sizes():
    assert _open(_cfg(width=1024, height=1024), 0, 4098, 4096) == (E_ARG, None)
    assert _open(_cfg(width=1022, height=1024), 0, 4090, 4096) == (E_ARG, None)      # 4090 > 4 * 1022
    assert _open(_cfg(width=2048, height=16), 0, 2048, 66) == (E_ARG, None)


@pytest.mark.parametrize("kw,flags", [
    ({"input_format": 3}, 0), ({"input_format": -1}, 0), ({"refs": 2}, 0), ({"refs": 4}, capi.STREAM_MULTIREF), ({"batch": 2}, 0),
    ({"band_count": 2, "slices": 4}, 0), ({"qp": 9}, 0), ({"qp": 52}, 0), ({"gop": 0}, 0), ({}, 2), ({}, 0x80000000)])
def test_everything_open_ex_refuses_is_refused_with_a_valid_source_size(kw, flags):
    h = C.c_void_p()
    assert capi.lib().mi355x_h264_stream_open_ex(C.byref(_cfg(**kw)), flags, C.byref(h)) == E_ARG and not h.value
    assert _open(_cfg(**kw), flags, 96, 64) == (E_ARG, None)
    assert _open(_cfg(**kw), flags, 64, 48) == (E_ARG, None)      # the source IS the coded size: mi355x_h264_stream_open_ex itself


def test_an_odd_or_small_coded_size_is_refused_too():
    assert _open(_cfg(width=63), 0, 96, 64) == (E_ARG, None)
    assert _open(_cfg(width=14, height=14), 0, 32, 32) == (E_ARG, None)


def test_plugin_source_size_keys_parse_and_junk_falls_back():
    ok = vc.parse_source_size
    assert ok("1920", "1080", 1280, 720) == (1920, 1080)
    assert ok("1280", "720", 1280, 720) == (1280, 720)          # the coded size itself: an ordinary stream
    assert ok("4096", "2880", 1280, 720) == (4096, 2880)
    assert ok("", "", 1280, 720) is None                         # neither key: nothing to say
    for w, h in (("1920", ""), ("", "1080"), ("1920", "junk"), ("1920x1080", "1080"), (" 1920", "1080"), ("1920", "1080 "), ("+1920", "1080"),
                 ("-1920", "1080"), ("1921", "1080"), ("1920", "1081"), ("1278", "720"), ("1280", "718"), ("5122", "720"), ("1280", "2882"),
                 ("4098", "2880"), ("0", "0"), ("14", "14"), ("1920.0", "1080"), ("0x780", "1080"), ("192000000000", "1080"), ("19200000", "1080")):
        assert ok(w, h, 1280, 720) is False, (w, h)
    assert ok("64", "64", 16, 16) == (64, 64) and ok("66", "64", 16, 16) is False
    # the property store carries the two keys like any other
    vc.set_video_mode(1280, 720, srcwidth=1920, srcheight=1080)
    assert vc.prop_get("persist.vmi.video.encode.srcwidth") == "1920" and vc.prop_get("persist.vmi.video.encode.srcheight") == "1080"
    vc.set_video_mode(1280, 720)
    assert vc.prop_get("persist.vmi.video.encode.srcwidth") == "" and vc.prop_get("persist.vmi.video.encode.srcheight") == ""
