"""Host-side checks of the stream inputs (include/mi355x_h264.h "streams": layouts and device-resident pictures) that need no
device: the argument checks mi355x_h264_stream_open and the new entry points make before the device is touched, and how the
plugin class reads its two input extension keys."""
import ctypes as C
from media_amd import capi
from media_amd import videocodec as vc

E_ARG = -1


def _cfg(**kw):
    cfg = capi.Config()
    capi.lib().mi355x_h264_default_config(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_stream_open_refuses_unknown_layouts_before_the_device_is_touched():
    L = capi.lib()
    h = C.c_void_p()
    for kw in ({"input_format": 3}, {"input_format": -1}, {"refs": 2}, {"refs": 2, "input_format": capi.INPUT_RGBA},
               {"batch": 2, "input_format": capi.INPUT_NV12}, {"band_count": 2, "slices": 4}):
        assert L.mi355x_h264_stream_open(C.byref(_cfg(**kw)), C.byref(h)) == E_ARG, kw
        assert not h.value


def test_create_still_refuses_rgba_and_the_abi_version_stands():
    L = capi.lib()
    h = C.c_void_p()
    assert capi.INPUT_RGBA == 2
    assert L.mi355x_h264_create(C.byref(_cfg(input_format=capi.INPUT_RGBA)), C.byref(h)) == E_ARG
    assert L.mi355x_h264_abi_version() == 3


def test_new_entry_points_refuse_a_null_stream():
    L = capi.lib()
    out, n, ft = C.c_void_p(), C.c_uint32(), C.c_int()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    assert L.mi355x_h264_stream_encode_device(None, p, C.byref(out), C.byref(n), C.byref(ft)) == E_ARG
    assert L.mi355x_h264_stream_encode_nv12(None, p, 16, p, 16, C.byref(out), C.byref(n), C.byref(ft)) == E_ARG
    assert L.mi355x_h264_stream_encode_rgba(None, p, 64, C.byref(out), C.byref(n), C.byref(ft)) == E_ARG
    for name in ("mi355x_h264_stream_encode_device", "mi355x_h264_stream_encode_nv12", "mi355x_h264_stream_encode_rgba"):
        assert name in capi.EXPORTS


def test_plugin_input_properties_parse_and_junk_falls_back():
    assert vc.parse_input_layout("nv12") == capi.INPUT_NV12
    assert vc.parse_input_layout("rgba") == capi.INPUT_RGBA
    for junk in ("", "i420", "NV12", "rgba ", "2", "yuv", "device"):
        assert vc.parse_input_layout(junk) == capi.INPUT_I420, junk      # the reference's videoFormatI420
    assert vc.parse_input_device("device") is True
    for junk in ("", "host", "Device", "1", "gpu", "rgba"):
        assert vc.parse_input_device(junk) is False, junk
    # the property store carries the two keys like any other
    vc.set_video_mode(320, 240, input="rgba", inputmem="device")
    assert vc.prop_get("persist.vmi.video.encode.input") == "rgba" and vc.prop_get("persist.vmi.video.encode.inputmem") == "device"
    vc.set_video_mode(320, 240)
    assert vc.prop_get("persist.vmi.video.encode.input") == "" and vc.prop_get("persist.vmi.video.encode.inputmem") == ""
