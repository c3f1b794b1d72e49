"""Host-side checks of streams with two and three reference pictures (include/mi355x_h264.h "streams", mi355x_h264_stream_open_ex)
that need no device: what the new entry point refuses before the device is touched, that mi355x_h264_stream_open keeps its
contract, how the plugin class reads persist.vmi.video.encode.refs, and the one rule for a picture's number of reference pictures
that the engine and the stream hub share (PicSeq::avail_refs, driven through the shim as both drive it)."""
import ctypes as C
import subprocess
from media_amd import capi
from media_amd import videocodec as vc
import stream_refs as sr

E_ARG = -1


def _cfg(**kw):
    cfg = capi.Config()
    capi.lib().mi355x_h264_default_config(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_the_export_exists_and_the_abi_version_stands():
    assert "mi355x_h264_stream_open_ex" in capi.EXPORTS and capi.STREAM_MULTIREF == 1
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T mi355x_h264_stream_open_ex\n" in syms
    assert capi.lib().mi355x_h264_abi_version() == 3


def test_stream_open_ex_refuses_before_the_device_is_touched():
    L = capi.lib()
    h = C.c_void_p()
    M = capi.STREAM_MULTIREF
    for flags, kw in ((2, {}), (3, {"refs": 3}), (0x80000000, {}), (M | 4, {"refs": 2}),     # unknown flag bits
                      (M, {"refs": 4}), (M, {"refs": 100}), (0, {"refs": 4}),                # more than three
                      (M, {"refs": 3, "band_count": 2, "slices": 4}), (M, {"band_count": 2, "slices": 4}),
                      (M, {"refs": 2, "batch": 2}), (M, {"batch": 8}),
                      (0, {"refs": 2}), (0, {"refs": 3}),                                    # flags 0 is mi355x_h264_stream_open
                      (M, {"refs": 3, "input_format": 3}), (M, {"refs": 3, "qp": 52}), (M, {"refs": 2, "gop": 0})):
        assert L.mi355x_h264_stream_open_ex(C.byref(_cfg(**kw)), flags, C.byref(h)) == E_ARG, (flags, kw)
        assert not h.value
    assert L.mi355x_h264_stream_open_ex(None, M, C.byref(h)) == E_ARG
    assert L.mi355x_h264_stream_open_ex(C.byref(_cfg(refs=3)), M, None) == E_ARG
    bad = _cfg(refs=3)
    bad.struct_size -= 4
    assert L.mi355x_h264_stream_open_ex(C.byref(bad), M, C.byref(h)) == E_ARG


def test_stream_open_still_refuses_two_reference_pictures():
    L = capi.lib()
    h = C.c_void_p()
    for refs in (2, 3, 4):
        assert L.mi355x_h264_stream_open(C.byref(_cfg(refs=refs)), C.byref(h)) == E_ARG, refs
        assert not h.value


def test_plugin_refs_property_parses_and_junk_falls_back():
    assert vc.parse_refs("2") == 2 and vc.parse_refs("3") == 3
    for junk in ("", "0", "1", "4", "3 ", "three", " 2", "-2", "2.0", "03"):
        assert vc.parse_refs(junk) == 1, junk           # the reference preset's iNumRefFrame
    vc.set_video_mode(320, 240, refs=3)
    assert vc.prop_get("persist.vmi.video.encode.refs") == "3"
    vc.set_video_mode(320, 240)
    assert vc.prop_get("persist.vmi.video.encode.refs") == ""


def test_the_shared_count_rule():
    assert vc.ref_counts(3, 30, 7) == [0, 1, 2, 3, 3, 3, 3]
    assert vc.ref_counts(2, 30, 5) == [0, 1, 2, 2, 2]
    assert vc.ref_counts(1, 30, 4) == [0, 1, 1, 1]
    # a forced IDR picture restarts it, in mid-GOP and on a GOP's first picture alike; so does the GOP's end
    assert vc.ref_counts(3, 30, 9, forced=(4,)) == [0, 1, 2, 3, 0, 1, 2, 3, 3]
    assert vc.ref_counts(3, 4, 10, forced=(4, 5)) == [0, 1, 2, 3, 0, 0, 1, 2, 3, 0]
    assert vc.ref_counts(3, 2, 6) == [0, 1, 0, 1, 0, 1]
    # and it is the rule the test lists restate (tests/stream_refs.py), for every stream of the mixed group
    for m in sr.MIXED:
        forced = [at for at, what in m.events if what == "idr"]
        assert vc.ref_counts(m.case.refs, m.case.gop, m.case.pictures, forced) == sr.member_counts(m), m.case.name
