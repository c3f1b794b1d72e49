"""Host-side checks of the quality report (include/mi355x_h264.h, "quality report") that need no device: the exports, what is
refused with MI355X_H264_E_ARG before anything is touched, how the plugin class reads persist.vmi.video.encode.psnr, and that the
record the Python binding declares is the header's struct.  (A `cap` too small needs a handle, so a device: tests/test_gpu_quality.py,
test_nothing_to_read_and_small_caps_are_refused.)"""
import ctypes as C
import math
import os
import subprocess
from media_amd import capi
from media_amd import videocodec as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mi355x_h264_quality_enable", "mi355x_h264_quality_read", "mi355x_h264_quality_map", "mi355x_h264_stream_quality_enable",
         "mi355x_h264_stream_last_quality", "mi355x_h264_stream_quality_map")


def test_the_exports_exist_and_the_abi_version_stands():
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert n in capi.EXPORTS and " T %s\n" % n in syms, n
    assert capi.lib().mi355x_h264_abi_version() == 3   # functions were added, nothing changed


def test_null_arguments_are_refused():
    L = capi.lib()
    q, m = capi.Quality(), (C.c_uint32 * 16)()
    assert L.mi355x_h264_quality_enable(None, 1) == capi.E_ARG
    assert L.mi355x_h264_quality_read(None, C.byref(q), 1) == capi.E_ARG
    assert L.mi355x_h264_quality_read(None, None, 0) == capi.E_ARG
    assert L.mi355x_h264_quality_map(None, 0, m, 16) == capi.E_ARG
    assert L.mi355x_h264_quality_map(None, 0, None, 0) == capi.E_ARG
    assert L.mi355x_h264_stream_quality_enable(None, 1) == capi.E_ARG
    assert L.mi355x_h264_stream_last_quality(None, C.byref(q)) == capi.E_ARG
    assert L.mi355x_h264_stream_quality_map(None, m, 16) == capi.E_ARG


def test_plugin_psnr_property_accepts_1_only():
    assert vc.parse_psnr("1") is True
    for junk in ("", "0", "2", "11", "1 ", " 1", "01", "on", "true", "yes", "-1", "1.0"):
        assert vc.parse_psnr(junk) is False, junk
    vc.set_video_mode(320, 240, psnr=1)
    assert vc.prop_get("persist.vmi.video.encode.psnr") == "1"
    vc.set_video_mode(320, 240)
    assert vc.prop_get("persist.vmi.video.encode.psnr") == ""
    assert vc.VideoEncoder is not None and hasattr(vc.lib(), "vc_last_quality")


def test_the_record_is_the_headers_struct(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355x_h264.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mi355x_h264_quality), offsetof(mi355x_h264_quality, sse),\n'
                   '  offsetof(mi355x_h264_quality, samples), offsetof(mi355x_h264_quality, bytes), offsetof(mi355x_h264_quality, qp),\n'
                   '  offsetof(mi355x_h264_quality, frame_type), offsetof(mi355x_h264_quality, valid)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Q = capi.Quality
    assert got == [C.sizeof(Q), Q.sse.offset, Q.samples.offset, Q.bytes.offset, Q.qp.offset, Q.frame_type.offset, Q.valid.offset]
    assert got == [64, 0, 24, 48, 52, 56, 60]


def test_psnr_is_computed_on_the_host():
    assert capi.psnr(0, 100) == math.inf
    assert abs(capi.psnr(65025, 1)) < 1e-12 and abs(capi.psnr(100, 100) - 10 * math.log10(65025.0)) < 1e-12
    q = capi.Quality()
    q.sse[0], q.samples[0], q.samples[1], q.samples[2], q.sse[2], q.valid = 0, 4, 1, 1, 65025, 1
    r = capi._quality_record(q)
    assert r["psnr"][0] == math.inf and r["psnr"][1] == math.inf and abs(r["psnr"][2]) < 1e-12 and r["valid"] is True
