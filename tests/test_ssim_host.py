"""Host-side checks of SSIM in the quality report (include/mi355x_h264.h, "quality report: SSIM") that need no device: the
exports, what is refused with MI355X_H264_E_ARG before anything is touched, which metrics the switch takes and what
MI355X_H264_QUALITY turns on (the library's own two rules, media_amd/csrc/host_framing.h, reached through the shim), how the plugin
class reads persist.vmi.video.encode.ssim, and that the record the Python binding declares is the header's struct.  (That a handle
refuses _ex(2) and _ex(4), small caps and "nothing to read" need a device: tests/test_gpu_ssim.py.)"""
import ctypes as C
import math
import os
import subprocess
from media_amd import capi
from media_amd import videocodec as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mi355x_h264_quality_enable_ex", "mi355x_h264_stream_quality_enable_ex", "mi355x_h264_quality_ssim_read",
         "mi355x_h264_quality_ssim_map", "mi355x_h264_stream_last_ssim", "mi355x_h264_stream_ssim_map")


def test_the_exports_exist_and_the_abi_version_stands():
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert n in capi.EXPORTS and " T %s\n" % n in syms, n
    assert capi.lib().mi355x_h264_abi_version() == 3   # functions, one struct and one enum were added, nothing changed
    assert (capi.QUALITY_SSE, capi.QUALITY_SSIM) == (1, 2)
    for n in ("vc_parse_ssim", "vc_last_ssim", "vc_debug_quality_metrics_ok", "vc_debug_quality_env"):
        assert hasattr(vc.lib(), n), n


def test_null_arguments_are_refused():
    L = capi.lib()
    s, m = capi.Ssim(), (C.c_int32 * 16)()
    for metrics in (0, 1, 2, 3, 4):
        assert L.mi355x_h264_quality_enable_ex(None, metrics) == capi.E_ARG
        assert L.mi355x_h264_stream_quality_enable_ex(None, metrics) == capi.E_ARG
    assert L.mi355x_h264_quality_ssim_read(None, C.byref(s), 1) == capi.E_ARG
    assert L.mi355x_h264_quality_ssim_read(None, None, 0) == capi.E_ARG
    assert L.mi355x_h264_quality_ssim_map(None, 0, m, 16) == capi.E_ARG
    assert L.mi355x_h264_quality_ssim_map(None, 0, None, 0) == capi.E_ARG
    assert L.mi355x_h264_stream_last_ssim(None, C.byref(s)) == capi.E_ARG
    assert L.mi355x_h264_stream_ssim_map(None, m, 16) == capi.E_ARG


def test_metrics_2_alone_and_any_other_bit_are_refused():
    """0 off, 1 the SSE alone, 3 both; SSIM alone (2), 4 and every other value: refused (the rule mi355x_h264_quality_enable_ex applies)"""
    assert [m for m in range(64) if vc.quality_metrics_ok(m)] == [0, 1, 3]
    assert not vc.quality_metrics_ok(2) and not vc.quality_metrics_ok(4)
    assert not vc.quality_metrics_ok(0x80000001) and not vc.quality_metrics_ok(0xFFFFFFFF)


def test_environment_value_3_turns_both_on_and_1_stays_what_it_is():
    assert vc.quality_env("1") == capi.QUALITY_SSE
    assert vc.quality_env("3") == capi.QUALITY_SSE | capi.QUALITY_SSIM
    for junk in (None, "", "0", "2", "4", "13", "31", "3 ", " 3", "03", "on", "-3", "3.0"):
        assert vc.quality_env(junk) == 0, junk


def test_plugin_ssim_property_accepts_1_only():
    assert vc.parse_ssim("1") is True
    for junk in ("", "0", "2", "3", "11", "1 ", " 1", "01", "on", "true", "yes", "-1", "1.0"):
        assert vc.parse_ssim(junk) is False, junk
    vc.set_video_mode(320, 240, ssim=1)
    assert vc.prop_get("persist.vmi.video.encode.ssim") == "1" and vc.prop_get("persist.vmi.video.encode.psnr") == ""
    vc.set_video_mode(320, 240)
    assert vc.prop_get("persist.vmi.video.encode.ssim") == ""


def test_the_record_is_the_headers_struct(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355x_h264.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(mi355x_h264_ssim), offsetof(mi355x_h264_ssim, sum),\n'
                   '  offsetof(mi355x_h264_ssim, windows), offsetof(mi355x_h264_ssim, valid), offsetof(mi355x_h264_ssim, reserved),\n'
                   '  sizeof(mi355x_h264_quality), MI355X_H264_QUALITY_SSE, MI355X_H264_QUALITY_SSIM); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    T = capi.Ssim
    assert got == [C.sizeof(T), T.sum.offset, T.windows.offset, T.valid.offset, T.reserved.offset, C.sizeof(capi.Quality), 1, 2]
    assert got == [56, 0, 24, 48, 52, 64, 1, 2]      # (mi355x_h264_quality keeps its layout)


def test_the_mean_is_computed_on_the_host():
    assert capi.ssim_mean(65536 * 7, 7) == 1.0 and capi.ssim_mean(-65305, 1) == -65305 / 65536.0 and math.isnan(capi.ssim_mean(0, 0))
    s = capi.Ssim()
    s.sum[0], s.windows[0], s.sum[1], s.windows[1], s.valid = 65536 * 9, 9, -32768, 1, 1
    r = capi._with_ssim({}, s)
    assert r["ssim"][0] == 1.0 and r["ssim"][1] == -0.5 and math.isnan(r["ssim"][2])
    assert r["ssim_sum"] == [65536 * 9, -32768, 0] and r["ssim_windows"] == [9, 1, 0]
