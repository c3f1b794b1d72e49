"""Damage tiles as far as they need no device (include/mi355x_h264.h, "damage tiles"): the exports, what every new call refuses on null
arguments, the plugin key's parser, the layouts of the structures the ABI and the payload share with the tests, and
media_amd/csrc/damage.h under AddressSanitizer + UBSan as a program of its own (tools/damage_harness.cpp).  What the calls do on the
GPU, refusals on an open stream included: tests/test_gpu_damage.py."""
import ctypes as C
import os
import re
import subprocess

import damage as dm
from media_amd import capi
from media_amd import videocodec as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "media_amd", "csrc")
NAMES = ("mi355x_h264_stream_encode_damage", "mi355x_h264_stream_encode_nv12_damage", "mi355x_h264_stream_encode_rgba_damage",
         "mi355x_h264_stream_last_upload", "mi355x_h264_stream_debug_patch_stats")


def test_damage_h_under_address_and_ub_sanitizer(tmp_path):
    """random sizes, layouts, strides, rectangles and changes, the caller's planes allocated to their exact size: the harness aborts
    unless tile sets, twin, payload and fallback are what damage.h states; the sanitizers must report nothing"""
    exe = str(tmp_path / "damage_harness")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                        os.path.join(ROOT, "tools", "damage_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, "the build failed: %s" % r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok damage"), (r.stdout[-300:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_the_exports_exist_and_the_abi_version_stands():
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NAMES:
        assert n in capi.EXPORTS and " T %s\n" % n in syms, n
    assert capi.lib().mi355x_h264_abi_version() == 3   # functions were added, nothing changed
    assert "k_patch_step" in syms, "the patch kernel's host stub"


def test_null_arguments_are_refused():
    L = capi.lib()
    out, n, ft = C.c_void_p(), C.c_uint32(), C.c_int()
    buf = (C.c_uint8 * 64)()
    rect = capi.Rect(0, 0, 4, 4)
    tail = (C.byref(rect), 1, C.byref(out), C.byref(n), C.byref(ft))
    assert L.mi355x_h264_stream_encode_damage(None, buf, 16, buf, 8, buf, 8, *tail) == capi.E_ARG
    assert L.mi355x_h264_stream_encode_nv12_damage(None, buf, 16, buf, 16, *tail) == capi.E_ARG
    assert L.mi355x_h264_stream_encode_rgba_damage(None, buf, 64, *tail) == capi.E_ARG
    assert L.mi355x_h264_stream_encode_damage(None, None, 0, None, 0, None, 0, None, 0, None, None, None) == capi.E_ARG
    assert L.mi355x_h264_stream_last_upload(None, None, None, None, None) == capi.E_ARG
    assert L.mi355x_h264_stream_debug_patch_stats(None, None, None) == capi.E_ARG


def test_the_header_states_what_the_tests_restate():
    """the sentinel, the modes, the rectangle and the tile and payload constants, read from the headers' text"""
    hdr = open(os.path.join(ROOT, "include", "mi355x_h264.h")).read()
    m = re.search(r"#define MI355X_H264_DAMAGE_DETECT \((-0x[0-9A-Fa-f]+)\)", hdr)
    assert m and int(m.group(1), 16) == capi.DAMAGE_DETECT and capi.DAMAGE_DETECT < 0
    for i, name in enumerate(("WHOLE", "PATCHED", "NOTHING", "IN_PLACE")):
        assert re.search(r"MI355X_H264_UPLOAD_%s = %d\b" % (name, i), hdr), name
        assert capi.UPLOAD_NAMES[i] == name.lower()
    assert "typedef struct mi355x_h264_rect { int32_t x, y, w, h; } mi355x_h264_rect;" in hdr
    assert C.sizeof(capi.Rect) == 16 and [f[0] for f in capi.Rect._fields_] == ["x", "y", "w", "h"]
    dh = open(os.path.join(CSRC, "damage.h")).read()
    assert "enum { TILE_W = 64, TILE_H = 16, HEADER_BYTES = 16 };" in dh and (dm.TILE_W, dm.TILE_H, dm.HEADER) == (64, 16, 16)
    assert "struct Header { uint32_t magic, layout, ntiles, tile_bytes; };" in dh
    assert "struct PatchSrc { unsigned long long payload, slot; uint32_t ntiles, layout, w, h; };" in open(os.path.join(CSRC, "k_patch.h")).read()


def test_the_damage_key_parser():
    for v, want in (("", 0), ("off", 0), ("detect", 1), ("on", -1), ("1", -1), ("Detect", -1), ("detect ", -1), ("rects", -1), ("0", -1)):
        assert vc.parse_damage(v) == want, v


def test_set_next_damage_refusals_need_no_device():
    vc.set_video_mode(176, 144)
    e = vc.VideoEncoder()
    try:
        assert e.rc_create == vc.SUCCESS
        L = vc.lib()
        bad = (C.c_int32 * 4)(0, 0, -1, 4)
        assert L.vc_set_next_damage(e.h, bad, 1) == 0
        assert L.vc_set_next_damage(e.h, None, 2) == 0 and L.vc_set_next_damage(e.h, bad, -1) == 0
        assert e.set_next_damage([(0, 0, 16, 16)]) and e.set_next_damage([])
        assert e.last_upload() is None   # no engine yet
    finally:
        e.delete()
