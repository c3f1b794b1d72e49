"""Host-side checks of the decoder's output size (include/mi355x_h264_dec.h, "output size") that need no device: the exports and
their declarations, what the set calls refuse, null arguments, and how the decoder plugin reads its two keys.  A decoder cannot be
made without a device, so the refusals of a live handle (and that the setting reads back) are in tests/test_gpu_dec_scale.py
(test_set_time_refusals_and_read_back); here every refusal is asked of a null handle, which is refused whatever the size."""
import ctypes as C
import os
import re
import subprocess

import pytest

from media_amd import capi, h264dec
from media_amd import videodecoder as vd

E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi355x_h264_dec_set_output_size", "mi355x_h264_dec_output_size", "mi355x_h264_dec_group_set_output_size",
       "mi355x_h264_dec_group_output_size")
# what the set calls refuse: an odd value, a value outside 2..4096, exactly one of the two values 0 (shared with the GPU test)
REFUSED = [(15, 16), (16, 15), (1, 1), (4098, 16), (16, 4098), (0, 16), (16, 0), (-2, -2), (-16, 16), (4097, 4097), (1 << 20, 2)]
TAKEN = [(2, 2), (4096, 4096), (16, 2), (480, 270), (0, 0)]


def test_the_exports_exist_are_declared_and_the_abi_version_stands():
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    text = open(os.path.join(ROOT, "include", "mi355x_h264_dec.h")).read()
    for name in NEW:
        assert name in capi.EXPORTS and " T %s\n" % name in syms, name
        assert re.search(r"\b%s\(" % name, text), name + " is not declared in the header"
    assert capi.lib().mi355x_h264_abi_version() == 3, "functions are added: the ABI version stays"
    assert C.sizeof(h264dec.OutPic) == 40 and C.sizeof(capi.Config) == 72, "every struct keeps its size"
    for word in ("_picture_info", "_read_i420(_device)", "_group_read_i420(_device)", "debug_plane"):
        assert word in text.split("output size: pictures resampled")[1], word + ": the header says it stays at the native size"


@pytest.mark.parametrize("w,h", REFUSED + TAKEN)
def test_null_handles_are_refused_whatever_the_size(w, h):
    L = h264dec._bind()
    assert L.mi355x_h264_dec_set_output_size(None, w, h) == E_ARG
    assert L.mi355x_h264_dec_group_set_output_size(None, 0, w, h) == E_ARG
    assert L.mi355x_h264_dec_group_set_output_size(None, -1, w, h) == E_ARG


def test_null_arguments_of_the_read_back():
    L = h264dec._bind()
    a, b = C.c_int(7), C.c_int(7)
    assert L.mi355x_h264_dec_output_size(None, C.byref(a), C.byref(b)) == E_ARG
    assert L.mi355x_h264_dec_group_output_size(None, 0, C.byref(a), C.byref(b)) == E_ARG
    assert (a.value, b.value) == (7, 7)


def test_plugin_output_size_keys_parse_and_junk_falls_back():
    ok = vd.parse_output_size
    assert ok("480", "270") == (480, 270) and ok("2", "2") == (2, 2) and ok("4096", "4096") == (4096, 4096) and ok("0480", "270") == (480, 270)
    assert ok("", "") is None                                    # neither key: nothing to say
    for w, h in (("480", ""), ("", "270"), ("480", "junk"), ("480x270", "270"), (" 480", "270"), ("480", "270 "), ("+480", "270"), ("-480", "270"),
                 ("481", "270"), ("480", "271"), ("0", "0"), ("0", "270"), ("4098", "270"), ("480", "4098"), ("480.0", "270"), ("0x1e0", "270"),
                 ("480000000000", "270"), ("100000", "270"), ("1", "1")):
        assert ok(w, h) is False, (w, h)
