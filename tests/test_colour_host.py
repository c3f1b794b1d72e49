"""Colour description, the parts that need no device: the exports and what they refuse before the device is touched, the plugin's
two keys, the layout of mi355x_h264_dec_out_pic, and the sequence parameter set the host code writes for a described stream
(media_amd/csrc/host_framing.h, built for the CPU into the plugin library and driven through its shim, as
tests/test_stream_refs_host.py drives PicSeq) read back with the spec-literal reader of tests/colour.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import colour as col
from media_amd import capi, h264dec
from media_amd import videocodec as vc
from oracle_lib import OracleEncoder

E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("mi355x_h264_create_colour", "mi355x_h264_stream_open_colour", "mi355x_h264_colour_of", "mi355x_h264_stream_colour",
               "mi355x_h264_dec_colour", "mi355x_h264_dec_set_rgba_colour", "mi355x_h264_dec_group_colour",
               "mi355x_h264_dec_group_set_rgba_colour", "mi355x_h264_parser_colour")


def _cfg(**kw):
    cfg = capi.Config()
    capi.lib().mi355x_h264_default_config(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _colour(matrix, full, size=None):
    return capi.Colour(C.sizeof(capi.Colour) if size is None else size, matrix, full)


def test_the_exports_exist_and_the_abi_version_and_config_stand():
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW_EXPORTS:
        assert name in capi.EXPORTS and " T %s\n" % name in syms, name
    assert capi.lib().mi355x_h264_abi_version() == 3
    assert C.sizeof(capi.Config) == 72 and C.sizeof(capi.Colour) == 12   # mi355x_h264_config keeps its size
    assert (capi.MATRIX_BT709, capi.MATRIX_BT601) == (1, 6) == (col.BT709, col.BT601)


BAD = [(0, 0, None), (2, 0, None), (5, 0, None), (7, 1, None), (9, 0, None), (-1, 0, None), (256 + 6, 0, None),     # the matrix
       (1, 2, None), (6, -1, None), (1, 256, None),                                                                  # the range
       (1, 0, 8), (6, 1, 16), (1, 1, 0)]                                                                             # struct_size


@pytest.mark.parametrize("matrix,full,size", BAD)
def test_bad_descriptions_are_refused_before_the_device_is_touched(matrix, full, size):
    L = capi.lib()
    h = C.c_void_p()
    bad = _colour(matrix, full, size)
    assert L.mi355x_h264_stream_open_colour(C.byref(_cfg(width=64, height=48)), 0, 64, 48, C.byref(bad), C.byref(h)) == E_ARG and not h.value
    assert L.mi355x_h264_create_colour(C.byref(_cfg(width=64, height=48)), C.byref(bad), C.byref(h)) == E_ARG and not h.value
    g = h264dec._bind()
    # a null handle is refused whatever the description; with a handle these are refused for the description (GPU tests)
    assert g.mi355x_h264_dec_set_rgba_colour(None, C.byref(bad)) == E_ARG
    assert g.mi355x_h264_dec_group_set_rgba_colour(None, 0, C.byref(bad)) == E_ARG


def test_null_handles_and_what_open_scaled_refuses():
    L = capi.lib()
    g = h264dec._bind()
    h = C.c_void_p()
    good = _colour(1, 1)
    out8 = (C.c_int32 * 8)()
    assert L.mi355x_h264_colour_of(None, C.byref(good)) == E_ARG and L.mi355x_h264_stream_colour(None, C.byref(good)) == E_ARG
    assert g.mi355x_h264_dec_colour(None, out8) == E_ARG and g.mi355x_h264_dec_group_colour(None, 0, out8) == E_ARG
    assert g.mi355x_h264_parser_colour(None, out8, 8) == -1
    assert g.mi355x_h264_dec_set_rgba_colour(None, None) == E_ARG
    assert L.mi355x_h264_stream_open_colour(None, 0, 64, 48, C.byref(good), C.byref(h)) == E_ARG
    assert L.mi355x_h264_stream_open_colour(C.byref(_cfg(width=64, height=48)), 0, 64, 48, C.byref(good), None) == E_ARG
    assert L.mi355x_h264_create_colour(None, C.byref(good), C.byref(h)) == E_ARG
    # everything mi355x_h264_stream_open_scaled refuses, with a good description
    for flags, sw, sh, kw in ((2, 64, 48, {}), (0, 65, 48, {}), (0, 32, 48, {}), (0, 64 * 5, 48, {}), (0, 64, 48, {"refs": 2}), (0, 64, 48, {"qp": 52}),
                              (0, 64, 48, {"input_format": 3}), (0, 64, 48, {"batch": 2})):
        assert L.mi355x_h264_stream_open_colour(C.byref(_cfg(width=64, height=48, **kw)), flags, sw, sh, C.byref(good), C.byref(h)) == E_ARG, (flags, sw, sh, kw)
        assert not h.value
    short = _cfg(width=64, height=48)
    short.struct_size -= 4
    assert L.mi355x_h264_stream_open_colour(C.byref(short), 0, 64, 48, C.byref(good), C.byref(h)) == E_ARG
    assert L.mi355x_h264_create_colour(C.byref(short), C.byref(good), C.byref(h)) == E_ARG
    with pytest.raises(ValueError):
        capi.colour_struct(("bt2020", "full"))
    c = capi.colour_struct(("bt709", "full"))
    assert (c.struct_size, c.matrix, c.full_range) == (12, 1, 1) and capi.colour_struct(None) is None


def test_the_plugin_keys_parse_and_junk_is_the_reference_behaviour():
    assert vc.parse_colour("", "") is None
    assert vc.parse_colour("bt709", "") == (1, 0) and vc.parse_colour("bt601", "") == (6, 0)
    assert vc.parse_colour("", "full") == (6, 1) and vc.parse_colour("", "limited") == (6, 0)
    assert vc.parse_colour("bt709", "full") == (1, 1) and vc.parse_colour("bt601", "limited") == (6, 0)
    for c, r in (("bt2020", ""), ("BT709", ""), ("bt709 ", "full"), ("709", ""), ("1", ""), ("bt709", "Full"), ("", "1"), ("", "studio"), ("junk", "junk"),
                 ("bt709", "junk"), ("junk", "full")):
        assert vc.parse_colour(c, r) is False, (c, r)
    vc.set_video_mode(320, 240, colour="bt709", range="full")
    assert vc.prop_get("persist.vmi.video.encode.colour") == "bt709" and vc.prop_get("persist.vmi.video.encode.range") == "full"
    vc.set_video_mode(320, 240)
    assert vc.prop_get("persist.vmi.video.encode.colour") == "" and vc.prop_get("persist.vmi.video.encode.range") == ""


def test_dec_out_pic_keeps_its_size_and_offsets(tmp_path):
    """as the C compiler lays the header's struct out, as the binding declares it, and as it has always been (reserved -> colour)"""
    want = {"offset": 0, "width": 8, "height": 12, "stride": 16, "chroma_stride": 20, "fresh": 24, "colour": 28, "serial": 32}
    assert C.sizeof(h264dec.OutPic) == 40
    assert {k: getattr(h264dec.OutPic, k).offset for k, _ in h264dec.OutPic._fields_} == want
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mi355x_h264_dec.h"\nint main(void) { printf("%zu", sizeof(mi355x_h264_dec_out_pic));\n'
                   + "".join('printf(" %%zu", offsetof(mi355x_h264_dec_out_pic, %s));\n' % k for k in want) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [40] + list(want.values())


# ---- the parameter sets of the host code ----
def sps_of(ps):
    nals = col.split_nals(ps)
    assert [n[0] & 0x1F for n in nals] == [7, 8]
    return nals[0]


@pytest.mark.parametrize("variant", col.VARIANTS, ids=[col.NAMES[v] for v in col.VARIANTS])
def test_described_sps_parses_to_exactly_the_fields_of_the_description(variant):
    for profile in col.PROFILES:
        for refs in col.REFS:
            for w, h in col.SPS_SIZES:
                for rgba_input in (False, True):
                    for fps in (30, 60):
                        what = (profile, refs, w, h, rgba_input, fps)
                        plain = vc.parameter_sets(profile, refs, w, h, fps=fps)
                        ps = vc.parameter_sets(profile, refs, w, h, fps=fps, colour=variant, chroma_loc=rgba_input)
                        s, removed = col.read_sps(sps_of(ps))
                        s0, removed0 = col.read_sps(sps_of(plain))
                        assert s["vui"] == col.expected_vui(variant, rgba_input, fps, refs), what
                        # num_units_in_tick = 1 is three zero bytes and a one: the SPS went through emulation prevention
                        assert removed >= 1 and b"\x00\x00\x03" in sps_of(ps), what
                        assert s0["vui"] is None and {k: v for k, v in s.items() if k != "vui"} == {k: v for k, v in s0.items() if k != "vui"}, what
                        assert (s["profile_idc"], s["max_refs"], s["mbw"], s["mbh"]) == (profile, refs, (w + 15) // 16, (h + 15) // 16), what
                        assert s["crop"] == (None if (w % 16, h % 16) == (0, 0) else (0, (16 * s["mbw"] - w) // 2, 0, (16 * s["mbh"] - h) // 2)), what
                        assert col.split_nals(ps)[1] == col.split_nals(plain)[1], "the picture parameter set does not depend on the description"
                        # what the writer of tests/colour.py makes of the same fields is the same NAL unit
                        assert col.sps_nal(s) == sps_of(ps), what


def test_undescribed_parameter_sets_are_todays_bytes():
    """today's bytes: the oracle encoder's parameter sets (every GPU parity test compares whole access units with them)"""
    for profile in col.PROFILES:
        for refs in col.REFS:
            for w, h in col.SPS_SIZES:
                for fps in (30, 60):
                    orc = OracleEncoder(w, h, qp=30, gop=4, fps=fps, profile_idc=profile, refs=refs)
                    try:
                        au, _ = orc.encode(np.full(w * h * 3 // 2, 128, np.uint8))
                    finally:
                        orc.close()
                    nals = col.split_nals(au)
                    assert [n[0] & 0x1F for n in nals[:2]] == [7, 8]
                    want = b"".join(b"\x00\x00\x00\x01" + n for n in nals[:2])
                    assert vc.parameter_sets(profile, refs, w, h, fps=fps) == want, (profile, refs, w, h, fps)
                    assert au.startswith(want)
