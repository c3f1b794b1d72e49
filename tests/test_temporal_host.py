"""Host-side checks of the two temporal layers (include/mi355x_h264.h, "temporal layers") that need no device: the exports, what is
refused before the device is touched, and the sequence rule of the host code itself - media_amd/csrc/host_framing.h (PicSeq,
slice_nal_hdr, build_slice_header) built alone into tools/pic_seq_harness.cpp and held, picture by picture, against the
restatement in tests/temporal.py."""
import ctypes as C
import os
import re
import subprocess
import pytest
import temporal as tl
from media_amd import capi
from media_amd import temporal as mt

E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355x_h264.h")
NEW = ("mi355x_h264_set_temporal_layers", "mi355x_h264_last_temporal_id", "mi355x_h264_stream_last_temporal_id")


def _cfg(**kw):
    cfg = capi.Config()
    capi.lib().mi355x_h264_default_config(C.byref(cfg))
    cfg.width, cfg.height = 64, 48
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_exports_flag_and_abi_version():
    L = capi.lib()
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    text = open(HEADER).read()
    for name in NEW:
        assert name in capi.EXPORTS and " T %s\n" % name in syms, name
        assert re.search(r"\b%s\(" % name, text), name + " is not declared in the header"
    m = re.search(r"MI355X_H264_STREAM_TEMPORAL2\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == capi.STREAM_TEMPORAL2 and capi.STREAM_TEMPORAL2 & capi.STREAM_MULTIREF == 0
    assert L.mi355x_h264_abi_version() == 3, "functions and a flag are added: the ABI version stays"
    assert _cfg().struct_size == C.sizeof(capi.Config) == 72


def test_refused_before_the_device_is_touched():
    L = capi.lib()
    T, M = capi.STREAM_TEMPORAL2, capi.STREAM_MULTIREF
    h = C.c_void_p()
    assert L.mi355x_h264_set_temporal_layers(None, 2) == E_ARG
    assert L.mi355x_h264_last_temporal_id(None) == E_ARG and L.mi355x_h264_stream_last_temporal_id(None) == E_ARG
    for flags, kw in ((T | 2, {}), (T | 4, {}), (T | 16, {}), (T | 0x80000000, {}),                 # unknown flag bits beside the new one
                      (T, {"band_count": 2, "slices": 4}), (T | M, {"refs": 3, "band_count": 2, "slices": 4}),   # band instances
                      (T, {"refs": 2}), (T | M, {"refs": 4}), (T, {"batch": 2}), (T, {"qp": 52}), (T, {"gop": 0}), (T, {"input_format": 3})):
        assert L.mi355x_h264_stream_open_ex(C.byref(_cfg(**kw)), flags, C.byref(h)) == E_ARG and not h.value, (flags, kw)
        assert L.mi355x_h264_stream_open_scaled(C.byref(_cfg(**kw)), flags, 128, 96, C.byref(h)) == E_ARG and not h.value, (flags, kw)
        assert L.mi355x_h264_stream_open_colour(C.byref(_cfg(**kw)), flags, 64, 48, None, C.byref(h)) == E_ARG and not h.value, (flags, kw)
    for layers in (0, 3, -1, 17):
        with pytest.raises(capi.EncoderError) as ei:
            capi.Encoder(64, 48, temporal_layers=layers)
        assert ei.value.rc == E_ARG
        with pytest.raises(capi.EncoderError) as ei:
            capi.Stream(64, 48, temporal_layers=layers)
        assert ei.value.rc == E_ARG
    with pytest.raises(capi.EncoderError) as ei:
        capi.Encoder(64, 64, slices=2, band_index=0, band_count=2, temporal_layers=2)
    assert ei.value.rc == E_ARG


# ---------------------------------------------------------------- the host code's own sequence rule

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pic_seq") / "pic_seq_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tools", "pic_seq_harness.cpp")], check=True)

    def run(layers, gop, refs, slices, qp, script):
        out = subprocess.run([exe, str(layers), str(gop), str(refs), str(slices), str(qp), script], capture_output=True, text=True, check=True).stdout
        return [ln.split() for ln in out.splitlines()]
    return run


SCRIPTS = (
    # layers, gop, refs, slices, qp, one letter per picture ('I': an IDR picture is forced before it, 'F': the picture fails)
    (2, 8, 1, 1, 26, "." * 20),                  # GOPs of even length
    (2, 7, 1, 2, 24, "." * 20),                  # of odd length: two reference pictures meet at the GOP's end
    (2, 1, 1, 1, 26, "....."),                   # every picture an IDR picture
    (2, 2, 1, 1, 30, "......."),
    (2, 30, 3, 1, 30, "." * 12),                 # the reference count grows with the layer-0 pictures only
    (2, 9, 3, 4, 22, "....I....I.I..I....."),    # IDR pictures forced behind layer-1 and behind layer-0 pictures
    (2, 10, 2, 1, 26, "...F....F.F...F....."),   # failed pictures of both layers
    (2, 6, 2, 1, 40, "..FI..IF...."),
    (2, 1000, 1, 1, 26, "." * 560),              # frame_num wraps after 256 layer-0 pictures
    (1, 7, 3, 1, 26, "....I...F......."),        # one layer: every picture as ever
    (1, 300, 1, 1, 26, "." * 280),               # frame_num wraps
)


@pytest.mark.parametrize("layers,gop,refs,slices,qp,script", SCRIPTS, ids=["L%d-gop%d-refs%d-%d" % (s[0], s[1], s[2], k) for k, s in enumerate(SCRIPTS)])
def test_host_sequence_rule_against_the_restatement(harness, layers, gop, refs, slices, qp, script):
    forced = [i for i, ch in enumerate(script) if ch == "I"]
    failed = [i for i, ch in enumerate(script) if ch == "F"]
    want = tl.sequence(layers, gop, refs, len(script), forced, failed)
    got = harness(layers, gop, refs, slices, qp, script)
    assert len(got) == len(want)
    idr_id = 0
    for i, (g, s) in enumerate(zip(got, want)):
        tag = "picture %d of %r" % (i, script)
        assert [int(v) for v in g[:6]] == [int(s.idr), s.layer, s.slot, s.frame_num, s.nref, s.nal_hdr], tag
        assert int(g[6]) == (0 if layers == 1 or s.idr else 1 if s.layer else 2), tag + ": the facts k_me takes"
        assert int(g[7]) == (-1 if i in failed else s.slot), tag + ": the slot of the last picture"
        bits = tl.slice_header_bits(s.idr, s.layer == 1, s.frame_num, idr_id, s.nref, max(refs, 1), qp, False, slices)
        assert g[8] == "".join(str(b) for b in bits), tag + ": slice header"
        if s.idr and i not in failed:
            idr_id = (idr_id + 1) & 0xFF
    if layers == 2 and gop > 2:
        assert any(s.layer for s in want)


def test_a_layer1_header_is_one_bit_shorter():
    for nact, nrefs in ((1, 1), (1, 3), (3, 3)):
        a = tl.slice_header_bits(False, False, 5, 0, nact, nrefs, 30, False, 1)
        b = tl.slice_header_bits(False, True, 5, 0, nact, nrefs, 30, False, 1)
        assert len(a) == len(b) + 1


def test_base_layer_on_other_start_codes():
    """three-byte start codes and zero bytes in front of a start code: what is dropped is dropped with its start code"""
    sps, idr, p0, p1 = b"\x67\x42\x00\x1f", b"\x65\x88\x84", b"\x41\x9a\x22", b"\x01\x9a\x33"
    s3 = b"\x00\x00\x01"
    s4 = b"\x00" + s3
    stream = s4 + sps + s3 + idr + s4 + p1 + s3 + p0 + b"\x00" + s4 + p1 + s4 + p0
    assert mt.base_layer(stream) == s4 + sps + s3 + idr + s3 + p0 + s4 + p0
    assert mt.layers(stream)[1] == s4 + p1 + b"\x00" + s4 + p1
    assert mt.base_layer(b"") == b""


def test_the_plugin_key_parser():
    """persist.vmi.video.encode.temporallayers: "2" two layers; unset or "1" one; anything else one, with the WARN mark"""
    from media_amd import videocodec as vc
    assert vc.parse_temporal_layers("2") == (2, False)
    assert vc.parse_temporal_layers("1") == (1, False) and vc.parse_temporal_layers("") == (1, False)
    for junk in ("0", "3", "4", "-1", "two", "2 ", " 2", "02", "2.0", "1,2", "22"):
        assert vc.parse_temporal_layers(junk) == (1, True), junk
    assert vc.lib().vc_last_temporal_id(None) == -1
