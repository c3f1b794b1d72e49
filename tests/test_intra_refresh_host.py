"""Host-side checks of intra refresh (include/mi355x_h264.h, "intra refresh") that need no device: the exports, the flag, what is
refused before the device is touched, and the host code's own sequence rule and SEI writer - media_amd/csrc/host_framing.h built
alone into tools/pic_seq_harness.cpp - against the restatement in tests/intra_refresh.py."""
import ctypes as C
import os
import re
import subprocess
import pytest
import intra_refresh as ir
from media_amd import capi
from media_amd import refresh as mr

E_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mi355x_h264.h")
NEW = ("mi355x_h264_set_intra_refresh", "mi355x_h264_last_refresh_band", "mi355x_h264_stream_last_refresh_band")


def _cfg(**kw):
    cfg = capi.Config()
    capi.lib().mi355x_h264_default_config(C.byref(cfg))
    cfg.width, cfg.height, cfg.slices = 64, 64, 2
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
    m = re.search(r"MI355X_H264_STREAM_INTRA_REFRESH\s*=\s*(\d+)", text)
    assert m and int(m.group(1)) == capi.STREAM_INTRA_REFRESH == 32
    assert L.mi355x_h264_abi_version() == 3, "functions and a flag are added: the ABI version stays"
    assert _cfg().struct_size == C.sizeof(capi.Config) == 72


def test_refused_before_the_device_is_touched():
    L = capi.lib()
    R, M, T = capi.STREAM_INTRA_REFRESH, capi.STREAM_MULTIREF, capi.STREAM_TEMPORAL2
    h = C.c_void_p()
    assert L.mi355x_h264_set_intra_refresh(None, 1) == E_ARG
    assert L.mi355x_h264_last_refresh_band(None) == E_ARG and L.mi355x_h264_stream_last_refresh_band(None) == E_ARG
    for flags, kw in ((R, {"slices": 0}), (R, {"slices": 1}), (R, {"slices": 33}), (R, {"slices": 64}),   # slices outside 2 .. 32
                      (R, {"slices": 3}),                          # 64 rows: four macroblock rows make two bands of two, not three
                      (R | M, {"refs": 2}), (R | M, {"refs": 3}), (R, {"refs": 2}),
                      (R | T, {}),                                 # two temporal layers
                      (R, {"band_count": 2}),                      # a band instance
                      (R | 16, {}), (R | 2, {}), (R | 4, {}), (16, {})):   # unknown flag bits beside the new one
        assert L.mi355x_h264_stream_open_ex(C.byref(_cfg(**kw)), flags, C.byref(h)) == E_ARG and not h.value, (flags, kw)
        assert L.mi355x_h264_stream_open_scaled(C.byref(_cfg(**kw)), flags, 128, 128, C.byref(h)) == E_ARG and not h.value, (flags, kw)
        assert L.mi355x_h264_stream_open_colour(C.byref(_cfg(**kw)), flags, 64, 64, None, C.byref(h)) == E_ARG and not h.value, (flags, kw)
    for kw in ({"slices": 0}, {"slices": 1}, {"slices": 33}, {"slices": 2, "refs": 2}, {"slices": 2, "temporal_layers": 2},
               {"slices": 2, "band_index": 0, "band_count": 2}):
        with pytest.raises(capi.EncoderError) as ei:
            capi.Encoder(64, 64, intra_refresh=True, **kw)
        assert ei.value.rc == E_ARG, kw
    for kw in ({"slices": 0}, {"slices": 33}, {"slices": 2, "refs": 2}, {"slices": 2, "temporal_layers": 2}):
        with pytest.raises(capi.EncoderError) as ei:
            capi.Stream(64, 64, intra_refresh=True, **kw)
        assert ei.value.rc == E_ARG, kw


# ---------------------------------------------------------------- the host code's own sequence rule and SEI writer

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pic_seq") / "pic_seq_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-o", exe, os.path.join(ROOT, "tools", "pic_seq_harness.cpp")], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout
        return [ln.split() for ln in out.splitlines()]
    return run


SCRIPTS = (
    (4, 30, "." * 14),
    (2, 7, "." * 20),                        # periodic IDR pictures: p restarts
    (3, 100, "....I....I.I..I......"),       # forced IDR pictures mid-cycle
    (8, 100, "...F.....F.F...F........."),   # failed pictures: the next one is an IDR picture
    (32, 1000, "." * 70),
    (2, 1, "....."),                         # every picture an IDR picture: never a band
)


@pytest.mark.parametrize("n,gop,script", SCRIPTS, ids=["n%d-gop%d-%d" % (s[0], s[1], k) for k, s in enumerate(SCRIPTS)])
def test_host_sequence_rule_against_the_restatement(harness, n, gop, script):
    forced = [i for i, ch in enumerate(script) if ch == "I"]
    failed = [i for i, ch in enumerate(script) if ch == "F"]
    want = ir.schedule(n, gop, len(script), forced, failed)
    got = harness("refresh", n, gop, script)
    assert len(got) == len(want)
    for i, (g, (idr, p, k)) in enumerate(zip(got, want)):
        assert [int(v) for v in g[:3]] == [int(idr), p, k], "picture %d of %r" % (i, script)
        assert g[3] == (ir.sei_bytes(n).hex() if k == 0 else "-"), "picture %d of %r: the SEI" % (i, script)
    if gop > n + 1 and not forced and not failed:
        assert {k for _, _, k in want} == set(range(-1, n))


def test_the_present_output_of_the_harness_is_unchanged(harness):
    got = harness(1, 4, 1, 2, 26, ".....")
    assert [g[:5] for g in got] == [["1", "0", "0", "0", "0"], ["0", "0", "1", "1", "1"], ["0", "0", "0", "2", "1"], ["0", "0", "1", "3", "1"],
                                    ["1", "0", "0", "0", "0"]]


def test_bands_of_the_picture(harness):
    for mbh, n in ((8, 4), (6, 3), (5, 2), (4, 2), (68, 8), (4, 3), (9, 4), (64, 32), (2, 2), (3, 2), (68, 33), (68, 1)):
        try:
            want = len(ir.band_rows(mbh, n)) if 2 <= n <= 32 else 0
        except AssertionError:
            want = None
        got = int(harness("bands", mbh, n)[0][0])
        assert (got == n) == (want == n), (mbh, n, got)


def test_schedule_and_recovery_of_the_python_side():
    assert mr.schedule(4, 10) == [-1, 0, 1, 2, 3, 0, 1, 2, 3, 0]
    assert mr.recovered_at(1, 4) == 4 and mr.recovered_at(5, 4) == 8 and mr.recovered_at(3, 2) == 4
    with pytest.raises(ValueError):
        mr.recovered_at(2, 4)
    with pytest.raises(ValueError):
        mr.schedule(1, 4)
    for n in (2, 4, 8, 32):
        s = b"\x00\x00\x00\x01\x67\x42" + ir.sei_bytes(n) + b"\x00\x00\x00\x01\x41\x9a"
        assert mr.recovery_points(s) == [(6, n - 1)]
    assert mr.recovery_points(b"\x00\x00\x00\x01\x41\x9a\x00") == []


def test_recovery_points_pass_over_truncated_and_foreign_sei():
    sc = b"\x00\x00\x00\x01"
    good = ir.sei_bytes(4)
    for cut in range(5, len(good)):                       # the encoder's own SEI cut short anywhere: passed over or read, never raised
        assert mr.recovery_points(good[:cut] + sc + b"\x41\x9a") in ([], [(0, 3)])
    foreign = sc + b"\x06\x05\xff\xff\x10" + b"\xaa" * 20          # user data that announces 526 bytes and has 20
    assert mr.recovery_points(foreign + good) == [(len(foreign), 3)]
    assert mr.recovery_points(sc + b"\x06\xff\xff\xff") == [] and mr.recovery_points(sc + b"\x06\x06") == [] and mr.recovery_points(sc + b"\x06\x06\x01\x00\x80") == []
    assert mr.recovery_points(sc + b"\x06\x05\x02\xaa\xbb" + good[5:]) == [(0, 3)]   # a message of another type in front, in one NAL unit


def test_the_plugin_key_parser():
    """persist.vmi.video.encode.intrarefresh: a decimal 2..32 the picture divides into, beside no conflicting key; unset is off
    without a WARN line; anything else is off with one"""
    from media_amd import videocodec as vc
    assert vc.parse_intra_refresh("") == (0, False)
    assert vc.parse_intra_refresh("8") == (8, False) and vc.parse_intra_refresh("2") == (2, False) and vc.parse_intra_refresh("32", height=1024) == (32, False)
    assert vc.parse_intra_refresh("32") == (0, True)              # 1080 rows: 68 macroblock rows in bands of three make 23
    assert vc.parse_intra_refresh("8", slices=8) == (8, False)
    for junk in ("0", "1", "33", "64", "-2", "eight", "8 ", " 8", "08", "8.0", "2,4", "100"):
        assert vc.parse_intra_refresh(junk) == (0, True), junk
    assert vc.parse_intra_refresh("8", slices=4) == (0, True) and vc.parse_intra_refresh("8", refs=2) == (0, True)
    assert vc.parse_intra_refresh("8", refs=3) == (0, True) and vc.parse_intra_refresh("8", layers=2) == (0, True)
    assert vc.parse_intra_refresh("3", height=64) == (0, True) and vc.parse_intra_refresh("2", height=64) == (2, False)   # four rows: two bands
    assert vc.parse_intra_refresh("4", height=144) == (0, True)      # nine rows in bands of three: three bands, not four
    assert vc.lib().vc_last_refresh_band(None) == -1
