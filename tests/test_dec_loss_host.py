"""Host-side checks of the decoder's loss mode (include/mi355x_h264_dec.h, "loss mode") that need no device: the exports, what is
refused before anything is touched, the plugin key's parser, the HIP-free arithmetic (media_amd/csrc/dec_loss.h) as a stand-alone
program under AddressSanitizer and UBSan, strict mode's unchanged messages on the damaged inputs of tests/dec_loss.py, and the
parser in conceal mode: what it recovers from a damaged stream is, array for array, what the strict parser recovers from the
composed stream (the lost NAL units replaced by all-P_Skip stand-ins)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import dec_loss as dl
from media_amd import capi, h264dec, videodecoder as vd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("mi355x_h264_dec_set_loss_mode", "mi355x_h264_dec_damage", "mi355x_h264_dec_damage_map", "mi355x_h264_dec_group_set_loss_mode",
               "mi355x_h264_dec_group_damage", "mi355x_h264_dec_group_damage_map", "mi355x_h264_parser_set_loss_mode", "mi355x_h264_parser_loss")
IDS = [c.name for c in dl.CASES]


def test_the_exports_exist_are_declared_and_refuse_null_handles():
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(ROOT, "include", "mi355x_h264_dec.h")).read()
    for name in NEW_EXPORTS:
        assert name in capi.EXPORTS and " T %s\n" % name in syms and name + "(" in header, name
    L = h264dec._bind()
    out, buf = (C.c_int32 * 6)(), (C.c_uint8 * 16)()
    assert L.mi355x_h264_dec_set_loss_mode(None, 1) == capi.E_ARG and L.mi355x_h264_dec_group_set_loss_mode(None, 0, 1) == capi.E_ARG
    assert L.mi355x_h264_dec_damage(None, out) == capi.E_ARG and L.mi355x_h264_dec_group_damage(None, 0, out) == capi.E_ARG
    assert L.mi355x_h264_dec_damage_map(None, buf, 16) == capi.E_ARG and L.mi355x_h264_dec_group_damage_map(None, 0, buf, 16) == capi.E_ARG
    assert L.mi355x_h264_parser_set_loss_mode(None, 1) == capi.E_ARG and L.mi355x_h264_parser_loss(None, out) == capi.E_ARG
    p = h264dec.Parser()
    for mode in (-1, 2, 7):
        assert L.mi355x_h264_parser_set_loss_mode(p.h, mode) == capi.E_ARG
    assert L.mi355x_h264_parser_set_loss_mode(p.h, 1) == 0 and L.mi355x_h264_parser_set_loss_mode(p.h, 0) == 0
    with pytest.raises(ValueError):
        h264dec._loss_mode("lenient")
    assert h264dec._loss_mode("conceal") == h264dec.LOSS_CONCEAL == 1 and h264dec._loss_mode("strict") == h264dec.LOSS_STRICT == 0


def test_the_plugin_key_parser():
    assert vd.parse_loss_mode("") is None
    assert vd.parse_loss_mode("0") == 0 and vd.parse_loss_mode("1") == 1
    for bad in ("2", "-1", "01", "1 ", " 1", "on", "conceal", "1.0", "0x1"):
        assert vd.parse_loss_mode(bad) is False, bad


def build_sanitized(tmp_path, tool):
    """tools/<tool>.cpp with AddressSanitizer and UBSan.  The source must compile WITHOUT them first: a compile error is a failure,
    and only a toolchain that lacks the sanitizers' runtime is a reason to skip"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    base = ["g++", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "media_amd", "csrc"), os.path.join(ROOT, "tools", tool + ".cpp")]
    r = subprocess.run(base + ["-o", str(tmp_path / (tool + "_plain"))], capture_output=True, text=True)
    assert r.returncode == 0, "tools/%s.cpp does not compile:\n%s" % (tool, r.stderr[-2000:])
    exe = str(tmp_path / tool)
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build not available: " + r.stderr[-200:])
    return exe


def test_the_arithmetic_as_a_program_under_sanitizers(tmp_path):
    """tools/dec_loss_harness.cpp: hole extents, g across the frame_num wrap, the age mapping, every taint rule once positive and
    once negative, a clean IDR picture resetting the map - built as tools/fuzz_parser.cpp is built, run as a program"""
    exe = build_sanitized(tmp_path, "dec_loss_harness")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("dec_loss ok: ") and not r.stderr, r.stdout + r.stderr


STRICT = {"ir3_lose_band1": "slices out of order (first_mb_in_slice 16, expected 8)", "ir3_lose_first": "first slice of the access unit starts at macroblock 8",
          "ir3_lose_two": "picture incomplete: slices cover 8 of 24 macroblocks", "ir2_lose_last": "picture incomplete: slices cover 6 of 12 macroblocks",
          "refs3_gap1": "frame_num 6 does not follow the previous reference picture's 4: a picture is missing",
          "refs3_gap2": "frame_num 7 does not follow the previous reference picture's 4: a picture is missing",
          "refs3_gap4": "frame_num 9 does not follow the previous reference picture's 4: a picture is missing",
          "idr2_lose_idr": "frame_num 1 does not follow the previous reference picture's 3: a picture is missing",
          "ir2_join_at_recovery": "P slice without a reference picture", "ir2_join_before": "P slice without a reference picture",
          "ir3_join_at_recovery": "P slice without a reference picture", "ir3_join_before": "P slice without a reference picture"}


@pytest.mark.parametrize("c", dl.CASES, ids=IDS)
def test_strict_mode_refuses_the_damaged_input_with_its_message(c):
    """the default parser and one set to strict explicitly: the first damaged unit is refused (what a Decoder reports with E_STREAM),
    with the message it always had; a lost non-reference picture is no damage at all"""
    p = dl.plan(c)
    msgs = []
    for explicit in (False, True):
        par = h264dec.Parser()
        if explicit:
            par.set_loss_mode("strict")
        msg = None
        for k, au in enumerate(p.fed):
            if au is None:
                continue
            try:
                par.parse(au)
            except h264dec.StreamError as e:
                msg = (k, str(e))
                break
        msgs.append(msg)
        par.close()
    assert msgs[0] == msgs[1]
    if c.kind == "nonref":
        assert msgs[0] is None
        return
    assert msgs[0] is not None, "%s: the strict parser takes the damaged stream" % c.name
    k, text = msgs[0]
    act = [a for _, a in c.loss if a[0] == "flip"]
    assert k == (p.first_loss if not (act and c.kind == "gap") else p.first_loss - 1)
    if c.name in STRICT:
        assert text.startswith(STRICT[c.name]), text


@pytest.mark.parametrize("c", dl.CASES, ids=IDS)
def test_conceal_mode_parses_what_the_composed_stream_holds(c):
    p = dl.plan(c)
    con, ref = h264dec.Parser(), h264dec.Parser()
    con.set_loss_mode("conceal")
    fed_ref = 0
    for k, au in enumerate(p.fed):
        if au is None:
            continue
        assert con.parse(au) == p.got[k], (k, con.loss())
        loss = con.loss()
        if not p.got[k]:
            assert loss["lost"] == (0 if c.join is not None and k == 0 else 1), (k, loss)
            continue
        while fed_ref <= p.ref[k]:
            assert ref.parse(p.composed[fed_ref])
            fed_ref += 1
        for name, a, b in zip(("mb", "mvq", "aux", "levels"), con.arrays(), ref.arrays()):
            assert np.array_equal(a, b), (k, name)
        assert np.array_equal(con.mbqp(), ref.mbqp()), k
        for a, b in zip(con.vectors4(), ref.vectors4()):
            assert np.array_equal(a, b), k
        assert con._read(7, np.empty(con.mbqp().size, np.uint8)).tolist() == ref._read(7, np.empty(con.mbqp().size, np.uint8)).tolist(), k
        assert con.info() == ref.info(), (k, con.info(), ref.info())
        assert loss["concealed"] == p.concealed[k] == int(con.concealed().sum()) and loss["gap"] == p.gap[k] and loss["lost"] == 0, (k, loss)
        assert loss["joined"] == (1 if c.join is not None and k == 1 else 0), (k, loss)
    con.close(); ref.close()


def test_a_p_picture_without_parameter_sets_is_still_refused_and_a_damaged_sei_is_passed_over():
    s = dl.stream("ir3_64x96")
    par = h264dec.Parser()
    par.set_loss_mode("conceal")
    with pytest.raises(h264dec.StreamError, match="missing parameter set"):
        par.parse(s.aus[4])
    par.close()
    for mode in ("strict", "conceal"):
        par = h264dec.Parser()
        par.set_loss_mode(mode)
        assert par.parse(s.aus[0]) and par.loss()["recovery_frame_cnt"] == -1
        assert par.parse(s.aus[1]) and par.loss()["recovery_frame_cnt"] == s.n - 1          # k = 0: the encoder's recovery point SEI
        assert par.parse(s.aus[2]) and par.loss()["recovery_frame_cnt"] == -1
        for sei in (b"\x00\x00\x00\x01\x06\x06", b"\x00\x00\x00\x01\x06\x06\xff", b"\x00\x00\x00\x01\x06\x06\x09\x00\x80", b"\x00\x00\x00\x01\x06\xff\xff\xff"):
            q = h264dec.Parser()
            q.set_loss_mode(mode)
            assert q.parse(s.aus[0]) and q.parse(sei + s.aus[1]), sei
            assert q.loss()["recovery_frame_cnt"] in (-1, s.n - 1)
            q.close()
        par.close()


def test_a_slice_that_names_a_larger_picture_is_dropped_not_filled_up_to():
    """the picture keeps the size it began with: a slice under another sequence parameter set is damage.  Strict refuses the unit as it
    did; conceal drops that slice and fills the picture's own six macroblocks"""
    before, au = dl.other_size_unit()
    par = h264dec.Parser()
    for u in before:
        assert par.parse(u)
    with pytest.raises(h264dec.StreamError, match=r"slices out of order \(first_mb_in_slice 20, expected 6\)"):
        par.parse(au)
    par.close()
    par = h264dec.Parser()
    par.set_loss_mode("conceal")
    for u in before:
        assert par.parse(u)
    assert par.parse(au)
    i = par.info()
    assert (i["mbw"], i["mbh"]) == (3, 4) and par.loss()["concealed"] == 6 and par.concealed().tolist() == [0] * 6 + [1] * 6
    par.close()


def test_an_access_unit_of_many_broken_slices_is_refused():
    s = dl.stream("ir3_64x96")
    other, sl = dl.slices_of(s.aus[2])
    broken = bytes([0x41, 0xFF, 0xFF])                      # a slice NAL unit whose header cannot be read
    par = h264dec.Parser()
    par.set_loss_mode("conceal")
    assert par.parse(s.aus[0]) and par.parse(s.aus[1])
    assert par.parse(dl.annexb([broken] * 20 + sl)) and par.loss()["concealed"] == 0        # some broken ones: passed over
    with pytest.raises(h264dec.StreamError, match="more than 32 damaged slices"):
        par.parse(dl.annexb([broken] * 2000 + sl))
    par.close()


def test_the_conceal_parser_under_sanitizers(tmp_path):
    """tools/fuzz_parser.cpp with its `conceal` argument: the hole, drop, rescan, gap and join paths over the cases' damaged inputs,
    the unit that names a larger picture, and some 2 000 units damaged at random (bit flips, truncations, splices, slices dropped,
    doubled and swapped, units of two streams mixed) - no read or write outside an array, no undefined arithmetic"""
    import random
    import struct
    exe = build_sanitized(tmp_path, "fuzz_parser")
    rng = random.Random(11)
    units = []
    for c in dl.CASES:
        units.extend(u for u in dl.plan(c).fed if u is not None)
    before, au = dl.other_size_unit()
    units.extend(before + (au,) + tuple(dl.stream("ir2_48x64").aus[2:5]))
    names = ("ir3_64x96", "ir2_48x64", "refs3_64x64", "tl2_refs3_112x64", "one_34x18")
    for name in names:
        aus = dl.stream(name).aus
        for rep in range(40):
            for i, u in enumerate(aus):
                how = rng.randrange(9)
                other, sl = dl.slices_of(u)
                b = bytearray(u)
                if how == 0:
                    for _ in range(rng.randint(1, 6)):
                        b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
                elif how == 1:
                    b = b[:rng.randrange(1, len(b))]
                elif how == 2:
                    a, e = sorted(rng.randrange(len(b)) for _ in range(2))
                    b[a:e] = bytes(rng.randrange(256) for _ in range(rng.randint(0, 12)))
                elif how == 3:
                    b = bytearray(dl.annexb(other + [n for n in sl if rng.random() < 0.6]))
                elif how == 4:
                    rng.shuffle(sl)
                    b = bytearray(dl.annexb(other + sl + sl[:1]))
                elif how == 5:
                    b = b + bytearray(rng.choice(dl.stream(rng.choice(names)).aus))
                elif how == 6:
                    continue                                  # the unit does not arrive
                elif how == 7:
                    b = bytearray(dl.annexb(other + [dl.restart_slice(n, rng.randrange(300), rng.randrange(3)) for n in sl]))
                units.append(bytes(b))
    path = str(tmp_path / "units.bin")
    with open(path, "wb") as f:
        for u in units:
            f.write(struct.pack("<I", len(u)) + u)
    for mode in ((), ("conceal",)):
        r = subprocess.run([exe, path, *mode], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("parsed ") and not r.stderr, (mode, r.stdout[-300:], r.stderr[-3000:])
