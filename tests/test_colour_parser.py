"""The decoder's host parser on sequence parameter sets with a VUI (media_amd/csrc/h264_parse.h: parse_vui; the report is
mi355x_h264_parser_colour), CPU only.  The parameter sets are written by tests/colour.py's writer, field by field from E.1.1; the
slices under them are I_PCM units of tests/pcm_stream.py and pictures of the oracle encoder.  What is checked: every field present
and absent, Extended_SAR, HRD parameter sets of 1 and 32 entries in front of the bitstream restriction, matrix codes the library
has no numbers for; the oracle's OpenH264-style streams; and that a VUI that is truncated at any bit or has bits flipped NEVER
refuses the stream, never reports a field out of its range, and leaves the picture what it is."""
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

import colour as col
import pcm_stream
import value_cube as vc
from media_amd import h264dec, synth
from media_amd import videocodec as vcodec
from oracle_lib import OracleEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HRD1 = {"bit_rate_scale": 4, "cpb_size_scale": 6, "cpb": [(9374, 1874, 1)], "lengths": (23, 23, 23, 24)}
HRD32 = {"bit_rate_scale": 1, "cpb_size_scale": 3, "cpb": [(100 * k + 7, 3 * k, k & 1) for k in range(32)], "lengths": (0, 31, 5, 0)}
RESTRICTION = (1, 0, 0, 16, 16, 0, 1)
FULL = {"aspect_ratio": (255, 40, 33), "overscan": 1, "signal": {"video_format": 5, "full_range": 1, "colour": (1, 1, 1)}, "chroma_loc": (1, 1),
        "timing": (1, 60, 1), "nal_hrd": HRD1, "vcl_hrd": HRD32, "low_delay_hrd": 0, "pic_struct": 1, "restriction": RESTRICTION}


def vui_cases():
    """(name, VUI dict): every field present and absent, one at a time and all together"""
    out = [("empty", {"pic_struct": 0}), ("full", FULL)]
    for key in col.VUI_KEYS:
        if key in ("low_delay_hrd", "pic_struct"):
            continue
        out.append(("only_" + key, dict({"pic_struct": 0, key: FULL[key]}, **({"low_delay_hrd": 0} if key.endswith("_hrd") else {}))))
        out.append(("without_" + key, {k: v for k, v in FULL.items() if k != key}))
    out.append(("aspect_ratio_idc", {"pic_struct": 0, "aspect_ratio": 14, "restriction": RESTRICTION}))
    out.append(("extended_sar", {"pic_struct": 0, "aspect_ratio": (255, 65535, 1), "signal": FULL["signal"], "restriction": (0, 16, 16, 0, 0, 2, 16)}))
    out.append(("signal_without_description", {"pic_struct": 0, "signal": {"video_format": 2, "full_range": 1}}))
    out.append(("hrd_1_in_front_of_restriction", {"pic_struct": 0, "nal_hrd": HRD1, "low_delay_hrd": 1, "restriction": (1, 2, 1, 12, 11, 1, 4)}))
    out.append(("hrd_32_in_front_of_restriction", {"pic_struct": 1, "vcl_hrd": HRD32, "low_delay_hrd": 0, "restriction": (1, 0, 0, 16, 16, 0, 3)}))
    out.append(("timing_29_97", {"pic_struct": 0, "timing": (1001, 60000, 1)}))
    out.append(("timing_widest", {"pic_struct": 0, "timing": (1, 0xFFFFFFFF, 0)}))
    for m in col.UNKNOWN_MATRICES:
        out.append(("matrix_%d" % m, col.described_vui(m, 1, restriction=RESTRICTION)))
    for top in range(6):
        out.append(("chroma_loc_%d" % top, {"pic_struct": 0, "chroma_loc": (top, 5 - top)}))
    return out


CASES = vui_cases()
# out of range: the VUI counts as absent, the stream decodes
OUT_OF_RANGE = [("chroma_loc_6", {"pic_struct": 0, "signal": FULL["signal"], "chroma_loc": (6, 0)}),
                ("chroma_loc_bottom_9", {"pic_struct": 0, "chroma_loc": (0, 9)}),
                ("no_ticks", {"pic_struct": 0, "signal": FULL["signal"], "timing": (0, 60, 1)}),
                ("no_time_scale", {"pic_struct": 0, "timing": (1, 0, 1)}),
                ("hrd_33", {"pic_struct": 0, "signal": FULL["signal"], "nal_hrd": dict(HRD32, cpb=HRD32["cpb"] + [(1, 1, 1)]), "low_delay_hrd": 0}),
                ("reorder_above_buffering", {"pic_struct": 0, "signal": FULL["signal"], "restriction": (1, 0, 0, 16, 16, 3, 2)}),
                ("buffering_17", {"pic_struct": 0, "restriction": (1, 0, 0, 16, 16, 0, 17)}),
                ("mv_length_17", {"pic_struct": 0, "restriction": (1, 0, 0, 17, 16, 0, 1)}),
                ("denominator_17", {"pic_struct": 0, "restriction": (1, 17, 0, 16, 16, 0, 1)}),
                ("huge_exp_golomb", {"pic_struct": 0, "signal": FULL["signal"], "chroma_loc": ((1 << 32) - 2, 0)})]


def pcm_unit(seed=3):
    """a 32x32 I_PCM access unit of tests/pcm_stream.py and its planes"""
    rng = np.random.RandomState(seed)
    y, u, v = rng.randint(0, 256, (32, 32)).astype(np.uint8), rng.randint(0, 256, (16, 16)).astype(np.uint8), rng.randint(0, 256, (16, 16)).astype(np.uint8)
    return pcm_stream.access_unit(y, u, v), (y, u, v)


def picture_of(par):
    """everything the parser recovered from the last unit, as bytes"""
    return b"".join(a.tobytes() for a in par.arrays()) + par.mbqp().tobytes() + repr(par.info()).encode()


@pytest.fixture(scope="module")
def pcm():
    au, planes = pcm_unit()
    par = h264dec.Parser()
    assert par.parse(au)
    want = picture_of(par)
    assert par.colour() == col.ABSENT
    # the samples are there: the I_PCM bytes of every macroblock in the level area
    lv = par.arrays()[3]
    assert np.array_equal(lv.view(np.uint8)[:, :384], pcm_stream.macroblocks(*planes))
    par.close()
    return au, want


@pytest.mark.parametrize("name,vui", CASES + OUT_OF_RANGE, ids=[n for n, _ in CASES + OUT_OF_RANGE])
def test_the_parser_reports_what_the_writer_wrote(pcm, name, vui):
    au, want = pcm
    nal = col.pcm_sps(2, 2, vui)
    if vui_ok := col.vui_in_range(vui):
        back, _ = col.read_sps(nal)
        assert back["vui"] == vui, "the reader reads what the writer wrote"
    assert vui_ok == ((name, vui) in CASES)
    par = h264dec.Parser()
    assert par.parse(col.replace_sps(au, nal)), name
    got = par.colour()
    assert got == col.report_of(vui) and col.report_in_range(got), (name, got, col.report_of(vui))
    assert picture_of(par) == want, "the picture does not depend on the VUI"
    par.close()


def test_the_report_follows_the_active_parameter_set():
    """two sets by id under one parser: the report is of the set the last slice referred to"""
    au, _ = pcm_unit()
    par = h264dec.Parser()
    assert par.parse(col.replace_sps(au, col.pcm_sps(2, 2, col.described_vui(1, 1))))
    assert (par.colour()["matrix"], par.colour()["full_range"]) == (1, 1)
    assert par.parse(col.replace_sps(au, col.pcm_sps(2, 2, col.described_vui(6, 0, chroma_loc=(1, 1)))))
    assert (par.colour()["matrix"], par.colour()["full_range"], par.colour()["chroma_loc"]) == (6, 0, 1)
    assert par.parse(au) and par.colour() == col.ABSENT     # the set without a VUI again
    par.close()


def test_streams_of_the_library_and_of_the_oracle():
    """the library's own described parameter sets (the host code through the plugin's shim) in front of the oracle encoder's
    pictures; and the oracle's OpenH264-style streams (feature 256): a VUI of nothing but the bitstream restriction"""
    w, h = 50, 34
    for variant in col.VARIANTS:
        for profile, refs, fps in ((66, 1, 30), (100, 3, 60)):
            enc = OracleEncoder(w, h, qp=30, gop=4, fps=fps, profile_idc=profile, refs=refs)
            par, plain = h264dec.Parser(), h264dec.Parser()
            for i, f in enumerate(synth.sequence("s1", w, h, 3)):
                au, idr = enc.encode(f)
                described = au
                if idr:
                    head = vcodec.parameter_sets(profile, refs, w, h, fps=fps)
                    assert au.startswith(head)
                    described = vcodec.parameter_sets(profile, refs, w, h, fps=fps, colour=variant, chroma_loc=True) + au[len(head):]
                assert par.parse(described) and plain.parse(au)
                assert picture_of(par) == picture_of(plain), (col.NAMES[variant], i)
                prim = 1 if variant[0] == col.BT709 else 6
                assert par.colour() == {"described": 1, "matrix": variant[0], "full_range": variant[1], "primaries": prim, "transfer": prim, "chroma_loc": 1,
                                        "fps": fps, "reorder": 0, "vui": 1, "dec_buffering": refs}
                assert plain.colour() == col.ABSENT
            par.close()
            plain.close()
    for refs in (1, 2, 3):
        enc = OracleEncoder(96, 80, qp=30, gop=4, profile_idc=66, refs=refs)
        par = h264dec.Parser()
        for i in range(4):
            au, _, _ = enc.random_picture(1000 + i, features=256 | 1 | 2 | 32)
            assert par.parse(au)
            assert par.colour() == dict(col.ABSENT, vui=1, reorder=0, dec_buffering=refs), (refs, i)
        par.close()


# ---- damage: the described SPS as a list of bits, the VUI's share of them known ----
def described_bits(vui):
    s = {"profile_idc": 66, "constraints": 0xC0, "level_idc": 40, "log2_max_frame_num_minus4": 0, "poc_type": 2, "max_refs": 1, "mbw": 2, "mbh": 2,
         "crop": None, "vui": vui}
    start = len(col.write_sps_bits(col.BitWriter(), dict(s, vui=None)).b)   # (the flag is the last bit in front of the VUI)
    return col.write_sps_bits(col.BitWriter(), s).b, start


def nal_of_bits(bits):
    w = col.BitWriter()
    w.b = list(bits)
    return b"\x67" + col.escape(w.rbsp())


def python_report(bits, start):
    """what a spec-literal reader makes of the VUI in these SPS bits: the report, or the absent one when it runs past the payload"""
    w = col.BitWriter()
    w.b = list(bits)
    r = col.BitReader(w.rbsp())
    r.at = start
    try:
        vui = col.read_vui(r)
    except AssertionError:
        return dict(col.ABSENT)
    return col.report_of(vui)


DAMAGE_VUIS = [("full", FULL), ("library", col.expected_vui((col.BT709, 1), True, 30, 3))]


@pytest.mark.parametrize("name,vui", DAMAGE_VUIS, ids=[n for n, _ in DAMAGE_VUIS])
def test_a_vui_truncated_at_any_bit_never_refuses_the_stream(pcm, name, vui):
    au, want = pcm
    bits, start = described_bits(vui)
    par = h264dec.Parser()
    for cut in range(start, len(bits) + 1):
        unit = col.replace_sps(au, nal_of_bits(bits[:cut]))
        assert par.parse(unit), "cut at bit %d of %d" % (cut, len(bits))
        got = par.colour()
        # a VUI that ends early runs into the trailing bits: absent as a whole - only the whole VUI is a VUI
        assert got == (col.report_of(vui) if cut == len(bits) else col.ABSENT), (cut, got)
        assert picture_of(par) == want, cut
    # bytes cut off the NAL unit itself (no trailing bits of its own any more)
    whole = nal_of_bits(bits)
    for n in range(len(nal_of_bits(bits[:start])), len(whole)):
        unit = col.replace_sps(au, whole[:n])
        assert par.parse(unit), "NAL unit cut to %d bytes" % n
        assert col.report_in_range(par.colour()) and picture_of(par) == want, n
    par.close()


def test_two_thousand_bit_flips_inside_the_vui(pcm):
    au, want = pcm
    rng = random.Random(2024)
    par = h264dec.Parser()
    agreed_present = agreed_absent = 0
    for case in range(2000):
        name, vui = DAMAGE_VUIS[case % 2]
        bits, start = described_bits(vui)
        bits = list(bits)
        for _ in range(rng.choice((1, 1, 1, 2, 3, 8))):
            bits[rng.randrange(start, len(bits))] ^= 1
        assert par.parse(col.replace_sps(au, nal_of_bits(bits))), "case %d" % case
        got = par.colour()
        assert col.report_in_range(got), (case, got)
        assert picture_of(par) == want, case
        # the differential: a spec-literal reader of the same bits
        expect = python_report(bits, start)
        assert got == expect, (case, got, expect)
        agreed_present += got["vui"]
        agreed_absent += 1 - got["vui"]
    par.close()
    assert agreed_present > 300 and agreed_absent > 300, (agreed_present, agreed_absent)


def test_described_streams_and_their_truncations_under_address_sanitizer(tmp_path, pcm):
    """tools/fuzz_parser.cpp, built as tests/test_dec_parser.py builds it: the host parser as a stand-alone program under
    AddressSanitizer + UBSan over every described parameter set of this file, every truncation and 500 flipped ones"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "fuzz_parser")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "media_amd", "csrc"), os.path.join(ROOT, "tools", "fuzz_parser.cpp"), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build not available: " + r.stderr[-200:])
    au, _ = pcm
    units = [col.replace_sps(au, col.pcm_sps(2, 2, vui)) for _, vui in CASES + OUT_OF_RANGE]
    rng = random.Random(7)
    for name, vui in DAMAGE_VUIS:
        bits, start = described_bits(vui)
        units += [col.replace_sps(au, nal_of_bits(bits[:cut])) for cut in range(start, len(bits) + 1)]
        whole = nal_of_bits(bits)
        units += [col.replace_sps(au, whole[:n]) for n in range(4, len(whole))]
        for _ in range(250):
            b = list(bits)
            for _ in range(rng.choice((1, 2, 8))):
                b[rng.randrange(start, len(b))] ^= 1
            units.append(col.replace_sps(au, nal_of_bits(b)))
    path = str(tmp_path / "units.bin")
    with open(path, "wb") as f:
        for u in units:
            f.write(struct.pack("<I", len(u)))
            f.write(u)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("parsed "), (r.stdout[-300:], r.stderr[-1500:])
    parsed, refused = int(r.stdout.split()[1]), int(r.stdout.split()[3])
    # nothing behind the cropping flags refuses; the few units refused are those cut inside the fields in front of the VUI
    assert parsed >= len(units) - 40 and parsed + refused == len(units), r.stdout
