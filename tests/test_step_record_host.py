"""The record of a step's picture and the device words that carry it (media_amd/csrc/item_word.h: ItemPic, item_word, me_word,
item_unpack; media_amd/csrc/host_framing.h: PicSeq::pic, batch_item_pic), without a device: the host code built alone into
tools/pic_seq_harness.cpp with g++, run as a program, and held against the layout restated here and the sequence rules restated in
tests/temporal.py and tests/intra_refresh.py."""
import os
import shutil
import subprocess
import pytest
import intra_refresh as ir
import temporal as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "pic_seq_harness.cpp")


def _runner(exe):
    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True)
        assert not r.stderr, r.stderr
        return [ln.split() for ln in r.stdout.splitlines()]
    return run


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("step_record") / "pic_seq_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-o", exe, SRC], check=True)
    return _runner(exe)


# ---------------------------------------------------------------- the layout, restated

# itemtab word: bits 0..7 batch item, 8..9 ring slot, 10..11 reference pictures, 12..13 the two facts of k_me, 16..21 QP, 22..27 band + 1
FIELDS = {"item": (0, 8), "cur": (8, 2), "nref": (10, 2), "me": (12, 2), "qp": (16, 6), "rband": (22, 6)}
ORDER = ("item", "cur", "qp", "nref", "me", "rband")      # the arguments of the harness's pack mode
BASE = {"item": 5, "cur": 1, "qp": 26, "nref": 1, "me": 2, "rband": 3}


def word_of(p):
    w = 0
    for name, (shift, _) in FIELDS.items():
        w |= (p[name] + (1 if name == "rband" else 0)) << shift
    return w


def check_tail(tail, p, refresh, tag):
    """the tail of a harness line: item_word in hex, its error flag, me_word, item_unpack of the word (item cur nref qp me rband)"""
    assert tail[0] == "%08x" % word_of(p) and tail[1] == "0", tag + ": item_word"
    mw = int(tail[2])
    assert mw & 3 == p["me"] and (mw >> 8) & 63 == (p["rband"] + 1 if refresh else 0), tag + ": me_word, bits 0..1 and 8..13"
    assert mw == p["me"] | ((p["rband"] + 1) << 8 if refresh else 0), tag + ": me_word, no other bit"
    assert [int(v) for v in tail[3:]] == [p["item"], p["cur"], p["nref"], p["qp"], p["me"], p["rband"]], tag + ": item_unpack"


@pytest.mark.parametrize("field", ORDER)
def test_round_trip_and_refusal_per_field(harness, field):
    """the field at 0 (the band: none), at its maximum and between, beside other fields that are not 0; one step beyond: refused"""
    width = FIELDS[field][1]
    off = 1 if field == "rband" else 0          # the band travels as k + 1
    top = (1 << width) - 1 - off
    for v in (0 - off, top // 2, top):
        p = dict(BASE, **{field: v})
        got = harness("pack", *[p[k] for k in ORDER])
        assert len(got) == 1
        check_tail(got[0], p, True, "%s = %d" % (field, v))
    for v in (top + 1, top + 1000, -1 - off):
        p = dict(BASE, **{field: v})
        got = harness("pack", *[p[k] for k in ORDER])[0]
        assert got[0] == "00000000" and got[1] == "1", "%s = %d does not fit %d bits: the word is 0 and the error is reported" % (field, v, width)


def test_every_field_at_its_maximum_together(harness):
    p = {"item": 255, "cur": 3, "qp": 63, "nref": 3, "me": 3, "rband": 62}
    check_tail(harness("pack", *[p[k] for k in ORDER])[0], p, True, "all at the maximum")
    p = {"item": 0, "cur": 0, "qp": 0, "nref": 0, "me": 0, "rband": -1}
    got = harness("pack", *[p[k] for k in ORDER])[0]
    check_tail(got, p, True, "all at 0")
    assert got[0] == "00000000" and got[1] == "0", "a word of 0 that is no error"


# ---------------------------------------------------------------- the derivation

CASES = (
    # layers, gop, refs, slices, refresh bands, qp, one letter per picture ('I': an IDR picture is forced before it, 'F': the picture fails)
    (1, 6, 1, 2, 2, 26, "....I...F......."),          # a GOP shorter than the script, refresh with n = 2
    (1, 100, 1, 5, 5, 38, "......I.....F......."),     # n = 5: more than one cycle, cut by a forced IDR and by a failed picture
    (2, 7, 3, 1, 0, 22, "...I....F........"),         # two layers, three reference pictures
    (2, 4, 1, 1, 0, 30, ".........."),                # two layers, one reference picture, short GOPs of even length
    (1, 5, 3, 1, 0, 51, "....F...I....."),            # one layer, three reference pictures
    (2, 9, 3, 5, 5, 10, "....I....F......."),         # the facts of k_me and a band in one word (the rule alone: the API refuses the pair)
    (1, 300, 1, 1, 0, 26, "." * 270),                 # frame_num wraps
)


@pytest.mark.parametrize("layers,gop,refs,slices,refresh,qp,script", CASES, ids=["L%d-gop%d-refs%d-n%d" % (c[:3] + (c[4],)) for c in CASES])
def test_the_records_against_the_restatements(harness, layers, gop, refs, slices, refresh, qp, script):
    forced = [i for i, ch in enumerate(script) if ch == "I"]
    failed = [i for i, ch in enumerate(script) if ch == "F"]
    seq = tl.sequence(layers, gop, refs, len(script), forced, failed)
    bands = ir.schedule(refresh, gop, len(script), forced, failed) if refresh else [(s.idr, 0, -1) for s in seq]
    got = harness("words", layers, gop, refs, slices, refresh, qp, script)
    assert len(got) == len(seq) == len(bands)
    idr_id = 0
    for i, (g, s, (idr, _, k)) in enumerate(zip(got, seq, bands)):
        tag = "picture %d of %r" % (i, script)
        assert bool(idr) == bool(s.idr), tag + ": the two restatements agree on the IDR pictures"
        p = {"item": 0, "cur": s.slot, "qp": qp, "nref": s.nref, "me": 0 if layers == 1 or s.idr else 1 if s.layer else 2, "rband": k}
        assert int(g[0]) == int(s.idr), tag
        # the record: item cur qp frame_num idr_id nref layer me rband
        assert [int(v) for v in g[1:10]] == [0, s.slot, qp, s.frame_num, idr_id, s.nref, s.layer, p["me"], k], tag + ": the record"
        check_tail(g[10:], p, refresh != 0, tag)
        if s.idr and i not in failed:
            idr_id = (idr_id + 1) & 0xFF
    if layers == 2:
        assert any(s.layer for s in seq)
    if refresh:
        assert {k for _, _, k in bands} == set(range(-1, refresh)), "every band and an IDR picture occur"
    assert any(s.idr for s in seq[1:]) or len(script) > 256


def test_item_g_of_a_direct_batch(harness):
    """item g differs from item 0 in `item` and in idr_pic_id, which steps by the engine's stride and wraps at 256"""
    assert harness("batch", 250, 3, 4) == [["0", "250"], ["1", "253"], ["2", "0"], ["3", "3"]]
    assert harness("batch", 255, 1, 3) == [["0", "255"], ["1", "0"], ["2", "1"]]
    assert harness("batch", 7, 0, 2) == [["0", "7"], ["1", "7"]]
    got = harness("batch", 0, 5, 64)
    assert [int(g[1]) for g in got] == [(5 * g) & 255 for g in range(64)] and int(got[52][1]) == 4


def test_the_harness_under_sanitizers(harness, tmp_path):
    """built once more with AddressSanitizer and UBSan and run as a program: the same lines, nothing on stderr.  The source compiled
    without them above: only a toolchain that lacks the sanitizers' runtime is a reason to skip"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "pic_seq_harness_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer build not available: " + r.stderr[-200:])
    san = _runner(exe)
    for args in (("words",) + CASES[0], ("words",) + CASES[5], ("pack", 255, 3, 63, 3, 3, 62), ("pack", 256, 4, 64, 4, 4, 63), ("pack", -1, -1, -1, -1, -1, -2),
                 ("batch", 250, 3, 4), (2, 7, 1, 2, 24, "....I..F..."), ("refresh", 3, 100, "....I....F..")):
        assert san(*args) == harness(*args), args
