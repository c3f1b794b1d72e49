"""What a decoder group holds (media_amd/csrc/pic_store.h, dec_group.h): last_step()'s device_bytes / pinned_bytes against a budget
this file states itself, array by array - the picture store's ring and per-macroblock arrays, the group's own device arrays and its
two pinned sets - and nothing of an encoder's.  The library is not asked what it allocates.

Over the budget, 2 % + 64 KB are allowed for what does not scale with the picture: position tables, flag arrays, the time-out
word, 256-byte pads, the lists of large levels at their smallest size (about 8 KB each).  For four_176x144 the budget is 1 256 520
device bytes and 435 600 pinned bytes; an encoder engine underneath (the parent of this change) adds about 1.7 MB and 1.4 MB to
them: three access-unit slots of 116 480 bytes per stream, each on the device and in pinned memory."""
import numpy as np
import pytest

import dec_group as dg
from media_amd import h264dec
from test_gpu_dec_group import check_stream

pytestmark = pytest.mark.gpu

NBUF = 4   # ring slots per stream: the picture being written and three reference pictures
# bytes per macroblock on the device: MbInfo, levels (416 int16), quadrant vectors, Intra4x4 modes, boundary strengths, 24 hand-off
# granules of 8 bytes, 8-bit levels, QP, availability, vectors per 4x4 block, reference indices
DEVICE_PER_MB = 32 + 832 + 16 + 16 + 32 + 24 * 8 + 416 + 1 + 1 + 64 + 4
# what the parser's picture is copied into, twice (the sets take turns): all of the above that comes from the host
PINNED_PER_MB = 2 * (32 + 16 + 16 + 416 + 1 + 1 + 64 + 4)
DEC_POS, DEC_OUT_POS = 32, 48   # bytes of a row of the position table / of the table of output positions


def budget(w, h, streams):
    """(device bytes, pinned bytes) of an unarmed group of `streams` streams of w x h"""
    cw, ch = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    ring_slot = cw * ch + 256 + 2 * (cw * ch // 4 + 256)
    mbs = cw * ch // 256
    return streams * (NBUF * ring_slot + mbs * DEVICE_PER_MB), streams * mbs * PINNED_PER_MB


def within(step, want, tag, armed=(0, 0)):
    """the listed arrays are all counted, and no more than the allowance (2 % of the unarmed budget + 64 KB) on top of them"""
    for key, b, more in zip(("device_bytes", "pinned_bytes"), want, armed):
        print("%s: %s %d, budget %d, allowed %d" % (tag, key, step[key], b + more, b + more + b // 50 + 65536))
        assert b + more <= step[key] <= b + more + b // 50 + 65536, (tag, key, step[key], b, more)


def test_the_budget_is_the_one_stated():
    assert (DEVICE_PER_MB, PINNED_PER_MB) == (1606, 2 * 550)
    assert budget(176, 144, 4) == (1256520, 435600)


def test_a_group_holds_its_store_and_its_sets_and_does_not_grow():
    case = dg.BY_NAME["four_176x144"]
    S = len(case.streams)
    want = [dg.stream_pictures(case, k) for k in range(S)]
    grp = h264dec.DecoderGroup(S)
    bad, held = [], []
    for t in range(case.pictures):
        assert grp.decode([want[k][t][0] for k in range(S)]) == [(0, 1)] * S
        for k in range(S):
            check_stream(grp, k, want[k][t], bad, "step %d" % t)
        if t in (0, case.pictures - 1):
            step = grp.last_step()
            within(step, budget(case.w, case.h, S), "step %d" % t)
            held.append((step["device_bytes"], step["pinned_bytes"]))
    assert not bad, bad[:8]
    assert held[0] == held[1], held
    grp.close()


def test_the_decoder_frees_the_old_size_through_the_store():
    """64x48, then an IDR picture of 96x80: what the decoder holds afterwards fits the budget of 96x80 alone"""
    small, big = dg.stream_pictures(dg.BY_NAME["five_64x48"], 0), dg.stream_pictures(dg.BY_NAME["one_96x80"], 0)
    dec = h264dec.Decoder()
    for tag, (au, planes, i420, size), (w, h) in (("64x48", small[0], (64, 48)), ("96x80", big[0], (96, 80))):
        assert dec.decode(au), tag
        for p in range(3):
            assert np.array_equal(dec.plane(p), planes[p]), "%s plane %d" % (tag, p)
        assert dec.info()[:2] == size and np.array_equal(dec.i420(), i420), tag
        within(dec.last_step(), budget(w, h, 1), tag)
    dec.close()


def test_an_armed_group_adds_its_output_buffers():
    """set_output(I420): two pinned sets and one device staging buffer of streams x align256(picture bytes at the coded size), and the
    combined position tables (DecPos and output rows of every stream: two pinned, one on the device)"""
    case = dg.BY_NAME["five_64x48"]
    S = len(case.streams)
    want = [dg.stream_pictures(case, k) for k in range(S)]
    grp = h264dec.DecoderGroup(S)
    grp.set_output(h264dec.PIX_I420)
    picture = (case.w * case.h * 3 // 2 + 255) // 256 * 256
    tables = S * (DEC_POS + DEC_OUT_POS)
    bad = []
    for t in range(3):
        assert grp.decode([want[k][t][0] for k in range(S)]) == [(0, 1)] * S
        data, pics = grp.output(0)
        for k in range(S):
            check_stream(grp, k, want[k][t], bad, "step %d" % t)
            o = pics[k]["offset"]
            if not np.array_equal(data[o:o + want[k][t][2].size], want[k][t][2]):
                bad.append("step %d stream %d: armed output" % (t, k))
        within(grp.last_step(), budget(case.w, case.h, S), "armed step %d" % t, armed=(S * picture + tables, 2 * S * picture + 2 * tables))
    assert not bad, bad[:8]
    grp.close()
