"""Decoder groups on the GPU (mi355x_h264_dec_group_*, media_amd.h264dec.DecoderGroup): the pictures of many streams reconstructed
in one step.  Every picture of every stream of every case of tests/dec_group.py (tests/test_dec_group_oracle.py proves what the
cases hold) must equal the oracle's independent decoder's, sample for sample, and what one Decoder per stream gives."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dec_group as dg
from media_amd import h264dec
from media_amd.capi import lib, EncoderError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_STREAM = -1, h264dec.E_STREAM


def check_stream(grp, k, want, bad, tag):
    """stream k's last picture against (access unit, planes, cropped I420, size) of the oracle decoder"""
    _, planes, i420, size = want
    got = grp.debug_planes(k)
    for p in range(3):
        if not np.array_equal(got[p], planes[p]):
            bad.append("%s stream %d plane %d: %d samples differ" % (tag, k, p, int((got[p] != planes[p]).sum())))
    if grp.info(k)[:2] != size:
        bad.append("%s stream %d: picture_info %s, the oracle decoder %s" % (tag, k, grp.info(k), size))
    elif not np.array_equal(grp.read_i420(k), i420):
        bad.append("%s stream %d: read_i420" % (tag, k))
    return got


def run_case(case, singles=True, schedule=None):
    """the case through a group, every stream's every picture compared; returns the list of differences.  schedule(t, k): stream k
    takes part in call t (it is then handed its next picture)"""
    import torch
    S = len(case.streams)
    want = [dg.stream_pictures(case, k) for k in range(S)]
    single = []
    if singles:   # one Decoder per stream, one after the other: what each stream decodes to alone
        for k in range(S):
            d = h264dec.Decoder()
            single.append([])
            for au, _, _, _ in want[k]:
                assert d.decode(au)
                single[k].append(dg.digest([d.plane(p) for p in range(3)]) + dg.digest([d.i420()]))
            d.close()
    grp = h264dec.DecoderGroup(S)
    bad, nxt, t = [], [0] * S, 0
    while min(nxt) < case.pictures and t < 8 * case.pictures:
        part = [k for k in range(S) if nxt[k] < case.pictures and (schedule is None or schedule(t, k))]
        aus = [want[k][nxt[k]][0] if k in part else None for k in range(S)]
        res = grp.decode(aus)
        step = grp.last_step()
        if step["pictures"] != len(part):
            bad.append("call %d: the step carried %d pictures of %d" % (t, step["pictures"], len(part)))
        for k in range(S):
            if res[k] != ((0, 1) if k in part else (0, 0)):
                bad.append("call %d stream %d: (rc, got) = %s: %s" % (t, k, res[k], grp.error(k)))
        for k in part:
            got = check_stream(grp, k, want[k][nxt[k]], bad, "call %d" % t)
            w, h = want[k][nxt[k]][3]
            dev = torch.zeros(w * h * 3 // 2, dtype=torch.uint8, device="cuda")
            if grp.read_i420_device(k, dev) != dev.numel() or not np.array_equal(dev.cpu().numpy(), want[k][nxt[k]][2]):
                bad.append("call %d stream %d: read_i420_device" % (t, k))
            if singles and single[k][nxt[k]] != dg.digest(got) + dg.digest([grp.read_i420(k)]):
                bad.append("call %d stream %d: differs from the single decoder" % (t, k))
            nxt[k] += 1
        t += 1
    grp.close()
    if min(nxt) < case.pictures:
        bad.append("the schedule did not finish")
    return bad


@pytest.mark.parametrize("case", dg.CASES, ids=[c.name for c in dg.CASES])
def test_group_equals_the_oracle_decoder_and_the_single_decoders(case):
    bad = run_case(case)
    assert not bad, bad[:8]


def expected_shape(infos):
    """launches and transfers of a step from what its pictures hold (media_amd/csrc/dec_group.h): widen, [patch], [inter, resid],
    [intra rows], [strengths, filter without bS 4, filter with]; six arrays + table, [vectors, reference indices], [large levels]"""
    inter = any(i["kinds"] & 2 for i in infos)
    intra = any(i["kinds"] & 1 for i in infos)
    big = any(i["big"] for i in infos)
    plain = any(i["deblock_idc"] != 1 and not i["kinds"] & 1 for i in infos)
    bs4 = any(i["deblock_idc"] != 1 and i["kinds"] & 1 for i in infos)
    return 1 + big + 2 * inter + intra + (1 + plain + bs4 if plain or bs4 else 0), 7 + 2 * inter + big


def test_step_shape_does_not_grow_with_the_streams():
    """a step's launches and transfers follow from the KINDS of its pictures, not from their number.  The 1-stream case against a
    group of twelve streams that are all that stream (the same picture kinds in every step): the same launches and transfers,
    step by step.  And in the 1-stream and the 12-stream case of the list, every step makes what the kinds of its pictures say.
    A build that loops over streams fails both."""
    from test_dec_group_oracle import parsed
    one = dg.BY_NAME["one_96x80"]
    aus = [au for au, _, _, _ in dg.stream_pictures(one, 0)]
    shapes = {}
    for S in (1, 12):
        grp = h264dec.DecoderGroup(S)
        shapes[S] = []
        for t, au in enumerate(aus):
            assert grp.decode([au] * S) == [(0, 1)] * S
            step = grp.last_step()
            assert step["pictures"] == S
            shapes[S].append((step["launches"], step["transfers"]))
        bad = []
        for k in (0, S - 1):
            check_stream(grp, k, dg.stream_pictures(one, 0)[-1], bad, "%d copies" % S)
        assert not bad, bad
        grp.close()
    assert shapes[1] == shapes[12], (shapes[1], shapes[12])
    for name in ("one_96x80", "twelve_96x80"):
        case = dg.BY_NAME[name]
        infos, S = parsed(case), len(case.streams)
        grp = h264dec.DecoderGroup(S)
        for t in range(case.pictures):
            grp.decode([dg.stream_pictures(case, k)[t][0] for k in range(S)])
            step = grp.last_step()
            assert step["pictures"] == S
            assert (step["launches"], step["transfers"]) == expected_shape(infos[t]), (name, t, step)
            assert step["launches"] <= 9 and step["transfers"] <= 10
            assert 1 <= step["parse_threads"] <= min(S, 8)
        grp.sync()
        grp.close()


def test_streams_that_sit_out_and_empty_units():
    case = dg.BY_NAME["five_64x48"]
    bad = run_case(case, singles=False, schedule=lambda t, k: (t * 7 + k * 3) % 5 < 2 or (t % 6 == 5 and k == 2) or t > 30)
    assert not bad, bad[:8]
    one = run_case(case, singles=False, schedule=lambda t, k: k == t % 5)   # one participant per call
    assert not one, one[:8]
    # an access unit of parameter sets only: no picture, no error, the stream decodes on
    import annexb
    S = len(case.streams)
    grp = h264dec.DecoderGroup(S)
    first = [dg.stream_pictures(case, k)[0] for k in range(S)]
    sets = b"".join(b"\x00\x00\x00\x01" + bytes([(ref << 5) | typ]) + payload for ref, typ, payload in annexb.split_nal_units(first[1][0]) if typ in (7, 8))
    assert sets
    res = grp.decode([first[0][0], sets] + [None] * (S - 2))
    assert res[0] == (0, 1) and res[1] == (0, 0) and grp.last_step()["pictures"] == 1
    res = grp.decode([None, first[1][0]] + [None] * (S - 2))
    assert res[1] == (0, 1)
    bad = []
    check_stream(grp, 0, first[0], bad, "after")
    check_stream(grp, 1, first[1], bad, "after")
    assert not bad, bad
    grp.close()


def test_a_failing_stream_fails_alone():
    case = dg.BY_NAME["five_64x48"]
    S, n = len(case.streams), case.pictures
    want = [dg.stream_pictures(case, k) for k in range(S)]
    victim = 3        # the oracle encoder's stream: gop 6, IDR pictures at 0 and 6
    grp = h264dec.DecoderGroup(S)
    alone = h264dec.Parser()    # the victim's units through the host parser alone: the message each refusal must carry
    bad, refused = [], 0
    for t in range(n):
        aus = [want[k][t][0] for k in range(S)]
        if t == 2:
            aus[victim] = aus[victim][: len(aus[victim]) * 3 // 5]   # truncated in the middle of its slice data
        said = ""
        try:
            alone.parse(aus[victim])
        except h264dec.StreamError as ex:
            said = str(ex)
        res = grp.decode(aus)
        for k in range(S):
            if k == victim and 2 <= t < 6:
                assert res[k] == (E_STREAM, 0), (t, res[k])
                # the message names what the parser met: the very words the parser alone has for this unit
                assert said and grp.error(k) == said, (t, grp.error(k), said)
                refused += 1
                if t > 2:
                    assert "reference" in grp.error(k), grp.error(k)
            else:
                assert res[k] == (0, 1), (t, k, res[k], grp.error(k))
                assert grp.error(k) == "", (t, k, grp.error(k))    # nobody else is told anything
                check_stream(grp, k, want[k][t], bad, "step %d" % t)
        if not 2 <= t < 6:
            assert said == "", (t, said)
        assert grp.last_step()["pictures"] == (S - 1 if 2 <= t < 6 else S)
    assert refused == 4 and not bad, bad[:8]
    # a stream of another coded size is refused by name of both sizes; the others go on
    other = dg.stream_pictures(dg.BY_NAME["one_96x80"], 0)[0][0]
    res = grp.decode([want[0][0][0], other] + [want[k][0][0] for k in range(2, S)])
    assert res[1] == (E_STREAM, 0) and "96x80" in grp.error(1) and "64x48" in grp.error(1), grp.error(1)
    assert all(res[k] == (0, 1) and grp.error(k) == "" for k in range(S) if k != 1)
    check_stream(grp, 0, want[0][0], bad, "after the refusal")
    assert not bad, bad
    grp.close()
    alone.close()
    # tests/golden/dec_damaged_i4_topright.h264 is a CONFORMING picture (tests/test_gpu_decoder.py says how it came about): one of
    # its Intra4x4 blocks reads the macroblock above-right.  No isolation check: it is decoded in a group and compared with the
    # oracle decoder, which covers the above-right wait of k_pintra_rows<true, true>
    au = open(os.path.join(ROOT, "tests", "golden", "dec_damaged_i4_topright.h264"), "rb").read()
    from oracle_lib import OracleDecoder
    ref = OracleDecoder()
    assert ref.decode(au) == 1
    g2 = h264dec.DecoderGroup(2)
    assert g2.decode([None, au]) == [(0, 0), (0, 1)]
    for p in range(3):
        assert np.array_equal(g2.debug_planes(1)[p], ref.plane(p))
    g2.close()


def child(case, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dec_group_child.py"), case], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **env))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["case"] == case and out["differences"] == [], out["differences"][:8]


def test_without_look_ahead_in_a_fresh_process():
    child("twelve_96x80", {"MI355X_H264_DEC_SYNC": "1"})


def test_forty_streams_walk_three_pictures_at_a_time_in_a_fresh_process():
    child("forty_32x32", {"MI355X_H264_DEC_INTRA_SLOTS": "3", "MI355X_H264_DEC_FILTER_SLOTS": "3"})


def test_arguments():
    import ctypes as C
    L = h264dec._bind()
    h = C.c_void_p()
    assert L.mi355x_h264_dec_group_create(0, 0, C.byref(h)) == E_ARG and L.mi355x_h264_dec_group_create(0, 65, C.byref(h)) == E_ARG
    assert L.mi355x_h264_dec_group_create(0, 2, None) == E_ARG
    grp = h264dec.DecoderGroup(2)
    got, rc = (C.c_int * 2)(), (C.c_int * 2)()
    assert L.mi355x_h264_dec_group_decode(grp.h, None, None, got, rc) == E_ARG
    buf = np.zeros(64, np.uint8)
    for s in (-1, 2):
        assert L.mi355x_h264_dec_group_read_i420(grp.h, s, buf.ctypes.data, 64) == E_ARG
        assert L.mi355x_h264_dec_group_debug_plane(grp.h, s, 0, buf.ctypes.data, 64) == E_ARG
        assert L.mi355x_h264_dec_group_picture_info(grp.h, s, None, None, None, None) == E_ARG
    assert L.mi355x_h264_dec_group_read_i420(grp.h, 0, buf.ctypes.data, 64) == E_ARG    # no picture yet
    with pytest.raises(EncoderError):
        grp.decode([None])
    grp.close()
