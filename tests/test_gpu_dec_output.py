"""Decoder output in four layouts on the GPU (mi355x_h264_dec_read, mi355x_h264_dec_group_read_all / _set_output / _output;
media_amd/csrc/k_dec_out.h).  Every comparison is exact: the expected bytes are tests/dec_output.pack() of the oracle decoder's
cropped I420 pictures (tests/test_dec_output_oracle.py proves the restatement and what the case list holds).  Every test ends by
asserting that each stream of its case was compared in each layout it names."""
import ctypes as C

import numpy as np
import pytest

import dec_group as dg
import dec_output as do
from media_amd import h264dec
from media_amd.capi import EncoderError

pytestmark = pytest.mark.gpu
E_ARG = -1
KEYS = ("offset", "width", "height", "stride", "chroma_stride")


def same_desc(got, want):
    return all(got[k] == want[k] for k in KEYS)


class Seen:
    """which (stream, layout) pairs a test compared"""

    def __init__(self, case, layouts):
        self.need = {(k, lay) for k in range(len(case.streams)) for lay in layouts}
        self.seen = set()

    def add(self, k, lay):
        self.seen.add((k, lay))

    def check(self):
        assert self.need <= self.seen, sorted(self.need - self.seen)[:8]


def decode_steps(case, schedule=None):
    """drives a group through the case: yields (grp, t, part, last) after every call; last[k] = the index of stream k's last
    decoded picture or None"""
    S = len(case.streams)
    grp = h264dec.DecoderGroup(S)
    nxt, t = [0] * S, 0
    try:
        while min(nxt) < case.pictures and t < 8 * case.pictures:
            part = [k for k in range(S) if nxt[k] < case.pictures and (schedule is None or schedule(t, k))]
            res = grp.decode([do.pictures(case, k)[nxt[k]][0] if k in part else None for k in range(S)])
            assert all(res[k] == ((0, 1) if k in part else (0, 0)) for k in range(S)), res
            for k in part:
                nxt[k] += 1
            yield grp, t, part, [n - 1 if n else None for n in nxt]
            t += 1
        assert min(nxt) == case.pictures
    finally:
        grp.close()


def expected(case, last, only=None):
    return [None if last[k] is None or (only is not None and k not in only) else (do.pictures(case, k)[last[k]][2], do.pictures(case, k)[last[k]][3])
            for k in range(len(case.streams))]


ALIGNS = {"out_50x34": (1, 64, 256)}


@pytest.mark.parametrize("case", do.CASES, ids=[c.name for c in do.CASES])
def test_read_all_to_host_and_device(case):
    import torch
    seen = Seen(case, do.LAYOUTS)
    sched = do.SCHEDULES.get(case.name)
    S = len(case.streams)
    for grp, t, part, last in decode_steps(case, sched):
        pics = expected(case, last)
        # every layout after every call on the small cases; the larger ones rotate through the layouts
        lays = do.LAYOUTS if S <= 5 else (do.LAYOUTS[t % 4], do.LAYOUTS[(t + 1) % 4]) if t + 1 < case.pictures else do.LAYOUTS
        for lay in lays:
            for ra in ALIGNS.get(case.name, (1, 64)):
                want, written, desc, total = do.pack(pics, lay, ra)
                # sizing: no GPU work, the same answer before and after
                sized = (h264dec.OutPic * S)()
                assert h264dec.lib().mi355x_h264_dec_group_read_all(grp.h, lay, ra, None, 0, 0, sized) == total
                buf, got = grp.read_all(lay, ra)
                step = grp.last_step()
                assert (step["read_launches"], step["read_transfers"]) == (1, 1)
                assert buf.size == total == grp.read_bytes
                for k in range(S):
                    assert same_desc(got[k], desc[k]) and same_desc(sized[k].as_dict(), desc[k]), (t, k, got[k], desc[k])
                    if last[k] is not None:
                        assert got[k]["fresh"] == (1 if k in part else 0) and got[k]["serial"] == step["serial"], (t, k, got[k])
                assert np.array_equal(buf[written], want[written]), (t, lay, ra, int((buf[written] != want[written]).sum()))
                # into device memory: rows only, every other byte of the tensor keeps its 0xA5
                dev = torch.full((total + 512,), 0xA5, dtype=torch.uint8, device="cuda")
                _, got_d = grp.read_all(lay, ra, device_tensor=dev)
                step = grp.last_step()
                assert (step["read_launches"], step["read_transfers"]) == (1, 0) and grp.read_bytes == total
                want_d = do.pack(pics, lay, ra, size=total + 512)[0]
                assert np.array_equal(dev.cpu().numpy(), want_d), (t, lay, ra)
                assert all(same_desc(got_d[k], desc[k]) for k in range(S))
                again = (h264dec.OutPic * S)()
                assert h264dec.lib().mi355x_h264_dec_group_read_all(grp.h, lay, ra, None, 0, 0, again) == total
                assert all(same_desc(again[k].as_dict(), desc[k]) for k in range(S))
                for k in range(S):
                    if last[k] is not None:
                        seen.add(k, lay)
            if lay == do.I420:   # the tight form is the concatenation of read_i420(k), each at its 256-byte start
                buf, got = grp.read_all(do.I420, 1)
                for k in range(S):
                    if last[k] is not None:
                        one = grp.read_i420(k)
                        assert np.array_equal(buf[got[k]["offset"]:got[k]["offset"] + one.size], one), (t, k)
    seen.check()


@pytest.mark.parametrize("name", sorted(do.SCHEDULES))
def test_armed_output_follows_every_step(name):
    """output(0) after every step = exactly the streams that took part; output(1) after the following call = what output(0) gave
    for that step, although the next step may have written the very ring slot (the picture before was a non-reference picture)"""
    case = do.BY_NAME[name]
    S = len(case.streams)
    seen = Seen(case, do.LAYOUTS)
    for lay, ra in zip(do.LAYOUTS, (1, 64, 1, 64)):
        prev = None
        armed_steps = 0
        for grp, t, part, last in decode_steps(case, do.SCHEDULES[name]):
            if t == 0:
                grp.set_output(lay, ra)
                continue   # armed from the next step on
            step = grp.last_step()
            if not part:
                assert (step["output_launches"], step["output_transfers"]) == (0, 0)
                continue
            assert (step["output_launches"], step["output_transfers"]) == (1, 1), step
            armed_steps += 1
            if prev is not None:   # before waiting for this step: the step before it, complete
                data1, pics1 = grp.output(1)
                assert np.array_equal(data1, prev[0]) and pics1 == prev[1], (t, lay)
            elif armed_steps == 1:
                with pytest.raises(EncoderError):
                    grp.output(1)
            data, pics = grp.output(0)
            want, written, desc, total = do.pack(expected(case, last, only=part), lay, ra)
            assert data.size == total
            for k in range(S):
                assert same_desc(pics[k], desc[k]), (t, k, pics[k], desc[k])
                assert (pics[k]["offset"] >= 0) == (k in part)
                if k in part:
                    assert pics[k]["fresh"] == 1 and pics[k]["serial"] == step["serial"]
                    seen.add(k, lay)
            assert np.array_equal(data[written], want[written]), (t, lay, int((data[written] != want[written]).sum()))
            prev = (data.copy(), pics)
    seen.check()


def test_disarm_and_step_shape():
    """an armed step adds one launch and one transfer at 1, 12, 40 and 64 streams, and its reconstruction launches and
    host-to-device transfers stay what the kinds of its pictures say; set_output(-1) takes both away again"""
    from test_dec_group_oracle import parsed
    from test_gpu_dec_group import expected_shape
    for name in ("one_96x80", "twelve_96x80", "forty_32x32", "sixtyfour_32x32"):
        case = do.BY_NAME.get(name) or dg.BY_NAME[name]
        S = len(case.streams)
        seen = Seen(case, (do.NV12,))
        infos = parsed(dg.BY_NAME[name]) if name in dg.BY_NAME else None
        grp = h264dec.DecoderGroup(S)
        grp.set_output(do.NV12, 16)
        for t in range(min(case.pictures, 3)):
            grp.decode([do.pictures(case, k)[t][0] for k in range(S)])
            step = grp.last_step()
            assert step["pictures"] == S and (step["output_launches"], step["output_transfers"]) == (1, 1), (name, t, step)
            if infos:
                assert (step["launches"], step["transfers"]) == expected_shape(infos[t]), (name, t, step)
            data, pics = grp.output(0)
            want, written, desc, _ = do.pack([(do.pictures(case, k)[t][2], do.pictures(case, k)[t][3]) for k in range(S)], do.NV12, 16)
            assert np.array_equal(data[written], want[written]) and all(same_desc(pics[k], desc[k]) for k in range(S)), (name, t)
            for k in range(S):
                seen.add(k, do.NV12)
        grp.set_output(-1)
        assert (grp.last_step()["output_launches"], grp.last_step()["output_transfers"]) == (0, 0)
        with pytest.raises(EncoderError):
            grp.output(0)
        if case.pictures > 3:
            grp.decode([do.pictures(case, k)[3][0] for k in range(S)])
            step = grp.last_step()
            assert (step["output_launches"], step["output_transfers"]) == (0, 0)
            if infos:
                assert (step["launches"], step["transfers"]) == expected_shape(infos[3])
        grp.close()
        seen.check()


def test_single_decoder_read_equals_the_groups():
    import torch
    case = do.BY_NAME["out_50x34"]
    S = len(case.streams)
    seen = Seen(case, do.LAYOUTS)
    decs = [h264dec.Decoder() for _ in range(S)]
    for grp, t, part, last in decode_steps(case):
        for k in range(S):
            assert decs[k].decode(do.pictures(case, k)[t][0])
        for lay in do.LAYOUTS:
            for ra in (1, 64):
                buf, pics = grp.read_all(lay, ra)
                for k in range(S):
                    one, pic = decs[k].read(lay, ra)
                    i420, size = do.pictures(case, k)[t][2], do.pictures(case, k)[t][3]
                    want, written, desc, total = do.pack([(i420, size)], lay, ra)
                    assert one.size == total == pic["bytes"] and same_desc(pic, desc[0]) and pic["fresh"] == 1
                    assert np.array_equal(one[written], want[written]), (t, k, lay, ra)
                    assert np.array_equal(buf[pics[k]["offset"]:pics[k]["offset"] + total][written], one[written])
                    dev = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                    decs[k].read(lay, ra, device_tensor=dev)
                    assert np.array_equal(dev.cpu().numpy(), do.pack([(i420, size)], lay, ra, size=total + 64)[0]), (t, k, lay, ra)
                    seen.add(k, lay)
    for d in decs:
        d.close()
    seen.check()


def test_arguments():
    L = h264dec._bind()
    case = do.BY_NAME["out_18x18"]
    S = len(case.streams)
    seen = Seen(case, (do.I420,))
    grp = h264dec.DecoderGroup(S)
    dec = h264dec.Decoder()
    pics, pic = (h264dec.OutPic * S)(), h264dec.OutPic()
    buf = np.zeros(1 << 16, np.uint8)
    data = C.c_void_p()
    # no picture yet
    assert L.mi355x_h264_dec_group_read_all(grp.h, 0, 1, buf.ctypes.data, buf.nbytes, 0, pics) == E_ARG
    assert L.mi355x_h264_dec_group_read_all(grp.h, 0, 1, None, 0, 0, pics) == E_ARG
    assert L.mi355x_h264_dec_read(dec.h, 0, 1, buf.ctypes.data, buf.nbytes, 0, C.byref(pic)) == E_ARG
    assert L.mi355x_h264_dec_group_output(grp.h, 0, C.byref(data), pics) == E_ARG          # unarmed
    grp.decode([do.pictures(case, 0)[0][0], None])
    assert dec.decode(do.pictures(case, 0)[0][0])
    before, got = grp.read_all(do.I420, 1)
    assert got[1]["offset"] == -1 and got[0]["offset"] == 0                                 # a stream without a picture is left out
    need = before.size
    for lay, ra, cap in ((-1, 1, need), (4, 1, need), (0, 0, need), (0, 3, need), (0, 48, need), (0, 512, need), (0, 1, need - 1)):
        assert L.mi355x_h264_dec_group_read_all(grp.h, lay, ra, buf.ctypes.data, cap, 0, pics) == E_ARG, (lay, ra, cap)
        assert L.mi355x_h264_dec_read(dec.h, lay, ra, buf.ctypes.data, cap, 0, C.byref(pic)) == E_ARG, (lay, ra, cap)
        if lay != -1 and cap == need:   # (-1 disarms; the pair of the cap case is a good one)
            assert L.mi355x_h264_dec_group_set_output(grp.h, lay, ra) == E_ARG, (lay, ra)
    assert L.mi355x_h264_dec_group_read_all(grp.h, 0, 1, buf.ctypes.data, buf.nbytes, 0, None) == E_ARG
    # nothing changed: still unarmed, the same picture, the same counts
    grp.set_output(-1)
    assert L.mi355x_h264_dec_group_output(grp.h, 0, C.byref(data), pics) == E_ARG
    after, _ = grp.read_all(do.I420, 1)
    assert np.array_equal(before, after) and np.array_equal(after, do.pictures(case, 0)[0][2])
    assert np.array_equal(dec.read(do.I420, 1)[0], dec.i420())
    seen.add(0, do.I420)
    # armed: back = 1 needs two steps, back outside 0 / 1 is refused
    grp.set_output(do.I420, 1)
    assert L.mi355x_h264_dec_group_output(grp.h, 0, C.byref(data), pics) == E_ARG          # no armed step yet
    grp.decode([do.pictures(case, 0)[1][0], do.pictures(case, 1)[0][0]])
    assert L.mi355x_h264_dec_group_output(grp.h, 1, C.byref(data), pics) == E_ARG
    assert L.mi355x_h264_dec_group_output(grp.h, 2, C.byref(data), pics) == E_ARG
    out, got = grp.output(0)
    want, written, _, _ = do.pack([(do.pictures(case, 0)[1][2], do.pictures(case, 0)[1][3]), (do.pictures(case, 1)[0][2], do.pictures(case, 1)[0][3])], do.I420, 1)
    assert np.array_equal(out[written], want[written])
    seen.add(1, do.I420)
    grp.close()
    dec.close()
    seen.check()
