"""Decoder output at a requested size on the GPU (include/mi355x_h264_dec.h, "output size"; media_amd/csrc/k_dec_out_scale.h).
Every comparison is exact: the expected bytes are dec_output.pack() of the oracle decoder's cropped pictures resampled by
scale.scale_i420() (tests/dec_scale.py; tests/test_dec_scale_oracle.py proves what the case list holds).  RGBA of a described
stream: the conversion of tests/colour.py on the resampled planes."""
import ctypes as C

import numpy as np
import pytest

import colour as col
import dec_output as do
import dec_scale as ds
import mem_guard as mg
import scale
import value_cube as vc
from media_amd import capi, h264dec, synth
from media_amd import videodecoder as vd
from media_amd.capi import EncoderError
from oracle_lib import OracleDecoder
from test_dec_scale_host import REFUSED, TAKEN
from test_gpu_colour_decoder import unit
from test_gpu_dec_output import same_desc

pytestmark = pytest.mark.gpu
E_ARG = -1
COMBOS = [(lay, ra) for lay in do.LAYOUTS for ra in ds.ROW_ALIGNS]
IDS = [c.name for c in ds.CASES]


def au_of(src, k, t):
    return do.pictures(src, k)[t][0]


def output_copy(grp, back=0):
    """output(back) with the bytes copied out of the pinned set: the set is freed when the group is closed, and a failing
    comparison is reported after that, with the arrays it was handed printed"""
    data, pics = grp.output(back)
    return data.copy(), pics


def same_bytes(got, want, written, what):
    bad = got[written] != want[written]
    print("%s: %d of %d bytes differ" % (what, int(bad.sum()), int(written.sum())))
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:8].tolist())


@pytest.mark.parametrize("case", ds.CASES, ids=IDS)
def test_decoder_read_to_host_and_to_device(case):
    """Decoder.read of a stream of every cropped size of the case, all layouts and alignments: to host, and into a device tensor
    filled with 0xA5 that is compared whole (pack's `written` mask: every byte outside the rows keeps its 0xA5)"""
    import torch
    src = ds.source(case)
    first = {}
    for k in range(len(src.streams)):
        first.setdefault(ds.size_of(case, k), k)
    streams = range(len(src.streams)) if len(src.streams) <= 4 else sorted(first.values())
    for k in streams:
        W, H = ds.target_of(case, k)
        dec = h264dec.Decoder()
        try:
            dec.set_output_size(W, H)
            assert dec.output_size() == (W, H)
            for t in range(ds.STEPS):
                assert dec.decode(au_of(src, k, t))
                assert dec.info()[:2] == ds.size_of(case, k), "picture_info stays at the native size"
                assert np.array_equal(dec.i420(), do.pictures(src, k)[t][2]), "read_i420 stays at the native size"
                pic = (ds.scaled(case.source, k, t, W, H), (W, H))
                for lay, ra in COMBOS:
                    want, written, desc, total = do.pack([pic], lay, ra)
                    sized = h264dec.OutPic()
                    assert h264dec.lib().mi355x_h264_dec_read(dec.h, lay, ra, None, 0, 0, C.byref(sized)) == total
                    got, p = dec.read(lay, ra)
                    assert got.size == total == p["bytes"] and same_desc(p, desc[0]) and same_desc(sized.as_dict(), desc[0]), (k, t, lay, ra, p, desc[0])
                    assert (p["width"], p["height"], p["fresh"]) == (W, H, 1)
                    step = dec.last_step()
                    assert (step["read_launches"], step["read_transfers"]) == (1, 1), step
                    same_bytes(got, want, written, "%s stream %d picture %d layout %d align %d, host" % (case.name, k, t, lay, ra))
                    dev = torch.full((total + 512,), 0xA5, dtype=torch.uint8, device="cuda")
                    dec.read(lay, ra, device_tensor=dev)
                    step = dec.last_step()
                    assert (step["read_launches"], step["read_transfers"]) == (1, 0), step
                    want_d = do.pack([pic], lay, ra, size=total + 512)[0]
                    got_d = dev.cpu().numpy()
                    same_bytes(got_d, want_d, np.ones(want_d.size, bool), "%s stream %d picture %d layout %d align %d, device" % (case.name, k, t, lay, ra))
        finally:
            dec.close()


@pytest.mark.parametrize("case", ds.CASES, ids=IDS)
def test_group_read_all_and_armed_output(case):
    """the whole group of the case, every stream at its size: read_all after every step in all layouts and alignments, then armed
    in every layout and alignment (the streams start again at their IDR pictures): output(0) of every step, output(1) of the one before"""
    src = ds.source(case)
    S = len(src.streams)
    tg = ds.targets(case)
    grp = h264dec.DecoderGroup(S)
    try:
        for k in range(S):
            grp.set_output_size(k, *tg[k])
        assert [grp.output_size(k) for k in range(S)] == [tuple(t) for t in tg]
        for t in range(ds.STEPS):
            assert grp.decode([au_of(src, k, t) for k in range(S)]) == [(0, 1)] * S
            pics = ds.expected_pics(case.source, tg, [t] * S)
            for lay, ra in COMBOS:
                want, written, desc, total = do.pack(pics, lay, ra)
                buf, got = grp.read_all(lay, ra)
                step = grp.last_step()
                assert (step["read_launches"], step["read_transfers"]) == (1, 1), step
                assert buf.size == total and all(same_desc(got[k], desc[k]) for k in range(S)), (t, lay, ra)
                same_bytes(buf, want, written, "%s step %d layout %d align %d, read_all" % (case.name, t, lay, ra))
        for lay, ra in COMBOS:
            grp.set_output(lay, ra)
            prev = None
            for t in range(ds.STEPS):
                assert grp.decode([au_of(src, k, t) for k in range(S)]) == [(0, 1)] * S
                step = grp.last_step()
                assert (step["output_launches"], step["output_transfers"]) == (1, 1), step
                if prev is not None:
                    data1, pics1 = output_copy(grp, 1)
                    assert np.array_equal(data1, prev[0]) and pics1 == prev[1], (t, lay, ra)
                data, got = output_copy(grp)
                want, written, desc, total = do.pack(ds.expected_pics(case.source, tg, [t] * S), lay, ra)
                assert data.size == total and all(same_desc(got[k], desc[k]) and got[k]["fresh"] == 1 for k in range(S)), (t, lay, ra)
                same_bytes(data, want, written, "%s step %d layout %d align %d, armed" % (case.name, t, lay, ra))
                prev = (data, got)
    finally:
        grp.close()


def run_mixed(check_guards=False):
    """five_64x48 under its schedule (streams sit out), two streams native and three at other sizes: one read_all call and one armed
    step per call, one launch each; the native streams' bytes are those of a group that never had a size"""
    name, tg = ds.MIXED
    src = do.BY_NAME[name]
    S = len(src.streams)
    sched = do.SCHEDULES[name]
    lay_of = lambda t: COMBOS[(5 * t) % len(COMBOS)]
    grp, plain = h264dec.DecoderGroup(S), h264dec.DecoderGroup(S)
    compared = set()
    try:
        for k in range(S):
            if tg[k] is not None:
                grp.set_output_size(k, *tg[k])
        nxt, t = [0] * S, 0
        while min(nxt) < ds.STEPS + 2 and t < 40:
            part = [k for k in range(S) if nxt[k] < src.pictures and sched(t, k)]
            lay, ra = lay_of(t)
            grp.set_output(lay, ra)
            plain.set_output(lay, ra)
            aus = [au_of(src, k, nxt[k]) if k in part else None for k in range(S)]
            assert grp.decode(aus) == plain.decode(aus) == [(0, 1) if k in part else (0, 0) for k in range(S)]
            for k in part:
                nxt[k] += 1
            last = [n - 1 if n else None for n in nxt]
            step = grp.last_step()
            if part:
                assert (step["output_launches"], step["output_transfers"]) == (1, 1), step
                data, got = output_copy(grp)
                pdata, pgot = output_copy(plain)
                want, written, desc, total = do.pack(ds.expected_pics(name, tg, last, only=part), lay, ra)
                assert data.size == total and all(same_desc(got[k], desc[k]) for k in range(S)), (t, got, desc)
                same_bytes(data, want, written, "mixed step %d layout %d align %d, armed" % (t, lay, ra))
                for k in part:
                    if tg[k] is None:
                        n = h264dec._pic_bytes(got[k], lay)
                        one = do.pack([(do.pictures(src, k)[last[k]][2], do.pictures(src, k)[last[k]][3])], lay, ra)[1]
                        a, b = data[got[k]["offset"]:got[k]["offset"] + n], pdata[pgot[k]["offset"]:pgot[k]["offset"] + n]
                        assert np.array_equal(a[one], b[one]), "step %d: native stream %d differs from the unscaled group's" % (t, k)
                        compared.add(k)
            else:
                assert (step["output_launches"], step["output_transfers"]) == (0, 0)
            if any(n is not None for n in last):
                want, written, desc, total = do.pack(ds.expected_pics(name, tg, last), lay, ra)
                buf, got = grp.read_all(lay, ra)
                step = grp.last_step()
                assert (step["read_launches"], step["read_transfers"]) == (1, 1), step
                assert buf.size == total and all(same_desc(got[k], desc[k]) for k in range(S))
                same_bytes(buf, want, written, "mixed step %d layout %d align %d, read_all" % (t, lay, ra))
            t += 1
        assert min(nxt) >= ds.STEPS and compared == {k for k in range(S) if tg[k] is None}
        if check_guards:
            assert grp.mem_check()[0] == 0
    finally:
        grp.close()
        plain.close()


def test_mixed_group_in_one_launch():
    run_mixed()


def test_mixed_group_under_guard_mode():
    """guard mode with poison on: every guard of the group's blocks and the ring's slack is untouched after the mixed run"""
    with mg.guarded() as seen:
        run_mixed(check_guards=True)
    mg.clean(seen, checks=2, kinds=["group"])


def test_the_ladder_three_sizes_from_one_picture():
    src = do.BY_NAME["twelve_96x80"]
    dec = h264dec.Decoder()
    try:
        for t in range(2):
            assert dec.decode(au_of(src, 0, t))
            n = dec.timing()[0]
            for W, H in ((64, 60), (48, 40), (24, 20), (96, 80), (48, 40)):
                dec.set_output_size(W, H)
                got, p = dec.read(do.NV12, 16)
                want, written, desc, _ = do.pack([(ds.scaled(src.name, 0, t, W, H), (W, H))], do.NV12, 16)
                assert same_desc(p, desc[0])
                same_bytes(got, want, written, "ladder picture %d at %dx%d" % (t, W, H))
            assert dec.timing()[0] == n, "nothing was decoded again"
    finally:
        dec.close()


def test_changing_the_size_between_armed_steps_and_back_to_native():
    """the size set holds from the next armed step on; (0, 0) gives the bytes of a group that never had a size"""
    src = do.BY_NAME["five_64x48"]
    S = len(src.streams)
    sizes = [(32, 24), (48, 36), (0, 0), (16, 12), (0, 0)]
    grp, plain = h264dec.DecoderGroup(S), h264dec.DecoderGroup(S)
    try:
        grp.set_output(do.RGBA, 16)
        plain.set_output(do.RGBA, 16)
        for t, size in enumerate(sizes):
            grp.set_output_size(-1, *size)
            assert all(grp.output_size(k) == size for k in range(S))
            aus = [au_of(src, k, t) for k in range(S)]
            assert grp.decode(aus) == plain.decode(aus) == [(0, 1)] * S
            data, got = output_copy(grp)
            tg = [None if size == (0, 0) else size] * S
            want, written, desc, total = do.pack(ds.expected_pics(src.name, tg, [t] * S), do.RGBA, 16)
            assert data.size == total and all(same_desc(got[k], desc[k]) for k in range(S))
            same_bytes(data, want, written, "armed step %d at %r" % (t, size))
            if size == (0, 0):
                pdata, pgot = output_copy(plain)
                assert [{k: v for k, v in p.items()} for p in got] == pgot and np.array_equal(data[written], pdata[written])
                buf, _ = grp.read_all(do.I420, 1)
                pbuf, _ = plain.read_all(do.I420, 1)
                assert np.array_equal(buf, pbuf)
    finally:
        grp.close()
        plain.close()


def test_a_described_stream_beside_an_undescribed_one_in_one_rgba_launch():
    """50x34 inside 64x48 at (2, 2), BT.709 full range beside no description, both resampled to 26x18: each gets its own variant"""
    w, h, coded, W, H = 50, 34, (64, 48, 2, 2), 26, 18
    planes = vc.edge_yuv(w, h)[:2]
    variants = [(col.BT709, 1), col.DEFAULT]
    grp = h264dec.DecoderGroup(2)
    try:
        grp.set_output(h264dec.PIX_RGBA, 1)
        grp.set_output_size(-1, W, H)
        aus = [unit(planes[0], col.described_vui(*variants[0]), coded, seed=0), unit(planes[1], None, coded, seed=1)]
        assert grp.decode(aus) == [(0, 1)] * 2
        step = grp.last_step()
        assert (step["output_launches"], step["output_transfers"]) == (1, 1), step
        data, armed = output_copy(grp)
        got, pics = grp.read_all(h264dec.PIX_RGBA, 1)
        assert grp.last_step()["read_launches"] == 1
        for k in range(2):
            y, u, v = (scale.scale_plane(p, W // (2 if i else 1), H // (2 if i else 1)) for i, p in enumerate(planes[k]))
            want = col.rgba_picture(y, u, v, variants[k])
            assert pics[k]["colour"] == armed[k]["colour"] == col.colour_word(variants[k])
            assert (pics[k]["width"], pics[k]["height"], pics[k]["stride"]) == (W, H, 4 * W)
            for what, buf, p in (("read_all", got, pics[k]), ("armed", data, armed[k])):
                one = np.asarray(buf[p["offset"]:p["offset"] + 4 * W * H]).reshape(H, W, 4)
                why = vc.explain_rgba(one, want, y, u, v)
                assert not why, "stream %d, %s: %s" % (k, what, why)
    finally:
        grp.close()


def test_refusals_at_delivery():
    """a target larger than the picture and one below a quarter of it: dec_read returns E_ARG and the message names both sizes; in a
    group the stream has offset -1, its message names the sizes, and the others are delivered"""
    L = h264dec._bind()
    src = do.BY_NAME["five_64x48"]
    S = len(src.streams)
    dec, grp = h264dec.Decoder(), h264dec.DecoderGroup(S)
    try:
        assert dec.decode(au_of(src, 0, 0))
        pic = h264dec.OutPic()
        buf = np.zeros(1 << 16, np.uint8)
        for W, H in ((66, 48), (64, 50), (14, 48), (64, 10), (128, 96)):
            dec.set_output_size(W, H)
            for dst, cap in ((None, 0), (buf.ctypes.data, buf.nbytes)):
                assert L.mi355x_h264_dec_read(dec.h, 0, 1, dst, cap, 0, C.byref(pic)) == E_ARG, (W, H)
                msg = L.mi355x_h264_dec_last_error(dec.h).decode()
                assert "%dx%d" % (W, H) in msg and "64x48" in msg, msg
            with pytest.raises(EncoderError) as ei:
                dec.read(0, 1)
            assert ei.value.rc == E_ARG
        dec.set_output_size(16, 12)     # exactly a quarter is served
        assert dec.read(0, 1)[1]["width"] == 16
        # the group: stream 1 asks for more than its picture, stream 3 for less than a quarter
        grp.set_output_size(1, 64, 48)  # its picture is 62x46
        grp.set_output_size(3, 14, 12)
        grp.set_output_size(4, 32, 24)
        grp.set_output(do.I420, 1)
        assert grp.decode([au_of(src, k, 0) for k in range(S)]) == [(0, 1)] * S
        tg = [None, None, None, None, (32, 24)]
        want, written, desc, total = do.pack([p if k not in (1, 3) else None for k, p in enumerate(ds.expected_pics(src.name, tg, [0] * S))], do.I420, 1)
        data, got = output_copy(grp)
        buf2, got2 = grp.read_all(do.I420, 1)
        for what, b, g in (("armed", data, got), ("read_all", buf2, got2)):
            assert [p["offset"] >= 0 for p in g] == [True, False, True, False, True], (what, g)
            assert all(same_desc(g[k], desc[k]) for k in range(S)), what
            same_bytes(b, want, written, "refusals, " + what)
        assert "64x48" in grp.error(1) and "62x46" in grp.error(1), grp.error(1)
        assert "14x12" in grp.error(3) and "64x48" in grp.error(3), grp.error(3)
        assert grp.last_step()["read_launches"] == 1
        # no stream deliverable: as for "no stream has a picture"
        grp.set_output_size(-1, 128, 96)
        pics = (h264dec.OutPic * S)()
        assert L.mi355x_h264_dec_group_read_all(grp.h, 0, 1, None, 0, 0, pics) == E_ARG
        grp.set_output_size(-1, 0, 0)
        assert grp.read_all(do.I420, 1)[0].size == do.pack(ds.expected_pics(src.name, [None] * S, [0] * S), do.I420, 1)[3]
    finally:
        dec.close()
        grp.close()


def test_set_time_refusals_and_read_back():
    """with live handles: every refused pair leaves the setting as it was; no such stream"""
    L = h264dec._bind()
    dec, grp = h264dec.Decoder(), h264dec.DecoderGroup(3)
    try:
        assert dec.output_size() == (0, 0) and grp.output_size(2) == (0, 0)
        for w, h in TAKEN:
            dec.set_output_size(w, h)
            grp.set_output_size(1, w, h)
            assert dec.output_size() == (w, h) and grp.output_size(1) == (w, h) and grp.output_size(0) == (0, 0)
        dec.set_output_size(480, 270)
        grp.set_output_size(-1, 480, 270)
        for w, h in REFUSED:
            assert L.mi355x_h264_dec_set_output_size(dec.h, w, h) == E_ARG, (w, h)
            assert L.mi355x_h264_dec_group_set_output_size(grp.h, 0, w, h) == E_ARG and L.mi355x_h264_dec_group_set_output_size(grp.h, -1, w, h) == E_ARG, (w, h)
        for stream in (3, -2, 64):
            assert L.mi355x_h264_dec_group_set_output_size(grp.h, stream, 16, 16) == E_ARG
            a = C.c_int(0)
            assert L.mi355x_h264_dec_group_output_size(grp.h, stream, C.byref(a), C.byref(a)) == E_ARG
        assert L.mi355x_h264_dec_group_output_size(grp.h, -1, C.byref(a), C.byref(a)) == E_ARG
        assert L.mi355x_h264_dec_output_size(dec.h, None, C.byref(a)) == E_ARG and L.mi355x_h264_dec_output_size(dec.h, C.byref(a), None) == E_ARG
        assert dec.output_size() == (480, 270) and [grp.output_size(k) for k in range(3)] == [(480, 270)] * 3
        with pytest.raises(EncoderError) as ei:
            dec.set_output_size(15, 16)
        assert ei.value.rc == E_ARG
    finally:
        dec.close()
        grp.close()


def test_the_two_resamplers_agree():
    """the decoder's native I420 in device memory through a scaled encoder stream (k_scale_to_i420_step) gives the staging picture
    that the decoder's own read at that size gives (k_dec_out_scaled)"""
    import torch
    src = do.BY_NAME["twelve_96x80"]
    W, H = 64, 48
    dec = h264dec.Decoder()
    st = capi.Stream(W, H, qp=30, gop=30, src_size=(96, 80))
    try:
        for t in range(2):
            assert dec.decode(au_of(src, 0, t)) and dec.info()[:2] == (96, 80)
            native = torch.zeros(96 * 80 * 3 // 2, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            assert dec.i420_device(native.data_ptr(), native.numel()) == native.numel()
            st.encode_device(native.data_ptr())
            dec.set_output_size(W, H)
            got, _ = dec.read(do.I420, 1)
            dec.set_output_size(0, 0)
            assert np.array_equal(st.debug_read(capi.DBG_SRC), got), "picture %d" % t
            assert np.array_equal(got, ds.scaled(src.name, 0, t, W, H))
    finally:
        st.close()
        dec.close()


@pytest.mark.parametrize("W,H", [(1280, 720), (480, 270)])
def test_a_1080p_picture_as_i420(W, H):
    """1920x1080 (coded 1920x1088): many tiles per row and per column, 3 : 2 and exactly 4 : 1"""
    w, h = 1920, 1080
    enc, dec, orc = capi.Encoder(w, h, qp=30, gop=30), h264dec.Decoder(), OracleDecoder()
    try:
        au, _ = enc.encode(synth.sequence("s1", w, h, 1)[0])
        orc.decode(au)
        assert dec.decode(au)
        i420 = vc.i420_of(*(np.ascontiguousarray(orc.cropped(p)) for p in range(3)))
        assert orc.size == (w, h) and np.array_equal(dec.i420(), i420)
        dec.set_output_size(W, H)
        for ra in (1, 256):
            got, p = dec.read(do.I420, ra)
            want, written, desc, total = do.pack([(scale.scale_i420(i420, w, h, W, H), (W, H))], do.I420, ra)
            assert got.size == total and same_desc(p, desc[0])
            same_bytes(got, want, written, "1080p to %dx%d align %d" % (W, H, ra))
    finally:
        enc.close()
        dec.close()
        orc.close()


def test_the_plugin_with_both_keys():
    """persist.vmi.video.decode.outwidth / .outheight: frames of 32x24 from a 64x48 stream, INDEX_PIC_INFO and the size-change event
    report the delivered size; a picture that cannot be resampled comes at its own size; junk keys change nothing"""
    src = do.BY_NAME["five_64x48"]
    small = do.BY_NAME["out_18x18"]
    W, H = 32, 24
    try:
        vd.set_output_size(W, H)
        d = vd.PluginDecoder()
        try:
            assert d.rc_create == vd.SUCCESS and d.create_decoder() == vd.SUCCESS and d.init() == vd.SUCCESS and d.install_hooks() == vd.SUCCESS
            assert d.set_pic_info(64, 48) == vd.SUCCESS and d.start() == vd.SUCCESS
            assert d.pic_info()[:2] == (64, 48)
            for t in range(ds.STEPS):
                assert d.send(au_of(src, 0, t)) == vd.SUCCESS
                if t == 0:   # the configured size is not the delivered one: the event names it, the owner follows
                    assert d.retrieve(1 << 16)[0] == vd.BAD_PIC_SIZE
                    assert (d.events.count, d.events.width, d.events.height) == (1, W, H)
                    assert d.set_pic_info(W, H) == vd.SUCCESS
                rc, got = d.retrieve(1 << 16)
                assert rc == vd.SUCCESS and got.size == W * H * 3 // 2
                assert np.array_equal(got, ds.scaled(src.name, 0, t, W, H)), "plugin picture %d" % t
                assert d.pic_info()[:2] == (W, H)
            # 18x18 cannot be resampled to 32x24: delivered as it is
            assert d.send(au_of(small, 1, 0)) == vd.SUCCESS
            assert d.retrieve(1 << 16)[0] == vd.BAD_PIC_SIZE and (d.events.width, d.events.height) == (18, 18)
            assert d.set_pic_info(18, 18) == vd.SUCCESS
            rc, got = d.retrieve(1 << 16)
            assert rc == vd.SUCCESS and np.array_equal(got, do.pictures(small, 1)[0][2])
            assert d.stop() == vd.SUCCESS
        finally:
            d.delete()
        for keys in ((W, None), ("junk", H), (None, None)):
            vd.set_output_size(*keys)
            d = vd.PluginDecoder()
            try:
                assert d.create_decoder() == vd.SUCCESS and d.init() == vd.SUCCESS and d.install_hooks() == vd.SUCCESS
                assert d.set_pic_info(64, 48) == vd.SUCCESS and d.start() == vd.SUCCESS
                assert d.send(au_of(src, 0, 0)) == vd.SUCCESS
                rc, got = d.retrieve(1 << 16)
                assert rc == vd.SUCCESS and np.array_equal(got, do.pictures(src, 0)[0][2]) and d.events.count == 0, keys
                assert d.pic_info()[:2] == (64, 48)
            finally:
                d.delete()
    finally:
        vd.set_output_size(None, None)
