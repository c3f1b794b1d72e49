"""Described streams end to end on the GPU (include/mi355x_h264.h, "colour description"): for each variant and each input layout, at
the smallest sizes with cropping, an odd number of macroblock columns and w % 4 == 2 - the slice NAL units, the reconstruction and
MbInfo are the CPU oracle encoder's for the restated I420 picture (RGBA: the restated conversion of tests/colour.py), the SPS
parses with the spec-literal reader to the fields the header states, and the oracle's independent decoder (which ignores a VUI)
decodes the whole stream to the GPU's reconstruction.  Then who shares an engine with whom, one scaled RGBA stream, one run with
guards and poison, and the plugin's two keys on both of its paths."""
import threading

import numpy as np
import pytest

import colour as col
import mem_guard
import scale
from media_amd import capi, synth
from media_amd import videocodec as vc
from oracle_lib import OracleEncoder, OracleDecoder
from test_gpu_stream_inputs import DevicePictures, I420, NV12, RGBA, to_nv12, to_rgba

pytestmark = pytest.mark.gpu
FMT_NAMES = {I420: "i420", NV12: "nv12", RGBA: "rgba"}
PICTURES, GOP, QP = 5, 3, 27


def inputs(fmt, variant, w, h, kind="s1", n=PICTURES):
    """(what the stream is handed, flat uint8; the I420 pictures the oracle codes: the restated conversion for RGBA)"""
    frames = synth.sequence(kind, w, h, n)
    if fmt == I420:
        return [np.ascontiguousarray(f) for f in frames], frames
    if fmt == NV12:
        return [to_nv12(f, w, h) for f in frames], frames
    rgba = [to_rgba(f, w, h, i) for i, f in enumerate(frames)]
    return [p.reshape(-1) for p in rgba], [col.rgba_to_i420(p, variant) for p in rgba]


def encode(s, fmt, pic, w, h):
    if fmt == I420:
        return s.encode(pic)
    if fmt == NV12:
        return s.encode_nv12(pic)
    return s.encode_rgba(pic.reshape(h, w, 4))


def check_access_unit(bs, obs, idr, variant, fmt, refs, what):
    """the oracle's access unit with another SPS: every other NAL unit equal, the SPS item 4's fields"""
    got, want = col.split_nals(bs), col.split_nals(obs)
    assert [n[0] & 0x1F for n in got] == [n[0] & 0x1F for n in want], what
    for a, b in zip(got, want):
        if a[0] & 0x1F == 7:
            s, removed = col.read_sps(a)
            s0, _ = col.read_sps(b)
            assert s["vui"] == col.expected_vui(variant, fmt == RGBA, 30, refs) and removed >= 1, what
            assert s0["vui"] is None and {k: v for k, v in s.items() if k != "vui"} == {k: v for k, v in s0.items() if k != "vui"}, what
        else:
            assert a == b, "%s: NAL unit type %d" % (what, a[0] & 0x1F)
    assert (got[0][0] & 0x1F == 7) == bool(idr), what


@pytest.mark.parametrize("w,h", col.STREAM_SIZES)
@pytest.mark.parametrize("fmt", [I420, NV12, RGBA], ids=["i420", "nv12", "rgba"])
@pytest.mark.parametrize("variant", col.VARIANTS, ids=[col.NAMES[v] for v in col.VARIANTS])
def test_described_stream_equals_the_oracle_under_another_sps(variant, fmt, w, h):
    pics, i420 = inputs(fmt, variant, w, h)
    dev = DevicePictures(fmt, pics)
    profile, refs = (100, 3) if fmt == NV12 else (66, 1)
    s = capi.Stream(w, h, qp=QP, gop=GOP, profile_idc=profile, refs=refs, input_format=fmt, colour=col.WORDS[variant])
    orc = OracleEncoder(w, h, qp=QP, gop=GOP, profile_idc=profile, refs=refs)
    dec = OracleDecoder()
    try:
        assert s.colour == col.WORDS[variant]
        for i in range(PICTURES):
            what = "%s %s %dx%d picture %d" % (col.NAMES[variant], FMT_NAMES[fmt], w, h, i)
            bs, ft = s.encode_device(dev.addr[i]) if i % 2 else encode(s, fmt, pics[i], w, h)
            obs, idr = orc.encode(i420[i])
            check_access_unit(bs, obs, idr, variant, fmt, refs, what)
            assert (ft == capi.FRAME_IDR) == bool(idr), what
            if fmt == RGBA:   # for RGBA input the description selects the conversion; for the others no sample is touched
                assert np.array_equal(s.debug_read(capi.DBG_SRC), i420[i]), what + ": staging"
            mb, omb = s.debug_read(capi.DBG_MBINFO), orc.mbinfo()
            for f in ("mvx", "mvy", "type", "i16_mode", "chroma_mode", "cbp", "tc"):
                assert np.array_equal(mb[f], omb[f]), "%s: mbinfo.%s" % (what, f)
            assert dec.decode(bs) == 1, what
            for p in range(3):
                assert np.array_equal(s.recon(p), orc.recon(p)), "%s: reconstruction plane %d" % (what, p)
                assert np.array_equal(dec.plane(p), s.recon(p)), "%s: the independent decoder's plane %d" % (what, p)
            assert dec.size == (w, h)
    finally:
        s.close()
        orc.close()
        dec.close()
    assert dev.untouched()


def test_described_encoder_of_its_own_equals_the_oracle_under_another_sps():
    """the direct path (mi355x_h264_create_colour): I420 from host memory and RGBA through k_rgba_to_i420_colour"""
    w, h = 50, 34
    for variant in col.VARIANTS:
        rgba = [to_rgba(f, w, h, i) for i, f in enumerate(synth.sequence("s1", w, h, PICTURES))]
        enc = capi.Encoder(w, h, qp=QP, gop=GOP, colour=col.WORDS[variant])
        orc = OracleEncoder(w, h, qp=QP, gop=GOP)
        try:
            for i, p in enumerate(rgba):
                bs, _ = enc.encode_rgba(p)
                obs, idr = orc.encode(col.rgba_to_i420(p, variant))
                check_access_unit(bs, obs, idr, variant, I420, 1, "%s picture %d" % (col.NAMES[variant], i))   # (an encoder's VUI has no chroma_loc)
                for pl in range(3):
                    assert np.array_equal(enc.debug_read(capi.DBG_RECON_Y + pl), orc.recon(pl))
        finally:
            enc.close()
            orc.close()


def run_together(streams, feed, n):
    """every stream codes n pictures on its own thread, all meeting at a barrier before each picture; returns each stream's step
    serials"""
    go = threading.Barrier(len(streams))
    serials = [[] for _ in streams]
    errors = []

    def work(j):
        try:
            for i in range(n):
                go.wait(timeout=60)
                feed(j, i)
                serials[j].append(streams[j].last_step()["serial"])
        except Exception as e:   # noqa: BLE001 - reported below, on the main thread
            errors.append(e)
            go.abort()

    ths = [threading.Thread(target=work, args=(j,)) for j in range(len(streams))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors
    return serials


def test_who_shares_an_engine_with_whom():
    """described streams of different variants, opened together, have different engines and never the same step; three of one
    variant share steps; a described and an undescribed stream never share, even where both are BT.601 limited"""
    w, h, n = 50, 34, 6
    frames = synth.sequence("s1", w, h, n)
    same = [capi.Stream(w, h, qp=QP, gop=1, colour=("bt709", "full")) for _ in range(3)]
    b = capi.Stream(w, h, qp=QP, gop=1, colour=("bt709", "limited"))
    d = capi.Stream(w, h, qp=QP, gop=1, colour=("bt601", "limited"))
    e = capi.Stream(w, h, qp=QP, gop=1)
    streams = same + [b, d, e]
    try:
        for s in same:
            assert s.hub_stats()["open_streams"] == 3
        for s in (b, d, e):
            assert s.hub_stats()["open_streams"] == 1
        out = [[] for _ in streams]
        serials = run_together(streams, lambda j, i: out[j].append(streams[j].encode(frames[i])[0]), n)
        # every picture is an IDR picture (gop 1) and an engine has one context for IDR steps: of three streams that arrive together
        # one leads a step and the two that come while it is busy share the next.  Each engine numbers its steps on its own
        st = same[0].hub_stats()
        assert st["pictures"] == 3 * n and st["steps"] < st["pictures"] and st["max_batch"] >= 2, st
        assert any(len({serials[0][i], serials[1][i], serials[2][i]}) < 3 for i in range(n)), "streams of one description share steps"
        for s in (b, d, e):
            st = s.hub_stats()
            assert st["pictures"] == n and st["steps"] == n and st["max_batch"] == 1, st
        # the streams say what they are, and differ in nothing but the SPS
        for i in range(n):
            nals = [col.split_nals(o[i]) for o in out]
            assert nals[0] == nals[1] == nals[2] and all(x[1:] == nals[5][1:] for x in nals)
            assert len({x[0] for x in nals}) == 4
        assert [col.read_sps(col.split_nals(o[0])[0])[0]["vui"] for o in out[2:]] == [
            col.expected_vui((col.BT709, 1), False, 30, 1), col.expected_vui((col.BT709, 0), False, 30, 1),
            col.expected_vui((col.BT601, 0), False, 30, 1), None]
    finally:
        for s in streams:
            s.close()


def test_scaled_rgba_stream_resamples_then_converts_with_the_description():
    """2 : 1, BT.709 full: staging is tests/scale.py's resampling of R, G and B followed by the restated conversion"""
    sw, sh, w, h = 100, 68, 50, 34
    variant = (col.BT709, 1)
    rgba = [to_rgba(f, sw, sh, i) for i, f in enumerate(synth.sequence("s1", sw, sh, 3))]
    rgba[2] = np.random.RandomState(5).randint(0, 256, (sh, sw, 4)).astype(np.uint8)
    dev = DevicePictures(RGBA, [p.reshape(-1) for p in rgba])
    s = capi.Stream(w, h, qp=QP, gop=GOP, input_format=RGBA, src_size=(sw, sh), colour=col.WORDS[variant])
    orc = OracleEncoder(w, h, qp=QP, gop=GOP)
    try:
        assert s.source_size() == (sw, sh) and s.colour == col.WORDS[variant]
        for i, p in enumerate(rgba):
            small = np.zeros((h, w, 4), np.uint8)
            for c in range(3):
                small[..., c] = scale.scale_plane(p[..., c], w, h)
            want = col.rgba_to_i420(small, variant)
            assert not np.array_equal(want, col.rgba_to_i420(small, col.DEFAULT))
            bs, _ = s.encode_device(dev.addr[i]) if i % 2 else s.encode_rgba(p)
            assert np.array_equal(s.debug_read(capi.DBG_SRC), want), "picture %d: staging" % i
            obs, idr = orc.encode(want)
            check_access_unit(bs, obs, idr, variant, RGBA, 1, "scaled picture %d" % i)
    finally:
        s.close()
        orc.close()
    assert dev.untouched()


def test_described_rgba_streams_and_encoder_with_guards_and_poison():
    """guard mode on (tests/mem_guard.py's size) and poison on: every guard intact after described RGBA pictures through both
    kernels and a scaled described stream"""
    w, h = 50, 34
    rgba = [to_rgba(f, w, h, i) for i, f in enumerate(synth.sequence("s1", w, h, 3))]
    big = [to_rgba(f, 2 * w, 2 * h, i) for i, f in enumerate(synth.sequence("s1", 2 * w, 2 * h, 3))]
    with mem_guard.guarded() as seen:
        for variant in col.NEW:
            enc = capi.Encoder(w, h, qp=QP, gop=GOP, colour=col.WORDS[variant])
            st = capi.Stream(w, h, qp=QP, gop=GOP, input_format=RGBA, colour=col.WORDS[variant])
            sc = capi.Stream(w, h, qp=QP, gop=GOP, input_format=RGBA, src_size=(2 * w, 2 * h), colour=col.WORDS[variant])
            for p, q in zip(rgba, big):
                enc.encode_rgba(p)
                st.encode_rgba(p)
                sc.encode_rgba(q)
                want = col.rgba_to_i420(p, variant)
                assert np.array_equal(enc.debug_read(capi.DBG_SRC), want) and np.array_equal(st.debug_read(capi.DBG_SRC), want)
            for obj in (enc, st, sc):
                obj.close()
    mem_guard.clean(seen, checks=9, kinds=("encoder", "stream"))


def _plugin(w, h, shared, **kw):
    vc.set_video_mode(w, h, **kw)
    vc.prop_set("persist.vmi.video.encode.shared", "1" if shared else "0")
    e = vc.VideoEncoder()
    assert e.rc_create == vc.SUCCESS
    assert e.init() == vc.SUCCESS and e.start() == vc.SUCCESS
    return e


@pytest.mark.parametrize("shared", [True, False], ids=["stream", "own_engine"])
def test_plugin_keys_describe_the_stream_on_both_paths(shared):
    """persist.vmi.video.encode.colour / .range through libVideoCodec.so: both keys, one key (the other defaults), junk (one WARN
    line and the reference's behaviour: no description), combined with .input = rgba and - on the stream path - .srcwidth /
    .srcheight"""
    w, h = 64, 48
    frames = synth.sequence("s1", w, h, 2)
    rgba = [to_rgba(f, w, h, i) for i, f in enumerate(frames)]
    try:
        for keys, variant in (({"colour": "bt709", "range": "full"}, (col.BT709, 1)), ({"colour": "bt709"}, (col.BT709, 0)),
                              ({"range": "full"}, (col.BT601, 1)), ({"colour": "bt601", "range": "limited"}, (col.BT601, 0)),
                              ({"colour": "bt2020", "range": "full"}, None), ({}, None)):
            for rgba_input in (False, True):
                e = _plugin(w, h, shared, qp=QP, gop=30, input="rgba" if rgba_input else None, **keys)
                orc = OracleEncoder(w, h, qp=QP, gop=30)
                assert e.colour() == variant, keys
                for i in range(2):
                    rc, bs = e.encode(rgba[i].reshape(-1) if rgba_input else frames[i])
                    assert rc == vc.SUCCESS
                    obs, idr = orc.encode(col.rgba_to_i420(rgba[i], variant or col.DEFAULT) if rgba_input else frames[i])
                    if variant is None:
                        assert bs == obs, (keys, i)
                    else:
                        check_access_unit(bs, obs, idr, variant, RGBA if rgba_input and shared else I420, 1, "%s picture %d" % (keys, i))
                e.destroy()
                assert e.delete() == vc.SUCCESS
                orc.close()
        if shared:   # with a source size: the scaled, described stream
            sw, sh = 2 * w, 2 * h
            big = to_rgba(synth.sequence("s1", sw, sh, 1)[0], sw, sh, 0)
            e = _plugin(w, h, True, qp=QP, gop=30, input="rgba", srcwidth=sw, srcheight=sh, colour="bt709", range="full")
            assert e.colour() == (col.BT709, 1)
            rc, bs = e.encode(big.reshape(-1))
            assert rc == vc.SUCCESS
            small = np.zeros((h, w, 4), np.uint8)
            for c in range(3):
                small[..., c] = scale.scale_plane(big[..., c], w, h)
            orc = OracleEncoder(w, h, qp=QP, gop=30)
            obs, idr = orc.encode(col.rgba_to_i420(small, (col.BT709, 1)))
            check_access_unit(bs, obs, idr, (col.BT709, 1), RGBA, 1, "scaled plugin stream")
            e.destroy()
            assert e.delete() == vc.SUCCESS
            orc.close()
    finally:
        vc.set_video_mode(w, h)
        vc.prop_set("persist.vmi.video.encode.shared", "")
