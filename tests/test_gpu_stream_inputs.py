"""Streams take what the engine takes (include/mi355x_h264.h "streams": layouts and device-resident pictures): I420, NV12 or
RGBA pictures, from host or from device memory, and a picture that lies in device memory is read where it lies.  Whatever the
door, a stream's access units, motion cost and reconstruction are the CPU oracle's for the I420 picture (NV12: de-interleaved
here; RGBA: the oracle's own conversion, oracle/h264_rgba.c) - equality of bytes everywhere."""
import threading
import numpy as np
import pytest
import adversarial
from media_amd import capi, synth
from media_amd import videocodec as vc
from oracle_lib import OracleEncoder, rgba_to_i420
from spec_pred import MB_IPCM

pytestmark = pytest.mark.gpu

I420, NV12, RGBA = capi.INPUT_I420, capi.INPUT_NV12, capi.INPUT_RGBA
# the header's contract of the device form: an RGBA picture starts on 8 bytes, I420 / NV12 pictures on any byte
MIN_ALIGN = {I420: 1, NV12: 1, RGBA: 8}
GUARD = 64


def to_nv12(f, w, h):
    y, u, v = f[: w * h], f[w * h: w * h * 5 // 4], f[w * h * 5 // 4:]
    return np.concatenate([y, np.stack([u, v], axis=1).reshape(-1)])


def to_rgba(f, w, h, seed):
    """an RGBA picture made from an I420 one (any will do: the oracle converts it back its own way); alpha is noise"""
    y = f[: w * h].reshape(h, w).astype(np.int32)
    u = f[w * h: w * h * 5 // 4].reshape(h // 2, w // 2).repeat(2, 0).repeat(2, 1).astype(np.int32)
    v = f[w * h * 5 // 4:].reshape(h // 2, w // 2).repeat(2, 0).repeat(2, 1).astype(np.int32)
    r = np.clip(y + ((359 * (v - 128)) >> 8), 0, 255)
    g = np.clip(y - ((88 * (u - 128) + 183 * (v - 128)) >> 8), 0, 255)
    b = np.clip(y + ((454 * (u - 128)) >> 8), 0, 255)
    a = np.random.RandomState(seed).randint(0, 256, (h, w))
    return np.stack([r, g, b, a], axis=2).astype(np.uint8)


def pictures(fmt, frames, w, h):
    """(what the stream is handed as flat uint8 arrays, the I420 pictures the oracle codes)"""
    if fmt == I420:
        return [np.ascontiguousarray(f) for f in frames], frames
    if fmt == NV12:
        return [to_nv12(f, w, h) for f in frames], frames
    rgba = [to_rgba(f, w, h, i) for i, f in enumerate(frames)]
    return [p.reshape(-1) for p in rgba], [rgba_to_i420(p, w, h) for p in rgba]


class DevicePictures:
    """the pictures in ONE device allocation, every picture at the smallest alignment the header allows (an address that is a
    multiple of `align` and of nothing larger), with guard bytes around each; untouched() compares the allocation with what was
    put there"""

    def __init__(self, fmt, pics):
        import torch
        align = MIN_ALIGN[fmt]
        n = pics[0].size
        slot = (n + 2 * GUARD + 255) & ~255
        host = np.random.RandomState(7).randint(0, 256, slot * len(pics) + 256).astype(np.uint8)
        self.dev = torch.empty(host.size, dtype=torch.uint8, device="cuda")
        base = self.dev.data_ptr()
        self.addr = []
        for i, p in enumerate(pics):
            a = base + i * slot + GUARD
            a += (align - a % (2 * align)) % (2 * align)      # a % (2 * align) == align
            assert a % align == 0 and a % (2 * align) != 0
            host[a - base: a - base + n] = p
            self.addr.append(a)
        self.host = host
        self.dev.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return np.array_equal(self.dev.cpu().numpy(), self.host)


def host_encode(s, fmt, pic, w, h):
    if fmt == I420:
        return s.encode(pic)
    if fmt == NV12:
        return s.encode_nv12(pic)
    return s.encode_rgba(pic.reshape(h, w, 4))


@pytest.mark.parametrize("mem", ["host", "device", "alternating"])
@pytest.mark.parametrize("fmt", [I420, NV12, RGBA])
def test_one_stream_per_layout_and_memory_equals_the_oracle(fmt, mem):
    w, h = 320, 240
    pics, i420 = pictures(fmt, synth.sequence("s1", w, h, 13), w, h)
    dev = DevicePictures(fmt, pics)
    s = capi.Stream(w, h, qp=26, gop=5, input_format=fmt)
    orc = OracleEncoder(w, h, qp=26, gop=5)
    for i in range(13):
        if i in (3, 8):
            s.set_qp(20 + i)
            orc.set_qp(20 + i)
        if i == 7:
            s.force_idr()
        from_device = mem == "device" or (mem == "alternating" and i % 2 == 1)
        bs, ft = s.encode_device(dev.addr[i]) if from_device else host_encode(s, fmt, pics[i], w, h)
        obs, idr = orc.encode(i420[i], force_idr=(i == 7))
        assert bs == obs, "picture %d" % i
        assert (ft == capi.FRAME_IDR) == bool(idr)
        assert s.me_cost() == orc.me_cost()
        for p in range(3):
            assert np.array_equal(s.recon(p), orc.recon(p)), "picture %d plane %d" % (i, p)
    assert s.hub_stats()["pictures"] == 13
    s.close()
    assert dev.untouched(), "the device pictures are only read"


@pytest.mark.parametrize("fmt,w,h,prof,slices,nstreams,npic", [
    (I420, 320, 240, 66, 0, 6, 12), (NV12, 176, 144, 100, 3, 5, 9), (RGBA, 176, 144, 77, 0, 6, 8),
    (NV12, 176, 144, 66, 0, 12, 8), (RGBA, 176, 144, 66, 0, 12, 6), (I420, 176, 144, 100, 0, 12, 6),   # 12 streams: steps of 8 pictures or more
    (I420, 200, 120, 77, 0, 5, 7), (RGBA, 200, 120, 100, 2, 4, 6),                                       # not a multiple of 16
    (I420, 178, 144, 66, 0, 5, 7), (NV12, 178, 144, 100, 0, 5, 7), (RGBA, 178, 144, 77, 0, 5, 6),        # width % 4 == 2
    (NV12, 1920, 1080, 100, 0, 3, 3)])
def test_host_and_device_fed_streams_of_one_engine_each_equal_their_oracle(fmt, w, h, prof, slices, nstreams, npic):
    """one engine, host-fed and device-fed streams mixed (odd streams from device memory); every stream has its own content, its own
    GOP length (IDR pictures fall on different ticks) and its own QP walk"""
    kinds = ["s1", "scroll", "split", "cut", "s3", "ramp"]
    streams, want, got, pics, devs = [], [], [[] for _ in range(nstreams)], [], []
    for k in range(nstreams):
        gop = 3 + (k % 4)
        qp0 = 22 + 3 * (k % 5)
        pk, i420 = pictures(fmt, synth.sequence(kinds[k % len(kinds)], w, h, npic, start=17 * k), w, h)
        pics.append(pk)
        devs.append(DevicePictures(fmt, pk) if k % 2 else None)
        streams.append(capi.Stream(w, h, qp=qp0, gop=gop, profile_idc=prof, slices=slices, input_format=fmt))
        orc = OracleEncoder(w, h, qp=qp0, gop=gop, profile_idc=prof, slices=slices)
        exp = []
        for i, f in enumerate(i420):
            orc.set_qp(min(51, qp0 + (i * (k + 1)) % 7))
            exp.append(orc.encode(f)[0])
        want.append(exp)
        orc.close()
    go = threading.Barrier(nstreams)

    def work(k):
        qp0 = 22 + 3 * (k % 5)
        go.wait()
        for i in range(npic):
            streams[k].set_qp(min(51, qp0 + (i * (k + 1)) % 7))
            got[k].append(streams[k].encode_device(devs[k].addr[i])[0] if devs[k] else host_encode(streams[k], fmt, pics[k][i], w, h)[0])

    ths = [threading.Thread(target=work, args=(k,)) for k in range(nstreams)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    for k in range(nstreams):
        assert len(got[k]) == npic, "stream %d stopped early" % k
        for i in range(npic):
            assert got[k][i] == want[k][i], "stream %d picture %d" % (k, i)
    st = streams[0].hub_stats()
    assert st["open_streams"] == nstreams
    assert st["pictures"] == nstreams * npic
    assert st["steps"] < st["pictures"], "at least one step carried pictures of two streams"
    if nstreams >= 12:
        assert st["max_batch"] >= 2
    for s in streams:
        s.close()
    for d in devs:
        assert d is None or d.untouched()


@pytest.mark.parametrize("prof", [66, 100])
def test_ipcm_samples_come_from_the_device_picture(prof):
    """I_PCM macroblocks carry SOURCE samples, read by the entropy coder: from the caller's picture when that is where they lie"""
    w, h = 176, 144
    frames = adversarial.sequence("contrast", w, h, 6)
    pics, i420 = pictures(NV12, frames, w, h)
    dev = DevicePictures(NV12, pics)
    s = capi.Stream(w, h, qp=10, gop=30, profile_idc=prof, input_format=NV12)
    orc = OracleEncoder(w, h, qp=10, gop=30, profile_idc=prof)
    for i in range(6):
        obs = orc.encode(i420[i])[0]
        npcm = int((orc.mbinfo()["type"] == MB_IPCM).sum())
        assert npcm >= 40, "picture %d: %d I_PCM macroblocks in the oracle's picture - the test would show nothing" % (i, npcm)
        assert s.encode_device(dev.addr[i])[0] == obs, "picture %d" % i
        for p in range(3):
            assert np.array_equal(s.recon(p), orc.recon(p)), "picture %d plane %d" % (i, p)
    s.close()
    assert dev.untouched()


def test_layouts_do_not_mix_and_a_mismatched_call_is_refused():
    w, h = 176, 144
    frames = synth.sequence("s1", w, h, 3)
    a = capi.Stream(w, h, qp=30, gop=30, input_format=I420)
    b = capi.Stream(w, h, qp=30, gop=30, input_format=NV12)       # same size, another layout: another engine
    oa, ob = OracleEncoder(w, h, qp=30, gop=30), OracleEncoder(w, h, qp=30, gop=30)
    assert a.hub_stats()["open_streams"] == 1 and b.hub_stats()["open_streams"] == 1
    assert a.encode(frames[0])[0] == oa.encode(frames[0])[0]
    assert b.encode_nv12(to_nv12(frames[0], w, h))[0] == ob.encode(frames[0])[0]
    L = capi.lib()
    for s, call in ((b, lambda: b.encode(frames[1])), (a, lambda: a.encode_nv12(to_nv12(frames[1], w, h))),
                    (a, lambda: a.encode_rgba(np.zeros((h, w, 4), np.uint8)))):
        with pytest.raises(capi.EncoderError, match="rc=-1"):       # MI355X_H264_E_ARG, refused on the host
            call()
        assert L.mi355x_h264_stream_last_error(s.h) != b""
    c = capi.Stream(w, h, qp=30, gop=30, input_format=RGBA)
    import torch
    odd = torch.zeros(w * h * 4 + 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(capi.EncoderError, match="rc=-1"):           # an RGBA picture that does not start on 8 bytes
        c.encode_device(odd.data_ptr() + 4)
    c.close()
    for i in (1, 2):                                                 # the refused calls left the streams as they were
        assert a.encode(frames[i])[0] == oa.encode(frames[i])[0]
        assert b.encode_nv12(to_nv12(frames[i], w, h))[0] == ob.encode(frames[i])[0]
    a.close()
    b.close()


def _plugin(w, h, shared, **kw):
    vc.set_video_mode(w, h, **kw)
    vc.prop_set("persist.vmi.video.encode.shared", "1" if shared else "0")
    e = vc.VideoEncoder()
    assert e.rc_create == vc.SUCCESS
    assert e.init() == vc.SUCCESS and e.start() == vc.SUCCESS
    return e


@pytest.mark.parametrize("mode", ["rgba_device", "nv12_host"])
def test_plugin_input_properties_shared_engine_and_own_engine(mode):
    """persist.vmi.video.encode.input / .inputmem through libVideoCodec.so; the content and the replay rule of
    test_gpu_plugin.py::test_scene_change_recodes_as_idr, so that the scene-change re-code reads the same picture twice"""
    w, h = 352, 288
    nmb = (w // 16) * (h // 16)
    frames = synth.sequence("s1", w, h, 3) + synth.sequence("s3", w, h, 1) + synth.sequence("s1", w, h, 2, start=500)
    fmt = RGBA if mode == "rgba_device" else NV12
    pics, i420 = pictures(fmt, frames, w, h)
    dev = DevicePictures(fmt, pics) if mode == "rgba_device" else None
    size = pics[0].size
    assert size == (w * h * 4 if fmt == RGBA else w * h * 3 // 2)
    orc = OracleEncoder(w, h, qp=28, gop=300)
    want = []
    for f in i420:
        obs, idr = orc.encode(f)
        if not idr and orc.me_cost() > 3000 * nmb:
            obs, idr = orc.encode(f, force_idr=True)
        want.append(obs)
    try:
        for shared in (True, False):
            e = _plugin(w, h, shared, qp=28, gop=300, input="rgba" if fmt == RGBA else "nv12", inputmem="device" if dev else None)
            kinds = []
            for i in range(len(frames)):
                rc, bs = e.encode_addr(dev.addr[i], size) if dev else e.encode(pics[i])
                assert rc == vc.SUCCESS
                assert bs == want[i], "shared %d picture %d" % (shared, i)
                kinds.append(bs[4] & 31)
            assert kinds == [7, 1, 1, 7, 7, 1] and e.scene_cuts() == 2
            # the size guard uses the layout's picture size
            rc, _ = e.encode_addr(dev.addr[0], size - 1) if dev else e.encode(pics[0], size=size - 1)
            assert rc == vc.ENCODE_FAIL
            e.destroy()
            assert e.delete() == vc.SUCCESS
    finally:
        vc.set_video_mode(w, h)
        vc.prop_set("persist.vmi.video.encode.shared", "")
    assert dev is None or dev.untouched()


def test_host_pictures_with_padded_rows_equal_the_oracle_on_the_tight_picture():
    """the row-copy branches of the stream hub's host forms: every plane its own stride, random bytes in the padding"""
    w, h = 178, 98
    for nv12 in (False, True):
        st = capi.Stream(w, h, qp=27, gop=4, input_format=capi.INPUT_NV12 if nv12 else capi.INPUT_I420)
        orc = OracleEncoder(w, h, qp=27, gop=4)
        try:
            for i, f in enumerate(synth.sequence("s1", w, h, 5)):
                rng = np.random.default_rng(100 + i)
                y, u, v = f[: w * h].reshape(h, w), f[w * h: w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)
                strides = (w + 9, w + 14) if nv12 else (w + 9, w // 2 + 1, w // 2 + 6)
                src = [y, np.stack([u, v], axis=2).reshape(h // 2, w)] if nv12 else [y, u, v]
                planes = []
                for t, s_ in zip(src, strides):
                    p = rng.integers(0, 256, (t.shape[0], s_), dtype=np.uint8)
                    p[:, : t.shape[1]] = t
                    planes.append(p)
                got = (st.encode_nv12 if nv12 else st.encode)(planes, strides)[0]
                assert got == orc.encode(f)[0], "picture %d (%s)" % (i, "NV12" if nv12 else "I420")
            with pytest.raises(capi.EncoderError) as ei:
                (st.encode_nv12 if nv12 else st.encode)(planes, (w - 1,) + tuple(strides[1:]))
            assert ei.value.rc == capi.E_ARG
        finally:
            st.close()
            orc.close()
