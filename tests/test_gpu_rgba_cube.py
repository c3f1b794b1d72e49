"""The RGBA ingest on the GPU, sample for sample over the whole RGB cube (tests/value_cube.py): what k_rgba_to_i420 and
k_rgba_to_i420_step (media_amd/csrc/rgba_kernels.h) wrote into the staging picture, read back with MI355X_H264_DBG_SRC, against the
oracle's conversion of the picture handed in (oracle/h264_rgba.c, which tests/test_value_cube_oracle.py proves equal to the header's
formula over the same pictures).  Integer arithmetic: every comparison is np.array_equal over the whole picture, and a failure
names the first wrong sample and the (R, G, B) that went in.  The encodes run at QP 51 with one reference picture: they only carry
the pictures in, their bytes are not the subject here."""
import functools
import threading

import numpy as np
import pytest

import value_cube as vc
from media_amd import capi
from oracle_lib import rgba_to_i420
from test_gpu_stream_inputs import DevicePictures, RGBA, I420, NV12, to_nv12

pytestmark = pytest.mark.gpu
N = vc.N

# the cubes split by picture index, never thinned: (set, pictures)
SETS = [("luma", range(0, 16))] + [("chroma", range(16 * p, 16 * p + 16)) for p in range(4)] + [("rounding", range(0, 8))]
IDS = ["%s_%d_%d" % (s, r[0], r[-1]) for s, r in SETS]


def picture(kind, k):
    if kind == "luma":
        return vc.rgb_luma_cube(k)
    if kind == "chroma":
        return vc.rgb_chroma_cube(k)
    # the rounding picture, and the same picture rolled by whole block rows (as random as the first: the streams get one each)
    return np.roll(vc.rounding_picture(), 2 * 37 * k, axis=0)


@functools.lru_cache(maxsize=None)
def reference(kind, k):
    """the I420 picture expected in staging: computed once, shared by the tests of both kernels, never written"""
    out = rgba_to_i420(picture(kind, k), N, N)
    out.setflags(write=False)
    return out


def padded(p, extra, seed):
    """the picture with rows 4 * w + extra bytes apart, random bytes in the padding: (array, stride)"""
    h, w = p.shape[:2]
    a = np.random.RandomState(seed).randint(0, 256, (h, 4 * w + extra)).astype(np.uint8)
    a[:, :4 * w] = p.reshape(h, 4 * w)
    return a, 4 * w + extra


def same(got, want, rgba, what):
    why = vc.explain_i420(got, want, rgba)
    assert not why, "%s: %s" % (what, why)


@pytest.mark.parametrize("kind,ks", SETS, ids=IDS)
def test_encoder_conversion_equals_the_oracle_over_the_cube(kind, ks):
    """k_rgba_to_i420: even pictures from host memory with padded rows, odd ones from device memory at an address that is a
    multiple of 8 and not of 16"""
    ks = list(ks) if kind != "rounding" else [0, 0]   # the one rounding picture through both doors
    pics = [picture(kind, k) for k in ks]
    dev = DevicePictures(RGBA, [p.reshape(-1) for p in pics[1::2]])
    enc = capi.Encoder(N, N, qp=51, gop=4, refs=1)
    try:
        for i, (k, p) in enumerate(zip(ks, pics)):
            if i % 2 == 0:
                a, stride = padded(p, 8, k)
                enc.encode_rgba(a, stride)
            else:
                assert dev.addr[i // 2] % 16 == 8
                enc.encode_rgba_device(dev.addr[i // 2])
            same(enc.debug_read(capi.DBG_SRC), reference(kind, k), p, "%s picture %d (%s)" % (kind, k, "device" if i % 2 else "host"))
    finally:
        enc.close()
    assert dev.untouched(), "the device pictures are only read"


@pytest.mark.parametrize("kind,ks", SETS, ids=IDS)
def test_stream_conversion_equals_the_oracle_over_the_cube(kind, ks):
    """k_rgba_to_i420_step: the pictures shared out over four streams of one engine, on threads started behind a barrier; odd
    streams are fed from device memory; every stream reads its staging picture back after each of its pictures"""
    ks = list(ks)
    S = 4
    pics = {k: picture(kind, k) for k in ks}
    want = {k: reference(kind, k) for k in ks}
    mine = [ks[j::S] for j in range(S)]
    devs = [DevicePictures(RGBA, [pics[k].reshape(-1) for k in mine[j]]) if j % 2 else None for j in range(S)]
    streams = [capi.Stream(N, N, qp=51, gop=4, refs=1, input_format=RGBA) for _ in range(S)]
    got = [[] for _ in range(S)]
    go = threading.Barrier(S)

    def work(j):
        go.wait()
        for i, k in enumerate(mine[j]):
            if devs[j]:
                streams[j].encode_device(devs[j].addr[i])
            else:
                streams[j].encode_rgba(pics[k])
            got[j].append(streams[j].debug_read(capi.DBG_SRC))

    ths = [threading.Thread(target=work, args=(j,)) for j in range(S)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    try:
        for j in range(S):
            assert len(got[j]) == len(mine[j]), "stream %d stopped early" % j
            for k, g in zip(mine[j], got[j]):
                same(g, want[k], pics[k], "%s picture %d (stream %d, %s)" % (kind, k, j, "device" if devs[j] else "host"))
        st = streams[0].hub_stats()
        assert st["open_streams"] == S and st["pictures"] == len(ks)
        # otherwise the step form of the table (blockIdx.z > 0) was never walked
        assert st["steps"] < st["pictures"] and st["max_batch"] >= 2, st
    finally:
        for s in streams:
            s.close()
    for d in devs:
        assert d is None or d.untouched()


@pytest.mark.parametrize("w,h", vc.EDGE_SIZES)
def test_edge_pictures_through_the_encoder(w, h):
    """widths with w % 4 == 2: every extreme triple through k_rgba_to_i420 from tight host rows, padded host rows and device memory"""
    pics = vc.edge_rgba(w, h)
    want = [rgba_to_i420(p, w, h) for p in pics]
    dev = DevicePictures(RGBA, [p.reshape(-1) for p in pics])
    enc = capi.Encoder(w, h, qp=51, gop=4, refs=1)
    try:
        for i, p in enumerate(pics):
            for door in ("tight", "padded", "device"):
                if door == "tight":
                    enc.encode_rgba(p)
                elif door == "padded":
                    enc.encode_rgba(*padded(p, 20, i))
                else:
                    enc.encode_rgba_device(dev.addr[i])
                same(enc.debug_read(capi.DBG_SRC), want[i], p, "%dx%d picture %d (%s)" % (w, h, i, door))
    finally:
        enc.close()
    assert dev.untouched()


@pytest.mark.parametrize("w,h", vc.EDGE_SIZES)
def test_edge_pictures_through_three_streams_of_one_engine(w, h):
    """k_rgba_to_i420_step at the same sizes: three streams of one engine take every picture each - tight host rows, padded host
    rows, device memory - so a step carries the same size through several table rows.  Pictures this small are coded faster than
    a thread comes round again, so the streams meet at a barrier before every picture and every picture is an IDR picture
    (gop 1): the engine has one context for IDR steps, and whoever arrives while it is busy shares the next step"""
    pics = vc.edge_rgba(w, h)
    want = [rgba_to_i420(p, w, h) for p in pics]
    dev = DevicePictures(RGBA, [p.reshape(-1) for p in pics])
    pads = [padded(p, 20, i) for i, p in enumerate(pics)]
    doors = ("tight", "padded", "device")
    streams = [capi.Stream(w, h, qp=51, gop=1, refs=1, input_format=RGBA) for _ in doors]
    got = [[] for _ in doors]
    go = threading.Barrier(len(doors))

    def work(j):
        for i, p in enumerate(pics):
            go.wait(timeout=60)
            if doors[j] == "tight":
                streams[j].encode_rgba(p)
            elif doors[j] == "padded":
                streams[j].encode_rgba(*pads[i])
            else:
                streams[j].encode_device(dev.addr[i])
            got[j].append(streams[j].debug_read(capi.DBG_SRC))

    ths = [threading.Thread(target=work, args=(j,)) for j in range(len(doors))]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    try:
        for j, door in enumerate(doors):
            assert len(got[j]) == len(pics), "stream %d stopped early" % j
            for i, g in enumerate(got[j]):
                same(g, want[i], pics[i], "%dx%d picture %d (%s)" % (w, h, i, door))
        st = streams[0].hub_stats()
        assert st["open_streams"] == 3 and st["pictures"] == 3 * len(pics)
        if len(pics) > 1:
            assert st["steps"] < st["pictures"] and st["max_batch"] >= 2, st
    finally:
        for s in streams:
            s.close()
    assert dev.untouched()


# ---- the hook itself ----
def padded_planes(f, w, h, nv12, seed):
    """the I420 picture f as separate planes with padded rows (random bytes in the padding): (planes, strides, the tight picture)"""
    rng = np.random.default_rng(seed)
    y, u, v = f[: w * h].reshape(h, w), f[w * h: w * h * 5 // 4].reshape(h // 2, w // 2), f[w * h * 5 // 4:].reshape(h // 2, w // 2)
    strides = (w + 9, w + 14) if nv12 else (w + 9, w // 2 + 1, w // 2 + 6)
    src = [y, np.stack([u, v], axis=2).reshape(h // 2, w)] if nv12 else [y, u, v]
    planes = []
    for t, s_ in zip(src, strides):
        p = rng.integers(0, 256, (t.shape[0], s_), dtype=np.uint8)
        p[:, : t.shape[1]] = t
        planes.append(p)
    return planes, strides, (to_nv12(f, w, h) if nv12 else f)


@pytest.mark.parametrize("nv12", [False, True], ids=["i420", "nv12"])
def test_source_hook_returns_the_tight_host_picture_and_refuses_pictures_read_in_place(nv12):
    """host pictures with padded rows arrive tight in staging (the row-copy branches, which the quantiser masks in the parity
    tests); after a device picture that was read where it lies there is nothing to read: E_ARG, a text, and the handle works on"""
    import torch
    w, h = 178, 98
    fmt = NV12 if nv12 else I420
    frames = [vc.i420_of(*vc.edge_yuv(w, h)[0]), np.random.RandomState(3).randint(0, 256, w * h * 3 // 2).astype(np.uint8)]
    tight = [to_nv12(f, w, h) if nv12 else f for f in frames]
    dev = DevicePictures(fmt, tight)
    enc = capi.Encoder(w, h, qp=51, gop=30, refs=1, input_format=fmt)
    st = capi.Stream(w, h, qp=51, gop=30, refs=1, input_format=fmt)
    try:
        for obj in (enc, st):
            with pytest.raises(capi.EncoderError) as ei:       # no picture yet
                obj.debug_read(capi.DBG_SRC)
            assert ei.value.rc == capi.E_ARG and "no picture" in obj.last_error()
            for i, f in enumerate(frames):
                planes, strides, want = padded_planes(f, w, h, nv12, 10 + i)
                (obj.encode_nv12 if nv12 else obj.encode)(planes, strides)
                assert np.array_equal(obj.debug_read(capi.DBG_SRC), want), "padded host picture %d" % i
                (obj.encode_nv12 if nv12 else obj.encode)(tight[i])
                assert np.array_equal(obj.debug_read(capi.DBG_SRC), tight[i]), "tight host picture %d" % i
            # in place: nothing in staging
            bs_dev = obj.encode_device(dev.addr[0])[0]   # (the handle's input_format names the layout)
            with pytest.raises(capi.EncoderError) as ei:
                obj.debug_read(capi.DBG_SRC)
            assert ei.value.rc == capi.E_ARG and "in place" in obj.last_error()
            recon = obj.debug_read(capi.DBG_RECON_Y)            # the other values are served as before
            assert recon.shape == (obj.ch, obj.cw) and len(bs_dev) > 0
            (obj.encode_nv12 if nv12 else obj.encode)(tight[1])  # and the handle is as usable as before
            assert np.array_equal(obj.debug_read(capi.DBG_SRC), tight[1])
    finally:
        enc.close()
        st.close()
    assert dev.untouched()
    torch.cuda.synchronize()


def test_source_hook_refuses_after_a_lockstep_batch_from_device_memory():
    """mi355x_h264_encode_gops_device reads the caller's pictures in place, as does mi355x_h264_encode_batch_device"""
    import torch
    w, h, G, T = 64, 48, 2, 2
    fb = w * h * 3 // 2
    host = np.random.RandomState(11).randint(0, 256, G * T * fb).astype(np.uint8)
    d = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    enc = capi.Encoder(w, h, qp=51, gop=30, refs=1, batch=G)
    out, sizes, gop_bytes = np.zeros(G * (1 << 16), np.uint8), np.zeros(G * T, np.uint32), np.zeros(G, np.uint64)
    try:
        enc.encode_gops_device(d.data_ptr(), fb, T * fb, T, out, 1 << 16, sizes, gop_bytes)
        assert (sizes > 0).all()
        with pytest.raises(capi.EncoderError) as ei:
            enc.debug_read(capi.DBG_SRC)
        assert ei.value.rc == capi.E_ARG and "in place" in enc.last_error()
    finally:
        enc.close()
    one = capi.Encoder(w, h, qp=51, gop=30, refs=1)
    try:
        one.encode(host[:fb])
        assert np.array_equal(one.debug_read(capi.DBG_SRC), host[:fb])
        out1, sizes1 = np.zeros(1 << 17, np.uint8), np.zeros(G * T, np.uint32)
        one.encode_batch_device(d.data_ptr(), fb, G * T, out1, sizes1)
        with pytest.raises(capi.EncoderError) as ei:
            one.debug_read(capi.DBG_SRC)
        assert ei.value.rc == capi.E_ARG
        one.encode(host[fb:2 * fb])
        assert np.array_equal(one.debug_read(capi.DBG_SRC), host[fb:2 * fb])
    finally:
        one.close()
    assert np.array_equal(d.cpu().numpy(), host)
