"""The RGBA ingest of the three described variants on the GPU, sample for sample over the whole RGB cube: what
k_rgba_to_i420_colour<V> (capi.Encoder(colour=...)) and k_rgba_to_i420_step_colour<V> (capi.Stream(colour=...)) wrote into the
staging picture, read back with MI355X_H264_DBG_SRC, against the restatement of tests/colour.py - over the picture sets of
tests/test_gpu_rgba_cube.py, whose pictures and helpers are imported, not copied.  Every comparison is np.array_equal over the whole
picture; a failure names the first wrong sample and the (R, G, B) that went in.  BT.601 limited runs once WITH a description, against
the undescribed path's staging: the default instantiation is the arithmetic there has always been."""
import functools
import threading

import numpy as np
import pytest

import colour as col
import value_cube as vc
from media_amd import capi
from oracle_lib import rgba_to_i420 as oracle_rgba_to_i420
from test_gpu_rgba_cube import SETS, IDS, picture, padded, same
from test_gpu_stream_inputs import DevicePictures, RGBA

pytestmark = pytest.mark.gpu
N = vc.N
VIDS = [col.NAMES[v] for v in col.NEW]


@functools.lru_cache(maxsize=None)
def reference(variant, kind, k):
    """the I420 picture expected in staging: computed once, shared by the tests of both kernels, never written"""
    out = col.rgba_to_i420(picture(kind, k), variant)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("kind,ks", SETS, ids=IDS)
@pytest.mark.parametrize("variant", col.NEW, ids=VIDS)
def test_encoder_conversion_equals_the_restatement_over_the_cube(variant, kind, ks):
    """k_rgba_to_i420_colour<V>: even pictures from host memory with padded rows, odd ones from device memory"""
    ks = list(ks) if kind != "rounding" else [0, 0]
    pics = [picture(kind, k) for k in ks]
    dev = DevicePictures(RGBA, [p.reshape(-1) for p in pics[1::2]])
    enc = capi.Encoder(N, N, qp=51, gop=4, refs=1, colour=col.WORDS[variant])
    try:
        assert enc.colour == col.WORDS[variant]
        for i, (k, p) in enumerate(zip(ks, pics)):
            if i % 2 == 0:
                enc.encode_rgba(*padded(p, 8, k))
            else:
                enc.encode_rgba_device(dev.addr[i // 2])
            same(enc.debug_read(capi.DBG_SRC), reference(variant, kind, k), p, "%s %s picture %d (%s)" % (col.NAMES[variant], kind, k, "device" if i % 2 else "host"))
    finally:
        enc.close()
    assert dev.untouched(), "the device pictures are only read"


@pytest.mark.parametrize("kind,ks", SETS, ids=IDS)
@pytest.mark.parametrize("variant", col.NEW, ids=VIDS)
def test_stream_conversion_equals_the_restatement_over_the_cube(variant, kind, ks):
    """k_rgba_to_i420_step_colour<V>: the pictures shared out over four streams of one engine, on threads started behind a barrier;
    odd streams are fed from device memory; every stream reads its staging picture back after each of its pictures"""
    ks = list(ks)
    S = 4
    pics = {k: picture(kind, k) for k in ks}
    mine = [ks[j::S] for j in range(S)]
    devs = [DevicePictures(RGBA, [pics[k].reshape(-1) for k in mine[j]]) if j % 2 else None for j in range(S)]
    streams = [capi.Stream(N, N, qp=51, gop=4, refs=1, input_format=RGBA, colour=col.WORDS[variant]) for _ in range(S)]
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
            assert streams[j].colour == col.WORDS[variant]
            assert len(got[j]) == len(mine[j]), "stream %d stopped early" % j
            for k, g in zip(mine[j], got[j]):
                same(g, reference(variant, kind, k), pics[k], "%s %s picture %d (stream %d, %s)" % (col.NAMES[variant], kind, k, j, "device" if devs[j] else "host"))
        st = streams[0].hub_stats()
        assert st["open_streams"] == S and st["pictures"] == len(ks)
        assert st["steps"] < st["pictures"] and st["max_batch"] >= 2, st   # otherwise blockIdx.z > 0 was never walked
    finally:
        for s in streams:
            s.close()
    for d in devs:
        assert d is None or d.untouched()


@pytest.mark.parametrize("w,h", vc.EDGE_SIZES)
@pytest.mark.parametrize("variant", col.NEW, ids=VIDS)
def test_edge_pictures_through_the_encoder_and_three_streams(variant, w, h):
    """widths with w % 4 == 2: every extreme triple through both kernels, from tight host rows, padded host rows and device memory;
    the three streams of one engine meet at a barrier before every picture and every picture is an IDR picture (gop 1), so a step
    carries the same size through several table rows"""
    pics = vc.edge_rgba(w, h)
    want = [col.rgba_to_i420(p, variant) for p in pics]
    dev = DevicePictures(RGBA, [p.reshape(-1) for p in pics])
    pads = [padded(p, 20, i) for i, p in enumerate(pics)]
    doors = ("tight", "padded", "device")
    enc = capi.Encoder(w, h, qp=51, gop=4, refs=1, colour=col.WORDS[variant])
    try:
        for i, p in enumerate(pics):
            for door in doors:
                if door == "tight":
                    enc.encode_rgba(p)
                elif door == "padded":
                    enc.encode_rgba(*pads[i])
                else:
                    enc.encode_rgba_device(dev.addr[i])
                same(enc.debug_read(capi.DBG_SRC), want[i], p, "%s %dx%d picture %d (encoder, %s)" % (col.NAMES[variant], w, h, i, door))
    finally:
        enc.close()
    streams = [capi.Stream(w, h, qp=51, gop=1, refs=1, input_format=RGBA, colour=col.WORDS[variant]) for _ in doors]
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
                same(g, want[i], pics[i], "%s %dx%d picture %d (stream, %s)" % (col.NAMES[variant], w, h, i, door))
        assert streams[0].hub_stats()["open_streams"] == 3
    finally:
        for s in streams:
            s.close()
    assert dev.untouched()


def test_bt601_limited_with_a_description_is_the_undescribed_arithmetic():
    """the default instantiation: an explicit ("bt601", "limited") description changes the parameter sets and nothing the
    conversion writes - staging equals the undescribed path's, byte for byte, and the oracle's conversion"""
    kinds = [("luma", 0), ("luma", 15), ("chroma", 40), ("rounding", 0)]
    pics = [picture(kind, k) for kind, k in kinds] + vc.edge_rgba(50, 34)[:1]
    for p in pics:
        h, w = p.shape[:2]
        want = oracle_rgba_to_i420(p, w, h)
        assert np.array_equal(want, col.rgba_to_i420(p, col.DEFAULT))
        described, plain = capi.Encoder(w, h, qp=51, gop=4, refs=1, colour=("bt601", "limited")), capi.Encoder(w, h, qp=51, gop=4, refs=1)
        sd, sp = capi.Stream(w, h, qp=51, gop=4, input_format=RGBA, colour=("bt601", "limited")), capi.Stream(w, h, qp=51, gop=4, input_format=RGBA)
        try:
            assert described.colour == ("bt601", "limited") and plain.colour is None and sd.colour == ("bt601", "limited") and sp.colour is None
            # a described and an undescribed stream never share an engine: their parameter sets differ
            assert sd.hub_stats()["open_streams"] == 1 and sp.hub_stats()["open_streams"] == 1
            a, b = described.encode_rgba(p)[0], plain.encode_rgba(p)[0]
            c, d = sd.encode_rgba(p)[0], sp.encode_rgba(p)[0]
            for obj in (described, plain, sd, sp):
                same(obj.debug_read(capi.DBG_SRC), want, p, "%dx%d" % (w, h))
            # the access units differ in the SPS alone
            na, nb = col.split_nals(a), col.split_nals(b)
            assert na[0] != nb[0] and na[1:] == nb[1:] and col.split_nals(c)[1:] == col.split_nals(d)[1:] == nb[1:]
            assert col.read_sps(nb[0])[0]["vui"] is None and d == b
            assert col.read_sps(na[0])[0]["vui"] == col.expected_vui(col.DEFAULT, False, 30, 1)      # an encoder's layout is the call's: no chroma_loc
            assert col.read_sps(col.split_nals(c)[0])[0]["vui"] == col.expected_vui(col.DEFAULT, True, 30, 1)
        finally:
            for obj in (described, plain):
                obj.close()
            for obj in (sd, sp):
                obj.close()
