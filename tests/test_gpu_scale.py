"""Scaled streams (include/mi355x_h264.h, mi355x_h264_stream_open_scaled) - run with -m gpu on an MI355X.

The stream is handed pictures of the source size; the step's scaling launch (k_scale_to_i420_step) writes the I420 staging picture
of the coded size.  debug_read(DBG_SRC) must be the numpy restatement of tests/scale.py byte for byte, and from there on the picture
takes the path of every other stream: access units and reconstruction are the CPU oracle's for the restated picture."""
import threading
import numpy as np
import pytest
import mem_guard as mg
import quality
import ref_mix as rm
import scale
from media_amd import capi
from media_amd import videocodec as vc
from oracle_lib import OracleEncoder
from test_gpu_stream_matrix import Job, WINDOW_US, build_tick

pytestmark = pytest.mark.gpu

I420, NV12, RGBA = capi.INPUT_I420, capi.INPUT_NV12, capi.INPUT_RGBA
DOORS = {I420: ("host", "strided", "device", "device+1", "device+3"), NV12: ("host", "strided", "device", "device+1", "device+3"),
         RGBA: ("host", "strided", "device", "device+8")}
PARAMS = [(c.name, f) for c in scale.CASES for f in ("i420", "nv12", "rgba") if f != "rgba" or c.rgba]


@pytest.fixture(scope="module")
def tick(tmp_path_factory):
    return build_tick(tmp_path_factory.mktemp("stream_tick_scale"))


class Device:
    """a picture in device memory at a chosen distance from a multiple of 256, guard bytes around it"""

    def __init__(self, pic, offset):
        import torch
        host = np.empty(pic.size + 512, np.uint8)
        host[: 256 + offset] = np.random.RandomState(offset).randint(0, 256, 256 + offset)
        host[256 + offset: 256 + offset + pic.size] = pic
        host[256 + offset + pic.size:] = np.random.RandomState(offset + 1).randint(0, 256, 256 - offset)
        self.host, self.dev = host, torch.from_numpy(host).cuda()
        assert self.dev.data_ptr() % 256 == 0
        self.addr = self.dev.data_ptr() + 256 + offset
        torch.cuda.synchronize()

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return np.array_equal(self.dev.cpu().numpy(), self.host)


def _padded(plane, stride, seed):
    p = np.random.RandomState(seed).randint(0, 256, (plane.shape[0], stride)).astype(np.uint8)
    p[:, : plane.shape[1]] = plane
    return p


def hand_in(s, fmt, pic, sw, sh, door, seed=0):
    """one picture of the source size through the door named; returns (access unit, frame type, what must stay alive / untouched)"""
    if door.startswith("device"):
        d = Device(pic, int(door[7:] or 0))
        return s.encode_device(d.addr) + (d,)
    if fmt == RGBA:
        p = pic.reshape(sh, sw, 4)
        if door == "strided":
            q = _padded(p.reshape(sh, 4 * sw), 4 * sw + 24, seed)
            return s.encode_rgba(q, stride=4 * sw + 24) + (None,)
        return s.encode_rgba(p) + (None,)
    if door == "host":
        return (s.encode(pic) if fmt == I420 else s.encode_nv12(pic)) + (None,)
    if fmt == I420:
        strides = (sw + 9, sw // 2 + 1, sw // 2 + 6)
        planes = [_padded(p, st, seed + k) for k, (p, st) in enumerate(zip(scale.planes_i420(pic, sw, sh), strides))]
        return s.encode(planes, strides) + (None,)
    strides = (sw + 9, sw + 14)
    planes = [_padded(pic[: sw * sh].reshape(sh, sw), strides[0], seed), _padded(pic[sw * sh:].reshape(sh // 2, sw), strides[1], seed + 1)]
    return s.encode_nv12(planes, strides) + (None,)


def _first_difference(got, want, w, h):
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    if i < w * h:
        return "%d bytes differ; first: Y(%d, %d) = %d, expected %d" % (bad.size, i % w, i // w, got[i], want[i])
    j = i - w * h
    pl, j = ("U", j) if j < (w // 2) * (h // 2) else ("V", j - (w // 2) * (h // 2))
    return "%d bytes differ; first: %s(%d, %d) = %d, expected %d" % (bad.size, pl, j % (w // 2), j // (w // 2), got[i], want[i])


def run_case(name, fmtname, refs=0):
    """the case's pictures through doors in turn (IDR + P ..), then picture 0 again through every door not yet used: staging bytes,
    access units, frame types and the final reconstruction"""
    c, fmt = scale.BY_NAME[name], scale.FORMATS[fmtname]
    pics, want = scale.pictures(name, fmt)
    doors = DOORS[fmt]
    first = 4 if c.pictures == 1 else 1 if c.pictures == 2 else 0      # (the short cases start at the doors the others reach late)
    plan = [(i, doors[(first + i) % len(doors)]) for i in range(c.pictures)]
    plan += [(0, d) for d in doors if d not in [p[1] for p in plan]]
    s = capi.Stream(c.w, c.h, qp=30, gop=30, input_format=fmt, src_size=(c.sw, c.sh), refs=refs)
    orc = OracleEncoder(c.w, c.h, qp=30, gop=30, refs=refs)
    try:
        assert s.source_size() == (c.sw, c.sh) and (s.width, s.height) == (c.w, c.h)
        for k, (i, door) in enumerate(plan):
            tag = "%s %s entry %d (picture %d, %s)" % (name, fmtname, k, i, door)
            au, ft, dev = hand_in(s, fmt, pics[i], c.sw, c.sh, door, seed=k)
            got = s.debug_read(capi.DBG_SRC)
            assert got.size == c.w * c.h * 3 // 2
            assert np.array_equal(got, want[i]), tag + ": staging picture: " + _first_difference(got, want[i], c.w, c.h)
            assert dev is None or dev.untouched(), tag + ": the device picture is only read"
            if k < c.pictures or c.w * c.h <= 208 * 160:      # (the large cases: IDR + 1 P only on the oracle)
                oau, idr = orc.encode(want[i])
                assert au == oau, tag + ": access unit differs from the oracle's on the restated picture"
                assert (ft == capi.FRAME_IDR) == bool(idr) == (k == 0), tag
                if k == len(plan) - 1 or k == c.pictures - 1:
                    for p in range(3):
                        assert np.array_equal(s.recon(p), orc.recon(p)), tag + ": plane %d" % p
    finally:
        s.close()
        orc.close()


@pytest.mark.parametrize("name,fmtname", PARAMS)
def test_staging_bytes_and_access_units(name, fmtname):
    run_case(name, fmtname)


def _group(tick, monkeypatch, n=6, npic=3):
    """n scaled streams of one geometry, a content of its own each, handed in together picture by picture"""
    monkeypatch.setenv("MI355X_H264_HUB_WINDOW_US", WINDOW_US)
    sw, sh, w, h = 96, 64, 64, 48
    src = [[np.random.RandomState(900 + 10 * k + i).randint(0, 256, sw * sh * 3 // 2).astype(np.uint8) for i in range(npic)] for k in range(n)]
    for k in range(n):      # (noise alone would all go out as I_PCM at a low QP: every other stream pans a picture)
        if k % 2:
            base = scale.source_i420("mid_320x240")[0]
            y, u, v = scale.planes_i420(base, 320, 240)
            src[k] = [np.concatenate([y[k: k + sh, 3 * i + k: 3 * i + k + sw].ravel(), u[k: k + sh // 2, i: i + sw // 2].ravel(), v[k: k + sh // 2, i: i + sw // 2].ravel()])
                      for i in range(npic)]
    streams = [capi.Stream(w, h, qp=24 + k, gop=30, src_size=(sw, sh)) for k in range(n)]
    orcs = [OracleEncoder(w, h, qp=24 + k, gop=30) for k in range(n)]
    shared = 0
    try:
        assert streams[0].hub_stats()["open_streams"] == n
        for i in range(npic):
            jobs = (Job * n)(*[Job(streams[k].h.value, src[k][i].ctypes.data, sw, sh, 0, 0, None, 0, 0) for k in range(n)])
            tick(jobs)
            for k in range(n):
                tag = "stream %d picture %d" % (k, i)
                want = scale.scale_i420(src[k][i], sw, sh, w, h)
                assert jobs[k].rc == 0, tag + ": " + streams[k].last_error()
                assert np.array_equal(streams[k].debug_read(capi.DBG_SRC), want), tag + ": staging picture"
                import ctypes as C
                assert C.string_at(jobs[k].out, jobs[k].len) == orcs[k].encode(want)[0], tag
                shared = max(shared, streams[k].last_step()["pictures"])
        assert shared >= 2, "no step carried pictures of two streams"
        st = streams[0].hub_stats()
        assert st["pictures"] == n * npic and st["steps"] < st["pictures"]
    finally:
        for s in streams:
            s.close()
        for o in orcs:
            o.close()


def test_six_scaled_streams_share_steps(tick, monkeypatch):
    _group(tick, monkeypatch)


def test_scaled_and_unscaled_streams_beside_each_other():
    """a scaled and an unscaled stream of one coded size have engines of their own; a stream whose source IS the coded size is an
    ordinary stream and shares the unscaled one's"""
    c = scale.BY_NAME["3to2_96x64"]
    pics, want = scale.pictures(c.name, I420)
    a = capi.Stream(c.w, c.h, qp=28, gop=30, src_size=(c.sw, c.sh))
    b = capi.Stream(c.w, c.h, qp=28, gop=30)
    same = capi.Stream(c.w, c.h, qp=28, gop=30, src_size=(c.w, c.h))
    oa, ob, osame = (OracleEncoder(c.w, c.h, qp=28, gop=30) for _ in range(3))
    try:
        assert a.hub_stats()["open_streams"] == 1
        assert b.hub_stats()["open_streams"] == 2 and same.hub_stats()["open_streams"] == 2
        assert same.source_size() == (c.w, c.h) and b.source_size() == (c.w, c.h)
        for i in range(c.pictures):
            assert a.encode(pics[i])[0] == oa.encode(want[i])[0], "scaled, picture %d" % i
            assert b.encode(want[i])[0] == ob.encode(want[i])[0], "unscaled, picture %d" % i
            assert same.encode(want[c.pictures - 1 - i])[0] == osame.encode(want[c.pictures - 1 - i])[0], "source == coded, picture %d" % i
        assert a.hub_stats()["pictures"] == c.pictures and b.hub_stats()["pictures"] == 2 * c.pictures
        with pytest.raises(capi.EncoderError) as ei:      # a scaled stream takes pictures of the source size: strides against its width
            a.encode(list(scale.planes_i420(want[0], c.w, c.h)), (c.w, c.w // 2, c.w // 2))
        assert ei.value.rc == capi.E_ARG
        assert a.encode(pics[0])[0] == oa.encode(want[0])[0], "the refused call left the stream as it was"
    finally:
        for x in (a, b, same, oa, ob, osame):
            x.close()


def test_three_reference_pictures_with_scaling():
    """refs = 3 on a ref_mix case: the source is the case's picture with every sample doubled in both dimensions, whose 2 : 1
    resampling is the case's picture again - the older reference pictures win as they do without scaling"""
    c = rm.BY_NAME["split_96x80_high"]
    frames = rm.frames(c)
    s = capi.Stream(c.w, c.h, qp=c.qp, gop=c.gop, profile_idc=c.prof, slices=c.slices, refs=c.refs, src_size=(2 * c.w, 2 * c.h))
    orc = rm.oracle_for(c, 1)
    older = 0
    try:
        for i, f in enumerate(frames):
            big = np.concatenate([p.repeat(2, 0).repeat(2, 1).ravel() for p in scale.planes_i420(f, c.w, c.h)])
            assert np.array_equal(scale.scale_i420(big, 2 * c.w, 2 * c.h, c.w, c.h), f)
            au, _ = s.encode(big)
            assert np.array_equal(s.debug_read(capi.DBG_SRC), f), "picture %d: staging picture" % i
            assert au == orc.encode(f)[0], "picture %d" % i
            mb = orc.mbinfo()
            older += int(((mb["chroma_mode"] > 0) & np.isin(mb["type"], rm.INTER)).sum())      # (ref_idx_l0 lies in chroma_mode)
        for p in range(3):
            assert np.array_equal(s.recon(p), orc.recon(p))
        assert older > 0, "no macroblock took an older reference picture: the case would show nothing"
    finally:
        s.close()
        orc.close()


@pytest.mark.parametrize("fmtname", ["i420", "rgba"])
def test_quality_report_is_of_the_resampled_picture(fmtname):
    c, fmt = scale.BY_NAME["odd_70x38"], scale.FORMATS[fmtname]
    pics, want = scale.pictures(c.name, fmt)
    s = capi.Stream(c.w, c.h, qp=34, gop=30, input_format=fmt, src_size=(c.sw, c.sh))
    orc = OracleEncoder(c.w, c.h, qp=34, gop=30)
    try:
        s.quality_enable(True)
        for i in range(c.pictures):
            hand_in(s, fmt, pics[i], c.sw, c.sh, "host" if i % 2 else "device")
            orc.encode(want[i])
            exp = quality.expected(quality.i420_planes(want[i], c.w, c.h), [orc.recon(p) for p in range(3)], c.w, c.h)
            q = s.quality()
            assert q["valid"] and tuple(q["sse"]) == exp.sse and tuple(q["samples"]) == exp.samples, "picture %d" % i
            assert sum(exp.sse) > 0
            assert np.array_equal(s.quality_map(), exp.map), "picture %d: map" % i
    finally:
        s.close()
        orc.close()


@pytest.mark.parametrize("name,fmtname", [("odd_70x38", "nv12"), ("five_70x62", "i420"), ("3to2_96x64", "rgba")])
def test_guarded_cases(name, fmtname):
    with mg.guarded() as seen:
        run_case(name, fmtname)
    mg.clean(seen, kinds=["stream"])
    assert capi.mem_tally() == seen.tally_before


def test_guarded_group(tick, monkeypatch):
    with mg.guarded() as seen:
        _group(tick, monkeypatch)
    mg.clean(seen, kinds=["stream"])
    assert capi.mem_tally() == seen.tally_before


def _plugin_object(shared=True):
    e = vc.VideoEncoder()
    assert e.rc_create == vc.SUCCESS
    return e


def _plugin_replay(want, w, h, qp):
    """the plugin class's pictures on the oracle: a P picture whose motion cost exceeds the scene-change threshold goes out re-coded as IDR"""
    orc = OracleEncoder(w, h, qp=qp, gop=300)
    nmb = ((w + 15) // 16) * ((h + 15) // 16)
    out = []
    for f in want:
        au, idr = orc.encode(f)
        if not idr and orc.me_cost() > 3000 * nmb:
            au, idr = orc.encode(f, force_idr=True)
        out.append(au)
    orc.close()
    return out


def test_plugin_objects_with_the_source_size_keys():
    """persist.vmi.video.encode.srcwidth / .srcheight through libVideoCodec.so: two objects on two threads take pictures of the source
    size; a short inputSize fails; with an engine of its own (.shared = 0) init fails"""
    c = scale.BY_NAME["mid_320x240"]
    pics, want = scale.pictures(c.name, I420)
    orders = ([0, 1, 2, 3], [3, 2, 1, 0])
    exp = [_plugin_replay([want[i] for i in o], c.w, c.h, 28) for o in orders]
    size = c.sw * c.sh * 3 // 2
    got, objs = [[], []], []
    try:
        vc.set_video_mode(c.w, c.h, qp=28, gop=300, srcwidth=c.sw, srcheight=c.sh)
        vc.prop_set("persist.vmi.video.encode.shared", "1")
        for _ in orders:
            e = _plugin_object()
            assert e.init() == vc.SUCCESS and e.start() == vc.SUCCESS
            objs.append(e)
        go = threading.Barrier(2)

        def work(k):
            go.wait()
            for i in orders[k]:
                got[k].append(objs[k].encode(pics[i]))

        ths = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        for k in range(2):
            assert [rc for rc, _ in got[k]] == [vc.SUCCESS] * 4
            for i in range(4):
                assert got[k][i][1] == exp[k][i], "object %d picture %d" % (k, i)
        # the size guard counts the source picture; a picture of the coded size is too short
        assert objs[0].encode(pics[0], size=size - 1)[0] == vc.ENCODE_FAIL
        assert objs[0].encode(pics[0], size=c.w * c.h * 3 // 2)[0] == vc.ENCODE_FAIL
        for e in objs:
            e.destroy()
            assert e.delete() == vc.SUCCESS
        objs = []
        # RGBA: four bytes per source sample
        vc.set_video_mode(c.w, c.h, qp=28, gop=300, srcwidth=c.sw, srcheight=c.sh, input="rgba")
        rp, rwant = scale.pictures(c.name, RGBA)
        e = _plugin_object()
        objs.append(e)
        assert e.init() == vc.SUCCESS and e.start() == vc.SUCCESS
        rexp = _plugin_replay(rwant[:2], c.w, c.h, 28)
        for i in range(2):
            assert e.encode(rp[i]) == (vc.SUCCESS, rexp[i]), "RGBA picture %d" % i
        assert e.encode(rp[0], size=c.sw * c.sh * 4 - 1)[0] == vc.ENCODE_FAIL
        e.destroy()
        assert e.delete() == vc.SUCCESS
        objs = []
        # junk in one key: the reference's behaviour - pictures of the coded size
        vc.set_video_mode(c.w, c.h, qp=28, gop=300, srcwidth=c.sw, srcheight="junk")
        e = _plugin_object()
        objs.append(e)
        assert e.init() == vc.SUCCESS and e.start() == vc.SUCCESS
        assert e.encode(want[0]) == (vc.SUCCESS, _plugin_replay(want[:1], c.w, c.h, 28)[0])
        e.destroy()
        assert e.delete() == vc.SUCCESS
        objs = []
        # an engine of its own does not scale
        vc.set_video_mode(c.w, c.h, qp=28, gop=300, srcwidth=c.sw, srcheight=c.sh)
        vc.prop_set("persist.vmi.video.encode.shared", "0")
        e = _plugin_object()
        objs.append(e)
        assert e.init() == vc.INIT_FAIL
        assert e.delete() == vc.SUCCESS
        objs = []
    finally:
        for e in objs:
            e.destroy()
            e.delete()
        vc.set_video_mode(c.w, c.h)
        vc.prop_set("persist.vmi.video.encode.shared", "")
