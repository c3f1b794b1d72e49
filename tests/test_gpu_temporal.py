"""Two temporal layers on the GPU (include/mi355x_h264.h, "temporal layers") - run with -m gpu on an MI355X.

The cases and the expected streams are those of tests/temporal.py, composed from the UNCHANGED oracle (tests/test_temporal_oracle.py
proves on the oracle alone that the composition decodes and what the case list holds).  Every access unit is compared byte for
byte and every stage of every picture exactly (test_gpu_parity._compare_all: MbInfo, levels, quadrant vectors, Intra4x4 modes, the
planes before and after the loop filter) - a layer-1 picture against the fresh oracle's last picture, a layer-0 picture against
the oracle that coded the layer-0 pictures alone.  A layer-0 picture whose motion search was seeded from the layer-1 picture in
front of it, a layer-1 picture that moved the ring or frame_num, or one that went out with marking syntax fails here."""
import ctypes as C
import numpy as np
import pytest
import mem_guard as mg
import quality as ql
import ssim as ss
import temporal as tl
from media_amd import capi, h264dec
from media_amd import temporal as mt
from oracle_lib import rgba_to_i420
from test_gpu_parity import _compare_all, _to_nv12
from test_gpu_stream_matrix import Job, build_tick, steps_of, WINDOW_US

pytestmark = pytest.mark.gpu
IDS = [c.name for c in tl.CASES]


@pytest.fixture(scope="module")
def tick(tmp_path_factory):
    return build_tick(tmp_path_factory.mktemp("stream_tick_temporal"))


def _kw(c):
    return dict(qp=c.qp, gop=c.gop, profile_idc=c.prof, slices=c.slices, search=c.search, refs=c.refs, disable_deblock=0 if c.deblock else 1)


def _events(owner, c, i):
    if i in c.forced:
        owner.force_idr()
    for at, qp in c.qps:
        if at == i:
            owner.set_qp(qp)


def _check_picture(owner, got, want, tag):
    au, ft = got
    assert (ft == capi.FRAME_IDR) == want.idr and ft in (capi.FRAME_IDR, capi.FRAME_P), tag + ": frame type"
    assert owner.last_temporal_id == want.layer, tag + ": temporal id"
    assert au == want.au, tag + ": access unit (%d bytes, expected %d)" % (len(au), len(want.au))
    _compare_all(owner, want.stages, tag)


@pytest.mark.parametrize("c", tl.CASES, ids=IDS)
def test_direct_path_every_stage(c):
    want = tl.expected(c)
    enc = capi.Encoder(c.w, c.h, temporal_layers=2, **_kw(c))
    try:
        enc.keep_pre(True)
        for i, f in enumerate(tl.frames(c)):
            _events(enc, c, i)
            _check_picture(enc, enc.encode(f), want[i], "%s direct picture %d layer %d" % (c.name, i, want[i].layer))
        with pytest.raises(capi.EncoderError) as ei:     # before the first picture only
            enc.set_temporal_layers(1)
        assert ei.value.rc == capi.E_ARG
    finally:
        enc.close()


@pytest.mark.parametrize("c", tl.CASES, ids=IDS)
def test_stream_every_stage(c):
    want = tl.expected(c)
    s = capi.Stream(c.w, c.h, temporal_layers=2, **_kw(c))
    try:
        s.keep_pre(True)
        for i, f in enumerate(tl.frames(c)):
            _events(s, c, i)
            _check_picture(s, s.encode(f), want[i], "%s stream picture %d layer %d" % (c.name, i, want[i].layer))
    finally:
        s.close()


def test_refusals_on_a_live_encoder():
    c = tl.BY_NAME["accel_48x48"]
    enc = capi.Encoder(c.w, c.h, **_kw(c))
    try:
        for layers in (0, 3, -2):
            assert capi.lib().mi355x_h264_set_temporal_layers(enc.h, layers) == capi.E_ARG
        enc.set_temporal_layers(2)
        enc.set_temporal_layers(1)
        enc.set_temporal_layers(2)
        n = enc.nmb
        out, ln, ft = C.c_void_p(), C.c_uint32(), C.c_int()
        mb, lv, mv, ax = np.zeros(n, capi.MBINFO_DTYPE), np.zeros((n, capi.LV_STRIDE), np.int16), np.zeros((n, 8), np.int16), np.zeros((n, 16), np.uint8)
        rc = capi.lib().mi355x_h264_debug_code_syntax(enc.h, mb.ctypes.data, lv.ctypes.data, mv.ctypes.data, ax.ctypes.data, tl.frames(c)[0].ctypes.data,
                                                      C.byref(out), C.byref(ln), C.byref(ft))
        assert rc == capi.E_ARG and "temporal" in enc.last_error()
    finally:
        enc.close()


def test_layers_off_is_the_ordinary_stream():
    """an encoder and a stream that do not ask for layers, one that asks for 1: the oracle's ordinary stream, temporal id 0"""
    c = tl.BY_NAME["odd_gop_96x80_high"]
    want = tl.expected_one_layer(c)
    owners = [capi.Encoder(c.w, c.h, **_kw(c)), capi.Encoder(c.w, c.h, temporal_layers=1, **_kw(c)), capi.Stream(c.w, c.h, **_kw(c)),
              capi.Stream(c.w, c.h, temporal_layers=1, **_kw(c))]
    try:
        for i, f in enumerate(tl.frames(c)):
            for o in owners:
                _events(o, c, i)
                au, ft = o.encode(f)
                assert (au, ft == capi.FRAME_IDR) == want[i] and o.last_temporal_id == 0, "picture %d" % i
    finally:
        for o in owners:
            o.close()
    assert b"".join(a for a, _ in want) != tl.stream_of(c)


def test_lockstep_batch_of_four_gops():
    """four closed GOPs in lockstep (encode_gops_device): every item's bytes are its own composed stream's (idr_pic_id runs on
    over the items), item 0's last picture - a layer-1 picture - matches stage by stage"""
    import torch
    G = 4
    b = tl.BY_NAME["accel_48x48"]._replace(gop=8, pictures=8)
    items = [b._replace(name="gop_item%d" % g, seed=5 * g) for g in range(G)]
    want = [tl.compose(c, tl.frames(c), idr_id=g) for g, c in enumerate(items)]
    assert want[0][-1].layer == 1
    fbytes = b.w * b.h * 3 // 2
    dev = torch.from_numpy(np.stack([f for c in items for f in tl.frames(c)])).cuda()
    enc = capi.Encoder(b.w, b.h, batch=G, temporal_layers=2, **_kw(b))
    try:
        enc.keep_pre(True)
        cap = 2 * b.gop * fbytes + 4096
        out, sizes, gb = np.zeros(G * cap, np.uint8), np.zeros(G * b.gop, np.uint32), np.zeros(G, np.uint64)
        for call in range(2):       # (the second call starts closed GOPs again, behind a layer-1 picture)
            enc.set_idr_pic_id(0, 1)
            enc.encode_gops_device(dev.data_ptr(), fbytes, b.gop * fbytes, b.gop, out, cap, sizes, gb)
            for g in range(G):
                aus = [p.au for p in want[g]]
                assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(aus), "call %d item %d: the GOP's bytes" % (call, g)
                assert [int(x) for x in sizes[g * b.gop:(g + 1) * b.gop]] == [len(x) for x in aus], "call %d item %d: sizes[]" % (call, g)
            _compare_all(enc, want[0][-1].stages, "call %d item 0, last picture" % call)
            assert enc.last_temporal_id == 1
    finally:
        enc.close()


def test_two_layer_and_ordinary_streams_share_steps(tick, monkeypatch):
    """six streams of one geometry, three of them two-layer, stream k handing in its first picture at tick k: steps hold layer-0 and
    layer-1 pictures and pictures of ordinary streams side by side (asserted from Stream.last_step), every picture of every stream
    is its own expected stream's"""
    monkeypatch.setenv("MI355X_H264_HUB_WINDOW_US", WINDOW_US)
    monkeypatch.setenv("MI355X_H264_HUB_CTX", "1")
    b = tl.BY_NAME["accel_48x48"]._replace(gop=6)
    N, TICKS, IDLE = 6, 12, 6
    members = [b._replace(name="mixed_%d" % k, seed=7 * k, pictures=TICKS - k, gop=6 + (k & 1)) for k in range(N)]
    two = [k < 3 for k in range(N)]     # (streams 0 and 1 join one tick apart with GOPs of 6 and 7: their layers differ tick by tick)
    want = [tl.expected(c) if two[k] else tuple(tl.Pic(au, idr, 0, None, None, None, None) for au, idr in tl.expected_one_layer(c)) for k, c in enumerate(members)]
    frames = [[np.ascontiguousarray(f) for f in tl.frames(c)] for c in members]
    streams, spare, log = [], [], []
    try:
        for k, c in enumerate(members):
            streams.append(capi.Stream(c.w, c.h, temporal_layers=2 if two[k] else 1, **_kw(c)))
        spare = [capi.Stream(b.w, b.h, **_kw(b)) for _ in range(IDLE)]      # (with one P context the P share is then all six)
        assert streams[0].hub_stats()["open_streams"] == N + IDLE, "two-layer and ordinary streams share an engine"
        streams[0].keep_pre(True)
        for t in range(TICKS):
            part = [k for k in range(N) if t >= k]
            jobs = (Job * len(part))(*[Job(streams[k].h.value, frames[k][t - k].ctypes.data, b.w, b.h, 0, 0, None, 0, 0) for k in part])
            tick(jobs)
            for k, job in zip(part, jobs):
                i = t - k
                streams[k]._check(job.rc)
                au, step, w = C.string_at(job.out, job.len), streams[k].last_step(), want[k][i]
                tag = "tick %d stream %d picture %d step %s" % (t, k, i, step)
                assert (job.frame_type == capi.FRAME_IDR) == w.idr and step["idr"] == w.idr, tag
                assert streams[k].last_temporal_id == w.layer, tag
                assert au == w.au, tag + ": access unit"
                if w.stages is not None:
                    _compare_all(streams[k], w.stages, tag)
                log.append((k, t, (w.layer, two[k]), w.idr, step))
    finally:
        for s in streams + spare:
            s.close()
    steps = steps_of(log)
    kinds = [{p[1] for p in pics} for pics in steps.values()]
    both = [k for k in kinds if {(0, True), (1, True)} <= k]
    mixed = [k for k in kinds if (1, True) in k and (0, False) in k]
    print("%d pictures in %d steps; %d held both layers of two-layer streams, %d a layer-1 picture beside an ordinary stream's" % (len(log), len(steps), len(both), len(mixed)))
    assert both and mixed, "no step held the two layers side by side (step sizes %s)" % sorted(len(p) for p in steps.values())


def _src_i420(owner):
    return owner.debug_read(capi.DBG_SRC).copy()


@pytest.mark.parametrize("layout", ["nv12", "rgba", "scaled", "scaled_refs3"])
def test_other_inputs(layout):
    """NV12 and RGBA pictures and a scaled stream (with and without several reference pictures): the stream is the composed stream
    of the pictures the kernels read (the staging picture behind the conversion / the scaler, which their own suites check)"""
    c = tl.BY_NAME["refs3_112x64_main" if layout == "scaled_refs3" else "accel_48x48"]._replace(pictures=7)
    fr = tl.frames(c)
    if layout == "nv12":
        s = capi.Stream(c.w, c.h, temporal_layers=2, input_format=capi.INPUT_NV12, **_kw(c))
        feed, coded = [lambda f=f: s.encode_nv12(_to_nv12(f, c.w, c.h)) for f in fr], [_to_nv12(f, c.w, c.h) for f in fr]
    elif layout == "rgba":
        s = capi.Stream(c.w, c.h, temporal_layers=2, input_format=capi.INPUT_RGBA, **_kw(c))
        rgba = [ql.frame_rgba(c.w, c.h, sum(tl.SPEEDS[:i])) for i in range(c.pictures)]
        feed, coded = [lambda r=r: s.encode_rgba(r) for r in rgba], [rgba_to_i420(r, c.w, c.h) for r in rgba]
    else:
        big = c._replace(w=2 * c.w, h=2 * c.h - 16)
        s = capi.Stream(c.w, c.h, temporal_layers=2, src_size=(big.w, big.h), **_kw(c))
        feed, coded = [lambda f=f: s.encode(f) for f in tl.frames(big)], None
    try:
        s.keep_pre(True)
        got, srcs = [], []
        for go in feed:
            got.append(go())
            srcs.append(_src_i420(s))
            got[-1] = got[-1] + (s.last_temporal_id, [s.debug_read(capi.DBG_RECON_Y + p) for p in range(3)])
        if coded is not None:
            assert all(np.array_equal(a, b) for a, b in zip(srcs, coded)), "the staging pictures are the converted pictures"
        want = tl.compose(c, fr if layout == "nv12" else srcs)       # (NV12 is read where it lies: the staging picture is the NV12 picture)
        for i, ((au, ft, tid, planes), w) in enumerate(zip(got, want)):
            assert (au, ft == capi.FRAME_IDR, tid) == (w.au, w.idr, w.layer), "%s picture %d" % (layout, i)
            assert all(np.array_equal(planes[p], w.stages.recon(p)) for p in range(3)), "%s picture %d: reconstruction" % (layout, i)
        assert sum(w.layer for w in want) == 3
    finally:
        s.close()


@pytest.mark.parametrize("path", ["direct", "stream"])
def test_quality_and_ssim_records_of_both_layers(path):
    """the quality report serves a layer-1 picture like any other - also when its ring slot is written again by the very next
    picture: SSE and SSIM records and both maps, exact"""
    c = tl.BY_NAME["refs3_112x64_main"]
    want = tl.expected(c)
    o = capi.Encoder(c.w, c.h, temporal_layers=2, **_kw(c)) if path == "direct" else capi.Stream(c.w, c.h, temporal_layers=2, **_kw(c))
    try:
        o.quality_enable(True, ssim=True)
        for i, f in enumerate(tl.frames(c)):
            au, ft = o.encode(f)
            assert au == want[i].au
            src, rec = ql.i420_planes(f, c.w, c.h), [want[i].stages.recon(p) for p in range(3)]
            eq, es = ql.expected(src, rec, c.w, c.h), ss.expected(src, rec, c.w, c.h)
            r = o.quality()[0] if path == "direct" else o.quality()
            tag = "%s picture %d layer %d" % (path, i, want[i].layer)
            assert r["valid"] and tuple(r["sse"]) == eq.sse and tuple(r["samples"]) == eq.samples and r["bytes"] == len(au), tag
            assert r["frame_type"] == ft and ft == (capi.FRAME_IDR if want[i].idr else capi.FRAME_P), tag
            assert tuple(r["ssim_sum"]) == es.sum and tuple(r["ssim_windows"]) == es.windows, tag + ": SSIM"
            assert np.array_equal(o.quality_map(), eq.map) and np.array_equal(o.ssim_map(), es.map), tag + ": maps"
    finally:
        o.close()


def test_pipelined_batch_call_with_the_quality_report():
    """mi355x_h264_encode_batch_device keeps pictures in flight with no host wait between them: a layer-1 picture's comparison and
    the next picture's rewrite of the same ring slot are ordered by the slot's event.  Bytes and every record, exact"""
    import torch
    c = tl.BY_NAME["accel_208x160"]
    want = tl.expected(c)
    assert not c.forced and not c.qps
    fr = tl.frames(c)
    fbytes = c.w * c.h * 3 // 2
    dev = torch.from_numpy(np.stack(fr)).cuda()
    enc = capi.Encoder(c.w, c.h, temporal_layers=2, **_kw(c))
    try:
        enc.quality_enable(True, ssim=True)
        out, sizes = np.zeros(2 * len(fr) * fbytes, np.uint8), np.zeros(len(fr), np.uint32)
        total = enc.encode_batch_device(dev.data_ptr(), fbytes, len(fr), out, sizes)
        assert out[:total].tobytes() == b"".join(p.au for p in want) and [int(x) for x in sizes] == [len(p.au) for p in want]
        recs = enc.quality()
        assert len(recs) == len(fr)
        for i, (r, f) in enumerate(zip(recs, fr)):
            src, rec = ql.i420_planes(f, c.w, c.h), [want[i].stages.recon(p) for p in range(3)]
            eq, es = ql.expected(src, rec, c.w, c.h), ss.expected(src, rec, c.w, c.h)
            assert r["valid"] and tuple(r["sse"]) == eq.sse and tuple(r["ssim_sum"]) == es.sum, "picture %d layer %d" % (i, want[i].layer)
    finally:
        enc.close()


def test_under_guard_mode():
    """one direct run and one stream run with every allocation guarded and poisoned: nothing is written outside a block, and the
    streams are still the composed ones (no kernel relies on what a layer-1 picture left where it should not look)"""
    c = tl.BY_NAME["refs3_112x64_main"]
    want = tl.expected(c)
    with mg.guarded() as seen:
        enc, s = capi.Encoder(c.w, c.h, temporal_layers=2, **_kw(c)), capi.Stream(c.w, c.h, temporal_layers=2, **_kw(c))
        try:
            for i, f in enumerate(tl.frames(c)):
                assert enc.encode(f)[0] == want[i].au and s.encode(f)[0] == want[i].au, "picture %d" % i
        finally:
            enc.close()
            s.close()
    mg.clean(seen, checks=2, kinds=("encoder", "stream"))


@pytest.mark.parametrize("c", [tl.BY_NAME[n] for n in ("odd_gop_96x80_high", "refs3_112x64_main", "tail_80x64")], ids=lambda c: c.name)
def test_decoder_peer_and_decoder_group(c):
    """the GPU's own stream and its base layer (media_amd.temporal.base_layer) through the decoder peer, both side by side through
    a decoder group: every picture is the reconstruction the composition names"""
    want = tl.expected(c)
    enc = capi.Encoder(c.w, c.h, temporal_layers=2, **_kw(c))
    try:
        aus = []
        for i, f in enumerate(tl.frames(c)):
            _events(enc, c, i)
            aus.append(enc.encode(f)[0])
    finally:
        enc.close()
    whole = b"".join(aus)
    base = [a for a, w in zip(aus, want) if w.layer == 0]
    assert mt.base_layer(whole) == b"".join(base) and [mt.base_layer(a) for a in aus] == [a if w.layer == 0 else b"" for a, w in zip(aus, want)]
    want0 = [w for w in want if w.layer == 0]
    for name, units, pics in (("whole", aus, want), ("base layer", base, want0)):
        dec = h264dec.Decoder(0)
        try:
            for i, (au, w) in enumerate(zip(units, pics)):
                assert dec.decode(au), "%s picture %d" % (name, i)
                for p in range(3):
                    assert np.array_equal(dec.plane(p), w.stages.recon(p)), "%s %s picture %d plane %d" % (c.name, name, i, p)
        finally:
            dec.close()
    grp = h264dec.DecoderGroup(2)
    try:
        for i in range(len(aus)):
            step = [aus[i], base[i] if i < len(base) else None]
            res = grp.decode(step)
            for k, (w, au) in enumerate(((want[i], step[0]), (want0[i] if i < len(base) else None, step[1]))):
                if au is None:
                    continue
                assert res[k] == (0, 1), "group stream %d picture %d: %s" % (k, i, grp.error(k))
                planes = grp.debug_planes(k)
                assert all(np.array_equal(planes[p], w.stages.recon(p)) for p in range(3)), "%s group stream %d picture %d" % (c.name, k, i)
    finally:
        grp.close()


@pytest.mark.parametrize("shared", ["", "0"], ids=["stream_path", "engine_of_its_own"])
def test_plugin_object_with_a_scene_cut_on_a_layer1_picture(shared):
    """persist.vmi.video.encode.temporallayers = 2 on both paths of the plugin class, fixed QP: the picture at position 3 is a scene
    cut, found on the layer-1 P picture and coded again as an IDR picture, from which the positions count anew.  Every access unit
    is the composed stream's with an IDR picture forced there; LastTemporalId() follows.  A junk value gives the ordinary stream"""
    from media_amd import videocodec as vc
    c = tl.PLUGIN
    nmb = ((c.w + 15) // 16) * ((c.h + 15) // 16)
    fr = tl.frames(c)
    attempt = tl.compose(c, fr[:4])[3]
    assert attempt.layer == 1 and attempt.cost > tl.SCENE_CUT_COST_PER_MB * nmb, "the cut is found on a layer-1 picture"
    want = tl.compose(c._replace(forced=(3,)), fr)
    assert all(p.cost <= tl.SCENE_CUT_COST_PER_MB * nmb for p in want) and [p.layer for p in want] == [0, 1, 0, 0, 1, 0, 1, 0]

    def run(value):
        vc.set_video_mode(c.w, c.h, qp=c.qp, gop=c.gop, temporallayers=value)
        vc.prop_set("persist.vmi.video.encode.shared", shared)
        e = vc.VideoEncoder()
        out = []
        try:
            assert e.rc_create == vc.SUCCESS and e.init() == vc.SUCCESS and e.start() == vc.SUCCESS
            assert e.last_temporal_id() == -1
            for f in fr:
                rc, au = e.encode(f)
                assert rc == vc.SUCCESS
                out.append((au, e.last_temporal_id()))
            cuts = e.scene_cuts()
        finally:
            e.stop()
            e.destroy()
            e.delete()
            vc.prop_set("persist.vmi.video.encode.shared", "")
            vc.set_video_mode(c.w, c.h)
        return out, cuts

    got, cuts = run(2)
    assert cuts == 1
    for i, ((au, tid), w) in enumerate(zip(got, want)):
        assert tid == w.layer and au == w.au, "picture %d" % i
    one, _ = run("two")
    assert all(tid == 0 for _, tid in one) and [au for au, _ in one] != [p.au for p in want]
    assert all(n[0] != 0x01 for au, _ in one for n in tl.nal_units(au)), "no non-reference slice in the ordinary stream"
