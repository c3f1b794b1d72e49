"""The quality report on the GPU (include/mi355x_h264.h, "quality report": k_sse) - run with -m gpu on an MI355X.

The cases are those of tests/quality.py (tests/test_quality_oracle.py proves on the oracle alone what they hold).  Every record and
every map is compared with the numpy restatement of the definition on the test's own input and the oracle's reconstruction, and must
be exactly equal: the GPU's reconstruction is the oracle's bit for bit, so there is no tolerance."""
import ctypes as C
import numpy as np
import pytest
import quality as q
from media_amd import capi
from media_amd import videocodec as vc
from test_gpu_stream_matrix import Job, build_tick, WINDOW_US

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tick(tmp_path_factory):
    return build_tick(tmp_path_factory.mktemp("stream_tick_quality"))


def check(rec, mp, want, tag, au=None, qp=None, idr=None):
    """one record (capi's dict) and its map against a quality.Record: exactly"""
    print("%s: sse %s samples %s psnr %s" % (tag, rec["sse"], rec["samples"], ["%.2f" % v for v in rec["psnr"]]))
    assert rec["valid"], tag
    assert tuple(rec["sse"]) == want.sse, "%s: sse %s, expected %s" % (tag, rec["sse"], want.sse)
    assert tuple(rec["samples"]) == want.samples, "%s: samples %s, expected %s" % (tag, rec["samples"], want.samples)
    assert rec["psnr"] == [q.psnr(a, b) for a, b in zip(want.sse, want.samples)], tag
    if au is not None:
        assert rec["bytes"] == len(au), tag
    if qp is not None:
        assert rec["qp"] == qp, tag
    if idr is not None:
        assert rec["frame_type"] == (capi.FRAME_IDR if idr else capi.FRAME_P), tag
    if mp is not None:
        assert mp.dtype == np.uint32 and mp.shape == want.map.shape, tag
        assert np.array_equal(mp, want.map), "%s: map differs at %s" % (tag, np.argwhere(mp != want.map)[:4].tolist())
        assert int(mp.astype(np.uint64).sum()) == sum(rec["sse"]), tag


def _encoder(c, **kw):
    return capi.Encoder(c.w, c.h, qp=c.qp, gop=c.gop, profile_idc=c.prof, disable_deblock=c.nodeblock, slices=c.slices, refs=c.refs, **kw)


def _stream(c, **kw):
    return capi.Stream(c.w, c.h, qp=c.qp, gop=c.gop, profile_idc=c.prof, disable_deblock=c.nodeblock, slices=c.slices, refs=c.refs, **kw)


def _run(c, enc, encode, tag):
    """picture by picture through encode(f) on an Encoder or a Stream with the switch on: access unit, record and map"""
    want = q.oracle_run(c)
    enc.quality_enable(True)
    for i, f in enumerate(q.frames(c)):
        au, ft = encode(f)
        t = "%s %s picture %d" % (c.name, tag, i)
        assert au == want[i].au and (ft == capi.FRAME_IDR) == want[i].idr, t + ": access unit"
        rec = enc.quality()
        if isinstance(rec, list):
            assert len(rec) == 1, t
            rec = rec[0]
        check(rec, enc.quality_map(), want[i].rec, t, au=au, qp=c.qp, idr=want[i].idr)


def _with(obj, fn):
    try:
        fn(obj)
    finally:
        obj.close()


def test_partial_macroblocks_from_host_i420():
    """34x18 at QP 30, gop 4, five pictures (IDR, P, P, P, IDR): partial macroblocks on both axes, width % 4 == 2"""
    c = q.CROP
    _with(_encoder(c), lambda e: _run(c, e, e.encode, "encoder"))
    _with(_stream(c), lambda s: _run(c, s, s.encode, "stream"))


@pytest.mark.parametrize("c", [q.PCM, q.NODEBLOCK], ids=lambda c: c.name)
def test_unfiltered_pictures_are_compared_as_they_stand(c):
    """an I_PCM picture (48x48 noise at QP 10) and disable_deblock = 1"""
    _with(_encoder(c), lambda e: _run(c, e, e.encode, "encoder"))
    _with(_stream(c), lambda s: _run(c, s, s.encode, "stream"))


def test_nv12_from_host_and_from_an_odd_device_address():
    import torch
    c = q.NV12
    _with(_encoder(c), lambda e: _run(c, e, e.encode_nv12, "encoder, host"))
    n = c.w * c.h * 3 // 2
    dev = torch.zeros(c.pictures * (n + 2) + 1, dtype=torch.uint8, device="cuda")
    at = {}
    for i, f in enumerate(q.frames(c)):
        off = 1 + i * (n + 2)       # every picture starts on an odd byte
        dev[off:off + n] = torch.from_numpy(np.array(f)).cuda()
        at[f.ctypes.data] = dev.data_ptr() + off
        assert at[f.ctypes.data] & 1
    torch.cuda.synchronize()
    _with(_encoder(c, input_format=capi.INPUT_NV12), lambda e: _run(c, e, lambda f: e.encode_device(at[f.ctypes.data]), "encoder, device"))
    _with(_stream(c, input_format=capi.INPUT_NV12), lambda s: _run(c, s, lambda f: s.encode_device(at[f.ctypes.data]), "stream, device"))
    _with(_stream(c, input_format=capi.INPUT_NV12), lambda s: _run(c, s, s.encode_nv12, "stream, host"))


def test_rgba_stream_from_host_and_device():
    """the source is the I420 staging picture the conversion kernel wrote (the oracle's conversion, bit for bit)"""
    import torch
    c = q.RGBA
    _with(_stream(c, input_format=capi.INPUT_RGBA), lambda s: _run(c, s, s.encode_rgba, "host"))
    dev = [torch.from_numpy(np.array(f)).cuda() for f in q.frames(c)]
    at = {f.ctypes.data: d.data_ptr() for f, d in zip(q.frames(c), dev)}
    torch.cuda.synchronize()
    _with(_stream(c, input_format=capi.INPUT_RGBA), lambda s: _run(c, s, lambda f: s.encode_device(at[f.ctypes.data]), "device"))


def test_three_reference_pictures_every_ring_slot():
    """refs = 3 on the split 48x48 content of tests/ref_mix.py: the four ring slots are each compared after having been rewritten"""
    c = q.REFS3
    _with(_encoder(c), lambda e: _run(c, e, e.encode, "encoder"))
    _with(_stream(c), lambda s: _run(c, s, s.encode, "stream"))


def test_two_slices_and_two_band_instances():
    """slices = 2 at 96x80: one instance; two band instances of one process with halo swaps - each band's record and map, and their
    sum against the single instance"""
    import torch
    c = q.SLICES
    one = q.oracle_run(c)
    _with(_encoder(c), lambda e: _run(c, e, e.encode, "one instance"))
    want = q.oracle_bands(c, 2)
    parts = [_encoder(c, band_index=r, band_count=2) for r in range(2)]
    try:
        buf = torch.empty(parts[0].band_info()[4], dtype=torch.uint8, device="cuda")
        for p in parts:
            p.quality_enable(True)
        for i, f in enumerate(q.frames(c)):
            aus = [p.encode(f)[0] for p in parts]
            assert b"".join(aus) == want[i][0] == one[i].au, "picture %d" % i
            recs, maps = [p.quality()[0] for p in parts], [p.quality_map() for p in parts]
            for r in range(2):
                check(recs[r], maps[r], want[i][1][r], "%s band %d picture %d" % (c.name, r, i), au=aus[r], qp=c.qp, idr=one[i].idr)
            assert tuple(a + b for a, b in zip(recs[0]["sse"], recs[1]["sse"])) == one[i].rec.sse
            assert tuple(a + b for a, b in zip(recs[0]["samples"], recs[1]["samples"])) == one[i].rec.samples
            assert np.array_equal(maps[0] + maps[1], one[i].rec.map)
            for r in range(2):   # (as tests/test_gpu_ref_mix.py drives them)
                if r > 0:
                    parts[r].halo_export(0, buf.data_ptr())
                    parts[r - 1].halo_import(1, buf.data_ptr())
                if r < 1:
                    parts[r].halo_export(1, buf.data_ptr())
                    parts[r + 1].halo_import(0, buf.data_ptr())
    finally:
        for p in parts:
            p.close()


def test_lockstep_gops_and_batch_in_sizes_order():
    """encode_gops_device with batch = 3 (three pictures per GOP, a content per GOP) and encode_batch_device with count = 4:
    quality_read is in sizes[] order, quality_map is checked for every item"""
    import torch
    G, c0 = len(q.GOPS), q.GOPS[0]
    n, fbytes = c0.pictures, c0.w * c0.h * 3 // 2
    want = q.oracle_gops()
    dev = torch.from_numpy(np.stack([f for c in q.GOPS for f in q.frames(c)])).cuda()
    enc = _encoder(c0, batch=G)
    try:
        enc.quality_enable(True)
        cap = 2 * n * fbytes + 4096
        out, sizes, gb = np.zeros(G * cap, np.uint8), np.zeros(G * n, np.uint32), np.zeros(G, np.uint64)
        enc.encode_gops_device(dev.data_ptr(), fbytes, n * fbytes, n, out, cap, sizes, gb)
        recs = enc.quality()
        assert len(recs) == G * n
        for g in range(G):
            assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(p.au for p in want[g]), "item %d: the GOP's bytes" % g
            for t in range(n):
                check(recs[g * n + t], enc.quality_map(g) if t == n - 1 else None, want[g][t].rec, "gops item %d picture %d" % (g, t),
                      au=want[g][t].au, qp=c0.qp, idr=t == 0)
                assert recs[g * n + t]["bytes"] == int(sizes[g * n + t])
        with pytest.raises(capi.EncoderError):
            enc.quality_map(G)
    finally:
        enc.close()
    c = q.BATCH4
    want = q.oracle_run(c)
    dev = torch.from_numpy(np.stack(q.frames(c))).cuda()
    enc = _encoder(c)
    try:
        enc.quality_enable(True)
        out, sizes = np.zeros(2 * c.pictures * fbytes + 4096, np.uint8), np.zeros(c.pictures, np.uint32)
        tot = enc.encode_batch_device(dev.data_ptr(), fbytes, c.pictures, out, sizes)
        assert out[:tot].tobytes() == b"".join(p.au for p in want)
        recs = enc.quality()
        assert len(recs) == c.pictures
        for t in range(c.pictures):
            check(recs[t], enc.quality_map(0) if t == c.pictures - 1 else None, want[t].rec, "batch picture %d" % t, au=want[t].au, qp=c.qp, idr=want[t].idr)
    finally:
        enc.close()


def test_hub_streams_of_different_qp_in_shared_steps(tick, monkeypatch):
    """five streams of 64x48 with different content and QPs 20 .. 44 started together (tests/test_gpu_stream_matrix.py's way); one
    hands over device pictures, one sits out a tick.  Every stream's records and maps; at least one P step carried two or more
    pictures of different QPs"""
    import torch
    monkeypatch.setenv("MI355X_H264_HUB_WINDOW_US", WINDOW_US)
    cases = q.HUB
    want = [q.oracle_run(c) for c in cases]
    frames = [[np.ascontiguousarray(f) for f in q.frames(c)] for c in cases]
    dev = torch.from_numpy(np.stack(frames[q.HUB_DEVICE])).cuda()
    torch.cuda.synchronize()
    streams = [_stream(c) for c in cases]
    try:
        streams[0].quality_enable(True)      # the switch belongs to the shared engine: it holds for all five
        done = [0] * len(cases)
        log = []
        t = 0
        while min(done) < cases[0].pictures:
            part = [k for k in range(len(cases)) if done[k] < cases[k].pictures and (k, t) != q.HUB_SITS_OUT]
            jobs = (Job * len(part))(*[Job(streams[k].h.value, dev[done[k]].data_ptr() if k == q.HUB_DEVICE else frames[k][done[k]].ctypes.data,
                                           cases[k].w, cases[k].h, int(k == q.HUB_DEVICE), 0, None, 0, 0) for k in part])
            tick(jobs)
            for k, job in zip(part, jobs):
                i = done[k]
                streams[k]._check(job.rc)
                au, step = C.string_at(job.out, job.len), streams[k].last_step()
                tag = "hub stream %d picture %d tick %d step %s" % (k, i, t, step)
                assert au == want[k][i].au and step["idr"] == want[k][i].idr, tag
                check(streams[k].quality(), streams[k].quality_map(), want[k][i].rec, tag, au=au, qp=cases[k].qp, idr=want[k][i].idr)
                log.append((k, cases[k].qp, step))
                done[k] += 1
            t += 1
        steps = {}
        for k, qp, st in log:
            steps.setdefault(st["serial"], []).append((k, qp, st["idr"], st["position"]))
        mixed = [p for p in steps.values() if not p[0][2] and len({x[1] for x in p}) >= 2]
        print("hub: %d pictures in %d steps, sizes %s, %d P steps with two QPs or more" % (len(log), len(steps), sorted(len(p) for p in steps.values()), len(mixed)))
        assert mixed, "no P step carried two pictures of different QPs"
        assert any(x[3] != x[0] for p in steps.values() for x in p), "every picture's position was its stream's item"
    finally:
        for s in streams:
            s.close()


def test_1080p_noise_luma_sse_needs_64_bits():
    c = q.BIG
    want = q.oracle_run(c)[0]
    assert want.rec.sse[0] > 2 ** 32
    enc = _encoder(c)
    try:
        enc.quality_enable(True)
        au, ft = enc.encode(q.frames(c)[0])
        assert au == want.au and ft == capi.FRAME_IDR
        rec = enc.quality()[0]
        assert rec["sse"][0] == want.rec.sse[0] and rec["sse"][0] > 2 ** 32
        check(rec, enc.quality_map(), want.rec, c.name, au=au, qp=c.qp, idr=True)
    finally:
        enc.close()


def _observed(c, plan, make, encode):
    """the case's pictures with the switch set by plan[i] before picture i (None: left alone); everything an observer could change"""
    enc = make(c)
    out = []
    try:
        if hasattr(enc, "stats_enable"):
            enc.stats_enable(True)
        for i, f in enumerate(q.frames(c)):
            if plan[i] is not None:
                enc.quality_enable(plan[i])
            au, ft = encode(enc, f)
            arrays = [enc.debug_read(w).tobytes() for w in (capi.DBG_RECON_Y, capi.DBG_RECON_U, capi.DBG_RECON_V, capi.DBG_MBINFO, capi.DBG_LEVELS, capi.DBG_MVQ)]
            try:
                rec, mp = enc.quality(), enc.quality_map()
                rec = rec[0] if isinstance(rec, list) else rec
            except capi.EncoderError as err:
                assert err.rc == capi.E_ARG and "quality" in str(err), str(err)
                rec = mp = None
            out.append((au, ft, arrays, rec, mp))
        counters = None
        if hasattr(enc, "stats"):
            st = enc.stats()
            counters = (st["frames"], st["p_mbs"], st["me_searched_mbs"], st["tq_coded_mbs"], [(k, v["launches"], v["mbs"]) for k, v in sorted(st["kernels"].items())])
    finally:
        enc.close()
    return out, counters


@pytest.mark.parametrize("kind", ["encoder", "stream"])
def test_the_switch_only_observes(kind):
    """off, on, and turned on after the second picture and off after the fourth: identical access units, debug_read arrays and
    statistics; quality_read refuses where nothing was compared"""
    c = q.HUB[2]
    n = c.pictures
    want = q.oracle_run(c)
    make, encode = (_encoder, lambda e, f: e.encode(f)) if kind == "encoder" else (_stream, lambda s, f: s.encode(f))
    off, st_off = _observed(c, [None] * n, make, encode)
    on, st_on = _observed(c, [True] + [None] * (n - 1), make, encode)
    mid, st_mid = _observed(c, [None, None, True, None, False, None], make, encode)
    assert st_off == st_on == st_mid
    for i in range(n):
        assert off[i][0] == on[i][0] == mid[i][0] == want[i].au, "picture %d: access unit" % i
        assert off[i][1:3] == on[i][1:3] == mid[i][1:3], "picture %d: frame type, debug_read arrays" % i
        assert off[i][3] is None and off[i][4] is None, "picture %d: the switch was never on" % i
        check(on[i][3], on[i][4], want[i].rec, "on, picture %d" % i, au=want[i].au, qp=c.qp, idr=want[i].idr)
        if i in (2, 3):
            check(mid[i][3], mid[i][4], want[i].rec, "turned on, picture %d" % i, au=want[i].au, qp=c.qp, idr=want[i].idr)
        else:
            assert mid[i][3] is None and mid[i][4] is None, "picture %d: nothing was compared" % i


def test_nothing_to_read_and_small_caps_are_refused():
    c = q.GOPS[0]
    L = capi.lib()
    rec, m = (capi.Quality * 4)(), np.zeros(64, np.uint32)
    enc, s = _encoder(c), _stream(c)
    try:
        for label in ("never enabled", "enabled, no picture yet"):
            assert L.mi355x_h264_quality_read(enc.h, rec, 4) == capi.E_ARG and "quality" in enc.last_error(), label
            assert L.mi355x_h264_quality_map(enc.h, 0, m.ctypes.data, 64) == capi.E_ARG, label
            assert L.mi355x_h264_stream_last_quality(s.h, rec) == capi.E_ARG and "quality" in s.last_error(), label
            assert L.mi355x_h264_stream_quality_map(s.h, m.ctypes.data, 64) == capi.E_ARG, label
            enc.quality_enable(True)
            s.quality_enable(True)
        f = q.frames(c)[0]
        want = q.oracle_run(c)[0]
        assert enc.encode(f)[0] == want.au and s.encode(f)[0] == want.au
        assert L.mi355x_h264_quality_read(enc.h, None, 4) == capi.E_ARG and L.mi355x_h264_quality_read(enc.h, rec, 0) == capi.E_ARG
        assert L.mi355x_h264_quality_map(enc.h, 0, None, 64) == capi.E_ARG and L.mi355x_h264_quality_map(enc.h, 0, m.ctypes.data, enc.nmb - 1) == capi.E_ARG
        assert L.mi355x_h264_quality_map(enc.h, 1, m.ctypes.data, 64) == capi.E_ARG and L.mi355x_h264_quality_map(enc.h, -1, m.ctypes.data, 64) == capi.E_ARG
        assert L.mi355x_h264_stream_last_quality(s.h, None) == capi.E_ARG
        assert L.mi355x_h264_stream_quality_map(s.h, None, 64) == capi.E_ARG and L.mi355x_h264_stream_quality_map(s.h, m.ctypes.data, s.nmb - 1) == capi.E_ARG
        # the handles are as usable as before
        check(enc.quality()[0], enc.quality_map(), want.rec, "encoder after the refusals", au=want.au)
        check(s.quality(), s.quality_map(), want.rec, "stream after the refusals", au=want.au)
        assert enc.encode(q.frames(c)[1])[0] == q.oracle_run(c)[1].au and s.encode(q.frames(c)[1])[0] == q.oracle_run(c)[1].au
    finally:
        enc.close()
        s.close()


def test_injected_and_refused_pictures_have_a_record_that_is_not_valid():
    """a picture of mi355x_h264_debug_code_syntax (its ring holds nothing meaningful) and one refused with E_OVERFLOW: the record
    is present, valid = 0; the real picture after them is compared again"""
    import test_gpu_entropy_random as er
    c = er.CASES[12]
    enc, o, ref = er.encoder_for(c), er.oracle_for(c), er.oracle_for(c)
    try:
        enc.quality_enable(True)
        want, _, _ = o.random_picture(c.seed, features=c.features)
        rc, (got,), ft = enc.code_syntax(*er.arrays(o))
        assert rc == 0 and got == want
        recs = enc.quality()
        assert len(recs) == 1 and not recs[0]["valid"] and recs[0]["bytes"] == len(got) and recs[0]["sse"] == [0, 0, 0]
        with pytest.raises(capi.EncoderError):
            enc.quality_map()
        pic = np.random.default_rng(5).integers(0, 256, c.width * c.height * 3 // 2, dtype=np.uint8)
        ref.random_picture(1, features=0)   # (one IDR done: the next idr_pic_id is 1, as the encoder's)
        want, idr = ref.encode(pic, force_idr=True)
        got, ft = enc.encode(pic)
        assert got == want and ft == capi.FRAME_IDR
        rec = q.expected(q.i420_planes(pic, c.width, c.height), tuple(ref.recon(p) for p in range(3)), c.width, c.height)
        check(enc.quality()[0], enc.quality_map(), rec, "the real picture after the injected one", au=got, idr=True)
    finally:
        enc.close()
        o.close()
        ref.close()
    enc = er.encoder_for(er.REFUSAL_CASE, 2)
    try:
        enc.quality_enable(True)
        seen = []
        for step, oracles, want in er.refusal_sequence(2):
            rc, got, ft = enc.code_syntax(*er._stack(oracles))
            recs = enc.quality()
            assert len(recs) == 2 and not any(r["valid"] for r in recs), step
            assert [r["bytes"] for r in recs] == [len(g) if g else 0 for g in got], step
            seen.append((step, rc))
        assert ("refused", capi.E_OVERFLOW) in seen, seen
    finally:
        enc.close()


@pytest.mark.parametrize("shared", ["", "0"], ids=["stream_path", "own_engine"])
def test_plugin_psnr_key(shared):
    """three pictures through vc_encode with persist.vmi.video.encode.psnr = 1; the last is a scene cut, re-coded as an IDR picture:
    vc_last_quality is that picture's, checked against the oracle replayed at vc_last_qp"""
    c = q.PLUGIN
    vc.set_video_mode(c.w, c.h, qp=c.qp, gop=c.gop, psnr=1, shared=shared)
    e = vc.VideoEncoder()
    try:
        assert e.rc_create == vc.SUCCESS and e.init() == vc.SUCCESS and e.start() == vc.SUCCESS
        assert e.last_quality() is None
        got, qps = [], []
        for f in q.frames(c):
            rc, au = e.encode(f)
            assert rc == vc.SUCCESS
            qps.append(e.last_qp())
            got.append((au, e.last_quality()))
        want = q.plugin_replay(c, tuple(qps))
        assert [cut for _, cut in want] == [False, False, True] and e.scene_cuts() == 1
        for i, ((au, rec), (pic, cut)) in enumerate(zip(got, want)):
            assert au == pic.au, "picture %d" % i
            assert rec is not None, "picture %d: no record" % i
            check(rec, None, pic.rec, "plugin (%s) picture %d" % (shared or "shared", i), au=au, qp=qps[i], idr=pic.idr)
    finally:
        e.stop()
        e.destroy()
        e.delete()
        vc.set_video_mode(c.w, c.h, shared="")
    vc.set_video_mode(c.w, c.h, qp=c.qp, gop=c.gop, shared=shared)      # without the key: nothing to read
    e = vc.VideoEncoder()
    try:
        assert e.init() == vc.SUCCESS and e.start() == vc.SUCCESS and e.encode(q.frames(c)[0])[0] == vc.SUCCESS
        assert e.last_quality() is None
    finally:
        e.stop()
        e.destroy()
        e.delete()
        vc.set_video_mode(c.w, c.h, shared="")
