"""Intra refresh on the GPU (include/mi355x_h264.h, "intra refresh") - run with -m gpu on an MI355X.  Every comparison is an equality.

1. every access unit decodes on the independent decoder to what debug_read(DBG_RECON_*) holds;
2. recovery: the second content's access units 0 .. c-1 followed by the case's c .. end decode to planes that differ from the case's
   reconstruction somewhere before picture c + n - 1 and equal it in every sample from there on, band j from picture c + j on;
   the same splice of two ordinary slices = n streams still differs at c + n - 1;
3. from DBG_MBINFO / DBG_MVQ: band k all intra, every quadrant of every clean-band macroblock within both row formulas, one at
   least exactly at the bound, no I_PCM; the SEI exactly at k = 0 with the restated bytes; last_refresh_band;
4. doors: five hub streams one tick apart that share steps at different bands while an ordinary slices = n stream beside them has
   another engine and the oracle's bytes; the decoder peer; NV12 from device memory at an odd address, an RGBA stream, a scaled
   stream; a lockstep batch of three; a forced IDR picture mid-cycle; the quality and SSIM records; guard mode; the refusals of
   the C entry points on live encoders; the plugin on both paths with a scene cut.
The oracle pins per band are in tests/test_gpu_intra_refresh_pins.py."""
import ctypes as C
import numpy as np
import pytest
import intra_refresh as ir
import mem_guard as mg
import quality as ql
import ssim as ss
from media_amd import capi, h264dec
from media_amd import refresh as mr
from oracle_lib import OracleDecoder, OracleEncoder, rgba_to_i420
from test_gpu_parity import _to_nv12
from test_gpu_stream_matrix import Job, build_tick, steps_of, WINDOW_US

pytestmark = pytest.mark.gpu
IDS = [c.name for c in ir.CASES]


@pytest.fixture(scope="module")
def tick(tmp_path_factory):
    return build_tick(tmp_path_factory.mktemp("stream_tick_refresh"))


def _kw(c, gop=1000):
    return dict(qp=c.qp, gop=gop, profile_idc=c.prof, slices=c.n, search=c.search)


def _recon(owner):
    return tuple(owner.debug_read(capi.DBG_RECON_Y + p).copy() for p in range(3))


def _encode_all(c, frames, refresh=True, check=False):
    """[(access unit, reconstruction, k)] of the direct path; check: the per-picture facts of point 3"""
    enc = capi.Encoder(c.w, c.h, intra_refresh=refresh, **_kw(c))
    mbw, mbh = (c.w + 15) // 16, (c.h + 15) // 16
    sched = ir.schedule(c.n, 1000, len(frames))
    out, at_bound = [], 0
    try:
        for i, f in enumerate(frames):
            au, ft = enc.encode(f)
            idr, p, k = sched[i] if refresh else (i == 0, 0, -1)
            assert (ft == capi.FRAME_IDR) == idr, "picture %d: frame type" % i
            assert enc.last_refresh_band == k, "picture %d: last_refresh_band" % i
            if check:
                nals = ir.split_nals(au)
                assert [n[0] & 0x1F for n in nals].count(6) == (1 if k == 0 else 0), "picture %d: SEI NAL units" % i
                if k == 0:
                    assert au.startswith(ir.sei_bytes(c.n)), "picture %d: the SEI bytes" % i
                assert sum(1 for n in nals if n[0] & 0x1F in (1, 5)) == c.n
                mb = enc.debug_read(capi.DBG_MBINFO)
                assert not (mb["type"] == ir.MB_IPCM).any(), "picture %d: I_PCM" % i
                if not idr:
                    at_bound += ir.check_picture(mb, enc.debug_read(capi.DBG_MVQ), mbw, mbh, c.n, k)
            out.append((au, _recon(enc), k))
        if refresh:
            with pytest.raises(capi.EncoderError) as ei:   # before the first picture only
                enc.set_intra_refresh(False)
            assert ei.value.rc == capi.E_ARG
    finally:
        enc.close()
    if check:
        assert at_bound > 0, "%s: no clean-band macroblock reads down to row L - the content is too tame" % c.name
    return out


def _decode_all(aus):
    dec, out = OracleDecoder(), []
    for au in aus:
        assert dec.decode(au) == 1
        out.append(tuple(dec.plane(p).copy() for p in range(3)))
    dec.close()
    return out


_STREAMS = {}


def _case_stream(c):
    if c.name not in _STREAMS:
        _STREAMS[c.name] = _encode_all(c, ir.frames(c), check=True)
    return _STREAMS[c.name]


@pytest.mark.parametrize("c", ir.CASES, ids=IDS)
def test_bound_intra_band_sei_and_decoder_equality(c):
    a = _case_stream(c)
    for i, (planes, (au, rec, k)) in enumerate(zip(_decode_all([x[0] for x in a]), a)):
        for p in range(3):
            assert np.array_equal(planes[p], rec[p]), "%s picture %d plane %d: the decoder differs from the reconstruction" % (c.name, i, p)


@pytest.mark.parametrize("c", ir.CASES, ids=IDS)
def test_recovery(c):
    n, cut = c.n, ir.cut_of(c)
    a = _case_stream(c)
    b = _encode_all(c, ir.frames_other(c)[:cut])
    assert all(x[0] != y[0] for x, y in zip(a[:cut], b)), "the prefixes do not differ"
    assert a[cut][2] == 0
    got = _decode_all([x[0] for x in b] + [x[0] for x in a[cut:]])
    bands = ir.band_rows((c.h + 15) // 16, n)
    assert any(ir.band_differs(got[i], a[i][1], bands, j) for i in range(cut, cut + n - 1) for j in range(n)), "nothing to recover from"
    for i in range(cut, c.pictures):
        for j in range(n):
            if i >= cut + j:
                assert not ir.band_differs(got[i], a[i][1], bands, j), "%s: picture %d band %d has not recovered" % (c.name, i, j)
    for i in range(cut + n - 1, c.pictures):
        for p in range(3):
            assert np.array_equal(got[i][p], a[i][1][p]), "%s: picture %d plane %d" % (c.name, i, p)


@pytest.mark.parametrize("c", ir.SMALL[:2], ids=IDS[:2])
def test_control_without_refresh_does_not_recover(c):
    n, cut = c.n, ir.cut_of(c)
    a = _encode_all(c, ir.frames(c), refresh=False)
    b = _encode_all(c, ir.frames_other(c)[:cut], refresh=False)
    got = _decode_all([x[0] for x in b] + [x[0] for x in a[cut:]])
    i = cut + n - 1
    assert any(not np.array_equal(got[i][p], a[i][1][p]) for p in range(3)), "%s: recovered without refresh" % c.name
    # and refresh off is the ordinary stream: the oracle's bytes
    orc = OracleEncoder(c.w, c.h, qp=c.qp, gop=1000, profile_idc=c.prof, slices=c.n, search=c.search)
    for k, f in enumerate(ir.frames(c)):
        assert orc.encode(f)[0] == a[k][0], "%s: picture %d differs from the oracle with refresh off" % (c.name, k)
    orc.close()


def test_five_streams_one_tick_apart_share_steps_at_different_bands(tick, monkeypatch):
    """five refresh streams of one geometry, stream k handing in its first picture at tick k, every tick's pictures handed to the hub
    at the same moment by native threads: P steps hold several pictures whose bands differ (asserted from Stream.last_step and each
    stream's own last_refresh_band), every access unit is the direct path's, and the vectors of every picture keep the bound -
    the indirect k_me reads each position's own band from its itemtab word.  An ordinary slices = n stream opened beside them is
    on another engine and keeps the oracle's bytes"""
    monkeypatch.setenv("MI355X_H264_HUB_WINDOW_US", WINDOW_US)
    monkeypatch.setenv("MI355X_H264_HUB_CTX", "1")
    c = ir.BY_NAME["A_96x128_n4"]
    want = _case_stream(c)
    fr = [np.ascontiguousarray(f) for f in ir.frames(c)]
    mbw, mbh = (c.w + 15) // 16, (c.h + 15) // 16
    N, IDLE = 5, 5
    TICKS = c.pictures + N - 1
    streams, spare, log = [], [], []
    plain = None
    orc = OracleEncoder(c.w, c.h, qp=c.qp, gop=1000, profile_idc=c.prof, slices=c.n, search=c.search)
    try:
        streams = [capi.Stream(c.w, c.h, intra_refresh=True, **_kw(c)) for _ in range(N)]
        spare = [capi.Stream(c.w, c.h, intra_refresh=True, **_kw(c)) for _ in range(IDLE)]   # (with one P context the P share is then all five)
        plain = capi.Stream(c.w, c.h, **_kw(c))
        assert streams[0].hub_stats()["open_streams"] == N + IDLE, "the refresh streams share one engine"
        assert plain.hub_stats()["open_streams"] == 1, "the ordinary stream of as many slices has an engine of its own"
        for t in range(TICKS):
            part = [k for k in range(N) if 0 <= t - k < c.pictures]
            jobs = (Job * len(part))(*[Job(streams[k].h.value, fr[t - k].ctypes.data, c.w, c.h, 0, 0, None, 0, 0) for k in part])
            tick(jobs)
            for k, job in zip(part, jobs):
                i = t - k
                streams[k]._check(job.rc)
                au, step, band = C.string_at(job.out, job.len), streams[k].last_step(), streams[k].last_refresh_band
                tag = "tick %d stream %d picture %d step %s" % (t, k, i, step)
                assert band == want[i][2], tag + ": last_refresh_band"
                assert au == want[i][0], tag + ": not the direct path's access unit"
                if band >= 0:
                    ir.check_picture(streams[k].debug_read(capi.DBG_MBINFO), streams[k].debug_read(capi.DBG_MVQ), mbw, mbh, c.n, band)
                log.append((k, t, band, want[i][0][4] & 0x1F == 7, step))
            if t < c.pictures:
                assert plain.encode(fr[t])[0] == orc.encode(fr[t])[0], "the ordinary stream's picture %d" % t
                assert plain.last_refresh_band == -1
    finally:
        for s in streams + spare + ([plain] if plain else []):
            s.close()
        orc.close()
    steps = steps_of(log)
    bands = [sorted(p[1] for p in pics) for pics in steps.values()]
    several = [b for b in bands if len(b) > 1 and len(set(b)) > 1 and -1 not in b]
    print("%d pictures in %d steps; %d P steps held different bands: %s" % (len(log), len(steps), len(several), several[:6]))
    assert several, "no P step held pictures at different bands (step sizes %s)" % sorted(len(b) for b in bands)


def test_forced_idr_mid_cycle_restarts_the_cycle():
    c = ir.BY_NAME["B_112x96_n3_seeded"]
    enc = capi.Encoder(c.w, c.h, intra_refresh=True, **_kw(c))
    sched = ir.schedule(c.n, 1000, c.pictures, forced=(5,))
    try:
        aus = []
        for i, f in enumerate(ir.frames(c)):
            if i == 5:
                enc.force_idr()
            au, ft = enc.encode(f)
            assert ((ft == capi.FRAME_IDR), enc.last_refresh_band) == (sched[i][0], sched[i][2]), "picture %d" % i
            assert au.startswith(ir.sei_bytes(c.n)) == (sched[i][2] == 0)
            aus.append((au, _recon(enc)))
        for i, planes in enumerate(_decode_all([x[0] for x in aus])):
            assert all(np.array_equal(planes[p], aus[i][1][p]) for p in range(3)), "picture %d" % i
    finally:
        enc.close()


@pytest.mark.parametrize("c", [ir.BY_NAME[n] for n in ("A_96x128_n4", "B_112x96_n3_seeded", "C_64x80_n2_high")], ids=lambda c: c.name)
def test_decoder_peer(c):
    """the decoder peer from the IDR picture on (it does not join at a recovery point): every picture is the reconstruction"""
    a = _case_stream(c)
    dec = h264dec.Decoder(0)
    try:
        for i, (au, rec, k) in enumerate(a):
            assert dec.decode(au), "%s picture %d: the decoder peer produced no picture" % (c.name, i)
            for p in range(3):
                assert np.array_equal(dec.plane(p), rec[p]), "%s picture %d plane %d" % (c.name, i, p)
    finally:
        dec.close()
    whole = b"".join(x[0] for x in a)
    pts = mr.recovery_points(whole)
    assert [cnt for _, cnt in pts] == [c.n - 1] * sum(1 for x in a if x[2] == 0)
    assert all(whole[o:].startswith(ir.sei_bytes(c.n)) for o, _ in pts)


@pytest.mark.parametrize("layout", ["nv12_device_odd", "rgba", "scaled"])
def test_other_inputs(layout):
    """NV12 read in place from device memory at an odd address, an RGBA stream, a scaled stream: the schedule, the SEI, the intra
    band and the bound hold, the independent decoder gives the reconstruction, and the stream is the direct path's stream of the
    pictures the kernels read (the staging picture behind the conversion / the scaler)"""
    import torch
    c = ir.BY_NAME["B_112x96_n3_seeded"]
    fr = ir.frames(c)[:8]
    mbw, mbh = (c.w + 15) // 16, (c.h + 15) // 16
    sched = ir.schedule(c.n, 1000, len(fr))
    keep = []
    if layout == "nv12_device_odd":
        s = capi.Stream(c.w, c.h, intra_refresh=True, input_format=capi.INPUT_NV12, **_kw(c))
        feed = []
        for f in fr:
            t = torch.zeros(len(f) + 1, dtype=torch.uint8, device="cuda")
            t[1:] = torch.from_numpy(_to_nv12(f, c.w, c.h)).cuda()
            keep.append(t)
            assert (t.data_ptr() + 1) & 1
            feed.append(lambda t=t: s.encode_device(t.data_ptr() + 1))
        coded = list(fr)
    elif layout == "rgba":
        s = capi.Stream(c.w, c.h, intra_refresh=True, input_format=capi.INPUT_RGBA, **_kw(c))
        rgba = [ql.frame_rgba(c.w, c.h, 3 * i) for i in range(len(fr))]
        feed, coded = [lambda r=r: s.encode_rgba(r) for r in rgba], [rgba_to_i420(r, c.w, c.h) for r in rgba]
    else:
        big = c._replace(w=2 * c.w, h=2 * c.h - 16)
        s = capi.Stream(c.w, c.h, intra_refresh=True, src_size=(big.w, big.h), **_kw(c))
        feed, coded = [lambda f=f: s.encode(f) for f in ir.frames(big)[:8]], None
    try:
        got = []
        for i, go in enumerate(feed):
            au, ft = go()
            idr, p, k = sched[i]
            assert (ft == capi.FRAME_IDR, s.last_refresh_band) == (idr, k), "%s picture %d" % (layout, i)
            assert au.startswith(ir.sei_bytes(c.n)) == (k == 0)
            if not idr:
                ir.check_picture(s.debug_read(capi.DBG_MBINFO), s.debug_read(capi.DBG_MVQ), mbw, mbh, c.n, k)
            src = None if layout == "nv12_device_odd" else s.debug_read(capi.DBG_SRC).copy()
            got.append((au, _recon(s), src))
        for i, planes in enumerate(_decode_all([x[0] for x in got])):
            assert all(np.array_equal(planes[p], got[i][1][p]) for p in range(3)), "%s picture %d: decoder" % (layout, i)
        if coded is None:
            coded = [x[2] for x in got]
        elif layout == "rgba":
            assert all(np.array_equal(x[2], w) for x, w in zip(got, coded)), "the staging pictures are the converted pictures"
        direct = _encode_all(c, coded)
        assert [x[0] for x in got] == [x[0] for x in direct], "%s: not the direct path's stream of the same pictures" % layout
    finally:
        s.close()


def test_lockstep_batch_of_three():
    """three closed GOPs in lockstep (encode_gops_device): every item's bytes are those of a direct encoder with the item's
    idr_pic_id; the band and the SEI are every item's"""
    import torch
    G = 3
    c = ir.BY_NAME["C_64x80_n2_high"]
    contents = [ir.frames(c), ir.frames_other(c), tuple(reversed(ir.frames(c)))]
    want = []
    for g, fr in enumerate(contents):
        e = capi.Encoder(c.w, c.h, intra_refresh=True, **_kw(c))
        try:
            e.set_idr_pic_id(g, 1)
            want.append([e.encode(f)[0] for f in fr])
        finally:
            e.close()
    fbytes, n = c.w * c.h * 3 // 2, c.pictures
    dev = torch.from_numpy(np.stack([f for fr in contents for f in fr])).cuda()
    enc = capi.Encoder(c.w, c.h, batch=G, intra_refresh=True, **_kw(c))
    try:
        cap = 2 * n * fbytes + 4096
        out, sizes, gb = np.zeros(G * cap, np.uint8), np.zeros(G * n, np.uint32), np.zeros(G, np.uint64)
        for call in range(2):
            enc.set_idr_pic_id(0, 1)
            enc.encode_gops_device(dev.data_ptr(), fbytes, n * fbytes, n, out, cap, sizes, gb)
            for g in range(G):
                assert [int(x) for x in sizes[g * n:(g + 1) * n]] == [len(x) for x in want[g]], "call %d item %d: sizes[]" % (call, g)
                assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(want[g]), "call %d item %d: the GOP's bytes" % (call, g)
            assert enc.last_refresh_band == ir.schedule(c.n, 1000, n)[-1][2]
        assert sum(a.startswith(ir.sei_bytes(c.n)) for a in want[1]) == (n - 1 + c.n - 1) // c.n
    finally:
        enc.close()


@pytest.mark.parametrize("path", ["direct", "stream"])
def test_quality_and_ssim_records(path):
    """the quality report of a refresh stream: SSE and SSIM records and both maps equal numpy on the reconstruction"""
    c = ir.BY_NAME["B_112x96_n3_seeded"]
    want = _case_stream(c)
    o = capi.Encoder(c.w, c.h, intra_refresh=True, **_kw(c)) if path == "direct" else capi.Stream(c.w, c.h, intra_refresh=True, **_kw(c))
    try:
        o.quality_enable(True, ssim=True)
        for i, f in enumerate(ir.frames(c)[:7]):
            au, ft = o.encode(f)
            assert au == want[i][0]
            src, rec = ql.i420_planes(f, c.w, c.h), list(want[i][1])
            eq, es = ql.expected(src, rec, c.w, c.h), ss.expected(src, rec, c.w, c.h)
            r = o.quality()[0] if path == "direct" else o.quality()
            tag = "%s picture %d" % (path, i)
            assert r["valid"] and tuple(r["sse"]) == eq.sse and tuple(r["samples"]) == eq.samples and r["bytes"] == len(au), tag
            assert tuple(r["ssim_sum"]) == es.sum and tuple(r["ssim_windows"]) == es.windows, tag + ": SSIM"
            assert np.array_equal(o.quality_map(), eq.map) and np.array_equal(o.ssim_map(), es.map), tag + ": maps"
    finally:
        o.close()


def test_under_guard_mode():
    """one direct run and one stream run with every allocation guarded and poisoned: nothing is written outside a block (the
    forced band's waves write MbInfo, vectors and me_cost before anything else), and the streams are the unguarded ones"""
    c = ir.BY_NAME["C_64x80_n2_high"]
    want = _case_stream(c)
    with mg.guarded() as seen:
        enc, s = capi.Encoder(c.w, c.h, intra_refresh=True, **_kw(c)), capi.Stream(c.w, c.h, intra_refresh=True, **_kw(c))
        try:
            for i, f in enumerate(ir.frames(c)):
                assert enc.encode(f)[0] == want[i][0] and s.encode(f)[0] == want[i][0], "picture %d" % i
        finally:
            enc.close()
            s.close()
    mg.clean(seen, checks=2, kinds=("encoder", "stream"))


def test_refusals_of_the_c_entry_points_on_live_encoders():
    """mi355x_h264_set_intra_refresh itself (capi.Encoder(intra_refresh=True) refuses the same in front of it): slices 1 and 33,
    a height that has no such bands, refs 2, two layers in either order, a band instance; mi355x_h264_debug_code_syntax"""
    L = capi.lib()
    for kw, why in ((dict(slices=0), "slices"), (dict(slices=1), "slices"), (dict(slices=33), "slices"), (dict(slices=3), "divide"),
                    (dict(slices=2, refs=2), "reference"), (dict(slices=2, temporal_layers=2), "layer"),
                    (dict(slices=2, band_index=0, band_count=2), "band instance")):
        enc = capi.Encoder(64, 64, **kw)
        try:
            assert L.mi355x_h264_set_intra_refresh(enc.h, 1) == capi.E_ARG and why in enc.last_error(), (kw, enc.last_error())
            assert L.mi355x_h264_set_intra_refresh(enc.h, 2) == capi.E_ARG
            assert L.mi355x_h264_set_intra_refresh(enc.h, 0) == 0 and enc.last_refresh_band == -1
        finally:
            enc.close()
    enc = capi.Encoder(64, 64, slices=2, intra_refresh=True)
    try:
        with pytest.raises(capi.EncoderError) as ei:      # the other order
            enc.set_temporal_layers(2)
        assert ei.value.rc == capi.E_ARG
        n = enc.nmb
        out, ln, ft = C.c_void_p(), C.c_uint32(), C.c_int()
        mb, lv, mv, ax = np.zeros(n, capi.MBINFO_DTYPE), np.zeros((n, capi.LV_STRIDE), np.int16), np.zeros((n, 8), np.int16), np.zeros((n, 16), np.uint8)
        src = np.zeros(64 * 64 * 3 // 2, np.uint8)
        rc = L.mi355x_h264_debug_code_syntax(enc.h, mb.ctypes.data, lv.ctypes.data, mv.ctypes.data, ax.ctypes.data, src.ctypes.data,
                                             C.byref(out), C.byref(ln), C.byref(ft))
        assert rc == capi.E_ARG and "intra refresh" in enc.last_error()
    finally:
        enc.close()


@pytest.mark.parametrize("shared", ["", "0"], ids=["stream_path", "engine_of_its_own"])
def test_plugin_object_with_a_scene_cut(shared):
    """persist.vmi.video.encode.intrarefresh = n on both paths of the plugin class, fixed QP, over the second content: its picture
    cut_of(c) (the first of the case's own, behind checkered ones) is a scene cut, found on the P picture and coded again as an IDR picture, from which p counts anew.  Every access
    unit is that of a direct encoder driven by the same rule; LastRefreshBand() follows.  Junk and a conflict give the
    ordinary stream"""
    from media_amd import videocodec as vc
    c = ir.BY_NAME["A_96x128_n4"]
    cut = ir.cut_of(c)

    def checkered(f, i):   # the second content under a coarse checker that scrolls with it: nothing of it matches the case's pictures
        f = f.copy()
        y = f[:c.w * c.h].reshape(c.h, c.w).astype(np.int32)
        yy, xx = np.arange(c.h)[:, None] + c.step * i, np.arange(c.w)[None, :]
        f[:c.w * c.h] = np.clip(y + ((((yy >> 3) + (xx >> 3)) & 1) * 120 - 60), 0, 255).astype(np.uint8).ravel()
        return f
    fr = [checkered(f, i) if i < cut else f for i, f in enumerate(ir.frames_other(c))]
    nmb = ((c.w + 15) // 16) * ((c.h + 15) // 16)
    want, cuts_want = [], 0
    d = capi.Encoder(c.w, c.h, intra_refresh=True, qp=c.qp, gop=30, slices=c.n)
    try:
        for f in fr:
            au, ft = d.encode(f)
            if ft == capi.FRAME_P and d.me_cost()[0] > ql.SCENE_CUT_COST_PER_MB * nmb:
                d.force_idr()
                au, ft = d.encode(f)
                cuts_want += 1
            want.append((au, d.last_refresh_band))
    finally:
        d.close()
    assert cuts_want >= 1 and want[cut][1] == -1 and want[cut + 1][1] == 0 and want[cut - 1][1] > 0, "a scene cut mid-cycle at picture %d" % cut

    def run(value, **other):
        vc.set_video_mode(c.w, c.h, qp=c.qp, gop=30, intrarefresh=value, **other)
        vc.prop_set("persist.vmi.video.encode.shared", shared)
        e = vc.VideoEncoder()
        out = []
        try:
            assert e.rc_create == vc.SUCCESS and e.init() == vc.SUCCESS and e.start() == vc.SUCCESS
            assert e.last_refresh_band() == -1
            for f in fr:
                rc, au = e.encode(f)
                assert rc == vc.SUCCESS
                out.append((au, e.last_refresh_band()))
            cuts = e.scene_cuts()
        finally:
            e.stop()
            e.destroy()
            e.delete()
            vc.prop_set("persist.vmi.video.encode.shared", "")
            vc.set_video_mode(c.w, c.h)
        return out, cuts

    got, cuts = run(c.n)
    assert cuts == cuts_want
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "picture %d: band %d, expected %d; %d bytes, expected %d" % (i, g[1], w[1], len(g[0]), len(w[0]))
    for value, other in (("four", {}), (c.n, {"slices": c.n + 1}), (c.n, {"refs": 2}), (c.n, {"temporallayers": 2}), (33, {})):
        off, _ = run(value, **other)
        assert all(b == -1 for _, b in off) and not any(au.startswith(ir.sei_bytes(c.n)) for au, _ in off), (value, other)
