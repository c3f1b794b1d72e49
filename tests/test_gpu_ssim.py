"""SSIM in the quality report on the GPU (include/mi355x_h264.h, "quality report: SSIM": k_ssim) - run with -m gpu on an MI355X.

The cases are those of tests/ssim.py (tests/test_ssim_oracle.py proves on the oracle alone what they hold).  Every sum, window count
and map is compared with the numpy restatement of the header's definition on the test's own input and the oracle's reconstruction,
and must be exactly equal: the GPU's reconstruction is the oracle's bit for bit and every term is an integer, so there is no
tolerance.  The SSE record beside each SSIM record is compared as well: asking for SSIM must not change it."""
import ctypes as C
import numpy as np
import pytest
import mem_guard as mg
import quality as q
import scale
import ssim as S
from media_amd import capi
from media_amd import videocodec as vc
from oracle_lib import OracleEncoder
from test_gpu_stream_matrix import Job, build_tick, WINDOW_US

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tick(tmp_path_factory):
    return build_tick(tmp_path_factory.mktemp("stream_tick_ssim"))


def check(rec, mp, want, tag, au=None, qp=None, idr=None):
    """one record (capi's dict, SSIM added) and its SSIM map against an ssim.Pic: exactly"""
    assert "ssim_sum" in rec, "%s: the record carries no SSIM" % tag
    print("%s: ssim sum %s windows %s mean %s" % (tag, rec["ssim_sum"], rec["ssim_windows"], ["%.4f" % v for v in rec["ssim"]]))
    assert rec["valid"], tag
    assert tuple(rec["ssim_sum"]) == want.rec.sum, "%s: sum %s, expected %s" % (tag, rec["ssim_sum"], want.rec.sum)
    assert tuple(rec["ssim_windows"]) == want.rec.windows, "%s: windows %s, expected %s" % (tag, rec["ssim_windows"], want.rec.windows)
    assert rec["ssim"] == S.mean(want.rec), tag
    assert tuple(rec["sse"]) == want.sse.sse and tuple(rec["samples"]) == want.sse.samples, "%s: the SSE record beside it" % tag
    if au is not None:
        assert rec["bytes"] == len(au), tag
    if qp is not None:
        assert rec["qp"] == qp, tag
    if idr is not None:
        assert rec["frame_type"] == (capi.FRAME_IDR if idr else capi.FRAME_P), tag
    if mp is not None:
        assert mp.dtype == np.int32 and mp.shape == want.rec.map.shape, tag
        assert np.array_equal(mp, want.rec.map), "%s: map differs at %s" % (tag, np.argwhere(mp != want.rec.map)[:4].tolist())
        assert int(mp.astype(np.int64).sum()) == rec["ssim_sum"][0], tag


def _encoder(c, **kw):
    return capi.Encoder(c.w, c.h, qp=c.qp, gop=c.gop, profile_idc=c.prof, disable_deblock=c.nodeblock, slices=c.slices, refs=c.refs, **kw)


def _stream(c, **kw):
    return capi.Stream(c.w, c.h, qp=c.qp, gop=c.gop, profile_idc=c.prof, disable_deblock=c.nodeblock, slices=c.slices, refs=c.refs, **kw)


def _run(c, enc, encode, tag):
    """picture by picture through encode(f) on an Encoder or a Stream with both metrics on: access unit, records and maps"""
    want = S.oracle_run(c)
    enc.quality_enable(True, ssim=True)
    for i, f in enumerate(q.frames(c)):
        au, ft = encode(f)
        t = "%s %s picture %d" % (c.name, tag, i)
        assert au == want[i].au and (ft == capi.FRAME_IDR) == want[i].idr, t + ": access unit"
        rec = enc.quality()
        if isinstance(rec, list):
            assert len(rec) == 1, t
            rec = rec[0]
        check(rec, enc.ssim_map(), want[i], t, au=au, qp=c.qp, idr=want[i].idr)
        assert np.array_equal(enc.quality_map(), want[i].sse.map), t + ": the SSE map beside it"


def _with(obj, fn):
    try:
        fn(obj)
    finally:
        obj.close()


@pytest.mark.parametrize("c", [S.TINY, q.CROP], ids=lambda c: c.name)
def test_host_i420_small_and_partial_macroblocks(c):
    """16x16 (9 luma windows, one per chroma plane) and 34x18 (partial macroblocks on both axes, chroma planes of 17x9)"""
    _with(_encoder(c), lambda e: _run(c, e, e.encode, "encoder"))
    _with(_stream(c), lambda s: _run(c, s, s.encode, "stream"))


def test_noise_at_qp_51_has_negative_windows():
    c = S.NOISE51
    assert all((p.rec.q[0] < 0).any() for p in S.oracle_run(c))
    _with(_encoder(c), lambda e: _run(c, e, e.encode, "encoder"))
    _with(_stream(c), lambda s: _run(c, s, s.encode, "stream"))


@pytest.mark.parametrize("c", [q.PCM, q.NODEBLOCK], ids=lambda c: c.name)
def test_unfiltered_pictures_are_compared_as_they_stand(c):
    """an I_PCM picture (48x48 noise at QP 10: 65536 in every window) and disable_deblock = 1"""
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


def test_rgba_stream():
    """the source is the I420 staging picture the conversion kernel wrote (the oracle's conversion, bit for bit)"""
    c = q.RGBA
    _with(_stream(c, input_format=capi.INPUT_RGBA), lambda s: _run(c, s, s.encode_rgba, "host"))


def test_scaled_stream_is_compared_with_the_resampled_picture():
    """70x38 I420 resampled to 34x18 on the device: src is the resampled picture (tests/scale.py restates it)"""
    c, fmt = scale.BY_NAME["odd_70x38"], scale.FORMATS["i420"]
    pics, want = scale.pictures(c.name, fmt)
    s = capi.Stream(c.w, c.h, qp=34, gop=30, input_format=fmt, src_size=(c.sw, c.sh))
    orc = OracleEncoder(c.w, c.h, qp=34, gop=30)
    try:
        s.quality_enable(True, ssim=True)
        for i in range(c.pictures):
            au, _ = s.encode(pics[i])
            assert au == orc.encode(want[i])[0], "picture %d" % i
            src, recon = q.i420_planes(want[i], c.w, c.h), tuple(orc.recon(p) for p in range(3))
            exp = S.Pic(au, i == 0, S.expected(src, recon, c.w, c.h), q.expected(src, recon, c.w, c.h))
            assert exp.rec.windows == (21, 3, 3) and exp.rec.sum[0] < 65536 * 21
            check(s.quality(), s.ssim_map(), exp, "scaled picture %d" % i, au=au, qp=34, idr=i == 0)
    finally:
        s.close()
        orc.close()


def test_three_reference_pictures_every_ring_slot():
    """refs = 3 over eight pictures: the four ring slots are each compared after having been rewritten"""
    c = q.REFS3
    assert c.pictures == 8 and min(q.ring_rewrites(c.refs, c.pictures)) >= 1
    _with(_encoder(c), lambda e: _run(c, e, e.encode, "encoder"))
    _with(_stream(c), lambda s: _run(c, s, s.encode, "stream"))


def test_two_band_instances_with_halo_swaps():
    """slices = 2 at 96x80: one instance; two band instances of one process with halo swaps - each band's record and map.  The
    bands do not add up to the single instance: the windows that straddle the edge belong to nobody"""
    import torch
    c = q.SLICES
    one = S.oracle_run(c)
    _with(_encoder(c), lambda e: _run(c, e, e.encode, "one instance"))
    want = S.oracle_bands(c, 2)
    parts = [_encoder(c, band_index=r, band_count=2) for r in range(2)]
    try:
        buf = torch.empty(parts[0].band_info()[4], dtype=torch.uint8, device="cuda")
        for p in parts:
            p.quality_enable(True, ssim=True)
        for i, f in enumerate(q.frames(c)):
            aus = [p.encode(f)[0] for p in parts]
            assert b"".join(aus) == want[i][0] == one[i].au, "picture %d" % i
            recs, maps = [p.quality()[0] for p in parts], [p.ssim_map() for p in parts]
            for r in range(2):
                check(recs[r], maps[r], want[i][1][r], "%s band %d picture %d" % (c.name, r, i), au=aus[r], qp=c.qp, idr=one[i].idr)
            assert [a + b for a, b in zip(recs[0]["ssim_windows"], recs[1]["ssim_windows"])] == [n - k for n, k in zip(one[i].rec.windows, (23, 11, 11))]
            assert not maps[0][3:].any() and not maps[1][:3].any()
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
    """encode_gops_device with batch = 3 and encode_batch_device with count = 4: quality_ssim_read is in sizes[] order, the map is
    checked for every item"""
    import torch
    G, c0 = len(q.GOPS), q.GOPS[0]
    n, fbytes = c0.pictures, c0.w * c0.h * 3 // 2
    want = S.oracle_gops()
    dev = torch.from_numpy(np.stack([f for c in q.GOPS for f in q.frames(c)])).cuda()
    enc = _encoder(c0, batch=G)
    try:
        enc.quality_enable(True, ssim=True)
        cap = 2 * n * fbytes + 4096
        out, sizes, gb = np.zeros(G * cap, np.uint8), np.zeros(G * n, np.uint32), np.zeros(G, np.uint64)
        enc.encode_gops_device(dev.data_ptr(), fbytes, n * fbytes, n, out, cap, sizes, gb)
        recs = enc.quality()
        assert len(recs) == G * n
        for g in range(G):
            assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(p.au for p in want[g]), "item %d: the GOP's bytes" % g
            for t in range(n):
                check(recs[g * n + t], enc.ssim_map(g) if t == n - 1 else None, want[g][t], "gops item %d picture %d" % (g, t),
                      au=want[g][t].au, qp=c0.qp, idr=t == 0)
                assert recs[g * n + t]["bytes"] == int(sizes[g * n + t])
        with pytest.raises(capi.EncoderError):
            enc.ssim_map(G)
    finally:
        enc.close()
    c = q.BATCH4
    want = S.oracle_run(c)
    dev = torch.from_numpy(np.stack(q.frames(c))).cuda()
    enc = _encoder(c)
    try:
        enc.quality_enable(True, ssim=True)
        out, sizes = np.zeros(2 * c.pictures * fbytes + 4096, np.uint8), np.zeros(c.pictures, np.uint32)
        tot = enc.encode_batch_device(dev.data_ptr(), fbytes, c.pictures, out, sizes)
        assert out[:tot].tobytes() == b"".join(p.au for p in want)
        recs = enc.quality()
        assert len(recs) == c.pictures
        for t in range(c.pictures):
            check(recs[t], enc.ssim_map(0) if t == c.pictures - 1 else None, want[t], "batch picture %d" % t, au=want[t].au, qp=c.qp, idr=want[t].idr)
    finally:
        enc.close()


def test_hub_streams_of_different_qp_in_shared_steps(tick, monkeypatch):
    """five streams of 64x48 with different content and QPs 20 .. 44 started together; one hands over device pictures, one sits out
    a tick, so positions differ from items afterwards.  Every stream's records and maps"""
    import torch
    monkeypatch.setenv("MI355X_H264_HUB_WINDOW_US", WINDOW_US)
    cases = q.HUB
    want = [S.oracle_run(c) for c in cases]
    frames = [[np.ascontiguousarray(f) for f in q.frames(c)] for c in cases]
    dev = torch.from_numpy(np.stack(frames[q.HUB_DEVICE])).cuda()
    torch.cuda.synchronize()
    streams = [_stream(c) for c in cases]
    try:
        streams[0].quality_enable(True, ssim=True)      # the switch belongs to the shared engine: it holds for all five
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
                check(streams[k].quality(), streams[k].ssim_map(), want[k][i], tag, au=au, qp=cases[k].qp, idr=want[k][i].idr)
                log.append((k, step))
                done[k] += 1
            t += 1
        steps = {}
        for k, st in log:
            steps.setdefault(st["serial"], []).append((k, st["position"]))
        print("hub: %d pictures in %d steps, sizes %s" % (len(log), len(steps), sorted(len(p) for p in steps.values())))
        assert any(len(p) >= 2 for p in steps.values()), "no step carried two pictures"
        assert any(pos != k for p in steps.values() for k, pos in p), "every picture's position was its stream's item"
    finally:
        for s in streams:
            s.close()


def test_1080p_noise_once():
    """1080 is no multiple of 16 (the last macroblock row holds 8 display rows) and 1093 luma windows are negative"""
    c = q.BIG
    want = S.oracle_run(c)[0]
    assert int((want.rec.q[0] < 0).sum()) == 1093
    enc = _encoder(c)
    try:
        enc.quality_enable(True, ssim=True)
        au, ft = enc.encode(q.frames(c)[0])
        assert au == want.au and ft == capi.FRAME_IDR
        check(enc.quality()[0], enc.ssim_map(), want, c.name, au=au, qp=c.qp, idr=True)
    finally:
        enc.close()


def _observed(c, plan, make, encode):
    """the case's pictures with the switch set to metrics plan[i] before picture i (None: left alone); everything an observer could
    change, and what can be read afterwards"""
    L = capi.lib()
    enc = make(c)
    out = []
    try:
        if hasattr(enc, "stats_enable"):
            enc.stats_enable(True)
        for i, f in enumerate(q.frames(c)):
            if plan[i] is not None:
                enc.quality_enable(plan[i] != 0, ssim=plan[i] == 3)
            au, ft = encode(enc, f)
            arrays = [enc.debug_read(w).tobytes() for w in (capi.DBG_RECON_Y, capi.DBG_RECON_U, capi.DBG_RECON_V, capi.DBG_MBINFO, capi.DBG_LEVELS, capi.DBG_MVQ)]
            try:
                rec, mp = enc.quality(), enc.quality_map()
                rec = rec[0] if isinstance(rec, list) else rec
            except capi.EncoderError as err:
                assert err.rc == capi.E_ARG and "quality" in str(err), str(err)
                rec = mp = None
            # what the SSIM entry points give, asked directly (the binding asks only when it was told to)
            s = capi.Ssim()
            if isinstance(enc, capi.Encoder):
                have = L.mi355x_h264_quality_ssim_read(enc.h, C.byref(s), 1)
                assert have in (1, capi.E_ARG)
                have = have == 1
            else:
                have = L.mi355x_h264_stream_last_ssim(enc.h, C.byref(s))
                assert have in (0, capi.E_ARG)
                have = have == 0
            try:
                smap = enc.ssim_map()
            except capi.EncoderError as err:
                assert err.rc == capi.E_ARG and "SSIM" in str(err), str(err)
                smap = None
            assert have == (smap is not None)
            out.append((au, ft, arrays, rec, mp, smap))
        counters = None
        if hasattr(enc, "stats"):
            st = enc.stats()
            counters = (st["frames"], st["p_mbs"], st["me_searched_mbs"], st["tq_coded_mbs"], [(k, v["launches"], v["mbs"]) for k, v in sorted(st["kernels"].items())])
    finally:
        enc.close()
    return out, counters


def _sse_part(rec):
    return None if rec is None else {k: v for k, v in rec.items() if not k.startswith("ssim")}


@pytest.mark.parametrize("kind", ["encoder", "stream"])
def test_the_switch_at_0_1_3_toggled_between_pictures(kind):
    """metrics 1 throughout, 3 throughout, and 0 / 3 / 1 / 3 / 0 toggled between pictures: identical access units, debug_read
    arrays, SSE records and statistics; SSIM is readable exactly after the pictures coded at 3, and not after 1"""
    c = q.HUB[2]
    n = c.pictures
    assert n == 6
    want = S.oracle_run(c)
    make, encode = (_encoder, lambda e, f: e.encode(f)) if kind == "encoder" else (_stream, lambda s, f: s.encode(f))
    sse, st_sse = _observed(c, [1] + [None] * (n - 1), make, encode)
    both, st_both = _observed(c, [3] + [None] * (n - 1), make, encode)
    plan = [0, 3, 1, 3, None, 0]
    mid, st_mid = _observed(c, plan, make, encode)
    assert st_sse == st_both == st_mid
    for i in range(n):
        assert sse[i][0] == both[i][0] == mid[i][0] == want[i].au, "picture %d: access unit" % i
        assert sse[i][1:3] == both[i][1:3] == mid[i][1:3], "picture %d: frame type, debug_read arrays" % i
        assert sse[i][5] is None and "ssim" not in sse[i][3], "picture %d: metrics = 1 gives no SSIM" % i
        assert _sse_part(both[i][3]) == sse[i][3] and np.array_equal(both[i][4], sse[i][4]), "picture %d: the SSE record with SSIM beside it" % i
        check(both[i][3], both[i][5], want[i], "3, picture %d" % i, au=want[i].au, qp=c.qp, idr=want[i].idr)
        if i in (1, 3, 4):
            check(mid[i][3], mid[i][5], want[i], "toggled, picture %d" % i, au=want[i].au, qp=c.qp, idr=want[i].idr)
            assert _sse_part(mid[i][3]) == sse[i][3]
        elif i == 2:
            assert mid[i][3] == sse[i][3] and np.array_equal(mid[i][4], sse[i][4]) and mid[i][5] is None, "picture 2: after 1 no SSIM is readable"
        else:
            assert mid[i][3] is None and mid[i][4] is None and mid[i][5] is None, "picture %d: nothing was compared" % i


def test_refusals_leave_the_handles_usable():
    """_ex(2), _ex(4) and other bits; nothing to read; small caps; null destinations"""
    c = q.GOPS[0]
    L = capi.lib()
    rec, m = (capi.Ssim * 4)(), np.zeros(64, np.int32)
    enc, s = _encoder(c), _stream(c)
    try:
        for bad in (2, 4, 5, 6, 7, 8, 0x80000003):
            assert L.mi355x_h264_quality_enable_ex(enc.h, bad) == capi.E_ARG and "metrics" in enc.last_error(), bad
            assert L.mi355x_h264_stream_quality_enable_ex(s.h, bad) == capi.E_ARG and "metrics" in s.last_error(), bad
        for label, metrics in (("never enabled", 1), ("SSE alone, no picture yet", 3), ("both, no picture yet", 3)):
            assert L.mi355x_h264_quality_ssim_read(enc.h, rec, 4) == capi.E_ARG and "SSIM" in enc.last_error(), label
            assert L.mi355x_h264_quality_ssim_map(enc.h, 0, m.ctypes.data, 64) == capi.E_ARG, label
            assert L.mi355x_h264_stream_last_ssim(s.h, rec) == capi.E_ARG and "SSIM" in s.last_error(), label
            assert L.mi355x_h264_stream_ssim_map(s.h, m.ctypes.data, 64) == capi.E_ARG, label
            assert L.mi355x_h264_quality_enable_ex(enc.h, metrics) == 0 and L.mi355x_h264_stream_quality_enable_ex(s.h, metrics) == 0
        enc._ssim = True
        f = q.frames(c)[0]
        want = S.oracle_run(c)[0]
        assert enc.encode(f)[0] == want.au and s.encode(f)[0] == want.au
        assert L.mi355x_h264_quality_enable_ex(enc.h, 2) == capi.E_ARG      # refused: the switch stays at 3
        assert L.mi355x_h264_quality_ssim_read(enc.h, None, 4) == capi.E_ARG and L.mi355x_h264_quality_ssim_read(enc.h, rec, 0) == capi.E_ARG
        assert L.mi355x_h264_quality_ssim_map(enc.h, 0, None, 64) == capi.E_ARG and L.mi355x_h264_quality_ssim_map(enc.h, 0, m.ctypes.data, enc.nmb - 1) == capi.E_ARG
        assert L.mi355x_h264_quality_ssim_map(enc.h, 1, m.ctypes.data, 64) == capi.E_ARG and L.mi355x_h264_quality_ssim_map(enc.h, -1, m.ctypes.data, 64) == capi.E_ARG
        assert L.mi355x_h264_stream_last_ssim(s.h, None) == capi.E_ARG
        assert L.mi355x_h264_stream_ssim_map(s.h, None, 64) == capi.E_ARG and L.mi355x_h264_stream_ssim_map(s.h, m.ctypes.data, s.nmb - 1) == capi.E_ARG
        check(enc.quality()[0], enc.ssim_map(), want, "encoder after the refusals", au=want.au)
        check(s.quality(), s.ssim_map(), want, "stream after the refusals", au=want.au)
        w1 = S.oracle_run(c)[1]
        assert enc.encode(q.frames(c)[1])[0] == w1.au and s.encode(q.frames(c)[1])[0] == w1.au
        check(enc.quality()[0], enc.ssim_map(), w1, "encoder, next picture", au=w1.au)
        check(s.quality(), s.ssim_map(), w1, "stream, next picture", au=w1.au)
    finally:
        enc.close()
        s.close()


def test_injected_picture_has_a_record_that_is_not_valid():
    """a picture of mi355x_h264_debug_code_syntax (its ring holds nothing meaningful): the SSIM record is present, valid = 0, no map"""
    import test_gpu_entropy_random as er
    c = er.CASES[12]
    enc, o = er.encoder_for(c), er.oracle_for(c)
    try:
        enc.quality_enable(True, ssim=True)
        want, _, _ = o.random_picture(c.seed, features=c.features)
        rc, (got,), ft = enc.code_syntax(*er.arrays(o))
        assert rc == 0 and got == want
        recs = (capi.Ssim * 2)()
        assert capi.lib().mi355x_h264_quality_ssim_read(enc.h, recs, 2) == 1
        assert recs[0].valid == 0 and list(recs[0].sum) == [0, 0, 0] and list(recs[0].windows) == [0, 0, 0]
        r = enc.quality()
        assert len(r) == 1 and not r[0]["valid"] and r[0]["ssim_sum"] == [0, 0, 0] and all(v != v for v in r[0]["ssim"])
        with pytest.raises(capi.EncoderError):
            enc.ssim_map()
    finally:
        enc.close()
        o.close()


def test_guard_mode_every_guard_untouched():
    """the partial-macroblock case and the two band instances' first picture under guard mode (262144 bytes, poison on): k_ssim's
    stores stay inside its two pinned arrays, and every other guard is untouched too"""
    assert mg.GUARD == 262144
    with mg.guarded() as seen:
        c = q.CROP
        _with(_encoder(c), lambda e: _run(c, e, e.encode, "guarded encoder"))
        _with(_stream(c), lambda s: _run(c, s, s.encode, "guarded stream"))
        c = q.SLICES
        want = S.oracle_bands(c, 2)[0]
        for r in range(2):
            e = _encoder(c, band_index=r, band_count=2)
            try:
                e.quality_enable(True, ssim=True)
                au, _ = e.encode(q.frames(c)[0])
                check(e.quality()[0], e.ssim_map(), want[1][r], "guarded band %d" % r, au=au)
            finally:
                e.close()
    mg.clean(seen, checks=2, kinds=["encoder", "stream"])
    assert capi.mem_tally() == seen.tally_before


@pytest.mark.parametrize("shared", ["", "0"], ids=["stream_path", "own_engine"])
def test_plugin_ssim_key(shared):
    """three pictures through vc_encode with persist.vmi.video.encode.ssim = 1 and no .psnr; the last is a scene cut, re-coded as an
    IDR picture: vc_last_ssim and vc_last_quality are that picture's, checked against the oracle replayed at vc_last_qp"""
    c = q.PLUGIN
    vc.set_video_mode(c.w, c.h, qp=c.qp, gop=c.gop, ssim=1, shared=shared)
    e = vc.VideoEncoder()
    try:
        assert e.rc_create == vc.SUCCESS and e.init() == vc.SUCCESS and e.start() == vc.SUCCESS
        assert e.last_ssim() is None and e.last_quality() is None
        got, qps = [], []
        for f in q.frames(c):
            rc, au = e.encode(f)
            assert rc == vc.SUCCESS
            qps.append(e.last_qp())
            got.append((au, e.last_quality(), e.last_ssim()))
        want = S.plugin_replay(c, tuple(qps))
        assert [cut for _, cut in want] == [False, False, True] and e.scene_cuts() == 1
        for i, ((au, rec, s), (pic, cut)) in enumerate(zip(got, want)):
            assert au == pic.au, "picture %d" % i
            assert rec is not None and s is not None and s["valid"], "picture %d: no record" % i
            rec.update(s)
            check(rec, None, pic, "plugin (%s) picture %d" % (shared or "shared", i), au=au, qp=qps[i], idr=pic.idr)
    finally:
        e.stop()
        e.destroy()
        e.delete()
        vc.set_video_mode(c.w, c.h, shared="")
    vc.set_video_mode(c.w, c.h, qp=c.qp, gop=c.gop, psnr=1, shared=shared)      # .psnr alone: the SSE record, no SSIM
    e = vc.VideoEncoder()
    try:
        assert e.init() == vc.SUCCESS and e.start() == vc.SUCCESS and e.encode(q.frames(c)[0])[0] == vc.SUCCESS
        assert e.last_quality() is not None and e.last_ssim() is None
    finally:
        e.stop()
        e.destroy()
        e.delete()
        vc.set_video_mode(c.w, c.h, shared="")
