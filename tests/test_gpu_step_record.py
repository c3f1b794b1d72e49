"""A step's pictures as records (media_amd/csrc/item_word.h ItemPic; engine.h submit_step) on the GPU - run with -m gpu on an MI355X.

Both paths read every fact of picture g of a step - frame_num, QP, idr_pic_id, reference count, temporal layer, refresh band - from
its record.  Here: hub steps whose positions differ in all of these, each stream held against a lone encoder of its configuration
(the direct path, whose records come from one stream state), and a direct batch whose items differ in idr_pic_id, against the oracle."""
import ctypes as C
import numpy as np
import pytest
import intra_refresh as ir
import temporal as tl
from media_amd import capi
from oracle_lib import OracleEncoder
from test_gpu_stream_matrix import Job, build_tick, steps_of, WINDOW_US

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tick(tmp_path_factory):
    return build_tick(tmp_path_factory.mktemp("stream_tick_step_record"))


def _frames(w, h, n, seed):
    return [np.ascontiguousarray(tl.frame("accel", w, h, i, seed)) for i in range(n)]


def _lone(w, h, frames, forced=(), **kw):
    """what a lone encoder of the configuration writes for the pictures: [(access unit, idr, temporal id, refresh band)]"""
    enc = capi.Encoder(w, h, **kw)
    out = []
    try:
        for i, f in enumerate(frames):
            if i in forced:
                enc.force_idr()
            au, ft = enc.encode(f)
            out.append((au, ft == capi.FRAME_IDR, enc.last_temporal_id, enc.last_refresh_band))
    finally:
        enc.close()
    return out


def _run_ticks(tick, streams, frames, first, forced, w, h, per_picture):
    """tick t hands picture t - first[k] of every stream k that has one to the hub at the same moment; per_picture(k, i, au, idr, step)"""
    ticks = max(first[k] + len(frames[k]) for k in range(len(streams)))
    for t in range(ticks):
        part = [k for k in range(len(streams)) if 0 <= t - first[k] < len(frames[k])]
        for k in part:
            if t - first[k] in forced[k]:
                streams[k].force_idr()
        jobs = (Job * len(part))(*[Job(streams[k].h.value, frames[k][t - first[k]].ctypes.data, w, h, 0, 0, None, 0, 0) for k in part])
        tick(jobs)
        for k, job in zip(part, jobs):
            streams[k]._check(job.rc)
            per_picture(k, t - first[k], C.string_at(job.out, job.len), job.frame_type == capi.FRAME_IDR, streams[k].last_step())


def test_a_hub_step_of_streams_that_differ_in_every_fact(tick, monkeypatch):
    """three streams of one engine, two reference pictures, QP 22 / 30 / 38, the last with two temporal layers, an IDR picture forced
    on the second at picture 3: P steps hold positions of different reference counts, layers and QPs (asserted from
    Stream.last_step), and every access unit, temporal id and the quality record's QP are the stream's own"""
    monkeypatch.setenv("MI355X_H264_HUB_WINDOW_US", WINDOW_US)
    monkeypatch.setenv("MI355X_H264_HUB_CTX", "1")
    w, h, n, gop = 96, 80, 6, 30
    qps, layers, forced = (22, 30, 38), (1, 1, 2), ((), (3,), ())
    frames = [_frames(w, h, n, 11 * k) for k in range(3)]
    want = [_lone(w, h, frames[k], forced[k], qp=qps[k], gop=gop, refs=2, temporal_layers=layers[k]) for k in range(3)]
    seqs = [tl.sequence(layers[k], gop, 2, n, forced[k]) for k in range(3)]
    for k in range(3):      # (the lone encoder against the restated rule: the reference is what the test takes it for)
        assert [(x[1], x[2]) for x in want[k]] == [(s.idr, s.layer) for s in seqs[k]], k
    streams, spare, log = [], [], []

    def check(k, i, au, idr, step):
        tag = "stream %d picture %d step %s" % (k, i, step)
        assert idr == want[k][i][1] == step["idr"], tag + ": frame type"
        assert au == want[k][i][0], tag + ": not the lone encoder's access unit"
        assert streams[k].last_temporal_id == seqs[k][i].layer, tag + ": last_temporal_id"
        q = streams[k].quality()
        assert q["qp"] == qps[k] and q["valid"] == 1 and q["bytes"] == len(au), tag + ": the quality record %s" % q
        log.append((k, i, (seqs[k][i].nref, seqs[k][i].layer, qps[k]), idr, step))

    try:
        streams = [capi.Stream(w, h, qp=qps[k], gop=gop, refs=2, temporal_layers=layers[k]) for k in range(3)]
        spare = [capi.Stream(w, h, qp=26, gop=gop, refs=2) for _ in range(3)]      # (with one P context the P share is then all three)
        assert streams[0].hub_stats()["open_streams"] == 6, "the streams share one engine"
        streams[0].quality_enable(True)
        _run_ticks(tick, streams, frames, (0, 0, 0), forced, w, h, check)
    finally:
        for s in streams + spare:
            s.close()
    psteps = [[p[1] for p in pics] for pics in steps_of(log).values() if not pics[0][2]]
    print("P steps (nref, layer, qp): %s" % psteps)
    for what, at in (("reference counts", 0), ("temporal layers", 1), ("QPs", 2)):
        assert any(len({f[at] for f in facts}) > 1 for facts in psteps), "no P step held positions of different %s" % what


def test_two_refresh_streams_one_picture_apart(tick, monkeypatch):
    """two intra refresh streams of five bands, the second one picture behind: every P step that holds both holds them at different
    bands, each access unit is the lone encoder's, and the recovery point SEI opens exactly the units of band 0.  (Five bands of two
    macroblock rows or more need ten rows: 96x160 - at 96x80 the picture makes two bands and five slices are refused)"""
    monkeypatch.setenv("MI355X_H264_HUB_WINDOW_US", WINDOW_US)
    monkeypatch.setenv("MI355X_H264_HUB_CTX", "1")
    w, h, n, nb, qp = 96, 160, 8, 5, 26
    frames = [_frames(w, h, n, 7 * k) for k in range(2)]
    want = [_lone(w, h, frames[k], qp=qp, gop=30, slices=nb, intra_refresh=True) for k in range(2)]
    sched = ir.schedule(nb, 30, n)
    for k in range(2):
        assert [(x[1], x[3]) for x in want[k]] == [(idr, band) for idr, _, band in sched], k
    sei = ir.sei_bytes(nb)
    streams, spare, log = [], [], []

    def check(k, i, au, idr, step):
        tag = "stream %d picture %d step %s" % (k, i, step)
        band = streams[k].last_refresh_band
        assert band == sched[i][2] and idr == sched[i][0], tag + ": last_refresh_band"
        assert au == want[k][i][0], tag + ": not the lone encoder's access unit"
        nals = ir.split_nals(au)
        assert au.startswith(sei) == (band == 0) and sum(1 for x in nals if x[0] & 0x1F == 6) == (1 if band == 0 else 0), tag + ": the recovery point SEI"
        log.append((k, i, band, idr, step))

    try:
        streams = [capi.Stream(w, h, qp=qp, gop=30, slices=nb, intra_refresh=True) for _ in range(2)]
        spare = [capi.Stream(w, h, qp=qp, gop=30, slices=nb, intra_refresh=True) for _ in range(2)]      # (the P share is then both)
        assert streams[0].hub_stats()["open_streams"] == 4
        _run_ticks(tick, streams, frames, (0, 1), ((), ()), w, h, check)
    finally:
        for s in streams + spare:
            s.close()
    shared = [[p[1] for p in pics] for pics in steps_of(log).values() if len(pics) == 2]
    print("steps of both streams, their bands: %s" % shared)
    # (ticks 2 .. n - 1 have a P picture of both: six steps when every tick's two pictures are gathered; which are is a matter of
    # timing, so half of them are asked for - what must hold in a shared step is asserted for every one)
    assert len(shared) >= (n - 2) // 2, "the streams did not share their P steps: %s" % shared
    assert all(-1 not in pair and pair[0] != pair[1] for pair in shared), "a step held both streams at one band"


def test_a_direct_batch_steps_idr_pic_id_over_its_items():
    """four closed GOPs in lockstep, set_idr_pic_id(250, 3): the IDR slice headers carry 250, 253, 0, 3 and every item's bytes are
    the oracle's"""
    import torch
    w, h, G, n, qp = 48, 48, 4, 5, 28
    ids = [(250 + 3 * g) & 255 for g in range(G)]
    assert ids == [250, 253, 0, 3]
    frames = [_frames(w, h, n, 5 * g) for g in range(G)]
    want = []
    for g in range(G):
        orc = OracleEncoder(w, h, qp=qp, gop=n)
        orc.set_idr_id(ids[g])
        want.append([orc.encode(f)[0] for f in frames[g]])
        orc.close()
    fbytes = w * h * 3 // 2
    dev = torch.from_numpy(np.stack([f for g in range(G) for f in frames[g]])).cuda()
    enc = capi.Encoder(w, h, qp=qp, gop=n, batch=G)
    try:
        cap = 2 * n * fbytes + 4096
        out, sizes, gb = np.zeros(G * cap, np.uint8), np.zeros(G * n, np.uint32), np.zeros(G, np.uint64)
        enc.set_idr_pic_id(250, 3)
        enc.encode_gops_device(dev.data_ptr(), fbytes, n * fbytes, n, out, cap, sizes, gb)
    finally:
        enc.close()
    got_ids = []
    for g in range(G):
        aus, pos = [], g * cap
        for i in range(n):
            aus.append(out[pos:pos + int(sizes[g * n + i])].tobytes())
            pos += int(sizes[g * n + i])
        assert pos - g * cap == int(gb[g])
        idr = [x for x in tl.nal_units(aus[0]) if x[0] & 0x1F == 5]
        assert len(idr) == 1 and not any(x[0] & 0x1F == 5 for au in aus[1:] for x in tl.nal_units(au)), "item %d: one IDR picture" % g
        r = tl.Bits(tl.unescape(idr[0][1:])[:16])
        assert r.ue() == 0 and r.ue() == 7 and r.ue() == 0 and r.u(8) == 0      # first_mb_in_slice, slice_type, pic_parameter_set_id, frame_num
        got_ids.append(r.ue())
        for i in range(n):
            assert aus[i] == want[g][i], "item %d picture %d: not the oracle's bytes" % (g, i)
    assert got_ids == ids
