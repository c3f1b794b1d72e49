"""Streams that search two and three reference pictures (mi355x_h264_stream_open_ex, MI355X_H264_STREAM_MULTIREF) on the GPU - run
with -m gpu on an MI355X.

The cases are those of tests/stream_refs.py (tests/test_stream_refs_oracle.py proves on the oracle alone what the list holds).  A
stream's pictures go through the hub's shared steps, whose indirect kernels take every position's own number of usable reference
pictures from the itemtab word.  Everything is compared exactly: access units byte for byte, MbInfo, levels, vectors, the planes
before and after the loop filter (test_gpu_parity._compare_all through Stream.debug_read)."""
import ctypes as C
import threading
import numpy as np
import pytest
import ref_mix as rm
import stream_refs as sr
from media_amd import capi
from media_amd import videocodec as vc
from test_gpu_parity import _compare_all
from test_gpu_stream_matrix import Job, build_tick, steps_of, WINDOW_US

pytestmark = pytest.mark.gpu
BOTH = [(c, s) for c in sr.ONE for s in rm.SEARCHES]
IDS = ["%s-search%d" % (c.name, s) for c, s in BOTH]


@pytest.fixture(scope="module")
def tick(tmp_path_factory):
    return build_tick(tmp_path_factory.mktemp("stream_tick_refs"))


def _stream(c, search, **kw):
    kw.setdefault("refs", c.refs)
    return capi.Stream(c.w, c.h, qp=c.qp, gop=c.gop, profile_idc=c.prof, slices=c.slices, search=search,
                       input_format=capi.INPUT_NV12 if c.nv12 else capi.INPUT_I420, **kw)


@pytest.mark.parametrize("c,search", BOTH, ids=IDS)
def test_one_stream_every_stage(c, search):
    want = rm.expected(c, search)
    s = _stream(c, search)
    try:
        s.keep_pre(True)
        for i, f in enumerate(rm.frames(c)):
            tag = "%s search %d picture %d" % (c.name, search, i)
            au, ft = s.encode_nv12(rm.to_nv12(f, c.w, c.h)) if c.nv12 else s.encode(f)
            assert (ft == capi.FRAME_IDR) == want[i].idr, tag
            assert au == want[i].au, tag + ": access unit"
            _compare_all(s, want[i].stages, tag)
    finally:
        s.close()


def test_mixed_counts_in_one_step(tick, monkeypatch):
    """the mixed group of tests/stream_refs.py: six streams, stream k handing in its first picture at tick k, GOP lengths of their
    own, a forced IDR picture and a QP walk in mid-run; every picture of every stream against an oracle driven the same way.  That
    pictures with one, two and three reference pictures DID share a step, and that a step's positions are ordered by the count, is
    asserted from what the hub reports (Stream.last_step), the counts worked out from the pictures since each stream's IDR"""
    monkeypatch.setenv("MI355X_H264_HUB_WINDOW_US", WINDOW_US)
    monkeypatch.setenv("MI355X_H264_HUB_CTX", "1")
    streams, spare, log = [], [], []
    since = [0] * len(sr.MIXED)
    try:
        for m in sr.MIXED:
            streams.append(_stream(m.case, 1))
        spare = [_stream(sr.MIXED[0].case, 1) for _ in range(sr.IDLE)]
        streams[0].keep_pre(True)
        want = [sr.expected(m) for m in sr.MIXED]
        frames = [[np.ascontiguousarray(f) for f in rm.frames(m.case)] for m in sr.MIXED]
        for t, sched in enumerate(sr.schedule()):
            part = [sr.MIXED[k] for k, _, _ in sched]
            for m in part:
                for at, what in m.events:
                    if at == t - m.join and what == "idr":
                        streams[m.k].force_idr()
                    elif at == t - m.join:
                        streams[m.k].set_qp(what)
            jobs = (Job * len(part))(*[Job(streams[m.k].h.value, frames[m.k][t - m.join].ctypes.data, m.case.w, m.case.h, 0, 0, None, 0, 0) for m in part])
            tick(jobs)
            for m, job in zip(part, jobs):
                i = t - m.join
                streams[m.k]._check(job.rc)
                au, step = C.string_at(job.out, job.len), streams[m.k].last_step()
                tag = "tick %d stream %d picture %d step %s" % (t, m.k, i, step)
                idr = job.frame_type == capi.FRAME_IDR
                assert idr == want[m.k][i].idr and step["idr"] == idr, tag + ": picture type"
                assert au == want[m.k][i].au, tag + ": access unit differs from the oracle's"
                _compare_all(streams[m.k], want[m.k][i].stages, tag)
                since[m.k] = 0 if idr else since[m.k] + 1
                count = min(sr.REFS, since[m.k])
                assert count == want[m.k][i].facts["available"], tag
                log.append((m.k, t, count, idr, step))
    finally:
        for s in streams + spare:
            s.close()
    steps = steps_of(log)       # {serial: [(stream, count, idr, position, pictures)]}, the reported facts checked against each other
    sizes = sorted(len(p) for p in steps.values())
    together = [pics for pics in steps.values() if {1, 2, 3} <= {p[1] for p in pics}]
    print("%d pictures in %d steps (sizes %s); %d steps held counts 1, 2 and 3 together" % (len(log), len(steps), sizes, len(together)))
    for serial, pics in steps.items():
        counts = [p[1] for p in sorted(pics, key=lambda p: p[3])]
        assert counts == sorted(counts, reverse=True), "step %d: positions are not ordered by their reference counts: %s" % (serial, counts)
    assert together, "no step carried positions with one, two and three reference pictures (step sizes %s)" % sizes


def test_streams_of_different_reference_counts_side_by_side():
    """a refs = 3 and a refs = 1 stream of one size: both correct, on engines of their own; a stream opened with the flag and
    refs = 1 shares the plain stream's engine and gives the same bytes"""
    c3 = rm.BY_NAME["split_48x48"]
    want3, want1 = rm.expected(c3, 1), sr.expected_with_refs(c3, 1)
    s3, s1 = _stream(c3, 1), _stream(c3, 1, refs=1)
    flagged = None
    try:
        assert s3.hub_stats()["open_streams"] == 1 and s1.hub_stats()["open_streams"] == 1, "engines of their own"
        flagged = _stream(c3, 1, refs=1, flags=capi.STREAM_MULTIREF)
        assert s1.hub_stats()["open_streams"] == 2 and flagged.hub_stats()["open_streams"] == 2 and s3.hub_stats()["open_streams"] == 1
        for s in (s3, s1):
            s.keep_pre(True)
        for i, f in enumerate(rm.frames(c3)):
            for s, want, name in ((s3, want3, "refs 3"), (s1, want1, "refs 1"), (flagged, want1, "refs 1 with the flag")):
                au, ft = s.encode(f)
                tag = "%s picture %d" % (name, i)
                assert au == want[i].au and (ft == capi.FRAME_IDR) == want[i].idr, tag
                _compare_all(s, want[i].stages, tag)
        assert any(a.au != b.au for a, b in zip(want3, want1)), "the two reference counts code different streams"
        assert s3.hub_stats()["pictures"] == c3.pictures and s1.hub_stats()["pictures"] == 2 * c3.pictures
    finally:
        for s in (s3, s1, flagged):
            if s is not None:
                s.close()


def _plugin_run(contents, **kw):
    """one VideoEncoder object per content on a thread of its own; returns the access units per object"""
    c = contents[0]
    vc.set_video_mode(c.w, c.h, qp=c.qp, gop=c.gop, profile={66: "baseline", 77: "main", 100: "high"}[c.prof], slices=c.slices or None, **kw)
    vc.prop_set("persist.vmi.video.encode.scenedetect", "0")
    encs = []
    got = [[] for _ in contents]
    try:
        for _ in contents:
            e = vc.VideoEncoder()
            assert e.rc_create == vc.SUCCESS and e.init() == vc.SUCCESS and e.start() == vc.SUCCESS
            encs.append(e)

        def work(k):
            for f in rm.frames(contents[k]):
                got[k].append(encs[k].encode(f))

        ths = [threading.Thread(target=work, args=(k,)) for k in range(len(contents))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    finally:
        for e in encs:
            e.stop()
            e.destroy()
            e.delete()
        vc.prop_set("persist.vmi.video.encode.shared", "")
        vc.set_video_mode(c.w, c.h)
    for k in range(len(contents)):
        assert all(rc == vc.SUCCESS for rc, _ in got[k]), "object %d" % k
    return [[bs for _, bs in g] for g in got]


def test_plugin_objects_with_the_refs_key():
    """two VideoEncoder objects on two threads, persist.vmi.video.encode.refs = 3, fixed QP: every access unit is the oracle's
    with refs = 3, through the stream path and (persist.vmi.video.encode.shared = 0) through engines of their own; a junk value
    gives the one-reference stream"""
    a = rm.BY_NAME["split_96x80_high"]._replace(name="split_96x80_high_gop30", gop=30)     # (the plugin surface takes GOP lengths of 30 .. 3000)
    contents = (a, a._replace(name="split_96x80_high_gop30_b", seed=5, start=4))
    want = [[p.au for p in rm.expected(c, 1)] for c in contents]
    assert _plugin_run(contents, refs=3) == want, "stream path"
    vc.prop_set("persist.vmi.video.encode.shared", "0")
    assert _plugin_run(contents, refs=3) == want, "engines of their own"
    one = [[p.au for p in sr.expected_with_refs(c, 1)] for c in contents]
    assert one != want
    assert _plugin_run(contents, refs="three") == one, "a junk value: one reference picture"
