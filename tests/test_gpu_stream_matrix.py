"""The stream hub's indirect kernels (the IND = true instantiations: quantiser constants and filter thresholds by the item's own
QP, pictures addressed [item][ring slot], flags per item) across QP, content and size - run with -m gpu on an MI355X.

The case list is tests/stream_matrix.py (tests/test_stream_matrix_oracle.py proves its coverage on the oracle).  Picture by picture, every
stream of a group hands its picture in from a native thread of its own; the threads start together (tools/stream_tick.cpp: a
barrier per picture) under a long gather window (MI355X_H264_HUB_WINDOW_US, set before the group's engine exists), so that
pictures of different streams and QPs leave in one lockstep step.  Every picture is compared with the oracle coding the same pictures at the same QPs, stage by stage
(test_gpu_parity._compare_all on capi.Stream: access unit, MbInfo, levels, quadrant vectors, Intra4x4 modes, pre-filter and
final planes).  That pictures DID share steps is asserted from what the hub reports (Stream.last_step): a run in which they
did not fails."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import adversarial
import spec_pred
import stream_matrix as sm
from media_amd import capi
from oracle_lib import OracleDecoder
from test_gpu_parity import _compare_all, _to_nv12

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_US = "200000"     # a step that is being gathered waits this long for pictures still on their way in (default 200 us)


class Job(C.Structure):   # StreamTickJob of tools/stream_tick.cpp
    _fields_ = [("stream", C.c_void_p), ("pic", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32), ("device", C.c_int32), ("rc", C.c_int32),
                ("out", C.c_void_p), ("len", C.c_uint32), ("frame_type", C.c_int32)]


def build_tick(directory):
    """tools/stream_tick.cpp: one picture of every stream of a group handed in by native threads that start together (Python
    threads arrive an interpreter-lock hand-over apart, longer than a step of small pictures takes)"""
    so = os.path.join(str(directory), "libstream_tick.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-pthread", os.path.join(ROOT, "tools", "stream_tick.cpp"), "-o", so])
    L = C.CDLL(so)
    L.stream_tick.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Job), C.c_int]
    host = C.cast(capi.lib().mi355x_h264_stream_encode, C.c_void_p)
    dev = C.cast(capi.lib().mi355x_h264_stream_encode_device, C.c_void_p)

    def run(jobs):
        assert L.stream_tick(host, dev, jobs, len(jobs)) == 0, "the helper's threads could not be started"
    return run


@pytest.fixture(scope="module")
def tick(tmp_path_factory):
    return build_tick(tmp_path_factory.mktemp("stream_tick"))


def _open(s):
    return capi.Stream(s.w, s.h, qp=s.qps[0], gop=s.gop, profile_idc=s.prof, disable_deblock=s.nodeblock, slices=s.slices, search=s.search,
                       input_format=capi.INPUT_NV12 if s.nv12_device else capi.INPUT_I420)


class Run:
    """one stream of a group: the capi.Stream, its oracle, its pictures"""

    def __init__(self, k, s, first=0):
        self.k, self.s, self.first = k, s, first   # first: the group's picture at which this stream starts
        self.frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in sm.frames(s)]
        self.dev = None
        if s.nv12_device:
            import torch
            self.dev = torch.from_numpy(np.stack([_to_nv12(f, s.w, s.h) for f in self.frames])).cuda()
        self.stream = _open(s)
        self.stream.keep_pre(True)
        self.orc = sm.oracle_for(s)

    def job(self, i):
        """set what picture i needs set; the picture as a job of the helper"""
        s = self.s
        if i and s.qps[i] != s.qps[i - 1]:
            self.stream.set_qp(s.qps[i])
            self.orc.set_qp(s.qps[i])
        if i in s.force_idr_at:
            self.stream.force_idr()
        pic = self.dev[i].data_ptr() if self.dev is not None else self.frames[i].ctypes.data
        return Job(self.stream.h.value, pic, s.w, s.h, int(self.dev is not None), 0, None, 0, 0)

    def close(self):
        self.stream.close()
        self.orc.close()


def run_group(tick, monkeypatch, specs, per_picture=None, full=True, idle=0, ctx=None, swap=None):
    """open the group's streams (in list order: the batch items); picture by picture, hand every stream's picture to the hub at
    the same moment (the helper's threads) and then check every stream's picture against its oracle; per_picture(run, i, au, idr,
    tag) adds a test's own checks.  swap = (picture, stream index, Spec): before that picture the stream closes and a new one of
    that Spec opens in its place.  Returns the step log: one (stream index, picture, qp, idr, last_step) per picture"""
    monkeypatch.setenv("MI355X_H264_HUB_WINDOW_US", WINDOW_US)
    if ctx:
        monkeypatch.setenv("MI355X_H264_HUB_CTX", str(ctx))
    runs, spare, log = [], [], []
    try:
        for k, s in enumerate(specs):
            runs.append(Run(k, s))
        spare = [_open(specs[0]) for _ in range(idle)]
        npic = len(specs[0].qps)
        assert all(len(s.qps) == npic for s in specs)
        for i in range(npic):
            if swap and swap[0] == i:
                runs[swap[1]].close()
                runs[swap[1]] = Run(swap[1], swap[2], first=i)
            jobs = (Job * len(runs))(*[r.job(i - r.first) for r in runs])
            tick(jobs)
            for r, job in zip(runs, jobs):
                j = i - r.first
                r.stream._check(job.rc)
                au, ft, step = C.string_at(job.out, job.len), job.frame_type, r.stream.last_step()
                want, idr = r.orc.encode(r.frames[j], force_idr=j in r.s.force_idr_at)
                tag = "stream %d (%s %dx%d profile %d) picture %d qp %d step %s" % (r.k, r.s.kind, r.s.w, r.s.h, r.s.prof, j, r.s.qps[j], step)
                assert (ft == capi.FRAME_IDR) == idr and step["idr"] == idr, tag + ": picture type"
                assert au == want, tag + ": access unit differs from the oracle's"
                if full:
                    _compare_all(r.stream, r.orc, tag)
                else:
                    for p in range(3):
                        assert np.array_equal(r.stream.debug_read(capi.DBG_RECON_Y + p), r.orc.recon(p)), "%s: recon plane %d" % (tag, p)
                if per_picture:
                    per_picture(r, j, au, idr, tag)
                log.append((r.k, i, r.s.qps[j], idr, step))
    finally:
        for r in runs:
            r.close()
        for s in spare:
            s.close()
    return log


def steps_of(log):
    """{step serial: [(stream index, qp, idr, position)]}, after checking that the reported facts agree with each other: every
    picture of a step reports the step's size, and the positions are 0 .. size - 1, each once"""
    steps = {}
    for k, i, qp, idr, st in log:
        steps.setdefault(st["serial"], []).append((k, qp, idr, st["position"], st["pictures"]))
    for serial, pics in steps.items():
        assert serial > 0 and len({p[4] for p in pics}) == 1 and len({p[2] for p in pics}) == 1, (serial, pics)
        assert sorted(p[3] for p in pics) == list(range(pics[0][4])), "step %d: %s" % (serial, pics)
    return steps


def mixed(steps, idr=None):
    """the steps in which pictures of different QPs were coded together (idr: only IDR / only P steps)"""
    return [pics for pics in steps.values() if len({p[1] for p in pics}) >= 2 and (idr is None or pics[0][2] == idr)]


def assert_mixed(log, what):
    steps = steps_of(log)
    sizes = sorted(len(p) for p in steps.values())
    print("%s: %d pictures in %d steps, %d of them with two QPs or more; step sizes %s" % (what, len(log), len(steps), len(mixed(steps)), sizes))
    assert mixed(steps, idr=False), "%s: no P step held pictures of two QPs (step sizes %s)" % (what, sizes)
    assert mixed(steps, idr=True), "%s: no IDR step held pictures of two QPs (step sizes %s)" % (what, sizes)
    return steps


@pytest.mark.parametrize("prof", [66, 100])
def test_every_qp_beside_the_others_in_shared_steps(tick, monkeypatch, prof):
    """21 streams at QPs 10, 12 .. 50, shifted by one, at the range ends and walking 10 -> 51 -> 10 inside a GOP, a different
    content each; Baseline (k_tq) and High (k_tq8)"""
    log = run_group(tick, monkeypatch, sm.all_qps(prof))
    steps = assert_mixed(log, "profile %d" % prof)
    assert any({10, 51} <= {p[1] for p in pics} for pics in steps.values()), "QP 10 and QP 51 never shared a step"
    in_mixed = {p[1] for pics in mixed(steps) for p in pics}
    print("QPs coded beside another QP: %d of 42" % len(in_mixed))
    assert len(in_mixed) >= 30, "only QPs %s were coded beside another QP" % sorted(in_mixed)


def test_saturation_matrix_through_streams(tick, monkeypatch):
    """every adversarial content at QP 10 and 51 as twelve streams of one engine, Baseline then High: beyond the stage comparison,
    the independent decoder reproduces the GPU's reconstruction and the GPU's own pre-filter planes hold the prediction restated
    from the standard, the references being the GPU's previous reconstructions.  The floors (stream_matrix.FLOORS: the oracle's
    counts on this list less a tenth) are asserted on what the GPU coded"""
    total = {}
    for prof in sm.SAT_PROFILES:
        state = {}

        def check(r, i, au, idr, tag):
            st = state.setdefault(r.k, {"dec": OracleDecoder(), "history": [], "cov": {}})
            dec, enc, s, cov = st["dec"], r.stream, r.s, st["cov"]
            assert dec.decode(au) == 1, tag
            recon = tuple(enc.debug_read(capi.DBG_RECON_Y + p) for p in range(3))
            for p in range(3):
                assert np.array_equal(dec.plane(p), recon[p]), "%s: decoder plane %d differs from the GPU reconstruction" % (tag, p)
            assert dec.max_mb_bits <= 3200 and dec.max_level_prefix <= 15, tag
            if idr:
                st["history"] = []
            mbinfo = enc.debug_read(capi.DBG_MBINFO)
            before = dict(cov)
            spec_pred.check_picture([enc.debug_read(capi.DBG_PRE_Y + p) for p in range(3)], st["history"],
                                    spec_pred.coded_planes(r.frames[i], s.w, s.h, enc.cw, enc.ch), mbinfo, enc.debug_read(capi.DBG_MVQ),
                                    enc.debug_read(capi.DBG_MBAUX), enc.debug_read(capi.DBG_LEVELS), adversarial.slice_rows(enc.ch // 16, s.slices),
                                    tag=tag + " (GPU)", counters=cov)
            sm.tally(cov, s.qps[i], mbinfo, dec.max_level_prefix, before)
            st["history"] = [recon]

        specs = sm.saturation(prof)
        log = run_group(tick, monkeypatch, specs, per_picture=check)
        assert mixed(steps_of(log), idr=False), "profile %d: no P step held a QP 10 picture beside a QP 51 picture" % prof
        for k, st in state.items():
            st["dec"].close()
            tot = total.setdefault(specs[k].kind, {})
            for key, v in st["cov"].items():
                tot[key] = tot.get(key, 0) + v
    for kind in adversarial.GENERATORS:
        short = sm.short_of_floors(kind, total[kind])
        assert not short, "%s: coverage below its floor: %s (counts %s)" % (kind, ", ".join(short), total[kind])


@pytest.mark.parametrize("order", sm.FLAGS_ORDERS)
def test_per_item_flags_beside_each_other(tick, monkeypatch, order):
    """I_PCM pictures (slice header idc 1, not filtered), all-skip pictures and P pictures with intra macroblocks in ONE step: the
    anypcm / anyintra flags are the item's, not the position's.  Three idle streams and one P context make the P share five of
    the six pictures, so whichever five a step takes hold all three kinds; the opening order moves the kinds over the items"""
    specs = sm.flags(order)

    def check(r, i, au, idr, tag):
        pre_eq = all(np.array_equal(r.stream.debug_read(capi.DBG_PRE_Y + p), r.stream.debug_read(capi.DBG_RECON_Y + p)) for p in range(3))
        want_eq = all(np.array_equal(r.orc.recon_pre(p), r.orc.recon(p)) for p in range(3))
        assert pre_eq == want_eq, tag + ": filtered where the oracle is not (or the reverse)"
        if r.s.kind == "noise":
            assert pre_eq, tag + ": an I_PCM picture was filtered"
        if r.s.kind == "flip":
            assert not pre_eq, tag + ": a picture with intra macroblocks was not filtered"

    log = run_group(tick, monkeypatch, specs, per_picture=check, idle=sm.FLAGS_IDLE, ctx=1)
    steps = steps_of(log)
    kinds = [{specs[p[0]].kind for p in pics} for pics in steps.values() if not pics[0][2]]
    assert any(k == {"noise", "s2", "flip"} for k in kinds), "no P step held an I_PCM, an all-skip and an intra picture together: %s" % kinds


def test_geometry_sweep(tick, monkeypatch):
    """one macroblock, one row, one column, crops, odd macroblock counts, wide and flat, then 24 seeded random even sizes: three
    streams each; loop filter on / off, both searches, one slice / three, I420 from the host / NV12 read in place from device memory"""
    groups, with_mixed = sm.geometry(), 0
    for group in groups:
        steps = steps_of(run_group(tick, monkeypatch, group, ctx=1))   # one P context: the P share of three streams is two pictures
        with_mixed += bool(mixed(steps))
    # the sweep is about geometry, and three streams seldom fill a step; still, most groups must have coded pictures of two
    # QPs in one launch somewhere in their twelve pictures (their streams' QPs differ in all but a few groups)
    assert 2 * with_mixed >= len(groups), "only %d of %d groups had a step with pictures of two QPs" % (with_mixed, len(groups))


@pytest.mark.parametrize("w,h", sm.FILTER_FORM_SIZES)
def test_both_loop_filter_forms_indirect(tick, monkeypatch, w, h):
    """steps of eight pictures or more take k_deblock_pairs<.., true>, smaller ones k_deblock_rows<.., true>: thirty streams make
    both, in IDR and in P steps"""
    log = run_group(tick, monkeypatch, sm.filter_forms(w, h))
    steps = assert_mixed(log, "%dx%d" % (w, h))
    for idr in (True, False):
        sizes = sorted(len(p) for p in steps.values() if p[0][2] == idr)
        assert sizes[-1] >= 8, "%s steps of %s pictures: none of eight or more" % ("IDR" if idr else "P", sizes)
    assert min(len(p) for p in steps.values()) < 8, "no step below eight pictures (the row form)"


def test_forced_idr_and_stream_churn_under_load(tick, monkeypatch):
    """force_idr on one stream while four others go on; then, between two pictures of the run, a stream closes and another opens
    on the freed item (the engine and the others' reference pictures stay): its
    first picture is an IDR picture equal to a fresh oracle's, the neighbours are unaffected; me_cost on every picture"""
    first = {}

    def check(r, i, au, idr, tag):
        assert r.stream.me_cost() == r.orc.me_cost(), tag + ": me_cost"
        if r.s is sm.CHURN_NEWCOMER and i == 0:
            first["idr"] = idr
            assert r.stream.hub_stats()["open_streams"] == len(sm.churn()), "the newcomer took the freed item of the same engine"
        if r.k == 1 and i == 3:
            assert idr, tag + ": forced IDR"

    log = run_group(tick, monkeypatch, sm.churn(), per_picture=check, swap=(sm.CHURN_CLOSE_AT, sm.CHURN_CLOSE_STREAM, sm.CHURN_NEWCOMER))
    assert first.get("idr") is True, "the newcomer's first picture is an IDR picture"
    steps = steps_of(log)
    assert mixed(steps), "no step held pictures of two QPs"
    forced = [st for k, i, qp, idr, st in log if k == 1 and i == 3][0]
    others = [st for k, i, qp, idr, st in log if k != 1 and i == 3]
    assert forced["idr"] and not any(st["idr"] for st in others), "the forced IDR picture left in a step of its own type while the others coded P pictures"


def test_four_streams_at_1080p(tick, monkeypatch):
    """full size once: bytes and final planes"""
    log = run_group(tick, monkeypatch, sm.full_size(), full=False)
    assert mixed(steps_of(log)), "no step held pictures of two QPs"
