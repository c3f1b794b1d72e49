"""Damage tiles on the GPU (include/mi355x_h264.h, "damage tiles"; media_amd/csrc/damage.h, k_patch.h, hub.h): a host call that
transfers only the tiles that changed, one patch launch per step.  Everything is an equality: the staging picture after every call
is the restated composition (tests/damage.py), every access unit and the final planes are the oracle's for that composition and -
where the damage set is complete - those of the same stream driven by the ordinary call, and last_upload is the restated byte count
and mode.  The cases and what they hold: tests/damage.py, tests/test_damage_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import damage as dm
import mem_guard as mg
import scale
from media_amd import capi
from media_amd import videocodec as vc
from oracle_lib import OracleEncoder, rgba_to_i420

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = [dm.I420, dm.NV12, dm.RGBA]
FMT_IDS = {dm.I420: "i420", dm.NV12: "nv12", dm.RGBA: "rgba"}
WINDOW_US = "200000"


def as_i420(fmt, pic, w, h):
    """the I420 picture the encoder codes for a picture in the layout (RGBA: the oracle's own conversion)"""
    if fmt == dm.I420:
        return pic
    if fmt == dm.NV12:
        return dm.nv12_to_i420(pic, w, h)
    return rgba_to_i420(pic.reshape(h, w, 4), w, h)


def staged(fmt, pic, w, h):
    """what debug_read(DBG_SRC) gives for it: the slot itself (I420, NV12) or the conversion's result (RGBA)"""
    return rgba_to_i420(pic.reshape(h, w, 4), w, h) if fmt == dm.RGBA else pic


def call(s, fmt, pic, w, h, damage=None):
    if fmt == dm.I420:
        return s.encode(pic, damage=damage)
    if fmt == dm.NV12:
        return s.encode_nv12(pic, damage=damage)
    return s.encode_rgba(pic.reshape(h, w, 4), damage=damage)


def run_case(case, fmt, ordinary_twin=True):
    w, h = case.w, case.h
    s = capi.Stream(w, h, qp=27, gop=case.gop, input_format=fmt)
    twin = capi.Stream(w, h, qp=27, gop=case.gop, input_format=fmt) if ordinary_twin else None   # the same stream, ordinary calls
    orc = OracleEncoder(w, h, qp=27, gop=case.gop)
    idrs = 0
    try:
        before = s.patch_stats()
        patched = tiles_patched = 0
        for i, (caller, arg, tiles, enc, up) in enumerate(dm.run_case(case, fmt)):
            tag = "%s %s picture %d (%s)" % (case.name, FMT_IDS[fmt], i, up["mode"])
            au, ft = call(s, fmt, caller, w, h, damage=arg)
            assert s.last_upload == up, tag
            assert np.array_equal(s.debug_read(capi.DBG_SRC), staged(fmt, enc, w, h)), tag + ": staging picture"
            want, idr = orc.encode(as_i420(fmt, enc, w, h))
            idrs += idr
            assert au == want and (ft == capi.FRAME_IDR) == idr, tag + ": access unit"
            if twin is not None:
                # (the composition handed over whole: with a complete damage set that is the caller's picture itself)
                assert call(twin, fmt, enc, w, h)[0] == au, tag + ": the ordinary call's access unit"
                assert twin.last_upload == dm.upload(fmt, w, h, 0, valid=False), tag
            patched += up["mode"] == "patched"
            tiles_patched += up["tiles"] if up["mode"] == "patched" else 0
        for p in range(3):
            assert np.array_equal(s.recon(p), orc.recon(p)), "%s: final plane %d" % (case.name, p)
        after = s.patch_stats()
        # one patch launch per patched picture (a stream alone: a step per picture), none for whole pictures and for nothing
        assert (after["launches"] - before["launches"], after["tiles"] - before["tiles"]) == (patched, tiles_patched)
        assert idrs >= 2, "an IDR picture inside the run"
    finally:
        s.close()
        if twin is not None:
            twin.close()
        orc.close()


@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: FMT_IDS[f])
@pytest.mark.parametrize("case", dm.CASES, ids=lambda c: c.name)
def test_gop_per_size_and_layout(case, fmt):
    run_case(case, fmt)


def test_1080p_pair_bottom_tiles_are_half_height():
    w, h, fmt = 1920, 1080, dm.I420
    ntx, nty = dm.grid(w, h)
    assert (ntx, nty) == (30, 68)
    a = dm.content(fmt, w, h, 1)
    b = a.copy()
    m = dm.rect_mask(fmt, w, h, [(1900, 1075, 20, 5), (100, 496, 200, 64), (0, 1079, 1920, 1)])
    b[m] += 77
    tiles = dm.detect_tiles(fmt, w, h, a, b)
    assert set(range(67 * 30, 68 * 30)) <= tiles and len(tiles) == 30 + 4 * 4   # the half-height bottom row and a 4 x 4 block
    s, twin, orc = capi.Stream(w, h, qp=30, gop=30), capi.Stream(w, h, qp=30, gop=30), OracleEncoder(w, h, qp=30, gop=30)
    try:
        assert s.encode(a, damage="detect")[0] == orc.encode(a)[0] == twin.encode(a)[0]
        assert s.last_upload == dm.upload(fmt, w, h, 0, valid=False)
        au = s.encode(b, damage="detect")[0]
        assert s.last_upload == dm.upload(fmt, w, h, len(tiles)) and s.last_upload["mode"] == "patched"
        assert np.array_equal(s.debug_read(capi.DBG_SRC), b)
        assert au == orc.encode(b)[0] and au == twin.encode(b)[0]
        for p in range(3):
            assert np.array_equal(s.recon(p), orc.recon(p))
    finally:
        s.close()
        twin.close()
        orc.close()


def test_validity_first_call_device_call_and_refusals():
    import torch
    w, h, fmt = 66, 34, dm.I420
    pics = [dm.content(fmt, w, h, 70 + i) for i in range(3)]
    one = [dm.tile_rect(w, h, 2)]
    s, orc = capi.Stream(w, h, qp=28, gop=30), OracleEncoder(w, h, qp=28, gop=30)
    whole = dm.upload(fmt, w, h, 0, valid=False)
    try:
        assert s.last_upload == {"bytes": 0, "tiles": 0, "tiles_total": 6, "mode": "whole"}
        # a first call with damage goes whole, whatever it says: the caller's picture is encoded
        assert s.encode(pics[0], damage=[])[0] == orc.encode(pics[0])[0] and s.last_upload == whole
        assert np.array_equal(s.debug_read(capi.DBG_SRC), pics[0])
        # now the slot is valid: one tile of pics[1]
        enc = dm.compose(fmt, w, h, pics[0], pics[1], {2})
        assert s.encode(pics[1], damage=one)[0] == orc.encode(enc)[0] and s.last_upload == dm.upload(fmt, w, h, 1)
        assert np.array_equal(s.debug_read(capi.DBG_SRC), enc)
        # a device-form call in between: the next damage call goes whole
        dev = torch.from_numpy(pics[2]).cuda()
        torch.cuda.synchronize()
        assert s.encode_device(dev.data_ptr())[0] == orc.encode(pics[2])[0]
        assert s.last_upload == {"bytes": 0, "tiles": 0, "tiles_total": 6, "mode": "in_place"}
        assert s.encode(pics[0], damage=one)[0] == orc.encode(pics[0])[0] and s.last_upload == whole
        assert np.array_equal(s.debug_read(capi.DBG_SRC), pics[0])
        # refused calls change nothing: not the report, not the slot, not its validity, not the stream's state
        L = capi.lib()
        out, n, ft = C.c_void_p(), C.c_uint32(), C.c_int()
        y, u, v = pics[1].ctypes.data, pics[1].ctypes.data + w * h, pics[1].ctypes.data + w * h * 5 // 4
        good, neg_w, neg_h = capi.Rect(0, 0, 8, 8), capi.Rect(0, 0, -1, 8), capi.Rect(0, 0, 8, -3)
        tail = (C.byref(out), C.byref(n), C.byref(ft))
        for rects, cnt in ((C.byref(good), -1), (None, 1), (C.byref(neg_w), 1), (C.byref(neg_h), 1), (C.byref(good), capi.DAMAGE_DETECT), (C.byref(good), -7)):
            assert L.mi355x_h264_stream_encode_damage(s.h, y, w, u, w // 2, v, w // 2, rects, cnt, *tail) == capi.E_ARG
            assert s.last_error() != "" and s.last_upload == whole
        assert L.mi355x_h264_stream_encode_damage(s.h, y, w - 2, u, w // 2, v, w // 2, None, 0, *tail) == capi.E_ARG   # stride < width
        assert np.array_equal(s.debug_read(capi.DBG_SRC), pics[0])
        enc = dm.compose(fmt, w, h, pics[0], pics[1], {2})
        assert s.encode(pics[1], damage=one)[0] == orc.encode(enc)[0] and s.last_upload == dm.upload(fmt, w, h, 1)
        assert s.encode(pics[1], damage="detect")[0] == orc.encode(pics[1])[0]
        assert s.last_upload == dm.upload(fmt, w, h, 5) and s.last_upload["mode"] == "whole"   # the five other tiles: over the boundary
        assert np.array_equal(s.debug_read(capi.DBG_SRC), pics[1])
    finally:
        s.close()
        orc.close()


@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: FMT_IDS[f])
def test_fallback_one_tile_under_goes_patched_one_over_goes_whole(fmt):
    w, h = 128, 48
    n = dm.most_patched_tiles(fmt, w, h)
    assert 0 < n < 6
    a, b = dm.content(fmt, w, h, 5), dm.content(fmt, w, h, 6)
    res = {}
    for k in (n, n + 1):
        s, orc = capi.Stream(w, h, qp=26, gop=30, input_format=fmt), OracleEncoder(w, h, qp=26, gop=30)
        try:
            call(s, fmt, a, w, h, damage="detect")
            orc.encode(as_i420(fmt, a, w, h))
            enc = dm.compose(fmt, w, h, a, b, set(range(k)))
            au = call(s, fmt, enc, w, h, damage=[dm.tile_rect(w, h, t) for t in range(k)])[0]
            assert s.last_upload == dm.upload(fmt, w, h, k) and s.last_upload["mode"] == ("patched" if k == n else "whole")
            assert np.array_equal(s.debug_read(capi.DBG_SRC), staged(fmt, enc, w, h))
            assert au == orc.encode(as_i420(fmt, enc, w, h))[0]
            res[k] = au
        finally:
            s.close()
            orc.close()
    # one tile under and one over, the SAME picture both ways: tile n unchanged in it, said or not
    s1, s2 = capi.Stream(w, h, qp=26, gop=30, input_format=fmt), capi.Stream(w, h, qp=26, gop=30, input_format=fmt)
    try:
        enc = dm.compose(fmt, w, h, a, b, set(range(n)))
        call(s1, fmt, a, w, h)
        call(s2, fmt, a, w, h)
        au1 = call(s1, fmt, enc, w, h, damage=[dm.tile_rect(w, h, t) for t in range(n)])[0]
        au2 = call(s2, fmt, enc, w, h, damage=[dm.tile_rect(w, h, t) for t in range(n + 1)])[0]
        assert (s1.last_upload["mode"], s2.last_upload["mode"]) == ("patched", "whole")
        assert s2.last_upload["bytes"] == dm.picture_bytes(fmt, w, h) > s1.last_upload["bytes"] == dm.payload_bytes(fmt, n)
        assert au1 == au2 == res[n], "the bytes are the same either way"
    finally:
        s1.close()
        s2.close()


class Job(C.Structure):   # DamageTickJob of tools/damage_tick.cpp
    _fields_ = [("stream", C.c_void_p), ("pic", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32), ("mode", C.c_int32), ("n_rects", C.c_int32),
                ("rects", C.c_void_p), ("rc", C.c_int32), ("out", C.c_void_p), ("len", C.c_uint32), ("frame_type", C.c_int32)]


@pytest.fixture(scope="module")
def tick(tmp_path_factory):
    """tools/damage_tick.cpp: one picture of every stream handed in by native threads that start together"""
    so = os.path.join(str(tmp_path_factory.mktemp("damage_tick")), "libdamage_tick.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-pthread", os.path.join(ROOT, "tools", "damage_tick.cpp"), "-o", so])
    L = C.CDLL(so)
    L.damage_tick.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Job), C.c_int]
    host = C.cast(capi.lib().mi355x_h264_stream_encode, C.c_void_p)
    dmg = C.cast(capi.lib().mi355x_h264_stream_encode_damage, C.c_void_p)

    def run(jobs):
        assert L.damage_tick(host, dmg, jobs, len(jobs)) == 0, "the helper's threads could not be started"
    return run


def test_six_streams_share_steps_and_patch_launches(tick, monkeypatch):
    """six streams of one engine, handed in together: an ordinary call, three pictures patched by rectangles, one found by
    comparing, one with nothing (three patched pictures of 1, 12 and 20 tiles).  One patch launch per step that holds a patched picture, however many it holds; every stream gets
    its own expected bytes; then a tick in which no stream has tiles: no launch."""
    monkeypatch.setenv("MI355X_H264_HUB_WINDOW_US", WINDOW_US)
    monkeypatch.setenv("MI355X_H264_HUB_CTX", "1")
    w, h, fmt, n = 320, 240, dm.I420, 6
    ntx, nty = dm.grid(w, h)
    says = [None, [dm.tile_rect(w, h, 8)], [(60, 30, 70, 50)], [], "detect", [(0, 96, 320, 64)]]
    assert [len(dm.rect_tiles(w, h, r)) if isinstance(r, list) else None for r in says] == [None, 1, 12, 0, None, 20]
    streams = [capi.Stream(w, h, qp=24 + k, gop=30) for k in range(n)]
    orcs = [OracleEncoder(w, h, qp=24 + k, gop=30) for k in range(n)]
    slots = [None] * n
    both = mixed = 0
    try:
        assert streams[0].hub_stats()["open_streams"] == n
        for i in range(5):
            quiet = i == 4                                     # the last tick: nobody has tiles (ordinary calls and "nothing changed")
            pics, args, keep = [], [], []
            for k in range(n):
                fresh = dm.content(fmt, w, h, 200 + 10 * k + i)
                if says[k] == "detect" and slots[k] is not None:   # a picture that differs from the last one in a few tiles only
                    m = dm.rect_mask(fmt, w, h, [(30 * i, 20 * i, 40, 30)])
                    fresh = np.where(m, fresh, slots[k]).astype(np.uint8)
                pics.append(fresh)
                args.append(None if says[k] is None or (quiet and k % 2 == 0) else [] if quiet else says[k])
            launches0 = streams[0].patch_stats()["launches"]
            jobs = []
            for k in range(n):
                if args[k] is None:
                    jobs.append(Job(streams[k].h.value, pics[k].ctypes.data, w, h, 0, 0, None, 0, None, 0, 0))
                else:
                    rects, nr, alive = capi._damage_args(args[k])
                    keep.append(alive)
                    jobs.append(Job(streams[k].h.value, pics[k].ctypes.data, w, h, 1, nr, C.cast(rects, C.c_void_p) if rects is not None else None, 0, None, 0, 0))
            jobs = (Job * n)(*jobs)
            tick(jobs)
            steps = {}
            for k in range(n):
                tag = "stream %d tick %d" % (k, i)
                assert jobs[k].rc == 0, tag + ": " + streams[k].last_error()
                if slots[k] is None or args[k] is None:
                    enc, up = pics[k], dm.upload(fmt, w, h, 0, valid=False)
                else:
                    tiles = dm.detect_tiles(fmt, w, h, slots[k], pics[k]) if args[k] == "detect" else dm.rect_tiles(w, h, args[k])
                    enc, up = dm.compose(fmt, w, h, slots[k], pics[k], tiles), dm.upload(fmt, w, h, len(tiles))
                slots[k] = enc
                assert streams[k].last_upload == up, tag
                assert np.array_equal(streams[k].debug_read(capi.DBG_SRC), enc), tag + ": staging picture"
                assert C.string_at(jobs[k].out, jobs[k].len) == orcs[k].encode(enc)[0], tag
                step = streams[k].last_step()
                steps.setdefault(step["serial"], []).append((up["mode"], up["tiles"], step["pictures"]))
            for serial, held in steps.items():
                assert len(held) == held[0][2], "every picture of step %d is one of this tick's" % serial
            with_patch = [held for held in steps.values() if any(m == "patched" for m, _, _ in held)]
            assert streams[0].patch_stats()["launches"] - launches0 == len(with_patch), "tick %d: one patch launch per step that has tiles" % i
            if quiet:
                assert not with_patch
            both += sum(1 for held in with_patch if len({t for m, t, _ in held if m == "patched"}) >= 2)
            mixed += sum(1 for held in with_patch if {m for m, _, _ in held} - {"patched"})
        assert both >= 1, "no step carried two patched pictures of different tile counts"
        assert mixed >= 1, "no step carried a patched picture beside a whole one or one with nothing"
        st = streams[0].hub_stats()
        assert st["pictures"] == n * 5 and st["steps"] < st["pictures"]
    finally:
        for x in streams + orcs:
            x.close()


def test_scaled_stream_takes_the_grid_of_the_source_size():
    sw, sh, w, h, fmt = 96, 64, 64, 48, dm.I420
    assert dm.grid(sw, sh) == (2, 4) and dm.grid(w, h) == (1, 3)
    s, orc = capi.Stream(w, h, qp=30, gop=30, src_size=(sw, sh)), OracleEncoder(w, h, qp=30, gop=30)
    try:
        slot = None
        for i, arg in enumerate(["detect", [(70, 20, 10, 10)], "detect", [], [(0, 0, 96, 64)], [(64, 48, 32, 16)]]):
            pic = dm.content(fmt, sw, sh, 300 + i)
            if i == 2:
                pic = np.where(dm.rect_mask(fmt, sw, sh, [(10, 50, 60, 4)]), pic, slot).astype(np.uint8)
            if slot is None:
                enc, up = pic, dm.upload(fmt, sw, sh, 0, valid=False)
            else:
                tiles = dm.detect_tiles(fmt, sw, sh, slot, pic) if arg == "detect" else dm.rect_tiles(sw, sh, arg)
                enc, up = dm.compose(fmt, sw, sh, slot, pic, tiles), dm.upload(fmt, sw, sh, len(tiles))
            slot = enc
            au = s.encode(pic, damage=arg)[0]
            assert s.last_upload == up and up["tiles_total"] == 8, "picture %d" % i
            small = scale.scale_i420(enc, sw, sh, w, h)
            assert np.array_equal(s.debug_read(capi.DBG_SRC), small), "picture %d: the resampled composition" % i
            assert au == orc.encode(small)[0], "picture %d" % i
        assert {"patched", "nothing", "whole"} <= {dm.upload(fmt, sw, sh, k)["mode"] for k in (0, 1, 2, 8)}
    finally:
        s.close()
        orc.close()


@pytest.mark.parametrize("kind", ["refs3", "temporal", "quality_ssim", "refresh"])
def test_other_stream_kinds_equal_the_ordinary_call(kind):
    """a stream of another kind driven by damage calls equals the same stream driven by ordinary calls in every byte it gives:
    access units, planes, layer / band, quality and SSIM records (none of them sees anything but the slot)"""
    w, h, fmt = 128, 160, dm.I420
    kw = {"refs3": dict(refs=3, gop=30), "temporal": dict(temporal_layers=2, gop=8), "quality_ssim": dict(gop=4),
          "refresh": dict(slices=5, intra_refresh=True, gop=30)}[kind]
    a, b = capi.Stream(w, h, qp=29, **kw), capi.Stream(w, h, qp=29, **kw)
    try:
        if kind == "quality_ssim":
            a.quality_enable(True, ssim=True)
        slot = None
        modes = set()
        for i in range(9):
            pic = dm.content(fmt, w, h, 400 + i)
            if slot is not None and i % 3:
                pic = np.where(dm.rect_mask(fmt, w, h, [(20 * i, 9 * i, 50, 20)]), pic, slot).astype(np.uint8)
            if i == 5:
                a.force_idr()
                b.force_idr()
            if i == 6:
                a.set_qp(35)
                b.set_qp(35)
            arg = "detect" if i != 4 else []
            enc = pic if (slot is None or arg == "detect") else slot
            au, ft = a.encode(pic, damage=arg)
            modes.add(a.last_upload["mode"])
            assert (au, ft) == b.encode(enc), "picture %d" % i
            assert np.array_equal(a.debug_read(capi.DBG_SRC), enc)
            assert a.last_temporal_id == b.last_temporal_id and a.last_refresh_band == b.last_refresh_band
            if kind == "quality_ssim":
                qa, qb = a.quality(), b.quality()
                assert qa == qb and qa["valid"] and "ssim" in qa, "picture %d" % i
                assert np.array_equal(a.quality_map(), b.quality_map()) and np.array_equal(a.ssim_map(), b.ssim_map())
            for p in range(3):
                assert np.array_equal(a.recon(p), b.recon(p)), "picture %d plane %d" % (i, p)
            slot = enc
        assert modes == {"whole", "patched", "nothing"}
    finally:
        a.close()
        b.close()


def test_guard_mode_partial_tiles_store_nothing_outside_the_slot(monkeypatch):
    """262144-byte guards, poison on, over the sizes whose tiles are partial.  One stream per engine (MI355X_H264_HUB_ITEMS = 1), so
    that the stream's slot ends where its block ends: a partial tile stored at full size lands in a guard"""
    monkeypatch.setenv("MI355X_H264_HUB_ITEMS", "1")
    with mg.guarded() as seen:
        for name in ("tiny_34x18", "tall_34x66", "edge_66x34"):
            for fmt in FMTS:
                run_case(dm.BY_NAME[name], fmt, ordinary_twin=False)
    assert len(seen) == 9
    for kind, damaged, regions, lines in seen:
        assert kind == "stream" and damaged == 0, lines
        blocks, slack = mg.header(lines)
        assert regions == 2 * blocks + slack and blocks >= 10, lines[0]
    assert capi.mem_tally() == seen.tally_before


def _plugin(w, h, **kw):
    vc.set_video_mode(w, h, **kw)
    e = vc.VideoEncoder()
    assert e.rc_create == vc.SUCCESS
    assert e.init() == vc.SUCCESS and e.start() == vc.SUCCESS
    return e


@pytest.mark.parametrize("fmtname", ["i420", "nv12", "rgba"])
def test_plugin_detect_gives_the_bytes_of_off_on_both_paths(fmtname):
    w, h = 176, 144
    fmt = {"i420": dm.I420, "nv12": dm.NV12, "rgba": dm.RGBA}[fmtname]
    pics = [dm.content(fmt, w, h, 500)]
    for i in range(1, 7):
        nxt = dm.content(fmt, w, h, 500 + i)
        pics.append(pics[-1] if i == 3 else np.where(dm.rect_mask(fmt, w, h, [(15 * i, 10 * i, 60, 30)]), nxt, pics[-1]).astype(np.uint8))
    outs = {}
    try:
        for shared in ("1", "0"):
            for damage in ("off", "detect"):
                e = _plugin(w, h, qp=28, gop=4, input=None if fmt == dm.I420 else fmtname, shared=shared, damage=damage)
                got, ups = [], []
                for p in pics:
                    rc, au = e.encode(p)
                    assert rc == vc.SUCCESS
                    got.append(au)
                    ups.append(e.last_upload())
                outs[(shared, damage)] = got
                if shared == "1":
                    modes = [u["mode"] for u in ups]
                    assert modes == (["whole"] * 7 if damage == "off" else ["whole", "patched", "patched", "nothing", "patched", "patched", "patched"]), modes
                    if damage == "detect":
                        for i in range(1, 7):
                            assert ups[i] == dm.upload(fmt, w, h, len(dm.detect_tiles(fmt, w, h, pics[i - 1], pics[i]))), i
                else:
                    assert ups == [None] * 7   # an engine of its own: whole pictures, nothing to report
                e.destroy()
                assert e.delete() == vc.SUCCESS
        assert outs[("1", "off")] == outs[("1", "detect")] == outs[("0", "off")] == outs[("0", "detect")]
        assert vc.prop_get("persist.vmi.video.encode.damage") == "detect"
        # junk in the key: whole pictures, "off" written back
        e = _plugin(w, h, qp=28, gop=4, input=None if fmt == dm.I420 else fmtname, shared="1", damage="sometimes")
        assert vc.prop_get("persist.vmi.video.encode.damage") == "off"
        assert [e.encode(p)[1] for p in pics[:3]] == outs[("1", "off")][:3] and e.last_upload()["mode"] == "whole"
        e.destroy()
        assert e.delete() == vc.SUCCESS
    finally:
        vc.set_video_mode(w, h)
        vc.prop_set("persist.vmi.video.encode.shared", "")


def test_plugin_set_next_damage_is_honoured():
    w, h, fmt = 176, 144, dm.I420
    a, b, c = (dm.content(fmt, w, h, 600 + i) for i in range(3))
    rects = [(70, 20, 20, 20), (0, 140, 10, 4)]
    tiles = dm.rect_tiles(w, h, rects)
    orc = OracleEncoder(w, h, qp=28, gop=30)
    try:
        vc.set_video_mode(w, h, qp=28, gop=30, shared="1")
        vc.prop_set("persist.vmi.video.encode.scenedetect", "0")   # (whole new pictures follow each other: no re-code as IDR)
        e = vc.VideoEncoder()
        assert e.rc_create == vc.SUCCESS and e.init() == vc.SUCCESS and e.start() == vc.SUCCESS
        assert e.encode(a) == (vc.SUCCESS, orc.encode(a)[0])
        assert e.set_next_damage(rects)
        enc = dm.compose(fmt, w, h, a, b, tiles)
        assert e.encode(b) == (vc.SUCCESS, orc.encode(enc)[0]) and e.last_upload() == dm.upload(fmt, w, h, len(tiles))
        # it held for that picture alone: the next one goes whole (the key is off)
        assert e.encode(c) == (vc.SUCCESS, orc.encode(c)[0]) and e.last_upload()["mode"] == "whole"
        assert e.set_next_damage([])
        assert e.encode(a) == (vc.SUCCESS, orc.encode(c)[0]) and e.last_upload() == dm.upload(fmt, w, h, 0)   # "nothing changed": c again
        e.destroy()
        assert e.delete() == vc.SUCCESS
    finally:
        orc.close()
        vc.set_video_mode(w, h)
        vc.prop_set("persist.vmi.video.encode.shared", "")
