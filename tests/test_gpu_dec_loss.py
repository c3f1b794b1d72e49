"""The decoder's conceal mode on the GPU (include/mi355x_h264_dec.h, "loss mode"): every case of tests/dec_loss.py through a Decoder
and through a DecoderGroup.  Every plane of every picture that comes out must equal the oracle's independent decoder's decode of the
COMPOSED stream (the lost NAL units replaced by all-P_Skip stand-ins; tests/test_dec_loss_oracle.py proves what the cases hold);
the damage report must count what the test removed; every macroblock the damage map calls clean must equal the LOSSLESS decode
(soundness); on the intra-refresh cases the map must come clean band by band as the refresh schedule says, and wholly clean at
the picture the CPU test names and not before (tightness); and the launch counts must be those of a strict decoder on the
composed stream, plus one in the steps where a stream joins."""
import numpy as np
import pytest

import dec_loss as dl
import intra_refresh as ir
import mem_guard as mg
from media_amd import h264dec, videodecoder as vd

pytestmark = pytest.mark.gpu
E_STREAM = h264dec.E_STREAM
IDS = [c.name for c in dl.CASES]


def geometry(c):
    s = dl.stream(c.stream)
    return s, (s.w + 15) // 16, (s.h + 15) // 16


def check_picture(tag, planes, m, d, c, k, bad):
    """one picture that came out at step k of case c: samples, report, soundness"""
    s, mbw, mbh = geometry(c)
    p, exp, ll = dl.plan(c), dl.expected(c)[k], dl.lossless(c)[k]
    for q in range(3):
        if not np.array_equal(planes[q], exp[q]):
            bad.append("%s step %d plane %d: %d samples differ from the composed stream's decode" % (tag, k, q, int((planes[q] != exp[q]).sum())))
    if d["concealed"] != p.concealed[k] or int(((m & dl.CONCEALED) != 0).sum()) != p.concealed[k]:
        bad.append("%s step %d: %d macroblocks reported concealed, %d in the map, %d removed" % (tag, k, d["concealed"], int(((m & dl.CONCEALED) != 0).sum()), p.concealed[k]))
    if d["gap"] != p.gap[k]:
        bad.append("%s step %d: gap %d, %d reference pictures lost" % (tag, k, d["gap"], p.gap[k]))
    if d["tainted"] != int((m & dl.TAINTED).sum()):
        bad.append("%s step %d: tainted %d, the map has %d" % (tag, k, d["tainted"], int((m & dl.TAINTED).sum())))
    if ll is not None:
        wrong = ~dl.mb_equal(planes, ll, mbw, mbh) & ((m & dl.TAINTED) == 0)
        if wrong.any():
            bad.append("%s step %d: %d macroblocks called clean differ from the lossless decode" % (tag, k, int(wrong.sum())))


def check_tightness(tag, m, d, c, k, bad):
    """intra-refresh cases, from the first refresh cycle that starts after the loss on: band j is clean from the picture with
    k = j on, the picture is exact at k = n - 1 and not before"""
    s, mbw, mbh = geometry(c)
    p, rec = dl.plan(c), dl.recovery_step(c)
    if k < p.first_loss:
        if d["tainted"]:
            bad.append("%s step %d: %d tainted macroblocks before any loss" % (tag, k, d["tainted"]))
        return
    if k >= rec:
        if d["tainted"] or d["joined"]:
            bad.append("%s step %d: tainted %d joined %d, the stream is exact from step %d on" % (tag, k, d["tainted"], d["joined"], rec))
        return
    if not d["tainted"]:
        bad.append("%s step %d: reported exact before step %d" % (tag, k, rec))
    if c.join is not None and not d["joined"]:
        bad.append("%s step %d: not reported as joined" % (tag, k))
    band = s.bands[p.orig[k]]
    if k > rec - s.n:     # inside the recovery cycle
        bands = ir.band_rows(mbh, s.n)
        for j in range(band + 1):
            if (m[bands[j][0]:bands[j][1]] & dl.TAINTED).any():
                bad.append("%s step %d (k = %d): band %d is not clean" % (tag, k, band, j))
        if c.join is not None:
            for j in range(band + 1, s.n):
                if not (m[bands[j][0]:bands[j][1]] & dl.TAINTED).any():
                    bad.append("%s step %d (k = %d): band %d of a joined stream is clean before its refresh" % (tag, k, band, j))


def run_single(c):
    """the case through a concealing Decoder, next to a strict Decoder on the composed stream (whose launch counts are the measure)"""
    s, mbw, mbh = geometry(c)
    p = dl.plan(c)
    dec, ref = h264dec.Decoder(loss="conceal"), h264dec.Decoder()
    bad, fed_ref = [], 0
    try:
        for k, au in enumerate(p.fed):
            if au is None:
                continue
            got = dec.decode(au)
            if got != p.got[k]:
                bad.append("step %d: got_picture %d, expected %d" % (k, got, p.got[k]))
                break
            if not got:
                continue
            while fed_ref <= p.ref[k]:
                ref.decode(p.composed[fed_ref])
                fed_ref += 1
            planes, m, d = [dec.plane(q) for q in range(3)], dec.damage_map(), dec.damage()
            check_picture(c.name, planes, m, d, c, k, bad)
            if s.n:
                check_tightness(c.name, m, d, c, k, bad)
            a, b = dec.last_step(), ref.last_step()
            join = 1 if c.join is not None and k == 1 else 0
            if a["launches"] != b["launches"] + join or a["pictures"] != 1:
                bad.append("step %d: %d launches, the strict decoder on the composed stream %d, joining streams %d" % (k, a["launches"], b["launches"], join))
            if k >= p.first_loss if p.first_loss is not None else False:
                if d["since_loss"] != sum(1 for j in range(p.first_loss + 1, k + 1) if p.got[j]):
                    bad.append("step %d: since_loss %d" % (k, d["since_loss"]))
    finally:
        dec.close()
        ref.close()
    return bad


@pytest.mark.parametrize("c", dl.CASES, ids=IDS)
def test_single_decoder(c):
    bad = run_single(c)
    assert not bad, "\n".join(bad[:20])


def test_recovery_point_sei_is_reported_in_both_modes():
    c = dl.BY_NAME["ir3_join_at_recovery"]
    s = dl.stream(c.stream)
    for mode in ("strict", "conceal"):
        dec = h264dec.Decoder(loss=mode)
        try:
            for i, au in enumerate(s.aus[:6]):
                assert dec.decode(au)
                d = dec.damage()
                assert d["recovery_frame_cnt"] == (s.n - 1 if s.bands[i] == 0 else -1), (mode, i, d)
                assert d["tainted"] == d["concealed"] == d["gap"] == d["joined"] == 0 and not dec.damage_map().any()
        finally:
            dec.close()


def test_strict_mode_refuses_what_it_refused():
    """the damaged inputs through a Decoder that never heard of loss modes and through one set to strict: E_STREAM, the same message"""
    for name in ("ir3_lose_band1", "ir3_lose_first", "refs3_gap1", "ir3_join_at_recovery"):
        c = dl.BY_NAME[name]
        p = dl.plan(c)
        msgs = []
        for explicit in (False, True):
            dec = h264dec.Decoder()
            if explicit:
                dec.set_loss_mode("strict")
            try:
                msg = None
                for au in p.fed:
                    if au is None:
                        continue
                    try:
                        dec.decode(au)
                    except h264dec.StreamError as e:
                        msg = str(e)
                        break
                assert msg is not None, name
                msgs.append(msg)
            finally:
                dec.close()
        assert msgs[0] == msgs[1], msgs
        want = {"ir3_lose_band1": "slices out of order", "ir3_lose_first": "first slice of the access unit starts at macroblock",
                "refs3_gap1": "a picture is missing", "ir3_join_at_recovery": "P slice without a reference picture"}[name]
        assert want in msgs[0], msgs[0]


# ---------------------------------------------------------------- the group

# six streams of 64x96: per stream (case or None for the undamaged stream, mode, the step its plan starts at).  In step 3 streams 0
# and 1 join, 2 conceals a slice, 3 has a gap, 4 is strict and refuses, 5 is undamaged
GROUP = (("ir3_join_at_recovery", "conceal", 2), ("ir3_join_before", "conceal", 2), ("ir3_lose_band1", "conceal", 0),
         ("ir3_gap_at_3", "conceal", 0), ("ir3_lose_band1", "strict", 0), (None, "strict", 0))
GROUP_GAP = dl.case("ir3_gap_at_3", "ir3_64x96", {2: ("lose",)}, kind="gap")
STEPS = 9


def group_case(name):
    return GROUP_GAP if name == "ir3_gap_at_3" else dl.BY_NAME[name]


def run_group():
    S = len(GROUP)
    s = dl.stream("ir3_64x96")
    grp = h264dec.DecoderGroup(S, loss=[m for _, m, _ in GROUP])
    ref = h264dec.DecoderGroup(S)          # strict, never told of loss modes: the composed streams (stream 4: the same damaged input)
    bad = []
    refused = False
    try:
        for t in range(STEPS):
            aus, raus, ks = [], [], []
            for i, (name, mode, t0) in enumerate(GROUP):
                k = t - t0
                ks.append(k)
                if name is None:
                    aus.append(s.aus[t]); raus.append(s.aus[t])
                    continue
                p = dl.plan(group_case(name))
                au = p.fed[k] if 0 <= k < len(p.fed) else None
                aus.append(au)
                # (the composed stream has one access unit per step of the plan: a lost reference picture's stand-in where nothing arrives)
                raus.append(au if mode == "strict" else (p.composed[k] if 0 <= k < len(p.composed) else None))
            res, rres = grp.decode(aus), ref.decode(raus)
            a, b = grp.last_step(), ref.last_step()
            joins = sum(1 for i, (name, mode, t0) in enumerate(GROUP) if name and group_case(name).join is not None and ks[i] == 1)
            for i, (name, mode, t0) in enumerate(GROUP):
                k = ks[i]
                if name is None:
                    if res[i] != (0, 1) or not all(np.array_equal(x, y) for x, y in zip(grp.debug_planes(i), dl.oracle_planes(s.aus)[t])):
                        bad.append("step %d: the undamaged stream %s" % (t, res[i],))
                    continue
                c = group_case(name)
                p = dl.plan(c)
                if aus[i] is None:
                    continue
                if mode == "strict":
                    if k >= p.first_loss:
                        refused = True
                        if res[i] != (E_STREAM, 0):
                            bad.append("step %d: the strict stream was not refused: %s" % (t, res[i],))
                    elif res[i] != (0, 1):
                        bad.append("step %d: the strict stream %s" % (t, res[i],))
                    continue
                if res[i] != (0, 1 if p.got[k] else 0):
                    bad.append("step %d stream %d: %s %s" % (t, i, res[i], grp.error(i)))
                    continue
                if not p.got[k]:
                    continue
                tag = "stream %d (%s)" % (i, name)
                m, d = grp.damage_map(i), grp.damage(i)
                check_picture(tag, grp.debug_planes(i), m, d, c, k, bad)
                check_tightness(tag, m, d, c, k, bad)
            # (step 2 apart: there the reference group decodes the grey IDR pictures and a stand-in picture this group never sees)
            if t != 2 and a["launches"] != b["launches"] + (1 if joins else 0):
                bad.append("step %d: %d launches, the strict group on the composed streams %d, %d streams join" % (t, a["launches"], b["launches"], joins))
            if t == 3 and (joins != 2 or a["pictures"] != 5):
                bad.append("step 3: %d streams join, %d pictures" % (joins, a["pictures"]))
        assert refused
        return bad, grp, ref
    except Exception:
        grp.close(); ref.close()
        raise


def test_group_of_six_streams_with_every_kind_of_loss_in_one_step():
    bad, grp, ref = run_group()
    grp.close(); ref.close()
    assert not bad, "\n".join(bad[:20])


def test_strict_only_group_counts_equal_a_group_never_told():
    s = dl.stream("ir3_64x96")
    a, b = h264dec.DecoderGroup(2), h264dec.DecoderGroup(2, loss="strict")
    try:
        for au in s.aus[:6]:
            assert a.decode([au, au]) == b.decode([au, au]) == [(0, 1), (0, 1)]
            x, y = a.last_step(), b.last_step()
            for key in ("pictures", "launches", "transfers", "device_bytes", "pinned_bytes"):
                assert x[key] == y[key], (key, x, y)
    finally:
        a.close(); b.close()


def test_under_guard_mode():
    """a join and the group case with 262144 guard bytes around every block and poison: every guard and the ring's zeroed slack
    intact - the grey pictures are stored inside their slots"""
    with mg.guarded() as seen:
        c = dl.BY_NAME["ir3_join_before"]
        p = dl.plan(c)
        dec = h264dec.Decoder(loss="conceal")
        try:
            for k, au in enumerate(p.fed):
                assert dec.decode(au) == p.got[k]
                if p.got[k]:
                    for q in range(3):
                        assert np.array_equal(dec.plane(q), dl.expected(c)[k][q]), (k, q)
                    assert dec.mem_check()[0] == 0, k
        finally:
            dec.close()
        bad, grp, ref = run_group()
        try:
            assert not bad, "\n".join(bad[:20])
            assert grp.mem_check()[0] == 0 and ref.mem_check()[0] == 0
        finally:
            grp.close(); ref.close()
    mg.clean(seen, kinds=["decoder", "group"])


def test_plugin_decoder_survives_a_dropped_slice_and_reports_exact_pictures():
    c = dl.BY_NAME["ir3_lose_band1"]
    p, exp = dl.plan(c), dl.expected(c)
    s = dl.stream(c.stream)
    rec = dl.recovery_step(c)
    vd.set_loss_mode(1)
    d = vd.PluginDecoder()
    try:
        assert d.create_decoder(vd.STREAM_AVC) == vd.SUCCESS and d.init() == vd.SUCCESS and d.install_hooks() == vd.SUCCESS
        assert d.set_pic_info(s.w, s.h) == vd.SUCCESS and d.start() == vd.SUCCESS
        for k, au in enumerate(p.fed):
            assert d.send(au) == vd.SUCCESS, k
            rc, frame = d.retrieve(s.w * s.h * 3 // 2)
            assert rc == vd.SUCCESS, k
            want = np.concatenate([exp[k][q][:(s.h if q == 0 else s.h // 2), :(s.w if q == 0 else s.w // 2)].ravel() for q in range(3)])
            assert np.array_equal(frame, want), k
            assert d.inexact() == (p.first_loss <= k < rec), k
        assert d.stop() == vd.SUCCESS
    finally:
        vd.set_loss_mode(None)
        d.delete()


def test_a_join_that_is_refused_makes_no_launch():
    """a stream of another coded size joins a group: the picture is refused behind the join's bookkeeping, and the step makes the
    launches of a step without it - no k_dec_ring_fill for a position that is not in the table"""
    big, small = dl.stream("ir3_64x96"), dl.stream("ir2_48x64")
    grp, ref = h264dec.DecoderGroup(2, loss="conceal"), h264dec.DecoderGroup(2)
    try:
        assert grp.decode([big.aus[0], dl.parameter_sets(small)]) == [(0, 1), (0, 0)] and ref.decode([big.aus[0], None]) == [(0, 1), (0, 0)]
        assert grp.decode([big.aus[1], small.aus[3]]) == [(0, 1), (E_STREAM, 0)] and "coded size 48x64 differs" in grp.error(1)
        assert ref.decode([big.aus[1], None]) == [(0, 1), (0, 0)]
        a, b = grp.last_step(), ref.last_step()
        assert a["pictures"] == b["pictures"] == 1 and a["launches"] == b["launches"], (a, b)
        assert all(np.array_equal(x, y) for x, y in zip(grp.debug_planes(0), dl.oracle_planes(big.aus)[1]))
    finally:
        grp.close(); ref.close()


def test_the_maps_go_on_when_a_stream_that_concealed_is_set_to_strict():
    """conceal, strict, conceal again between calls: the stream's reference pictures stay as tainted as they were, the report goes on
    saying so, and it comes clean at the picture the schedule names"""
    c = dl.BY_NAME["ir3_join_at_recovery"]
    p, exp, rec = dl.plan(c), dl.expected(c), dl.recovery_step(c)
    dec = h264dec.Decoder(loss="conceal")
    try:
        for k, au in enumerate(p.fed):
            if k == 2:
                dec.set_loss_mode("strict")
            if k == 3:
                dec.set_loss_mode("conceal")
            assert dec.decode(au) == p.got[k]
            if not p.got[k]:
                continue
            for q in range(3):
                assert np.array_equal(dec.plane(q), exp[k][q]), (k, q)
            d, m = dec.damage(), dec.damage_map()
            assert (d["tainted"] > 0) == (k < rec) and d["tainted"] == int((m & dl.TAINTED).sum()), (k, d)
            wrong = ~dl.mb_equal([dec.plane(q) for q in range(3)], dl.lossless(c)[k], m.shape[1], m.shape[0]) & ((m & dl.TAINTED) == 0)
            assert not wrong.any(), k
    finally:
        dec.close()
