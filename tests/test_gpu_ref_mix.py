"""The multi-reference motion search where the older pictures win, on the GPU - run with -m gpu on an MI355X.

The cases are those of tests/ref_mix.py (tests/test_ref_mix_oracle.py proves on the oracle alone that ref_idx_l0 1 and 2 are
chosen under every partition shape, beside P_Skip, across slice boundaries and with nothing else to tell neighbours apart).
Everything is compared exactly: access units byte for byte, every stage array, the planes before and after the loop filter."""
import numpy as np
import pytest
import ref_mix as rm
from media_amd import capi, h264dec
from oracle_lib import OracleDecoder
from test_gpu_parity import _compare_all

pytestmark = pytest.mark.gpu
BOTH = [(c, s) for c in rm.CASES for s in rm.SEARCHES]
IDS = ["%s-search%d" % (c.name, s) for c, s in BOTH]


def _encoder(c, search, **kw):
    return capi.Encoder(c.w, c.h, qp=c.qp, gop=c.gop, profile_idc=c.prof, slices=c.slices, refs=c.refs, search=search, **kw)


def _decodes_to(dec, au, enc, tag):
    """the independent decoder decodes the GPU's bytes to the GPU's reconstruction"""
    assert dec.decode(au) == 1, tag
    for p in range(3):
        assert np.array_equal(dec.plane(p), enc.debug_read(capi.DBG_RECON_Y + p)), "%s: the independent decoder's plane %d" % (tag, p)


def _frame_by_frame(c, search, events=(), gdec=None):
    want = rm.expected(c, search, events)
    enc, dec = _encoder(c, search), OracleDecoder()
    try:
        enc.keep_pre(True)
        for i, f in enumerate(rm.frames(c)):
            for at, what in events:
                if at == i and what == "idr":
                    enc.force_idr()
                elif at == i:
                    enc.set_qp(what)
            tag = "%s search %d picture %d" % (c.name, search, i)
            au, ft = enc.encode_nv12(rm.to_nv12(f, c.w, c.h)) if c.nv12 else enc.encode(f)
            assert (ft == capi.FRAME_IDR) == want[i].idr, tag
            assert au == want[i].au, tag + ": access unit"
            _compare_all(enc, want[i].stages, tag)
            _decodes_to(dec, au, enc, tag)
            if gdec is not None:
                assert gdec.decode(au), tag
                for p in range(3):
                    assert np.array_equal(gdec.plane(p), enc.debug_read(capi.DBG_RECON_Y + p)), "%s: the decoder peer's plane %d" % (tag, p)
    finally:
        enc.close()
        dec.close()


@pytest.mark.parametrize("c,search", BOTH, ids=IDS)
def test_frame_by_frame_every_stage(c, search):
    _frame_by_frame(c, search)


@pytest.mark.parametrize("form", ["pairs", "rows"])
@pytest.mark.parametrize("name", ["still_96x80", "split_96x80_high", "split_208x160"])
def test_both_loop_filter_forms(monkeypatch, name, form):
    """boundary strength 1 from a reference difference alone (still), and under partitions, in both forms of the loop filter"""
    monkeypatch.setenv("MI355X_H264_PAIR_FILTER", "1" if form == "pairs" else "0")
    _frame_by_frame(rm.BY_NAME[name], 1)


@pytest.mark.parametrize("b", rm.BATCHES, ids=lambda b: b.name)
@pytest.mark.parametrize("search", rm.SEARCHES)
def test_lockstep_batches(b, search):
    """G closed GOPs in lockstep, every item the content at a seed and a start of its own: every item's bytes equal its own
    oracle's, item 0's stages match, and K_ME was launched once per reference picture a P picture may use"""
    import torch
    c = b.case
    items, stages0 = rm.batch_expected(b, search)
    fbytes = c.w * c.h * 3 // 2
    dev = torch.from_numpy(np.stack([f for g in range(b.G) for f in rm.frames(rm.batch_item(b, g))])).cuda()
    enc = _encoder(c, search, batch=b.G)
    try:
        enc.keep_pre(True)
        enc.stats_enable(True)
        cap = 2 * c.gop * fbytes + 4096
        out, sizes, gb = np.zeros(b.G * cap, np.uint8), np.zeros(b.G * c.gop, np.uint32), np.zeros(b.G, np.uint64)
        enc.encode_gops_device(dev.data_ptr(), fbytes, c.gop * fbytes, c.gop, out, cap, sizes, gb)
        for g in range(b.G):
            want = [p.au for p in items[g]]
            assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(want), "%s item %d: the GOP's bytes" % (b.name, g)
            assert [int(x) for x in sizes[g * c.gop:(g + 1) * c.gop]] == [len(x) for x in want], "%s item %d: sizes[]" % (b.name, g)
        _compare_all(enc, stages0, "%s item 0, last picture" % b.name)
        st = enc.stats(reset=True)
        assert st["frames"] == b.G * c.gop
        assert st["kernels"]["me"]["launches"] == rm.me_launches(c.refs, [i == 0 for i in range(c.gop)]), st["kernels"]["me"]
    finally:
        enc.close()


def test_window_restarts_at_a_forced_idr_and_qp_changes():
    """force_idr() in the middle of a GOP: one, then two references are available again; set_qp(20) two pictures later, then
    set_qp(40): the GPU against the oracle driven the same way"""
    c = rm.BY_NAME["s1_208x160"]
    want = rm.expected(c, 1, rm.WINDOW_EVENTS)
    assert want[4].idr and [p.facts["available"] for p in want[3:8]] == [3, 0, 1, 2, 3]
    _frame_by_frame(c, 1, rm.WINDOW_EVENTS)


@pytest.mark.parametrize("name,W", [("fast_96x128", 2), ("fast_96x128", 4), ("scroll_112x96", 3)])
def test_band_instances_read_the_older_pictures_halo_rows(name, W):
    """W band instances of one GPU, halo export / import after every picture: the access units put together equal the oracle's
    (one instance, the same slices) and decode.  The older references' vectors cross the band boundaries (asserted on the
    oracle in tests/test_ref_mix_oracle.py), so the halo rows of the two older ring slots are read"""
    import torch
    c = rm.BY_NAME[name]
    want = rm.expected(c, 1)
    parts = [_encoder(c, 1, band_index=r, band_count=W) for r in range(W)]
    dec = OracleDecoder()
    try:
        info = [p.band_info() for p in parts]
        assert info[0][0] == 0 and sum(i[1] for i in info) == (c.h + 15) // 16 and all(i[1] > 0 for i in info)
        buf = torch.empty(info[0][4], dtype=torch.uint8, device="cuda")
        for i, f in enumerate(rm.frames(c)[:10]):
            got = b"".join(p.encode(f)[0] for p in parts)
            assert got == want[i].au, "%s on %d instances, picture %d" % (name, W, i)
            assert dec.decode(got) == 1
            for pl in range(3):
                assert np.array_equal(dec.plane(pl), want[i].stages.recon(pl)), "picture %d plane %d" % (i, pl)
            for r in range(W):
                if r > 0:            # my top rows become the rows below my upper neighbour
                    parts[r].halo_export(0, buf.data_ptr())
                    parts[r - 1].halo_import(1, buf.data_ptr())
                if r < W - 1:        # my bottom rows become the rows above my lower neighbour
                    parts[r].halo_export(1, buf.data_ptr())
                    parts[r + 1].halo_import(0, buf.data_ptr())
    finally:
        for p in parts:
            p.close()
        dec.close()


def test_nv12_through_the_device_form():
    """the nv12 case from device memory (the host form runs in test_frame_by_frame_every_stage)"""
    import torch
    c = rm.BY_NAME["nv12"]
    want = rm.expected(c, 1)
    dev = torch.from_numpy(np.stack([rm.to_nv12(f, c.w, c.h) for f in rm.frames(c)])).cuda()
    enc = _encoder(c, 1, input_format=capi.INPUT_NV12)
    try:
        enc.keep_pre(True)
        for i in range(c.pictures):
            assert enc.encode_device(dev[i].data_ptr())[0] == want[i].au, "picture %d" % i
            _compare_all(enc, want[i].stages, "nv12 device picture %d" % i)
    finally:
        enc.close()


@pytest.mark.parametrize("name", ["split_208x160", "still_96x80"])
def test_decoder_peer_on_the_encoders_streams(name):
    """h264dec.Decoder on the GPU encoder's stream: its planes equal the encoder's reconstruction after every picture"""
    gdec = h264dec.Decoder()
    try:
        _frame_by_frame(rm.BY_NAME[name], 1, gdec=gdec)
    finally:
        gdec.close()


def test_decoder_group_of_three_streams_one_picture_apart():
    """one DecoderGroup holds the three 96x80 streams, started one picture apart so that their rings stand at different
    positions: every stream's planes equal the independent decoder's (which reconstructed the encoder's planes: ref_mix.expected)"""
    cases = [rm.BY_NAME[n] for n in ("split_96x80_high", "still_96x80", "two_refs_s1_96x80")]
    want = [rm.expected(c, 1) for c in cases]
    grp = h264dec.DecoderGroup(3)
    try:
        steps = max(k + c.pictures for k, c in enumerate(cases))
        for t in range(steps):
            part = [k for k, c in enumerate(cases) if 0 <= t - k < c.pictures]
            res = grp.decode([want[k][t - k].au if k in part else None for k in range(3)])
            assert res == [(0, 1) if k in part else (0, 0) for k in range(3)], (t, res, [grp.error(k) for k in range(3)])
            for k in part:
                planes = grp.debug_planes(k)
                for p in range(3):
                    assert np.array_equal(planes[p], want[k][t - k].stages.recon(p)), "step %d stream %d (%s) plane %d" % (t, k, cases[k].name, p)
    finally:
        grp.close()
