"""The loop filter's wait for the row above (media_amd/csrc/k_deblock.h, db_rerequest / db_wait_tags): the first look at the
hand-off granule stands in front of the spin and waits for none of the iteration's own stores - the prefetched copy where it came
fresh, the re-requested one behind a counted wait where it came stale - and the row form asks for the next macroblock with a
fixed number of loads, clamped into the row.  What can go wrong is which copy of a granule a lane ends up with, and what the
clamped prefetch leaves in the registers at the ends of a row: so the sizes are the smallest at which those paths differ - one
macroblock (the closing publish is the only one, nothing to prefetch), one pair, a pair and a lone upper row, one row that is
first and last, a first row in mid-picture (slices) - in both forms, with one picture in flight and in lockstep batches of 16 and
32, and two encoders on two host threads (uneven load, warm consumers).  Every case is compared with the oracle exactly: every
access unit byte for byte, all three planes after the filter sample for sample.  A filter wait that timed out fails the call
(the engine turns *R.err into an error).  The decoder's form (thresholds per macroblock, indirect launch) decodes the oracle's
own streams."""
import functools
import threading
import numpy as np
import pytest
from media_amd import capi, synth, h264dec
from oracle_lib import OracleEncoder

gpu = pytest.mark.gpu
FORMS = ["pairs", "rows"]
GOP, QP = 4, 33
SIZES = [(16, 16, 0), (16, 32, 0), (16, 48, 0), (32, 16, 0), (32, 48, 0), (48, 80, 0), (16, 64, 2), (32, 96, 3)]   # w, h, slices
SIZE_IDS = ["%dx%d" % (w, h) + ("-%dslices" % s if s else "") for w, h, s in SIZES]
DEC_SIZES = [(16, 48), (32, 48), (48, 80)]
INTRA_TYPES = (0, 3, 4)   # MbInfo type: Intra16x16, I_PCM, Intra4x4


# Where each plain item's stretch of the pan starts.  At 16x16 and 32x16 some stretches leave a P picture all P_Skip - nothing to
# filter -; these sixteen are filtered in every picture at every size used here, which the oracle tests below assert.
S1_STARTS = (2, 4, 5, 6, 7, 8, 10, 15, 16, 17, 18, 19, 20, 21, 22, 23)


def _item(kind, w, h, gop, g):
    """the gop pictures of batch item g: every plain item its own stretch of the pan"""
    return synth.sequence("s1", w, h, gop, start=S1_STARTS[(g // 2) % 16]) if kind == "s1" else synth.sequence(kind, w, h, gop, start=0)


@functools.lru_cache(maxsize=None)
def _oracle(kinds, w, h, gop, slices=0):
    """kinds: one content name per batch item.  (frames, per picture (access unit, (Y, U, V), intra macroblocks, filter changed a
    sample)); computed once per configuration and shared, never modified"""
    frames = [f for g, k in enumerate(kinds) for f in _item(k, w, h, gop, g)]
    orc = OracleEncoder(w, h, qp=QP, gop=gop, slices=slices)
    out = []
    for f in frames:
        au = orc.encode(f)[0]
        planes = tuple(orc.recon(p).copy() for p in range(3))
        for a in planes:
            a.setflags(write=False)
        changed = any(not np.array_equal(planes[p], orc.recon_pre(p)) for p in range(3))
        out.append((au, planes, int(np.isin(orc.mbinfo()["type"], INTRA_TYPES).sum()), changed))
    orc.close()
    return frames, out


def _mixed_kinds(n):
    """n items, cut and pan + noise in turn"""
    return ("cut", "s1") * (n // 2)


def _assert_filtered(kinds, w, h, gop, slices=0):
    """every picture of the case is changed by the filter (a case that stops being filtered proves nothing and must fail), and
    where the case has a cut and more than one macroblock, P picture 2 of the cut holds intra macroblocks: both picture bodies
    of the P-step kernels run"""
    _, out = _oracle(kinds, w, h, gop, slices)
    for i, o in enumerate(out):
        assert o[3], "%dx%d slices %d item %d (%s) picture %d: the filter changes nothing" % (w, h, slices, i // gop, kinds[i // gop], i % gop)
    for g, k in enumerate(kinds):
        if k == "cut":
            assert out[g * gop + 1][2] == 0, "P picture 1 of a cut item has no intra macroblock"
            if (w, h) != (16, 16):
                assert out[g * gop + 2][2] > 0, "%dx%d: P picture 2 of the cut holds intra macroblocks" % (w, h)


def _set_form(monkeypatch, form):
    monkeypatch.setenv("MI355X_H264_PAIR_FILTER", "1" if form == "pairs" else "0")


def _single(kinds, w, h, gop, slices=0):
    """item after item through one encoder, one picture in flight; planes compared after every picture"""
    frames, want = _oracle(kinds, w, h, gop, slices)
    enc = capi.Encoder(w, h, qp=QP, gop=gop, slices=slices)
    try:
        for i, f in enumerate(frames):
            assert enc.encode(f)[0] == want[i][0], "picture %d: access unit" % i
            for p in range(3):
                bad = np.argwhere(enc.debug_read(capi.DBG_RECON_Y + p) != want[i][1][p])
                assert bad.size == 0, "picture %d plane %d: first differing sample (row, column) %s" % (i, p, bad[0])
    finally:
        enc.close()


def _batch(kinds, w, h, gop, slices=0):
    """one lockstep call; raises on a filter timeout.  Every item's stream, and the planes of the first item's last picture"""
    import torch
    frames, want = _oracle(kinds, w, h, gop, slices)
    n, fbytes = len(kinds), w * h * 3 // 2
    dev = torch.from_numpy(np.stack(frames)).cuda()
    enc = capi.Encoder(w, h, qp=QP, gop=gop, slices=slices, batch=n)
    try:
        cap = 4 * gop * fbytes + 4096
        out, szs, gb = np.zeros(n * cap, np.uint8), np.zeros(n * gop, np.uint32), np.zeros(n, np.uint64)
        enc.encode_gops_device(dev.data_ptr(), fbytes, gop * fbytes, gop, out, cap, szs, gb)
        for g in range(n):
            assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(w_[0] for w_ in want[g * gop:(g + 1) * gop]), "item %d (%s)" % (g, kinds[g])
        for p in range(3):
            bad = np.argwhere(enc.debug_read(capi.DBG_RECON_Y + p) != want[gop - 1][1][p])
            assert bad.size == 0, "item 0 plane %d: first differing sample (row, column) %s" % (p, bad[0])
    finally:
        enc.close()


# ---- what the GPU cases rely on, stated of the oracle alone (no GPU needed)

@pytest.mark.parametrize("w,h,slices", SIZES, ids=SIZE_IDS)
def test_oracle_every_picture_is_filtered_and_the_cut_brings_intra_macroblocks(w, h, slices):
    _assert_filtered(("cut",), w, h, GOP, slices)
    _assert_filtered(("s1",), w, h, GOP, slices)
    _assert_filtered(_mixed_kinds(32), w, h, GOP, slices)   # (its first sixteen items are the batch of 16)


def test_oracle_uneven_load_content_is_filtered():
    _assert_filtered(_mixed_kinds(16), 176, 144, 6)


@pytest.mark.parametrize("w,h", DEC_SIZES, ids=["%dx%d" % s for s in DEC_SIZES])
def test_oracle_decoder_streams_are_filtered(w, h):
    _assert_filtered(("cut",), w, h, GOP)


# ---- the GPU cases

@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("w,h,slices", SIZES, ids=SIZE_IDS)
def test_one_picture_in_flight(monkeypatch, w, h, slices, form):
    for kinds in (("cut",), ("s1",)):
        _assert_filtered(kinds, w, h, GOP, slices)
    _set_form(monkeypatch, form)
    _single(("cut",), w, h, GOP, slices)
    _single(("s1",), w, h, GOP, slices)


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [16, 32])
@pytest.mark.parametrize("w,h,slices", SIZES, ids=SIZE_IDS)
def test_lockstep_batch(monkeypatch, w, h, slices, n, form):
    kinds = _mixed_kinds(n)
    _assert_filtered(kinds, w, h, GOP, slices)
    _set_form(monkeypatch, form)
    _batch(kinds, w, h, GOP, slices)


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_two_encoders_on_two_threads(monkeypatch, form):
    """176x144, six pictures, sixteen items each: thirty-two pictures at a time place their waves over time, rows find granules
    both published and not yet there, and the consumers of one encoder are warm while the other's kernels run beside them"""
    w, h, gop = 176, 144, 6
    kinds = _mixed_kinds(16)
    _assert_filtered(kinds, w, h, gop)
    _oracle(kinds, w, h, gop)   # (computed before the threads start: they only read it)
    _set_form(monkeypatch, form)
    errors = []

    def run(k):
        try:
            _batch(kinds, w, h, gop)
        except BaseException as ex:  # noqa: BLE001
            errors.append((k, repr(ex)))

    ths = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors


@gpu
@pytest.mark.parametrize("w,h", DEC_SIZES, ids=["%dx%d" % s for s in DEC_SIZES])
def test_decoder_form_on_the_oracles_stream(w, h):
    """k_deblock_rows<.., PERMB, IND>: thresholds per macroblock, seven loads per prefetch"""
    _assert_filtered(("cut",), w, h, GOP)
    _, want = _oracle(("cut",), w, h, GOP)
    dec = h264dec.Decoder()
    try:
        for i, o in enumerate(want):
            assert dec.decode(o[0]), "picture %d: no picture" % i
        for p in range(3):
            bad = np.argwhere(dec.plane(p) != want[-1][1][p])
            assert bad.size == 0, "plane %d of the last picture: first differing sample (row, column) %s" % (p, bad[0])
    finally:
        dec.close()
