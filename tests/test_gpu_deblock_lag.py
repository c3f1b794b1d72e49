"""The two ends of the loop filter's row pipeline (media_amd/csrc/k_deblock.h).  A row waits for the bottom sample rows of
the macroblock above between its vertical- and its horizontal-edge phase and publishes its previous macroblock right after
the current one's left edge; in the pair form the lower row of a wave runs one macroblock behind the upper one.  On pictures
1 to 3 macroblocks wide the start-up, the closing publish of a row and the slots of the ring inside a pair all fall into the
same few iterations, and 1 to 5 macroblock rows give no lower row, full pairs and an odd last row.  Every case is compared with
the oracle: access units byte for byte, reconstruction planes sample for sample.  The content is an IDR picture followed by P
pictures with intra macroblocks at a QP at which the oracle's own filter changes samples (asserted), so an apron taken too
early or a hand-off published too early changes the result.  In a lockstep batch the planes read back are those of the
first GOP's last picture; the earlier pictures of every GOP are the references of the ones that follow them, so their
samples are covered by the streams."""
import functools
import numpy as np
import pytest
from media_amd import capi, synth, h264dec
from oracle_lib import OracleEncoder

pytestmark = pytest.mark.gpu

GOP, NGOP = 4, 8
SIZES = [(w, h) for w in (16, 32, 48) for h in (16, 32, 48, 64, 80)]


@functools.lru_cache(maxsize=None)
def _oracle(kind, w, h, qp, slices=0):
    """(frames, [(access unit, (Y, U, V))]) of NGOP GOPs; computed once per configuration and shared, never modified"""
    frames = synth.sequence(kind, w, h, GOP * NGOP)
    orc = OracleEncoder(w, h, qp=qp, gop=GOP, slices=slices)
    out, filtered, intra_in_p = [], False, False
    for i, f in enumerate(frames):
        au = orc.encode(f)[0]
        planes = tuple(orc.recon(p).copy() for p in range(3))
        filtered |= any(not np.array_equal(planes[p], orc.recon_pre(p)) for p in range(3))
        if i % GOP:
            intra_in_p |= bool(np.isin(orc.mbinfo()["type"], (0, 3, 4)).any())
        out.append((au, planes))
    orc.close()
    for _, planes in out:
        for a in planes:
            a.setflags(write=False)
    assert filtered, "the oracle's filter changes no sample: the case would prove nothing"
    return frames, out, intra_in_p


def _set_form(monkeypatch, form):
    monkeypatch.setenv("MI355X_H264_PAIR_FILTER", "1" if form == "pairs" else "0")


def _single(kind, w, h, qp, slices=0, count=2 * GOP):
    frames, want, _ = _oracle(kind, w, h, qp, slices)
    enc = capi.Encoder(w, h, qp=qp, gop=GOP, slices=slices)
    try:
        for i in range(count):
            assert enc.encode(frames[i])[0] == want[i][0], "picture %d: access unit" % i
            for p in range(3):
                got = enc.debug_read(capi.DBG_RECON_Y + p)
                bad = np.argwhere(got != want[i][1][p])
                assert bad.size == 0, "picture %d plane %d: first differing sample (row, column) %s" % (i, p, bad[0])
    finally:
        enc.close()


def _batch(kind, w, h, qp, slices=0):
    import torch
    frames, want, _ = _oracle(kind, w, h, qp, slices)
    fbytes = w * h * 3 // 2
    dev = torch.from_numpy(np.stack(frames)).cuda()
    enc = capi.Encoder(w, h, qp=qp, gop=GOP, slices=slices, batch=NGOP)
    try:
        cap = 4 * GOP * fbytes + 4096
        out, szs, gb = np.zeros(NGOP * cap, np.uint8), np.zeros(NGOP * GOP, np.uint32), np.zeros(NGOP, np.uint64)
        enc.encode_gops_device(dev.data_ptr(), fbytes, GOP * fbytes, GOP, out, cap, szs, gb)
        for g in range(NGOP):
            assert out[g * cap: g * cap + int(gb[g])].tobytes() == b"".join(a for a, _ in want[g * GOP:(g + 1) * GOP]), "GOP %d" % g
        for p in range(3):
            got = enc.debug_read(capi.DBG_RECON_Y + p)
            bad = np.argwhere(got != want[GOP - 1][1][p])
            assert bad.size == 0, "GOP 0 plane %d: first differing sample (row, column) %s" % (p, bad[0])
    finally:
        enc.close()


def test_the_content_has_intra_macroblocks_in_p_pictures():
    """what the cases below rely on, stated of the oracle alone: at the largest size both kinds of content put intra
    macroblocks (bS 3 / 4 edges) into P pictures"""
    assert _oracle("cut", 48, 80, 33)[2]
    assert _oracle("s3", 48, 80, 36)[2]


@pytest.mark.parametrize("form", ["pairs", "rows"])
@pytest.mark.parametrize("w,h", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_narrow_pictures_single_and_batch_of_eight(monkeypatch, w, h, form):
    _set_form(monkeypatch, form)
    _single("cut", w, h, 33)
    _batch("cut", w, h, 33)


@pytest.mark.parametrize("form", ["pairs", "rows"])
@pytest.mark.parametrize("kind,w,h,qp", [("s3", 16, 32, 36), ("s3", 32, 48, 36), ("s3", 48, 80, 36), ("cut", 48, 80, 51), ("s3", 32, 64, 51)])
def test_other_content_and_the_top_qp(monkeypatch, kind, w, h, qp, form):
    _set_form(monkeypatch, form)
    _single(kind, w, h, qp)
    _batch(kind, w, h, qp)


@pytest.mark.parametrize("w,h,slices", [(48, 96, 3), (32, 80, 2)])
def test_row_form_with_several_slices(w, h, slices):
    """every slice is a wavefront of its own, with a first row that waits for nobody and a last row that stores all sixteen
    sample rows; pictures of several slices take the row form in a batch too"""
    _single("cut", w, h, 33, slices)
    _batch("cut", w, h, 33, slices)


def test_hub_stream():
    """the indirect kernels (a stream of the shared engine)"""
    w, h, qp = 48, 80, 33
    frames, want, _ = _oracle("cut", w, h, qp)
    st = capi.Stream(w, h, qp=qp, gop=GOP)
    try:
        for i in range(2 * GOP):
            assert st.encode(frames[i])[0] == want[i][0], "picture %d: access unit" % i
            for p in range(3):
                assert np.array_equal(st.recon(p), want[i][1][p]), "picture %d plane %d" % (i, p)
    finally:
        st.close()


def test_decoder_peer_on_the_encoders_stream():
    """the decoder's row form (thresholds per macroblock) on a stream the encoder wrote"""
    w, h, qp = 48, 80, 33
    frames, want, _ = _oracle("cut", w, h, qp)
    enc = capi.Encoder(w, h, qp=qp, gop=GOP)
    dec = h264dec.Decoder()
    try:
        for i in range(2 * GOP):
            au = enc.encode(frames[i])[0]
            assert au == want[i][0], "picture %d: access unit" % i
            assert dec.decode(au), "picture %d" % i
            for p in range(3):
                got = dec.plane(p)
                assert np.array_equal(got, enc.debug_read(capi.DBG_RECON_Y + p)), "picture %d plane %d: decoder != encoder" % (i, p)
                assert np.array_equal(got, want[i][1][p]), "picture %d plane %d: decoder != oracle" % (i, p)
    finally:
        dec.close()
        enc.close()
