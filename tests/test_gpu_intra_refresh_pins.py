"""Intra refresh on the GPU, the two oracle pins (run with -m gpu on an MI355X).  The unchanged oracle knows no refresh, yet pins two
parts of every refresh stream stage by stage:
(a) in the first P picture after an IDR picture (k = 0) the bands 1 .. n-1 are unrestricted and see the same reference picture as
    the ordinary slices = n stream: their rows equal the oracle's, and so do their slice NAL units byte for byte;
(b) in every P picture the rows of band k equal those rows of a fresh oracle encoder's IDR picture of the same source picture at the
    same QP with slices = n: the oracle has one intra coder for both picture types, slices do not see each other, and no picture
    holds I_PCM.
Compared per macroblock row range: MbInfo, the levels the entropy coder reads (by type and pattern), vectors (a) / Intra4x4 modes
(b), the planes before and after the loop filter."""
import numpy as np
import pytest
import intra_refresh as ir
from media_amd import capi
from oracle_lib import OracleEncoder

pytestmark = pytest.mark.gpu


def _compare_rows(enc, orc, r0, r1, mbw, tag, inter):
    sel = slice(r0 * mbw, r1 * mbw)
    mb, omb = enc.debug_read(capi.DBG_MBINFO)[sel], orc.mbinfo()[sel]
    for f in ("mvx", "mvy", "type", "i16_mode", "chroma_mode", "cbp", "tc"):
        assert np.array_equal(mb[f], omb[f]), "%s: mbinfo.%s" % (tag, f)
    assert not (omb["type"] == ir.MB_IPCM).any(), tag + ": I_PCM"
    glv, olv = enc.debug_read(capi.DBG_LEVELS)[sel], orc.levels()[sel]
    read = np.zeros(olv.shape, dtype=bool)
    cbp = omb["cbp"].astype(np.int32)
    read[omb["type"] == 0, 0:16] = True
    for q in range(4):
        read[(cbp >> q) & 1 == 1, 16 + 64 * q: 16 + 64 * (q + 1)] = True
    read[(cbp >> 4) >= 1, 272:280] = True
    read[(cbp >> 4) == 2, 280:408] = True
    assert np.array_equal(np.where(read, glv, 0), np.where(read, olv, 0)), tag + ": levels"
    if inter:
        m = np.isin(omb["type"], (1, 2, 5, 6, 7))
        assert np.array_equal(enc.debug_read(capi.DBG_MVQ)[sel][m], orc.mvq()[sel][m]), tag + ": quadrant vectors"
    else:
        assert np.isin(omb["type"], ir.INTRA).all(), tag + ": the oracle's IDR picture"
        i4 = omb["type"] == 4
        assert np.array_equal(enc.debug_read(capi.DBG_MBAUX)[sel][i4], orc.mbaux()[sel][i4]), tag + ": Intra4x4 modes"
    for p in range(3):
        a, b = (16 if p == 0 else 8) * r0, (16 if p == 0 else 8) * r1
        assert np.array_equal(enc.debug_read(capi.DBG_PRE_Y + p)[a:b], orc.recon_pre(p)[a:b]), "%s: pre-filter plane %d" % (tag, p)
        assert np.array_equal(enc.debug_read(capi.DBG_RECON_Y + p)[a:b], orc.recon(p)[a:b]), "%s: recon plane %d" % (tag, p)


@pytest.mark.parametrize("c", ir.SMALL, ids=[c.name for c in ir.SMALL])
def test_oracle_pins(c):
    kw = dict(qp=c.qp, gop=1000, profile_idc=c.prof, slices=c.n, search=c.search)
    mbw, mbh = (c.w + 15) // 16, (c.h + 15) // 16
    bands = ir.band_rows(mbh, c.n)
    sched = ir.schedule(c.n, 1000, c.pictures)
    enc = capi.Encoder(c.w, c.h, intra_refresh=True, **kw)
    orc = OracleEncoder(c.w, c.h, **kw)
    try:
        enc.keep_pre(True)
        for i, f in enumerate(ir.frames(c)[:c.n + 2]):
            au, _ = enc.encode(f)
            k = sched[i][2]
            if i <= 1:
                oau, _ = orc.encode(f)
            if i == 0:
                assert au == oau, "the IDR picture is the oracle's"
            if i == 1:   # (a)
                _compare_rows(enc, orc, bands[1][0], mbh, mbw, "%s (a) bands 1..%d" % (c.name, c.n - 1), True)
                got, want = ir.split_nals(au), ir.split_nals(oau)
                assert len(got) == c.n + 1 and len(want) == c.n and got[2:] == want[1:], "%s (a): the slice NAL units of bands 1.." % c.name
            if k >= 0:   # (b)
                fresh = OracleEncoder(c.w, c.h, **kw)
                fresh.encode(f)
                _compare_rows(enc, fresh, bands[k][0], bands[k][1], mbw, "%s (b) picture %d band %d" % (c.name, i, k), False)
                fresh.close()
    finally:
        enc.close()
        orc.close()
