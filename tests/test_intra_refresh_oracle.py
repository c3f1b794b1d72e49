"""Intra refresh on the oracle alone (CPU): the control of the recovery test - two ordinary slices = n streams of the case's two
contents, spliced, do NOT recover by chance - the SEI restatement against hand-written bytes, and the schedule restatement against
hand-written lists.  Nothing of the encoder under test runs here."""
import numpy as np
import pytest
import intra_refresh as ir
from oracle_lib import OracleDecoder, OracleEncoder

IDS = [c.name for c in ir.SMALL]


def oracle_stream(c, frames):
    """[(access unit, (Y, U, V) reconstruction)] of the unchanged oracle with slices = n"""
    enc = OracleEncoder(c.w, c.h, qp=c.qp, gop=1000, profile_idc=c.prof, slices=c.n, search=c.search)
    out = []
    for f in frames:
        au, _ = enc.encode(f)
        assert not (enc.mbinfo()["type"] == ir.MB_IPCM).any(), "%s: I_PCM macroblocks" % c.name
        out.append((au, tuple(enc.recon(p).copy() for p in range(3))))
    enc.close()
    return out


def decode_all(aus):
    dec, out = OracleDecoder(), []
    for au in aus:
        assert dec.decode(au) == 1
        out.append(tuple(dec.plane(p).copy() for p in range(3)))
    dec.close()
    return out


@pytest.mark.parametrize("c", ir.SMALL, ids=IDS)
def test_control_ordinary_streams_do_not_recover(c):
    cut = ir.cut_of(c)
    a, b = oracle_stream(c, ir.frames(c)), oracle_stream(c, ir.frames_other(c))
    assert all(x[0] != y[0] for x, y in zip(a[:cut], b[:cut])), "the prefixes do not differ"
    got = decode_all([x[0] for x in b[:cut]] + [x[0] for x in a[cut:]])
    bands = ir.band_rows((c.h + 15) // 16, c.n)
    for i in range(cut, min(cut + 2 * c.n, c.pictures - 1) + 1):
        for j in range(c.n):
            assert ir.band_differs(got[i], a[i][1], bands, j), "%s: picture %d band %d recovered by chance" % (c.name, i, j)


def test_the_decoder_passes_over_the_sei():
    c = ir.BY_NAME["D_48x64_n2_qp51"]
    a = oracle_stream(c, ir.frames(c)[:4])
    got = decode_all([a[0][0], ir.sei_bytes(2) + a[1][0], a[2][0], ir.sei_bytes(2) + a[3][0]])
    for i in range(4):
        for p in range(3):
            assert np.array_equal(got[i][p], a[i][1][p])


def test_sei_bytes_by_hand():
    sc = b"\x00\x00\x00\x01"
    assert ir.sei_bytes(2) == sc + bytes([0x06, 0x06, 0x01, 0x51, 0x80])          # 010 1 0 00 | 1
    assert ir.sei_bytes(4) == sc + bytes([0x06, 0x06, 0x02, 0x24, 0x40, 0x80])    # 00100 1 0 00 | 1 000000
    assert ir.sei_bytes(8) == sc + bytes([0x06, 0x06, 0x02, 0x11, 0x10, 0x80])    # 0001000 1 0 00 | 1 0000
    assert ir.sei_bytes(32) == sc + bytes([0x06, 0x06, 0x02, 0x04, 0x11, 0x80])   # 00000100000 1 0 00 | 1


def test_schedule_by_hand():
    assert [k for _, _, k in ir.schedule(4, 100, 11)] == [-1, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1]
    assert [k for _, _, k in ir.schedule(2, 5, 9)] == [-1, 0, 1, 0, 1, -1, 0, 1, 0]
    assert [k for _, _, k in ir.schedule(3, 100, 9, forced=(4,))] == [-1, 0, 1, 2, -1, 0, 1, 2, 0]
    assert [(i, k) for i, (idr, _, k) in enumerate(ir.schedule(3, 100, 7, failed=(2,)))] == [(0, -1), (1, 0), (2, 1), (3, -1), (4, 0), (5, 1), (6, 2)]
    assert ir.band_rows(5, 2) == [(0, 3), (3, 5)] and ir.band_rows(68, 8)[-1] == (63, 68) and ir.band_rows(6, 3) == [(0, 2), (2, 4), (4, 6)]
    assert ir.last_luma_row(16, 8, 0) == 23 and ir.last_luma_row(16, 8, -9) == 16 - 3 + 7 + 3 and ir.last_luma_row(0, 16, 5) == 1 + 15 + 3
    assert ir.last_chroma_row(16, 8, 0) == 11 and ir.last_chroma_row(16, 8, -9) == 8 - 2 + 3 + 1 and ir.last_chroma_row(16, 8, 8) == 12
    assert {ir.cut_of(c) for c in ir.CASES} == {1, 3, 4, 5}
