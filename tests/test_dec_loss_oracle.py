"""The cases of tests/dec_loss.py on the oracle alone (CPU): the composed streams - lost NAL units replaced by all-P_Skip stand-ins -
decode on the oracle's independent decoder; content moves (the first damaged picture of the composed decode differs from the
lossless decode in a concealed macroblock); every intra-refresh case is sample-equal to the lossless decode again at the picture
with k = n - 1 of the first refresh cycle that starts after the loss, and differs from it in every picture before.  The writer of
the stand-in slice is checked against hand-written bytes.  Nothing of the decoder under test runs here."""
import numpy as np
import pytest

import dec_loss as dl
from oracle_lib import OracleDecoder

IDS = [c.name for c in dl.CASES]


def test_skip_slice_bytes_by_hand():
    # first_mb 8 (0001001), slice_type 5 (00110), pps 0 (1), frame_num 3 (00000011), no override (0), no modification (0), no marking (0),
    # slice_qp_delta 0 (1), idc 2 (011), offsets 0 0 (1 1), mb_skip_run 8 (0001001), stop bit (1), alignment
    bits = "0001001" "00110" "1" "00000011" "0" "0" "0" "1" "011" "1" "1" "0001001" "1"
    bits += "0" * (-len(bits) % 8)
    want = bytes([0x41]) + bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    assert dl.skip_slice(8, 8, 3, 2, None, 26, 2) == want
    # a non-reference picture has no marking bit and nal_ref_idc 0; an override of 2 active references; QP 29 (se(3) = ue(5) = 00110); idc 1: no offsets;
    # mb_skip_run 23 (000011000)
    bits = "1" "00110" "1" "00000001" "1" "010" "0" "00110" "010" "000011000" "1"
    bits += "0" * (-len(bits) % 8)
    want = bytes([0x01]) + bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    assert dl.skip_slice(0, 23, 1, 0, 2, 29, 1) == want


def test_headers_read_back():
    s = dl.stream("ir3_64x96")
    _, sl = dl.slices_of(s.aus[2])
    hs = [dl.read_header(n) for n in sl]
    assert [h.first_mb for h in hs] == [0, 8, 16] and all(h.frame_num == 2 and h.idc == 2 and not h.idr and h.ref_idc for h in hs)
    assert dl.read_header(dl.rewrite_frame_num(sl[1], 200)).frame_num == 200
    h = dl.read_header(dl.skip_slice(8, 8, 2, 2, None, hs[0].qp, 2))
    assert (h.first_mb, h.slice_type, h.frame_num, h.ref_idc, h.nact, h.qp, h.idc, h.oa, h.ob) == (8, 5, 2, 2, None, hs[0].qp, 2, 0, 0)


@pytest.mark.parametrize("c", dl.CASES, ids=IDS)
def test_composed_stream_decodes_and_content_moves(c):
    s, p = dl.stream(c.stream), dl.plan(c)
    mbw, mbh = (s.w + 15) // 16, (s.h + 15) // 16
    exp, ll = dl.expected(c), dl.lossless(c)            # (raises if the oracle refuses a composed unit)
    assert [e is not None for e in exp] == list(p.got)
    if c.kind == "nonref":                              # a lost non-reference picture: no gap, every picture that arrives stays exact
        assert p.first_loss is None and not any(p.gap)
        assert all(dl.mb_equal(exp[k], ll[k], mbw, mbh).all() for k in range(len(exp)) if exp[k] is not None)
        return
    k = p.first_loss
    differs = ~dl.mb_equal(exp[k], ll[k], mbw, mbh)
    if c.kind == "slice":
        # the stand-in macroblocks of the first damaged picture: its concealed macroblocks are those of the slices the plan removed
        _, sl = dl.slices_of(s.aus[p.orig[k]])
        act = dict(c.loss)[p.orig[k]]
        lost = act[1] if act[0] == "drop" else (act[1],)
        firsts = [dl.read_header(n).first_mb for n in sl] + [mbw * mbh]
        conc = np.zeros(mbw * mbh, bool)
        for j in lost:
            conc[firsts[j]:firsts[j + 1]] = True
        assert int(conc.sum()) == p.concealed[k]
        assert (differs.ravel() & conc).any(), "%s: no concealed macroblock differs from the lossless decode - the content does not move" % c.name
    else:
        assert differs.any(), "%s: the first picture after the loss equals the lossless decode" % c.name


@pytest.mark.parametrize("c", [c for c in dl.CASES if dl.stream(c.stream).n], ids=[c.name for c in dl.CASES if dl.stream(c.stream).n])
def test_intra_refresh_cases_recover_at_the_end_of_the_next_cycle_and_not_before(c):
    s, p = dl.stream(c.stream), dl.plan(c)
    mbw, mbh = (s.w + 15) // 16, (s.h + 15) // 16
    exp, ll = dl.expected(c), dl.lossless(c)
    rec = dl.recovery_step(c)
    assert s.bands[p.orig[rec]] == s.n - 1 and rec < len(exp) - 1
    for k in range(len(exp)):
        if exp[k] is None:
            continue
        same = bool(dl.mb_equal(exp[k], ll[k], mbw, mbh).all())
        if k < p.first_loss or k >= rec:
            assert same, "%s: picture %d differs from the lossless decode (recovery at %d)" % (c.name, k, rec)
        else:
            assert not same, "%s: picture %d equals the lossless decode before the recovery at %d" % (c.name, k, rec)


def test_the_grey_picture_is_grey():
    s = dl.stream("ir2_48x64")
    dec = OracleDecoder()
    assert dec.decode(dl.parameter_sets(s) + dl.annexb([dl.grey_idr(3, 4)])) == 1
    for q in range(3):
        assert (dec.plane(q) == 128).all()
    dec.close()
